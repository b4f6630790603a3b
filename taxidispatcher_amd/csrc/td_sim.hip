// td_sim.hip — a simulator world that lives in HBM behind the C ABI (td_sim_*): Simulator.java's tick loop
// (:151-211) with the cab and request tables on the device.
//
// The specification is taxidispatcher_amd/simulator.py (Simulator.tick on a backend with .tick, i.e. _tick_one_call);
// the per-element rules are in td_sim_core.h.  One tick is a chain of small kernels around the existing td_pool2 and
// td_tick, all on the library's stream, one concern per kernel and the kernel boundary as the only barrier between
// workgroups:
//
//   begin   k_arrive                     checkIfCabAtDestination, one thread per cab (a cab touches only its own request)
//           k_flags<cab>                 "some client-less cab heads here", one bit per stand (LDS bitset per workgroup, OR-ed out)
//           k_dem_count / k_scatter      createTempDemand: the drop and the per-workgroup count in one pass, then the ordered scatter
//           k_flags<req>                 "some unassigned request starts here" (after the drop)
//           k_count / k_scatter          createTempSupply
//           td_pool2 (device lists)      findPool
//           k_pool_mark, k_count / k_scatter   analyzePool: B customers out, A customers annotated, order kept
//   apply   k_pair_map                   first pair per cab / per request (setdefault), indices checked
//           k_apply_pairs                analyzePairs' two loops, one thread per cab / request of the model
//           k_count / k_scatter  x 2     the kept lists, ordered: what row_to_col indexes
//           k_apply_solution             analyzeSolution, one thread per (kept) cab
//
// Ordered compaction = count per workgroup, exclusive scan of the counts, scatter by rank: ascending index order is the
// reference's list order and the golden log depends on it.  The scan of the (few) workgroup counts is done by each
// scatter workgroup for itself (a bounded reduction over the counts before it): no workgroup waits for another.
// Counters are reduced per workgroup and added with one 64-bit atomic per workgroup.
//
// A world on a distance table (td_sim_create_dist): the handle owns a copy of the table and two neighbour bit matrices built
// from it once (k_nb_build in td_sim_core.h, which also validates the table).  The near test of createTempDemand / createTempSupply is then
// one more kernel after each k_flags, k_near: near[s] = any(nb[s][q] & flags[q]), one wave per stand; the predicates read
// one bit of it, and arrival / dispatch / analyzeSolution read one table cell (td_sim_core.h way()).  The direction rule:
// the row of the table is always the cab's stand, dist[cab.to][request.from]:
//   nb_dem[s] bit s'  <=>  dist[s'][s] < drop_time   (request at s, a cab heading to s': a COLUMN of the table)
//   nb_sup[s] bit s'  <=>  dist[s][s'] < drop_time   (cab at s, a request starting at s': a ROW)
// A line world (dist == nullptr) launches exactly what it launched before.
#include <limits.h>

#include <algorithm>
#include <vector>

#include "td_common.h"
#include "td_sim_core.h"

using namespace td;
using namespace tdsim;

struct td_sim {
    World w;
    int max_non_lcm = 0;
    int cap = 1;                 // capacity of every per-tick list: max(n_cabs, n_req, 1)
    Buf mem;                     // every device array of the handle
    Ctl *ctl = nullptr;
    uint32_t *bits_cab = nullptr, *bits_req = nullptr;
    // a table world: the table (= w.dist), the neighbour bit matrices [n_stands][words], the near bitsets [words]
    int32_t *dist = nullptr;
    uint32_t *nb_dem = nullptr, *nb_sup = nullptr, *near_cab = nullptr, *near_req = nullptr;
    int32_t *blockcnt = nullptr;
    // temp lists: demand before pooling, supply, demand after pooling, kept lists
    int32_t *dem_idx, *dem_from, *dem_to;
    int32_t *sup_cab, *sup_to;
    int32_t *d2_idx, *d2_from, *d2_partner, *d2_plan, *d2_cost;
    int32_t *ks_cab, *ks_to;
    int32_t *kd_idx, *kd_from, *kd_partner, *kd_plan, *kd_cost;
    int32_t *isb, *ainfo;                       // analyzePool: is a B customer / first plan as the A customer
    int32_t *pl_a, *pl_b, *pl_plan, *pl_cost;   // td_pool2's plan list
    int32_t *pair_cab, *pair_dem;               // first pair of a cab / request
    int32_t *in_rows, *in_cols, *in_r2c;        // this tick's decisions
    int32_t *tmp;                               // td_sim_state: client ids
    // pinned host block: Ctl read-back, then td_tick's host results for td_sim_step
    void *pin = nullptr;
    int32_t *h_rows, *h_cols, *h_kc, *h_kd, *h_r2c;
    // sequencing
    int last_t = -1;
    bool begun = false;          // a tick with demand waits for td_sim_apply
    int n_dem = 0, n_sup = 0, n_dem2 = 0;
    // the host side of Simulator.m
    int64_t lcm_used = 0, max_model = 0, max_solver = 0, max_pool_mem = 0, max_pool = 0;
};

namespace {

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// sum over the workgroup, returned to every thread (s_red: one slot per wave)
template <class T>
__device__ __forceinline__ T block_sum(T v, T *s_red)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    if (lane == 0) s_red[wv] = v;
    __syncthreads();
    T tot = 0;
    for (int q = 0; q < nw; q++) tot += s_red[q];
    __syncthreads();
    return tot;
}

// rank of this thread among the flagged threads of the workgroup (ascending thread order), *tot = how many
__device__ __forceinline__ int block_rank(bool f, int *s_w, int *tot)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wv] = __popcll(m);
    __syncthreads();
    int off = 0, t = 0;
    for (int q = 0; q < nw; q++) {
        if (q < wv) off += s_w[q];
        t += s_w[q];
    }
    __syncthreads();
    *tot = t;
    return off + before;
}

// the error word as ONE value for the whole workgroup (a kernel is skipped as a whole once an earlier one failed)
__device__ __forceinline__ int block_err(const Ctl *ctl)
{
    __shared__ int s_e;
    if (threadIdx.x == 0) s_e = ctl->err;
    __syncthreads();
    return s_e;
}

__global__ __launch_bounds__(256) void k_init_fleet(World w)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.n_cabs) return;
    w.c_from[c] = w.c_to[c] = c % w.n_stands;   // initSupply, Simulator.java:565-573
    w.c_clnt[c] = -1;
    w.c_onb[c] = 0;
    w.c_start[c] = -1;
}

__global__ __launch_bounds__(256) void k_init_requests(World w)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= w.n_req) return;
    w.r_cab[d] = w.r_pick[d] = w.r_pid[d] = w.r_plan[d] = -1;
    w.r_pcost[d] = 0;
}

__global__ __launch_bounds__(CB) void k_arrive(World w, int t, Ctl *ctl)
{
    __shared__ int s_red[16];
    const int c = blockIdx.x * CB + threadIdx.x;
    const int got = c < w.n_cabs ? arrive(w, t, c) : 0;
    const int tot = block_sum(got, s_red);
    if (threadIdx.x == 0 && tot) atomicAdd((unsigned long long *)&ctl->pickup_numb, (unsigned long long)tot);
}

// bits[s] |= some element i with who[i] == -1 has stand[i] == s
__global__ __launch_bounds__(CB) void k_flags(int n, int n_stands, const int32_t *__restrict__ stand, const int32_t *__restrict__ who,
                                              uint32_t *__restrict__ bits)
{
    extern __shared__ uint32_t s_bits[];
    const int words = (n_stands + 31) / 32;
    for (int i = threadIdx.x; i < words; i += CB) s_bits[i] = 0;
    __syncthreads();
    const int i = blockIdx.x * CB + threadIdx.x;
    if (i < n && who[i] == -1) {
        const int s = stand[i];
        atomicOr(&s_bits[s >> 5], 1u << (s & 31));
    }
    __syncthreads();
    for (int q = threadIdx.x; q < words; q += CB)
        if (s_bits[q]) atomicOr(&bits[q], s_bits[q]);
}

// near[s] = any(nb[s][q] & flags[q]): one wave per stand, the lanes stride over the words (at most two strides: 128 words),
// then a ballot.  A workgroup of 16 waves owns the 32 stands of ONE output word (two stands per wave) and writes it with a
// plain store, so the near bitset needs no clearing and no global atomic.
__global__ __launch_bounds__(CB) void k_near(int n_stands, int words, const uint32_t *__restrict__ nb, const uint32_t *__restrict__ flags,
                                             uint32_t *__restrict__ near)
{
    __shared__ uint32_t s_word;
    if (threadIdx.x == 0) s_word = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j = 0; j < 2; j++) {
        const int bit = 2 * wv + j, s = (int)blockIdx.x * 32 + bit;
        if (s >= n_stands) break;   // the same for the whole wave
        const uint32_t *row = nb + (size_t)s * words;
        uint32_t acc = 0;
        for (int q = lane; q < words; q += 64) acc |= row[q] & flags[q];
        if (__ballot(acc != 0) != 0ull && lane == 0) atomicOr(&s_word, 1u << bit);
    }
    __syncthreads();
    if (threadIdx.x == 0) near[blockIdx.x] = s_word;
}

// createTempDemand's predicate (Simulator.java:329-355) on the table as the drop pass left it.  near: the near bitset of a
// table world (k_near on nb_dem), nullptr = the line's window over bits_cab
struct DemPred {
    World w;
    int t;
    const uint32_t *bits_cab, *near;
    __device__ bool operator()(int d) const
    {
        return w.r_cab[d] == -1 && t >= w.r_at[d] && t - w.r_at[d] < w.drop_time &&
               (near ? bit_of(near, w.r_from[d]) : near_window(bits_cab, w.n_stands, w.drop_time, w.r_from[d]));
    }
};
struct DemEmit {
    World w;
    int32_t *idx, *from, *to;
    __device__ void operator()(int o, int d) const
    {
        idx[o] = d;
        from[o] = w.r_from[d];
        to[o] = w.r_to[d];
    }
};
// createTempSupply (Simulator.java:358-372)
struct SupPred {
    World w;
    const uint32_t *bits_req, *near;   // near: k_near on nb_sup, nullptr = the line
    __device__ bool operator()(int c) const
    {
        return w.c_from[c] == w.c_to[c] && w.c_clnt[c] == -1 &&
               (near ? bit_of(near, w.c_to[c]) : near_window(bits_req, w.n_stands, w.drop_time, w.c_to[c]));
    }
};
struct SupEmit {
    World w;
    int32_t *cab, *to;
    __device__ void operator()(int o, int c) const
    {
        cab[o] = c;
        to[o] = w.c_to[c];
    }
};
// analyzePool (Simulator.java:760-784): every custB leaves, a custA carries its first plan
struct PoolPred {
    const int32_t *isb;
    __device__ bool operator()(int d) const { return !isb[d]; }
};
struct PoolEmit {
    int n_plans;
    const int32_t *dem_idx, *dem_from, *ainfo, *pl_b, *pl_plan, *pl_cost;
    int32_t *idx, *from, *partner, *plan, *cost;
    __device__ void operator()(int o, int d) const
    {
        idx[o] = dem_idx[d];
        from[o] = dem_from[d];
        const int p = ainfo[d];
        const bool a = p >= 0 && p < n_plans;
        partner[o] = a ? dem_idx[pl_b[p]] : -1;
        plan[o] = a ? pl_plan[p] : -1;
        cost[o] = a ? pl_cost[p] : 0;
    }
};
// the cabs / requests that are in no pair (analyzePairs' supply2 / demand2)
struct KeptPred {
    const int32_t *pair_of;
    __device__ bool operator()(int i) const { return pair_of[i] == NONE; }
};
struct KeptSupEmit {
    const int32_t *cab, *to;
    int32_t *cab2, *to2;
    __device__ void operator()(int o, int s) const
    {
        cab2[o] = cab[s];
        to2[o] = to[s];
    }
};
struct KeptDemEmit {
    const int32_t *idx, *from, *partner, *plan, *cost;
    int32_t *idx2, *from2, *partner2, *plan2, *cost2;
    __device__ void operator()(int o, int d) const
    {
        idx2[o] = idx[d];
        from2[o] = from[d];
        partner2[o] = partner[d];
        plan2[o] = plan[d];
        cost2[o] = cost[d];
    }
};

// the request pass of createTempDemand: drop what waited DROP_TIME (cab_assigned = -2), count the kept per workgroup
__global__ __launch_bounds__(CB) void k_dem_count(DemPred pred, int32_t *__restrict__ blockcnt, Ctl *ctl)
{
    __shared__ int s_red[16];
    const World &w = pred.w;
    const int d = blockIdx.x * CB + threadIdx.x;
    int drop = 0, keep = 0;
    if (d < w.n_req) {
        if (w.r_cab[d] == -1 && pred.t >= w.r_at[d] && pred.t - w.r_at[d] >= w.drop_time) {
            w.r_cab[d] = -2;
            drop = 1;
        }
        keep = pred(d) ? 1 : 0;
    }
    const int nd = block_sum(drop, s_red), nk = block_sum(keep, s_red);
    if (threadIdx.x == 0) {
        blockcnt[blockIdx.x] = nk;
        if (nd) atomicAdd((unsigned long long *)&ctl->dropped, (unsigned long long)nd);
    }
}

template <class P>
__global__ __launch_bounds__(CB) void k_count(int n, P pred, int32_t *__restrict__ blockcnt)
{
    __shared__ int s_red[16];
    const int i = blockIdx.x * CB + threadIdx.x;
    const int nk = block_sum((i < n && pred(i)) ? 1 : 0, s_red);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = nk;
}

// out[base + rank] = element, base = the counts of the workgroups before this one; the last workgroup writes the total
template <class P, class E>
__global__ __launch_bounds__(CB) void k_scatter(int n, P pred, E emit, const int32_t *__restrict__ blockcnt, int32_t *__restrict__ total)
{
    __shared__ int s_red[16];
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += CB) part += blockcnt[j];
    const int base = block_sum(part, s_red);
    const int i = blockIdx.x * CB + threadIdx.x;
    const bool f = i < n && pred(i);
    int tot;
    const int rank = block_rank(f, s_red, &tot);
    if (f) emit(base + rank, i);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = base + tot;
}

__global__ __launch_bounds__(256) void k_pool_mark(int n_plans, int n_dem, const int32_t *__restrict__ pl_a, const int32_t *__restrict__ pl_b,
                                                   int32_t *__restrict__ isb, int32_t *__restrict__ ainfo, Ctl *ctl)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_plans) return;
    const int a = pl_a[p], b = pl_b[p];
    if (a < 0 || a >= n_dem || b < 0 || b >= n_dem) {
        atomicMax(&ctl->err, 1);
        return;
    }
    isb[b] = 1;
    atomicMin(&ainfo[a], p);   // the first plan of an A customer (plans are disjoint anyway)
}

// by_cab / by_clnt of analyzePairs (Simulator.java:613-674): the FIRST pair of a cab / of a request
__global__ __launch_bounds__(256) void k_pair_map(int n_pairs, int n_sup, int n_dem, const int32_t *__restrict__ rows,
                                                  const int32_t *__restrict__ cols, int32_t *__restrict__ pair_cab,
                                                  int32_t *__restrict__ pair_dem, Ctl *ctl)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int r = rows[p], c = cols[p];
    if (r < 0 || r >= n_sup || c < 0 || c >= n_dem) {
        atomicMax(&ctl->err, 2);
        return;
    }
    atomicMin(&pair_cab[r], p);
    atomicMin(&pair_dem[c], p);
}

// analyzePairs: thread i < n_sup is the cab loop, the rest the request loop.  A cab and a request occur in at most one
// pair, so the two loops write disjoint state (fleet / request table) and share only the counters.
__global__ __launch_bounds__(CB) void k_apply_pairs(World w, int t, int n_sup, int n_dem, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ cols, const int32_t *__restrict__ pair_cab,
                                                    const int32_t *__restrict__ pair_dem, const int32_t *__restrict__ sup_cab,
                                                    const int32_t *__restrict__ sup_to, const int32_t *__restrict__ d_idx,
                                                    const int32_t *__restrict__ d_partner, const int32_t *__restrict__ d_cost, Ctl *ctl)
{
    __shared__ int s_red[16];
    if (block_err(ctl)) return;
    const int i = blockIdx.x * CB + threadIdx.x;
    int numb = 0, ptime = 0, second = 0;
    if (i < n_sup) {
        const int p = pair_cab[i];
        if (p != NONE) {
            const int d = cols[p];
            dispatch(w, t, sup_cab[i], sup_to[i], d_idx[d], d_partner[d], d_cost[d], numb, ptime);
        }
    } else if (i < n_sup + n_dem) {
        const int d = i - n_sup, p = pair_dem[d];
        if (p != NONE) {   // the request side is not guarded by the distance
            const int cab = sup_cab[rows[p]], idx = d_idx[d];
            w.r_cab[idx] = cab;
            w.r_pick[idx] = t;
            if (d_partner[d] > -1) {
                w.r_cab[d_partner[d]] = cab;   // assignPooled; pool info is NOT copied into the table on this path
                second = 1;
                numb = 1;
            }
        }
    }
    const int tn = block_sum(numb, s_red), tp = block_sum(ptime, s_red), ts = block_sum(second, s_red);
    if (threadIdx.x == 0) {
        if (tn) atomicAdd((unsigned long long *)&ctl->pickup_numb, (unsigned long long)tn);
        if (tp) atomicAdd((unsigned long long *)&ctl->pickup_time, (unsigned long long)tp);
        if (ts) atomicAdd((unsigned long long *)&ctl->second, (unsigned long long)ts);
    }
}

// analyzeSolution (Simulator.java:375-421): one thread per cab of the solver's model.  n_s / n_d: the list sizes, read
// from the device counters when the lists are the kept ones (n_s_dev non-null).  A supply entry's from == to holds by
// construction (createTempSupply admits only standing cabs and the lists are copies), so that test is not repeated.
__global__ __launch_bounds__(CB) void k_apply_solution(World w, int t, int n_s, int n_d, const int32_t *n_s_dev, const int32_t *n_d_dev,
                                                       int n_r2c, const int32_t *__restrict__ r2c, const int32_t *__restrict__ sup_cab,
                                                       const int32_t *__restrict__ sup_to, const int32_t *__restrict__ d_idx,
                                                       const int32_t *__restrict__ d_from, const int32_t *__restrict__ d_partner,
                                                       const int32_t *__restrict__ d_plan, const int32_t *__restrict__ d_cost, Ctl *ctl)
{
    __shared__ int s_red[16];
    if (block_err(ctl)) return;
    if (n_s_dev) {
        n_s = *n_s_dev;
        n_d = *n_d_dev;
    }
    const int s = blockIdx.x * CB + threadIdx.x;
    int count = 0, numb = 0, ptime = 0, second = 0;
    if (s < n_s) {
        const int c = s < n_r2c ? r2c[s] : -1;
        if (c >= 0 && c < n_d) {
            const int dist = way(w, sup_to[s], d_from[c]);
            const int cell = dist < w.drop_time ? dist : w.big_cost;   // the thresholded model's cell
            if (cell < w.big_cost) {
                count = 1;
                const int idx = d_idx[c], cab = sup_cab[s], partner = d_partner[c];
                w.r_cab[idx] = cab;
                w.r_pick[idx] = t;
                if (partner > -1) {
                    w.r_cab[partner] = cab;
                    second = 1;
                    w.r_pid[idx] = w.r_id[partner];   // pool info reaches the table on the OPT path only (:391-396)
                    w.r_plan[idx] = d_plan[c];
                    w.r_pcost[idx] = d_cost[c];
                    numb = 1;
                }
                dispatch(w, t, cab, sup_to[s], idx, partner, d_cost[c], numb, ptime);
            }
        }
    }
    const int tc = block_sum(count, s_red), tn = block_sum(numb, s_red), tp = block_sum(ptime, s_red), ts = block_sum(second, s_red);
    if (threadIdx.x == 0) {
        if (tc) atomicAdd(&ctl->opt_count, tc);
        if (tn) atomicAdd((unsigned long long *)&ctl->pickup_numb, (unsigned long long)tn);
        if (tp) atomicAdd((unsigned long long *)&ctl->pickup_time, (unsigned long long)tp);
        if (ts) atomicAdd((unsigned long long *)&ctl->second, (unsigned long long)ts);
    }
}

// Simulator.c_clnt holds the request id
__global__ __launch_bounds__(256) void k_client_ids(World w, int32_t *__restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= w.n_cabs) return;
    const int d = w.c_clnt[c];
    out[c] = d < 0 ? -1 : w.r_id[d];
}

inline int nblocks(int n) { return (n + CB - 1) / CB; }

// ordered compaction of [0, n): *total (device) = how many; n == 0 leaves *total as the caller zeroed it
template <class P, class E>
int compact(td_sim *s, int n, const P &pred, const E &emit, int32_t *total)
{
    if (n <= 0) return TD_OK;
    Ctx &c = ctx();
    k_count<P><<<nblocks(n), CB, 0, c.stream>>>(n, pred, s->blockcnt);
    k_scatter<P, E><<<nblocks(n), CB, 0, c.stream>>>(n, pred, emit, s->blockcnt, total);
    TD_HIP(hipGetLastError());
    return TD_OK;
}

// the device counters on the host (one stream synchronisation)
int read_ctl(td_sim *s, Ctl *out)
{
    Ctx &c = ctx();
    TD_HIP(hipMemcpyAsync(s->pin, s->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    *out = *(const Ctl *)s->pin;
    return TD_OK;
}

int put(int32_t *dst, const int32_t *src, int n)
{
    if (n <= 0) return TD_OK;
    TD_HIP(hipMemcpyAsync(dst, src, sizeof(int32_t) * (size_t)n, is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          ctx().stream));
    return TD_OK;
}

int get(int32_t *dst, const int32_t *src, int n)
{
    if (n <= 0 || !dst) return TD_OK;
    TD_HIP(hipMemcpyAsync(dst, src, sizeof(int32_t) * (size_t)n, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          ctx().stream));
    return TD_OK;
}

int sim_begin(td_sim *s, int t, int32_t info[4])
{
    Ctx &c = ctx();
    const World &w = s->w;
    int rc;
    info[0] = info[1] = info[2] = info[3] = 0;
    // this tick's list sizes and flags start from zero; the sums and the error word stay
    TD_HIP(hipMemsetAsync(&s->ctl->n_dem, 0, sizeof(int32_t) * 7, c.stream));
    const int words = (w.n_stands + 31) / 32;
    TD_HIP(hipMemsetAsync(s->bits_cab, 0, sizeof(uint32_t) * 2 * (size_t)words, c.stream));   // bits_req follows bits_cab
    const size_t shm = sizeof(uint32_t) * (size_t)words;
    k_arrive<<<nblocks(w.n_cabs), CB, 0, c.stream>>>(w, t, s->ctl);
    k_flags<<<nblocks(w.n_cabs), CB, shm, c.stream>>>(w.n_cabs, w.n_stands, w.c_to, w.c_clnt, s->bits_cab);
    if (s->dist) k_near<<<words, CB, 0, c.stream>>>(w.n_stands, words, s->nb_dem, s->bits_cab, s->near_cab);
    if (w.n_req > 0) {
        const DemPred dp{w, t, s->bits_cab, s->near_cab};
        k_dem_count<<<nblocks(w.n_req), CB, 0, c.stream>>>(dp, s->blockcnt, s->ctl);
        k_scatter<DemPred, DemEmit><<<nblocks(w.n_req), CB, 0, c.stream>>>(w.n_req, dp, DemEmit{w, s->dem_idx, s->dem_from, s->dem_to}, s->blockcnt,
                                                                         &s->ctl->n_dem);
        k_flags<<<nblocks(w.n_req), CB, shm, c.stream>>>(w.n_req, w.n_stands, w.r_from, w.r_cab, s->bits_req);
    }
    if (s->dist) k_near<<<words, CB, 0, c.stream>>>(w.n_stands, words, s->nb_sup, s->bits_req, s->near_req);
    TD_HIP(hipGetLastError());
    // createTempSupply changes nothing, so it is queued before the demand count is known: one read-back for both
    if ((rc = compact(s, w.n_cabs, SupPred{w, s->bits_req, s->near_req}, SupEmit{w, s->sup_cab, s->sup_to}, &s->ctl->n_sup))) return rc;
    Ctl h;
    if ((rc = read_ctl(s, &h))) return rc;
    if (h.err) return fail(TD_EINTERNAL, "td_sim: device error word %d", h.err);
    s->last_t = t;
    s->n_dem = h.n_dem;
    s->n_sup = s->n_dem2 = 0;
    if (h.n_dem == 0) return TD_OK;   // Simulator.java:160: nothing to do in this tick
    s->n_sup = h.n_sup;
    s->n_dem2 = h.n_dem;
    s->begun = true;
    info[0] = 1;
    info[1] = h.n_dem;
    info[2] = h.n_sup;
    info[3] = h.n_dem;
    if (h.n_sup == 0) return TD_OK;   // no pool without supply
    // findPool on the device lists, the plans stay on the device
    int32_t k = 0;
    const int n = h.n_dem;
    if (n >= 2) {
        s->max_pool_mem = std::max(s->max_pool_mem, (int64_t)n * (n - 1));
        if ((rc = td_pool2(n, s->dem_from, s->dem_to, s->dist, s->dist ? w.n_stands : 0, s->pl_a, s->pl_b, s->pl_plan, s->pl_cost, &k))) return rc;
        s->max_pool = std::max(s->max_pool, (int64_t)k);
    }
    TD_HIP(hipMemsetAsync(s->isb, 0, sizeof(int32_t) * (size_t)n, c.stream));
    TD_HIP(hipMemsetAsync(s->ainfo, 0x7f, sizeof(int32_t) * (size_t)n, c.stream));
    if (k > 0) k_pool_mark<<<(k + 255) / 256, 256, 0, c.stream>>>(k, n, s->pl_a, s->pl_b, s->isb, s->ainfo, s->ctl);
    if ((rc = compact(s, n, PoolPred{s->isb},
                      PoolEmit{k, s->dem_idx, s->dem_from, s->ainfo, s->pl_b, s->pl_plan, s->pl_cost, s->d2_idx, s->d2_from, s->d2_partner, s->d2_plan,
                               s->d2_cost},
                      &s->ctl->n_dem2)))
        return rc;
    if ((rc = read_ctl(s, &h))) return rc;
    if (h.err) return fail(TD_EINTERNAL, "td_sim: a pool plan names a customer outside the demand list");
    s->n_dem2 = h.n_dem2;
    info[3] = h.n_dem2;
    s->max_model = std::max(s->max_model, (int64_t)std::max(s->n_sup, s->n_dem2));
    return TD_OK;
}

int sim_apply(td_sim *s, int n_pairs, const int32_t *rows, const int32_t *cols, int solved, int n_r2c, const int32_t *r2c, int32_t *opt_count)
{
    Ctx &c = ctx();
    const World &w = s->w;
    const int t = s->last_t, n_s = s->n_sup, n_d = s->n_dem2, n = std::max(n_s, n_d);
    int rc;
    *opt_count = 0;
    if (n_s == 0) {   // no supply: analyzeSolution walks an empty list, the line ends in "; OPT count=0"
        s->begun = false;
        return TD_OK;
    }
    const bool lcm = n > s->max_non_lcm;
    if (lcm && !solved) *opt_count = -1;
    if (lcm) {
        if ((rc = put(s->in_rows, rows, n_pairs)) || (rc = put(s->in_cols, cols, n_pairs))) return rc;
        TD_HIP(hipMemsetAsync(s->pair_cab, 0x7f, sizeof(int32_t) * (size_t)n_s, c.stream));
        TD_HIP(hipMemsetAsync(s->pair_dem, 0x7f, sizeof(int32_t) * (size_t)n_d, c.stream));
        if (n_pairs > 0)
            k_pair_map<<<(n_pairs + 255) / 256, 256, 0, c.stream>>>(n_pairs, n_s, n_d, s->in_rows, s->in_cols, s->pair_cab, s->pair_dem, s->ctl);
        k_apply_pairs<<<nblocks(n_s + n_d), CB, 0, c.stream>>>(w, t, n_s, n_d, s->in_rows, s->in_cols, s->pair_cab, s->pair_dem, s->sup_cab, s->sup_to,
                                                             s->d2_idx, s->d2_partner, s->d2_cost, s->ctl);
        TD_HIP(hipGetLastError());
        if ((rc = compact(s, n_s, KeptPred{s->pair_cab}, KeptSupEmit{s->sup_cab, s->sup_to, s->ks_cab, s->ks_to}, &s->ctl->n_ks))) return rc;
        if ((rc = compact(s, n_d, KeptPred{s->pair_dem},
                          KeptDemEmit{s->d2_idx, s->d2_from, s->d2_partner, s->d2_plan, s->d2_cost, s->kd_idx, s->kd_from, s->kd_partner, s->kd_plan,
                                      s->kd_cost},
                          &s->ctl->n_kd)))
            return rc;
    }
    if (!lcm || solved) {
        const int nr = solved ? n_r2c : 0;
        if ((rc = put(s->in_r2c, r2c, nr))) return rc;
        if (lcm)
            k_apply_solution<<<nblocks(n_s), CB, 0, c.stream>>>(w, t, 0, 0, &s->ctl->n_ks, &s->ctl->n_kd, nr, s->in_r2c, s->ks_cab, s->ks_to, s->kd_idx,
                                                              s->kd_from, s->kd_partner, s->kd_plan, s->kd_cost, s->ctl);
        else
            k_apply_solution<<<nblocks(n_s), CB, 0, c.stream>>>(w, t, n_s, n_d, nullptr, nullptr, nr, s->in_r2c, s->sup_cab, s->sup_to, s->d2_idx,
                                                              s->d2_from, s->d2_partner, s->d2_plan, s->d2_cost, s->ctl);
        TD_HIP(hipGetLastError());
    }
    Ctl h;
    if ((rc = read_ctl(s, &h))) return rc;
    if (h.err) {
        // nothing was applied (every kernel after the failing one is skipped): the tick still waits for its decisions
        TD_HIP(hipMemsetAsync(&s->ctl->err, 0, sizeof(int32_t), c.stream));
        TD_HIP(hipStreamSynchronize(c.stream));
        if (h.err == 2) return fail(TD_EINVAL, "td_sim_apply: a pair lies outside the model (%d cabs, %d requests)", n_s, n_d);
        return fail(TD_EINTERNAL, "td_sim: device error word %d", h.err);
    }
    s->begun = false;
    if (lcm) s->lcm_used++;
    if (!lcm || solved) {
        *opt_count = h.opt_count;
        s->max_solver = std::max(s->max_solver, (int64_t)(lcm ? std::max(h.n_ks, h.n_kd) : n));
    }
    return TD_OK;
}

// td_sim_create (dist == nullptr) and td_sim_create_dist
int sim_create(int n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost, int n_req, const int32_t *req_id,
               const int32_t *req_from, const int32_t *req_to, const int32_t *req_at, const int32_t *dist, td_sim **out)
{
    TD_REQUIRE_INIT();
    Ctx &c = ctx();
    if (!out) return fail(TD_EINVAL, "null handle pointer");
    *out = nullptr;
    if (n_cabs < 1 || n_stands < 1 || drop_time < 0 || max_non_lcm < 0 || big_cost < 0 || n_req < 0)
        return fail(TD_EINVAL, "td_sim_create: n_cabs and n_stands at least 1, nothing negative");
    if (n_stands > (1 << 18)) return fail(TD_EINVAL, "td_sim_create: at most %d stands (one bit per stand in LDS)", 1 << 18);
    if (dist && n_stands > MAX_DIST_STANDS) return fail(TD_EINVAL, "td_sim_create_dist: at most %d stands with a distance table", MAX_DIST_STANDS);
    if (n_req && (!req_id || !req_from || !req_to || !req_at)) return fail(TD_EINVAL, "null request array");
    // the request file on the host once: ids unique and not negative, stands inside the line, arrival times not negative
    std::vector<int32_t> h((size_t)4 * n_req);
    const int32_t *src[4] = {req_id, req_from, req_to, req_at};
    for (int q = 0; q < 4 && n_req; q++) TD_HIP(hipMemcpy(h.data() + (size_t)q * n_req, src[q], sizeof(int32_t) * (size_t)n_req, hipMemcpyDefault));
    for (int i = 0; i < n_req; i++) {
        const int32_t id = h[i], f = h[(size_t)n_req + i], to = h[(size_t)2 * n_req + i], at = h[(size_t)3 * n_req + i];
        if (id < 0 || f < 0 || f >= n_stands || to < 0 || to >= n_stands || at < 0)
            return fail(TD_EINVAL, "td_sim_create: request %d (id %d, from %d, to %d, at %d) is outside the world", i, id, f, to, at);
    }
    {
        std::vector<int32_t> ids(h.begin(), h.begin() + n_req);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return fail(TD_EINVAL, "td_sim_create: request ids must be unique");
    }
    td_sim *s = new td_sim();
    s->max_non_lcm = max_non_lcm;
    const size_t nr = (size_t)std::max(n_req, 1), nc = (size_t)n_cabs, cap = std::max(nr, nc), words = (size_t)(n_stands + 31) / 32;
    s->cap = (int)cap;
    const size_t ns = (size_t)n_stands, table_ints = dist ? ns * ns + 2 * ns * words + 2 * words : 0;
    const size_t ints = table_ints + 64 + 2 * words + (cap + CB - 1) / CB + 9 * nr + 5 * nc + 3 * nr + 2 * nc + 5 * nr + 2 * nc + 5 * nr + 2 * nr + 4 * (nr / 2 + 1) +
                        nc + nr + 3 * cap + cap + 64;
    int rc = ensure(s->mem, sizeof(int32_t) * ints);
    if (rc) {
        delete s;
        return rc;
    }
    int32_t *p = (int32_t *)s->mem.p;
    auto take = [&](size_t k) {
        int32_t *r = p;
        p += k;
        return r;
    };
    s->ctl = (Ctl *)take(64);
    s->bits_cab = (uint32_t *)take(words);
    s->bits_req = (uint32_t *)take(words);   // must stay directly behind bits_cab: sim_begin clears both with ONE memset
    if (dist) {
        s->near_cab = (uint32_t *)take(words);
        s->near_req = (uint32_t *)take(words);
        s->nb_dem = (uint32_t *)take(ns * words);
        s->nb_sup = (uint32_t *)take(ns * words);
        s->dist = take(ns * ns);
    }
    s->blockcnt = take((cap + CB - 1) / CB);
    World &w = s->w;
    w.n_cabs = n_cabs;
    w.n_req = n_req;
    w.n_stands = n_stands;
    w.drop_time = drop_time;
    w.big_cost = big_cost;
    w.dist = s->dist;
    int32_t *rid = take(nr), *rfrom = take(nr), *rto = take(nr), *rat = take(nr);
    w.r_id = rid;
    w.r_from = rfrom;
    w.r_to = rto;
    w.r_at = rat;
    w.r_cab = take(nr);
    w.r_pick = take(nr);
    w.r_pid = take(nr);
    w.r_plan = take(nr);
    w.r_pcost = take(nr);
    w.c_from = take(nc);
    w.c_to = take(nc);
    w.c_clnt = take(nc);
    w.c_onb = take(nc);
    w.c_start = take(nc);
    s->dem_idx = take(nr);
    s->dem_from = take(nr);
    s->dem_to = take(nr);
    s->sup_cab = take(nc);
    s->sup_to = take(nc);
    s->d2_idx = take(nr);
    s->d2_from = take(nr);
    s->d2_partner = take(nr);
    s->d2_plan = take(nr);
    s->d2_cost = take(nr);
    s->ks_cab = take(nc);
    s->ks_to = take(nc);
    s->kd_idx = take(nr);
    s->kd_from = take(nr);
    s->kd_partner = take(nr);
    s->kd_plan = take(nr);
    s->kd_cost = take(nr);
    s->isb = take(nr);
    s->ainfo = take(nr);
    s->pl_a = take(nr / 2 + 1);
    s->pl_b = take(nr / 2 + 1);
    s->pl_plan = take(nr / 2 + 1);
    s->pl_cost = take(nr / 2 + 1);
    s->pair_cab = take(nc);
    s->pair_dem = take(nr);
    s->in_rows = take(cap);
    s->in_cols = take(cap);
    s->in_r2c = take(cap);
    s->tmp = take(cap);
    auto bail = [&](int code) {
        td_sim_destroy(s);
        return code;
    };
    hipError_t e = hipHostMalloc(&s->pin, 256 + sizeof(int32_t) * 5 * cap, hipHostMallocDefault);
    if (e != hipSuccess) {
        s->pin = nullptr;
        return bail(hip_fail(e, "hipHostMalloc(td_sim)"));
    }
    int32_t *hp = (int32_t *)((char *)s->pin + 256);
    s->h_rows = hp;
    s->h_cols = hp + cap;
    s->h_kc = hp + 2 * cap;
    s->h_kd = hp + 3 * cap;
    s->h_r2c = hp + 4 * cap;
    if ((e = hipMemsetAsync(s->ctl, 0, sizeof(int32_t) * 64, c.stream)) != hipSuccess) return bail(hip_fail(e, "hipMemsetAsync"));
    int32_t *dst[4] = {rid, rfrom, rto, rat};
    for (int q = 0; q < 4 && n_req; q++)
        if ((e = hipMemcpyAsync(dst[q], h.data() + (size_t)q * n_req, sizeof(int32_t) * (size_t)n_req, hipMemcpyHostToDevice, c.stream)) != hipSuccess)
            return bail(hip_fail(e, "hipMemcpyAsync(request table)"));
    k_init_fleet<<<(n_cabs + 255) / 256, 256, 0, c.stream>>>(w);
    if (n_req) k_init_requests<<<(n_req + 255) / 256, 256, 0, c.stream>>>(w);
    if ((e = hipGetLastError()) != hipSuccess) return bail(hip_fail(e, "td_sim_create launch"));
    if (dist) {
        // the handle's own copy of the table, then its bit matrices; k_nb_build reports an invalid table in the error word
        if ((e = hipMemcpyAsync(s->dist, dist, sizeof(int32_t) * ns * ns, is_device_ptr(dist) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                c.stream)) != hipSuccess)
            return bail(hip_fail(e, "hipMemcpyAsync(distance table)"));
        const int cells = n_stands * (int)words;
        k_nb_build<<<(cells + 255) / 256, 256, 0, c.stream>>>(n_stands, (int)words, drop_time, s->dist, s->nb_dem, s->nb_sup, &s->ctl->err);
        if ((e = hipGetLastError()) != hipSuccess) return bail(hip_fail(e, "td_sim_create_dist launch"));
    }
    if ((e = hipStreamSynchronize(c.stream)) != hipSuccess) return bail(hip_fail(e, "hipStreamSynchronize"));   // `h` leaves scope
    if (dist) {
        Ctl hc;
        int rc = read_ctl(s, &hc);
        if (rc) return bail(rc);
        if (hc.err)
            return bail(fail(TD_EINVAL, "td_sim_create_dist: the distance table needs a zero diagonal and every other entry in 1 .. %d", MAX_DIST));
    }
    *out = s;
    return TD_OK;
}

}  // namespace

extern "C" int td_sim_create(int n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost, int n_req, const int32_t *req_id,
                             const int32_t *req_from, const int32_t *req_to, const int32_t *req_at, td_sim **out)
{
    return sim_create(n_cabs, n_stands, drop_time, max_non_lcm, big_cost, n_req, req_id, req_from, req_to, req_at, nullptr, out);
}

extern "C" int td_sim_create_dist(int n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost, int n_req, const int32_t *req_id,
                                  const int32_t *req_from, const int32_t *req_to, const int32_t *req_at, const int32_t *dist, td_sim **out)
{
    return sim_create(n_cabs, n_stands, drop_time, max_non_lcm, big_cost, n_req, req_id, req_from, req_to, req_at, dist, out);
}

extern "C" int td_sim_destroy(td_sim *s)
{
    if (!s) return TD_OK;
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
    buf_free(s->mem);
    if (s->pin) (void)hipHostFree(s->pin);
    delete s;
    return TD_OK;
}

extern "C" int td_sim_begin(td_sim *s, int t, int32_t info[4])
{
    TD_REQUIRE_INIT();
    if (!s || !info) return fail(TD_EINVAL, "null argument");
    if (t < 0) return fail(TD_EINVAL, "negative tick");
    if (s->begun) return fail(TD_EINVAL, "td_sim_begin: tick %d still waits for td_sim_apply", s->last_t);
    if (t <= s->last_t) return fail(TD_EINVAL, "td_sim_begin: tick %d after tick %d (a tick begins once, time runs forward)", t, s->last_t);
    return sim_begin(s, t, info);
}

extern "C" int td_sim_model(td_sim *s, int32_t *cab_to, int32_t *dem_from)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!s->begun) return fail(TD_EINVAL, "td_sim_model: no tick with demand has begun");
    if ((s->n_sup && !cab_to) || (s->n_dem2 && !dem_from)) return fail(TD_EINVAL, "null destination");
    int rc;
    // without supply the demand was not pooled: the model's requests are the temp demand itself
    if ((rc = get(cab_to, s->sup_to, s->n_sup)) || (rc = get(dem_from, s->n_sup ? s->d2_from : s->dem_from, s->n_dem2))) return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_sim_apply(td_sim *s, int n_pairs, const int32_t *lcm_rows, const int32_t *lcm_cols, int solved, int n_r2c,
                            const int32_t *row_to_col, int32_t *opt_count)
{
    TD_REQUIRE_INIT();
    if (!s || !opt_count) return fail(TD_EINVAL, "null argument");
    if (!s->begun) return fail(TD_EINVAL, "td_sim_apply: no tick with demand has begun");
    if (n_pairs < 0 || n_r2c < 0 || n_pairs > s->cap || n_r2c > s->cap) return fail(TD_EINVAL, "td_sim_apply: list length outside 0 .. %d", s->cap);
    if ((n_pairs && (!lcm_rows || !lcm_cols)) || (solved && n_r2c && !row_to_col)) return fail(TD_EINVAL, "null decision array");
    return sim_apply(s, n_pairs, lcm_rows, lcm_cols, solved, n_r2c, row_to_col, opt_count);
}

extern "C" int td_sim_step(td_sim *s, int t, int32_t line[9])
{
    TD_REQUIRE_INIT();
    if (!s || !line) return fail(TD_EINVAL, "null argument");
    int32_t info[4];
    int rc = td_sim_begin(s, t, info);
    if (rc) return rc;
    for (int q = 0; q < 9; q++) line[q] = 0;
    if (!info[0]) return TD_OK;
    line[0] = 1;
    line[1] = info[1];
    line[2] = info[2];
    const int n_s = s->n_sup, n_d = s->n_dem2, n = std::max(n_s, n_d);
    int32_t k = 0, lm = 0, n_rest = 0, opt = 0;
    int64_t total = 0;
    int solved = 0;
    if (n_s > 0) {
        // the arguments HipTickBackend.tick hands td_tick, with the position lists (and the table) where they already are
        if ((rc = td_tick(s->sup_to, n_s, s->d2_from, n_d, s->dist, s->dist ? s->w.n_stands : 0, s->w.big_cost, s->w.drop_time, s->max_non_lcm, s->h_rows, s->h_cols, &k, &lm,
                          s->h_kc, s->h_kd, &n_rest, s->h_r2c, &total)))
            return rc;
        const bool lcm = s->max_non_lcm < n;
        solved = n_rest > 0 && !(lcm && lm == s->w.big_cost);
        line[3] = lcm;
        line[4] = lcm ? k : 0;
        line[5] = lcm && solved;
        line[6] = n_d - k;
        line[7] = n_s - k;
    }
    if ((rc = sim_apply(s, k, s->h_rows, s->h_cols, solved, solved ? n_rest : 0, s->h_r2c, &opt))) return rc;
    line[8] = opt;
    return TD_OK;
}

extern "C" int td_sim_state(td_sim *s, int32_t *c_from, int32_t *c_to, int32_t *c_clnt, int32_t *c_onboard, int32_t *c_start, int32_t *d_cab,
                            int32_t *d_pick, int32_t *d_pool_id, int32_t *d_pool_plan, int32_t *d_pool_cost)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    Ctx &c = ctx();
    const World &w = s->w;
    int rc;
    if (c_clnt) {
        k_client_ids<<<(w.n_cabs + 255) / 256, 256, 0, c.stream>>>(w, s->tmp);
        TD_HIP(hipGetLastError());
    }
    int32_t *cd[5] = {c_from, c_to, c_clnt, c_onboard, c_start};
    const int32_t *cs[5] = {w.c_from, w.c_to, s->tmp, w.c_onb, w.c_start};
    int32_t *rd[5] = {d_cab, d_pick, d_pool_id, d_pool_plan, d_pool_cost};
    const int32_t *rs[5] = {w.r_cab, w.r_pick, w.r_pid, w.r_plan, w.r_pcost};
    for (int q = 0; q < 5; q++)
        if ((rc = get(cd[q], cs[q], w.n_cabs)) || (rc = get(rd[q], rs[q], w.n_req))) return rc;
    TD_HIP(hipStreamSynchronize(c.stream));
    return TD_OK;
}

extern "C" int td_sim_metrics(td_sim *s, int64_t out[TD_SIM_N_METRICS])
{
    TD_REQUIRE_INIT();
    if (!s || !out) return fail(TD_EINVAL, "null argument");
    Ctl h;
    int rc = read_ctl(s, &h);
    if (rc) return rc;
    out[0] = h.dropped;
    out[1] = h.pickup_time;
    out[2] = h.pickup_numb;
    out[3] = s->lcm_used;
    out[4] = s->max_model;
    out[5] = s->max_solver;
    out[6] = s->max_pool_mem;
    out[7] = s->max_pool;
    out[8] = h.second;
    return TD_OK;
}
