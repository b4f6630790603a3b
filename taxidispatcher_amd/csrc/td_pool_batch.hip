// td_pool_batch.hip — td_pool_n_batched: pools of 2..4 passengers (pool_n.c / Pool.java) for MANY ragged models per call.
//
// One workgroup per model, models dealt grid-stride; no launch, sort call or host synchronisation per model.
//
//   staging     the model's from / to / max_wait / max_loss in LDS (8 KiB at 512 requests); with a table every stand is
//               checked against [0, S) here, before anything indexes the table
//   enumerate   level by level, the SURVIVORS of each level compacted into an LDS queue: (first, second) pairs that pass
//               the wait rule, then (pair, third) triples, then quads.  A queue is drained into the next level when it
//               cannot take another step's worth of candidates, so every step spreads PNB_CH candidates — one cheap wait
//               test each — over the threads, and the expensive part, the k! drop-off orders, runs on full k-tuples
//               only, one tuple per thread.  Happy plans are appended to the workgroup's key slab with one LDS atomic per
//               wave and drop-off order; keys past the capacity are counted and not stored.
//   select      "stable sort by cost, keep a plan iff it shares no request with an earlier kept one" = "repeatedly take
//               the smallest key among the plans none of whose requests is used" (the LCM pattern): per round every wave
//               scans ITS segment of the slab, drops the dead keys in place and reduces the minimum; at most n_b / k
//               rounds, each shorter than the one before.  The append order of the keys is free: the key carries the
//               reference's order.
//
// Results go to library-owned staging; the caller's arrays are written only after the error words were read back, so
// a refused call leaves them untouched.
#include <utility>
#include <vector>

#include "td_stage.h"
#include "td_pool_core.h"

using namespace td;

namespace {

constexpr int PNB_MAXN = 512;                  // 4 * 9 bits of requests in a queue entry; 8 KiB of staged requests
constexpr int PNB_T = 256;                     // threads per workgroup
constexpr int PNB_W = PNB_T / 64;
constexpr int PNB_U = 2;                       // candidates per thread and step
constexpr int PNB_CH = PNB_T * PNB_U;          // candidates per step
constexpr int PNB_CAP = 2 * PNB_CH;            // entries per queue: a queue below CAP - CH takes any step's survivors
constexpr int PNB_GRID = 1024;                 // workgroups in flight (256 CUs x 4 by LDS): the slab is PNB_GRID x max_happy keys
constexpr int64_t PNB_MAX_HAPPY = 1ll << 22;
constexpr int64_t PNB_DEF_HAPPY = 65536;
constexpr size_t PNB_SLAB_BYTES = (size_t)1 << 30;

struct PnbErr {
    int cost;       // a happy plan's cost does not fit the key
    int over;       // batch - (first model with more than max_happy happy plans), 0: none
    int bad;        // batch - (first model with a stand outside the table), 0: none
    int pad;
};

// floor(c / d) for 2 <= d <= 512 and c * d < 2^32, with m = 2^32 / d + 1 (the error term of m is at most d / 2^32 per unit)
__device__ __forceinline__ uint32_t pnb_div(uint32_t c, uint32_t m) { return __umulhi(c, m); }

struct PnbModel {
    const int32_t *sf, *st, *sw, *sl;   // LDS
    const int32_t *dist;
    int S, nb, f0, f1;
    uint32_t magic;                     // 2^32 / nb + 1
    unsigned long long *keys;           // this workgroup's slab
    unsigned long long cap;
};

template <int K>
struct PnbShared {
    int32_t req[4 * PNB_MAXN];
    uint32_t qa[K - 1][PNB_CAP];     // p0 | p1 << 9 | p2 << 18
    int32_t qb[K - 1][PNB_CAP];      // pick-up path so far; in the queue of quads the fourth pick-up
    int qn[K - 1];
    unsigned long long happy;
    unsigned long long wmin[PNB_W];
    unsigned int used[PNB_MAXN / 32];
    int err, bad;
};

// index of this lane's entry when the lanes with `pass` append to a counter in LDS: one atomic per wave
template <class C>
__device__ __forceinline__ C pnb_append(bool pass, C *counter)
{
    const unsigned long long m = __ballot(pass);
    if (!m) return 0;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = (unsigned long long)atomicAdd(counter, (C)__popcll(m));
    base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), leader) << 32) |
           (unsigned long long)(uint32_t)__shfl((int)(uint32_t)base, leader);
    return (C)(base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull)));
}

// one drop-off order of this thread's tuple: happiness, cost, and the wave's happy plans appended with one atomic
template <int K, int QI>
__device__ __forceinline__ void pnb_order(PnbShared<K> &sh, const PnbModel &x, bool valid, const int *p, unsigned long long seq0)
{
    constexpr PnOrder o = pn_order(K, QI);
    const int q[4] = {o.q[0], o.q[1], o.q[2], o.q[3]};
    int cost = 0;
    const bool happy = valid && pn_check<K>(p, q, x.sf, x.st, x.sl, x.dist, x.S, &cost);
    const unsigned long long idx = pnb_append(happy, &sh.happy);
    if (happy) {
        if (cost > PN_MAXCOST || cost < 0) sh.err = 1;
        else if (idx < x.cap) x.keys[idx] = ((unsigned long long)cost << PN_SEQ_BITS) | (seq0 + (unsigned long long)QI);
    }
}

template <int K, int... QI>
__device__ __forceinline__ void pnb_orders(std::integer_sequence<int, QI...>, PnbShared<K> &sh, const PnbModel &x, bool valid, const int *p,
                                           unsigned long long seq0)
{
    (pnb_order<K, QI>(sh, x, valid, p, seq0), ...);
}

// the k! drop-off orders of every full tuple of the last queue: one tuple per thread
template <int K>
__device__ __forceinline__ void pnb_check(PnbShared<K> &sh, const PnbModel &x)
{
    constexpr int NP = K == 2 ? 2 : K == 3 ? 6 : 24;
    const int cnt = sh.qn[K - 2];
    const unsigned long long nn = (unsigned long long)x.nb;
    for (int base = 0; base < cnt; base += PNB_T) {
        const int e = base + (int)threadIdx.x;
        const bool valid = e < cnt;
        const uint32_t a = valid ? sh.qa[K - 2][e] : 0u;
        int p[4] = {(int)(a & 511u), (int)((a >> 9) & 511u), K >= 3 ? (int)((a >> 18) & 511u) : 0, 0};
        if (K == 4) p[3] = valid ? sh.qb[K - 2][e] : 0;
        const unsigned long long seq0 = ((((unsigned long long)p[0] * nn + p[1]) * nn + p[2]) * nn + p[3]) * 24ull;
        pnb_orders<K>(std::make_integer_sequence<int, NP>{}, sh, x, valid, p, seq0);
    }
    __syncthreads();
    if (threadIdx.x == 0) sh.qn[K - 2] = 0;
    __syncthreads();
}

// empties the queue of M-tuples into the queue of (M+1)-tuples, draining that one whenever it may not take a step's
// survivors; `final`: everything downstream is emptied too.  Every branch here is uniform over the workgroup.
template <int K, int M>
__device__ __forceinline__ void pnb_drain(PnbShared<K> &sh, const PnbModel &x, bool final)
{
    if constexpr (M == K) {
        pnb_check<K>(sh, x);
    } else {
        const int cnt = sh.qn[M - 2];
        const int total = cnt * x.nb;   // <= PNB_CAP * 512 = 2^19
        for (int c0 = 0; c0 < total; c0 += PNB_CH) {
            const bool full = sh.qn[M - 1] + PNB_CH > PNB_CAP;
            __syncthreads();   // every thread has read the count before any appends to it
            if (full) pnb_drain<K, M + 1>(sh, x, false);
#pragma unroll
            for (int j = 0; j < PNB_U; j++) {
                const int c = c0 + j * PNB_T + (int)threadIdx.x;
                bool pass = c < total;
                uint32_t a = 0;
                int len = 0, cand = 0;
                if (pass) {
                    const int e = (int)pnb_div((uint32_t)c, x.magic);
                    cand = c - e * x.nb;
                    a = sh.qa[M - 2][e];
                    const int p0 = (int)(a & 511u), p1 = (int)((a >> 9) & 511u), p2 = (int)((a >> 18) & 511u);
                    const int last = M == 2 ? p1 : p2;
                    pass = cand != p0 && cand != p1 && (M == 2 || cand != p2);
                    len = sh.qb[M - 2][e] + pn_d(x.dist, x.S, x.sf[last], x.sf[cand]);
                    pass = pass && !(len > x.sw[cand]);   // pool_n.c:177-178
                }
                const int at = pnb_append(pass, &sh.qn[M - 1]);
                if (pass) {
                    sh.qa[M - 1][at] = M == 2 ? (a | ((uint32_t)cand << 18)) : a;
                    sh.qb[M - 1][at] = M == 2 ? len : cand;
                }
            }
            __syncthreads();
        }
        __syncthreads();
        if (threadIdx.x == 0) sh.qn[M - 2] = 0;
        __syncthreads();
        if (final) pnb_drain<K, M + 1>(sh, x, true);
    }
}

// the requests and the drop-off order behind a key, as td_pool_n decodes it (radix nb); exact: seq < 2^41, so the double
// quotient is off by at most one and the remainder test repairs it
__device__ __forceinline__ void pnb_decode(unsigned long long key, int nb, uint32_t magic, double inv_d2, int *c, int *qi)
{
    const long long seq = (long long)(key & PN_SEQ_MASK);
    const long long d2 = 24ll * nb * nb;
    long long hi = (long long)((double)seq * inv_d2);
    long long r = seq - hi * d2;
    if (r < 0) {
        hi--;
        r += d2;
    } else if (r >= d2) {
        hi++;
        r -= d2;
    }
    const uint32_t lo = (uint32_t)r, t = lo / 24u;   // t = p2 * nb + p3 < 2^18
    *qi = (int)(lo - t * 24u);
    c[2] = (int)pnb_div(t, magic);
    c[3] = (int)t - c[2] * nb;
    c[0] = (int)pnb_div((uint32_t)hi, magic);
    c[1] = (int)hi - c[0] * nb;
}

template <int K, int... QI>
__device__ __forceinline__ unsigned char pnb_perm_codes(std::integer_sequence<int, QI...>, int qi)
{
    constexpr unsigned char code[] = {(unsigned char)(pn_order(K, QI).q[0] | pn_order(K, QI).q[1] << 2 | pn_order(K, QI).q[2] << 4 |
                                                      pn_order(K, QI).q[3] << 6)...};
    return code[qi];
}

// V: the models are worlds (td::pool_n_worlds): model b's requests lie at off[b], sel.cnt[b] of them, and only where the world's
// cascade has a stage of K (sel.k_lo[b] <= K <= sel.k_hi[b]), else the model is empty; wait / loss hold one rule per model
template <bool V>
struct PnbSel {};
template <>
struct PnbSel<true> {
    const int32_t *cnt, *k_hi, *k_lo;
};

template <int K, bool V = false>
__global__ __launch_bounds__(PNB_T) void k_pooln_batched(int batch, int n, const int32_t *__restrict__ off,
                                                         const int32_t *__restrict__ from, const int32_t *__restrict__ to,
                                                         const int32_t *__restrict__ wait, const int32_t *__restrict__ loss,
                                                         const int32_t *__restrict__ dist, int S, const int32_t *__restrict__ first,
                                                         unsigned long long cap, unsigned long long *__restrict__ slab,
                                                         int32_t *__restrict__ pools, int32_t *__restrict__ n_pools,
                                                         long long *__restrict__ n_happy, long long *__restrict__ total,
                                                         PnbErr *__restrict__ err, PnbSel<V> sel)
{
    __shared__ PnbShared<K> sh;
    __shared__ unsigned char s_perm[24];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NP = K == 2 ? 2 : K == 3 ? 6 : 24;
    // the drop-off orders as 2 bits per slot, for the record writer
    if (tid < NP) s_perm[tid] = pnb_perm_codes<K>(std::make_integer_sequence<int, NP>{}, tid);
    const size_t rec = (size_t)(2 * K + 1), stride = (size_t)(n / K) * rec;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int o = off[b];
        int nb;
        if constexpr (V)
            nb = sel.k_lo[b] <= K && K <= sel.k_hi[b] ? max(0, min(sel.cnt[b], min(n, PNB_MAXN))) : 0;
        else
            nb = off[b + 1] - o;
        int f0 = 0, f1 = nb;
        if (first) {
            f0 = max(first[2 * b], 0);
            f1 = min(first[2 * b + 1], nb);
        }
        __syncthreads();   // the previous model is finished with LDS
        bool bad = false;
        for (int i = tid; i < nb; i += PNB_T) {
            const int32_t f = from[o + i], t = to[o + i];
            sh.req[i] = f;
            sh.req[PNB_MAXN + i] = t;
            sh.req[2 * PNB_MAXN + i] = wait[V ? b : o + i];
            sh.req[3 * PNB_MAXN + i] = loss[V ? b : o + i];
            bad = bad || (dist && ((uint32_t)f >= (uint32_t)S || (uint32_t)t >= (uint32_t)S));
        }
        if (tid < K - 1) sh.qn[tid] = 0;
        if (tid < PNB_MAXN / 32) sh.used[tid] = 0u;
        if (tid == 0) {
            sh.happy = 0ull;
            sh.err = 0;
            sh.bad = 0;
        }
        __syncthreads();
        if (bad) sh.bad = 1;
        __syncthreads();
        PnbModel x;
        x.sf = sh.req;
        x.st = sh.req + PNB_MAXN;
        x.sw = sh.req + 2 * PNB_MAXN;
        x.sl = sh.req + 3 * PNB_MAXN;
        x.dist = dist;
        x.S = S;
        x.nb = nb;
        x.f0 = f0;
        x.f1 = f1;
        x.magic = nb >= 2 ? (uint32_t)(0x100000000ull / (unsigned long long)nb) + 1u : 0u;
        x.keys = slab + (size_t)blockIdx.x * (size_t)cap;
        x.cap = cap;
        if (sh.bad) {   // nothing of this model may index the table
            if (tid == 0) {
                atomicMax(&err->bad, batch - b);
                n_pools[b] = 0;
                n_happy[b] = 0;
                total[b] = 0;
            }
            continue;
        }
        if (nb >= K && f1 > f0) {
            // level 1: the (first, second) pairs of the slice
            const int space = (f1 - f0) * nb;   // <= 2^18
            for (int c0 = 0; c0 < space; c0 += PNB_CH) {
                const bool full = sh.qn[0] + PNB_CH > PNB_CAP;
                __syncthreads();
                if (full) pnb_drain<K, 2>(sh, x, false);
#pragma unroll
                for (int j = 0; j < PNB_U; j++) {
                    const int c = c0 + j * PNB_T + tid;
                    bool pass = c < space;
                    int p0 = 0, p1 = 0, len = 0;
                    if (pass) {
                        const int e = (int)pnb_div((uint32_t)c, x.magic);
                        p0 = f0 + e;
                        p1 = c - e * nb;
                        len = pn_d(dist, S, x.sf[p0], x.sf[p1]);
                        // pool_n.c:177 at level 0 (an empty path against WAIT), then :177-178 for the second pick-up
                        pass = !(0 > x.sw[p0]) && p1 != p0 && !(len > x.sw[p1]);
                    }
                    const int at = pnb_append(pass, &sh.qn[0]);
                    if (pass) {
                        sh.qa[0][at] = (uint32_t)p0 | ((uint32_t)p1 << 9);
                        sh.qb[0][at] = len;
                    }
                }
                __syncthreads();
            }
            pnb_drain<K, 2>(sh, x, true);
        }
        __syncthreads();
        const unsigned long long happy = sh.happy;
        const bool cost_err = sh.err != 0;
        int kept = 0;
        long long sum = 0;
        if (cost_err) {
            if (tid == 0) atomicOr(&err->cost, 1);
        } else if (happy > cap) {
            if (tid == 0) atomicMax(&err->over, batch - b);
        } else if (happy > 0) {
            // selection: every wave owns a segment of the slab and keeps its live keys at the segment's front
            const int m = (int)happy;   // <= 2^22
            const int seg = (m + PNB_W - 1) / PNB_W;
            unsigned long long *mine = x.keys + (size_t)w * (size_t)seg;
            int wcnt = max(0, min(seg, m - w * seg));
            const double inv_d2 = 1.0 / (24.0 * (double)nb * (double)nb);
            const int max_kept = nb / K;
            int32_t *out = pools + (size_t)b * stride;
            for (;;) {
                unsigned long long lmin = ~0ull;
                int newcnt = 0;
                for (int j = 0; j < wcnt; j += 64) {
                    const int i = j + lane;
                    unsigned long long key = ~0ull;
                    bool live = i < wcnt;
                    if (live) key = mine[i];
                    if (live && kept > 0) {
                        int c[4], qi;
                        pnb_decode(key, nb, x.magic, inv_d2, c, &qi);
#pragma unroll
                        for (int a = 0; a < K; a++) live = live && !((sh.used[c[a] >> 5] >> (c[a] & 31)) & 1u);
                    }
                    const unsigned long long mk = __ballot(live);
                    if (live) {
                        // at or before every position this wave has read: the load above has returned for all lanes
                        mine[newcnt + __popcll(mk & ((1ull << lane) - 1ull))] = key;
                        lmin = key < lmin ? key : lmin;
                    }
                    newcnt += __popcll(mk);
                }
                wcnt = newcnt;
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const unsigned long long o2 = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(lmin >> 32), s) << 32) |
                                                  (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)lmin, s);
                    lmin = o2 < lmin ? o2 : lmin;
                }
                if (lane == 0) sh.wmin[w] = lmin;
                __syncthreads();
                unsigned long long g = sh.wmin[0];
#pragma unroll
                for (int q = 1; q < PNB_W; q++) g = sh.wmin[q] < g ? sh.wmin[q] : g;
                if (g == ~0ull) break;   // no live plan left
                int c[4], qi;
                pnb_decode(g, nb, x.magic, inv_d2, c, &qi);
                const int cost = (int)(g >> PN_SEQ_BITS);
                if (tid < K) {
                    const int mine_c = tid == 0 ? c[0] : tid == 1 ? c[1] : tid == 2 ? c[2] : c[3];
                    atomicOr(&sh.used[mine_c >> 5], 1u << (mine_c & 31));
                    const int qd = (s_perm[qi] >> (2 * tid)) & 3;
                    const int drop = qd == 0 ? c[0] : qd == 1 ? c[1] : qd == 2 ? c[2] : c[3];
                    int32_t *r = out + (size_t)kept * rec;
                    r[tid] = mine_c;
                    r[K + tid] = drop;
                    if (tid == 0) r[2 * K] = cost;
                }
                kept++;
                sum += cost;
                __syncthreads();   // the used bits are set, wmin may be rewritten, this wave's stores to its segment are done
                if (kept >= max_kept) break;
            }
        }
        if (tid == 0) {
            n_pools[b] = kept;
            n_happy[b] = (long long)happy;
            total[b] = sum;
        }
    }
}

// staged records -> the caller's device array: only the records a model has
__global__ void k_pooln_batched_copy(int batch, int per_model, const int32_t *__restrict__ n_pools, int rec,
                                     const int32_t *__restrict__ src, int32_t *__restrict__ dst)
{
    const size_t total = (size_t)batch * (size_t)per_model;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / (size_t)per_model;
        if ((int)((i - b * (size_t)per_model) / (size_t)rec) < n_pools[b]) dst[i] = src[i];
    }
}

Buf g_slab, g_stage, g_err;
std::vector<int32_t> g_h;

}  // namespace

void td::pool_batch_release_workspace()
{
    Buf *bs[] = {&g_slab, &g_stage, &g_err};
    for (Buf *b : bs) buf_free(*b);
}

// td_pool_n_batched's workgroup-per-model core for the world layer (td_simb_pooling_n): every array is the caller's and on the
// device, model b = the cnt[b] requests at off[b] (at most n <= 512 each), one wait / loss per model, a model outside
// k_lo[b] <= k <= k_hi[b] is empty; records go to pools + b * (n / k) * (2 k + 1) as they are.  One launch whatever the batch.
// TD_ERANGE with *over_model / *over_count set: that model has more happy plans than max_happy (*over_model = -1: a cost).
int td::pool_n_worlds(int k, int batch, int n, const int32_t *off, const int32_t *cnt, const int32_t *k_hi, const int32_t *k_lo,
                      const int32_t *from, const int32_t *to, const int32_t *wait, const int32_t *loss, const int32_t *dist, int S,
                      int64_t max_happy, int32_t *pools, int32_t *n_pools, long long *n_happy, long long *total, int *over_model,
                      long long *over_count)
{
    Ctx &c = ctx();
    const char *fn = "td_pool_n_batched";
    *over_model = -1;
    *over_count = 0;
    if (k < 2 || k > 4 || batch < 1 || n < 0 || n > PNB_MAXN || max_happy > PNB_MAX_HAPPY) return fail(TD_EINVAL, "%s: bad world call", fn);
    if (max_happy <= 0) max_happy = PNB_DEF_HAPPY;
    int rc;
    const int grid_cap = (int)std::max<size_t>(1, std::min<size_t>((size_t)PNB_GRID, PNB_SLAB_BYTES / (sizeof(unsigned long long) * (size_t)max_happy)));
    if ((rc = ensure(g_slab, sizeof(unsigned long long) * (size_t)max_happy * (size_t)grid_cap))) return rc;
    if ((rc = ensure(g_err, 256))) return rc;
    PnbErr *d_err = (PnbErr *)g_err.p;
    TD_HIP(hipMemsetAsync(d_err, 0, sizeof(PnbErr), c.stream));
    const int grid = std::min(batch, grid_cap);
    const PnbSel<true> sel{cnt, k_hi, k_lo};
    {
        ProfScope ps(TD_K_LCM);
#define TD_PNW(KV)                                                                                                                  \
    k_pooln_batched<KV, true><<<grid, PNB_T, 0, c.stream>>>(batch, n, off, from, to, wait, loss, dist, S, nullptr, (unsigned long long)max_happy, \
                                                            (unsigned long long *)g_slab.p, pools, n_pools, n_happy, total, d_err, sel)
        if (k == 2) TD_PNW(2);
        else if (k == 3) TD_PNW(3);
        else TD_PNW(4);
#undef TD_PNW
        TD_HIP(hipGetLastError());
    }
    TD_HIP(hipMemcpyAsync(c.pinned, d_err, sizeof(PnbErr), hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    const PnbErr e = *(const PnbErr *)c.pinned;
    if (e.bad) return fail(TD_EINVAL, "%s: model %d has a stand outside the %d x %d distance table", fn, batch - e.bad, S, S);
    if (e.cost) return fail(TD_ERANGE, "%s: a plan cost does not fit 14 bits", fn);
    if (e.over) {
        *over_model = batch - e.over;
        TD_HIP(hipMemcpyAsync(over_count, n_happy + *over_model, sizeof(long long), hipMemcpyDeviceToHost, c.stream));
        TD_HIP(hipStreamSynchronize(c.stream));
        return fail(TD_ERANGE, "%s: model %d has %lld happy plans, more than max_happy = %lld", fn, *over_model, *over_count, (long long)max_happy);
    }
    return TD_OK;
}

extern "C" int td_pool_n_batched(int k, int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to,
                                 const int32_t *max_wait, const int32_t *max_loss, const int32_t *dist, int S, const int32_t *first,
                                 int64_t max_happy, int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *total)
{
    TD_REQUIRE_INIT();
    Ctx &c = ctx();
    const char *fn = "td_pool_n_batched";
    if (k < 2 || k > 4) return fail(TD_EINVAL, "%s: pool size %d (2..4)", fn, k);
    if (batch < 0) return fail(TD_EINVAL, "%s: batch = %d < 0", fn, batch);
    if (n < 0 || n > PNB_MAXN) return fail(TD_EINVAL, "%s: n = %d outside [0, %d] (larger models: td_pool_n over slices)", fn, n, PNB_MAXN);
    if (dist && S <= 0) return fail(TD_EINVAL, "%s: dist given but S = %d", fn, S);
    if (max_happy > PNB_MAX_HAPPY) return fail(TD_EINVAL, "%s: max_happy = %lld above %lld", fn, (long long)max_happy, (long long)PNB_MAX_HAPPY);
    if (max_happy <= 0) max_happy = PNB_DEF_HAPPY;
    if (batch == 0) return TD_OK;
    if (!off) return fail(TD_EINVAL, "%s: null offsets", fn);
    if (!n_pools || (n / k > 0 && !pools)) return fail(TD_EINVAL, "%s: null output array", fn);
    int rc;
    if ((rc = host_copy(off, (size_t)batch + 1, g_h))) return rc;
    Ragged rg;
    if ((rc = ragged_check(fail, fn, "off", "model", g_h.data(), batch, &rg, [&](int b, int m) {
            return m > n ? fail(TD_EINVAL, "%s: model %d has %d requests, more than n = %d", fn, b, m, n) : 0;
        })))
        return rc;
    const size_t B = (size_t)batch, R = (size_t)rg.total, rec = (size_t)(2 * k + 1), per = (size_t)(n / k) * rec;
    if (R && (!from || !to || !max_wait || !max_loss)) return fail(TD_EINVAL, "%s: null request array", fn);
    // one staging block, grown in 4 MiB steps: host inputs, then the results of every model
    const int32_t *h_in[6] = {off, from, to, max_wait, max_loss, first};
    const size_t n_in[6] = {B + 1, R, R, R, R, first ? 2 * B : 0};
    bool stage[6];
    for (int q = 0; q < 6; q++) stage[q] = n_in[q] && !is_device_ptr(h_in[q]);
    int32_t *s_in[6], *s_pools, *s_np;
    long long *s_nh, *s_tot;
    auto layout = [&](Carve &cv) {
        for (int q = 0; q < 6; q++) s_in[q] = cv.take<int32_t>(stage[q] ? n_in[q] : 0);
        s_pools = cv.take<int32_t>(B * per);
        s_np = cv.take<int32_t>(B);
        s_nh = cv.take<long long>(B);
        s_tot = cv.take<long long>(B);
    };
    Carve size;
    layout(size);
    if ((rc = ensure(g_stage, (size.at + ((size_t)4 << 20) - 1) & ~(((size_t)4 << 20) - 1)))) return rc;
    Carve block(g_stage.p);
    layout(block);
    const int32_t *d_in[6];
    for (int q = 0; q < 6; q++) {
        d_in[q] = h_in[q];
        if (stage[q]) {
            TD_HIP(hipMemcpyAsync(s_in[q], q == 0 ? g_h.data() : h_in[q], sizeof(int32_t) * n_in[q], hipMemcpyHostToDevice, c.stream));
            d_in[q] = s_in[q];
        }
    }
    const void *d_dist = nullptr;
    if (dist && (rc = to_device(dist, sizeof(int32_t) * (size_t)S * S, c.stage_c, &d_dist))) return rc;
    // plan storage: workgroups in flight x max_happy keys, whatever the batch; fewer workgroups rather than more than 1 GiB
    const int grid_cap = (int)std::max<size_t>(1, std::min<size_t>((size_t)PNB_GRID, PNB_SLAB_BYTES / (sizeof(unsigned long long) * (size_t)max_happy)));
    if ((rc = ensure(g_slab, sizeof(unsigned long long) * (size_t)max_happy * (size_t)grid_cap))) return rc;
    if ((rc = ensure(g_err, 256))) return rc;
    PnbErr *d_err = (PnbErr *)g_err.p;
    TD_HIP(hipMemsetAsync(d_err, 0, sizeof(PnbErr), c.stream));
    const int grid = std::min(batch, grid_cap);
    {
        ProfScope ps(TD_K_LCM);
#define TD_PNB(KV)                                                                                                               \
    k_pooln_batched<KV><<<grid, PNB_T, 0, c.stream>>>(batch, n, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], (const int32_t *)d_dist, S, \
                                                      d_in[5], (unsigned long long)max_happy, (unsigned long long *)g_slab.p, s_pools, \
                                                      s_np, s_nh, s_tot, d_err, PnbSel<false>{})
        if (k == 2) TD_PNB(2);
        else if (k == 3) TD_PNB(3);
        else TD_PNB(4);
#undef TD_PNB
        TD_HIP(hipGetLastError());
    }
    TD_HIP(hipMemcpyAsync(c.pinned, d_err, sizeof(PnbErr), hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    const PnbErr e = *(const PnbErr *)c.pinned;
    if (e.bad) return fail(TD_EINVAL, "%s: model %d has a stand outside the %d x %d distance table", fn, batch - e.bad, S, S);
    if (e.cost) return fail(TD_ERANGE, "%s: a plan cost does not fit 14 bits", fn);
    if (n_happy) TD_HIP(hipMemcpyAsync(n_happy, s_nh, sizeof(int64_t) * B, hipMemcpyDefault, c.stream));
    if (e.over) {
        const int b = batch - e.over;
        long long cnt = 0;
        TD_HIP(hipMemcpyAsync(&cnt, s_nh + b, sizeof(cnt), hipMemcpyDeviceToHost, c.stream));
        TD_HIP(hipStreamSynchronize(c.stream));
        return fail(TD_ERANGE, "%s: model %d has %lld happy plans, more than max_happy = %lld", fn, b, cnt, (long long)max_happy);
    }
    TD_HIP(hipMemcpyAsync(n_pools, s_np, sizeof(int32_t) * B, hipMemcpyDefault, c.stream));
    if (total) TD_HIP(hipMemcpyAsync(total, s_tot, sizeof(int64_t) * B, hipMemcpyDefault, c.stream));
    if (per) {
        if (is_device_ptr(pools)) {
            const size_t cells = B * per;
            k_pooln_batched_copy<<<(int)std::min<size_t>((cells + 255) / 256, 2048), 256, 0, c.stream>>>(batch, (int)per, s_np, (int)rec,
                                                                                                     s_pools, pools);
            TD_HIP(hipGetLastError());
            TD_HIP(hipStreamSynchronize(c.stream));
        } else {
            // host destination: only the records a model has are written
            std::vector<int32_t> h_pools(B * per), h_np(B);
            TD_HIP(hipMemcpyAsync(h_pools.data(), s_pools, sizeof(int32_t) * B * per, hipMemcpyDeviceToHost, c.stream));
            TD_HIP(hipMemcpyAsync(h_np.data(), s_np, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c.stream));
            TD_HIP(hipStreamSynchronize(c.stream));
            for (size_t b = 0; b < B; b++)
                if (h_np[b] > 0) memcpy(pools + b * per, h_pools.data() + b * per, sizeof(int32_t) * (size_t)h_np[b] * rec);
        }
    } else {
        TD_HIP(hipStreamSynchronize(c.stream));
    }
    return TD_OK;
}
