// td_sim.hip — a simulator world that lives in HBM behind the C ABI (td_sim_*): Simulator.java's tick loop
// (:151-211) with the cab and request tables on the device.
//
// The specification is taxidispatcher_amd/simulator.py (Simulator.tick on a backend with .tick, i.e. _tick_one_call);
// the per-element rules are in td_sim_core.h, and the kernels that apply them in td_sim_world.h, shared with td_simb.hip:
// this file launches them on a grid (chunks, 1) with its list sizes in the kernel arguments (Seg1).  Its own are the
// handle, the fleet's first state, the ordered scatter of ONE world and the host flow.  One tick is a chain of small
// kernels around the existing td_pool2 and td_tick, all on the library's stream, one concern per kernel and the kernel
// boundary as the only barrier
// between workgroups:
//
//   begin   k_arrive                     checkIfCabAtDestination, one thread per cab (a cab touches only its own request)
//           k_flags<cab>                 "some client-less cab heads here", one bit per stand (LDS bitset per workgroup, OR-ed out)
//           k_dem_count / k_scatter      createTempDemand: the drop and the per-workgroup count in one pass, then the ordered scatter
//           k_flags<req>                 "some unassigned request starts here" (after the drop)
//           k_count / k_scatter          createTempSupply
//           td_pool2 (device lists)      findPool; under td_sim_pooling: td_pool2_loss (the candidate rule), td_pool2_batched on
//                                        the one model (the optimum), or nothing (TD_POOL_NONE: the demand is copied as it is)
//           k_pool_mark, k_count / k_scatter   analyzePool: B customers out, A customers annotated, order kept
//           under td_sim_pooling_n (sim_begin_pool_n): per stage k = k_hi .. k_lo the pool call on the device lists
//           (td_pool_n_batched on the one model, td_pool_n above 512 requests; td_pool_n_banded for every stage once
//           td_sim_pool_buffer set a plan buffer), k_pool_records (the stage's records as the
//           tick's, and analyzePool's marks), k_count / k_scatter (the rest for the next stage); then k_count / k_scatter
//           with PoolEmitN: the first pick-up carries up to three partners, the size and the cost
//   apply   k_pair_map                   first pair per cab / per request (setdefault), indices checked
//           k_apply_pairs                analyzePairs' two loops, one thread per cab / request of the model
//           k_count / k_scatter  x 2     the kept lists, ordered: what row_to_col indexes
//           k_apply_solution             analyzeSolution, one thread per (kept) cab
//
// Ordered compaction = count per workgroup, exclusive scan of the counts, scatter by rank: ascending index order is the
// reference's list order and the golden log depends on it.  The scan of the (few) workgroup counts is done by each
// scatter workgroup for itself (a bounded reduction over the counts before it): no workgroup waits for another, and the
// last one writes the list's size into the head block, so one world needs no k_offsets.  Counters are reduced per
// workgroup and added with one 64-bit atomic per workgroup.
//
// The head block (struct Head): Ctl and the sizes of the five per-tick lists (zeroed per tick), read back in one copy.
// A list's segment, the plans of td_pool2 and the decisions of td_sim_apply reach the kernels by value (Seg1, Plans1,
// Dec1): the host has their sizes from the last read-back, nothing is uploaded or loaded for them.  Only the kept
// lists' sizes are read on the device, by k_apply_solution, which is queued before they are known.
//
// A world on a distance table (td_sim_create_dist): the handle owns a copy of the table and two neighbour bit matrices built
// from it once (k_nb_build in td_sim_core.h, which also validates the table).  The near test of createTempDemand / createTempSupply is then
// one more kernel after each k_flags, k_near_b: near[s] = any(nb[s][q] & flags[q]), one wave per stand; the predicates read
// one bit of it, and arrival / dispatch / analyzeSolution read one table cell (td_sim_core.h way()).  The direction rule:
// the row of the table is always the cab's stand, dist[cab.to][request.from]:
//   nb_dem[s] bit s'  <=>  dist[s'][s] < drop_time   (request at s, a cab heading to s': a COLUMN of the table)
//   nb_sup[s] bit s'  <=>  dist[s][s'] < drop_time   (cab at s, a request starting at s': a ROW)
// A line world (dist == nullptr) launches exactly what it launched before.
//
// The route model (td_sim_route): off by default, and then every kernel above runs in its RouteOff instantiation.
// With routes on, the last compaction of sim_begin_pool_n and the kept-demand compaction carry the record index of a first
// pick-up as one more column (WithRec / KeptRec), k_apply_pairs / k_apply_solution hand the dispatched cab its stop list and
// k_arrive drives it (td_sim_core.h: route_give, route_advance); no launch is added per tick.
//
// The event log (td_sim_log / td_sim_events): off by default, and then every kernel above runs in its EvOff
// instantiation and nothing else is queued.  With the log on, k_arrive, k_dem_count, k_apply_pairs and k_apply_solution write
// their records into fixed staging slots, and the call that ends a tick queues ONE ordered flush (td_sim_world.h: k_ev_count,
// k_ev_offsets, k_ev_scatter) that appends the tick's records to the log in Simulator.java's write order.
#include <limits.h>

#include "td_sim_world.h"

using namespace td;
using namespace tdsim;

// the head block, on the device and as the host reads it back: Ctl, then this tick's list sizes (demand, supply, demand after
// pooling, the two kept lists), which td_sim's k_scatter writes
struct Head {
    Ctl ctl;
    int32_t n_dem, n_sup, n_dem2, n_ks, n_kd;
    int32_t n_stage;   // td_sim_pooling_n: the requests the last stage compaction kept; begin checks it against the pool counts
};

// what td_sim_pooling_n adds to a handle, allocated by its first call: nothing of it is touched per tick by another policy
struct PoolNDev {
    int32_t *wait = nullptr, *loss = nullptr;        // the world's scalar rule, once per request slot
    int32_t *st_from[2], *st_to[2], *st_map[2];      // a stage's request list and its positions in the tick's demand list
    int32_t *used = nullptr;                         // a stage's requests that its pools took
    int32_t *out = nullptr;                          // a stage's records as the pool call writes them
    int32_t *recs = nullptr, *size = nullptr;        // the tick's plans: 9 ints each, and their sizes
    int32_t *d2_more[2], *kd_more[2];                // the third and fourth pick-up of the demand after pooling / the kept demand
};

// what td_sim_route adds to a handle, allocated by its first call with on != 0
struct RouteDev {
    int32_t *stops = nullptr, *pos = nullptr, *r_drop = nullptr;   // 8 stop words and a position per cab, the drop-off tick per request
    int32_t *d2_rec = nullptr, *kd_rec = nullptr;                  // the record of each customer of the demand after pooling / the kept demand
    long long *cnt = nullptr;                                      // drop_numb, ride_time, solo_time, max_over_loss
};

struct td_sim : SimDev, SimPin {   // td_sim_layout.h: every device array of the handle, and the pinned block
    World w;
    int max_non_lcm = 0;
    int cap = 1;                 // capacity of every per-tick list: max(n_cabs, n_req, 1)
    int words = 0;               // of one stand bitset
    Buf mem;                     // the device block
    Head *head = nullptr;        // = head_blk
    Ctl *ctl = nullptr;          // = &head->ctl
    void *pin = nullptr;         // the pinned block: the head's read-back at its front
    // sequencing
    int last_t = -1;
    bool begun = false;          // a tick with demand waits for td_sim_apply
    int n_dem = 0, n_sup = 0, n_dem2 = 0;
    int n_pool = 0;              // this tick's plans (the event log reads them where td_pool2 left them)
    int n_pooled = 0;            // the customers findPool looked at in this tick: the demand, or 0 where it did not run
    int pool_mode = TD_POOL_GREEDY;   // td_sim_pooling: the policy from the next begin on
    double max_loss = 0.0;            // <= 0: every ordered pair is a candidate
    // td_sim_pooling_n: pools of pn_hi down to pn_lo from the next begin on; pn_hi == 0: the pair policy above holds
    int pn_hi = 0, pn_lo = 0, pn_wait = 0, pn_loss = 0;
    int64_t pn_max_happy = 0;
    int64_t pn_buffer = 0;       // td_sim_pool_buffer: > 0: every stage is td_pool_n_banded with this plan buffer
    PoolNDev pn;
    Buf pn_mem;
    // td_sim_dispatch: the dispatch method from the next begin on.  The world kernels take the LCM rule as one number
    // ("the LCM ran when the model is larger than it"), so a policy is that number: lcm_rule() below.
    int disp_mode = TD_DISPATCH_LCM_OPT, disp_parts = 4;
    // the model size above which the LCM ran in this world: its max_non_lcm; -1 where it always runs (with supply a model has
    // at least one row); INT_MAX where it never does
    int lcm_rule() const { return disp_mode == TD_DISPATCH_LCM_OPT ? max_non_lcm : disp_mode == TD_DISPATCH_LCM ? -1 : INT_MAX; }
    EvLog ev;                    // td_sim_log
    // td_sim_route: route_on: the apply kernels hand out routes from the next begin on; rt_mem.p: the handle has route
    // storage, and k_arrive drives what is in it (cabs mid-route finish theirs after on = 0)
    bool route_on = false;
    RouteDev rt;
    Buf rt_mem;
    RouteOn route() const { return RouteOn{rt.stops, rt.pos, rt.r_drop, rt.cnt, pn_loss, pn.recs, dem_idx, rt.d2_rec, rt.kd_rec}; }
    // the host side of Simulator.m
    int64_t lcm_used = 0, max_model = 0, max_solver = 0, max_pool_mem = 0, max_pool = 0;
};

namespace {

constexpr int SIM_POOL_OPT_NMAX = 2048;   // largest model of td_pool2_batched: the optimum of a tick is one such model
static_assert(sizeof(Head) <= sizeof(int32_t) * SIM_HEAD_INTS && sizeof(Head) <= SIM_PIN_HEAD, "the head fits its device block and the pinned block's front");

// world 0's segment of a list: it begins at 0; its size is the host's (n), or still on the device (dev non-null: a kept list)
struct Seg1 {
    int n;
    const int32_t *dev;
    __device__ __forceinline__ void operator()(int, int *lo, int *cnt) const
    {
        *lo = 0;
        *cnt = dev ? *dev : n;
    }
};

// the plans of td_pool2 over the n customers of the demand list: k of them, from the front of the list
struct Plans1 {
    int k, n;
    __device__ int n_act(int) const { return n; }
    __device__ int count(int) const { return k; }
    __device__ int base(int) const { return 0; }
};

// td_sim_pooling_n, one stage of the cascade: record p of the pool call (2 K + 1 ints, members = positions in the stage's list)
// becomes plan base + p of the tick (9 ints, members = positions in the tick's demand list through `map`; nullptr: the first
// stage, whose list is the demand list).  analyzePool's marks with it: every member but the first pick-up leaves (isb), the
// first pick-up gets its plan (ainfo), and the stage's list forgets all of them (used).  pl_a / pl_b: first and second
// pick-up, where the event log reads a pair.  A member outside its list raises the error word.
__global__ __launch_bounds__(256) void k_pool_records(int K, int np, int base, int cap_plans, int m_stage, int n_dem,
                                                      const int32_t *__restrict__ out, const int32_t *__restrict__ map,
                                                      int32_t *__restrict__ recs, int32_t *__restrict__ size, int32_t *__restrict__ pl_a,
                                                      int32_t *__restrict__ pl_b, int32_t *__restrict__ used, int32_t *__restrict__ isb,
                                                      int32_t *__restrict__ ainfo, int32_t *gerr)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    if (base + p >= cap_plans) {
        atomicMax(gerr, 1);
        return;
    }
    const int32_t *r = out + (size_t)p * (size_t)(2 * K + 1);
    int pick[4] = {-1, -1, -1, -1}, drop[4] = {-1, -1, -1, -1};
    bool bad = false;
    for (int i = 0; i < K; i++) {
        const int a = r[i], d = r[K + i];
        if (a < 0 || a >= m_stage || d < 0 || d >= m_stage) {
            bad = true;
            continue;
        }
        pick[i] = map ? map[a] : a;
        drop[i] = map ? map[d] : d;
        bad = bad || pick[i] < 0 || pick[i] >= n_dem || drop[i] < 0 || drop[i] >= n_dem;
    }
    if (bad) {
        atomicMax(gerr, 1);
        return;
    }
    int32_t *o = recs + (size_t)9 * (size_t)(base + p);
    for (int i = 0; i < 4; i++) {
        o[i] = pick[i];
        o[4 + i] = drop[i];
    }
    o[8] = r[2 * K];
    size[base + p] = K;
    pl_a[base + p] = pick[0];
    pl_b[base + p] = pick[1];
    atomicMin(&ainfo[pick[0]], base + p);
    for (int i = 0; i < K; i++) {
        used[r[i]] = 1;
        if (i) isb[pick[i]] = 1;
    }
}

// the requests a stage leaves to the next one, in list order, with their positions in the tick's demand list
struct StageEmit {
    const int32_t *from, *to, *map;
    int32_t *from2, *to2, *map2;
    __device__ void operator()(int o, int, int i, int) const
    {
        from2[o] = from[i];
        to2[o] = to[i];
        map2[o] = map ? map[i] : i;
    }
};

__global__ __launch_bounds__(256) void k_fill2(int n, int32_t *__restrict__ a, int va, int32_t *__restrict__ b, int vb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a[i] = va;
    b[i] = vb;
}

// this tick's decisions as td_sim_apply got them
struct Dec1 {
    const int32_t *rows, *cols, *r2c;
    int n_pairs, n_r2c, solved;
    __device__ void pairs(int, int *base, int *cnt) const
    {
        *base = 0;
        *cnt = n_pairs;
    }
    __device__ void r2c_of(int, bool, int, int *base, int *nr, bool *sol) const
    {
        *base = 0;
        *sol = solved != 0;
        *nr = solved ? n_r2c : 0;
    }
};

// the route storage's first state: no stop anywhere, nobody dropped off, the counters empty
__global__ __launch_bounds__(256) void k_route_init(int n_cabs, int n_req, int32_t *__restrict__ stops, int32_t *__restrict__ pos,
                                                    int32_t *__restrict__ r_drop, long long *__restrict__ cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 8 * n_cabs) stops[i] = -1;
    if (i < n_cabs) pos[i] = 0;
    if (i < n_req) r_drop[i] = -1;
    if (i < 4) cnt[i] = i == 3 ? INT64_MIN : 0;
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

// out[base + rank] = element of [0, n), base = the counts of the workgroups before this one; the last workgroup writes the total
template <class P, class E>
__global__ __launch_bounds__(CB) void k_scatter(int n, P pred, E emit, const int32_t *__restrict__ blockcnt, int32_t *__restrict__ total)
{
    __shared__ int s_red[16];
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += CB) part += blockcnt[j];
    const int base = block_sum(part, s_red);
    const int i = blockIdx.x * CB + threadIdx.x;
    const bool f = i < n && pred(i, 0);
    int tot;
    const int rank = block_rank(f, s_red, &tot);
    if (f) emit(base + rank, -1, i, 0);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = base + tot;
}

inline int nblocks(int n) { return (n + CB - 1) / CB; }

// ordered compaction of [0, n): *total (device) = how many; n == 0 leaves *total as the tick's memset zeroed it
template <class P, class E>
int compact(td_sim *s, int n, const P &pred, const E &emit, int32_t *total)
{
    if (n <= 0) return TD_OK;
    Ctx &c = ctx();
    k_count<Seg1, P><<<nblocks(n), CB, 0, c.stream>>>(Seg1{n, nullptr}, pred, s->blockcnt);
    k_scatter<P, E><<<nblocks(n), CB, 0, c.stream>>>(n, pred, emit, s->blockcnt, total);
    TD_HIP(hipGetLastError());
    return TD_OK;
}

// the device counters and list sizes on the host (one copy, one stream synchronisation)
int read_head(td_sim *s, Head *out)
{
    Ctx &c = ctx();
    TD_HIP(hipMemcpyAsync(s->pin, s->head, sizeof(Head), hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    *out = *(const Head *)s->pin;
    return TD_OK;
}

// the event log: this tick's records, sections `phase`, behind the log.  The host has every list size.
int sim_ev_flush(td_sim *s, int phase)
{
    const World &w = s->w;
    const EvLog &e = s->ev;
    const Seg1 cabs{w.n_cabs, nullptr}, reqs{w.n_req, nullptr}, dem{s->n_dem, nullptr}, sup{s->n_sup, nullptr}, d2{s->n_dem2, nullptr};
    const EvSrc<Seg1, Plans1> src{w, cabs, reqs, dem, sup, d2, Plans1{s->n_pool, s->n_pooled}, LcmRule1{s->lcm_rule()}, s->last_t, phase, e.kinds,
                                  e.st_arr, e.st_drop, e.st_pairs, e.st_sol, s->dem_idx, s->pl_a, s->pl_b};
    const size_t vmax = (size_t)w.n_cabs + w.n_req + 2 + s->n_dem + s->n_pool + 2 * ((size_t)s->n_sup + s->n_dem2) + 2 * (size_t)s->n_sup;
    return ev_flush(s->ev, src, 1, vmax);
}

// a tick is over (nothing to apply, or applied): what the log has not seen of it goes there
int sim_ev_tick_done(td_sim *s)
{
    if (!s->ev.kinds) return TD_OK;
    const int phase = s->ev.begin_flushed ? 2 : 3;
    s->ev.begin_flushed = false;
    return sim_ev_flush(s, phase);
}

constexpr int SIM_POOL_N_NMAX = 2047;   // td_pool_n's largest model
constexpr int SIM_POOL_NB_NMAX = 512;   // td_pool_n_batched's

// findPool and analyzePool of a tick under td_sim_pooling_n (the specification: Simulator.find_pool_n / analyze_pool_n).  The
// cascade runs on the device lists: stage k is td_pool_n_batched's device code on the one model (up to 512 requests) or
// td_pool_n with every request as a possible first pick-up (up to 2047), each with device inputs and a device destination;
// k_pool_records translates and marks, one compaction hands the rest to the next stage.  The host learns a stage's pool
// count from the pool call itself and derives the next list's size from it: a stage adds no read-back of its own.
int sim_begin_pool_n(td_sim *s, int t, int32_t info[4])
{
    Ctx &c = ctx();
    const int n = s->n_dem;
    const PoolNDev &pn = s->pn;
    int rc;
    if (n > SIM_POOL_N_NMAX)
        return fail(TD_EINVAL, "td_sim_begin: world 0 has %d requests before pooling in tick %d, more than the %d td_pool_n takes", n, t,
                    SIM_POOL_N_NMAX);
    s->n_pooled = n;
    TD_HIP(hipMemsetAsync(s->isb, 0, sizeof(int32_t) * (size_t)n, c.stream));
    TD_HIP(hipMemsetAsync(s->ainfo, 0x7f, sizeof(int32_t) * (size_t)n, c.stream));
    const int cap_plans = std::max(s->w.n_req, 1) / 2 + 1, S = s->dist ? s->w.n_stands : 0;   // what pl_a / pl_b hold; recs and size hold no less
    int total = 0, m = n, cur = 0, m_left = -1;   // m_left: what the last compaction between two stages must have counted
    int64_t happy = 0;
    const int32_t *from = s->dem_from, *to = s->dem_to, *map = nullptr;
    for (int k = s->pn_hi; k >= s->pn_lo && n >= 2; k--) {
        if (m < k) continue;   // a stage list shorter than its k yields no pools
        int32_t np = 0;
        int64_t nh = 0;
        if (s->pn_buffer > 0) {
            rc = td_pool_n_banded(k, m, from, to, pn.wait, pn.loss, s->dist, S, 0, m, s->pn_buffer, m / k + 1, pn.out, &np, &nh, nullptr);
        } else if (m <= SIM_POOL_NB_NMAX) {
            const int32_t off[2] = {0, m};
            rc = td_pool_n_batched(k, 1, m, off, from, to, pn.wait, pn.loss, s->dist, S, nullptr, s->pn_max_happy, pn.out, &np, &nh, nullptr);
        } else {
            rc = td_pool_n(k, m, from, to, pn.wait, pn.loss, s->dist, S, 0, m, s->pn_max_happy, m / k + 1, pn.out, &np, &nh);
        }
        if (rc) return rc;
        happy += nh;
        if (np <= 0) continue;
        if (np > m / k) return fail(TD_EINTERNAL, "td_sim_begin: %d pools of %d among %d requests", np, k, m);
        TD_HIP(hipMemsetAsync(pn.used, 0, sizeof(int32_t) * (size_t)m, c.stream));
        k_pool_records<<<(np + 255) / 256, 256, 0, c.stream>>>(k, np, total, cap_plans, m, n, pn.out, map, pn.recs, pn.size, s->pl_a, s->pl_b,
                                                              pn.used, s->isb, s->ainfo, &s->ctl->err);
        TD_HIP(hipGetLastError());
        total += np;
        if (k > s->pn_lo) {   // the requests this stage did not pool, in list order, for the next one
            if ((rc = compact(s, m, PoolPred{pn.used}, StageEmit{from, to, map, pn.st_from[cur], pn.st_to[cur], pn.st_map[cur]}, &s->head->n_stage)))
                return rc;
            from = pn.st_from[cur], to = pn.st_to[cur], map = pn.st_map[cur];
            cur ^= 1;
            m -= k * np;   // pools of a stage share no request
            m_left = m;
        }
    }
    if (n >= 2) {
        s->max_pool_mem = std::max(s->max_pool_mem, happy);
        s->max_pool = std::max(s->max_pool, (int64_t)total);
    }
    s->n_pool = total;
    const Seg1 dem{n, nullptr};
    auto pooled = [&](auto emit) {   // with routes the record of a first pick-up travels beside its columns
        if (s->route_on) return compact(s, n, PoolPred{s->isb}, WithRec<decltype(emit)>{emit, s->ainfo, total, s->rt.d2_rec}, &s->head->n_dem2);
        return compact(s, n, PoolPred{s->isb}, emit, &s->head->n_dem2);
    };
    if (s->pn_hi > 2)
        rc = pooled(PoolEmitN<3, Seg1>{dem, total, s->dem_idx, s->dem_from, s->ainfo, pn.recs, pn.size, s->d2_idx, s->d2_from, s->d2_partner,
                                       s->d2_plan, s->d2_cost, {pn.d2_more[0], pn.d2_more[1]}});
    else
        rc = pooled(PoolEmitN<1, Seg1>{dem, total, s->dem_idx, s->dem_from, s->ainfo, pn.recs, pn.size, s->d2_idx, s->d2_from, s->d2_partner,
                                       s->d2_plan, s->d2_cost, {nullptr, nullptr}});
    if (rc) return rc;
    Head h;
    if ((rc = read_head(s, &h))) return rc;
    if (h.ctl.err) return fail(TD_EINTERNAL, "td_sim: a pool record names a customer outside the demand list");
    if (m_left >= 0 && h.n_stage != m_left)
        return fail(TD_EINTERNAL, "td_sim_begin: a stage of tick %d left %d requests on the device, %d by the pool counts", t, h.n_stage, m_left);
    s->n_dem2 = h.n_dem2;
    info[3] = h.n_dem2;
    s->max_model = std::max(s->max_model, (int64_t)std::max(s->n_sup, s->n_dem2));
    return TD_OK;
}

int sim_begin(td_sim *s, int t, int32_t info[4])
{
    Ctx &c = ctx();
    const World &w = s->w;
    int rc;
    info[0] = info[1] = info[2] = info[3] = 0;
    // this tick's list sizes start from zero; the sums and the error word stay (k_arrive zeroes the OPT count)
    TD_HIP(hipMemsetAsync(&s->head->n_dem, 0, sizeof(int32_t) * 5, c.stream));
    const int words = s->words;
    TD_HIP(hipMemsetAsync(s->bits, 0, sizeof(uint32_t) * 2 * (size_t)words, c.stream));
    const size_t shm = sizeof(uint32_t) * (size_t)words;
    const Seg1 cabs{w.n_cabs, nullptr}, reqs{w.n_req, nullptr};
    const bool log = s->ev.kinds != 0;
    s->n_pool = s->n_pooled = 0;
    if (log)
        k_arrive<<<nblocks(w.n_cabs), CB, 0, c.stream>>>(w, cabs, t, s->ctl, EvOn{s->ev.st_arr}, RouteOff{});
    else if (s->rt_mem.p)   // a handle with route storage never logs
        k_arrive<<<nblocks(w.n_cabs), CB, 0, c.stream>>>(w, cabs, t, s->ctl, EvOff{}, s->route());
    else
        k_arrive<<<nblocks(w.n_cabs), CB, 0, c.stream>>>(w, cabs, t, s->ctl, EvOff{}, RouteOff{});
    k_flags<<<nblocks(w.n_cabs), CB, shm, c.stream>>>(cabs, w.n_stands, w.c_to, w.c_clnt, s->bits, 0);
    if (s->dist) k_near_b<<<near_grid(1, words), CB, near_lds(words), c.stream>>>(1, w.n_stands, words, s->nb_dem, s->bits, s->near, 0);
    if (w.n_req > 0) {
        const DemPred dp{w, t, words, s->bits, s->near};
        if (log)
            k_dem_count<<<nblocks(w.n_req), CB, 0, c.stream>>>(dp, reqs, s->blockcnt, s->ctl, EvOn{s->ev.st_drop});
        else
            k_dem_count<<<nblocks(w.n_req), CB, 0, c.stream>>>(dp, reqs, s->blockcnt, s->ctl, EvOff{});
        k_scatter<DemPred, DemEmit><<<nblocks(w.n_req), CB, 0, c.stream>>>(
            w.n_req, dp, DemEmit{w, s->dem_idx, s->dem_from, s->dem_to, nullptr, nullptr}, s->blockcnt, &s->head->n_dem);
        k_flags<<<nblocks(w.n_req), CB, shm, c.stream>>>(reqs, w.n_stands, w.r_from, w.r_cab, s->bits, 1);
    }
    if (s->dist) k_near_b<<<near_grid(1, words), CB, near_lds(words), c.stream>>>(1, w.n_stands, words, s->nb_sup, s->bits, s->near, 1);
    TD_HIP(hipGetLastError());
    // createTempSupply changes nothing, so it is queued before the demand count is known: one read-back for both
    if ((rc = compact(s, w.n_cabs, SupPred{w, words, s->bits, s->near}, SupEmit{w, s->sup_cab, s->sup_to}, &s->head->n_sup))) return rc;
    Head h;
    if ((rc = read_head(s, &h))) return rc;
    if (h.ctl.err) return fail(TD_EINTERNAL, "td_sim: device error word %d", h.ctl.err);
    s->last_t = t;
    s->n_dem = h.n_dem;
    s->n_sup = s->n_dem2 = 0;
    if (h.n_dem == 0) return sim_ev_tick_done(s);   // Simulator.java:160: nothing to do in this tick
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
    if (s->pn_hi) return sim_begin_pool_n(s, t, info);
    const bool find = s->pool_mode != TD_POOL_NONE;   // NONE: no findPool; the demand list is copied below as it is, no mark set
    if (find) s->n_pooled = n;
    if (find && n >= 2) {
        const int S = s->dist ? w.n_stands : 0;
        if (s->pool_mode == TD_POOL_OPTIMAL && n > SIM_POOL_OPT_NMAX)
            return fail(TD_EINVAL, "td_sim_begin: world 0 has %d requests before pooling in tick %d, more than the %d an optimal pool model holds", n,
                        t, SIM_POOL_OPT_NMAX);
        s->max_pool_mem = std::max(s->max_pool_mem, (int64_t)n * (n - 1));   // the pairs examined, whatever the rule admits
        if (s->pool_mode == TD_POOL_OPTIMAL) {   // the batched call's device code on one model: its plans lie at 0 .. k
            const int32_t off[2] = {0, n};
            int64_t tot = 0;
            rc = td_pool2_batched(1, n, off, s->dem_from, s->dem_to, s->dist, S, s->max_loss, 1, s->pl_a, s->pl_b, s->pl_plan, s->pl_cost, &k, &tot);
        } else if (s->max_loss > 0) {
            rc = td_pool2_loss(n, s->dem_from, s->dem_to, s->dist, S, s->max_loss, s->pl_a, s->pl_b, s->pl_plan, s->pl_cost, &k);
        } else {
            rc = td_pool2(n, s->dem_from, s->dem_to, s->dist, S, s->pl_a, s->pl_b, s->pl_plan, s->pl_cost, &k);
        }
        if (rc) return rc;
        s->max_pool = std::max(s->max_pool, (int64_t)k);
        s->n_pool = k;
    }
    TD_HIP(hipMemsetAsync(s->isb, 0, sizeof(int32_t) * (size_t)n, c.stream));
    TD_HIP(hipMemsetAsync(s->ainfo, 0x7f, sizeof(int32_t) * (size_t)n, c.stream));
    const Plans1 pl{k, n};
    const Seg1 dem{n, nullptr};
    if (k > 0) k_pool_mark<<<(k + 255) / 256, 256, 0, c.stream>>>(pl, dem, s->pl_a, s->pl_b, s->isb, s->ainfo, &s->ctl->err);
    if ((rc = compact(s, n, PoolPred{s->isb},
                      PoolEmit<Plans1, Seg1>{pl, dem, s->dem_idx, s->dem_from, s->ainfo, s->pl_b, s->pl_plan, s->pl_cost, s->d2_idx, s->d2_from,
                                             s->d2_partner, s->d2_plan, s->d2_cost, nullptr},
                      &s->head->n_dem2)))
        return rc;
    if ((rc = read_head(s, &h))) return rc;
    if (h.ctl.err) return fail(TD_EINTERNAL, "td_sim: a pool plan names a customer outside the demand list");
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
    const LcmRule1 mnl{s->lcm_rule()};
    int rc;
    *opt_count = 0;
    if (s->disp_mode == TD_DISPATCH_LCM) solved = 0;   // the LCM alone: never a solution, whatever the caller says
    if (n_s == 0) {   // no supply: analyzeSolution walks an empty list, the line ends in "; OPT count=0"
        s->begun = false;
        return sim_ev_tick_done(s);
    }
    const bool log = s->ev.kinds != 0;
    // pools of three or four: the partner columns behind the first travel with the apply kernels (such a handle never logs)
    const bool more = s->pn_hi > 2;
    // routes (td_sim_route): the apply kernels hand out stop lists; only a tick that pooled by records has the record column
    const bool route = s->route_on && s->pn_hi > 0;
    auto px3 = [&] { return MorePartners<3>{{s->pn.d2_more[0], s->pn.d2_more[1]}, {s->pn.kd_more[0], s->pn.kd_more[1]}}; };
    if (log && (rc = ev_clear_apply(s->ev, (size_t)n_s, (size_t)n_d))) return rc;
    const bool lcm = n > mnl.v;
    if (lcm && !solved) *opt_count = -1;
    const int nr = solved ? n_r2c : 0;
    const Dec1 dec{s->in_rows, s->in_cols, s->in_r2c, n_pairs, nr, solved};
    int32_t *gerr = &s->ctl->err;
    const Seg1 cabs{w.n_cabs, nullptr}, sup{n_s, nullptr}, d2{n_d, nullptr};
    if (lcm) {
        if ((rc = put(s->in_rows, rows, (size_t)n_pairs)) || (rc = put(s->in_cols, cols, (size_t)n_pairs))) return rc;
        TD_HIP(hipMemsetAsync(s->pair_cab, 0x7f, sizeof(int32_t) * (size_t)n_s, c.stream));
        TD_HIP(hipMemsetAsync(s->pair_dem, 0x7f, sizeof(int32_t) * (size_t)n_d, c.stream));
        if (n_pairs > 0) k_pair_map<<<(n_pairs + 255) / 256, 256, 0, c.stream>>>(dec, mnl, sup, d2, s->pair_cab, s->pair_dem, gerr);
        auto pairs = [&](auto ev, auto px, auto rt) {
            k_apply_pairs<<<nblocks(n_s + n_d), CB, 0, c.stream>>>(w, t, dec, mnl, cabs, sup, d2, s->pair_cab, s->pair_dem, s->sup_cab,
                                                                 s->sup_to, s->d2_idx, s->d2_partner, s->d2_cost, s->ctl, gerr, ev, px, rt);
        };
        if (route && more)
            pairs(EvOff{}, px3(), s->route());
        else if (route)
            pairs(EvOff{}, MorePartners<1>{}, s->route());
        else if (more)
            pairs(EvOff{}, px3(), RouteOff{});
        else if (log)
            pairs(EvOn{s->ev.st_pairs}, MorePartners<1>{}, RouteOff{});
        else
            pairs(EvOff{}, MorePartners<1>{}, RouteOff{});
        TD_HIP(hipGetLastError());
        if ((rc = compact(s, n_s, KeptPred<Seg1>{s->pair_cab, sup, d2, mnl}, KeptSupEmit{s->sup_cab, s->sup_to, s->ks_cab, s->ks_to},
                          &s->head->n_ks)))
            return rc;
        const KeptDemEmit ke{s->d2_idx, s->d2_from, s->d2_partner, s->d2_plan, s->d2_cost, s->kd_idx, s->kd_from, s->kd_partner, s->kd_plan, s->kd_cost};
        auto kept = [&](auto emit) {   // with routes the record column travels to the kept demand too
            if (route) return compact(s, n_d, KeptPred<Seg1>{s->pair_dem, sup, d2, mnl}, KeptRec<decltype(emit)>{emit, s->rt.d2_rec, s->rt.kd_rec}, &s->head->n_kd);
            return compact(s, n_d, KeptPred<Seg1>{s->pair_dem, sup, d2, mnl}, emit, &s->head->n_kd);
        };
        if (more)
            rc = kept(KeptDemEmitN<3>{ke, {s->pn.d2_more[0], s->pn.d2_more[1]}, {s->pn.kd_more[0], s->pn.kd_more[1]}});
        else
            rc = kept(ke);
        if (rc) return rc;
    }
    if (!lcm || solved) {
        if ((rc = put(s->in_r2c, r2c, (size_t)nr))) return rc;
        // the kernel takes the kept lists where the LCM ran (their sizes are on the device), else the whole model
        const Seg1 ks{0, &s->head->n_ks}, kd{0, &s->head->n_kd};
        auto solution = [&](auto ev, auto px, auto rt) {
            k_apply_solution<<<nblocks(n_s), CB, 0, c.stream>>>(w, t, dec, mnl, cabs, sup, d2, ks, kd, s->sup_cab, s->sup_to, s->d2_idx, s->d2_from,
                                                              s->d2_partner, s->d2_plan, s->d2_cost, s->ks_cab, s->ks_to, s->kd_idx, s->kd_from,
                                                              s->kd_partner, s->kd_plan, s->kd_cost, s->ctl, gerr, ev, px, rt);
        };
        if (route && more)
            solution(EvOff{}, px3(), s->route());
        else if (route)
            solution(EvOff{}, MorePartners<1>{}, s->route());
        else if (more)
            solution(EvOff{}, px3(), RouteOff{});
        else if (log)
            solution(EvOn{s->ev.st_sol}, MorePartners<1>{}, RouteOff{});
        else
            solution(EvOff{}, MorePartners<1>{}, RouteOff{});
        TD_HIP(hipGetLastError());
    }
    Head h;
    if ((rc = read_head(s, &h))) return rc;
    if (h.ctl.err) {
        // nothing was applied (every kernel after the failing one is skipped): the tick still waits for its decisions
        TD_HIP(hipMemsetAsync(gerr, 0, sizeof(int32_t), c.stream));
        TD_HIP(hipStreamSynchronize(c.stream));
        if (h.ctl.err == 2) return fail(TD_EINVAL, "td_sim_apply: a pair lies outside the model (%d cabs, %d requests)", n_s, n_d);
        return fail(TD_EINTERNAL, "td_sim: device error word %d", h.ctl.err);
    }
    s->begun = false;
    if (lcm) s->lcm_used++;
    if (!lcm || solved) {
        *opt_count = h.ctl.opt_count;
        s->max_solver = std::max(s->max_solver, (int64_t)(lcm ? std::max(h.n_ks, h.n_kd) : n));
    }
    return sim_ev_tick_done(s);
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
    std::vector<int32_t> h;
    int rc = load_requests(n_req, req_id, req_from, req_to, req_at, h);
    if (rc) return rc;
    const int i = bad_request(h, n_req, n_stands, 0, n_req);
    if (i >= 0)
        return fail(TD_EINVAL, "td_sim_create: request %d (id %d, from %d, to %d, at %d) is outside the world", i, h[i], h[(size_t)n_req + i],
                    h[(size_t)2 * n_req + i], h[(size_t)3 * n_req + i]);
    if (!ids_unique(h, 0, n_req)) return fail(TD_EINVAL, "td_sim_create: request ids must be unique");
    td_sim *s = new td_sim();
    s->max_non_lcm = max_non_lcm;
    const size_t nr = (size_t)std::max(n_req, 1), nc = (size_t)n_cabs, cap = std::max(nr, nc), words = (size_t)(n_stands + 31) / 32;
    s->cap = (int)cap;
    s->words = (int)words;
    const SimDims dims{nc, nr, cap, words, (cap + CB - 1) / CB, (size_t)n_stands, dist != nullptr};
    rc = carve_buf(s->mem, [&](Carve &cv) { sim_layout(cv, dims, *s); });
    if (rc) {
        delete s;
        return rc;
    }
    s->head = (Head *)s->head_blk;
    s->ctl = &s->head->ctl;
    World &w = s->w;
    w = World{n_cabs, n_req, n_stands, drop_time, big_cost};
    set_tables(w, *s, s->dist);
    auto bail = [&](int code) {
        td_sim_destroy(s);
        return code;
    };
    Carve pin_size;
    sim_pin_layout(pin_size, dims, *s);
    hipError_t e = hipHostMalloc(&s->pin, pin_size.at, hipHostMallocDefault);
    if (e != hipSuccess) {
        s->pin = nullptr;
        return bail(hip_fail(e, "hipHostMalloc(td_sim)"));
    }
    Carve pin(s->pin);
    sim_pin_layout(pin, dims, *s);
    if ((e = hipMemsetAsync(s->ctl, 0, sizeof(int32_t) * SIM_HEAD_INTS, c.stream)) != hipSuccess) return bail(hip_fail(e, "hipMemsetAsync"));
    int32_t *dst[4] = {s->r_id, s->r_from, s->r_to, s->r_at};
    for (int q = 0; q < 4 && n_req; q++)
        if ((e = hipMemcpyAsync(dst[q], h.data() + (size_t)q * n_req, sizeof(int32_t) * (size_t)n_req, hipMemcpyHostToDevice, c.stream)) != hipSuccess)
            return bail(hip_fail(e, "hipMemcpyAsync(request table)"));
    k_init_fleet<<<(n_cabs + 255) / 256, 256, 0, c.stream>>>(w);
    if (n_req) k_init_requests<<<(n_req + 255) / 256, 256, 0, c.stream>>>(w);
    if ((e = hipGetLastError()) != hipSuccess) return bail(hip_fail(e, "td_sim_create launch"));
    if (dist && (rc = table_upload("td_sim_create_dist launch", dist, n_stands, (int)words, drop_time, s->dist, s->nb_dem, s->nb_sup, &s->ctl->err)))
        return bail(rc);
    if ((e = hipStreamSynchronize(c.stream)) != hipSuccess) return bail(hip_fail(e, "hipStreamSynchronize"));   // `h` leaves scope
    if (dist) {
        Head hd;
        if ((rc = read_head(s, &hd)) || (rc = table_verdict("td_sim_create_dist", hd.ctl.err))) return bail(rc);
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
    buf_free(s->pn_mem);
    buf_free(s->rt_mem);
    ev_off(s->ev);
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

extern "C" int td_sim_pooling(td_sim *s, int mode, double max_loss)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (mode < TD_POOL_NONE || mode > TD_POOL_OPTIMAL) return fail(TD_EINVAL, "td_sim_pooling: mode = %d outside 0 .. 2", mode);
    if (max_loss != max_loss) return fail(TD_EINVAL, "td_sim_pooling: max_loss is not a number");
    if (s->begun) return fail(TD_EINVAL, "td_sim_pooling: tick %d still waits for td_sim_apply", s->last_t);
    if (s->route_on) return fail(TD_EINVAL, "td_sim_pooling: routes are on (td_sim_route) and pairs have no drop-off order to drive; switch them off first");
    s->pool_mode = mode;
    s->max_loss = max_loss;
    s->pn_hi = s->pn_lo = 0;   // back on a pair policy
    return TD_OK;
}

extern "C" int td_sim_pooling_n(td_sim *s, int k_hi, int k_lo, int max_wait, int max_loss_pct, int64_t max_happy)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!(2 <= k_lo && k_lo <= k_hi && k_hi <= 4)) return fail(TD_EINVAL, "td_sim_pooling_n: k_hi = %d, k_lo = %d outside 2 <= k_lo <= k_hi <= 4", k_hi, k_lo);
    if (max_wait < 0 || max_loss_pct < 0) return fail(TD_EINVAL, "td_sim_pooling_n: max_wait = %d, max_loss_pct = %d: nothing negative", max_wait, max_loss_pct);
    if (max_happy > ((int64_t)1 << 22)) return fail(TD_EINVAL, "td_sim_pooling_n: max_happy = %lld above %lld", (long long)max_happy, 1ll << 22);
    if (s->begun) return fail(TD_EINVAL, "td_sim_pooling_n: tick %d still waits for td_sim_apply", s->last_t);
    if (k_hi > 2 && s->ev.kinds)
        return fail(TD_EINVAL, "td_sim_pooling_n: not built: the event log of pools of three and four (the handle logs; k_hi = 2 can be logged)");
    Ctx &c = ctx();
    PoolNDev &pn = s->pn;
    if (!s->pn_mem.p) {   // the handle's, from the first call on: nothing is allocated per tick
        const size_t cap = (size_t)s->cap, plans = cap / 2 + 1;
        PoolNDev d;
        int rc = carve_buf(s->pn_mem, [&](Carve &cv) {
            for (int32_t **a : {&d.wait, &d.loss, &d.st_from[0], &d.st_from[1], &d.st_to[0], &d.st_to[1], &d.st_map[0], &d.st_map[1], &d.used,
                                &d.d2_more[0], &d.d2_more[1], &d.kd_more[0], &d.kd_more[1]})
                *a = cv.take<int32_t>(cap);
            d.out = cv.take<int32_t>(3 * cap + 9);   // (m / k) records of 2 k + 1 ints: at most 2.5 m
            d.recs = cv.take<int32_t>(9 * plans);
            d.size = cv.take<int32_t>(plans);
        });
        if (rc) return rc;
        pn = d;
    }
    k_fill2<<<(s->cap + 255) / 256, 256, 0, c.stream>>>(s->cap, pn.wait, max_wait, pn.loss, max_loss_pct);
    TD_HIP(hipGetLastError());
    s->pn_hi = k_hi, s->pn_lo = k_lo, s->pn_wait = max_wait, s->pn_loss = max_loss_pct, s->pn_max_happy = max_happy;
    return TD_OK;
}

extern "C" int td_sim_pool_buffer(td_sim *s, int64_t plan_buffer)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (plan_buffer < 0 || (plan_buffer > 0 && plan_buffer < (int64_t)24 * SIM_POOL_N_NMAX))
        return fail(TD_EINVAL, "td_sim_pool_buffer: plan_buffer = %lld: 0, or at least 24 * %d = %d", (long long)plan_buffer, SIM_POOL_N_NMAX,
                    24 * SIM_POOL_N_NMAX);
    if (s->begun) return fail(TD_EINVAL, "td_sim_pool_buffer: tick %d still waits for td_sim_apply", s->last_t);
    s->pn_buffer = plan_buffer;
    return TD_OK;
}

extern "C" int td_sim_pools_n(td_sim *s, int max_pools, int32_t *records, int32_t *size, int32_t *n)
{
    TD_REQUIRE_INIT();
    if (!s || !n) return fail(TD_EINVAL, "null argument");
    if (!s->pn_hi) return fail(TD_EINVAL, "td_sim_pools_n: the world pools pairs (td_sim_pooling): read them with td_sim_pools");
    if (max_pools < 0) return fail(TD_EINVAL, "td_sim_pools_n: negative max_pools");
    const int k = s->n_pool;
    *n = k;
    if (k > max_pools) return fail(TD_EINVAL, "td_sim_pools_n: %d plans, more than max_pools = %d", k, max_pools);
    if (k == 0) return TD_OK;
    if (!records || !size) return fail(TD_EINVAL, "null destination");
    int rc;
    if ((rc = get(records, s->pn.recs, (size_t)9 * k)) || (rc = get(size, s->pn.size, (size_t)k))) return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_sim_dispatch(td_sim *s, int mode, int max_non_lcm, int parts)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (mode < TD_DISPATCH_LCM_OPT || mode > TD_DISPATCH_SPLIT) return fail(TD_EINVAL, "td_sim_dispatch: mode = %d outside 0 .. 3", mode);
    if (max_non_lcm < 0) return fail(TD_EINVAL, "td_sim_dispatch: max_non_lcm = %d is negative", max_non_lcm);
    if (mode == TD_DISPATCH_SPLIT && (parts < 1 || parts > 32 || parts > s->w.n_stands))
        return fail(TD_EINVAL, "td_sim_dispatch: parts = %d outside 1 .. min(32, n_stands = %d)", parts, s->w.n_stands);
    if (s->begun) return fail(TD_EINVAL, "td_sim_dispatch: tick %d still waits for td_sim_apply", s->last_t);
    s->disp_mode = mode;
    s->max_non_lcm = max_non_lcm;
    if (mode == TD_DISPATCH_SPLIT) s->disp_parts = parts;
    return TD_OK;
}

extern "C" int td_sim_pools(td_sim *s, int max_pools, int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n)
{
    TD_REQUIRE_INIT();
    if (!s || !n) return fail(TD_EINVAL, "null argument");
    if (s->pn_hi) return fail(TD_EINVAL, "td_sim_pools: the world pools up to %d (td_sim_pooling_n): read the records with td_sim_pools_n", s->pn_hi);
    if (max_pools < 0) return fail(TD_EINVAL, "td_sim_pools: negative max_pools");
    const int k = s->n_pool;
    *n = k;
    if (k > max_pools) return fail(TD_EINVAL, "td_sim_pools: %d plans, more than max_pools = %d", k, max_pools);
    if (k == 0) return TD_OK;
    if (!cust_a || !cust_b || !plan || !cost) return fail(TD_EINVAL, "null destination");
    int rc;
    if ((rc = get(cust_a, s->pl_a, (size_t)k)) || (rc = get(cust_b, s->pl_b, (size_t)k)) || (rc = get(plan, s->pl_plan, (size_t)k)) ||
        (rc = get(cost, s->pl_cost, (size_t)k)))
        return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_sim_model(td_sim *s, int32_t *cab_to, int32_t *dem_from)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!s->begun) return fail(TD_EINVAL, "td_sim_model: no tick with demand has begun");
    if ((s->n_sup && !cab_to) || (s->n_dem2 && !dem_from)) return fail(TD_EINVAL, "null destination");
    int rc;
    // without supply the demand was not pooled: the model's requests are the temp demand itself
    if ((rc = get(cab_to, s->sup_to, (size_t)s->n_sup)) || (rc = get(dem_from, s->n_sup ? s->d2_from : s->dem_from, (size_t)s->n_dem2))) return rc;
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
    if (n_s > 0 && s->disp_mode == TD_DISPATCH_SPLIT) {
        // the batched call's device code on this one model: the lists stay where they are, the offsets are two host words
        if (n > 1024)
            return fail(TD_EINVAL,
                        "td_sim_step: the split model of tick %d has %d cabs and %d requests, more than 1024 per side; finish the tick through "
                        "td_sim_model / td_sim_apply", t, n_s, n_d);
        const int32_t c_off[2] = {0, n_s}, d_off[2] = {0, n_d}, mode = TD_DISPATCH_SPLIT, parts = s->disp_parts;
        if ((rc = td_dispatch_batched(1, n, c_off, s->sup_to, d_off, s->d2_from, s->dist, s->dist ? s->w.n_stands : 0, s->w.big_cost, s->w.drop_time,
                                      s->w.n_stands, &mode, nullptr, &parts, s->h_rows, s->h_cols, &k, &lm, s->h_kc, s->h_kd, &n_rest, s->h_r2c,
                                      &total, nullptr)))
            return rc;
        solved = 1;   // row_to_col is over the whole model: the request of each cab
        line[6] = n_d;
        line[7] = n_s;
    } else if (n_s > 0) {
        // the arguments HipTickBackend.tick hands td_tick, with the position lists (and the table) where they already are; the stop
        // size is the policy's: the world's max_non_lcm, -1 (the optimum alone: the LCM never runs) or 0 (the LCM alone, to its end)
        const int stop = s->disp_mode == TD_DISPATCH_OPT ? -1 : s->disp_mode == TD_DISPATCH_LCM ? 0 : s->max_non_lcm;
        if ((rc = td_tick(s->sup_to, n_s, s->d2_from, n_d, s->dist, s->dist ? s->w.n_stands : 0, s->w.big_cost, s->w.drop_time, stop, s->h_rows, s->h_cols, &k, &lm,
                          s->h_kc, s->h_kd, &n_rest, s->h_r2c, &total)))
            return rc;
        const bool lcm = s->lcm_rule() < n;
        solved = s->disp_mode != TD_DISPATCH_LCM && n_rest > 0 && !(lcm && lm == s->w.big_cost);
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
    int32_t *cd[5] = {c_from, c_to, c_clnt, c_onboard, c_start}, *rd[5] = {d_cab, d_pick, d_pool_id, d_pool_plan, d_pool_cost};
    return state_out(s->w, 0, s->w.n_cabs, 0, s->w.n_req, s->tmp, cd, rd);
}

extern "C" int td_sim_metrics(td_sim *s, int64_t out[TD_SIM_N_METRICS])
{
    TD_REQUIRE_INIT();
    if (!s || !out) return fail(TD_EINVAL, "null argument");
    Head h;
    int rc = read_head(s, &h);
    if (rc) return rc;
    fill_metrics(h.ctl, s->lcm_used, s->max_model, s->max_solver, s->max_pool_mem, s->max_pool, out);
    return TD_OK;
}

extern "C" int td_sim_log(td_sim *s, uint32_t kinds, int64_t capacity)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (kinds & ~TD_EV_ALL) return fail(TD_EINVAL, "td_sim_log: kinds = 0x%x has bits outside 1 .. 11", kinds);
    if (kinds && (capacity <= 0 || capacity > INT_MAX)) return fail(TD_EINVAL, "td_sim_log: capacity = %lld outside 1 .. 2^31 - 1", (long long)capacity);
    if (s->begun) return fail(TD_EINVAL, "td_sim_log: tick %d still waits for td_sim_apply", s->last_t);
    if (kinds && s->pn_hi > 2)
        return fail(TD_EINVAL, "td_sim_log: not built: the event log of pools of three and four (td_sim_pooling_n with k_hi = %d)", s->pn_hi);
    if (kinds && s->rt_mem.p) return fail(TD_EINVAL, "td_sim_log: not built: the event log of routed worlds (the handle has routes, td_sim_route)");
    const size_t nc = (size_t)s->w.n_cabs, nr = (size_t)s->w.n_req;
    return ev_setup(s->ev, kinds, capacity, 1, nc, nr, nc + nr + 2 + nr + nr / 2 + 2 * (nc + nr) + 2 * nc);
}

extern "C" int td_sim_events(td_sim *s, int64_t max_records, int32_t *records, int64_t *n, int64_t *lost)
{
    TD_REQUIRE_INIT();
    if (!s || !n) return fail(TD_EINVAL, "null argument");
    if (max_records < 0) return fail(TD_EINVAL, "td_sim_events: negative max_records");
    int rc;
    if (s->ev.kinds && s->begun && !s->ev.begin_flushed) {   // a tick waits for its apply: what it has written so far
        if ((rc = sim_ev_flush(s, 1))) return rc;
        s->ev.begin_flushed = true;
    }
    return ev_drain(s->ev, "td_sim_events", max_records, records, n, lost);
}

extern "C" int td_sim_route(td_sim *s, int on)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (s->begun) return fail(TD_EINVAL, "td_sim_route: tick %d still waits for td_sim_apply", s->last_t);
    if (!on) {   // no new routes; the cabs that are mid-route finish theirs
        s->route_on = false;
        return TD_OK;
    }
    if (!s->pn_hi) return fail(TD_EINVAL, "td_sim_route: the world pools pairs, which have no drop-off order to drive; set a td_sim_pooling_n policy first");
    if (s->ev.kinds) return fail(TD_EINVAL, "td_sim_route: not built: the event log of routed worlds (the handle logs)");
    if (!s->rt_mem.p) {   // the handle's, from the first call on: nothing is allocated per tick
        Ctx &c = ctx();
        const size_t nc = (size_t)s->w.n_cabs, nr = (size_t)std::max(s->w.n_req, 1), cap = (size_t)s->cap;
        RouteDev d;
        int rc = carve_buf(s->rt_mem, [&](Carve &cv) {
            d.stops = (int32_t *)cv.take<int4>(2 * nc);   // a cab's eight words are two 16-byte vectors
            d.cnt = cv.take<long long>(4);
            d.pos = cv.take<int32_t>(nc);
            d.r_drop = cv.take<int32_t>(nr);
            d.d2_rec = cv.take<int32_t>(cap);
            d.kd_rec = cv.take<int32_t>(cap);
        });
        if (rc) return rc;
        s->rt = d;
        const int n = (int)std::max<size_t>(std::max(8 * nc, nr), 4);   // the four counters are the first four threads'
        k_route_init<<<(n + 255) / 256, 256, 0, c.stream>>>(s->w.n_cabs, s->w.n_req, d.stops, d.pos, d.r_drop, d.cnt);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            buf_free(s->rt_mem);
            s->rt = RouteDev();
            return hip_fail(e, "td_sim_route launch");
        }
    }
    s->route_on = true;
    return TD_OK;
}

extern "C" int td_sim_route_state(td_sim *s, int32_t *r_drop, int32_t *c_pos, int32_t *c_stops)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!s->rt_mem.p) return fail(TD_EINVAL, "td_sim_route_state: the handle has no routes (td_sim_route)");
    int rc;
    if ((rc = get(r_drop, s->rt.r_drop, (size_t)s->w.n_req)) || (rc = get(c_pos, s->rt.pos, (size_t)s->w.n_cabs)) ||
        (rc = get(c_stops, s->rt.stops, (size_t)8 * s->w.n_cabs)))
        return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_sim_route_metrics(td_sim *s, int64_t out[TD_SIM_N_ROUTE_METRICS])
{
    TD_REQUIRE_INIT();
    if (!s || !out) return fail(TD_EINVAL, "null argument");
    if (!s->rt_mem.p) return fail(TD_EINVAL, "td_sim_route_metrics: the handle has no routes (td_sim_route)");
    static_assert(sizeof(long long) == sizeof(int64_t), "the counters are read back as they lie");
    TD_HIP(hipMemcpyAsync(s->pin, s->rt.cnt, sizeof(int64_t) * TD_SIM_N_ROUTE_METRICS, hipMemcpyDeviceToHost, ctx().stream));
    TD_HIP(hipStreamSynchronize(ctx().stream));
    for (int q = 0; q < TD_SIM_N_ROUTE_METRICS; q++) out[q] = ((const int64_t *)s->pin)[q];
    return TD_OK;
}
