// td_simb.hip — B independent simulator worlds in HBM behind one handle (td_simb_*).  The world kernels, predicates and
// emitters are td_sim_world.h's, shared with td_sim.hip; this file holds what B worlds need of their own: the handle and
// its head block, k_offsets, the scatter behind it, where the batched calls leave plans and decisions (SimbPlans,
// SimbDec), and the host flow.
//
// Layout.  The B fleets are ONE cab table and the B request tables ONE request table (world after world; cab_off / req_off
// say where a world begins).  c_clnt and the pool partner stay indices into the concatenated request table; the cab number
// a request stores (r_cab) and td_simb_state reports is world-local.  Every per-tick list (demand, supply, demand after
// pooling, kept lists) is packed world-major, ascending within a world, with an offset array [B+1]: exactly the ragged
// lists td_pool2_batched and td_tick_batched take.  Two stand bitsets and one Ctl per world.
//
// Grid.  Every world kernel runs on a grid (chunks, B): workgroup (x, b) owns elements [x * CB, (x + 1) * CB) of world b's
// segment, so a workgroup never straddles a world boundary and a per-world sum is one atomic per workgroup on that world's
// Ctl.  The index space is padded to a multiple of CB per world, the memory is not; `chunks` comes from sizes the host
// knows (create-time table sizes, or list sizes from the last read-back), so neither the number of launches nor of
// read-backs depends on B.
//
// Ordered compaction with a world dimension: k_count (per workgroup) -> k_offsets (ONE workgroup: per-world totals and their
// exclusive scan = the list's offset array) -> k_scatter (out[off[b] + counts of the world's earlier chunks + rank]).  No
// atomic append, no workgroup waits for another; the kernel boundary is the only barrier between workgroups.
//
//   begin   k_arrive, k_flags<cab>, k_dem_count (drop + count), k_flags<req>, k_count<supply>, k_offsets, k_scatter x 2,
//           read-back, td_pool2_batched on the device lists, k_pool_mark, k_count / k_offsets / k_scatter, read-back
//   apply   k_pair_map, k_apply_pairs, k_count x 2, k_offsets, k_scatter x 2, k_apply_solution, read-back
//   step    begin + td_tick_batched on the device lists + apply (the decisions stay on the device, strided as written)
//
// A world without demand in a tick has empty lists (its supply is not listed either); a world with demand and no supply keeps
// its demand list as its model and is left out of the pool and tick calls (their lists pl_* / tk_* hold the worlds WITH
// supply only).  The error word is one for the handle: a pair outside its world's model applies nothing in any world.
// Under td_simb_pooling every world has its own policy: ONE td_pool2_batched_v call serves them all (a policy per model), and
// a world whose policy is TD_POOL_NONE is left out of pl_* as a world without supply is (k_offsets' gate), but not out of tk_*.
//
// A batch on a distance table (td_simb_create_dist): the worlds share ONE city, so the handle owns one copy of the table and
// one pair of neighbour bit matrices (k_nb_build of td_sim_core.h, which also validates the table); the near bitsets are
// per world, laid out like `bits`.  k_near_b after each k_flags serves NEAR_WPG worlds per workgroup: two launches
// per tick whatever B is.  The predicates then read one bit, arrival / dispatch / analyzeSolution read one table cell
// (way()), and the batched calls get the handle's table.  The direction rule is td_sim.hip's: the row of the table is
// always the stand the cab is at or heads to.  A line batch (dist == nullptr) launches exactly what it launched before.
//
// The event log (td_simb_log / td_simb_events) is td_sim's with the world dimension of the grid: one flush per
// tick over all worlds, three launches whatever B is, world 0's records first.  Off by default: the EvOff instantiations.
//
// The route model (td_simb_route) is td_sim's with the world bound per workgroup (RouteOnB::of, td_sim_core.h):
// a world whose routes are on hands a dispatched cab its record's stop list, every other world of the batch behaves as
// without routes (its record column holds -1 everywhere).  A handle that never asked for routes launches the RouteOff
// instantiations, as before; with route storage k_arrive runs routed, and a tick in which some world's routes are on runs
// the last begin compaction, the kept-demand compaction and the two apply kernels in their routed forms: the same launches
// in the same order.
#include <limits.h>

#include "td_sim_world.h"

using namespace td;
using namespace tdsim;

namespace {
constexpr int SIMB_NMAX = 2048;   // largest model of td_tick_batched / td_pool2_batched
}  // namespace

// decisions of a tick: packed ragged arrays from the caller (stride == 0), or td_tick_batched's strided outputs
struct SimbDec {
    const int32_t *rows, *cols, *r2c;
    const int32_t *pair_off, *r2c_off, *solved;
    const int32_t *n_pairs, *n_rest, *last_min;
    int stride;
    const int32_t *rule;   // td_simb_dispatch's per-world LCM rule (null without one): -1 = the LCM alone, a world that is never solved
    __device__ __forceinline__ void pairs(int b, int *base, int *cnt) const
    {
        if (stride) {
            *base = b * stride;
            *cnt = n_pairs[b];
        } else {
            *base = pair_off[b];
            *cnt = pair_off[b + 1] - *base;
        }
    }
    // row_to_col of world b: where it begins and how many entries count (0 when the world was not solved)
    __device__ __forceinline__ void r2c_of(int b, bool lcm, int big_cost, int *base, int *nr, bool *sol) const
    {
        if (stride) {
            *base = b * stride;
            *sol = n_rest[b] > 0 && !(lcm && last_min[b] == big_cost) && !(rule && rule[b] < 0);
            *nr = *sol ? n_rest[b] : 0;
        } else {
            *base = r2c_off[b];
            *sol = solved[b] != 0 && !(rule && rule[b] < 0);
            *nr = *sol ? r2c_off[b + 1] - *base : 0;
        }
    }
};

// this tick's plan lists: world b's at b * pool_h (td_pool2_batched), or packed at pl_off[b] / 2 (td_pool2 world by world);
// pl_off delimits the customers that were pooled, the demand of the worlds with supply
struct SimbPlans {
    int pool_h, ragged;
    const int32_t *pl_off, *n_pools;
    __device__ __forceinline__ int n_act(int b) const { return pl_off[b + 1] - pl_off[b]; }
    __device__ __forceinline__ int count(int b) const { return n_pools[b]; }
    __device__ __forceinline__ int base(int b) const { return ragged ? pl_off[b] >> 1 : b * pool_h; }
};

// td_simb_pooling_n: what the first call adds to a handle; a world with hi[b] == 0 keeps its pair policy.  The stage lists lie
// where the world's demand list lies (dem_off[b]), cnt[b] entries long; world b's records at b * stride.
struct SimbPoolN {
    bool set = false;            // some world pools records
    int any3 = 0;                // some world has k_hi > 2: the apply kernels carry three partners
    std::vector<int32_t> hi, lo, wait, loss;
    int64_t max_happy = 0;
    int64_t buffer = 0;          // td_simb_pool_buffer: > 0: every round is td_pool_n_banded_batched's core with this plan buffer
    int stride = 1, nmax = 1;    // plans per world in recs / size; the largest stage list (<= 512)
    Buf mem;
    int32_t *d_hi = nullptr, *d_lo, *d_wait, *d_loss;   // [B]
    int32_t *cnt[2], *np;                               // [B]: the stage list's size (ping-pong), the stage's pools
    int32_t *rec_base = nullptr;                        // [B]: where a record world's pairs lie in pa / pb, for the event log (k_hi == 2)
    std::vector<int32_t> h_cnt, h_base;                 // this tick's first stage sizes and rec_base on the host
    long long *nh, *happy, *tot;                        // [B]: the stage's happy plans, the tick's, the stage's cost
    int32_t *st_from[2], *st_to[2], *st_map[2], *used;  // the stage lists and their positions in the world's demand list
    int32_t *out;                                       // a stage's records as the pool call writes them
    int32_t *recs, *size;                               // the tick's plans: 9 ints each, and their sizes
    int32_t *d2_more[2], *kd_more[2];                   // the third and fourth pick-up of the demand after pooling / the kept demand
};

// the plan lists as the event log reads them in a batch with record worlds (td_simb_pooling_n, k_hi == 2 everywhere): a record
// world pooled its whole demand list and mirrors its pairs in pa / pb at rec_base[b]
struct SimbPlansN {
    SimbPlans pl;
    const int32_t *k_hi, *dem_off, *rec_base;
    __device__ __forceinline__ int n_act(int b) const { return k_hi[b] ? dem_off[b + 1] - dem_off[b] : pl.n_act(b); }
    __device__ __forceinline__ int count(int b) const { return pl.count(b); }
    __device__ __forceinline__ int base(int b) const { return k_hi[b] ? rec_base[b] : pl.base(b); }
};

// td_simb_route: what the first call with a world on adds to a handle
struct SimbRoute {
    bool any = false;            // some world's routes are on: the ticks from the next begin on run the routed forms
    bool tick = false;           // the begun tick carries the record columns
    std::vector<int32_t> on;     // [B] on the host
    Buf mem;                     // mem.p: the handle has route storage, and k_arrive drives what is in it
    int32_t *stops = nullptr, *pos, *r_drop;   // 8 stop words and a position per cab of the concatenated fleet, the drop-off tick per request
    int32_t *d2_rec, *kd_rec;                  // the record of each customer of the demand after pooling / the kept demand
    long long *cnt;                            // [4 B]: drop_numb, ride_time, solo_time, max_over_loss of every world
    int32_t *d_on;                             // [B]
    int32_t *local;                            // [8 max_cabs]: one world's stop words, world-local, for td_simb_route_state
};

struct td_simb : SimbDev, SimbPin {   // td_sim_layout.h: every device array of the handle, and the pinned block
    SimbPoolN pn;
    SimbRoute rt;
    RouteOnB route() const
    {
        return RouteOnB{rt.stops, rt.pos, rt.r_drop, rt.cnt, pn.d_loss, pn.recs, dem_idx, rt.d2_rec, rt.kd_rec, dem_off, pn.stride};
    }
    World w;                     // the concatenated tables
    int B = 0, max_non_lcm = 0;
    int words = 0;               // of one stand bitset
    int max_cabs = 0, max_req = 0, nc_tot = 0, nr_tot = 0;
    int ncap = 1, hcap = 1;      // strides the batched calls may use at most: models / pools per world
    size_t pool_cap = 0, in_cap = 0;
    std::vector<int32_t> cab_off, req_off;   // host copies
    Buf mem;
    // head block (device) and its pinned mirror h_head: Ctl[B], the error word, the offset arrays, the per-world words
    int32_t *head = nullptr;     // = ctl_blk
    size_t head_ints = 0;
    Ctl *ctl = nullptr;
    void *pin = nullptr;
    // sequencing
    int last_t = -1;
    bool begun = false;
    int pool_ragged = 0;         // this tick's plans lie at pl_off[b] / 2 (the per-world td_pool2 path) instead of b * pool_h
    int pool_h = 1;
    std::vector<int32_t> n_dem, n_sup, n_d2;
    EvLog ev;                    // td_simb_log
    std::vector<int64_t> lcm_used, max_model, max_solver, max_pool_mem, max_pool;
    // td_simb_pooling: the policy of every world from the next begin on.  pool_set == false: the handle pools as it always did
    bool pool_set = false, has_none = false;
    std::vector<int32_t> pool_mode, pool_opt;   // TD_POOL_*; 1 where the mode is TD_POOL_OPTIMAL
    std::vector<double> pool_ml;                // (d_none is read only when has_none)
    std::vector<int32_t> h_npool, h_pbase;      // this tick's plans per world and where they begin in pa / pb / pp / pc
    // td_simb_dispatch: the dispatch policy of every world from the next begin on.  disp_set == false: the handle dispatches as it
    // always did, through td_tick_batched and the one-number instantiations of the world kernels
    bool disp_set = false;
    std::vector<int32_t> disp_mode, disp_mnl, disp_parts;   // host mirrors: what td_dispatch_batched is handed; d_rule[b] = rule(b)
    // the model size above which the LCM ran in world b (LcmRuleB of td_sim_world.h)
    int rule(int b) const
    {
        if (!disp_set) return max_non_lcm;
        return disp_mode[b] == TD_DISPATCH_LCM_OPT ? disp_mnl[b] : disp_mode[b] == TD_DISPATCH_LCM ? -1 : INT_MAX;
    }
    bool lcm_alone(int b) const { return disp_set && disp_mode[b] == TD_DISPATCH_LCM; }
};

// f(the LCM rule as the world kernels take it): one number for a handle without td_simb_dispatch, else a number per world
template <class F>
static auto with_rule(const td_simb *s, F f)
{
    return s->disp_set ? f(LcmRuleB{s->d_rule}) : f(LcmRule1{s->max_non_lcm});
}

namespace {

// the route storage's first state in every world: no stop anywhere, nobody dropped off, the counters empty
__global__ __launch_bounds__(256) void k_routeb_init(int B, int n_cabs, int n_req, int32_t *__restrict__ stops, int32_t *__restrict__ pos,
                                                     int32_t *__restrict__ r_drop, long long *__restrict__ cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 8 * n_cabs) stops[i] = -1;
    if (i < n_cabs) pos[i] = 0;
    if (i < n_req) r_drop[i] = -1;
    if (i < 4 * B) cnt[i] = (i & 3) == 3 ? INT64_MIN : 0;
}

// a world's stop words as a one-world handle reports them: the request index counts from where the world's table begins
__global__ __launch_bounds__(256) void k_route_local(const int32_t *__restrict__ stops, int n, int r0, int32_t *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int wd = stops[i];
    out[i] = wd < 0 ? -1 : wd - 2 * r0;
}

// ONE workgroup: per-workgroup counts -> per-world totals -> offset arrays (exclusive scans over the worlds, B in slices of CB).
//   off_a = the list counted in cnt_a; off_b (cnt_b non-null) = the list counted in cnt_b.
//   begin_mode: a = demand, b = supply: a world without demand lists no supply, off_c = the demand of the worlds WITH supply
//   that pool (gate non-null: gate[b] != 0 leaves world b out, its policy is TD_POOL_NONE).
//   else: off_c (non-null) = list a restricted to the worlds with gate[b + 1] > gate[b].
__global__ __launch_bounds__(CB) void k_offsets(int B, const int32_t *__restrict__ cnt_a, int nc_a, const int32_t *__restrict__ cnt_b, int nc_b,
                                                int begin_mode, const int32_t *__restrict__ gate, int32_t *__restrict__ off_a,
                                                int32_t *__restrict__ off_b, int32_t *__restrict__ off_c)
{
    __shared__ int s_w[16];
    int ca = 0, cb = 0, cc = 0;   // the running totals, the same in every thread
    for (int b0 = 0; b0 < B; b0 += CB) {
        const int b = b0 + threadIdx.x;
        int na = 0, nb = 0, nc = 0;
        if (b < B) {
            for (int j = 0; j < nc_a; j++) na += cnt_a[b * nc_a + j];
            if (cnt_b)
                for (int j = 0; j < nc_b; j++) nb += cnt_b[b * nc_b + j];
            if (begin_mode) {
                if (na == 0) nb = 0;
                nc = nb > 0 && !(gate && gate[b]) ? na : 0;
            } else if (off_c) {
                nc = gate[b + 1] > gate[b] ? na : 0;
            }
        }
        int ta, tb, tc;
        const int ea = block_excl_scan(na, s_w, &ta), eb = block_excl_scan(nb, s_w, &tb), ec = block_excl_scan(nc, s_w, &tc);
        if (b < B) {
            off_a[b] = ca + ea;
            if (off_b) off_b[b] = cb + eb;
            if (off_c) off_c[b] = cc + ec;
        }
        ca += ta;
        cb += tb;
        cc += tc;
    }
    if (threadIdx.x == 0) {
        off_a[B] = ca;
        if (off_b) off_b[B] = cb;
        if (off_c) off_c[B] = cc;
    }
}

// out[off_out[b] + the counts of the world's earlier chunks + rank] = element; a world whose output segment is empty
// (no demand: its supply is not listed) writes nothing.  off_out2: the list of the worlds with a non-empty segment there.
template <class P, class E>
__global__ __launch_bounds__(CB) void k_scatter(const int32_t *__restrict__ off, P pred, E emit, const int32_t *__restrict__ cnt,
                                                const int32_t *__restrict__ off_out, const int32_t *__restrict__ off_out2)
{
    __shared__ int s_red[16];
    const int b = blockIdx.y, lo = off[b], n = off[b + 1] - lo, l = blockIdx.x * CB + threadIdx.x;
    const int cap = off_out[b + 1] - off_out[b];
    if (cap == 0 || (int)blockIdx.x * CB >= n) return;
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += CB) part += cnt[b * gridDim.x + j];
    const int before = block_sum(part, s_red);
    const bool f = l < n && pred(lo + l, b);
    int tot;
    const int rank = block_rank(f, s_red, &tot);
    const int pos = before + rank;
    const bool two = off_out2 && off_out2[b + 1] > off_out2[b];
    if (f && pos < cap) emit(off_out[b] + pos, two ? off_out2[b] + pos : -1, lo + l, b);
}

// ---- td_simb_pooling_n: the cascade of every world at once.  The stage lists lie where the worlds' demand lists lie.
struct PnArgs {
    const int32_t *dem_off, *dem_from, *dem_to;
    int32_t *cnt[2], *np, *n_rec;
    long long *nh, *happy;
    int32_t *st_from[2], *st_to[2], *st_map[2], *used;
};

// One compaction pass per stage for all worlds, one workgroup per world (a stage list holds at most 512 requests): the
// requests no pool of the stage took stay, in list order, with their positions in the world's demand list; the world's plan
// and happy-plan counts move on.  ident: the demand list itself becomes the first stage's list.
__global__ __launch_bounds__(CB) void k_pn_compact(PnArgs a, int cur, int ident)
{
    __shared__ int s_red[16];
    const int b = blockIdx.x, d0 = a.dem_off[b], n_dem = a.dem_off[b + 1] - d0;
    const int m = min(max(a.cnt[ident ? 0 : cur][b], 0), n_dem);
    const int32_t *sf = ident ? a.dem_from : a.st_from[cur], *st = ident ? a.dem_to : a.st_to[cur], *sm = a.st_map[cur];
    const int nxt = ident ? 0 : cur ^ 1;
    int kept = 0;
    for (int i0 = 0; i0 < m; i0 += CB) {
        const int i = i0 + threadIdx.x;
        bool f = false;
        if (i < m) {
            f = !a.used[d0 + i];
            a.used[d0 + i] = 0;   // the next stage starts from a clean list
        }
        int tot;
        const int o = d0 + kept + block_rank(f, s_red, &tot);
        if (f) {
            a.st_from[nxt][o] = sf[d0 + i];
            a.st_to[nxt][o] = st[d0 + i];
            a.st_map[nxt][o] = ident ? i : sm[d0 + i];
        }
        kept += tot;
    }
    if (threadIdx.x == 0 && !ident) {
        a.cnt[nxt][b] = kept;
        a.n_rec[b] += a.np[b];
        a.happy[b] += a.nh[b];
        a.np[b] = 0;
    }
}

// k_pool_mark for records, a stage of every world: record p of world b's pool call (2 K + 1 ints, members = positions in the
// stage list) becomes plan n_rec[b] + p of the world's tick (9 ints, members = positions in the demand list).  Every member but
// the first pick-up gets the leave mark, the first its plan index, the stage list forgets all of them.  A member outside
// the list raises the error word.  rec_base non-null: the pair is mirrored in pl_a / pl_b for the event log.
__global__ __launch_bounds__(256) void k_pn_records(int K, int nmax, int cur, int stride, PnArgs a, const int32_t *__restrict__ out,
                                                    int32_t *__restrict__ recs, int32_t *__restrict__ size, int32_t *__restrict__ isb,
                                                    int32_t *__restrict__ ainfo, const int32_t *__restrict__ rec_base,
                                                    int32_t *__restrict__ pl_a, int32_t *__restrict__ pl_b, int32_t *gerr)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.np[b] || p >= nmax / K) return;
    const int d0 = a.dem_off[b], n_dem = a.dem_off[b + 1] - d0, m = min(a.cnt[cur][b], n_dem), base = a.n_rec[b];
    if (base < 0 || base + p >= stride) {
        atomicMax(gerr, 1);
        return;
    }
    const int32_t *r = out + ((size_t)b * (size_t)(nmax / K) + (size_t)p) * (size_t)(2 * K + 1), *map = a.st_map[cur] + d0;
    int pick[4] = {-1, -1, -1, -1}, drop[4] = {-1, -1, -1, -1};
    bool bad = false;
    for (int i = 0; i < K; i++) {
        const int u = r[i], v = r[K + i];
        if (u < 0 || u >= m || v < 0 || v >= m) {
            bad = true;
            continue;
        }
        pick[i] = map[u];
        drop[i] = map[v];
        bad = bad || pick[i] < 0 || pick[i] >= n_dem || drop[i] < 0 || drop[i] >= n_dem;
    }
    if (bad) {
        atomicMax(gerr, 1);
        return;
    }
    const size_t q = (size_t)b * (size_t)stride + (size_t)(base + p);
    int32_t *o = recs + 9 * q;
    for (int i = 0; i < 4; i++) {
        o[i] = pick[i];
        o[4 + i] = drop[i];
    }
    o[8] = r[2 * K];
    size[q] = K;
    if (rec_base) {   // the handle logs (every pool is a pair): first and second pick-up where the event log reads a pair
        const int e = rec_base[b] + base + p;   // base + p < n_dem / 2: inside the world's slice of pa / pb
        pl_a[e] = pick[0];
        pl_b[e] = pick[1];
    }
    atomicMin(&ainfo[d0 + pick[0]], base + p);
    for (int i = 0; i < K; i++) {
        a.used[d0 + r[i]] = 1;
        if (i) isb[d0 + pick[i]] = 1;
    }
}

// analyzePool of a batch that mixes policies: a pair world's customer through PoolEmit, a record world's through its records
template <int NP>
struct PoolEmitB {
    PoolEmit<SimbPlans, SegOff> pair;
    const int32_t *k_hi, *recs, *size;
    int stride;
    int32_t *more[2];
    __device__ void operator()(int o, int o2, int d, int b) const
    {
        if (!k_hi[b]) {
            pair(o, o2, d, b);
            if constexpr (NP > 1) more[0][o] = more[1][o] = -1;
            return;
        }
        pair.idx[o] = pair.dem_idx[d];
        pair.from[o] = pair.dem_from[d];
        const int p = pair.ainfo[d];
        const bool a = p >= 0 && p < min(pair.pl.count(b), stride);
        const size_t q = (size_t)b * (size_t)stride + (size_t)(a ? p : 0);
        const int32_t *r = recs + 9 * q;
        int d0, n_dem;
        pair.dem(b, &d0, &n_dem);
        auto member = [&](int j) {   // k_pn_records raised the error word for a member outside the list; never index by it
            const int m = a ? r[j] : -1;
            return m >= 0 && m < n_dem ? pair.dem_idx[d0 + m] : -1;
        };
        pair.partner[o] = member(1);
        if constexpr (NP > 1) {
            more[0][o] = member(2);
            more[1][o] = member(3);
        }
        pair.plan[o] = a ? size[q] : -1;
        pair.cost[o] = a ? r[8] : 0;
        if (o2 >= 0) pair.tk_from[o2] = pair.dem_from[d];
    }
};

inline int nchunks(int n) { return std::max(1, (n + CB - 1) / CB); }

// the head block on the host: every world's Ctl, the error word, the offset arrays, the per-world words, in ONE copy
int read_head(td_simb *s)
{
    Ctx &c = ctx();
    TD_HIP(hipMemcpyAsync(s->h_head, s->head, sizeof(int32_t) * s->head_ints, hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    return TD_OK;
}

inline const Ctl *h_ctl(const td_simb *s) { return (const Ctl *)s->h_head; }
inline const int32_t *h_of(const td_simb *s, const int32_t *dev) { return s->h_head + (dev - s->head); }

int clear_err(td_simb *s)
{
    TD_HIP(hipMemsetAsync(s->gerr, 0, sizeof(int32_t), ctx().stream));
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

// the event log: this tick's records, sections `phase`, behind the log: world after world, whatever B is
int simb_ev_flush(td_simb *s, int phase)
{
    const EvLog &e = s->ev;
    size_t vmax = 0;
    for (int b = 0; b < s->B; b++) {
        const size_t nc = (size_t)(s->cab_off[b + 1] - s->cab_off[b]), nr = (size_t)(s->req_off[b + 1] - s->req_off[b]), ns = (size_t)s->n_sup[b];
        vmax = std::max(vmax, nc + nr + 2 + s->n_dem[b] + s->n_dem[b] / 2 + 2 * (ns + s->n_d2[b]) + 2 * ns);
    }
    const SimbPlans pl{s->pool_h, s->pool_ragged, s->pl_off, s->n_pools};
    if (s->pn.set)
        return with_rule(s, [&](auto rule) {
            const EvSrc<SegOff, SimbPlansN, decltype(rule)> src{s->w, SegOff{s->d_cab_off}, SegOff{s->d_req_off}, SegOff{s->dem_off}, SegOff{s->sup_off},
                                                                SegOff{s->d2_off}, SimbPlansN{pl, s->pn.d_hi, s->dem_off, s->pn.rec_base}, rule,
                                                                s->last_t, phase, e.kinds, e.st_arr, e.st_drop, e.st_pairs, e.st_sol, s->dem_idx, s->pa,
                                                                s->pb};
            return ev_flush(s->ev, src, s->B, vmax);
        });
    return with_rule(s, [&](auto rule) {
        const EvSrc<SegOff, SimbPlans, decltype(rule)> src{s->w, SegOff{s->d_cab_off}, SegOff{s->d_req_off}, SegOff{s->dem_off}, SegOff{s->sup_off},
                                                           SegOff{s->d2_off}, pl, rule,
                                                           s->last_t, phase, e.kinds, e.st_arr, e.st_drop, e.st_pairs, e.st_sol, s->dem_idx, s->pa,
                                                           s->pb};
        return ev_flush(s->ev, src, s->B, vmax);
    });
}

// a tick is over (no world has anything to apply, or applied): what the log has not seen of it goes there
int simb_ev_tick_done(td_simb *s)
{
    if (!s->ev.kinds) return TD_OK;
    const int phase = s->ev.begin_flushed ? 2 : 3;
    s->ev.begin_flushed = false;
    return simb_ev_flush(s, phase);
}

constexpr int SIMB_POOL_N_NMAX = 512;   // td_pool_n_batched's largest model

// findPool of the worlds under td_simb_pooling_n, after the pair worlds' (the specification: Simulator.find_pool_n in every
// such world).  Round k = 4, 3, 2 serves every world whose cascade has a stage of k, so a world's stages run k_hi down to k_lo
// and a tick has at most three pool launches whatever B is; a world of another policy, without supply or with fewer than
// two requests is an empty model.  Marks go to isb / ainfo, the plan count of a world to n_pools[b] (read with the head).
// the first stage's list of every record world (0: the world does not pool in this tick) and the rounds the tick needs;
// a world beyond the pool call's model is refused before anything is pooled
int simb_pool_n_sizes(td_simb *s, int t)
{
    SimbPoolN &pn = s->pn;
    pn.nmax = 0;
    for (int b = 0; b < s->B; b++) {
        const int m = pn.hi[b] && s->n_sup[b] > 0 && s->n_dem[b] >= 2 ? s->n_dem[b] : 0;
        if (m > SIMB_POOL_N_NMAX)
            return fail(TD_EINVAL, "td_simb_begin: world %d has %d requests before pooling in tick %d, more than the %d td_pool_n_batched takes", b, m, t,
                        SIMB_POOL_N_NMAX);
        pn.h_cnt[b] = m;
        pn.nmax = std::max(pn.nmax, m);
    }
    return TD_OK;
}

int simb_pool_n(td_simb *s, int t)
{
    Ctx &c = ctx();
    SimbPoolN &pn = s->pn;
    const int B = s->B, nmax = pn.nmax;
    const bool log = s->ev.kinds != 0;
    if (nmax == 0) return TD_OK;
    bool round[5] = {false, false, false, false, false};
    for (int b = 0; b < B; b++)
        for (int k = pn.lo[b]; pn.h_cnt[b] && k <= pn.hi[b]; k++) round[k] = true;
    // h_stage (pinned, at least 3 (B + 1) ints) serves twice, ordered on the stream: 2 B ints up (sizes, rec_base), then B 64-bit
    // happy-plan counts down.  The per-world pair path queued an upload from it: that one has to be over first.
    if (s->pool_ragged) TD_HIP(hipStreamSynchronize(c.stream));
    int32_t *st = s->h_stage;
    memcpy(st, pn.h_cnt.data(), sizeof(int32_t) * B);
    memcpy(st + B, pn.h_base.data(), sizeof(int32_t) * B);
    TD_HIP(hipMemcpyAsync(pn.cnt[0], st, sizeof(int32_t) * 2 * B, hipMemcpyHostToDevice, c.stream));   // cnt[0] and rec_base are one block
    const size_t nd_tot = (size_t)h_of(s, s->dem_off)[B];
    TD_HIP(hipMemsetAsync(pn.np, 0, sizeof(int32_t) * B, c.stream));
    TD_HIP(hipMemsetAsync(pn.happy, 0, sizeof(long long) * B, c.stream));
    TD_HIP(hipMemsetAsync(pn.used, 0, sizeof(int32_t) * nd_tot, c.stream));
    const PnArgs a{s->dem_off, s->dem_from, s->dem_to, {pn.cnt[0], pn.cnt[1]}, pn.np, s->n_pools, pn.nh, pn.happy,
                   {pn.st_from[0], pn.st_from[1]}, {pn.st_to[0], pn.st_to[1]}, {pn.st_map[0], pn.st_map[1]}, pn.used};
    k_pn_compact<<<B, CB, 0, c.stream>>>(a, 0, 1);
    TD_HIP(hipGetLastError());
    int cur = 0;
    for (int k = 4; k >= 2; k--) {
        if (!round[k]) continue;
        int over = -1, rc;
        long long count = 0;
        if (pn.buffer > 0)
            rc = pool_n_worlds_banded(k, B, nmax, s->dem_off, pn.cnt[cur], pn.d_hi, pn.d_lo, pn.st_from[cur], pn.st_to[cur], pn.d_wait, pn.d_loss,
                                      s->dist, s->dist ? s->w.n_stands : 0, pn.buffer, pn.out, pn.np, pn.nh, pn.tot);
        else
            rc = pool_n_worlds(k, B, nmax, s->dem_off, pn.cnt[cur], pn.d_hi, pn.d_lo, pn.st_from[cur], pn.st_to[cur], pn.d_wait, pn.d_loss, s->dist,
                               s->dist ? s->w.n_stands : 0, pn.max_happy, pn.out, pn.np, pn.nh, pn.tot, &over, &count);
        if (rc == TD_ERANGE && over >= 0)
            return fail(TD_ERANGE, "td_simb_begin: world %d has %lld happy plans of %d in tick %d, more than max_happy", over, count, k, t);
        if (rc) return rc;
        k_pn_records<<<dim3((std::max(1, nmax / k) + 255) / 256, B), 256, 0, c.stream>>>(k, nmax, cur, pn.stride, a, pn.out, pn.recs, pn.size, s->isb,
                                                                                       s->ainfo, log ? pn.rec_base : nullptr, s->pa, s->pb, s->gerr);
        k_pn_compact<<<B, CB, 0, c.stream>>>(a, cur, 0);
        TD_HIP(hipGetLastError());
        cur ^= 1;
    }
    // the happy plans of the tick per world, for max_POOL_MEM_size: read after the head's synchronisation
    TD_HIP(hipMemcpyAsync(st, pn.happy, sizeof(long long) * B, hipMemcpyDeviceToHost, c.stream));
    return TD_OK;
}

int simb_begin(td_simb *s, int t, int32_t *info)
{
    Ctx &c = ctx();
    const World &w = s->w;
    const int B = s->B;
    int rc;
    for (int q = 0; q < 4 * B; q++) info[q] = 0;
    // this tick's offsets and per-world words start from zero; the sums and the error word stay
    TD_HIP(hipMemsetAsync(s->dem_off, 0, sizeof(int32_t) * (SIMB_N_OFF * (B + 1) + SIMB_N_PER * B), c.stream));
    TD_HIP(hipMemsetAsync(s->bits, 0, sizeof(uint32_t) * 2 * (size_t)s->words * B, c.stream));
    const size_t shm = sizeof(uint32_t) * (size_t)s->words;
    const int gc = nchunks(s->max_cabs), gr = nchunks(s->max_req);
    const dim3 grid_c(gc, B), grid_r(gr, B);
    const SegOff cabs{s->d_cab_off}, reqs{s->d_req_off};
    const bool log = s->ev.kinds != 0;
    if (log)
        k_arrive<<<grid_c, CB, 0, c.stream>>>(w, cabs, t, s->ctl, EvOn{s->ev.st_arr}, RouteOff{});
    else if (s->rt.mem.p)   // a handle with route storage never logs
        k_arrive<<<grid_c, CB, 0, c.stream>>>(w, cabs, t, s->ctl, EvOff{}, s->route());
    else
        k_arrive<<<grid_c, CB, 0, c.stream>>>(w, cabs, t, s->ctl, EvOff{}, RouteOff{});
    k_flags<<<grid_c, CB, shm, c.stream>>>(cabs, w.n_stands, w.c_to, w.c_clnt, s->bits, 0);
    const dim3 grid_n = near_grid(B, s->words);
    const size_t shm_n = near_lds(s->words);
    if (s->dist) k_near_b<<<grid_n, CB, shm_n, c.stream>>>(B, w.n_stands, s->words, s->nb_dem, s->bits, s->near, 0);
    const DemPred dp{w, t, s->words, s->bits, s->near};
    if (log)
        k_dem_count<<<grid_r, CB, 0, c.stream>>>(dp, reqs, s->cnt_a, s->ctl, EvOn{s->ev.st_drop});
    else
        k_dem_count<<<grid_r, CB, 0, c.stream>>>(dp, reqs, s->cnt_a, s->ctl, EvOff{});
    k_flags<<<grid_r, CB, shm, c.stream>>>(reqs, w.n_stands, w.r_from, w.r_cab, s->bits, 1);
    if (s->dist) k_near_b<<<grid_n, CB, shm_n, c.stream>>>(B, w.n_stands, s->words, s->nb_sup, s->bits, s->near, 1);
    const SupPred sp{w, s->words, s->bits, s->near};
    k_count<SegOff, SupPred><<<grid_c, CB, 0, c.stream>>>(cabs, sp, s->cnt_b);
    k_offsets<<<1, CB, 0, c.stream>>>(B, s->cnt_a, gr, s->cnt_b, gc, 1, s->has_none ? s->d_none : nullptr, s->dem_off, s->sup_off, s->pl_off);
    k_scatter<DemPred, DemEmit><<<grid_r, CB, 0, c.stream>>>(s->d_req_off, dp, DemEmit{w, s->dem_idx, s->dem_from, s->dem_to, s->pl_from, s->pl_to},
                                                           s->cnt_a, s->dem_off, s->pl_off);
    k_scatter<SupPred, SupEmit><<<grid_c, CB, 0, c.stream>>>(s->d_cab_off, sp, SupEmit{w, s->sup_cab, s->sup_to}, s->cnt_b, s->sup_off, nullptr);
    TD_HIP(hipGetLastError());
    if ((rc = read_head(s))) return rc;
    if (*h_of(s, s->gerr)) return fail(TD_EINTERNAL, "td_simb: device error word %d", *h_of(s, s->gerr));
    s->last_t = t;
    s->pool_ragged = 0;
    s->rt.tick = s->rt.any;   // td_simb_route is refused inside a tick: the begin and the apply agree
    s->h_npool.assign((size_t)B, 0);
    const int32_t *hd = h_of(s, s->dem_off), *hs = h_of(s, s->sup_off), *hp = h_of(s, s->pl_off);
    int max_dem = 0, max_act = 0;
    for (int b = 0; b < B; b++) {
        s->n_dem[b] = s->n_d2[b] = hd[b + 1] - hd[b];
        s->n_sup[b] = hs[b + 1] - hs[b];
        max_dem = std::max(max_dem, s->n_dem[b]);
        max_act = std::max(max_act, hp[b + 1] - hp[b]);
    }
    if (hd[B] == 0) return simb_ev_tick_done(s);   // Simulator.java:160 in every world: nothing to do in this tick
    s->begun = true;
    // the record worlds' sizes first: their pairs are mirrored for the event log at the stride of the pair worlds' plans
    int n_all = max_act;
    if (s->pn.set) {
        if ((rc = simb_pool_n_sizes(s, t))) return rc;
        if (log && max_act <= SIMB_NMAX) {
            n_all = std::max(max_act, s->pn.nmax);
            s->pool_h = std::max(1, n_all / 2);
        }
    }
    // findPool for the worlds with supply, the plans stay on the device
    if (max_act >= 2) {
        if (s->pool_set)   // the optimum of a world is ONE model of the batched call: refused before anything is pooled
            for (int b = 0; b < B; b++)
                if (s->pool_opt[b] && hp[b + 1] - hp[b] > SIMB_NMAX)
                    return fail(TD_EINVAL, "td_simb_begin: world %d has %d requests before pooling in tick %d, more than the %d an optimal pool model holds", b,
                                hp[b + 1] - hp[b], t, SIMB_NMAX);
        for (int b = 0; b < B; b++)   // the pairs examined, whatever the world's rule admits; a world that does not pool has hp's segment empty
            if (hp[b + 1] - hp[b] >= 2) s->max_pool_mem[b] = std::max(s->max_pool_mem[b], (int64_t)s->n_dem[b] * (s->n_dem[b] - 1));
        const int S = s->dist ? w.n_stands : 0;
        if (max_act <= SIMB_NMAX) {
            s->pool_h = std::max(1, n_all / 2);
            if (!s->pool_set)
                rc = td_pool2_batched(B, n_all, hp, s->pl_from, s->pl_to, s->dist, S, 0.0, 0, s->pa, s->pb, s->pp, s->pc, s->n_pools, s->p_total);
            else   // one call for every policy of the batch: its launches do not depend on B or on the mix
                rc = td_pool2_batched_v(B, n_all, hp, s->pl_from, s->pl_to, s->dist, S, s->pool_ml.data(), s->pool_opt.data(), s->pa, s->pb, s->pp, s->pc,
                                        s->n_pools, s->p_total);
            if (rc) return rc;
        } else if (s->pool_set) {
            // world by world as below, each under its own policy (an optimal world: the batched call on its one model)
            s->pool_ragged = 1;
            int32_t *np = s->h_stage;
            for (int b = 0; b < B; b++) {
                const int m = hp[b + 1] - hp[b], q = hp[b] >> 1;
                np[b] = 0;
                if (m < 2) continue;
                if (s->pool_opt[b]) {
                    const int32_t off[2] = {0, m};
                    int64_t tot = 0;
                    rc = td_pool2_batched(1, m, off, s->pl_from + hp[b], s->pl_to + hp[b], s->dist, S, s->pool_ml[b], 1, s->pa + q, s->pb + q, s->pp + q, s->pc + q,
                                          &np[b], &tot);
                } else {
                    rc = td_pool2_loss(m, s->pl_from + hp[b], s->pl_to + hp[b], s->dist, S, s->pool_ml[b], s->pa + q, s->pb + q, s->pp + q, s->pc + q, &np[b]);
                }
                if (rc) return rc;
            }
            TD_HIP(hipMemcpyAsync(s->n_pools, np, sizeof(int32_t) * B, hipMemcpyHostToDevice, c.stream));
        } else {
            // a world beyond the batched call's model size: td_pool2 world by world, plans packed at pl_off[b] / 2 (a world
            // of m customers has at most m / 2 plans).  Only td_simb_begin / _model / _apply serve such a tick.
            s->pool_ragged = 1;
            int32_t *np = s->h_stage;
            for (int b = 0; b < B; b++) {
                const int m = hp[b + 1] - hp[b], q = hp[b] >> 1;
                np[b] = 0;
                if (m >= 2 && (rc = td_pool2(m, s->pl_from + hp[b], s->pl_to + hp[b], s->dist, s->dist ? w.n_stands : 0, s->pa + q, s->pb + q, s->pp + q, s->pc + q, &np[b])))
                    return rc;
            }
            TD_HIP(hipMemcpyAsync(s->n_pools, np, sizeof(int32_t) * B, hipMemcpyHostToDevice, c.stream));
        }
    }
    const size_t nd_tot = (size_t)hd[B];
    TD_HIP(hipMemsetAsync(s->isb, 0, sizeof(int32_t) * nd_tot, c.stream));
    TD_HIP(hipMemsetAsync(s->ainfo, 0x7f, sizeof(int32_t) * nd_tot, c.stream));
    const SimbPlans pl{s->pool_h, s->pool_ragged, s->pl_off, s->n_pools};
    const SegOff dem{s->dem_off};
    if (max_act >= 2)
        k_pool_mark<<<dim3((max_act / 2 + 255) / 256, B), 256, 0, c.stream>>>(pl, dem, s->pa, s->pb, s->isb, s->ainfo, s->gerr);
    if (s->pn.set) {
        // where a record world mirrors its pairs: its slot of the strided plan lists, or, beside the packed lists of the per-world
        // pair path (at most pl_off[B] / 2 plans), packed behind them: together never more than half the requests
        int at = (hp[B] >> 1) + 1;
        for (int b = 0; b < B; b++) {
            s->pn.h_base[b] = s->pool_ragged ? at : b * s->pool_h;
            if (s->pn.hi[b]) at += s->n_dem[b] >> 1;
        }
        if ((rc = simb_pool_n(s, t))) return rc;
    }
    const dim3 grid_d(nchunks(max_dem), B);
    const PoolPred pp{s->isb};
    k_count<SegOff, PoolPred><<<grid_d, CB, 0, c.stream>>>(dem, pp, s->cnt_a);
    k_offsets<<<1, CB, 0, c.stream>>>(B, s->cnt_a, (int)grid_d.x, nullptr, 0, 0, s->sup_off, s->d2_off, nullptr, s->tk_off);
    const PoolEmit<SimbPlans, SegOff> pe{pl, dem, s->dem_idx, s->dem_from, s->ainfo, s->pb, s->pp, s->pc, s->d2_idx, s->d2_from, s->d2_partner,
                                         s->d2_plan, s->d2_cost, s->tk_from};
    const SimbPoolN &pn = s->pn;
    // with routes the record of a first pick-up travels beside its columns (a world on implies pn.set)
    const RecCountB rcnt{pn.d_hi, s->rt.d_on, s->n_pools, pn.stride};
    if (s->rt.tick && pn.any3)
        k_scatter<PoolPred, WithRec<PoolEmitB<3>, RecCountB>><<<grid_d, CB, 0, c.stream>>>(
            s->dem_off, pp,
            WithRec<PoolEmitB<3>, RecCountB>{PoolEmitB<3>{pe, pn.d_hi, pn.recs, pn.size, pn.stride, {pn.d2_more[0], pn.d2_more[1]}}, s->ainfo, rcnt, s->rt.d2_rec},
            s->cnt_a, s->d2_off, s->tk_off);
    else if (s->rt.tick)
        k_scatter<PoolPred, WithRec<PoolEmitB<1>, RecCountB>><<<grid_d, CB, 0, c.stream>>>(
            s->dem_off, pp, WithRec<PoolEmitB<1>, RecCountB>{PoolEmitB<1>{pe, pn.d_hi, pn.recs, pn.size, pn.stride, {nullptr, nullptr}}, s->ainfo, rcnt, s->rt.d2_rec},
            s->cnt_a, s->d2_off, s->tk_off);
    else if (!pn.set)
        k_scatter<PoolPred, PoolEmit<SimbPlans, SegOff>><<<grid_d, CB, 0, c.stream>>>(s->dem_off, pp, pe, s->cnt_a, s->d2_off, s->tk_off);
    else if (pn.any3)
        k_scatter<PoolPred, PoolEmitB<3>><<<grid_d, CB, 0, c.stream>>>(
            s->dem_off, pp, PoolEmitB<3>{pe, pn.d_hi, pn.recs, pn.size, pn.stride, {pn.d2_more[0], pn.d2_more[1]}}, s->cnt_a, s->d2_off, s->tk_off);
    else
        k_scatter<PoolPred, PoolEmitB<1>><<<grid_d, CB, 0, c.stream>>>(s->dem_off, pp, PoolEmitB<1>{pe, pn.d_hi, pn.recs, pn.size, pn.stride, {nullptr, nullptr}},
                                                                     s->cnt_a, s->d2_off, s->tk_off);
    TD_HIP(hipGetLastError());
    if ((rc = read_head(s))) return rc;
    if (*h_of(s, s->gerr)) {
        (void)clear_err(s);
        return fail(TD_EINTERNAL, "td_simb: a pool plan names a customer outside the demand list");
    }
    const int32_t *h2 = h_of(s, s->d2_off), *hn = h_of(s, s->n_pools);
    hp = h_of(s, s->pl_off);
    for (int b = 0; b < B; b++) {
        const int m = hp[b + 1] - hp[b];
        s->h_npool[b] = m >= 2 ? std::min(std::max(hn[b], 0), m / 2) : 0;
        s->h_pbase[b] = s->pool_ragged ? hp[b] >> 1 : b * s->pool_h;
        s->n_d2[b] = h2[b + 1] - h2[b];
        if (s->pn.set && s->pn.hi[b]) {   // a record world: its plans of all stages, and the happy plans behind them
            const bool ran = s->pn.nmax > 0 && s->n_sup[b] > 0 && s->n_dem[b] >= 2;
            s->h_npool[b] = ran ? std::min(std::max(hn[b], 0), s->pn.stride) : 0;
            if (ran) {
                long long happy;
                memcpy(&happy, s->h_stage + 2 * (size_t)b, sizeof(happy));
                s->max_pool_mem[b] = std::max(s->max_pool_mem[b], (int64_t)happy);
                s->max_pool[b] = std::max(s->max_pool[b], (int64_t)s->h_npool[b]);
            }
        }
        if (s->n_dem[b] == 0) continue;
        info[4 * b] = 1;
        info[4 * b + 1] = s->n_dem[b];
        info[4 * b + 2] = s->n_sup[b];
        info[4 * b + 3] = s->n_d2[b];
        if (s->n_sup[b] > 0) {
            if (m >= 2) s->max_pool[b] = std::max(s->max_pool[b], (int64_t)hn[b]);
            s->max_model[b] = std::max(s->max_model[b], (int64_t)std::max(s->n_sup[b], s->n_d2[b]));
        }
    }
    return TD_OK;
}

// the decisions are on the device (dec); h_solved: the packed path's flags on the host (NULL: td_tick_batched's words of the head)
int simb_apply(td_simb *s, const SimbDec &dec, int max_pairs, const int32_t *h_solved, int32_t *opt_count)
{
    Ctx &c = ctx();
    const World &w = s->w;
    const int B = s->B, t = s->last_t;
    int rc;
    int max_s = 0, max_d = 0, max_sd = 0;
    bool any_lcm = false, any_sup = false;
    for (int b = 0; b < B; b++) {
        const int n_s = s->n_sup[b], n_d = s->n_d2[b];
        if (n_s == 0) continue;
        any_sup = true;
        max_s = std::max(max_s, n_s);
        if (std::max(n_s, n_d) > s->rule(b)) {
            any_lcm = true;
            max_d = std::max(max_d, n_d);
            max_sd = std::max(max_sd, n_s + n_d);
        }
    }
    const int32_t *hs = h_of(s, s->sup_off), *h2 = h_of(s, s->d2_off);
    const SegOff cabs{s->d_cab_off}, sup{s->sup_off}, d2{s->d2_off};
    const bool log = s->ev.kinds != 0;
    // pools of three or four in some world: the partner columns behind the first travel with the apply kernels (such a handle never logs)
    const bool more = s->pn.set && s->pn.any3;
    const bool route = s->rt.tick;   // some world hands out routes in this tick (such a handle never logs)
    const MorePartners<3> px3{{s->pn.d2_more[0], s->pn.d2_more[1]}, {s->pn.kd_more[0], s->pn.kd_more[1]}};
    if (log && (rc = ev_clear_apply(s->ev, (size_t)hs[B], (size_t)h2[B]))) return rc;
    rc = with_rule(s, [&](auto mnl) -> int {
    using L = decltype(mnl);
    if (any_lcm) {
        TD_HIP(hipMemsetAsync(s->pair_cab, 0x7f, sizeof(int32_t) * (size_t)hs[B], c.stream));
        TD_HIP(hipMemsetAsync(s->pair_dem, 0x7f, sizeof(int32_t) * (size_t)h2[B], c.stream));
        if (max_pairs > 0)
            k_pair_map<<<dim3((max_pairs + 255) / 256, B), 256, 0, c.stream>>>(dec, mnl, sup, d2, s->pair_cab, s->pair_dem, s->gerr);
        auto pairs = [&](auto ev, auto px, auto rt) {
            k_apply_pairs<<<dim3(nchunks(max_sd), B), CB, 0, c.stream>>>(w, t, dec, mnl, cabs, sup, d2, s->pair_cab, s->pair_dem, s->sup_cab, s->sup_to,
                                                                       s->d2_idx, s->d2_partner, s->d2_cost, s->ctl, s->gerr, ev, px, rt);
        };
        if (route && more)
            pairs(EvOff{}, px3, s->route());
        else if (route)
            pairs(EvOff{}, MorePartners<1>{}, s->route());
        else if (more)
            pairs(EvOff{}, px3, RouteOff{});
        else if (log)
            pairs(EvOn{s->ev.st_pairs}, MorePartners<1>{}, RouteOff{});
        else
            pairs(EvOff{}, MorePartners<1>{}, RouteOff{});
        const dim3 grid_s(nchunks(max_s), B), grid_d(nchunks(max_d), B);
        const KeptPred<SegOff, L> ps{s->pair_cab, sup, d2, mnl}, pd{s->pair_dem, sup, d2, mnl};
        k_count<SegOff, KeptPred<SegOff, L>><<<grid_s, CB, 0, c.stream>>>(sup, ps, s->cnt_a);
        k_count<SegOff, KeptPred<SegOff, L>><<<grid_d, CB, 0, c.stream>>>(d2, pd, s->cnt_b);
        k_offsets<<<1, CB, 0, c.stream>>>(B, s->cnt_a, (int)grid_s.x, s->cnt_b, (int)grid_d.x, 0, nullptr, s->ks_off, s->kd_off, nullptr);
        k_scatter<KeptPred<SegOff, L>, KeptSupEmit><<<grid_s, CB, 0, c.stream>>>(s->sup_off, ps, KeptSupEmit{s->sup_cab, s->sup_to, s->ks_cab, s->ks_to},
                                                                            s->cnt_a, s->ks_off, nullptr);
        const KeptDemEmit ke{s->d2_idx, s->d2_from, s->d2_partner, s->d2_plan, s->d2_cost, s->kd_idx, s->kd_from, s->kd_partner, s->kd_plan, s->kd_cost};
        const KeptDemEmitN<3> ke3{ke, {s->pn.d2_more[0], s->pn.d2_more[1]}, {s->pn.kd_more[0], s->pn.kd_more[1]}};
        if (route && more)   // with routes the record column travels to the kept demand too
            k_scatter<KeptPred<SegOff, L>, KeptRec<KeptDemEmitN<3>>><<<grid_d, CB, 0, c.stream>>>(
                s->d2_off, pd, KeptRec<KeptDemEmitN<3>>{ke3, s->rt.d2_rec, s->rt.kd_rec}, s->cnt_b, s->kd_off, nullptr);
        else if (route)
            k_scatter<KeptPred<SegOff, L>, KeptRec<KeptDemEmit>><<<grid_d, CB, 0, c.stream>>>(
                s->d2_off, pd, KeptRec<KeptDemEmit>{ke, s->rt.d2_rec, s->rt.kd_rec}, s->cnt_b, s->kd_off, nullptr);
        else if (more)
            k_scatter<KeptPred<SegOff, L>, KeptDemEmitN<3>><<<grid_d, CB, 0, c.stream>>>(s->d2_off, pd, ke3, s->cnt_b, s->kd_off, nullptr);
        else
            k_scatter<KeptPred<SegOff, L>, KeptDemEmit><<<grid_d, CB, 0, c.stream>>>(s->d2_off, pd, ke, s->cnt_b, s->kd_off, nullptr);
    }
    auto solution = [&](auto ev, auto px, auto rt) {
        k_apply_solution<<<dim3(nchunks(max_s), B), CB, 0, c.stream>>>(w, t, dec, mnl, cabs, sup, d2, SegOff{s->ks_off}, SegOff{s->kd_off}, s->sup_cab,
                                                                     s->sup_to, s->d2_idx, s->d2_from, s->d2_partner, s->d2_plan, s->d2_cost, s->ks_cab,
                                                                     s->ks_to, s->kd_idx, s->kd_from, s->kd_partner, s->kd_plan, s->kd_cost, s->ctl, s->gerr,
                                                                     ev, px, rt);
    };
    if (any_sup && route && more)
        solution(EvOff{}, px3, s->route());
    else if (any_sup && route)
        solution(EvOff{}, MorePartners<1>{}, s->route());
    else if (any_sup && more)
        solution(EvOff{}, px3, RouteOff{});
    else if (any_sup && log)
        solution(EvOn{s->ev.st_sol}, MorePartners<1>{}, RouteOff{});
    else if (any_sup)
        solution(EvOff{}, MorePartners<1>{}, RouteOff{});
    return TD_OK;
    });
    if (rc) return rc;
    TD_HIP(hipGetLastError());
    if ((rc = read_head(s))) return rc;
    const int err = *h_of(s, s->gerr);
    if (err) {
        // nothing was applied in any world (every kernel after the failing one is skipped): the tick still waits
        if ((rc = clear_err(s))) return rc;
        if (err == 2) return fail(TD_EINVAL, "td_simb_apply: a pair lies outside its world's model");
        return fail(TD_EINTERNAL, "td_simb: device error word %d", err);
    }
    s->begun = false;
    const int32_t *hks = h_of(s, s->ks_off), *hkd = h_of(s, s->kd_off), *hrest = h_of(s, s->tk_rest), *hlm = h_of(s, s->tk_lm);
    for (int b = 0; b < B; b++) {
        opt_count[b] = 0;
        const int n_s = s->n_sup[b], n = std::max(n_s, s->n_d2[b]);
        if (s->n_dem[b] == 0 || n_s == 0) continue;
        const bool lcm = n > s->rule(b);
        const bool solved = !s->lcm_alone(b) && (h_solved ? h_solved[b] != 0 : (hrest[b] > 0 && !(lcm && hlm[b] == w.big_cost)));
        if (lcm) s->lcm_used[b]++;
        if (lcm && !solved) {
            opt_count[b] = -1;
            continue;
        }
        opt_count[b] = h_ctl(s)[b].opt_count;
        s->max_solver[b] = std::max(s->max_solver[b], (int64_t)(lcm ? std::max(hks[b + 1] - hks[b], hkd[b + 1] - hkd[b]) : n));
    }
    return simb_ev_tick_done(s);
}

// offsets [B + 1] from the caller: start at 0, never decrease, world b's segment at most cap(b) long
int check_offsets(const td_simb *s, const char *what, const std::vector<int32_t> &h, int *longest)
{
    Ragged rg;
    int rc = ragged_check(fail, "td_simb_apply", what, "world", h.data(), s->B, &rg, [&](int b, int m) {
        const int cap = std::max(std::max(s->cab_off[b + 1] - s->cab_off[b], s->req_off[b + 1] - s->req_off[b]), 1);
        return m > cap ? fail(TD_EINVAL, "td_simb_apply: world %d's segment of %s has %d entries, more than %d", b, what, m, cap) : 0;
    });
    *longest = rg.longest;
    return rc;
}

}  // namespace

// td_simb_create (dist == nullptr) and td_simb_create_dist
static int simb_create(int batch, const int32_t *n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost, const int32_t *req_off,
                       const int32_t *req_id, const int32_t *req_from, const int32_t *req_to, const int32_t *req_at, const int32_t *dist,
                       td_simb **out)
{
    TD_REQUIRE_INIT();
    Ctx &c = ctx();
    if (!out) return fail(TD_EINVAL, "null handle pointer");
    *out = nullptr;
    if (batch < 1 || batch > 65535) return fail(TD_EINVAL, "td_simb_create: batch = %d outside 1 .. 65535", batch);
    if (!n_cabs || !req_off) return fail(TD_EINVAL, "td_simb_create: null n_cabs / req_off");
    if (n_stands < 1 || drop_time < 0 || max_non_lcm < 0 || big_cost < 0) return fail(TD_EINVAL, "td_simb_create: n_stands at least 1, nothing negative");
    if (n_stands > (1 << 18)) return fail(TD_EINVAL, "td_simb_create: at most %d stands (one bit per stand in LDS)", 1 << 18);
    if (dist && n_stands > MAX_DIST_STANDS) return fail(TD_EINVAL, "td_simb_create_dist: at most %d stands with a distance table", MAX_DIST_STANDS);
    if (max_non_lcm > 1024)
        return fail(TD_EINVAL, "td_simb_create: max_non_lcm = %d > 1024 (the remainder td_tick_batched hands its solver)", max_non_lcm);
    const int B = batch;
    int rc;
    std::vector<int32_t> hc, ho;
    if ((rc = host_copy(n_cabs, (size_t)B, hc)) || (rc = host_copy(req_off, (size_t)B + 1, ho))) return rc;
    Ragged rg;
    if ((rc = ragged_check(fail, "td_simb_create", "req_off", "world", ho.data(), B, &rg, [&](int b, int) {
            return hc[b] < 1 || hc[b] > SIMB_NMAX ? fail(TD_EINVAL, "td_simb_create: world %d has %d cabs, outside 1 .. %d", b, hc[b], SIMB_NMAX) : 0;
        })))
        return rc;
    std::vector<int32_t> cab_off((size_t)B + 1, 0);
    int max_cabs = 0;
    size_t in_cap = 0;
    for (int b = 0; b < B; b++) {
        cab_off[b + 1] = cab_off[b] + hc[b];
        max_cabs = std::max(max_cabs, hc[b]);
        in_cap += (size_t)std::max(std::max(hc[b], ho[b + 1] - ho[b]), 1);
    }
    const int max_req = rg.longest, n_req = rg.total, nc_tot = cab_off[B];
    if (n_req && (!req_id || !req_from || !req_to || !req_at)) return fail(TD_EINVAL, "null request array");
    // the request files on the host once: ids unique within a world and not negative, stands inside the line, times not negative
    std::vector<int32_t> h;
    if ((rc = load_requests(n_req, req_id, req_from, req_to, req_at, h))) return rc;
    for (int b = 0; b < B; b++) {
        const int i = bad_request(h, n_req, n_stands, ho[b], ho[b + 1]);
        if (i >= 0)
            return fail(TD_EINVAL, "td_simb_create: world %d, request %d (id %d, from %d, to %d, at %d) is outside the world", b, i - ho[b], h[i],
                        h[(size_t)n_req + i], h[(size_t)2 * n_req + i], h[(size_t)3 * n_req + i]);
        if (!ids_unique(h, ho[b], ho[b + 1])) return fail(TD_EINVAL, "td_simb_create: request ids must be unique within world %d", b);
    }
    td_simb *s = new td_simb();
    s->B = B;
    s->max_non_lcm = max_non_lcm;
    s->max_cabs = max_cabs;
    s->max_req = max_req;
    s->nc_tot = nc_tot;
    s->nr_tot = n_req;
    s->words = (n_stands + 31) / 32;
    s->cab_off = cab_off;
    s->req_off = ho;
    s->ncap = std::max(1, std::min(SIMB_NMAX, std::max(max_cabs, max_req)));
    s->hcap = std::max(1, std::min(SIMB_NMAX, max_req) / 2);
    s->in_cap = in_cap;
    for (std::vector<int32_t> *v : {&s->n_dem, &s->n_sup, &s->n_d2, &s->pool_opt, &s->h_npool, &s->h_pbase, &s->pn.hi, &s->pn.lo, &s->pn.wait, &s->pn.loss,
                                    &s->pn.h_cnt, &s->pn.h_base})
        v->assign((size_t)B, 0);
    s->pool_mode.assign((size_t)B, TD_POOL_GREEDY);
    s->pool_ml.assign((size_t)B, 0.0);
    for (std::vector<int64_t> *v : {&s->lcm_used, &s->max_model, &s->max_solver, &s->max_pool_mem, &s->max_pool}) v->assign((size_t)B, 0);
    const size_t nb = (size_t)B, nr = (size_t)std::max(n_req, 1), nc = (size_t)nc_tot;
    s->pool_cap = std::max(nb * (size_t)s->hcap, nr / 2 + 1);
    const SimbDims dims{nb, nc, nr, (size_t)s->words, (size_t)n_stands, nb * (size_t)nchunks(std::max(max_cabs, max_req)), s->pool_cap, in_cap,
                        nb * (size_t)s->ncap, std::max<size_t>(max_cabs, 1), dist != nullptr};
    s->head_ints = dims.head_ints();
    rc = carve_buf(s->mem, [&](Carve &cv) { simb_layout(cv, dims, *s); });
    if (rc) {
        delete s;
        return rc;
    }
    s->head = (int32_t *)s->ctl_blk;
    s->ctl = (Ctl *)s->ctl_blk;
    World &w = s->w;
    w = World{nc_tot, n_req, n_stands, drop_time, big_cost};
    set_tables(w, *s, s->dist);
    auto bail = [&](int code) {
        td_simb_destroy(s);
        return code;
    };
    Carve pin_size;
    simb_pin_layout(pin_size, dims, *s);
    hipError_t e = hipHostMalloc(&s->pin, pin_size.at, hipHostMallocDefault);
    if (e != hipSuccess) {
        s->pin = nullptr;
        return bail(hip_fail(e, "hipHostMalloc(td_simb)"));
    }
    Carve pin(s->pin);
    simb_pin_layout(pin, dims, *s);
    // the initial world, made on the host: cab c of a world stands at c % n_stands (initSupply :565-573), no request is assigned
    int32_t *st = s->h_stage;
    memcpy(st, cab_off.data(), sizeof(int32_t) * (nb + 1));
    memcpy(st + nb + 1, ho.data(), sizeof(int32_t) * (nb + 1));
    int32_t *ic = st + 2 * (nb + 1), *ir = ic + 5 * nc;
    for (int b = 0; b < B; b++)
        for (int l = 0; l < hc[b]; l++) {
            const size_t g = (size_t)cab_off[b] + l;
            ic[g] = ic[nc + g] = l % n_stands;
            ic[2 * nc + g] = -1;
            ic[3 * nc + g] = 0;
            ic[4 * nc + g] = -1;
        }
    for (size_t d = 0; d < nr; d++) {
        ir[d] = ir[nr + d] = ir[2 * nr + d] = ir[3 * nr + d] = -1;
        ir[4 * nr + d] = 0;
    }
    if ((e = hipMemsetAsync(s->mem.p, 0, sizeof(int32_t) * (4 * nb + s->head_ints), c.stream)) != hipSuccess) return bail(hip_fail(e, "hipMemsetAsync"));
    struct Up {
        void *dst;
        const void *src;
        size_t n;
    } ups[] = {{s->d_cab_off, st, nb + 1},           {s->d_req_off, st + nb + 1, nb + 1},  {w.c_from, ic, nc},
               {w.c_to, ic + nc, nc},                 {w.c_clnt, ic + 2 * nc, nc},          {w.c_onb, ic + 3 * nc, nc},
               {w.c_start, ic + 4 * nc, nc},          {w.r_cab, ir, nr},                    {w.r_pick, ir + nr, nr},
               {w.r_pid, ir + 2 * nr, nr},            {w.r_plan, ir + 3 * nr, nr},          {w.r_pcost, ir + 4 * nr, nr},
               {s->r_id, h.data(), (size_t)n_req},     {s->r_from, h.data() + (size_t)n_req, (size_t)n_req},
               {s->r_to, h.data() + (size_t)2 * n_req, (size_t)n_req}, {s->r_at, h.data() + (size_t)3 * n_req, (size_t)n_req}};
    for (const Up &u : ups)
        if (u.n && (e = hipMemcpyAsync(u.dst, u.src, sizeof(int32_t) * u.n, hipMemcpyHostToDevice, c.stream)) != hipSuccess)
            return bail(hip_fail(e, "hipMemcpyAsync(td_simb tables)"));
    if (dist && (rc = table_upload("td_simb_create_dist launch", dist, n_stands, s->words, drop_time, s->dist, s->nb_dem, s->nb_sup, s->gerr)))
        return bail(rc);
    if ((e = hipStreamSynchronize(c.stream)) != hipSuccess) return bail(hip_fail(e, "hipStreamSynchronize"));   // `h` leaves scope
    if (dist && ((rc = read_head(s)) || (rc = table_verdict("td_simb_create_dist", *h_of(s, s->gerr))))) return bail(rc);
    *out = s;
    return TD_OK;
}

extern "C" int td_simb_create(int batch, const int32_t *n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost,
                              const int32_t *req_off, const int32_t *req_id, const int32_t *req_from, const int32_t *req_to,
                              const int32_t *req_at, td_simb **out)
{
    return simb_create(batch, n_cabs, n_stands, drop_time, max_non_lcm, big_cost, req_off, req_id, req_from, req_to, req_at, nullptr, out);
}

extern "C" int td_simb_create_dist(int batch, const int32_t *n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost,
                                   const int32_t *req_off, const int32_t *req_id, const int32_t *req_from, const int32_t *req_to,
                                   const int32_t *req_at, const int32_t *dist, td_simb **out)
{
    return simb_create(batch, n_cabs, n_stands, drop_time, max_non_lcm, big_cost, req_off, req_id, req_from, req_to, req_at, dist, out);
}

extern "C" int td_simb_destroy(td_simb *s)
{
    if (!s) return TD_OK;
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
    buf_free(s->mem);
    buf_free(s->pn.mem);
    buf_free(s->rt.mem);
    ev_off(s->ev);
    if (s->pin) (void)hipHostFree(s->pin);
    delete s;
    return TD_OK;
}

extern "C" int td_simb_begin(td_simb *s, int t, int32_t *info)
{
    TD_REQUIRE_INIT();
    if (!s || !info) return fail(TD_EINVAL, "null argument");
    if (t < 0) return fail(TD_EINVAL, "negative tick");
    if (s->begun) return fail(TD_EINVAL, "td_simb_begin: tick %d still waits for td_simb_apply", s->last_t);
    if (t <= s->last_t) return fail(TD_EINVAL, "td_simb_begin: tick %d after tick %d (a tick begins once, time runs forward)", t, s->last_t);
    return simb_begin(s, t, info);
}

extern "C" int td_simb_pooling(td_simb *s, const int32_t *mode, const double *max_loss)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (s->begun) return fail(TD_EINVAL, "td_simb_pooling: tick %d still waits for td_simb_apply", s->last_t);
    for (int b = 0; b < s->B && s->rt.any; b++)
        if (s->rt.on[b])
            return fail(TD_EINVAL, "td_simb_pooling: world %d's routes are on (td_simb_route) and pairs have no drop-off order to drive; switch them off first", b);
    const size_t B = (size_t)s->B;
    int rc;
    std::vector<int32_t> hm(B, TD_POOL_GREEDY);
    std::vector<double> hl(B, 0.0);
    if (mode && (rc = host_copy(mode, B, hm))) return rc;
    if (max_loss) TD_HIP(hipMemcpy(hl.data(), max_loss, sizeof(double) * B, hipMemcpyDefault));
    bool none = false;
    for (size_t b = 0; b < B; b++) {
        if (hm[b] < TD_POOL_NONE || hm[b] > TD_POOL_OPTIMAL) return fail(TD_EINVAL, "td_simb_pooling: mode[%zu] = %d outside 0 .. 2", b, hm[b]);
        if (hl[b] != hl[b]) return fail(TD_EINVAL, "td_simb_pooling: max_loss[%zu] is not a number", b);
        none = none || hm[b] == TD_POOL_NONE;
    }
    int32_t *st = s->h_stage;   // pinned, at least 3 (B + 1) ints
    for (size_t b = 0; b < B; b++) st[b] = hm[b] == TD_POOL_NONE;
    TD_HIP(hipMemcpyAsync(s->d_none, st, sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipStreamSynchronize(ctx().stream));
    s->pool_mode = hm;
    s->pool_ml = hl;
    for (size_t b = 0; b < B; b++) s->pool_opt[b] = hm[b] == TD_POOL_OPTIMAL;
    s->has_none = none;
    s->pool_set = true;
    // every world is back on a pair policy
    s->pn.set = false;
    s->pn.any3 = 0;
    for (std::vector<int32_t> *v : {&s->pn.hi, &s->pn.lo, &s->pn.wait, &s->pn.loss}) v->assign(B, 0);
    return TD_OK;
}

extern "C" int td_simb_pooling_n(td_simb *s, const int32_t *k_hi, const int32_t *k_lo, const int32_t *max_wait, const int32_t *max_loss_pct,
                                 int64_t max_happy)
{
    TD_REQUIRE_INIT();
    if (!s || !k_hi || !k_lo || !max_wait || !max_loss_pct) return fail(TD_EINVAL, "td_simb_pooling_n: null argument");
    if (s->begun) return fail(TD_EINVAL, "td_simb_pooling_n: tick %d still waits for td_simb_apply", s->last_t);
    if (max_happy > ((int64_t)1 << 22)) return fail(TD_EINVAL, "td_simb_pooling_n: max_happy = %lld above %lld", (long long)max_happy, 1ll << 22);
    const size_t B = (size_t)s->B;
    SimbPoolN &pn = s->pn;
    int rc;
    std::vector<int32_t> hh, hl, hw, hs;
    if ((rc = host_copy(k_hi, B, hh)) || (rc = host_copy(k_lo, B, hl)) || (rc = host_copy(max_wait, B, hw)) || (rc = host_copy(max_loss_pct, B, hs)))
        return rc;
    bool any = false;
    int any3 = 0;
    for (size_t b = 0; b < B; b++) {
        if (hh[b] == 0) {   // world b keeps the policy it has
            hh[b] = pn.hi[b], hl[b] = pn.lo[b], hw[b] = pn.wait[b], hs[b] = pn.loss[b];
        } else {
            if (!(2 <= hl[b] && hl[b] <= hh[b] && hh[b] <= 4))
                return fail(TD_EINVAL, "td_simb_pooling_n: k_hi[%zu] = %d, k_lo[%zu] = %d outside 2 <= k_lo <= k_hi <= 4", b, hh[b], b, hl[b]);
            if (hw[b] < 0 || hs[b] < 0)
                return fail(TD_EINVAL, "td_simb_pooling_n: max_wait[%zu] = %d, max_loss_pct[%zu] = %d: nothing negative", b, hw[b], b, hs[b]);
        }
        if (hh[b] == 0 && s->rt.any && s->rt.on[b])
            return fail(TD_EINVAL, "td_simb_pooling_n: world %zu's routes are on (td_simb_route) and k_hi[%zu] = 0 leaves it pooling pairs", b, b);
        any = any || hh[b];
        any3 = any3 || hh[b] > 2;
    }
    if (any3 && s->ev.kinds)
        return fail(TD_EINVAL, "td_simb_pooling_n: not built: the event log of pools of three and four (the handle logs; k_hi = 2 can be logged)");
    if (!pn.mem.p) {   // the handle's, from the first call on: nothing is allocated per tick
        const size_t nr = (size_t)std::max(s->nr_tot, 1), ncap = (size_t)std::max(1, std::min(SIMB_POOL_N_NMAX, s->max_req));
        const size_t stride = std::max<size_t>(1, ncap / 2);
        SimbPoolN d;
        rc = carve_buf(pn.mem, [&](Carve &cv) {
            for (long long **a : {&d.nh, &d.happy, &d.tot}) *a = cv.take<long long>(B);
            for (int32_t **a : {&d.d_hi, &d.d_lo, &d.d_wait, &d.d_loss, &d.cnt[0], &d.rec_base, &d.cnt[1], &d.np}) *a = cv.take<int32_t>(B);   // cnt[0], rec_base: one upload
            for (int32_t **a : {&d.st_from[0], &d.st_from[1], &d.st_to[0], &d.st_to[1], &d.st_map[0], &d.st_map[1], &d.used, &d.d2_more[0], &d.d2_more[1],
                                &d.kd_more[0], &d.kd_more[1]})
                *a = cv.take<int32_t>(nr);
            d.out = cv.take<int32_t>(B * 3 * ncap + 16);   // per world (n / k) records of 2 k + 1 ints: at most 2.5 n
            d.recs = cv.take<int32_t>(9 * B * stride);
            d.size = cv.take<int32_t>(B * stride);
        });
        if (rc) return rc;
        pn.d_hi = d.d_hi, pn.d_lo = d.d_lo, pn.d_wait = d.d_wait, pn.d_loss = d.d_loss, pn.np = d.np, pn.rec_base = d.rec_base, pn.nh = d.nh, pn.happy = d.happy, pn.tot = d.tot;
        pn.used = d.used, pn.out = d.out, pn.recs = d.recs, pn.size = d.size;
        for (int q = 0; q < 2; q++)
            pn.cnt[q] = d.cnt[q], pn.st_from[q] = d.st_from[q], pn.st_to[q] = d.st_to[q], pn.st_map[q] = d.st_map[q], pn.d2_more[q] = d.d2_more[q],
            pn.kd_more[q] = d.kd_more[q];
        pn.stride = (int)stride;
    }
    // the worlds of this policy leave the pair lists as a world without pooling does (k_offsets' gate)
    std::vector<int32_t> none(B);
    bool gate = false;
    for (size_t b = 0; b < B; b++) {
        none[b] = hh[b] || (s->pool_set && s->pool_mode[b] == TD_POOL_NONE);
        gate = gate || none[b];
    }
    TD_HIP(hipMemcpyAsync(s->d_none, none.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipMemcpyAsync(pn.d_hi, hh.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipMemcpyAsync(pn.d_lo, hl.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipMemcpyAsync(pn.d_wait, hw.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipMemcpyAsync(pn.d_loss, hs.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipStreamSynchronize(ctx().stream));
    s->has_none = gate;
    pn.hi = hh, pn.lo = hl, pn.wait = hw, pn.loss = hs;
    pn.set = any;
    pn.any3 = any3;
    pn.max_happy = max_happy;
    return TD_OK;
}

extern "C" int td_simb_pool_buffer(td_simb *s, int64_t plan_buffer)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (plan_buffer < 0 || (plan_buffer > 0 && plan_buffer < (int64_t)24 * SIMB_POOL_N_NMAX) || plan_buffer > ((int64_t)1 << 22))
        return fail(TD_EINVAL, "td_simb_pool_buffer: plan_buffer = %lld: 0, or 24 * %d = %d .. %lld", (long long)plan_buffer, SIMB_POOL_N_NMAX,
                    24 * SIMB_POOL_N_NMAX, 1ll << 22);
    if (s->begun) return fail(TD_EINVAL, "td_simb_pool_buffer: tick %d still waits for td_simb_apply", s->last_t);
    s->pn.buffer = plan_buffer;
    return TD_OK;
}

extern "C" int td_simb_pools_n(td_simb *s, int world, int max_pools, int32_t *records, int32_t *size, int32_t *n)
{
    TD_REQUIRE_INIT();
    if (!s || !n) return fail(TD_EINVAL, "null argument");
    if (world < 0 || world >= s->B) return fail(TD_EINVAL, "td_simb_pools_n: world %d outside 0 .. %d", world, s->B - 1);
    if (!s->pn.set || !s->pn.hi[world])
        return fail(TD_EINVAL, "td_simb_pools_n: world %d pools pairs (td_simb_pooling): read them with td_simb_pools", world);
    if (max_pools < 0) return fail(TD_EINVAL, "td_simb_pools_n: negative max_pools");
    const int k = s->h_npool[world];
    *n = k;
    if (k > max_pools) return fail(TD_EINVAL, "td_simb_pools_n: world %d has %d plans, more than max_pools = %d", world, k, max_pools);
    if (k == 0) return TD_OK;
    if (!records || !size) return fail(TD_EINVAL, "null destination");
    const size_t q = (size_t)world * (size_t)s->pn.stride;
    int rc;
    if ((rc = get(records, s->pn.recs + 9 * q, (size_t)9 * k)) || (rc = get(size, s->pn.size + q, (size_t)k))) return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_simb_dispatch(td_simb *s, const int32_t *mode, const int32_t *max_non_lcm, const int32_t *parts)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (s->begun) return fail(TD_EINVAL, "td_simb_dispatch: tick %d still waits for td_simb_apply", s->last_t);
    const size_t B = (size_t)s->B;
    int rc;
    std::vector<int32_t> hm(B, TD_DISPATCH_LCM_OPT), hl(B, s->max_non_lcm), hp(B, 4);
    if (mode && (rc = host_copy(mode, B, hm))) return rc;
    if (max_non_lcm && (rc = host_copy(max_non_lcm, B, hl))) return rc;
    if (parts && (rc = host_copy(parts, B, hp))) return rc;
    for (size_t b = 0; b < B; b++) {
        if (hm[b] < TD_DISPATCH_LCM_OPT || hm[b] > TD_DISPATCH_SPLIT) return fail(TD_EINVAL, "td_simb_dispatch: mode[%zu] = %d outside 0 .. 3", b, hm[b]);
        if (hl[b] < 0) return fail(TD_EINVAL, "td_simb_dispatch: max_non_lcm[%zu] = %d is negative", b, hl[b]);
        if (hl[b] > 1024)
            return fail(TD_EINVAL, "td_simb_dispatch: max_non_lcm[%zu] = %d > 1024 (the remainder td_dispatch_batched hands its solver)", b, hl[b]);
        if (hm[b] == TD_DISPATCH_SPLIT && (hp[b] < 1 || hp[b] > 32 || hp[b] > s->w.n_stands))
            return fail(TD_EINVAL, "td_simb_dispatch: parts[%zu] = %d outside 1 .. min(32, n_stands = %d)", b, hp[b], s->w.n_stands);
    }
    int32_t *st = s->h_stage;   // pinned, at least 3 (B + 1) ints
    for (size_t b = 0; b < B; b++)
        st[b] = hm[b] == TD_DISPATCH_LCM_OPT ? hl[b] : hm[b] == TD_DISPATCH_LCM ? -1 : INT_MAX;
    TD_HIP(hipMemcpyAsync(s->d_rule, st, sizeof(int32_t) * B, hipMemcpyHostToDevice, ctx().stream));
    TD_HIP(hipStreamSynchronize(ctx().stream));
    for (size_t b = 0; b < B; b++)
        if (hm[b] != TD_DISPATCH_SPLIT) hp[b] = 4;   // read for the split only
    s->disp_mode = hm;
    s->disp_mnl = hl;
    s->disp_parts = hp;
    s->disp_set = true;
    return TD_OK;
}

extern "C" int td_simb_pools(td_simb *s, int world, int max_pools, int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n)
{
    TD_REQUIRE_INIT();
    if (!s || !n) return fail(TD_EINVAL, "null argument");
    if (world < 0 || world >= s->B) return fail(TD_EINVAL, "td_simb_pools: world %d outside 0 .. %d", world, s->B - 1);
    if (s->pn.set && s->pn.hi[world])
        return fail(TD_EINVAL, "td_simb_pools: world %d pools up to %d (td_simb_pooling_n): read the records with td_simb_pools_n", world, s->pn.hi[world]);
    if (max_pools < 0) return fail(TD_EINVAL, "td_simb_pools: negative max_pools");
    const int k = s->h_npool[world];
    *n = k;
    if (k > max_pools) return fail(TD_EINVAL, "td_simb_pools: world %d has %d plans, more than max_pools = %d", world, k, max_pools);
    if (k == 0) return TD_OK;
    if (!cust_a || !cust_b || !plan || !cost) return fail(TD_EINVAL, "null destination");
    const size_t q = (size_t)s->h_pbase[world];
    int rc;
    if ((rc = get(cust_a, s->pa + q, (size_t)k)) || (rc = get(cust_b, s->pb + q, (size_t)k)) || (rc = get(plan, s->pp + q, (size_t)k)) ||
        (rc = get(cost, s->pc + q, (size_t)k)))
        return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_simb_model(td_simb *s, int32_t *cab_off, int32_t *cab_to, int32_t *dem_off, int32_t *dem_from)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!s->begun) return fail(TD_EINVAL, "td_simb_model: no tick with demand has begun");
    const size_t B = (size_t)s->B;
    const int n_s = h_of(s, s->sup_off)[B], n_d = h_of(s, s->d2_off)[B];
    if (!cab_off || !dem_off || (n_s && !cab_to) || (n_d && !dem_from)) return fail(TD_EINVAL, "null destination");
    int rc;
    // a world without supply was not pooled: its model's requests are its temp demand (d2 is a copy of it there)
    if ((rc = get(cab_off, s->sup_off, B + 1)) || (rc = get(dem_off, s->d2_off, B + 1)) || (rc = get(cab_to, s->sup_to, (size_t)n_s)) ||
        (rc = get(dem_from, s->d2_from, (size_t)n_d)))
        return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_simb_apply(td_simb *s, const int32_t *pair_off, const int32_t *lcm_rows, const int32_t *lcm_cols, const int32_t *solved,
                             const int32_t *r2c_off, const int32_t *row_to_col, int32_t *opt_count)
{
    TD_REQUIRE_INIT();
    if (!s || !opt_count || !pair_off || !solved || !r2c_off) return fail(TD_EINVAL, "null argument");
    if (!s->begun) return fail(TD_EINVAL, "td_simb_apply: no tick with demand has begun");
    Ctx &c = ctx();
    const size_t B = (size_t)s->B;
    int rc, max_pairs, max_r2c;
    std::vector<int32_t> hp, hr, hsol;
    if ((rc = host_copy(pair_off, B + 1, hp)) || (rc = host_copy(r2c_off, B + 1, hr)) || (rc = host_copy(solved, B, hsol))) return rc;
    if ((rc = check_offsets(s, "pair_off", hp, &max_pairs)) || (rc = check_offsets(s, "r2c_off", hr, &max_r2c))) return rc;
    if ((hp[B] && (!lcm_rows || !lcm_cols)) || (hr[B] && !row_to_col)) return fail(TD_EINVAL, "null decision array");
    int32_t *st = s->h_stage;
    memcpy(st, hp.data(), sizeof(int32_t) * (B + 1));
    memcpy(st + B + 1, hr.data(), sizeof(int32_t) * (B + 1));
    memcpy(st + 2 * (B + 1), hsol.data(), sizeof(int32_t) * B);
    // in_pair_off, in_r2c_off and in_solved are one block of the handle's memory, in this order
    TD_HIP(hipMemcpyAsync(s->in_pair_off, st, sizeof(int32_t) * (3 * B + 2), hipMemcpyHostToDevice, c.stream));
    if ((rc = put(s->in_rows, lcm_rows, (size_t)hp[B])) || (rc = put(s->in_cols, lcm_cols, (size_t)hp[B])) ||
        (rc = put(s->in_r2c, row_to_col, (size_t)hr[B])))
        return rc;
    const SimbDec dec{s->in_rows, s->in_cols, s->in_r2c, s->in_pair_off, s->in_r2c_off, s->in_solved, nullptr, nullptr, nullptr, 0, s->disp_set ? s->d_rule : nullptr};
    return simb_apply(s, dec, max_pairs, hsol.data(), opt_count);
}

extern "C" int td_simb_step(td_simb *s, int t, int32_t *line)
{
    TD_REQUIRE_INIT();
    if (!s || !line) return fail(TD_EINVAL, "null argument");
    const int B = s->B;
    std::vector<int32_t> info((size_t)4 * B), opt((size_t)B, 0);
    int rc = td_simb_begin(s, t, info.data());
    if (rc) return rc;
    for (int q = 0; q < 9 * B; q++) line[q] = 0;
    if (!s->begun) return TD_OK;
    int n = 0;
    for (int b = 0; b < B; b++) {
        if (s->n_sup[b] == 0) continue;
        if (s->n_dem[b] > SIMB_NMAX)
            return fail(TD_EINVAL,
                        "td_simb_step: world %d has %d requests before pooling in tick %d, more than %d; finish the tick through td_simb_model / "
                        "td_simb_apply",
                        b, s->n_dem[b], t, SIMB_NMAX);
        n = std::max(n, std::max(s->n_sup[b], s->n_d2[b]));
    }
    // some world has a policy that is not the handle's own: every world's model goes through td_dispatch_batched
    bool policy = false;
    for (int b = 0; b < B && s->disp_set; b++)
        policy = policy || s->disp_mode[b] != TD_DISPATCH_LCM_OPT || s->disp_mnl[b] != s->max_non_lcm;
    if (n > 0 && policy) {
        for (int b = 0; b < B; b++) {
            const int n_s = s->n_sup[b], n_d = s->n_d2[b], md = s->disp_mode[b];
            if (n_s == 0 || std::max(n_s, n_d) <= 1024) continue;
            if (md == TD_DISPATCH_SPLIT || md == TD_DISPATCH_OPT)
                return fail(TD_EINVAL,
                            "td_simb_step: world %d's %s model has %d cabs and %d requests in tick %d, more than 1024 per side; finish the tick "
                            "through td_simb_model / td_simb_apply",
                            b, md == TD_DISPATCH_SPLIT ? "split" : "optimum-alone", n_s, n_d, t);
        }
        // the host mirrors of the policy go with the device lists: no read-back of a policy array per tick
        if ((rc = td_dispatch_batched(B, n, h_of(s, s->sup_off), s->sup_to, h_of(s, s->tk_off), s->tk_from, s->dist, s->dist ? s->w.n_stands : 0,
                                      s->w.big_cost, s->w.drop_time, s->w.n_stands, s->disp_mode.data(), s->disp_mnl.data(), s->disp_parts.data(),
                                      s->tk_rows, s->tk_cols, s->tk_np, s->tk_lm, nullptr, nullptr, s->tk_rest, s->tk_r2c, s->tk_total, nullptr)))
            return rc;
    } else if (n > 0) {
        // the arguments HipTickBackend.tick hands td_tick, for every world with supply at once; the lists stay where they are
        if ((rc = td_tick_batched(B, n, h_of(s, s->sup_off), s->sup_to, h_of(s, s->tk_off), s->tk_from, s->dist, s->dist ? s->w.n_stands : 0, s->w.big_cost, s->w.drop_time,
                                  s->max_non_lcm, s->tk_rows, s->tk_cols, s->tk_np, s->tk_lm, nullptr, nullptr, s->tk_rest, s->tk_r2c, s->tk_total,
                                  nullptr)))
            return rc;
    }
    const int stride = std::max(n, 1);
    const SimbDec dec{s->tk_rows, s->tk_cols, s->tk_r2c, nullptr, nullptr, nullptr, s->tk_np, s->tk_rest, s->tk_lm, stride,
                      s->disp_set ? s->d_rule : nullptr};
    if ((rc = simb_apply(s, dec, stride, nullptr, opt.data()))) return rc;
    const int32_t *hk = h_of(s, s->tk_np), *hrest = h_of(s, s->tk_rest), *hlm = h_of(s, s->tk_lm);
    for (int b = 0; b < B; b++) {
        int32_t *ln = line + 9 * b;
        if (s->n_dem[b] == 0) continue;
        ln[0] = 1;
        ln[1] = s->n_dem[b];
        ln[2] = s->n_sup[b];
        const int n_s = s->n_sup[b], n_d = s->n_d2[b];
        if (n_s > 0) {
            const bool lcm = s->rule(b) < std::max(n_s, n_d);
            const bool solved = !s->lcm_alone(b) && hrest[b] > 0 && !(lcm && hlm[b] == s->w.big_cost);
            const int k = lcm ? hk[b] : 0;
            ln[3] = lcm;
            ln[4] = k;
            ln[5] = lcm && solved;
            ln[6] = n_d - k;
            ln[7] = n_s - k;
        }
        ln[8] = opt[b];
    }
    return TD_OK;
}

extern "C" int td_simb_state(td_simb *s, int world, int32_t *c_from, int32_t *c_to, int32_t *c_clnt, int32_t *c_onboard, int32_t *c_start,
                             int32_t *d_cab, int32_t *d_pick, int32_t *d_pool_id, int32_t *d_pool_plan, int32_t *d_pool_cost)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (world < 0 || world >= s->B) return fail(TD_EINVAL, "td_simb_state: world %d outside 0 .. %d", world, s->B - 1);
    const int c0 = s->cab_off[world], ncab = s->cab_off[world + 1] - c0, r0 = s->req_off[world], nreq = s->req_off[world + 1] - r0;
    int32_t *cd[5] = {c_from, c_to, c_clnt, c_onboard, c_start}, *rd[5] = {d_cab, d_pick, d_pool_id, d_pool_plan, d_pool_cost};
    return state_out(s->w, c0, ncab, r0, nreq, s->tmp, cd, rd);
}

extern "C" int td_simb_metrics(td_simb *s, int64_t *out)
{
    TD_REQUIRE_INIT();
    if (!s || !out) return fail(TD_EINVAL, "null argument");
    int rc = read_head(s);
    if (rc) return rc;
    for (int b = 0; b < s->B; b++)
        fill_metrics(h_ctl(s)[b], s->lcm_used[b], s->max_model[b], s->max_solver[b], s->max_pool_mem[b], s->max_pool[b], out + (size_t)TD_SIM_N_METRICS * b);
    return TD_OK;
}

extern "C" int td_simb_log(td_simb *s, uint32_t kinds, int64_t capacity)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (kinds & ~TD_EV_ALL) return fail(TD_EINVAL, "td_simb_log: kinds = 0x%x has bits outside 1 .. 11", kinds);
    if (kinds && (capacity <= 0 || capacity > INT_MAX)) return fail(TD_EINVAL, "td_simb_log: capacity = %lld outside 1 .. 2^31 - 1", (long long)capacity);
    if (s->begun) return fail(TD_EINVAL, "td_simb_log: tick %d still waits for td_simb_apply", s->last_t);
    if (kinds && s->rt.mem.p) return fail(TD_EINVAL, "td_simb_log: not built: the event log of routed worlds (the handle has routes, td_simb_route)");
    if (kinds && s->pn.set && s->pn.any3)
        return fail(TD_EINVAL, "td_simb_log: not built: the event log of pools of three and four (a world under td_simb_pooling_n has k_hi > 2)");
    const size_t nc = (size_t)s->max_cabs, nr = (size_t)s->max_req;
    return ev_setup(s->ev, kinds, capacity, s->B, (size_t)s->nc_tot, (size_t)s->nr_tot, nc + nr + 2 + nr + nr / 2 + 2 * (nc + nr) + 2 * nc);
}

extern "C" int td_simb_events(td_simb *s, int64_t max_records, int32_t *records, int64_t *n, int64_t *lost)
{
    TD_REQUIRE_INIT();
    if (!s || !n) return fail(TD_EINVAL, "null argument");
    if (max_records < 0) return fail(TD_EINVAL, "td_simb_events: negative max_records");
    int rc;
    if (s->ev.kinds && s->begun && !s->ev.begin_flushed) {   // a tick waits for its apply: what it has written so far
        if ((rc = simb_ev_flush(s, 1))) return rc;
        s->ev.begin_flushed = true;
    }
    return ev_drain(s->ev, "td_simb_events", max_records, records, n, lost);
}

extern "C" int td_simb_route(td_simb *s, const int32_t *on)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!on) return fail(TD_EINVAL, "td_simb_route: null on");
    if (s->begun) return fail(TD_EINVAL, "td_simb_route: tick %d still waits for td_simb_apply", s->last_t);
    Ctx &c = ctx();
    const size_t B = (size_t)s->B;
    SimbRoute &rt = s->rt;
    int rc;
    std::vector<int32_t> ho;
    if ((rc = host_copy(on, B, ho))) return rc;
    bool any = false;
    for (size_t b = 0; b < B; b++) {
        ho[b] = ho[b] != 0;
        if (ho[b] && !(s->pn.set && s->pn.hi[b]))
            return fail(TD_EINVAL, "td_simb_route: world %zu pools pairs, which have no drop-off order to drive; give it a td_simb_pooling_n policy first", b);
        any = any || ho[b];
    }
    if (any && s->ev.kinds) return fail(TD_EINVAL, "td_simb_route: not built: the event log of routed worlds (the handle logs)");
    if (!any && !rt.mem.p) return TD_OK;   // a handle that never had routes stays one
    if (!rt.mem.p) {   // the handle's, from the first call on: nothing is allocated per tick
        const size_t nc = (size_t)s->nc_tot, nr = (size_t)std::max(s->nr_tot, 1);
        SimbRoute d;
        rc = carve_buf(rt.mem, [&](Carve &cv) {
            d.stops = (int32_t *)cv.take<int4>(2 * nc);   // a cab's eight words are two 16-byte vectors
            d.cnt = cv.take<long long>(4 * B);
            d.pos = cv.take<int32_t>(nc);
            d.r_drop = cv.take<int32_t>(nr);
            d.d2_rec = cv.take<int32_t>(nr);
            d.kd_rec = cv.take<int32_t>(nr);
            d.d_on = cv.take<int32_t>(B);
            d.local = cv.take<int32_t>(8 * (size_t)std::max(s->max_cabs, 1));
        });
        if (rc) return rc;
        rt.stops = d.stops, rt.cnt = d.cnt, rt.pos = d.pos, rt.r_drop = d.r_drop, rt.d2_rec = d.d2_rec, rt.kd_rec = d.kd_rec, rt.d_on = d.d_on, rt.local = d.local;
        const int n = (int)std::max(std::max(8 * nc, nr), 4 * B);
        k_routeb_init<<<(n + 255) / 256, 256, 0, c.stream>>>((int)B, s->nc_tot, s->nr_tot, rt.stops, rt.pos, rt.r_drop, rt.cnt);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            buf_free(rt.mem);
            return hip_fail(e, "td_simb_route launch");
        }
    }
    TD_HIP(hipMemcpyAsync(rt.d_on, ho.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));   // `ho` leaves scope
    rt.on = ho;
    rt.any = any;
    return TD_OK;
}

extern "C" int td_simb_route_state(td_simb *s, int world, int32_t *r_drop, int32_t *c_pos, int32_t *c_stops)
{
    TD_REQUIRE_INIT();
    if (!s) return fail(TD_EINVAL, "null handle");
    if (!s->rt.mem.p) return fail(TD_EINVAL, "td_simb_route_state: the handle has no routes (td_simb_route)");
    if (world < 0 || world >= s->B) return fail(TD_EINVAL, "td_simb_route_state: world %d outside 0 .. %d", world, s->B - 1);
    const int c0 = s->cab_off[world], ncab = s->cab_off[world + 1] - c0, r0 = s->req_off[world], nreq = s->req_off[world + 1] - r0;
    int rc;
    if (c_stops) {
        k_route_local<<<(8 * ncab + 255) / 256, 256, 0, ctx().stream>>>(s->rt.stops + (size_t)8 * c0, 8 * ncab, r0, s->rt.local);
        TD_HIP(hipGetLastError());
    }
    if ((rc = get(r_drop, s->rt.r_drop + r0, (size_t)nreq)) || (rc = get(c_pos, s->rt.pos + c0, (size_t)ncab)) ||
        (rc = get(c_stops, s->rt.local, (size_t)8 * ncab)))
        return rc;
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}

extern "C" int td_simb_route_metrics(td_simb *s, int64_t *out)
{
    TD_REQUIRE_INIT();
    if (!s || !out) return fail(TD_EINVAL, "null argument");
    if (!s->rt.mem.p) return fail(TD_EINVAL, "td_simb_route_metrics: the handle has no routes (td_simb_route)");
    static_assert(sizeof(long long) == sizeof(int64_t), "the counters are read back as they lie");
    TD_HIP(hipMemcpyAsync(out, s->rt.cnt, sizeof(int64_t) * TD_SIM_N_ROUTE_METRICS * (size_t)s->B, hipMemcpyDeviceToHost, ctx().stream));
    TD_HIP(hipStreamSynchronize(ctx().stream));
    return TD_OK;
}
