// td_sim_world.h — the world layer under both simulator handles (td_sim.hip: one world, td_simb.hip: B worlds), once.
//
// Every kernel here is the batched form: grid (chunks, B), workgroup (x, b) owns elements [x * CB, (x + 1) * CB) of world
// b's segment; sums go to ctl[b], failures to ONE error word.  td_sim launches the same kernels with B = 1: at b == 0
// every index below is the one-world index.  The per-element rules are in td_sim_core.h.  What differs between the
// handles stays with them: how a list's size comes about (their own k_scatter, td_simb's k_offsets), and where segments,
// plans and decisions lie, which the kernels take as by-value template parameters:
//
//   S   a list's segments             s(b, &lo, &n): world b's elements are [lo, lo + n).  td_simb: an offset array [B + 1] on
//                                     the device (SegOff); td_sim: lo = 0 and the size the host already has, in the kernel
//                                     arguments (Seg1 of td_sim.hip), so a one-world kernel does not begin with a load
//   PL  the plan list of findPool     n_act(b) customers that were pooled, count(b) plans, the first at base(b)
//   D   a tick's decisions            rows / cols / r2c, pairs(b, &base, &cnt), r2c_of(b, lcm, big_cost, &base, &nr, &solved)
//
// Everything sits in an anonymous namespace: each translation unit keeps its own instance and no device symbol crosses a file.
#pragma once
#include <algorithm>
#include <vector>

#include "td_sim_layout.h"   // (brings td_stage.h and the HIP runtime)
#include "td_sim_core.h"

#ifndef TD_NEAR_WPG
#define TD_NEAR_WPG 4             // DESIGN.md 3.9 compares 4, 8 and 16
#endif

namespace tdsim {
namespace {

constexpr int NEAR_WPG = TD_NEAR_WPG;   // worlds one k_near_b workgroup serves with one read of its 32 matrix rows (at most 64)
static_assert(NEAR_WPG >= 1 && NEAR_WPG <= 64, "k_near_b keeps world l's bits in lane l");

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

// the route counters of a launch (td_sim_route): what the workgroup's threads served, one atomic per counter and workgroup.
// RouteOff: nothing, and no LDS.  Every thread of the workgroup calls it.
template <class R>
__device__ __forceinline__ void route_flush(const R &rt, const typename R::Acc &acc)
{
    if constexpr (R::on) {
        __shared__ long long s_rt[16];
        const long long nd = block_sum(acc.drops, s_rt);
        if (nd == 0) return;   // the same for the whole workgroup
        const long long ride = block_sum(acc.ride, s_rt), solo = block_sum(acc.solo, s_rt);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
        long long over = acc.over;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long u = __shfl_down(over, o);
            over = u > over ? u : over;
        }
        if (lane == 0) s_rt[wv] = over;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < nw; q++) over = s_rt[q] > over ? s_rt[q] : over;
            atomicAdd((unsigned long long *)&rt.cnt[0], (unsigned long long)nd);
            atomicAdd((unsigned long long *)&rt.cnt[1], (unsigned long long)ride);
            atomicAdd((unsigned long long *)&rt.cnt[2], (unsigned long long)solo);
            atomicMax(&rt.cnt[3], over);
        }
    }
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

// exclusive scan of v over the workgroup (full waves), *tot = the sum
__device__ __forceinline__ int block_excl_scan(int v, int *s_w, int *tot)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int off = 0, t = 0;
    for (int q = 0; q < nw; q++) {
        if (q < wv) off += s_w[q];
        t += s_w[q];
    }
    __syncthreads();
    *tot = t;
    return off + inc - v;
}

// the handle's error word as ONE value for the whole workgroup (a kernel is skipped as a whole once an earlier one failed)
__device__ __forceinline__ int block_err(const int32_t *gerr)
{
    __shared__ int s_e;
    if (threadIdx.x == 0) s_e = *gerr;
    __syncthreads();
    return s_e;
}

// does world b's model go through the LCM (analyzePairs)?  Without supply there is no model at all.
__device__ __forceinline__ bool world_lcm(int n_s, int n_d, int max_non_lcm) { return n_s > 0 && (n_s > n_d ? n_s : n_d) > max_non_lcm; }
// the model size above which the LCM ran in world b, as the kernels below take it (`max_non_lcm(b)`): one number for every
// world of the launch (a td_sim world, a td_simb handle without td_simb_dispatch), or a number per world (td_simb_dispatch:
// the world's own max_non_lcm; -1 where the LCM always runs, a model with supply has a row; INT_MAX where it never does)
struct LcmRule1 {
    int v;
    __device__ __forceinline__ int operator()(int) const { return v; }
};
struct LcmRuleB {
    const int32_t *v;
    __device__ __forceinline__ int operator()(int b) const { return v[b]; }
};

// the segments of a list behind an offset array [B + 1]
struct SegOff {
    const int32_t *off;
    __device__ __forceinline__ void operator()(int b, int *lo, int *n) const
    {
        *lo = off[b];
        *n = off[b + 1] - *lo;
    }
};

// ev: the event log's emitter (td_sim_core.h): EvOff, or EvOn on the arrival stage, slot = the cab's row
// rt: the route model (td_sim_core.h): RouteOff, or RouteOn / RouteOnB of a handle that has route storage
template <class S, class EV, class R>
__global__ __launch_bounds__(CB) void k_arrive(World w, S cabs, int t, Ctl *ctl, EV ev, R rt)
{
    __shared__ int s_red[16];
    const int b = blockIdx.y, l = blockIdx.x * CB + threadIdx.x;
    int lo, n;
    cabs(b, &lo, &n);
    const auto &rv = rt.of(b);   // the route of this workgroup's world
    typename R::Acc acc;
    const int got = l < n ? arrive_as(w, t, lo + l, l, ev, lo + l, rv, acc) : 0;
    route_flush(rv, acc);
    const int tot = block_sum(got, s_red);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) ctl[b].opt_count = 0;   // this tick's OPT count starts from zero
        if (tot) atomicAdd((unsigned long long *)&ctl[b].pickup_numb, (unsigned long long)tot);
    }
}

// world b's bitset `which` |= some element i of the world with who[i] == -1 has stand[i] == s.  World b: cab bits (which 0)
// at (2 b) * words, request bits (which 1) at (2 b + 1) * words.
template <class S>
__global__ __launch_bounds__(CB) void k_flags(S seg, int n_stands, const int32_t *__restrict__ stand, const int32_t *__restrict__ who,
                                              uint32_t *__restrict__ bits, int which)
{
    extern __shared__ uint32_t s_bits[];
    const int words = (n_stands + 31) / 32;
    const int b = blockIdx.y, l = blockIdx.x * CB + threadIdx.x;
    int lo, n;
    seg(b, &lo, &n);
    if ((int)blockIdx.x * CB >= n) return;   // the whole workgroup lies behind the world's segment
    for (int i = threadIdx.x; i < words; i += CB) s_bits[i] = 0;
    __syncthreads();
    if (l < n && who[lo + l] == -1) {
        const int s = stand[lo + l];
        atomicOr(&s_bits[s >> 5], 1u << (s & 31));
    }
    __syncthreads();
    uint32_t *out = bits + ((size_t)2 * b + which) * words;
    for (int q = threadIdx.x; q < words; q += CB)
        if (s_bits[q]) atomicOr(&out[q], s_bits[q]);
}

// near[b][which][q] bit j = any(nb[32 q + j][*] & flags_b[*]) for every world b; near is laid out like bits.
// Grid (words, ceil(B / NEAR_WPG)).  A workgroup of 16 waves owns the 32 stands of ONE output word (two stands per wave) for
// NEAR_WPG worlds: it stages those worlds' flag words in LDS, every wave loads its stand's matrix row into registers once
// (words <= 128: at most two words per lane) and then walks the worlds with one ballot each; lane l of the wave keeps the
// wave's two bits of world l, so a wave ORs them into LDS once, and a world's word leaves with a plain store.  The matrix
// is read ceil(B / NEAR_WPG) times, not B times; nothing needs clearing, there is no global atomic and no workgroup waits
// for another.  Every loop is bounded by NEAR_WPG or words.  Dynamic LDS: (NEAR_WPG * words + NEAR_WPG) words.
__global__ __launch_bounds__(CB) void k_near_b(int B, int n_stands, int words, const uint32_t *__restrict__ nb,
                                               const uint32_t *__restrict__ bits, uint32_t *__restrict__ near, int which)
{
    extern __shared__ uint32_t s_near[];
    uint32_t *s_flags = s_near, *s_out = s_near + NEAR_WPG * words;
    const int b0 = (int)blockIdx.y * NEAR_WPG, nw = B - b0 < NEAR_WPG ? B - b0 : NEAR_WPG;   // 1 <= nw <= NEAR_WPG by the grid
    for (int i = threadIdx.x; i < nw * words; i += CB) {
        const int wl = i / words, q = i - wl * words;
        s_flags[i] = bits[((size_t)2 * (b0 + wl) + which) * words + q];
    }
    if ((int)threadIdx.x < NEAR_WPG) s_out[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool in0 = lane < words, in1 = lane + 64 < words;
    uint32_t mine = 0;   // lane wl: this wave's two bits of world wl
    for (int j = 0; j < 2; j++) {
        const int bit = 2 * wv + j, s = (int)blockIdx.x * 32 + bit;
        if (s >= n_stands) break;   // the same for the whole wave
        const uint32_t *row = nb + (size_t)s * words;
        const uint32_t r0 = in0 ? row[lane] : 0u, r1 = in1 ? row[lane + 64] : 0u;
        for (int wl = 0; wl < nw; wl++) {
            const uint32_t *f = s_flags + wl * words;
            const uint32_t acc = (in0 ? r0 & f[lane] : 0u) | (in1 ? r1 & f[lane + 64] : 0u);
            if (__ballot(acc != 0) != 0ull && lane == wl) mine |= 1u << bit;
        }
    }
    if (mine) atomicOr(&s_out[lane], mine);   // mine != 0 only in a lane below nw
    __syncthreads();
    if ((int)threadIdx.x < nw) near[((size_t)2 * (b0 + threadIdx.x) + which) * words + blockIdx.x] = s_out[threadIdx.x];
}

inline dim3 near_grid(int B, int words) { return dim3(words, (B + NEAR_WPG - 1) / NEAR_WPG); }
inline size_t near_lds(int words) { return sizeof(uint32_t) * ((size_t)NEAR_WPG * words + NEAR_WPG); }

// predicates: (element in the concatenated index space, world).  createTempDemand's (Simulator.java:329-355) on the table as
// the drop pass left it.  near: the near bitsets of a table world (k_near_b), nullptr = the line's window over the flag bits
struct DemPred {
    World w;
    int t, words;
    const uint32_t *bits, *near;
    __device__ bool operator()(int d, int b) const
    {
        return w.r_cab[d] == -1 && t >= w.r_at[d] && t - w.r_at[d] < w.drop_time &&
               (near ? bit_of(near + (size_t)2 * b * words, w.r_from[d])
                     : near_window(bits + (size_t)2 * b * words, w.n_stands, w.drop_time, w.r_from[d]));
    }
};
// emitters: (position in the list, position in the list of the worlds with supply or -1, element, world)
struct DemEmit {
    World w;
    int32_t *idx, *from, *to, *pl_from, *pl_to;
    __device__ void operator()(int o, int o2, int d, int) const
    {
        idx[o] = d;
        from[o] = w.r_from[d];
        to[o] = w.r_to[d];
        if (o2 >= 0) {
            pl_from[o2] = w.r_from[d];
            pl_to[o2] = w.r_to[d];
        }
    }
};
// createTempSupply (Simulator.java:358-372)
struct SupPred {
    World w;
    int words;
    const uint32_t *bits, *near;
    __device__ bool operator()(int c, int b) const
    {
        return w.c_from[c] == w.c_to[c] && w.c_clnt[c] == -1 &&
               (near ? bit_of(near + ((size_t)2 * b + 1) * words, w.c_to[c])
                     : near_window(bits + ((size_t)2 * b + 1) * words, w.n_stands, w.drop_time, w.c_to[c]));
    }
};
struct SupEmit {
    World w;
    int32_t *cab, *to;
    __device__ void operator()(int o, int, int c, int) const
    {
        cab[o] = c;
        to[o] = w.c_to[c];
    }
};
// analyzePool (Simulator.java:760-784): every custB leaves, a custA carries its first plan
struct PoolPred {
    const int32_t *isb;
    __device__ bool operator()(int d, int) const { return !isb[d]; }
};
template <class PL, class S>
struct PoolEmit {
    PL pl;
    S dem;
    const int32_t *dem_idx, *dem_from, *ainfo, *pl_b, *pl_plan, *pl_cost;
    int32_t *idx, *from, *partner, *plan, *cost, *tk_from;
    __device__ void operator()(int o, int o2, int d, int b) const
    {
        idx[o] = dem_idx[d];
        from[o] = dem_from[d];
        const int p = ainfo[d];
        const bool a = p >= 0 && p < pl.count(b);
        const int q = pl.base(b) + (a ? p : 0);
        const int pb = a ? pl_b[q] : -1;   // k_pool_mark raised the error word for a plan outside the list; never index by it
        int d0, n_dem;
        dem(b, &d0, &n_dem);
        partner[o] = pb >= 0 && pb < n_dem ? dem_idx[d0 + pb] : -1;
        plan[o] = a ? pl_plan[q] : -1;
        cost[o] = a ? pl_cost[q] : 0;
        if (o2 >= 0) tk_from[o2] = dem_from[d];
    }
};
// ---- pools of up to four (td_sim_pooling_n).  A plan is a record of 9 ints: 4 pick-ups (-1 behind the pool's size), 4
// drop-offs, the cost; its members are positions in the tick's demand list.  The first pick-up stays in the demand and carries
// the size (in the plan column) and the cost; the second pick-up is its `partner`, the third and fourth lie in two more
// columns.  NP = the partners a customer can carry: 1 while every pool is a pair (the columns of a pair world are enough),
// 3 with pools of three or four.
template <int NP>
struct MorePartners {   // the partner columns behind the first: of the demand after pooling, of the kept demand
    const int32_t *d[NP - 1], *kd[NP - 1];
};
template <>
struct MorePartners<1> {};

// analyzePool for records: ainfo = the record of a first pick-up (k_pool_records marked it), every other member has left
template <int NP, class S>
struct PoolEmitN {
    S dem;
    int n_rec;
    const int32_t *dem_idx, *dem_from, *ainfo, *recs, *size;
    int32_t *idx, *from, *partner, *plan, *cost, *more[2];
    __device__ void operator()(int o, int, int d, int b) const
    {
        idx[o] = dem_idx[d];
        from[o] = dem_from[d];
        const int p = ainfo[d];
        const bool a = p >= 0 && p < n_rec;
        const int32_t *r = recs + (size_t)9 * (a ? p : 0);
        int d0, n_dem;
        dem(b, &d0, &n_dem);
        auto member = [&](int q) {   // k_pool_records raised the error word for a member outside the list; never index by it
            const int m = a ? r[q] : -1;
            return m >= 0 && m < n_dem ? dem_idx[d0 + m] : -1;
        };
        partner[o] = member(1);
        if constexpr (NP > 1) {
            more[0][o] = member(2);
            more[1][o] = member(3);
        }
        plan[o] = a ? size[p] : -1;
        cost[o] = a ? r[8] : 0;
    }
};

// ---- the route model (td_sim_route): the record of a first pick-up travels as one more column beside whatever the emitter E
// writes, the way MorePartners carries the partner columns; the dispatching thread builds the stop list from the record.
// (The record index and not the stops: one word per customer and list instead of eight, and the tick's records stay where
// k_pool_records left them until the apply.)  Handles without routes keep their emitters, and so their kernels, as they are.
// N: how many records world b has: a number (td_sim), or RecCountB of a batch: the world's own count, and none at all in a
// world that pools pairs (its ainfo holds a plan index, not a record index) or whose routes are off; no customer of such a
// world has a record, so no cab of it ever gets a stop
struct RecCountB {
    const int32_t *k_hi, *on, *n_rec;
    int stride;
    __device__ __forceinline__ int operator()(int b) const { return k_hi[b] && on[b] ? min(n_rec[b], stride) : 0; }
};
__device__ __forceinline__ int rec_count(int n, int) { return n; }
__device__ __forceinline__ int rec_count(const RecCountB &n, int b) { return n(b); }
template <class E, class N = int>
struct WithRec {   // the demand after pooling
    E e;
    const int32_t *ainfo;
    N n_rec;
    int32_t *rec;
    __device__ void operator()(int o, int o2, int d, int b) const
    {
        e(o, o2, d, b);
        const int p = ainfo[d];
        rec[o] = p >= 0 && p < rec_count(n_rec, b) ? p : -1;
    }
};
template <class E>
struct KeptRec {   // the kept demand
    E e;
    const int32_t *rec;
    int32_t *rec2;
    __device__ void operator()(int o, int o2, int d, int b) const
    {
        e(o, o2, d, b);
        rec2[o] = rec[d];
    }
};

// the cabs / requests of an LCM world that are in no pair (analyzePairs' supply2 / demand2)
template <class S, class L = LcmRule1>
struct KeptPred {
    const int32_t *pair_of;
    S sup, d2;
    L max_non_lcm;
    __device__ bool operator()(int i, int b) const
    {
        int s0, n_s, d0, n_d;
        sup(b, &s0, &n_s);
        d2(b, &d0, &n_d);
        return world_lcm(n_s, n_d, max_non_lcm(b)) && pair_of[i] == NONE;
    }
};
struct KeptSupEmit {
    const int32_t *cab, *to;
    int32_t *cab2, *to2;
    __device__ void operator()(int o, int, int s, int) const
    {
        cab2[o] = cab[s];
        to2[o] = to[s];
    }
};
struct KeptDemEmit {
    const int32_t *idx, *from, *partner, *plan, *cost;
    int32_t *idx2, *from2, *partner2, *plan2, *cost2;
    __device__ void operator()(int o, int, int d, int) const
    {
        idx2[o] = idx[d];
        from2[o] = from[d];
        partner2[o] = partner[d];
        plan2[o] = plan[d];
        cost2[o] = cost[d];
    }
};
// the same with the NP - 1 partner columns behind the first: from the demand after pooling (more) to the kept demand (more2)
template <int NP>
struct KeptDemEmitN {
    KeptDemEmit kept;
    const int32_t *more[NP - 1];
    int32_t *more2[NP - 1];
    __device__ void operator()(int o, int o2, int d, int b) const
    {
        kept(o, o2, d, b);
#pragma unroll
        for (int q = 0; q < NP - 1; q++) more2[q][o] = more[q][d];
    }
};

// the request pass of createTempDemand: drop what waited DROP_TIME (cab_assigned = -2), count the kept per workgroup.
// ev: EvOff, or EvOn on the drop stage, slot = the request's row (every request writes its slot: :339 or none)
template <class S, class EV>
__global__ __launch_bounds__(CB) void k_dem_count(DemPred pred, S reqs, int32_t *__restrict__ cnt, Ctl *ctl, EV ev)
{
    __shared__ int s_red[16];
    const World &w = pred.w;
    const int b = blockIdx.y, l = blockIdx.x * CB + threadIdx.x;
    int lo, n;
    reqs(b, &lo, &n);
    int drop = 0, keep = 0;
    if (l < n) {
        const int d = lo + l;
        if (w.r_cab[d] == -1 && pred.t >= w.r_at[d] && pred.t - w.r_at[d] >= w.drop_time) {
            w.r_cab[d] = -2;
            drop = 1;
        }
        if constexpr (EV::on) ev.put(d, drop ? TD_EV_DROPPED : 0, 0, drop ? w.r_id[d] : -1, -1, -1);
        keep = pred(d, b) ? 1 : 0;
    }
    const int nd = block_sum(drop, s_red), nk = block_sum(keep, s_red);
    if (threadIdx.x == 0) {
        cnt[b * gridDim.x + blockIdx.x] = nk;
        if (nd) atomicAdd((unsigned long long *)&ctl[b].dropped, (unsigned long long)nd);
    }
}

template <class S, class P>
__global__ __launch_bounds__(CB) void k_count(S seg, P pred, int32_t *__restrict__ cnt)
{
    __shared__ int s_red[16];
    const int b = blockIdx.y, l = blockIdx.x * CB + threadIdx.x;
    int lo, n;
    seg(b, &lo, &n);
    const int nk = block_sum((l < n && pred(lo + l, b)) ? 1 : 0, s_red);
    if (threadIdx.x == 0) cnt[b * gridDim.x + blockIdx.x] = nk;
}

// analyzePool's marks: plan p of world b makes its B customer leave and annotates its A customer (positions in the demand list)
template <class PL, class S>
__global__ __launch_bounds__(256) void k_pool_mark(PL pl, S dem, const int32_t *__restrict__ pl_a,
                                                   const int32_t *__restrict__ pl_b, int32_t *__restrict__ isb, int32_t *__restrict__ ainfo,
                                                   int32_t *gerr)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_act = pl.n_act(b);   // 0 for a world without supply: it has no pool
    if (p >= pl.count(b) || p >= n_act / 2) return;
    const int q = pl.base(b) + p;
    const int a = pl_a[q], c = pl_b[q];
    if (a < 0 || a >= n_act || c < 0 || c >= n_act) {
        atomicMax(gerr, 1);
        return;
    }
    int d0, n_dem;
    dem(b, &d0, &n_dem);
    isb[d0 + c] = 1;
    atomicMin(&ainfo[d0 + a], p);   // the first plan of an A customer (plans are disjoint anyway)
}

// by_cab / by_clnt of analyzePairs (Simulator.java:613-674) in every LCM world: the FIRST pair of a cab / of a request
template <class D, class S, class L>
__global__ __launch_bounds__(256) void k_pair_map(D dec, L max_non_lcm, S sup, S d2, int32_t *__restrict__ pair_cab,
                                                  int32_t *__restrict__ pair_dem, int32_t *gerr)
{
    const int b = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
    int s0, n_s, d0, n_d;
    sup(b, &s0, &n_s);
    d2(b, &d0, &n_d);
    if (!world_lcm(n_s, n_d, max_non_lcm(b))) return;
    int base, cnt;
    dec.pairs(b, &base, &cnt);
    if (p >= cnt) return;
    const int r = dec.rows[base + p], c = dec.cols[base + p];
    if (r < 0 || r >= n_s || c < 0 || c >= n_d) {
        atomicMax(gerr, 2);
        return;
    }
    atomicMin(&pair_cab[s0 + r], p);
    atomicMin(&pair_dem[d0 + c], p);
}

// analyzePairs: thread l < n_s of a world is the cab loop, the rest the request loop.  A cab and a request occur in at most
// one pair, so the two loops write disjoint state (fleet / request table) and share only the counters.  The cab number a
// request stores is world-local: cab minus where the world's fleet begins.
// ev: EvOff, or EvOn on the pairs stage (cleared by the host before the launch): thread l of world b owns slots
// 2 (s0 + d0 + l) and + 1, so the cab loop's records precede the request loop's and :654 precedes the same request's :432.
// px: the partner columns behind the first (NP = 3: a world of td_*_pooling_n with pools of three or four, never logged)
// rt: RouteOff, or RouteOn / RouteOnB bound to world b: the cab loop hands a pooled customer's cab its stop list
template <class D, class S, class EV, class L, int NP, class R>
__global__ __launch_bounds__(CB) void k_apply_pairs(World w, int t, D dec, L max_non_lcm, S cabs, S sup, S d2,
                                                    const int32_t *__restrict__ pair_cab, const int32_t *__restrict__ pair_dem,
                                                    const int32_t *__restrict__ sup_cab, const int32_t *__restrict__ sup_to,
                                                    const int32_t *__restrict__ d_idx, const int32_t *__restrict__ d_partner,
                                                    const int32_t *__restrict__ d_cost, Ctl *ctl, const int32_t *gerr, EV ev,
                                                    MorePartners<NP> px, R rt)
{
    static_assert(NP == 1 || !EV::on, "the apply stages own two staging slots per thread: a pool of four needs four");
    __shared__ int s_red[16];
    if (block_err(gerr)) return;
    const int b = blockIdx.y;
    int c0, n_c, s0, n_s, d0, n_d;
    cabs(b, &c0, &n_c);
    sup(b, &s0, &n_s);
    d2(b, &d0, &n_d);
    if (!world_lcm(n_s, n_d, max_non_lcm(b)) || (int)blockIdx.x * CB >= n_s + n_d) return;
    int base, cnt;
    dec.pairs(b, &base, &cnt);
    const int l = blockIdx.x * CB + threadIdx.x;
    const int slot = 2 * (s0 + d0 + l);
    int numb = 0, ptime = 0, second = 0;
    const auto &rv = rt.of(b);
    typename R::Acc acc;
    if (l < n_s) {
        const int p = pair_cab[s0 + l];
        if (p != NONE) {
            const int d = d0 + dec.cols[base + p];
            int rec = -1;
            if constexpr (R::on) rec = rv.d_rec[d];
            dispatch(w, t, sup_cab[s0 + l], sup_to[s0 + l], d_idx[d], d_partner[d], d_cost[d], numb, ptime, ev, slot, EV_LCM, sup_cab[s0 + l] - c0, rv,
                     rec, acc);
        }
    } else if (l < n_s + n_d) {
        const int d = d0 + l - n_s, p = pair_dem[d];
        if (p != NONE) {   // the request side is not guarded by the distance
            const int cab = sup_cab[s0 + dec.rows[base + p]] - c0, idx = d_idx[d];
            w.r_cab[idx] = cab;
            // with routes the cab loop's thread of a standing cab stores r_pick[idx] too (route_advance serves stop 0 = this request
            // at t): two threads, one value.  A change that makes the two values differ has to order the two stores
            w.r_pick[idx] = t;
            if constexpr (EV::on) ev.put(slot, TD_EV_ASSIGNED_LCM, 0, w.r_id[idx], cab, -1);
            if (d_partner[d] > -1) {
                w.r_cab[d_partner[d]] = cab;   // assignPooled; pool info is NOT copied into the table on this path
                second = 1;
                numb = 1;
                if constexpr (EV::on) ev.put(slot + 1, TD_EV_POOLED_SECOND, EV_LCM, w.r_id[d_partner[d]], cab, -1);
            }
            if constexpr (NP > 1) {
#pragma unroll
                for (int q = 0; q < NP - 1; q++) {
                    const int o = px.d[q][d];
                    if (o > -1) {   // assignPooled once per other member
                        w.r_cab[o] = cab;
                        second++;
                        numb++;
                    }
                }
            }
        }
    }
    route_flush(rv, acc);
    const int tn = block_sum(numb, s_red), tp = block_sum(ptime, s_red), ts = block_sum(second, s_red);
    if (threadIdx.x == 0) {
        if (tn) atomicAdd((unsigned long long *)&ctl[b].pickup_numb, (unsigned long long)tn);
        if (tp) atomicAdd((unsigned long long *)&ctl[b].pickup_time, (unsigned long long)tp);
        if (ts) atomicAdd((unsigned long long *)&ctl[b].second, (unsigned long long)ts);
    }
}

// analyzeSolution (Simulator.java:375-421): one thread per cab of the solver's model of world b: the kept lists where the
// LCM ran, else the whole model.  A supply entry's from == to holds by construction (createTempSupply admits only standing
// cabs and the lists are copies), so that test is not repeated.
// ev: EvOff, or EvOn on the solution stage (cleared by the host before the launch): cab l of world b's model owns slots
// 2 (s0 + l) and + 1 with s0 = where the world's SUPPLY list begins (a kept list is no longer): :432 first, then :448 / :486.
// rt: RouteOff, or RouteOn, as k_apply_pairs takes it
template <class D, class S, class EV, class L, int NP, class R>
__global__ __launch_bounds__(CB) void k_apply_solution(World w, int t, D dec, L max_non_lcm, S cabs, S sup, S d2, S ks, S kd,
                                                       const int32_t *__restrict__ sup_cab, const int32_t *__restrict__ sup_to,
                                                       const int32_t *__restrict__ d_idx, const int32_t *__restrict__ d_from,
                                                       const int32_t *__restrict__ d_partner, const int32_t *__restrict__ d_plan,
                                                       const int32_t *__restrict__ d_cost, const int32_t *__restrict__ ks_cab,
                                                       const int32_t *__restrict__ ks_to, const int32_t *__restrict__ kd_idx,
                                                       const int32_t *__restrict__ kd_from, const int32_t *__restrict__ kd_partner,
                                                       const int32_t *__restrict__ kd_plan, const int32_t *__restrict__ kd_cost, Ctl *ctl,
                                                       const int32_t *gerr, EV ev, MorePartners<NP> px, R rt)
{
    static_assert(NP == 1 || !EV::on, "the apply stages own two staging slots per thread: a pool of four needs four");
    __shared__ int s_red[16];
    if (block_err(gerr)) return;
    const int b = blockIdx.y;
    int c0, n_c, s0, n_s, d0, n_d;
    cabs(b, &c0, &n_c);
    sup(b, &s0, &n_s);
    d2(b, &d0, &n_d);
    if (n_s == 0 || (int)blockIdx.x * CB >= n_s) return;
    const bool lcm = world_lcm(n_s, n_d, max_non_lcm(b));
    int rb, nr;
    bool solved;
    dec.r2c_of(b, lcm, w.big_cost, &rb, &nr, &solved);
    if (lcm && !solved) return;
    const int slot0 = 2 * s0;
    if (lcm) {   // the kept lists: their sizes are on the device in both handles
        ks(b, &s0, &n_s);
        kd(b, &d0, &n_d);
    }
    const int32_t *l_cab = lcm ? ks_cab : sup_cab, *l_to = lcm ? ks_to : sup_to, *l_idx = lcm ? kd_idx : d_idx, *l_from = lcm ? kd_from : d_from;
    const int32_t *l_partner = lcm ? kd_partner : d_partner, *l_plan = lcm ? kd_plan : d_plan, *l_cost = lcm ? kd_cost : d_cost;
    const int l = blockIdx.x * CB + threadIdx.x;
    int count = 0, numb = 0, ptime = 0, second = 0;
    const auto &rv = rt.of(b);
    typename R::Acc acc;
    if (l < n_s) {
        const int s = s0 + l;
        const int c = l < nr ? dec.r2c[rb + l] : -1;
        if (c >= 0 && c < n_d) {
            const int e = d0 + c;
            const int dist = way(w, l_to[s], l_from[e]);
            const int cell = dist < w.drop_time ? dist : w.big_cost;   // the thresholded model's cell
            if (cell < w.big_cost) {
                count = 1;
                const int idx = l_idx[e], cab = l_cab[s], partner = l_partner[e];
                w.r_cab[idx] = cab - c0;
                w.r_pick[idx] = t;
                if (partner > -1) {
                    w.r_cab[partner] = cab - c0;
                    second = 1;
                    w.r_pid[idx] = w.r_id[partner];   // pool info reaches the table on the OPT path only (:391-396)
                    w.r_plan[idx] = l_plan[e];
                    w.r_pcost[idx] = l_cost[e];
                    numb = 1;
                    if constexpr (EV::on) ev.put(slot0 + 2 * l, TD_EV_POOLED_SECOND, EV_OPT, w.r_id[partner], cab - c0, -1);
                }
                if constexpr (NP > 1) {
#pragma unroll
                    for (int q = 0; q < NP - 1; q++) {
                        const int o = (lcm ? px.kd[q] : px.d[q])[e];
                        if (o > -1) {   // assignPooled once per other member; the table keeps the second pick-up's id
                            w.r_cab[o] = cab - c0;
                            second++;
                            numb++;
                        }
                    }
                }
                int rec = -1;
                if constexpr (R::on) rec = (lcm ? rv.kd_rec : rv.d_rec)[e];
                dispatch(w, t, cab, l_to[s], idx, partner, l_cost[e], numb, ptime, ev, slot0 + 2 * l + 1, EV_OPT, cab - c0, rv, rec, acc);
            }
        }
    }
    route_flush(rv, acc);
    const int tc = block_sum(count, s_red), tn = block_sum(numb, s_red), tp = block_sum(ptime, s_red), ts = block_sum(second, s_red);
    if (threadIdx.x == 0) {
        if (tc) atomicAdd(&ctl[b].opt_count, tc);
        if (tn) atomicAdd((unsigned long long *)&ctl[b].pickup_numb, (unsigned long long)tn);
        if (tp) atomicAdd((unsigned long long *)&ctl[b].pickup_time, (unsigned long long)tp);
        if (ts) atomicAdd((unsigned long long *)&ctl[b].second, (unsigned long long)ts);
    }
}

// ---- the event log: one tick's records of world b as ONE virtual slot sequence, in the order Simulator.java writes them:
//   A  n_cabs   the arrival stage (k_arrive)          E  0 / 1      the pool header, where findPool ran
//   B  n_req    the drop stage (k_dem_count)          F  plans      the plan list of findPool, as the pool call left it
//   C  1        the tempDemand header                 G  2 (ns+nd)  the pairs stage (k_apply_pairs), LCM worlds
//   D  n_dem    the demand list before pooling        H  2 ns       the solution stage (k_apply_solution)
// C .. F are not staged: they are read from the lists where they lie.  phase bit 0 = A .. F (td_*_begin's), bit 1 = G, H.
template <class S, class PL, class L = LcmRule1>
struct EvSrc {
    World w;
    S cabs, reqs, dem, sup, d2;
    PL pl;
    L max_non_lcm;
    int t, phase;
    uint32_t kinds;
    const int4 *st_arr, *st_drop, *st_pairs, *st_sol;
    const int32_t *dem_idx, *pl_a, *pl_b;
    // slot v of world b -> its kind (0: no record, a masked kind, or v behind the sequence); *o = {kind | method << 8, customer, cab, aux}
    __device__ int read(int b, int v, int4 *o) const
    {
        int c0, nc, r0, nr, e0, ne, s0, ns, d0, nd;
        cabs(b, &c0, &nc);
        reqs(b, &r0, &nr);
        dem(b, &e0, &ne);
        sup(b, &s0, &ns);
        d2(b, &d0, &nd);
        const bool p1 = phase & 1, p2 = phase & 2, pooled = ne > 0 && ns > 0;
        const bool found = pooled && pl.n_act(b) > 0;   // findPool ran: not in a world whose policy is TD_POOL_NONE
        int np = 0;   // plans: never more than the pooled customers allow, whatever the count word says
        if (found) np = min(max(pl.count(b), 0), pl.n_act(b) / 2);
        const int nA = p1 ? nc : 0, nB = p1 ? nr : 0, nC = p1 ? 1 : 0, nD = p1 ? ne : 0, nE = p1 && found ? 1 : 0, nF = p1 ? np : 0;
        const int nG = p2 && ne > 0 && world_lcm(ns, nd, max_non_lcm(b)) ? 2 * (ns + nd) : 0, nH = p2 && pooled ? 2 * ns : 0;
        int4 r = make_int4(0, -1, -1, -1);
        int u = v;
        if (u < nA) {
            r = st_arr[c0 + u];
        } else if ((u -= nA) < nB) {
            r = st_drop[r0 + u];
        } else if ((u -= nB) < nC) {
            r.x = TD_EV_TEMP_DEMAND;
            r.w = ne;
        } else if ((u -= nC) < nD) {
            r.x = TD_EV_TEMP_DEMAND_ID;
            r.y = w.r_id[dem_idx[e0 + u]];
        } else if ((u -= nD) < nE) {
            r.x = TD_EV_POOL;
            r.w = np;
        } else if ((u -= nE) < nF) {
            const int q = pl.base(b) + u, a = pl_a[q], c = pl_b[q], n_act = pl.n_act(b);
            r.x = TD_EV_POOL_PAIR;
            r.y = a >= 0 && a < n_act ? w.r_id[dem_idx[e0 + a]] : -1;   // k_pool_mark raised the error word for such a plan
            r.w = c >= 0 && c < n_act ? w.r_id[dem_idx[e0 + c]] : -1;
        } else if ((u -= nF) < nG) {
            r = st_pairs[2 * (s0 + d0) + u];
        } else if ((u -= nG) < nH) {
            r = st_sol[2 * s0 + u];
        }
        *o = r;
        const int kind = r.x & 255;
        return (kinds >> kind) & 1u ? kind : 0;   // bit 0 is never set
    }
};

// the log's device words: records held, records that did not fit since the last drain, where this flush appends
struct EvCtl {
    long long n, lost, base, pad;
};

template <class SRC>
__global__ __launch_bounds__(CB) void k_ev_count(SRC src, int32_t *__restrict__ cnt)
{
    __shared__ int s_red[16];
    int4 r;
    const int nk = block_sum(src.read(blockIdx.y, blockIdx.x * CB + threadIdx.x, &r) ? 1 : 0, s_red);
    if (threadIdx.x == 0) cnt[blockIdx.y * gridDim.x + blockIdx.x] = nk;
}

// ONE workgroup: per-workgroup counts -> where each world's records begin within this flush (B in slices of CB), then the
// log's words: the flush appends at lg->base, as much of it as fits is counted in, the rest is counted as lost
__global__ __launch_bounds__(CB) void k_ev_offsets(int B, const int32_t *__restrict__ cnt, int nc, int32_t *__restrict__ woff, EvCtl *lg,
                                                   long long cap)
{
    __shared__ int s_w[16];
    int run = 0;
    for (int b0 = 0; b0 < B; b0 += CB) {
        const int b = b0 + threadIdx.x;
        int na = 0;
        if (b < B)
            for (int j = 0; j < nc; j++) na += cnt[b * nc + j];
        int ta;
        const int ea = block_excl_scan(na, s_w, &ta);
        if (b < B) woff[b] = run + ea;
        run += ta;
    }
    if (threadIdx.x == 0) {
        const long long base = lg->n, room = cap - base, kept = run < room ? run : room;
        lg->base = base;
        lg->n = base + kept;
        lg->lost += run - kept;
    }
}

// log[base + the world's offset + the counts of the world's earlier chunks + rank] = the record; nothing at or behind cap
template <class SRC>
__global__ __launch_bounds__(CB) void k_ev_scatter(SRC src, const int32_t *__restrict__ cnt, const int32_t *__restrict__ woff,
                                                   const EvCtl *__restrict__ lg, long long cap, int4 *__restrict__ log)
{
    __shared__ int s_red[16];
    const int b = blockIdx.y;
    int part = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += CB) part += cnt[b * gridDim.x + j];
    const int before = block_sum(part, s_red);
    int4 r;
    const int kind = src.read(b, blockIdx.x * CB + threadIdx.x, &r);
    int tot;
    const int rank = block_rank(kind != 0, s_red, &tot);
    if (!kind) return;
    const long long pos = lg->base + woff[b] + before + rank;
    if (pos < 0 || pos >= cap) return;
    log[2 * pos] = make_int4(src.t, b, kind, (r.x >> 8) & 255);
    log[2 * pos + 1] = make_int4(r.y, r.z, r.w, 0);
}

// Simulator.c_clnt holds the request id; cabs [lo, lo + n)
__global__ __launch_bounds__(256) void k_client_ids(World w, int lo, int n, int32_t *__restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int d = w.c_clnt[lo + c];
    out[c] = d < 0 ? -1 : w.r_id[d];
}

// ---- host helpers of both handles; everything is queued on the library's stream

inline int put(int32_t *dst, const int32_t *src, size_t n)
{
    if (!n) return TD_OK;
    TD_HIP(hipMemcpyAsync(dst, src, sizeof(int32_t) * n, td::is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, td::ctx().stream));
    return TD_OK;
}

inline int get(int32_t *dst, const int32_t *src, size_t n)
{
    if (!n || !dst) return TD_OK;
    TD_HIP(hipMemcpyAsync(dst, src, sizeof(int32_t) * n, td::is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, td::ctx().stream));
    return TD_OK;
}

// the world's tables where the handle's layout put them; dist == nullptr: the world lives on the line
inline void set_tables(World &w, const WorldDev &d, const int32_t *dist)
{
    w.dist = dist;
    w.r_id = d.r_id, w.r_from = d.r_from, w.r_to = d.r_to, w.r_at = d.r_at;
    w.r_cab = d.r_cab, w.r_pick = d.r_pick, w.r_pid = d.r_pid, w.r_plan = d.r_plan, w.r_pcost = d.r_pcost;
    w.c_from = d.c_from, w.c_to = d.c_to, w.c_clnt = d.c_clnt, w.c_onb = d.c_onb, w.c_start = d.c_start;
}

// the request file on the host once: h = ids, from, to, at behind one another (n_req each; host or device sources)
inline int load_requests(int n_req, const int32_t *id, const int32_t *from, const int32_t *to, const int32_t *at, std::vector<int32_t> &h)
{
    h.resize((size_t)4 * n_req);
    const int32_t *src[4] = {id, from, to, at};
    for (int q = 0; q < 4 && n_req; q++) TD_HIP(hipMemcpy(h.data() + (size_t)q * n_req, src[q], sizeof(int32_t) * (size_t)n_req, hipMemcpyDefault));
    return TD_OK;
}

// the first request of [lo, hi) that is outside the world (id or arrival time negative, a stand outside the city); -1: none
inline int bad_request(const std::vector<int32_t> &h, int n_req, int n_stands, int lo, int hi)
{
    for (int i = lo; i < hi; i++) {
        const int32_t id = h[i], f = h[(size_t)n_req + i], to = h[(size_t)2 * n_req + i], at = h[(size_t)3 * n_req + i];
        if (id < 0 || f < 0 || f >= n_stands || to < 0 || to >= n_stands || at < 0) return i;
    }
    return -1;
}

inline bool ids_unique(const std::vector<int32_t> &h, int lo, int hi)
{
    std::vector<int32_t> ids(h.begin() + lo, h.begin() + hi);
    std::sort(ids.begin(), ids.end());
    return std::adjacent_find(ids.begin(), ids.end()) == ids.end();
}

// the handle's own copy of the table (d_dist), then its bit matrices; k_nb_build reports an invalid table in *err, which the
// handle reads back after the stream is drained and hands to table_verdict
inline int table_upload(const char *launch, const int32_t *dist, int n_stands, int words, int drop_time, int32_t *d_dist, uint32_t *nb_dem,
                        uint32_t *nb_sup, int32_t *err)
{
    const hipStream_t st = td::ctx().stream;
    hipError_t e = hipMemcpyAsync(d_dist, dist, sizeof(int32_t) * (size_t)n_stands * n_stands,
                                  td::is_device_ptr(dist) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return td::hip_fail(e, "hipMemcpyAsync(distance table)");
    const int cells = n_stands * words;
    k_nb_build<<<(cells + 255) / 256, 256, 0, st>>>(n_stands, words, drop_time, d_dist, nb_dem, nb_sup, err);
    if ((e = hipGetLastError()) != hipSuccess) return td::hip_fail(e, launch);
    return TD_OK;
}

inline int table_verdict(const char *who, int err)
{
    return err ? td::fail(TD_EINVAL, "%s: the distance table needs a zero diagonal and every other entry in 1 .. %d", who, MAX_DIST) : TD_OK;
}

// ---- the event log's host side, one per handle.  Everything *_log allocates is in `mem`.
struct EvLog {
    uint32_t kinds = 0;          // 0: logging is off
    long long cap = 0;           // records the log holds
    td::Buf mem;
    EvCtl *ctl = nullptr;
    int4 *log = nullptr, *st_arr = nullptr, *st_drop = nullptr, *st_pairs = nullptr, *st_sol = nullptr;
    int32_t *cnt = nullptr, *woff = nullptr;
    int chunks = 0;              // workgroups per world the count array has room for
    bool begin_flushed = false;  // the begun tick's sections A .. F are in the log already (a drain before its apply)
};

inline int ev_off(EvLog &ev)
{
    if (ev.mem.p && td::ctx().inited) (void)hipStreamSynchronize(td::ctx().stream);
    td::buf_free(ev.mem);
    ev = EvLog();
    return TD_OK;
}

// td_sim_log / td_simb_log after their argument checks: B worlds, nc cabs and nr requests in all, at most vmax slots per world
inline int ev_setup(EvLog &ev, uint32_t kinds, int64_t capacity, int B, size_t nc, size_t nr, size_t vmax)
{
    ev_off(ev);
    if (!kinds) return TD_OK;
    const size_t chunks = (vmax + CB - 1) / CB;
    int rc = td::carve_buf(ev.mem, [&](td::Carve &c) {
        ev.ctl = c.take<EvCtl>(1);
        ev.log = c.take<int4>(2 * (size_t)capacity);
        ev.st_arr = c.take<int4>(nc);
        ev.st_drop = c.take<int4>(nr);
        ev.st_pairs = c.take<int4>(2 * (nc + nr));
        ev.st_sol = c.take<int4>(2 * nc);
        ev.cnt = c.take<int32_t>((size_t)B * chunks);
        ev.woff = c.take<int32_t>((size_t)B);
    });
    if (rc) return rc;
    ev.chunks = (int)chunks;
    ev.cap = capacity;
    hipError_t e = hipMemsetAsync(ev.ctl, 0, sizeof(EvCtl), td::ctx().stream);
    if (e != hipSuccess) {
        ev_off(ev);
        return td::hip_fail(e, "hipMemsetAsync(event log)");
    }
    ev.kinds = kinds;
    return TD_OK;
}

// the pairs and solution stages start a td_*_apply empty, as far as this tick's lists reach (n_sup, n_d2: the totals)
inline int ev_clear_apply(EvLog &ev, size_t n_sup, size_t n_d2)
{
    const hipStream_t st = td::ctx().stream;
    if (n_sup + n_d2) TD_HIP(hipMemsetAsync(ev.st_pairs, 0, sizeof(int4) * 2 * (n_sup + n_d2), st));
    if (n_sup) TD_HIP(hipMemsetAsync(ev.st_sol, 0, sizeof(int4) * 2 * n_sup, st));
    return TD_OK;
}

// appends the records src yields, in order, to the log: count, offsets, scatter; vmax = the longest world's slot sequence
template <class SRC>
int ev_flush(EvLog &ev, const SRC &src, int B, size_t vmax)
{
    const hipStream_t st = td::ctx().stream;
    const int chunks = (int)std::min<size_t>(std::max<size_t>((vmax + CB - 1) / CB, 1), (size_t)ev.chunks);
    const dim3 grid(chunks, B);
    k_ev_count<<<grid, CB, 0, st>>>(src, ev.cnt);
    k_ev_offsets<<<1, CB, 0, st>>>(B, ev.cnt, chunks, ev.woff, ev.ctl, ev.cap);
    k_ev_scatter<<<grid, CB, 0, st>>>(src, ev.cnt, ev.woff, ev.ctl, ev.cap, ev.log);
    TD_HIP(hipGetLastError());
    return TD_OK;
}

// td_sim_events / td_simb_events once every record of the work done so far is queued for the log
inline int ev_drain(EvLog &ev, const char *who, int64_t max_records, int32_t *records, int64_t *n, int64_t *lost)
{
    const hipStream_t st = td::ctx().stream;
    *n = 0;
    if (lost) *lost = 0;
    if (!ev.kinds) return TD_OK;
    long long h[2];
    TD_HIP(hipMemcpyAsync(h, ev.ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    TD_HIP(hipStreamSynchronize(st));
    *n = h[0];
    if (h[0] > max_records) return td::fail(TD_EINVAL, "%s: %lld records are buffered, max_records = %lld", who, h[0], (long long)max_records);
    if (h[0] && !records) return td::fail(TD_EINVAL, "%s: null records", who);
    int rc = get(records, (const int32_t *)ev.log, (size_t)h[0] * 8);
    if (rc) return rc;
    TD_HIP(hipMemsetAsync(ev.ctl, 0, sizeof(EvCtl), st));
    TD_HIP(hipStreamSynchronize(st));
    if (lost) *lost = h[1];
    return TD_OK;
}

// td_sim_state / td_simb_state: cabs [c0, c0 + ncab) and requests [r0, r0 + nreq) of the tables, five arrays each (a null
// destination is skipped); the client column is the request id, made in tmp
inline int state_out(const World &w, int c0, int ncab, int r0, int nreq, int32_t *tmp, int32_t *const cd[5], int32_t *const rd[5])
{
    const hipStream_t st = td::ctx().stream;
    int rc;
    if (cd[2]) {
        k_client_ids<<<(ncab + 255) / 256, 256, 0, st>>>(w, c0, ncab, tmp);
        TD_HIP(hipGetLastError());
    }
    const int32_t *cs[5] = {w.c_from + c0, w.c_to + c0, tmp, w.c_onb + c0, w.c_start + c0};
    const int32_t *rs[5] = {w.r_cab + r0, w.r_pick + r0, w.r_pid + r0, w.r_plan + r0, w.r_pcost + r0};
    for (int q = 0; q < 5; q++)
        if ((rc = get(cd[q], cs[q], (size_t)ncab)) || (rc = get(rd[q], rs[q], (size_t)nreq))) return rc;
    TD_HIP(hipStreamSynchronize(st));
    return TD_OK;
}

// one world's nine metrics: the device sums of its Ctl and the host side of Simulator.m
inline void fill_metrics(const Ctl &h, int64_t lcm_used, int64_t max_model, int64_t max_solver, int64_t max_pool_mem, int64_t max_pool, int64_t *o)
{
    o[0] = h.dropped;
    o[1] = h.pickup_time;
    o[2] = h.pickup_numb;
    o[3] = lcm_used;
    o[4] = max_model;
    o[5] = max_solver;
    o[6] = max_pool_mem;
    o[7] = max_pool;
    o[8] = h.second;
}

}  // namespace
}  // namespace tdsim
