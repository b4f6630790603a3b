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
// td_pool_n_banded_batched is the same walk with td_pool_n_banded's band loop inside the workgroup: a model is
// answered one key interval at a time (count by cost, cut, enumerate, select, the used requests carried along), so the slab
// of a workgroup is bounded by the caller and no model is refused for its plan count.  k_pooln_banded_batched shares the
// queues, the append, the decode and the selection with k_pooln_batched; that kernel keeps its own statements inline, because
// the same statements behind pnb_stage / pnb_pairs / pnb_select changed its register counts.
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
    int internal;   // td_pool_n_banded_batched: batch - (first model whose band loop met what cannot be), 0: none
    int kind, level;                 // of that model: 1 keys != histogram, 2 an empty histogram, 3 an over-full last digit; the cut level
    unsigned long long got, want;    // the two counts
};

// floor(c / d) for 2 <= d <= 512 and c * d < 2^32, with m = 2^32 / d + 1 (the error term of m is at most d / 2^32 per unit)
__device__ __forceinline__ uint32_t pnb_div(uint32_t c, uint32_t m) { return __umulhi(c, m); }

struct PnbModel {
    static constexpr bool banded = false;
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

// ---- td_pool_n_banded_batched: the same walk as one PASS of td_pool_n_banded's band loop ----
constexpr int PNB_BINS = PN_MAXCOST + 1;         // the cost histogram of a workgroup, in global memory
constexpr int PNB_GROUPS = PNB_BINS / 64;        // its sums per 64 costs, in LDS
constexpr unsigned long long PNB_END = ~0ull;    // above every key

// what a pass filters by and where its plans go: counted into a histogram (the cost in global memory, a pick-up in LDS) or
// appended as keys.  Every member is uniform over the workgroup.
struct PnbBandModel : PnbModel {
    static constexpr bool banded = true;
    unsigned long long klo, khi;        // the key interval [klo, khi)
    bool count;
    int level;                          // count: the digit to histogram: 0 the cost, l >= 1 pick-up p[l - 1]
    unsigned long long *hist;           // PNB_BINS counters, all zero between two count passes
};

template <int K>
struct PnbBandShared : PnbShared<K> {
    unsigned long long hist[PNB_MAXN];      // levels 1 ..: plans per pick-up under the prefix
    unsigned long long gsum[PNB_GROUPS];    // level 0: plans per 64 costs
    unsigned long long tot;                 // level 0: all of them
    unsigned long long hi, expect, prefix;  // the choice, made by thread 0
    int b0;                                 // level 0: the lowest cost with a plan
    int act;                                // 0: the band is [lo, hi), 1: count one digit deeper under prefix, 2: internal error
};

// One happy-or-not plan per lane, every lane of the wave here.  Count: the lanes inside the interval go to the histogram, one
// atomic per distinct bin of the wave (k_band_enum's pb_sink); else their keys are appended, one LDS atomic per wave.
template <class SH>
__device__ __forceinline__ void pnb_band_sink(SH &sh, const PnbBandModel &x, bool happy, int cost, const int *p, unsigned long long seq)
{
    bool in = happy;
    if (happy && (cost > PN_MAXCOST || cost < 0)) {   // never a bin or a key
        sh.err = 1;
        in = false;
    }
    const unsigned long long key = ((unsigned long long)(in ? cost : 0) << PN_SEQ_BITS) | seq;
    in = in && key >= x.klo && key < x.khi;
    if (x.count) {
        unsigned long long m = __ballot(in);
        if (!m) return;
        const int lane = threadIdx.x & 63;
        const int bin = x.level == 0 ? cost : x.level == 1 ? p[0] : x.level == 2 ? p[1] : p[2];   // no indexed p[]: it stays in registers
        while (m) {
            const int leader = __ffsll((long long)m) - 1;
            const int b = __shfl(bin, leader);
            const unsigned long long same = __ballot(in && bin == b);
            if (lane == leader) {
                if (x.level == 0) atomicAdd(&x.hist[b], (unsigned long long)__popcll(same));
                else atomicAdd(&sh.hist[b], (unsigned long long)__popcll(same));
            }
            m &= ~same;
        }
    } else {
        const unsigned long long idx = pnb_append(in, &sh.happy);
        if (in && idx < x.cap) x.keys[idx] = key;
    }
}

// one drop-off order of this thread's tuple: happiness, cost, and the wave's happy plans appended with one atomic
template <int K, int QI, class SH, class X>
__device__ __forceinline__ void pnb_order(SH &sh, const X &x, bool valid, const int *p, unsigned long long seq0)
{
    constexpr PnOrder o = pn_order(K, QI);
    const int q[4] = {o.q[0], o.q[1], o.q[2], o.q[3]};
    int cost = 0;
    const bool happy = valid && pn_check<K>(p, q, x.sf, x.st, x.sl, x.dist, x.S, &cost);
    if constexpr (X::banded) {
        pnb_band_sink(sh, x, happy, cost, p, seq0 + (unsigned long long)QI);
    } else {
        const unsigned long long idx = pnb_append(happy, &sh.happy);
        if (happy) {
            if (cost > PN_MAXCOST || cost < 0) sh.err = 1;
            else if (idx < x.cap) x.keys[idx] = ((unsigned long long)cost << PN_SEQ_BITS) | (seq0 + (unsigned long long)QI);
        }
    }
}

template <int K, class SH, class X, int... QI>
__device__ __forceinline__ void pnb_orders(std::integer_sequence<int, QI...>, SH &sh, const X &x, bool valid, const int *p,
                                           unsigned long long seq0)
{
    (pnb_order<K, QI>(sh, x, valid, p, seq0), ...);
}

// the k! drop-off orders of every full tuple of the last queue: one tuple per thread
template <int K, class SH, class X>
__device__ __forceinline__ void pnb_check(SH &sh, const X &x)
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
// A banded model (td_pool_n_banded_batched) drops a candidate whose newest member is used here, before the k! orders.
template <int K, int M, class SH, class X>
__device__ __forceinline__ void pnb_drain(SH &sh, const X &x, bool final)
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
                    if constexpr (X::banded) pass = pass && !((sh.used[cand >> 5] >> (cand & 31)) & 1u);
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

// The selection over the m keys at x.keys: every wave owns a segment of the slab and keeps its live keys at the segment's
// front; a round takes the smallest live key, marks its requests in sh.used and writes its record at out + kept.  Ends when no
// key is live or nb / K pools are kept.  sh.used and kept come in as the caller left them: td_pool_n_banded_batched calls this
// once per band.
template <int K, class SH, class X>
__device__ __forceinline__ void pnb_select(SH &sh, const X &x, const unsigned char *s_perm, int m, int32_t *out, int &kept, long long &sum)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nb = x.nb;
    const size_t rec = (size_t)(2 * K + 1);
    const int seg = (m + PNB_W - 1) / PNB_W;
    unsigned long long *mine = x.keys + (size_t)w * (size_t)seg;
    int wcnt = max(0, min(seg, m - w * seg));
    const double inv_d2 = 1.0 / (24.0 * (double)nb * (double)nb);
    const int max_kept = nb / K;
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

// V: the models are worlds (td::pool_n_worlds): model b's requests lie at off[b], sel.cnt[b] of them, and only where the world's
// cascade has a stage of K (sel.k_lo[b] <= K <= sel.k_hi[b]), else the model is empty; wait / loss hold one rule per model
template <bool V>
struct PnbSel {};
template <>
struct PnbSel<true> {
    const int32_t *cnt, *k_hi, *k_lo;
};

// model b into LDS and x (all but the slab): the requests, the slice, empty queues, nothing used, no error
template <int K, bool V, class SH>
__device__ __forceinline__ void pnb_stage(SH &sh, PnbModel &x, int b, int n, const int32_t *__restrict__ off, const int32_t *__restrict__ from,
                                          const int32_t *__restrict__ to, const int32_t *__restrict__ wait, const int32_t *__restrict__ loss,
                                          const int32_t *__restrict__ dist, int S, const int32_t *__restrict__ first, const PnbSel<V> &sel)
{
    const int tid = threadIdx.x;
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
}

// level 1: the (first, second) pairs of the first pick-ups [f0, f1), then everything behind them
template <int K, class SH, class X>
__device__ __forceinline__ void pnb_pairs(SH &sh, const X &x, int f0, int f1)
{
    const int tid = threadIdx.x, nb = x.nb;
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
                len = pn_d(x.dist, x.S, x.sf[p0], x.sf[p1]);
                // pool_n.c:177 at level 0 (an empty path against WAIT), then :177-178 for the second pick-up
                pass = !(0 > x.sw[p0]) && p1 != p0 && !(len > x.sw[p1]);
                if constexpr (X::banded) pass = pass && !(((sh.used[p0 >> 5] >> (p0 & 31)) | (sh.used[p1 >> 5] >> (p1 & 31))) & 1u);
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

__device__ __forceinline__ unsigned long long pnb_ld(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // where the atomics went, not L1
}

// thread 0 after a count at level 0: the longest run of costs from the lowest non-empty one that fits `room`, or one digit deeper
template <class SH>
__device__ __forceinline__ void pnb_choose_cost(SH &sh, const unsigned long long *hist, unsigned long long room)
{
    const int b0 = sh.b0;
    if (pnb_ld(hist + b0) > room) {
        sh.prefix = (unsigned long long)b0 << PN_SEQ_BITS;
        sh.act = 1;
        return;
    }
    unsigned long long acc = 0;
    int g = b0 >> 6;   // the costs below b0 are empty
    while (g < PNB_GROUPS && acc + sh.gsum[g] <= room) acc += sh.gsum[g++];
    int b1 = PNB_BINS;
    if (g < PNB_GROUPS) {   // this group does not fit whole: the run ends inside it
        b1 = g * 64;
        while (b1 < g * 64 + 64) {
            const unsigned long long v = pnb_ld(hist + b1);
            if (acc + v > room) break;
            acc += v;
            b1++;
        }
    }
    sh.hi = b1 == PNB_BINS ? PNB_END : (unsigned long long)b1 << PN_SEQ_BITS;
    sh.expect = acc;
    sh.act = 0;
}

// thread 0 after a count at level >= 1: the same over the nb pick-ups under `prefix`; wgt: the digit's weight in the key
template <int K, class SH>
__device__ __forceinline__ void pnb_choose_pick(SH &sh, int nb, int level, unsigned long long prefix, unsigned long long wgt,
                                                unsigned long long room)
{
    int b0 = 0;
    while (b0 < nb && sh.hist[b0] == 0) b0++;
    sh.act = 2;
    sh.expect = 0;
    if (b0 == nb) return;   // the level above counted plans here
    if (sh.hist[b0] <= room) {
        unsigned long long acc = 0;
        int b1 = b0;
        while (b1 < nb && acc + sh.hist[b1] <= room) acc += sh.hist[b1++];
        sh.hi = prefix + (unsigned long long)b1 * wgt;
        sh.expect = acc;
        sh.act = 0;
    } else if (level < K - 1) {
        sh.prefix = prefix + (unsigned long long)b0 * wgt;
        sh.act = 1;
    } else {   // one value of the last digit but one holds more than 24 nb plans
        sh.expect = sh.hist[b0];
    }
}

// td_pool_n_banded_batched: k_pooln_batched's workgroup per model with td_pool_n_banded's band loop inside the workgroup.
// Per model: count the live plans from lo on by cost, choose [lo, hi), write its live plans to the slab (at most cap), select
// over them with sh.used carried on, lo = hi.  Every pass is the same walk (pnb_pairs); a model's passes are iterations of
// ONE loop, so the walk is compiled once.  hist_all: PNB_BINS zeroed counters per workgroup, zero again when the kernel ends.
template <int K, bool V = false>
__global__ __launch_bounds__(PNB_T) void k_pooln_banded_batched(int batch, int n, const int32_t *__restrict__ off,
                                                                const int32_t *__restrict__ from, const int32_t *__restrict__ to,
                                                                const int32_t *__restrict__ wait, const int32_t *__restrict__ loss,
                                                                const int32_t *__restrict__ dist, int S, const int32_t *__restrict__ first,
                                                                unsigned long long cap, unsigned long long *__restrict__ slab,
                                                                unsigned long long *__restrict__ hist_all, int32_t *__restrict__ pools,
                                                                int32_t *__restrict__ n_pools, long long *__restrict__ n_happy,
                                                                long long *__restrict__ total, long long *__restrict__ stats,
                                                                PnbErr *__restrict__ err, PnbSel<V> sel)
{
    __shared__ PnbBandShared<K> sh;
    __shared__ unsigned char s_perm[24];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NP = K == 2 ? 2 : K == 3 ? 6 : 24;
    if (tid < NP) s_perm[tid] = pnb_perm_codes<K>(std::make_integer_sequence<int, NP>{}, tid);
    const size_t rec = (size_t)(2 * K + 1), stride = (size_t)(n / K) * rec;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        PnbBandModel x;
        pnb_stage<K, V>(sh, x, b, n, off, from, to, wait, loss, dist, S, first, sel);
        x.keys = slab + (size_t)blockIdx.x * (size_t)cap;
        x.cap = cap;
        x.hist = hist_all + (size_t)blockIdx.x * PNB_BINS;
        const int nb = x.nb;
        unsigned long long happy = 0;
        long long st_bands = 0, st_passes = 0, st_deep = 0, st_most = 0, sum = 0;
        int kept = 0;
        bool cost_err = false;
        int internal = 0;   // the kind, as PnbErr has it
        unsigned long long bad_got = 0, bad_want = 0;
        int bad_level = 0;
        if (sh.bad) {   // nothing of this model may index the table
            if (tid == 0) atomicMax(&err->bad, batch - b);
        } else if (nb >= K && x.f1 > x.f0) {
            const unsigned long long nn = (unsigned long long)nb;
            const unsigned long long w1 = nn * nn * nn * 24ull;   // the first pick-up's weight in the key
            unsigned long long lo = 0, hi = PNB_END, expect = 0, prefix = 0;
            int level = 0;
            bool count = true, first_pass = true;
            for (;;) {
                // ---- the pass: what it filters by
                x.count = count;
                x.level = level;
                if (!count) x.klo = lo, x.khi = hi;
                else if (level == 0) x.klo = lo, x.khi = PNB_END;
                else {
                    const unsigned long long wl = level == 1 ? w1 : level == 2 ? nn * nn * 24ull : nn * 24ull;
                    x.klo = lo > prefix ? lo : prefix;
                    x.khi = prefix + nn * wl;
                }
                if (count && level == 0) {
                    if (tid < PNB_GROUPS) sh.gsum[tid] = 0ull;
                    if (tid == 0) {
                        sh.tot = 0ull;
                        sh.b0 = PNB_BINS;
                    }
                } else if (count) {
                    for (int i = tid; i < nb; i += PNB_T) sh.hist[i] = 0ull;
                } else if (tid == 0) {
                    sh.happy = 0ull;
                }
                // inside one cost the interval bounds the first pick-up
                int f0 = x.f0, f1 = x.f1;
                if (x.khi != PNB_END && (x.klo >> PN_SEQ_BITS) == ((x.khi - 1ull) >> PN_SEQ_BITS)) {
                    // in 64 bits: a band that ends at a cost's edge has khi - 1 = the largest sequence number, far above nb w1
                    const unsigned long long q0 = (x.klo & PN_SEQ_MASK) / w1, q1 = ((x.khi - 1ull) & PN_SEQ_MASK) / w1 + 1ull;
                    f0 = (int)max((unsigned long long)f0, min(q0, nn));
                    f1 = (int)min((unsigned long long)f1, q1);
                }
                __syncthreads();
                if (f1 > f0) pnb_pairs<K>(sh, x, f0, f1);
                __threadfence();   // the histogram's atomics have arrived
                __syncthreads();
                st_passes++;
                if (!count) {
                    // ---- the band's keys: select, then the next band
                    if (sh.happy != expect) {
                        internal = 1, bad_got = sh.happy, bad_want = expect, bad_level = level;
                        break;
                    }
                    st_most = max(st_most, (long long)expect);
                    pnb_select<K>(sh, x, s_perm, (int)expect, pools + (size_t)b * stride, kept, sum);
                    st_bands++;
                    if (hi == PNB_END) break;   // nothing lies above: no further count
                    lo = hi;
                    level = 0, prefix = 0, count = true;
                    continue;
                }
                if (level == 0) {
                    // every wave reads its quarter of the counters, 64 consecutive ones a step; what is not zero is remembered
                    unsigned long long mysum = 0, nz = 0;
                    int myb0 = PNB_BINS;
                    const int base = w * (PNB_BINS / PNB_W) + lane;
                    for (int s = 0; s < PNB_BINS / PNB_T; s++) {
                        const int bin = base + s * 64;
                        const unsigned long long v = pnb_ld(x.hist + bin);
                        if (v) {
                            mysum += v;
                            nz |= 1ull << s;
                            myb0 = min(myb0, bin);
                            atomicAdd(&sh.gsum[bin >> 6], v);
                        }
                    }
                    if (mysum) {
                        atomicAdd(&sh.tot, mysum);
                        atomicMin(&sh.b0, myb0);
                    }
                    __syncthreads();
                    const unsigned long long tot = sh.tot;
                    const bool stop = tot == 0 || kept >= nb / K;
                    if (tid == 0 && !stop) pnb_choose_cost(sh, x.hist, cap);
                    __syncthreads();
                    // the counters are zero again before the next count
                    for (int s = 0; s < PNB_BINS / PNB_T; s++)
                        if ((nz >> s) & 1ull) __hip_atomic_store(x.hist + base + s * 64, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __threadfence();
                    if (first_pass) {
                        happy = tot;
                        first_pass = false;
                        if (sh.err) {
                            cost_err = true;
                            break;
                        }
                    }
                    if (stop) break;
                } else {
                    const unsigned long long wl = level == 1 ? w1 : level == 2 ? nn * nn * 24ull : nn * 24ull;
                    if (tid == 0) pnb_choose_pick<K>(sh, nb, level, prefix, wl, cap);
                    __syncthreads();
                }
                // ---- the choice
                const int act = sh.act;
                if (act == 2) {
                    internal = sh.expect ? 3 : 2, bad_got = sh.expect, bad_want = cap, bad_level = level;
                    break;
                }
                if (act == 1) {
                    prefix = sh.prefix;
                    level++;
                } else {
                    hi = sh.hi;
                    expect = sh.expect;
                    st_deep = max(st_deep, (long long)level);
                    count = false;
                }
            }
        }
        if (tid == 0) {
            if (cost_err) atomicOr(&err->cost, 1);
            if (internal && atomicMax(&err->internal, batch - b) < batch - b) {   // the report of the first such model stays
                err->kind = internal, err->level = bad_level;
                err->got = bad_got, err->want = bad_want;
            }
            n_pools[b] = kept;
            n_happy[b] = (long long)happy;
            total[b] = sum;
            if (stats) {
                long long *st = stats + 4 * (size_t)b;
                st[0] = st_bands, st[1] = st_passes, st[2] = st_deep, st[3] = st_most;
            }
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

Buf g_slab, g_stage, g_err, g_hist;
std::vector<int32_t> g_h;

// workgroups in flight with `keys` keys of plan storage each: fewer workgroups rather than a slab above 1 GiB
int pnb_grid_cap(int64_t keys)
{
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)PNB_GRID, PNB_SLAB_BYTES / (sizeof(unsigned long long) * (size_t)keys)));
}

// the banded kernel over device arrays: slab and cost counters for the workgroups in flight, one launch, the error words read
// back.  The counters are zeroed when they are allocated; the kernel leaves them zero.
template <bool V>
int pnb_banded_launch(const char *fn, int k, int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to, const int32_t *wait,
                      const int32_t *loss, const int32_t *dist, int S, const int32_t *first, int64_t plan_buffer, int32_t *pools,
                      int32_t *n_pools, long long *n_happy, long long *total, long long *stats, PnbSel<V> sel)
{
    Ctx &c = ctx();
    int rc;
    const int grid_cap = pnb_grid_cap(plan_buffer);
    if ((rc = ensure(g_slab, sizeof(unsigned long long) * (size_t)plan_buffer * (size_t)grid_cap))) return rc;
    const size_t hist_bytes = sizeof(unsigned long long) * PNB_BINS * (size_t)grid_cap;
    if (!g_hist.p || g_hist.cap < hist_bytes) {
        if ((rc = ensure(g_hist, hist_bytes))) return rc;
        TD_HIP(hipMemsetAsync(g_hist.p, 0, g_hist.cap, c.stream));
    }
    if ((rc = ensure(g_err, 256))) return rc;
    PnbErr *d_err = (PnbErr *)g_err.p;
    TD_HIP(hipMemsetAsync(d_err, 0, sizeof(PnbErr), c.stream));
    const int grid = std::min(batch, grid_cap);
    {
        ProfScope ps(TD_K_LCM);
#define TD_PNBB(KV)                                                                                                                    \
    k_pooln_banded_batched<KV, V><<<grid, PNB_T, 0, c.stream>>>(batch, n, off, from, to, wait, loss, dist, S, first,                  \
                                                                 (unsigned long long)plan_buffer, (unsigned long long *)g_slab.p,     \
                                                                 (unsigned long long *)g_hist.p, pools, n_pools, n_happy, total, stats, \
                                                                 d_err, sel)
        if (k == 2) TD_PNBB(2);
        else if (k == 3) TD_PNBB(3);
        else TD_PNBB(4);
#undef TD_PNBB
        TD_HIP(hipGetLastError());
    }
    TD_HIP(hipMemcpyAsync(c.pinned, d_err, sizeof(PnbErr), hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    const PnbErr e = *(const PnbErr *)c.pinned;
    if (e.bad) return fail(TD_EINVAL, "%s: model %d has a stand outside the %d x %d distance table", fn, batch - e.bad, S, S);
    if (e.cost) return fail(TD_ERANGE, "%s: a plan cost does not fit 14 bits", fn);
    if (e.internal) {
        TD_HIP(hipMemsetAsync(g_hist.p, 0, g_hist.cap, c.stream));
        const char *what[4] = {"?", "keys in a band, not the number its histogram counted:", "plans in an empty histogram under", "plans behind one value of the last digit but one, room"};
        return fail(TD_EINTERNAL, "%s: model %d, cut level %d: %llu %s %llu", fn, batch - e.internal, e.level, e.got, what[e.kind & 3], e.want);
    }
    return TD_OK;
}

}  // namespace

void td::pool_batch_release_workspace()
{
    Buf *bs[] = {&g_slab, &g_stage, &g_err, &g_hist};
    for (Buf *b : bs) buf_free(*b);
}

// td_pool_n_banded_batched's core for the world layer (td_simb_pool_buffer): pool_n_worlds' arguments and records, with
// plan_buffer keys of plan storage per workgroup instead of max_happy; never refused for a model's plan count, n_happy[b] is
// the true one.  plan_buffer >= 24 n is the caller's to keep.  One launch whatever the batch.
int td::pool_n_worlds_banded(int k, int batch, int n, const int32_t *off, const int32_t *cnt, const int32_t *k_hi, const int32_t *k_lo,
                             const int32_t *from, const int32_t *to, const int32_t *wait, const int32_t *loss, const int32_t *dist, int S,
                             int64_t plan_buffer, int32_t *pools, int32_t *n_pools, long long *n_happy, long long *total)
{
    const char *fn = "td_pool_n_banded_batched";
    if (k < 2 || k > 4 || batch < 1 || n < 0 || n > PNB_MAXN || plan_buffer > PNB_MAX_HAPPY || plan_buffer < (int64_t)24 * n || plan_buffer < 1)
        return fail(TD_EINVAL, "%s: bad world call", fn);
    return pnb_banded_launch<true>(fn, k, batch, n, off, from, to, wait, loss, dist, S, nullptr, plan_buffer, pools, n_pools, n_happy, total,
                                   nullptr, PnbSel<true>{cnt, k_hi, k_lo});
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

// td_pool_n_batched and td_pool_n_banded_batched: checks, staging, one launch, the caller's arrays.  banded: `max_happy` is the
// plan buffer (keys per workgroup, at least 24 x the largest model), no model is refused for its plan count, stats may be asked
static int pnb_call(const char *fn, bool banded, int k, int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to,
                    const int32_t *max_wait, const int32_t *max_loss, const int32_t *dist, int S, const int32_t *first, int64_t max_happy,
                    int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *total, int64_t *stats)
{
    TD_REQUIRE_INIT();
    Ctx &c = ctx();
    if (k < 2 || k > 4) return fail(TD_EINVAL, "%s: pool size %d (2..4)", fn, k);
    if (batch < 0) return fail(TD_EINVAL, "%s: batch = %d < 0", fn, batch);
    if (n < 0 || n > PNB_MAXN) return fail(TD_EINVAL, "%s: n = %d outside [0, %d] (larger models: td_pool_n over slices)", fn, n, PNB_MAXN);
    if (dist && S <= 0) return fail(TD_EINVAL, "%s: dist given but S = %d", fn, S);
    if (max_happy > PNB_MAX_HAPPY)
        return fail(TD_EINVAL, "%s: %s = %lld above %lld", fn, banded ? "plan_buffer" : "max_happy", (long long)max_happy, (long long)PNB_MAX_HAPPY);
    if (max_happy <= 0) max_happy = PNB_DEF_HAPPY;
    if (batch == 0) return TD_OK;
    if (!off) return fail(TD_EINVAL, "%s: null offsets", fn);
    if (!n_pools || (n / k > 0 && !pools)) return fail(TD_EINVAL, "%s: null output array", fn);
    int rc;
    if ((rc = host_copy(off, (size_t)batch + 1, g_h))) return rc;
    Ragged rg;
    if ((rc = ragged_check(fail, fn, "off", "model", g_h.data(), batch, &rg, [&](int b, int m) {
            if (banded && (int64_t)24 * m > max_happy)
                return fail(TD_EINVAL, "%s: plan_buffer = %lld below 24 * %d = %lld, the room model %d needs", fn, (long long)max_happy, m, 24ll * m, b);
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
    long long *s_nh, *s_tot, *s_stats;
    auto layout = [&](Carve &cv) {
        for (int q = 0; q < 6; q++) s_in[q] = cv.take<int32_t>(stage[q] ? n_in[q] : 0);
        s_pools = cv.take<int32_t>(B * per);
        s_np = cv.take<int32_t>(B);
        s_nh = cv.take<long long>(B);
        s_tot = cv.take<long long>(B);
        s_stats = cv.take<long long>(banded ? 4 * B : 0);
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
    PnbErr e{};
    if (banded) {
        if ((rc = pnb_banded_launch<false>(fn, k, batch, n, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], (const int32_t *)d_dist, S, d_in[5], max_happy,
                                           s_pools, s_np, s_nh, s_tot, s_stats, PnbSel<false>{})))
            return rc;
    } else {
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
        e = *(const PnbErr *)c.pinned;
    }
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
    if (banded && stats) TD_HIP(hipMemcpyAsync(stats, s_stats, sizeof(int64_t) * 4 * B, hipMemcpyDefault, c.stream));
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

extern "C" int td_pool_n_batched(int k, int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to,
                                 const int32_t *max_wait, const int32_t *max_loss, const int32_t *dist, int S, const int32_t *first,
                                 int64_t max_happy, int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *total)
{
    return pnb_call("td_pool_n_batched", false, k, batch, n, off, from, to, max_wait, max_loss, dist, S, first, max_happy, pools, n_pools, n_happy,
                    total, nullptr);
}

extern "C" int td_pool_n_banded_batched(int k, int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to,
                                        const int32_t *max_wait, const int32_t *max_loss, const int32_t *dist, int S, const int32_t *first,
                                        int64_t plan_buffer, int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *total, int64_t *stats)
{
    return pnb_call("td_pool_n_banded_batched", true, k, batch, n, off, from, to, max_wait, max_loss, dist, S, first, plan_buffer, pools, n_pools,
                    n_happy, total, stats);
}
