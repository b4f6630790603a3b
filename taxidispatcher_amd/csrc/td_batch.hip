// td_batch.hip — many small independent models in one call: optimal assignment (td_assign_batched) and the LCM greedy
// (td_lcm_batched) of B square models of size <= 1024, one workgroup per model; and the same solve and LCM for B ragged
// dispatch models made from cab / request positions (td_build_assign_batched, td_tick_batched: cells through PosCells, no
// cost matrix); and split.py's whole heuristic for B ragged cases (td_split_batched: partition into stand ranges, the region
// models, the left-overs' fifth model, the sums); and a dispatch call with a policy per model (td_dispatch_batched: the tick,
// the optimum alone, the LCM alone or the split heuristic on thresholded cells, chosen per model).  gfx950 only.
//
// Nothing here waits on another workgroup: a model's whole solve lives in one workgroup's LDS and registers (no
// cross-workgroup atomics, no spins), and a grid-stride loop over the models covers batches larger than the grid.
//
// Optimal assignment (Jonker-Volgenant shape, exact int64 arithmetic):
//   1. column reduction v[j] = min_i c[i][j]; the first minimum row of each column is a tight edge, and the lowest such
//      column of a row is matched to it (an LDS atomicMin per column); then every row still free takes its lowest free
//      column of zero reduced cost (one reduction per free row: what makes heavily tied models cheap);
//   2. one Dijkstra shortest augmenting path per free row over the reduced costs c[i][j] - v[j] - u[i] (u[i] of a matched
//      row is implicit: c[i][x[i]] - v[x[i]]).  A lane keeps the labels of its own columns (j = lane + k*T) in registers;
//      each step takes the lexicographic (label, column) minimum of the unvisited columns, packed into one 64-bit key, by
//      a wave shuffle reduction (plus one LDS exchange between the waves of a 256-thread workgroup);
//   3. potentials of the visited columns move by label - mu, the path is flipped;
//   4. total = sum c[i][x[i]] and dual_bound = sum_i min_j (c[i][j] - v[j]) + sum_j v[j], both recomputed from the cells,
//      so dual_bound is a valid lower bound whatever the search did and dual_bound == total certifies the optimum.
// n <= 124 stages the model's cells in LDS (<= 64 KiB per workgroup); larger models read their rows through L2.
//
// LCM: td_lcm's rules per model (csrc/td_lcm.hip, k_lcm_loop): a per-row cache of the row's first minimum among the live
// columns (key = biased value << 32 | column); a pick is the (value, row) minimum of the caches, i.e. the first minimum in
// row-major order; only the rows whose cached column was just taken are scanned again.
#include <limits.h>

#include <vector>

#include "td_stage.h"

using namespace td;

namespace {

constexpr int BATCH_NMAX = 1024;
constexpr uint64_t KEY_INF = ~0ull;
constexpr int COL_BITS = 11;                             // column index of a packed Dijkstra key (n <= 1024 < 2^11)
constexpr int64_t LABEL_LIM = (int64_t)1 << 52;          // labels at or above this cannot be packed
constexpr size_t STAGE_LDS_MAX = 64 * 1024 - 1024;       // dynamic LDS a staged model may take
enum { ERR_STEPS = 1, ERR_AUGMENT = 2, ERR_LABEL = 4, ERR_SIZE = 8 };

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = __shfl_xor(k, o);
        k = t < k ? t : k;
    }
    return k;
}

__device__ __forceinline__ int64_t wave_min_i64(int64_t k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = __shfl_xor(k, o);
        k = t < k ? t : k;
    }
    return k;
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t s)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// minimum of `k` over the workgroup; NW > 1 exchanges through s_red[2][NW] (alternating halves, one barrier per call)
template <int NW>
__device__ __forceinline__ uint64_t block_min_u64(uint64_t k, uint64_t *s_red, int &par)
{
    k = wave_min_u64(k);
    if constexpr (NW == 1) {
        return k;
    } else {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (lane == 0) s_red[par * NW + w] = k;
        __syncthreads();
        uint64_t r = s_red[par * NW];
#pragma unroll
        for (int q = 1; q < NW; q++) {
            const uint64_t t = s_red[par * NW + q];
            r = t < r ? t : r;
        }
        par ^= 1;
        return r;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// cell sources: the solve and the LCM read a model's cells row by row through `C.row(i)(j)`
// ---------------------------------------------------------------------------------------------------------------------
// a slab model: its rows at `base` with stride n (global) or nb (STAGE: the LDS copy)
template <bool STAGE>
struct SlabCells {
    const int32_t *base;
    int nb, n;
    struct Row {
        const int32_t *p;
        __device__ __forceinline__ int32_t operator()(int j) const { return p[j]; }
    };
    __device__ __forceinline__ Row row(int i) const { return Row{STAGE ? base + i * nb : base + (int64_t)i * n}; }
};

// a model made from positions (td_cost_build's positional rule, k_cost_build / CellSrc): cell (i, j) is the distance
// dist[cab[i]][dem[j]] (|cab[i] - dem[j]| without a table) when threshold < 0 or it is below the threshold, else fill;
// a row i >= ns, a column j >= nd or a stand outside [0, S) of a table is fill.  cab / dem are LDS copies; the table is
// an LDS copy (LDS_DIST), a global array, or null.
template <bool LDS_DIST>
struct PosCells {
    const int32_t *cab, *dem, *dist;
    int ns, nd, S;
    int32_t fill, thr;
    struct Row {
        const int32_t *drow, *dem;
        int a, nd, S;
        int32_t fill, thr;
        bool ok;
        __device__ __forceinline__ int32_t operator()(int j) const
        {
            if (!ok || j >= nd) return fill;
            const int b = dem[j];
            int x;
            if (drow) {
                if ((uint32_t)b >= (uint32_t)S) return fill;   // never index outside the table
                x = drow[b];
            } else {
                x = a > b ? a - b : b - a;
            }
            return (thr < 0 || x < thr) ? x : fill;
        }
    };
    __device__ __forceinline__ Row row(int i) const
    {
        const int a = i < ns ? cab[i] : 0;
        const bool ok = i < ns && (!dist || (uint32_t)a < (uint32_t)S);
        const int32_t *drow = dist && ok ? (LDS_DIST ? dist + a * S : dist + (int64_t)a * S) : nullptr;
        return Row{drow, dem, a, nd, S, fill, thr, ok};
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// optimal assignment of one nb x nb model by one workgroup of T threads, CPT columns per thread (nb <= T * CPT).
// s_x / s_y / s_pred / s_v: LDS arrays of at least nb entries.  Outputs: row b of r2c / price (stride n_out, -1 / 0 beyond
// nb), total[b], dual[b].  The caller has put the model's cells in place before the call; they are read after its first
// barrier.
// ---------------------------------------------------------------------------------------------------------------------
template <int T, int CPT, class Cells>
__device__ __forceinline__ void assign_model(const Cells &C, int nb, int b, int n_out, int64_t *s_v, int32_t *s_pred, int32_t *s_y,
                                             int32_t *s_x, uint64_t *s_red, int64_t *s_sum, int &par, int32_t *__restrict__ r2c,
                                             int64_t *__restrict__ total, int64_t *__restrict__ dual, int64_t *__restrict__ price,
                                             int *__restrict__ err)
{
    constexpr int NW = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < nb; i += T) {
        s_x[i] = INT_MAX;
        s_y[i] = -1;
    }
    __syncthreads();
    // 1. column reduction; each column's first minimum row is tight: the row takes the lowest such column
    int64_t vr[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) {
        const int j = tid + k * T;
        vr[k] = 0;
        if (j < nb) {
            int32_t m = C.row(0)(j);
            int r = 0;
            for (int i = 1; i < nb; i++) {
                const int32_t cv = C.row(i)(j);
                if (cv < m) {
                    m = cv;
                    r = i;
                }
            }
            vr[k] = m;
            s_v[j] = m;
            atomicMin(&s_x[r], j);
        }
    }
    __syncthreads();
    for (int i = tid; i < nb; i += T) {
        const int j = s_x[i];
        if (j == INT_MAX)
            s_x[i] = -1;
        else
            s_y[j] = i;
    }
    __syncthreads();
    // a free row takes its lowest free column of zero reduced cost (its u = 0 stays tight).  With heavy ties
    // (U{1..39}) the claims above leave most rows free, all first minima sitting in the top rows; this pass
    // matches nearly all of them, one row read and one reduction per free row, instead of a search each.
    for (int f = 0; f < nb; f++) {
        if (s_x[f] >= 0) continue;   // uniform: x changes only between barriers
        const auto rf = C.row(f);
        uint64_t key = KEY_INF;
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const int j = tid + k * T;
            if (j < nb && s_y[j] < 0 && (int64_t)rf(j) == vr[k]) key = key < (uint64_t)j ? key : (uint64_t)j;
        }
        key = block_min_u64<NW>(key, s_red, par);
        if (key != KEY_INF) {
            if (tid == 0) {
                s_x[f] = (int)key;
                s_y[key] = f;
            }
            __syncthreads();
        }
    }
    // 2./3. one shortest augmenting path per free row
    int bad = 0;
    for (int f = 0; f < nb && !bad; f++) {
        if (s_x[f] >= 0) continue;   // uniform: x changes only between barriers
        int64_t d[CPT];
        uint32_t vis = 0;   // bit k: column tid + k*T is visited (or does not exist)
        const auto rf = C.row(f);
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const int j = tid + k * T;
            d[k] = 0;
            if (j < nb) {
                d[k] = (int64_t)rf(j) - vr[k];
                s_pred[j] = f;
            } else {
                vis |= 1u << k;
            }
        }
        int jstar = -1, steps = 0;
        int64_t mu = 0;
        for (;;) {
            uint64_t key = KEY_INF;
#pragma unroll
            for (int k = 0; k < CPT; k++) {
                if (!((vis >> k) & 1u)) {
                    const int64_t dd = d[k] < LABEL_LIM ? d[k] : LABEL_LIM - 1;
                    const uint64_t kk = ((uint64_t)dd << COL_BITS) | (uint64_t)(tid + k * T);
                    key = kk < key ? kk : key;
                }
            }
            key = block_min_u64<NW>(key, s_red, par);
            if (key == KEY_INF || ++steps > nb) {   // a free column is always reachable within nb steps
                bad = ERR_STEPS;
                break;
            }
            mu = (int64_t)(key >> COL_BITS);
            jstar = (int)(key & ((1u << COL_BITS) - 1));
            if (mu >= LABEL_LIM - 1) {
                bad = ERR_LABEL;
                break;
            }
            if ((jstar & (T - 1)) == tid) vis |= 1u << (jstar / T);
            const int i = s_y[jstar];
            if (i < 0) break;   // a free column: augment
            const auto ri_row = C.row(i);
            const int64_t ri = (int64_t)ri_row(jstar) - s_v[jstar];
#pragma unroll
            for (int k = 0; k < CPT; k++) {
                if (!((vis >> k) & 1u)) {
                    const int j = tid + k * T;
                    const int64_t nd = mu + ((int64_t)ri_row(j) - vr[k] - ri);
                    if (nd < d[k]) {
                        d[k] = nd;
                        s_pred[j] = i;
                    }
                }
            }
        }
        if (bad) break;
        // potentials of the visited columns (the last one, label mu, does not move)
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const int j = tid + k * T;
            if (((vis >> k) & 1u) && j < nb) {
                vr[k] += d[k] - mu;
                s_v[j] = vr[k];
            }
        }
        __syncthreads();   // pred of every column written
        if (tid == 0) {
            int j = jstar;
            for (int g = 0;; g++) {
                if (g > nb) {
                    *err = ERR_AUGMENT;
                    break;
                }
                const int i = s_pred[j];
                s_y[j] = i;
                const int nxt = s_x[i];
                s_x[i] = j;
                if (i == f) break;
                j = nxt;
            }
        }
        __syncthreads();
    }
    if (bad && tid == 0) *err = bad;   // any non-zero word fails the call: a plain store suffices
    // 4. total and dual bound from the cells
    int64_t tsum = 0, vsum = 0, rsum = 0;
    for (int i = tid; i < nb; i += T) {
        const int j = s_x[i];
        tsum += j >= 0 ? (int64_t)C.row(i)(j) : 0;
    }
    if (dual) {
#pragma unroll
        for (int k = 0; k < CPT; k++)
            if (tid + k * T < nb) vsum += vr[k];
        for (int i = w; i < nb; i += NW) {
            const auto ri = C.row(i);
            int64_t m = INT64_MAX;
            for (int j = lane; j < nb; j += 64) {
                const int64_t r = (int64_t)ri(j) - s_v[j];
                m = r < m ? r : m;
            }
            m = wave_min_i64(m);
            if (lane == 0) rsum += m;
        }
    }
    tsum = wave_sum_i64(tsum);
    vsum = wave_sum_i64(vsum);
    if (lane == 0) {
        s_sum[w] = tsum;
        s_sum[NW + w] = vsum + rsum;
    }
    for (int i = tid; i < n_out; i += T) {
        r2c[(int64_t)b * n_out + i] = i < nb ? s_x[i] : -1;
        if (price) price[(int64_t)b * n_out + i] = i < nb ? s_v[i] : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int64_t t = 0, dsum = 0;
        for (int q = 0; q < NW; q++) {
            t += s_sum[q];
            dsum += s_sum[NW + q];
        }
        total[b] = t;
        if (dual) dual[b] = dsum;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// optimal assignment of slab models: T threads (64 or 256), CPT columns per thread (n <= T * CPT), STAGE: cells in LDS
// dynamic LDS: v int64[n] | pred int32[n] | y (column -> row) int32[n] | x (row -> column) int32[n] | cells int32[n*n]
// ---------------------------------------------------------------------------------------------------------------------
template <int T, int CPT, bool STAGE>
__global__ __launch_bounds__(T) void k_assign_batched(int batch, int n, const int32_t *__restrict__ ns,
                                                      const int32_t *__restrict__ cost, int32_t *__restrict__ r2c,
                                                      int64_t *__restrict__ total, int64_t *__restrict__ dual,
                                                      int64_t *__restrict__ price, int *__restrict__ err)
{
    constexpr int NW = T / 64;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    int64_t *s_v = reinterpret_cast<int64_t *>(s_dyn);
    int32_t *s_pred = reinterpret_cast<int32_t *>(s_v + n);
    int32_t *s_y = s_pred + n;
    int32_t *s_x = s_y + n;
    int32_t *s_c = s_x + n;
    __shared__ uint64_t s_red[2 * NW];
    __shared__ int64_t s_sum[2 * NW];
    const int tid = threadIdx.x;
    int par = 0;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int nb = ns ? ns[b] : n;
        const int32_t *base = cost + (int64_t)b * n * n;
        __syncthreads();   // the previous model's LDS is no longer read
        if constexpr (STAGE) {
            for (int i = 0; i < nb; i++)
                for (int j = tid; j < nb; j += T) s_c[i * nb + j] = base[(int64_t)i * n + j];
        }
        const SlabCells<STAGE> C{STAGE ? s_c : base, nb, n};
        assign_model<T, CPT>(C, nb, b, n, s_v, s_pred, s_y, s_x, s_red, s_sum, par, r2c, total, dual, price, err);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// optimal assignment of position models (td_build_assign_batched, td_tick_batched's remainder): model b's cabs are
// cab[cab_off[b] ...], its requests dem[dem_off[b] ...]; the counts are cab_off[b + 1] - cab_off[b] (cnt == null) or
// cnt[2b] / cnt[2b + 1] (the tick's kept lists, 0 / 0 = no solve; -1 / -1: model b is not this launch's, nothing of it is
// written).  nl >= every max(count) bounds the LDS arrays.
// dynamic LDS: v int64[nl] | pred, y, x int32[nl] | cab, dem int32[nl] | table int32[S*S] (LDS_DIST)
// ---------------------------------------------------------------------------------------------------------------------
template <int T, int CPT, bool LDS_DIST>
__global__ __launch_bounds__(T) void k_assign_pos_batched(int batch, int n_out, int nl, const int32_t *__restrict__ cab_off,
                                                          const int32_t *__restrict__ cab, const int32_t *__restrict__ dem_off,
                                                          const int32_t *__restrict__ dem, const int32_t *__restrict__ cnt,
                                                          const int32_t *__restrict__ dist, int S, int32_t fill, int32_t thr,
                                                          int32_t *__restrict__ r2c, int64_t *__restrict__ total,
                                                          int64_t *__restrict__ dual, int *__restrict__ err)
{
    constexpr int NW = T / 64;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    int64_t *s_v = reinterpret_cast<int64_t *>(s_dyn);
    int32_t *s_pred = reinterpret_cast<int32_t *>(s_v + nl);
    int32_t *s_y = s_pred + nl;
    int32_t *s_x = s_y + nl;
    int32_t *s_cab = s_x + nl;
    int32_t *s_dem = s_cab + nl;
    int32_t *s_dist = s_dem + nl;
    __shared__ uint64_t s_red[2 * NW];
    __shared__ int64_t s_sum[2 * NW];
    const int tid = threadIdx.x;
    int par = 0;
    if constexpr (LDS_DIST)
        for (int q = tid; q < S * S; q += T) s_dist[q] = dist[q];   // read after the first model's barrier
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int c0 = cab_off[b], d0 = dem_off[b];
        const int ns = cnt ? cnt[2 * b] : cab_off[b + 1] - c0;
        const int nd = cnt ? cnt[2 * b + 1] : dem_off[b + 1] - d0;
        if (ns < 0 || nd < 0) continue;   // uniform: both counts are -1 for td_dispatch_batched's split models and in a refused call
        const int nb = ns > nd ? ns : nd;
        if (nb > nl) {   // validated on the host; never index LDS past nl
            if (tid == 0) *err = ERR_SIZE;
            continue;
        }
        __syncthreads();   // the previous model's LDS is no longer read
        for (int i = tid; i < ns; i += T) s_cab[i] = cab[c0 + i];
        for (int j = tid; j < nd; j += T) s_dem[j] = dem[d0 + j];
        const PosCells<LDS_DIST> C{s_cab, s_dem, LDS_DIST ? s_dist : dist, ns, nd, S, fill, thr};
        assign_model<T, CPT>(C, nb, b, n_out, s_v, s_pred, s_y, s_x, s_red, s_sum, par, r2c, total, dual, nullptr, err);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// LCM of one model by one workgroup: rows [0, nr) and columns [0, nc) are scanned, `size` counts down from nsize (the
// model's n).  Every cell outside nr x nc must be one that is never a candidate (>= cand_limit): true of a slab (nr = nc =
// nsize) and of the tick's padded rows and columns (fill, cand_limit = fill).  s_rb uint64[nr], s_list int32[nr],
// s_cm uint32[(nc + 31) / 32]; s_rm (may be null) uint32[(nr + 31) / 32] gets the taken rows.  Pairs go to rows / cols.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lcm_bias(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int32_t lcm_unbias(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }

// SYM: a pick (r, c) retires row and column r AND row and column c (td_pool2's symmetric masking: both customers of a pool
// leave the game in both roles); the slab callers use SYM = false.
template <int T, bool SYM = false, class Cells>
__device__ __forceinline__ void lcm_model(const Cells &C, int nr, int nc, int nsize, int64_t cand_limit, int32_t mask,
                                          int32_t threshold, int stop_value_on, int32_t stop_value, int stop_size, int64_t sum_below,
                                          uint64_t *s_rb, int32_t *s_list, uint32_t *s_cm, uint32_t *s_rm, uint64_t *s_red, int *s_cnt,
                                          int &par, int32_t *__restrict__ rows, int32_t *__restrict__ cols, int &np_out,
                                          int32_t &lm_out, int64_t &tot_out)
{
    constexpr int NW = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int q = tid; q < (nc + 31) / 32; q += T) s_cm[q] = 0u;
    if (s_rm)
        for (int q = tid; q < (nr + 31) / 32; q += T) s_rm[q] = 0u;
    for (int i = tid; i < nr; i += T) s_list[i] = i;
    if (tid == 0) *s_cnt = nr;
    __syncthreads();
    int np = 0, size = nsize;
    int32_t lm = stop_value;
    int64_t tot = 0;
    for (int it = 0; it <= nsize; it++) {
        // rows in the list: first minimum among the live columns below cand_limit (one wave per row)
        const int cnt = *s_cnt;
        for (int q = w; q < cnt; q += NW) {
            const int r = s_list[q];
            const auto rr = C.row(r);
            uint64_t key = KEY_INF;
            for (int j = lane; j < nc; j += 64) {
                if (!((s_cm[j >> 5] >> (j & 31)) & 1u)) {
                    const int32_t v = rr(j);
                    if ((int64_t)v < cand_limit) {
                        const uint64_t kk = ((uint64_t)lcm_bias(v) << 32) | (uint32_t)j;
                        key = kk < key ? kk : key;
                    }
                }
            }
            key = wave_min_u64(key);
            if (lane == 0) s_rb[r] = key;
        }
        __syncthreads();
        if (it == nsize) break;   // every row taken
        // the pick: (value, row) minimum of the row caches
        uint64_t key = KEY_INF;
        for (int i = tid; i < nr; i += T) {
            const uint64_t k = s_rb[i];
            if (k != KEY_INF) {
                const uint64_t kk = (k & 0xFFFFFFFF00000000ull) | (uint32_t)i;
                key = kk < key ? kk : key;
            }
        }
        key = block_min_u64<NW>(key, s_red, par);
        if (key == KEY_INF) {   // nothing left to look at
            lm = stop_value_on ? stop_value : mask;
            break;
        }
        const int r = (int)(uint32_t)key;
        const int32_t v = lcm_unbias(key);
        const int c = (int)(uint32_t)s_rb[r];
        lm = v;
        if (threshold >= 0 && v > threshold) break;   // greedy_opt.py:68-69
        if (stop_value_on && v >= stop_value) break;   // Simulator.java:538
        if (v >= mask) break;                          // only masked-valued cells remain
        if (tid == 0) {
            rows[np] = r;
            cols[np] = c;
        }
        np++;
        if ((int64_t)v < sum_below) tot += v;
        size--;
        __syncthreads();   // everyone has read s_rb[r]
        if (tid == 0) {
            s_rb[r] = KEY_INF;
            s_cm[c >> 5] |= 1u << (c & 31);
            if (s_rm) s_rm[r >> 5] |= 1u << (r & 31);
            if constexpr (SYM) {
                s_rb[c] = KEY_INF;
                s_cm[r >> 5] |= 1u << (r & 31);
                if (s_rm) s_rm[c >> 5] |= 1u << (c & 31);
            }
            *s_cnt = 0;
        }
        __syncthreads();
        if (stop_size >= 0 && size == stop_size) break;   // Simulator.java:544-545
        for (int i = tid; i < nr; i += T) {
            const uint64_t k = s_rb[i];
            if (k != KEY_INF && ((int)(uint32_t)k == c || (SYM && (int)(uint32_t)k == r))) s_list[atomicAdd(s_cnt, 1)] = i;
        }
        __syncthreads();
    }
    np_out = np;
    lm_out = lm;
    tot_out = tot;
}

// ---------------------------------------------------------------------------------------------------------------------
// LCM of slab models: dynamic LDS: row cache uint64[n] | rescan list int32[n] | column mask uint32[(n + 31) / 32]
// ---------------------------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_lcm_batched(int batch, int n, const int32_t *__restrict__ ns, const int32_t *__restrict__ cost,
                                                   int64_t cand_limit, int32_t mask, int32_t threshold, int stop_value_on,
                                                   int32_t stop_value, int stop_size, int64_t sum_below, int32_t *__restrict__ rows,
                                                   int32_t *__restrict__ cols, int32_t *__restrict__ n_pairs,
                                                   int64_t *__restrict__ total, int32_t *__restrict__ last_min)
{
    constexpr int NW = T / 64;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    uint64_t *s_rb = reinterpret_cast<uint64_t *>(s_dyn);
    int32_t *s_list = reinterpret_cast<int32_t *>(s_rb + n);
    uint32_t *s_cm = reinterpret_cast<uint32_t *>(s_list + n);
    __shared__ uint64_t s_red[2 * NW];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    int par = 0;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int nb = ns ? ns[b] : n;
        __syncthreads();
        const SlabCells<false> C{cost + (int64_t)b * n * n, nb, n};
        int np;
        int32_t lm;
        int64_t tot;
        lcm_model<T>(C, nb, nb, nb, cand_limit, mask, threshold, stop_value_on, stop_value, stop_size, sum_below, s_rb, s_list, s_cm,
                     nullptr, s_red, &s_cnt, par, rows + (int64_t)b * n, cols + (int64_t)b * n, np, lm, tot);
        if (tid == 0) {
            n_pairs[b] = np;
            total[b] = tot;
            last_min[b] = lm;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// td_pool2_batched's greedy (pool_opt_min.py:81-102 = Simulator.java:723-739): the LCM with symmetric masking over each
// model's pair-cost block (slab stride n; INT_MAX = not a candidate).  Pairs go to rows / cols at b * (n / 2) in pick
// order, which is the reference's keep order (stable sort by cost, A-major insertion order).
// dynamic LDS: as k_lcm_batched
// ---------------------------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_pool2_lcm_batched(int batch, int n, const int32_t *__restrict__ ns, const int32_t *__restrict__ cost,
                                                         int32_t *__restrict__ rows, int32_t *__restrict__ cols, int32_t *__restrict__ n_pairs)
{
    constexpr int NW = T / 64;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    uint64_t *s_rb = reinterpret_cast<uint64_t *>(s_dyn);
    int32_t *s_list = reinterpret_cast<int32_t *>(s_rb + n);
    uint32_t *s_cm = reinterpret_cast<uint32_t *>(s_list + n);
    __shared__ uint64_t s_red[2 * NW];
    __shared__ int s_cnt;
    int par = 0;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int nb = ns[b];
        __syncthreads();
        const SlabCells<false> C{cost + (int64_t)b * n * n, nb, n};
        int np;
        int32_t lm;
        int64_t tot;
        lcm_model<T, true>(C, nb, nb, nb, (int64_t)INT_MAX, INT_MAX, -1, 0, 0, -1, (int64_t)INT64_MAX, s_rb, s_list, s_cm, nullptr, s_red,
                           &s_cnt, par, rows + (int64_t)b * (n / 2), cols + (int64_t)b * (n / 2), np, lm, tot);
        if (threadIdx.x == 0) n_pairs[b] = np;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// td_tick_batched, first launch: per model the tick's LCM (Simulator.java:523-549: cells >= fill are never candidates,
// stop on fill or when stop_size rows are left; skipped when stop_size < 0 or >= n(b)) over the real n_s x n_d cells,
// then the shrink: the cabs / requests in no pair, in order (k_tick_shrink's ordered compaction, per model).  Their
// indices go to kept_c / kept_d (may be null), their positions to cab2 / dem2 at the model's own offsets, their counts to
// cnt[2b] / cnt[2b + 1] for the solve (0 / 0 when the LCM ended on fill: no solve, Simulator.java:188-189).
// td_dispatch_batched hands in a policy per model (mode non-null; stop_arr non-null: model b's own stop size): TD_DISPATCH_OPT
// is stop size -1, TD_DISPATCH_LCM is stop size 0 and never a solve (0 / 0), a TD_DISPATCH_SPLIT model is not this launch's
// (counts -1 / -1, nothing else written); and gate (non-null): a non-zero word = the split launches before this one refused
// the input, every model gets -1 / -1 and no output is written.  All of that is the POLICY instantiation; td_tick_batched's
// (POLICY = false) reads none of the three and is the kernel it was.
// dynamic LDS (nl = the largest n(b)): row cache uint64[nl] | rescan list, cab, dem int32[nl] | column mask, row mask
// uint32[(nl + 31) / 32] each | table int32[S*S] (LDS_DIST)
// ---------------------------------------------------------------------------------------------------------------------
template <int T, bool LDS_DIST, bool POLICY>
__global__ __launch_bounds__(T) void k_tick_lcm_batched(int batch, int n_out, int nl, const int32_t *__restrict__ cab_off,
                                                        const int32_t *__restrict__ cab, const int32_t *__restrict__ dem_off,
                                                        const int32_t *__restrict__ dem, const int32_t *__restrict__ dist, int S,
                                                        int32_t fill, int32_t thr, int stop_size, const int32_t *__restrict__ mode,
                                                        const int32_t *__restrict__ stop_arr, const int *__restrict__ gate,
                                                        int32_t *__restrict__ rows, int32_t *__restrict__ cols,
                                                        int32_t *__restrict__ n_pairs,
                                                        int32_t *__restrict__ last_min, int32_t *__restrict__ kept_c,
                                                        int32_t *__restrict__ kept_d, int32_t *__restrict__ n_rest,
                                                        int32_t *__restrict__ cab2, int32_t *__restrict__ dem2, int32_t *__restrict__ cnt)
{
    constexpr int NW = T / 64;
    const int WL = (nl + 31) / 32;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    uint64_t *s_rb = reinterpret_cast<uint64_t *>(s_dyn);
    int32_t *s_list = reinterpret_cast<int32_t *>(s_rb + nl);
    int32_t *s_cab = s_list + nl;
    int32_t *s_dem = s_cab + nl;
    uint32_t *s_cm = reinterpret_cast<uint32_t *>(s_dem + nl);
    uint32_t *s_rm = s_cm + WL;
    int32_t *s_dist = reinterpret_cast<int32_t *>(s_rm + WL);
    __shared__ uint64_t s_red[2 * NW];
    __shared__ int s_cnt, s_kept[2];
    __shared__ int s_w[NW];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int par = 0;
    if (POLICY && gate) {   // nothing in this launch writes the word: one read per workgroup
        if (tid == 0) s_cnt = *gate;
        __syncthreads();
        const int refused = s_cnt;
        __syncthreads();
        if (refused) {
            if (tid == 0)
                for (int q = blockIdx.x; q < batch; q += gridDim.x) cnt[2 * q] = cnt[2 * q + 1] = -1;
            return;
        }
    }
    if constexpr (LDS_DIST)
        for (int q = tid; q < S * S; q += T) s_dist[q] = dist[q];   // read after the first model's barrier
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int md = POLICY && mode ? mode[b] : TD_DISPATCH_LCM_OPT;
        if (POLICY && md == TD_DISPATCH_SPLIT) {   // uniform
            if (tid == 0) cnt[2 * b] = cnt[2 * b + 1] = -1;
            continue;
        }
        const int stop_b = !POLICY ? stop_size : md == TD_DISPATCH_OPT ? -1 : md == TD_DISPATCH_LCM ? 0 : stop_arr ? stop_arr[b] : stop_size;
        const int c0 = cab_off[b], d0 = dem_off[b];
        const int ns = cab_off[b + 1] - c0, nd = dem_off[b + 1] - d0, nb = ns > nd ? ns : nd;
        __syncthreads();   // the previous model's LDS is no longer read
        for (int i = tid; i < ns; i += T) s_cab[i] = cab[c0 + i];
        for (int j = tid; j < nd; j += T) s_dem[j] = dem[d0 + j];
        const bool lcm_runs = stop_b >= 0 && stop_b < nb;
        int np = 0;
        int32_t lm = fill;
        if (lcm_runs) {
            const PosCells<LDS_DIST> C{s_cab, s_dem, LDS_DIST ? s_dist : dist, ns, nd, S, fill, thr};
            int64_t tot;
            lcm_model<T>(C, ns, nd, nb, (int64_t)fill, fill, -1, 1, fill, stop_b, (int64_t)fill, s_rb, s_list, s_cm, s_rm, s_red,
                         &s_cnt, par, rows + (int64_t)b * n_out, cols + (int64_t)b * n_out, np, lm, tot);
        } else {
            for (int q = tid; q < WL; q += T) {
                s_cm[q] = 0u;
                s_rm[q] = 0u;
            }
        }
        __syncthreads();   // the masks are final
        // the shrink: per side a contiguous slice per thread, a wave scan of the slice counts, the waves' sums through LDS
        for (int side = 0; side < 2; side++) {
            const int m = side ? nd : ns;
            const uint32_t *bits = side ? s_cm : s_rm;
            const int32_t *pos = side ? s_dem : s_cab;
            int32_t *pos2 = (side ? dem2 + d0 : cab2 + c0);
            int32_t *keep = side ? kept_d : kept_c;
            const int per = (m + T - 1) / T, lo = min(m, tid * per), hi = min(m, lo + per);
            int cnt_t = 0;
            for (int i = lo; i < hi; i++) cnt_t += ((bits[i >> 5] >> (i & 31)) & 1u) ? 0 : 1;
            int incl = cnt_t;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == 63) s_w[w] = incl;
            __syncthreads();
            int base = 0;
            for (int q = 0; q < w; q++) base += s_w[q];
            int at = base + incl - cnt_t;
            for (int i = lo; i < hi; i++)
                if (!((bits[i >> 5] >> (i & 31)) & 1u)) {
                    if (keep) keep[(int64_t)b * n_out + at] = i;
                    pos2[at] = pos[i];
                    at++;
                }
            if (tid == T - 1) s_kept[side] = base + incl;
            __syncthreads();   // s_w is reused by the next side
        }
        if (tid == 0) {
            const int kc = s_kept[0], kd = s_kept[1];
            const bool solve = md != TD_DISPATCH_LCM && !(lcm_runs && lm == fill);   // Simulator.java:188-189
            n_pairs[b] = np;
            last_min[b] = lm;
            n_rest[b] = kc > kd ? kc : kd;
            cnt[2 * b] = solve ? kc : 0;
            cnt[2 * b + 1] = solve ? kd : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
Buf g_out;                    // device results for host destinations + the error word (grow-only)
std::vector<int32_t> g_ns;    // host copy of ns (validated here; stays alive while its upload may still be in flight)

// validates the arguments shared by both entry points; *d_ns = device copy of ns (nullptr: every model is n x n)
int batch_args(const char *fn, int batch, int n, const int32_t *ns, const int32_t *cost, const int32_t **d_ns,
               const int32_t **d_cost)
{
    Ctx &c = ctx();
    if (batch < 0) return fail(TD_EINVAL, "%s: batch = %d < 0", fn, batch);
    if (n < 0) return fail(TD_EINVAL, "%s: n = %d < 0", fn, n);
    if (n > BATCH_NMAX)
        return fail(TD_EINVAL, "%s: n = %d > %d; a model this large is one td_assign call (td_assign / td_lcm solve it over the "
                    "whole GPU)", fn, n, BATCH_NMAX);
    *d_ns = nullptr;
    *d_cost = nullptr;
    if (ns && batch > 0) {
        std::vector<int32_t> &h = g_ns;
        int rc = host_copy(ns, (size_t)batch, h);
        if (rc) return rc;
        for (int b = 0; b < batch; b++)
            if (h[b] < 0 || h[b] > n) return fail(TD_EINVAL, "%s: ns[%d] = %d outside [0, %d]", fn, b, h[b], n);
        const void *p;
        if ((rc = to_device(is_device_ptr(ns) ? (const void *)ns : (const void *)h.data(), sizeof(int32_t) * h.size(), c.stage_a, &p))) return rc;
        *d_ns = (const int32_t *)p;
    }
    if (batch > 0 && n > 0) {
        if (!cost) return fail(TD_EINVAL, "%s: null cost", fn);
        const void *p;
        int rc = to_device(cost, sizeof(int32_t) * (size_t)batch * n * n, c.stage_d, &p);
        if (rc) return rc;
        *d_cost = (const int32_t *)p;
    }
    return TD_OK;
}

// what the solver kernels leave in the error word
int cap_error(const char *fn, int e)
{
    if (e)
        return fail(TD_EINTERNAL, "%s: a model hit a defensive loop cap (error word 0x%x: 1 search steps, 2 augmenting path, "
                    "4 label range, 8 model size)", fn, e);
    return TD_OK;
}

int batch_finish(const char *fn, const Out *o, int k, const int *d_err)
{
    return outputs_finish(o, k, d_err, [fn](int e) { return cap_error(fn, e); });
}

template <int T, int CPT, bool STAGE>
void launch_assign(int batch, int n, const int32_t *d_ns, const int32_t *d_cost, int32_t *r2c, int64_t *tot, int64_t *dual,
                   int64_t *price, int *err, size_t shm)
{
    const int grid = std::min(batch, 1 << 20);
    k_assign_batched<T, CPT, STAGE><<<grid, T, shm, ctx().stream>>>(batch, n, d_ns, d_cost, r2c, tot, dual, price, err);
}

// ---------------------------------------------------------------------------------------------------------------------
// position models (td_build_assign_batched / td_tick_batched)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TICK_NMAX = 2048;                 // largest model of td_tick_batched (Simulator.java's 1300 x 900 tick)
Buf g_in[5];                                    // device copies of host inputs: cab_off, dem_off, cab_to, dem_from, dist
Buf g_ws;                                       // td_tick_batched: kept positions (ragged, at the models' offsets) + counts
std::vector<int32_t> g_off[2];                  // host copies of the offsets (validated here)

struct PosIn {
    const int32_t *cab_off, *dem_off, *cab, *dem, *dist;   // device pointers
    int nmax;                                              // the largest max(n_s, n_d)
};

// validates and uploads the arguments shared by both entry points; model b's n(b) must not exceed n (<= nlim)
int pos_args(const char *fn, int batch, int n, int nlim, const int32_t *cab_off, const int32_t *cab_to, const int32_t *dem_off,
             const int32_t *dem_from, const int32_t *dist, int S, PosIn *in)
{
    *in = PosIn{};
    if (batch < 0) return fail(TD_EINVAL, "%s: batch = %d < 0", fn, batch);
    if (n < 0) return fail(TD_EINVAL, "%s: n = %d < 0", fn, n);
    if (n > nlim)
        return fail(TD_EINVAL, "%s: n = %d > %d; a model this large is one td_build_assign / td_tick call", fn, n, nlim);
    if (dist && (S <= 0 || S > 46340)) return fail(TD_EINVAL, "%s: S = %d outside [1, 46340] with a distance table", fn, S);
    if (batch == 0) return TD_OK;
    if (!cab_off || !dem_off) return fail(TD_EINVAL, "%s: null offsets", fn);
    int rc = host_copy({{cab_off, (size_t)batch + 1, &g_off[0]}, {dem_off, (size_t)batch + 1, &g_off[1]}});
    if (rc) return rc;
    Ragged rg;
    if ((rc = ragged_check(fail, fn, "cab_off", "model", g_off[0].data(), batch, &rg)) ||
        (rc = ragged_check(fail, fn, "dem_off", "model", g_off[1].data(), batch, &rg)))
        return rc;
    int nmax = 0;
    for (int b = 0; b < batch; b++) {
        const int ns = g_off[0][b + 1] - g_off[0][b], nd = g_off[1][b + 1] - g_off[1][b], nb = std::max(ns, nd);
        if (nb > n) return fail(TD_EINVAL, "%s: model %d has %d cabs and %d requests, more than n = %d", fn, b, ns, nd, n);
        nmax = std::max(nmax, nb);
    }
    const size_t nc = (size_t)g_off[0][batch], nd = (size_t)g_off[1][batch];
    if ((nc && !cab_to) || (nd && !dem_from)) return fail(TD_EINVAL, "%s: null position array", fn);
    const void *p;
    const int32_t *srcs[5] = {is_device_ptr(cab_off) ? cab_off : g_off[0].data(), is_device_ptr(dem_off) ? dem_off : g_off[1].data(),
                              cab_to, dem_from, dist};
    const size_t bytes[5] = {sizeof(int32_t) * ((size_t)batch + 1), sizeof(int32_t) * ((size_t)batch + 1), sizeof(int32_t) * nc,
                             sizeof(int32_t) * nd, dist ? sizeof(int32_t) * (size_t)S * S : 0};
    const int32_t **dsts[5] = {&in->cab_off, &in->dem_off, &in->cab, &in->dem, &in->dist};
    for (int k = 0; k < 5; k++) {
        if (!bytes[k]) continue;
        if ((rc = to_device(srcs[k], bytes[k], g_in[k], &p))) return rc;
        *dsts[k] = (const int32_t *)p;
    }
    in->nmax = nmax;
    return TD_OK;
}

// the optimum of every position model: nl >= every model's max(count); cnt: see k_assign_pos_batched
template <int T, int CPT>
void launch_pos_assign_t(int batch, int n_out, int nl, const PosIn &in, const int32_t *cab, const int32_t *dem, const int32_t *cnt, int S,
                         int32_t fill, int32_t thr, int32_t *r2c, int64_t *tot, int64_t *dual, int *err)
{
    const size_t shm = (size_t)nl * (sizeof(int64_t) + 5 * sizeof(int32_t));
    const size_t tab = in.dist ? sizeof(int32_t) * (size_t)S * S : 0;
    const int grid = std::min(batch, 1 << 20);
    hipStream_t st = ctx().stream;
    if (in.dist && shm + tab <= lds_budget()) {
        lds_allow(k_assign_pos_batched<T, CPT, true>, shm + tab);
        k_assign_pos_batched<T, CPT, true><<<grid, T, shm + tab, st>>>(batch, n_out, nl, in.cab_off, cab, in.dem_off, dem, cnt, in.dist, S,
                                                                       fill, thr, r2c, tot, dual, err);
    } else {
        k_assign_pos_batched<T, CPT, false><<<grid, T, shm, st>>>(batch, n_out, nl, in.cab_off, cab, in.dem_off, dem, cnt, in.dist, S,
                                                                  fill, thr, r2c, tot, dual, err);
    }
}

void launch_pos_assign(int batch, int n_out, int nl, const PosIn &in, const int32_t *cab, const int32_t *dem, const int32_t *cnt, int S,
                       int32_t fill, int32_t thr, int32_t *r2c, int64_t *tot, int64_t *dual, int *err)
{
    if (nl <= 64)
        launch_pos_assign_t<64, 1>(batch, n_out, nl, in, cab, dem, cnt, S, fill, thr, r2c, tot, dual, err);
    else if (nl <= 128)
        launch_pos_assign_t<64, 2>(batch, n_out, nl, in, cab, dem, cnt, S, fill, thr, r2c, tot, dual, err);
    else if (nl <= 256)
        launch_pos_assign_t<256, 1>(batch, n_out, nl, in, cab, dem, cnt, S, fill, thr, r2c, tot, dual, err);
    else if (nl <= 512)
        launch_pos_assign_t<256, 2>(batch, n_out, nl, in, cab, dem, cnt, S, fill, thr, r2c, tot, dual, err);
    else
        launch_pos_assign_t<256, 4>(batch, n_out, nl, in, cab, dem, cnt, S, fill, thr, r2c, tot, dual, err);
}

template <int T, bool POLICY>
void launch_tick_lcm_t(int batch, int n_out, int nl, const PosIn &in, int S, int32_t fill, int32_t thr, int stop_size,
                       const int32_t *mode, const int32_t *stop_arr, const int *gate, void *const *o, int32_t *cab2, int32_t *dem2,
                       int32_t *cnt)
{
    const size_t shm = (size_t)nl * (sizeof(uint64_t) + 3 * sizeof(int32_t)) + 2 * sizeof(uint32_t) * (((size_t)nl + 31) / 32);
    const size_t tab = in.dist ? sizeof(int32_t) * (size_t)S * S : 0;
    const int grid = std::min(batch, 1 << 20);
    hipStream_t st = ctx().stream;
#define TD_TICK_LCM_ARGS                                                                                                          \
    batch, n_out, nl, in.cab_off, in.cab, in.dem_off, in.dem, in.dist, S, fill, thr, stop_size, mode, stop_arr, gate,              \
        (int32_t *)o[0], (int32_t *)o[1], (int32_t *)o[2], (int32_t *)o[3], (int32_t *)o[4], (int32_t *)o[5], (int32_t *)o[6], cab2, \
        dem2, cnt
    if (in.dist && shm + tab <= lds_budget()) {
        lds_allow(k_tick_lcm_batched<T, true, POLICY>, shm + tab);
        k_tick_lcm_batched<T, true, POLICY><<<grid, T, shm + tab, st>>>(TD_TICK_LCM_ARGS);
    } else {
        k_tick_lcm_batched<T, false, POLICY><<<grid, T, shm, st>>>(TD_TICK_LCM_ARGS);
    }
#undef TD_TICK_LCM_ARGS
}

// ---------------------------------------------------------------------------------------------------------------------
// td_split_batched (split.py:61-119): the stand ranges of every case are solved as region models, whoever they leave
// over is solved once more per case.  Both solves are k_assign_pos_batched launches; the three kernels below partition a
// case into its regions, collect the left-overs and sum up.  One workgroup per case (grid-stride beyond SPLIT_GRID),
// every loop bounded by the case's counts or the number of ranges, no atomic on global memory except the error word.
// ---------------------------------------------------------------------------------------------------------------------
enum { ERR_POS = 16, ERR_CELL = 32 };   // further bits of the error word: a position outside [0, size), a cell outside [0, fill)
constexpr int SPLIT_GRID = 2048;
constexpr int SPLIT_RMAX = 64;          // parts <= 32 gives at most 2 * parts - 1 ranges

__device__ __forceinline__ int32_t pos_dist(const int32_t *dist, int S, int a, int b)
{
    return dist ? dist[(int64_t)a * S + b] : (a > b ? a - b : b - a);
}

// sum of v over the workgroup (any number of full waves); s_sum int64[4]
__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t *s_sum)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum_i64(v);
    if (lane == 0) s_sum[w] = v;
    __syncthreads();
    int64_t t = 0;
    for (int q = 0; q < nw; q++) t += s_sum[q];
    __syncthreads();
    return t;
}

// rank of this thread among the threads with f set, in thread order, and their number (block_rank of td_sim_world.h)
__device__ __forceinline__ int split_rank(bool f, int *s_w, int *tot)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = 0, t = 0;
    for (int q = 0; q < nw; q++) {
        if (q < w) off += s_w[q];
        t += s_w[q];
    }
    __syncthreads();
    *tot = t;
    return off + before;
}

// true when a cell of the a x b model over the LDS position lists is outside [0, fill)
__device__ __forceinline__ bool split_cells_bad(const int32_t *pa, int na, const int32_t *pb, int nb, const int32_t *dist, int S,
                                                int32_t fill)
{
    bool bad = false;
    for (int q = threadIdx.x; q < na * nb; q += blockDim.x) {
        const int32_t v = dist[(int64_t)pa[q / nb] * S + pb[q % nb]];
        bad |= (uint32_t)v >= (uint32_t)fill;
    }
    return bad;
}

// launch 1: checks the positions of case c and sorts its cabs (by cab_to) and requests (by dem_from) into range order,
// stably: scab / sdem get the positions, scab_idx / sdem_idx the index within the case.  Region model m = c * R + r starts
// at roff_c[m] / roff_d[m] (absolute, inside the case's segment) and has rcnt[2m] / rcnt[2m + 1] rows / columns: 0 / 0 for
// a region with one side empty, which the solver reads as "no solve".  With a table, every cell of a region model is checked.
// td_dispatch_batched: mode (non-null) leaves every case that is not TD_DISPATCH_SPLIT out as an empty case, and parts
// (non-null) gives case c its own range width size / parts[c]; R is then the largest range count of the batch, and the
// regions beyond a case's own count are empty.
__global__ __launch_bounds__(256) void k_split_part(int batch, int R, int ss, int size, const int32_t *__restrict__ mode,
                                                    const int32_t *__restrict__ parts, const int32_t *__restrict__ cab_off,
                                                    const int32_t *__restrict__ cab, const int32_t *__restrict__ dem_off,
                                                    const int32_t *__restrict__ dem, const int32_t *__restrict__ dist, int S,
                                                    int32_t fill, int32_t *__restrict__ roff_c, int32_t *__restrict__ roff_d,
                                                    int32_t *__restrict__ rcnt, int32_t *__restrict__ scab,
                                                    int32_t *__restrict__ scab_idx, int32_t *__restrict__ sdem,
                                                    int32_t *__restrict__ sdem_idx, int32_t *__restrict__ cnt2,
                                                    int *__restrict__ err)
{
    __shared__ int32_t s_rng[2][BATCH_NMAX];   // range of each cab / request, case order
    __shared__ int32_t s_srt[2][BATCH_NMAX];   // positions in region order
    __shared__ int s_hist[2][SPLIT_RMAX], s_start[2][SPLIT_RMAX + 1];
    __shared__ int s_bad;
    const int tid = threadIdx.x, T = blockDim.x;
    for (int c = blockIdx.x; c < batch; c += gridDim.x) {
        const bool act = !mode || mode[c] == TD_DISPATCH_SPLIT;
        const int c0 = cab_off[c], d0 = dem_off[c];
        const int ns = act ? cab_off[c + 1] - c0 : 0, nd = act ? dem_off[c + 1] - d0 : 0;
        const int pc = parts && act ? parts[c] : 0;
        const int ssc = pc >= 1 && pc <= size ? size / pc : ss;   // validated on the host; never divide by zero
        if (ns > BATCH_NMAX || nd > BATCH_NMAX || (size + ssc - 1) / ssc > R) {   // validated on the host; never index LDS past its arrays
            if (tid == 0) {
                atomicOr(err, ERR_SIZE);
                cnt2[2 * c] = cnt2[2 * c + 1] = 0;
                for (int r = 0; r < R; r++) rcnt[2 * (c * R + r)] = rcnt[2 * (c * R + r) + 1] = 0;
            }
            continue;
        }
        __syncthreads();   // the previous case's LDS is no longer read
        if (tid < SPLIT_RMAX) s_hist[0][tid] = s_hist[1][tid] = 0;
        if (tid == 0) s_bad = 0;
        __syncthreads();
        for (int side = 0; side < 2; side++) {
            const int m = side ? nd : ns;
            const int32_t *src = side ? dem + d0 : cab + c0;
            for (int i = tid; i < m; i += T) {
                const int p = src[i];
                const bool ok = (uint32_t)p < (uint32_t)size;
                const int r = ok ? p / ssc : 0;
                if (!ok) s_bad = 1;
                s_rng[side][i] = r;
                atomicAdd(&s_hist[side][r], 1);
            }
        }
        __syncthreads();
        if (tid < 2) {
            int at = 0;
            for (int r = 0; r < R; r++) {
                s_start[tid][r] = at;
                at += s_hist[tid][r];
            }
            s_start[tid][R] = at;
        }
        __syncthreads();
        const bool bad = s_bad != 0, empty = ns == 0 || nd == 0;
        for (int side = 0; side < 2; side++) {
            const int m = side ? nd : ns, base = side ? d0 : c0;
            const int32_t *src = side ? dem : cab;
            int32_t *dst = side ? sdem : scab, *idx = side ? sdem_idx : scab_idx;
            for (int i = tid; i < m; i += T) {
                const int r = s_rng[side][i];
                int rank = 0;
                for (int j = 0; j < i; j++) rank += s_rng[side][j] == r ? 1 : 0;
                const int at = s_start[side][r] + rank;
                const int32_t p = src[base + i];
                s_srt[side][at] = p;
                dst[base + at] = p;
                idx[base + at] = i;
            }
        }
        if (tid < R) {
            const int m = c * R + tid, hc = s_hist[0][tid], hd = s_hist[1][tid];
            const bool solve = !bad && !empty && hc > 0 && hd > 0;
            roff_c[m] = c0 + s_start[0][tid];
            roff_d[m] = d0 + s_start[1][tid];
            rcnt[2 * m] = solve ? hc : 0;
            rcnt[2 * m + 1] = solve ? hd : 0;
        }
        if (tid == 0) cnt2[2 * c] = cnt2[2 * c + 1] = 0;   // the fifth solve reads them even when launch 3 stops at a refused input
        if (c == batch - 1 && tid == 0) {
            roff_c[batch * R] = c0 + ns;
            roff_d[batch * R] = d0 + nd;
        }
        if (bad && tid == 0) atomicOr(err, ERR_POS);
        __syncthreads();   // s_srt is complete
        if (dist && !bad && !empty) {
            bool cb = false;
            for (int r = 0; r < R; r++) {
                const int hc = s_hist[0][r], hd = s_hist[1][r];
                if (hc > 0 && hd > 0) cb |= split_cells_bad(s_srt[0] + s_start[0][r], hc, s_srt[1] + s_start[1][r], hd, dist, S, fill);
            }
            if (cb) atomicOr(err, ERR_CELL);
        }
    }
}

// launch 3: reads the region models' row_to_col.  A pair on a real cell is served (stage 0): ws_req[cab] = the request,
// both in case indices, and its distance joins sum0[c]; gap0[c] = the regions' total - dual_bound.  Every other cab and
// request of the case goes to the rest lists in case order (ballot + popcount ranks): positions to rcab / rdem, case
// indices to rcab_idx / rdem_idx, at the case's own offsets; nrest = their sizes, cnt2 = the same when both are non-empty
// (else 0 / 0: no fifth solve).  A case with no cabs or no requests has no solve and no lists (split.py:62-64).
// thr >= 0 (td_dispatch_batched): the models were solved on thresholded cells, and a pair on a cell at or above thr is no
// service: both its cab and its request go to the rest.  mode (non-null): a case that is not TD_DISPATCH_SPLIT is empty.
__global__ __launch_bounds__(256) void k_split_rest(int batch, int R, int n_out, int32_t thr, const int32_t *__restrict__ mode,
                                                    const int32_t *__restrict__ cab_off,
                                                    const int32_t *__restrict__ cab, const int32_t *__restrict__ dem_off,
                                                    const int32_t *__restrict__ dem, const int32_t *__restrict__ dist, int S,
                                                    int32_t fill, const int32_t *__restrict__ roff_c,
                                                    const int32_t *__restrict__ roff_d, const int32_t *__restrict__ rcnt,
                                                    const int32_t *__restrict__ scab, const int32_t *__restrict__ scab_idx,
                                                    const int32_t *__restrict__ sdem, const int32_t *__restrict__ sdem_idx,
                                                    const int32_t *__restrict__ r2c1, const int64_t *__restrict__ tot1,
                                                    const int64_t *__restrict__ dual1, int32_t *__restrict__ ws_req,
                                                    int32_t *__restrict__ rcab, int32_t *__restrict__ rcab_idx,
                                                    int32_t *__restrict__ rdem, int32_t *__restrict__ rdem_idx,
                                                    int32_t *__restrict__ cnt2, int32_t *__restrict__ nrest,
                                                    int64_t *__restrict__ sum0, int64_t *__restrict__ gap0, int *err)
{
    __shared__ int32_t s_req[BATCH_NMAX];     // cab -> request served in its region, or -1
    __shared__ int32_t s_dsv[BATCH_NMAX];     // request served in its region
    __shared__ int32_t s_rp[2][BATCH_NMAX];   // positions of the rest lists
    __shared__ int64_t s_sum[4];
    __shared__ int s_w[4], s_err;
    const int tid = threadIdx.x, T = blockDim.x;
    if (tid == 0) s_err = *(volatile int *)err;   // one read per workgroup: another workgroup may set a bit meanwhile
    __syncthreads();
    if (s_err) return;   // an earlier launch refused the input: nothing below is needed
    for (int c = blockIdx.x; c < batch; c += gridDim.x) {
        const bool act = !mode || mode[c] == TD_DISPATCH_SPLIT;
        const int c0 = cab_off[c], d0 = dem_off[c];
        const int ns = act ? cab_off[c + 1] - c0 : 0, nd = act ? dem_off[c + 1] - d0 : 0;
        if (ns > BATCH_NMAX || nd > BATCH_NMAX) continue;   // k_split_part has set the error word
        __syncthreads();   // the previous case's LDS is no longer read
        for (int i = tid; i < ns; i += T) s_req[i] = -1;
        for (int j = tid; j < nd; j += T) s_dsv[j] = 0;
        __syncthreads();
        if (ns == 0 || nd == 0) {
            for (int i = tid; i < ns; i += T) ws_req[c0 + i] = -1;
            if (tid == 0) {
                cnt2[2 * c] = cnt2[2 * c + 1] = 0;
                nrest[2 * c] = nrest[2 * c + 1] = 0;
                sum0[c] = 0;
                gap0[c] = 0;
            }
            continue;
        }
        int64_t sum = 0, gap = 0;
        for (int r = 0; r < R; r++) {
            const int m = c * R + r, nsr = rcnt[2 * m], ndr = rcnt[2 * m + 1];
            if (nsr == 0) continue;   // uniform
            const int rc = roff_c[m], rd = roff_d[m];
            for (int i = tid; i < nsr; i += T) {
                const int j = r2c1[(int64_t)m * n_out + i];
                if ((uint32_t)j < (uint32_t)ndr) {   // a real cell; a dummy column leaves the cab to the rest
                    const int32_t x = pos_dist(dist, S, scab[rc + i], sdem[rd + j]);
                    if (thr < 0 || x < thr) {   // a thresholded cell is fill: no service
                        const int ci = scab_idx[rc + i], dj = sdem_idx[rd + j];
                        s_req[ci] = dj;
                        s_dsv[dj] = 1;
                        sum += x;
                    }
                }
            }
            if (tid == 0) gap += tot1[m] - dual1[m];
        }
        __syncthreads();
        int kc = 0, kd = 0;
        for (int base = 0; base < ns; base += T) {
            const int i = base + tid;
            const bool f = i < ns && s_req[i] < 0;
            int tot;
            const int at = kc + split_rank(f, s_w, &tot);
            if (f) {
                const int32_t p = cab[c0 + i];
                rcab[c0 + at] = p;
                rcab_idx[c0 + at] = i;
                s_rp[0][at] = p;
            }
            kc += tot;
        }
        for (int base = 0; base < nd; base += T) {
            const int j = base + tid;
            const bool f = j < nd && !s_dsv[j];
            int tot;
            const int at = kd + split_rank(f, s_w, &tot);
            if (f) {
                const int32_t p = dem[d0 + j];
                rdem[d0 + at] = p;
                rdem_idx[d0 + at] = j;
                s_rp[1][at] = p;
            }
            kd += tot;
        }
        for (int i = tid; i < ns; i += T) ws_req[c0 + i] = s_req[i];
        sum = block_sum_i64(sum, s_sum);   // its barriers also complete s_rp
        if (dist && split_cells_bad(s_rp[0], kc, s_rp[1], kd, dist, S, fill)) atomicOr(err, ERR_CELL);
        if (tid == 0) {
            const bool solve = kc > 0 && kd > 0;
            cnt2[2 * c] = solve ? kc : 0;
            cnt2[2 * c + 1] = solve ? kd : 0;
            nrest[2 * c] = kc;
            nrest[2 * c + 1] = kd;
            sum0[c] = sum;
            gap0[c] = gap;
        }
    }
}

// launch 5: the fifth models' row_to_col back to case indices (stage 1), their real-cell sums, and the caller's outputs.
// Nothing is written when the error word is set: a refused call leaves every output as it was.
// thr >= 0: as in k_split_rest.  td_dispatch_batched (dp.mode non-null) has only its TD_DISPATCH_SPLIT cases finished here, and
// their results written in td_tick_batched's layout (stride dp.n): no pairs, last minimum fill, the kept lists = the whole
// model in order, row_to_col = the request of each cab, dual_bound = total - the case's dual gap.
struct SplitDisp {
    const int32_t *mode;
    int n;
    int32_t fill;
    int32_t *n_pairs, *last_min, *kept_c, *kept_d, *n_rest, *r2c;
    int64_t *total, *dual;
};

__global__ __launch_bounds__(256) void k_split_final(int batch, int n_out, int32_t thr, SplitDisp dp,
                                                     const int32_t *__restrict__ cab_off,
                                                     const int32_t *__restrict__ dem_off, const int32_t *__restrict__ dist, int S,
                                                     const int32_t *__restrict__ ws_req, const int32_t *__restrict__ rcab,
                                                     const int32_t *__restrict__ rcab_idx, const int32_t *__restrict__ rdem,
                                                     const int32_t *__restrict__ rdem_idx, const int32_t *__restrict__ cnt2,
                                                     const int32_t *__restrict__ nrest, const int64_t *__restrict__ sum0,
                                                     const int64_t *__restrict__ gap0, const int32_t *__restrict__ r2c2,
                                                     const int64_t *__restrict__ tot2, const int64_t *__restrict__ dual2,
                                                     int32_t *__restrict__ cab_req, int32_t *__restrict__ cab_stage,
                                                     int64_t *__restrict__ total, int64_t *__restrict__ rest_total,
                                                     int32_t *__restrict__ n_rest, int64_t *__restrict__ dual_gap,
                                                     const int *__restrict__ err)
{
    __shared__ int32_t s_req[BATCH_NMAX], s_stage[BATCH_NMAX];
    __shared__ int64_t s_sum[4];
    const int tid = threadIdx.x, T = blockDim.x;
    if (*err) return;   // uniform: nothing in this launch writes the word
    for (int c = blockIdx.x; c < batch; c += gridDim.x) {
        if (dp.mode && dp.mode[c] != TD_DISPATCH_SPLIT) continue;   // uniform: the tick's launches have written this model
        const int c0 = cab_off[c], d0 = dem_off[c];
        const int ns = cab_off[c + 1] - c0;
        __syncthreads();   // the previous case's LDS is no longer read
        for (int i = tid; i < ns; i += T) {
            const int v = ws_req[c0 + i];
            s_req[i] = v;
            s_stage[i] = v >= 0 ? 0 : -1;
        }
        __syncthreads();
        const int kc = cnt2[2 * c], kd = cnt2[2 * c + 1];
        int64_t sum = 0;
        for (int i = tid; i < kc; i += T) {
            const int j = r2c2[(int64_t)c * n_out + i];
            if ((uint32_t)j < (uint32_t)kd) {
                const int32_t x = pos_dist(dist, S, rcab[c0 + i], rdem[d0 + j]);
                if (thr < 0 || x < thr) {
                    const int ci = rcab_idx[c0 + i];
                    s_req[ci] = rdem_idx[d0 + j];
                    s_stage[ci] = 1;
                    sum += x;
                }
            }
        }
        sum = block_sum_i64(sum, s_sum);
        if (dp.mode) {
            const int nd = dem_off[c + 1] - d0;
            const int64_t at = (int64_t)c * dp.n;
            for (int i = tid; i < dp.n; i += T) {
                dp.r2c[at + i] = i < ns ? s_req[i] : -1;
                if (dp.kept_c && i < ns) dp.kept_c[at + i] = i;
                if (dp.kept_d && i < nd) dp.kept_d[at + i] = i;
            }
            if (tid == 0) {
                const int64_t tot = sum0[c] + sum;
                dp.n_pairs[c] = 0;
                dp.last_min[c] = dp.fill;
                dp.n_rest[c] = ns > nd ? ns : nd;
                dp.total[c] = tot;
                if (dp.dual) dp.dual[c] = tot - (gap0[c] + tot2[c] - dual2[c]);
            }
            continue;
        }
        for (int i = tid; i < ns; i += T) {
            cab_req[c0 + i] = s_req[i];
            if (cab_stage) cab_stage[c0 + i] = s_stage[i];
        }
        if (tid == 0) {
            total[c] = sum0[c] + sum;
            if (rest_total) rest_total[c] = sum;
            if (n_rest) {
                n_rest[2 * c] = nrest[2 * c];
                n_rest[2 * c + 1] = nrest[2 * c + 1];
            }
            if (dual_gap) dual_gap[c] = gap0[c] + tot2[c] - dual2[c];
        }
    }
}

Buf g_sp;                       // td_split_batched's device workspace (grow-only)
std::vector<char> g_sp_host;    // its host destinations land here first: a refused call leaves the caller's arrays unwritten

// the split launches' workspace inside g_sp: B cases, M = B * R region models, nl = the largest model, nc / nd positions
struct SplitWs {
    int64_t *tot1, *dual1, *tot2, *dual2, *sum0, *gap0;
    int32_t *roff_c, *roff_d, *rcnt, *scab, *scab_idx, *sdem, *sdem_idx, *r2c1, *ws_req, *rcab, *rcab_idx, *rdem, *rdem_idx, *cnt2, *nrest,
        *r2c2;
};

int split_ws(size_t B, size_t M, size_t nl, size_t nc, size_t nd, SplitWs *s)
{
    return carve_buf(g_sp, [&](Carve &c) {
        for (int64_t **a : {&s->tot1, &s->dual1}) *a = c.take<int64_t>(M);
        for (int64_t **a : {&s->tot2, &s->dual2, &s->sum0, &s->gap0}) *a = c.take<int64_t>(B);
        s->roff_c = c.take<int32_t>(M + 1);
        s->roff_d = c.take<int32_t>(M + 1);
        s->rcnt = c.take<int32_t>(2 * M);
        s->scab = c.take<int32_t>(nc);
        s->scab_idx = c.take<int32_t>(nc);
        s->sdem = c.take<int32_t>(nd);
        s->sdem_idx = c.take<int32_t>(nd);
        s->r2c1 = c.take<int32_t>(M * nl);
        for (int32_t **a : {&s->ws_req, &s->rcab, &s->rcab_idx}) *a = c.take<int32_t>(nc);
        for (int32_t **a : {&s->rdem, &s->rdem_idx}) *a = c.take<int32_t>(nd);
        s->cnt2 = c.take<int32_t>(2 * B);
        s->nrest = c.take<int32_t>(2 * B);
        s->r2c2 = c.take<int32_t>(B * nl);
    });
}

// launches 1 to 4 of the split: partition, the region models, collection, the fifth models (thr, mode, parts: see the kernels)
void split_launches(int batch, int R, int ss, int size, int nl, const PosIn &in, int S, int32_t fill, int32_t thr, const int32_t *mode,
                    const int32_t *parts, const SplitWs &w, int *d_err)
{
    Ctx &c = ctx();
    const int T = nl <= 64 ? 64 : 256, grid = std::min(batch, SPLIT_GRID);
    const int M = batch * R;
    k_split_part<<<grid, T, 0, c.stream>>>(batch, R, ss, size, mode, parts, in.cab_off, in.cab, in.dem_off, in.dem, in.dist, S, fill,
                                           w.roff_c, w.roff_d, w.rcnt, w.scab, w.scab_idx, w.sdem, w.sdem_idx, w.cnt2, d_err);
    PosIn rin = in;
    rin.cab_off = w.roff_c;
    rin.dem_off = w.roff_d;
    launch_pos_assign(M, nl, nl, rin, w.scab, w.sdem, w.rcnt, S, fill, thr, w.r2c1, w.tot1, w.dual1, d_err);
    k_split_rest<<<grid, T, 0, c.stream>>>(batch, R, nl, thr, mode, in.cab_off, in.cab, in.dem_off, in.dem, in.dist, S, fill, w.roff_c,
                                           w.roff_d, w.rcnt, w.scab, w.scab_idx, w.sdem, w.sdem_idx, w.r2c1, w.tot1, w.dual1, w.ws_req,
                                           w.rcab, w.rcab_idx, w.rdem, w.rdem_idx, w.cnt2, w.nrest, w.sum0, w.gap0, d_err);
    launch_pos_assign(batch, nl, nl, in, w.rcab, w.rdem, w.cnt2, S, fill, thr, w.r2c2, w.tot2, w.dual2, d_err);
}

// the split's refusals that are found on the device, from the error word
int split_error(const char *fn, int e, int size, int32_t fill)
{
    if (e & ERR_POS) return fail(TD_EINVAL, "%s: a cab_to / dem_from position outside [0, %d)", fn, size);
    if (e & ERR_CELL) return fail(TD_EINVAL, "%s: a table entry used as a cell is outside [0, fill = %d)", fn, (int)fill);
    return cap_error(fn, e);
}

// the split's argument refusals, in the order they are tested; `which` selects the groups a call tests at this point.
// model >= 0: p is parts[model] of td_dispatch_batched, named so in the message
enum { SPLIT_PARTS = 1, SPLIT_CITY = 2, SPLIT_RANGES = 4 };
int split_refusal(const char *fn, int which, int model, int p, int size, const int32_t *dist, int S, int32_t fill, int batch, int R)
{
    if ((which & SPLIT_PARTS) && (p < 1 || p > 32 || size < p)) {
        char idx[24] = "";
        if (model >= 0) snprintf(idx, sizeof(idx), "[%d]", model);
        if (p < 1 || p > 32) return fail(TD_EINVAL, "%s: parts%s = %d outside [1, 32]", fn, idx, p);
        return fail(TD_EINVAL, "%s: size = %d < parts%s = %d", fn, size, idx, p);
    }
    if (which & SPLIT_CITY) {
        if (dist && S < size) return fail(TD_EINVAL, "%s: the table has S = %d stands, fewer than size = %d", fn, S, size);
        if (dist && fill < 1) return fail(TD_EINVAL, "%s: fill = %d < 1", fn, (int)fill);
        if (!dist && (int64_t)size - 1 >= (int64_t)fill)
            return fail(TD_EINVAL, "%s: the distance %d of the line's ends is not below fill = %d", fn, size - 1, (int)fill);
    }
    if (which & SPLIT_RANGES) {
        if (R >= SPLIT_RMAX) return fail(TD_EINTERNAL, "%s: %d ranges", fn, R);   // parts <= 32 gives at most 63
        if ((int64_t)batch * R > INT_MAX / 2)
            return fail(TD_EINVAL, "%s: %d cases of %d ranges are more than 2^30 region models", fn, batch, R);
    }
    return TD_OK;
}

Buf g_pol[3];                    // td_dispatch_batched: device copies of host mode / stop_size / parts
std::vector<int32_t> g_polh[3];  // their host copies (validated there)

}  // namespace

void td::pool2_greedy_launch(int batch, int n, const int32_t *d_ns, const int32_t *d_cost, int32_t *rows, int32_t *cols, int32_t *n_pairs)
{
    const size_t shm = (size_t)n * (sizeof(uint64_t) + sizeof(int32_t)) + sizeof(uint32_t) * (((size_t)n + 31) / 32);
    const int grid = std::min(batch, 1 << 20);
    Ctx &c = ctx();
    if (n <= 128) {
        k_pool2_lcm_batched<64><<<grid, 64, shm, c.stream>>>(batch, n, d_ns, d_cost, rows, cols, n_pairs);
    } else {
        lds_allow(k_pool2_lcm_batched<256>, shm);
        k_pool2_lcm_batched<256><<<grid, 256, shm, c.stream>>>(batch, n, d_ns, d_cost, rows, cols, n_pairs);
    }
}

extern "C" {

int td_assign_batched(int batch, int n, const int32_t *ns, const int32_t *cost, int32_t *row_to_col, int64_t *total,
                      int64_t *dual_bound, int64_t *col_price)
{
    TD_REQUIRE_INIT();
    const int32_t *d_ns, *d_cost;
    int rc = batch_args("td_assign_batched", batch, n, ns, cost, &d_ns, &d_cost);
    if (rc) return rc;
    if (batch == 0) return TD_OK;
    if (!row_to_col || !total) return fail(TD_EINVAL, "td_assign_batched: null row_to_col / total");
    const size_t B = (size_t)batch, N = (size_t)n;
    Out o[4] = {{row_to_col, sizeof(int32_t) * B * N}, {total, sizeof(int64_t) * B}, {dual_bound, sizeof(int64_t) * B},
                {col_price, sizeof(int64_t) * B * N}};
    int *d_err;
    if ((rc = outputs_prepare(g_out, o, 4, &d_err))) return rc;
    int32_t *r2c = (int32_t *)o[0].dptr();
    int64_t *tot = (int64_t *)o[1].dptr(), *dual = (int64_t *)o[2].dptr(), *price = (int64_t *)o[3].dptr();
    const size_t shm = N * (sizeof(int64_t) + 3 * sizeof(int32_t));
    const size_t shm_staged = shm + sizeof(int32_t) * N * N;
    if (n <= 64)
        launch_assign<64, 1, true>(batch, n, d_ns, d_cost, r2c, tot, dual, price, d_err, shm_staged);
    else if (n <= 128 && shm_staged <= STAGE_LDS_MAX)
        launch_assign<64, 2, true>(batch, n, d_ns, d_cost, r2c, tot, dual, price, d_err, shm_staged);
    else if (n <= 128)
        launch_assign<64, 2, false>(batch, n, d_ns, d_cost, r2c, tot, dual, price, d_err, shm);
    else if (n <= 256)
        launch_assign<256, 1, false>(batch, n, d_ns, d_cost, r2c, tot, dual, price, d_err, shm);
    else if (n <= 512)
        launch_assign<256, 2, false>(batch, n, d_ns, d_cost, r2c, tot, dual, price, d_err, shm);
    else
        launch_assign<256, 4, false>(batch, n, d_ns, d_cost, r2c, tot, dual, price, d_err, shm);
    return batch_finish("td_assign_batched", o, 4, d_err);
}

int td_lcm_batched(int batch, int n, const int32_t *ns, const int32_t *cost, int32_t mask, int32_t threshold, int stop_value_on,
                   int32_t stop_value, int stop_size, int64_t sum_below, int32_t *rows, int32_t *cols, int32_t *n_pairs,
                   int64_t *total, int32_t *last_min)
{
    TD_REQUIRE_INIT();
    const int32_t *d_ns, *d_cost;
    int rc = batch_args("td_lcm_batched", batch, n, ns, cost, &d_ns, &d_cost);
    if (rc) return rc;
    if (batch == 0) return TD_OK;
    if (!rows || !cols || !n_pairs || !total || !last_min) return fail(TD_EINVAL, "td_lcm_batched: null output array");
    const size_t B = (size_t)batch, N = (size_t)n;
    Out o[5] = {{rows, sizeof(int32_t) * B * N}, {cols, sizeof(int32_t) * B * N}, {n_pairs, sizeof(int32_t) * B},
                {total, sizeof(int64_t) * B}, {last_min, sizeof(int32_t) * B}};
    int *d_err;
    if ((rc = outputs_prepare(g_out, o, 5, &d_err))) return rc;
    // Java's scan only ever sees cells strictly below big_cost (Simulator.java:529-537)
    const int64_t cand_limit = stop_value_on ? (int64_t)stop_value : (int64_t)INT64_MAX;
    const size_t shm = N * (sizeof(uint64_t) + sizeof(int32_t)) + sizeof(uint32_t) * ((N + 31) / 32);
    const int grid = std::min(batch, 1 << 20);
    Ctx &c = ctx();
    if (n <= 128)
        k_lcm_batched<64><<<grid, 64, shm, c.stream>>>(batch, n, d_ns, d_cost, cand_limit, mask, threshold, stop_value_on, stop_value,
                                                       stop_size, sum_below, (int32_t *)o[0].dptr(), (int32_t *)o[1].dptr(),
                                                       (int32_t *)o[2].dptr(), (int64_t *)o[3].dptr(), (int32_t *)o[4].dptr());
    else
        k_lcm_batched<256><<<grid, 256, shm, c.stream>>>(batch, n, d_ns, d_cost, cand_limit, mask, threshold, stop_value_on,
                                                         stop_value, stop_size, sum_below, (int32_t *)o[0].dptr(),
                                                         (int32_t *)o[1].dptr(), (int32_t *)o[2].dptr(), (int64_t *)o[3].dptr(),
                                                         (int32_t *)o[4].dptr());
    return batch_finish("td_lcm_batched", o, 5, d_err);
}

int td_build_assign_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to, const int32_t *dem_off,
                            const int32_t *dem_from, const int32_t *dist, int S, int32_t fill, int32_t threshold, int32_t *row_to_col,
                            int64_t *total, int64_t *dual_bound)
{
    TD_REQUIRE_INIT();
    PosIn in;
    int rc = pos_args("td_build_assign_batched", batch, n, BATCH_NMAX, cab_off, cab_to, dem_off, dem_from, dist, S, &in);
    if (rc) return rc;
    if (batch == 0) return TD_OK;
    if (!row_to_col || !total) return fail(TD_EINVAL, "td_build_assign_batched: null row_to_col / total");
    const size_t B = (size_t)batch, N = (size_t)n;
    Out o[3] = {{row_to_col, sizeof(int32_t) * B * N}, {total, sizeof(int64_t) * B}, {dual_bound, sizeof(int64_t) * B}};
    int *d_err;
    if ((rc = outputs_prepare(g_out, o, 3, &d_err))) return rc;
    launch_pos_assign(batch, n, in.nmax, in, in.cab, in.dem, nullptr, S, fill, threshold, (int32_t *)o[0].dptr(), (int64_t *)o[1].dptr(),
                      (int64_t *)o[2].dptr(), d_err);
    return batch_finish("td_build_assign_batched", o, 3, d_err);
}

int td_tick_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to, const int32_t *dem_off, const int32_t *dem_from,
                    const int32_t *dist, int S, int32_t fill, int32_t threshold, int stop_size, int32_t *lcm_rows, int32_t *lcm_cols,
                    int32_t *n_pairs, int32_t *lcm_last_min, int32_t *kept_cabs, int32_t *kept_dems, int32_t *n_rest,
                    int32_t *row_to_col, int64_t *total, int64_t *dual_bound)
{
    TD_REQUIRE_INIT();
    PosIn in;
    int rc = pos_args("td_tick_batched", batch, n, TICK_NMAX, cab_off, cab_to, dem_off, dem_from, dist, S, &in);
    if (rc) return rc;
    if (batch == 0) return TD_OK;
    if (!lcm_rows || !lcm_cols || !n_pairs || !lcm_last_min || !n_rest || !row_to_col || !total)
        return fail(TD_EINVAL, "td_tick_batched: null output array");
    // the remainder that goes to the solver: stop_size rows where the LCM runs, the whole model where it does not
    int nsol = 0;
    for (int b = 0; b < batch; b++) {
        const int nb = std::max(g_off[0][b + 1] - g_off[0][b], g_off[1][b + 1] - g_off[1][b]);
        const int rest = stop_size >= 0 && stop_size < nb ? stop_size : nb;
        if (rest > BATCH_NMAX)
            return fail(TD_EINVAL, "td_tick_batched: model %d leaves %d rows to the solver, more than %d (stop_size = %d)", b, rest,
                        BATCH_NMAX, stop_size);
        nsol = std::max(nsol, rest);
    }
    const size_t B = (size_t)batch, N = (size_t)n;
    const size_t nc = (size_t)g_off[0][batch], nd = (size_t)g_off[1][batch];
    if ((rc = ensure(g_ws, sizeof(int32_t) * (nc + nd + 2 * B)))) return rc;
    int32_t *cab2 = (int32_t *)g_ws.p, *dem2 = cab2 + nc, *cnt = dem2 + nd;
    Out o[10] = {{lcm_rows, sizeof(int32_t) * B * N}, {lcm_cols, sizeof(int32_t) * B * N}, {n_pairs, sizeof(int32_t) * B},
                 {lcm_last_min, sizeof(int32_t) * B},  {kept_cabs, sizeof(int32_t) * B * N}, {kept_dems, sizeof(int32_t) * B * N},
                 {n_rest, sizeof(int32_t) * B},       {row_to_col, sizeof(int32_t) * B * N}, {total, sizeof(int64_t) * B},
                 {dual_bound, sizeof(int64_t) * B}};
    int *d_err;
    if ((rc = outputs_prepare(g_out, o, 10, &d_err))) return rc;
    void *od[7];
    for (int k = 0; k < 7; k++) od[k] = o[k].dptr();
    if (in.nmax <= 128)
        launch_tick_lcm_t<64, false>(batch, n, in.nmax, in, S, fill, threshold, stop_size, nullptr, nullptr, nullptr, od, cab2, dem2, cnt);
    else
        launch_tick_lcm_t<256, false>(batch, n, in.nmax, in, S, fill, threshold, stop_size, nullptr, nullptr, nullptr, od, cab2, dem2, cnt);
    launch_pos_assign(batch, n, nsol, in, cab2, dem2, cnt, S, fill, threshold, (int32_t *)o[7].dptr(), (int64_t *)o[8].dptr(),
                      (int64_t *)o[9].dptr(), d_err);
    return batch_finish("td_tick_batched", o, 10, d_err);
}

int td_split_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to, const int32_t *dem_off, const int32_t *dem_from,
                     const int32_t *dist, int S, int size, int parts, int32_t fill, int32_t *cab_req, int32_t *cab_stage,
                     int64_t *total, int64_t *rest_total, int32_t *n_rest, int64_t *dual_gap)
{
    TD_REQUIRE_INIT();
    const char *fn = "td_split_batched";
    int rc = split_refusal(fn, SPLIT_PARTS | SPLIT_CITY, -1, parts, size, dist, S, fill, 0, 0);
    if (rc) return rc;
    PosIn in;
    if ((rc = pos_args(fn, batch, n, BATCH_NMAX, cab_off, cab_to, dem_off, dem_from, dist, S, &in))) return rc;
    if (batch == 0) return TD_OK;
    if (!cab_req || !total) return fail(TD_EINVAL, "%s: null cab_req / total", fn);
    const int ss = size / parts, R = (size + ss - 1) / ss, nl = in.nmax;
    if ((rc = split_refusal(fn, SPLIT_RANGES, -1, parts, size, dist, S, fill, batch, R))) return rc;
    const size_t B = (size_t)batch, M = B * (size_t)R, nc = (size_t)g_off[0][batch], nd = (size_t)g_off[1][batch];
    SplitWs w;
    if ((rc = split_ws(B, M, (size_t)nl, nc, nd, &w))) return rc;
    Out o[6] = {{cab_req, sizeof(int32_t) * nc},   {cab_stage, sizeof(int32_t) * nc}, {total, sizeof(int64_t) * B},
                {rest_total, sizeof(int64_t) * B}, {n_rest, sizeof(int32_t) * 2 * B}, {dual_gap, sizeof(int64_t) * B}};
    int *d_err;
    if ((rc = outputs_prepare(g_out, o, 6, &d_err))) return rc;
    Ctx &c = ctx();
    split_launches(batch, R, ss, size, nl, in, S, fill, -1, nullptr, nullptr, w, d_err);
    k_split_final<<<std::min(batch, SPLIT_GRID), nl <= 64 ? 64 : 256, 0, c.stream>>>(
        batch, nl, -1, SplitDisp{}, in.cab_off, in.dem_off, in.dist, S, w.ws_req, w.rcab, w.rcab_idx, w.rdem, w.rdem_idx, w.cnt2, w.nrest,
        w.sum0, w.gap0, w.r2c2, w.tot2, w.dual2, (int32_t *)o[0].dptr(), (int32_t *)o[1].dptr(), (int64_t *)o[2].dptr(),
        (int64_t *)o[3].dptr(), (int32_t *)o[4].dptr(), (int64_t *)o[5].dptr(), d_err);
    // host destinations: through g_sp_host, handed over only when the call succeeded
    return outputs_finish_on_success(o, 6, d_err, g_sp_host, [&](int e) { return split_error(fn, e, size, fill); });
}

// A policy per model, structured as td_pool2_batched_v is: the tick's two launches take every model that is not a split model
// (a split model is not theirs), the split's launches take the split models (every other case is empty for them) and run
// only when there is one: 2 launches without a split model, 7 with one, whatever the batch and the mix.  The split launches
// come first, so that an input they refuse on the device (a position, a table entry) stops the tick's launches before they
// write an output.
int td_dispatch_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to, const int32_t *dem_off, const int32_t *dem_from,
                        const int32_t *dist, int S, int32_t fill, int32_t threshold, int size, const int32_t *mode,
                        const int32_t *stop_size, const int32_t *parts, int32_t *lcm_rows, int32_t *lcm_cols, int32_t *n_pairs,
                        int32_t *lcm_last_min, int32_t *kept_cabs, int32_t *kept_dems, int32_t *n_rest, int32_t *row_to_col,
                        int64_t *total, int64_t *dual_bound)
{
    TD_REQUIRE_INIT();
    const char *fn = "td_dispatch_batched";
    PosIn in;
    int rc = pos_args(fn, batch, n, TICK_NMAX, cab_off, cab_to, dem_off, dem_from, dist, S, &in);
    if (rc) return rc;
    if (batch == 0) return TD_OK;
    if (!lcm_rows || !lcm_cols || !n_pairs || !lcm_last_min || !n_rest || !row_to_col || !total)
        return fail(TD_EINVAL, "%s: null output array", fn);
    Ctx &c = ctx();
    const size_t B = (size_t)batch;
    // the policy arrays on the host (validated there) and on the device
    const int32_t *pol[3] = {mode, stop_size, parts}, *d_pol[3] = {nullptr, nullptr, nullptr};
    // the device arrays come home in one synchronisation
    if ((rc = host_copy({{mode, B, &g_polh[0]}, {stop_size, B, &g_polh[1]}, {parts, B, &g_polh[2]}}))) return rc;
    int nsol = 0, nsplit = 0, nl_split = 0, R = 1;
    for (int b = 0; b < batch; b++) {
        const int md = mode ? g_polh[0][b] : TD_DISPATCH_LCM_OPT;
        const int ns = g_off[0][b + 1] - g_off[0][b], nd = g_off[1][b + 1] - g_off[1][b], nb = std::max(ns, nd);
        if (md < TD_DISPATCH_LCM_OPT || md > TD_DISPATCH_SPLIT) return fail(TD_EINVAL, "%s: mode[%d] = %d outside 0 .. 3", fn, b, md);
        if (md == TD_DISPATCH_SPLIT) {
            const int p = parts ? g_polh[2][b] : 4;
            if (nb > BATCH_NMAX)
                return fail(TD_EINVAL, "%s: split model %d has %d cabs and %d requests, more than %d", fn, b, ns, nd, BATCH_NMAX);
            if ((rc = split_refusal(fn, SPLIT_PARTS, b, p, size, dist, S, fill, batch, R))) return rc;
            const int ss = size / p;
            R = std::max(R, (size + ss - 1) / ss);
            nl_split = std::max(nl_split, nb);
            nsplit++;
        } else if (md != TD_DISPATCH_LCM) {
            // the remainder that goes to the solver: stop_size rows where the LCM runs, the whole model where it does not
            const int st = md == TD_DISPATCH_OPT || !stop_size ? -1 : g_polh[1][b];
            const int rest = st >= 0 && st < nb ? st : nb;
            if (rest > BATCH_NMAX)
                return fail(TD_EINVAL, "%s: model %d leaves %d rows to the solver, more than %d (stop_size = %d)", fn, b, rest, BATCH_NMAX, st);
            nsol = std::max(nsol, rest);
        }
    }
    if (nsplit && (rc = split_refusal(fn, SPLIT_CITY | SPLIT_RANGES, -1, 0, size, dist, S, fill, batch, R))) return rc;
    const void *p;
    for (int k = 0; k < 3; k++) {
        if (!pol[k]) continue;
        if ((rc = to_device(is_device_ptr(pol[k]) ? (const void *)pol[k] : (const void *)g_polh[k].data(), sizeof(int32_t) * B, g_pol[k], &p)))
            return rc;
        d_pol[k] = (const int32_t *)p;
    }
    const size_t N = (size_t)n, nc = (size_t)g_off[0][batch], nd = (size_t)g_off[1][batch];
    if ((rc = ensure(g_ws, sizeof(int32_t) * (nc + nd + 2 * B)))) return rc;
    int32_t *cab2 = (int32_t *)g_ws.p, *dem2 = cab2 + nc, *cnt = dem2 + nd;
    SplitWs w{};
    if (nsplit && (rc = split_ws(B, B * (size_t)R, (size_t)nl_split, nc, nd, &w))) return rc;
    Out o[10] = {{lcm_rows, sizeof(int32_t) * B * N}, {lcm_cols, sizeof(int32_t) * B * N}, {n_pairs, sizeof(int32_t) * B},
                 {lcm_last_min, sizeof(int32_t) * B},  {kept_cabs, sizeof(int32_t) * B * N}, {kept_dems, sizeof(int32_t) * B * N},
                 {n_rest, sizeof(int32_t) * B},       {row_to_col, sizeof(int32_t) * B * N}, {total, sizeof(int64_t) * B},
                 {dual_bound, sizeof(int64_t) * B}};
    int *d_err;
    if ((rc = outputs_prepare(g_out, o, 10, &d_err))) return rc;
    void *od[7];
    for (int k = 0; k < 7; k++) od[k] = o[k].dptr();
    // the range width of a case without a parts entry: 4 parts (parts == NULL), or any width for a case that is not split
    if (nsplit) split_launches(batch, R, parts ? size : size / 4, size, nl_split, in, S, fill, threshold, d_pol[0], d_pol[2], w, d_err);
    const int *gate = nsplit ? d_err : nullptr;
    if (in.nmax <= 128)
        launch_tick_lcm_t<64, true>(batch, n, in.nmax, in, S, fill, threshold, -1, d_pol[0], d_pol[1], gate, od, cab2, dem2, cnt);
    else
        launch_tick_lcm_t<256, true>(batch, n, in.nmax, in, S, fill, threshold, -1, d_pol[0], d_pol[1], gate, od, cab2, dem2, cnt);
    launch_pos_assign(batch, n, nsol, in, cab2, dem2, cnt, S, fill, threshold, (int32_t *)o[7].dptr(), (int64_t *)o[8].dptr(),
                      (int64_t *)o[9].dptr(), d_err);
    if (nsplit) {
        const SplitDisp dp{d_pol[0],          n,
                           fill,              (int32_t *)od[2],
                           (int32_t *)od[3],  (int32_t *)od[4],
                           (int32_t *)od[5],  (int32_t *)od[6],
                           (int32_t *)o[7].dptr(), (int64_t *)o[8].dptr(),
                           (int64_t *)o[9].dptr()};
        k_split_final<<<std::min(batch, SPLIT_GRID), nl_split <= 64 ? 64 : 256, 0, c.stream>>>(
            batch, nl_split, threshold, dp, in.cab_off, in.dem_off, in.dist, S, w.ws_req, w.rcab, w.rcab_idx, w.rdem, w.rdem_idx, w.cnt2,
            w.nrest, w.sum0, w.gap0, w.r2c2, w.tot2, w.dual2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_err);
    }
    // host destinations: through g_sp_host, handed over only when the call succeeded
    return outputs_finish_on_success(o, 10, d_err, g_sp_host, [&](int e) { return split_error(fn, e, size, fill); });
}

}  // extern "C"

void td::batch_release_workspace()
{
    Buf *bs[] = {&g_out, &g_ws, &g_sp, &g_in[0], &g_in[1], &g_in[2], &g_in[3], &g_in[4], &g_pol[0], &g_pol[1], &g_pol[2]};
    for (Buf *b : bs) buf_free(*b);
}
