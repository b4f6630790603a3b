// td_batch.hip — many small independent models in one call: optimal assignment (td_assign_batched) and the LCM greedy
// (td_lcm_batched) of B square models of size <= 1024, one workgroup per model.  gfx950 only.
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

#include "td_common.h"

using namespace td;

namespace {

constexpr int BATCH_NMAX = 1024;
constexpr uint64_t KEY_INF = ~0ull;
constexpr int COL_BITS = 11;                             // column index of a packed Dijkstra key (n <= 1024 < 2^11)
constexpr int64_t LABEL_LIM = (int64_t)1 << 52;          // labels at or above this cannot be packed
constexpr size_t STAGE_LDS_MAX = 64 * 1024 - 1024;       // dynamic LDS a staged model may take
enum { ERR_STEPS = 1, ERR_AUGMENT = 2, ERR_LABEL = 4 };

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
// optimal assignment: T threads (64 or 256), CPT columns per thread (n <= T * CPT), STAGE: cells in LDS
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
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int par = 0;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int nb = ns ? ns[b] : n;
        const int32_t *base = cost + (int64_t)b * n * n;
        __syncthreads();   // the previous model's LDS is no longer read
        if constexpr (STAGE) {
            for (int i = 0; i < nb; i++)
                for (int j = tid; j < nb; j += T) s_c[i * nb + j] = base[(int64_t)i * n + j];
        }
        for (int i = tid; i < nb; i += T) {
            s_x[i] = INT_MAX;
            s_y[i] = -1;
        }
        __syncthreads();
#define CELL(i, j) (STAGE ? s_c[(i) * nb + (j)] : base[(int64_t)(i) * n + (j)])
        // 1. column reduction; each column's first minimum row is tight: the row takes the lowest such column
        int64_t vr[CPT];
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const int j = tid + k * T;
            vr[k] = 0;
            if (j < nb) {
                int32_t m = CELL(0, j);
                int r = 0;
                for (int i = 1; i < nb; i++) {
                    const int32_t cv = CELL(i, j);
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
            uint64_t key = KEY_INF;
#pragma unroll
            for (int k = 0; k < CPT; k++) {
                const int j = tid + k * T;
                if (j < nb && s_y[j] < 0 && (int64_t)CELL(f, j) == vr[k]) key = key < (uint64_t)j ? key : (uint64_t)j;
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
#pragma unroll
            for (int k = 0; k < CPT; k++) {
                const int j = tid + k * T;
                d[k] = 0;
                if (j < nb) {
                    d[k] = (int64_t)CELL(f, j) - vr[k];
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
                const int64_t ri = (int64_t)CELL(i, jstar) - s_v[jstar];
#pragma unroll
                for (int k = 0; k < CPT; k++) {
                    if (!((vis >> k) & 1u)) {
                        const int j = tid + k * T;
                        const int64_t nd = mu + ((int64_t)CELL(i, j) - vr[k] - ri);
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
            tsum += j >= 0 ? (int64_t)CELL(i, j) : 0;
        }
        if (dual) {
#pragma unroll
            for (int k = 0; k < CPT; k++)
                if (tid + k * T < nb) vsum += vr[k];
            for (int i = w; i < nb; i += NW) {
                int64_t m = INT64_MAX;
                for (int j = lane; j < nb; j += 64) {
                    const int64_t r = (int64_t)CELL(i, j) - s_v[j];
                    m = r < m ? r : m;
                }
                m = wave_min_i64(m);
                if (lane == 0) rsum += m;
            }
        }
#undef CELL
        tsum = wave_sum_i64(tsum);
        vsum = wave_sum_i64(vsum);
        if (lane == 0) {
            s_sum[w] = tsum;
            s_sum[NW + w] = vsum + rsum;
        }
        for (int i = tid; i < n; i += T) {
            r2c[(int64_t)b * n + i] = i < nb ? s_x[i] : -1;
            if (price) price[(int64_t)b * n + i] = i < nb ? s_v[i] : 0;
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
}

// ---------------------------------------------------------------------------------------------------------------------
// LCM: dynamic LDS: row cache uint64[n] | rescan list int32[n] | column mask uint32[(n + 31) / 32]
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lcm_bias(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
__device__ __forceinline__ int32_t lcm_unbias(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }

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
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int par = 0;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int nb = ns ? ns[b] : n;
        const int32_t *base = cost + (int64_t)b * n * n;
        __syncthreads();
        for (int q = tid; q < (nb + 31) / 32; q += T) s_cm[q] = 0u;
        for (int i = tid; i < nb; i += T) s_list[i] = i;
        if (tid == 0) s_cnt = nb;
        __syncthreads();
        int np = 0, size = nb;
        int32_t lm = stop_value;
        int64_t tot = 0;
        for (int it = 0; it <= nb; it++) {
            // rows in the list: first minimum among the live columns below cand_limit (one wave per row)
            const int cnt = s_cnt;
            for (int q = w; q < cnt; q += NW) {
                const int r = s_list[q];
                uint64_t key = KEY_INF;
                for (int j = lane; j < nb; j += 64) {
                    if (!((s_cm[j >> 5] >> (j & 31)) & 1u)) {
                        const int32_t v = base[(int64_t)r * n + j];
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
            if (it == nb) break;   // every row taken
            // the pick: (value, row) minimum of the row caches
            uint64_t key = KEY_INF;
            for (int i = tid; i < nb; i += T) {
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
                rows[(int64_t)b * n + np] = r;
                cols[(int64_t)b * n + np] = c;
            }
            np++;
            if ((int64_t)v < sum_below) tot += v;
            size--;
            __syncthreads();   // everyone has read s_rb[r]
            if (tid == 0) {
                s_rb[r] = KEY_INF;
                s_cm[c >> 5] |= 1u << (c & 31);
                s_cnt = 0;
            }
            __syncthreads();
            if (stop_size >= 0 && size == stop_size) break;   // Simulator.java:544-545
            for (int i = tid; i < nb; i += T) {
                const uint64_t k = s_rb[i];
                if (k != KEY_INF && (int)(uint32_t)k == c) s_list[atomicAdd(&s_cnt, 1)] = i;
            }
            __syncthreads();
        }
        if (tid == 0) {
            n_pairs[b] = np;
            total[b] = tot;
            last_min[b] = lm;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
Buf g_out;                    // device results for host destinations + the error word (grow-only)
std::vector<int32_t> g_ns;    // host copy of ns (validated here; stays alive while its upload may still be in flight)

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
        h.resize((size_t)batch);
        if (is_device_ptr(ns)) {
            TD_HIP(hipMemcpyAsync(h.data(), ns, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, c.stream));
            TD_HIP(hipStreamSynchronize(c.stream));
        } else {
            memcpy(h.data(), ns, sizeof(int32_t) * h.size());
        }
        for (int b = 0; b < batch; b++)
            if (h[b] < 0 || h[b] > n) return fail(TD_EINVAL, "%s: ns[%d] = %d outside [0, %d]", fn, b, h[b], n);
        const void *p;
        int rc = to_device(is_device_ptr(ns) ? (const void *)ns : (const void *)h.data(), sizeof(int32_t) * h.size(), c.stage_a, &p);
        if (rc) return rc;
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

// one output array: the caller's device pointer, or a slice of g_out that is copied back to the caller's host array
struct Out {
    void *user;
    size_t bytes, off;
    bool dev;
    void *dptr() const { return dev ? user : (user ? (char *)g_out.p + off : nullptr); }
};

int outputs_prepare(Out *o, int k, size_t *err_off)
{
    size_t off = 0;
    for (int i = 0; i < k; i++) {
        o[i].dev = o[i].user && is_device_ptr(o[i].user);
        o[i].off = off;
        if (o[i].user && !o[i].dev) off += align256(o[i].bytes);
    }
    *err_off = off;
    int rc = ensure(g_out, off + 256);
    if (rc) return rc;
    TD_HIP(hipMemsetAsync((char *)g_out.p + off, 0, sizeof(int), ctx().stream));
    return TD_OK;
}

int outputs_finish(const char *fn, const Out *o, int k, size_t err_off)
{
    Ctx &c = ctx();
    TD_HIP(hipGetLastError());
    for (int i = 0; i < k; i++)
        if (o[i].user && !o[i].dev && o[i].bytes)
            TD_HIP(hipMemcpyAsync(o[i].user, (char *)g_out.p + o[i].off, o[i].bytes, hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipMemcpyAsync(c.pinned, (char *)g_out.p + err_off, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    const int e = *(int *)c.pinned;
    if (e)
        return fail(TD_EINTERNAL, "%s: a model hit a defensive loop cap (error word 0x%x: 1 search steps, 2 augmenting path, "
                    "4 label range)", fn, e);
    return TD_OK;
}

template <int T, int CPT, bool STAGE>
void launch_assign(int batch, int n, const int32_t *d_ns, const int32_t *d_cost, int32_t *r2c, int64_t *tot, int64_t *dual,
                   int64_t *price, int *err, size_t shm)
{
    const int grid = std::min(batch, 1 << 20);
    k_assign_batched<T, CPT, STAGE><<<grid, T, shm, ctx().stream>>>(batch, n, d_ns, d_cost, r2c, tot, dual, price, err);
}

}  // namespace

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
    size_t err_off;
    if ((rc = outputs_prepare(o, 4, &err_off))) return rc;
    int *d_err = (int *)((char *)g_out.p + err_off);
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
    return outputs_finish("td_assign_batched", o, 4, err_off);
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
    size_t err_off;
    if ((rc = outputs_prepare(o, 5, &err_off))) return rc;
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
    return outputs_finish("td_lcm_batched", o, 5, err_off);
}

}  // extern "C"

void td::batch_release_workspace()
{
    if (g_out.p) (void)hipFree(g_out.p);
    g_out.p = nullptr;
    g_out.cap = 0;
}
