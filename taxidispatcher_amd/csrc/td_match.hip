// td_match.hip — maximum-weight matching of many general graphs per call (td_match_batched) and the greedy / optimal pools
// of two of many ragged pool models per call (td_pool2_batched).  gfx950 only.
//
// One workgroup of ONE wave per model: the weighted blossom method of csrc/td_match_core.h, its control run by the 64
// lanes in lockstep, its O(n) loops (row scan, delta reductions, dual update, least-slack rebuild) split between them.  No
// workgroup ever waits on another; a grid-stride loop covers the models.  A model's state (tdm::bytes(n) = 152 n bytes)
// lives in LDS when it fits, else in one slice per workgroup of a library workspace.  Every model ends with a certificate
// pass over all its pairs (tdm::Match::certify): a violated pair, or a dual bound other than the matched weight, fails the
// call with TD_EINTERNAL.
//
// Pools (pool_opt_min.py:51-122): one workgroup per model writes the model's pair-cost block (cost of the ordered pair
// (A, B), INT_MAX when it is no candidate) once into a workspace slab; the greedy is td_batch.hip's LCM with symmetric
// masking over that block, the optimum is the matching above with weight K - min(c_AB, c_BA), K = floor(m/2) * span + 1
// (one more pool outweighs any cost difference: the lexicographic optimum, most pools, then the least total cost).
#include <limits.h>

#include <vector>

#include "td_stage.h"
#include "td_match_core.h"
#include "td_pool_rule.h"

using namespace td;

namespace {

constexpr int MATCH_NMAX = 2048;
constexpr int64_t POOL_KMAX = (int64_t)1 << 33;   // pool weights stay well inside the solver's range
enum { ERR_POOL_RANGE = 16 };

// a slab model's edge weight: max(W[i][j], W[j][i]), 64-bit cell index
struct SlabW {
    const int32_t *base;
    int n;
    __host__ __device__ __forceinline__ int64_t operator()(int i, int j) const
    {
        const int32_t a = base[(int64_t)i * n + j], b = base[(int64_t)j * n + i];
        return a > b ? a : b;
    }
};

// a pool model's edge weight: K - the cheaper candidate direction; 0 (no edge) when neither direction is a candidate
struct PoolW {
    const int32_t *base;
    int n;
    int64_t K;
    __host__ __device__ __forceinline__ int64_t operator()(int i, int j) const
    {
        const int32_t a = base[(int64_t)i * n + j], b = base[(int64_t)j * n + i];
        const int32_t m = a < b ? a : b;
        return m == INT_MAX ? 0 : K - m;
    }
};

// one model: the solve, the certificate, the outputs (row b of the caller's arrays, stride n; duals optional)
template <class WT>
__device__ __forceinline__ void match_model(const WT &wt, int nb, int b, int n, unsigned char *mem, int32_t *__restrict__ mate,
                                            int64_t *__restrict__ total, int64_t *__restrict__ bound, int64_t *__restrict__ yv,
                                            int32_t *__restrict__ bpar, int64_t *__restrict__ zb, int *__restrict__ err)
{
    tdm::Match<WT> M(tdm::carve(mem, nb), wt, nb);
    int e = nb > 0 ? M.run() : 0;
    int64_t tot = 0, bnd = 0;
    if (!e && nb > 0) e = M.certify(tot, bnd);
    if (!e && tot != bnd) e = tdm::ERR_CERT;
    const int lane = threadIdx.x;
    for (int i = lane; i < n; i += 64) {
        mate[(int64_t)b * n + i] = i < nb ? M.s.mate[i] : -1;
        if (yv) yv[(int64_t)b * n + i] = i < nb ? M.s.dual[i] : 0;
        if (zb) zb[(int64_t)b * n + i] = (i < nb && M.s.base[nb + i] >= 0) ? 2 * M.s.dual[nb + i] : 0;
    }
    if (bpar)   // exported node ids: vertices 0..n-1; blossom nb + k of the solve is n + k
        for (int x = lane; x < 2 * n; x += 64) {
            int p = -1;
            if (x < nb) p = M.s.par[x];
            else if (x >= n && x - n < nb && M.s.base[nb + x - n] >= 0) p = M.s.par[nb + x - n];
            bpar[(int64_t)b * 2 * n + x] = p < 0 ? -1 : n + (p - nb);
        }
    if (lane == 0) {
        total[b] = tot;
        if (bound) bound[b] = bnd;
        if (e) atomicOr(err, e);   // the error bits of every model and kernel of the call accumulate
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// td_match_batched: slab models; state in LDS (LDS) or in ws + blockIdx.x * per
// ---------------------------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(64) void k_match_batched(int batch, int n, const int32_t *__restrict__ ns, const int32_t *__restrict__ w,
                                                      unsigned char *__restrict__ ws, size_t per, int32_t *__restrict__ mate,
                                                      int64_t *__restrict__ total, int64_t *__restrict__ bound, int64_t *__restrict__ yv,
                                                      int32_t *__restrict__ bpar, int64_t *__restrict__ zb, int *__restrict__ err)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    unsigned char *mem = LDS ? s_dyn : ws + (size_t)blockIdx.x * per;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        const int nb = ns ? ns[b] : n;
        __syncthreads();   // the previous model's state is no longer read
        const SlabW W{w + (int64_t)b * n * n, n};
        match_model(W, nb, b, n, mem, mate, total, bound, yv, bpar, zb, err);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// pools: distances, the candidate rule, the pair-cost block
// ---------------------------------------------------------------------------------------------------------------------
// (pd / pool_pair, the candidate rule: td_pool_rule.h, shared with td_lcm.hip)

// model b0 + q of the chunk: pc[q][A][B] = min(cost1, cost2) of a candidate, INT_MAX otherwise (stride n);
// K[q] = floor(m/2) * (max(c_max, 0) + max(-c_min, 0)) + 1, range-checked only for the optimum (the greedy never reads it).
// The policy is per model: opt_v / ml_v [batch] when given (td_pool2_batched_v), the scalars otherwise.  The model's size
// goes to the list of its own kind, ns_g (greedy) or ns_m (optimum), and 0 to the other: the greedy launch and k_pool_match
// each see the other kind as an empty model.  256 threads per model.
__global__ __launch_bounds__(256) void k_pool_costs(int nq, int b0, int n, int optimal, const int32_t *__restrict__ opt_v,
                                                    const int32_t *__restrict__ off, const int32_t *__restrict__ from,
                                                    const int32_t *__restrict__ to, const int32_t *__restrict__ dist, int S, double max_loss,
                                                    const double *__restrict__ ml_v, int32_t *__restrict__ pc, int32_t *__restrict__ ns_g,
                                                    int32_t *__restrict__ ns_m, int64_t *__restrict__ K, int *__restrict__ err)
{
    __shared__ int64_t s_mx[4], s_mn[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int o = off[b0 + q], m = off[b0 + q + 1] - o;
        const int opt = opt_v ? opt_v[b0 + q] : optimal;
        const double ml = ml_v ? ml_v[b0 + q] : max_loss;
        int32_t *blk = pc + (int64_t)q * n * n;
        int64_t mx = INT64_MIN, mn = INT64_MAX;
        for (int a = 0; a < m; a++)
            for (int bb = tid; bb < m; bb += 256) {
                int32_t v = INT_MAX;
                int64_t c1, c2;
                if (a != bb && pool_pair(from[o + a], to[o + a], from[o + bb], to[o + bb], dist, S, ml, &c1, &c2)) {
                    const int64_t cc = c1 < c2 ? c1 : c2;
                    if (cc >= INT_MAX || cc <= INT_MIN) atomicOr(err, ERR_POOL_RANGE);
                    v = (int32_t)cc;
                    mx = cc > mx ? cc : mx;
                    mn = cc < mn ? cc : mn;
                }
                blk[(int64_t)a * n + bb] = v;
            }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const int64_t x = __shfl_xor(mx, s), y = __shfl_xor(mn, s);
            mx = x > mx ? x : mx;
            mn = y < mn ? y : mn;
        }
        if (lane == 0) {
            s_mx[w] = mx;
            s_mn[w] = mn;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; k++) {
                mx = s_mx[k] > mx ? s_mx[k] : mx;
                mn = s_mn[k] < mn ? s_mn[k] : mn;
            }
            ns_g[q] = opt ? 0 : m;
            ns_m[q] = opt ? m : 0;
            int64_t kk = 1;
            if (mx != INT64_MIN) {
                const int64_t span = (mx > 0 ? mx : 0) + (mn < 0 ? -mn : 0);
                kk = (int64_t)(m / 2) * span + 1;
                if (opt && kk + span >= POOL_KMAX) atomicOr(err, ERR_POOL_RANGE);
            }
            K[q] = kk;
        }
        __syncthreads();
    }
}

// the optimum of every pool model of the chunk: mates at q * n (workspace)
template <bool LDS>
__global__ __launch_bounds__(64) void k_pool_match(int nq, int n, const int32_t *__restrict__ ns, const int32_t *__restrict__ pc,
                                                   const int64_t *__restrict__ K, unsigned char *__restrict__ ws, size_t per,
                                                   int32_t *__restrict__ mate, int64_t *__restrict__ total, int *__restrict__ err)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    unsigned char *mem = LDS ? s_dyn : ws + (size_t)blockIdx.x * per;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        __syncthreads();
        const PoolW W{pc + (int64_t)q * n * n, n, K[q]};
        match_model(W, ns[q], q, n, mem, mate, total, nullptr, nullptr, nullptr, nullptr, err);
    }
}

// the pools of model b0 + q: greedy (pairs in pick order from rows / cols) or optimal (from the mates: each pair in its
// cheaper candidate direction, the smaller custA on a tie, listed in ascending (cost, custA, custB)); plan = cost1 < cost2.
// The kind is per model (opt_v [batch] when given).  One wave per model; dynamic LDS: custA, custB, cost int32[n / 2 + 1] each.
__global__ __launch_bounds__(64) void k_pool_finish(int nq, int b0, int n, int optimal_s, const int32_t *__restrict__ opt_v,
                                                    const int32_t *__restrict__ off,
                                                    const int32_t *__restrict__ from, const int32_t *__restrict__ to,
                                                    const int32_t *__restrict__ dist, int S, const int32_t *__restrict__ pc,
                                                    const int32_t *__restrict__ mate, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ cols, const int32_t *__restrict__ npairs,
                                                    int32_t *__restrict__ cust_a, int32_t *__restrict__ cust_b, int32_t *__restrict__ plan,
                                                    int32_t *__restrict__ cost, int32_t *__restrict__ n_pools, int64_t *__restrict__ total)
{
    extern __shared__ __align__(16) unsigned char s_dyn[];
    const int half = n / 2, cap = half + 1;
    int32_t *s_a = reinterpret_cast<int32_t *>(s_dyn), *s_b = s_a + cap, *s_c = s_b + cap;
    const int lane = threadIdx.x;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int b = b0 + q, o = off[b], m = off[b + 1] - o;
        const int optimal = opt_v ? opt_v[b] : optimal_s;   // uniform over the wave
        const int32_t *blk = pc + (int64_t)q * n * n;
        __syncthreads();
        int k = 0;
        if (optimal) {
            for (int i0 = 0; i0 < m; i0 += 64) {
                const int i = i0 + lane;
                const int j = i < m ? mate[(int64_t)q * n + i] : -1;
                const bool p = j > i && j < m;
                const uint64_t msk = __ballot(p);
                if (p && k + tdm::popc(msk) <= cap) {
                    const int32_t cij = blk[(int64_t)i * n + j], cji = blk[(int64_t)j * n + i];
                    const int at = k + tdm::popc(tdm::below(msk));
                    s_a[at] = cij <= cji ? i : j;
                    s_b[at] = cij <= cji ? j : i;
                    s_c[at] = cij <= cji ? cij : cji;
                }
                k += tdm::popc(msk);
            }
            k = k < half ? k : half;
        } else {
            k = npairs[q];
            k = k < half ? k : half;
            for (int t = lane; t < k; t += 64) {
                const int a = rows[(int64_t)q * half + t], c = cols[(int64_t)q * half + t];
                s_a[t] = a;
                s_b[t] = c;
                s_c[t] = blk[(int64_t)a * n + c];
            }
        }
        __syncthreads();
        int64_t tsum = 0;
        for (int t = lane; t < k; t += 64) {
            const int a = s_a[t], c = s_b[t];
            int dst = t;
            if (optimal) {   // rank under (cost, custA, custB); the keys are distinct (the pools are disjoint)
                const uint64_t key = (uint64_t)(uint32_t)(s_c[t] ^ INT_MIN) << 24 | (uint64_t)a << 12 | (uint64_t)c;
                dst = 0;
                for (int r = 0; r < k; r++) {
                    const uint64_t kr = (uint64_t)(uint32_t)(s_c[r] ^ INT_MIN) << 24 | (uint64_t)s_a[r] << 12 | (uint64_t)s_b[r];
                    dst += kr < key;
                }
            }
            int64_t c1, c2;
            pool_pair(from[o + a], to[o + a], from[o + c], to[o + c], dist, S, 0.0, &c1, &c2);
            const int64_t at = (int64_t)b * half + dst;
            cust_a[at] = a;
            cust_b[at] = c;
            plan[at] = c1 < c2 ? 1 : 0;   // CLNT_B_ENDS : CLNT_A_ENDS, even when the cheaper plan failed its test (:65-79)
            cost[at] = s_c[t];
            tsum += s_c[t];
        }
        tsum = tdm::wsum(tsum);
        if (lane == 0) {
            n_pools[b] = k;
            total[b] = tsum;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
Buf g_ws;                   // per-workgroup solver state (models too large for LDS)
Buf g_res;                  // device results for host destinations + the error word
Buf g_pool;                 // pool chunk: pair-cost slab, sizes, K, mates, totals, greedy pairs
Buf g_in[6];                // device copies of host inputs
std::vector<int32_t> g_h;   // host copies (validation)

// solver state for `batch` models of up to nmax vertices: *lds = in LDS, else *ws = slices of *per bytes, one per workgroup;
// *grid = the workgroups to launch
int state_plan(int batch, int nmax, bool *lds, unsigned char **ws, size_t *per, int *grid)
{
    *per = align256(tdm::bytes(std::max(nmax, 1)));
    *lds = *per <= lds_budget();
    *ws = nullptr;
    *grid = std::min(batch, 1 << 20);
    if (!*lds) {
        *grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)*grid, ((size_t)512 << 20) / *per));
        int rc = ensure(g_ws, *per * (size_t)*grid);
        if (rc) return rc;
        *ws = (unsigned char *)g_ws.p;
    }
    return TD_OK;
}

// what the matching kernels leave in the error word
int match_finish(const char *fn, const Out *o, int k, const int *d_err)
{
    return outputs_finish(o, k, d_err, [fn](int e) {
        if (e & ERR_POOL_RANGE)
            return fail(TD_ERANGE, "%s: a pool cost, or a pool weight K - cost (K = floor(m/2) * cost span + 1), leaves the solver's "
                        "integer range", fn);
        if (e)
            return fail(TD_EINTERNAL, "%s: a model failed (error word 0x%x: 1 defensive loop cap, 2 inconsistent state, 4 certificate "
                        "violated, 8 weight range)", fn, e);
        return (int)TD_OK;
    });
}

}  // namespace

size_t td::lds_budget()
{
    static size_t cap = 0;
    static int device = -1;   // the answer is this device's: td_shutdown and a td_init elsewhere ask again
    if (device != ctx().device) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx().device) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            v = 64 * 1024;
        }
        cap = std::min<size_t>((size_t)v, 160 * 1024) - 1024;
        device = ctx().device;
    }
    return cap;
}

extern "C" {

int td_match_batched(int batch, int n, const int32_t *ns, const int32_t *weight, int32_t *mate, int64_t *total, int64_t *dual_bound,
                     int64_t *dual_vertex, int32_t *blossom_parent, int64_t *dual_blossom)
{
    TD_REQUIRE_INIT();
    Ctx &c = ctx();
    const char *fn = "td_match_batched";
    c.stats[14] = 0;   // match_path (TD_MP_*): filled in below once the launch is decided
    if (batch < 0) return fail(TD_EINVAL, "%s: batch = %d < 0", fn, batch);
    if (n < 0 || n > MATCH_NMAX) return fail(TD_EINVAL, "%s: n = %d outside [0, %d]", fn, n, MATCH_NMAX);
    if (batch == 0) return TD_OK;
    if (!mate || !total) return fail(TD_EINVAL, "%s: null mate / total", fn);
    int rc;
    const void *d_ns = nullptr, *d_w = nullptr;
    int nmax = n;
    if (ns) {
        if ((rc = host_copy(ns, (size_t)batch, g_h))) return rc;
        nmax = 0;
        for (int b = 0; b < batch; b++) {
            if (g_h[b] < 0 || g_h[b] > n) return fail(TD_EINVAL, "%s: ns[%d] = %d outside [0, %d]", fn, b, g_h[b], n);
            nmax = std::max(nmax, g_h[b]);
        }
        if ((rc = to_device(is_device_ptr(ns) ? (const void *)ns : (const void *)g_h.data(), sizeof(int32_t) * (size_t)batch, g_in[0],
                            &d_ns)))
            return rc;
    }
    if (n > 0) {
        if (!weight) return fail(TD_EINVAL, "%s: null weight", fn);
        if ((rc = to_device(weight, sizeof(int32_t) * (size_t)batch * n * n, c.stage_d, &d_w))) return rc;
    }
    const size_t B = (size_t)batch, N = (size_t)n;
    Out o[6] = {{mate, sizeof(int32_t) * B * N},          {total, sizeof(int64_t) * B},
                {dual_bound, sizeof(int64_t) * B},       {dual_vertex, sizeof(int64_t) * B * N},
                {blossom_parent, sizeof(int32_t) * B * 2 * N}, {dual_blossom, sizeof(int64_t) * B * N}};
    int *d_err;
    if ((rc = outputs_prepare(g_res, o, 6, &d_err))) return rc;
    bool lds;
    unsigned char *ws;
    size_t per;
    int grid;
    if ((rc = state_plan(batch, nmax, &lds, &ws, &per, &grid))) return rc;
    c.stats[14] = (lds ? TD_MP_LDS : TD_MP_WS) | 1 << TD_MP_CHUNK_SHIFT;
#define TD_MATCH_ARGS                                                                                                               \
    batch, n, (const int32_t *)d_ns, (const int32_t *)d_w, ws, per, (int32_t *)o[0].dptr(), (int64_t *)o[1].dptr(),                 \
        (int64_t *)o[2].dptr(), (int64_t *)o[3].dptr(), (int32_t *)o[4].dptr(), (int64_t *)o[5].dptr(), d_err
    if (lds) {
        lds_allow(k_match_batched<true>, per);
        k_match_batched<true><<<grid, 64, per, c.stream>>>(TD_MATCH_ARGS);
    } else {
        k_match_batched<false><<<grid, 64, 0, c.stream>>>(TD_MATCH_ARGS);
    }
#undef TD_MATCH_ARGS
    return match_finish(fn, o, 6, d_err);
}

}  // extern "C"

namespace {

// td_pool2_batched and td_pool2_batched_v: the policy of model b is (ml_v[b], opt_v[b]) where the arrays are given, the
// scalars otherwise.  The launches of a chunk: k_pool_costs, the greedy and / or k_pool_match, k_pool_finish; which of the
// two middle ones run depends on whether opt_v is given (both) or on the scalar, never on the batch or the arrays' contents.
int pool2_batched_impl(const char *fn, int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to, const int32_t *dist,
                       int S, double max_loss, int optimal, const double *ml_v, const int32_t *opt_v, int32_t *cust_a, int32_t *cust_b,
                       int32_t *plan, int32_t *cost, int32_t *n_pools, int64_t *total)
{
    Ctx &c = ctx();
    c.stats[14] = 0;   // match_path (TD_MP_*): filled in below as the launches are decided and made
    if (batch < 0) return fail(TD_EINVAL, "%s: batch = %d < 0", fn, batch);
    if (n < 0 || n > MATCH_NMAX) return fail(TD_EINVAL, "%s: n = %d outside [0, %d]", fn, n, MATCH_NMAX);
    if (dist && (S <= 0 || S > 46340)) return fail(TD_EINVAL, "%s: S = %d outside [1, 46340] with a distance table", fn, S);
    if (batch == 0) return TD_OK;
    if (!off) return fail(TD_EINVAL, "%s: null offsets", fn);
    if (!cust_a || !cust_b || !plan || !cost || !n_pools || !total) return fail(TD_EINVAL, "%s: null output array", fn);
    int rc;
    std::vector<int32_t> h_off;
    if ((rc = host_copy(off, (size_t)batch + 1, h_off))) return rc;
    Ragged rg;
    if ((rc = ragged_check(fail, fn, "off", "model", h_off.data(), batch, &rg, [&](int b, int m) {
            return m > n ? fail(TD_EINVAL, "%s: model %d has %d customers, more than n = %d", fn, b, m, n) : 0;
        })))
        return rc;
    const int nmax = rg.longest;
    const size_t tot_c = (size_t)rg.total;
    if (tot_c && (!from || !to)) return fail(TD_EINVAL, "%s: null from / to", fn);
    const void *d_optv = nullptr, *d_mlv = nullptr;
    if (opt_v) {
        std::vector<int32_t> ho;
        if ((rc = host_copy(opt_v, (size_t)batch, ho))) return rc;
        for (int b = 0; b < batch; b++)
            if (ho[b] != 0 && ho[b] != 1) return fail(TD_EINVAL, "%s: optimal[%d] = %d, neither 0 nor 1", fn, b, ho[b]);
        if ((rc = to_device(opt_v, sizeof(int32_t) * (size_t)batch, g_in[4], &d_optv))) return rc;
    }
    if (ml_v && (rc = to_device(ml_v, sizeof(double) * (size_t)batch, g_in[5], &d_mlv))) return rc;
    const bool run_match = opt_v || optimal, run_greedy = opt_v || !optimal;
    if (dist && tot_c) {   // never index outside the table
        std::vector<int32_t> hf, ht;
        if ((rc = host_copy(from, tot_c, hf)) || (rc = host_copy(to, tot_c, ht))) return rc;
        for (size_t i = 0; i < tot_c; i++)
            if ((uint32_t)hf[i] >= (uint32_t)S || (uint32_t)ht[i] >= (uint32_t)S)
                return fail(TD_EINVAL, "%s: customer %zu's stands (%d -> %d) lie outside the %d x %d distance table", fn, i, hf[i], ht[i],
                            S, S);
    }
    const void *d_off, *d_from = nullptr, *d_to = nullptr, *d_dist = nullptr;
    if ((rc = to_device(is_device_ptr(off) ? (const void *)off : (const void *)h_off.data(), sizeof(int32_t) * ((size_t)batch + 1), g_in[0],
                        &d_off)))
        return rc;
    if (tot_c) {
        if ((rc = to_device(from, sizeof(int32_t) * tot_c, g_in[1], &d_from))) return rc;
        if ((rc = to_device(to, sizeof(int32_t) * tot_c, g_in[2], &d_to))) return rc;
    }
    if (dist && (rc = to_device(dist, sizeof(int32_t) * (size_t)S * S, g_in[3], &d_dist))) return rc;
    const size_t B = (size_t)batch, H = (size_t)(n / 2);
    Out o[6] = {{cust_a, sizeof(int32_t) * B * H}, {cust_b, sizeof(int32_t) * B * H}, {plan, sizeof(int32_t) * B * H},
                {cost, sizeof(int32_t) * B * H},   {n_pools, sizeof(int32_t) * B},    {total, sizeof(int64_t) * B}};
    int *d_err;
    if ((rc = outputs_prepare(g_res, o, 6, &d_err))) return rc;
    // models in chunks whose pair-cost slabs take at most 256 MiB
    const size_t NN = std::max<size_t>((size_t)n * n, 1);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(B, ((size_t)256 << 20) / (sizeof(int32_t) * NN)));
    const size_t Q = (size_t)chunk, Hs = std::max<size_t>(H, 1);
    int32_t *pc, *d_ns, *d_nsm, *d_mate, *d_rows, *d_cols, *d_np;
    int64_t *d_K, *d_tot;
    if ((rc = carve_buf(g_pool, [&](Carve &c) {
            pc = c.take<int32_t>(Q * NN);
            d_ns = c.take<int32_t>(Q);    // sizes as the greedy sees them
            d_nsm = c.take<int32_t>(Q);   // sizes as k_pool_match sees them
            d_K = c.take<int64_t>(Q);
            d_mate = c.take<int32_t>(Q * (size_t)std::max(n, 1));
            d_tot = c.take<int64_t>(Q);
            d_rows = c.take<int32_t>(Q * Hs);
            d_cols = c.take<int32_t>(Q * Hs);
            d_np = c.take<int32_t>(Q);
        })))
        return rc;
    bool lds = false;
    unsigned char *ws = nullptr;
    size_t per = 0;
    int mgrid = 0;
    if (run_match && (rc = state_plan(chunk, nmax, &lds, &ws, &per, &mgrid))) return rc;
    const size_t shm_fin = sizeof(int32_t) * 3 * (H + 1);
    int64_t path = TD_MP_POOL | (opt_v ? TD_MP_PER_MODEL : 0) | (run_greedy ? TD_MP_GREEDY : 0);
    if (run_match) path |= TD_MP_MATCH | (lds ? TD_MP_LDS : TD_MP_WS);
    int64_t chunks = 0;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        chunks++;
        const int nq = std::min(chunk, batch - b0);
        const int grid = std::min(nq, 1 << 20);
        k_pool_costs<<<grid, 256, 0, c.stream>>>(nq, b0, n, optimal, (const int32_t *)d_optv, (const int32_t *)d_off, (const int32_t *)d_from,
                                                 (const int32_t *)d_to, (const int32_t *)d_dist, S, max_loss, (const double *)d_mlv, pc, d_ns,
                                                 d_nsm, d_K, d_err);
        if (run_match) {
            const int g = std::min(nq, mgrid);
            if (lds) {
                lds_allow(k_pool_match<true>, per);
                k_pool_match<true><<<g, 64, per, c.stream>>>(nq, n, d_nsm, pc, d_K, ws, per, d_mate, d_tot, d_err);
            } else {
                k_pool_match<false><<<g, 64, 0, c.stream>>>(nq, n, d_nsm, pc, d_K, ws, per, d_mate, d_tot, d_err);
            }
        }
        if (run_greedy) pool2_greedy_launch(nq, n, d_ns, pc, d_rows, d_cols, d_np);
        k_pool_finish<<<grid, 64, shm_fin, c.stream>>>(nq, b0, n, optimal, (const int32_t *)d_optv, (const int32_t *)d_off, (const int32_t *)d_from,
                                                        (const int32_t *)d_to, (const int32_t *)d_dist, S, pc, d_mate, d_rows, d_cols, d_np,
                                                        (int32_t *)o[0].dptr(), (int32_t *)o[1].dptr(), (int32_t *)o[2].dptr(),
                                                        (int32_t *)o[3].dptr(), (int32_t *)o[4].dptr(), (int64_t *)o[5].dptr());
    }
    c.stats[14] = path | std::min<int64_t>(chunks, TD_MP_CHUNK_MAX) << TD_MP_CHUNK_SHIFT;
    return match_finish(fn, o, 6, d_err);
}

}  // namespace

extern "C" {

int td_pool2_batched(int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to, const int32_t *dist, int S,
                     double max_loss, int optimal, int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n_pools,
                     int64_t *total)
{
    TD_REQUIRE_INIT();
    return pool2_batched_impl("td_pool2_batched", batch, n, off, from, to, dist, S, max_loss, optimal, nullptr, nullptr, cust_a, cust_b, plan,
                              cost, n_pools, total);
}

int td_pool2_batched_v(int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to, const int32_t *dist, int S,
                       const double *max_loss, const int32_t *optimal, int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost,
                       int32_t *n_pools, int64_t *total)
{
    TD_REQUIRE_INIT();
    return pool2_batched_impl("td_pool2_batched_v", batch, n, off, from, to, dist, S, 0.0, 0, max_loss, optimal, cust_a, cust_b, plan, cost,
                              n_pools, total);
}

}  // extern "C"

void td::match_release_workspace()
{
    Buf *bs[] = {&g_ws, &g_res, &g_pool, &g_in[0], &g_in[1], &g_in[2], &g_in[3], &g_in[4], &g_in[5]};
    for (Buf *b : bs) buf_free(*b);
}
