// td_pool_core.h — what td_pool_n (td_pool.hip), td_pool_n_banded (td_pool_band.hip) and td_pool_n_batched (td_pool_batch.hip) share: the plan key, the k!
// drop-off orders, the distance and the happiness / cost test of pool_n.c:101-153.  One definition, so both calls answer alike.
//
//   key = cost << 50 | sequence number;  sequence number = (((p0 * n + p1) * n + p2) * n + p3) * 24 + drop-off order, the
//   plan's position in the reference's enumeration (unused pick-up slots are 0, n = the model's size): ascending keys ARE
//   the reference's stable sort by cost, and the key alone names the plan.
#pragma once
#include "td_common.h"

namespace td {

constexpr int PN_MAXN = 2047;          // 4 * 11 bits + 5 bits of drop-off order < 2^50
constexpr int PN_SEQ_BITS = 50;
constexpr unsigned long long PN_SEQ_MASK = (1ull << PN_SEQ_BITS) - 1ull;
constexpr int PN_MAXCOST = (1 << 14) - 1;

// the k! drop-off orders in lexicographic order (the recursion order of pool_n.c:140-153), 2 bits per slot
__host__ __device__ constexpr int pn_perm(int k, int qi, int *q)
{
    // generate the qi-th permutation of 0..k-1 in lexicographic order
    int avail[4] = {0, 1, 2, 3};
    int f = 1;
    for (int i = 2; i < k; i++) f *= i;   // (k-1)!
    int left = k;
    for (int i = 0; i < k; i++) {
        const int idx = qi / f;
        qi -= idx * f;
        q[i] = avail[idx];
        for (int j = idx; j < left - 1; j++) avail[j] = avail[j + 1];
        left--;
        if (left > 1) f /= left;
    }
    return 0;
}

// the same at compile time: a kernel that unrolls over the orders gets them as constants
struct PnOrder {
    int q[4];
};
constexpr PnOrder pn_order(int k, int qi)
{
    PnOrder o{{0, 0, 0, 0}};
    pn_perm(k, qi, o.q);
    return o;
}

// the pick-ups behind a key (radix n; the slots behind the pool's size decode to 0)
__device__ __forceinline__ void pn_key_requests(int n, unsigned long long key, int *c)
{
    unsigned long long s = (key & PN_SEQ_MASK) / 24ull;
    for (int i = 3; i >= 0; i--) {
        c[i] = (int)(s % (unsigned long long)n);
        s /= (unsigned long long)n;
    }
}

__device__ __forceinline__ int pn_d(const int32_t *dist, int S, int a, int b)
{
    return dist ? dist[(int64_t)a * S + b] : (a > b ? a - b : b - a);
}

// happiness of all passengers + plan cost for pick-ups p and drop-off order q
template <int K>
__device__ __forceinline__ bool pn_check(const int *p, const int *q, const int32_t *sf, const int32_t *st,
                                         const int32_t *sl, const int32_t *dist, int S, int *cost_out)
{
    int pick[K];   // pick[i] = d(from p[i], from p[i+1]); suffix sums give "rest of the pick-up path"
    int ptot = 0;
#pragma unroll
    for (int i = 0; i < K - 1; i++) {
        pick[i] = pn_d(dist, S, sf[p[i]], sf[p[i + 1]]);
        ptot += pick[i];
    }
    const int first = pn_d(dist, S, sf[p[K - 1]], st[p[q[0]]]);
    int drop = 0;
    bool happy = true;
#pragma unroll
    for (int d = 0; d < K; d++) {
        if (d > 0) drop += pn_d(dist, S, st[p[q[d - 1]]], st[p[q[d]]]);
        int c = first + drop;
#pragma unroll
        for (int ph = 0; ph < K - 1; ph++) c += (ph >= q[d]) ? pick[ph] : 0;
        const int x = p[q[d]];
        const double lim = (double)pn_d(dist, S, sf[x], st[x]) * (1 + sl[x] / 100.0);
        if ((double)c > lim) happy = false;
    }
    *cost_out = ptot + first + drop;
    return happy;
}

}  // namespace td
