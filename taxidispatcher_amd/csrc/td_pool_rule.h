// td_pool_rule.h — the candidate rule of a pool of two, defined ONCE: td_match.hip (td_pool2_batched, one workgroup per
// model) and td_lcm.hip (td_pool2_loss, one model spread over the device) both include it.
#pragma once
#include <stdint.h>

namespace td {

__device__ __forceinline__ int64_t pd(const int32_t *dist, int S, int a, int b)
{
    return dist ? (int64_t)dist[(int64_t)a * S + b] : (int64_t)(a > b ? a - b : b - a);
}

// pool_opt_min.py:56-64 for the ordered pair (A, B): cost1 / cost2, and whether the pair is a candidate (every pair is one
// when max_loss <= 0: Simulator.java:691).  The comparisons are made in double, as Python makes them.
__device__ __forceinline__ bool pool_pair(int af, int at, int bf, int bt, const int32_t *dist, int S, double max_loss, int64_t *c1,
                                          int64_t *c2)
{
    const int64_t ab = pd(dist, S, af, bf), bfat = pd(dist, S, bf, at), atbt = pd(dist, S, at, bt), bfbt = pd(dist, S, bf, bt),
                  btat = pd(dist, S, bt, at);
    *c1 = ab + bfat + atbt;
    *c2 = ab + bfbt + btat;
    if (max_loss <= 0) return true;
    const double aa = (double)pd(dist, S, af, at);
    const bool p1 = (double)(bfat + atbt) < (double)bfbt * max_loss && (double)(ab + bfat) < aa * max_loss;
    const bool p2 = (double)*c2 < aa * max_loss;
    return p1 || p2;
}

}  // namespace td
