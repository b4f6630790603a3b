"""Pooling policies of the simulator worlds (Simulator(pool=, max_loss=), td_sim_pooling / td_simb_pooling): the CPU
restatement of every policy and the checks a GPU test makes of plans that came from the device.  TEST INFRASTRUCTURE ONLY.

The candidate rule, the greedy and the matching weights are pool_opt_data's (pool_opt_min.py restated with numpy).  The
optimum of a model comes from exhaustive search over subsets for up to EXH_MAX customers and from networkx above that
(optimum()); both are CPU only and networkx is imported inside the one function that needs it, so a GPU test that
imports this module for its checks never needs it."""
import numpy as np

import pool_opt_data as po
import sim_backend

EXH_MAX = 16
POLICIES = [("none", None), ("greedy", 1.01), ("optimal", None), ("optimal", 1.01)]


def pair_best(c):
    """c of pair_costs -> (w, dir): w[i, j] = the cheaper candidate direction's cost of the pool {i, j} (-1: no candidate
    direction), a_first[i, j] = True when that direction picks i up first (the smaller custA on a tie)"""
    big = np.iinfo(np.int64).max
    x = np.where(c >= 0, c, big)
    w = np.minimum(x, x.T)
    return np.where(w == big, -1, w), x <= x.T


def exhaustive(c, want_pairs=False):
    """(count, total) of the lexicographic optimum by search over subsets: the lowest free customer stays alone or pools
    with a later free one; want_pairs: (count, total, the pools of one optimum as undirected pairs)"""
    w, _ = pair_best(c)
    m = c.shape[0]
    memo = {0: ((0, 0), -1)}

    def best(mask):
        if mask in memo:
            return memo[mask][0]
        i = (mask & -mask).bit_length() - 1
        rest = mask & ~(1 << i)
        out, pick = best(rest), -1
        r = rest
        while r:
            j = (r & -r).bit_length() - 1
            r &= r - 1
            if w[i, j] >= 0:
                k, t = best(rest & ~(1 << j))
                cand = (k + 1, t - int(w[i, j]))
                if cand > out:
                    out, pick = cand, j
        memo[mask] = (out, pick)
        return out
    full = (1 << m) - 1
    k, neg = best(full)
    if not want_pairs:
        return k, -neg
    pairs, mask = [], full
    while mask:
        i = (mask & -mask).bit_length() - 1
        j = memo[mask][1]
        mask &= ~(1 << i)
        if j >= 0:
            pairs.append((i, j))
            mask &= ~(1 << j)
    return k, -neg, pairs


def optimum(c):
    """the pools of one lexicographic optimum, as undirected pairs (i < j): exhaustive search up to EXH_MAX customers,
    networkx's max_weight_matching on lex_weights above"""
    m = c.shape[0]
    if m <= EXH_MAX:
        return sorted(exhaustive(c, True)[2])
    import networkx as nx
    _, W = po.lex_weights(c)
    g = nx.Graph()
    g.add_nodes_from(range(m))
    ew = np.maximum(W, W.T)
    for i, j in zip(*np.nonzero(np.triu(ew, 1) > 0)):
        g.add_edge(int(i), int(j), weight=int(ew[i, j]))
    return sorted(tuple(sorted(e)) for e in nx.max_weight_matching(g))


def listed(c, plan1, pairs):
    """undirected pools -> the plan list of the optimal policy: each pool in its cheaper candidate direction, ascending
    (cost, custA, custB); (custA, custB, plan, cost)"""
    w, a_first = pair_best(c)
    out = []
    for i, j in pairs:
        a, b = (i, j) if a_first[i, j] else (j, i)
        out.append((a, b, int(plan1[a, b]), int(w[i, j])))
    return sorted(out, key=lambda p: (p[3], p[0], p[1]))


def greedy_plans(c, plan1):
    return [(a, b, int(plan1[a, b]), cost) for a, b, cost in po.greedy(c)]


class PolicyBackend(sim_backend.OracleTickBackend):
    """the oracle's tick with find_pool under any policy, on the line; `calls` keeps per call (n, greedy plans, optimal
    plans or None) so that a test can compare the two on the SAME model"""

    def __init__(self, both=False):
        self.both = both
        self.calls = []

    def find_pool(self, frm, to, max_loss=None, optimal=False):
        c, plan1 = po.pair_costs(frm, to, None, max_loss)
        g = greedy_plans(c, plan1)
        o = listed(c, plan1, optimum(c)) if optimal or self.both else None
        self.calls.append((len(frm), g, o))
        return o if optimal else g


def check_plans(frm, to, max_loss, optimal, plans, certified_total=None):
    """plans that came from the device against the CPU: every plan a candidate with the right plan and cost, the plans
    disjoint; greedy: equal to the restatement; optimal: the stated order, and count * K - total equal to certified_total, the
    maximum matching weight of lex_weights that the caller established (a certified matching, or exhaustive search)"""
    c, plan1 = po.pair_costs(frm, to, None, max_loss)
    seen = set()
    for a, b, plan, cost in plans:
        assert 0 <= a < len(frm) and 0 <= b < len(frm) and a != b, (a, b)
        assert c[a, b] >= 0, ("not a candidate", a, b)
        assert cost == c[a, b] and plan == int(plan1[a, b]), (a, b, plan, cost, int(c[a, b]), int(plan1[a, b]))
        assert a not in seen and b not in seen, ("customer in two plans", a, b)
        seen.update((a, b))
    if not optimal:
        assert plans == greedy_plans(c, plan1)
        return
    w, a_first = pair_best(c)
    for a, b, _, cost in plans:
        assert cost == w[a, b] and (c[b, a] < 0 or c[a, b] < c[b, a] or (c[a, b] == c[b, a] and a < b)), ("direction", a, b)
    assert plans == sorted(plans, key=lambda p: (p[3], p[0], p[1])), "not in ascending (cost, custA, custB)"
    K, _ = po.lex_weights(c)
    assert len(plans) * K - sum(p[3] for p in plans) == certified_total, (len(plans), sum(p[3] for p in plans), K, certified_total)


def exhaustive_weight(c):
    """the maximum matching weight of lex_weights(c) by exhaustive search (models up to EXH_MAX)"""
    K, _ = po.lex_weights(c)
    k, t = exhaustive(c)
    return k * K - t
