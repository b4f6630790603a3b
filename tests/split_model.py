"""Host restatement of split.py:61-119 and the checker of td_split_batched's outputs.

Which cab of a region sits on a dummy column is the solver's choice among equal optima, and the rest lists (hence the
fifth solve and the total) follow from that choice.  So a total cannot be compared with an independent run; the checker
takes the outputs of ONE case and verifies every step of them against optima computed here (`opt`: the oracle by default,
brute force in the CPU tests): what a region serves is unique in its SUM whatever ties are broken, the rest lists follow
from the served pairs by the side rule, and the fifth solve is again unique in its sum given those lists.
"""
import itertools

import numpy as np

from oracle import oracle

FILL = 250000


def ranges(size, parts):
    """split.py:69-72,106: split_size = size / parts, a range per start < size (the last may reach past size)"""
    ss = size // parts
    assert ss >= 1
    return [(start, start + ss) for start in range(0, size, ss)]


def cell(dist, a, b):
    return abs(int(a) - int(b)) if dist is None else int(dist[int(a)][int(b)])


def padded(cab, dem, dist, fill):
    """calculate_cost (split.py:123-136): the square model, dummy rows / columns hold fill"""
    n = max(len(cab), len(dem))
    c = np.full((n, n), fill, np.int64)
    for i, a in enumerate(cab):
        for j, b in enumerate(dem):
            c[i, j] = cell(dist, a, b)
    return c


def opt_oracle(cab, dem, dist, fill):
    """the optimum of the lists' model over real cells: the padded optimum less its |n_s - n_d| dummy cells"""
    if len(cab) == 0 or len(dem) == 0:
        return 0
    return int(oracle.assign(padded(cab, dem, dist, fill))[0]) - abs(len(cab) - len(dem)) * fill


def opt_brute(cab, dem, dist, fill):
    """the same by enumeration: the cheapest way to match all of the smaller side into the larger"""
    if len(cab) == 0 or len(dem) == 0:
        return 0
    if len(cab) <= len(dem):
        return min(sum(cell(dist, a, dem[j]) for a, j in zip(cab, p)) for p in itertools.permutations(range(len(dem)), len(cab)))
    return min(sum(cell(dist, cab[i], b) for b, i in zip(dem, p)) for p in itertools.permutations(range(len(cab)), len(dem)))


def solve_split_host(cab, dem, size, parts=4, dist=None, fill=FILL):
    """split.py:61-119 with the oracle as the solver; returns td_split_batched's outputs for the case"""
    cab, dem = [int(x) for x in cab], [int(x) for x in dem]
    ns, nd = len(cab), len(dem)
    req, stage = [-1] * ns, [-1] * ns
    if ns == 0 or nd == 0:
        return {"cab_req": req, "cab_stage": stage, "total": 0, "rest_total": 0, "n_rest": (0, 0), "dual_gap": 0}
    rest_c, rest_d, total = [], [], 0
    for lo, hi in ranges(size, parts):
        ci = [i for i in range(ns) if lo <= cab[i] < hi]
        dj = [j for j in range(nd) if lo <= dem[j] < hi]
        if ci and dj:
            c = padded([cab[i] for i in ci], [dem[j] for j in dj], dist, fill)
            r2c = oracle.assign(c)[1]
            for t, j in enumerate(r2c):
                if t < len(ci) and j < len(dj):
                    req[ci[t]], stage[ci[t]] = dj[j], 0
                    total += int(c[t, j])
                elif len(ci) > len(dj):
                    rest_c.append(ci[t])
                else:
                    rest_d.append(dj[j])
        elif dj:
            rest_d += dj
        else:
            rest_c += ci
    rest_c.sort()   # filter(cabs, rest_cabs, 0, ...) keeps the case's order
    rest_d.sort()
    rest_total = 0
    if rest_c and rest_d:
        c = padded([cab[i] for i in rest_c], [dem[j] for j in rest_d], dist, fill)
        for t, j in enumerate(oracle.assign(c)[1]):
            if t < len(rest_c) and j < len(rest_d):
                req[rest_c[t]], stage[rest_c[t]] = rest_d[j], 1
                rest_total += int(c[t, j])
    return {"cab_req": req, "cab_stage": stage, "total": total + rest_total, "rest_total": rest_total,
            "n_rest": (len(rest_c), len(rest_d)), "dual_gap": 0}


def check_case(cab, dem, size, parts, dist, fill, out, opt=opt_oracle):
    """verifies one case's outputs (a dict as solve_split_host returns); raises AssertionError naming the step"""
    cab, dem = [int(x) for x in cab], [int(x) for x in dem]
    ns, nd = len(cab), len(dem)
    req, stage = [int(x) for x in out["cab_req"]], [int(x) for x in out["cab_stage"]]
    n_rest = tuple(int(x) for x in out["n_rest"])
    assert len(req) == ns and len(stage) == ns
    if ns == 0 or nd == 0:
        assert all(r == -1 for r in req) and all(s == -1 for s in stage), "empty case: somebody is served"
        assert (int(out["total"]), int(out["rest_total"]), n_rest, int(out["dual_gap"])) == (0, 0, (0, 0), 0), "empty case: sums"
        return
    # 1. a partial matching
    served = [r for r in req if r != -1]
    assert all(0 <= r < nd for r in served), "1: a request index outside the case"
    assert len(set(served)) == len(served), "1: a request served twice"
    assert all((s == -1) == (r == -1) and s in (-1, 0, 1) for r, s in zip(req, stage)), "1: stage and request disagree"
    # 2. per region
    rs = ranges(size, parts)
    rng_of = lambda p: p // (size // parts)
    assert all(0 <= rng_of(p) < len(rs) for p in cab + dem)
    for r in range(len(rs)):
        ci = [i for i in range(ns) if rng_of(cab[i]) == r]
        dj = [j for j in range(nd) if rng_of(dem[j]) == r]
        pairs = [(i, req[i]) for i in ci if stage[i] == 0]
        assert all(rng_of(dem[j]) == r for _, j in pairs), "2: a stage-0 pair leaves region %d" % r
        assert len(pairs) == min(len(ci), len(dj)), "2: region %d serves %d of its smaller side %d" % (r, len(pairs), min(len(ci), len(dj)))
        got = sum(cell(dist, cab[i], dem[j]) for i, j in pairs)
        want = opt([cab[i] for i in ci], [dem[j] for j in dj], dist, fill)
        assert got == want, "2: region %d sums %d, optimum %d" % (r, got, want)
    # 3. the rest lists, by the side rule, in the case's order
    taken0 = {req[i] for i in range(ns) if stage[i] == 0}
    rest_c = [i for i in range(ns) if stage[i] != 0]
    rest_d = [j for j in range(nd) if j not in taken0]
    assert n_rest == (len(rest_c), len(rest_d)), "3: n_rest %s, derived %s" % (n_rest, (len(rest_c), len(rest_d)))
    # 4. the fifth solve
    pairs1 = [(i, req[i]) for i in range(ns) if stage[i] == 1]
    assert all(j in set(rest_d) for _, j in pairs1), "4: a stage-1 request is not in the rest list"
    assert len(pairs1) == min(len(rest_c), len(rest_d)), "4: the fifth solve leaves part of its smaller side unserved"
    got1 = sum(cell(dist, cab[i], dem[j]) for i, j in pairs1)
    want1 = opt([cab[i] for i in rest_c], [dem[j] for j in rest_d], dist, fill)
    assert got1 == want1, "4: the fifth solve sums %d, optimum %d" % (got1, want1)
    assert int(out["rest_total"]) == got1, "4: rest_total %d, pairs sum %d" % (int(out["rest_total"]), got1)
    # 5. the total
    all_sum = sum(cell(dist, cab[i], dem[req[i]]) for i in range(ns) if req[i] != -1)
    assert int(out["total"]) == all_sum, "5: total %d, served distances %d" % (int(out["total"]), all_sum)
    # 6. every model certified
    assert int(out["dual_gap"]) == 0, "6: dual_gap %d" % int(out["dual_gap"])


def case_of(res, cabs, c):
    """case c of split_batched's dict"""
    lo, hi = int(res["cab_off"][c]), int(res["cab_off"][c + 1])
    assert hi - lo == len(cabs[c])
    return {"cab_req": res["cab_req"][lo:hi], "cab_stage": res["cab_stage"][lo:hi], "total": res["total"][c],
            "rest_total": res["rest_total"][c], "n_rest": res["n_rest"][c], "dual_gap": res["dual_gap"][c]}


def check_batch(cabs, dems, size, parts, dist, fill, res, opt=opt_oracle):
    assert len(res["total"]) == len(cabs) == len(dems)
    for c in range(len(cabs)):
        check_case(cabs[c], dems[c], size, parts, dist, fill, case_of(res, cabs, c), opt)
