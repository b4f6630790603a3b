"""The case generators of tests/pool_band_cases.py without a GPU: every generator runs (each asserts from the band trace that its
cases reach the condition they are named for), the host model's records equal oracle.pool_n's on every case, the cut table of
the same-stand models is asserted value by value, and the trace itself is checked against the plan list."""
import numpy as np
import pytest

import pool_band_cases as pc
import pool_band_model as M

KS = [2, 3, 4]


def names():
    return ["cut_relations", "k2_bands", "slice_deep_cut"] + ["%s_k%d" % (g, k) for k in KS for g in
                                                              ("bitmap_edges", "grid_edges_banded", "top_band", "greedy_chunks", "max_pools_edges")]


def cases_of(name):
    if name[-3:-1] == "_k" and name[:-3] in ("bitmap_edges", "grid_edges_banded", "top_band", "greedy_chunks", "max_pools_edges"):
        return getattr(pc, name[:-3])(int(name[-1]))
    return getattr(pc, name)()


@pytest.mark.parametrize("name", names())
def test_generator_and_model_against_the_oracle(name):
    cases = cases_of(name)
    assert cases and len({c.name for c in cases}) == len(cases)
    for bc in cases:
        s = pc.solve(bc)      # asserts inside: the model's records are the oracle's first max_pools, its happy count the oracle's
        n, k = int(bc.case.frm.size), bc.case.k
        assert s.recs == s.exp and s.nh == s.plans[0].size
        assert bc.room >= 24 * n and s.stats[3] <= bc.room and s.stats[0] == len(s.trace)
        # the trace against the plan list: consecutive intervals, the expected keys, the kept plans are the records
        cost, p, qi = s.plans
        kept, lo = [], 0
        for t in s.trace:
            assert t["lo"] == lo < t["hi"] and t["expect"] == len(t["rows"]) <= bc.room and len(t["first_bins"]) == t["level"] + 1
            assert all(b > bc.room for b in t["first_bins"][:-1]) and t["first_bins"][-1] <= t["expect"]
            assert t["kept"] == sorted(t["kept"]) and (not t["kept"] or t["kept"][0] == 0) and len(t["kills_later"]) == len(t["kept"])
            kept += [p[t["rows"][at], :k].tolist() for at in t["kept"]]
            lo = t["hi"]
        assert kept == [r[:k] for r in s.recs]


def test_the_cut_table_value_by_value():
    by = {c.name: c for c in pc.cut_relations()}
    want = {
        (14, 2, 364): (1, 2, 0, 364), (14, 2, 363): (1, 4, 1, 338), (14, 2, 336): (2, 5, 1, 312),
        (12, 3, 7920): (1, 2, 0, 7920), (12, 3, 7919): (1, 4, 1, 7260), (12, 3, 660): (3, 10, 1, 660), (12, 3, 659): (3, 11, 2, 600),
        (12, 4, 23760): (3, 8, 1, 23760), (12, 4, 23759): (3, 9, 2, 21600), (12, 4, 2160): (3, 10, 2, 2160),
        (12, 4, 2159): (3, 11, 3, 1944),
    }
    assert want == pc.CUT_TABLE
    for (n, k, room), stats in want.items():
        bc = by["same%d_k%d_room%d" % (n, k, room)]
        assert bc.room == room and int(bc.case.frm.size) == n and bc.case.k == k
        assert pc.solve(bc).stats == stats, (n, k, room)
    assert pc.solve(by["same14_k2_room336"]).nh == 364 and 336 == 24 * 14


def test_the_cluster_counts():
    """the building block: m! / (m - k)! * k! plans at cost 0 (285 120 and 7 920 for 12 of 66), and the dear members' rule"""
    for k, want in ((4, 285120), (3, 7920)):
        cost, p, qi, exp, nh = pc.plans(pc.cluster(66, range(20, 32), k))
        assert nh == want and not cost.any() and set(np.unique(p[:, :k]).tolist()) == set(range(20, 32))
    for k in KS:
        c = pc.cluster(12, range(8), k, dear=(1, 6))
        cost, p, qi, exp, nh = pc.plans(c)
        has_dear = np.isin(p[:, :k], (1, 6)).any(axis=1)
        assert (cost == has_dear).all() and nh > 0
        # a dear member is never dropped before a plain one: 2 plain and j dear members bring j! * (k - j)! drop-off orders
        sets = {}
        for row in p[:, :k].tolist():
            sets[tuple(row)] = sets.get(tuple(row), 0) + 1
        for row, count in sets.items():
            j = len(set(row) & {1, 6})
            assert count == pc._perm(j, j) * pc._perm(k - j, k - j), (row, count)


@pytest.mark.parametrize("k", KS)
def test_the_chunk_conditions_by_name(k):
    got = pc.chunk_conditions(pc.greedy_chunks(k))
    assert got == pc.ALL_CHUNK_CONDITIONS - pc.NOT_REACHED[k]
    assert pc.NOT_REACHED[2] == pc.NOT_REACHED[3] == set() and pc.NOT_REACHED[4] == {"band of 1024", "kept at 1023"}
    assert pc.CHUNK == 1024


def test_the_trace_is_optional_and_changes_nothing():
    d = M.same_stand(12)
    cost, p, qi = M.happy_plans(3, d)
    trace = []
    assert M.banded(3, 12, cost, p, qi, 660) == M.banded(3, 12, cost, p, qi, 660, trace=trace)
    assert len(trace) == 3 and [t["level"] for t in trace][0] == 1 and trace[0]["expect"] == 660 == trace[0]["first_bins"][1]
    assert [sorted(t) for t in trace][0] == sorted(["lo", "hi", "level", "expect", "first_bins", "prefix", "kept", "kills_later", "rows"])
