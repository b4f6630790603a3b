"""The case generators of tests/pool_edge_cases.py without a GPU: every generator runs (each asserts that its cases reach
the condition they are named for), the oracle and the pure Python restatement of pool_n.c's happiness rule agree on every
case of the sweep, and the merge comparator equals findpool.c's restatement on the committed fixtures."""
import numpy as np
import pytest

import pool_edge_cases as pe
import pool_fixtures as pf

KS = [2, 3, 4]


@pytest.mark.parametrize("k", KS)
def test_happy_ties_oracle_equals_python_rule(k):
    cases = pe.happy_ties(k)
    assert len({c.name for c in cases}) == len(cases) >= 2 * len(pe.integer_pairs(60, 100))
    fewer = set()
    for c in cases:
        nh = pe.reference(c)[1]
        assert nh == pe.py_happy_count(c), c.name
        i = c.info
        if not pe.happy_rule(i["T"], i["direct"], i["loss_x"]) and i["T"] in i["want"]:
            # the plans in which X rides exactly T: unhappy for the oracle, happy in exact arithmetic
            assert pe.py_happy_count(c, pe.happy_rule_exact) > nh, c.name
            fewer.add((i["direct"], i["loss_x"]))
    assert set(pe.KNOWN_MISROUNDED) <= fewer


def test_happiness_rule_known_pairs():
    for (d, l), T in pe.KNOWN_MISROUNDED.items():
        assert d * (1 + l / 100.0) < T == d * (100 + l) // 100
        assert [pe.happy_rule(c, d, l) for c in (T - 1, T, T + 1)] == [True, False, False]
        assert [pe.happy_rule_exact(c, d, l) for c in (T - 1, T, T + 1)] == [True, True, False]
    assert pe.happy_rule(30, 25, 20) and pe.happy_rule_exact(30, 25, 20)     # an integer product the double meets exactly


@pytest.mark.parametrize("k", KS)
def test_wait_edges(k):
    cases = pe.wait_edges(k)
    names = {c.name for c in cases}
    for level in range(1, k):
        assert {"wait_l%d_%s_%s" % (level, m, v) for m in ("line", "table") for v in ("equal", "longer")} <= names
    assert {"wait0_one_stand", "wait_negative"} <= names


@pytest.mark.parametrize("k", KS)
def test_grid_edges(k):
    cases = pe.grid_edges(k)
    assert [int(c.frm.size) for c in cases] == [255, 256, 257, k, k - 1]


@pytest.mark.parametrize("k", KS)
def test_top_of_key(k):
    (c,) = pe.top_of_key(k)
    assert c.frm.size == pe.PN_MAXN == 2047 and (c.first0, c.first1) == (2040, 2047)
    assert {0, 1, 1023, 1024} | set(range(2040, 2047)) <= set(c.info["cluster"])
    # a filler can never follow a cluster member: its WAIT is 0 and it stands at least 51 stands away
    filler = np.setdiff1d(np.arange(c.frm.size), c.info["cluster"])
    assert (c.wait[filler] == 0).all() and c.frm[filler].max() < 50 and (c.frm[c.info["cluster"]] == 100).all()


def test_cost_limit():
    fits, too_large = pe.cost_limit()
    assert pe.reference(fits)[0][-1][-1] == pe.PN_MAXCOST and pe.reference(too_large)[0][-1][-1] == pe.PN_MAXCOST + 1


@pytest.mark.parametrize("k", KS)
def test_merge_cases(k):
    cases = pe.merge_cases(k)
    sizes = {c.recs.shape[0] for c in cases}
    assert set(pe.MERGE_SIZES) <= sizes
    for kind in ("chain", "dense", "sparse"):
        for n_in in pe.MERGE_SIZES:
            assert {"%s_%d_s%d" % (kind, n_in, s) for s in (0, 1)} <= {c.name for c in cases}
    for _, rec, bad, recs in pe.bad_id_inputs(k):
        ids = recs[:, :k]
        wrong = np.argwhere((ids < 0) | (ids >= pe.PN_MAXN))
        assert recs.shape[0] == pe.CHUNK + 1 and wrong.shape[0] == 1 and wrong[0, 0] == rec and ids[tuple(wrong[0])] == bad


def test_merge_scan_equals_restatement_on_fixtures():
    seen = 0
    for name, k in pf.cases():
        _, exp = pf.load(name, k)
        lists = [exp[c] for c in range(8)]
        allp = [r for lst in lists for r in lst]
        if not allp:
            continue
        seen += 1
        assert pe.merge_scan(k, allp, 1 if k == 4 else 0, len(allp))[0] == pf.merge_restatement(k, lists), (name, k)
    assert seen >= 3


def test_merge_scan_sorts_for_every_k():
    """what pool_fixtures.merge_restatement does not do: a stable sort by the last field for k = 2 and 3 as well"""
    for k in KS:
        recs = np.array([list(range(j * k, j * k + k)) * 2 + [c] for j, c in enumerate((5, 3, 5, 3, 0))])
        kept, pos = pe.merge_scan(k, recs, 1, 10)
        assert [r[-1] for r in kept] == [0, 3, 3, 5, 5] and [r[0] // k for r in kept] == [4, 1, 3, 0, 2] and pos == list(range(5))
        assert [r[0] // k for r in pe.merge_scan(k, recs, 0, 3)[0]] == [0, 1, 2]
