"""td_pool_n_banded without a GPU: the host restatement of its band loop (pool_band_model.py) against oracle.pool_n on the
inputs the GPU tests use, the cut level it predicts for each of them by name, and the Python surface of the new calls."""
import re

import numpy as np
import pytest

import pool_band_model as M
import test_abi
from oracle import oracle

# (input, k, buffer kind) -> the deepest level a band is cut at.  "min": 24 n; "quarter": max(24 n, happy // 4); "default": 2^22.
# same12 is worked out by hand in DESIGN.md 3.16: with k = 4 every plan costs 0 and one first, one second pick-up still hold
# 23 760 and 2 160 plans, one third pick-up 216 <= 288, so the first band is cut at level 3; with k = 3 one second pick-up holds
# 60; with k = 2 all 264 plans fit.  The random inputs' levels are the model's: a band rule that never descends fails r24 / r40 /
# r64 at k = 4 and same12 at k = 3 and 4.
DEEPEST = {
    ("same12", 2, "min"): 0, ("same12", 3, "min"): 2, ("same12", 4, "min"): 3,
    ("same12", 2, "quarter"): 0, ("same12", 3, "quarter"): 1, ("same12", 4, "quarter"): 1,
    ("r24", 2, "min"): 0, ("r24", 3, "min"): 0, ("r24", 4, "min"): 1,
    ("r40", 2, "min"): 0, ("r40", 3, "min"): 0, ("r40", 4, "min"): 1,
    ("r64", 2, "min"): 0, ("r64", 3, "min"): 0, ("r64", 4, "min"): 1,
}
# the oracle's counts of the issue: happy plans and pools at k = 4, and the same-stand model's at every k
HAPPY4 = {"r24": (49382, 5), "r40": (30620, 9), "r64": (45131, 13)}
SAME = {2: (264, 6), 3: (7920, 4), 4: (285120, 3)}


def buffers(n, happy):
    return {"min": 24 * n, "quarter": max(24 * n, happy // 4), "default": 0}


@pytest.fixture(scope="module")
def plans():
    """(name, k) -> (n, the happy plans in key order, the oracle's records and happy count), computed once"""
    oracle.build()
    out = {}
    for name, (d, dist) in M.inputs().items():
        for k in (2, 3, 4):
            exp, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], dist, cap=400000)
            out[name, k] = (len(d), M.happy_plans(k, d, dist), exp.tolist(), nh)
    return out


def test_the_enumeration_is_the_oracles(plans):
    for (name, k), (n, (cost, p, qi), exp, nh) in plans.items():
        assert cost.size == nh, (name, k)
        assert M.scan_all(k, cost, p, qi) == exp, (name, k)
    for name, want in HAPPY4.items():
        assert (plans[name, 4][3], len(plans[name, 4][2])) == want
    for k, want in SAME.items():
        assert (plans["same12", k][3], len(plans["same12", k][2])) == want


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("name", ["same12", "r24", "r40", "r64"])
def test_the_banded_scan_equals_the_oracle(plans, name, k):
    n, (cost, p, qi), exp, nh = plans[name, k]
    for kind, room in buffers(n, nh).items():
        recs, happy, (bands, passes, deepest, most) = M.banded(k, n, cost, p, qi, room)
        assert recs == exp and happy == nh, (name, k, kind)
        assert most <= (room or M.DEFAULT_BUFFER) and bands >= 1 and passes >= 2 * bands
        if kind == "default":
            assert (bands, passes, deepest, most) == (1, 2, 0, nh)
        if (name, k, kind) in DEEPEST:
            assert deepest == DEEPEST[name, k, kind], (name, k, kind)
        if kind == "quarter" and name != "same12" and k > 2:      # cost bands only, and more than one
            assert deepest == 0 and bands >= 2, (name, k, bands)
        if kind == "quarter" and k == 2:      # 24 n is above the whole list of pairs: the smallest legal buffer holds it
            assert nh <= 24 * n and bands == 1


def test_the_same_stand_model_is_cut_at_the_third_pick_up(plans):
    n, (cost, p, qi), exp, nh = plans["same12", 4]
    recs, happy, stats = M.banded(4, n, cost, p, qi, 288)
    assert [r[:4] for r in recs] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]] and happy == 285120
    assert stats[0] == 3 and stats[2] == 3 and stats[3] <= 288
    with pytest.raises(AssertionError):
        M.banded(4, n, cost, p, qi, 287)


def test_slice_table_and_max_pools(plans):
    d = M.inputs()["r64"][0]
    n = len(d)
    for k in (2, 3, 4):
        cost, p, qi = M.happy_plans(k, d, None, n // 3, 2 * n // 3)
        exp, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], None, n // 3, 2 * n // 3, cap=400000)
        recs, happy, _ = M.banded(k, n, cost, p, qi, 24 * n)
        assert recs == exp.tolist() and happy == nh
        assert M.banded(k, n, cost, p, qi, 24 * n, max_pools=2)[0] == exp.tolist()[:2]
        dt, dist = M.table_case(k)
        cost, p, qi = M.happy_plans(k, dt, dist)
        exp, nh = oracle.pool_n(k, dt[:, 1], dt[:, 2], dt[:, 3], dt[:, 4], dist, cap=400000)
        recs, happy, _ = M.banded(k, len(dt), cost, p, qi, 24 * len(dt))
        assert recs == exp.tolist() and happy == nh


# ---- the surface -------------------------------------------------------------------------------------------------------------------
def test_the_prototypes_match_the_header():
    import ctypes
    from taxidispatcher_amd import _ffi
    hdr = open(test_abi.HEADER).read()
    m = re.search(r"TD_API\s+int\s+td_pool_n_banded\s*\(([^;]*)\)\s*;", hdr)
    assert m, "td_pool_n_banded is not declared"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    res, types = _ffi.SIGNATURES["td_pool_n_banded"]
    assert res is ctypes.c_int and len(types) == len(args) == 16
    assert "int64_t plan_buffer" in args[10] and "stats" in args[15]
    assert types[10] is ctypes.c_int64 and types[11] is ctypes.c_int
    m = re.search(r"TD_API\s+int\s+td_sim_pool_buffer\s*\(([^;]*)\)\s*;", hdr)
    assert m and "int64_t plan_buffer" in m.group(1)
    assert _ffi.SIGNATURES["td_sim_pool_buffer"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64])


def test_the_source_is_built_and_exported():
    import __graft_entry__ as entry
    entry.build()
    from taxidispatcher_amd import _ffi, build
    assert any(s.endswith("td_pool_band.hip") for s in build.SRC)
    lib = _ffi.load()
    assert lib.td_pool_n_banded is not None and lib.td_sim_pool_buffer is not None
    import taxidispatcher_amd as td
    assert callable(td.find_pool_n_banded)


def test_pool_buffer_values():
    from taxidispatcher_amd import simulator
    assert simulator.POOL_BUFFER_MIN == 24 * 2047
    assert simulator.pool_buffer_size(0) == 0 and simulator.pool_buffer_size(24 * 2047) == 24 * 2047
    for bad in (-1, 1, 24 * 2047 - 1, 1.5, "1", None, True):
        with pytest.raises(ValueError):
            simulator.pool_buffer_size(bad)
    with pytest.raises(ValueError):
        simulator.HipBackend(pool_buffer=100)


def test_the_backend_routes_every_stage_through_the_banded_call():
    from taxidispatcher_amd import simulator
    calls = []

    class D:
        POOL_N_BATCHED_NMAX = 512

        def find_pool_n_banded(self, k, rows, dist, plan_buffer=0):
            calls.append(("banded", k, len(rows), plan_buffer))
            return np.zeros((0, 2 * k + 1), np.int32), 7, (0, 1, 0, 0)

        def pool_n_batched(self, k, demands, dist, max_happy=0):
            calls.append(("batched", k, len(demands[0]), max_happy))
            return [np.zeros((0, 2 * k + 1), np.int32)], [3]

    be = simulator.HipBackend(pool_buffer=24 * 2047)
    be.d = D()
    z = np.zeros(5, np.int32)
    recs, nh = be.find_pool_n(3, z, z, z, z)
    assert nh == 7 and recs.shape == (0, 7) and calls == [("banded", 3, 5, 24 * 2047)]
    be.pool_buffer = 0
    assert be.find_pool_n(3, z, z, z, z)[1] == 3 and calls[-1][0] == "batched"
