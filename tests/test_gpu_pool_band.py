"""td_pool_n_banded on the GPU: its records against oracle.pool_n and td_pool_n, its stats against the host restatement of the
band loop (pool_band_model.py), the reference binary's fixtures through the smallest buffer, the refusal it removes, and the
contract of the C call."""
import ctypes

import numpy as np
import pytest

import pool_band_model as M
from pool_band_call import raw
import pool_fixtures as pf
from oracle import oracle

pytestmark = pytest.mark.gpu

TD_EINVAL = -1


def ffi():
    from taxidispatcher_amd import _ffi
    return _ffi


def err():
    return ffi().lib().td_last_error().decode()


@pytest.fixture(scope="module")
def cases():
    """(name, k) -> (demand, n, the oracle's records, its happy count, the happy plans in key order), computed once"""
    out = {}
    for name, (d, dist) in M.inputs().items():
        for k in (2, 3, 4):
            exp, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], dist, cap=400000)
            out[name, k] = (d, len(d), exp.tolist(), nh, M.happy_plans(k, d, dist))
    return out


# ---- the same-stand model: every plan is happy at cost 0, so the first band must be cut at the deepest level -------------------------
def test_same_stand_with_the_smallest_buffer(td, cases):
    d, n, exp, nh, _ = cases["same12", 4]
    recs, happy, stats = td.find_pool_n_banded(4, d, plan_buffer=288)
    assert (nh, len(exp)) == (285120, 3)
    assert recs[:, :4].tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]] and recs.tolist() == exp
    assert happy == 285120
    assert stats[0] == 3 and stats[2] == 3 and stats[3] <= 288, stats
    with pytest.raises(ffi().TdError) as e:
        td.find_pool_n_banded(4, d, plan_buffer=287)
    assert "287" in str(e.value) and "288" in str(e.value)


@pytest.mark.parametrize("k,counts,deepest", [(3, (7920, 4), 2), (2, (264, 6), 0)])
def test_same_stand_with_smaller_pools(td, cases, k, counts, deepest):
    d, n, exp, nh, (cost, p, qi) = cases["same12", k]
    assert (nh, len(exp)) == counts
    recs, happy, stats = td.find_pool_n_banded(k, d, plan_buffer=288)
    assert recs.tolist() == exp and happy == nh
    assert stats[2] == deepest and stats[3] <= 288
    assert stats == M.banded(k, n, cost, p, qi, 288)[2]
    with pytest.raises(ffi().TdError):
        td.find_pool_n_banded(k, d, plan_buffer=287)


# ---- random demands, three buffers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("name", ["r24", "r40", "r64"])
def test_random_demand_under_three_buffers(td, cases, name, k):
    """24 n: the smallest legal buffer (at k = 4 a cost level is cut); about a quarter of the happy plans: cost bands only, more
    than one; the default: one band.  With k = 2 the whole list is shorter than 24 n (at most 2 n (n - 1) pairs of which the wait
    rule leaves 392 / 510 / 796 here), so no legal buffer makes a second band: the model says one, and that is asserted."""
    d, n, exp, nh, (cost, p, qi) = cases[name, k]
    if k == 4:
        assert (nh, len(exp)) == {"r24": (49382, 5), "r40": (30620, 9), "r64": (45131, 13)}[name]
    ref, ref_happy = td.find_pool_n(k, d)
    assert ref.tolist() == exp and ref_happy == nh
    for kind, room in (("min", 24 * n), ("quarter", max(24 * n, nh // 4)), ("default", 0)):
        recs, happy, stats = td.find_pool_n_banded(k, d, plan_buffer=room)
        print(name, k, kind, room, stats)
        assert recs.tolist() == exp == ref.tolist() and happy == nh == ref_happy, (name, k, kind)
        assert stats[3] <= (room or 1 << 22), (kind, stats)
        assert stats == M.banded(k, n, cost, p, qi, room)[2], (name, k, kind)
        if kind == "min" and k == 4:
            assert stats[2] >= 1 and stats[0] >= 2, stats
        if kind == "quarter" and k > 2:
            assert stats[2] == 0 and stats[0] >= 2, stats
        if kind == "quarter" and k == 2:
            assert nh <= 24 * n and stats[0] == 1, stats
        if kind == "default":
            assert stats == (1, 2, 0, nh)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_a_first_pick_up_slice(td, cases, k):
    d, n = cases["r64", k][:2]
    first = (n // 3, 2 * n // 3)
    exp, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], None, first[0], first[1], cap=400000)
    cols = [np.ascontiguousarray(d[:, c].astype(np.int32)) for c in (1, 2, 3, 4)]
    got = raw(k, n, cols, None, first, 24 * n, n // k + 1)
    assert got["rc"] == 0 and got["recs"] == exp.tolist() and got["happy"] == nh
    cost, p, qi = M.happy_plans(k, d, None, *first)
    assert got["stats"] == M.banded(k, n, cost, p, qi, 24 * n)[2]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_an_asymmetric_table(td, k):
    d, dist = M.table_case(k)
    exp, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], dist, 0, 80, cap=3000000)
    ref, ref_happy = td.find_pool_n(k, d, dist)
    recs, happy, stats = td.find_pool_n_banded(k, d, dist, plan_buffer=24 * 80)
    assert recs.tolist() == exp.tolist() == ref.tolist() and happy == nh == ref_happy
    assert stats[3] <= 24 * 80 and (stats[0] >= 2 or nh <= 24 * 80)


def test_the_reference_fixtures_through_the_smallest_buffer(td):
    for name, k in pf.cases():
        d, exp = pf.load(name, k)
        for child in range(8):
            recs, _, stats = td.find_pool_n_banded(k, d, child=child, plan_buffer=24 * len(d))
            assert recs.tolist() == exp[child], (name, k, child)
            assert stats[3] <= 24 * len(d)


def test_the_refusal_it_removes(td):
    """test_gpu_pool.py::test_pool_n_limits' input: 300 requests, pools of four, refused by a buffer of 1000 plans"""
    d = M.random_demand(np.random.default_rng(1), 300, 9, [90])
    with pytest.raises(ffi().TdError):
        td.find_pool_n(4, d, max_happy=1000)
    want, want_happy = td.find_pool_n(4, d)
    recs, happy, stats = td.find_pool_n_banded(4, d, plan_buffer=7200)
    assert recs.tolist() == want.tolist() and happy == want_happy > 7200
    assert stats[0] >= 2 and stats[3] <= 7200


# ---- the contract of the C call ---------------------------------------------------------------------------------------------------
def test_host_and_device_pointers_and_a_short_output(td, cases):
    import torch
    d, n, exp, nh, _ = cases["r40", 3]
    cols = [np.ascontiguousarray(d[:, c].astype(np.int32)) for c in (1, 2, 3, 4)]
    dev = [torch.from_numpy(c).cuda() for c in cols]
    full = n // 3 + 1
    a = raw(3, n, cols, None, (0, n), 24 * n, full)
    out = torch.full((full + 2, 7), -7, dtype=torch.int32, device="cuda")
    b = raw(3, n, dev, None, (0, n), 24 * n, full, out=out)
    for got in (a, b):
        assert got["rc"] == 0 and got["recs"] == exp and got["happy"] == nh and got["n_pools"] == len(exp)
        assert (got["behind"] == -7).all()      # nothing behind the records
    assert a["stats"] == b["stats"]
    # max_pools below the answer: its first records, nothing behind them
    short = raw(3, n, cols, None, (0, n), 24 * n, 2)
    assert short["rc"] == 0 and short["n_pools"] == 2 and short["recs"] == exp[:2] and (short["behind"] == -7).all()
    assert short["happy"] == nh
    mixed = raw(3, n, [dev[0], cols[1], dev[2], cols[3]], None, (0, n), 0, 2)
    assert mixed["recs"] == exp[:2]


def test_null_stats_and_null_happy(td, cases):
    d, n, exp, nh, _ = cases["r24", 4]
    cols = [np.ascontiguousarray(d[:, c].astype(np.int32)) for c in (1, 2, 3, 4)]
    got = raw(4, n, cols, None, (0, n), 24 * n, n // 4 + 1, stats=False, happy=False)
    assert got["rc"] == 0 and got["recs"] == exp and got["stats"] == (-5,) * 4 and got["happy"] == -5


def test_a_refusal_writes_no_output(td, cases):
    d, n, exp, nh, _ = cases["r24", 3]
    cols = [np.ascontiguousarray(d[:, c].astype(np.int32)) for c in (1, 2, 3, 4)]
    lib = ffi().lib()
    for nn, room, what in ((n, 24 * n - 1, "plan_buffer"), (2048, 0, "n=2048"), (-1, 0, "n=-1")):
        got = raw(3, nn, cols, None, (0, n), room, 8)
        assert got["rc"] == TD_EINVAL and what in err(), (nn, room, err())
        assert got["n_pools"] == -5 and got["happy"] == -5 and got["stats"] == (-5,) * 4 and (got["behind"] == -7).all()
    assert raw(3, n, cols, None, (0, n), 24 * n - 1, 8)["rc"] == TD_EINVAL
    assert str(24 * n - 1) in err() and str(24 * n) in err()      # both numbers
    for k in (1, 5):
        m, h = ctypes.c_int32(-5), ctypes.c_int64(-5)
        out, st = np.full(64, -7, np.int32), np.full(4, -5, np.int64)
        rc = lib.td_pool_n_banded(k, n, *[c.ctypes.data for c in cols], None, 0, 0, n, 0, 8, out.ctypes.data, ctypes.byref(m), ctypes.byref(h),
                                  st.ctypes.data)
        assert rc == TD_EINVAL and "pool size" in err()
        assert m.value == -5 and h.value == -5 and (out == -7).all() and (st == -5).all()
    # null outputs, a table without a size
    m = ctypes.c_int32(-5)
    assert lib.td_pool_n_banded(3, n, *[c.ctypes.data for c in cols], None, 0, 0, n, 0, 8, None, ctypes.byref(m), None, None) == TD_EINVAL
    assert m.value == -5
    assert lib.td_pool_n_banded(3, n, *[c.ctypes.data for c in cols], None, 0, 0, n, 0, 8, np.zeros(64, np.int32).ctypes.data, None, None,
                                None) == TD_EINVAL
    table = np.zeros((1, 1), np.int32)
    m, out = ctypes.c_int32(-5), np.full(64, -7, np.int32)
    assert lib.td_pool_n_banded(3, n, *[c.ctypes.data for c in cols], table.ctypes.data, 0, 0, n, 0, 8, out.ctypes.data, ctypes.byref(m), None,
                                None) == TD_EINVAL and "S=0" in err()
    assert m.value == -5 and (out == -7).all()


def test_the_empty_cases(td, cases):
    d, n, exp, nh, _ = cases["r24", 3]
    cols = [np.ascontiguousarray(d[:, c].astype(np.int32)) for c in (1, 2, 3, 4)]
    for nn, first, max_pools in ((2, (0, 2), 8), (n, (5, 5), 8), (n, (n, n + 3), 8), (n, (0, n), 0), (0, (0, 0), 8)):
        got = raw(3, nn, cols, None, first, 0, max_pools)
        assert got["rc"] == 0 and got["n_pools"] == 0 and got["happy"] == 0 and got["stats"] == (0, 0, 0, 0), (nn, first, max_pools)
        assert (got["behind"] == -7).all()


def test_a_second_call_starts_with_nothing_used(td, cases):
    """the used bitmap and the counts live in device memory between the bands of ONE call: another model right behind, and the
    first one again, get their own answers"""
    first = cases["same12", 4]
    second = cases["r24", 4]
    for d, n, exp, nh, _ in (first, second, first, second):
        recs, happy, _ = td.find_pool_n_banded(4, d, plan_buffer=24 * n)
        assert recs.tolist() == exp and happy == nh


def test_a_cost_above_14_bits_is_refused_like_td_pool_n(td):
    """two requests 20 000 stands apart on |a - b|: the pair is happy under a loose rule and costs more than 16383"""
    d = np.array([[0, 0, 20000, 30000, 900], [1, 20000, 0, 30000, 900]], np.int64)
    f = ffi()
    with pytest.raises(f.TdError) as e1:
        td.find_pool_n(2, d)
    with pytest.raises(f.TdError) as e2:
        td.find_pool_n_banded(2, d)
    assert "14 bits" in str(e1.value) and "14 bits" in str(e2.value)
    cols = [np.ascontiguousarray(d[:, c].astype(np.int32)) for c in (1, 2, 3, 4)]
    lib = f.lib()
    out = np.zeros((4, 5), np.int32)
    m, h1, h2 = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.td_pool_n(2, 2, *[c.ctypes.data for c in cols], None, 0, 0, 2, 0, 2, out.ctypes.data, ctypes.byref(m), ctypes.byref(h1)) == -4
    assert lib.td_pool_n_banded(2, 2, *[c.ctypes.data for c in cols], None, 0, 0, 2, 0, 2, out.ctypes.data, ctypes.byref(m), ctypes.byref(h2),
                                None) == -4
    assert h1.value == h2.value > 0
