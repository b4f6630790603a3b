"""GPU tests of the batched position entry points (td_build_assign_batched / td_tick_batched, csrc/td_batch.hip): every
model of a ragged batch against the oracle's tick pipeline (cost build -> LCM with the Simulator's stop rules -> shrink ->
cost build -> optimum) bit for bit, agreement with one td_tick per model at the Simulator's 1300 x 900 shape, split.py's
regions, the committed tick-49 instance, the size limits, device memory and argument errors."""

import json
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu
BIG = 250000
I32_MAX = 2**31 - 1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_cost(cab, dem, dist, fill, thr):
    """oracle.cost_build with td_cost_build's rule for a stand outside the table (its cells are fill): such stands are
    pointed at an extra row / column of fill, which the oracle, indexing without a check, then reads"""
    cab, dem = np.asarray(cab, np.int32), np.asarray(dem, np.int32)
    if dist is None:
        return oracle.cost_build(cab, dem, None, fill, thr)
    S = dist.shape[0]
    ext = np.full((S + 1, S + 1), fill, np.int32)
    ext[:S, :S] = dist
    return oracle.cost_build(np.where((cab >= 0) & (cab < S), cab, S), np.where((dem >= 0) & (dem < S), dem, S), ext, fill, thr)


def oracle_tick(cab, dem, dist, fill, thr, stop):
    """the pipeline of test_config5_tick_in_one_call_gpu / sim_backend.OracleTickBackend with every parameter free"""
    cab, dem = np.asarray(cab, np.int32), np.asarray(dem, np.int32)
    n, cost = oracle_cost(cab, dem, dist, fill, thr)
    rows = cols = np.zeros(0, np.int64)
    lm, ran = fill, False
    if 0 <= stop < n:
        _, rows, cols, lm = oracle.lcm(cost, mask=fill, stop_value_on=1, stop_value=fill, stop_size=stop, sum_below=fill,
                                       java_scan=1)
        ran = True
    kc = np.setdiff1d(np.arange(len(cab)), rows)
    kd = np.setdiff1d(np.arange(len(dem)), cols)
    n2, cost2 = oracle_cost(cab[kc], dem[kd], dist, fill, thr)
    solved = n2 > 0 and not (ran and lm == fill)
    tot = oracle.assign(cost2)[0] if solved else 0
    return {"lcm_rows": rows, "lcm_cols": cols, "lcm_min_val": lm, "kept_cabs": kc, "kept_dems": kd, "n_rest": n2,
            "total": tot, "solved": solved, "cost2": cost2}


def check_tick(got, ref, what):
    assert got["lcm_rows"].tolist() == ref["lcm_rows"].tolist(), what
    assert got["lcm_cols"].tolist() == ref["lcm_cols"].tolist(), what
    assert got["lcm_min_val"] == ref["lcm_min_val"], (what, got["lcm_min_val"], ref["lcm_min_val"])
    assert got["kept_cabs"].tolist() == ref["kept_cabs"].tolist(), what
    assert got["kept_dems"].tolist() == ref["kept_dems"].tolist(), what
    assert got["n_rest"] == ref["n_rest"] and got["solved"] == ref["solved"], what
    assert got["total"] == ref["total"], (what, got["total"], ref["total"])
    assert got["dual_bound"] == got["total"], (what, got["dual_bound"], got["total"])
    if got["solved"]:
        k = got["n_rest"]
        p = got["row_to_col"]
        assert sorted(p.tolist()) == list(range(k)), what
        assert int(ref["cost2"].astype(np.int64)[np.arange(k), p].sum()) == got["total"], what
    else:
        assert got["row_to_col"].size == 0


def sizes(rng, B, stop):
    """ragged shapes: more cabs, more requests, empty sides, models at / below stop_size (no LCM) and above it"""
    fixed = [(0, 0), (0, 7), (9, 0), (1, 1), (stop, stop), (stop + 1, 3), (3, stop + 1), (2 * stop + 5, stop), (stop, 2 * stop + 5)]
    out = list(fixed)
    while len(out) < B:
        out.append((int(rng.integers(0, 3 * stop)), int(rng.integers(0, 3 * stop))))
    return out


def positions(rng, k, S, outside):
    p = rng.integers(0, S, k).astype(np.int32)
    if outside and k:
        bad = rng.random(k) < 0.05
        p[bad] = rng.choice(np.array([-1, S, S + 7, -S], np.int32), int(bad.sum()))
    return p


TABLES = ("abs50", "abs4000", "asym50", "big600")


def table_for(kind, rng):
    if kind == "abs50":
        return 50, None
    if kind == "abs4000":
        return 4000, None
    if kind == "asym50":
        return 50, rng.integers(0, 25, (50, 50)).astype(np.int32)
    d = rng.integers(0, 40, (600, 600)).astype(np.int32)   # 1.4 MB: read through L2
    return 600, d


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("thr", [-1, 0, 1, 10])
def test_tick_batched_vs_oracle(td, kind, thr):
    rng = np.random.default_rng(100 * TABLES.index(kind) + thr + 1)
    S, dist = table_for(kind, rng)
    stop = 20
    shapes = sizes(rng, 72, stop)
    cabs = [positions(rng, a, S, dist is not None) for a, _ in shapes]
    dems = [positions(rng, d, S, dist is not None) for _, d in shapes]
    got = td.tick_batched(cabs, dems, dist, big_cost=BIG, drop_time=None if thr < 0 else thr, max_non_lcm=stop)
    assert len(got) == len(shapes)
    ends_on_fill = 0
    for b in range(len(shapes)):
        ref = oracle_tick(cabs[b], dems[b], dist, BIG, thr, stop)
        check_tick(got[b], ref, (kind, thr, b, shapes[b]))
        ends_on_fill += int(not ref["solved"] and ref["n_rest"] > 0)
    if thr in (0, 1):
        assert ends_on_fill > 0   # the LCM ran out of cells below fill: no solve


def test_tick_batched_general_fill_and_stop(td):
    """fill below some real cells (those are never LCM candidates), stop_size < 0 (= build_assign_batched, no pairs)"""
    rng = np.random.default_rng(77)
    S = 50
    dist = rng.integers(0, 300, (S, S)).astype(np.int32)
    shapes = sizes(rng, 64, 15)
    cabs = [positions(rng, a, S, True) for a, _ in shapes]
    dems = [positions(rng, d, S, True) for _, d in shapes]
    for fill, stop in ((150, 15), (-5, 15), (150, -1), (BIG, -1)):
        got = td.tick_batched(cabs, dems, dist, big_cost=fill, drop_time=None, max_non_lcm=None if stop < 0 else stop)
        for b in range(len(shapes)):
            check_tick(got[b], oracle_tick(cabs[b], dems[b], dist, fill, -1, stop), (fill, stop, b))
        if stop < 0:
            r2c, tot, dual = td.build_assign_batched(cabs, dems, dist, fill=fill, threshold=-1, want_dual=True)
            assert [g["total"] for g in got] == tot.tolist() == dual.tolist()
            assert all(g["lcm_rows"].size == 0 and g["lcm_min_val"] == fill for g in got)


def test_tick_batched_matches_td_tick_1300x900(td):
    """Simulator.java's tick shape (1300 cabs, 900 requests, 50 stands, DROP_TIME 10, MAX_NON_LCM 600): 8 models in one call
    against one td.tick per model"""
    from taxidispatcher_amd.simulator import BIG_COST, DROP_TIME, MAX_NON_LCM
    rng = np.random.default_rng(1300)
    shapes = [(1300, 900), (900, 1300), (1300, 900), (1100, 700), (1300, 1300), (640, 610), (1300, 900), (601, 2)]
    cabs = [rng.integers(0, 50, a).astype(np.int32) for a, _ in shapes]
    dems = [rng.integers(0, 50, d).astype(np.int32) for _, d in shapes]
    got = td.tick_batched(cabs, dems, None, big_cost=BIG_COST, drop_time=DROP_TIME, max_non_lcm=MAX_NON_LCM)
    for b in range(len(shapes)):
        t = td.tick(cabs[b], dems[b], None, big_cost=BIG_COST, drop_time=DROP_TIME, max_non_lcm=MAX_NON_LCM)
        g = got[b]
        assert g["lcm_rows"].tolist() == t["lcm_rows"].tolist() and g["lcm_cols"].tolist() == t["lcm_cols"].tolist(), b
        assert g["lcm_min_val"] == t["lcm_min_val"] and g["solved"] == t["solved"] and g["n_rest"] == t["n_rest"], b
        assert g["kept_cabs"].tolist() == t["kept_cabs"].tolist() and g["kept_dems"].tolist() == t["kept_dems"].tolist(), b
        assert g["total"] == t["total"] and (not g["solved"] or g["dual_bound"] == g["total"]), b
    assert any(g["solved"] for g in got)


def test_build_assign_batched_vs_oracle(td):
    rng = np.random.default_rng(5)
    for S, dist, thr in ((50, None, 10), (50, rng.integers(0, 99, (50, 50)).astype(np.int32), -1), (4000, None, -1),
                         (600, rng.integers(0, 1000, (600, 600)).astype(np.int32), 500)):
        shapes = sizes(rng, 40, 60)
        cabs = [positions(rng, a, S, dist is not None) for a, _ in shapes]
        dems = [positions(rng, d, S, dist is not None) for _, d in shapes]
        r2c, tot, dual = td.build_assign_batched(cabs, dems, dist, fill=BIG, threshold=thr, want_dual=True)
        n = max(max(a, d) for a, d in shapes)
        assert r2c.shape == (len(shapes), n)
        for b, (a, d) in enumerate(shapes):
            k, cost = oracle_cost(cabs[b], dems[b], dist, BIG, thr)
            assert tot[b] == (oracle.assign(cost)[0] if k else 0) == dual[b], (S, b)
            assert sorted(r2c[b, :k].tolist()) == list(range(k)) and (r2c[b, k:] == -1).all()
            assert int(cost.astype(np.int64)[np.arange(k), r2c[b, :k]].sum()) == tot[b]
            if k:
                assert td.build_assign(cabs[b], dems[b], dist, fill=BIG, threshold=thr)[2] == tot[b]


def test_build_assign_batched_split_regions(td):
    """split.py's shape: one 400-request instance on 4000 stands (|a - b|) cut into four stand ranges, one model each"""
    rng = np.random.default_rng(400)
    cab, dem = rng.integers(0, 4000, 400), rng.integers(0, 4000, 400)
    cabs = [cab[(cab >= lo) & (cab < lo + 1000)] for lo in range(0, 4000, 1000)]
    dems = [dem[(dem >= lo) & (dem < lo + 1000)] for lo in range(0, 4000, 1000)]
    r2c, tot, dual = td.build_assign_batched(cabs, dems, None, fill=BIG, threshold=-1, want_dual=True)
    for b in range(4):
        k, cost = oracle.cost_build(cabs[b], dems[b], None, BIG, -1)
        assert tot[b] == oracle.assign(cost)[0] == dual[b]


def test_build_assign_batched_tick49(td):
    """the committed tick-49 instance (600 cabs, 218 requests) as one model of a batch"""
    with open(os.path.join(GOLD, "tick49_instance.json")) as f:
        g = json.load(f)
    rng = np.random.default_rng(49)
    cabs = [rng.integers(0, 50, 30), np.asarray(g["cab_to"]), rng.integers(0, 50, 7)]
    dems = [rng.integers(0, 50, 40), np.asarray(g["dem_from"]), rng.integers(0, 50, 0)]
    r2c, tot, dual = td.build_assign_batched(cabs, dems, None, fill=g["fill"], threshold=g["threshold"], want_dual=True)
    n, cost = oracle.cost_build(g["cab_to"], g["dem_from"], None, g["fill"], g["threshold"])
    p = r2c[1, :n]
    assert n == g["n"] == 600 and tot[1] == g["total"] == dual[1]
    assert td.count_sum(n, cost, p) == g["real_total"]
    opt_count = int((cost[np.arange(n), p] < g["fill"]).sum())   # Simulator.java:378-383
    assert opt_count == g["opt_count"] == 32


def _raw_tick(lib, B, n, co, cv, do, dv, stop, dist=None, S=0, fill=BIG, thr=-1):
    rows, cols, kc, kd, r2c = (np.zeros(max(B * n, 1), np.int32) for _ in range(5))
    k, lm, n2 = (np.zeros(max(B, 1), np.int32) for _ in range(3))
    tot, dual = np.zeros(max(B, 1), np.int64), np.zeros(max(B, 1), np.int64)
    rc = lib.td_tick_batched(B, n, co.ctypes.data, cv.ctypes.data, do.ctypes.data, dv.ctypes.data,
                             None if dist is None else dist.ctypes.data, S, fill, thr, stop, rows.ctypes.data, cols.ctypes.data,
                             k.ctypes.data, lm.ctypes.data, kc.ctypes.data, kd.ctypes.data, n2.ctypes.data, r2c.ctypes.data,
                             tot.ctypes.data, dual.ctypes.data)
    return rc, tot, dual, n2


def test_size_limits(td):
    from taxidispatcher_amd import _ffi
    from taxidispatcher_amd.dispatch import pack_ragged
    lib = _ffi.lib()
    rng = np.random.default_rng(2048)
    # n = 2048 with an LCM down to 600 is accepted, 2049 refused
    for n, ok in ((2048, True), (2049, False)):
        cv, co, dv, do, B, nn = pack_ragged([rng.integers(0, 50, n).astype(np.int32)], [rng.integers(0, 50, n - 500).astype(np.int32)])
        rc, tot, dual, n2 = _raw_tick(lib, B, nn, co, cv, do, dv, 600, thr=10)
        assert (rc == 0) == ok, (n, lib.td_last_error())
        if not ok:
            assert b"2048" in lib.td_last_error()
        else:
            assert n2[0] == 600 and tot[0] == dual[0]
    # a remainder of 1024 rows is accepted, 1025 refused (no LCM: stop_size >= n)
    for n, ok in ((1024, True), (1025, False)):
        cv, co, dv, do, B, nn = pack_ragged([rng.integers(0, 4000, n).astype(np.int32)], [rng.integers(0, 4000, n - 3).astype(np.int32)])
        rc, tot, dual, n2 = _raw_tick(lib, B, nn, co, cv, do, dv, 2000)
        assert (rc == 0) == ok, (n, lib.td_last_error())
        if ok:
            assert n2[0] == 1024 and tot[0] == dual[0]
        else:
            assert b"1024" in lib.td_last_error()
    cv, co, dv, do, B, nn = pack_ragged([rng.integers(0, 4000, 2048).astype(np.int32)], [rng.integers(0, 4000, 2000).astype(np.int32)])
    assert _raw_tick(lib, B, nn, co, cv, do, dv, 1024)[0] == 0
    assert _raw_tick(lib, B, nn, co, cv, do, dv, 1025)[0] != 0
    # td_build_assign_batched: n = 1024 accepted, 1025 refused
    for n, ok in ((1024, True), (1025, False)):
        cabs = [rng.integers(0, 4000, n), rng.integers(0, 4000, 5)]
        dems = [rng.integers(0, 4000, n // 2), rng.integers(0, 4000, 9)]
        if ok:
            r2c, tot, dual = td.build_assign_batched(cabs, dems, None, want_dual=True)
            k, cost = oracle.cost_build(cabs[0], dems[0], None, BIG, -1)
            assert tot[0] == dual[0] == oracle.assign(cost)[0]
        else:
            with pytest.raises(td.TdError, match="1024"):
                td.build_assign_batched(cabs, dems)


def test_int32_max_fill_and_wide_stride(td):
    """fill = INT32_MAX with table values near it: int64 totals; an output stride larger than every model"""
    from taxidispatcher_amd import _ffi
    from taxidispatcher_amd.dispatch import pack_ragged
    rng = np.random.default_rng(31)
    S = 40
    dist = rng.integers(I32_MAX - 1000, I32_MAX, (S, S)).astype(np.int32)
    dist[rng.random((S, S)) < 0.2] = I32_MAX   # equal to fill: never an LCM candidate
    shapes = [(30, 20), (20, 30), (0, 5), (25, 25), (12, 3)]
    cabs = [positions(rng, a, S, True) for a, _ in shapes]
    dems = [positions(rng, d, S, True) for _, d in shapes]
    got = td.tick_batched(cabs, dems, dist, big_cost=I32_MAX, drop_time=None, max_non_lcm=10)
    for b in range(len(shapes)):
        ref = oracle_tick(cabs[b], dems[b], dist, I32_MAX, -1, 10)
        check_tick(got[b], ref, b)
    assert max(g["total"] for g in got) > 2**32
    # the same models through the C ABI with a stride of 64: the same numbers, -1 beyond each model
    cv, co, dv, do, B, n = pack_ragged(cabs, dems)
    W = 64
    r2c = np.zeros(B * W, np.int32)
    tot = np.zeros(B, np.int64)
    _ffi.check(_ffi.lib().td_build_assign_batched(B, W, co.ctypes.data, cv.ctypes.data, do.ctypes.data, dv.ctypes.data, dist.ctypes.data,
                                                  S, I32_MAX, -1, r2c.ctypes.data, tot.ctypes.data, None))
    r_ref, t_ref = td.build_assign_batched(cabs, dems, dist, fill=I32_MAX)
    assert np.array_equal(tot, t_ref)
    r2c = r2c.reshape(B, W)
    assert np.array_equal(r2c[:, :n], r_ref) and (r2c[:, n:] == -1).all()


def test_empty_and_single_batch(td):
    r2c, tot = td.build_assign_batched([], [])
    assert r2c.shape == (0, 0) and tot.shape == (0,)
    assert td.tick_batched([], []) == []
    from taxidispatcher_amd import _ffi
    assert _ffi.lib().td_tick_batched(0, 5, None, None, None, None, None, 0, BIG, 10, 3, None, None, None, None, None, None, None, None,
                                      None, None) == 0
    rng = np.random.default_rng(1)
    cab, dem = rng.integers(0, 50, 90), rng.integers(0, 50, 70)
    g = td.tick_batched([cab], [dem], None, drop_time=10, max_non_lcm=30)
    check_tick(g[0], oracle_tick(cab, dem, None, BIG, 10, 30), "B=1")


def test_device_inputs_and_outputs(td):
    import torch
    from taxidispatcher_amd import _ffi
    from taxidispatcher_amd.dispatch import pack_ragged
    rng = np.random.default_rng(9)
    S = 50
    dist = rng.integers(0, 30, (S, S)).astype(np.int32)
    shapes = sizes(rng, 70, 25)
    cabs = [positions(rng, a, S, True) for a, _ in shapes]
    dems = [positions(rng, d, S, True) for _, d in shapes]
    host = td.tick_batched(cabs, dems, dist, drop_time=12, max_non_lcm=25)
    cv, co, dv, do, B, n = pack_ragged(cabs, dems)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev = td.tick_batched((t(cv), t(co)), (t(dv), t(do)), t(dist), drop_time=12, max_non_lcm=25)
    for g, h in zip(dev, host):
        for key in h:
            assert np.array_equal(np.asarray(g[key]), np.asarray(h[key])), key
    r_h, t_h, d_h = td.build_assign_batched(cabs, dems, dist, threshold=12, want_dual=True)
    r_d, t_d, d_d = td.build_assign_batched((t(cv), t(co)), (t(dv), t(do)), t(dist), threshold=12, want_dual=True)
    assert np.array_equal(r_h, r_d) and np.array_equal(t_h, t_d) and np.array_equal(d_h, d_d)
    # every output in device memory through the C ABI
    o32 = [torch.full((B * n,), -7, dtype=torch.int32, device="cuda") for _ in range(5)]
    s32 = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3)]
    s64 = [torch.zeros(B, dtype=torch.int64, device="cuda") for _ in range(2)]
    rows, cols, kc, kd, r2c = o32
    k, lm, n2 = s32
    _ffi.check(_ffi.lib().td_tick_batched(B, n, co.ctypes.data, cv.ctypes.data, do.ctypes.data, dv.ctypes.data, dist.ctypes.data, S, BIG,
                                          12, 25, rows.data_ptr(), cols.data_ptr(), k.data_ptr(), lm.data_ptr(), kc.data_ptr(),
                                          kd.data_ptr(), n2.data_ptr(), r2c.data_ptr(), s64[0].data_ptr(), s64[1].data_ptr()))
    rows, cols, kc, kd, r2c = (x.cpu().numpy().reshape(B, n) for x in o32)
    k, lm, n2 = (x.cpu().numpy() for x in s32)
    tot, dual = (x.cpu().numpy() for x in s64)
    for b, h in enumerate(host):
        kk = int(k[b])
        assert rows[b, :kk].tolist() == h["lcm_rows"].tolist() and cols[b, :kk].tolist() == h["lcm_cols"].tolist()
        assert kc[b, :len(h["kept_cabs"])].tolist() == h["kept_cabs"].tolist()
        assert kd[b, :len(h["kept_dems"])].tolist() == h["kept_dems"].tolist()
        assert lm[b] == h["lcm_min_val"] and n2[b] == h["n_rest"] and tot[b] == h["total"] and dual[b] == h["dual_bound"]
        assert r2c[b, :h["row_to_col"].size].tolist() == h["row_to_col"].tolist()


def test_argument_errors(td):
    """every refusal is a TdError and leaves the outputs untouched"""
    from taxidispatcher_amd import _ffi
    from taxidispatcher_amd.dispatch import pack_ragged
    lib = _ffi.lib()
    cv = np.arange(10, dtype=np.int32)
    dv = np.arange(8, dtype=np.int32)
    B, n = 2, 6
    dist = np.zeros((4, 4), np.int32)

    def call(co, do, n=n, dist_p=None, S=0, null_out=None):
        co, do = np.asarray(co, np.int32), np.asarray(do, np.int32)
        outs = [np.full(B * n + 16, 0x5A5A, np.int32) for _ in range(5)]
        sc = [np.full(B + 4, 0x5A5A, np.int32) for _ in range(3)]
        s64 = [np.full(B + 4, 0x5A5A, np.int64) for _ in range(2)]
        ptrs = [o.ctypes.data for o in outs[:2]] + [sc[0].ctypes.data, sc[1].ctypes.data] + [o.ctypes.data for o in outs[2:4]] + \
               [sc[2].ctypes.data, outs[4].ctypes.data, s64[0].ctypes.data, s64[1].ctypes.data]
        if null_out is not None:
            ptrs[null_out] = None
        rc = lib.td_tick_batched(B, n, co.ctypes.data, cv.ctypes.data, do.ctypes.data, dv.ctypes.data, dist_p, S, BIG, -1, 2, *ptrs)
        untouched = all((o == 0x5A5A).all() for o in outs + sc + s64)
        r2c = np.full(B * n + 16, 0x5A5A, np.int32)
        tot = np.full(B + 4, 0x5A5A, np.int64)
        rc2 = lib.td_build_assign_batched(B, n, co.ctypes.data, cv.ctypes.data, do.ctypes.data, dv.ctypes.data, dist_p, S, BIG, -1,
                                          r2c.ctypes.data if null_out is None else None, tot.ctypes.data, None)
        return rc, rc2, untouched and (r2c == 0x5A5A).all() and (tot == 0x5A5A).all()

    ok = call([0, 5, 10], [0, 4, 8])
    assert ok[0] == 0 and ok[1] == 0
    for args, msg in ((([0, 6, 5], [0, 4, 8]), b"decreases"),          # decreasing offsets
                      (([1, 5, 10], [0, 4, 8]), b"not 0"),             # not starting at 0
                      (([0, 3, 10], [0, 4, 8]), b"more than n"),       # a model larger than n
                      ):
        rc, rc2, untouched = call(*args)
        assert rc == -1 and rc2 == -1 and untouched, msg
    rc, rc2, untouched = call([0, 5, 10], [0, 4, 8], dist_p=dist.ctypes.data, S=0)   # S <= 0 with a table
    assert rc == -1 and rc2 == -1 and untouched
    assert b"S = 0" in lib.td_last_error()
    for k in (0, 1, 2, 3, 6, 7, 8):   # every required output
        rc, rc2, untouched = call([0, 5, 10], [0, 4, 8], null_out=k)
        assert rc == -1 and rc2 == -1 and untouched, k
    with pytest.raises(td.TdError, match="beyond"):   # an offset beyond the values
        td.tick_batched((cv, np.array([0, 5, 11], np.int32)), (dv, np.array([0, 4, 8], np.int32)))
    with pytest.raises(td.TdError, match="beyond"):
        td.build_assign_batched((cv, np.array([0, 5, 10], np.int32)), (dv, np.array([0, 4, 9], np.int32)))
    with pytest.raises(td.TdError, match="decrease"):
        td.build_assign_batched((cv, np.array([0, 5, 3], np.int32)), (dv, np.array([0, 4, 8], np.int32)))
    with pytest.raises(td.TdError, match="S = -3"):
        lib_cv, lib_co, lib_dv, lib_do, _, _ = pack_ragged([cv], [dv])
        _ffi.check(lib.td_build_assign_batched(1, 10, lib_co.ctypes.data, lib_cv.ctypes.data, lib_do.ctypes.data, lib_dv.ctypes.data,
                                               dist.ctypes.data, -3, BIG, -1, np.zeros(10, np.int32).ctypes.data,
                                               np.zeros(1, np.int64).ctypes.data, None))
