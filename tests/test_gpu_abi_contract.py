"""GPU tests of the C ABI's memory, stream and life-cycle contract (include/taxidispatcher_amd.h): every entry point is
called through _ffi.lib() with RAW addresses (never _ffi.addr(), whose synchronisation would hide the stream rule) on
buffers from tests/abi_buffers.py: outputs are windows between guard bands, inputs sit in host, pinned or device memory and
in device views that are aligned to their element size only.  Expected values come from the CPU oracle (or the host
restatements the suite already uses) and are compared bit for bit in every pointer combination; after every call the
guards of every output are checked.  Where the header defines only the first k entries of an output, entries [0, k),
k <= capacity and the guards behind the capacity are asserted; entries between k and the capacity are unspecified."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import abi_buffers as ab
from oracle import oracle
from sim_backend import OracleBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 250000
I32_MIN = -2**31
IN_KINDS = (("host", 0), ("pinned", 0), ("device", 0), ("device", 1))   # the last one: a device view inside an allocation
OUT_KINDS = (("host", 0), ("device", 0), ("device", 1))                 # the last one with n % 4 == 0: the scalar store branch
HD = (("host", 0), ("device", 0))
P = ab.ptr
PAT32 = int(ab.pattern_value(np.int32))


@pytest.fixture()
def lib(td):
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def ok(lib, rc):
    assert rc == 0, (rc, lib.td_last_error())


def cycle(seq):
    return itertools.cycle(seq)


class Placed:
    """one input array in every kind of memory, made on first use"""

    def __init__(self, array):
        self.a = np.ascontiguousarray(array)
        self.made = {}

    def __call__(self, kind):
        if kind not in self.made:
            self.made[kind] = ab.place(self.a, *kind)
        return self.made[kind]


def stats(lib):
    out = (ctypes.c_int64 * 16)()
    ok(lib, lib.td_last_stats(out, 16))
    return list(out)


# ------------------------------------------------------------------------------------------------------------------
# td_cost_build, td_cost_build_rows, td_gen_uniform
# ------------------------------------------------------------------------------------------------------------------
CB_N = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1028]   # quad remainders 0..3, one and two 256-thread column blocks


def row_windows(n):
    """row0 > 0 with an odd number of rows, and the last row alone"""
    w = []
    if n >= 2:
        k = n - 1 if (n - 1) % 2 else n - 2
        if k >= 1:
            w.append((1, k))
        w.append((n - 1, 1))
    return w


def with_holes(rng, k):
    ids = np.arange(k, dtype=np.int32)
    if k:
        ids[rng.random(k) < 0.2] = -1
        ids[rng.integers(0, k)] = -1
    return ids


@pytest.mark.parametrize("n", CB_N)
def test_cost_build(lib, n):
    rng = np.random.default_rng(1000 + n)
    small = n - 3 if n > 3 else n - 1
    outs, ins = cycle(OUT_KINDS), cycle(IN_KINDS)
    seen = set()
    for n_s, n_d in ((n, small), (small, n)):
        for S in (0, 128, 129):   # |a - b|; exactly 64 KiB: the table staged in LDS; one more: read through L2
            hi = S or 4000
            cab, dem = rng.integers(0, hi, n_s).astype(np.int32), rng.integers(0, hi, n_d).astype(np.int32)
            dist = rng.integers(0, 30, (S, S)).astype(np.int32) if S else None
            cid, did = with_holes(rng, n_s), with_holes(rng, n_d)
            p_cab, p_dem, p_cid, p_did = Placed(cab), Placed(dem), Placed(cid), Placed(did)
            p_dist = Placed(dist) if S else None
            for thr, ids in itertools.product((-1, 10), (False, True)):
                _, ref = oracle.cost_build(cab, dem, dist, BIG, thr, cid if ids else None, did if ids else None)
                for _ in range(3):   # every output kind; the input kind moves on with every call: all 12 pairs occur
                    ok_, ik = next(outs), next(ins)
                    seen.add((ok_, ik))
                    a_cab, a_dem = P(p_cab(ik)) if n_s else None, P(p_dem(ik)) if n_d else None
                    a_cid = P(p_cid(ik)) if ids and n_s else None
                    a_did = P(p_did(ik)) if ids and n_d else None
                    a_dist = P(p_dist(ik)) if S else None
                    out, check = ab.guarded((n, n), np.int32, *ok_)
                    ok(lib, lib.td_cost_build(a_cab, a_cid, n_s, a_dem, a_did, n_d, a_dist, S, BIG, thr, 0, P(out)))
                    ok(lib, lib.td_synchronize())
                    check()
                    assert np.array_equal(ab.host(out), ref), (n_s, n_d, S, thr, ids, ok_, ik)
                    for row0, nrows in row_windows(n):
                        out, check = ab.guarded((nrows, n), np.int32, *ok_)
                        ok(lib, lib.td_cost_build_rows(a_cab, a_cid, n_s, a_dem, a_did, n_d, a_dist, S, BIG, thr, 0, row0, nrows,
                                                       P(out)))
                        ok(lib, lib.td_synchronize())
                        check()
                        assert np.array_equal(ab.host(out), ref[row0:row0 + nrows]), (n_s, n_d, S, thr, ids, ok_, ik, row0)
    assert len(seen) == len(OUT_KINDS) * len(IN_KINDS)


@pytest.mark.parametrize("n", CB_N)
def test_cost_build_by_id(lib, n):
    """procedure.py's rule: cells addressed by a permuted id set, fill n * n; the row window applies to the cab ids"""
    rng = np.random.default_rng(2000 + n)
    small = n - 3 if n > 3 else n - 1
    outs, ins = cycle(OUT_KINDS), cycle(IN_KINDS)
    for n_s, n_d in ((n, small), (small, n)):
        for S in (0, 128):
            hi = S or 4000
            cab, dem = rng.integers(0, hi, n_s).astype(np.int32), rng.integers(0, hi, n_d).astype(np.int32)
            cid, did = rng.permutation(n)[:n_s].astype(np.int32), rng.permutation(n)[:n_d].astype(np.int32)
            dist = rng.integers(0, 30, (S, S)).astype(np.int32) if S else None
            _, ref = oracle.cost_build_by_id(cid, cab, did, dem, dist)
            p = [Placed(x) for x in (cab, cid, dem, did)] + [Placed(dist) if S else None]
            for _ in range(4):
                ok_, ik = next(outs), next(ins)
                a = [P(q(ik)) if q is not None else None for q in p]   # (an empty side still hands over its window's address)
                for row0, nrows in [(0, n)] + row_windows(n):
                    out, check = ab.guarded((nrows, n), np.int32, *ok_)
                    ok(lib, lib.td_cost_build_rows(a[0], a[1], n_s, a[2], a[3], n_d, a[4], S, n * n, -1, 1, row0, nrows, P(out)))
                    ok(lib, lib.td_synchronize())
                    check()
                    assert np.array_equal(ab.host(out), ref[row0:row0 + nrows]), (n_s, n_d, S, ok_, ik, row0, nrows)
                if n_s and n_d:
                    out, check = ab.guarded((n, n), np.int32, *ok_)
                    ok(lib, lib.td_cost_build(a[0], a[1], n_s, a[2], a[3], n_d, a[4], S, n * n, -1, 1, P(out)))
                    ok(lib, lib.td_synchronize())
                    check()
                    assert np.array_equal(ab.host(out), ref)


@pytest.mark.parametrize("n", CB_N)
def test_gen_uniform(lib, n):
    for (lo, hi), seed in (((10, 40), 7), ((0, 10**6), 2**40 + 3)):
        ref = oracle.gen_uniform(n, seed, lo, hi)
        for ok_ in OUT_KINDS:
            for row0, nrows in [(0, n)] + row_windows(n):
                out, check = ab.guarded((nrows, n), np.int32, *ok_)
                ok(lib, lib.td_gen_uniform(n, seed, lo, hi, row0, nrows, P(out)))
                ok(lib, lib.td_synchronize())
                check()
                assert np.array_equal(ab.host(out), ref[row0:row0 + nrows]), (n, lo, hi, ok_, row0, nrows)
                assert np.array_equal(ref[row0:row0 + nrows], oracle.gen_uniform(n, seed, lo, hi, row0, nrows))


# ------------------------------------------------------------------------------------------------------------------
# td_expand_x, td_count_sum
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_expand_x_and_count_sum(lib, n):
    rng = np.random.default_rng(n)
    r2c = rng.permutation(n).astype(np.int32)
    x_ref = np.zeros((n, n), np.uint8)
    x_ref[np.arange(n), r2c] = 1
    cost = rng.integers(0, 60, (n, n)).astype(np.int32)
    cost[rng.random((n, n)) < 0.3] = BIG
    s_ref, k_ref = oracle.count_sum(cost, r2c, BIG)
    p_r2c, p_cost = Placed(r2c), Placed(cost)
    for ok_, ik in itertools.product(OUT_KINDS, IN_KINDS):
        x, check = ab.guarded((n, n), np.uint8, *ok_)
        ok(lib, lib.td_expand_x(n, P(p_r2c(ik)), P(x)))
        check()
        assert np.array_equal(ab.host(x), x_ref), (n, ok_, ik)
    for ck, rk in itertools.product(IN_KINDS, IN_KINDS):
        s, k = ctypes.c_int64(-1), ctypes.c_int32(-1)
        ok(lib, lib.td_count_sum(n, P(p_cost(ck)), P(p_r2c(rk)), BIG, ctypes.byref(s), ctypes.byref(k)))
        assert (s.value, k.value) == (s_ref, k_ref), (n, ck, rk)


# ------------------------------------------------------------------------------------------------------------------
# td_assign, td_solver_assign
# ------------------------------------------------------------------------------------------------------------------
def check_assignment(cost, r2c, total, dual, ref_total, what):
    n = cost.shape[0]
    assert total == ref_total == dual, (what, total, ref_total, dual)
    assert sorted(r2c.tolist()) == list(range(n)), what
    assert int(cost.astype(np.int64)[np.arange(n), r2c].sum()) == total, what


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000])
def test_assign_every_pointer_kind(lib, n):
    rng = np.random.default_rng(3000 + n)
    h = ctypes.c_void_p()
    ok(lib, lib.td_solver_create(ctypes.byref(h)))
    try:
        for lo, hi in ((10, 40), (0, 10**6)):
            cost = rng.integers(lo, hi + 1, (n, n)).astype(np.int32)
            ref_total = oracle.assign(cost)[0]
            p_cost = Placed(cost)
            first = {}
            for ck, rk in itertools.product(IN_KINDS, OUT_KINDS):
                for name in ("td_assign", "td_solver_assign"):
                    r2c, check = ab.guarded((n,), np.int32, *rk)
                    tot, dual = ctypes.c_int64(-1), ctypes.c_int64(-2)
                    args = (n, P(p_cost(ck)), P(r2c), ctypes.byref(tot), ctypes.byref(dual))
                    ok(lib, lib.td_assign(*args) if name == "td_assign" else lib.td_solver_assign(h, *args))
                    check()
                    got = ab.host(r2c)
                    check_assignment(cost, got, tot.value, dual.value, ref_total, (n, lo, hi, ck, rk, name))
                    # the same answer whatever memory the cells and the result live in
                    assert np.array_equal(first.setdefault(name, got), got), (n, lo, hi, ck, rk, name)
    finally:
        ok(lib, lib.td_solver_destroy(h))


def _device_checks(torch, cost_t, r2c, total):
    n = cost_t.shape[0]
    assert sorted(r2c.tolist()) == list(range(n))
    idx = torch.from_numpy(r2c.astype(np.int64)).cuda()
    assert int(cost_t.gather(1, idx[:, None]).to(torch.int64).sum().item()) == total


def test_assign_12288_from_a_misaligned_view(lib):
    """n = 12 288, U{10..40}, generated on the device: the smallest size of the headline path (round 0's bids out of the
    1-byte compress pass, the block-local start).  The same cells once 16-byte aligned and once in a view aligned to 4
    bytes only, which takes the scalar loads and with them the fallback without round 0 inside the compress pass.
    Which start ran is read from td_last_stats word [0]: on these cells the block-local start leaves nothing to the bid
    rounds (0, as bench.py reports for its headline), the fallback solves by the rounds (10 on an MI355X).  A compress
    pass that picked its vector path without looking at the base address would show 0 for the view as well.
    Wall time on an MI355X: 0.2 s."""
    import torch
    n = 12288
    c0, _ = ab.guarded((n, n), np.int32, "device", 0)
    ok(lib, lib.td_gen_uniform(n, 12288, 10, 40, 0, n, P(c0)))
    ok(lib, lib.td_synchronize())
    c1, _ = ab.guarded((n, n), np.int32, "device", 1)
    c1.copy_(c0)
    torch.cuda.synchronize()
    assert P(c0) % 16 == 0 and P(c1) % 16 == 4
    totals, rounds = [], []
    for c in (c0, c1):
        r2c, check = ab.guarded((n,), np.int32, "host")
        tot, dual = ctypes.c_int64(-1), ctypes.c_int64(-2)
        ok(lib, lib.td_assign(n, P(c), P(r2c), ctypes.byref(tot), ctypes.byref(dual)))
        check()
        assert dual.value == tot.value
        _device_checks(torch, c, r2c, tot.value)
        st = stats(lib)
        assert st[4] == 1           # the 1-byte working copy
        totals.append(tot.value)
        rounds.append(st[0])
    assert totals[0] == totals[1]
    # Which start ran, read from td_last_stats word [0] (more than the issue asks; it is what notices a compress pass that
    # picks its vector path without looking at the base address).  Aligned: the block-local start leaves nothing to the
    # bid rounds.  The view: the fallback solves by the rounds.  A later change that gives a 4-byte-aligned matrix a round-0
    # start of its own makes rounds[1] == 0 legitimate: then replace this line by whatever tells the two paths apart.
    assert rounds[0] == 0 and rounds[1] > 0, rounds
    assert torch.equal(c0, c1)      # inputs are read only


def test_assign_padded_model_from_a_misaligned_view(lib):
    """a model padded with dummy requests (constant trailing columns = fill) above n = 2048: td_assign solves the transposed
    problem and reads the caller's matrix in its fused transposing compress pass, whose 16-byte loads need a 16-byte aligned
    base.  The same cells aligned and in a view aligned to 4 bytes only: equal totals, each certified by its dual bound."""
    import torch
    n, n_d = 2304, 1500
    rng = np.random.default_rng(2304)
    cab, dem = rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n_d).astype(np.int32)
    c0, _ = ab.guarded((n, n), np.int32, "device", 0)
    ok(lib, lib.td_cost_build(cab.ctypes.data, None, n, dem.ctypes.data, None, n_d, None, 0, BIG, 10, 0, P(c0)))
    ok(lib, lib.td_synchronize())
    assert np.array_equal(ab.host(c0), oracle.cost_build(cab, dem, None, BIG, 10)[1])
    c1, _ = ab.guarded((n, n), np.int32, "device", 1)
    c1.copy_(c0)
    torch.cuda.synchronize()
    assert P(c0) % 16 == 0 and P(c1) % 16 == 4
    totals = []
    for c in (c0, c1):
        r2c, check = ab.guarded((n,), np.int32, "host")
        tot, dual = ctypes.c_int64(-1), ctypes.c_int64(-2)
        ok(lib, lib.td_assign(n, P(c), P(r2c), ctypes.byref(tot), ctypes.byref(dual)))
        check()
        assert dual.value == tot.value
        _device_checks(torch, c, r2c, tot.value)
        assert stats(lib)[7] == 1   # the transposed formulation was solved
        totals.append(tot.value)
    assert totals[0] == totals[1]
    assert torch.equal(c0, c1)


def test_assign_line_metric_from_a_misaligned_view(lib):
    """|a_i - b_j| at n = 4096: the line-metric certificate pass over an aligned matrix and over a view aligned to 4 bytes
    only; the sorted matching's closed form is the reference"""
    import torch
    n = 4096
    rng = np.random.default_rng(4096)
    a, b = rng.integers(0, 40000, n), rng.integers(0, 40000, n)
    ref = int(np.abs(np.sort(a) - np.sort(b)).sum())
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    c0, _ = ab.guarded((n, n), np.int32, "device", 0)
    c1, _ = ab.guarded((n, n), np.int32, "device", 1)
    c0.copy_((ta[:, None] - tb[None, :]).abs().to(torch.int32))
    c1.copy_(c0)
    torch.cuda.synchronize()
    for c in (c0, c1):
        r2c, check = ab.guarded((n,), np.int32, "host")
        tot, dual = ctypes.c_int64(-1), ctypes.c_int64(-2)
        ok(lib, lib.td_assign(n, P(c), P(r2c), ctypes.byref(tot), ctypes.byref(dual)))
        check()
        assert tot.value == dual.value == ref
        _device_checks(torch, c, r2c, tot.value)
        assert stats(lib)[8] == 1   # answered by the line-metric path
    assert torch.equal(c0, c1)


# ------------------------------------------------------------------------------------------------------------------
# td_build_assign, td_tick
# ------------------------------------------------------------------------------------------------------------------
TICK_SHAPES = [(1, 1), (3, 5), (5, 3), (65, 64), (130, 90)]


def oracle_tick(cab, dem, dist, fill, thr, stop):
    """sim_backend.OracleTickBackend.tick (Simulator.java:163-208) with the table, fill, threshold and stop size free"""
    cab, dem = np.asarray(cab, np.int32), np.asarray(dem, np.int32)
    n, cost = oracle.cost_build(cab, dem, dist, fill, thr)
    rows = cols = np.zeros(0, np.int64)
    lm, ran = fill, False
    if 0 <= stop < n:
        _, rows, cols, lm = oracle.lcm(cost, mask=fill, stop_value_on=1, stop_value=fill, stop_size=stop, sum_below=fill, java_scan=1)
        ran = True
    kc = np.setdiff1d(np.arange(len(cab)), rows)
    kd = np.setdiff1d(np.arange(len(dem)), cols)
    n2, cost2 = oracle.cost_build(cab[kc], dem[kd], dist, fill, thr)
    solved = n2 > 0 and not (ran and lm == fill)
    return {"rows": rows, "cols": cols, "lm": lm, "kc": kc, "kd": kd, "n2": n2, "total": oracle.assign(cost2)[0] if solved else 0,
            "solved": solved, "cost2": cost2, "ran": ran}


@pytest.mark.parametrize("n_s,n_d", TICK_SHAPES)
def test_build_assign(lib, n_s, n_d):
    rng = np.random.default_rng(100 * n_s + n_d)
    n, S = max(n_s, n_d), 50
    cab, dem = rng.integers(0, S, n_s).astype(np.int32), rng.integers(0, S, n_d).astype(np.int32)
    table = rng.integers(0, 25, (S, S)).astype(np.int32)
    p_cab, p_dem, p_tab = Placed(cab), Placed(dem), Placed(table)
    h = ctypes.c_void_p()
    ok(lib, lib.td_solver_create(ctypes.byref(h)))
    try:
        outs = cycle(OUT_KINDS)
        for thr, tk in itertools.product((-1, 10), (None,) + HD):
            dist = None if tk is None else table
            _, cost = oracle.cost_build(cab, dem, dist, BIG, thr)
            ref_total = oracle.assign(cost)[0]
            first = {}
            for ik in IN_KINDS:
                for name in ("td_build_assign", "td_solver_build_assign"):
                    rk = next(outs)
                    r2c, check = ab.guarded((n,), np.int32, *rk)
                    tot, dual = ctypes.c_int64(-1), ctypes.c_int64(-2)
                    args = (P(p_cab(ik)), n_s, P(p_dem(ik)), n_d, None if tk is None else P(p_tab(tk)), S if tk else 0, BIG, thr,
                            P(r2c), ctypes.byref(tot), ctypes.byref(dual))
                    ok(lib, lib.td_build_assign(*args) if name == "td_build_assign" else lib.td_solver_build_assign(h, *args))
                    check()
                    got = ab.host(r2c)
                    check_assignment(cost, got, tot.value, dual.value, ref_total, (n_s, n_d, thr, tk, ik, rk, name))
                    assert np.array_equal(first.setdefault(name, got), got), (n_s, n_d, thr, tk, ik, rk, name)
    finally:
        ok(lib, lib.td_solver_destroy(h))


def raw_tick(lib, cab, n_s, dem, n_d, dist, S, fill, thr, stop, out_kind, r2c_kind=None):
    """td_tick with every output array a guarded window of capacity max(n_s, n_d) -> (rc, arrays, scalars, checks)"""
    n = max(n_s, n_d)
    arrs, checks = {}, []
    for name in ("rows", "cols", "kc", "kd", "r2c"):
        kind = r2c_kind if (name == "r2c" and r2c_kind is not None) else out_kind
        arrs[name], chk = ab.guarded((n,), np.int32, *kind)
        checks.append(chk)
    k, lm, n2, tot = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int64(-7)
    rc = lib.td_tick(cab, n_s, dem, n_d, dist, S, fill, thr, stop, P(arrs["rows"]), P(arrs["cols"]), ctypes.byref(k), ctypes.byref(lm),
                     P(arrs["kc"]), P(arrs["kd"]), ctypes.byref(n2), P(arrs["r2c"]), ctypes.byref(tot))
    for chk in checks:
        chk()
    return rc, arrs, (k.value, lm.value, n2.value, tot.value)


def check_tick(arrs, sc, ref, n_s, n_d, what):
    k, lm, n2, tot = sc
    n = max(n_s, n_d)
    assert k == len(ref["rows"]) <= n, what
    assert arrs["rows"][:k].tolist() == ref["rows"].tolist() and arrs["cols"][:k].tolist() == ref["cols"].tolist(), what
    assert lm == ref["lm"] and n2 == ref["n2"] and tot == ref["total"], (what, sc, ref["lm"], ref["n2"], ref["total"])
    assert arrs["kc"][:n_s - k].tolist() == ref["kc"].tolist() and arrs["kd"][:n_d - k].tolist() == ref["kd"].tolist(), what
    if ref["solved"]:
        p = arrs["r2c"][:n2]
        assert sorted(p.tolist()) == list(range(n2)), what
        assert int(ref["cost2"].astype(np.int64)[np.arange(n2), p].sum()) == tot, what
    else:
        assert (arrs["r2c"] == PAT32).all(), what   # left untouched (header: the tick has no input for the solver)


@pytest.mark.parametrize("n_s,n_d", TICK_SHAPES)
def test_tick(lib, n_s, n_d):
    rng = np.random.default_rng(7000 + 100 * n_s + n_d)
    n, S = max(n_s, n_d), 50
    cab, dem = rng.integers(0, S, n_s).astype(np.int32), rng.integers(0, S, n_d).astype(np.int32)
    table = rng.integers(0, 25, (S, S)).astype(np.int32)
    p_cab, p_dem, p_tab = Placed(cab), Placed(dem), Placed(table)
    ins, outs = cycle(IN_KINDS), cycle((("host", 0), ("pinned", 0)))
    ended_on_fill = 0
    for stop in sorted({-1, 0, 1, n - 1, n}):
        for thr, tk in ((10, None), (1, None), (10, ("host", 0)), (10, ("device", 0)), (-1, None)):
            dist = None if tk is None else table
            ref = oracle_tick(cab, dem, dist, BIG, thr, stop)
            ended_on_fill += int(ref["ran"] and ref["lm"] == BIG)
            first = None
            for _ in range(2):
                ik, ok_ = next(ins), next(outs)
                rc, arrs, sc = raw_tick(lib, P(p_cab(ik)), n_s, P(p_dem(ik)), n_d, None if tk is None else P(p_tab(tk)), S if tk else 0,
                                        BIG, thr, stop, ok_)
                ok(lib, rc)
                check_tick(arrs, sc, ref, n_s, n_d, (n_s, n_d, stop, thr, tk, ik, ok_))
                got = (sc, arrs["rows"][:sc[0]].tolist(), arrs["cols"][:sc[0]].tolist())
                first = first or got
                assert got == first
    assert ended_on_fill > 0 or n == 1   # a tick whose LCM ran out of cells below fill
    # results go to HOST arrays: a device row_to_col is refused and nothing is written
    rc, arrs, sc = raw_tick(lib, P(p_cab(("host", 0))), n_s, P(p_dem(("host", 0))), n_d, None, 0, BIG, 10, 1, ("host", 0), ("device", 0))
    assert rc == -1   # TD_EINVAL
    for name, a in arrs.items():
        assert (ab.host(a) == PAT32).all(), name


# ------------------------------------------------------------------------------------------------------------------
# td_lcm, td_lcm_batched
# ------------------------------------------------------------------------------------------------------------------
LCM_RULES = [
    # (library arguments: mask, threshold, stop_value_on, stop_value, stop_size, sum_below), the oracle's
    ((100, -1, 0, 0, -1, 2**62), dict(mask=100, threshold=-1)),                                               # heuristic.py
    ((BIG, 10, 0, 0, -1, BIG), dict(mask=BIG, threshold=10, sum_below=BIG)),                                  # greedy_opt.py
    ((BIG, -1, 1, BIG, 4, BIG), dict(mask=BIG, stop_value_on=1, stop_value=BIG, stop_size=4, sum_below=BIG, java_scan=1)),
    ((BIG, -1, 1, BIG, -1, BIG), dict(mask=BIG, stop_value_on=1, stop_value=BIG, stop_size=-1, sum_below=BIG, java_scan=1)),
]


def lcm_matrix(rng, n, rule):
    if rule == 0:
        return rng.integers(1, 40, (n, n)).astype(np.int32)
    c = rng.integers(0, 30, (n, n)).astype(np.int32)
    c[rng.random((n, n)) < 0.4] = BIG
    return c


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129])   # both sides of the level lists (64) and of the narrow copy (128)
def test_lcm(lib, n):
    rng = np.random.default_rng(500 + n)
    ins = cycle(IN_KINDS)
    pairs = cycle([(("host", 0), ("host", 0)), (("device", 0), ("device", 0)), (("host", 0), ("device", 0)), (("device", 0), ("host", 0))])
    for rule, (args, kw) in enumerate(LCM_RULES):
        c = lcm_matrix(rng, n, rule)
        p_c = Placed(c)
        for cap in sorted({0, 1, n // 2, n}):
            t_o, r_o, c_o, lm_o = oracle.lcm(c, max_iter=cap, **kw)
            for _ in range(2):
                ik, (rk, ck) = next(ins), next(pairs)
                rows, chk_r = ab.guarded((cap,), np.int32, *rk)
                cols, chk_c = ab.guarded((cap,), np.int32, *ck)
                k, tot, lm = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int32(-1)
                ok(lib, lib.td_lcm(n, P(p_c(ik)), *args, cap, P(rows), P(cols), ctypes.byref(k), ctypes.byref(tot), ctypes.byref(lm)))
                chk_r()
                chk_c()
                what = (n, rule, cap, ik, rk, ck)
                assert k.value == r_o.size <= cap, what
                assert ab.host(rows)[:k.value].tolist() == r_o.tolist() and ab.host(cols)[:k.value].tolist() == c_o.tolist(), what
                assert (tot.value, lm.value) == (t_o, lm_o), (what, tot.value, t_o, lm.value, lm_o)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129])
def test_lcm_batched(lib, n):
    rng = np.random.default_rng(900 + n)
    B = 3
    ns = np.array([0, 1, n], np.int32)
    p_ns = Placed(ns)
    kinds = cycle(itertools.product(IN_KINDS, HD, HD))
    for rule, (args, kw) in enumerate(LCM_RULES):
        slab = np.full((B, n, n), I32_MIN, np.int32)   # outside a model's block: would be every pick if read
        mats = []
        for b in range(B):
            m = lcm_matrix(rng, int(ns[b]), rule)
            slab[b, :ns[b], :ns[b]] = m
            mats.append(m)
        p_slab = Placed(slab)
        for _ in range(4):
            ik, ok_, nk = next(kinds)
            outs = {"rows": ab.guarded((B, n), np.int32, *ok_), "cols": ab.guarded((B, n), np.int32, *ok_),
                    "k": ab.guarded((B,), np.int32, *ok_), "tot": ab.guarded((B,), np.int64, *ok_), "lm": ab.guarded((B,), np.int32, *ok_)}
            ok(lib, lib.td_lcm_batched(B, n, P(p_ns(nk)), P(p_slab(ik)), *args, *(P(outs[q][0]) for q in ("rows", "cols", "k", "tot", "lm"))))
            for _, chk in outs.values():
                chk()
            rows, cols, k, tot, lm = (ab.host(outs[q][0]) for q in ("rows", "cols", "k", "tot", "lm"))
            for b, m in enumerate(mats):
                t_o, r_o, c_o, lm_o = oracle.lcm(m, **kw) if m.size else (0, np.zeros(0), np.zeros(0), None)
                kk = int(k[b])
                assert kk == r_o.size <= ns[b], (n, rule, b)
                assert rows[b, :kk].tolist() == r_o.tolist() and cols[b, :kk].tolist() == c_o.tolist(), (n, rule, b, ik, ok_, nk)
                if m.size:
                    assert (int(tot[b]), int(lm[b])) == (t_o, lm_o), (n, rule, b)
                else:
                    assert int(tot[b]) == 0


# ------------------------------------------------------------------------------------------------------------------
# the batched entry points: B = 3, strides 7 and 8, model sizes {0, 1, n}
# ------------------------------------------------------------------------------------------------------------------
def opt_outputs(shapes, kind, want):
    """{name: (view, check)} of guarded outputs; names not in `want` are left out (passed as NULL)"""
    return {name: ab.guarded(shape, dt, *kind) for name, (shape, dt) in shapes.items() if name in want}


def addr_of(outs, name):
    return P(outs[name][0]) if name in outs else None


def run_checks(outs):
    for _, chk in outs.values():
        chk()


@pytest.mark.parametrize("n", [7, 8])
def test_assign_batched(lib, n):
    rng = np.random.default_rng(n)
    B, ns = 3, np.array([0, 1, n], np.int32)
    slab = np.full((B, n, n), I32_MIN, np.int32)
    for b in range(B):
        slab[b, :ns[b], :ns[b]] = rng.integers(1, 40, (ns[b], ns[b]))
    p_slab, p_ns = Placed(slab), Placed(ns)
    shapes = {"r2c": ((B, n), np.int32), "tot": ((B,), np.int64), "dual": ((B,), np.int64), "price": ((B, n), np.int64)}
    first = None
    for ik, ok_, opt in itertools.product(IN_KINDS, HD, (True, False)):   # optional outputs present and NULL with every kind
        outs = opt_outputs(shapes, ok_, shapes if opt else ("r2c", "tot"))
        ok(lib, lib.td_assign_batched(B, n, P(p_ns(ik)), P(p_slab(ik)), *(addr_of(outs, q) for q in ("r2c", "tot", "dual", "price"))))
        run_checks(outs)
        r2c, tot = ab.host(outs["r2c"][0]), ab.host(outs["tot"][0])
        for b in range(B):
            k, c = int(ns[b]), slab[b, :ns[b], :ns[b]].astype(np.int64)
            assert (r2c[b, k:] == -1).all(), (n, b)          # the documented fill of the ragged tail
            assert sorted(r2c[b, :k].tolist()) == list(range(k))
            assert int(tot[b]) == (oracle.assign(c)[0] if k else 0) == int(c[np.arange(k), r2c[b, :k]].sum()), (n, b, ik, ok_)
            if opt:
                dual, v = ab.host(outs["dual"][0]), ab.host(outs["price"][0])
                assert (v[b, k:] == 0).all(), (n, b)
                assert int(dual[b]) == int(tot[b])
                if k:
                    assert int((c - v[b, None, :k]).min(1).sum() + v[b, :k].sum()) == int(dual[b])
        first = first if first is not None else (r2c, tot)
        assert np.array_equal(first[0], r2c) and np.array_equal(first[1], tot)


def ragged(models):
    off = np.zeros(len(models) + 1, np.int32)
    off[1:] = np.cumsum([len(m) for m in models])
    vals = np.concatenate(models).astype(np.int32) if models else np.zeros(0, np.int32)
    return off, np.ascontiguousarray(vals)


@pytest.mark.parametrize("n", [7, 8])
def test_build_assign_and_tick_batched(lib, n):
    rng = np.random.default_rng(70 + n)
    B, S, thr, stop = 3, 50, 10, 2
    shapes_sd = [(0, 0), (1, 1), (n, n - 2)]
    cabs = [rng.integers(0, S, a).astype(np.int32) for a, _ in shapes_sd]
    dems = [rng.integers(0, S, d).astype(np.int32) for _, d in shapes_sd]
    (co, cv), (do, dv) = ragged(cabs), ragged(dems)
    p = {q: Placed(x) for q, x in (("co", co), ("cv", cv), ("do", do), ("dv", dv))}
    nb = [max(a, d) for a, d in shapes_sd]
    ba_shapes = {"r2c": ((B, n), np.int32), "tot": ((B,), np.int64), "dual": ((B,), np.int64)}
    tk_names = ("rows", "cols", "k", "lm", "kc", "kd", "n2", "r2c", "tot", "dual")
    tk_shapes = {q: ((B, n), np.int32) for q in ("rows", "cols", "kc", "kd", "r2c")}
    tk_shapes.update({q: ((B,), np.int32) for q in ("k", "lm", "n2")})
    tk_shapes.update({q: ((B,), np.int64) for q in ("tot", "dual")})
    first_ba = first_tk = None
    for ik, ok_, opt in itertools.product(IN_KINDS, HD, (True, False)):   # optional outputs present and NULL with every kind
        a_in = [P(p[q](ik)) for q in ("co", "cv", "do", "dv")]
        outs = opt_outputs(ba_shapes, ok_, ba_shapes if opt else ("r2c", "tot"))
        ok(lib, lib.td_build_assign_batched(B, n, *a_in, None, 0, BIG, thr, *(addr_of(outs, q) for q in ("r2c", "tot", "dual"))))
        run_checks(outs)
        r2c, tot = ab.host(outs["r2c"][0]), ab.host(outs["tot"][0])
        for b in range(B):
            k, cost = oracle.cost_build(cabs[b], dems[b], None, BIG, thr)
            assert k == nb[b] and (r2c[b, k:] == -1).all(), (n, b)
            assert sorted(r2c[b, :k].tolist()) == list(range(k))
            assert int(tot[b]) == (oracle.assign(cost)[0] if k else 0) == int(cost.astype(np.int64)[np.arange(k), r2c[b, :k]].sum())
            if opt:
                assert int(ab.host(outs["dual"][0])[b]) == int(tot[b])
        first_ba = first_ba if first_ba is not None else (r2c, tot)
        assert np.array_equal(first_ba[0], r2c) and np.array_equal(first_ba[1], tot)
        # the tick of the same models; kept lists and the dual bound are optional
        outs = opt_outputs(tk_shapes, ok_, tk_names if opt else [q for q in tk_names if q not in ("kc", "kd", "dual")])
        ok(lib, lib.td_tick_batched(B, n, *a_in, None, 0, BIG, thr, stop, *(addr_of(outs, q) for q in tk_names)))
        run_checks(outs)
        g = {q: ab.host(v[0]) for q, v in outs.items()}
        for b, (a, d) in enumerate(shapes_sd):
            ref = oracle_tick(cabs[b], dems[b], None, BIG, thr, stop)
            kk = int(g["k"][b])
            what = (n, b, ik, ok_)
            assert kk == len(ref["rows"]) <= n, what
            assert g["rows"][b, :kk].tolist() == ref["rows"].tolist() and g["cols"][b, :kk].tolist() == ref["cols"].tolist(), what
            assert (int(g["lm"][b]), int(g["n2"][b]), int(g["tot"][b])) == (ref["lm"], ref["n2"], ref["total"]), what
            if opt:
                assert g["kc"][b, :a - kk].tolist() == ref["kc"].tolist() and g["kd"][b, :d - kk].tolist() == ref["kd"].tolist(), what
                assert int(g["dual"][b]) == int(g["tot"][b])
            if ref["solved"]:
                q = g["r2c"][b, :ref["n2"]]
                assert sorted(q.tolist()) == list(range(ref["n2"])), what
                assert int(ref["cost2"].astype(np.int64)[np.arange(ref["n2"]), q].sum()) == ref["total"], what
                assert (g["r2c"][b, ref["n2"]:] == -1).all(), what   # the documented tail: -1 beyond n_rest(b)
            else:
                assert (g["r2c"][b] == -1).all(), what   # no solve (an empty model, or the LCM ended on fill): the whole row
        key = (g["rows"][2, :int(g["k"][2])].tolist(), g["tot"].tolist(), g["n2"].tolist())
        first_tk = first_tk or key
        assert key == first_tk


def best_matching(W):
    """maximum-weight matching of a small general graph by exhaustion (edge {i, j}: max(W[i][j], W[j][i]), <= 0: none)"""
    m = W.shape[0]
    w = np.maximum(W, W.T).astype(np.int64)

    def go(free):
        if len(free) < 2:
            return 0
        i, rest = free[0], free[1:]
        best = go(rest)
        for q, j in enumerate(rest):
            if w[i, j] > 0:
                best = max(best, int(w[i, j]) + go(rest[:q] + rest[q + 1:]))
        return best
    return go(tuple(range(m)))


@pytest.mark.parametrize("n", [7, 8])
def test_match_batched(lib, n):
    rng = np.random.default_rng(700 + n)
    B, ns = 3, np.array([0, 1, n], np.int32)
    slab = np.full((B, n, n), 10**9, np.int32)   # outside a model's block: would join every matching if read
    for b in range(B):
        W = rng.integers(-5, 30, (ns[b], ns[b]))
        slab[b, :ns[b], :ns[b]] = W
    p_slab, p_ns = Placed(slab), Placed(ns)
    names = ("mate", "tot", "dual", "y", "par", "z")
    shapes = {"mate": ((B, n), np.int32), "tot": ((B,), np.int64), "dual": ((B,), np.int64), "y": ((B, n), np.int64),
              "par": ((B, 2 * n), np.int32), "z": ((B, n), np.int64)}
    first = None
    for ik, ok_, opt in itertools.product(IN_KINDS, HD, (True, False)):   # optional outputs present and NULL with every kind
        outs = opt_outputs(shapes, ok_, names if opt else ("mate", "tot"))
        ok(lib, lib.td_match_batched(B, n, P(p_ns(ik)), P(p_slab(ik)), *(addr_of(outs, q) for q in names)))
        run_checks(outs)
        mate, tot = ab.host(outs["mate"][0]), ab.host(outs["tot"][0])
        for b in range(B):
            k = int(ns[b])
            W = slab[b, :k, :k]
            w = np.maximum(W, W.T).astype(np.int64)
            assert (mate[b, k:] == -1).all(), (n, b)           # the documented fill of the ragged tail
            got = 0
            for i in range(k):
                j = int(mate[b, i])
                assert j == -1 or (0 <= j < k and j != i and int(mate[b, j]) == i and w[i, j] > 0), (n, b, i, j)
                got += int(w[i, j]) if j > i else 0
            assert got == int(tot[b]) == best_matching(W), (n, b, ik, ok_)
            if opt:
                assert int(ab.host(outs["dual"][0])[b]) == int(tot[b])
        first = first if first is not None else (mate, tot)
        assert np.array_equal(first[0], mate) and np.array_equal(first[1], tot)


def best_pools(frm, to):
    """(count, total) of the lexicographic optimum of every-pair pools of two on a line, by exhaustion"""
    import pool_opt_data as D
    c, _ = D.pair_costs(frm, to)
    m = len(frm)
    und = np.minimum(c, c.T)

    def go(free):
        if len(free) < 2:
            return (0, 0)
        i, rest = free[0], free[1:]
        best = go(rest)
        for q, j in enumerate(rest):
            k, t = go(rest[:q] + rest[q + 1:])
            cand = (k + 1, t + int(und[i, j]))
            if cand[0] > best[0] or (cand[0] == best[0] and cand[1] < best[1]):
                best = cand
        return best
    return go(tuple(range(m)))


@pytest.mark.parametrize("n", [7, 8])
def test_pool2_batched(lib, n):
    rng = np.random.default_rng(800 + n)
    B, S, half = 3, 50, n // 2
    sizes = [0, 1, n]
    froms = [rng.integers(0, S, m).astype(np.int32) for m in sizes]
    tos = [rng.integers(0, S, m).astype(np.int32) for m in sizes]
    (off, fv), (_, tv) = ragged(froms), ragged(tos)
    p_off, p_f, p_t = Placed(off), Placed(fv), Placed(tv)
    # model b's pools sit at b * (n / 2): with n = 7 the extent is B * 3 records and the guards start right behind it
    shapes = {q: ((B * half,), np.int32) for q in ("a", "b", "plan", "cost")}
    shapes.update({"k": ((B,), np.int32), "tot": ((B,), np.int64)})
    names = ("a", "b", "plan", "cost", "k", "tot")
    for optimal in (0, 1):
        first = None
        for ik, ok_ in itertools.product(IN_KINDS, HD):
            outs = opt_outputs(shapes, ok_, names)
            ok(lib, lib.td_pool2_batched(B, n, P(p_off(ik)), P(p_f(ik)), P(p_t(ik)), None, 0, 0.0, optimal, *(addr_of(outs, q) for q in names)))
            run_checks(outs)
            g = {q: ab.host(outs[q][0]) for q in names}
            got_all = []
            for b, m in enumerate(sizes):
                k = int(g["k"][b])
                assert k <= m // 2 <= half
                got = [tuple(int(g[q][b * half + i]) for q in ("a", "b", "plan", "cost")) for i in range(k)]
                got_all.append(got)
                assert int(g["tot"][b]) == sum(x[3] for x in got)
                if optimal == 0:
                    assert got == OracleBackend().find_pool(froms[b], tos[b]), (n, b, ik, ok_)
                else:
                    used = [x for q in got for x in q[:2]]
                    assert len(set(used)) == len(used) and all(0 <= x < m for x in used)
                    assert (k, int(g["tot"][b])) == best_pools(froms[b], tos[b]), (n, b, ik, ok_)
            first = first or got_all
            assert got_all == first


# ------------------------------------------------------------------------------------------------------------------
# td_pool2, td_pool_n, td_pool_merge
# ------------------------------------------------------------------------------------------------------------------
POOL_IN = (("host", 0), ("pinned", 0), ("device", 1))


@pytest.mark.parametrize("n", [0, 1, 2, 5, 64, 65])
def test_pool2(lib, n):
    rng = np.random.default_rng(60 + n)
    frm, to = rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
    ref = OracleBackend().find_pool(frm, to)
    p_f, p_t = Placed(frm), Placed(to)
    cap = n // 2                                       # an odd n has capacity n / 2
    for ik, ok_ in itertools.product(POOL_IN, HD):
        outs = [ab.guarded((cap,), np.int32, *ok_) for _ in range(4)]
        k = ctypes.c_int32(-1)
        ok(lib, lib.td_pool2(n, P(p_f(ik)), P(p_t(ik)), None, 0, *(P(o[0]) for o in outs), ctypes.byref(k)))
        for _, chk in outs:
            chk()
        assert k.value == len(ref) <= cap
        a, b, plan, cost = (ab.host(o[0]) for o in outs)
        assert [(int(a[i]), int(b[i]), int(plan[i]), int(cost[i])) for i in range(k.value)] == ref, (n, ik, ok_)


def random_demand(rng, n, max_wait, losses, stands=50):
    frm = rng.integers(0, stands, n)
    to = np.clip(frm + rng.integers(1, 9, n) * rng.choice([-1, 1], n), 0, stands - 1)
    to = np.where(to == frm, np.where(frm > 0, frm - 1, 1), to)
    return [np.ascontiguousarray(x.astype(np.int32)) for x in (frm, to, rng.integers(0, max_wait + 1, n), rng.choice(losses, n))]


def raw_pool_n(lib, k, n, addrs, first0, first1, max_pools, out_kind):
    """-> (records of the first n_pools pools, n_happy); the output has exactly max_pools records between its guards"""
    w = 2 * k + 1
    out, check = ab.guarded((max_pools * w,), np.int32, *out_kind)
    m, nh = ctypes.c_int32(-1), ctypes.c_int64(-1)
    ok(lib, lib.td_pool_n(k, n, *addrs, None, 0, first0, first1, 0, max_pools, P(out), ctypes.byref(m), ctypes.byref(nh)))
    check()
    assert 0 <= m.value <= max_pools
    return ab.host(out)[:m.value * w].reshape(m.value, w), nh.value


@pytest.mark.parametrize("k", [2, 3, 4])
def test_pool_n_and_merge(lib, k):
    import pool_fixtures as pf
    rng = np.random.default_rng(40 + k)
    w = 2 * k + 1
    for n in sorted({k, 17, 40}):
        d = random_demand(rng, n, 5, [10, 50])
        exp, nh_o = oracle.pool_n(k, d[0], d[1], d[2], d[3], None, 0, n, cap=3000000)
        m = exp.shape[0]
        p = [Placed(x) for x in d]
        caps = sorted({max(1, m // 2), max(1, m - 1), m + 3})   # below and above the number of pools the oracle finds
        for ik, ok_, cap in itertools.product(POOL_IN, HD, caps):
            got, nh = raw_pool_n(lib, k, n, [P(q(ik)) for q in p], 0, n, cap, ok_)
            assert nh == nh_o, (k, n)
            # a short max_pools: the first max_pools pools of the full list (the greedy stops when the output is full)
            assert got.tolist() == exp[:cap].tolist(), (k, n, cap, ik, ok_, m)
        assert any(c < m for c in caps) or m <= 1
        # two first-pick-up slices, merged: findpool.c's merge restated on the host
        lists = [oracle.pool_n(k, d[0], d[1], d[2], d[3], None, f0, f1, cap=3000000)[0] for f0, f1 in ((0, n // 2), (n // 2, n))]
        ref = pf.merge_restatement(k, [x.tolist() for x in lists])
        allp = np.ascontiguousarray(np.concatenate(lists, 0).astype(np.int32)).reshape(-1, w)
        if allp.shape[0] == 0:
            continue
        p_in = Placed(allp)
        mcaps = sorted({max(1, len(ref) // 2), max(1, len(ref) - 1), len(ref) + 2})   # below and above, met by host and device outputs alike
        for ik, ok_, cap in itertools.product(POOL_IN, HD, mcaps):
            out, check = ab.guarded((cap * w,), np.int32, *ok_)
            mo = ctypes.c_int32(-1)
            ok(lib, lib.td_pool_merge(k, n, allp.shape[0], P(p_in(ik)), 1 if k == 4 else 0, cap, P(out), ctypes.byref(mo)))
            check()
            assert 0 <= mo.value <= cap
            assert ab.host(out)[:mo.value * w].reshape(-1, w).tolist() == ref[:cap], (k, n, cap, ik, ok_)


# ------------------------------------------------------------------------------------------------------------------
# td_lcm_shard_*, td_shard_*: one in-process pair, n = 65, rows split 33 + 32, rows in a misaligned device view
# ------------------------------------------------------------------------------------------------------------------
def test_shard_pair(lib):
    import torch
    from taxidispatcher_amd import sharded
    n, world = 65, 2
    rng = np.random.default_rng(65)
    cost = rng.integers(0, 30, (n, n)).astype(np.int32)
    bounds = [sharded.shard_bounds(n, world, r)[:2] for r in range(world)]
    assert [b[1] for b in bounds] == [33, 32]
    views = [ab.place(cost[r0:r0 + k], "device", 1) for r0, k in bounds]
    assert all(P(v) % 16 == 4 for v in views)
    checks = []

    # --- the lowest-cost method in rounds, every round vector between guards
    args, kw = LCM_RULES[1]
    rows, cols = np.zeros(n, np.int32), np.zeros(n, np.int32)
    k, tot, lm = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
    ok(lib, lib.td_lcm(n, cost.ctypes.data, *args, n, rows.ctypes.data, cols.ctypes.data, ctypes.byref(k), ctypes.byref(tot), ctypes.byref(lm)))
    t_o, r_o, c_o, lm_o = oracle.lcm(cost, **kw)
    assert (tot.value, lm.value, rows[:k.value].tolist(), cols[:k.value].tolist()) == (t_o, lm_o, r_o.tolist(), c_o.tolist())

    class GuardedLcmShard(sharded.HipLcmShard):
        def round_colmin(self, limit, out):
            g, chk = ab.guarded((n,), np.int64, "device", 1)
            ok(lib, lib.td_lcm_shard_round_colmin(self.h, int(limit), P(g)))
            chk()
            out.copy_(g)
            torch.cuda.synchronize()

        def round_apply(self, limit, colmin, out):
            torch.cuda.synchronize()
            g, chk = ab.guarded((n,), np.int64, "device", 1)
            ok(lib, lib.td_lcm_shard_round_apply(self.h, int(limit), P(colmin), P(g)))
            chk()
            out.copy_(g)
            torch.cuda.synchronize()

        def round_commit(self, taken):
            torch.cuda.synchronize()
            ok(lib, lib.td_lcm_shard_round_commit(self.h, P(taken)))

    shards = []
    try:
        for (r0, nr), v in zip(bounds, views):
            shards.append(GuardedLcmShard(n, r0, nr, P(v)))   # an int is handed on as the raw address
        got = sharded.lcm_sharded(shards, None, n, mask=args[0], threshold=args[1], stop_value_on=args[2], stop_value=args[3],
                                  stop_size=args[4], sum_below=args[5])
    finally:
        for s in shards:
            s.close()
    assert got == (t_o, r_o.tolist(), c_o.tolist(), lm_o)

    # --- the optimal assignment over the two shards, the bid keys between guards
    class GuardedShard(sharded.HipShard):
        def new_keys(self):
            g, chk = ab.guarded((self.lib.td_shard_keys_len(self.h) + 16,), np.int64, "device", 1)
            g.zero_()
            torch.cuda.synchronize()
            checks.append(chk)
            return g

    shards = []
    try:
        for (r0, nr), v in zip(bounds, views):
            shards.append(GuardedShard(n, r0, nr, P(v), share_torch_stream=False))
        r2c, total, dual, info = sharded.solve_shards_in_process(shards, want_dual=True)
        for chk in checks:
            chk()
    finally:
        for s in shards:
            s.close()
    assert len(checks) == world
    ref_r2c = np.zeros(n, np.int32)
    t, d = ctypes.c_int64(0), ctypes.c_int64(0)
    ok(lib, lib.td_assign(n, cost.ctypes.data, ref_r2c.ctypes.data, ctypes.byref(t), ctypes.byref(d)))
    check_assignment(cost, r2c, total, dual, oracle.assign(cost)[0], "shards")
    assert total == t.value == d.value
    for v, (r0, nr) in zip(views, bounds):
        assert np.array_equal(ab.host(v), cost[r0:r0 + nr])


# ------------------------------------------------------------------------------------------------------------------
# "the library keeps no pointer past return"
# ------------------------------------------------------------------------------------------------------------------
def thrice(call):
    """call(seed) runs the entry point on fresh buffers made from `seed`, overwrites every input with the pattern after the
    call returns and gives the result: first data, other data, the first data again"""
    first, other, again = call(1), call(2), call(1)
    assert first == again and repr(first) == repr(again)
    return first, other


@pytest.mark.parametrize("kind", IN_KINDS)
def test_keeps_no_pointer_past_return(lib, kind):
    n = 130

    def assign(seed):
        c = ab.place(np.random.default_rng(seed).integers(0, 1000, (n, n)).astype(np.int32), *kind)
        r2c, chk = ab.guarded((n,), np.int32, "host")
        t, d = ctypes.c_int64(0), ctypes.c_int64(0)
        ok(lib, lib.td_assign(n, P(c), P(r2c), ctypes.byref(t), ctypes.byref(d)))
        ab.scribble(c)
        chk()
        return (t.value, d.value, r2c.tolist())

    def lcm(seed):
        c = ab.place(np.random.default_rng(seed).integers(0, 30, (n, n)).astype(np.int32), *kind)
        rows, c1 = ab.guarded((n,), np.int32, "host")
        cols, c2 = ab.guarded((n,), np.int32, "host")
        k, t, lm = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
        ok(lib, lib.td_lcm(n, P(c), BIG, 10, 0, 0, -1, BIG, n, P(rows), P(cols), ctypes.byref(k), ctypes.byref(t), ctypes.byref(lm)))
        ab.scribble(c)
        c1(), c2()
        return (k.value, t.value, lm.value, rows[:k.value].tolist(), cols[:k.value].tolist())

    def positions(seed):
        rng = np.random.default_rng(seed)
        return [ab.place(rng.integers(0, 50, m).astype(np.int32), *kind) for m in (n, n - 40)]

    def cost_build(seed):
        cab, dem = positions(seed)
        tab = ab.place(np.random.default_rng(seed).integers(0, 30, (50, 50)).astype(np.int32), *kind)
        out, chk = ab.guarded((n, n), np.int32, "device")
        ok(lib, lib.td_cost_build(P(cab), None, n, P(dem), None, n - 40, P(tab), 50, BIG, 10, 0, P(out)))
        ok(lib, lib.td_synchronize())
        for x in (cab, dem, tab):
            ab.scribble(x)
        chk()
        return ab.host(out).tolist()

    def tick(seed):
        cab, dem = positions(seed)
        rc, arrs, sc = raw_tick(lib, P(cab), n, P(dem), n - 40, None, 0, BIG, 10, 60, ("host", 0))
        ok(lib, rc)
        ab.scribble(cab), ab.scribble(dem)
        return (sc, arrs["rows"][:sc[0]].tolist(), arrs["cols"][:sc[0]].tolist(), arrs["kc"][:n - sc[0]].tolist(), arrs["r2c"][:sc[2]].tolist())

    def pool_n(seed):
        d = [ab.place(x, *kind) for x in random_demand(np.random.default_rng(seed), 40, 6, [30, 90])]
        got, nh = raw_pool_n(lib, 3, 40, [P(x) for x in d], 0, 40, 14, ("host", 0))
        for x in d:
            ab.scribble(x)
        return (nh, got.tolist())

    for call in (assign, lcm, cost_build, tick, pool_n):
        first, other = thrice(call)
        assert first != other, call.__name__   # the second call did work on other data


# ------------------------------------------------------------------------------------------------------------------
# the stream rule of td_set_stream
# ------------------------------------------------------------------------------------------------------------------
CHAIN = 300


def chained(torch, big, values):
    """`values` (int64 numpy) arrive in the first cells of `big` at the END of a few hundred dependent in-place operations
    on all 2^24 elements, queued on the current stream: whoever reads them without waiting for this stream reads the
    pattern the tensor was filled with.  Returns the int32 device tensor of the values (also queued)."""
    m = values.size
    big.fill_(-(CHAIN + 1))
    big[:m] = torch.from_numpy(values - (CHAIN + 1)).to(big.device, non_blocking=False)
    for _ in range(CHAIN):
        big.add_(1)
    big.add_(1)
    return big[:m].to(torch.int32)


STREAMS = 4   # HIP maps a process's streams onto a few hardware queues (4 by default) and two streams on one queue run in
              # submission order: with four side streams alive at once, at least three do not share the library's own queue


def test_stream_rule(lib):
    """td_set_stream: the library must enqueue on the caller's stream.  Inputs are made on a torch side stream by a long chain
    of dependent kernels and handed over with no synchronisation; a library that enqueued elsewhere would read them early.
    Every stream gets other data, so that nothing left in recycled memory by the previous one can pass for it."""
    import torch
    n, S = 1024, 50
    rng = np.random.default_rng(99)
    cells = rng.integers(10, 41, n * n)
    ref_total = oracle.assign(cells.reshape(n, n).astype(np.int32))[0]
    streams = [torch.cuda.Stream() for _ in range(STREAMS)]
    big = torch.empty(1 << 24, dtype=torch.int64, device="cuda")
    r2c, check_r = ab.guarded((n,), np.int32, "host")
    torch.cuda.synchronize()
    try:
        for i, s in enumerate(streams):
            assert s.cuda_stream != 0
            cab, dem = rng.integers(0, S, n), rng.integers(0, S, n - 300)
            _, ref_cost = oracle.cost_build(cab, dem, None, BIG, 10)
            out, check = ab.guarded((n, n), np.int32, "device")
            ok(lib, lib.td_set_stream(ctypes.c_void_p(s.cuda_stream)))
            with torch.cuda.stream(s):
                # td_cost_build, device destination: inputs complete in the stream's order, the output ready in its order
                pos = chained(torch, big, np.concatenate([cab, dem]))
                ok(lib, lib.td_cost_build(P(pos), None, n, P(pos) + 4 * n, None, n - 300, None, 0, BIG, 10, 0, P(out)))
                got = (out + 0).cpu()          # a torch operation on s that reads the result, then the copy home
                assert np.array_equal(got.numpy(), ref_cost), i
                # td_assign returns after its results are complete; its input is still being made when it is called
                # (every cell i larger than on the stream before: the same optimum, n * i more in total)
                cost = chained(torch, big, cells + i)
                tot, dual = ctypes.c_int64(-1), ctypes.c_int64(-2)
                ok(lib, lib.td_assign(n, P(cost), P(r2c), ctypes.byref(tot), ctypes.byref(dual)))
                assert tot.value == dual.value == ref_total + n * i, i
                assert sorted(r2c.tolist()) == list(range(n))
                assert int(cells.reshape(n, n)[np.arange(n), r2c].sum()) == ref_total
            torch.cuda.synchronize()
            check()
            check_r()
    finally:
        torch.cuda.synchronize()
        ok(lib, lib.td_set_stream(None))
    # back on the library's own stream, the default rule: inputs complete before the call
    t2, d2 = ctypes.c_int64(-1), ctypes.c_int64(-2)
    ok(lib, lib.td_assign(n, P(cost), P(r2c), ctypes.byref(t2), ctypes.byref(d2)))
    assert t2.value == d2.value == ref_total + n * (STREAMS - 1)


# ------------------------------------------------------------------------------------------------------------------
# life cycle: td_init -> every family -> td_shutdown -> td_init -> the same calls, in one fresh child process
# ------------------------------------------------------------------------------------------------------------------
LIFE_CYCLE_CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, @ROOT@)
import taxidispatcher_amd as td
from taxidispatcher_amd import _ffi, sharded

lib = _ffi.load()


def ws():
    b = ctypes.c_int64(-1)
    assert lib.td_workspace_bytes(ctypes.byref(b)) == 0
    return b.value


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if hasattr(x, "tolist"):
        return x.tolist()
    return x


def one_round():
    rng = np.random.default_rng(5)
    res = {}
    c = rng.integers(10, 41, (96, 96)).astype(np.int32)
    cab, dem = rng.integers(0, 50, 90), rng.integers(0, 50, 70)
    frm, to = rng.integers(0, 50, 31), rng.integers(0, 50, 31)
    pf_ = rng.integers(0, 50, 24)
    demand = np.stack([np.arange(24), pf_, (pf_ + rng.integers(1, 9, 24)) % 50, rng.integers(0, 6, 24), rng.choice([30, 90], 24)], 1)
    cb = rng.integers(1, 40, (4, 33, 33)).astype(np.int32)
    cabs, dems = [cab[:20], cab[20:50], cab[:0]], [dem[:25], dem[25:40], dem[:3]]
    res["assign"] = td.assign(c, want_dual=True)
    res["build_assign"] = td.build_assign(cab, dem, None, threshold=10, want_dual=True)
    res["tick"] = td.tick(cab, dem, None, drop_time=10, max_non_lcm=30)
    res["lcm"] = td.LCM(96, c, threshold=20, with_pairs=True)
    res["pool2"] = td.find_pool(frm, to)
    lists = [td.find_pool_n(3, demand, child=t, children=2)[0] for t in range(2)]   # max_happy = 0: the default plan buffer
    res["pool_n"] = lists
    res["merge"] = td.merge_pools(3, 24, lists)
    res["assign_batched"] = td.assign_batched(cb, want_dual=True, want_prices=True)
    res["lcm_batched"] = td.LCM_batched(cb, mask=100)
    res["build_assign_batched"] = td.build_assign_batched(cabs, dems, None, threshold=10, want_dual=True)
    res["tick_batched"] = td.tick_batched(cabs, dems, None, drop_time=10, max_non_lcm=5)
    res["match"] = td.match_batched([cb[0], cb[1][:7, :7]])
    res["pool2_batched"] = [td.pool2_batched([frm, frm[:9]], [to, to[:9]], None, None, optimal=o) for o in (False, True)]
    grown = ws()
    assert grown > 2 * 8 * (1 << 22), grown   # td_pool_n's default plan buffers alone are 64 MiB
    # handles: after each destroy the workspace is back at its size before the matching create
    before = ws()
    with td.Solver() as sv:
        res["solver"] = [sv.assign(c, want_dual=True), sv.build_assign(cab, dem, None, threshold=10, want_dual=True)]
        assert ws() > before
    assert ws() == before, ("td_solver_destroy", ws(), before)
    n = 65
    c65 = rng.integers(0, 30, (n, n)).astype(np.int32)
    bounds = [sharded.shard_bounds(n, 2, r)[:2] for r in range(2)]
    shards = [sharded.HipShard(n, r0, k, np.ascontiguousarray(c65[r0:r0 + k]), share_torch_stream=False) for r0, k in bounds]
    assert ws() > before
    try:
        res["shards"] = sharded.solve_shards_in_process(shards, want_dual=True)[:3]
    finally:
        for s in shards:
            s.close()
    assert ws() == before, ("td_shard_destroy", ws(), before)
    ls = [sharded.HipLcmShard(n, r0, k, np.ascontiguousarray(c65[r0:r0 + k])) for r0, k in bounds]
    assert ws() > before
    try:
        res["lcm_shards"] = sharded.lcm_sharded(ls, None, n, mask=250000, threshold=10, sum_below=250000)
    finally:
        for s in ls:
            s.close()
    assert ws() == before, ("td_lcm_shard_destroy", ws(), before)
    return plain(res)


assert ws() == 0                       # callable before td_init
rounds = []
for r in range(2):
    td.init(0)
    rounds.append(one_round())
    print("round", r, "done, workspace", ws(), flush=True)
    td.shutdown()
    assert ws() == 0, ("td_shutdown left device memory behind", ws())
for key in rounds[0]:
    assert repr(rounds[0][key]) == repr(rounds[1][key]), key
assert rounds[0]["assign"][1] == rounds[0]["assign"][2] == rounds[0]["solver"][0][1]
print("life cycle ok")
""".replace("@ROOT@", repr(ROOT))


def test_life_cycle_in_a_child_process():
    """the session fixture owns the library in this process, so the sequence runs in a child (one more process with the
    GPU open, nothing else started); the child stops at its first failing step"""
    r = subprocess.run([sys.executable, "-c", LIFE_CYCLE_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "child failed:\n" + r.stdout[-4000:] + r.stderr[-4000:]
    assert "life cycle ok" in r.stdout
