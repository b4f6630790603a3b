"""td_tick on the case table of tests/tick_path_cases.py: every constant by which csrc/td_tick.hip and csrc/td_lcm.hip choose
among the stands LCM, hinted / redone / measured level lists and k_lcm_loop, the staged-copy and shrink-slice edges, and
every relation between fill and threshold -- each case against the oracle's tick pipeline bit for bit, twice, and through
td_tick_batched as a batch of one where its size limits allow.

Which path ran is observable for the stands LCM alone: it is the one path on which no n x n int32 matrix exists, so
td_tick's workspace (td_tick_release_workspace + td_workspace_bytes) grows by less than 4 n^2 bytes on it and by at least
that much on every other.  Hinted, redone and measured lists and k_lcm_loop leave no such trace: for them the table can
only place a case on each side of every edge and hold the answers to the oracle.  The stands-eligible cases also run
through the matrix path, in one child process with TD_LCM_STANDS=0 (the switch is read once per process)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tick_path_cases as T
from test_gpu_tick_batched import check_tick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("lcm_rows", "lcm_cols", "lcm_min_val", "kept_cabs", "kept_dems", "n_rest", "row_to_col", "total", "solved")


def run(td, c, device=False):
    _, cab, dem, dist, fill, thr, stop, _ = c
    if device:
        import torch
        cab, dem = torch.from_numpy(cab.copy()).cuda(), torch.from_numpy(dem.copy()).cuda()
        dist = None if dist is None else torch.from_numpy(dist.copy()).cuda()
    return td.tick(cab, dem, dist, big_cost=fill, drop_time=thr, max_non_lcm=stop)


def check(got, ref, what):
    """check_tick without its dual_bound line: td_tick has no dual output"""
    check_tick(dict(got, dual_bound=got["total"]), ref, what)


def same(a, b, what, keys=KEYS):
    for key in keys:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (what, key)


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_tick_against_the_oracle(td, name):
    c = T.case(name)
    ref = T.reference(name)
    got = run(td, c)
    check(got, ref, name)
    same(run(td, c), got, name + ": second run")
    if T.batched_ok(c):
        _, cab, dem, dist, fill, thr, stop, _ = c
        one = td.tick_batched([cab], [dem], dist, big_cost=fill, drop_time=thr, max_non_lcm=stop)
        assert len(one) == 1
        check_tick(one[0], ref, name + ": td_tick_batched")   # with dual_bound == total
        # (its solver is another one: among equal optima row_to_col may differ, check_tick holds both to the remainder's cells)
        same(one[0], got, name + ": td_tick_batched against td_tick", [k for k in KEYS if k != "row_to_col"])


@pytest.mark.parametrize("name", T.DEVICE_CASES)
def test_positions_and_table_on_the_device(td, name):
    c = T.case(name)
    got = run(td, c, device=True)
    check(got, T.reference(name), name)
    same(run(td, c, device=True), got, name + ": second run")
    same(run(td, c), got, name + ": host arrays")


def workspace_growth(td, c):
    """bytes td_tick's own buffers take for one tick of c.  A first tick brings the library's other grow-only buffers (the
    LCM's, the solver's) to their size for this model, so that the difference is td_tick's buffers alone."""
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()

    def held():
        b = ctypes.c_int64(-1)
        assert lib.td_workspace_bytes(ctypes.byref(b)) == 0
        return b.value

    run(td, c)
    lib.td_tick_release_workspace()
    before = held()
    got = run(td, c)
    return held() - before, got


@pytest.mark.parametrize("base,others", T.WITNESS, ids=[w[0] for w in T.WITNESS])
def test_only_the_stands_path_goes_without_a_matrix(td, base, others):
    for name, on_stands in [(base, True)] + [(m, False) for m in others]:
        c = T.case(name)
        n = max(len(c[1]), len(c[2]))
        grown, got = workspace_growth(td, c)
        check(got, T.reference(name), name)
        assert (grown < 4 * n * n) == on_stands, (name, grown, 4 * n * n)


_MATRIX_CHILD = r"""
import ctypes, os, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import taxidispatcher_amd as td
import tick_path_cases as T
import test_gpu_tick_paths as G
from taxidispatcher_amd import _ffi
assert os.environ["TD_LCM_STANDS"] == "0"
td.init(0)
cnt = bad = 0
for name in T.CASE_NAMES:
    c = T.case(name)
    if not T.stands_eligible(c):
        continue
    cnt += 1
    try:
        G.check(G.run(td, c), T.reference(name), name)
    except AssertionError as e:
        bad += 1
        print("FAIL", name, str(e)[:300], flush=True)
c = T.case("s_300x200")
grown, _ = G.workspace_growth(td, c)
print("matrix path: %%d" %% int(grown >= 4 * 300 * 300))
print("stands-eligible cases through the matrix path: %%d cases, %%d failures" %% (cnt, bad))
td.shutdown()
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_stands_cases_through_the_matrix_path(td):
    """TD_LCM_STANDS=0: the cases the stands LCM would take, through the cost matrix and the level lists / k_lcm_loop"""
    r = subprocess.run([sys.executable, "-c", _MATRIX_CHILD], env=dict(os.environ, TD_LCM_STANDS="0"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    m = re.search(r"(\d+) cases, (\d+) failures", r.stdout)
    assert m and "FAIL" not in r.stdout, r.stdout[-3000:]
    assert "matrix path: 1" in r.stdout, r.stdout[-2000:]   # the switch was read: s_300x200 built its matrix
    assert int(m.group(1)) == sum(T.stands_eligible(T.case(n)) for n in T.CASE_NAMES) and int(m.group(2)) == 0
