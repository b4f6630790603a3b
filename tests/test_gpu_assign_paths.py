"""Every branch of td_assign's host driver against the results recorded before the driver was split into steps
(csrc/td_assign.hip: assign_impl and its step_* functions; profiles/assign_driver).

tools/assign_paths_golden.py solves one small seeded instance per branch, each with a device and with a host row_to_col,
in child processes (one per environment switch); tests/golden/assign_paths_parent.json is its output with the parent
commit's library (two runs there gave the same file).  Everything must be equal: return code, total, dual bound, the sha1
of row_to_col and every word of last_stats() but lcm_path.  The script also records that row_to_col is a permutation,
what it costs in the matrix and, for n <= 600, that the total is the CPU oracle's.  The block-local start and its one-trip
and read-back variants (n >= 12 288) are pinned by test_gpu_hop_chain.py, test_gpu_hop_fold.py and test_gpu_one_trip.py.

Which case covers which branch (bytes per cell / narrow prices / transposed / warm rounds / line_path as the parent's
statistics recorded them; the passes as TD_DEBUG printed them at the parent commit):
  n0, n1                  the trivial sizes
  line_64                 |a - b| table: the line attempt accepted, balanced (line_path has LP_BALANCED | LP_ACCEPTED)
  line_rows_96            64 cabs x 96 requests, 32 constant rows: accepted with verdict 3 (LP_UNBAL, line_dummies 32)
  line_cols_96            96 cabs x 64 requests, constant trailing columns: verdict 2, accepted on the transpose (LP_TRANSPOSE)
  line_refused_64         line_64 with one cell beside the sorted matching made free: plausible to the probe, refused by the certificate
                          (LP_BALANCED without LP_ACCEPTED), the skipped compress pass is run and the general path solves it
  build_192x64            td_build_assign, threshold 10, fill 250 000: hinted fused pass, 4-byte cells, no matrix
  build_2304x1200         ... n > 2048: hinted fused pass with 1-byte cells + escape
  build_96x96             td_build_assign without dummy requests: no fuse, the matrix is built and solved as any other
  tick_192x64_nolcm       td_tick without an LCM (stop size < 0): the whole model goes through the hint with `tick` set
  tick_192x64_stop0       td_tick with stop size 0: the LCM runs until only fill cells are left, so like Simulator.java:188
                          the tick has no input for the solver (solved false): the branch of td_tick that skips the solve
  matrix_2304x1200        the same model as a matrix: the line probe's shape estimate starts the speculative fused pass
  matrix_2304x1200_neg    ... with one negative real cell: the speculative pass is refused by the final read-back, the call
                          restarts on the general path (early check of the 1-byte attempt, then the explicit transpose)
  u8_256, u16_256         uniform 0..100 / 0..40 000: the speculative 1-byte solve / 2-byte cells
  np_256, u32_256         uniform 0..10^6 / 0..2^30: 4-byte cells with 32-bit / 64-bit prices (range above NP_RANGE)
  plimit/np_256           TD_NP_PLIMIT=2000: a price reaches the 32-bit limit, the attempt is redone with 64-bit prices
  transpose_256           64 constant trailing columns of 77 (no fill value): the line probe's estimate starts the fused
                          pass, checked (not speculative)
  transpose_256_neg       ... with a negative cell the fused pass refuses: the skipped 1-byte pass is rerun, its early
                          check reads the shape probe's flag and the explicit transpose follows
  transpose_256_lineoff   ... with the line attempt off: the shape probe's flag comes with the final read-back of the
                          1-byte attempt, then the explicit transpose
  warm_512                uniform 0..40 000 at n = 512 = TD_WARM_MIN_N, the smallest size of test_gpu_widths.py's warm-start
                          ladder: wide, tie-free 2-byte rows, warm_rounds > 0
  eps/u8_128              TD_SOLVER=eps, the comparison mode
  erange_1024             a row spanning 2^32 - 2 at n = 1024: (range + 1) (n + 1) >= 4e12, TD_ERANGE as a return code
  handles                 two td.Solver() handles used alternately on build_192x64's model and u8_256's matrix
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "assign_paths_parent.json")
TD_ERANGE = -4


@pytest.fixture(scope="module")
def solved():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "assign_paths_golden.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


def records(tree):
    for sec, cases in sorted(tree.items()):
        for name, outs in sorted(cases.items()):
            for o, rec in sorted(outs.items()):
                yield (sec, name, o), rec


@pytest.mark.gpu
def test_every_case_was_solved(td, solved, want):
    assert sorted(solved) == sorted(want) == ["default", "eps", "plimit"]
    assert [k for k, _ in records(solved)] == [k for k, _ in records(want)]
    assert len(want["default"]) == 23 and list(want["plimit"]) == ["np_256"] and list(want["eps"]) == ["u8_128"]
    for (sec, name, o), rec in records(want):
        assert rec["rc"] == (TD_ERANGE if name == "erange_1024" else 0), (sec, name, o)


@pytest.mark.gpu
def test_row_to_col_is_a_permutation_that_costs_the_total(td, solved):
    for key, got in records(solved):
        if got["rc"] != 0 or "is_permutation" not in got:
            continue
        assert got["is_permutation"], key
        assert got["cost_of_r2c"] == got["total"] == got["dual"], (key, got)
        assert got.get("oracle_total_equal", True), key


@pytest.mark.gpu
def test_handles_equal_the_default_handle(td, solved):
    for key, got in solved["default"]["handles"].items():
        assert got["equals_default_handle"], key


@pytest.mark.gpu
def test_the_cases_take_their_branches(td, want):
    """what the docstring claims about the recorded (parent) statistics"""
    d = {k: dict(rec["stats"], **{x: rec.get(x) for x in ("solved",)}) for k, rec in records(want)}
    LP_BALANCED, LP_TRANSPOSE, LP_UNBAL, LP_ACCEPTED = 2, 4, 8, 1024
    for o in ("dev", "host"):
        assert d["default", "line_64", o]["line_path"] & (LP_BALANCED | LP_ACCEPTED) == LP_BALANCED | LP_ACCEPTED
        assert d["default", "line_rows_96", o]["line_path"] & (LP_UNBAL | LP_ACCEPTED) == LP_UNBAL | LP_ACCEPTED
        assert d["default", "line_rows_96", o]["line_dummies"] == 32
        assert d["default", "line_cols_96", o]["line_path"] & (LP_TRANSPOSE | LP_ACCEPTED) == LP_TRANSPOSE | LP_ACCEPTED
        assert d["default", "line_refused_64", o]["line_path"] & (LP_BALANCED | LP_ACCEPTED) == LP_BALANCED
        assert (d["default", "build_192x64", o]["bytes_per_cell"], d["default", "build_192x64", o]["transposed"]) == (4, 1)
        assert (d["default", "build_2304x1200", o]["bytes_per_cell"], d["default", "build_2304x1200", o]["transposed"]) == (1, 1)
        assert d["default", "build_96x96", o]["transposed"] == 0
        assert (d["default", "matrix_2304x1200", o]["bytes_per_cell"], d["default", "matrix_2304x1200", o]["transposed"]) == (1, 1)
        assert d["default", "matrix_2304x1200_neg", o]["transposed"] == 1
        assert d["default", "u8_256", o]["bytes_per_cell"] == 1 and d["default", "u16_256", o]["bytes_per_cell"] == 2
        assert (d["default", "np_256", o]["bytes_per_cell"], d["default", "np_256", o]["narrow_price"]) == (4, 1)
        assert (d["default", "u32_256", o]["bytes_per_cell"], d["default", "u32_256", o]["narrow_price"]) == (4, 0)
        assert (d["plimit", "np_256", o]["bytes_per_cell"], d["plimit", "np_256", o]["narrow_price"]) == (4, 0)
        for name in ("transpose_256", "transpose_256_neg", "transpose_256_lineoff"):
            assert d["default", name, o]["transposed"] == 1, name
        assert d["default", "warm_512", o]["warm_rounds"] > 0 and d["default", "warm_512", o]["bytes_per_cell"] == 2
    assert d["default", "tick_192x64_nolcm", "host"]["solved"] and d["default", "tick_192x64_nolcm", "host"]["transposed"] == 1
    assert not d["default", "tick_192x64_stop0", "host"]["solved"]


@pytest.mark.gpu
def test_results_equal_the_parent_commit(td, solved, want):
    for (sec, name, o), w in records(want):
        got = solved[sec][name][o]
        print(sec, name, o, got["rc"], got["total"], got["sha1"], w["sha1"])
        assert got == w, (sec, name, o)
