"""td_assign's block-local start and two-hop chain against the results recorded before the chain was trimmed
(k_hop_match as a one-wave walk, k_hop_table of the pass over the whole matrix split by segment; profiles/hop_chain).

tools/hop_chain_golden.py solves seeded instances made on the device, each with a device and with a host row_to_col, in
child processes; tests/golden/hop_chain_parent.json is its output at the parent commit (two runs there gave the same
file).  Everything must be equal: total, dual bound, the sha1 of row_to_col and last_stats().  The script also records
that row_to_col is a permutation and what it costs in the matrix.

Which case covers what (free rows per block as TD_DEBUG printed them at the parent commit):
  perfjl_12288   U{10..40}, the smallest n of the block-local path, a slice of 384 quads straddles two 512-quad pieces of
                 the compress pass; 17..20 free rows per block in the first in-block pass, 1 in the second (blocks with
                 between 1 and 63 free rows), 2 rows left for the pass over the whole matrix, which places both: a row
                 has about n / 31 zero cells, so every one of its 3 segments holds candidates
  perfjl_16384   the benchmark's shape; 21..25 free rows per block, then 1, then 3 rows over 4 segments
  perfjl_32768   the 1024 x 16 compress shape; 29..37 free rows per block
  sparse0_16384  zero cells mostly outside the diagonal blocks; about 1000 free rows per block: above TD_HOP_MAX_ROWS, every
                 two-hop kernel leaves the blocks alone, 7980 rows go to the rounds and the finisher
  sparse1_12288  more rows left (10752) than TD_HOP_MAX_ROWS: the gate stays shut
  constrows      constant rows: nothing is free after the rounds, the two-hop kernels see empty lists
  maxrows/*      TD_ZS_ROUNDS=0 and TD_HOP_MAX_ROWS lifted: no local round after round 0, no limit on the free rows of a
                 block.  This is where a block's first in-block pass sees at least HOP_FMAX = 128 free rows:
  maxrows/perfjl_16384  744..773 free rows and columns per block in the first in-block pass, 616..645 in the second; each
                 pass walks the first 128 rows against the first 128 columns with full tables (1020 of 8 x 128 rows matched
                 in either pass); 4039 rows left, the pass over the whole matrix (4 segments a row) places 128 of them,
                 the rounds and the finisher take the rest
  maxrows/perfjl_12288  539..584, then 411..457 free rows per block; 2445 rows left, 128 placed over 3 segments a row
  maxrows/sparse0_16384  about 1000 free rows per block and nearly empty tables: 128-row walks that match nothing
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hop_chain_parent.json")


@pytest.fixture(scope="module")
def solved():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hop_chain_golden.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_every_case_was_solved(td, solved):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(solved) == sorted(want) == ["default", "maxrows"]
    for sec in want:
        assert sorted(solved[sec]) == sorted(want[sec]), sec
    assert len(want["default"]) == 12 and len(want["maxrows"]) == 6


@pytest.mark.gpu
def test_row_to_col_is_a_permutation_that_costs_the_total(td, solved):
    for sec, cases in solved.items():
        for name, got in cases.items():
            assert got["is_permutation"], (sec, name)
            assert got["cost_of_r2c"] == got["total"] == got["dual"], (sec, name, got)


@pytest.mark.gpu
def test_results_equal_the_parent_commit(td, solved):
    with open(GOLDEN) as f:
        want = json.load(f)
    for sec, cases in want.items():
        for name, w in cases.items():
            got = solved[sec][name]
            print(sec, name, got["total"], got["sha1"], w["sha1"])
            assert got == w, (sec, name)
