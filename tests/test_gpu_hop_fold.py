"""td_assign's two-hop passes with the tight sets of the assigned rows tested inside k_hop_table, for the rows a free row
reaches (csrc/td_blocks.h), against the results recorded when a kernel of its own, k_hop_esc, made a mask for every
assigned row.

tools/hop_fold_golden.py solves seeded instances made on the device, each with a device and with a host row_to_col, in
child processes; tests/golden/hop_fold_parent.json is its output at the parent commit (two runs there gave the same
file).  Everything must be equal: total, dual bound, the sha1 of row_to_col and last_stats().  Every section forces 8
diagonal blocks (td_set_blocks(8), TD_BLOCKS_MIN_N=0).

The sizes.  The shapes first meant for this file were n = 1024, 2048 and 4224.  At the parent commit td_assign does not start
block-locally at any of them, whatever TD_BLOCKS_MIN_N says: the compress pass that prepares the start needs n / 4 >= 3072
(sv_compress_t, "bid0"), and TD_DEBUG prints no phase A line for n = 1024, 2048, 4224, 8192 or 12 160
(profiles/hop_fold/coverage_parent_debug.txt, the probe at its end).  n = 12 288 is the smallest multiple of 128 at which a
two-hop kernel runs at all, so each case moved to the next multiple of 128 that gives what it was chosen for:
  n = 12 288  rpb = 1536, the smallest block of the block-local start; 3 segments a row in the pass over the whole matrix
  n = 12 416  rpb = 1552, no multiple of 256; n / 4 = 3104, so the table of the pass over the
              whole matrix has 4 segments and the last one holds 32 quads (the "nearly empty last segment" 4224 was for)

Which case covers what (free rows / columns per block as TD_DEBUG printed them at the parent commit):
  default/0_perfjl_12416   U{10..40}; first in-block pass 19..23 free rows per block (between 1 and 63), second 0 or 1;
                 1 row left, the gated pass over the whole matrix runs and places it
  default/1_perfjl_12288, 2_perfjl_12416   17..23 and 15..24 free rows per block, 3 rows left each, all placed by the
                 gated pass.  With case 0 this is the sequence 12 416, 12 288, 12 416 on one handle: the tables and lists
                 of one n are what the solve of the next n finds
  default/3_sparse1_12288  one zero cell per row outside the blocks: 1332..1359 free rows per block (above
                 TD_HOP_MAX_ROWS, every kernel leaves the blocks alone), 10 752 rows left: the gate stays shut
  default/4_sparse0_12416  518..521 free rows per block, 4158 left: the gate stays shut; the rounds and the finisher run
                 behind three solves that used the SPLIT table
  maxrows/0_perfjl_12416   TD_ZS_ROUNDS=0, TD_HOP_MAX_ROWS lifted: 561..592 free rows and columns per block in the first
                 in-block pass, 434..465 in the second (>= HOP_FMAX = 128: the "first 128" cut of both lists, full
                 tables); 2562 rows left, the pass over the whole matrix places 128 of them
  shards/0_perfjl_12288    td_assign, then the same matrix through the shard API in this process, one block per shard (the
                 kernels see nb = 1 and row0 > 0).  The blocks leave 3 rows, so the sharded sequence goes on with its own
                 rounds and need not end in td_assign's row_to_col; it is compared with its own record, and with td_assign
                 where the blocks leave nothing, as tests/test_gpu_sharded.py does.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hop_fold_parent.json")


@pytest.fixture(scope="module")
def solved():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hop_fold_golden.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
def test_every_case_was_solved(td, solved, want):
    assert sorted(solved) == sorted(want) == ["default", "maxrows", "shards"]
    for sec in want:
        assert sorted(solved[sec]) == sorted(want[sec]), sec
    assert len(want["default"]) == 10 and len(want["maxrows"]) == 2 and len(want["shards"]) == 3


@pytest.mark.gpu
def test_row_to_col_is_a_permutation_that_costs_the_total(td, solved):
    for sec, cases in solved.items():
        for name, got in cases.items():
            assert got["is_permutation"], (sec, name)
            assert got["cost_of_r2c"] == got["total"] == got["dual"], (sec, name, got)


@pytest.mark.gpu
def test_results_equal_the_parent_commit(td, solved, want):
    for sec, cases in want.items():
        for name, w in cases.items():
            got = solved[sec][name]
            print(sec, name, got["total"], got["sha1"], w["sha1"])
            assert got == w, (sec, name)


@pytest.mark.gpu
def test_shard_api_agrees_with_td_assign(td, solved):
    api, dev, host = (solved["shards"]["0_perfjl_12288_" + k] for k in ("api", "dev", "host"))
    assert dict(map(tuple, api["stats"]))["path"] == "blocks"
    assert api["total"] == api["dual"] == dev["total"] == host["total"]
    assert dev["sha1"] == host["sha1"]
    if dict(map(tuple, api["stats"]))["left"] == 0:   # both sequences coincide when the blocks leave nothing
        assert api["sha1"] == dev["sha1"]
