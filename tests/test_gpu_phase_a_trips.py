"""The chain of short kernels behind td_assign's compress pass (phase A of the block-local start, the two-hop passes,
k_place_const, k_final: csrc/td_blocks.h) with the flag, gate and count loads of every kernel issued together with its
first data loads and k_zs_bid taking one row per wave, against the results recorded at the commit before.

tools/phase_a_trips_golden.py solves seeded instances made on the device, each with a device and with a host row_to_col, in
child processes that run with TD_DEBUG=1; tests/golden/phase_a_trips_parent.json is its output at the parent commit (two
runs there gave the same file).  Everything must be equal: total, dual bound, the sha1 of row_to_col, last_stats() and the
HopCtl words of TD_DEBUG's phase A line (free rows / columns per block in front of the last in-block two-hop pass,
matched, left).  Every section forces 8 diagonal blocks (td_set_blocks(8), TD_BLOCKS_MIN_N=0).

The sizes are the smallest at which these kernels run at all (tests/test_gpu_hop_fold.py: no block-local start below
n = 12 288):
  n = 12 288  rpb = 1536, 96 chunks per column slice: in k_zs_bid half of a wave's lanes have one chunk and half have two
  n = 12 416  rpb = 1552, 97 chunks: the ragged tail (one lane has a second chunk, 63 read the clamped last chunk again)
  n = 16 384  rpb = 2048, exactly two chunks per lane (the benchmark's size), once

Which case reaches which branch (profiles/phase_a_trips/coverage_parent_debug.txt, the parent's TD_DEBUG output):
  passes1/*      TD_HOP_PASSES=1: the only in-block pass finds 16..29 free rows and columns per block; 2, 2 and 5 rows
                 left, the gated pass over the whole matrix places them.  All three `passes` sections solve
                 n = 12 416, 12 288, 12 416 on one handle: lists and tables of another n are what the next solve finds
  passes2/*      the default: the second in-block pass finds 0 or 1 free row per block (k_hop_table: 1016+ of its 1024
                 workgroups leave on the counts; k_hop_match: nfr == 0 in most blocks); 2, 1 and 4 rows left
  passes3/*      a third in-block pass over blocks with 0 or 1 free row that matches nothing
  rounds0/*, rounds1/*   TD_ZS_ROUNDS=0 / 1 at the default TD_HOP_MAX_ROWS: 544..594 and 187..221 free rows per block, more
                 than TD_HOP_MAX_ROWS (k_hop_table leaves, k_hop_match adds the block's count to `left`), 4536 / 1674 rows
                 left, the gate stays shut, the rounds and the finisher run.  rounds0 runs no k_zs_bid at all, rounds1 one
  rounds2/*      two rounds: 0..2 free rows per block in the second pass (the one block with 2 is the nearest any setting
                 came to "2 - 10 rows in the second pass"; no setting gave a block 30 - 127 rows in its SECOND pass at the
                 default TD_HOP_MAX_ROWS: the nearest are passes1's 16 - 29 in the first and maxrows' 441 - 463)
  maxrows/*      TD_ZS_ROUNDS=0 with TD_HOP_MAX_ROWS lifted: 441..463 free rows and columns per block in the second pass
                 (both lists cut at HOP_FMAX = 128 in both passes, full tables: k_hop_match's staging loop behind its
                 hoisted loads), 2603 rows left, the pass over the whole matrix places 128 of them
  const64/*      64 constant rows (r2c = -2, deferred): 7..9 more free columns than free rows per block in k_hop_lists'
                 two lists, and k_place_const has work behind its hoisted flag / gate / count loads
  wide/*         one cell of 10^6: the compress pass raises the width flag, every chain kernel runs its hoisted loads with
                 the flag set and leaves without a store (HopCtl all 0 as the solve before left it cleared); the result is
                 the parent's after the wider attempt
  sparse/*       sparse1: 1332..1359 free rows per block, 10 752 left; sparse0: 518..521, 4158 left: gate shut, rounds and
                 finisher
  shards/*       td_assign, then the same matrix through the shard API, one block per shard (nb = 1, row0 > 0), compared
                 with its own record
  n16384/*       the benchmark's shape
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "phase_a_trips_parent.json")
SECTIONS = ["const64", "maxrows", "n16384", "passes1", "passes2", "passes3", "rounds0", "rounds1", "rounds2", "shards", "sparse", "wide"]


@pytest.fixture(scope="module")
def solved():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "phase_a_trips_golden.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
def test_every_case_was_solved(td, solved, want):
    assert sorted(solved) == sorted(want) == SECTIONS
    for sec in want:
        assert sorted(solved[sec]) == sorted(want[sec]), sec
    assert sum(len(v) for v in want.values()) == 2 * (3 * 3 + 3 * 2 + 1 + 1 + 1 + 2 + 1 + 1) + 1   # dev + host, and the shard API
    for sec, cases in want.items():   # the golden file itself holds the HopCtl words of every td_assign solve
        for name, w in cases.items():
            assert len(w["phase_a"]) == (8 if name.endswith("_api") else 1), (sec, name)


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
            print(sec, name, got["total"], got["sha1"], w["sha1"], got["phase_a"][-1]["matched"], got["phase_a"][-1]["left"])
            assert got == w, (sec, name)


@pytest.mark.gpu
def test_shard_api_agrees_with_td_assign(td, solved):
    api, dev, host = (solved["shards"]["0_perfjl_12288_" + k] for k in ("api", "dev", "host"))
    assert dict(map(tuple, api["stats"]))["path"] == "blocks"
    assert api["total"] == api["dual"] == dev["total"] == host["total"]
    assert dev["sha1"] == host["sha1"]
    if dict(map(tuple, api["stats"]))["left"] == 0:   # both sequences coincide when the blocks leave nothing
        assert api["sha1"] == dev["sha1"]
