"""td_assign's finishers at their selection, chunk and LDS edges (sv_finish_t, csrc/td_assign.hip).

tools/finisher_paths.py solves every case of tests/finisher_cases.py once, one child process per environment (section); the
module fixture runs it and every test reads its output.  Per case:
  * rc == 0 and row_to_col is a permutation (the model is square: a finisher that drops or misreads a column of a partial chunk
    or slice cannot return one);
  * what row_to_col costs in the matrix (int64, on the host) == total == dual == the reference: the closed form
    sum |sort a - sort b|, or the monotone-matching dynamic program + k BIG; no reference comes from the GPU (a finisher that
    mis-relaxes returns a dearer total than the exact optimum);
  * sap_free_rows > 0: an instance that stops reaching the finisher is a failure, not a skip;
  * finisher_path (td_last_stats word 13) has exactly the flags, the CH and the speculative batch count of the host model
    finisher_cases.expected(), evaluated with the free-row counts the statistics report where a rule reads them back (the
    speculative gate, k_sapx's rows rule, FP_FOREST_NONE), and those are the flags the table names for the row (a finisher the
    selection silently stopped choosing shows in the word);
  * FP_FOREST_REFUSED and FP_SAPX_REFUSED are never set.

Which case reaches which kernel instantiation is the `kernel` / `spec_kernel` of the host model; the table's `emulates` marks the
rows that run the fallback of a refused cooperative launch, emulated by TD_FOREST=0 / TD_SAPX=0.

Wall time of each section's child on the MI355X (library and torch start-up included, about 2 s of each), measured with the
library of this commit's parent plus the statistics word; the children's timeouts in finisher_cases.SECTIONS are ten times
these and at least 120 s:
    default 3.3 s, psap8_off 2.1 s, sap8_off 2.1 s, sap8_sap512_off 2.1 s, psap_off 2.0 s, psap_cap1 2.0 s, forest_off 2.6 s,
    forest_sap512_off 2.2 s, forest_off_sapx_rows 2.1 s, serial 4.7 s, serial_large 6.2 s, sapx_min1 2.3 s, forest_min64 2.0 s
    (36 s for the whole script)
The slowest single calls: serial_n19204 2.5 s, serial_n16388 1.7 s (both on the near-diagonal family LN: on the plain |a - b|
family the single workgroup took 15.7 s and 6.1 s for 5215 and 4106 free rows), serial_n8192 0.74 s, forest_n16388 0.61 s.

Out of scope here:
  * KX = 64 and 65 and n = 32768 and 32769 for k_sapx and k_forest: 4 GiB matrices, and the single-workgroup fallback takes
    many seconds there;
  * PS_CAP overruns (a speculative search longer than its record);
  * sharded tables (tab.count > 1);
  * a cooperative launch that is really refused (the off switches emulate it);
  * k_sap8<false, ...>: unreachable (k_sap8 needs CH = 1, so npad <= 16384 and 128 KiB of state, within the 150 KiB rule);
  * the CH = 16 instance of k_sap (n > 32768 in 4-byte cells) and k_sap<.., 4, .., 512> (ch5 == CH == 4 needs nchunks in
    (2048, 4096] for ch5 and (4096, ..] for CH: never equal above CH = 1, so only k_sap<.., 1, .., 512> is reachable)."""
import json
import os
import subprocess
import sys

import pytest

import finisher_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solved():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "finisher_paths.py")], capture_output=True, text=True,
                       timeout=sum(t for _, t in fc.SECTIONS.values()) + 60)
    lines = r.stdout.strip().splitlines()
    out = json.loads(lines[-1]) if lines else {}
    for sec, d in out.items():
        print("section %s: status %s, %.1f s" % (sec, d["status"], d["wall_s"]))
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_every_section_ended_normally_and_solved_its_cases(solved):
    assert list(solved) == list(fc.SECTIONS)
    for sec, d in solved.items():
        assert d["status"] == 0, sec
        assert list(d["cases"]) == [c["name"] for c in fc.cases_of(sec)], sec


def test_no_cooperative_launch_was_refused(solved):
    for sec, d in solved.items():
        for name, got in d["cases"].items():
            assert not got["finisher_path"] & (fc.FP_FOREST_REFUSED | fc.FP_SAPX_REFUSED), (sec, name)


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_case(solved, name):
    c = fc.CASES[name]
    inst, env = c["inst"], fc.SECTIONS[c["section"]][0]
    got = solved[c["section"]]["cases"][name]
    st, word = got["stats"], got["finisher_path"]
    want = fc.reference(name)
    print(name, "rc", got["rc"], "total", got["total"], "dual", got["dual"], "cost", got.get("cost_of_r2c"), "reference", want,
          "finisher_path", hex(word), fc.flag_names(word), "free", st["sap_free_rows"], "speculative rows", st["parallel_sap_rows"],
          "call ms", got["call_ms"])
    assert got["rc"] == 0
    assert got["is_permutation"]
    assert got["cost_of_r2c"] == got["total"] == got["dual"] == want
    assert st["line_metric"] == 0 and st["transposed"] == 0
    assert (st["bytes_per_cell"], st["narrow_price"]) == (fc.TYPES[c["kind"]]["bytes"], fc.TYPES[c["kind"]]["narrow"])
    assert st["sap_free_rows"] > 0, "the instance no longer reaches the finisher"
    e = fc.expected(c["kind"], inst["n"], env, st["sap_free_rows"], st["parallel_sap_rows"])
    assert word & fc.FP_FLAGS == e["flags"], (fc.flag_names(word), fc.flag_names(e["flags"]))
    assert e["flags"] == c["flags"], "the free-row counts moved the case off the finisher its row names"
    assert (word & fc.FP_CH_MASK) >> fc.FP_CH_SHIFT == e["ch"]
    batches = word >> fc.FP_BATCH_SHIFT
    if e["batches_exact"] is not None:
        assert batches == e["batches_exact"]
    else:
        assert batches >= e["batches_min"]
    if e["flags"] & fc.FP_PSAP:
        assert st["parallel_sap_rows"] > 0
    if not e["flags"] & (fc.FP_PSAP | fc.FP_SAP8_BATCH):
        assert st["parallel_sap_rows"] == 0 and batches == 0
    assert (st["forest_levels"] > 0) == bool(e["flags"] & fc.FP_FOREST)
