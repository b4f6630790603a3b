"""CPU tier of the finisher boundary suite: the table of tests/finisher_cases.py stands on what it claims.

The references (closed form, monotone-matching dynamic program) equal the CPU oracle on small instances of every cell width;
every row's instance has the row range of the cell type it names; every edge the suite is about is in the table from the sides
claimed, and the host model's CH, T, KX, LDS and forest geometry differ across each pair exactly as stated; the host model gives
every row the finisher it names when fed the free-row counts recorded for it; the FP_* bits are the header's."""
import os
import re

import numpy as np
import pytest

import finisher_cases as fc
from finisher_cases import CASES, L, LN, LP, U, expected, forest_geometry, geometry
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = {"u8": 255, "u16": 60000, "u32n": 150000, "u32": 5 * 10**7}


def env_of(name):
    return fc.SECTIONS[CASES[name]["section"]][0]


def geo(name):
    return geometry(CASES[name]["kind"], CASES[name]["inst"]["n"])


# ---- the references
@pytest.mark.parametrize("kind", list(WIDTHS))
def test_closed_form_and_dp_equal_the_oracle(kind):
    S = WIDTHS[kind]
    for inst in (L(90, S, 1), L(131, S, 2), LN(120, 30, S, 3), LP(100, 7, S, 4), LP(65, 1, S, 5), LP(140, 40, S, 6)):
        c = fc.numpy_matrix(inst)
        assert fc.reference_total(inst) == int(oracle.assign(c)[0]), inst
        lo, hi = fc.row_ranges(inst)
        r = c.astype(np.int64).max(axis=1) - c.astype(np.int64).min(axis=1)
        assert (lo, hi) == (int(r.min()), int(r.max())), inst
        assert fc.kind_of_range(hi) == kind, inst


def test_dp_at_the_sizes_the_issue_checked():
    for n, k, S in ((200, 17, 254), (300, 60, 30000), (257, 1, 10**6)):
        inst = LP(n, k, S, n + k)
        assert fc.reference_total(inst) == int(oracle.assign(fc.numpy_matrix(inst))[0])


def test_uniform_family_is_the_oracles():
    inst = U(64, 100, 9)
    c = fc.numpy_matrix(inst)
    assert c.shape == (64, 64) and 0 <= c.min() and c.max() <= 100
    assert fc.reference_total(inst) == int(oracle.assign(c)[0])
    with pytest.raises(AssertionError):
        U(fc.ORACLE_NMAX + 1, 100, 9)


def test_cost_of_agrees_with_the_matrix():
    for inst in (L(50, 255, 1), LP(60, 9, 150000, 2)):
        c = fc.numpy_matrix(inst)
        r2c = np.random.default_rng(3).permutation(inst["n"])
        assert fc.cost_of(inst, r2c) == fc.cost_of(inst, r2c, c) == int(c[np.arange(inst["n"]), r2c].astype(np.int64).sum())


# ---- every row
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_row_has_the_range_of_its_cell_type(name):
    c = CASES[name]
    lo, hi = fc.row_ranges(c["inst"])
    assert fc.kind_of_range(hi) == c["kind"], (lo, hi)
    if c["inst"]["family"] == "LP":
        assert lo == 0 and c["inst"]["k"] > 0       # the constant rows
    assert (c["inst"]["n"] >= fc.DEVICE_MIN) == fc.on_device(c["inst"])
    if fc.on_device(c["inst"]):
        a, b = fc.positions(c["inst"])
        assert c["inst"]["k"] == 0 and max(int(a.max()), int(b.max())) < 2**31     # td.cost_build takes int32 positions


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_model_gives_the_row_its_finisher(name):
    c = CASES[name]
    entry, serial = c["free"]
    assert entry >= serial > 0, "a case must leave rows to the last finisher"
    e = expected(c["kind"], c["inst"]["n"], env_of(name), serial, entry - serial)
    assert e["flags"] == c["flags"], (fc.flag_names(e["flags"]), fc.flag_names(c["flags"]))
    assert not e["flags"] & (fc.FP_FOREST_REFUSED | fc.FP_SAPX_REFUSED | fc.FP_FOREST_NONE)


def test_sections_and_environments():
    assert all(fc.cases_of(s) for s in fc.SECTIONS)
    for env, timeout in fc.SECTIONS.values():
        assert set(env) <= set(fc.DEFAULTS) and timeout >= 120
        t = fc.tunables(env)
        # every knob only lowers a threshold or switches a finisher off
        for k in ("TD_FOREST", "TD_SAPX", "TD_SAP512", "TD_SAP8", "TD_PSAP", "TD_PSAP8", "TD_PSAP_CAP", "TD_FOREST_MIN_N", "TD_SAPX_MIN",
                  "TD_WIDE_U16_N", "TD_U16_REDO_FREE"):
            assert t[k] <= fc.DEFAULTS[k], (k, env)
    assert fc.tunables({"TD_FOREST_MIN_N": "1"})["TD_FOREST_MIN_N"] == 64
    assert fc.tunables({"TD_PSAP": "1000"})["TD_PSAP"] == 64


def test_bits_are_the_headers():
    text = open(os.path.join(ROOT, "include", "taxidispatcher_amd.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define TD_FP_(\w+) (\w+)", text)}
    for name, bit in (("FOREST", fc.FP_FOREST), ("FOREST_NONE", fc.FP_FOREST_NONE), ("FOREST_REFUSED", fc.FP_FOREST_REFUSED), ("PSAP", fc.FP_PSAP),
                      ("SAPX", fc.FP_SAPX), ("SAPX_REFUSED", fc.FP_SAPX_REFUSED), ("SAP8_BATCH", fc.FP_SAP8_BATCH), ("SAP8", fc.FP_SAP8),
                      ("SAP512", fc.FP_SAP512), ("SAP", fc.FP_SAP), ("NOLDS", fc.FP_NOLDS), ("CH_SHIFT", fc.FP_CH_SHIFT), ("CH_MASK", fc.FP_CH_MASK),
                      ("BATCH_SHIFT", fc.FP_BATCH_SHIFT)):
        assert defs[name] == bit, name
    flags = [b for b in fc.FP_NAMES]
    assert sum(flags) == fc.FP_FLAGS and len(set(flags)) == 11      # disjoint, and clear of the CH field


# ---- the edges, from the sides the table claims
def test_edges_k_sap8():
    a, b = geo("sap8_n1024"), geo("sap8_n1025")
    assert (a["nchunks"], a["T"], a["last_chunk_cols"]) == (64, 64, 16) and (b["nchunks"], b["T"], b["last_chunk_cols"]) == (65, 128, 1)
    assert CASES["sap8_n63"]["flags"] == fc.FP_SAP8 and CASES["sap8_n64"]["flags"] == fc.FP_SAP8 | fc.FP_SAP8_BATCH
    assert CASES["sap8_n63"]["inst"]["n"] + 1 == CASES["sap8_n64"]["inst"]["n"] == 64
    assert CASES["sap8_psap8_off_n1024"]["flags"] == fc.FP_SAP8 and env_of("sap8_psap8_off_n1024") == {"TD_PSAP8": "0"}
    assert CASES["sap8_lp_n200_k17"]["inst"]["k"] == 17 and CASES["sap8_lp_n200_k17"]["kind"] == "u8"
    assert CASES["sap8_off_n1024"]["flags"] == fc.FP_SAP512 and CASES["sap8_sap512_off_n1024"]["flags"] == fc.FP_SAP
    for name in ("sap8_off_n1024", "sap8_sap512_off_n1024"):      # IsLean8 is the type's: no generic speculative batches for 1-byte cells
        assert expected("u8", 1024, env_of(name), 252, 0)["batches_min"] == 0
    assert all(CASES[n]["inst"] == CASES["sap8_n1024"]["inst"] for n in ("sap8_psap8_off_n1024", "sap8_off_n1024", "sap8_sap512_off_n1024"))


def test_edges_speculative_batches():
    for name in ("psap_n1500", "psap_u16_n1500", "psap_cap1_n1500"):
        assert CASES[name]["flags"] & fc.FP_PSAP
    assert not CASES["psap_off_n1500"]["flags"] & fc.FP_PSAP and CASES["psap_u16_n1500"]["kind"] == "u16"
    entry, serial = CASES["psap_cap1_n1500"]["free"]
    one = expected("u32n", 1500, env_of("psap_cap1_n1500"), serial, entry - serial)
    dflt = expected("u32n", 1500, {}, serial, entry - serial)
    assert one["batches_exact"] == one["batches_min"] == 14 == (entry + 31) // 32 and dflt["batches_exact"] is None and dflt["batches_min"] == 14
    # below psap_min (32 for n < 2048, 12 from there on) no group goes out
    assert not expected("u32n", 1500, {}, 31, 0)["flags"] & fc.FP_PSAP and expected("u32n", 1500, {}, 32, 0)["flags"] & fc.FP_PSAP
    assert not expected("u32n", 2048, {"TD_FOREST": "0"}, 11, 0)["flags"] & fc.FP_PSAP
    assert expected("u32n", 2048, {"TD_FOREST": "0"}, 12, 0)["flags"] & fc.FP_PSAP
    a, b = geo("serial_n6144"), geo("serial_n6148")
    assert a["shm"] == a["cshm"] == fc.DYN_LDS_OPT_IN and not a["shm_opt_in"] and not a["cshm_opt_in"]
    assert b["shm"] == b["cshm"] == 49184 and b["shm_opt_in"] and b["cshm_opt_in"]
    assert env_of("serial_n6144")["TD_FOREST"] == env_of("serial_n6144")["TD_SAPX"] == "0"


def test_edges_sap512():
    a, b = geo("sap512_n2048"), geo("sap512_n2052")
    assert (a["nchunks"], a["CH"], a["ch5"], a["T5"]) == (512, 1, 1, 512) and CASES["sap512_n2048"]["flags"] == fc.FP_PSAP | fc.FP_SAP512
    assert (b["nchunks"], b["CH"], b["ch5"], b["T"]) == (513, 1, 2, 576) and CASES["sap512_n2052"]["flags"] == fc.FP_PSAP | fc.FP_SAP
    assert CASES["sap512_off_n2048"]["flags"] == fc.FP_PSAP | fc.FP_SAP and geo("sap512_off_n2048")["T"] == 512
    assert env_of("sap512_off_n2048") == {"TD_FOREST": "0", "TD_SAP512": "0"}


def test_edges_ch_steps():
    want = {"serial_n4096": (1024, 1, 1024), "serial_n4100": (1025, 2, 576), "serial_n8192": (2048, 2, 1024), "serial_n8196": (2049, 4, 576),
            "serial_u16_n8192": (1024, 1, 1024), "serial_u16_n8200": (1025, 2, 576), "serial_n16388": (4097, 8, 576), "serial_n19204": (4801, 8, 640)}
    for name, (nchunks, CH, T) in want.items():
        g = geo(name)
        assert (g["nchunks"], g["CH"], g["T"]) == (nchunks, CH, T), name
        assert CASES[name]["flags"] & fc.FP_SAP and CASES[name]["emulates"], name
        assert env_of(name)["TD_FOREST"] == env_of(name)["TD_SAPX"] == "0"
    for name in ("serial_u16_n8192", "serial_u16_n8200"):
        assert CASES[name]["kind"] == "u16" and env_of(name)["TD_WIDE_U16_N"] == env_of(name)["TD_U16_REDO_FREE"] == "0"
    # CH = 8: no speculative batches whatever is free; the LDS rule flips between npad 19200 and 19204
    assert not CASES["serial_n16388"]["flags"] & fc.FP_PSAP and expected("u32n", 16388, env_of("serial_n16388"), 5000, 0)["batches_min"] == 0
    assert geo("serial_n16388")["lds"] and not geo("serial_n19204")["lds"] and geo("serial_n19204")["npad"] == 19204
    assert geometry("u32n", 19200)["lds"] and geometry("u32n", 19200)["st"] == fc.LDS_STATE_MAX
    assert CASES["serial_n19204"]["flags"] == fc.FP_SAP | fc.FP_NOLDS and CASES["serial_n16388"]["flags"] == fc.FP_SAP


def test_k_sap8_without_lds_state_is_unreachable():
    """k_sap8 needs CH = 1: nchunks <= 1024, npad <= 16384, 131072 bytes of state: always within the 150 KiB rule"""
    g = geometry("u8", 16384)
    assert g["CH"] == 1 and g["npad"] == 16384 and g["st"] == 131072 <= fc.LDS_STATE_MAX
    assert geometry("u8", 16385)["CH"] == 2


def test_edges_k_sapx():
    g = geo("sapx_n8192")
    assert g["KX"] == 16 and CASES["sapx_n8192"]["flags"] == fc.FP_PSAP | fc.FP_SAPX and env_of("sapx_n8192") == {"TD_FOREST": "0"}
    g = geo("sapx_rows_n4100")
    assert 8 * 128 <= g["KX"] * g["TX"] < 8 * 256 and CASES["sapx_rows_n4100"]["free"][1] >= 24
    assert CASES["sapx_rows_n4100"]["flags"] & fc.FP_SAPX and not CASES["sapx_rows_off_n4100"]["flags"] & fc.FP_SAPX
    assert CASES["sapx_rows_n4100"]["inst"] == CASES["sapx_rows_off_n4100"]["inst"]
    assert not expected("u32n", 4100, {"TD_FOREST": "0"}, 23, 1000)["flags"] & fc.FP_SAPX       # the rule's other side
    want = {"sapx_min1_n1000": (250, 128, 2, 122), "sapx_min1_n1024": (256, 128, 2, 128), "sapx_min1_n1026": (257, 128, 3, 1),
            "sapx_min1_u16_n2048": (256, 256, 1, 256), "sapx_min1_u16_n2056": (257, 256, 2, 1)}
    for name, (nchunks, TX, KX, last) in want.items():
        g = geo(name)
        assert (g["nchunks"], g["TX"], g["KX"], g["sapx_last_wg_chunks"]) == (nchunks, TX, KX, last), name
        assert CASES[name]["flags"] & fc.FP_SAPX and env_of(name)["TD_SAPX_MIN"] == "1"
    assert CASES["sapx_min1_n1026"]["inst"]["n"] % 4 != 0
    assert all(geo(n)["KX"] <= fc.SX_KMAX for n in CASES)


def test_edges_k_forest():
    want = {64: (1, 64), 65: (2, 1), 66: (2, 2), 67: (2, 3), 127: (2, 63), 128: (2, 64), 129: (3, 1), 1000: (16, 40)}
    for n, (grid, last) in want.items():
        f = forest_geometry(n)
        assert (f["CW"], f["TB"], f["grid"], f["last_slice_cols"], f["a_pcl"]) == (64, 1024, grid, last, 1), n
        assert CASES["forest_n%d" % n]["flags"] == fc.FP_FOREST and env_of("forest_n%d" % n) == {"TD_FOREST_MIN_N": "64"}
    assert {n % 4 for n in want} == {0, 1, 2, 3}
    assert CASES["forest_wide_n129"]["kind"] == "u32" and CASES["forest_n2049"]["section"] == "default"
    assert forest_geometry(2049)["grid"] == 33 and forest_geometry(2049)["last_slice_cols"] == 1
    a, b = forest_geometry(16384), forest_geometry(16388)
    assert (a["CW"], a["TB"], a["grid"], a["a_pcl"], a["dyn"]) == (64, 1024, 256, 1, 6 * 16384)
    assert (b["CW"], b["TB"], b["grid"], b["a_pcl"], b["dyn"]) == (128, 512, 129, 0, 2 * 16388)
    assert CASES["forest_n16384"]["section"] == CASES["forest_n16388"]["section"] == "default"
    # nothing free: the early return, no launch; below the threshold, 2-byte cells or TD_FOREST=0: another finisher
    assert expected("u32n", 2049, {}, 0, 0)["flags"] == fc.FP_FOREST_NONE
    assert not expected("u32n", 2047, {}, 40, 0)["flags"] & fc.FP_FOREST and not expected("u16", 4096, {}, 40, 0)["flags"] & fc.FP_FOREST


def test_fallback_rows_say_what_they_emulate():
    """items 3 to 5: the sizes where a cooperative kernel is the default, run with that kernel switched off"""
    for name, c in CASES.items():
        env, n = env_of(name), c["inst"]["n"]
        dflt = expected(c["kind"], n, {k: v for k, v in env.items() if k not in ("TD_FOREST", "TD_SAPX")}, c["free"][1], c["free"][0] - c["free"][1])
        took = {"k_forest": fc.FP_FOREST, "k_sapx": fc.FP_SAPX}
        if c["emulates"] is None:
            continue
        first = c["emulates"].split("+")[0]
        assert dflt["flags"] & took[first], name                     # by default the cooperative kernel answers this size
        assert not c["flags"] & (fc.FP_FOREST | (fc.FP_SAPX if "k_sapx" in c["emulates"] else 0)), name
        assert env.get("TD_FOREST") == "0" or c["kind"] == "u16", name
    assert sum(1 for c in CASES.values() if c["emulates"]) >= 15
