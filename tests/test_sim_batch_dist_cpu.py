"""CPU tier of the batched simulator handle on a distance table (td_simb_create_dist, DeviceSimulatorBatch(dist=...)): the
families of sim_batch_dist_worlds.py reach what the GPU tier (tests/test_gpu_sim_batch_dist.py) compares them on; the
argument checks of DeviceSimulatorBatch that need no GPU raise before the library is touched; the header declares the call
and the binding lists it."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_dist_worlds as sbd
import sim_dist_worlds as sd

ROOT = os.path.dirname(HERE)


def test_families_reach_every_branch_both_directions_and_the_second_stride():
    sbd.check_cover()
    for which in "DRH":
        c, D, runs = sbd.family(which)
        assert D.shape == (c["stands"], c["stands"])
        print(which, [(n, r["cover"]) for n, r in runs])
    assert sbd.city("D")["stands"] == 65 and sbd.city("R")["stands"] == 12 and sbd.city("H")["stands"] == 2100
    assert [n for n, _ in sbd.family("D")[2]] == ["D1", "D7", "D40", "D200", "Dempty"]
    assert [n for n, _ in sbd.family("H")[2]][0] == "H1025"


ROWS = np.array([[0, 1, 2, 0, 0], [1, 4, 3, 0, 1]], np.int64)


def bad_arguments():
    ok = sd.line(5)
    zero = ok.copy()
    zero[3, 1] = 0
    far = ROWS.copy()
    far[1, 1] = 5
    far_to = ROWS.copy()
    far_to[0, 2] = -1
    return {
        "non-square": dict(dist=ok[:4]),
        "bad entry": dict(dist=zero),
        "n_stands disagrees": dict(dist=ok, n_stands=6),
        "request from outside": dict(dist=ok, tables=[ROWS, far]),
        "request to outside": dict(dist=ok, tables=[far_to, ROWS]),
    }


@pytest.mark.parametrize("what", list(bad_arguments()))
def test_bad_arguments_raise_before_the_library_is_touched(what, monkeypatch):
    from taxidispatcher_amd import _ffi, simulator

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_ffi, "lib", touched)
    kw = bad_arguments()[what]
    tables = kw.pop("tables", [ROWS, ROWS])
    with pytest.raises(ValueError, match="distance table"):
        simulator.DeviceSimulatorBatch(tables, [2, 3], drop_time=3, max_non_lcm=4, **kw)
    # the same arguments with a good table get as far as the library
    with pytest.raises(AssertionError, match="touched"):
        simulator.DeviceSimulatorBatch([ROWS, ROWS], [2, 3], drop_time=3, max_non_lcm=4, dist=sd.line(5))
    with pytest.raises(AssertionError, match="touched"):
        simulator.DeviceSimulatorBatch([ROWS, ROWS], [2, 3], n_stands=5, drop_time=3, max_non_lcm=4, dist=sd.line(5))


def test_the_header_declares_the_call_and_the_binding_lists_it():
    import ctypes
    from taxidispatcher_amd import _ffi
    text = open(os.path.join(ROOT, "include", "taxidispatcher_amd.h")).read()
    m = re.search(r"TD_API int td_simb_create_dist\((.*?)\);", text, flags=re.S)
    assert m, "td_simb_create_dist is not declared"
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 13 and "dist" in params[11] and "td_simb **out" in params[12]
    res, args = _ffi.SIGNATURES["td_simb_create_dist"]
    assert res is ctypes.c_int and len(args) == 13
    # td_simb_create plus one table pointer before the handle
    _, base = _ffi.SIGNATURES["td_simb_create"]
    assert args[:11] == base[:11] and args[11] is _ffi.c_i32p and args[12] is base[11]
