"""Routed worlds in a batch, what needs no device: the three C-ABI declarations, their ctypes signatures and their export from
the built library, the refusals DeviceSimulatorBatch(route=...) makes before it touches the library, and the command line of
tools/gpu_simulate.py (--route with a --cabs list).  The worlds themselves: tests/test_gpu_simb_route.py."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("td_simb_route", "td_simb_route_state", "td_simb_route_metrics")


def test_the_header_and_the_ffi_agree_on_the_new_calls():
    from taxidispatcher_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "taxidispatcher_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    counts = {}
    for name in NAMES:
        m = re.search(r"TD_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[0].startswith("td_simb *"), (name, params[0])
        res, args = _ffi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            assert a is (ctypes.c_void_p if "*" in p or "[" in p else ctypes.c_int), (name, p, a)
        counts[name] = len(params)
    assert counts == dict(td_simb_route=2, td_simb_route_state=5, td_simb_route_metrics=2)


def test_the_calls_are_built_and_exported():
    import __graft_entry__ as entry
    entry.build()
    from taxidispatcher_amd import _ffi
    lib = _ffi.load()
    for name in NAMES:
        assert getattr(lib, name) is not None, name


def test_keyword_refusals_come_before_the_library():
    """no device is needed: each refusal is raised before the handle is made"""
    from taxidispatcher_amd import simulator as S
    rows = np.zeros((0, 5), np.int64)
    # route= is a keyword of the batch (taken with its extra keywords; nothing else is)
    assert inspect.signature(S.DeviceSimulatorBatch.__init__).parameters["routing"].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(TypeError, match="unexpected keyword argument 'routes'"):
        S.DeviceSimulatorBatch([rows, rows], [3, 5], routes=True)
    for name in ("set_route", "route_state", "route_metrics"):
        assert callable(getattr(S.DeviceSimulatorBatch, name)), name
    with pytest.raises(ValueError, match="world 0 needs a pool_n policy"):
        S.DeviceSimulatorBatch([rows, rows], [3, 5], route=True)
    with pytest.raises(ValueError, match="world 1 needs a pool_n policy"):      # the world is named
        S.DeviceSimulatorBatch([rows, rows], [3, 5], route=[True, True], pool_n=[(4, 2), None])
    with pytest.raises(ValueError, match="world 0 needs a pool_n policy"):
        S.DeviceSimulatorBatch([rows, rows], [3, 5], route=[True, False], pool=["optimal", "greedy"])
    with pytest.raises(ValueError, match="not built"):
        S.DeviceSimulatorBatch([rows, rows], [3, 5], route=True, pool_n=2, events=True)
    with pytest.raises(ValueError, match="not built"):
        S.DeviceSimulatorBatch([rows, rows], [3, 5], route=[False, True], pool_n=[None, (3, 2)], events=True)
    with pytest.raises(ValueError, match="3 entries for 2 worlds"):
        S.DeviceSimulatorBatch([rows, rows], [3, 5], route=[True, False, True], pool_n=2)
    assert S.DeviceSimulatorBatch.ROUTE_M_KEYS == S.DeviceSimulator.ROUTE_M_KEYS


def test_the_command_line_of_gpu_simulate(capsys):
    """the parser only: no world is made"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gpu_simulate
    finally:
        sys.path.pop(0)
    with pytest.raises(SystemExit) as e:
        gpu_simulate.parse(["--route", "--cabs", "3,5", "--events", "x"])
    assert e.value.code == 2 and "--route goes with --pool-n and no --events" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        gpu_simulate.parse(["--route", "--cabs", "3,5", "--pool-n", "4,2", "--events", "x"])
    assert e.value.code == 2 and "no --events" in capsys.readouterr().err
    ap, args = gpu_simulate.parse(["--route", "--cabs", "3,5", "--pool-n", "4,2"])
    assert args.route and args.cabs == "3,5" and args.pool_n == "4,2"
