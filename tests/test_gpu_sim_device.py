"""The device-resident simulator world (td_sim_*, simulator.DeviceSimulator) against the Python world model.

1. the reference's committed log t = 0 .. 49 through DeviceSimulator.tick (td_sim_step);
2. trace-driven: the CPU run of Simulator + OracleTickBackend gives, per tick, the temp lists and the backend's decisions;
   the device world must build the same lists (td_sim_begin / td_sim_model) and, fed the SAME decisions (td_sim_apply),
   hold the same ten state arrays, metrics and log line after every tick -- exact, whatever ties the GPU solver breaks;
3. lockstep with the product path (Simulator + HipTickBackend) on the committed input for all 120 ticks, which rests on
   td_tick being bit-reproducible (test_deterministic_output);
4. small worlds through td_sim_step;
5. the C-ABI contract of the eight entry points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_worlds as sw

GOLD = os.path.join(HERE, "golden")
pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ENOINIT = -1, -3


def golden_rows():
    from taxidispatcher_amd import simulator
    return simulator.read_demand(os.path.join(GOLD, "taxi_demand.txt.gz"))


def device_world(td, name):
    w = sw.WORLDS[name]
    return td.DeviceSimulator(sw.gen_demand(**w), n_cabs=w["cabs"], n_stands=w["stands"], drop_time=w["drop_time"],
                              max_non_lcm=w["max_non_lcm"], big_cost=sw.BIG_COST)


def assert_same_state(dev, host_state, where):
    got = dev.state()
    for k, v in host_state.items():
        assert np.array_equal(got[k], v), (where, k, np.nonzero(got[k] != v)[0][:8].tolist())


def test_golden_log(td):
    dev = td.DeviceSimulator(golden_rows())
    log = [l.strip() for l in dev.run(50)]
    gold = [l.strip() for l in open(os.path.join(GOLD, "simulog_solv_t0_49.txt")).read().split("\n") if l.strip()]
    assert len(gold) == 50 and log == gold
    assert log[49].endswith("demand=218, supply=600. ; OPT count=32")
    dev.close()


@pytest.mark.parametrize("name", list(sw.WORLDS))
def test_trace_driven_against_the_oracle(td, name):
    run = sw.oracle_run(name)
    w = run["world"]
    dev = device_world(td, name)
    for rec in run["ticks"]:
        t = rec["t"]
        info = dev.begin(t)
        if rec["n_dem"] == 0:
            assert info == (0, 0, 0, 0), t
            line = None
        else:
            assert info == (1, rec["n_dem"], rec["n_sup"], len(rec["dem_from"])), t
            cab_to, dem_from = dev.model()
            assert cab_to.tolist() == rec["cab_to"] and dem_from.tolist() == rec["dem_from"], t
            res = rec["res"]
            if res is None:     # no supply: no pool, no model, the line ends in "; OPT count=0"
                opt = dev.apply()
                line = dev.format_line(t, [1, rec["n_dem"], 0, 0, 0, 0, 0, 0, opt])
            else:
                opt = dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
                lcm = max(info[2], info[3]) > w["max_non_lcm"]
                line = dev.format_line(t, [1, rec["n_dem"], rec["n_sup"], lcm, len(res["lcm_rows"]), lcm and res["solved"],
                                           len(res["kept_dems"]), len(res["kept_cabs"]), opt])
        assert line == rec["line"], t
        assert dev.m == rec["m"], t
        assert_same_state(dev, rec["state"], (name, t))
    dev.close()


def lockstep(td, rows, ticks, **kw):
    from taxidispatcher_amd import simulator
    host = simulator.Simulator(rows, simulator.HipTickBackend(), n_cabs=kw.get("n_cabs", simulator.N_CABS))
    dev = td.DeviceSimulator(rows, **kw)
    for t in range(ticks):
        a, b = host.tick(t), dev.tick(t)
        assert a == b, t
        if a is not None:
            host.log.append(a)
            dev.log.append(b)
    assert dev.log == host.log
    assert dev.m == host.m
    assert dev.metrics_text() == host.metrics_text()
    assert_same_state(dev, sw.state_of(host), "final")
    dev.close()
    return host


def test_lockstep_with_the_product_path_120_ticks(td):
    host = lockstep(td, golden_rows(), 120)
    assert len(host.log) == 120 and host.m["max_POOL_size"] > 0 and host.m["total_LCM_used"] > 0


@pytest.mark.parametrize("name", ["tiny", "mid65"])
def test_small_worlds_through_step(td, name, monkeypatch):
    w = sw.WORLDS[name]
    sw.patch_constants(monkeypatch, w)
    lockstep(td, sw.gen_demand(**w), w["ticks"], n_cabs=w["cabs"], n_stands=w["stands"], drop_time=w["drop_time"],
             max_non_lcm=w["max_non_lcm"], big_cost=sw.BIG_COST)


def test_one_cab(td, monkeypatch):
    w = dict(sw.WORLDS["tiny"], cabs=1)
    sw.patch_constants(monkeypatch, w)
    host = lockstep(td, sw.gen_demand(**w), w["ticks"], n_cabs=1, n_stands=w["stands"], drop_time=w["drop_time"],
                    max_non_lcm=w["max_non_lcm"], big_cost=sw.BIG_COST)
    assert host.m["total_pickup_numb"] > 0 and host.m["total_dropped"] > 0


def test_empty_request_table(td):
    dev = td.DeviceSimulator(np.zeros((0, 5), np.int64), n_cabs=3, n_stands=5, drop_time=3, max_non_lcm=4, big_cost=sw.BIG_COST)
    assert dev.run(5) == []
    assert all(v == 0 for v in dev.m.values())
    st = dev.state()
    assert st["c_from"].tolist() == [0, 1, 2] == st["c_to"].tolist() and st["c_clnt"].tolist() == [-1, -1, -1]
    assert st["d_cab"].size == 0
    dev.close()


def test_two_handles_are_independent_worlds(td):
    alone = {}
    for name in ("tiny", "small"):
        dev = device_world(td, name)
        alone[name] = (dev.run(30), dev.m, dev.state())
        dev.close()
    a, b = device_world(td, "tiny"), device_world(td, "small")
    for t in range(30):
        for dev in (a, b):
            line = dev.tick(t)
            if line is not None:
                dev.log.append(line)
    for name, dev in (("tiny", a), ("small", b)):
        log, m, st = alone[name]
        assert dev.log == log and dev.m == m
        assert_same_state(dev, st, name)
        dev.close()


def test_workspace_bytes_return_after_destroy(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()

    def ws():
        v = ctypes.c_int64(-1)
        assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
        return v.value
    device_world(td, "small").run(10)      # the library's own grow-only buffers reach their size for this world
    before = ws()
    dev = device_world(td, "small")
    held = ws() - before
    n_req, n_cabs = dev.n_req, dev.n_cabs
    assert held >= 4 * (14 * n_req + 5 * n_cabs)     # at least the two tables
    dev.run(10)
    assert ws() - before == held                  # a handle does not grow
    dev.close()
    assert ws() == before


def split_tick_raw(lib, td, h, t, cap, device):
    """one tick through begin / model / td_tick / apply on the raw ABI; device=True: every array is device memory"""
    import torch
    from taxidispatcher_amd import _ffi
    info = np.zeros(4, np.int32)
    assert lib.td_sim_begin(h, t, info.ctypes.data) == 0
    if not info[0]:
        return None
    n_s, n_d = int(info[2]), int(info[3])
    opt = ctypes.c_int32(0)
    if n_s == 0:
        assert lib.td_sim_apply(h, 0, None, None, 0, 0, None, ctypes.byref(opt)) == 0
        return [1, info[1], 0, 0, 0, 0, 0, 0, opt.value]
    if device:
        cab, dem = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(cap, dtype=torch.int32, device="cuda")
    else:
        cab, dem = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    assert lib.td_sim_model(h, _ffi.addr(cab), _ffi.addr(dem)) == 0
    return cab[:n_s], dem[:n_d], info


def test_split_tick_with_host_and_device_arrays(td):
    """begin -> model -> decisions (dispatch.tick = td_tick) -> apply, with the model and the decisions in host memory
    and in device memory: both worlds keep the log of DeviceSimulator.tick"""
    import torch
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    w = sw.WORLDS["mid"]
    ref = device_world(td, "mid")
    ref.run(25)
    for device in (False, True):
        dev = device_world(td, "mid")
        cap = max(dev.n_req, dev.n_cabs)
        for t in range(25):
            got = split_tick_raw(lib, td, dev._h, t, cap, device)
            if got is None:
                continue
            if isinstance(got, list):
                dev.log.append(dev.format_line(t, got))
                continue
            cab, dem, info = got
            res = td.tick(cab, dem, None, big_cost=sw.BIG_COST, drop_time=w["drop_time"], max_non_lcm=w["max_non_lcm"])
            rows, cols, r2c = res["lcm_rows"], res["lcm_cols"], res["row_to_col"]
            if device:
                rows, cols, r2c = (torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in (rows, cols, r2c))
            opt = ctypes.c_int32(0)
            assert lib.td_sim_apply(dev._h, len(rows), _ffi.addr(rows) if len(rows) else None, _ffi.addr(cols) if len(cols) else None,
                                    int(res["solved"]), len(r2c), _ffi.addr(r2c) if len(r2c) else None, ctypes.byref(opt)) == 0
            lcm = max(info[2], info[3]) > w["max_non_lcm"]
            dev.log.append(dev.format_line(t, [1, info[1], info[2], lcm, len(rows), lcm and res["solved"], len(res["kept_dems"]),
                                               len(res["kept_cabs"]), opt.value]))
        assert dev.log == ref.log and dev.m == ref.m
        assert_same_state(dev, ref.state(), "device arrays" if device else "host arrays")
        dev.close()
    ref.close()


def test_argument_and_sequencing_rules(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    ids, frm, to, at = (np.array(v, np.int32) for v in ([7, 9], [0, 3], [1, 4], [0, 2]))
    p = lambda a: a.ctypes.data
    h = ctypes.c_void_p()

    def create(n_cabs=2, n_stands=5, drop=3, mnl=4, big=sw.BIG_COST, n_req=2, a=ids, b=frm, c=to, d=at, out=h):
        return lib.td_sim_create(n_cabs, n_stands, drop, mnl, big, n_req, p(a) if a is not None else None, p(b) if b is not None else None,
                                 p(c) if c is not None else None, p(d) if d is not None else None, ctypes.byref(out) if out is not None else None)
    # null or negative arguments
    assert create(out=None) == TD_EINVAL
    for kw in (dict(n_cabs=0), dict(n_cabs=-1), dict(n_stands=0), dict(drop=-1), dict(mnl=-1), dict(big=-1), dict(n_req=-1), dict(a=None),
               dict(b=None), dict(c=None), dict(d=None)):
        assert create(**kw) == TD_EINVAL, kw
        assert h.value is None
    assert create(a=np.array([7, 7], np.int32)) == TD_EINVAL and b"unique" in lib.td_last_error()      # request ids must be unique
    assert create(b=np.array([0, 5], np.int32)) == TD_EINVAL       # a stand outside 0 .. n_stands - 1
    assert create(c=np.array([-1, 4], np.int32)) == TD_EINVAL
    assert create(d=np.array([0, -2], np.int32)) == TD_EINVAL
    assert create() == 0 and h.value
    info, line, opt = np.zeros(4, np.int32), np.zeros(9, np.int32), ctypes.c_int32(7)
    cab, dem = np.zeros(4, np.int32), np.zeros(4, np.int32)
    assert lib.td_sim_begin(None, 0, p(info)) == TD_EINVAL and lib.td_sim_begin(h, 0, None) == TD_EINVAL
    assert lib.td_sim_begin(h, -1, p(info)) == TD_EINVAL
    assert lib.td_sim_step(None, 0, p(line)) == TD_EINVAL and lib.td_sim_step(h, 0, None) == TD_EINVAL and lib.td_sim_step(h, -1, p(line)) == TD_EINVAL
    assert lib.td_sim_model(None, p(cab), p(dem)) == TD_EINVAL
    assert lib.td_sim_apply(None, 0, None, None, 0, 0, None, ctypes.byref(opt)) == TD_EINVAL
    assert lib.td_sim_state(None, *([None] * 10)) == TD_EINVAL and lib.td_sim_metrics(None, p(np.zeros(9, np.int64))) == TD_EINVAL
    assert lib.td_sim_metrics(h, None) == TD_EINVAL
    # model / apply without a begin
    assert lib.td_sim_model(h, p(cab), p(dem)) == TD_EINVAL
    assert lib.td_sim_apply(h, 0, None, None, 1, 0, None, ctypes.byref(opt)) == TD_EINVAL
    # t = 0: request 7 (stand 0) is due, cabs stand at 0 and 1 -> a model of 2 cabs x 1 request
    assert lib.td_sim_begin(h, 0, p(info)) == 0 and info.tolist() == [1, 1, 2, 1]
    assert lib.td_sim_begin(h, 0, p(info)) == TD_EINVAL            # twice for one tick
    assert lib.td_sim_begin(h, 1, p(info)) == TD_EINVAL            # the tick still waits for its apply
    assert lib.td_sim_step(h, 1, p(line)) == TD_EINVAL
    assert lib.td_sim_model(h, None, p(dem)) == TD_EINVAL and lib.td_sim_model(h, p(cab), None) == TD_EINVAL
    assert lib.td_sim_model(h, p(cab), p(dem)) == 0 and cab[:2].tolist() == [0, 1] and dem[:1].tolist() == [0]
    r2c = np.array([0, 1], np.int32)
    assert lib.td_sim_apply(h, -1, None, None, 1, 2, p(r2c), ctypes.byref(opt)) == TD_EINVAL
    assert lib.td_sim_apply(h, 0, None, None, 1, -1, p(r2c), ctypes.byref(opt)) == TD_EINVAL
    assert lib.td_sim_apply(h, 0, None, None, 1, 2, None, ctypes.byref(opt)) == TD_EINVAL
    assert lib.td_sim_apply(h, 0, None, None, 1, 2, p(r2c), None) == TD_EINVAL
    assert lib.td_sim_apply(h, 1, None, None, 1, 2, p(r2c), ctypes.byref(opt)) == TD_EINVAL
    assert lib.td_sim_apply(h, 0, None, None, 1, 2, p(r2c), ctypes.byref(opt)) == 0 and opt.value == 1
    assert lib.td_sim_apply(h, 0, None, None, 1, 2, p(r2c), ctypes.byref(opt)) == TD_EINVAL   # applied already
    assert lib.td_sim_model(h, p(cab), p(dem)) == TD_EINVAL
    assert lib.td_sim_begin(h, 0, p(info)) == TD_EINVAL            # time runs forward
    # any state pointer may be NULL; the client is reported by its id
    c_clnt, d_cab = np.zeros(2, np.int32), np.zeros(2, np.int32)
    assert lib.td_sim_state(h, None, None, p(c_clnt), None, None, p(d_cab), None, None, None, None) == 0
    assert c_clnt.tolist() == [7, -1] and d_cab.tolist() == [0, -1]
    assert lib.td_sim_state(h, *([None] * 10)) == 0
    # t = 1: request 9 is not due: no demand, so nothing to model or apply
    assert lib.td_sim_begin(h, 1, p(info)) == 0 and info.tolist() == [0, 0, 0, 0]
    assert lib.td_sim_apply(h, 0, None, None, 0, 0, None, ctypes.byref(opt)) == TD_EINVAL
    assert lib.td_sim_model(h, p(cab), p(dem)) == TD_EINVAL
    assert lib.td_sim_begin(h, 1, p(info)) == TD_EINVAL
    assert lib.td_sim_destroy(h) == 0 and lib.td_sim_destroy(None) == 0


def test_a_pair_outside_the_model_applies_nothing(td):
    run = sw.oracle_run("tiny")
    rec = next(r for r in run["ticks"] if r["res"] is not None and len(r["res"]["lcm_rows"]) > 0)
    dev, ref = device_world(td, "tiny"), device_world(td, "tiny")
    for world in (dev, ref):      # the recorded decisions up to the chosen tick: both worlds are the oracle run's world
        for r in run["ticks"][:rec["t"]]:
            if world.begin(r["t"])[0]:
                res = r["res"]
                world.apply(*((res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"]) if res is not None else ()))
    info = dev.begin(rec["t"])
    assert ref.begin(rec["t"]) == info == (1, rec["n_dem"], rec["n_sup"], len(rec["dem_from"]))
    before = dev.state()
    res = rec["res"]
    bad = np.asarray(res["lcm_cols"]).copy()
    bad[-1] = info[3]
    with pytest.raises(td.TdError):
        dev.apply(res["lcm_rows"], bad, res["solved"], res["row_to_col"])
    for k, v in dev.state().items():
        assert np.array_equal(v, before[k]), k
    args = (res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
    assert dev.apply(*args) == ref.apply(*args)      # the tick still waited for its decisions
    assert dev.m == ref.m == rec["m"]
    assert_same_state(dev, rec["state"], "after the refused apply")
    dev.close()
    ref.close()


def test_enoinit_before_td_init():
    """every td_sim entry point refuses to run before td_init (a fresh process that never opens the GPU)"""
    from taxidispatcher_amd import _ffi
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
h = ctypes.c_void_p()
a = (ctypes.c_int32 * 16)()
m = (ctypes.c_int64 * 9)()
o = ctypes.c_int32(0)
V = ctypes.c_void_p
lib.td_sim_create.argtypes = [ctypes.c_int] * 6 + [V] * 5
lib.td_sim_begin.argtypes = [V, ctypes.c_int, V]
lib.td_sim_step.argtypes = [V, ctypes.c_int, V]
lib.td_sim_model.argtypes = [V, V, V]
lib.td_sim_apply.argtypes = [V, ctypes.c_int, V, V, ctypes.c_int, ctypes.c_int, V, V]
lib.td_sim_state.argtypes = [V] * 11
lib.td_sim_metrics.argtypes = [V, V]
lib.td_sim_destroy.argtypes = [V]
fake = ctypes.addressof(a)
rcs = [lib.td_sim_create(2, 5, 3, 4, 250000, 0, None, None, None, None, ctypes.byref(h)),
       lib.td_sim_begin(fake, 0, a), lib.td_sim_step(fake, 0, a), lib.td_sim_model(fake, a, a),
       lib.td_sim_apply(fake, 0, None, None, 0, 0, None, ctypes.byref(o)), lib.td_sim_state(fake, *([None] * 10)),
       lib.td_sim_metrics(fake, m), lib.td_sim_destroy(None)]
print(rcs, h.value)
"""
    out = subprocess.run([sys.executable, "-c", code, _ffi.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "%r None" % ([TD_ENOINIT] * 7 + [0]), out.stdout
