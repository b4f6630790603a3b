"""The device-resident simulator world on a stand-to-stand distance table (td_sim_create_dist, DeviceSimulator(dist=...))
against the Python world model on the same table.  All comparisons are exact integer equality.

1. trace-driven, every world of sim_dist_worlds.py: the CPU run of Simulator + OracleDistTickBackend gives, per tick, the temp
   lists and the backend's decisions; the device world must build the same lists and, fed the SAME decisions, hold the same
   ten state arrays, metrics and log line after every tick, whatever ties the GPU solver breaks;
2. a table filled with |a - b| is the line world (the oracle runs of sim_worlds.py);
3. through td_sim_step in lockstep with Simulator + HipTickBackend(dist=D): both sides call td_tick with the same arguments;
4. the reference's committed log t = 0 .. 49 with dist = line(50);
5. the hand-checked one-way pair, both orientations;
6. the C-ABI contract of td_sim_create_dist."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_dist_worlds as sd
import sim_worlds as sw

GOLD = os.path.join(HERE, "golden")
pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ENOINIT = -1, -3


def device_world(td, w, rows, D):
    return td.DeviceSimulator(rows, n_cabs=w["cabs"], drop_time=w["drop_time"], max_non_lcm=w["max_non_lcm"], big_cost=sw.BIG_COST, dist=D)


def assert_same_state(dev, host_state, where):
    got = dev.state()
    for k, v in host_state.items():
        assert np.array_equal(got[k], v), (where, k, np.nonzero(got[k] != v)[0][:8].tolist())


def trace_driven(td, run, D, name):
    w = run["world"]
    dev = device_world(td, w, run["rows"], D)
    assert dev.n_stands == D.shape[0]
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


@pytest.mark.parametrize("name", list(sd.WORLDS))
def test_trace_driven_against_the_oracle(td, name):
    trace_driven(td, sd.oracle_run(name), sd.table(name), name)


@pytest.mark.parametrize("name", ["tiny", "mid65"])
def test_line_table_is_the_line_world(td, name):
    run = sw.oracle_run(name)
    trace_driven(td, run, sd.line(run["world"]["stands"]), name)


def lockstep(td, rows, D, w, monkeypatch):
    from taxidispatcher_amd import simulator
    sw.patch_constants(monkeypatch, w)
    host = simulator.Simulator(rows, simulator.HipTickBackend(dist=D), n_cabs=w["cabs"], dist=D)
    dev = device_world(td, w, rows, D)
    for t in range(w["ticks"]):
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


@pytest.mark.parametrize("name", sd.SMALL)
def test_through_step_in_lockstep_with_the_product_path(td, name, monkeypatch):
    w, D = sd.world(name), sd.table(name)
    host = lockstep(td, sd.gen_demand(D, **w), D, w, monkeypatch)
    assert len(host.log) > 0 and host.m["total_pickup_numb"] > 0


def test_golden_log_on_a_line_table(td):
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(GOLD, "taxi_demand.txt.gz"))
    dev = td.DeviceSimulator(rows, dist=sd.line(50))
    log = [l.strip() for l in dev.run(50)]
    gold = [l.strip() for l in open(os.path.join(GOLD, "simulog_solv_t0_49.txt")).read().split("\n") if l.strip()]
    assert len(gold) == 50 and log == gold
    assert log[49].endswith("demand=218, supply=600. ; OPT count=32")
    dev.close()


ONE_WAY = np.array([[0, 1, 9], [9, 0, 9], [9, 9, 0]], np.int32)
PAIR_ROWS = np.array([[0, 1, 2, 0, 0]], np.int64)


def pair_world(td, D):
    return td.DeviceSimulator(PAIR_ROWS, n_cabs=1, drop_time=3, max_non_lcm=4, big_cost=sw.BIG_COST, dist=D)


def test_one_way_pair(td):
    """one cab at stand 0, one request 1 -> 2 at t = 0, d[0][1] = 1 but d[1][0] = 9, drop_time 3"""
    dev = pair_world(td, ONE_WAY)
    assert dev.tick(0) == "t:0. Initial Count of demand=1, supply=1. ; OPT count=1"
    st = dev.state()
    assert [int(st[k][0]) for k in ("c_from", "c_to", "c_clnt", "c_onboard", "c_start", "d_cab")] == [0, 1, 0, 0, 0, 0]
    assert dev.m["total_pickup_time"] == 1 and dev.m["total_pickup_numb"] == 0
    assert dev.tick(1) is None                         # arrives exactly at t = 1 = d[0][1]: the passenger is picked up
    st = dev.state()
    assert [int(st[k][0]) for k in ("c_from", "c_to", "c_onboard", "c_start", "d_pick")] == [1, 2, 1, 1, 1]
    assert dev.m["total_pickup_numb"] == 1
    for t in range(2, 12):                             # the trip takes d[1][2] = 9 ticks
        assert dev.tick(t) is None
        st = dev.state()
        assert (int(st["c_onboard"][0]), int(st["c_from"][0])) == ((1, 1) if t < 10 else (0, 2)), t
    assert dev.m["total_dropped"] == 0
    dev.close()


def test_one_way_pair_transposed(td):
    dev = pair_world(td, ONE_WAY.T.copy())
    for t in range(6):
        assert dev.tick(t) is None, t                  # no cab is near: no demand, no line
        assert dev.m["total_dropped"] == (1 if t >= 3 else 0), t
        st = dev.state()
        assert int(st["d_cab"][0]) == (-2 if t >= 3 else -1) and int(st["c_to"][0]) == 0 and int(st["c_clnt"][0]) == -1, t
    dev.close()


# ---- the C-ABI contract of td_sim_create_dist
def ws_bytes(lib):
    v = ctypes.c_int64(-1)
    assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
    return v.value


def raw_create(lib, w, rows, dist, fn="td_sim_create_dist"):
    from taxidispatcher_amd import _ffi
    cols = [_ffi.as_i32(rows[:, k]) for k in (0, 1, 2, 4)]
    h = ctypes.c_void_p()
    args = [w["cabs"], w["stands"], w["drop_time"], w["max_non_lcm"], sw.BIG_COST, int(rows.shape[0])] + [_ffi.addr(c) for c in cols]
    if fn == "td_sim_create_dist":
        args.append(_ffi.addr(dist))
    rc = getattr(lib, fn)(*args, ctypes.byref(h))
    return rc, h


def raw_run(lib, h, w, ticks):
    n_req_cap = 4096
    lines = []
    for t in range(ticks):
        line = np.zeros(9, np.int32)
        assert lib.td_sim_step(h, t, line.ctypes.data) == 0
        lines.append(line.tolist())
    arrs = [np.zeros(max(w["cabs"], n_req_cap), np.int32) for _ in range(10)]
    assert lib.td_sim_state(h, *[a.ctypes.data for a in arrs]) == 0
    m = np.zeros(9, np.int64)
    assert lib.td_sim_metrics(h, m.ctypes.data) == 0
    return lines, [a.tolist() for a in arrs], m.tolist()


def test_null_table_is_td_sim_create(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    w = sw.WORLDS["tiny"]
    rows = sw.gen_demand(**w)
    assert rows.shape[0] <= 4096
    out = []
    for fn in ("td_sim_create", "td_sim_create_dist"):
        rc, h = raw_create(lib, w, rows, None, fn)
        assert rc == 0 and h.value
        out.append(raw_run(lib, h, w, 12))
        assert lib.td_sim_destroy(h) == 0
    assert out[0] == out[1] and any(l[0] for l in out[0][0])


def test_host_table_device_table_and_the_copy(td):
    """a host table and a device table give the same world, and the handle keeps its own copy of either"""
    import torch
    name = "grid13x5ow"
    w, D = sd.world(name), sd.table(name)
    rows = sd.gen_demand(D, **w)
    ref = device_world(td, w, rows, D)
    ref.run(12)
    host_t = np.array(D, np.int32)
    dev_t = torch.as_tensor(np.array(D, np.int32), device="cuda")
    for tab in (host_t, dev_t):
        dev = device_world(td, w, rows, tab)
        if tab is host_t:
            tab[:] = 1                                 # the caller's table is the caller's again
        else:
            tab.fill_(1)
            torch.cuda.synchronize()
        assert dev.run(12) == ref.log and len(ref.log) > 0
        assert dev.m == ref.m
        assert_same_state(dev, ref.state(), "host table" if tab is host_t else "device table")
        dev.close()
    ref.close()


def test_4096_stands_create_and_destroy(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    w = dict(cabs=1, stands=4096, drop_time=10, max_non_lcm=600)
    rows = np.array([[0, 4095, 4090, 0, 0]], np.int64)
    before = ws_bytes(lib)
    rc, h = raw_create(lib, w, rows, sd.line(4096))
    assert rc == 0 and h.value
    assert ws_bytes(lib) - before >= 4 * (4096 * 4096 + 2 * 4096 * 128)     # the copy and the two bit matrices
    line = np.zeros(9, np.int32)
    assert lib.td_sim_step(h, 0, line.ctypes.data) == 0 and line[0] == 0     # the one cab (stand 0) is far from stand 4095
    assert lib.td_sim_destroy(h) == 0
    assert ws_bytes(lib) == before


def bad_table(what):
    d = sd.line(5).astype(np.int32)
    if what == "negative":
        d[1, 3] = -1
    elif what == "diagonal":
        d[2, 2] = 1
    elif what == "zero":
        d[3, 1] = 0
    elif what == "too large":
        d[0, 4] = 0x20000000
    return d


@pytest.mark.parametrize("what", ["4097 stands", "negative", "diagonal", "zero", "too large"])
def test_invalid_table_is_einval(td, what):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    rows = np.array([[0, 1, 2, 0, 0]], np.int64)
    if what == "4097 stands":
        w, D = dict(cabs=1, stands=4097, drop_time=3, max_non_lcm=4), sd.line(4097)
    else:
        w, D = dict(cabs=2, stands=5, drop_time=3, max_non_lcm=4), bad_table(what)
    before = ws_bytes(lib)
    rc, h = raw_create(lib, w, rows, D)
    assert rc == TD_EINVAL and h.value is None and lib.td_last_error()
    assert ws_bytes(lib) == before
    if what == "too large":     # the largest entry a table may hold is accepted
        D[0, 4] = 0x1fffffff
        rc, h = raw_create(lib, w, rows, D)
        assert rc == 0 and h.value and lib.td_sim_destroy(h) == 0 and ws_bytes(lib) == before
    with pytest.raises((ValueError, td.TdError)):
        td.DeviceSimulator(rows, n_cabs=w["cabs"], drop_time=3, max_non_lcm=4, big_cost=sw.BIG_COST, dist=D if what != "too large" else bad_table(what))


def test_python_arguments(td):
    rows = np.array([[0, 1, 2, 0, 0]], np.int64)
    with pytest.raises(ValueError):
        td.DeviceSimulator(rows, n_cabs=1, n_stands=6, dist=sd.line(5))     # an explicit n_stands that is not the table's
    dev = td.DeviceSimulator(rows, n_cabs=1, n_stands=5, dist=sd.line(5))
    assert dev.n_stands == 5
    dev.close()


def test_enoinit_before_td_init():
    """td_sim_create_dist refuses to run before td_init (a fresh process that never opens the GPU)"""
    from taxidispatcher_amd import _ffi
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
h = ctypes.c_void_p()
d = (ctypes.c_int32 * 25)()
V = ctypes.c_void_p
lib.td_sim_create_dist.argtypes = [ctypes.c_int] * 6 + [V] * 6
print(lib.td_sim_create_dist(2, 5, 3, 4, 250000, 0, None, None, None, None, d, ctypes.byref(h)), h.value)
"""
    out = subprocess.run([sys.executable, "-c", code, _ffi.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "%d None" % TD_ENOINIT, out.stdout
