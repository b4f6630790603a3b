"""B simulator worlds on ONE shared distance table behind one handle (td_simb_create_dist, DeviceSimulatorBatch(dist=...)).
All comparisons are exact integer equality.

1. trace-driven, exact: the CPU runs of three families of table worlds give, per world and tick, the lists and the backend's
   decisions; the batch must report every world's info and model and, fed ALL worlds' recorded decisions in one
   td_simb_apply, hold every world's ten state arrays, metrics and log line after every tick (k_near_b, way() in the apply
   kernels, arrival);
2. a table batch equals its worlds alone (td_simb_step);
3. a table batch of one and a td_sim table world, fed the same decisions, agree after every tick;
4. lockstep with the host world model on td_tick_batched's / td_pool2_batched's decisions on the table;
5. line(12) as a table equals the line batch;
6. the 2048 limit of td_simb_step on a table;
7. the one-way direction by hand;
8. the C-ABI contract of td_simb_create_dist."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_dist_worlds as sbd
import sim_batch_worlds as sb
import sim_dist_worlds as sd
import sim_worlds as sw

pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ENOINIT = -1, -3
BIG = sb.BIG_COST


@pytest.mark.parametrize("which", ["D", "R", "H"])
def test_trace_driven_table_batch_against_the_oracle(td, which):
    city, D, runs = sbd.family(which)
    dev = sbd.device_batch(td, city, D, runs)
    assert dev.n_stands == D.shape[0]
    B = len(runs)
    for t in range(city["ticks"]):
        recs = [run["ticks"][t] for _, run in runs]
        info = dev.begin(t)
        for b, rec in enumerate(recs):
            want = (0, 0, 0, 0) if rec["n_dem"] == 0 else (1, rec["n_dem"], rec["n_sup"], len(rec["dem_from"]))
            assert tuple(info[b].tolist()) == want, (t, b)
        if any(rec["n_dem"] for rec in recs):
            cab_off, cab_to, dem_off, dem_from = dev.model()
            assert cab_off[0] == 0 and dem_off[0] == 0
            for b, rec in enumerate(recs):
                assert cab_to[cab_off[b]:cab_off[b + 1]].tolist() == rec["cab_to"], (t, b)
                assert dem_from[dem_off[b]:dem_off[b + 1]].tolist() == (rec["dem_from"] if rec["n_dem"] else []), (t, b)
            opt = dev.apply([sb.decisions_of(rec) if rec["n_dem"] else None for rec in recs])
        else:
            opt = np.zeros(B, np.int32)
        m = dev.m
        for b, rec in enumerate(recs):
            assert sb.line_of(dev, city, rec, info[b], int(opt[b])) == rec["line"], (t, b)
            assert m[b] == rec["m"], (t, b)
            sb.assert_same_state(dev, b, rec["state"], (which, t))
    dev.close()


def test_a_table_batch_equals_its_worlds_alone(td):
    city, D, runs = sbd.family("D")
    whole = sbd.device_batch(td, city, D, runs)
    whole.run(city["ticks"])
    assert all(len(l) > 0 for l in whole.logs[:4]) and whole.logs[4] == []
    m = whole.m
    for b in range(len(runs)):
        one = sbd.device_batch(td, city, D, runs, only=[b])
        one.run(city["ticks"])
        assert one.logs[0] == whole.logs[b], b
        assert one.m[0] == m[b], b
        sb.assert_same_state(one, 0, whole.state(b), "alone")
        one.close()
    whole.close()


def test_a_table_batch_of_one_and_a_td_sim_table_world(td):
    """D40 as a batch of one and as DeviceSimulator(dist=D), both fed the recorded decisions"""
    city, D, runs = sbd.family("D")
    run = dict(runs)["D40"]
    bat = sbd.device_batch(td, city, D, runs, only=[2])
    one = td.DeviceSimulator(run["rows"], n_cabs=40, drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"], big_cost=BIG, dist=D)
    applied = 0
    for rec in run["ticks"]:
        t = rec["t"]
        ib, io = bat.begin(t), one.begin(t)
        assert tuple(ib[0].tolist()) == io, t
        if io[0]:
            res = rec["res"]
            if res is None:
                ob, oo = bat.apply([None]), one.apply()
            else:
                ob = bat.apply([sb.decisions_of(rec)])
                oo = one.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
                applied += 1
            assert int(ob[0]) == oo, t
        assert bat.m[0] == one.m, t
        sb.assert_same_state(bat, 0, one.state(), ("td_sim", t))
    assert applied > 20
    bat.close()
    one.close()


def test_lockstep_with_the_product_path_family_r(td, monkeypatch):
    city, D, runs = sbd.family("R")
    dev, hosts = sbd.lockstep(td, monkeypatch, city, D, [r["rows"] for _, r in runs], [r["world"]["cabs"] for _, r in runs], city["ticks"])
    assert all(len(h.log) > 0 and h.m["total_pickup_numb"] > 0 for h in hosts)
    assert hosts[2].m["total_LCM_used"] > 0 and hosts[2].m["max_POOL_size"] > 0
    dev.close()


def test_lockstep_with_the_product_path_d40_as_a_batch_of_one(td, monkeypatch):
    city, D, runs = sbd.family("D")
    run = dict(runs)["D40"]
    dev, hosts = sbd.lockstep(td, monkeypatch, city, D, [run["rows"]], [40], city["ticks"])
    assert len(hosts[0].log) > 20 and hosts[0].m["total_LCM_used"] > 0 and hosts[0].m["max_POOL_size"] > 0
    dev.close()


def test_a_line_table_equals_the_line_batch(td):
    """family A of sim_batch_worlds through td_simb_step with dist = line(12) and without: the cells of every model are the
    same numbers, and both batched calls are deterministic functions of one model's cells"""
    city, runs = sb.family("A")
    on_line = sb.device_batch(td, city, runs)
    on_table = sbd.device_batch(td, city, sd.line(city["stands"]), runs)
    on_line.run(city["ticks"])
    on_table.run(city["ticks"])
    assert on_table.logs == on_line.logs and all(len(l) > 0 for l in on_line.logs[:4])
    assert on_table.m == on_line.m
    for b in range(len(runs)):
        sb.assert_same_state(on_table, b, on_line.state(b), "line(12)")
    on_line.close()
    on_table.close()


def test_step_limit_of_2048_requests_before_pooling_on_a_table(td):
    """grid(3, 2): one world with 1 cab and 2049 requests due at tick 0 beside a normal world: step refuses, the states are
    as after begin, and the tick finishes through model / td.tick_batched(..., D) / apply"""
    n = 2049
    D = sd.grid(3, 2)
    # every request starts within the one cab's reach: the cab stands at 0, D[0][0 .. 2] = 0, 1, 2 < drop_time 3
    big = np.stack([np.arange(n), np.arange(n) % 3, np.arange(n) % 3 + 3, np.zeros(n), np.zeros(n)], axis=1).astype(np.int64)
    small = np.array([[7, 0, 1, 0, 0], [9, 3, 4, 2, 2]], np.int64)
    kw = dict(drop_time=3, max_non_lcm=4, big_cost=BIG, dist=D)
    dev, ref = td.DeviceSimulatorBatch([big, small], [1, 2], **kw), td.DeviceSimulatorBatch([big, small], [1, 2], **kw)
    with pytest.raises(td.TdError) as e:
        dev.tick(0)
    assert "error -1" in str(e.value) and "world 0" in str(e.value) and "2049" in str(e.value)
    info = ref.begin(0)
    assert info[0, :3].tolist() == [1, n, 1] and info[1].tolist() == [1, 1, 2, 1] and 1024 < info[0, 3] <= n
    assert dev.m == ref.m
    for b in (0, 1):
        sb.assert_same_state(dev, b, ref.state(b), "as after begin")
    with pytest.raises(td.TdError):
        dev.begin(1)                                            # the refused step left the tick begun
    for world in (dev, ref):
        cab_off, cab_to, dem_off, dem_from = world.model()
        assert cab_off.tolist() == [0, 1, 3] and dem_off.tolist() == [0, int(info[0, 3]), int(info[0, 3]) + 1]
        res = td.tick_batched((cab_to, cab_off), (dem_from, dem_off), D, big_cost=BIG, drop_time=3, max_non_lcm=4)
        world.apply([(r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"]) for r in res])
    assert dev.m == ref.m and dev.m[0]["total_LCM_used"] == 1 and dev.m[0]["max_POOL_size"] >= 1024 and dev.m[1]["total_pickup_numb"] == 1
    for b in (0, 1):
        sb.assert_same_state(dev, b, ref.state(b), "finished through model / apply")
    assert dev.state(0)["c_clnt"][0] >= 0
    assert dev.tick(1) == ref.tick(1)                           # and the handle goes on
    dev.close()
    ref.close()


ONE_WAY = np.array([[0, 1, 9], [9, 0, 9], [9, 9, 0]], np.int32)
PAIR_ROWS = np.array([[0, 1, 2, 0, 0]], np.int64)


def pair_batch(td, D):
    """world 0: one cab (stand 0) and one request 1 -> 2 at t = 0; world 1: the same request and two cabs (stands 0 and 1)"""
    return td.DeviceSimulatorBatch([PAIR_ROWS, PAIR_ROWS], [1, 2], drop_time=3, max_non_lcm=4, big_cost=BIG, dist=D)


def test_one_way_pair_in_a_batch(td):
    """d[0][1] = 1 but d[1][0] = 9, drop_time 3: the cab at stand 0 reaches the request at stand 1"""
    dev = pair_batch(td, ONE_WAY)
    lines = dev.tick(0)
    assert lines[0] == "t:0. Initial Count of demand=1, supply=1. ; OPT count=1"
    assert lines[1].startswith("t:0. Initial Count of demand=1, supply=2. ")        # both cabs are near the request
    st, m = dev.state(0), dev.m[0]
    assert [int(st[k][0]) for k in ("c_from", "c_to", "c_clnt", "c_onboard", "c_start", "d_cab")] == [0, 1, 0, 0, 0, 0]
    assert m["total_pickup_time"] == 1 and m["total_pickup_numb"] == 0
    dev.tick(1)                                        # arrives exactly at t = 1 = d[0][1]: the passenger is picked up
    st = dev.state(0)
    assert [int(st[k][0]) for k in ("c_from", "c_to", "c_onboard", "c_start", "d_pick")] == [1, 2, 1, 1, 1]
    assert dev.m[0]["total_pickup_numb"] == 1
    for t in range(2, 12):                             # the trip takes d[1][2] = 9 ticks
        dev.tick(t)
        st = dev.state(0)
        assert (int(st["c_onboard"][0]), int(st["c_from"][0])) == ((1, 1) if t < 10 else (0, 2)), t
    assert dev.m[0]["total_dropped"] == 0
    dev.close()


def test_one_way_pair_transposed_in_a_batch(td):
    dev = pair_batch(td, ONE_WAY.T.copy())
    for t in range(6):
        lines = dev.tick(t)
        # world 0: no cab is near (d[0][1] = 9): no demand, no line; world 1: only the cab at stand 1 is near
        assert (lines is None or lines[0] is None), t
        if t == 0:
            assert lines[1].startswith("t:0. Initial Count of demand=1, supply=1. ")
        assert dev.m[0]["total_dropped"] == (1 if t >= 3 else 0), t
        st = dev.state(0)
        assert int(st["d_cab"][0]) == (-2 if t >= 3 else -1) and int(st["c_to"][0]) == 0 and int(st["c_clnt"][0]) == -1, t
    dev.close()


# ---- the C-ABI contract of td_simb_create_dist ---------------------------------------------------------------------------
def ws_bytes(lib):
    v = ctypes.c_int64(-1)
    assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
    return v.value


def raw_create(lib, tables, cabs, n_stands, drop_time, max_non_lcm, dist, fn="td_simb_create_dist"):
    from taxidispatcher_amd import _ffi, simulator
    packed = simulator.pack_worlds(tables, cabs)
    h = ctypes.c_void_p()
    args = [len(cabs), _ffi.addr(packed[0]), n_stands, drop_time, max_non_lcm, BIG, _ffi.addr(packed[1])] + [_ffi.addr(c) for c in packed[2:]]
    if fn == "td_simb_create_dist":
        args.append(_ffi.addr(dist))
    rc = getattr(lib, fn)(*args, ctypes.byref(h))
    return rc, h


def raw_run(lib, h, B, ticks, cap):
    lines = []
    for t in range(ticks):
        line = np.zeros(9 * B, np.int32)
        assert lib.td_simb_step(h, t, line.ctypes.data) == 0
        lines.append(line.tolist())
    states = []
    for b in range(B):
        arrs = [np.zeros(cap, np.int32) for _ in range(10)]
        assert lib.td_simb_state(h, b, *[a.ctypes.data for a in arrs]) == 0
        states.append([a.tolist() for a in arrs])
    m = np.zeros(9 * B, np.int64)
    assert lib.td_simb_metrics(h, m.ctypes.data) == 0
    return lines, states, m.tolist()


def test_null_table_is_td_simb_create(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    city, runs = sb.family("A")
    tables, cabs = [runs[b][1]["rows"] for b in (0, 1)], [runs[b][1]["world"]["cabs"] for b in (0, 1)]
    cap = max(max(t.shape[0] for t in tables), max(cabs))
    out = []
    for fn in ("td_simb_create", "td_simb_create_dist"):
        rc, h = raw_create(lib, tables, cabs, city["stands"], city["drop_time"], city["max_non_lcm"], None, fn)
        assert rc == 0 and h.value
        out.append(raw_run(lib, h, 2, 12, cap))
        assert lib.td_simb_destroy(h) == 0
    assert out[0] == out[1] and any(l[0] for l in out[0][0]) and any(l[9] for l in out[0][0])


def test_host_table_device_table_and_the_copy(td):
    """a host table and a device table give the same batch, and the handle keeps its own copy of either"""
    import torch
    city, D, runs = sbd.family("D")
    ref = sbd.device_batch(td, city, D, runs)
    ref.run(12)
    host_t = np.array(D, np.int32)
    dev_t = torch.as_tensor(np.array(D, np.int32), device="cuda")
    for tab in (host_t, dev_t):
        dev = sbd.device_batch(td, city, tab, runs)
        if tab is host_t:
            tab[:] = 1                                 # the caller's table is the caller's again
        else:
            tab.fill_(1)
            torch.cuda.synchronize()
        assert dev.run(12) == ref.logs and all(len(l) > 0 for l in ref.logs[:4])
        assert dev.m == ref.m
        for b in range(len(runs)):
            sb.assert_same_state(dev, b, ref.state(b), "host table" if tab is host_t else "device table")
        dev.close()
    ref.close()


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
    tables, cabs = [PAIR_ROWS, PAIR_ROWS], [1, 2]
    n_stands, D = (4097, sd.line(4097)) if what == "4097 stands" else (5, bad_table(what))
    before = ws_bytes(lib)
    rc, h = raw_create(lib, tables, cabs, n_stands, 3, 4, D)
    assert rc == TD_EINVAL and h.value is None and b"td_simb_create_dist" in lib.td_last_error()
    assert ws_bytes(lib) == before
    if what == "too large":     # the largest entry a table may hold is accepted
        D[0, 4] = 0x1fffffff
        rc, h = raw_create(lib, tables, cabs, n_stands, 3, 4, D)
        assert rc == 0 and h.value and lib.td_simb_destroy(h) == 0 and ws_bytes(lib) == before
    # td_simb_create's own limits stay with a good table
    rc, h = raw_create(lib, tables, [1, 2049], 5, 3, 4, sd.line(5))
    assert rc == TD_EINVAL and h.value is None and b"2049" in lib.td_last_error() and ws_bytes(lib) == before
    with pytest.raises((ValueError, td.TdError)):
        td.DeviceSimulatorBatch(tables, cabs, drop_time=3, max_non_lcm=4, big_cost=BIG, dist=D if what != "too large" else bad_table(what))


def test_a_bad_device_table_is_refused_on_the_device(td):
    """a device tensor is not checked on the host: td_simb_create_dist validates its copy"""
    import torch
    dev_t = torch.as_tensor(bad_table("zero"), device="cuda")
    with pytest.raises(td.TdError, match="zero diagonal"):
        td.DeviceSimulatorBatch([PAIR_ROWS], [1], drop_time=3, max_non_lcm=4, big_cost=BIG, dist=dev_t)


def test_workspace_bytes_count_the_table_and_return_after_destroy(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    city, D, runs = sbd.family("D")
    warm = sbd.device_batch(td, city, D, runs)      # the library's own grow-only buffers reach their size for these worlds
    warm.run(10)
    warm.close()
    before = ws_bytes(lib)
    on_line = sbd.device_batch(td, city, D, runs, dist=False)
    held_line = ws_bytes(lib) - before
    on_line.close()
    assert ws_bytes(lib) == before
    dev = sbd.device_batch(td, city, D, runs)
    held = ws_bytes(lib) - before
    ns, words, B = 65, 3, len(runs)
    assert held - held_line >= 4 * (ns * ns + 2 * ns * words + 2 * words * B)     # the copy, the two bit matrices, the near bitsets
    dev.run(10)
    assert ws_bytes(lib) - before == held                  # a handle does not grow
    dev.close()
    assert ws_bytes(lib) == before


def test_4096_stands_create_and_destroy_with_two_worlds(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    rows = np.array([[0, 4095, 4090, 0, 0]], np.int64)
    before = ws_bytes(lib)
    rc, h = raw_create(lib, [rows, rows], [1, 2], 4096, 10, 600, sd.line(4096))
    assert rc == 0 and h.value
    assert ws_bytes(lib) - before >= 4 * (4096 * 4096 + 2 * 4096 * 128 + 2 * 128 * 2)
    line = np.zeros(18, np.int32)
    assert lib.td_simb_step(h, 0, line.ctypes.data) == 0 and line[0] == 0 and line[9] == 0     # the cabs (stands 0, 1) are far from stand 4095
    assert lib.td_simb_destroy(h) == 0
    assert ws_bytes(lib) == before


def test_enoinit_before_td_init():
    """td_simb_create_dist refuses to run before td_init (a fresh process that never opens the GPU)"""
    from taxidispatcher_amd import _ffi
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
h = ctypes.c_void_p()
a = (ctypes.c_int32 * 32)()
d = (ctypes.c_int32 * 25)()
V, I = ctypes.c_void_p, ctypes.c_int
lib.td_simb_create_dist.argtypes = [I, V, I, I, I, ctypes.c_int32, V, V, V, V, V, V, V]
print(lib.td_simb_create_dist(1, a, 5, 3, 4, 250000, a, None, None, None, None, d, ctypes.byref(h)), h.value)
"""
    out = subprocess.run([sys.executable, "-c", code, _ffi.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "%d None" % TD_ENOINIT, out.stdout


def test_table_batch_line_batch_and_td_sim_table_world_interleaved_stay_independent(td):
    city, D, runs = sbd.family("D")
    w40 = dict(runs)["D40"]
    mk_table = lambda: sbd.device_batch(td, city, D, runs)
    mk_line = lambda: sbd.device_batch(td, city, D, runs, only=[3, 0], dist=False)
    mk_one = lambda: td.DeviceSimulator(w40["rows"], n_cabs=40, drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"], big_cost=BIG, dist=D)
    want, states = [], []
    for mk in (mk_table, mk_line, mk_one):
        dev = mk()
        dev.run(city["ticks"])
        batch = hasattr(dev, "logs")
        want.append((dev.logs if batch else dev.log, dev.m))
        states.append([dev.state(b) for b in range(dev.batch)] if batch else dev.state())
        dev.close()
    a, b, c = mk_table(), mk_line(), mk_one()
    for t in range(city["ticks"]):
        for dev in (a, b):
            lines = dev.tick(t)
            for q, line in enumerate(lines or []):
                if line is not None:
                    dev.logs[q].append(line)
        line = c.tick(t)
        if line is not None:
            c.log.append(line)
    assert (a.logs, a.m) == want[0] and (b.logs, b.m) == want[1] and (c.log, c.m) == want[2]
    for q in range(5):
        sb.assert_same_state(a, q, states[0][q], "a")
    for q in range(2):
        sb.assert_same_state(b, q, states[1][q], "b")
    got = c.state()
    assert all(np.array_equal(got[k], v) for k, v in states[2].items())
    for dev in (a, b, c):
        dev.close()
