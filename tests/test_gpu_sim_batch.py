"""B simulator worlds behind one handle (td_simb_*, simulator.DeviceSimulatorBatch).

1. trace-driven, exact: the CPU runs of two families of worlds give, per world and tick, the lists and the backend's
   decisions; the batch must report every world's info and model and, fed ALL worlds' recorded decisions in one
   td_simb_apply, hold every world's ten state arrays, metrics and log line after every tick;
2. a batch equals its worlds alone (td_simb_step on five worlds against five batches of one);
3. a batch of one in lockstep with the host world model on td_tick_batched's / td_pool2_batched's decisions;
4. the committed input as three worlds (1300, 1300 and 300 cabs);
5. the split tick with every array in device memory;
6. the C-ABI contract of the eight entry points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_worlds as sb
import sim_worlds as sw

GOLD = os.path.join(HERE, "golden")
pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ENOINIT = -1, -3
BIG = sb.BIG_COST


@pytest.mark.parametrize("which", ["A", "W"])
def test_trace_driven_batch_against_the_oracle(td, which):
    city, runs = sb.family(which)
    dev = sb.device_batch(td, city, runs)
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


def test_a_batch_equals_its_worlds_alone(td):
    city, runs = sb.family("A")
    whole = sb.device_batch(td, city, runs)
    whole.run(city["ticks"])
    assert all(len(l) > 0 for l in whole.logs[:4]) and whole.logs[4] == []
    m = whole.m
    for b in range(len(runs)):
        one = sb.device_batch(td, city, runs, only=[b])
        one.run(city["ticks"])
        assert one.logs[0] == whole.logs[b], b
        assert one.m[0] == m[b], b
        sb.assert_same_state(one, 0, whole.state(b), "alone")
        one.close()
    whole.close()


def test_a_batch_of_one_equals_the_host_world_model(td, monkeypatch):
    city, runs = sb.family("A")
    run = dict(runs)["A40"]
    dev, hosts = sb.lockstep(td, monkeypatch, city, [run["rows"]], [40], city["ticks"])
    assert len(hosts[0].log) > 20 and hosts[0].m["total_LCM_used"] > 0 and hosts[0].m["max_POOL_size"] > 0
    dev.close()


def test_committed_input_as_three_worlds(td, monkeypatch):
    """20 ticks of the committed demand file with 1300, 1300 and 300 cabs; equality with the committed log is not asserted
    (it rests on tie-breaking td_tick_batched does not promise to share with td_tick).  With 300 cabs the requests pile up:
    from tick 16 on that world has 2078 .. 2525 requests before pooling, more than td_simb_step and td_pool2_batched take
    (2048), so those ticks go through begin / model / td.tick_batched / apply on the device side and through td_pool2 in the
    host world's find_pool, as the header prescribes; every tick is still compared line by line, and the end states too."""
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(GOLD, "taxi_demand.txt.gz"))
    city = dict(stands=50, drop_time=10, max_non_lcm=600)
    dev, hosts = sb.lockstep(td, monkeypatch, city, [rows, rows, rows], [1300, 1300, 300], 20, hosts_for=[0, 0, 2])
    assert dev.logs[0] == dev.logs[1] and len(dev.logs[0]) == 20
    m = dev.m
    assert m[0] == m[1]
    a, b = dev.state(0), dev.state(1)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for q in (0, 1):
        assert m[q]["max_POOL_size"] > 0 and m[q]["total_LCM_used"] > 0
    assert m[2]["max_POOL_MEM_size"] > 2048 * 2047               # the 300-cab world did pass the limit
    dev.close()


def test_split_tick_with_device_arrays(td):
    """begin -> model -> td.tick_batched -> apply with every array in device memory keeps td_simb_step's log"""
    import torch
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    city, runs = sb.family("A")
    B = len(runs)
    ref = sb.device_batch(td, city, runs)
    ref.run(city["ticks"])
    dev = sb.device_batch(td, city, runs)
    cap_c, cap_r = sum(dev.n_cabs), max(sum(dev.n_req), 1)
    z = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")
    for t in range(city["ticks"]):
        info = dev.begin(t)
        if not info[:, 0].any():
            continue
        cab_off, dem_off, cab_to, dem_from = z(B + 1), z(B + 1), z(cap_c), z(cap_r)
        assert lib.td_simb_model(dev._h, *[_ffi.addr(a) for a in (cab_off, cab_to, dem_off, dem_from)]) == 0
        res = td.tick_batched((cab_to, cab_off), (dem_from, dem_off), None, big_cost=BIG, drop_time=city["drop_time"],
                              max_non_lcm=city["max_non_lcm"])
        rows = torch.as_tensor(np.concatenate([r["lcm_rows"] for r in res]).astype(np.int32), device="cuda")
        cols = torch.as_tensor(np.concatenate([r["lcm_cols"] for r in res]).astype(np.int32), device="cuda")
        r2c = torch.as_tensor(np.concatenate([r["row_to_col"] for r in res]).astype(np.int32), device="cuda")
        p_off = torch.as_tensor(np.cumsum([0] + [len(r["lcm_rows"]) for r in res]).astype(np.int32), device="cuda")
        r_off = torch.as_tensor(np.cumsum([0] + [len(r["row_to_col"]) for r in res]).astype(np.int32), device="cuda")
        solved = torch.as_tensor(np.array([int(r["solved"]) for r in res], np.int32), device="cuda")
        opt = np.zeros(B, np.int32)
        ad = lambda a: _ffi.addr(a) if a.numel() else None
        assert lib.td_simb_apply(dev._h, _ffi.addr(p_off), ad(rows), ad(cols), _ffi.addr(solved), _ffi.addr(r_off), ad(r2c), _ffi.addr(opt)) == 0
        for b in range(B):
            if not info[b, 0]:
                continue
            n_s, n_d = int(info[b, 2]), int(info[b, 3])
            lcm = n_s > 0 and max(n_s, n_d) > city["max_non_lcm"]
            k = len(res[b]["lcm_rows"]) if lcm else 0
            line = [1, info[b, 1], n_s, lcm, k, lcm and res[b]["solved"], n_d - k, n_s - k, opt[b]] if n_s else [1, info[b, 1], 0, 0, 0, 0, 0, 0, 0]
            dev.logs[b].append(dev.format_line(t, line))
    assert dev.logs == ref.logs and dev.m == ref.m
    for b in range(B):
        sb.assert_same_state(dev, b, ref.state(b), "device arrays")
    dev.close()
    ref.close()


# ---- the contract -----------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data


def _two_worlds():
    """world 0: 2 cabs, requests 7 (stand 0, due at 0) and 9 (stand 3, due at 2); world 1: 3 cabs, request 7 (stand 1, due at 0)"""
    return dict(cabs=np.array([2, 3], np.int32), off=np.array([0, 2, 3], np.int32), ids=np.array([7, 9, 7], np.int32),
                frm=np.array([0, 3, 1], np.int32), to=np.array([1, 4, 2], np.int32), at=np.array([0, 2, 0], np.int32))


def _create(lib, h, batch=2, n_stands=5, drop=3, mnl=4, big=BIG, out=True, **over):
    a = dict(_two_worlds(), **over)
    return lib.td_simb_create(batch, _p(a["cabs"]), n_stands, drop, mnl, big, _p(a["off"]), _p(a["ids"]), _p(a["frm"]), _p(a["to"]), _p(a["at"]),
                              ctypes.byref(h) if out else None)


def test_create_arguments(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    h = ctypes.c_void_p()
    i32 = lambda *v: np.array(v, np.int32)
    assert _create(lib, h, out=False) == TD_EINVAL
    bad = [dict(batch=0), dict(batch=-1), dict(n_stands=0), dict(n_stands=(1 << 18) + 1), dict(drop=-1), dict(mnl=-1), dict(mnl=1025), dict(big=-1),
           dict(cabs=None), dict(off=None), dict(ids=None), dict(frm=None), dict(to=None), dict(at=None),
           dict(cabs=i32(0, 3)), dict(cabs=i32(2, 2049)), dict(off=i32(1, 2, 3)), dict(off=i32(0, 2, 1)),
           dict(ids=i32(7, 7, 7)), dict(ids=i32(7, -1, 7)), dict(frm=i32(0, 5, 1)), dict(to=i32(-1, 4, 2)), dict(at=i32(0, -2, 0))]
    for kw in bad:
        assert _create(lib, h, **kw) == TD_EINVAL, kw
        assert h.value is None
    assert _create(lib, h, ids=i32(7, 7, 7)) == TD_EINVAL and b"unique within world 0" in lib.td_last_error()
    assert _create(lib, h, cabs=i32(2, 2049)) == TD_EINVAL and b"2049" in lib.td_last_error()
    assert _create(lib, h, mnl=1024) == 0 and h.value      # the same id in two worlds is fine; so are the limits themselves
    assert lib.td_simb_destroy(h) == 0 and lib.td_simb_destroy(None) == 0
    # a world may have an empty request table, and so may all of them
    assert _create(lib, h, off=i32(0, 0, 1), ids=i32(7), frm=i32(1), to=i32(2), at=i32(0)) == 0 and lib.td_simb_destroy(h) == 0
    assert _create(lib, h, off=i32(0, 0, 0), ids=None, frm=None, to=None, at=None) == 0 and lib.td_simb_destroy(h) == 0


def test_argument_and_sequencing_rules(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    h = ctypes.c_void_p()
    assert _create(lib, h) == 0
    info, line, opt = np.zeros(8, np.int32), np.zeros(18, np.int32), np.full(2, 7, np.int32)
    c_off, d_off, cab, dem = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    z3, z2, met = np.zeros(3, np.int32), np.zeros(2, np.int32), np.zeros(18, np.int64)
    # null handles and outputs
    assert lib.td_simb_begin(None, 0, _p(info)) == TD_EINVAL and lib.td_simb_begin(h, 0, None) == TD_EINVAL and lib.td_simb_begin(h, -1, _p(info)) == TD_EINVAL
    assert lib.td_simb_step(None, 0, _p(line)) == TD_EINVAL and lib.td_simb_step(h, 0, None) == TD_EINVAL and lib.td_simb_step(h, -1, _p(line)) == TD_EINVAL
    assert lib.td_simb_model(None, _p(c_off), _p(cab), _p(d_off), _p(dem)) == TD_EINVAL
    assert lib.td_simb_apply(None, _p(z3), None, None, _p(z2), _p(z3), None, _p(opt)) == TD_EINVAL
    assert lib.td_simb_state(None, 0, *([None] * 10)) == TD_EINVAL
    assert lib.td_simb_state(h, -1, *([None] * 10)) == TD_EINVAL and lib.td_simb_state(h, 2, *([None] * 10)) == TD_EINVAL
    assert b"world 2" in lib.td_last_error()
    assert lib.td_simb_metrics(None, _p(met)) == TD_EINVAL and lib.td_simb_metrics(h, None) == TD_EINVAL
    # model / apply without a begin
    assert lib.td_simb_model(h, _p(c_off), _p(cab), _p(d_off), _p(dem)) == TD_EINVAL
    assert lib.td_simb_apply(h, _p(z3), None, None, _p(z2), _p(z3), None, _p(opt)) == TD_EINVAL
    # t = 0: world 0 has request 7 at stand 0 and cabs at 0, 1; world 1 request 7 at stand 1 and cabs at 0, 1, 2
    assert lib.td_simb_begin(h, 0, _p(info)) == 0 and info.tolist() == [1, 1, 2, 1, 1, 1, 3, 1]
    assert lib.td_simb_begin(h, 0, _p(info)) == TD_EINVAL and lib.td_simb_begin(h, 1, _p(info)) == TD_EINVAL     # waits for its apply
    assert lib.td_simb_step(h, 1, _p(line)) == TD_EINVAL
    for args in ((None, cab, d_off, dem), (c_off, None, d_off, dem), (c_off, cab, None, dem), (c_off, cab, d_off, None)):
        assert lib.td_simb_model(h, *[_p(a) for a in args]) == TD_EINVAL
    assert lib.td_simb_model(h, _p(c_off), _p(cab), _p(d_off), _p(dem)) == 0
    assert c_off.tolist() == [0, 2, 5] and d_off.tolist() == [0, 1, 2] and cab[:5].tolist() == [0, 1, 0, 1, 2] and dem[:2].tolist() == [0, 1]
    r_off, r2c, sol, p_off = np.array([0, 2, 5], np.int32), np.array([0, 1, 1, 0, 2], np.int32), np.ones(2, np.int32), np.zeros(3, np.int32)
    ok = (p_off, None, None, sol, r_off, r2c, opt)
    for q in (0, 3, 4, 5, 6):         # pair_off, solved, r2c_off, row_to_col (needed: r2c_off says 5 entries), opt_count
        args = list(ok)
        args[q] = None
        assert lib.td_simb_apply(h, *[_p(a) for a in args]) == TD_EINVAL, q
    for bad_off in ([1, 2, 5], [0, 3, 2], [0, 2, 9]):          # not from 0, decreasing, a segment longer than its world
        assert lib.td_simb_apply(h, _p(p_off), None, None, _p(sol), _p(np.array(bad_off, np.int32)), _p(r2c), _p(opt)) == TD_EINVAL, bad_off
    assert lib.td_simb_apply(h, _p(np.array([0, 1, 1], np.int32)), None, None, _p(sol), _p(r_off), _p(r2c), _p(opt)) == TD_EINVAL   # pairs, no arrays
    assert lib.td_simb_apply(h, *[_p(a) for a in ok]) == 0 and opt.tolist() == [1, 1]
    assert lib.td_simb_apply(h, *[_p(a) for a in ok]) == TD_EINVAL            # applied already
    assert lib.td_simb_model(h, _p(c_off), _p(cab), _p(d_off), _p(dem)) == TD_EINVAL
    assert lib.td_simb_begin(h, 0, _p(info)) == TD_EINVAL                      # time runs forward
    # any state pointer may be NULL; the client is reported by its id, the cab by its world-local number
    c_clnt, d_cab = np.zeros(3, np.int32), np.zeros(2, np.int32)
    assert lib.td_simb_state(h, 0, None, None, _p(c_clnt), None, None, _p(d_cab), None, None, None, None) == 0
    assert c_clnt[:2].tolist() == [7, -1] and d_cab.tolist() == [0, -1]
    assert lib.td_simb_state(h, 1, None, None, _p(c_clnt), None, None, _p(d_cab), None, None, None, None) == 0
    assert c_clnt.tolist() == [-1, 7, -1] and d_cab[:1].tolist() == [1]
    assert lib.td_simb_state(h, 1, *([None] * 10)) == 0
    assert lib.td_simb_metrics(h, _p(met)) == 0 and met.reshape(2, 9)[:, 2].tolist() == [1, 1]
    # t = 1: nothing is due in any world: the tick is over, nothing to model or apply
    assert lib.td_simb_begin(h, 1, _p(info)) == 0 and info.tolist() == [0] * 8
    assert lib.td_simb_apply(h, *[_p(a) for a in ok]) == TD_EINVAL and lib.td_simb_model(h, _p(c_off), _p(cab), _p(d_off), _p(dem)) == TD_EINVAL
    assert lib.td_simb_begin(h, 1, _p(info)) == TD_EINVAL
    # t = 2: only world 0 has demand; world 1's segments are empty and its solved / opt_count are ignored and 0
    assert lib.td_simb_step(h, 2, _p(line)) == 0
    assert line[0] == 1 and line[9:].tolist() == [0] * 9
    assert lib.td_simb_destroy(h) == 0


def test_a_pair_outside_its_world_applies_nothing_anywhere(td):
    city, runs = sb.family("A")
    t0 = next(t for t in range(city["ticks"]) if len((runs[2][1]["ticks"][t]["res"] or {"lcm_rows": []})["lcm_rows"]) > 0
              and runs[1][1]["ticks"][t]["res"] is not None)
    dev, ref = sb.device_batch(td, city, runs), sb.device_batch(td, city, runs)
    for world in (dev, ref):
        for t in range(t0):
            recs = [run["ticks"][t] for _, run in runs]
            if world.begin(t)[:, 0].any():
                world.apply([sb.decisions_of(rec) if rec["n_dem"] else None for rec in recs])
    recs = [run["ticks"][t0] for _, run in runs]
    info = dev.begin(t0)
    assert np.array_equal(ref.begin(t0), info)
    before = [dev.state(b) for b in range(dev.batch)]
    m_before = dev.m
    good = [sb.decisions_of(rec) if rec["n_dem"] else None for rec in recs]
    # world 2's last pair names the request just behind its own model (a valid position of the packed lists: world 3's)
    bad = list(good)
    cols = np.asarray(good[2][1]).copy()
    cols[-1] = info[2, 3]
    bad[2] = (good[2][0], cols, good[2][2], good[2][3])
    with pytest.raises(td.TdError, match="outside its world"):
        dev.apply(bad)
    assert dev.m == m_before
    for b in range(dev.batch):
        for k, v in dev.state(b).items():
            assert np.array_equal(v, before[b][k]), (b, k)
    assert np.array_equal(dev.apply(good), ref.apply(good))       # the tick still waited for its decisions
    m = dev.m
    for b, rec in enumerate(recs):
        assert m[b] == rec["m"], b
        sb.assert_same_state(dev, b, rec["state"], "after the refused apply")
    dev.close()
    ref.close()


def test_step_limit_of_2048_requests_before_pooling(td):
    """one world with 1 cab and 2049 requests due at tick 0 beside a normal world: step refuses, the states are as after begin,
    and the tick finishes through model / apply"""
    n = 2049
    # every request starts within the one cab's window (stands 0 .. 2 of 5, drop_time 3)
    big = np.stack([np.arange(n), np.arange(n) % 3, np.arange(n) % 3 + 1, np.zeros(n), np.zeros(n)], axis=1).astype(np.int64)
    small = np.array([[7, 0, 1, 0, 0], [9, 3, 4, 2, 2]], np.int64)
    kw = dict(n_stands=5, drop_time=3, max_non_lcm=4, big_cost=BIG)
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
        res = td.tick_batched((cab_to, cab_off), (dem_from, dem_off), None, big_cost=BIG, drop_time=3, max_non_lcm=4)
        opt = world.apply([(r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"]) for r in res])
    assert dev.m == ref.m and dev.m[0]["total_LCM_used"] == 1 and dev.m[0]["max_POOL_size"] >= 1024 and dev.m[1]["total_pickup_numb"] == 1
    for b in (0, 1):
        sb.assert_same_state(dev, b, ref.state(b), "finished through model / apply")
    assert dev.state(0)["c_clnt"][0] >= 0
    assert dev.tick(1) == ref.tick(1)                           # and the handle goes on
    dev.close()
    ref.close()


def test_enoinit_before_td_init():
    """every td_simb entry point refuses to run before td_init (a fresh process that never opens the GPU)"""
    from taxidispatcher_amd import _ffi
    code = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
h = ctypes.c_void_p()
a = (ctypes.c_int32 * 32)()
m = (ctypes.c_int64 * 9)()
V, I = ctypes.c_void_p, ctypes.c_int
lib.td_simb_create.argtypes = [I, V, I, I, I, ctypes.c_int32, V, V, V, V, V, V]
lib.td_simb_begin.argtypes = [V, I, V]
lib.td_simb_step.argtypes = [V, I, V]
lib.td_simb_model.argtypes = [V] * 5
lib.td_simb_apply.argtypes = [V] * 8
lib.td_simb_state.argtypes = [V, I] + [V] * 10
lib.td_simb_metrics.argtypes = [V, V]
lib.td_simb_destroy.argtypes = [V]
fake = ctypes.addressof(a)
rcs = [lib.td_simb_create(1, a, 5, 3, 4, 250000, a, None, None, None, None, ctypes.byref(h)),
       lib.td_simb_begin(fake, 0, a), lib.td_simb_step(fake, 0, a), lib.td_simb_model(fake, a, a, a, a),
       lib.td_simb_apply(fake, a, None, None, a, a, None, a), lib.td_simb_state(fake, 0, *([None] * 10)),
       lib.td_simb_metrics(fake, m), lib.td_simb_destroy(None)]
print(rcs, h.value)
"""
    out = subprocess.run([sys.executable, "-c", code, _ffi.LIB_PATH], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "%r None" % ([TD_ENOINIT] * 7 + [0]), out.stdout


def test_workspace_bytes_return_after_destroy(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    city, runs = sb.family("A")

    def ws():
        v = ctypes.c_int64(-1)
        assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
        return v.value
    warm = sb.device_batch(td, city, runs)      # the library's own grow-only buffers reach their size for these worlds
    warm.run(10)
    warm.close()
    before = ws()
    dev = sb.device_batch(td, city, runs)
    held = ws() - before
    assert held >= 4 * (14 * sum(dev.n_req) + 5 * sum(dev.n_cabs))     # at least the two tables
    dev.run(10)
    assert ws() - before == held                  # a handle does not grow
    dev.close()
    assert ws() == before


def test_two_batches_and_one_world_interleaved_stay_independent(td):
    city, runs = sb.family("A")
    w40 = dict(runs)["A40"]
    mk_one = lambda: td.DeviceSimulator(w40["rows"], n_cabs=40, n_stands=city["stands"], drop_time=city["drop_time"],
                                        max_non_lcm=city["max_non_lcm"], big_cost=BIG)
    alone_a, alone_b, alone_c = sb.device_batch(td, city, runs), sb.device_batch(td, city, runs, only=[3, 0]), mk_one()
    want = []
    for dev in (alone_a, alone_b, alone_c):
        dev.run(city["ticks"])
        want.append((dev.logs if hasattr(dev, "logs") else dev.log, dev.m))
    states = [[alone_a.state(b) for b in range(5)], [alone_b.state(b) for b in range(2)], alone_c.state()]
    for dev in (alone_a, alone_b, alone_c):
        dev.close()
    a, b, c = sb.device_batch(td, city, runs), sb.device_batch(td, city, runs, only=[3, 0]), mk_one()
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
