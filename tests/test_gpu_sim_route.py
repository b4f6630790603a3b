"""The route model in a device world: td_sim_route / td_sim_route_state / td_sim_route_metrics, DeviceSimulator(route=True).

1. the hand-made worlds of sim_route_worlds on the device: state and route state equal to the specification after every tick,
   and the pick-up and drop-off ticks the ones written out by hand;
2. family A7 and A40, and a world on an asymmetric table, three ways (td_sim_step; begin -> model -> td_tick -> apply; the host
   Simulator on HipBackend), equal in state, route state, metrics and route metrics after every tick (the three ways share the
   library's solver; the oracle's may break a tie between equal optima differently, so the oracle-backed runs of
   test_sim_route_cpu.py are not the comparator here);
3. a 513-request tick (td_pool_n underneath) and a banded world (td_sim_pool_buffer);
4. the life cycle: every refusal, on = 0 with cabs mid-route, the workspace bytes;
5. handles without routes: byte for byte the states recorded from the commit before the route model (tests/golden/sim_route)."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_worlds as sbw
import sim_dist_worlds as sdw
import sim_pool_n_worlds as W
import sim_route_worlds as R
import sim_worlds as sw

pytestmark = pytest.mark.gpu

TD_EINVAL = -1
CITY = sbw.CITY_A
BIG = sw.BIG_COST
WAIT, LOSS = 1, 50
GOLDEN = os.path.join(HERE, "golden", "sim_route", "parent_states.npz")


def lib_of():
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def err():
    return lib_of().td_last_error().decode()


def ws():
    v = ctypes.c_int64(-1)
    assert lib_of().td_workspace_bytes(ctypes.byref(v)) == 0
    return v.value


@pytest.fixture(scope="module")
def worlds():
    city, runs = sbw.family("A")
    return {name: run for name, run in runs}


def device_world(td, rows, cabs, city, pn, wait=WAIT, loss=LOSS, route=True, **kw):
    return td.DeviceSimulator(rows, n_cabs=cabs, n_stands=city["stands"], drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"],
                              big_cost=BIG, pool_n=pn, pool_wait=wait, pool_loss=loss, route=route, **kw)


def assert_same(dev, rec, where):
    assert dev.m == rec["m"], where
    got = dev.state()
    for k, v in rec["state"].items():
        assert np.array_equal(got[k], v), (where, k, np.nonzero(got[k] != v)[0][:8].tolist())
    if "route" in rec:
        got = dev.route_state()
        for k, v in rec["route"].items():
            assert np.array_equal(got[k], v), (where, k, np.nonzero(got[k] != v)[0][:8].tolist())
        assert dev.route_metrics() == rec["route_m"], where


def split_tick(td, dev, city, t, dist=None):
    """begin -> model -> the library's own tick call -> apply; -> the line"""
    info = dev.begin(t)
    if not info[0]:
        return None
    if info[2] == 0:
        return dev.format_line(t, [1, info[1], 0, 0, 0, 0, 0, 0, dev.apply()])
    cab_to, dem_from = dev.model()
    res = td.tick(cab_to, dem_from, dist, big_cost=BIG, drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"])
    opt = dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
    lcm = max(info[2], info[3]) > city["max_non_lcm"]
    return dev.format_line(t, [1, info[1], info[2], lcm, len(res["lcm_rows"]), lcm and res["solved"], len(res["kept_dems"]), len(res["kept_cabs"]), opt])


def three_ways(td, rows, cabs, city, ticks, pn, wait, loss, dist=None, **kw):
    """the host Simulator on HipBackend (recorded, invariants checked every tick), a td_sim_step world and a split-tick world;
    -> the specification's run"""
    from taxidispatcher_amd import simulator
    be = simulator.HipBackend(dist=dist, pool_buffer=kw.get("pool_buffer", 0))
    run = R.spec_run(rows, cabs, city, ticks, pn, wait, loss, backend=be, dist=dist)
    step, split = (device_world(td, rows, cabs, city, pn, wait, loss, dist=dist, **kw) for _ in range(2))
    for rec in run["ticks"]:
        t = rec["t"]
        assert step.tick(t) == rec["line"], t
        assert_same(step, rec, ("step", t))
        assert split_tick(td, split, city, t, dist) == rec["line"], t
        assert_same(split, rec, ("split", t))
    step.close(), split.close()
    return run


# ---- 0. the surface (these fail on a library without the route model) ---------------------------------------------------------
def test_the_symbols_are_exported_and_null_handles_refused(td):
    lib = lib_of()
    out = np.zeros(4, np.int64)
    assert lib.td_sim_route(None, 1) == TD_EINVAL and "null handle" in err()
    assert lib.td_sim_route_state(None, None, None, None) == TD_EINVAL
    assert lib.td_sim_route_metrics(None, out.ctypes.data) == TD_EINVAL


# ---- 1. the hand-made worlds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.HAND))
def test_a_hand_made_world(td, name):
    from taxidispatcher_amd import simulator
    w = R.HAND[name]
    D = w.get("dist")
    run = R.hand_run(name, backend=simulator.HipBackend(dist=D))
    dev = device_world(td, w["rows"], w["cabs"], w, w["pool_n"], w["wait"], w["loss"], dist=D)
    for rec in run["ticks"]:
        assert dev.tick(rec["t"]) == rec["line"], rec["t"]
        assert_same(dev, rec, (name, rec["t"]))
    assert dev.state()["d_pick"].tolist() == w["d_pick"] and dev.route_state()["d_drop"].tolist() == w["d_drop"]
    st, c = dev.state(), w["cab"]
    assert (st["c_from"][c], st["c_to"][c], st["c_clnt"][c], st["c_onboard"][c], st["c_start"][c]) == (w["free_at"], w["free_at"], -1, 0, -1)
    assert dev.route_state()["c_pos"][c] == 2 * len(w["d_pick"]) and dev.route_metrics()["drop_numb"] == len(w["d_pick"])
    dev.close()


# ---- 2. three ways -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", [(4, 2), (3, 3)])
@pytest.mark.parametrize("name", ["A7", "A40"])
def test_a_fleet_three_ways(td, worlds, name, pn):
    run = three_ways(td, worlds[name]["rows"], worlds[name]["world"]["cabs"], CITY, CITY["ticks"], pn, WAIT, LOSS)
    tr = run["sim"].route_trace
    assert sum(tr["dispatches"].values()) > 0 and tr["zero_pick"] + tr["zero_drop"] > 0 and run["sim"].route_m["drop_numb"] > 0
    if name == "A40":      # both paths hand out routes, standing and heading
        assert {m for m, _ in tr["dispatches"]} == {1, 2} and {h for _, h in tr["dispatches"]} == {"standing", "heading"}


def test_a_world_on_an_asymmetric_table_three_ways(td):
    """ring12: the way from a to b is (b - a) mod 12, one-way"""
    D, w = sdw.table("ring12"), sdw.world("ring12")
    rows = sdw.gen_demand(D, **{k: w[k] for k in ("per_tick", "ticks", "span", "max_wait", "seed")})
    run = three_ways(td, rows, w["cabs"], w, 20, (4, 2), 2, 100, dist=D)
    # on a one-way ring every ride is the direct way: a detour would go round the ring
    assert run["sim"].route_m["drop_numb"] > 0 and run["sim"].route_m["ride_time"] == run["sim"].route_m["solo_time"] > 0


# ---- 3. the pool calls underneath ------------------------------------------------------------------------------------------------
def test_a_tick_of_513_requests(td):
    """td_pool_n underneath (more than td_pool_n_batched's 512): pools of two that start at one stand, rides no longer than alone"""
    from taxidispatcher_amd import simulator
    rows = W.one_tick_world(513)
    run = R.spec_run(rows, W.WIDE["stands"], W.WIDE, 6, (2, 2), 0, 0, backend=simulator.HipBackend())
    dev = device_world(td, rows, W.WIDE["stands"], W.WIDE, (2, 2), 0, 0)
    for rec in run["ticks"]:
        assert dev.tick(rec["t"]) == rec["line"], rec["t"]
        assert_same(dev, rec, rec["t"])
    assert run["ticks"][0]["line"].startswith("t:0. Initial Count of demand=513") and run["sim"].route_m["drop_numb"] > 0
    dev.close()


def test_a_banded_world(td, worlds):
    run = three_ways(td, worlds["A40"]["rows"], 40, CITY, 16, (4, 2), WAIT, LOSS, pool_buffer=24 * 2047)
    assert run["sim"].route_m["drop_numb"] > 0


# ---- 4. the life cycle -------------------------------------------------------------------------------------------------------------
def test_refusals(td, worlds):
    lib = lib_of()
    rows = worlds["A7"]["rows"]
    kw = dict(n_cabs=7, n_stands=CITY["stands"], drop_time=CITY["drop_time"], max_non_lcm=CITY["max_non_lcm"], big_cost=BIG)
    out, buf = np.zeros(4, np.int64), np.zeros(8 * 7, np.int32)
    pair = td.DeviceSimulator(rows, **kw)
    assert lib.td_sim_route(pair._h, 1) == TD_EINVAL and "td_sim_pooling_n" in err()      # no pool_n policy
    assert lib.td_sim_route(pair._h, 0) == 0                                              # nothing to switch off is no error
    assert lib.td_sim_route_state(pair._h, None, None, buf.ctypes.data) == TD_EINVAL and "no routes" in err()
    assert lib.td_sim_route_metrics(pair._h, out.ctypes.data) == TD_EINVAL and "no routes" in err()
    pair.close()
    logs = td.DeviceSimulator(rows, events=True, pool_n=2, **kw)
    assert lib.td_sim_route(logs._h, 1) == TD_EINVAL and "not built" in err()             # a handle that logs
    logs.close()
    dev = td.DeviceSimulator(rows, pool_n=(3, 2), pool_wait=WAIT, pool_loss=LOSS, route=True, **kw)
    assert lib.td_sim_log(dev._h, 0xffe, 4096) == TD_EINVAL and "not built" in err()      # the log of a routed handle
    assert lib.td_sim_log(dev._h, 0, 0) == 0                                              # an empty mask is no log
    assert lib.td_sim_pooling(dev._h, 1, 0.0) == TD_EINVAL and "td_sim_route" in err()    # back to pairs while routes are on
    assert lib.td_sim_route_metrics(dev._h, None) == TD_EINVAL
    t = next(t for t in range(CITY["ticks"]) if dev.begin(t)[0])
    assert lib.td_sim_route(dev._h, 0) == TD_EINVAL and "waits for td_sim_apply" in err()  # only between ticks
    assert lib.td_sim_route(dev._h, 1) == TD_EINVAL and "waits for td_sim_apply" in err()
    dev.apply()
    assert lib.td_sim_route(dev._h, 0) == 0 and lib.td_sim_pooling(dev._h, 1, 0.0) == 0   # off: pairs are allowed again
    assert lib.td_sim_route(dev._h, 1) == TD_EINVAL                                       # and routes refused on the pair policy
    assert lib.td_sim_log(dev._h, 0xffe, 4096) == TD_EINVAL and "not built" in err()      # the handle keeps its route storage
    # null destinations are skipped
    assert lib.td_sim_route_state(dev._h, None, None, None) == 0 and lib.td_sim_route_state(dev._h, None, None, buf.ctypes.data) == 0
    dev.close()


def test_off_lets_the_cabs_mid_route_finish(td, worlds, monkeypatch):
    """routes are switched off at tick 8 and on again at tick 16, on the device and in the specification: the two stay equal
    tick by tick; the cabs that are mid-route at tick 8 drop their members off, and no list is handed out while routes are off"""
    from taxidispatcher_amd import simulator
    sw.patch_constants(monkeypatch, CITY)
    rows = worlds["A40"]["rows"]
    host = R.traced_simulator()(rows, simulator.HipBackend(), n_cabs=40, pool_n=(4, 2), pool_wait=WAIT, pool_loss=LOSS, route=True)
    dev = device_world(td, rows, 40, CITY, (4, 2))
    given, drops, mid = [], [], 0
    for t in range(24):
        if t == 8:
            mid = sum(bool(host._has_stops(c)) for c in range(40))
        if t in (8, 16):
            dev.set_route(t == 16)
            host.set_route(t == 16)
        assert dev.tick(t) == host.tick(t), t
        R.check_invariants(host, t)
        assert_same(dev, dict(m=host.m, state=sw.state_of(host), route=R.route_state_of(host), route_m=host.route_m), t)
        given.append(sum(host.route_trace["dispatches"].values()))
        drops.append(host.route_m["drop_numb"])
    assert given[7] > 0 and given[15] == given[7] and given[23] > given[15] and mid > 0
    assert drops[15] > drops[7]      # members dropped off while routes were off: the cabs mid-route finished their lists
    dev.close()


def test_workspace_bytes_count_the_route_storage(td, worlds):
    rows = worlds["A40"]["rows"]
    base = ws()
    dev = device_world(td, rows, 40, CITY, (3, 2), route=False)
    plain = ws()
    dev.set_route(True)
    grown = ws() - plain
    # 8 stop words and a position per cab, the drop-off tick per request, a record column per list, four 64-bit counters
    assert grown >= 4 * (9 * 40 + rows.shape[0] + 2 * max(40, rows.shape[0])) + 32
    dev.set_route(False)
    dev.set_route(True)
    assert ws() - plain == grown      # allocated once
    dev.close()
    assert ws() == base


# ---- 5. handles without routes ----------------------------------------------------------------------------------------------------
def golden_states(td, worlds):
    """A40 for 30 ticks through td_sim_step on a default handle and on a (3, 2) handle without routes: per tick the CRC of the ten
    state arrays and the nine metrics, and the final state arrays (the file was written with this function on the library of the commit before)"""
    rows = worlds["A40"]["rows"]
    kw = dict(n_cabs=40, n_stands=CITY["stands"], drop_time=CITY["drop_time"], max_non_lcm=CITY["max_non_lcm"], big_cost=BIG)
    out = {}
    for tag, more in (("default", {}), ("pool32", dict(pool_n=(3, 2), pool_wait=WAIT, pool_loss=LOSS))):
        dev = td.DeviceSimulator(rows, **kw, **more)
        crc, lines = [], []
        for t in range(CITY["ticks"]):
            lines.append(dev.tick(t) or "")
            st = dev.state()
            c = 0
            for k in dev.CAB_KEYS + dev.REQ_KEYS:
                c = zlib.crc32(np.ascontiguousarray(st[k], np.int32).tobytes(), c)
            m = dev.m
            crc.append(zlib.crc32(np.asarray([m[k] for k in dev.M_KEYS], np.int64).tobytes(), c))
        out[tag + "_crc"] = np.asarray(crc, np.int64)
        out[tag + "_lines"] = np.asarray(lines)
        for k, v in dev.state().items():
            out[tag + "_" + k] = np.asarray(v, np.int32)
        dev.close()
    return out


def test_handles_without_routes_compute_what_they_computed_before(td, worlds):
    want = np.load(GOLDEN)
    got = golden_states(td, worlds)
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k
