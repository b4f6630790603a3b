"""Pools of up to four in a device world: td_sim_pooling_n / td_sim_pools_n, DeviceSimulator(pool_n=, pool_wait=, pool_loss=).

1. a world under the policy three ways (td_sim_step; begin -> model -> td_tick -> apply; the host Simulator on HipBackend),
   equal in state, metrics and line after every tick, the plans of every tick equal to the cascade restated on oracle.pool_n
   (the three ways share the library's solver; the oracle's solver may break a tie between equal optima differently, so the
   oracle-backed run of test_sim_pool_n_cpu.py is not the comparator of the states here);
3. the path boundaries of the single world: 512 / 513 requests in a tick (td_pool_n_batched's device code / td_pool_n), 2047
   accepted, 2048 refused;
4. max_happy: TD_ERANGE from begin, the handle as the header leaves it;
5. the life cycle of the two entry points, the log with pools of two, its refusal with pools of three;
6. a world on an asymmetric distance table.
2., the batch, and the batched halves of 3., 5. and 6. are in test_gpu_simb_pool_n.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_worlds as sbw
import sim_dist_worlds as sdw
import sim_pool_n_worlds as W
import sim_worlds as sw

pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ERANGE = -1, -4
CITY = sbw.CITY_A
NAMES = ("A1", "A7", "A40", "A90")
BIG = sw.BIG_COST


def lib_of():
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def err():
    return lib_of().td_last_error().decode()


def test_null_handles_are_refused(td):
    n = ctypes.c_int32(0)
    assert lib_of().td_sim_pooling_n(None, 2, 2, 0, 0, 0) == TD_EINVAL and "null handle" in err()
    assert lib_of().td_sim_pools_n(None, 0, None, None, ctypes.byref(n)) == TD_EINVAL


@pytest.fixture(scope="module")
def worlds():
    city, runs = sbw.family("A")
    return {name: run for name, run in runs}


_SPEC = {}


def spec(worlds, name, pn, **kw):
    """the recorded run of the host specification on HipBackend, a fleet under a size pair, computed once; every tick's plans
    are checked against the cascade restated on oracle.pool_n, with the invariants (check_tick)"""
    from taxidispatcher_amd import simulator
    key = (name, pn, tuple(sorted(kw)))
    if key not in _SPEC:
        _SPEC[key] = W.spec_run(worlds[name]["rows"], worlds[name]["world"]["cabs"], CITY, CITY["ticks"], pn, backend=simulator.HipBackend(), **kw)
        for rec in _SPEC[key]["ticks"]:
            W.check_tick(rec, pn)
    return _SPEC[key]


def device_world(td, rows, cabs, city, pn, wait=W.WAIT, loss=W.LOSS, **kw):
    return td.DeviceSimulator(rows, n_cabs=cabs, n_stands=city["stands"], drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"],
                              big_cost=BIG, pool_n=pn, pool_wait=wait, pool_loss=loss, **kw)


def assert_same(dev, rec, where):
    assert dev.m == rec["m"], where
    got = dev.state()
    for k, v in rec["state"].items():
        assert np.array_equal(got[k], v), (where, k, np.nonzero(got[k] != v)[0][:8].tolist())


def split_tick(td, dev, city, t, dist=None):
    """begin -> model -> the library's own tick call -> apply; -> (the line, pools_n() of the tick)"""
    info = dev.begin(t)
    if not info[0]:
        return None, []
    plans = dev.pools_n()
    if info[2] == 0:
        opt = dev.apply()
        return dev.format_line(t, [1, info[1], 0, 0, 0, 0, 0, 0, opt]), plans
    cab_to, dem_from = dev.model()
    res = td.tick(cab_to, dem_from, dist, big_cost=BIG, drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"])
    opt = dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
    lcm = max(info[2], info[3]) > city["max_non_lcm"]
    return dev.format_line(t, [1, info[1], info[2], lcm, len(res["lcm_rows"]), lcm and res["solved"], len(res["kept_dems"]),
                               len(res["kept_cabs"]), opt]), plans


# ---- 1. a world under the policy, three ways ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pn", W.SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_a_world_three_ways(td, worlds, name, pn):
    run = spec(worlds, name, pn)
    rows, cabs = worlds[name]["rows"], worlds[name]["world"]["cabs"]
    step, split = device_world(td, rows, cabs, CITY, pn), device_world(td, rows, cabs, CITY, pn)
    for rec in run["ticks"]:
        t, want = rec["t"], rec["plans"]
        assert step.tick(t) == rec["line"], t
        assert step.pools_n() == want, t
        assert_same(step, rec, ("step", name, pn, t))
        line, plans = split_tick(td, split, CITY, t)
        assert line == rec["line"] and plans == want, t
        assert_same(split, rec, ("split", name, pn, t))
    step.close(), split.close()


def test_the_runs_above_reach_both_paths_with_every_size(td, worlds):
    """what test_sim_pool_n_cpu.py asserts of the oracle-backed runs holds for the runs on the library's solver too: pools of
    three and of four are dispatched on the LCM path and on the OPT path, some find no cab, some stage lists are too short"""
    tot = dict(lcm=set(), opt=set(), lost=0, no_supply=0)
    for name in NAMES:
        for pn in W.SIZES:
            for rec in spec(worlds, name, pn)["ticks"]:
                sizes = {len(p[0]) for p in rec["plans"]}
                if rec["lcm_pools"] == len(rec["plans"]) > 0:
                    tot["lcm"] |= sizes
                if rec["opt_pools"] == len(rec["plans"]) > 0:
                    tot["opt"] |= sizes
                tot["lost"] += rec["lost_pools"]
                tot["no_supply"] += rec["line"] is not None and "supply=0." in rec["line"]
    assert tot["lcm"] == {2, 3, 4} and tot["opt"] == {2, 3, 4} and tot["lost"] > 0 and tot["no_supply"] > 0, tot


# ---- 3. the path boundaries of the single world ------------------------------------------------------------------------------------
WIDE, one_tick_world = W.WIDE, W.one_tick_world


@pytest.mark.parametrize("n", [512, 513])
def test_512_and_513_requests_in_a_tick(td, n):
    """512: td_pool_n_batched's device code on the one model; 513: td_pool_n.  Pools of two whose second pick-up stands where
    the first does (wait 0) and whose rides are no longer than alone (loss 0): far fewer happy plans than the default max_happy"""
    rows = one_tick_world(n)
    dev = device_world(td, rows, WIDE["stands"], WIDE, (2, 2), wait=0, loss=0)
    info = dev.begin(0)
    want, happy, _ = W.cascade(2, 2, rows[:, 1], rows[:, 2], 0, 0)
    assert info[:3] == (1, n, WIDE["stands"]) and 0 < happy < 65536 and len(want) > 50
    assert dev.pools_n() == want
    assert info[3] == n - len(want) and dev.m["max_POOL_MEM_size"] == happy and dev.m["max_POOL_size"] == len(want)
    dev.close()


def test_2047_requests_are_accepted_and_2048_refused(td):
    rows = one_tick_world(2048)
    dev = device_world(td, rows[:2047], WIDE["stands"], WIDE, (2, 2), wait=0, loss=0)
    info = dev.begin(0)
    want, happy, _ = W.cascade(2, 2, rows[:2047, 1], rows[:2047, 2], 0, 0)
    assert info[1] == 2047 and dev.pools_n() == want and dev.m["max_POOL_MEM_size"] == happy
    dev.close()
    dev = device_world(td, rows, WIDE["stands"], WIDE, (2, 2), wait=0, loss=0)
    info = np.zeros(4, np.int32)
    assert lib_of().td_sim_begin(dev._h, 0, info.ctypes.data) == TD_EINVAL and "2048 requests" in err()
    dev.close()


# ---- 4. max_happy ------------------------------------------------------------------------------------------------------------------
def test_max_happy_is_refused_by_begin_with_the_count(td):
    rng = np.random.default_rng(9)
    n = 40
    frm = rng.integers(0, 9, n)
    rows = np.stack([np.arange(n), frm, frm + rng.integers(1, 4, n), np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1).astype(np.int64)
    city = dict(stands=12, drop_time=4, max_non_lcm=16)
    want, happy, _ = W.cascade(4, 4, rows[:, 1], rows[:, 2], 0, 50)
    assert happy > 1000 and want
    lib = lib_of()
    tight = device_world(td, rows, 12, city, (4, 4), wait=0, loss=50, max_happy=happy - 1)
    info = np.zeros(4, np.int32)
    assert lib.td_sim_begin(tight._h, 0, info.ctypes.data) == TD_ERANGE and str(happy) in err()
    # the handle as a failing pool call inside begin leaves it: the tick counts as begun and cannot be completed
    assert lib.td_sim_begin(tight._h, 1, info.ctypes.data) == TD_EINVAL and "still waits for td_sim_apply" in err()
    assert lib.td_sim_pooling_n(tight._h, 4, 4, 0, 50, 0) == TD_EINVAL and "still waits" in err()
    tight.close()
    for room in (happy, 0):
        dev = device_world(td, rows, 12, city, (4, 4), wait=0, loss=50, max_happy=room)
        assert dev.begin(0)[1] == n and dev.pools_n() == want and dev.m["max_POOL_MEM_size"] == happy
        dev.close()


# ---- 5. the life cycle -------------------------------------------------------------------------------------------------------------
def first_tick_with(run, what):
    return next(rec for rec in run["ticks"] if what(rec))


def test_refusals_leave_the_policy_unchanged(td, worlds):
    lib = lib_of()
    run = spec(worlds, "A40", (3, 2))
    rows = worlds["A40"]["rows"]
    dev = device_world(td, rows, 40, CITY, (3, 2))
    assert dev.pool_n == (3, 2)
    for args, word in (((1, 1, 0, 0, 0), "k_lo"), ((5, 2, 0, 0, 0), "k_hi"), ((2, 3, 0, 0, 0), "k_lo"), ((4, 1, 0, 0, 0), "k_lo"),
                       ((3, 2, -1, 0, 0), "negative"), ((3, 2, 0, -1, 0), "negative"), ((3, 2, 0, 0, (1 << 22) + 1), "max_happy")):
        assert lib.td_sim_pooling_n(dev._h, *args) == TD_EINVAL and word in err(), args
    assert lib.td_sim_pooling_n(dev._h, 3, 2, W.WAIT, W.LOSS, 1 << 22) == 0      # the limit itself is taken
    assert lib.td_sim_pooling_n(dev._h, 3, 2, W.WAIT, W.LOSS, 0) == 0
    rec = first_tick_with(run, lambda r: len(r["plans"]) >= 2)
    for r in run["ticks"][:rec["t"]]:
        assert dev.tick(r["t"]) == r["line"]
    info = dev.begin(rec["t"])
    assert info[0] == 1 and lib.td_sim_pooling_n(dev._h, 4, 4, 0, 0, 0) == TD_EINVAL and "waits for td_sim_apply" in err()
    assert lib.td_sim_pooling(dev._h, 1, 0.0) == TD_EINVAL
    assert dev.pools_n() == rec["plans"]      # every refusal left (3, 2) under the rule in force
    # pools_n with too little room: *n is set, nothing is copied; td_sim_pools on this world names td_sim_pools_n
    recs, size, n = np.full((len(rec["plans"]), 9), -7, np.int32), np.full(len(rec["plans"]), -7, np.int32), ctypes.c_int32(0)
    assert lib.td_sim_pools_n(dev._h, len(rec["plans"]) - 1, recs.ctypes.data, size.ctypes.data, ctypes.byref(n)) == TD_EINVAL
    assert n.value == len(rec["plans"]) and (recs == -7).all() and (size == -7).all()
    a = np.zeros(64, np.int32)
    assert lib.td_sim_pools(dev._h, 64, a.ctypes.data, a.ctypes.data, a.ctypes.data, a.ctypes.data, ctypes.byref(n)) == TD_EINVAL
    assert "td_sim_pools_n" in err()
    assert lib.td_sim_pools_n(dev._h, len(rec["plans"]), recs.ctypes.data, size.ctypes.data, ctypes.byref(n)) == 0
    assert size.tolist() == [len(p[0]) for p in rec["plans"]]
    for r, (picks, drops, cost) in zip(recs.tolist(), rec["plans"]):
        k = len(picks)
        assert r[:k] == list(picks) and r[4:4 + k] == list(drops) and r[8] == cost and set(r[k:4] + r[4 + k:8]) <= {-1}
    dev.close()
    pair = td.DeviceSimulator(rows, n_cabs=40, n_stands=CITY["stands"], drop_time=CITY["drop_time"], max_non_lcm=CITY["max_non_lcm"], big_cost=BIG)
    assert lib.td_sim_pools_n(pair._h, 64, recs.ctypes.data, size.ctypes.data, ctypes.byref(n)) == TD_EINVAL and "td_sim_pools" in err()
    pair.close()


def test_a_switch_to_pairs_and_back_takes_effect_at_the_next_begin(td, worlds, monkeypatch):
    """the world pools up to four, then pairs (td_sim_pooling), then up to four again; the host specification switches its
    policy at the same ticks, and the two stay equal line by line: each policy holds from the begin after its call"""
    from taxidispatcher_amd import simulator
    sw.patch_constants(monkeypatch, CITY)
    rows = worlds["A40"]["rows"]
    host = simulator.Simulator(rows, simulator.HipBackend(), n_cabs=40, pool_n=(4, 2), pool_wait=W.WAIT, pool_loss=W.LOSS)
    dev = device_world(td, rows, 40, CITY, (4, 2))
    seconds = []
    for t in range(14):
        if t == 4:
            dev.set_pool_n(None)
            host.pool_n = None
        if t == 9:
            dev.set_pool_n((4, 2), W.WAIT, W.LOSS)
            host.pool_n = (4, 2)
        assert dev.tick(t) == host.tick(t), t
        assert dev.m == host.m, t
        got = dev.state()
        for k, v in sw.state_of(host).items():
            assert np.array_equal(got[k], v), (t, k)
        seconds.append(host.m["total_second_passengers"])
        with pytest.raises(td.TdError):
            dev.pools() if dev.pool_n is not None else dev.pools_n()
    assert seconds[3] > 0 and seconds[8] > seconds[3] and seconds[13] > seconds[8]      # each policy pooled somebody
    dev.close()


def test_the_log_is_refused_with_pools_of_three_both_ways_round(td, worlds):
    lib = lib_of()
    rows = worlds["A7"]["rows"]
    dev = device_world(td, rows, 7, CITY, (3, 2))
    assert lib.td_sim_log(dev._h, 0xffe, 4096) == TD_EINVAL and "not built" in err()
    assert lib.td_sim_log(dev._h, 0, 0) == 0      # an empty mask is no log
    dev.close()
    dev = td.DeviceSimulator(rows, n_cabs=7, n_stands=CITY["stands"], drop_time=CITY["drop_time"], max_non_lcm=CITY["max_non_lcm"], big_cost=BIG,
                             events=True)
    assert lib.td_sim_pooling_n(dev._h, 3, 2, W.WAIT, W.LOSS, 0) == TD_EINVAL and "not built" in err()
    assert lib.td_sim_pooling_n(dev._h, 2, 2, W.WAIT, W.LOSS, 0) == 0
    dev.close()


@pytest.mark.parametrize("name", ["A7", "A40"])
def test_the_log_with_pools_of_two_equals_the_specifications(td, worlds, name):
    rows, cabs = worlds[name]["rows"], worlds[name]["world"]["cabs"]
    run = spec(worlds, name, (2, 2), events=True)
    dev = device_world(td, rows, cabs, CITY, (2, 2), events=True)
    got = []
    for rec in run["ticks"]:
        assert dev.tick(rec["t"]) == rec["line"]
        got += dev.events().tolist()
    assert dev.events_lost == 0
    assert [tuple(r) for r in got] == [tuple(int(v) for v in r) for r in run["events"]]
    assert sum(r[2] == 11 for r in got) == run["m"]["total_second_passengers"] > 0
    dev.close()


# ---- 6. a distance-table world -------------------------------------------------------------------------------------------------------
def test_a_world_on_an_asymmetric_table(td):
    """ring12: the way from a to b is (b - a) mod 12, one-way.  (4, 2) with a pick-up path of up to 2 and rides up to twice as long"""
    D, w = sdw.table("ring12"), sdw.world("ring12")
    assert not np.array_equal(D, D.T)
    rows = sdw.gen_demand(D, **{k: w[k] for k in ("per_tick", "ticks", "span", "max_wait", "seed")})
    ticks, wait, loss = 20, 2, 100
    from taxidispatcher_amd import simulator
    run = W.spec_run(rows, w["cabs"], w, ticks, (4, 2), wait, loss, backend=simulator.HipBackend(dist=D), dist=D)
    sizes = set()
    step = device_world(td, rows, w["cabs"], w, (4, 2), wait, loss, dist=D)
    split = device_world(td, rows, w["cabs"], w, (4, 2), wait, loss, dist=D)
    for rec in run["ticks"]:
        W.check_tick(rec, (4, 2), wait, loss, D)
        sizes |= {len(p[0]) for p in rec["plans"]}
        assert step.tick(rec["t"]) == rec["line"] and step.pools_n() == rec["plans"], rec["t"]
        assert_same(step, rec, ("step", rec["t"]))
        line, plans = split_tick(td, split, w, rec["t"], D)
        assert line == rec["line"] and plans == rec["plans"], rec["t"]
        assert_same(split, rec, ("split", rec["t"]))
    assert sizes == {2, 3, 4} and run["m"]["total_second_passengers"] > 0
    step.close(), split.close()
