"""Pools of up to four in batched worlds: td_simb_pooling_n / td_simb_pools_n, DeviceSimulatorBatch(pool_n=[...], pool_wait=, pool_loss=).

2. family A's four fleets and its empty world in one batch under two policy lists that mix none, greedy with max_loss, optimal
   and (4, 2), (3, 3), (2, 2) with a wait and a loss per world: every world equals a DeviceSimulator handle under the same
   policy tick by tick, through td_simb_step and through begin -> model -> apply with outside decisions.  The handle's tick
   is begin -> model -> td.tick_batched on its one model -> apply: the batch dispatches through td_tick_batched, whose solver
   may break a tie between equal optima differently from td_tick's, and the subject here is the world layer;
3. the batch boundary: a world with 512 requests in a tick equals the oracle's cascade, 513 are refused naming the world;
5. the life cycle of the two entry points; the log refused with pools of three both ways round; the log of a batch with pools of
   two against the specification's records; a pair world past 2048 requests beside a record world;
6. a batch on an asymmetric distance table against the host specification with dist=."""
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

TD_EINVAL = -1
CITY = sbw.CITY_A
BIG = sw.BIG_COST
# world order: A1, A7, A40, A90, Aempty.  An entry: (pool, max_loss, pool_n, pool_wait, pool_loss)
NONE, GREEDY, OPT = ("none", None, None, 0, 0), ("greedy", 1.5, None, 0, 0), ("optimal", None, None, 0, 0)
P42, P33, P22 = ("greedy", None, (4, 2), 1, 50), ("greedy", None, (3, 3), 1, 40), ("greedy", None, (2, 2), 2, 100)
POLICY_LISTS = ((P42, NONE, P33, GREEDY, P22), (OPT, P22, GREEDY, P42, NONE))


def lib_of():
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def err():
    return lib_of().td_last_error().decode()


def kw_of(city):
    return dict(n_stands=city["stands"], drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"], big_cost=BIG)


def batch_of(td, runs, policies, city=CITY, **kw):
    pool, ml, pn, wait, loss = (list(c) for c in zip(*policies))
    return td.DeviceSimulatorBatch([r["rows"] for _, r in runs], [r["world"]["cabs"] for _, r in runs], pool=pool, max_loss=ml, pool_n=pn,
                                   pool_wait=wait, pool_loss=loss, **kw_of(city), **kw)


def handle_of(td, run, policy, city=CITY, **kw):
    pool, ml, pn, wait, loss = policy
    return td.DeviceSimulator(run["rows"], n_cabs=run["world"]["cabs"], pool=pool, max_loss=ml, pool_n=pn, pool_wait=wait, pool_loss=loss,
                              **kw_of(city), **kw)


def handle_tick(td, dev, city, t):
    """one tick of a DeviceSimulator with td.tick_batched on its one model as the dispatcher; the line as sim_batch_worlds.split_tick writes it"""
    info = dev.begin(t)
    if not info[0]:
        return None
    if info[2] == 0:
        return dev.format_line(t, [1, info[1], 0, 0, 0, 0, 0, 0, dev.apply()])
    cab_to, dem_from = dev.model()
    r = td.tick_batched([np.asarray(cab_to, np.int32)], [np.asarray(dem_from, np.int32)], None, big_cost=BIG, drop_time=city["drop_time"],
                        max_non_lcm=city["max_non_lcm"])[0]
    opt = dev.apply(r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"])
    lcm = max(info[2], info[3]) > city["max_non_lcm"]
    k = len(r["lcm_rows"]) if lcm else 0
    return dev.format_line(t, [1, info[1], info[2], lcm, k, lcm and r["solved"], info[3] - k, info[2] - k, opt])


def plans_of(dev, policy, b=None):
    args = () if b is None else (b,)
    return dev.pools_n(*args) if policy[2] is not None else dev.pools(*args)


# ---- 2. a batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["step", "split"])
@pytest.mark.parametrize("which", [0, 1])
def test_a_mixed_batch_equals_a_handle_per_world(td, which, way):
    city, runs = sbw.family("A")
    policies = POLICY_LISTS[which]
    dev = batch_of(td, runs, policies)
    assert dev.pool_n == [p[2] for p in policies]
    alone = [handle_of(td, run, policies[b]) for b, (name, run) in enumerate(runs) if name != "Aempty"]
    sizes, seconds = [set() for _ in runs], None
    for t in range(city["ticks"]):
        lines = dev.tick(t) if way == "step" else sbw.split_tick(td, dev, city, t)
        for b, one in enumerate(alone):
            want = handle_tick(td, one, city, t)
            assert (None if lines is None else lines[b]) == want, (t, b)
            if want is not None:
                plans = plans_of(one, policies[b])
                assert plans_of(dev, policies[b], b) == plans, (t, b)
                if policies[b][2] is not None:
                    sizes[b] |= {len(p[0]) for p in plans}
            sbw.assert_same_state(dev, b, one.state(), (which, way, t))
        assert lines is None or lines[-1] is None, t      # the world without requests
        m = dev.m
        assert [m[b] for b in range(len(alone))] == [one.m for one in alone], t
    seconds = [x["total_second_passengers"] for x in m]
    for b, p in enumerate(policies[:-1]):
        assert (seconds[b] == 0) == (p[0] == "none"), (b, seconds)
        if p[2] is not None:      # a (4, 2) world pooled four, three and two; a (k, k) world pools of k alone
            assert sizes[b] == set(range(p[2][1], p[2][0] + 1)), (b, sizes[b])
    sbw.assert_same_state(dev, len(runs) - 1, runs[-1][1]["ticks"][-1]["state"], "the empty world")
    for one in alone:
        one.close()
    dev.close()


# ---- 3. the batch boundary -------------------------------------------------------------------------------------------------------------
def wide_batch(td, n):
    rows = W.one_tick_world(n)
    small = W.one_tick_world(30, seed=4)
    return rows, td.DeviceSimulatorBatch([small, rows], [W.WIDE["stands"]] * 2, pool_n=[None, (2, 2)], pool_wait=0, pool_loss=0, **kw_of(W.WIDE))


def test_512_requests_in_a_world_of_a_batch(td):
    rows, dev = wide_batch(td, 512)
    info = dev.begin(0)
    want, happy, _ = W.cascade(2, 2, rows[:, 1], rows[:, 2], 0, 0)
    assert info[1].tolist()[:3] == [1, 512, W.WIDE["stands"]] and 0 < happy < 65536 and len(want) > 50
    assert dev.pools_n(1) == want and info[1][3] == 512 - len(want)
    m = dev.m[1]
    assert m["max_POOL_MEM_size"] == happy and m["max_POOL_size"] == len(want)
    assert len(dev.pools(0)) > 0      # the pair world beside it pooled as it always does
    dev.close()


def test_513_requests_in_a_world_of_a_batch_are_refused_naming_the_world(td):
    rows, dev = wide_batch(td, 513)
    info = np.zeros((2, 4), np.int32)
    assert lib_of().td_simb_begin(dev._h, 0, info.ctypes.data) == TD_EINVAL
    assert "world 1 has 513 requests" in err()
    dev.close()


# ---- 5. the life cycle -----------------------------------------------------------------------------------------------------------------
def i32(*v):
    return np.array(v, np.int32)


def test_the_life_cycle_of_the_batch_policy_call(td):
    lib = lib_of()
    city, runs = sbw.family("A")
    two = runs[1:3]      # A7, A40
    policies = (P42, GREEDY)
    dev, twin = batch_of(td, two, policies), batch_of(td, two, policies)
    call = lambda h, hi, lo, wt, ls, mh=0: lib.td_simb_pooling_n(h, hi.ctypes.data, lo.ctypes.data, wt.ctypes.data, ls.ctypes.data, mh)
    keep, z = i32(0, 0), i32(0, 0)
    for args, word in (((i32(5, 0), i32(2, 0), z, z), "k_hi[0]"), ((i32(0, 2), i32(0, 3), z, z), "k_lo[1]"), ((i32(4, 0), i32(1, 0), z, z), "k_lo[0]"),
                       ((i32(4, 0), i32(2, 0), i32(-1, 0), z), "negative"), ((i32(0, 2), i32(0, 2), z, i32(0, -1)), "negative"),
                       ((i32(4, 0), i32(2, 0), z, z, (1 << 22) + 1), "max_happy")):
        assert call(dev._h, *args) == TD_EINVAL and word in err(), word
    assert lib.td_simb_pooling_n(dev._h, None, None, None, None, 0) == TD_EINVAL
    assert call(dev._h, keep, keep, z, z, 1 << 22) == 0 and call(dev._h, keep, keep, z, z) == 0      # every world keeps what it has
    n = ctypes.c_int32(0)
    a = np.full((64, 9), -7, np.int32)
    ad = a.ctypes.data
    t_plans, threes = None, 0
    for t in range(city["ticks"]):
        info, same = dev.begin(t), twin.begin(t)
        assert np.array_equal(info, same), t      # the refusals and the keep-calls above changed no policy
        for b in range(2):
            read = "pools_n" if dev.pool_n[b] is not None else "pools"
            assert getattr(dev, read)(b) == getattr(twin, read)(b), (t, b)
        if t < 12 and info[0][0] and len(dev.pools_n(0)) >= 2 and t_plans is None:
            t_plans = t
            plans = dev.pools_n(0)
            assert call(dev._h, i32(2, 2), i32(2, 2), z, z) == TD_EINVAL and "waits for td_simb_apply" in err()
            assert lib.td_simb_pools(dev._h, 0, 64, ad, ad, ad, ad, ctypes.byref(n)) == TD_EINVAL and "td_simb_pools_n" in err()
            assert lib.td_simb_pools_n(dev._h, 1, 64, ad, ad, ctypes.byref(n)) == TD_EINVAL and "td_simb_pools" in err()
            assert lib.td_simb_pools_n(dev._h, 2, 64, ad, ad, ctypes.byref(n)) == TD_EINVAL and "world 2" in err()
            size = np.full(64, -7, np.int32)
            assert lib.td_simb_pools_n(dev._h, 0, len(plans) - 1, ad, size.ctypes.data, ctypes.byref(n)) == TD_EINVAL
            assert n.value == len(plans) and (a == -7).all() and (size == -7).all()
            assert dev.pools_n(0) == plans
        if info[:, 0].any():
            for d in (dev, twin):
                cab_off, cab_to, dem_off, dem_from = d.model()
                d.apply([None if not (info[b][0] and info[b][2]) else ((), (), False, np.arange(0)) for b in range(2)])
        if t == 12:      # back on pairs, both worlds; then world 1 alone under (3, 3): each from the next begin on
            dev.set_pool_n(None), twin.set_pool_n(None)
            with pytest.raises(td.TdError):
                dev.pools_n(0)
        if t == 20:
            dev.set_pool_n([None, (3, 3)], 1, 50), twin.set_pool_n([None, 3], [0, 1], [0, 50])
            assert dev.pool_n == [None, (3, 3)]
            with pytest.raises(td.TdError):
                dev.pools(1)
            dev.pools(0)
        if t > 20 and info[1][0] and info[1][2]:
            threes += len(dev.pools_n(1))
            assert all(len(p[0]) == 3 for p in dev.pools_n(1)), t
    assert t_plans is not None and threes > 0
    dev.close(), twin.close()


def test_the_log_is_refused_with_pools_of_three_in_a_batch_both_ways_round(td):
    lib = lib_of()
    city, runs = sbw.family("A")
    dev = batch_of(td, runs[1:3], (P33, GREEDY))
    assert lib.td_simb_log(dev._h, 0xffe, 4096) == TD_EINVAL and "not built" in err()
    assert lib.td_simb_log(dev._h, 0, 0) == 0      # an empty mask is no log
    dev.set_pool_n([(2, 2), None], 1, 50)
    assert lib.td_simb_log(dev._h, 0xffe, 4096) == 0      # pools of two can be logged
    hi, lo = i32(0, 3), i32(0, 2)
    assert lib.td_simb_pooling_n(dev._h, hi.ctypes.data, lo.ctypes.data, lo.ctypes.data, lo.ctypes.data, 0) == TD_EINVAL and "not built" in err()
    assert dev.pool_n == [(2, 2), None]
    hi = i32(0, 2)
    assert lib.td_simb_pooling_n(dev._h, hi.ctypes.data, hi.ctypes.data, hi.ctypes.data, hi.ctypes.data, 0) == 0
    dev.close()


@pytest.mark.parametrize("name", ["A7", "A40"])
def test_the_log_of_a_batch_with_pools_of_two_equals_the_specifications(td, name):
    """world 0 under (2, 2) beside a pair world, both logged; decisions from td.tick, the host specification's own dispatcher on
    HipBackend: world 0's records equal the specification's, record for record"""
    from taxidispatcher_amd import simulator
    city, runs = sbw.family("A")
    run0 = dict(runs)[name]
    spec = W.spec_run(run0["rows"], run0["world"]["cabs"], city, city["ticks"], (2, 2), backend=simulator.HipBackend(), events=True)
    p22 = ("greedy", None, (2, 2), W.WAIT, W.LOSS)
    dev = batch_of(td, [(name, run0), ("A90", dict(runs)["A90"])], (p22, GREEDY), events=True)
    got, pair_world = [], 0
    for rec in spec["ticks"]:
        t = rec["t"]
        info = dev.begin(t)
        if info[:, 0].any():
            assert dev.pools_n(0) == (rec["plans"] if info[0][0] else []), t
            cab_off, cab_to, dem_off, dem_from = dev.model()
            dec = []
            for b in range(2):
                if not (info[b][0] and info[b][2]):
                    dec.append(None)
                    continue
                r = td.tick(cab_to[cab_off[b]:cab_off[b + 1]], dem_from[dem_off[b]:dem_off[b + 1]], None, big_cost=BIG, drop_time=city["drop_time"],
                            max_non_lcm=city["max_non_lcm"])
                dec.append((r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"]))
            dev.apply(dec)
        ev = dev.events().tolist()
        got += [r for r in ev if r[1] == 0]
        pair_world += sum(r[1] == 1 and r[2] == 7 for r in ev)
        sbw.assert_same_state(dev, 0, rec["state"], t)
    assert dev.events_lost == 0
    assert [tuple(r) for r in got] == [tuple(int(v) for v in r) for r in spec["events"]]
    assert sum(r[2] == 7 for r in got) > 0 and sum(r[2] == 11 for r in got) == spec["m"]["total_second_passengers"] > 0
    assert pair_world > 0      # the pair world beside it logged its own pairs
    dev.close()


def test_a_pair_world_past_2048_requests_beside_a_record_world(td):
    """the pair world is pooled by the per-world pair path (td_pool2, beyond td_pool2_batched's model), the record world as always"""
    big, small = W.one_tick_world(2049), W.one_tick_world(60, seed=4)
    both = td.DeviceSimulatorBatch([big, small], [W.WIDE["stands"]] * 2, pool_n=[None, (3, 2)], pool_wait=1, pool_loss=50, **kw_of(W.WIDE))
    alone = td.DeviceSimulatorBatch([big], [W.WIDE["stands"]], **kw_of(W.WIDE))
    info, one = both.begin(0), alone.begin(0)
    assert info[0].tolist() == one[0].tolist() and info[0][1] == 2049
    assert both.pools(0) == alone.pools(0) and len(both.pools(0)) > 500
    want, happy, _ = W.cascade(3, 2, small[:, 1], small[:, 2], 1, 50)
    assert both.pools_n(1) == want and {len(p[0]) for p in want} == {2, 3}
    assert both.m[1]["max_POOL_MEM_size"] == happy
    both.close(), alone.close()


# ---- 6. a batch on a distance table ------------------------------------------------------------------------------------------------------
def test_a_batch_on_an_asymmetric_table(td):
    """ring12 under (4, 2) beside a pair world, decisions from td.tick with the table (the host specification's own dispatcher)"""
    from taxidispatcher_amd import simulator
    D, w = sdw.table("ring12"), sdw.world("ring12")
    rows = sdw.gen_demand(D, **{k: w[k] for k in ("per_tick", "ticks", "span", "max_wait", "seed")})
    ticks, wait, loss = 20, 2, 100
    run = W.spec_run(rows, w["cabs"], w, ticks, (4, 2), wait, loss, backend=simulator.HipBackend(dist=D), dist=D)
    dev = td.DeviceSimulatorBatch([rows, rows], [w["cabs"]] * 2, pool_n=[(4, 2), None], pool_wait=wait, pool_loss=loss, dist=D, **kw_of(w))
    sizes = set()
    for rec in run["ticks"]:
        t = rec["t"]
        info = dev.begin(t)
        assert bool(info[0][0]) == (rec["line"] is not None), t
        if not info[:, 0].any():
            continue
        assert dev.pools_n(0) == rec["plans"], t
        sizes |= {len(p[0]) for p in rec["plans"]}
        cab_off, cab_to, dem_off, dem_from = dev.model()
        dec = []
        for b in range(2):
            if not (info[b][0] and info[b][2]):
                dec.append(None)
                continue
            r = td.tick(cab_to[cab_off[b]:cab_off[b + 1]], dem_from[dem_off[b]:dem_off[b + 1]], D, big_cost=BIG, drop_time=w["drop_time"],
                        max_non_lcm=w["max_non_lcm"])
            dec.append((r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"]))
        dev.apply(dec)
        sbw.assert_same_state(dev, 0, rec["state"], t)
        assert dev.m[0] == rec["m"], t
    assert sizes == {2, 3, 4} and dev.m[0]["total_second_passengers"] == run["m"]["total_second_passengers"] > 0
    dev.close()
