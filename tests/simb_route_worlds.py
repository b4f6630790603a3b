"""Routed worlds in a batch (td_simb_route, DeviceSimulatorBatch(route=...)): the helpers of tests/test_gpu_simb_route.py.

The comparator is the one tests/test_gpu_simb_pool_n.py established: every world of a batch equals a DeviceSimulator handle on
the same inputs and policy, tick by tick.  The handle's dispatcher is td.tick_batched on its one model (the batch dispatches
through td_tick_batched, whose solver may break a tie between equal optima differently from td_tick's)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sim_batch_worlds as sbw
import sim_worlds as sw

BIG = sw.BIG_COST
TD_EINVAL = -1
NONE_SEEN = -(1 << 63)
EMPTY_ROWS = np.zeros((0, 5), np.int64)
NO_ROUTE_M = dict(drop_numb=0, ride_time=0, solo_time=0, max_over_loss=NONE_SEEN)


def lib_of():
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def err():
    return lib_of().td_last_error().decode()


def ws():
    v = ctypes.c_int64(-1)
    assert lib_of().td_workspace_bytes(ctypes.byref(v)) == 0
    return v.value


def i32(*v):
    return np.array(v, np.int32)


def kw_of(city):
    return dict(n_stands=city["stands"], drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"], big_cost=BIG)


# a world of a batch: dict(rows, cabs, pool=, max_loss=, pn=(k_hi, k_lo) | k | None, wait=, loss=, route=bool)
def world(rows, cabs, pn=None, wait=0, loss=0, route=False, pool="greedy", max_loss=None):
    return dict(rows=rows, cabs=cabs, pn=pn, wait=wait, loss=loss, route=route, pool=pool, max_loss=max_loss)


def batch_of(td, worlds, city, route=None, dist=None, **kw):
    """route: None = every world's own flag; False = the same batch without routes (td_simb_route is never called)"""
    routes = [w["route"] for w in worlds] if route is None else route
    return td.DeviceSimulatorBatch([w["rows"] for w in worlds], [w["cabs"] for w in worlds], pool=[w["pool"] for w in worlds],
                                   max_loss=[w["max_loss"] for w in worlds], pool_n=[w["pn"] for w in worlds], pool_wait=[w["wait"] for w in worlds],
                                   pool_loss=[w["loss"] for w in worlds], route=routes, dist=dist, **kw_of(city), **kw)


def handle_of(td, w, city, dist=None, **kw):
    return td.DeviceSimulator(w["rows"], n_cabs=w["cabs"], pool=w["pool"], max_loss=w["max_loss"], pool_n=w["pn"], pool_wait=w["wait"],
                              pool_loss=w["loss"], route=w["route"], dist=dist, **kw_of(city), **kw)


def handle_tick(td, dev, city, t, dist=None):
    """one tick of a DeviceSimulator with td.tick_batched on its one model as the dispatcher -> (the line as
    sim_batch_worlds.split_tick writes it, did the world's LCM run in this tick)"""
    info = dev.begin(t)
    if not info[0]:
        return None, False
    if info[2] == 0:
        return dev.format_line(t, [1, info[1], 0, 0, 0, 0, 0, 0, dev.apply()]), False
    cab_to, dem_from = dev.model()
    r = td.tick_batched([np.asarray(cab_to, np.int32)], [np.asarray(dem_from, np.int32)], dist, big_cost=BIG, drop_time=city["drop_time"],
                        max_non_lcm=city["max_non_lcm"])[0]
    opt = dev.apply(r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"])
    lcm = bool(max(info[2], info[3]) > city["max_non_lcm"])
    k = len(r["lcm_rows"]) if lcm else 0
    return dev.format_line(t, [1, info[1], info[2], lcm, k, lcm and r["solved"], info[3] - k, info[2] - k, opt]), lcm


def batch_tick(td, dev, city, t, way):
    lines = dev.tick(t) if way == "step" else sbw.split_tick(td, dev, city, t)
    return [None] * dev.batch if lines is None else lines


def has_stops(rs):
    """per cab: a stop is left at its position"""
    pos, stops = rs["c_pos"], rs["c_stops"]
    at = np.where(pos < 8, stops[np.arange(len(pos)), np.minimum(pos, 7)], -1)
    return at >= 0


def assert_no_routes(dev, b, where):
    """world b of a routed batch never had a route: no stop, nobody dropped off, the counters empty"""
    rs = dev.route_state(b)
    assert (rs["c_stops"] == -1).all() and (rs["c_pos"] == 0).all() and (rs["d_drop"] == -1).all(), (where, b)
    assert dev.route_metrics()[b] == NO_ROUTE_M, (where, b)


def assert_world_is_handle(dev, b, one, where, m=None, rm=None):
    """state, metrics and, where the handle has routes, route state and route metrics of world b equal the handle's"""
    sbw.assert_same_state(dev, b, one.state(), where)
    assert (dev.m if m is None else m)[b] == one.m, (where, b)
    if one.route or getattr(one, "had_routes", False):
        got, want = dev.route_state(b), one.route_state()
        for k, v in want.items():
            assert np.array_equal(got[k], v), (where, b, k, np.nonzero(got[k] != v)[0][:8].tolist())
        assert (dev.route_metrics() if rm is None else rm)[b] == one.route_metrics(), (where, b)
