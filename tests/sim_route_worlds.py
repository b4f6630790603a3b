"""The route model of the simulator worlds (Simulator(route=True), td_sim_route): hand-made worlds whose expected pick-up and
drop-off ticks are written out by hand, the oracle backend on a line or a table, and the recorded specification run that the
CPU tests check and the GPU tests compare a device world with, tick by tick."""
import copy

import numpy as np
import pytest

import sim_dist_worlds as sdw
import sim_worlds as sw
from oracle import oracle

ROUTE_KEYS = ("d_drop", "c_pos", "c_stops")


class RouteOracleBackend(sdw.OracleDistTickBackend):
    """the oracle's tick on the world's table (None: the line) and oracle.pool_n as the pool finder of a stage"""

    def __init__(self, D=None):
        self.D = None if D is None else np.ascontiguousarray(D, dtype=np.int32)

    def find_pool_n(self, k, frm, to, wait, loss):
        return oracle.pool_n(k, frm, to, wait, loss, self.D)


def req(*trips, at=0):
    """requests (from, to), all known and wanted at tick `at` -> demand rows (id, from, to, time, at)"""
    return np.asarray([(i, f, t, at, at) for i, (f, t) in enumerate(trips)], np.int64).reshape(-1, 5)


# an asymmetric table of 6 stands: a one-way ring, one step costs 1 (0 -> 1 -> .. -> 5 -> 0), so the way back is 6 minus the way there
RING6 = sdw.ring(6)

# Hand-made worlds.  Cab c starts at stand c.  Every world: the requests; the rule; and, worked out by hand from the rules of
# Simulator(route=True), d_pick and d_drop per request, the routed cab, the tick it is free again and the stand it is free at.
# `ticks` runs one tick past the free tick.  The comments walk the cab through its stops.
HAND = {
    # the cab stands at from[p0] = 0: t0 picks r0; 0 -> 1: t1 picks r1; 1 -> 2: t2 drops r1; 2 -> 3: t3 drops r0.  cost 3
    "standing": dict(stands=12, cabs=1, drop_time=4, max_non_lcm=16, pool_n=2, wait=1, loss=100, rows=req((0, 3), (1, 2)),
                     d_pick=[0, 1], d_drop=[3, 2], cab=0, free_t=3, free_at=3, cost=3, path="opt", how="standing"),
    # the cab at 0 heads to from[p0] = 2 (two ticks): t2 picks r0; t3 picks r1 at 3; t4 drops r1 at 4; t5 drops r0 at 5.  cost 3
    "heading": dict(stands=12, cabs=1, drop_time=4, max_non_lcm=16, pool_n=2, wait=1, loss=100, rows=req((2, 5), (3, 4)),
                    d_pick=[2, 3], d_drop=[5, 4], cab=0, free_t=5, free_at=5, cost=3, path="opt", how="heading"),
    # both members start at 0, where the cab stands: t0 picks both (a zero-length pick leg); t1 drops r1 at 1; t2 drops r0 at 2
    "same_from": dict(stands=12, cabs=1, drop_time=4, max_non_lcm=16, pool_n=2, wait=1, loss=100, rows=req((0, 2), (0, 1)),
                      d_pick=[0, 0], d_drop=[2, 1], cab=0, free_t=2, free_at=2, cost=2, path="opt", how="standing", zero_pick=1),
    # pool of three; the last pick-up's stand 2 is where r0 and r1 get off: t0 picks r0, t1 picks r1, t2 picks r2 and drops r0
    # and r1 (two zero-length drop legs, the drop stand equals the next stop's), t3 drops r2 at 3.  cost 3
    "drop_at_next": dict(stands=12, cabs=1, drop_time=4, max_non_lcm=16, pool_n=3, wait=2, loss=100, rows=req((0, 2), (1, 2), (2, 3)),
                         d_pick=[0, 1, 2], d_drop=[2, 2, 3], cab=0, free_t=3, free_at=3, cost=3, path="opt", how="standing", zero_drop=2),
    # the last two drops at one stand: t0 picks r0, t1 picks r1, t2 drops both at 2 and the cab is free in that tick.  cost 2
    "last_two": dict(stands=12, cabs=1, drop_time=4, max_non_lcm=16, pool_n=2, wait=1, loss=100, rows=req((0, 2), (1, 2)),
                     d_pick=[0, 1], d_drop=[2, 2], cab=0, free_t=2, free_at=2, cost=2, path="opt", how="standing", zero_drop=1, same_tick_free=1),
    # pool of four: t0..t3 pick r0..r3 at 0..3; t4 drops r1 and r3 at 4; t5 drops r0 and r2 at 5.  cost 5
    "four": dict(stands=12, cabs=1, drop_time=4, max_non_lcm=16, pool_n=4, wait=3, loss=100, rows=req((0, 5), (1, 4), (2, 5), (3, 4)),
                 d_pick=[0, 1, 2, 3], d_drop=[5, 4, 5, 4], cab=0, free_t=5, free_at=5, cost=5, path="opt", how="standing", zero_drop=2, same_tick_free=1),
    # the LCM path (max_non_lcm 1, two cabs, the model has two rows), the cab heading: cab 1 at stand 1 is the nearest to
    # from[p0] = 3: t2 picks r0; t3 picks r1 at 4; t4 drops r1 at 5; t5 drops r0 at 6.  Without routes the cab forgets the pool at
    # the pick-up and drives r0's own trip; r1 is never picked up
    "lcm_heading": dict(stands=12, cabs=2, drop_time=4, max_non_lcm=1, pool_n=2, wait=1, loss=100, rows=req((3, 6), (4, 5)),
                        d_pick=[2, 3], d_drop=[5, 4], cab=1, free_t=5, free_at=6, cost=3, path="lcm", how="heading"),
    # a line of 10 stands; the pool's first pick-up starts at 5 and the pool costs 7: 5 + 7 and 5 - 7 are both off the line, so
    # without routes cheat_a_bit sends the cab to stand 0 and it is free there after 5 ticks.  With routes, cab 5 stands at 5:
    # t0 picks r1 (5 -> 3); 5 -> 4: t1 picks r0 (4 -> 8); 4 -> 3: t2 drops r1; 3 -> 8: t7 drops r0.  cost 1 + 1 + 5 = 7
    "off_line": dict(stands=10, cabs=6, drop_time=2, max_non_lcm=16, pool_n=2, wait=1, loss=50, rows=req((4, 8), (5, 3)),
                     d_pick=[1, 0], d_drop=[7, 2], cab=5, free_t=7, free_at=8, cost=7, path="opt", how="standing"),
    # the one-way ring of six stands; the cab at 0 heads to from[p0] = 1: t1 picks r0 (1 -> 4); t2 picks r1 at 2 (2 -> 3); t3 drops
    # r1 at 3; t4 drops r0 at 4.  cost 3; on this table the way back from 4 to 1 would be 3 more
    "ring6": dict(stands=6, cabs=1, drop_time=3, max_non_lcm=16, pool_n=2, wait=1, loss=100, rows=req((1, 4), (2, 3)), dist=RING6,
                  d_pick=[1, 2], d_drop=[4, 3], cab=0, free_t=4, free_at=4, cost=3, path="opt", how="heading"),
}


def traced_simulator():
    """Simulator with the bookkeeping the tests count and check, kept out of the specification: route_trace = dispatches
    {(method, "standing" | "heading"): routed dispatches}; zero_pick / zero_drop = the stops served at a stand the cab was already
    at (behind the stop it came for); same_tick_free = the cabs freed by a zero-length last leg; freed = one (cab, tick stop 0
    was served, the record's cost, tick it became free, stand, 1 = the last stop was a drop, that stop's request's `to`) per
    finished route; n_pick / n_drop = how often the route served each request's pick-up / drop-off"""
    from taxidispatcher_amd import simulator

    class TracedSimulator(simulator.Simulator):
        def set_route(self, on):
            if on and not self._has_routes:
                nd = self.d_id.size
                self.route_trace = dict(dispatches={}, zero_pick=0, zero_drop=0, same_tick_free=0, freed=[],
                                        n_pick=np.zeros(nd, np.int64), n_drop=np.zeros(nd, np.int64))
                self._route_run = {}     # cab -> [tick stop 0 was served, the record's cost]
            super().set_route(on)

        def _give_route(self, c, cust, method, how):
            super()._give_route(c, cust, method, how)
            self._route_run[c] = [None, self._routes[cust[0]][1]]
            d = self.route_trace["dispatches"]
            d[method, how] = d.get((method, how), 0) + 1

        def _serve(self, t, d, drop):
            super()._serve(t, d, drop)
            self.route_trace["n_drop" if drop else "n_pick"][d] += 1

        def _advance(self, t, c, cur):
            tr, run, before = self.route_trace, self._route_run[c], int(self.c_pos[c])
            if run[0] is None:           # this call serves stop 0
                run[0] = t
            super()._advance(t, c, cur)
            pos = int(self.c_pos[c])
            # the first stop served here is the one the cab came for; every further one is a zero-length leg
            for q in range(before + 1, pos):
                tr["zero_drop" if self.c_stops[c, q] & 1 else "zero_pick"] += 1
            if self.c_clnt[c] == -1:     # free
                if pos - before > 1:     # the last leg was a zero-length one
                    tr["same_tick_free"] += 1
                last = int(self.c_stops[c, pos - 1])
                tr["freed"].append((int(c), run[0], run[1], int(t), int(cur), last & 1, int(self.d_to[last >> 1])))
                del self._route_run[c]
    return TracedSimulator


def route_state_of(sim):
    return {k: np.asarray(getattr(sim, k)).copy() for k in ROUTE_KEYS}


def spec_run(rows, cabs, city, ticks, pool_n, wait, loss, backend=None, dist=None, route=True, **kw):
    """Simulator(route=...) on `backend` (default: RouteOracleBackend on the world's table) with the city's constants patched in,
    recorded per tick: t, line, state, m, and with routes route (route_state_of) and route_m; -> dict(ticks, sim)"""
    from taxidispatcher_amd import simulator
    with pytest.MonkeyPatch.context() as mp:
        sw.patch_constants(mp, city)
        be = RouteOracleBackend(dist) if backend is None else backend
        sim = traced_simulator()(rows, be, n_cabs=cabs, pool_n=pool_n, pool_wait=wait, pool_loss=loss, dist=dist, route=route, **kw)
        recs = []
        for t in range(ticks):
            line = sim.tick(t)
            rec = dict(t=t, line=line, state=sw.state_of(sim), m=copy.deepcopy(sim.m))
            if route:
                rec.update(route=route_state_of(sim), route_m=dict(sim.route_m))
                check_invariants(sim, t)
            recs.append(rec)
        return dict(ticks=recs, sim=sim)


def hand_run(name, backend=None, route=True):
    w = HAND[name]
    return spec_run(w["rows"], w["cabs"], w, w["free_t"] + 2, w["pool_n"], w["wait"], w["loss"], backend=backend, dist=w.get("dist"), route=route)


def check_invariants(sim, t):
    """the three invariants of the specification, after any tick: a routed cab becomes free exactly `cost` ticks after it served
    stop 0, at the stand of its last drop-off; the route serves every member's pick-up and drop-off at most once, a dropped-off
    member exactly once each with d_pick <= d_drop; max_over_loss <= 0"""
    tr = sim.route_trace
    for cab, t0, cost, t_free, stand, last_is_drop, last_to in tr["freed"]:
        assert t_free == t0 + cost and last_is_drop and stand == last_to, (t, cab, t0, cost, t_free, stand, last_to)
    assert tr["n_pick"].max(initial=0) <= 1 and tr["n_drop"].max(initial=0) <= 1, t
    dropped = sim.d_drop >= 0
    assert np.array_equal(dropped, tr["n_drop"] == 1) and (tr["n_pick"][dropped] == 1).all(), t
    assert (sim.d_pick[dropped] <= sim.d_drop[dropped]).all() and (sim.d_pick[dropped] >= 0).all(), t
    assert sim.route_m["drop_numb"] == int(dropped.sum()), t
    assert sim.route_m["max_over_loss"] <= 0, (t, sim.route_m)
