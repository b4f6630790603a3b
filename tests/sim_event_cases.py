"""Cases for the event log (Simulator(events=True), td_sim_log / td_sim_events and their td_simb twins): a hand-made world
with its simulog.txt written out from Simulator.java, the CPU runs that record a world's events tick by tick, and the
invariants that tie the records to the independent outputs (the simulog_solv line, the metrics)."""
import copy
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sim_worlds as sw

(PICKED_UP, CAB_FREE, DROPPED, TEMP_DEMAND, TEMP_DEMAND_ID, POOL, POOL_PAIR, ASSIGNED_PICKED, HEADING, ASSIGNED_LCM,
 POOLED_SECOND) = range(1, 12)
LCM, OPT = 1, 2
ALL_KINDS = tuple(range(1, 12))

# ---- the hand-made world: 10 stands on the line, cabs 0, 1, 2 at stands 0, 1, 2 (initSupply :565-573), DROP_TIME 3,
# MAX_NON_LCM 2 (a model of 3 goes through the LCM, which then takes exactly one pair, :545)
HAND = dict(stands=10, cabs=3, drop_time=3, max_non_lcm=2, ticks=8)
# id, from, to, time, at
HAND_ROWS = np.asarray([(11, 0, 3, 1, 1), (12, 0, 4, 1, 1), (13, 2, 5, 1, 1), (14, 4, 6, 1, 1), (15, 9, 8, 1, 1), (16, 3, 5, 2, 2),
                        (18, 7, 9, 6, 6), (19, 4, 3, 6, 6), (20, 5, 2, 7, 7)], np.int64)
# simulog.txt of that world, derived by hand from Simulator.java (the line that writes each string is cited):
#  t=0  no request is due: createTempDemand writes its header alone (:331, :352).
#  t=1  11 .. 14 start within 2 stands of a free cab; 15 (stand 9) does not (:343-349).  findPool (:681-758): the cheapest
#       plans are 11+12 (0->0->3->4, cost 4), 12+11 (cost 4, shares 11), 13+14 (2->4->5->6, cost 4): 11(12) and 13(14) stay
#       (:746).  Model: cabs at 0, 1, 2 x customers at 0, 2 -> size 3 > MAX_NON_LCM: the LCM takes the first smallest cell,
#       cab 0 / customer 11 (cost 0), and stops at size 2 (:545).  analyzePairs' cab loop: cab 0 stands at 11's stand ->
#       assignToCabAndGo with the POOL clause (:448-465); its request loop: :654, then assignPooledCustomer (:432-433).
#       The solver gets cabs 1, 2 x customer 13 (costs 1, 0): cab 2.  analyzeSolution: the pooled 14 first (:392), then
#       assignToCabAndGo (:406).  Cab 0 drives 0 -> cheatAbit(0, 4) = 4, cab 2 drives 2 -> 6: both arrive at t=5.
#  t=2  16 (stand 3): only cab 1 is free, 2 stands away.  One customer: findPool writes no pair (:742, :756); a model of 1
#       goes to the solver alone: goToPickupUp (:486-487).  15 has no free cab heading near it.
#  t=3  no cab is without a client: the list is empty.
#  t=4  cab 1 reaches 16 (:233) and leaves for stand 5; 15 has waited DROP_TIME (:339).
#  t=5  cabs 0 and 2 finish their trips (:251).
#  t=6  cab 1 is free at 5.  18 (7->9) and 19 (4->3): plan 18+19 costs 3+1+6 = 10, 19+18 costs 11 -> 18(19).  Cabs at 4, 5,
#       6 x customer at 7: size 3 -> LCM takes cab 2 (cost 1): goToPickupUp with LCM (:632), then :654 and :432-433.  The
#       solver gets two cabs and no customer: nothing.
#  t=7  cab 2 reaches 18 (:233).  20 (stand 5): cabs 0 (at 4) and 1 (at 5), size 2 -> solver: cab 1 is there (:406, no POOL).
HAND_TEXT = """\
Time 0. tempDemand:
Time 1. tempDemand: 11, 12, 13, 14,
Time 1. Customers in pool: 11(12), 13(14),
Time 1. Customer 11 assigned to and picked up by Cab 0 (POOL: the other Customer 12) (method LCM)
Time 1. Customer 11 assigned by LCM to Cab 0
Time 1. Customer 12 assigned in a pool as second passenger to Cab 0 (method LCM)
Time 1. Customer 14 assigned in a pool as second passenger to Cab 2 (method OPT)
Time 1. Customer 13 assigned to and picked up by Cab 2 (POOL: the other Customer 14) (method OPT)
Time 2. tempDemand: 16,
Time 2. Customers in pool:
Time 2. Customer 16 assigned to Cab 1, cab is heading to the customer (method OPT)
Time 3. tempDemand:
Time 4. Customer 16 picked up by Cab 1
Time 4. Customer 15 dropped
Time 4. tempDemand:
Time 5. Cab 0 is free at stand 4
Time 5. Cab 2 is free at stand 6
Time 5. tempDemand:
Time 6. Cab 1 is free at stand 5
Time 6. tempDemand: 18, 19,
Time 6. Customers in pool: 18(19),
Time 6. Customer 18 assigned to Cab 2, cab is heading to the customer (method LCM)
Time 6. Customer 18 assigned by LCM to Cab 2
Time 6. Customer 19 assigned in a pool as second passenger to Cab 2 (method LCM)
Time 7. Customer 18 picked up by Cab 2
Time 7. tempDemand: 20,
Time 7. Customers in pool:
Time 7. Customer 20 assigned to and picked up by Cab 1 (method OPT)
"""
# the Java strings "tempDemand: ", "Customers in pool: " and every "id, " end in a blank; the literal above leaves the blank at
# the end of a line out (it would be invisible there), it is put back here
HAND_LINES = [l + " " if l.endswith((":", ",")) else l for l in HAND_TEXT.split("\n")[:-1]]


def as_records(ev):
    return np.asarray(ev, np.int32).reshape(-1, 8)


_RUNS = {}


def event_run(name, rows=None, world=None, ticks=None, events=True):
    """Simulator(events=...) + OracleTickBackend on world `name` of sim_worlds.WORLDS (or `world` with `rows`), once:
    {"rows", "world", "ticks": [per tick: t, line, ev (its records, (n, 8) int32), res (the backend's decisions or None),
    n_dem, n_sup, n_d2, state, m], "log", "m"}"""
    key = (name, events)
    if key in _RUNS:
        return _RUNS[key]
    import sim_backend
    from taxidispatcher_amd import simulator
    w = sw.WORLDS[name] if world is None else world
    rows = sw.gen_demand(**w) if rows is None else rows
    with pytest.MonkeyPatch.context() as mp:
        sw.patch_constants(mp, w)
        be = sim_backend.OracleTickBackend()
        sim = simulator.Simulator(rows, be, n_cabs=w["cabs"], events=events)
        cur = {}
        real_tick, real_dem, real_sup = be.tick, sim.create_temp_demand, sim.create_temp_supply

        def tick(cab_to, dem_from):
            res = real_tick(cab_to, dem_from)
            cur.update(res=res, n_d2=len(dem_from))
            return res

        def temp_demand(t):
            out = real_dem(t)
            cur.update(n_dem=len(out))
            return out

        def temp_supply():
            out = real_sup()
            cur.update(n_sup=len(out))
            return out
        be.tick, sim.create_temp_demand, sim.create_temp_supply = tick, temp_demand, temp_supply
        out = []
        for t in range(w["ticks"] if ticks is None else ticks):
            cur.clear()
            cur.update(res=None, n_dem=0, n_sup=0, n_d2=0)
            n0 = len(sim.events)
            line = sim.tick(t)
            if line is not None:
                sim.log.append(line)
            out.append(dict(t=t, line=line, ev=as_records(sim.events[n0:]), res=cur["res"], n_dem=cur["n_dem"], n_sup=cur["n_sup"],
                            n_d2=cur["n_d2"], state=sw.state_of(sim), m=copy.deepcopy(sim.m)))
    _RUNS[key] = dict(rows=rows, world=w, ticks=out, log=list(sim.log), m=dict(sim.m))
    return _RUNS[key]


def hand_run(events=True):
    return event_run("hand", rows=HAND_ROWS, world=HAND, events=events)


def count(ev, kind, method=None):
    sel = ev[:, 2] == kind
    if method is not None:
        sel &= ev[:, 3] == method
    return int(sel.sum())


def check_record_shape(ev, t):
    """the fixed words of every record: its tick, world 0, a kind, the method where the kind has one, -1 in unused fields"""
    used = {PICKED_UP: (1, 1, 0), CAB_FREE: (0, 1, 1), DROPPED: (1, 0, 0), TEMP_DEMAND: (0, 0, 1), TEMP_DEMAND_ID: (1, 0, 0), POOL: (0, 0, 1),
            POOL_PAIR: (1, 0, 1), ASSIGNED_PICKED: (1, 1, None), HEADING: (1, 1, 0), ASSIGNED_LCM: (1, 1, 0), POOLED_SECOND: (1, 1, 0)}
    for r in ev.tolist():
        assert r[0] == t and r[1] == 0 and r[7] == 0 and r[2] in used, r
        assert (r[3] in (LCM, OPT)) == (r[2] in (ASSIGNED_PICKED, HEADING, POOLED_SECOND)) and (r[3] in (0, LCM, OPT)), r
        for word, u in zip(r[4:7], used[r[2]]):
            assert u is None or (word >= 0 if u else word == -1), r


def check_invariants(ticks, final_m):
    """per tick and at the end: the records against the simulog_solv line and the metrics (both made without them)"""
    tot = {k: 0 for k in ALL_KINDS}
    heading, loaded = set(), {}
    for rec in ticks:
        ev, line, t = rec["ev"], rec["line"], rec["t"]
        check_record_shape(ev, t)
        hdr = ev[ev[:, 2] == TEMP_DEMAND]
        assert hdr.shape[0] == 1, t                                                     # once per tick, also for an empty list
        n_dem = int(re.search(r"demand=(\d+)", line).group(1)) if line else 0
        assert int(hdr[0, 6]) == n_dem == count(ev, TEMP_DEMAND_ID), t
        m = re.search(r"LCM n_pairs=(\d+)", line or "")
        n_pairs = int(m.group(1)) if m else 0
        assert count(ev, ASSIGNED_LCM) == count(ev, ASSIGNED_PICKED, LCM) + count(ev, HEADING, LCM) == n_pairs, t
        m = re.search(r"OPT count=(-?\d+)", line or "")
        assert count(ev, ASSIGNED_PICKED, OPT) + count(ev, HEADING, OPT) == (int(m.group(1)) if m else 0), t
        pools = ev[ev[:, 2] == POOL]
        supply = int(re.search(r"supply=(\d+)", line).group(1)) if line else 0
        assert pools.shape[0] == (1 if line and supply > 0 else 0), t                    # where findPool ran
        if pools.shape[0]:
            assert int(pools[0, 6]) == count(ev, POOL_PAIR), t
        for k in ALL_KINDS:
            tot[k] += count(ev, k)
        assert tot[DROPPED] == rec["m"]["total_dropped"], t
        assert tot[POOLED_SECOND] == rec["m"]["total_second_passengers"], t
        assert tot[PICKED_UP] + tot[ASSIGNED_PICKED] + tot[POOLED_SECOND] == rec["m"]["total_pickup_numb"], t
        for r in ev.tolist():
            kind, cust, cab = r[2], r[4], r[5]
            if kind == HEADING:
                heading.add((cust, cab))
            elif kind == PICKED_UP:
                assert (cust, cab) in heading, (t, r)                                    # an earlier HEADING of the same customer and cab
                loaded[cab] = True
            elif kind == ASSIGNED_PICKED:
                loaded[cab] = True
            elif kind == CAB_FREE:
                assert loaded.get(cab), (t, r)                                           # follows a record that loaded that cab
                loaded[cab] = False
    assert tot[DROPPED] == final_m["total_dropped"] and tot[POOLED_SECOND] == final_m["total_second_passengers"]
    return tot


def kinds_mask(kinds):
    return sum(1 << k for k in kinds)
