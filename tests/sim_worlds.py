"""Small simulator worlds for the device-resident world (td_sim_*, DeviceSimulator): a seeded demand generator in the
shape of the reference's gendemand.py, the table of worlds, and the CPU comparator run (Simulator + OracleTickBackend
with the module constants patched) that records, per tick, what the device world is compared with."""
import copy

import numpy as np
import pytest

BIG_COST = 250000

# name: stands, cabs, drop_time, max_non_lcm, about requests / tick, ticks, trip span, max wait, seed
WORLDS = {
    "tiny": dict(stands=5, cabs=7, drop_time=3, max_non_lcm=4, per_tick=3, ticks=40, span=3, max_wait=6, seed=1),
    "small": dict(stands=12, cabs=40, drop_time=4, max_non_lcm=16, per_tick=12, ticks=40, span=4, max_wait=10, seed=2),
    "mid": dict(stands=50, cabs=150, drop_time=10, max_non_lcm=64, per_tick=40, ticks=40, span=4, max_wait=10, seed=3),
    # beyond the 64 stands of td_tick's stands LCM: the matrix LCM
    "mid65": dict(stands=65, cabs=200, drop_time=10, max_non_lcm=64, per_tick=60, ticks=30, span=4, max_wait=10, seed=4),
    # the supply list exactly at, and one past, a 1024-thread workgroup
    "wide1024": dict(stands=50, cabs=1024, drop_time=10, max_non_lcm=600, per_tick=500, ticks=3, span=4, max_wait=10, seed=5),
    "wide1025": dict(stands=50, cabs=1025, drop_time=10, max_non_lcm=600, per_tick=500, ticks=3, span=4, max_wait=10, seed=5),
}
FIRST_FOUR = ("tiny", "small", "mid", "mid65")
WIDE = ("wide1024", "wide1025")


def gen_demand(stands, per_tick, ticks, span, max_wait, seed, **_):
    """rows (id, from, to, time, at): per tick up to 2 * per_tick requests, a short trip of up to `span` stands either way
    (none of length 0; a trip that would leave the line starts at that end of the line and goes to stand 0, as the
    reference's generator has it), half of the customers want the cab now, the rest within max_wait ticks"""
    rng = np.random.default_rng(seed)
    rows = []
    for time in range(ticks):
        for _k in range(int(rng.integers(0, 2 * per_tick))):
            frm = int(rng.integers(0, stands))
            step = int(rng.integers(-span, span))
            if step == 0:
                continue
            to = frm + step
            if to >= stands:
                frm, to = stands - 1, 0
            elif to < 0:
                frm, to = 0, 0
            if frm == to:
                continue
            wait = int(rng.integers(0, max_wait))
            if wait < max_wait // 2:
                wait = 0
            rows.append((len(rows), frm, to, time, time + wait))
    return np.asarray(rows, np.int64).reshape(-1, 5)


def patch_constants(mp, w):
    """the constants are module globals read at call time"""
    import sim_backend
    from taxidispatcher_amd import simulator
    mp.setattr(simulator, "N_STANDS", w["stands"])
    mp.setattr(simulator, "DROP_TIME", w["drop_time"])
    mp.setattr(simulator, "MAX_NON_LCM", w["max_non_lcm"])
    mp.setattr(sim_backend, "DROP_TIME", w["drop_time"])
    mp.setattr(sim_backend, "MAX_NON_LCM", w["max_non_lcm"])


def state_of(sim):
    return {k: np.asarray(getattr(sim, k)).copy() for k in ("c_from", "c_to", "c_clnt", "c_onboard", "c_start", "d_cab", "d_pick",
                                                            "d_pool_id", "d_pool_plan", "d_pool_cost")}


_RUNS = {}


def oracle_run(name):
    """Simulator + OracleTickBackend on world `name`, computed once: {"rows", "log", "ticks": [per tick dict], "cover": {...}}.
    A tick's dict: t, line, n_dem (before pooling; 0 = no demand), n_sup, cab_to, dem_from (the model, after pooling),
    res (the backend's result, None when it was not called), state, m."""
    if name in _RUNS:
        return _RUNS[name]
    import sim_backend
    from taxidispatcher_amd import simulator
    w = WORLDS[name]
    rows = gen_demand(**w)
    cover = dict(empty_ticks=0, no_lcm=0, lcm_ends_on_big=0, lcm_then_solver=0, assign_and_go=0, go_to_pickup=0, cheat=[0, 0, 0],
                 arrive_empty=0, arrive_loaded=0)
    with pytest.MonkeyPatch.context() as mp:
        patch_constants(mp, w)
        real_cheat = simulator.cheat_a_bit

        def cheat(frm, cost):
            cover["cheat"][0 if frm + cost < w["stands"] else (1 if frm - cost < 0 else 2)] += 1
            return real_cheat(frm, cost)
        mp.setattr(simulator, "cheat_a_bit", cheat)
        be = sim_backend.OracleTickBackend()
        sim = simulator.Simulator(rows, be, n_cabs=w["cabs"])
        cur = {}
        real_tick, real_dem, real_sup = be.tick, sim.create_temp_demand, sim.create_temp_supply
        real_arrive, real_go, real_pick = sim.check_if_cab_at_destination, sim._assign_to_cab_and_go, sim._go_to_pickup

        def tick(cab_to, dem_from):
            res = real_tick(cab_to, dem_from)
            cur.update(cab_to=list(cab_to), dem_from=list(dem_from), res=res)
            return res

        def temp_demand(t):
            out = real_dem(t)
            cur.update(n_dem=len(out), dem_from=[r[1] for r in out])
            return out

        def temp_supply():
            out = real_sup()
            cur.update(n_sup=len(out))
            return out

        def arrive(t):
            moving = (sim.c_from != sim.c_to) & (np.abs(sim.c_from - sim.c_to) == t - sim.c_start)
            cover["arrive_empty"] += int((moving & (sim.c_onboard == 0)).sum())
            cover["arrive_loaded"] += int((moving & (sim.c_onboard != 0)).sum())
            return real_arrive(t)

        def go(*a):
            cover["assign_and_go"] += 1
            return real_go(*a)

        def pick(*a):
            cover["go_to_pickup"] += 1
            return real_pick(*a)
        be.tick, sim.create_temp_demand, sim.create_temp_supply = tick, temp_demand, temp_supply
        sim.check_if_cab_at_destination, sim._assign_to_cab_and_go, sim._go_to_pickup = arrive, go, pick
        ticks = []
        for t in range(w["ticks"]):
            cur.clear()
            cur.update(n_dem=0, n_sup=0, cab_to=[], dem_from=[], res=None)
            line = sim.tick(t)
            if line is not None:
                sim.log.append(line)
            if line is None:
                cover["empty_ticks"] += 1
            elif cur["res"] is not None and "LCM" not in line:
                cover["no_lcm"] += 1
            elif cur["res"] is not None and "OPT" not in line:
                cover["lcm_ends_on_big"] += 1
            elif cur["res"] is not None:
                cover["lcm_then_solver"] += 1
            ticks.append(dict(t=t, line=line, n_dem=cur["n_dem"], n_sup=cur["n_sup"], cab_to=cur["cab_to"], dem_from=cur["dem_from"],
                              res=cur["res"], state=state_of(sim), m=copy.deepcopy(sim.m)))
        cover.update(second_passengers=sim.m["total_second_passengers"], drops=sim.m["total_dropped"],
                     pool_info_copied=int((sim.d_pool_id != -1).sum()))
    _RUNS[name] = dict(rows=rows, log=list(sim.log), ticks=ticks, cover=cover, world=w)
    return _RUNS[name]
