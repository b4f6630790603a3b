"""Worlds for the batched simulator handle (td_simb_*, DeviceSimulatorBatch): two families that share a city each, their
CPU comparator runs (sim_worlds.oracle_run on names registered for the length of the call), and the host backend whose
decisions are td_tick_batched's and td_pool2_batched's on ONE model -- what td_simb_step uses for every world at once."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sim_worlds as sw

BIG_COST = sw.BIG_COST
POOL_NMAX = 2048        # td_pool2_batched's largest model = td_simb_step's limit on a world's requests before pooling

CITY_A = dict(stands=12, drop_time=4, max_non_lcm=16, span=4, max_wait=10, ticks=30)
CITY_W = dict(stands=50, drop_time=10, max_non_lcm=600, span=4, max_wait=10, ticks=3)
FAMILY_A = {
    "A1": dict(CITY_A, cabs=1, per_tick=12, seed=11),
    "A7": dict(CITY_A, cabs=7, per_tick=12, seed=12),
    "A40": dict(CITY_A, cabs=40, per_tick=12, seed=13),
    "A90": dict(CITY_A, cabs=90, per_tick=30, seed=14),
}
EMPTY_CABS = 3          # family A's fifth world: an empty request table
# W1025 first: without padding the next world would begin inside a 1024-thread workgroup
FAMILY_W = {
    "W1025": dict(CITY_W, cabs=1025, per_tick=500, seed=5),
    "W1024": dict(CITY_W, cabs=1024, per_tick=500, seed=6),
    "W150": dict(CITY_W, cabs=150, per_tick=40, seed=7),
    "W1": dict(CITY_W, cabs=1, per_tick=2, seed=8),
}
N_REQUESTS = dict(A1=257, A7=313, A40=323, A90=667, W1025=1690, W1024=1479, W150=144, W1=4)


def family_run(name, w):
    """sim_worlds.oracle_run of a world of this module: the name is in sim_worlds.WORLDS only while the run is made"""
    key = "simb_" + name
    sw.WORLDS[key] = w
    try:
        run = sw.oracle_run(key)
    finally:
        del sw.WORLDS[key]
    assert run["rows"].shape[0] == N_REQUESTS[name], (name, run["rows"].shape)
    return run


def empty_run(city, cabs):
    """the record of a world without requests: no tick has demand, nothing ever moves"""
    from taxidispatcher_amd import simulator
    sim = simulator.Simulator(np.zeros((0, 5), np.int64), backend=object(), n_cabs=cabs)
    sim.c_from = np.arange(cabs, dtype=np.int64) % city["stands"]
    sim.c_to = sim.c_from.copy()
    ticks = [dict(t=t, line=None, n_dem=0, n_sup=0, cab_to=[], dem_from=[], res=None, state=sw.state_of(sim), m=dict(sim.m))
             for t in range(city["ticks"])]
    return dict(rows=np.zeros((0, 5), np.int64), log=[], ticks=ticks, cover={}, world=dict(city, cabs=cabs))


_FAMILIES = {}


def family(which):
    """-> (city, [(name, run)] in batch order); family A ends with the world without requests"""
    if which in _FAMILIES:
        return _FAMILIES[which]
    fam, city = (FAMILY_A, CITY_A) if which == "A" else (FAMILY_W, CITY_W)
    runs = [(name, family_run(name, w)) for name, w in fam.items()]
    if which == "A":
        runs.append(("Aempty", empty_run(city, EMPTY_CABS)))
        check_cover_a(dict(runs))
    else:
        check_shape_w(dict(runs))
    _FAMILIES[which] = (city, runs)
    return _FAMILIES[which]


def check_cover_a(runs):
    """family A reaches every branch of the world model on the CPU: a change to the generator cannot empty the tests"""
    cov = [r["cover"] for n, r in runs.items() if n != "Aempty"]
    tot = lambda k: sum(c[k] for c in cov)
    assert runs["A1"]["cover"]["empty_ticks"] == 21 and runs["A1"]["cover"]["drops"] == 191
    a1_empty = [rec["t"] for rec in runs["A1"]["ticks"] if rec["n_dem"] == 0]
    assert any(runs[n]["ticks"][t]["n_dem"] > 0 for t in a1_empty for n in ("A7", "A40", "A90"))
    c7 = runs["A7"]["cover"]
    assert (c7["no_lcm"], c7["lcm_ends_on_big"], c7["lcm_then_solver"]) == (23, 2, 3)
    for k in ("empty_ticks", "no_lcm", "lcm_ends_on_big", "lcm_then_solver", "assign_and_go", "go_to_pickup", "arrive_empty", "arrive_loaded",
              "second_passengers", "drops"):
        assert tot(k) > 0, k
    assert all(sum(c["cheat"][q] for c in cov) > 0 for q in range(3))
    assert all(runs[n]["cover"]["pool_info_copied"] > 0 for n in ("A1", "A7", "A40"))


def check_shape_w(runs):
    sizes = [max(len(rec["cab_to"]), len(rec["dem_from"])) for rec in runs["W1025"]["ticks"]]
    assert max(sizes) > CITY_W["max_non_lcm"] and any(len(rec["cab_to"]) == 1025 for rec in runs["W1025"]["ticks"])
    assert max(rec["n_dem"] for r in runs.values() for rec in r["ticks"]) <= 369
    assert all(rec["n_dem"] == 0 for rec in runs["W1"]["ticks"])
    assert runs["W1025"]["cover"]["lcm_then_solver"] + runs["W1025"]["cover"]["lcm_ends_on_big"] > 0


def device_batch(td, city, runs, only=None):
    """DeviceSimulatorBatch over the family's worlds (only: a list of positions -> a smaller batch)"""
    pick = range(len(runs)) if only is None else only
    return td.DeviceSimulatorBatch([runs[i][1]["rows"] for i in pick], [runs[i][1]["world"]["cabs"] for i in pick], n_stands=city["stands"],
                                   drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"], big_cost=BIG_COST)


def decisions_of(rec):
    res = rec["res"]
    return None if res is None else (res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])


def line_of(dev, city, rec, info, opt):
    """the log line of a trace-driven tick (test_trace_driven_against_the_oracle's rule)"""
    if rec["n_dem"] == 0:
        return None
    res = rec["res"]
    if res is None:
        return dev.format_line(rec["t"], [1, rec["n_dem"], 0, 0, 0, 0, 0, 0, opt])
    lcm = max(int(info[2]), int(info[3])) > city["max_non_lcm"]
    return dev.format_line(rec["t"], [1, rec["n_dem"], rec["n_sup"], lcm, len(res["lcm_rows"]), lcm and res["solved"], len(res["kept_dems"]),
                                      len(res["kept_cabs"]), opt])


def assert_same_state(dev, b, host_state, where):
    got = dev.state(b)
    for k, v in host_state.items():
        assert np.array_equal(got[k], v), (where, b, k, np.nonzero(got[k] != v)[0][:8].tolist())


class BatchedCallsBackend:
    """Simulator backend whose tick is td.tick_batched on one model and whose find_pool is td.pool2_batched(optimal=False)
    on one model: the two calls td_simb_step makes for all worlds at once (a model's result does not depend on the batch)"""

    def __init__(self, td, city):
        self.td, self.city = td, city

    def tick(self, cab_to, dem_from):
        return self.td.tick_batched([np.asarray(cab_to, np.int32)], [np.asarray(dem_from, np.int32)], None, big_cost=BIG_COST,
                                    drop_time=self.city["drop_time"], max_non_lcm=self.city["max_non_lcm"])[0]

    def find_pool(self, frm, to):
        if len(frm) > POOL_NMAX:      # beyond td_pool2_batched's model size: the same greedy through td_pool2, as td_simb_begin does
            from taxidispatcher_amd import dispatch
            return dispatch.find_pool(frm, to, None)
        a, b, plan, cost, k, _ = self.td.pool2_batched([np.asarray(frm, np.int32)], [np.asarray(to, np.int32)], None, None, optimal=False)
        return [(int(a[0, i]), int(b[0, i]), int(plan[0, i]), int(cost[0, i])) for i in range(int(k[0]))]


def split_tick(td, dev, city, t):
    """one tick of every world through begin / model / td.tick_batched / apply: the way the header prescribes for a tick that
    td_simb_step refuses (a world with more than 2048 requests before pooling); -> the B log lines, or None"""
    info = dev.begin(t)
    if not info[:, 0].any():
        return None
    cab_off, cab_to, dem_off, dem_from = dev.model()
    # a world without supply has no model to solve: td_simb_step leaves it out of the call
    d_off = np.zeros_like(dem_off)
    d_off[1:] = np.cumsum([dem_off[b + 1] - dem_off[b] if info[b, 2] else 0 for b in range(dev.batch)])
    dems = np.concatenate([dem_from[dem_off[b]:dem_off[b + 1]] if info[b, 2] else dem_from[:0] for b in range(dev.batch)])
    res = td.tick_batched((cab_to, cab_off), (dems, d_off), None, big_cost=BIG_COST, drop_time=city["drop_time"],
                          max_non_lcm=city["max_non_lcm"])
    opt = dev.apply([(r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"]) for r in res])
    lines = []
    for b in range(dev.batch):
        n_s, n_d = int(info[b, 2]), int(info[b, 3])
        lcm = n_s > 0 and max(n_s, n_d) > city["max_non_lcm"]
        k = len(res[b]["lcm_rows"]) if lcm else 0
        lines.append(dev.format_line(t, [info[b, 0], info[b, 1], n_s, lcm, k, lcm and res[b]["solved"], n_d - k if n_s else 0, n_s - k,
                                         opt[b]]))
    return lines


def host_world(td, city, rows, cabs):
    from taxidispatcher_amd import simulator
    return simulator.Simulator(rows, BatchedCallsBackend(td, city), n_cabs=cabs)


def lockstep(td, mp, city, tables, cabs, ticks, hosts_for=None):
    """DeviceSimulatorBatch.tick (split_tick where td_simb_step's limit is passed) against one host Simulator per world (hosts_for: batch position -> position of the host
    world it must equal; default: its own) with the module constants patched; returns (batch, hosts)"""
    sw.patch_constants(mp, city)
    hosts_for = list(range(len(tables))) if hosts_for is None else hosts_for
    hosts = {h: host_world(td, city, tables[h], cabs[h]) for h in sorted(set(hosts_for))}
    dev = td.DeviceSimulatorBatch(tables, cabs, n_stands=city["stands"], drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"],
                                  big_cost=BIG_COST)
    for t in range(ticks):
        want = {h: sim.tick(t) for h, sim in hosts.items()}
        for h, line in want.items():
            if line is not None:
                hosts[h].log.append(line)
        # a tick in which some world has more requests before pooling than td_simb_step takes goes through the split tick
        over = any(line is not None and int(line.split("demand=")[1].split(",")[0]) > POOL_NMAX for line in want.values())
        got = split_tick(td, dev, city, t) if over else dev.tick(t)
        got = [None] * dev.batch if got is None else got
        for b, h in enumerate(hosts_for):
            assert got[b] == want[h], (t, b)
            if got[b] is not None:
                dev.logs[b].append(got[b])
    m = dev.m
    for b, h in enumerate(hosts_for):
        assert dev.logs[b] == hosts[h].log and m[b] == hosts[h].m, b
        assert dev.metrics_text(b) == hosts[h].metrics_text(), b
        assert_same_state(dev, b, sw.state_of(hosts[h]), "final")
    return dev, hosts
