"""Worlds for the batched simulator handle on ONE shared distance table (td_simb_create_dist, DeviceSimulatorBatch(dist=...)):
three families that share a city and a table each, their CPU comparator runs (sim_dist_worlds.run_world: Simulator +
OracleDistTickBackend on the table), and the host backend whose decisions are td_tick_batched's and td_pool2_batched's on
ONE model with the table -- what td_simb_step uses for every world of a table batch at once.  The records have the shape
sim_batch_worlds' have, so its line_of / decisions_of / assert_same_state serve here too."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sim_batch_worlds as sb
import sim_dist_worlds as sd
import sim_worlds as sw

BIG_COST = sw.BIG_COST
POOL_NMAX = sb.POOL_NMAX

# 65 stands: a third flag word
CITY_D = dict(drop_time=6, max_non_lcm=16, span=4, max_wait=10, ticks=30)
CITY_R = dict(drop_time=4, max_non_lcm=16, span=4, max_wait=10, ticks=30)
# 2100 stands = 66 flag words: the second stride of the near kernel
CITY_H = dict(drop_time=10, max_non_lcm=64, span=6, max_wait=10, ticks=4)
TABLES = {"D": lambda: sd.oneway(sd.grid(13, 5), 4, 2), "R": lambda: sd.ring(12), "H": lambda: sd.permuted(sd.ring(2100), 7)}
CITIES = {"D": CITY_D, "R": CITY_R, "H": CITY_H}
FAMILIES = {
    "D": {
        "D1": dict(cabs=1, per_tick=12, seed=21),
        "D7": dict(cabs=7, per_tick=12, seed=22),
        "D40": dict(cabs=40, per_tick=12, seed=23),
        "D200": dict(cabs=200, per_tick=60, seed=24),
    },
    "R": {
        "R1": dict(cabs=1, per_tick=3, seed=31),
        "R7": dict(cabs=7, per_tick=3, seed=32),
        "R40": dict(cabs=40, per_tick=12, seed=33),
        "R90": dict(cabs=90, per_tick=30, seed=34),
    },
    # H1025 first: without the padded grid the next world would begin inside a 1024-thread workgroup
    "H": {
        "H1025": dict(cabs=1025, per_tick=150, seed=41),
        "H1024": dict(cabs=1024, per_tick=150, seed=42),
        "H300": dict(cabs=300, per_tick=40, seed=43),
        "H1": dict(cabs=1, per_tick=2, seed=44),
    },
}
EMPTY_CABS = 3          # family D's fifth world: an empty request table
N_REQUESTS = dict(D1=348, D7=260, D40=446, D200=2008, R1=77, R7=84, R40=356, R90=823, H1025=489, H1024=570, H300=139, H1=8)

_TABLES, _FAMILIES = {}, {}


def table(which):
    if which not in _TABLES:
        _TABLES[which] = np.ascontiguousarray(TABLES[which](), dtype=np.int32)
        _TABLES[which].setflags(write=False)
    return _TABLES[which]


def city(which):
    """the family's city with `stands` filled in (what sw.patch_constants reads)"""
    return dict(CITIES[which], stands=int(table(which).shape[0]))


def family(which):
    """-> (city, table, [(name, run)] in batch order); family D ends with the world without requests.  Computed once."""
    if which in _FAMILIES:
        return _FAMILIES[which]
    D, c = table(which), city(which)
    runs = []
    for name, own in FAMILIES[which].items():
        w = dict(c, **own)
        rows = sd.gen_demand(D, **w)
        assert rows.shape[0] == N_REQUESTS[name], (name, rows.shape)
        runs.append((name, sd.run_world(rows, D, w)))
    if which == "D":
        runs.append(("Dempty", sb.empty_run(c, EMPTY_CABS)))
    _FAMILIES[which] = (c, D, runs)
    return _FAMILIES[which]


def max_demand(runs):
    return max(rec["n_dem"] for _, r in runs for rec in r["ticks"])


def check_cover():
    """the three families reach every branch of the world model, both directions of the near test and the second stride of the
    near kernel on the CPU: a change to a generator cannot empty the tests"""
    _, _, runs_d = family("D")
    _, _, runs_r = family("R")
    _, _, runs_h = family("H")
    d, r, h = dict(runs_d), dict(runs_r), dict(runs_h)
    cov_d = [run["cover"] for n, run in runs_d if n != "Dempty"]
    cov_r = [run["cover"] for _, run in runs_r]
    for k in ("empty_ticks", "no_lcm", "lcm_ends_on_big", "lcm_then_solver", "assign_and_go", "go_to_pickup", "arrive_empty", "arrive_loaded",
              "second_passengers", "drops", "pool_info_copied"):
        assert sum(c[k] for c in cov_d + cov_r) > 0, k
    assert all(sum(c["cheat"][q] for c in cov_r) > 0 for q in range(3))
    assert d["D40"]["cover"]["lcm_then_solver"] > 0 and r["R40"]["cover"]["lcm_then_solver"] > 0
    assert all(c["dir_dem"] > 0 for c in cov_d)
    assert all(h[n]["cover"]["dir_sup"] > 0 for n in ("H1025", "H1024", "H300"))
    assert all(h[n]["cover"]["hi_dem"] > 0 for n in ("H1025", "H1024"))
    assert max_demand(runs_h) <= 96 and max_demand(runs_d) <= 164           # far under td_simb_step's 2048
    assert all(rec["n_dem"] == 0 for rec in h["H1"]["ticks"])
    d1_empty = [rec["t"] for rec in d["D1"]["ticks"] if rec["n_dem"] == 0]
    assert d["D1"]["cover"]["empty_ticks"] == 27 == len(d1_empty)
    assert all(any(d[n]["ticks"][t]["n_dem"] > 0 for n in ("D7", "D40", "D200")) for t in d1_empty)


def device_batch(td, c, D, runs, only=None, dist=True):
    """DeviceSimulatorBatch over the family's worlds on the table (only: a list of positions -> a smaller batch; dist=False: the
    same worlds on the line)"""
    pick = range(len(runs)) if only is None else only
    return td.DeviceSimulatorBatch([runs[i][1]["rows"] for i in pick], [runs[i][1]["world"]["cabs"] for i in pick], n_stands=c["stands"],
                                   drop_time=c["drop_time"], max_non_lcm=c["max_non_lcm"], big_cost=BIG_COST, dist=D if dist else None)


class BatchedCallsDistBackend:
    """sim_batch_worlds.BatchedCallsBackend on a table: tick is td.tick_batched(..., D, ...) on one model, find_pool
    td.pool2_batched(..., D, ..., optimal=False) on one model"""

    def __init__(self, td, c, D):
        self.td, self.city, self.D = td, c, np.ascontiguousarray(D, dtype=np.int32)

    def tick(self, cab_to, dem_from):
        return self.td.tick_batched([np.asarray(cab_to, np.int32)], [np.asarray(dem_from, np.int32)], self.D, big_cost=BIG_COST,
                                    drop_time=self.city["drop_time"], max_non_lcm=self.city["max_non_lcm"])[0]

    def find_pool(self, frm, to):
        if len(frm) > POOL_NMAX:      # beyond td_pool2_batched's model size: the same greedy through td_pool2, as td_simb_begin does
            from taxidispatcher_amd import dispatch
            return dispatch.find_pool(frm, to, self.D)
        a, b, plan, cost, k, _ = self.td.pool2_batched([np.asarray(frm, np.int32)], [np.asarray(to, np.int32)], self.D, None, optimal=False)
        return [(int(a[0, i]), int(b[0, i]), int(plan[0, i]), int(cost[0, i])) for i in range(int(k[0]))]


def host_world(td, c, D, rows, cabs):
    from taxidispatcher_amd import simulator
    return simulator.Simulator(rows, BatchedCallsDistBackend(td, c, D), n_cabs=cabs, dist=D)


def lockstep(td, mp, c, D, tables, cabs, ticks):
    """DeviceSimulatorBatch(dist=D).tick against one host Simulator(dist=D) per world on the table-aware batched-calls backend,
    with the module constants patched: line by line, then logs, metrics, metrics text and final states; returns (batch, hosts)"""
    sw.patch_constants(mp, c)
    hosts = [host_world(td, c, D, tables[b], cabs[b]) for b in range(len(tables))]
    dev = td.DeviceSimulatorBatch(tables, cabs, n_stands=c["stands"], drop_time=c["drop_time"], max_non_lcm=c["max_non_lcm"],
                                  big_cost=BIG_COST, dist=D)
    for t in range(ticks):
        want = [sim.tick(t) for sim in hosts]
        for sim, line in zip(hosts, want):
            if line is not None:
                sim.log.append(line)
        got = dev.tick(t)
        got = [None] * dev.batch if got is None else got
        for b in range(dev.batch):
            assert got[b] == want[b], (t, b)
            if got[b] is not None:
                dev.logs[b].append(got[b])
    m = dev.m
    for b, sim in enumerate(hosts):
        assert dev.logs[b] == sim.log and m[b] == sim.m, b
        assert dev.metrics_text(b) == sim.metrics_text(), b
        sb.assert_same_state(dev, b, sw.state_of(sim), "final")
    return dev, hosts
