"""Times the pooling policies of the simulator worlds (td_simb_pooling).

    python tools/sim_pool_policy_time.py [--out profiles/sim_pool_policy/sim_pool_policy_time.json] [--reps 3]
    python tools/sim_pool_policy_time.py --one-run --seeds 1       (one batched run and nothing else: for a kernel trace; B = 4 x seeds)

1. worlds: 64 worlds of 150 cabs on 50 stands, 40 ticks, 16 demand seeds x the four policies (none, greedy 1.01, optimal over
   every pair, optimal 1.01) in ONE DeviceSimulatorBatch, against the route that existed before for such a policy: one host
   Simulator per world on HipTickBackend(pool=, max_loss=), i.e. find_pool / find_pool_optimal and td_tick per world and tick.
   Per policy: the time of its 16 host worlds, and the dropped customers, second passengers and pickup time of both routes
   (they need not be equal: td_tick and td_tick_batched may break ties differently, and two optima may be equal).
2. pool2: td_pool2_loss (1.01) on one model of n = 1445 customers on the 50-stand line against td_pool2 on the same customers
   and against td_pool2_batched(batch = 1, optimal = 0, 1.01), which gives the model one workgroup.
3. optimal world: the time per tick of one DeviceSimulator(pool="optimal") whose ticks hold a few hundred requests.
Host clock around synchronous calls; every side is warmed up once, then the median of --reps runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sim_batch_time import BIG, gen_demand, timed

POLICIES = [("none", None), ("greedy", 1.01), ("optimal", None), ("optimal", 1.01)]
CITY = dict(n_stands=50, drop_time=10, max_non_lcm=600, big_cost=BIG)
TICKS, CABS = 40, 150
KEYS = ("total_dropped", "total_second_passengers", "total_pickup_time", "total_pickup_numb", "max_POOL_size")


def worlds(seeds):
    """-> (tables, pools, losses): the four policies on each of `seeds` request files, policy-minor"""
    tables, pools, losses = [], [], []
    for s in range(seeds):
        rows = gen_demand(CITY["n_stands"], 46, TICKS, 4, 10, 100 + s)
        for pool, ml in POLICIES:
            tables.append(rows)
            pools.append(pool)
            losses.append(ml)
    return tables, pools, losses


def run_batched(td, tables, pools, losses):
    sim = td.DeviceSimulatorBatch(tables, [CABS] * len(tables), pool=pools, max_loss=losses, **CITY)
    sim.run(TICKS)
    m = sim.m
    sim.close()
    return m


def run_host(tables, pool, ml):
    """one host Simulator per world (the module's constants are this city's: 50 stands, DROP_TIME 10, MAX_NON_LCM 600)"""
    from taxidispatcher_amd import simulator
    out = []
    for rows in tables:
        sim = simulator.Simulator(rows, simulator.HipTickBackend(pool=pool, max_loss=ml), n_cabs=CABS, pool=pool, max_loss=ml)
        sim.run(TICKS)
        out.append(sim.m)
    return out


def sums(ms):
    return {k: int(max(m[k] for m in ms)) if k.startswith("max") else int(sum(m[k] for m in ms)) for k in KEYS}


def time_worlds(td, seeds, reps):
    tables, pools, losses = worlds(seeds)
    run_batched(td, tables, pools, losses)
    row = {"B": len(tables), "seeds": seeds, "cabs": CABS, "ticks": TICKS, **CITY}
    row["batched_ms"], row["batched_min_ms"], row["batched_max_ms"], mb = timed(lambda: run_batched(td, tables, pools, losses), reps)
    row["batched_ms_per_tick"] = row["batched_ms"] / TICKS
    host_total = 0.0
    row["policies"] = []
    for q, (pool, ml) in enumerate(POLICIES):
        mine = tables[q::4]
        run_host(mine[:1], pool, ml)
        ms, lo, hi, mh = timed(lambda: run_host(mine, pool, ml), reps)
        host_total += ms
        row["policies"].append({"pool": pool, "max_loss": ml, "host_ms_16_worlds": ms, "host_min_ms": lo, "host_max_ms": hi,
                                "device": sums(mb[q::4]), "host": sums(mh)})
    row["host_ms"] = host_total
    row["host_over_batched"] = host_total / row["batched_ms"]
    return row


def time_pool2(td, reps, n=1445):
    rng = np.random.default_rng(1445)
    frm, to = rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 50, n).astype(np.int32)
    calls = {"td_pool2": lambda: td.find_pool(frm, to),
             "td_pool2_loss_1.01": lambda: td.find_pool(frm, to, max_loss=1.01),
             "td_pool2_batched_1_greedy_1.01": lambda: td.pool2_batched([frm], [to], None, 1.01, optimal=False)}
    row = {"n": n, "stands": 50}
    for name, fn in calls.items():
        fn()
        ms, lo, hi, out = timed(fn, max(reps, 5))
        row[name + "_ms"], row[name + "_min_ms"], row[name + "_max_ms"] = ms, lo, hi
        row[name + "_plans"] = len(out) if isinstance(out, list) else int(out[4][0])
        if name != "td_pool2_batched_1_greedy_1.01":
            row[name + "_lcm_path"] = int(td.last_stats()["lcm_path"])
    a = td.find_pool(frm, to, max_loss=1.01)
    o = td.pool2_batched([frm], [to], None, 1.01, optimal=False)
    row["loss_equals_batched"] = a == [(int(o[0][0, i]), int(o[1][0, i]), int(o[2][0, i]), int(o[3][0, i])) for i in range(int(o[4][0]))]
    return row


def time_optimal_world(td, reps, per_tick=120, cabs=600, ticks=12):
    rows = gen_demand(50, per_tick, ticks, 4, 10, 7)
    row = {"cabs": cabs, "ticks": ticks, "requests": int(rows.shape[0])}
    for pool, ml in (("greedy", None), ("greedy", 1.01), ("optimal", None), ("optimal", 1.01)):
        def run():
            sim = td.DeviceSimulator(rows, n_cabs=cabs, pool=pool, max_loss=ml, **CITY)
            biggest, per = 0, []
            for t in range(ticks):
                t0 = time.perf_counter()
                line = sim.tick(t)
                per.append((time.perf_counter() - t0) * 1e3)
                if line is not None:
                    biggest = max(biggest, int(line.split("demand=")[1].split(",")[0]))
            m = sim.m
            sim.close()
            return biggest, per, m
        run()
        ms, lo, hi, (biggest, per, m) = timed(run, reps)
        row["%s_%s" % (pool, ml)] = {"run_ms": ms, "ms_per_tick_mean": ms / ticks, "ms_per_tick_max": float(max(per)), "largest_demand": biggest,
                                     "second_passengers": m["total_second_passengers"], "max_POOL_size": m["max_POOL_size"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_pool_policy", "sim_pool_policy_time.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=16, help="request files; the batch holds 4 worlds per file")
    ap.add_argument("--one-run", action="store_true", help="run the batch once and exit")
    ap.add_argument("--only", default="worlds,pool2,optimal_world")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    if a.one_run:
        tables, pools, losses = worlds(a.seeds)
        run_batched(td, tables, pools, losses)
        print(json.dumps({"B": len(tables), "ticks": TICKS, "runs": 1}))
        return
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps,
            "timing": "host clock around synchronous calls; a run = create the handle(s), tick, read the metrics, destroy; median of reps "
                      "after one warm-up run of each side"}
    for part in a.only.split(","):
        info[part] = {"worlds": lambda: time_worlds(td, a.seeds, a.reps), "pool2": lambda: time_pool2(td, a.reps),
                      "optimal_world": lambda: time_optimal_world(td, a.reps)}[part]()
        print(json.dumps({part: info[part]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
