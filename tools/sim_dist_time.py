"""Times the simulator worlds with and without a stand-to-stand distance table on the committed 120-tick input.

    python tools/sim_dist_time.py [--out profiles/sim_dist/sim_dist_time.json] [--reps 5]
    python tools/sim_dist_time.py --one-run table50 | ring2100      (one run and nothing else: for a kernel trace)

Variants (the committed demand file, 1300 cabs, 50 stands, Simulator.java's constants, 120 ticks):
  line         DeviceSimulator(rows)                                  the line world, |a - b|
  table        DeviceSimulator(rows, dist=line(50))                   the same city as a table (td_sim_create_dist)
  host_table   Simulator(rows, HipTickBackend(dist=...), dist=...)    the Python world around td_pool2 / td_tick with the table
A table world's td_tick takes the matrix LCM (the stands LCM needs dist == NULL), so `table` against `line` is the price of
the table in td_tick and td_pool2 plus the two k_near launches per tick.  Host clock around whole runs that end synchronised
(a run = create, 120 ticks, read the metrics, destroy); one warm-up run per variant, then --reps rounds that alternate the
variants; medians.  Whether the three logs and metrics are equal is reported, not required: the worlds may break ties
between equal optima differently once the solver runs (t = 49 and later).
ring2100 (--one-run only): a one-way ring of 2100 stands, permuted, 2100 cabs, about 400 requests per tick, 20 ticks."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def line(n):
    a = np.arange(n)
    return np.abs(a[:, None] - a[None, :]).astype(np.int32)


def ring_world(n=2100, per_tick=400, ticks=20, span=6, seed=7):
    """-> (table, rows): (b - a) mod n under a seeded permutation of the stands; trips of 1 .. span ticks"""
    rng = np.random.default_rng(seed)
    a = np.arange(n)
    P = rng.permutation(n)
    D = np.empty((n, n), np.int32)
    D[np.ix_(P, P)] = (a[None, :] - a[:, None]) % n
    inv = np.argsort(P)
    rows = []
    for t in range(ticks):
        for _ in range(int(rng.integers(0, 2 * per_tick))):
            frm = int(rng.integers(0, n))
            to = int(P[(inv[frm] + int(rng.integers(1, span + 1))) % n])
            wait = int(rng.integers(0, 10))
            rows.append((len(rows), frm, to, t, t + (0 if wait < 5 else wait)))
    return D, np.asarray(rows, np.int64).reshape(-1, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_dist", "sim_dist_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-run", default=None, choices=("table50", "ring2100"))
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    from taxidispatcher_amd import simulator
    td.init(0)
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    D50 = line(50)

    def device(dist, rows=rows, ticks=120, **kw):
        sim = simulator.DeviceSimulator(rows, dist=dist, **kw)
        log = sim.run(ticks)
        m = sim.m
        sim.close()
        return log, m

    def host_table():
        sim = simulator.Simulator(rows, simulator.HipTickBackend(dist=D50), dist=D50)
        log = sim.run(120)
        td._ffi.check(td._ffi.lib().td_synchronize())
        return log, sim.m

    if a.one_run == "table50":
        log, m = device(D50)
        print(json.dumps({"run": "table50", "ticks": 120, "lines": len(log), "m": m}))
        return
    if a.one_run == "ring2100":
        D, rr = ring_world()
        log, m = device(D, rr, 20, n_cabs=2100)
        print(json.dumps({"run": "ring2100", "ticks": 20, "requests": int(rr.shape[0]), "lines": len(log), "m": m}))
        return
    variants = {"line": lambda: device(None), "table": lambda: device(D50), "host_table": host_table}
    out = {k: fn() for k, fn in variants.items()}                      # warm-up, and the results to compare
    ts = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    res = {k: {"runs_s": [round(v, 4) for v in ts[k]], "median_s": float(np.median(ts[k])), "min_s": min(ts[k]), "max_s": max(ts[k]),
               "ticks_per_s": 120 / float(np.median(ts[k]))} for k in variants}
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "ticks": 120,
            "timing": "host clock around whole runs that end synchronised; one warm-up run per variant, then rounds that alternate the variants",
            "logs_equal": out["line"][0] == out["table"][0] == out["host_table"][0],
            "metrics_equal": out["line"][1] == out["table"][1] == out["host_table"][1],
            "metrics": {k: v[1] for k, v in out.items()}, "results": res}
    print(json.dumps(info, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
