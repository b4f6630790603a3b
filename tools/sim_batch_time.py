"""Times DeviceSimulatorBatch.run (one td_simb_step per tick for B worlds) against a loop that ticks B DeviceSimulator
handles (one td_sim_step per world and tick) over the same worlds in the same process.

    python tools/sim_batch_time.py [--out profiles/sim_batch/sim_batch_time.json] [--reps 5] [--only small_a,small_w,golden]
    python tools/sim_batch_time.py --one-run small_a --batch 64      (one batched run and nothing else: for a kernel trace)

Shapes (name: worlds, city, ticks):
  small_a   64 worlds, 12 stands, DROP_TIME 4, MAX_NON_LCM 16, 150 cabs, about 40 requests per tick, 40 ticks
  small_w   64 worlds, 50 stands, DROP_TIME 10, MAX_NON_LCM 600, 150 cabs, about 40 requests per tick, 40 ticks
  golden    8 worlds of the committed demand file with 900 .. 1300 cabs, Simulator.java's constants, 120 ticks
Every world of a shape has its own seeded request file (golden: its own fleet size).  Host clock around synchronous calls;
a run creates its handles, ticks them and reads the metrics; each side is warmed up once, then the median of --reps runs.
The metrics of both sides are printed; they need not be equal (td_tick and td_tick_batched may break ties differently).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIG = 250000


def gen_demand(stands, per_tick, ticks, span, max_wait, seed):
    """gendemand.py's shape: per tick up to 2 * per_tick requests, a short trip of up to `span` stands either way (a trip that
    would leave the line starts at that end of the line and goes to stand 0), half of the customers want the cab now"""
    rng = np.random.default_rng(seed)
    rows = []
    for t in range(ticks):
        for _ in range(int(rng.integers(0, 2 * per_tick))):
            frm, step = int(rng.integers(0, stands)), int(rng.integers(-span, span))
            if step == 0:
                continue
            to = frm + step
            if to >= stands:
                frm, to = stands - 1, 0
            elif to < 0:
                continue
            wait = int(rng.integers(0, max_wait))
            rows.append((len(rows), frm, to, t, t + (0 if wait < max_wait // 2 else wait)))
    return np.asarray(rows, np.int64).reshape(-1, 5)


def shape(name, batch=None):
    """-> (tables, fleets, city keywords, ticks)"""
    if name in ("small_a", "small_w"):
        city = dict(n_stands=12, drop_time=4, max_non_lcm=16) if name == "small_a" else dict(n_stands=50, drop_time=10, max_non_lcm=600)
        B = batch or 64
        tables = [gen_demand(city["n_stands"], 46, 40, 4, 10, 100 + b) for b in range(B)]
        return tables, [150] * B, dict(city, big_cost=BIG), 40
    if name == "golden":
        from taxidispatcher_amd import simulator
        rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
        B = batch or 8
        fleets = [int(v) for v in np.linspace(900, 1300, B).round()]
        return [rows] * B, fleets, dict(n_stands=50, drop_time=10, max_non_lcm=600, big_cost=BIG), 120
    raise ValueError(name)


def run_batched(td, tables, fleets, city, ticks):
    sim = td.DeviceSimulatorBatch(tables, fleets, **city)
    sim.run(ticks)
    m = sim.m
    sim.close()
    return m


def run_loop(td, tables, fleets, city, ticks):
    sims = [td.DeviceSimulator(rows, n_cabs=n, **city) for rows, n in zip(tables, fleets)]
    for t in range(ticks):
        for sim in sims:
            line = sim.tick(t)
            if line is not None:
                sim.log.append(line)
    m = [sim.m for sim in sims]
    for sim in sims:
        sim.close()
    return m


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), out


def summary(ms):
    keys = ("total_dropped", "total_pickup_numb", "total_pickup_time", "total_LCM_used", "max_model_size", "max_POOL_size",
            "total_second_passengers")
    return {k: int(sum(m[k] for m in ms)) if k.startswith("total") else int(max(m[k] for m in ms)) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_batch", "sim_batch_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="small_a,small_w,golden")
    ap.add_argument("--one-run", default=None, help="run this shape batched once and exit")
    ap.add_argument("--batch", type=int, default=None, help="number of worlds (default: the shape's)")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    if a.one_run:
        tables, fleets, city, ticks = shape(a.one_run, a.batch)
        run_batched(td, tables, fleets, city, ticks)
        print(json.dumps({"shape": a.one_run, "B": len(fleets), "ticks": ticks, "runs": 1}))
        return
    results = []
    for name in a.only.split(","):
        tables, fleets, city, ticks = shape(name, a.batch)
        row = {"shape": name, "B": len(fleets), "ticks": ticks, "cabs": [min(fleets), max(fleets)],
               "requests_per_world": [int(min(t.shape[0] for t in tables)), int(max(t.shape[0] for t in tables))], **city}
        run_batched(td, tables, fleets, city, ticks)      # warm-up of both sides
        run_loop(td, tables, fleets, city, ticks)
        row["batched_ms"], row["batched_min_ms"], row["batched_max_ms"], mb = timed(lambda: run_batched(td, tables, fleets, city, ticks), a.reps)
        row["loop_ms"], row["loop_min_ms"], row["loop_max_ms"], ml = timed(lambda: run_loop(td, tables, fleets, city, ticks), a.reps)
        row["loop_over_batched"] = row["loop_ms"] / row["batched_ms"]
        row["batched_ms_per_tick"] = row["batched_ms"] / ticks
        row["loop_ms_per_tick"] = row["loop_ms"] / ticks
        row["metrics_batched"], row["metrics_loop"] = summary(mb), summary(ml)
        row["metrics_equal"] = mb == ml
        print(json.dumps(row), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps,
            "timing": "host clock around synchronous calls; a run = create the handle(s), tick, read the metrics, destroy; median of "
                      "reps after one warm-up run of each side",
            "results": results}
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
