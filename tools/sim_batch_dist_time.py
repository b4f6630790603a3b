"""Times a batch of worlds on ONE shared distance table (DeviceSimulatorBatch(dist=...), td_simb_create_dist) against the
line batch over the same request files and against a loop over DeviceSimulator(dist=...) handles, in the same process.

    python tools/sim_batch_dist_time.py [--out profiles/sim_batch_dist/sim_batch_dist_time.json] [--rounds 5] [--only line50,grid10x5]
    python tools/sim_batch_dist_time.py --one-run ring2100 --variant table       (one run and nothing else: for a kernel trace)
    python tools/sim_batch_dist_time.py --line-shapes                            (sim_batch_time.py's first two shapes, the line batch alone:
                                                                                  run from two trees in turn to compare two builds)

Shapes (name: worlds, table, city, ticks):
  line50     64 worlds of 150 cabs, line(50) = |a - b|, DROP_TIME 10, MAX_NON_LCM 600, about 40 requests per tick, 40 ticks
  grid10x5   the same on grid(10, 5) (Manhattan distance, 50 stands)
  ring2100   8 worlds of 300 cabs on a permuted one-way ring of 2100 stands (66 flag words), DROP_TIME 10, MAX_NON_LCM 64, 8 ticks
Variants: line (the line batch; on a table that is not the line it simulates another city and serves as the cost baseline
only), table (the table batch), loop (one DeviceSimulator(dist=...) per world, ticked in turn).  Host clock around whole runs
that end synchronised (a run = create the handle(s), tick, read the metrics, destroy); one warm-up run per variant, then
--rounds rounds that alternate the variants; median and min .. max per variant.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BIG = 250000


def line(n):
    a = np.arange(n)
    return np.abs(a[:, None] - a[None, :]).astype(np.int32)


def grid(w, h):
    s = np.arange(w * h)
    x, y = s % w, s // w
    return (np.abs(x[:, None] - x[None, :]) + np.abs(y[:, None] - y[None, :])).astype(np.int32)


def ring_permuted(n, seed):
    a = np.arange(n)
    D = ((a[None, :] - a[:, None]) % n).astype(np.int32)
    P = np.random.default_rng(seed).permutation(n)
    out = np.empty_like(D)
    out[np.ix_(P, P)] = D
    return out


def gen_demand(D, per_tick, ticks, span, max_wait, seed):
    """per tick up to 2 * per_tick requests, `from` uniform over the stands, `to` uniform among the other stands within `span`
    of it on the table, half of the customers want the cab now"""
    rng = np.random.default_rng(seed)
    n = D.shape[0]
    rows = []
    for t in range(ticks):
        for _ in range(int(rng.integers(0, 2 * per_tick))):
            frm = int(rng.integers(0, n))
            ok = D[frm] <= span
            ok[frm] = False
            cand = np.nonzero(ok)[0]
            if cand.size == 0:
                continue
            wait = int(rng.integers(0, max_wait))
            rows.append((len(rows), frm, int(cand[rng.integers(0, cand.size)]), t, t + (0 if wait < max_wait // 2 else wait)))
    return np.asarray(rows, np.int64).reshape(-1, 5)


def shape(name, batch=None):
    """-> (table, request tables, fleets, city keywords, ticks)"""
    if name in ("line50", "grid10x5"):
        D = line(50) if name == "line50" else grid(10, 5)
        B = batch or 64
        return D, [gen_demand(D, 46, 40, 4, 10, 100 + b) for b in range(B)], [150] * B, dict(drop_time=10, max_non_lcm=600, big_cost=BIG), 40
    if name == "ring2100":
        D = ring_permuted(2100, 7)
        B = batch or 8
        return D, [gen_demand(D, 40, 8, 6, 10, 200 + b) for b in range(B)], [300] * B, dict(drop_time=10, max_non_lcm=64, big_cost=BIG), 8
    raise ValueError(name)


def run_batch(td, D, tables, fleets, city, ticks, on_line=False):
    """on_line: the line batch over the same stands and request files"""
    sim = td.DeviceSimulatorBatch(tables, fleets, n_stands=int(D.shape[0]), dist=None if on_line else D, **city)
    sim.run(ticks)
    m = sim.m
    sim.close()
    return m


def run_loop(td, D, tables, fleets, city, ticks):
    sims = [td.DeviceSimulator(rows, n_cabs=n, dist=D, **city) for rows, n in zip(tables, fleets)]
    for t in range(ticks):
        for sim in sims:
            sim.tick(t)
    m = [sim.m for sim in sims]
    for sim in sims:
        sim.close()
    return m


def summary(ms):
    keys = ("total_dropped", "total_pickup_numb", "total_pickup_time", "total_LCM_used", "max_model_size", "max_POOL_size",
            "total_second_passengers")
    return {k: int(sum(m[k] for m in ms)) if k.startswith("total") else int(max(m[k] for m in ms)) for k in keys}


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "runs_ms": [round(float(v), 2) for v in ts]}


def line_shapes(td, rounds):
    """sim_batch_time.py's small_a and small_w as line batches: one warm-up, then `rounds` timed runs each"""
    import sim_batch_time as sbt
    out = {}
    for name in ("small_a", "small_w"):
        tables, fleets, city, ticks = sbt.shape(name)
        sbt.run_batched(td, tables, fleets, city, ticks)
        ts = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            sbt.run_batched(td, tables, fleets, city, ticks)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = stats(ts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_batch_dist", "sim_batch_dist_time.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="line50,grid10x5")
    ap.add_argument("--one-run", default=None, help="run this shape once and exit")
    ap.add_argument("--variant", choices=("line", "table", "loop"), default="table", help="what --one-run runs")
    ap.add_argument("--batch", type=int, default=None, help="number of worlds (default: the shape's)")
    ap.add_argument("--line-shapes", action="store_true", help="time sim_batch_time.py's small_a and small_w line batches and exit")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    if a.line_shapes:
        print(json.dumps({"line_shapes": line_shapes(td, a.rounds)}))
        return
    if a.one_run:
        D, tables, fleets, city, ticks = shape(a.one_run, a.batch)
        run_variant(td, a.variant, D, tables, fleets, city, ticks)
        print(json.dumps({"shape": a.one_run, "variant": a.variant, "B": len(fleets), "ticks": ticks, "runs": 1}))
        return
    results = []
    for name in a.only.split(","):
        D, tables, fleets, city, ticks = shape(name, a.batch)
        row = {"shape": name, "B": len(fleets), "ticks": ticks, "stands": int(D.shape[0]), "cabs": [min(fleets), max(fleets)],
               "requests_per_world": [int(min(t.shape[0] for t in tables)), int(max(t.shape[0] for t in tables))], **city}
        names = ("line", "table", "loop")
        for v in names:                                   # one warm-up run per variant
            run_variant(td, v, D, tables, fleets, city, ticks)
        ts, ms = {v: [] for v in names}, {}
        for _ in range(a.rounds):                         # the rounds alternate the variants
            for v in names:
                t0 = time.perf_counter()
                ms[v] = run_variant(td, v, D, tables, fleets, city, ticks)
                ts[v].append((time.perf_counter() - t0) * 1e3)
        for v in names:
            row[v] = dict(stats(ts[v]), ms_per_tick=float(np.median(ts[v])) / ticks, metrics=summary(ms[v]))
        row["table_over_line"] = row["table"]["median_ms"] / row["line"]["median_ms"]
        row["loop_over_table"] = row["loop"]["median_ms"] / row["table"]["median_ms"]
        row["table_equals_line"] = ms["table"] == ms["line"]          # expected on line50 only
        print(json.dumps(row), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds,
            "timing": "host clock around whole runs that end synchronised; a run = create the handle(s), tick, read the metrics, destroy; "
                      "one warm-up run per variant, then rounds alternating line / table / loop; median and min .. max",
            "results": results}
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


def run_variant(td, v, D, tables, fleets, city, ticks):
    if v == "loop":
        return run_loop(td, D, tables, fleets, city, ticks)
    return run_batch(td, D, tables, fleets, city, ticks, on_line=v == "line")


if __name__ == "__main__":
    main()
