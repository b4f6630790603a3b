"""Times td_pool_n_batched (pool_n_batched, find_pool_fanout) against a loop of find_pool_n over the same models.

    python tools/pool_n_batched_time.py [--out profiles/pool_n_batched/pool_n_batched_time.json] [--reps 5] [--loop 100]
    python tools/pool_n_batched_time.py --only 1000x100 --k 4 --no-loop --out /dev/null      # the shape to put under rocprofv3

Shapes, each for k = 2, 3, 4 (tests/pool_n_batched_cases.py's demand recipe: 50 stands, trips of +-1..8):
  1000x40, 1000x100   max_wait <= 3, losses 1, 10, 30
  64x256              max_wait <= 2, losses 1, 10, 25 (max_happy 2^18)
  fixtures            the 8 children of every committed fixture demand as one batch of 8 models (find_pool_fanout without
                      the merge), against 8 find_pool_n(child = c) calls
Host clock around synchronous calls; host inputs; one warm-up call per shape; the median of --reps.  The loop over the
1000-model shapes is timed on --loop models and scaled (the JSON says so).  Every timed batch is compared with the loop.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"1000x40": (1000, 40, 3, [1, 10, 30], 0), "1000x100": (1000, 100, 3, [1, 10, 30], 0), "64x256": (64, 256, 2, [1, 10, 25], 1 << 18)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_n_batched", "pool_n_batched_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=100, help="models timed in the find_pool_n loop of a 1000-model shape (scaled to all)")
    ap.add_argument("--only", default="", help="one shape name, or 'fixtures'")
    ap.add_argument("--k", default="2,3,4")
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    import pool_fixtures as pf
    import pool_n_batched_cases as pc
    td.init(0)
    ks = [int(x) for x in a.k.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timing": "host clock around synchronous calls, host inputs, results copied to the host; median of reps after one warm-up",
           "loop": "find_pool_n model by model; for the 1000-model shapes timed on %d models and scaled to all" % a.loop, "shapes": []}
    for name, (B, m, mw, losses, max_happy) in SHAPES.items():
        if a.only and a.only != name:
            continue
        rng = np.random.default_rng(2025)
        ds = [pc.random_demand(rng, m, mw, losses) for _ in range(B)]
        for k in ks:
            row = {"shape": name, "models": B, "requests": m, "k": k, "max_happy": max_happy or 65536}
            lists, nh = td.pool_n_batched(k, ds, max_happy=max_happy)
            row["happy_mean"], row["happy_max"] = float(nh.mean()), int(nh.max())
            row["pools_mean"] = float(np.mean([len(x) for x in lists]))
            row["batched_ms"] = [x * 1e3 for x in timed(lambda: td.pool_n_batched(k, ds, max_happy=max_happy), a.reps)]
            if not a.no_loop:
                L = min(a.loop, B)
                td.find_pool_n(k, ds[0])
                t0 = time.perf_counter()
                loop = [td.find_pool_n(k, ds[q]) for q in range(L)]
                dt = time.perf_counter() - t0
                assert all(loop[q][0].tolist() == lists[q].tolist() and loop[q][1] == int(nh[q]) for q in range(L))
                row["loop_models_timed"] = L
                row["loop_ms_per_model"] = dt * 1e3 / L
                row["loop_ms_scaled"] = dt * 1e3 / L * B
                row["loop_over_batched"] = row["loop_ms_scaled"] / row["batched_ms"][0]
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    if not a.only or a.only == "fixtures":
        for name, k in pf.cases():
            if k not in ks:
                continue
            ds, firsts, exp = pc.fixture_batch(name, k)
            row = {"shape": "fixture " + name, "models": 8, "requests": len(ds[0]), "k": k, "max_happy": 65536}
            lists, nh = td.pool_n_batched(k, ds, firsts=firsts)
            assert [x.tolist() for x in lists] == exp
            row["happy_max"] = int(nh.max())
            row["batched_ms"] = [x * 1e3 for x in timed(lambda: td.pool_n_batched(k, ds, firsts=firsts), a.reps)]
            row["fanout_and_merge_ms"] = [x * 1e3 for x in timed(lambda: td.find_pool_fanout(k, ds[0]), a.reps)]
            if not a.no_loop:
                row["loop_ms"] = [x * 1e3 for x in timed(lambda: [td.find_pool_n(k, ds[0], child=c) for c in range(8)], a.reps)]
                row["loop_over_batched"] = row["loop_ms"][0] / row["batched_ms"][0]
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
