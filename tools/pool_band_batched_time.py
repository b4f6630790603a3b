"""Times td_pool_n_banded_batched (pool_n_banded_batched) against td_pool_n_batched and against a loop of td_pool_n_banded.

    python tools/pool_band_batched_time.py [--out profiles/pool_n_banded_batched/pool_band_batched_time.json] [--reps 5]
    python tools/pool_band_batched_time.py --only dense --k 4 --out /dev/null

Shapes, each for k = 2, 3, 4 (tests/pool_n_batched_cases.py's demand recipe: 50 stands, trips of +-1..8):
  1000x100, 64x256   tools/pool_n_batched_time.py's: every list fits 65 536 plans.  The new call with the default buffer against
                     td_pool_n_batched with the max_happy that tool uses.
  dense              64 models of 256 requests of which DENSE_BY_K[k] wait on one stand (every pool of them is happy at cost 0), so a
                     list does not fit 65 536 plans at k = 3, 4.  The new call at 65 536 against td_pool_n_batched(max_happy =
                     2^22, 32 workgroups in flight) and against a loop of td_pool_n_banded(plan_buffer = 65 536) over --loop
                     models, scaled.  At k = 2 the list fits and the row says so.
Host clock around synchronous calls; host inputs; one warm-up call per timed function; median, min, max of --reps.  Every timed
answer is compared with the call it is timed against.
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

FIT = {"1000x100": (1000, 100, 3, [1, 10, 30], 0), "64x256": (64, 256, 2, [1, 10, 25], 1 << 18)}
DENSE_BY_K = {2: 64, 3: 48, 4: 16}      # members of the cluster: 8 064 / 622 656 / 1 048 320 plans at cost 0


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [float(np.median(ts)) * 1e3, float(min(ts)) * 1e3, float(max(ts)) * 1e3]


def dense_models(pc, k, batch=64, n=256):
    """the random recipe with the first DENSE_BY_K[k] requests of every model waiting on stand 60 and riding to it"""
    rng = np.random.default_rng(2026)
    ds = []
    for _ in range(batch):
        d = pc.random_demand(rng, n, 2, [1, 10, 25])
        m = DENSE_BY_K[k]
        d[:m, 1], d[:m, 2], d[:m, 3], d[:m, 4] = 60, 60, 0, 0
        ds.append(d)
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_n_banded_batched", "pool_band_batched_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=8, help="models timed in the td_pool_n_banded loop of the dense shape (scaled to all)")
    ap.add_argument("--only", default="", help="one shape name: 1000x100, 64x256 or dense")
    ap.add_argument("--k", default="2,3,4")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    import pool_n_batched_cases as pc
    td.init(0)
    ks = [int(x) for x in a.k.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timing": "host clock around synchronous calls, host inputs, results copied to the host; [median, min, max] ms of reps after one warm-up",
           "shapes": []}
    for name, (B, m, mw, losses, max_happy) in FIT.items():
        if a.only and a.only != name:
            continue
        rng = np.random.default_rng(2025)
        ds = [pc.random_demand(rng, m, mw, losses) for _ in range(B)]
        for k in ks:
            row = {"shape": name, "models": B, "requests": m, "k": k, "max_happy": max_happy or 65536, "plan_buffer": 65536}
            want, nh = td.pool_n_batched(k, ds, max_happy=max_happy)
            got, gh, st = td.pool_n_banded_batched(k, ds, stats=True)
            assert [x.tolist() for x in got] == [x.tolist() for x in want] and gh.tolist() == nh.tolist()
            row["happy_mean"], row["happy_max"] = float(nh.mean()), int(nh.max())
            row["bands_max"], row["passes_mean"] = int(st[:, 0].max()), float(st[:, 1].mean())
            row["batched_ms"] = timed(lambda: td.pool_n_batched(k, ds, max_happy=max_happy), a.reps)
            row["banded_batched_ms"] = timed(lambda: td.pool_n_banded_batched(k, ds), a.reps)
            row["banded_over_batched"] = row["banded_batched_ms"][0] / row["batched_ms"][0]
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    if not a.only or a.only == "dense":
        for k in ks:
            ds = dense_models(pc, k)
            row = {"shape": "dense", "models": len(ds), "requests": 256, "k": k, "cluster": DENSE_BY_K[k], "plan_buffer": 65536}
            got, gh, st = td.pool_n_banded_batched(k, ds, plan_buffer=65536, stats=True)
            row["happy_mean"], row["happy_max"] = float(gh.mean()), int(gh.max())
            row["bands_mean"], row["passes_mean"], row["deepest"] = float(st[:, 0].mean()), float(st[:, 1].mean()), int(st[:, 2].max())
            row["fits_65536"] = bool(gh.max() <= 65536)
            row["banded_batched_ms"] = timed(lambda: td.pool_n_banded_batched(k, ds, plan_buffer=65536), a.reps)
            if gh.max() <= 1 << 22:
                want, nh = td.pool_n_batched(k, ds, max_happy=1 << 22)
                assert [x.tolist() for x in got] == [x.tolist() for x in want] and gh.tolist() == nh.tolist()
                row["batched_2p22_ms"] = timed(lambda: td.pool_n_batched(k, ds, max_happy=1 << 22), a.reps)
                row["banded_over_batched_2p22"] = row["banded_batched_ms"][0] / row["batched_2p22_ms"][0]
            L = min(a.loop, len(ds))
            td.find_pool_n_banded(k, ds[0], plan_buffer=65536)
            t0 = time.perf_counter()
            loop = [td.find_pool_n_banded(k, ds[q], plan_buffer=65536) for q in range(L)]
            dt = time.perf_counter() - t0
            assert all(loop[q][0].tolist() == got[q].tolist() and loop[q][1] == int(gh[q]) for q in range(L))
            row["loop_models_timed"], row["loop_ms_scaled"] = L, dt * 1e3 / L * len(ds)
            row["loop_over_banded_batched"] = row["loop_ms_scaled"] / row["banded_batched_ms"][0]
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
