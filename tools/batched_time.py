"""Times the batched entry points against a per-model loop of the single-model calls on the same models.

    python tools/batched_time.py [--out profiles/batched/batched_time.json] [--reps 5] [--families g4,wide]

For every (B, n) of heuristic.py (1000 x 100), (4096, 64), (512, 256), (64, 1024) and every cost family:
  assign_batched (device input)  vs  a Python loop of Solver.assign over the same device-resident models
  LCM_batched    (device input)  vs  a Python loop of dispatch._lcm (td_lcm, behind LCM_heuristic)
with heuristic.py's LCM rule (mask 100, n picks).  Host clock around calls that end in a device synchronisation
(every call here is synchronous); one warm-up call of every shape; the batched calls report the median of --reps.
Every loop total equals the batched total (checked), so the two sides compute the same answer.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1000, 100), (4096, 64), (512, 256), (64, 1024)]


def gen(fam, B, n, seed):
    rng = np.random.default_rng(seed)
    if fam == "g4":      # heuristic.py:21 U{1..39}
        return rng.integers(1, 40, (B, n, n)).astype(np.int32)
    if fam == "wide":    # uniform 0..1e6
        return rng.integers(0, 1000001, (B, n, n)).astype(np.int32)
    raise ValueError(fam)


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "batched_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--families", default="g4,wide")
    ap.add_argument("--shapes", default=None, help="B:n,B:n,... (default: the four shapes of the issue)")
    ap.add_argument("--loop-max", type=int, default=1000, help="models timed in the per-model loop (scaled to B)")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    from taxidispatcher_amd import dispatch
    td.init(0)
    shapes = SHAPES if not a.shapes else [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    results = []
    for fam in a.families.split(","):
        for B, n in shapes:
            c = gen(fam, B, n, seed=B * 7 + n)
            dev = torch.from_numpy(c).cuda()
            torch.cuda.synchronize()
            row = {"family": fam, "B": B, "n": n}
            # --- optimum
            td.assign_batched(dev)   # warm-up
            _, tot = td.assign_batched(dev)
            row["assign_batched_ms"], row["assign_batched_min_ms"], row["assign_batched_max_ms"] = \
                (x * 1e3 for x in median_time(lambda: td.assign_batched(dev), a.reps))
            t0 = time.perf_counter()
            _, _, dual = td.assign_batched(dev, want_dual=True)
            row["assign_batched_with_dual_ms"] = (time.perf_counter() - t0) * 1e3
            assert (dual == tot).all()
            L = min(B, a.loop_max)
            with td.Solver() as s:
                s.assign(dev[0])   # warm-up
                t0 = time.perf_counter()
                loop_tot = [s.assign(dev[b])[1] for b in range(L)]
                dt = time.perf_counter() - t0
            assert np.array_equal(np.array(loop_tot), tot[:L]), "per-model totals differ from the batched totals"
            row["assign_loop_models"] = L
            row["assign_loop_ms_per_model"] = dt * 1e3 / L
            row["assign_loop_ms_extrapolated"] = dt * 1e3 / L * B
            row["assign_speedup"] = row["assign_loop_ms_extrapolated"] / row["assign_batched_ms"]
            # --- LCM, heuristic.py's rule
            td.LCM_batched(dev, mask=100)
            lt = td.LCM_batched(dev, mask=100)[0]
            row["lcm_batched_ms"], row["lcm_batched_min_ms"], row["lcm_batched_max_ms"] = \
                (x * 1e3 for x in median_time(lambda: td.LCM_batched(dev, mask=100), a.reps))
            dispatch._lcm(n, dev[0], 100, -1, 0, 0, -1, 2**62)
            t0 = time.perf_counter()
            loop_l = [dispatch._lcm(n, dev[b], 100, -1, 0, 0, -1, 2**62)[0] for b in range(L)]
            dt = time.perf_counter() - t0
            assert np.array_equal(np.array(loop_l), lt[:L]), "per-model LCM totals differ from the batched totals"
            row["lcm_loop_ms_per_model"] = dt * 1e3 / L
            row["lcm_loop_ms_extrapolated"] = dt * 1e3 / L * B
            row["lcm_speedup"] = row["lcm_loop_ms_extrapolated"] / row["lcm_batched_ms"]
            row["mean_gap_pct"] = float(np.mean(100.0 * (lt - tot) / tot)) if (tot > 0).all() else None
            print(json.dumps(row), flush=True)
            results.append(row)
            del dev
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps,
            "timing": "host clock around synchronous calls, device-resident input, results copied to the host",
            "results": results}
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
