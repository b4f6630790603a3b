"""Times the batched position entry points (tick_batched / build_assign_batched) against per-model loops on the same models.

    python tools/tick_batched_time.py [--out profiles/tick_batched/tick_batched_time.json] [--reps 5] [--only tick_small]

Shapes (name: B models, cabs x requests, stands, rule):
  tick_small   256 x (200 x 150), |a - b| on 50 stands, DROP_TIME 10, MAX_NON_LCM 100   vs a loop of td.tick
  tick_sim     64 x (1300 x 900), Simulator.java's constants (50 stands, 10, 600)       vs a loop of td.tick
  greedy_opt   1000 x (100 x 100), |a - b| on 4000 stands, no threshold, no LCM         vs cost_build per model +
               assign_batched, and vs a loop of build_assign
  split        split.py: 1000 cases of 400 requests / 400 cabs on 4000 stands, each cut into 4 stand ranges = 4000 region
               models                                                                   vs a loop of build_assign
Host clock around synchronous calls with host position arrays, every shape warmed up first; the batched calls report the
median of --reps, the loops one pass (median of --loop-reps passes).  Both sides' totals are checked equal.
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


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(min(ts)) * 1e3, float(max(ts)) * 1e3


def models(name, seed):
    rng = np.random.default_rng(seed)
    if name == "tick_small":
        return [rng.integers(0, 50, 200) for _ in range(256)], [rng.integers(0, 50, 150) for _ in range(256)], 10, 100
    if name == "tick_sim":
        return [rng.integers(0, 50, 1300) for _ in range(64)], [rng.integers(0, 50, 900) for _ in range(64)], 10, 600
    if name == "greedy_opt":
        return [rng.integers(0, 4000, 100) for _ in range(1000)], [rng.integers(0, 4000, 100) for _ in range(1000)], None, None
    if name == "split":
        cabs, dems = [], []
        for _ in range(1000):
            c, d = rng.integers(0, 4000, 400), rng.integers(0, 4000, 400)
            for lo in range(0, 4000, 1000):
                cabs.append(c[(c >= lo) & (c < lo + 1000)])
                dems.append(d[(d >= lo) & (d < lo + 1000)])
        return cabs, dems, None, None
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tick_batched", "tick_batched_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--only", default="tick_small,tick_sim,greedy_opt,split")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    cabs_all = {}
    results = []
    for name in a.only.split(","):
        cabs, dems, drop, stop = models(name, seed=len(name))
        cabs = [np.ascontiguousarray(c, np.int32) for c in cabs]
        dems = [np.ascontiguousarray(d, np.int32) for d in dems]
        cabs_all[name] = len(cabs)
        row = {"shape": name, "B": len(cabs), "max_cabs": max(c.size for c in cabs), "max_requests": max(d.size for d in dems),
               "drop_time": drop, "max_non_lcm": stop}
        if stop is not None:   # a tick per model
            batched = lambda: td.tick_batched(cabs, dems, None, big_cost=BIG, drop_time=drop, max_non_lcm=stop)
            loop = lambda: [td.tick(c, d, None, big_cost=BIG, drop_time=drop, max_non_lcm=stop) for c, d in zip(cabs, dems)]
            got = batched()
            ref = loop()   # warm-up of both sides
            assert [g["total"] for g in got] == [t["total"] for t in ref], "batched totals differ from the td.tick loop"
            assert [len(g["lcm_rows"]) for g in got] == [len(t["lcm_rows"]) for t in ref]
            row["solved_models"] = int(sum(g["solved"] for g in got))
            row["lcm_pairs_total"] = int(sum(len(g["lcm_rows"]) for g in got))
            row["batched_ms"], row["batched_min_ms"], row["batched_max_ms"] = median_time(batched, a.reps)
            row["tick_loop_ms"] = median_time(loop, a.loop_reps)[0]
            row["speedup_vs_tick_loop"] = row["tick_loop_ms"] / row["batched_ms"]
        else:                  # an optimum per model
            thr = -1
            batched = lambda: td.build_assign_batched(cabs, dems, None, fill=BIG, threshold=thr)
            loop = lambda: [td.build_assign(c, d, None, fill=BIG, threshold=thr)[2] for c, d in zip(cabs, dems)]
            _, tot = batched()
            ref = loop()
            assert tot.tolist() == ref, "batched totals differ from the build_assign loop"
            _, _, dual = td.build_assign_batched(cabs, dems, None, fill=BIG, threshold=thr, want_dual=True)
            assert (dual == tot).all()
            row["batched_ms"], row["batched_min_ms"], row["batched_max_ms"] = median_time(batched, a.reps)
            row["build_assign_loop_ms"] = median_time(loop, a.loop_reps)[0]
            row["speedup_vs_build_assign_loop"] = row["build_assign_loop_ms"] / row["batched_ms"]
            if name == "greedy_opt":   # the slab route: td_cost_build per model, pack, assign_batched
                n = max(max(c.size, d.size) for c, d in zip(cabs, dems))

                def slab_route():
                    slab = np.full((len(cabs), n, n), BIG, np.int32)
                    ns = np.zeros(len(cabs), np.int32)
                    for b, (c, d) in enumerate(zip(cabs, dems)):
                        k, m = td.cost_build(c, d, None, fill=BIG, threshold=thr)
                        slab[b, :k, :k] = m
                        ns[b] = k
                    return td.assign_batched(slab, ns=ns)[1]
                assert slab_route().tolist() == tot.tolist()
                row["cost_build_plus_assign_batched_ms"] = median_time(slab_route, a.loop_reps)[0]
                row["speedup_vs_cost_build_plus_assign_batched"] = row["cost_build_plus_assign_batched_ms"] / row["batched_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "loop_reps": a.loop_reps,
            "timing": "host clock around synchronous calls, host position arrays in, results copied to the host; batched: median "
                      "of reps after a warm-up call",
            "results": results}
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
