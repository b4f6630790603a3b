"""Times dispatch_batched (td_dispatch_batched: a dispatch method per model) in each single mode and in an even mix, beside
tick_batched and split_batched on the same models.

    python tools/dispatch_batched_time.py [--out profiles/sim_dispatch_policy/dispatch_batched_time.json] [--reps 7]
                                          [--models 1000] [--per-side 100] [--stands 50] [--drop-time 10] [--max-non-lcm 16]

Shape: --models models of --per-side cabs and requests each on --stands stands (the line), cells below --drop-time, 4 parts.
Host clock around synchronous calls with host position arrays, every route warmed up first, median of --reps (min and max
beside it).  The even mix gives model b mode b % 4; "sum_of_parts" is the sum of the four single-mode calls on the quarter of
the models each mode has in the mix, which is what four separate calls would cost.  The service each method gives on these
static models (served pairs, mean distance of a served pair) is recorded with the times.
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
MODES = ["lcm+opt", "opt", "lcm", "split"]


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"ms": float(np.median(ts)) * 1e3, "min_ms": float(min(ts)) * 1e3, "max_ms": float(max(ts)) * 1e3}


def service(td, res, cabs, dems, modes, drop):
    """served pairs and their summed distance, per method, from one result"""
    out = {m: [0, 0] for m in MODES}
    for b, (c, d) in enumerate(zip(cabs, dems)):
        k = int(res["n_pairs"][b])
        pairs = [(int(res["lcm_rows"][b, i]), int(res["lcm_cols"][b, i])) for i in range(k)]
        if modes[b] == "split":
            pairs = [(i, int(j)) for i, j in enumerate(res["row_to_col"][b, :c.size]) if j >= 0]
        elif modes[b] != "lcm":
            kc, kd = res["kept_cabs"][b, :c.size - k], res["kept_dems"][b, :d.size - k]
            pairs += [(int(kc[i]), int(kd[j])) for i, j in enumerate(res["row_to_col"][b, :kc.size]) if 0 <= j < kd.size]
        dist = [abs(int(c[i]) - int(d[j])) for i, j in pairs]
        real = [x for x in dist if x < drop]
        out[modes[b]][0] += len(real)
        out[modes[b]][1] += sum(real)
    return {m: {"served": v[0], "mean_distance": (v[1] / v[0] if v[0] else None)} for m, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_dispatch_policy", "dispatch_batched_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--models", type=int, default=1000)
    ap.add_argument("--per-side", type=int, default=100)
    ap.add_argument("--stands", type=int, default=50)
    ap.add_argument("--drop-time", type=int, default=10)
    ap.add_argument("--max-non-lcm", type=int, default=16)
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    rng = np.random.default_rng(a.models + a.per_side)
    cabs = [rng.integers(0, a.stands, a.per_side).astype(np.int32) for _ in range(a.models)]
    dems = [rng.integers(0, a.stands, a.per_side).astype(np.int32) for _ in range(a.models)]
    kw = dict(big_cost=BIG, drop_time=a.drop_time, size=a.stands, max_non_lcm=a.max_non_lcm, parts=4)
    mix = [MODES[b % 4] for b in range(a.models)]
    rows = {}
    for m in MODES:
        call = lambda m=m: td.dispatch_batched(cabs, dems, None, mode=m, **kw)
        res = call()
        assert (res["dual_bound"] == res["total"]).all(), m
        rows[m] = dict(median_time(call, a.reps), service=service(td, res, cabs, dems, [m] * a.models, a.drop_time)[m])
        q = [b for b in range(a.models) if mix[b] == m]
        part = lambda m=m, q=q: td.dispatch_batched([cabs[b] for b in q], [dems[b] for b in q], None, mode=m, **kw)
        part()
        rows[m]["quarter"] = median_time(part, a.reps)
    call = lambda: td.dispatch_batched(cabs, dems, None, mode=mix, **kw)
    res = call()
    assert (res["dual_bound"] == res["total"]).all()
    rows["mix"] = dict(median_time(call, a.reps), service=service(td, res, cabs, dems, mix, a.drop_time),
                       sum_of_parts_ms=sum(rows[m]["quarter"]["ms"] for m in MODES))
    tick = lambda: td.tick_batched(cabs, dems, None, big_cost=BIG, drop_time=a.drop_time, max_non_lcm=a.max_non_lcm)
    tick()
    rows["tick_batched"] = median_time(tick, a.reps)
    raw = lambda: td.dispatch_batched(cabs, dems, None, mode=None, **kw)
    raw()
    rows["lcm+opt, mode NULL"] = median_time(raw, a.reps)
    split = lambda: td.split_batched(cabs, dems, a.stands, 4)
    split()
    rows["split_batched (no threshold)"] = median_time(split, a.reps)
    free = lambda: td.dispatch_batched(cabs, dems, None, mode="split", **dict(kw, drop_time=None))
    free()
    rows["split, no threshold"] = median_time(free, a.reps)
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps, "models": a.models, "per_side": a.per_side,
            "stands": a.stands, "drop_time": a.drop_time, "max_non_lcm": a.max_non_lcm, "parts": 4,
            "timing": "host clock around synchronous calls, host position arrays in, results copied to the host; median of reps after "
                      "a warm-up call; tick_batched also builds its list of per-model dicts, dispatch_batched returns the arrays",
            "results": rows}
    for k, v in rows.items():
        print(json.dumps({k: v}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
