"""Times split_batched (td_split_batched: split.py:61-119 in one call) against what the library offered before it: two
build_assign_batched calls with a numpy pass between them that cuts the lists, reads the regions' row_to_col, collects the
unserved and repacks them.

    python tools/split_time.py [--out profiles/split/split_time.json] [--reps 5] [--only split_py,paper] [--gaps]
    python tools/split_time.py --one-call paper      # a warm-up-free single call, for a kernel trace of its own

Shapes:
  split_py  split.py's own: 1000 cases on 20 stands, 10 draws per side by rand_list's rule (from == to is dropped), 4 parts
  paper     1000 cases of 400 cabs / 400 requests on 4000 stands, 4 parts (tools/tick_batched_time.py's `split` draw)
Host clock around synchronous calls with host position arrays, both routes warmed up first, median of --reps.  The two
routes hand the solver the same models in the same order, so their totals are compared for equality.  --gaps also runs
split_gap at both shapes and records the split and LCM gaps (the paper's section 5: +16 % / +20 %).
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
SHAPES = {"split_py": (20, 10, 1000), "paper": (4000, 400, 1000)}


def draw(name, seed):
    size, per, cases = SHAPES[name]
    rng = np.random.default_rng(seed)
    if name == "split_py":
        from taxidispatcher_amd.dispatch import _rand_positions
        return _rand_positions(rng, per, size, cases, 1), _rand_positions(rng, per, size, cases, 0), size
    cabs = [rng.integers(0, size, per).astype(np.int32) for _ in range(cases)]
    dems = [rng.integers(0, size, per).astype(np.int32) for _ in range(cases)]
    return cabs, dems, size


def two_calls(td, cabs, dems, size, parts):
    """the split heuristic as the library ran it before td_split_batched -> totals int64[cases]"""
    ss = size // parts
    R = (size + ss - 1) // ss
    reg_c, reg_d, idx = [], [], []
    empty = np.zeros(0, np.int32)
    for c, d in zip(cabs, dems):
        rc, rd = c // ss, d // ss
        for r in range(R):
            ic, jd = np.nonzero(rc == r)[0], np.nonzero(rd == r)[0]
            solve = ic.size > 0 and jd.size > 0 and c.size > 0 and d.size > 0
            reg_c.append(c[ic] if solve else empty)
            reg_d.append(d[jd] if solve else empty)
            idx.append((ic, jd, solve))
    r2c, tot = td.build_assign_batched(reg_c, reg_d, None, fill=BIG)
    totals = np.zeros(len(cabs), np.int64)
    rest_c, rest_d = [], []
    for k, (c, d) in enumerate(zip(cabs, dems)):
        keep_c, keep_d = np.ones(c.size, bool), np.ones(d.size, bool)
        if c.size and d.size:
            for r in range(R):
                ic, jd, solve = idx[k * R + r]
                if not solve:
                    continue
                m = k * R + r
                cols = r2c[m, :ic.size]
                real = cols < jd.size
                keep_c[ic[real]] = False
                keep_d[jd[cols[real]]] = False
                totals[k] += tot[m] - abs(ic.size - jd.size) * BIG
            rest_c.append(c[keep_c])
            rest_d.append(d[keep_d])
        else:
            rest_c.append(empty)
            rest_d.append(empty)
    _, tot2 = td.build_assign_batched(rest_c, rest_d, None, fill=BIG)
    for k in range(len(cabs)):
        if rest_c[k].size and rest_d[k].size:
            totals[k] += tot2[k] - abs(rest_c[k].size - rest_d[k].size) * BIG
    return totals


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(min(ts)) * 1e3, float(max(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split", "split_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="split_py,paper")
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--gaps", action="store_true")
    ap.add_argument("--one-call", default=None, metavar="SHAPE")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    if a.one_call:
        cabs, dems, size = draw(a.one_call, seed=len(a.one_call))
        res = td.split_batched(cabs, dems, size, a.parts)
        print(json.dumps({"shape": a.one_call, "sum_total": int(res["total"].sum()), "max_dual_gap": int(res["dual_gap"].max())}))
        return
    results = []
    for name in a.only.split(","):
        cabs, dems, size = draw(name, seed=len(name))
        one = lambda: td.split_batched(cabs, dems, size, a.parts)
        two = lambda: two_calls(td, cabs, dems, size, a.parts)
        res, ref = one(), two()   # warm-up of both routes
        assert np.array_equal(res["total"], ref), "split_batched totals differ from the two-call route"
        assert not res["dual_gap"].any()
        row = {"shape": name, "cases": len(cabs), "stands": size, "parts": a.parts, "max_cabs": int(max(c.size for c in cabs)),
               "max_requests": int(max(d.size for d in dems)), "sum_total": int(res["total"].sum()),
               "rest_cabs_mean": float(res["n_rest"][:, 0].mean()), "rest_requests_mean": float(res["n_rest"][:, 1].mean())}
        row["split_batched_ms"], row["split_batched_min_ms"], row["split_batched_max_ms"] = median_time(one, a.reps)
        row["two_calls_ms"], row["two_calls_min_ms"], row["two_calls_max_ms"] = median_time(two, a.reps)
        row["speedup_vs_two_calls"] = row["two_calls_ms"] / row["split_batched_ms"]
        if a.gaps:
            stands, per, cases = SHAPES[name]
            opt, split, lcm, gs, gl = td.split_gap(stands, per, cases, seed=1, parts=a.parts)
            row.update({"gap_seed": 1, "sum_opt": int(opt.sum()), "sum_split": int(split.sum()), "sum_lcm": int(lcm.sum()),
                        "split_gap_percent": gs, "lcm_gap_percent": gl})
        print(json.dumps(row), flush=True)
        results.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps,
            "timing": "host clock around synchronous calls, host position arrays in, results copied to the host; median of reps "
                      "after a warm-up call of both routes",
            "paper_section_5": {"split_gap_percent": 16, "lcm_gap_percent": 20,
                                "note": "the paper's stand count is not stated and its ties are GLPK's: not comparable digit by digit"},
            "results": results}
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
