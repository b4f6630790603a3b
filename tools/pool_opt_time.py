"""Times optimal pooling (td_pool2_batched optimal = 1, td_match_batched) against the greedy and the per-model ways.

    python tools/pool_opt_time.py [--out profiles/pool_opt/pool_opt_time.json] [--reps 5] [--loop 100]

(a) pool_opt_min.py's shape: 1000 models x 100 customers on one 100 x 100 U{1..39} table at max_loss 1.01 (from == to
    removed): one greedy call and one optimal call, against a loop of find_pool_optimal over the same models, and a
    networkx loop on the host (the lexicographic weights K - w) when networkx can be imported (--nx-models of them).
(b) single every-pair models on 50 stands with |a - b| at m = 200, 400, 722, 1445 (the committed simulation's largest
    pool) and 2048: the optimal call against find_pool (the greedy td_pool2).
Host clock around synchronous calls; one warm-up call per shape; the median of --reps (single runs above 1 s).
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


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
        if ts[-1] > 1.0:
            break
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_opt", "pool_opt_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=100, help="models timed in the find_pool_optimal loop (scaled to 1000)")
    ap.add_argument("--nx-models", type=int, default=20)
    ap.add_argument("--sizes", default="200,400,722,1445,2048")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    import pool_opt_data as D
    td.init(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "timing": "host clock around synchronous calls, host inputs, results copied to the host"}
    # (a)
    rng = np.random.default_rng(2024)
    table = rng.integers(1, 40, (100, 100)).astype(np.int32)
    froms, tos = [], []
    for _ in range(1000):
        d = rng.integers(0, 100, (100, 2)).astype(np.int32)
        d = d[d[:, 0] != d[:, 1]]
        froms.append(np.ascontiguousarray(d[:, 0]))
        tos.append(np.ascontiguousarray(d[:, 1]))
    row = {"models": 1000, "customers": 100, "max_loss": 1.01}
    g = td.pool2_batched(froms, tos, table, 1.01, optimal=False)
    o = td.pool2_batched(froms, tos, table, 1.01, optimal=True)
    row["greedy_ms"] = [x * 1e3 for x in timed(lambda: td.pool2_batched(froms, tos, table, 1.01, optimal=False), a.reps)]
    row["optimal_ms"] = [x * 1e3 for x in timed(lambda: td.pool2_batched(froms, tos, table, 1.01, optimal=True), a.reps)]
    L = min(a.loop, 1000)
    td.find_pool_optimal(froms[0], tos[0], table, 1.01)
    t0 = time.perf_counter()
    loop = [td.find_pool_optimal(froms[q], tos[q], table, 1.01) for q in range(L)]
    dt = time.perf_counter() - t0
    assert [len(x) for x in loop] == o[4][:L].tolist() and [sum(p[3] for p in x) for x in loop] == o[5][:L].tolist()
    row["find_pool_optimal_loop_ms_per_model"] = dt * 1e3 / L
    row["find_pool_optimal_loop_ms_extrapolated"] = dt * 1e3 / L * 1000
    eq = (o[4] == g[4]) & (o[5] > 0)
    row["greedy_pools_mean"], row["optimal_pools_mean"] = float(g[4].mean()), float(o[4].mean())
    row["iterations_more_pools"] = int((o[4] > g[4]).sum())
    row["mean_gap_pct_equal_counts"] = float(np.mean(100.0 * (g[5][eq] - o[5][eq]) / o[5][eq]))
    try:
        if a.nx_models <= 0:
            raise ImportError
        import networkx as nx
        t0 = time.perf_counter()
        for q in range(a.nx_models):
            c, _ = D.pair_costs(froms[q], tos[q], table, 1.01)
            K, W = D.lex_weights(c)
            w = np.maximum(W, W.T)
            G = nx.Graph()
            iu, ju = np.nonzero(np.triu(w, 1) > 0)
            G.add_weighted_edges_from((int(i), int(j), int(w[i, j])) for i, j in zip(iu, ju))
            M = nx.max_weight_matching(G)
            assert len(M) == int(o[4][q])
        row["networkx_ms_per_model"] = (time.perf_counter() - t0) * 1e3 / a.nx_models
        row["networkx_ms_extrapolated"] = row["networkx_ms_per_model"] * 1000
    except ImportError:
        row["networkx_ms_per_model"] = None
    res["pool_opt_min_shape"] = row
    print(json.dumps(row), flush=True)
    # (b)
    res["single_every_pair"] = []
    for m in [int(x) for x in a.sizes.split(",")]:
        frm, to = D.pool_model(m, m, 50)
        r = {"m": m, "stands": 50}
        t0 = time.perf_counter()
        opt = td.pool2_batched([frm], [to], None, None, optimal=True)
        r["optimal_s"] = time.perf_counter() - t0
        if r["optimal_s"] < 2.0:
            r["optimal_s"] = timed(lambda: td.pool2_batched([frm], [to], None, None, optimal=True), 3)[0]
        r["find_pool_ms"] = timed(lambda: td.find_pool(frm, to), a.reps)[0] * 1e3
        gr = td.find_pool(frm, to)
        r["optimal_pools"], r["optimal_total"] = int(opt[4][0]), int(opt[5][0])
        r["greedy_pools"], r["greedy_total"] = len(gr), sum(p[3] for p in gr)
        res["single_every_pair"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
