"""Writes tests/golden/pool_opt/golden.json: the expected answers of tests/test_gpu_pool_opt.py, computed with networkx's
max_weight_matching (never imported by the GPU tests).  Models come from tests/pool_opt_data.py's seeds.

    python tests/golden/pool_opt/make_pool_opt_golden.py
"""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np
import networkx as nx

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pool_opt_data as D  # noqa: E402


def max_matching(w):
    """w: symmetric int64 edge weights (<= 0: no edge) -> (mate list, total)"""
    n = w.shape[0]
    G = nx.Graph()
    G.add_nodes_from(range(n))
    iu, ju = np.nonzero(np.triu(w, 1) > 0)
    G.add_weighted_edges_from((int(i), int(j), int(w[i, j])) for i, j in zip(iu, ju))
    mate = [-1] * n
    for a, b in nx.max_weight_matching(G):
        mate[a], mate[b] = b, a
    return mate, sum(int(w[i, mate[i]]) for i in range(n) if mate[i] > i)


def sym(W):
    W = np.asarray(W, np.int64)
    w = np.maximum(W, W.T)
    np.fill_diagonal(w, 0)
    return w


def job(key):
    kind = key[0]
    if kind == "blossom":
        mate, tot = max_matching(sym(D.blossom_matrix(D.BLOSSOM_CASES[key[1]])))
        return key, {"mate": mate, "total": tot}
    if kind == "family":
        return key, max_matching(sym(D.family(key[1], key[2])))[1]
    name, m, seed, tab, ml = [c for c in D.POOL_CASES if c[0] == key[1]][0]
    frm, to = D.pool_model(m, seed, 100 if tab else 50)
    c, _ = D.pair_costs(frm, to, D.pool_table() if tab else None, ml)
    K, W = D.lex_weights(c)
    mate, _ = max_matching(sym(W))
    pairs = [(i, mate[i]) for i in range(m) if mate[i] > i]
    cost = sum(min(x for x in (c[i, j], c[j, i]) if x >= 0) for i, j in pairs)
    return key, {"count": len(pairs), "total": int(cost)}


def main():
    keys = [("blossom", k) for k in D.BLOSSOM_CASES] + [("family", f, n) for f in D.FAMILIES for n in D.SIZES] + \
           [("pool", c[0]) for c in D.POOL_CASES]
    keys.sort(key=lambda k: -(k[2] if k[0] == "family" else 300 if k[0] == "pool" else 0))
    with Pool(min(8, os.cpu_count() or 1)) as p:
        res = dict(p.map(job, keys, chunksize=1))
    out = {"blossom": {k[1]: res[k] for k in keys if k[0] == "blossom"},
           "families": {f: {str(n): res[("family", f, n)] for n in D.SIZES} for f in D.FAMILIES},
           "pools": {k[1]: res[k] for k in keys if k[0] == "pool"}}
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "golden.json"))


if __name__ == "__main__":
    main()
