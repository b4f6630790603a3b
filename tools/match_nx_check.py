"""Checks the host build of the blossom solver (csrc/td_match_core.h via tools/match_proto.cpp) against networkx's
max_weight_matching on random graphs, and every answer's certificate with tests/match_cert.py.  Needs networkx and a C++
compiler; no GPU.

    python tools/match_nx_check.py [--seeds 0,1,2,3] [--graphs 2100] [--nmax 40]

Six families in turn: ties (1..5), 1..10^6, sparse (90 % <= 0), near 2^31 - 1, 30 % dense 1..3, pool-shaped K - w.
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def family(rng, t, n):
    fam = t % 6
    if fam == 0:
        return rng.integers(1, 6, (n, n))
    if fam == 1:
        return rng.integers(1, 10**6, (n, n))
    if fam == 2:
        return np.where(rng.random((n, n)) < 0.9, -rng.integers(0, 5, (n, n)), rng.integers(1, 20, (n, n)))
    if fam == 3:
        return 2**31 - 1 - rng.integers(0, 100, (n, n))
    if fam == 4:
        return rng.integers(1, 4, (n, n)) * (rng.random((n, n)) < 0.3)
    return 200 - rng.integers(1, 120, (n, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", default="0,1,2,3")
    ap.add_argument("--graphs", type=int, default=2100)
    ap.add_argument("--nmax", type=int, default=40)
    a = ap.parse_args()
    import networkx as nx
    import match_cert
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    exe = os.path.join(tempfile.mkdtemp(), "match_proto")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "taxidispatcher_amd", "csrc"),
                           os.path.join(ROOT, "tools", "match_proto.cpp"), "-o", exe])
    total_bad = total = 0
    for seed in [int(s) for s in a.seeds.split(",")]:
        rng = np.random.default_rng(seed)
        graphs = [np.asarray(family(rng, t, int(rng.integers(0, a.nmax))), np.int64) for t in range(a.graphs)]
        inp = [str(len(graphs))]
        for W in graphs:
            inp += [str(W.shape[0]), " ".join(map(str, W.ravel().tolist()))]
        out = subprocess.run([exe], input="\n".join(inp), capture_output=True, text=True, check=True).stdout.split("\n")
        bad = 0
        for t, W in enumerate(graphs):
            n = W.shape[0]
            err, tot, bnd = map(int, out[5 * t].split())
            mate, y, par, z = (list(map(int, out[5 * t + r].split())) for r in range(1, 5))
            w = match_cert.edge_weights(W)
            G = nx.Graph()
            G.add_nodes_from(range(n))
            iu, ju = np.nonzero(np.triu(w, 1) > 0)
            G.add_weighted_edges_from((int(i), int(j), int(w[i, j])) for i, j in zip(iu, ju))
            ref = sum(int(w[i, j]) for i, j in nx.max_weight_matching(G))
            ok = err == 0 and tot == ref
            if ok:
                try:
                    match_cert.check(W, mate, tot, bnd, y, par, z)
                except AssertionError as e:
                    ok = False
                    print("certificate", seed, t, e)
            if not ok:
                bad += 1
                print("mismatch: seed %d graph %d n %d family %d: err %d total %d bound %d networkx %d" % (seed, t, n, t % 6, err, tot, bnd, ref))
        print("seed %d: %d graphs, %d mismatches" % (seed, len(graphs), bad), flush=True)
        total_bad += bad
        total += len(graphs)
    print("all: %d graphs, %d mismatches" % (total, total_bad))
    sys.exit(1 if total_bad else 0)


if __name__ == "__main__":
    main()
