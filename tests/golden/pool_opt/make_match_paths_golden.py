"""Writes tests/golden/pool_opt/match_paths.json: the expected answers of tests/test_match_paths_cpu.py and
tests/test_gpu_match_paths.py for the cases of tests/match_path_cases.py.  Needs networkx and a host C++ compiler; it is
not part of the suite.  Three kinds of entry:
  "matching": per matching case (the placement unions included) its size, networkx's max_weight_matching total, and the
              SHA-256 of the host build's (mate, y, blossom_parent, z) (tools/match_proto.cpp, match_path_cases.digest), whole
              and array by array ("parts", to name the first array that differs);
  "pools":    per pool model networkx's (count, total) on the lexicographic weights K - cost, computed with Python integers.

    python tests/golden/pool_opt/make_match_paths_golden.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import networkx as nx

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
import match_path_cases as C  # noqa: E402
import pool_opt_data as D  # noqa: E402


def nx_total(edges, n):
    """edges: (i, j, weight as a Python int > 0) -> (mate list, total)"""
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from(edges)
    mate = [-1] * n
    for a, b in nx.max_weight_matching(G):
        mate[a], mate[b] = b, a
    return mate, sum(G[i][mate[i]]["weight"] for i in range(n) if mate[i] > i)


def matching_total(W):
    W = np.asarray(W, np.int64)
    w = np.maximum(W, W.T)
    iu, ju = np.nonzero(np.triu(w, 1) > 0)
    return nx_total([(int(i), int(j), int(w[i, j])) for i, j in zip(iu, ju)], w.shape[0])[1]


def pool_optimum(c, cand):
    """(count, total) of the lexicographic optimum: the most pools, then the least total cost"""
    m = c.shape[0]
    if m < 2 or not cand.any():
        return [0, 0]
    K, W = C.lex_weights_masked(c, cand)
    edges = []
    for i in range(m):
        for j in range(i + 1, m):
            w = max(int(W[i, j]), int(W[j, i]))
            if w > 0:
                edges.append((i, j, w))
    mate, _ = nx_total(edges, m)
    pairs = [(i, mate[i]) for i in range(m) if mate[i] > i]
    cost = sum(min(int(c[i, j]) if cand[i, j] else 2**62, int(c[j, i]) if cand[j, i] else 2**62) for i, j in pairs)
    return [len(pairs), int(cost)]


def host_digests(mats):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "match_proto")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "taxidispatcher_amd", "csrc"),
                               os.path.join(ROOT, "tools", "match_proto.cpp"), "-o", exe])
        inp = [str(len(mats))]
        for W in mats:
            inp.append(str(W.shape[0]))
            inp.append(" ".join(map(str, np.asarray(W).ravel().tolist())))
        out = subprocess.run([exe], input="\n".join(inp), capture_output=True, text=True, check=True).stdout.split("\n")
    res = []
    for t in range(len(mats)):
        err, tot, bnd = map(int, out[5 * t].split())
        assert err == 0 and tot == bnd
        mate, y, par, z = (list(map(int, out[5 * t + r].split())) for r in range(1, 5))
        res.append((tot, C.digest(mate, y, par, z), C.digest_parts(mate, y, par, z)))
    return res


def main():
    named = [(cs["name"], cs["make"]()) for cs in C.MATCH_CASES]
    for edge in sorted(C.PLACEMENT_BUDGETS.values()):
        named += [("placement_union_%d" % ns, C.placement_union(ns)) for ns in (edge, edge + 1)]
    host = host_digests([W for _, W in named])
    matching = {}
    for (name, W), (tot, dg, parts) in zip(named, host):
        ref = matching_total(W)
        assert ref == tot, (name, ref, tot)
        matching[name] = {"n": int(W.shape[0]), "total": int(ref), "digest": dg, "parts": parts}
        print(name, W.shape[0], ref)
    pools = {}
    for stride in C.SEAMS:
        for tab in (False, True):
            table, ml = C.seam_table(tab)
            rows = []
            for frm, to in C.seam_models(stride, tab):
                c, _ = D.pair_costs(frm, to, table, ml)
                rows.append(pool_optimum(c, c >= 0))
            pools[C.seam_key(stride, tab)] = rows
    for key, (m, span) in C.SPAN_EDGES.items():
        frm, to, table = C.span_case(span, m)
        pools[key] = pool_optimum(*C.pair_costs_masked(frm, to, table)[:2])
    frm, to, table = C.negative_case()
    pools["negative"] = pool_optimum(*C.pair_costs_masked(frm, to, table)[:2])
    with open(os.path.join(HERE, "match_paths.json"), "w") as f:
        json.dump({"matching": matching, "pools": pools}, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(HERE, "match_paths.json"))


if __name__ == "__main__":
    main()
