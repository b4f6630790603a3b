"""CPU tier of the matching / pool path tests (no GPU): the host build of the blossom solver with its path counters
(tools/match_proto.cpp with -DTDM_TRACE) on every case of tests/match_path_cases.py, the coverage those cases give, and
the pool references and the restated launch arithmetic of csrc/td_match.hip against the golden file and the source."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import match_cert
import match_path_cases as C
import pool_opt_data as D
from test_pool_opt_cpu import _run_proto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "pool_opt", "match_paths.json")))
NAMES = [cs["name"] for cs in C.MATCH_CASES]


@pytest.fixture(scope="module")
def proto_trace(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("proto_trace") / "match_proto")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-DTDM_TRACE", "-I", os.path.join(ROOT, "taxidispatcher_amd", "csrc"),
                           os.path.join(ROOT, "tools", "match_proto.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def solved(proto_trace):
    """every matching case through the host build, once: name -> (W, result, counters by name)"""
    mats = [cs["make"]() for cs in C.MATCH_CASES]
    out = {}
    for cs, W, r in zip(C.MATCH_CASES, mats, _run_proto(proto_trace, mats, trace=True)):
        assert len(r[7]) == len(C.TRACE_FIELDS)
        out[cs["name"]] = (W, r[:7], dict(zip(C.TRACE_FIELDS, r[7])))
    return out


def _check_model(name, W, res, total=None):
    err, tot, bnd, mate, y, par, z = res
    g = GOLD["matching"][name]
    assert g["n"] == W.shape[0]
    assert err == 0 and tot == bnd == g["total"], (name, err, tot, bnd, g["total"])
    if total is not None:
        assert tot == total, (name, tot, total)
    match_cert.check(W, mate, tot, bnd, y, par, z)
    assert C.digest(mate, y, par, z) == g["digest"], name


@pytest.mark.parametrize("name", NAMES)
def test_case_on_the_host_build(solved, name):
    cs = C.MATCH_CASES[NAMES.index(name)]
    W, res, tr = solved[name]
    _check_model(name, W, res, cs["total"])
    for counter, least in cs["trace"].items():
        assert tr[counter] >= least, (name, counter, tr[counter], least)
    leaves, depth = C.structure(res[5], W.shape[0])
    assert leaves >= cs["final"].get("leaves", 0) and depth >= cs["final"].get("depth", 0), (name, leaves, depth)


def test_every_path_is_walked_past_one_wave(solved):
    """every counter is non-zero in at least one case whose vertex ids pass one wave, the rarely walked paths in at least
    two: written against the case table, so a case that leaves takes its paths with it only where another case walks them"""
    wide = [n for n in NAMES if solved[n][0].shape[0] > C.WAVE]
    for counter in C.TRACE_FIELDS:
        assert [n for n in wide if solved[n][2][counter] > 0], counter
    for counter in C.RARE_PATHS:
        assert len([n for n in wide if solved[n][2][counter] > 0]) >= 2, counter


def test_unions_are_sums_of_the_committed_totals():
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "pool_opt", "golden.json")))["blossom"]
    assert sum(committed[k]["total"] for k in C.BLOSSOM_NAMES) == C.UNION_TOTAL
    assert C.union(1).shape[0] == C.UNION_SIZE == 118
    for r in (1, 2, 4):
        W = C.union(r)
        assert W.shape[0] == 118 * r and GOLD["matching"]["union_r%d" % r]["total"] == r * C.UNION_TOTAL
        assert (np.triu(W, 1) > 0).any() and (np.tril(W, -1) > 0).any()   # the weight lies in either triangle


def test_placement_arithmetic_and_models(proto_trace):
    src = open(os.path.join(ROOT, "taxidispatcher_amd", "csrc", "td_match.hip")).read()
    core = open(os.path.join(ROOT, "taxidispatcher_amd", "csrc", "td_match_core.h")).read()
    for quoted in ("*per = align256(tdm::bytes(std::max(nmax, 1)));", "*lds = *per <= lds_budget();", "v = 64 * 1024;",
                   "cap = std::min<size_t>((size_t)v, 160 * 1024) - 1024;", "((size_t)256 << 20) / (sizeof(int32_t) * NN)",
                   "((size_t)512 << 20) / *per", "constexpr int64_t POOL_KMAX = (int64_t)1 << 33;",
                   "if (opt && kk + span >= POOL_KMAX)", "if (cc >= INT_MAX || cc <= INT_MIN)", "constexpr int MATCH_NMAX = 2048;"):
        assert quoted in src, quoted
    assert "return (size_t)n * (2 * 2 * 8 + 6 * 4 + 2 * 4 + 11 * 2 * 4) + 64;" in core
    assert C.state_bytes(100) == 152 * 100 + 64
    for budget, edge in C.PLACEMENT_BUDGETS.items():
        assert C.placement_edge(budget) == edge
        assert C.in_lds(edge, budget) and not C.in_lds(edge + 1, budget)
        assert C.align256(C.state_bytes(edge)) <= C.lds_budget(budget) < C.align256(C.state_bytes(edge + 1))
    assert C.PLACEMENT_BUDGETS == {64 * 1024: 424, 160 * 1024: 1070}
    assert C.ws_grid(1 << 20, 1071) == 3292   # the grid cap of the workspace placement at the edge
    # the placement models on the host build: one edge, and the padded unions with the union at the top vertex ids
    names, mats = [], []
    for edge in C.PLACEMENT_BUDGETS.values():
        for ns in (edge, edge + 1):
            W = C.placement_union(ns)
            top = ns - C.placement_r(ns) * C.UNION_SIZE
            assert not W[:top].any() and not W[:, :top].any() and np.maximum(W, W.T)[top:, top:].any(axis=1).all()
            names.append("placement_union_%d" % ns)
            mats.append(W)
            assert C.one_edge(ns).shape == (ns, ns) and np.count_nonzero(C.one_edge(ns)) == 1
    for name, W, r in zip(names, mats, _run_proto(proto_trace, mats, trace=True)):
        _check_model(name, W, r[:7], C.placement_union_total(W.shape[0]))
    assert C.placement_union_total(1070) == C.placement_union_total(1071) == 10233


def test_chunk_arithmetic():
    for stride, chunk in C.SEAMS.items():
        assert C.chunk_of(stride, 10**6) == chunk
        assert [C.chunks_launched(stride, b) for b in C.seam_batches(stride)] == [1, 2, 3]
        assert C.chunk_of(stride, chunk - 1) == chunk - 1   # a short batch is one chunk of its own size
    assert (256 << 20) % (4 * 2048 * 2048) == 0 and (256 << 20) % (4 * 1449 * 1449) != 0
    assert C.chunk_of(100, 1000) == 1000 and C.chunk_of(100, 10**6) == 6710   # pool_gap(100, 1000) never left chunk 0
    w = C.expected_pool_path(2048, 33, 40, None, True, 160 * 1024)
    assert w == (C.MP_POOL | C.MP_PER_MODEL | C.MP_GREEDY | C.MP_MATCH | C.MP_LDS | 3 << 8)
    assert C.expected_pool_path(2048, 16, 40, False, False, 160 * 1024) == (C.MP_POOL | C.MP_GREEDY | 1 << 8)
    assert C.expected_pool_path(2048, 17, 2048, True, False, 160 * 1024) == (C.MP_POOL | C.MP_MATCH | C.MP_WS | 2 << 8)


@pytest.mark.parametrize("stride", sorted(C.SEAMS))
@pytest.mark.parametrize("with_table", [False, True])
def test_seam_models_against_golden(proto_trace, stride, with_table):
    """the numpy references against the golden file: the golden (count, total) is the maximum of the lexicographic weights
    (the host build of the solver on D.lex_weights), and no worse than the greedy"""
    c0 = C.SEAMS[stride]
    models = C.seam_models(stride, with_table)
    gold = GOLD["pools"][C.seam_key(stride, with_table)]
    assert len(models) == len(gold) == 2 * c0 + 1
    sizes = [m[0].size for m in models]
    assert [sizes[k] for k in (c0 - 1, c0, 2 * c0 - 1, 2 * c0)] == [40, 39, 38, 37] and max(sizes) == 40 and sizes[0] == 0
    table, ml = C.seam_table(with_table)
    Ks, mats = [], []
    for frm, to in models:
        c, _ = D.pair_costs(frm, to, table, ml)
        K, W = D.lex_weights(c)
        Ks.append(K)
        mats.append(W.astype(np.int64))
    differs = []
    for q, r in enumerate(_run_proto(proto_trace, mats, trace=True)):
        count, total = gold[q]
        assert r[0] == 0 and r[1] == r[2] == count * Ks[q] - total, (q, r[:3], gold[q], Ks[q])
        c, _ = D.pair_costs(*models[q], table, ml)
        gr = D.greedy(c)
        gt = sum(x[2] for x in gr)
        assert count >= len(gr) and (count > len(gr) or total <= gt), q
        differs.append((count, total) != (len(gr), gt))
    # the optimum beats the greedy (more pools, or cheaper ones) in most models and in all four seam models, so a mixed batch
    # that took the wrong kind for a model shows
    assert sum(differs) > len(models) // 2 and all(differs[k] for k in (c0 - 1, c0, 2 * c0 - 1, 2 * c0))


def test_policies_change_kind_at_the_seams():
    for stride, c0 in C.SEAMS.items():
        for batch in C.seam_batches(stride):
            arg, kinds = C.seam_policy("mix", stride, batch)
            assert arg == kinds and len(kinds) == batch
            for seam in range(c0, batch, c0):
                assert kinds[seam - 1] != kinds[seam]
            assert all(kinds[b] == kinds[b - 1] for b in range(1, batch) if b % c0)
            assert C.seam_policy("greedy", stride, batch) == (False, [0] * batch)
            assert C.seam_policy("optimal", stride, batch) == (True, [1] * batch)
    models, kinds = C.v_wrapper_case()
    assert models[0][0].size == 2048 and kinds == [0] + [1] * 32 and max(m[0].size for m in models[1:]) == 40


def test_range_edges(proto_trace):
    """the largest accepted span and the first refused one through D.lex_weights; the negative table; the limit cells"""
    assert 33 * C.SPAN_MAX + 1 < 2**33 <= 33 * (C.SPAN_MAX + 1) + 1
    assert 23 * C.EXACT_SPAN + 1 == 2**33 and C.SPAN_EDGES == {"span_max": (64, 260301048), "span_exact": (44, 373475416)}
    for m, span, ok in ((64, C.SPAN_MAX, True), (64, C.SPAN_MAX + 1, False), (44, C.EXACT_SPAN - 1, True), (44, C.EXACT_SPAN, False)):
        frm, to, table = C.span_case(span, m)
        c, _ = D.pair_costs(frm, to, table, None)
        cand = c >= 0
        assert frm.size == m and int(c.max()) == span == int(c[0, 1]) == int(c[1, 0]) and int(c[cand].min()) > 0
        assert np.sort(c[cand])[-3] <= 117   # only the two ordered pairs of customers 0 and 1 are dear
        K, W = D.lex_weights(c)
        assert K == (m // 2) * span + 1 and (K + span < C.POOL_KMAX) == ok == C.accepted(m, span)
        cm, candm, _ = C.pair_costs_masked(frm, to, table)
        assert np.array_equal(cm[candm], c[cand]) and C.span_of(cm, candm) == span
    for key, (m, _) in C.SPAN_EDGES.items():
        count, total = GOLD["pools"][key]
        assert count == m // 2 and 0 < total < count * 117   # a perfect matching that leaves the dear pair out
    frm, to, table = C.negative_case()
    c, cand, _ = C.pair_costs_masked(frm, to, table)
    assert int(c[cand].max()) > 0 > int(c[cand].min()) and C.span_of(c, cand) == int(c[cand].max()) - int(c[cand].min())
    assert C.accepted(frm.size, C.span_of(c, cand)) and GOLD["pools"]["negative"][0] == 24
    K, W = C.lex_weights_masked(c, cand)
    r = _run_proto(proto_trace, [W.astype(np.int64)], trace=True)[0]
    kept = [min(int(c[i, j]), int(c[j, i])) for i, j in enumerate(r[3]) if j > i]
    assert r[0] == 0 and [len(kept), sum(kept)] == GOLD["pools"]["negative"] and min(kept) < 0 < max(kept)
    for value, ok in C.LIMIT_CELLS.items():
        frm, to, table = C.limit_cell_case(value)
        c, cand, _ = C.pair_costs_masked(frm, to, table)
        assert int(c[0, 1]) == int(c[1, 0]) == value and ok == (C.INT_MIN < value < C.INT_MAX)
        assert C.greedy_masked(c, cand) == [(0, 1, value)]
