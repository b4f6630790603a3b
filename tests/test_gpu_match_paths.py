"""GPU tests of csrc/td_match.hip at its path, placement, chunk and range edges (cases: tests/match_path_cases.py; expected
answers: tests/golden/pool_opt/match_paths.json, by networkx and the host build of the solver).

Matching: the device runs the control code of csrc/td_match_core.h that the host build runs, with the same min-key choices
(pack(value, index)), the same ascending queue order and the same order of tight edges, so its (mate, y, blossom_parent, z)
must hash to the host build's digest: that is what carries the path coverage counted on the host (test_match_paths_cpu.py)
onto the 64-lane build.  Placement: td.match_path() says where the solver state lay; the edge is probed with one-edge
models and then crossed with a real model.  Pools: batches that end at, one past and one past twice the 256 MiB chunk, every
model against its own reference; the range edges of the pool weights.

Not covered: a second model per workgroup on the WORKSPACE placement.  The grid is capped at 512 MiB of slices (3 292
workgroups at n = 1071), so through td_match_batched that needs a slab of over 15 GB, and the pool path never strides there
(chunk <= grid).  The LDS placement's second model is tests/test_gpu_second_model.py's.

Measured on one MI355X (pytest --durations, profiles/match_paths/pytest_gpu.txt): see the times beside the tests."""
import json
import os

import numpy as np
import pytest

import match_cert
import match_path_cases as C
import pool_opt_data as D

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_opt", "match_paths.json")))
SMALL = (np.array([1, 2, 3, 4], np.int32), np.array([2, 3, 4, 5], np.int32))   # a call that must work after a refusal


def _check_exported(name, W, k, stride, mate, total, bound, duals, final=None):
    """model k of a match_batched result (slab stride `stride`) against golden total, certificate, structure and digest"""
    y, par, z = duals
    m = W.shape[0]
    g = GOLD["matching"][name]
    assert int(total[k]) == int(bound[k]) == g["total"], (name, int(total[k]), int(bound[k]), g["total"])
    parent = C.own_ids(par[k], stride, m)
    match_cert.check(W, mate[k, :m], total[k], bound[k], y[k, :m], parent, z[k, :m])
    assert (mate[k, m:] == -1).all() and (y[k, m:] == 0).all() and (z[k, m:] == 0).all(), name
    leaves, depth = C.structure(parent, m)
    final = final or {}
    assert leaves >= final.get("leaves", 0) and depth >= final.get("depth", 0), (name, leaves, depth, final)
    parts = C.digest_parts(mate[k, :m], y[k, :m], parent, z[k, :m])
    differ = [what for what, p, q in zip(("mate", "y", "blossom_parent", "z"), parts, g["parts"]) if p != q]
    assert not differ and C.digest(mate[k, :m], y[k, :m], parent, z[k, :m]) == g["digest"], \
        "%s: the device's %s differ from the host build's" % (name, ", ".join(differ))


def test_matching_cases_in_one_slab(td):
    """every matching case in one call, mixed sizes in one slab (stride 472), the models side by side (0.24 s)"""
    mats = [cs["make"]() for cs in C.MATCH_CASES]
    mate, total, bound, duals = td.match_batched(mats, want_dual=True)
    path = td.match_path()
    stride = mate.shape[1]
    assert stride == max(W.shape[0] for W in mats)
    assert path >> C.MP_CHUNK_SHIFT == 1 and path & 0xFF in (C.MP_LDS, C.MP_WS)
    failures = []
    for k, (cs, W) in enumerate(zip(C.MATCH_CASES, mats)):
        if cs["total"] is not None:
            assert int(total[k]) == cs["total"], cs["name"]
        try:
            _check_exported(cs["name"], W, k, stride, mate, total, bound, duals, cs["final"])
        except AssertionError as e:
            failures.append("%s: %s" % (cs["name"], e))
    assert not failures, "\n".join(failures)


@pytest.fixture(scope="module")
def edge(td):
    """(budget, n_edge) of this device, probed with one-edge models: exactly one candidate shows the state in LDS at n_edge
    and in the workspace at n_edge + 1; any other edge fails"""
    seen = {}
    for budget, n_edge in C.PLACEMENT_BUDGETS.items():
        words = []
        for ns in (n_edge, n_edge + 1):
            mate, total, bound = td.match_batched([C.one_edge(ns)])
            assert int(total[0]) == int(bound[0]) == 7 and mate[0, 0] == ns - 1 and mate[0, ns - 1] == 0
            assert np.count_nonzero(mate[0] >= 0) == 2
            w = td.match_path()
            assert w >> C.MP_CHUNK_SHIFT == 1 and w & 0xFF in (C.MP_LDS, C.MP_WS), hex(w)
            words.append(w & 0xFF)
        seen[budget] = words
    at = [b for b, w in seen.items() if w == [C.MP_LDS, C.MP_WS]]
    assert len(at) == 1, "no candidate edge, or more than one, is this device's: %r" % (seen,)
    for b, w in seen.items():   # the other candidate lies wholly on one side, the side the device's edge puts it on
        if b != at[0]:
            n_other = C.PLACEMENT_BUDGETS[b]
            assert w == [C.MP_LDS if C.in_lds(n, at[0]) else C.MP_WS for n in (n_other, n_other + 1)], seen
    return at[0], C.PLACEMENT_BUDGETS[at[0]]


def test_placement_edge_probe(edge):
    budget, n_edge = edge
    assert C.placement_edge(budget) == n_edge


def test_placement_edge_crossed_by_a_real_model(td, edge):
    """the padded union at the edge (state in LDS) and one vertex above it (state in a workspace slice): the same optimum,
    a valid certificate, the host build's digest, and the same mates in either placement (2.8 s for the two solves and
    their numpy certificate checks)"""
    budget, n_edge = edge
    mates = []
    for ns, bit in ((n_edge, C.MP_LDS), (n_edge + 1, C.MP_WS)):
        W = C.placement_union(ns)
        mate, total, bound, duals = td.match_batched([W], want_dual=True)
        assert td.match_path() == bit | 1 << C.MP_CHUNK_SHIFT
        assert int(total[0]) == C.placement_union_total(ns)
        _check_exported("placement_union_%d" % ns, W, 0, ns, mate, total, bound, duals)
        top = ns - C.placement_r(ns) * C.UNION_SIZE
        assert (mate[0, :top] == -1).all()
        mates.append(np.where(mate[0, top:] >= 0, mate[0, top:] - top, -1))
    assert np.array_equal(mates[0], mates[1])


# ----------------------------------------------------------------------------------------------------------------------
# chunk seams
# ----------------------------------------------------------------------------------------------------------------------
def _rows(res, q):
    a, b, plan, cost, k, tot = res
    return [(int(a[q, i]), int(b[q, i]), int(plan[q, i]), int(cost[q, i])) for i in range(int(k[q]))], int(tot[q])


def _check_optimal_rows(c, cand, p1, rows, total, gold, greedy_rows):
    """tests/test_gpu_pool_opt.py's _check_optimal with the candidate mask apart, plus the golden (count, total)"""
    used = [x for r in rows for x in r[:2]]
    assert len(used) == len(set(used)), "pools share a customer"
    for x, y, pl, co in rows:
        assert cand[x, y] and co == c[x, y] and pl == int(p1[x, y])
        assert not cand[y, x] or c[y, x] > co or (c[y, x] == co and x < y), "not the cheaper direction"
    assert rows == sorted(rows, key=lambda r: (r[3], r[0], r[1]))
    assert total == sum(r[3] for r in rows)
    assert [len(rows), total] == list(gold)
    gk, gt = len(greedy_rows), sum(r[3] for r in greedy_rows)
    assert len(rows) >= gk and (len(rows) > gk or total <= gt)


@pytest.fixture(scope="module")
def seam_refs():
    """per (stride, with_table): the models and per model (c, cand, plan1, greedy rows with plan), computed once"""
    out = {}
    for stride in C.SEAMS:
        for tab in (False, True):
            table, ml = C.seam_table(tab)
            refs = []
            for frm, to in C.seam_models(stride, tab):
                c, p1 = D.pair_costs(frm, to, table, ml)
                gr = [(x, y, int(p1[x, y]), co) for x, y, co in D.greedy(c)]
                refs.append((c, c >= 0, p1, gr))
            out[stride, tab] = (C.seam_models(stride, tab), refs)
    return out


def _check_batch(res, kinds, refs, gold, first=0):
    for q, kind in enumerate(kinds):
        c, cand, p1, gr = refs[first + q]
        rows, total = _rows(res, q)
        if kind:
            _check_optimal_rows(c, cand, p1, rows, total, gold[first + q], gr)
        else:
            assert rows == gr and total == sum(r[3] for r in gr), (first + q, "greedy")


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("stride", sorted(C.SEAMS))
def test_pool_chunk_seams(td, edge, seam_refs, stride, with_table):
    """batches of chunk, chunk + 1 and 2 chunk + 1 models at this stride, all greedy, all optimal and a per-model mix that
    changes kind exactly at each seam: every model against its own reference, the chunk count and the policy bits in
    match_path, and the two models of the first seam alone in a uniform call (eleven calls, 0.01 to 0.02 s in all)"""
    budget, _ = edge
    models, refs = seam_refs[stride, with_table]
    gold = GOLD["pools"][C.seam_key(stride, with_table)]
    table, ml = C.seam_table(with_table)
    c0 = C.SEAMS[stride]
    at_seam = {}
    for batch in C.seam_batches(stride):
        froms, tos = [m[0] for m in models[:batch]], [m[1] for m in models[:batch]]
        for kind in C.POLICIES:
            arg, kinds = C.seam_policy(kind, stride, batch)
            res = td.pool2_batched(froms, tos, table, ml, optimal=arg, n=stride)
            word = td.match_path()
            want = C.expected_pool_path(stride, batch, max(f.size for f in froms), arg if kind != "mix" else None, kind == "mix", budget)
            assert word == want, (batch, kind, hex(word), hex(want))
            assert word >> C.MP_CHUNK_SHIFT == -(-batch // c0)
            assert res[0].shape == (batch, stride // 2)
            _check_batch(res, kinds, refs, gold)
            if batch > c0:
                for q in (c0 - 1, c0):
                    at_seam.setdefault((q, kinds[q]), []).append(_rows(res, q))
    # the two models at the first seam, alone: the same rows whatever batch and policy they came out of
    pair = [c0 - 1, c0]
    for optimal in (0, 1):
        res = td.pool2_batched([models[q][0] for q in pair], [models[q][1] for q in pair], table, ml, optimal=bool(optimal), n=stride)
        assert td.match_path() >> C.MP_CHUNK_SHIFT == 1
        for k, q in enumerate(pair):
            alone = _rows(res, k)
            assert at_seam[q, optimal] and all(x == alone for x in at_seam[q, optimal]), (q, optimal)


def test_pool_per_model_batch_through_the_plain_wrapper(td, seam_refs):
    """33 models, no n=: model 0 has 2048 customers and is greedy, which makes the stride 2048 (three chunks of 16) and puts
    the solver state of the 32 small optimal models behind it in the workspace (0.85 s, most of it the numpy reference of
    the 2048-customer greedy)"""
    models, kinds = C.v_wrapper_case()
    res = td.pool2_batched([m[0] for m in models], [m[1] for m in models], None, None, optimal=kinds)
    assert td.match_path() == (C.MP_POOL | C.MP_PER_MODEL | C.MP_GREEDY | C.MP_MATCH | C.MP_WS | 3 << C.MP_CHUNK_SHIFT)
    assert res[0].shape == (33, 1024)
    c, p1 = D.pair_costs(models[0][0], models[0][1])
    gr = [(x, y, int(p1[x, y]), co) for x, y, co in C.greedy_masked(c, c >= 0)]
    rows, total = _rows(res, 0)
    assert len(gr) == 1024 and rows == gr and total == sum(r[3] for r in gr)
    _, refs = seam_refs[2048, False]
    _check_batch(tuple(x[1:] for x in res), kinds[1:], refs, GOLD["pools"][C.V_WRAPPER_KEY], first=1)


# ----------------------------------------------------------------------------------------------------------------------
# range edges of the pool weights
# ----------------------------------------------------------------------------------------------------------------------
def _still_usable(td):
    assert td.pool2_batched([SMALL[0]], [SMALL[1]], None, None, optimal=True)[4][0] == 2


@pytest.mark.parametrize("key", sorted(C.SPAN_EDGES))
def test_largest_accepted_span_and_the_first_refused(td, key):
    """span_max: the issue's 64 customers, K + span = 33 span + 1 steps over 2^33; span_exact: 44 customers, where the first
    refused K + span = 23 span + 1 is exactly 2^33"""
    m, span = C.SPAN_EDGES[key]
    frm, to, table = C.span_case(span, m)
    c, cand, p1 = C.pair_costs_masked(frm, to, table)
    gr = [(x, y, int(p1[x, y]), co) for x, y, co in C.greedy_masked(c, cand)]
    res = td.pool2_batched([frm], [to], table, None, optimal=True)
    assert td.match_path() & C.MP_MATCH
    rows, total = _rows(res, 0)
    _check_optimal_rows(c, cand, p1, rows, total, GOLD["pools"][key], gr)
    assert _rows(td.pool2_batched([frm], [to], table, None, optimal=False), 0)[0] == gr
    frm, to, table = C.span_case(span + 1, m)
    with pytest.raises(td.TdError, match="error -4"):
        td.pool2_batched([frm], [to], table, None, optimal=True)
    _still_usable(td)
    # the greedy never reads K: the same model is accepted there
    c, cand, p1 = C.pair_costs_masked(frm, to, table)
    assert _rows(td.pool2_batched([frm], [to], table, None, optimal=False), 0)[0] == \
        [(x, y, int(p1[x, y]), co) for x, y, co in C.greedy_masked(c, cand)]


def test_negative_table_crosses_the_sign_change(td):
    frm, to, table = C.negative_case()
    c, cand, p1 = C.pair_costs_masked(frm, to, table)
    gr = [(x, y, int(p1[x, y]), co) for x, y, co in C.greedy_masked(c, cand)]
    rows, total = _rows(td.pool2_batched([frm], [to], table, None, optimal=True), 0)
    _check_optimal_rows(c, cand, p1, rows, total, GOLD["pools"]["negative"], gr)
    costs = [r[3] for r in rows]
    assert costs[0] < 0 < costs[-1], "the listing does not cross the sign change"
    assert _rows(td.pool2_batched([frm], [to], table, None, optimal=False), 0)[0] == gr


@pytest.mark.parametrize("value", sorted(C.LIMIT_CELLS))
def test_limit_cells_of_the_greedy(td, value):
    frm, to, table = C.limit_cell_case(value)
    if C.LIMIT_CELLS[value]:
        res = td.pool2_batched([frm], [to], table, None, optimal=False)
        rows, total = _rows(res, 0)
        assert [r[:2] + r[3:] for r in rows] == [(0, 1, value)] and total == value
    else:
        with pytest.raises(td.TdError, match="error -4"):
            td.pool2_batched([frm], [to], table, None, optimal=False)
        _still_usable(td)


def test_stride_keyword_is_checked(td):
    frm, to = D.pool_model(9, 1, 50)
    with pytest.raises(td.TdError):
        td.pool2_batched([frm], [to], None, None, n=8)
    with pytest.raises(td.TdError):
        td.pool2_batched([frm], [to], None, None, n=2049)
    wide = td.pool2_batched([frm], [to], None, None, n=64)
    tight = td.pool2_batched([frm], [to], None, None)
    assert wide[0].shape == (1, 32) and _rows(wide, 0) == _rows(tight, 0)
