"""GPU tests of td_match_batched / td_pool2_batched (csrc/td_match.hip): maximum-weight matching of many general graphs
per call, certified by the device and re-checked by tests/match_cert.py, and the greedy / optimal pools of two of
pool_opt_min.py.  Expected answers: tests/golden/pool_opt/golden.json (networkx, by make_pool_opt_golden.py)."""
import json
import os

import numpy as np
import pytest

import match_cert
import pool_opt_data as D

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_opt", "golden.json")))


def check_models(mats, mate, total, bound, duals):
    """every model of a match_batched result against the numpy certificate checker"""
    y, par, z = duals
    n = mate.shape[1]
    for k, W in enumerate(mats):
        m = W.shape[0]
        conv = lambda a: np.where(a >= n, a - n + m, a)   # exported blossom ids n + k -> the checker's m + k
        parent = np.concatenate([conv(par[k, :m]), conv(par[k, n:n + m])])
        match_cert.check(W, mate[k, :m], total[k], bound[k], y[k, :m], parent, z[k, :m])
        assert (mate[k, m:] == -1).all()


def test_blossom_cases(td):
    names = sorted(D.BLOSSOM_CASES)
    mats = [D.blossom_matrix(D.BLOSSOM_CASES[k]) for k in names]
    mate, total, bound, duals = td.match_batched(mats, want_dual=True)
    for k, name in enumerate(names):
        g = GOLD["blossom"][name]
        m = mats[k].shape[0]
        assert mate[k, :m].tolist() == g["mate"], name
        assert total[k] == bound[k] == g["total"], name
    check_models(mats, mate, total, bound, duals)


@pytest.mark.parametrize("fam", D.FAMILIES)
def test_families_golden(td, fam):
    order = np.random.default_rng(3).permutation(len(D.SIZES))
    sizes = [D.SIZES[i] for i in order]
    mats = [D.family(fam, n) for n in sizes]
    mate, total, bound, duals = td.match_batched(mats, want_dual=True)
    for k, n in enumerate(sizes):
        assert total[k] == bound[k] == GOLD["families"][fam][str(n)], (fam, n)
    check_models(mats, mate, total, bound, duals)


def test_large_models(td):
    """n = 1024 and n = 2048 models and the 1445-customer every-pair pool model of 50 stands (|a - b|) as lexicographic
    weights (the largest models take seconds each: DESIGN.md 3.5)"""
    W1 = D.family("wide", 1024, seed=11)
    W3 = D.family("sparse", 2048, seed=12)
    frm, to = D.pool_model(1445, 1445, 50)
    c, _ = D.pair_costs(frm, to)
    K, W2 = D.lex_weights(c)
    W2 = W2.astype(np.int32)
    totals = []
    for W in (W1, W2, W3):
        mate, total, bound, duals = td.match_batched([W], want_dual=True)
        assert total[0] == bound[0]
        check_models([W], mate, total, bound, duals)
        totals.append(int(total[0]))
    # the pool path answers the same model alike: count and total from the same optimum
    a, b, plan, cost, k, tot = td.pool2_batched([frm], [to], None, None, optimal=True)
    assert int(k[0]) * K - int(tot[0]) == totals[1]


def _models(rng, count, S, lo=0, hi=120):
    sizes = rng.integers(lo, hi, count)
    return [D.pool_model(int(m), int(rng.integers(1 << 30)), S) for m in sizes]


@pytest.mark.parametrize("with_table", [False, True])
def test_pool2_greedy_equals_find_pool(td, with_table):
    rng = np.random.default_rng(21 + with_table)
    S = 50
    table = rng.integers(0, 40, (S, S)).astype(np.int32) if with_table else None
    models = _models(rng, 64, S)
    a, b, plan, cost, k, tot = td.pool2_batched([m[0] for m in models], [m[1] for m in models], table, None, optimal=False)
    for q, (frm, to) in enumerate(models):
        ref = td.find_pool(frm, to, table)
        got = [(int(a[q, i]), int(b[q, i]), int(plan[q, i]), int(cost[q, i])) for i in range(int(k[q]))]
        assert got == ref, q
        assert int(tot[q]) == sum(r[3] for r in ref)


def test_pool2_greedy_max_loss(td):
    rng = np.random.default_rng(5)
    table = D.pool_table()
    models = _models(rng, 48, 100, 0, 200)
    a, b, plan, cost, k, tot = td.pool2_batched([m[0] for m in models], [m[1] for m in models], table, 1.01, optimal=False)
    for q, (frm, to) in enumerate(models):
        c, p1 = D.pair_costs(frm, to, table, 1.01)
        ref = D.greedy(c)
        got = [(int(a[q, i]), int(b[q, i]), int(cost[q, i])) for i in range(int(k[q]))]
        assert got == ref, q
        assert [int(plan[q, i]) for i in range(int(k[q]))] == [int(p1[x, y]) for x, y, _ in ref]


def _check_optimal(frm, to, table, ml, a, b, plan, cost, k, tot, greedy_k, greedy_t):
    c, p1 = D.pair_costs(frm, to, table, ml)
    pools = [(int(a[i]), int(b[i]), int(plan[i]), int(cost[i])) for i in range(k)]
    used = [x for p in pools for x in p[:2]]
    assert len(used) == len(set(used)), "pools share a customer"
    for x, y, pl, co in pools:
        assert c[x, y] >= 0 and co == c[x, y] and pl == int(p1[x, y])
        assert c[y, x] < 0 or c[y, x] > co or (c[y, x] == co and x < y), "not the cheaper direction"
    assert pools == sorted(pools, key=lambda p: (p[3], p[0], p[1]))
    assert tot == sum(p[3] for p in pools)
    assert k >= greedy_k and (k > greedy_k or tot <= greedy_t)


def test_pool2_optimal_golden(td):
    for tab in (True, False):
        cases = [cs for cs in D.POOL_CASES if cs[3] == tab]
        ml = cases[0][4]
        table = D.pool_table() if tab else None
        models = [D.pool_model(m, seed, 100 if tab else 50) for _, m, seed, _, _ in cases]
        froms, tos = [x[0] for x in models], [x[1] for x in models]
        opt = td.pool2_batched(froms, tos, table, ml, optimal=True)
        gr = td.pool2_batched(froms, tos, table, ml, optimal=False)
        for q, (name, m, *_rest) in enumerate(cases):
            g = GOLD["pools"][name]
            assert (int(opt[4][q]), int(opt[5][q])) == (g["count"], g["total"]), name
            _check_optimal(models[q][0], models[q][1], table, ml, *(x[q] for x in opt[:4]), int(opt[4][q]), int(opt[5][q]),
                           int(gr[4][q]), int(gr[5][q]))


def test_pool2_optimal_matches_match_batched(td):
    """models above the golden sizes: the optimum's (count, total) is the matching of K - w weights"""
    rng = np.random.default_rng(8)
    models = [D.pool_model(m, int(rng.integers(1 << 30)), 50) for m in (400, 517, 640)]
    opt = td.pool2_batched([x[0] for x in models], [x[1] for x in models], None, None, optimal=True)
    gr = td.pool2_batched([x[0] for x in models], [x[1] for x in models], None, None, optimal=False)
    for q, (frm, to) in enumerate(models):
        c, _ = D.pair_costs(frm, to)
        K, W = D.lex_weights(c)
        _, total, bound = td.match_batched([W.astype(np.int32)])
        assert total[0] == bound[0] == int(opt[4][q]) * K - int(opt[5][q])
        _check_optimal(frm, to, None, None, *(x[q] for x in opt[:4]), int(opt[4][q]), int(opt[5][q]), int(gr[4][q]), int(gr[5][q]))


def test_find_pool_optimal(td):
    frm, to = D.pool_model(90, 4, 50)
    got = td.find_pool_optimal(frm, to)
    a, b, plan, cost, k, tot = td.pool2_batched([frm], [to], None, None, optimal=True)
    assert got == [(int(a[0, i]), int(b[0, i]), int(plan[0, i]), int(cost[0, i])) for i in range(int(k[0]))]
    assert len(got) == 45   # every ordered pair is a candidate: a perfect matching


def test_pool_gap(td):
    gt, ot, gk, ok, gap = td.pool_gap(100, 1000, seed=9)
    assert gt.shape == ot.shape == gk.shape == ok.shape == (1000,)
    assert (ok >= gk).all() and ((ok > gk) | (ot <= gt)).all()
    eq = (ok == gk) & (ot > 0)
    assert eq.any() and np.isfinite(gap) and gap >= 0
    assert abs(gap - float(np.mean(100.0 * (gt[eq] - ot[eq]) / ot[eq]))) < 1e-9


def test_device_inputs(td):
    import torch
    mats = [D.family("ties", n, seed=n) for n in (17, 64, 100)]
    slab = np.zeros((3, 100, 100), np.int32)
    for k, W in enumerate(mats):
        slab[k, :W.shape[0], :W.shape[0]] = W
    ns = np.array([17, 64, 100], np.int32)
    host = td.match_batched(slab, ns)
    dev = td.match_batched(torch.from_numpy(slab).cuda(), torch.from_numpy(ns).cuda())
    for x, y in zip(host, dev):
        assert np.array_equal(x, y)
    rng = np.random.default_rng(2)
    models = _models(rng, 16, 100, 0, 150)
    fv = np.concatenate([m[0] for m in models])
    tv = np.concatenate([m[1] for m in models])
    off = np.zeros(17, np.int32)
    off[1:] = np.cumsum([m[0].size for m in models])
    table = D.pool_table()
    for optimal in (False, True):
        h = td.pool2_batched([m[0] for m in models], [m[1] for m in models], table, 1.01, optimal=optimal)
        to_dev = lambda x: torch.from_numpy(x).cuda()
        d = td.pool2_batched((to_dev(fv), to_dev(off)), (to_dev(tv), to_dev(off)), to_dev(table), 1.01, optimal=optimal)
        for x, y in zip(h, d):
            assert np.array_equal(x, y)


def test_cells_beyond_2_31(td):
    """B * n * n > 2^31 cells: the last model's block lies past 2^31 cells and is read correctly"""
    import torch
    B, n = 513, 2048
    W = D.family("wide", 200, seed=5)
    slab = torch.zeros((B, n, n), dtype=torch.int32, device="cuda")
    slab[B - 1, :200, :200] = torch.from_numpy(W).cuda()
    ns = torch.zeros(B, dtype=torch.int32, device="cuda")
    ns[B - 1] = 200
    mate, total, bound = td.match_batched(slab, ns)
    ref = td.match_batched([W])
    assert total[B - 1] == bound[B - 1] == ref[1][0] and (total[:B - 1] == 0).all()
    assert np.array_equal(mate[B - 1, :200], ref[0][0])
    del slab
    torch.cuda.empty_cache()


def test_invalid_arguments(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    with pytest.raises(td.TdError):
        td.match_batched(np.zeros((1, 2049, 2049), np.int32))
    with pytest.raises(td.TdError):
        td.match_batched(np.zeros((2, 8, 8), np.int32), np.array([3, 9], np.int32))
    with pytest.raises(td.TdError):
        td.match_batched(np.zeros((2, 8, 8), np.int32), np.array([3, -1], np.int32))
    z = np.zeros(64, np.int64)
    zi = np.zeros(64, np.int32)
    assert lib.td_match_batched(-1, 4, None, zi.ctypes.data, zi.ctypes.data, z.ctypes.data, None, None, None, None) == -1
    assert lib.td_match_batched(0, 4, None, None, None, None, None, None, None, None) == 0   # a batch of 0 is a no-op
    frm = np.array([1, 2, 3, 4], np.int32)
    to = np.array([2, 3, 4, 5], np.int32)
    outs = [np.zeros(64, np.int32) for _ in range(5)] + [z]
    addrs = [o.ctypes.data for o in outs]

    def call(batch, n, off, f=frm, t=to, dist=None, S=0):
        return lib.td_pool2_batched(batch, n, np.asarray(off, np.int32).ctypes.data, f.ctypes.data, t.ctypes.data,
                                    None if dist is None else dist.ctypes.data, S, 0.0, 1, *addrs)

    assert call(1, 4, [0, 4]) == 0
    assert call(1, 2049, [0, 4]) == -1           # n > 2048
    assert call(-1, 4, [0, 4]) == -1             # batch < 0
    assert call(1, 4, [1, 4]) == -1              # off[0] != 0
    assert call(2, 4, [0, 3, 2]) == -1           # decreasing offsets
    assert call(1, 3, [0, 4]) == -1              # a model larger than n
    assert call(0, 4, [0]) == 0                  # no-op
    tab = np.zeros((5, 5), np.int32)
    assert call(1, 4, [0, 4], dist=tab, S=5) == -1   # stand 5 outside the 5 x 5 table
    with pytest.raises(td.TdError):
        td.pool2_batched([frm], [to], tab)
    with pytest.raises(td.TdError):
        td.pool2_batched([frm], [to[:3]])


def test_range_checks(td):
    """pool costs near 2^31: the greedy takes them as td_pool2 does; the optimum's weights K - cost would reach 2^33, and
    that call fails with TD_ERANGE (not TD_EINTERNAL)"""
    rng = np.random.default_rng(13)
    S = 6
    table = rng.choice(np.array([1, 700_000_000], np.int32), (S, S)).astype(np.int32)
    models = [D.pool_model(m, 40 + m, S) for m in (10, 17, 2)]
    froms, tos = [x[0] for x in models], [x[1] for x in models]
    a, b, plan, cost, k, tot = td.pool2_batched(froms, tos, table, None, optimal=False)
    c, _ = D.pair_costs(froms[0], tos[0], table)
    K, _ = D.lex_weights(c)
    assert c.max() > 2_000_000_000 and K + c.max() >= 2**33
    for q, (frm, to) in enumerate(models):
        got = [(int(a[q, i]), int(b[q, i]), int(plan[q, i]), int(cost[q, i])) for i in range(int(k[q]))]
        assert got == td.find_pool(frm, to, table), q
    with pytest.raises(td.TdError, match="error -4"):
        td.pool2_batched(froms, tos, table, None, optimal=True)
    # the library stays usable after the refused call
    assert td.pool2_batched([froms[2]], [tos[2]], table, None, optimal=True)[4][0] == 1
