"""The batched solvers where a workgroup takes a second model.

Every "many models per call" kernel loops `for (b = blockIdx.x; b < batch; b += gridDim.x)` under a grid of
min(batch, 2^20) workgroups, so the batches of tests/second_model_cases.py (B = 2^20 + 4096 models) make model b >= 2^20
the second model of workgroup b - 2^20: the top-of-loop barrier, the LDS state that is set up again, the parity of the
block reduction carried from model to model, the table staged once per workgroup and the matching state reused in LDS all
run between a large, full head model and a different tail model.  Checks: an exact numpy reference for every model of the
slab families; the oracle on a fixed sample for the position and pool families; and for every family the split-call
check: the rows of [0, HEAD) and of [GRID, B) equal those of two small calls in which every model is a first model.
Also here: td_pool2_batched's chunk loop, td_pool_n_batched under a grid below 1024, td_split_batched's region solve past
2^20 region models, and the two model sizes on either side of the place where a matching model's state leaves LDS.

Out of scope: the reuse of a workspace slice by k_match_batched<false> (grid < batch with the state outside LDS).  It
needs more than 3292 models at a stride of at least 1071, a weight slab of 15 GB.
"""
import numpy as np
import pytest

import match_cert
import pool_opt_data as D
import second_model_cases as C
from oracle import oracle

pytestmark = pytest.mark.gpu

GRID, HEAD, B, N, BIG = C.GRID, C.HEAD, C.B, C.N, C.BIG
PARTS = (np.arange(0, HEAD), np.arange(GRID, B))     # the two small calls of the split-call check


def upto(a, k):
    """the entries a[b, :k[b]] of every row, flattened"""
    return a[np.arange(a.shape[1])[None, :] < np.asarray(k)[:, None]]


def assert_permutations(r2c, nb, what):
    """r2c[b, :nb[b]] is a permutation of range(nb[b]) and -1 beyond"""
    k = np.arange(r2c.shape[1])[None, :]
    live = k < np.asarray(nb)[:, None]
    assert (r2c[~live] == -1).all(), what
    assert np.array_equal(np.sort(np.where(live, r2c, r2c.shape[1]), axis=1), np.where(live, k, r2c.shape[1])), what


# ---- a. td_assign_batched -----------------------------------------------------------------------------------------------
def test_assign_batched(td):
    slab, ns = C.assign_batch()
    r2c, total, dual, price = td.assign_batched(slab, ns=ns, want_dual=True, want_prices=True)
    ref = C.assign_ref(slab, ns)
    bad = np.nonzero(total != ref)[0]
    assert bad.size == 0, (bad[:8], total[bad[:8]], ref[bad[:8]])
    assert np.array_equal(dual, total)
    assert_permutations(r2c, ns, "assign")
    live = np.arange(N)[None, :] < ns[:, None]
    assert (price[~live] == 0).all()
    cells = np.take_along_axis(slab.astype(np.int64), np.where(live, r2c, 0).astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    assert np.array_equal(np.where(live, cells, 0).sum(axis=1), total)
    reduced = np.where(C.in_block(ns), slab.astype(np.int64) - price[:, None, :], C.INF).min(axis=2)
    assert np.array_equal(np.where(live, reduced, 0).sum(axis=1) + price.sum(axis=1), total)      # the prices certify the total
    for part in PARTS:
        small = td.assign_batched(slab[part], ns=ns[part], want_dual=True, want_prices=True)
        for x, y in zip(small, (r2c, total, dual, price)):
            assert np.array_equal(x, y[part]), int(part[0])


# ---- b. td_lcm_batched --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["greedy_opt", "heuristic", "simulator", "simulator_stop2"])
def test_lcm_batched(td, rule):
    kw_gpu, kw_oracle = C.lcm_rules()[rule]
    slab, ns = C.lcm_batch(rule)
    total, rows, cols, lm, k = td.LCM_batched(slab, ns=ns, **kw_gpu)
    t_r, rows_r, cols_r, lm_r, k_r = C.lcm_ref(slab, ns, **kw_oracle)
    bad = np.nonzero((k != k_r) | (total != t_r) | (lm != lm_r))[0]
    assert bad.size == 0, (bad[:8], k[bad[:8]], k_r[bad[:8]], total[bad[:8]], t_r[bad[:8]], lm[bad[:8]], lm_r[bad[:8]])
    assert np.array_equal(upto(rows, k), upto(rows_r, k)) and np.array_equal(upto(cols, k), upto(cols_r, k))
    for part in PARTS:
        t_s, rows_s, cols_s, lm_s, k_s = td.LCM_batched(slab[part], ns=ns[part], **kw_gpu)
        assert np.array_equal(k_s, k[part]) and np.array_equal(t_s, total[part]) and np.array_equal(lm_s, lm[part])
        assert np.array_equal(upto(rows_s, k_s), upto(rows[part], k_s)) and np.array_equal(upto(cols_s, k_s), upto(cols[part], k_s))


# ---- c, d. td_build_assign_batched ----------------------------------------------------------------------------------------
THR = 10


def check_position_sample(p, dist, sample, r2c_of, total, dual):
    """the oracle's optimum, the permutation and its cells for the models `sample`; r2c_of(b) -> model b's row"""
    from test_gpu_tick_batched import oracle_cost
    for b in sample:
        cab, dem = C.ragged_model(p["co"], p["cv"], b), C.ragged_model(p["do"], p["dv"], b)
        k, cost = oracle_cost(cab, dem, dist, BIG, THR)
        assert total[b] == (oracle.assign(cost)[0] if k else 0) == dual[b], (b, k)
        row = r2c_of(b)
        assert sorted(row[:k].tolist()) == list(range(k)) and (row[k:] == -1).all(), b
        assert int(cost.astype(np.int64)[np.arange(k), row[:k]].sum()) == total[b], b


def test_build_assign_batched_64_threads(td):
    """at most 4 cabs / requests: k_assign_pos_batched<64, 1>; with the table, its copy in LDS is staged before the first
    model and read by the second"""
    p = C.pos_batch(4, 44)
    nb = np.maximum(p["nc"], p["nd"])
    for dist in (None, C.pos_table()):
        r2c, total, dual = td.build_assign_batched((p["cv"], p["co"]), (p["dv"], p["do"]), dist, fill=BIG, threshold=THR, want_dual=True)
        assert r2c.shape == (B, 4)
        assert np.array_equal(dual, total)
        assert_permutations(r2c, nb, "build_assign")
        check_position_sample(p, dist, C.sample(), lambda b: r2c[b], total, dual)
        for part in PARTS:
            co, cv = C.ragged_take(p["co"], p["cv"], part)
            do, dv = C.ragged_take(p["do"], p["dv"], part)
            r_s, t_s, d_s = td.build_assign_batched((cv, co), (dv, do), dist, fill=BIG, threshold=THR, want_dual=True)
            assert np.array_equal(r_s, r2c[part]) and np.array_equal(t_s, total[part]) and np.array_equal(d_s, dual[part])


@pytest.mark.parametrize("one", [False, True])
def test_build_assign_batched_256_threads(td, one):
    """32 head and 32 tail models of 129..140 cabs: k_assign_pos_batched<256, 1>, four waves, the halves of s_red and the
    parity carried across models; one = True adds a model of 257..260 cabs: <256, 2>.  Outputs stay in device memory (r2c is
    B x 140 and B x 260 int32); the head, the tail and the sample are copied back."""
    import torch
    from taxidispatcher_amd import _ffi
    p = C.pos_batch(4, 44, big=True, one=one)
    nb = np.maximum(p["nc"], p["nd"])
    n = int(nb.max())
    assert 257 <= n <= 260 if one else 129 <= n <= 140
    big = np.r_[C.BIG_HEAD, C.BIG_TAIL, C.BIG_TAIL - GRID] if not one else np.r_[C.BIG_HEAD, C.BIG_TAIL, C.BIG_TAIL - GRID, C.ONE_BIG]
    sample = C.sample(extra=big)
    # the small calls keep the batch's largest model, so that they run the same kernel template
    largest = int(np.argmax(nb))
    parts = [part if nb[part].max() == n else np.r_[part, largest] for part in PARTS]
    for dist in (None, C.pos_table()):
        r2c = torch.full((B, n), -7, dtype=torch.int32, device="cuda")
        tot = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        dua = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        _ffi.check(_ffi.lib().td_build_assign_batched(B, n, _ffi.addr(p["co"]), _ffi.addr(p["cv"]), _ffi.addr(p["do"]), _ffi.addr(p["dv"]),
                                                      _ffi.addr(dist), 0 if dist is None else dist.shape[0], BIG, THR, _ffi.addr(r2c),
                                                      _ffi.addr(tot), _ffi.addr(dua)))
        total, dual = tot.cpu().numpy(), dua.cpu().numpy()
        assert np.array_equal(dual, total)
        rows = dict(zip(sample.tolist(), r2c[torch.from_numpy(sample).cuda()].cpu().numpy()))
        check_position_sample(p, dist, sample, lambda b: rows[int(b)], total, dual)
        for part in parts:
            got = r2c[torch.from_numpy(part).cuda()].cpu().numpy()
            assert_permutations(got, nb[part], "build_assign 256")
            co, cv = C.ragged_take(p["co"], p["cv"], part)
            do, dv = C.ragged_take(p["do"], p["dv"], part)
            r_s, t_s, d_s = td.build_assign_batched((cv, co), (dv, do), dist, fill=BIG, threshold=THR, want_dual=True)
            assert r_s.shape[1] == n
            assert np.array_equal(r_s, got) and np.array_equal(t_s, total[part]) and np.array_equal(d_s, dual[part])
        del r2c, tot, dua
    torch.cuda.empty_cache()


# ---- e. td_tick_batched -------------------------------------------------------------------------------------------------
STOP = 2
TICK_KEYS = ("rows", "cols", "k", "lm", "kc", "kd", "n2", "r2c", "tot", "dual")


def raw_tick(lib, co, cv, do, dv, n, dist, thr):
    """td_tick_batched on host arrays, every output (test_gpu_tick_batched._raw_tick keeps only four)"""
    from taxidispatcher_amd import _ffi
    nb = co.size - 1
    o = {key: np.full((nb, n), -7, np.int32) for key in ("rows", "cols", "kc", "kd", "r2c")}
    o.update({key: np.full(nb, -7, np.int32) for key in ("k", "lm", "n2")})
    o.update({key: np.full(nb, -7, np.int64) for key in ("tot", "dual")})
    _ffi.check(lib.td_tick_batched(nb, n, _ffi.addr(co), _ffi.addr(cv), _ffi.addr(do), _ffi.addr(dv), _ffi.addr(dist),
                                   0 if dist is None else dist.shape[0], BIG, thr, STOP, _ffi.addr(o["rows"]), _ffi.addr(o["cols"]),
                                   _ffi.addr(o["k"]), _ffi.addr(o["lm"]), _ffi.addr(o["kc"]), _ffi.addr(o["kd"]), _ffi.addr(o["n2"]),
                                   _ffi.addr(o["r2c"]), _ffi.addr(o["tot"]), _ffi.addr(o["dual"])))
    return o


def tick_defined(o, nc, nd):
    """every entry of a raw result that the header defines, as a list of arrays"""
    ran = (STOP < np.maximum(nc, nd))
    solved = (o["n2"] > 0) & ~(ran & (o["lm"] == BIG))
    return [o["k"], o["lm"], o["n2"], o["tot"], o["dual"], upto(o["rows"], o["k"]), upto(o["cols"], o["k"]), upto(o["kc"], nc - o["k"]),
            upto(o["kd"], nd - o["k"]), upto(o["r2c"], np.where(solved, o["n2"], 0)), solved]


@pytest.mark.parametrize("table,thr", [(False, 10), (True, 10), (True, 0)])
def test_tick_batched(td, table, thr):
    """at most 6 x 6 with stop_size = 2: every head model runs the LCM, a tail model of at most 2 rows does not and clears
    the masks the head model left; with thr = 0 every cell is fill, the LCM ends on it and the solve gets 0 / 0"""
    from taxidispatcher_amd import _ffi
    from test_gpu_tick_batched import check_tick, oracle_tick
    lib = _ffi.lib()
    p = C.pos_batch(6, 46)
    nc, nd = p["nc"], p["nd"]
    dist = C.pos_table() if table else None
    o = raw_tick(lib, p["co"], p["cv"], p["do"], p["dv"], 6, dist, thr)
    ran = STOP < np.maximum(nc, nd)
    solved = (o["n2"] > 0) & ~(ran & (o["lm"] == BIG))
    assert np.array_equal(o["dual"], o["tot"])
    assert (o["k"][~ran] == 0).all() and (o["lm"][~ran] == BIG).all()
    assert np.array_equal(o["n2"], np.maximum(nc, nd) - o["k"])
    assert_permutations(np.where(solved[:, None], o["r2c"], -1), np.where(solved, o["n2"], 0), "tick")
    assert (o["r2c"][~solved] == -1).all() and (o["tot"][~solved] == 0).all()
    if thr == 0:
        assert not solved[ran].any() and solved[~ran & (o["n2"] > 0)].all()
    else:
        assert solved[ran].mean() > 0.5
    for b in C.sample():
        ref = oracle_tick(C.ragged_model(p["co"], p["cv"], b), C.ragged_model(p["do"], p["dv"], b), dist, BIG, thr, STOP)
        kk, nr = int(o["k"][b]), int(o["n2"][b])
        got = {"lcm_rows": o["rows"][b, :kk], "lcm_cols": o["cols"][b, :kk], "lcm_min_val": int(o["lm"][b]),
               "kept_cabs": o["kc"][b, :nc[b] - kk], "kept_dems": o["kd"][b, :nd[b] - kk], "n_rest": nr,
               "row_to_col": o["r2c"][b, :nr if solved[b] else 0], "total": int(o["tot"][b]), "solved": bool(solved[b]),
               "dual_bound": int(o["dual"][b])}
        check_tick(got, ref, (table, thr, int(b)))
    for part in PARTS:
        co, cv = C.ragged_take(p["co"], p["cv"], part)
        do, dv = C.ragged_take(p["do"], p["dv"], part)
        small = tick_defined(raw_tick(lib, co, cv, do, dv, 6, dist, thr), nc[part], nd[part])
        whole = tick_defined({key: o[key][part] for key in TICK_KEYS}, nc[part], nd[part])
        for x, y in zip(small, whole):
            assert np.array_equal(x, y), int(part[0])


# ---- f. td_split_batched's region solve ---------------------------------------------------------------------------------
def test_split_batched_region_models_past_the_grid(td):
    """17000 cases x 63 ranges = 1 071 000 region models for 2^20 workgroups: the cnt-driven k_assign_pos_batched launch
    strides, and the 22 424 region models of the last 356 cases are second models"""
    import split_model as M
    p = C.split_batch()
    res = td.split_batched((p["cv"], p["co"]), (p["dv"], p["do"]), C.SPLIT_SIZE, C.SPLIT_PARTS)
    assert (res["dual_gap"] == 0).all()
    cases = C.split_checked_cases()

    def case(r, off, c):
        lo, hi = int(off[c]), int(off[c + 1])
        return {"cab_req": r["cab_req"][lo:hi], "cab_stage": r["cab_stage"][lo:hi], "total": r["total"][c], "rest_total": r["rest_total"][c],
                "n_rest": r["n_rest"][c], "dual_gap": r["dual_gap"][c]}

    for c in cases:
        M.check_case(C.ragged_model(p["co"], p["cv"], c), C.ragged_model(p["do"], p["dv"], c), C.SPLIT_SIZE, C.SPLIT_PARTS, None, M.FILL,
                     case(res, p["co"], c))
    co, cv = C.ragged_take(p["co"], p["cv"], cases)
    do, dv = C.ragged_take(p["do"], p["dv"], cases)
    small = td.split_batched((cv, co), (dv, do), C.SPLIT_SIZE, C.SPLIT_PARTS)
    for key in ("total", "rest_total", "n_rest", "dual_gap"):
        assert np.array_equal(small[key], res[key][cases]), key
    for key in ("cab_req", "cab_stage"):
        assert np.array_equal(small[key], C.ragged_take(p["co"], res[key], cases)[1]), key


# ---- g. td_match_batched ------------------------------------------------------------------------------------------------
def test_match_batched(td):
    from test_gpu_pool_opt import check_models
    W, ns = C.match_batch()
    mate, total, bound, (y, par, z) = td.match_batched(W, ns, want_dual=True)
    ref = C.match_ref(W, ns)
    bad = np.nonzero(total != ref)[0]
    assert bad.size == 0, (bad[:8], total[bad[:8]], ref[bad[:8]])
    assert np.array_equal(bound, total)
    C.check_mates(W, ns, mate, total)
    s = C.sample()
    check_models([W[b, :ns[b], :ns[b]] for b in s], mate[s], total[s], bound[s], (y[s], par[s], z[s]))
    for part in PARTS:
        m_s, t_s, b_s, (y_s, _, _) = td.match_batched(W[part], ns[part], want_dual=True)
        assert np.array_equal(m_s, mate[part]) and np.array_equal(t_s, total[part]) and np.array_equal(b_s, bound[part])
        assert np.array_equal(upto(y_s, ns[part]), upto(y[part], ns[part]))


# ---- h. td_pool2_batched, grid-stride -----------------------------------------------------------------------------------
def test_pool2_batched_grid_stride(td):
    """one chunk of B models of at most 4 customers: k_pool_costs, the greedy's LCM, k_pool_match and k_pool_finish all stride"""
    from test_gpu_pool_opt import _check_optimal
    p = C.pool_batch()
    table = C.pool_table()
    off, m = p["off"], p["m"]
    out = {opt: td.pool2_batched((p["frm"], off), (p["to"], off), table, C.POOL_MAX_LOSS, optimal=opt) for opt in (False, True)}
    frm, to, live = C.pool_padded(p)
    c = C.pair_costs_batch(frm, to, live, table, C.POOL_MAX_LOSS)
    K, W = C.lex_weights_batch(c, m)
    for opt in (False, True):
        a, b, plan, cost, k, tot = out[opt]
        assert a.shape == (B, 2) and (k >= 0).all() and (k <= m // 2).all()
        listed = np.arange(2)[None, :] < k[:, None]
        assert np.array_equal(np.where(listed, cost, 0).sum(axis=1), tot)
        at = (np.where(listed, a, 0).astype(np.int64), np.where(listed, b, 0).astype(np.int64))
        assert np.array_equal(upto(c[np.arange(B)[:, None], at[0], at[1]], k), upto(cost, k))    # every pool a candidate at its cost
    a, b, plan, cost, k, tot = out[True]
    assert np.array_equal(k * K - tot, C.match_ref(W, m.astype(np.int32)))                          # the lexicographic optimum
    assert (k >= out[False][4]).all() and (k[:HEAD] > out[False][4][:HEAD]).any()
    for q in C.sample():
        f, t = C.ragged_model(off, p["frm"], q), C.ragged_model(off, p["to"], q)
        c1, p1 = D.pair_costs(f, t, table, C.POOL_MAX_LOSS)
        ga, gb, gplan, gcost, gk, gtot = (x[q] for x in out[False])
        ref = D.greedy(c1)
        assert [(int(ga[i]), int(gb[i]), int(gcost[i])) for i in range(int(gk))] == ref, q
        assert [int(gplan[i]) for i in range(int(gk))] == [int(p1[x, y]) for x, y, _ in ref], q
        _check_optimal(f, t, table, C.POOL_MAX_LOSS, a[q], b[q], plan[q], cost[q], int(k[q]), int(tot[q]), int(gk), int(gtot))
    for part in PARTS:
        o_s, fv = C.ragged_take(off, p["frm"], part)
        _, tv = C.ragged_take(off, p["to"], part)
        for opt in (False, True):
            small = td.pool2_batched((fv, o_s), (tv, o_s), table, C.POOL_MAX_LOSS, optimal=opt)
            k_s = small[4]
            assert np.array_equal(k_s, out[opt][4][part]) and np.array_equal(small[5], out[opt][5][part])
            for x, y in zip(small[:4], out[opt][:4]):
                assert np.array_equal(upto(x, k_s), upto(y[part], k_s)), (opt, int(part[0]))


# ---- i. td_pool2_batched, chunk loop ------------------------------------------------------------------------------------
FILL32 = -77


@pytest.mark.parametrize("optimal", [False, True])
@pytest.mark.parametrize("with_table", [False, True])
def test_pool2_batched_chunk_loop(td, optimal, with_table):
    """a stride of 2048 makes the chunk 16 models, so 37 models run in chunks of 16, 16 and 5: offsets and outputs are
    indexed by b0 + q, the workspace by q.  Every ordered pair is a candidate (max_loss 0), so the greedy is td_pool2's.
    Outputs are device arrays filled beforehand.  The header lists n_pools[b] pools per model and says nothing of the entries
    behind them, so for a host destination (copied back whole from a staging block) nothing can be asked of those; a
    device destination is written in place by the kernel, and there the entries behind a model's pools keep the fill:
    a pool written under another model's index, or a second time, would show."""
    import torch
    from taxidispatcher_amd import _ffi
    from test_gpu_pool_opt import _check_optimal
    models = C.chunk_models()
    table = np.random.default_rng(62).integers(0, 40, (50, 50)).astype(np.int32) if with_table else None
    off = np.zeros(C.CHUNK_B + 1, np.int32)
    off[1:] = np.cumsum([f.size for f, _ in models])
    fv, tv = np.concatenate([f for f, _ in models]), np.concatenate([t for _, t in models])
    half = C.CHUNK_N // 2
    o32 = [torch.full((C.CHUNK_B, half), FILL32, dtype=torch.int32, device="cuda") for _ in range(4)]
    k_d = torch.full((C.CHUNK_B,), FILL32, dtype=torch.int32, device="cuda")
    t_d = torch.full((C.CHUNK_B,), FILL32, dtype=torch.int64, device="cuda")
    _ffi.check(_ffi.lib().td_pool2_batched(C.CHUNK_B, C.CHUNK_N, _ffi.addr(off), _ffi.addr(fv), _ffi.addr(tv), _ffi.addr(table),
                                           0 if table is None else 50, 0.0, int(optimal), *[_ffi.addr(x) for x in o32], _ffi.addr(k_d),
                                           _ffi.addr(t_d)))
    a, b, plan, cost = (x.cpu().numpy() for x in o32)
    k, tot = k_d.cpu().numpy(), t_d.cpu().numpy()
    for q, (f, t) in enumerate(models):
        kk = int(k[q])
        assert kk == (f.size // 2 if f.size >= 2 else 0), q         # every pair is a candidate: a perfect matching, greedy or not
        for x in (a, b, plan, cost):
            assert (x[q, kk:] == FILL32).all(), q
        a1, b1, plan1, cost1, k1, tot1 = td.pool2_batched([f], [t], table, None, optimal=optimal)
        assert k1[0] == kk and tot1[0] == tot[q], q
        for x, y in ((a, a1), (b, b1), (plan, plan1), (cost, cost1)):
            assert x[q, :kk].tolist() == y[0, :kk].tolist(), q
        got = [(int(a[q, i]), int(b[q, i]), int(plan[q, i]), int(cost[q, i])) for i in range(kk)]
        if not optimal:
            assert got == td.find_pool(f, t, table), q
        elif f.size >= 2:
            c, _ = D.pair_costs(f, t, table)
            K, W = D.lex_weights(c)
            _, mt, mb = td.match_batched([W.astype(np.int32)])
            assert mt[0] == mb[0] == kk * K - int(tot[q]), q
            gr = td.pool2_batched([f], [t], table, None, optimal=False)
            _check_optimal(f, t, table, None, a[q], b[q], plan[q], cost[q], kk, int(tot[q]), int(gr[4][0]), int(gr[5][0]))


# ---- j. td_pool_n_batched, reduced grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4])
def test_pool_n_batched_reduced_grid(td, k):
    """max_happy = 2^22, the largest accepted value, leaves 2^30 / (8 * 2^22) = 32 workgroups for 400 tiny models: more
    than 12 models per workgroup and key slab slice.  The 1 GiB key slab this call makes the library keep is grow-only
    workspace, a small part of the device's memory, counted by td_workspace_bytes and released by td_shutdown;
    test_plan_storage_does_not_grow_with_batch, the one test that measures the workspace, shuts the library down and starts
    from zero before it measures, so it sees none of it."""
    import pool_n_batched_cases as pc
    from test_gpu_pool_n_batched import assert_equal_oracle, call
    assert k in pc.KS and len(pc.KS) == 3
    ds = pc.tiny_batch()[:400]
    assert_equal_oracle(call(td, k, ds, max_happy=1 << 22), pc.expected("tiny", k)[:400], ("reduced grid", k))


# ---- k. the matching state boundary -------------------------------------------------------------------------------------
def lds_edge():
    """the largest nmax whose matching state (tdm::bytes(n) = 152 n + 64, rounded up to 256) fits the LDS budget of
    state_plan: min(the device's shared memory per block, 160 KiB) - 1 KiB"""
    import torch
    budget = min(int(torch.cuda.get_device_properties(0).shared_memory_per_block), 160 * 1024) - 1024
    fits = lambda n: ((152 * n + 64 + 255) & ~255) <= budget
    n = 1
    while fits(n + 1):
        n += 1
    assert fits(n) and not fits(n + 1) and 1 <= n < 2047
    return n


@pytest.mark.parametrize("beyond", [0, 1])
def test_match_state_leaves_lds(td, beyond, fam="sparse"):
    """one model of n_lds (state in LDS) or n_lds + 1 vertices (state in the workspace) between two small models, in a slab
    whose stride is n_lds + 1 either way: the largest model, not the stride, decides where the state lives.  Measured on an
    MI355X (n_lds = 1070): "sparse" takes 2.0 s and 3.9 s, "ties" 3.3 s and 6.2 s, so only "sparse" runs here."""
    from test_gpu_pool_opt import check_models
    n_lds = lds_edge()
    print("n_lds = %d" % n_lds)
    n = n_lds + 1
    mats = [D.family("wide", 5, seed=1), D.family(fam, n_lds + beyond, seed=70 + beyond), D.family("ties", 17, seed=2)]
    ns = np.array([w.shape[0] for w in mats], np.int32)
    slab = np.full((3, n, n), 2**31 - 1, np.int32)                     # outside a block: the heaviest edge if read
    for q, w in enumerate(mats):
        slab[q, :ns[q], :ns[q]] = w
    mate, total, bound, duals = td.match_batched(slab, ns, want_dual=True)
    assert np.array_equal(total, bound) and total[1] > 0
    check_models(mats, mate, total, bound, duals)
    alone = td.match_batched([mats[0], mats[2]])
    assert alone[1].tolist() == [int(total[0]), int(total[2])]
