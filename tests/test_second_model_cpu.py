"""CPU checks of tests/second_model_cases.py: the numpy references against the oracle and networkx, the shape of every
family (head largest, tail different with sizes 0, 1 and full, the oracle's sample holding the required models), and the
launch rules in the sources that make model b >= 2^20 a workgroup's second model."""
import os
import re

import numpy as np
import pytest

import match_cert
import pool_opt_data as D
import second_model_cases as C
from oracle import oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "taxidispatcher_amd", "csrc")


def _block(slab, ns, b):
    k = int(ns[b])
    return np.ascontiguousarray(slab[b, :k, :k])


def test_constants():
    assert C.GRID == 1 << 20 and C.HEAD == 4096 and C.B == C.GRID + C.HEAD
    assert all(C.GRID <= b < C.B for b in C.FULL_TAIL)


def test_assign_reference_equals_oracle():
    slab, ns = C.assign_batch()
    ref = C.assign_ref(slab, ns)
    s = C.sample()
    assert s.size >= 256
    for b in s:
        assert ref[b] == (oracle.assign(_block(slab, ns, b))[0] if ns[b] else 0), b
    assert (ref[ns == 0] == 0).all()


@pytest.mark.parametrize("rule", sorted(C.lcm_rules()))
def test_lcm_reference_equals_oracle(rule):
    slab, ns = C.lcm_batch(rule)
    kw = C.lcm_rules()[rule][1]
    tot, rows, cols, lm, k = C.lcm_ref(slab, ns, **kw)
    stopped_early = 0
    for b in C.sample():
        t_o, r_o, c_o, lm_o = oracle.lcm(_block(slab, ns, b), **kw) if ns[b] else (0, np.zeros(0), np.zeros(0), kw.get("stop_value", 0))
        assert k[b] == r_o.size and rows[b, :k[b]].tolist() == r_o.tolist() and cols[b, :k[b]].tolist() == c_o.tolist(), b
        assert (rows[b, k[b]:] == -1).all() and (cols[b, k[b]:] == -1).all()
        assert tot[b] == t_o and lm[b] == lm_o, (b, int(tot[b]), t_o, int(lm[b]), lm_o)
        stopped_early += int(k[b] < ns[b])
    assert (rule == "heuristic") == (stopped_early == 0)      # every other rule ends some models before their last row


def test_match_reference_equals_networkx():
    import networkx as nx
    W, ns = C.match_batch()
    ref = C.match_ref(W, ns)
    for b in C.sample():
        w = match_cert.edge_weights(_block(W, ns, b))
        g = nx.Graph()
        g.add_weighted_edges_from((i, j, int(w[i, j])) for i in range(w.shape[0]) for j in range(i) if w[i, j] > 0)
        assert ref[b] == sum(int(w[i, j]) for i, j in nx.max_weight_matching(g)), b
    # the vectorised mate checker accepts a maximum matching and refuses a wrong total, an asymmetric mate and a pair beyond ns
    b = int(C.FULL_TAIL[0])
    w = C.edge_weights(W[b:b + 1], ns[b:b + 1])[0]
    mates = [m for m in C.MATCHINGS if all(w[i, j] > 0 for i, j in m) and sum(w[i, j] for i, j in m) == ref[b]]
    mate = np.full((1, C.N), -1, np.int32)
    for i, j in mates[0]:
        mate[0, i], mate[0, j] = j, i
    C.check_mates(W[b:b + 1], ns[b:b + 1], mate, ref[b:b + 1])
    with pytest.raises(AssertionError):
        C.check_mates(W[b:b + 1], ns[b:b + 1], mate, ref[b:b + 1] + 1)
    bad = mate.copy()
    bad[0, mates[0][0][0]] = -1
    with pytest.raises(AssertionError):
        C.check_mates(W[b:b + 1], ns[b:b + 1], bad, ref[b:b + 1])
    with pytest.raises(AssertionError):
        C.check_mates(W[b:b + 1], np.array([1], np.int32), mate, ref[b:b + 1])


def test_pool_references_equal_the_restated_script():
    p = C.pool_batch()
    table = C.pool_table()
    frm, to, live = C.pool_padded(p)
    c = C.pair_costs_batch(frm, to, live, table, C.POOL_MAX_LOSS)
    K, W = C.lex_weights_batch(c, p["m"])
    pools = 0
    for b in C.sample():
        m = int(p["m"][b])
        f, t = C.ragged_model(p["off"], p["frm"], b), C.ragged_model(p["off"], p["to"], b)
        assert f.tolist() == frm[b, :m].tolist() and t.tolist() == to[b, :m].tolist()
        c1, _ = D.pair_costs(f, t, table, C.POOL_MAX_LOSS)
        assert np.array_equal(c1, c[b, :m, :m]) and (c[b, m:] == -1).all() and (c[b, :, m:] == -1).all(), b
        K1, W1 = D.lex_weights(c1)
        assert K1 == K[b] and np.array_equal(W1, W[b, :m, :m]), b
        pools += len(D.greedy(c1))
    cand = (c[:C.HEAD] >= 0).sum(axis=(1, 2))
    assert pools > 50 and (cand == 0).any() and (cand >= 4).any()     # the loss test passes some pairs and refuses others


def _assert_head_and_tail(sizes, full, what):
    """the head is of full size, the tail holds 0, 1 and the full size and mostly differs from its head partner"""
    head, tail = C.first_models(sizes), C.second_models(sizes)
    assert (head == full).all(), what
    assert {0, 1, full} <= set(tail.tolist()), what
    assert (tail != head).mean() > 0.5, what
    assert all(sizes[b] == full for b in C.FULL_TAIL), what
    assert (sizes[C.HEAD:C.GRID] <= 1).all(), what


def test_families_have_the_described_shape():
    _assert_head_and_tail(C.assign_batch()[1], C.N, "assign")
    for rule in C.lcm_rules():
        _assert_head_and_tail(C.lcm_batch(rule)[1], C.N, rule)
    _assert_head_and_tail(C.match_batch()[1], C.N, "match")
    _assert_head_and_tail(C.pool_batch()["m"], C.N, "pool2")
    for maxk in (4, 6):
        p = C.pos_batch(maxk, 40 + maxk)
        _assert_head_and_tail(np.maximum(p["nc"], p["nd"]), maxk, ("positions", maxk))
        assert all(p["nc"][b] == p["nd"][b] == maxk for b in C.FULL_TAIL)
        assert ((p["cv"] < 0) | (p["cv"] >= C.POS_S)).any() and ((p["dv"] < 0) | (p["dv"] >= C.POS_S)).any()
    # content: the tail's cells are not its head partner's
    slab, ns = C.assign_batch()
    full = np.array(C.FULL_TAIL)
    assert (slab[full] != slab[full - C.GRID]).any(axis=(1, 2)).all()
    s = set(C.sample().tolist())
    assert len(s) >= 256 and set(C.FULL_TAIL) <= s and {b - C.GRID for b in C.FULL_TAIL} <= s


def test_large_position_models():
    p = C.pos_batch(4, 44, big=True)
    nb = np.maximum(p["nc"], p["nd"])
    assert ((p["nc"][C.BIG_HEAD] >= 129) & (p["nc"][C.BIG_HEAD] <= 140)).all() and (C.BIG_HEAD < C.HEAD).all()
    assert ((p["nc"][C.BIG_TAIL] >= 129) & (p["nc"][C.BIG_TAIL] <= 140)).all() and (C.BIG_TAIL >= C.GRID).all() and (C.BIG_TAIL < C.B).all()
    assert 128 < nb.max() <= 140                                       # nl > 128: the 256-thread template, one column per thread
    behind_big = np.isin(C.BIG_TAIL - C.GRID, C.BIG_HEAD)
    assert behind_big.any() and not behind_big.all()
    q = C.pos_batch(4, 44, big=True, one=True)
    assert 257 <= q["nc"][C.ONE_BIG] <= 260 and np.maximum(q["nc"], q["nd"]).max() == q["nc"][C.ONE_BIG]   # CPT = 2
    assert C.ONE_BIG >= C.GRID and (C.ONE_BIG - C.GRID) in C.BIG_HEAD
    s = C.sample(extra=np.r_[C.BIG_HEAD, C.BIG_TAIL, C.BIG_TAIL - C.GRID, C.ONE_BIG])
    assert set(C.BIG_TAIL.tolist()) <= set(s.tolist())


def test_tick_batch_takes_both_lcm_branches():
    p = C.pos_batch(6, 46)
    nb = np.maximum(p["nc"], p["nd"])
    stop = 2
    assert (C.first_models(nb) > stop).all()                           # every head model runs the LCM
    tail = C.second_models(nb)
    assert (tail <= stop).sum() > 100 and (tail > stop).sum() > 100    # behind it: models that skip it and models that run it


def test_split_batch_crosses_the_grid():
    p = C.split_batch()
    assert C.SPLIT_SIZE // C.SPLIT_PARTS == 1 and C.SPLIT_R == len(range(0, C.SPLIT_SIZE, C.SPLIT_SIZE // C.SPLIT_PARTS))
    assert C.SPLIT_CASES * C.SPLIT_R == 1071000 > C.GRID
    nc, nd = np.diff(p["co"]), np.diff(p["do"])
    assert max(nc.max(), nd.max()) == 12
    cases = C.split_checked_cases()
    assert cases.size == 1000
    first_model, last_model = cases * C.SPLIT_R, cases * C.SPLIT_R + C.SPLIT_R - 1
    assert (last_model < C.GRID).sum() >= 300 and (first_model >= C.GRID).sum() > 300   # region models on both sides of GRID
    straddling = cases[(first_model < C.GRID) & (last_model >= C.GRID)]
    assert straddling.tolist() == [C.GRID // C.SPLIT_R]
    # the checked cases alone are fewer region models than workgroups: in that call every model is a first model
    assert cases.size * C.SPLIT_R < C.GRID


def test_chunk_models():
    ms = C.chunk_models()
    sizes = [f.size for f, _ in ms]
    assert len(ms) == C.CHUNK_B == 37 and min(sizes) == 0 and max(sizes) == 60 and 1 in sizes
    chunk = (256 << 20) // (4 * C.CHUNK_N * C.CHUNK_N)
    assert chunk == 16 and [min(chunk, C.CHUNK_B - b0) for b0 in range(0, C.CHUNK_B, chunk)] == [16, 16, 5]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_launch_rules_still_make_second_models():
    """the GPU tests of test_gpu_second_model.py reach a workgroup's second model only while these caps stand; if one
    changes, the batches of second_model_cases.py have to follow"""
    batch = _src("td_batch.hip")
    # k_assign_batched, k_assign_pos_batched, k_tick_lcm_batched, k_pool2_lcm_batched, k_lcm_batched
    assert batch.count("const int grid = std::min(batch, 1 << 20);") == 5
    assert len(re.findall(r"for \(int b = blockIdx\.x; b < batch; b \+= gridDim\.x\)", batch)) == 5
    assert "constexpr int SPLIT_GRID = 2048;" in batch
    match = _src("td_match.hip")
    assert "*grid = std::min(batch, 1 << 20);" in match                 # state_plan: k_match_batched, k_pool_match
    assert "const int grid = std::min(nq, 1 << 20);" in match           # k_pool_costs, k_pool_finish
    assert "((size_t)256 << 20) / (sizeof(int32_t) * NN)" in match      # the pool chunk
    assert "*lds = *per <= lds_budget();" in match and "*per = align256(tdm::bytes(std::max(nmax, 1)));" in match
    assert "std::min<size_t>((size_t)v, 160 * 1024) - 1024" in match
    core = _src("td_match_core.h")
    assert "size_t bytes(int n) { return (size_t)n * (2 * 2 * 8 + 6 * 4 + 2 * 4 + 11 * 2 * 4) + 64; }" in core
    assert 2 * 2 * 8 + 6 * 4 + 2 * 4 + 11 * 2 * 4 == 152
    pool = _src("td_pool_batch.hip")
    assert "constexpr int PNB_GRID = 1024;" in pool
    assert "constexpr size_t PNB_SLAB_BYTES = (size_t)1 << 30;" in pool
    assert "std::min<size_t>((size_t)PNB_GRID, PNB_SLAB_BYTES / (sizeof(unsigned long long) * (size_t)max_happy))" in pool
    assert (1 << 30) // (8 * (1 << 22)) == 32
