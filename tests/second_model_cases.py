"""Batches that make a workgroup of the "many models per call" kernels take a SECOND model, and their references.

Every such kernel wraps its workgroup in `for (b = blockIdx.x; b < batch; b += gridDim.x)` and the host launches
min(batch, 2^20) workgroups, so with B = GRID + HEAD models, model b >= GRID is the second model of workgroup b - GRID.
Every family below makes the head models [0, HEAD) the largest and fullest, the tail models [GRID, B) different in size
and content (sizes 0 and 1 included, a few of full size: FULL_TAIL), and the middle trivial (size 0 or 1), all from
fixed seeds.  The references are numpy restatements, exact and independent of the library; test_second_model_cpu.py
checks them against the oracle and networkx.  No GPU is needed to import this module.
"""
import functools
import itertools

import numpy as np

GRID = 1 << 20            # the workgroups a batched launch has at most (td_batch.hip, td_match.hip)
HEAD = 4096
B = GRID + HEAD
N = 4                     # the slab stride
BIG = 250000
I32_MIN, I32_MAX = -2**31, 2**31 - 1
ENDS = np.r_[0:HEAD, GRID:B]                                              # the models with real content
FULL_TAIL = tuple(GRID + t for t in (2, 3, 64, 1023, HEAD - 1))           # tail models of the family's full size
INF = 1 << 40


def first_models(a):
    """rows of the models that are a workgroup's first and have content"""
    return a[:HEAD]


def second_models(a):
    """rows of the models that are a workgroup's second"""
    return a[GRID:B]


def slab_sizes(seed, full=N):
    rng = np.random.default_rng(seed)
    ns = np.zeros(B, np.int32)
    ns[:HEAD] = full
    ns[HEAD:GRID] = np.arange(GRID - HEAD) & 1
    tail = rng.integers(0, full, HEAD)
    tail[0], tail[1] = 0, 1
    ns[GRID:] = tail
    ns[list(FULL_TAIL)] = full
    return ns


def in_block(ns):
    k = np.arange(N)
    return (k[None, :, None] < ns[:, None, None]) & (k[None, None, :] < ns[:, None, None])


def _slab(ns, ends_vals, outside_even, outside_odd):
    """(B, N, N) int32: ends_vals at ENDS, a value from the index in the middle, `outside_*` beyond each model's block"""
    slab = np.empty((B, N, N), np.int32)
    slab[0::2] = outside_even
    slab[1::2] = outside_odd
    vals = np.empty((B, N, N), np.int32)
    vals[:] = ((np.arange(B) * 7) % 39 + 1)[:, None, None]
    vals[ENDS] = ends_vals
    inb = in_block(ns)
    slab[inb] = vals[inb]
    return slab


def sample(seed=99, extra=()):
    """the models the oracle runs on: every full-size tail model, its head partner b - GRID, further head, tail and
    middle models"""
    rng = np.random.default_rng(seed)
    s = set(FULL_TAIL) | {b - GRID for b in FULL_TAIL} | {0, 1, HEAD - 1, HEAD, HEAD + 1, GRID - 1, GRID, GRID + 1, B - 1}
    s |= set(rng.choice(HEAD, 100, replace=False).tolist()) | set((GRID + rng.choice(HEAD, 150, replace=False)).tolist())
    s |= {int(b) for b in extra}
    return np.array(sorted(s), np.int64)


# ---- assignment, slab of stride 4 ---------------------------------------------------------------------------------------
PERMS = np.array(list(itertools.permutations(range(N))), np.int64)      # 24 x 4


@functools.lru_cache(maxsize=None)
def assign_batch():
    """-> (slab, ns); outside a block INT32_MIN / INT32_MAX: read once, such a cell wins or overflows the total"""
    ns = slab_sizes(1)
    rng = np.random.default_rng(2)
    shape = (ENDS.size, N, N)
    fam = (ENDS & 3)[:, None, None]
    tied = np.where(rng.random(shape) < 0.3, BIG, rng.integers(10, 41, shape))
    v = np.choose(fam, [rng.integers(1, 40, shape), rng.integers(0, 1000001, shape), rng.integers(-100000, 100000, shape), tied])
    return _slab(ns, v, I32_MIN, I32_MAX), ns


def assign_ref(slab, ns):
    """the optimum of every model: the minimum over the 24 permutations, rows and columns beyond ns[b] pinned to each other"""
    out = np.where(ns == 1, slab[:, 0, 0].astype(np.int64), 0)          # one cell, or no model at all
    sel = np.nonzero(ns >= 2)[0]
    c = np.where(in_block(ns[sel]), slab[sel].astype(np.int64), INF)
    k = np.arange(N)
    beyond = k[None, :] >= ns[sel, None]
    c[:, k, k] = np.where(beyond, 0, c[:, k, k])
    out[sel] = c[:, k[None, :], PERMS].sum(axis=2).min(axis=1)          # models x 24 sums
    return out


# ---- LCM, slab of stride 4 ----------------------------------------------------------------------------------------------
def lcm_rules():
    """tests/test_gpu_batched.py::RULES (library keywords, oracle keywords), and the simulator's rule with a stop_size that
    ends models of 3 and 4 rows early"""
    from test_gpu_batched import RULES
    rules = dict(RULES)
    g, o = RULES["simulator"]
    rules["simulator_stop2"] = (dict(g, stop_size=2), dict(o, stop_size=2))
    return rules


@functools.lru_cache(maxsize=None)
def lcm_batch(rule):
    """-> (slab, ns); outside a block INT32_MIN: it would be every pick if read"""
    names = sorted(lcm_rules())
    ns = slab_sizes(10 + names.index(rule))
    rng = np.random.default_rng(20 + names.index(rule))
    shape = (ENDS.size, N, N)
    if rule == "heuristic":
        v = rng.integers(1, 40, shape)
    elif rule == "greedy_opt":          # threshold 10: some models stop before their last row
        v = np.where(rng.random(shape) < 0.25, BIG, rng.integers(0, 21, shape))
    else:                               # unreachable cells; a model may run out of cells below big_cost
        v = np.where(rng.random(shape) < 0.4, BIG, rng.integers(1, 61, shape))
    return _slab(ns, v, I32_MIN, I32_MIN), ns


def lcm_ref(slab, ns, mask=BIG, threshold=-1, stop_value_on=0, stop_value=0, stop_size=-1, sum_below=2**62, java_scan=0):
    """the oracle's greedy on every model's own block: the first minimum in row-major order, at most ns[b] picks
    -> (total, rows, cols, last_min, n_pairs); rows / cols are -1 beyond n_pairs"""
    nb = ns.astype(np.int64)
    m = slab.shape[0]
    outside = ~in_block(ns)
    d = np.where(outside, INF, slab.astype(np.int64))
    rows, cols = np.full((m, N), -1, np.int32), np.full((m, N), -1, np.int32)
    k, tot = np.zeros(m, np.int64), np.zeros(m, np.int64)
    lm = np.full(m, stop_value, np.int64)
    done = np.zeros(m, bool)
    idx = np.arange(m)
    for it in range(N):
        alive = ~done & (it < nb)
        flat = d.reshape(m, N * N)
        best = flat.argmin(axis=1)
        bv = flat[idx, best]
        if java_scan:
            found = bv < stop_value
            lm = np.where(alive, np.where(found, bv, stop_value), lm)
            stop = ~found
        else:
            lm = np.where(alive, bv, lm)
            stop = np.zeros(m, bool)
            if threshold >= 0:
                stop |= bv > threshold
            if stop_value_on:
                stop |= bv == stop_value
        take = alive & ~stop
        done |= alive & stop
        r, c = best // N, best % N
        t = idx[take]
        rows[t, k[t]] = r[t]
        cols[t, k[t]] = c[t]
        k[t] += 1
        tot[t] += np.where(bv[t] < sum_below, bv[t], 0)
        d[t, r[t], :] = mask
        d[t, :, c[t]] = mask
        d[outside] = INF
        if stop_size >= 0:
            done |= take & (nb - k == stop_size)
    return tot, rows, cols, lm.astype(np.int32), k.astype(np.int32)


# ---- maximum-weight matching, stride 4 ----------------------------------------------------------------------------------
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
MATCHINGS = [()] + [(p,) for p in PAIRS] + [((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2))]   # the 10 of 4 vertices


@functools.lru_cache(maxsize=None)
def match_batch():
    """-> (W, ns); the diagonal and every cell outside a block INT32_MAX: read once, it is the heaviest edge"""
    ns = slab_sizes(30)
    rng = np.random.default_rng(31)
    shape = (ENDS.size, N, N)
    fam = (ENDS & 3)[:, None, None]
    sparse = np.where(rng.random(shape) < 0.6, -rng.integers(0, 5, shape), rng.integers(1, 1000, shape))
    v = np.choose(fam, [rng.integers(1, 6, shape), rng.integers(1, 10**6 + 1, shape), sparse, I32_MAX - rng.integers(0, 1000, shape)])
    W = _slab(ns, v, I32_MAX, I32_MAX)
    k = np.arange(N)
    W[:, k, k] = I32_MAX
    return W, ns


def edge_weights(W, ns):
    """w[b, i, j] = max(W[i][j], W[j][i]) of an edge inside model b (i != j, both below ns[b], weight > 0), else 0"""
    W = W.astype(np.int64)
    w = np.maximum(W, W.transpose(0, 2, 1))
    w[:, np.arange(N), np.arange(N)] = 0
    return np.where(in_block(ns) & (w > 0), w, 0)


def match_ref(W, ns):
    """the maximum over the 10 matchings of 4 vertices; a matching with a pair that is no edge does not count"""
    w = edge_weights(W, ns)
    best = np.zeros(W.shape[0], np.int64)
    for mt in MATCHINGS:
        s = np.zeros(W.shape[0], np.int64)
        for i, j in mt:
            s += np.where(w[:, i, j] > 0, w[:, i, j], -INF)
        best = np.maximum(best, s)
    return best


def check_mates(W, ns, mate, total):
    """mate is a matching of edges inside each model, -1 beyond it, and `total` is its weight (vectorised over the batch)"""
    w = edge_weights(W, ns)
    m = mate.astype(np.int64)
    k = np.arange(N)[None, :]
    has = m >= 0
    assert ((m >= -1) & (m < ns[:, None])).all(), "mate out of range"
    assert not (has & (k >= ns[:, None])).any(), "a vertex beyond ns is matched"
    back = np.take_along_axis(m, np.where(has, m, 0), axis=1)
    assert (back == k)[has].all(), "mates not symmetric"
    we = np.take_along_axis(w, np.where(has, m, 0)[:, :, None], axis=2)[:, :, 0]
    assert (we[has] > 0).all(), "a matched pair is not an edge"
    assert np.array_equal(np.where(has, we, 0).sum(axis=1) // 2, np.asarray(total, np.int64)), "total is not the mates' weight"


# ---- position models (td_build_assign_batched, td_tick_batched) ----------------------------------------------------------
POS_S = 20
BIG_HEAD = np.arange(32) * 128 + 5                                      # d: models of 129..140 cabs
BIG_TAIL = GRID + np.arange(32) * 128 + 5 + (np.arange(32) & 1)          # half of them behind a large head model, half not
ONE_BIG = GRID + 5                                                      # d, second run: the model of 257..260 cabs


def _offsets(sizes):
    off = np.zeros(sizes.size + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    assert off[-1] < 2**31
    return off.astype(np.int32)


@functools.lru_cache(maxsize=None)
def pos_batch(maxk, seed, big=False, one=False):
    """B position models of at most maxk cabs / requests on POS_S stands, about 1 % of the stands outside [0, POS_S);
    big: BIG_HEAD and BIG_TAIL have 129..140 cabs; one: ONE_BIG has 257..260 -> dict(co, cv, do, dv, nc, nd)"""
    rng = np.random.default_rng(seed)
    nc, nd = np.zeros(B, np.int64), np.zeros(B, np.int64)
    nc[:HEAD] = nd[:HEAD] = maxk
    nc[HEAD:GRID] = 1
    nd[HEAD:GRID] = np.arange(GRID - HEAD) & 1
    nc[GRID:], nd[GRID:] = rng.integers(0, maxk + 1, HEAD), rng.integers(0, maxk + 1, HEAD)
    for t, (a, d) in enumerate([(0, 0), (1, 1)]):
        nc[GRID + t], nd[GRID + t] = a, d
    for t, (a, d) in ((4, (0, 3)), (6, (maxk, 0)), (7, (1, maxk))):
        nc[GRID + t], nd[GRID + t] = a, d
    nc[list(FULL_TAIL)] = nd[list(FULL_TAIL)] = maxk
    if big:
        for ix in (BIG_HEAD, BIG_TAIL):
            nc[ix], nd[ix] = rng.integers(129, 141, ix.size), rng.integers(100, 141, ix.size)
    if one:
        nc[ONE_BIG], nd[ONE_BIG] = rng.integers(257, 261), rng.integers(240, 261)
    co, do = _offsets(nc), _offsets(nd)

    def stands(k):
        p = rng.integers(0, POS_S, k).astype(np.int32)
        bad = rng.random(k) < 0.01
        p[bad] = rng.choice(np.array([-1, POS_S, POS_S + 7], np.int32), int(bad.sum()))
        return p

    return {"co": co, "cv": stands(int(co[-1])), "do": do, "dv": stands(int(do[-1])), "nc": nc, "nd": nd}


def pos_table(seed=41, hi=25):
    return np.random.default_rng(seed).integers(0, hi, (POS_S, POS_S)).astype(np.int32)


def ragged_take(off, vals, idx):
    """the models `idx` of a ragged array, in that order, as a batch of their own -> (offsets from 0, values)"""
    idx = np.asarray(idx, np.int64)
    o = off.astype(np.int64)
    sizes = o[idx + 1] - o[idx]
    new = np.zeros(idx.size + 1, np.int64)
    new[1:] = np.cumsum(sizes)
    src = np.repeat(o[idx] - new[:-1], sizes) + np.arange(new[-1])
    return new.astype(np.int32), np.ascontiguousarray(vals[src])


def ragged_model(off, vals, b):
    return vals[int(off[b]):int(off[b + 1])]


# ---- pools of two (td_pool2_batched) -----------------------------------------------------------------------------------
def pool_table():
    """20 stands nearly on a line, asymmetric: 4 |a - b| + U{0..2}, zero diagonal: with max_loss = 1.01 a ride inside another
    one is a candidate only when the noise allows it"""
    rng = np.random.default_rng(51)
    k = np.arange(POS_S)
    t = 4 * np.abs(k[:, None] - k[None, :]) + rng.integers(0, 3, (POS_S, POS_S))
    t[k, k] = 0
    return t.astype(np.int32)


POOL_MAX_LOSS = 1.01


@functools.lru_cache(maxsize=None)
def pool_batch():
    """B pool models of at most 4 customers -> dict(off, frm, to, m)"""
    rng = np.random.default_rng(52)
    m = slab_sizes(53).astype(np.int64)
    m[GRID + 5] = 2
    m[GRID + 6] = 3
    off = _offsets(m)
    k = int(off[-1])
    return {"off": off, "frm": rng.integers(0, POS_S, k).astype(np.int32), "to": rng.integers(0, POS_S, k).astype(np.int32), "m": m}


def pool_padded(p):
    """the customers of every model as (B, 4) arrays (0 beyond a model's size)"""
    m = p["m"]
    k = np.arange(N)[None, :]
    at = np.minimum(p["off"][:-1, None].astype(np.int64) + k, max(p["frm"].size - 1, 0))
    live = k < m[:, None]
    return np.where(live, p["frm"][at], 0), np.where(live, p["to"][at], 0), live


def pair_costs_batch(frm, to, live, table, max_loss):
    """pool_opt_data.pair_costs for every model at once: c[b, A, B] = min(cost1, cost2) of a candidate, else -1"""
    T = np.asarray(table, np.int64)
    d = lambda a, b: T[a, b]
    Af, At, Bf, Bt = frm[:, :, None], to[:, :, None], frm[:, None, :], to[:, None, :]
    ab, bfat, atbt, bfbt, btat, aa = d(Af, Bf), d(Bf, At), d(At, Bt), d(Bf, Bt), d(Bt, At), d(Af, At)
    c1, c2 = ab + bfat + atbt, ab + bfbt + btat
    cand = live[:, :, None] & live[:, None, :] & ~np.eye(N, dtype=bool)[None]
    p1 = ((bfat + atbt) < bfbt * max_loss) & ((ab + bfat) < aa * max_loss)
    p2 = c2 < aa * max_loss
    cand &= p1 | p2
    return np.where(cand, np.minimum(c1, c2), -1)


def lex_weights_batch(c, m):
    """pool_opt_data.lex_weights for every model at once -> (K int64[B], W int64[B, 4, 4])"""
    cand = c >= 0
    mx = np.where(cand, c, -INF).max(axis=(1, 2))
    mn = np.where(cand, c, INF).min(axis=(1, 2))
    anyc = cand.any(axis=(1, 2))
    K = np.where(anyc, (m // 2) * (np.maximum(mx, 0) + np.maximum(-mn, 0)) + 1, 1)
    return K, np.where(cand, K[:, None, None] - c, 0)


# ---- the chunk loop of td_pool2_batched ---------------------------------------------------------------------------------
CHUNK_N = 2048            # the stride: 256 MiB / (4 * 2048^2) = 16 models per chunk
CHUNK_B = 37              # chunks of 16, 16 and 5


@functools.lru_cache(maxsize=None)
def chunk_models():
    """37 models of 0..60 customers on 50 stands -> list of (frm, to)"""
    rng = np.random.default_rng(61)
    sizes = rng.integers(0, 61, CHUNK_B)
    sizes[[0, 15, 16, 31, 32, 36]] = (60, 1, 59, 0, 60, 57)             # both sides of either chunk border, and the last model
    return [(rng.integers(0, 50, int(k)).astype(np.int32), rng.integers(0, 50, int(k)).astype(np.int32)) for k in sizes]


# ---- td_split_batched's region solve ------------------------------------------------------------------------------------
SPLIT_SIZE, SPLIT_PARTS, SPLIT_R = 63, 32, 63     # split_size 1: one range per stand
SPLIT_CASES = 17000                               # 1 071 000 region models; region model c * 63 + r belongs to case c
SPLIT_FIRST, SPLIT_LAST = 300, 700                # the cases that are checked: the first 300 and the last 700


@functools.lru_cache(maxsize=None)
def split_batch():
    """17000 cases of at most 12 cabs / requests on 63 stands -> dict(co, cv, do, dv)"""
    rng = np.random.default_rng(71)
    nc, nd = rng.integers(0, 13, SPLIT_CASES), rng.integers(0, 13, SPLIT_CASES)
    nc[0] = nd[0] = nc[-1] = nd[-1] = 12
    co, do = _offsets(nc), _offsets(nd)
    return {"co": co, "cv": rng.integers(0, SPLIT_SIZE, int(co[-1])).astype(np.int32), "do": do,
            "dv": rng.integers(0, SPLIT_SIZE, int(do[-1])).astype(np.int32)}


def split_checked_cases():
    return np.r_[0:SPLIT_FIRST, SPLIT_CASES - SPLIT_LAST:SPLIT_CASES]
