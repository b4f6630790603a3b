"""The models of the td_pool_n_batched tests and their oracle answers, each computed once per process.

Demand recipe: tests/test_gpu_pool.py::random_demand (stands 0..49 unless stated, trips of +-1..8 stands), seeds fixed
here.  Every batch names the max_happy its GPU test passes (0 = the library's default, 65536 plans per model);
test_pool_n_batched_cpu.py checks with the oracle that every model stays within HALF of it and that every cost fits
the key, so the GPU tests never run near the capacity by accident (the capacity edge has its own test).
"""
import functools

import numpy as np

import pool_fixtures as pf
from oracle import oracle

DEFAULT_MAX_HAPPY = 65536
KS = (2, 3, 4)


def random_demand(rng, n, max_wait, losses, stands=50):
    frm = rng.integers(0, stands, n)
    to = np.clip(frm + rng.integers(1, 9, n) * rng.choice([-1, 1], n), 0, stands - 1)
    to = np.where(to == frm, np.where(frm > 0, frm - 1, 1), to)
    return np.stack([np.arange(n), frm, to, rng.integers(0, max_wait + 1, n), rng.choice(losses, n)], 1)


# ---- 1. tiny models, more of them than the library launches workgroups (its grid cap is 1024) ----------------------
TINY_B = 6000
TINY_SEED = 11
TINY_MAX_HAPPY = 16384


@functools.lru_cache(maxsize=None)
def tiny_batch():
    """6000 models of 0..9 requests on 8 stands, max_wait <= 9, loss 90: many equal costs, n_b < k, == k and 0 included"""
    rng = np.random.default_rng(TINY_SEED)
    sizes = rng.integers(0, 10, TINY_B)
    sizes[:6] = (0, 1, 2, 3, 4, 9)
    return [random_demand(rng, int(m), 9, [90], stands=8) for m in sizes]


# ---- 2. mixed sizes in one batch, stride 256 -----------------------------------------------------------------------
MIXED_SEED = 23
MIXED_SIZES = (3, 17, 64, 100, 128, 256)
MIXED_N = 256
MIXED_MAX_HAPPY = 1 << 18


def _mixed_recipe(m):
    if m <= 17:
        return dict(max_wait=9, losses=[90], stands=8)
    if m <= 128:
        return dict(max_wait=3, losses=[1, 10, 30])
    return dict(max_wait=2, losses=[1, 10, 25])


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """24 models, four of every size, in a fixed shuffled order"""
    rng = np.random.default_rng(MIXED_SEED)
    sizes = list(MIXED_SIZES) * 4
    rng.shuffle(sizes)
    return [random_demand(rng, int(m), **_mixed_recipe(int(m))) for m in sizes]


TABLE_SEED = 31
TABLE_S = 30
TABLE_B = 6
TABLE_MAX_HAPPY = 1 << 19


@functools.lru_cache(maxsize=None)
def table_batch():
    """test_pool_n_random_vs_oracle's table: asymmetric 30 x 30, entries 0..11, zero diagonal; models of 80 requests"""
    rng = np.random.default_rng(TABLE_SEED)
    dist = rng.integers(0, 12, (TABLE_S, TABLE_S)).astype(np.int32)
    np.fill_diagonal(dist, 0)
    return dist, [random_demand(rng, 80, 6, [20, 60], stands=TABLE_S) for _ in range(TABLE_B)]


# ---- 3. the size limit: one model of 512 requests ------------------------------------------------------------------
LIMIT_SEED = {2: 3, 3: 3, 4: 6}
LIMIT_MAX_HAPPY = {2: 0, 3: 0, 4: 1 << 19}


@functools.lru_cache(maxsize=None)
def limit_model(k):
    rng = np.random.default_rng(LIMIT_SEED[k])
    if k == 4:
        return random_demand(rng, 512, 0, [1, 5, 20])
    return random_demand(rng, 512, 1, [1, 5])


# ---- 4. the reference binary's fixtures: the 8 children of one demand as one batch ---------------------------------
FIXTURE_MAX_HAPPY = 0


def fixture_batch(name, k):
    """-> demands (the same demand 8 times), firsts (the children's slices), expected lists child by child"""
    d, exp = pf.load(name, k)
    firsts = [pf.child_slice(len(d), c) for c in range(8)]
    return [d] * 8, firsts, [exp[c] for c in range(8)]


# ---- 7. the capacity edge: one 100-request model -------------------------------------------------------------------
def edge_model():
    return next(d for d in mixed_batch() if len(d) == 100)


# ---- oracle answers -------------------------------------------------------------------------------------------------
def eff(max_happy):
    return max_happy if max_happy > 0 else DEFAULT_MAX_HAPPY


def oracle_model(k, d, dist=None, first=None, cap=200000):
    """-> (records as a list of lists, happy plans) of one model"""
    f0, f1 = (0, len(d)) if first is None else first
    if len(d) == 0:
        return [], 0
    got, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], dist, f0, f1, cap=cap)
    return got.tolist(), nh


@functools.lru_cache(maxsize=None)
def expected(name, k):
    """-> list of (records, happy plans) per model of the named batch.  The oracle's cap is HALF the batch's max_happy (it
    zero-fills cap records per call, so a small cap also keeps 18000 calls quick): a model beyond it raises OverflowError
    here, and the inputs, not the library, are then at fault"""
    for name_, demands, dist, max_happy in batches(k):
        if name_ == name:
            return [oracle_model(k, d, dist, cap=eff(max_happy) // 2) for d in demands]
    raise KeyError(name)


def batches(k):
    """every generated batch of the module: (name, demands, dist, max_happy)"""
    return [("tiny", tiny_batch(), None, TINY_MAX_HAPPY), ("mixed", mixed_batch(), None, MIXED_MAX_HAPPY),
            ("table", table_batch()[1], table_batch()[0], TABLE_MAX_HAPPY), ("limit", [limit_model(k)], None, LIMIT_MAX_HAPPY[k])]
