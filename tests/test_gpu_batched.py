"""GPU tests of the batched entry points (td_assign_batched / td_lcm_batched, csrc/td_batch.hip): every model of a
batch against the CPU oracle — totals, permutations, the dual certificate from the cells and from the column prices,
LCM pair lists bit-exact — plus ragged batches, device input, more than 2^31 cells and argument errors."""

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu
BIG = 250000
I32_MIN, I32_MAX = -2**31, 2**31 - 1
FAMILIES = ("g4", "g1", "wide", "neg", "const", "absdiff", "padded")


def make(kind, n, rng):
    if kind == "g4":        # heuristic.py:21 U{1..39}
        return rng.integers(1, 40, (n, n)).astype(np.int32)
    if kind == "g1":        # perf.jl:5 U{10..40}, heavily tied
        return rng.integers(10, 41, (n, n)).astype(np.int32)
    if kind == "wide":
        return rng.integers(0, 1000001, (n, n)).astype(np.int32)
    if kind == "neg":
        return rng.integers(-100000, 100000, (n, n)).astype(np.int32)
    if kind == "const":
        return np.full((n, n), int(rng.integers(-50, 50)), np.int32)
    if kind == "absdiff":   # |a - b| (greedy_opt.py:122-127)
        a, b = rng.integers(0, 10 * n + 1, n), rng.integers(0, 10 * n + 1, n)
        return np.abs(a[:, None] - b[None, :]).astype(np.int32)
    if kind == "padded":    # a cost_build model: fewer requests than cabs, dummy columns = fill, threshold 10
        n_d = max(1, (2 * n) // 3)
        cab, dem = rng.integers(0, 50, n), rng.integers(0, 50, n_d)
        return oracle.cost_build(cab, dem, None, fill=BIG, threshold=10)[1]
    raise ValueError(kind)


def batch_for(n):
    return 64 if n <= 64 else 16 if n <= 129 else 8 if n <= 300 else 4


def numpy_dual(c, v):
    c = c.astype(np.int64)
    return int((c - v[None, :]).min(axis=1).sum() + v.sum()) if c.size else 0


def check_models(mats, r2c, total, dual, price):
    for b, c in enumerate(mats):
        k = c.shape[0]
        ref = oracle.assign(c)[0]
        assert total[b] == ref, (b, k, int(total[b]), ref)
        p = r2c[b, :k]
        assert sorted(p.tolist()) == list(range(k)), b
        assert int(c.astype(np.int64)[np.arange(k), p].sum()) == total[b]
        assert dual[b] == total[b], (b, int(dual[b]), int(total[b]))
        assert numpy_dual(c, price[b, :k]) == total[b], b


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 100, 127, 128, 129, 255, 256, 300, 512, 1024])
def test_assign_batched_totals_vs_oracle(td, n):
    rng = np.random.default_rng(1000 + n)
    B = batch_for(n)
    for fam in FAMILIES:
        mats = [make(fam, n, rng) for _ in range(B)]
        slab = np.ascontiguousarray(np.stack(mats))
        r2c, total, dual, price = td.assign_batched(slab, want_dual=True, want_prices=True)
        assert r2c.shape == (B, n) and total.shape == (B,) and price.shape == (B, n)
        check_models(mats, r2c, total, dual, price)


@pytest.mark.parametrize("n", [5, 100, 200, 700])
def test_assign_batched_ragged(td, n):
    """ns with 0, 1 and n; every cell outside a model's block is INT32_MIN / INT32_MAX: read once, it would win or
    overflow the total.  The row_to_col tail is -1, the price tail 0."""
    rng = np.random.default_rng(7 + n)
    ns = np.array([0, 1, n, n // 2, 2, n - 1, n, 3][: 8], np.int32).clip(0, n)
    B = ns.size
    slab = np.empty((B, n, n), np.int32)
    slab[0::2] = I32_MIN
    slab[1::2] = I32_MAX
    mats = []
    for b, k in enumerate(ns):
        c = make(("g4", "wide", "neg", "padded")[b % 4], int(k), rng) if k else np.zeros((0, 0), np.int32)
        slab[b, :k, :k] = c
        mats.append(c)
    r2c, total, dual, price = td.assign_batched(slab, ns=ns, want_dual=True, want_prices=True)
    check_models(mats, r2c, total, dual, price)
    for b, k in enumerate(ns):
        assert (r2c[b, k:] == -1).all() and (price[b, k:] == 0).all()
    assert total[0] == dual[0] == 0
    # the same models as a list of arrays: packed with ns by the wrapper
    r2c_l, total_l = td.assign_batched(mats)
    assert np.array_equal(total_l, total)


def test_assign_batched_device_input(td):
    import torch
    rng = np.random.default_rng(11)
    for n, B in ((100, 40), (300, 6)):
        slab = np.stack([make(("g1", "wide", "absdiff")[b % 3], n, rng) for b in range(B)])
        ns = np.full(B, n, np.int32)
        ns[1] = n // 3
        r_h, t_h, d_h, p_h = td.assign_batched(slab, ns=ns, want_dual=True, want_prices=True)
        dev = torch.from_numpy(slab).cuda()
        r_d, t_d, d_d, p_d = td.assign_batched(dev, ns=torch.from_numpy(ns).cuda(), want_dual=True, want_prices=True)
        assert np.array_equal(r_h, r_d) and np.array_equal(t_h, t_d) and np.array_equal(d_h, d_d) and np.array_equal(p_h, p_d)
        solver = td.Solver()
        try:
            for b in range(B):
                k = int(ns[b])
                c = np.ascontiguousarray(slab[b, :k, :k])
                assert td.assign(c)[1] == t_h[b] == solver.assign(c)[1]
        finally:
            solver.close()


def test_assign_batched_device_outputs(td):
    """outputs in device memory through the C ABI: the same numbers as host outputs"""
    import torch
    from taxidispatcher_amd import _ffi
    rng = np.random.default_rng(5)
    B, n = 12, 90
    slab = np.stack([make("g4", n, rng) for _ in range(B)])
    r_h, t_h, d_h, p_h = td.assign_batched(slab, want_dual=True, want_prices=True)
    r = torch.empty((B, n), dtype=torch.int32, device="cuda")
    t = torch.empty(B, dtype=torch.int64, device="cuda")
    d = torch.empty(B, dtype=torch.int64, device="cuda")
    p = torch.empty((B, n), dtype=torch.int64, device="cuda")
    _ffi.check(_ffi.lib().td_assign_batched(B, n, None, slab.ctypes.data, r.data_ptr(), t.data_ptr(), d.data_ptr(), p.data_ptr()))
    assert np.array_equal(r.cpu().numpy(), r_h) and np.array_equal(t.cpu().numpy(), t_h)
    assert np.array_equal(d.cpu().numpy(), d_h) and np.array_equal(p.cpu().numpy(), p_h)


RULES = {
    # heuristic.py:24-33: mask 100, n picks, every taken cell summed
    "heuristic": (dict(mask=100, threshold=-1), dict(mask=100, threshold=-1)),
    # greedy_opt.py:61-82: threshold 10, cells summed below big_cost
    "greedy_opt": (dict(mask=BIG, threshold=10, sum_below=BIG), dict(mask=BIG, threshold=10, sum_below=BIG)),
    # Simulator.java:523-549: Java's scan (cells >= big_cost never candidates), stop on big_cost or at MAX_NON_LCM rows left
    "simulator": (dict(mask=BIG, stop_value_on=1, stop_value=BIG, stop_size=4, sum_below=BIG),
                  dict(mask=BIG, stop_value_on=1, stop_value=BIG, stop_size=4, sum_below=BIG, java_scan=1)),
}


def lcm_model(rule, k, rng, b):
    if rule == "heuristic":
        return make("g4", k, rng)
    if rule == "greedy_opt":
        return make(("padded", "g1", "absdiff")[b % 3], k, rng) if k else np.zeros((0, 0), np.int32)
    c = make(("padded", "g4")[b % 2], k, rng) if k else np.zeros((0, 0), np.int32)
    if k and b % 2:
        c[rng.random((k, k)) < 0.3] = BIG   # unreachable cells
    return c


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("n,ragged", [(1, False), (7, False), (64, False), (100, False), (128, True), (129, False), (300, True),
                                      (1024, False)])
def test_lcm_batched_bit_exact(td, rule, n, ragged):
    rng = np.random.default_rng(10000 * sorted(RULES).index(rule) + n)
    B = 2 if n > 300 else 12
    ns = np.full(B, n, np.int32)
    if ragged:
        ns[:4] = [0, 1, n // 2, 3]
    slab = np.full((B, n, n), I32_MIN, np.int32)   # outside a block: would be every pick if read
    mats = []
    for b in range(B):
        k = int(ns[b])
        c = lcm_model(rule, k, rng, b)
        slab[b, :k, :k] = c
        mats.append(c)
    kw_gpu, kw_oracle = RULES[rule]
    total, rows, cols, lm, npairs = td.LCM_batched(slab, ns=ns if ragged else None, **kw_gpu)
    for b, c in enumerate(mats):
        t_o, r_o, c_o, lm_o = oracle.lcm(c, **kw_oracle)
        k = int(npairs[b])
        assert k == r_o.size, (b, k, r_o.size)
        assert rows[b, :k].tolist() == r_o.tolist() and cols[b, :k].tolist() == c_o.tolist(), b
        assert total[b] == t_o and lm[b] == lm_o, (b, int(total[b]), t_o, int(lm[b]), lm_o)


def test_heuristic_py_experiment(td):
    """heuristic.py:20-40 in full: 1000 scenarios of 100 x 100 U{1..39}; every optimum and every LCM total against the
    oracle, no optimum above its LCM total, the PDF's ~78 % gap (p.4)."""
    seed, n, iters = 20201, 100, 1000
    lcm_tot, opt, gap = td.heuristic_gap(n=n, iters=iters, seed=seed)
    c = np.random.default_rng(seed).integers(1, 40, (iters, n, n)).astype(np.int32)
    for b in range(iters):
        assert opt[b] == oracle.assign(c[b])[0], b
        assert lcm_tot[b] == oracle.lcm(c[b], mask=100, threshold=-1)[0], b
    assert (opt <= lcm_tot).all()
    assert 75.0 <= gap <= 81.0, gap


def test_assign_batched_beyond_2g_cells(td):
    """B = 2100 models of 1024 x 1024 (2.2e9 cells, made on the device): the models around cell 2^31 and the ends
    against the oracle, every model certified by dual_bound == total."""
    import torch
    B, n = 2100, 1024
    g = torch.Generator(device="cuda")
    g.manual_seed(2100)
    dev = torch.randint(0, 1000001, (B, n, n), dtype=torch.int32, device="cuda", generator=g)
    r2c, total, dual = td.assign_batched(dev, want_dual=True)
    assert (dual == total).all()
    for b in (0, 1, 2047, 2048, 2049, B - 1):   # model 2048 starts at cell 2^31
        c = dev[b].cpu().numpy()
        assert total[b] == oracle.assign(c)[0], b
        assert sorted(r2c[b].tolist()) == list(range(n))
    del dev
    torch.cuda.empty_cache()


def test_batched_argument_errors(td):
    from taxidispatcher_amd import _ffi
    with pytest.raises(td.TdError, match="td_assign"):
        td.assign_batched(np.zeros((1, 1025, 1025), np.int32))
    with pytest.raises(td.TdError, match="td_assign"):
        td.LCM_batched(np.zeros((1, 1025, 1025), np.int32))
    with pytest.raises(td.TdError, match=r"ns\[1\]"):
        td.assign_batched(np.zeros((2, 4, 4), np.int32), ns=[4, 5])
    with pytest.raises(td.TdError, match=r"ns\[0\]"):
        td.LCM_batched(np.zeros((2, 4, 4), np.int32), ns=[-1, 2])
    lib = _ffi.lib()
    c = np.zeros((1, 4, 4), np.int32)
    r = np.zeros(4, np.int32)
    t = np.zeros(1, np.int64)
    k = np.zeros(1, np.int32)
    assert lib.td_assign_batched(-1, 4, None, c.ctypes.data, r.ctypes.data, t.ctypes.data, None, None) == -1
    assert b"batch" in lib.td_last_error()
    assert lib.td_lcm_batched(-1, 4, None, c.ctypes.data, 100, -1, 0, 0, -1, 2**62, r.ctypes.data, r.ctypes.data,
                              k.ctypes.data, t.ctypes.data, k.ctypes.data) == -1
    assert b"batch" in lib.td_last_error()
    # an empty batch is a no-op, not an error
    r2c, total = td.assign_batched(np.zeros((0, 5, 5), np.int32))
    assert r2c.shape == (0, 5) and total.shape == (0,)
