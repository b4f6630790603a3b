"""td_pool_n_batched on the GPU: exact equality of pools, n_pools, n_happy and total with the oracle model by model, with
the reference binary's committed outputs, and with td_pool_n; the capacity edge, the contract and the refusals."""
import ctypes

import numpy as np
import pytest

import pool_fixtures as pf
import pool_n_batched_cases as pc

pytestmark = pytest.mark.gpu

GUARD = -77


def call(td, k, demands, dist=None, firsts=None, max_happy=0, n=None, want=True):
    """the raw C call on host arrays, every output pre-filled with GUARD -> (rc, pools [B, n // k, 2k+1], n_pools, n_happy, total)"""
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    off, frm, to, wait, loss, first, batch, nmax = td.pack_pool_n(demands, firsts)
    n = nmax if n is None else n
    d = None if dist is None else np.ascontiguousarray(dist, np.int32)
    pools = np.full((batch, n // k, 2 * k + 1), GUARD, np.int32)
    m = np.full(batch, GUARD, np.int32)
    nh, tot = np.full(batch, GUARD, np.int64), np.full(batch, GUARD, np.int64)
    rc = lib.td_pool_n_batched(k, batch, n, _ffi.addr(off), _ffi.addr(frm), _ffi.addr(to), _ffi.addr(wait), _ffi.addr(loss),
                               _ffi.addr(d), 0 if d is None else d.shape[0], _ffi.addr(first), max_happy,
                               _ffi.addr(pools) if pools.size else None, _ffi.addr(m), _ffi.addr(nh) if want else None,
                               _ffi.addr(tot) if want else None)
    return rc, pools, m, nh, tot


def assert_equal_oracle(got, exp, what):
    """exp: list of (records, happy plans) per model"""
    rc, pools, m, nh, tot = got
    assert rc == 0, what
    assert m.tolist() == [len(r) for r, _ in exp], what
    assert nh.tolist() == [h for _, h in exp], what
    assert tot.tolist() == [sum(x[-1] for x in r) for r, _ in exp], what
    for b, (r, _) in enumerate(exp):
        assert pools[b, :len(r)].tolist() == r, (what, b)
        assert (pools[b, len(r):] == GUARD).all(), (what, b)      # nothing behind a model's records


def last_error(td):
    from taxidispatcher_amd import _ffi
    return _ffi.lib().td_last_error().decode()


@pytest.mark.parametrize("k", pc.KS)
def test_tiny_models_more_than_workgroups(td, k):
    """6000 models of 0..9 requests for at most 1024 workgroups: every workgroup runs several models in turn, so LDS or
    key-slab contents left by a model would show in the next; equal costs abound, so the enumeration order decides"""
    ds = pc.tiny_batch()
    assert {len(d) for d in ds} >= {0, k - 1, k, 9} and len(ds) > 1024
    assert_equal_oracle(call(td, k, ds, max_happy=pc.TINY_MAX_HAPPY), pc.expected("tiny", k), ("tiny", k))


@pytest.mark.parametrize("k", pc.KS)
def test_mixed_sizes_abs_metric(td, k):
    ds = pc.mixed_batch()
    assert sorted({len(d) for d in ds}) == list(pc.MIXED_SIZES)
    assert_equal_oracle(call(td, k, ds, max_happy=pc.MIXED_MAX_HAPPY, n=pc.MIXED_N), pc.expected("mixed", k), ("mixed", k))


@pytest.mark.parametrize("k", pc.KS)
def test_distance_table(td, k):
    dist, ds = pc.table_batch()
    assert_equal_oracle(call(td, k, ds, dist, max_happy=pc.TABLE_MAX_HAPPY), pc.expected("table", k), ("table", k))


@pytest.mark.parametrize("k", pc.KS)
def test_size_limit_512(td, k):
    d = pc.limit_model(k)
    assert len(d) == 512
    assert_equal_oracle(call(td, k, [d], max_happy=pc.LIMIT_MAX_HAPPY[k]), pc.expected("limit", k), ("limit", k))


def test_513_is_refused(td):
    d = pc.random_demand(np.random.default_rng(5), 513, 1, [1, 5])
    rc, pools, m, nh, tot = call(td, 2, [d])
    assert rc == _ffi_code("TD_EINVAL")
    assert (pools == GUARD).all() and (m == GUARD).all() and (nh == GUARD).all() and (tot == GUARD).all()


def test_reference_binary_children_as_one_batch(td):
    for name, k in pf.cases():
        ds, firsts, exp = pc.fixture_batch(name, k)
        rc, pools, m, nh, tot = call(td, k, ds, firsts=firsts, max_happy=pc.FIXTURE_MAX_HAPPY)
        assert rc == 0, (name, k)
        for c in range(8):
            assert pools[c, :m[c]].tolist() == exp[c], (name, k, c)
            assert tot[c] == sum(r[-1] for r in exp[c])
        merged = td.find_pool_fanout(k, ds[0])
        assert merged.tolist() == pf.merge_restatement(k, exp), (name, k)


@pytest.mark.parametrize("k", pc.KS)
def test_equals_td_pool_n(td, k):
    ds = pc.mixed_batch()[:20]
    lists, nh = td.pool_n_batched(k, ds, max_happy=pc.MIXED_MAX_HAPPY)
    for b, d in enumerate(ds):
        one, nh1 = td.find_pool_n(k, d)
        assert lists[b].tolist() == one.tolist() and int(nh[b]) == nh1, (k, b)


@pytest.mark.parametrize("k", pc.KS)
def test_batch_equals_its_models_alone_in_any_order(td, k):
    ds = pc.mixed_batch()
    exp = pc.expected("mixed", k)
    order = np.random.default_rng(99).permutation(len(ds)).tolist()
    assert_equal_oracle(call(td, k, [ds[i] for i in order], max_happy=pc.MIXED_MAX_HAPPY, n=pc.MIXED_N), [exp[i] for i in order],
                        ("shuffled", k))
    for i in (0, 1, 8, 15):     # sizes 17, 256, 100, 128
        assert_equal_oracle(call(td, k, [ds[i]], max_happy=pc.MIXED_MAX_HAPPY), [exp[i]], ("alone", k, i))


def test_capacity_edge(td):
    from taxidispatcher_amd import _ffi
    k, d = 4, pc.edge_model()
    small = pc.mixed_batch()[2], pc.mixed_batch()[6]          # 3 and 64 requests: 0 and 111 happy plans
    rc, pools0, m0, nh0, tot0 = call(td, k, [d])
    assert rc == 0
    happy = int(nh0[0])
    assert 1000 < happy < 32768
    rc, pools1, m1, nh1, tot1 = call(td, k, [d], max_happy=happy)
    assert rc == 0 and pools1.tolist() == pools0.tolist() and m1.tolist() == m0.tolist() and nh1.tolist() == nh0.tolist()
    rc, pools, m, nh, tot = call(td, k, [small[0], d, small[1]], max_happy=happy - 1)
    assert rc == _ffi_code("TD_ERANGE")
    msg = last_error(td)
    assert "model 1" in msg and str(happy) in msg
    exp = [pc.oracle_model(k, x, cap=2 * happy)[1] for x in (small[0], d, small[1])]
    assert exp[1] == happy and max(exp[0], exp[2]) < happy - 1
    assert nh.tolist() == exp                                   # written for all three, the true counts
    assert (pools == GUARD).all() and (m == GUARD).all() and (tot == GUARD).all()


def _ffi_code(name):
    """the header's error codes"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "taxidispatcher_amd.h")).read()
    return int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, hdr).group(1))


def test_device_pointers_equal_host_arrays(td):
    import torch
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    k = 3
    dist, ds = pc.table_batch()
    exp = pc.expected("table", k)
    off, frm, to, wait, loss, first, batch, n = td.pack_pool_n(ds, [None, (10, 50)] + [None] * (len(ds) - 2))
    exp = list(exp)
    exp[1] = pc.oracle_model(k, ds[1], dist, (10, 50))
    dev = [torch.from_numpy(a).cuda() for a in (off, frm, to, wait, loss, first.reshape(-1), np.ascontiguousarray(dist))]
    pools = torch.full((batch, n // k, 2 * k + 1), GUARD, dtype=torch.int32, device="cuda")
    m = torch.full((batch,), GUARD, dtype=torch.int32, device="cuda")
    nh = torch.full((batch,), GUARD, dtype=torch.int64, device="cuda")
    tot = torch.full((batch,), GUARD, dtype=torch.int64, device="cuda")
    rc = lib.td_pool_n_batched(k, batch, n, *[_ffi.addr(t) for t in dev[:5]], _ffi.addr(dev[6]), dist.shape[0], _ffi.addr(dev[5]),
                               pc.TABLE_MAX_HAPPY, _ffi.addr(pools), _ffi.addr(m), _ffi.addr(nh), _ffi.addr(tot))
    assert_equal_oracle((rc, pools.cpu().numpy(), m.cpu().numpy(), nh.cpu().numpy(), tot.cpu().numpy()), exp, "device pointers")
    # the same call on host arrays, and without the optional outputs
    host = call(td, k, ds, dist, [None, (10, 50)] + [None] * (len(ds) - 2), pc.TABLE_MAX_HAPPY)
    assert_equal_oracle(host, exp, "host arrays")
    rc, pools2, m2, nh2, tot2 = call(td, k, ds, dist, [None, (10, 50)] + [None] * (len(ds) - 2), pc.TABLE_MAX_HAPPY, want=False)
    assert rc == 0 and pools2.tolist() == host[1].tolist() and (nh2 == GUARD).all() and (tot2 == GUARD).all()


def test_batch_zero_writes_nothing(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    g = np.full(4, GUARD, np.int32)
    g64 = np.full(4, GUARD, np.int64)
    off = np.zeros(1, np.int32)
    assert lib.td_pool_n_batched(3, 0, 9, _ffi.addr(off), None, None, None, None, None, 0, None, 0, _ffi.addr(g), _ffi.addr(g),
                                 _ffi.addr(g64), _ffi.addr(g64)) == 0
    assert (g == GUARD).all() and (g64 == GUARD).all()
    lists, nh = td.pool_n_batched(3, [])
    assert lists == [] and nh.size == 0


def test_plan_storage_does_not_grow_with_batch(td):
    """both batches stage less than the 4 MiB step of the staging block, so the workspace differs only if the key slab
    depends on the batch; runs on a fresh library state and leaves one behind"""
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()

    def ws():
        v = ctypes.c_int64(-1)
        assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
        return v.value

    ds = pc.tiny_batch()
    lib.td_shutdown()
    assert ws() == 0
    assert lib.td_init(0) == 0
    try:
        base = ws()
        assert call(td, 2, ds[:10], max_happy=4096)[0] == 0
        small = ws()
        assert small - base >= 1024 * 4096 * 8            # the slab of every workgroup in flight is there already
        assert call(td, 2, ds, max_happy=4096)[0] == 0
        assert ws() == small
        lib.td_shutdown()
        assert ws() == 0
    finally:
        assert lib.td_init(0) == 0


def test_refusals_leave_the_outputs_alone(td):
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    einval, erange = _ffi_code("TD_EINVAL"), _ffi_code("TD_ERANGE")
    rng = np.random.default_rng(77)
    ds = [pc.random_demand(rng, m, 3, [10, 30]) for m in (20, 7, 33)]

    def untouched(got, code, what):
        rc, pools, m, nh, tot = got
        assert rc == code, (what, rc, last_error(td))
        assert (pools == GUARD).all() and (m == GUARD).all() and (nh == GUARD).all() and (tot == GUARD).all(), what

    def raw(k, off, n, ds=ds, max_happy=0):
        off_, frm, to, wait, loss, _, batch, _ = td.pack_pool_n(ds)
        off = np.ascontiguousarray(off, np.int32)
        pools = np.full((batch, max(n // max(k, 1), 1), 2 * max(k, 1) + 1), GUARD, np.int32)
        m = np.full(batch, GUARD, np.int32)
        nh, tot = np.full(batch, GUARD, np.int64), np.full(batch, GUARD, np.int64)
        rc = lib.td_pool_n_batched(k, batch, n, _ffi.addr(off), _ffi.addr(frm), _ffi.addr(to), _ffi.addr(wait), _ffi.addr(loss), None,
                                   0, None, max_happy, _ffi.addr(pools), _ffi.addr(m), _ffi.addr(nh), _ffi.addr(tot))
        return rc, pools, m, nh, tot

    good = [0, 20, 27, 60]
    assert raw(2, good, 33)[0] == 0
    for k in (1, 5):
        untouched(raw(k, good, 33), einval, ("k", k))
    untouched(raw(2, [1, 20, 27, 60], 33), einval, "off[0] = 1")
    untouched(raw(2, [0, 27, 20, 60], 33), einval, "decreasing offset")
    untouched(raw(2, good, 33, max_happy=(1 << 22) + 1), einval, "max_happy")
    untouched(raw(2, good, 513), einval, "n = 513")
    big = pc.random_demand(rng, 300, 1, [1, 5])
    untouched(call(td, 2, [ds[0], big], n=256), einval, "a model of 300 with n = 256")
    dist, tds = pc.table_batch()
    bad = [x.copy() for x in tds[:3]]
    bad[1][40, 2] = pc.TABLE_S                                  # a drop-off stand = S
    untouched(call(td, 3, bad, dist), einval, "stand = S")
    assert "model 1" in last_error(td)
    # a happy pair with cost 20000 on |a - b|: 0 -> 10000 and 10000 -> 20000, both patient and tolerant
    far = np.array([[0, 0, 10000, 20000, 1000], [1, 10000, 20000, 20000, 1000]])
    untouched(call(td, 2, [ds[1], far]), erange, "cost 20000")
