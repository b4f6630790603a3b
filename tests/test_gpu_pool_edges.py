"""td_pool_n / td_pool_merge on the GPU at their rule and chunk boundaries (the cases of tests/pool_edge_cases.py, whose
own conditions tests/test_pool_edges_cpu.py checks): the happiness rule at equality in double precision, the wait rule at
equality, the 256-thread grid edge, the top of the plan key, the 14-bit cost limit, max_happy, and the greedy's 1024-plan
chunks driven through td_pool_merge with crafted records.  Every comparison is exact (records as integer lists, counts,
return codes) and every case is called twice: plan slots are handed out by atomics, only the sort may decide the order."""
import ctypes

import numpy as np
import pytest

import abi_buffers as ab
import pool_edge_cases as pe

pytestmark = pytest.mark.gpu

KS = [2, 3, 4]
TD_OK, TD_EINVAL, TD_ERANGE = 0, -1, -4
PAT32 = int(ab.pattern_value(np.int32))


@pytest.fixture()
def lib(td):
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def call_pool_n(lib, c, max_happy=0, max_pools=None):
    """-> (return code, records of the n_pools pools, n_happy) of one td_pool_n call on host arrays"""
    k, n = c.k, int(c.frm.size)
    cap = max(1, n // k + 1) if max_pools is None else max_pools
    out = np.full((cap, 2 * k + 1), PAT32, np.int32)
    m, nh = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = lib.td_pool_n(k, n, ab.ptr(c.frm), ab.ptr(c.to), ab.ptr(c.wait), ab.ptr(c.loss), ab.ptr(c.dist),
                       0 if c.dist is None else c.dist.shape[0], c.first0, c.first1, max_happy, cap, ab.ptr(out), ctypes.byref(m),
                       ctypes.byref(nh))
    if rc == TD_EINVAL:                                      # refused before anything was looked at: no output is touched
        assert m.value == -1 and (out == PAT32).all(), c.name
        return rc, [], nh.value
    assert 0 <= m.value <= cap, (c.name, m.value)
    assert (out[m.value:] == PAT32).all(), c.name            # nothing behind the pools it reports
    return rc, out[:m.value].tolist(), nh.value


def check_pool_n(lib, c):
    exp, nh = pe.reference(c)
    first = call_pool_n(lib, c)
    assert first == (TD_OK, exp, nh), (c.name, c.k, first[0], first[2], nh, lib.td_last_error())
    assert call_pool_n(lib, c) == first, (c.name, "second call differs")


def call_merge(lib, c, recs=None, out_kind=("host", 0), max_pools=None):
    """-> (return code, kept records) of one td_pool_merge call; the output sits between guard bands"""
    k, w = c.k, 2 * c.k + 1
    cap = c.max_pools if max_pools is None else max_pools
    out, check = ab.guarded((cap * w,), np.int32, *out_kind)
    m = ctypes.c_int32(-1)
    rc = lib.td_pool_merge(k, c.n_requests, c.recs.shape[0], ab.ptr(c.recs if recs is None else recs), c.sort_by_cost, cap, ab.ptr(out),
                           ctypes.byref(m))
    check()
    got = ab.host(out)
    if rc == TD_EINVAL:
        assert m.value in (-1, 0) and (got == PAT32).all(), c.name
        return rc, []
    assert 0 <= m.value <= cap, (c.name, m.value)
    assert (got[m.value * w:] == PAT32).all(), c.name
    return rc, got[:m.value * w].reshape(-1, w).tolist()


# ------------------------------------------------------------------------------------------------------------------
# td_pool_n
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_happy_ties(lib, k):
    cases = pe.happy_ties(k)
    for c in cases:
        check_pool_n(lib, c)
    # the rides of exactly direct * (100 + loss) / 100 that the reference's double arithmetic refuses were among them
    names = {c.name for c in cases}
    assert {"tie_table_d%d_l%d" % p for p in pe.KNOWN_MISROUNDED} <= names


@pytest.mark.parametrize("k", KS)
def test_wait_edges(lib, k):
    for c in pe.wait_edges(k):
        check_pool_n(lib, c)


@pytest.mark.parametrize("k", KS)
def test_grid_edges(lib, k):
    for c in pe.grid_edges(k):
        check_pool_n(lib, c)


@pytest.mark.parametrize("k", KS)
def test_top_of_key(lib, k):
    for c in pe.top_of_key(k):
        check_pool_n(lib, c)


def test_cost_limit(lib):
    fits, too_large = pe.cost_limit()
    check_pool_n(lib, fits)
    assert pe.reference(fits)[0][-1][-1] == pe.PN_MAXCOST
    for _ in range(2):
        rc, recs, nh = call_pool_n(lib, too_large)
        assert (rc, recs, nh) == (TD_ERANGE, [], pe.reference(too_large)[1]), lib.td_last_error()
    check_pool_n(lib, fits)                                  # and the refusal leaves nothing behind


@pytest.mark.parametrize("k", KS)
def test_max_happy_met_and_exceeded_by_one(lib, k):
    c = pe.grid_edges(k)[1]
    assert c.name == "grid_n256"
    exp, nh = pe.reference(c)
    for _ in range(2):
        assert call_pool_n(lib, c, max_happy=nh) == (TD_OK, exp, nh)
        assert call_pool_n(lib, c, max_happy=nh - 1) == (TD_ERANGE, [], nh), lib.td_last_error()
    assert call_pool_n(lib, c, max_happy=nh + 1) == (TD_OK, exp, nh)


def test_refusals(lib):
    n = pe.PN_MAXN + 1
    z = np.zeros(n, np.int32)
    c = pe.PoolCase("n2048", 2, z, z + 1, z, z + 100, None, 0, n, {})
    assert call_pool_n(lib, c) == (TD_EINVAL, [], -1), lib.td_last_error()
    m = pe.merge_cases(2)[0]
    assert call_merge(lib, m._replace(n_requests=n)) == (TD_EINVAL, [])
    assert call_merge(lib, m)[0] == TD_OK                    # the same records with n_requests = 2047


# ------------------------------------------------------------------------------------------------------------------
# td_pool_merge: the greedy's chunks
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_merge_cases(lib, k):
    for c in pe.merge_cases(k):
        exp = pe.merge_scan(k, c.recs, c.sort_by_cost, c.max_pools)[0]
        first = call_merge(lib, c)
        assert first == (TD_OK, exp), (c.name, k, first[0], len(first[1]), len(exp), lib.td_last_error())
        assert call_merge(lib, c) == first, (c.name, "second call differs")


@pytest.mark.parametrize("k", KS)
def test_merge_from_device_memory(lib, k):
    (c,) = [x for x in pe.merge_cases(k) if x.name == "sparse_2049_s1"]
    exp = pe.merge_scan(k, c.recs, 1, c.max_pools)[0]
    dev = ab.place(c.recs, "device", 1)                      # a device view aligned to its element size only
    for out_kind in (("host", 0), ("device", 0)):
        for _ in range(2):
            assert call_merge(lib, c, dev, out_kind) == (TD_OK, exp), (k, out_kind)
    cut = len(exp) - 1
    assert call_merge(lib, c, dev, ("device", 1), max_pools=cut) == (TD_OK, exp[:cut])


@pytest.mark.parametrize("k", KS)
def test_merge_refuses_ids_outside_the_requests(lib, k):
    """a record naming a request < 0 or >= n_requests: TD_EINVAL naming the record and the id, *n_out = 0, pools_out untouched"""
    c = pe.merge_cases(k)[0]._replace(n_requests=pe.PN_MAXN, sort_by_cost=1, max_pools=pe.PN_MAXN // k + 1)
    w = 2 * k + 1
    for label, rec, bad, recs in pe.bad_id_inputs(k):
        for in_kind in ("host", "device"):
            buf = ab.place(recs, in_kind, 0)
            for out_kind in (("host", 0), ("device", 0)):
                out, check = ab.guarded((c.max_pools * w,), np.int32, *out_kind)
                m = ctypes.c_int32(-1)
                rc = lib.td_pool_merge(k, c.n_requests, recs.shape[0], ab.ptr(buf), 1, c.max_pools, ab.ptr(out), ctypes.byref(m))
                msg = lib.td_last_error().decode()
                check()
                assert (rc, m.value) == (TD_EINVAL, 0), (label, in_kind, rc, m.value, msg)
                assert (ab.host(out) == PAT32).all(), (label, in_kind, out_kind)
                assert "record %d " % rec in msg and "request %d " % bad in msg, (label, msg)
    good = pe.bad_id_inputs(k)[0][3].copy()
    good[0, 0] = 0                                           # the same list with every id valid is merged
    ok = c._replace(recs=good)
    assert call_merge(lib, ok) == (TD_OK, pe.merge_scan(k, good, 1, c.max_pools)[0])
