"""td_pool_n_banded on the GPU at every band cut, chunk and bitmap boundary: the cases of tests/pool_band_cases.py (whose own
conditions tests/test_pool_band_cases_cpu.py checks) through the raw C call -- records, n_pools and n_happy against
oracle.pool_n, all four stats against the host model, nothing written behind the records -- and through td_pool_n; the whole
corpus of tests/pool_edge_cases.py through the smallest buffer; device pointers; calls back to back.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import pool_band_cases as pc
import pool_edge_cases as pe
from pool_band_call import raw

pytestmark = pytest.mark.gpu

KS = [2, 3, 4]
TD_OK, TD_ERANGE = 0, -4
PER_K = ("bitmap_edges", "grid_edges_banded", "top_band", "greedy_chunks", "max_pools_edges")
GENERATORS = ["cut_relations", "k2_bands", "slice_deep_cut"] + ["%s_k%d" % (g, k) for k in KS for g in PER_K]


def cases_of(name):
    if name[:-3] in PER_K:
        return getattr(pc, name[:-3])(int(name[-1]))
    return getattr(pc, name)()


def cols_of(case):
    return [case.frm, case.to, case.wait, case.loss]


def cap_of(bc):
    n = int(bc.case.frm.size)
    return n // bc.case.k + 1 if bc.max_pools is None else bc.max_pools


def banded(bc, cols=None, out=None):
    c = bc.case
    return raw(c.k, int(c.frm.size), cols_of(c) if cols is None else cols, c.dist, (c.first0, c.first1), bc.room, cap_of(bc), out=out)


def check_banded(bc, got=None):
    """one td_pool_n_banded call against the oracle (records, counts) and the model (stats)"""
    s = pc.solve(bc)
    got = banded(bc) if got is None else got
    print(bc.name, "n_happy", got["happy"], "stats", got["stats"], "model", s.stats)
    assert got["rc"] == TD_OK, (bc.name, got["rc"])
    assert got["n_pools"] == len(s.exp) and got["happy"] == s.nh, (bc.name, got["n_pools"], len(s.exp), got["happy"], s.nh)
    assert got["recs"] == s.exp, (bc.name, got["stats"], s.stats)
    assert got["stats"] == s.stats, (bc.name, got["stats"], s.stats)
    assert (got["behind"] == got["fill"]).all(), bc.name
    return got


def pool_n(lib, case, max_pools):
    """td_pool_n on the same input -> (return code, records, n_happy); nothing behind the records"""
    k, n = case.k, int(case.frm.size)
    out = np.full((max(max_pools, 1) + 2, 2 * k + 1), -7, np.int32)
    m, nh = ctypes.c_int32(-5), ctypes.c_int64(-5)
    rc = lib.td_pool_n(k, n, *[a.ctypes.data for a in cols_of(case)], None if case.dist is None else case.dist.ctypes.data,
                       0 if case.dist is None else case.dist.shape[0], case.first0, case.first1, 0, max_pools, out.ctypes.data,
                       ctypes.byref(m), ctypes.byref(nh))
    kept = max(m.value, 0)
    assert (out[kept:] == -7).all(), case.name
    return rc, out[:kept].tolist(), nh.value


@pytest.fixture()
def lib(td):
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


# ---- every case of pool_band_cases.py -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GENERATORS)
def test_band_cases(lib, name):
    for bc in cases_of(name):
        s = pc.solve(bc)
        first = check_banded(bc)
        again = banded(bc)      # plan slots are handed out by atomics: only the sort may decide the order
        assert (again["recs"], again["happy"], again["stats"]) == (first["recs"], first["happy"], first["stats"]), bc.name
        assert pool_n(lib, bc.case, cap_of(bc)) == (TD_OK, s.exp, s.nh), bc.name


# ---- the corpus of pool_edge_cases.py through the smallest buffer ---------------------------------------------------------------------
def check_corpus(lib, c):
    exp, nh = pe.reference(c)
    n = int(c.frm.size)
    got = raw(c.k, n, cols_of(c), c.dist, (c.first0, c.first1), 24 * n, n // c.k + 1)
    assert (got["rc"], got["recs"], got["n_pools"], got["happy"]) == (TD_OK, exp, len(exp), nh), (c.name, c.k, got["rc"], got["happy"], nh)
    assert (got["behind"] == got["fill"]).all() and got["stats"][3] <= max(24 * n, 0), c.name
    return got


@pytest.mark.parametrize("k", KS)
def test_happy_ties_banded(lib, k):
    cases = pe.happy_ties(k)
    for c in cases:
        check_corpus(lib, c)
    assert {"tie_table_d%d_l%d" % p for p in pe.KNOWN_MISROUNDED} <= {c.name for c in cases}


@pytest.mark.parametrize("k", KS)
def test_wait_edges_banded(lib, k):
    for c in pe.wait_edges(k):
        check_corpus(lib, c)


@pytest.mark.parametrize("k", KS)
def test_grid_edges_and_top_of_key_banded(lib, k):
    for c in pe.grid_edges(k) + pe.top_of_key(k):
        got = check_corpus(lib, c)
        if c.name == "top_of_key":      # at most 31 896 happy plans against 24 * 2047: one band, as the host model says
            assert got["stats"][0] == 1 and got["stats"][2] == 0, got["stats"]


def test_cost_limit_banded(lib):
    fits, too_large = pe.cost_limit()
    got = check_corpus(lib, fits)
    assert got["recs"][-1] == [0, 1, 0, 1, pe.PN_MAXCOST]
    for _ in range(2):
        rc, recs, nh = pool_n(lib, too_large, 3)
        bad = raw(2, 4, cols_of(too_large), too_large.dist, (0, 4), 24 * 4, 3)
        assert rc == bad["rc"] == TD_ERANGE and nh == bad["happy"] == pe.reference(too_large)[1], (rc, bad["rc"], nh, bad["happy"])
        assert bad["n_pools"] == 0 and (bad["behind"] == bad["fill"]).all()
    check_corpus(lib, fits)      # and the refusal leaves nothing behind


# ---- device pointers: the form td_sim.hip uses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_device_pointers(lib, k):
    import torch
    for bc in (pc.bitmap_edges(k)[-2], pc.greedy_chunks(k)[1]):
        c = bc.case
        host = check_banded(bc)
        dev = [torch.from_numpy(a).cuda() for a in cols_of(c)]
        out = torch.full((cap_of(bc) + 2, 2 * k + 1), -7, dtype=torch.int32, device="cuda")
        got = check_banded(bc, banded(bc, cols=dev, out=out))
        assert (got["recs"], got["n_pools"], got["happy"], got["stats"]) == (host["recs"], host["n_pools"], host["happy"], host["stats"])
    t = pe._line_table(8)      # and a distance table on the device: the cluster's stands 3 and 4 lie inside it
    bc = pc._band("device_table_k%d" % k, pc.cluster(2 * k + 2, range(2 * k + 2), k, dear=(1, 2))._replace(dist=t), 24 * (2 * k + 2))
    host = check_banded(bc)
    c = bc.case
    got = raw(k, int(c.frm.size), [torch.from_numpy(a).cuda() for a in cols_of(c)], torch.from_numpy(t).cuda(), (c.first0, c.first1), bc.room,
              cap_of(bc), out=torch.full((cap_of(bc) + 2, 2 * k + 1), -7, dtype=torch.int32, device="cuda"))
    check_banded(bc, got)
    assert got["recs"] == host["recs"]


# ---- back to back ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_back_to_back(lib, k):
    """n = 2047 with requests up to 2046 used (the last word of the bitmap), then 33 requests, then the first again: the bitmap
    and the counters of a call are its own"""
    big, small, chunks = pc.top_band(k)[0], pc.bitmap_edges(k)[0], pc.greedy_chunks(k)[0]
    assert max(x for r in pc.solve(big).exp for x in r[:k]) >= 2040 and int(small.case.frm.size) == 33
    for bc in (big, small, big, chunks, small, big):
        check_banded(bc)
