"""td_pool_n_batched without a GPU: the symbol in the header, the binding and the cross-compiled library; the packing of
ragged inputs; and the condition on the GPU tests' inputs (every model within half of the max_happy its test passes)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pool_fixtures as pf
import pool_n_batched_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_in_header_binding_and_library():
    from taxidispatcher_amd import _ffi, build
    hdr = open(os.path.join(ROOT, "include", "taxidispatcher_amd.h")).read()
    m = re.search(r"TD_API\s+int\s+td_pool_n_batched\s*\(([^;]*)\)\s*;", hdr)
    assert m, "td_pool_n_batched is not declared in the header"
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    res, args = _ffi.SIGNATURES["td_pool_n_batched"]
    assert res is ctypes.c_int and len(args) == len(params) == 16
    for p, a in zip(params, args):
        if "*" in p:
            assert a is ctypes.c_void_p, p
        elif "int64_t" in p:
            assert a is ctypes.c_int64, p
        else:
            assert a is ctypes.c_int, p
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "td_pool_n_batched")
    import taxidispatcher_amd as td
    assert callable(td.pool_n_batched) and callable(td.find_pool_fanout)


def test_packing_round_trips_ragged_and_empty_models():
    import taxidispatcher_amd as td
    rng = np.random.default_rng(3)
    sizes = [5, 0, 1, 12, 0, 7]
    ds = [pc.random_demand(rng, m, 9, [10, 90]) for m in sizes]
    ds[3] = ds[3].tolist()                                           # rows as lists, as the reference's reader gives them
    firsts = [None, None, (0, 1), (3, 9), (0, 0), (-2, 99)]
    off, frm, to, wait, loss, first, batch, n = td.pack_pool_n(ds, firsts)
    assert batch == 6 and n == 12
    assert off.dtype == np.int32 and off.tolist() == [0, 5, 5, 6, 18, 18, 25]
    for a in (frm, to, wait, loss):
        assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] and a.size == 25
    for b, d in enumerate(ds):
        d = np.asarray(d).reshape(-1, 5)
        for col, a in zip((1, 2, 3, 4), (frm, to, wait, loss)):
            assert a[off[b]:off[b + 1]].tolist() == d[:, col].tolist()
    # [2 * batch], a missing slice = the whole model; clamping is the library's, as td_pool_n's
    assert first.dtype == np.int32 and first.shape == (6, 2) and first.flags["C_CONTIGUOUS"]
    assert first.tolist() == [[0, 5], [0, 0], [0, 1], [3, 9], [0, 0], [-2, 99]]
    assert td.pack_pool_n(ds)[5] is None
    off0, frm0, *_, batch0, n0 = td.pack_pool_n([])
    assert off0.tolist() == [0] and frm0.size == 0 and batch0 == 0 and n0 == 0
    with pytest.raises(td.TdError):
        td.pack_pool_n(ds, firsts[:3])
    # output strides of the C call: model b's records start at b * (n / k) * (2k + 1)
    for k in pc.KS:
        assert (n // k) * (2 * k + 1) == {2: 30, 3: 28, 4: 27}[k]


@pytest.mark.parametrize("k", pc.KS)
def test_inputs_stay_within_half_of_max_happy(k):
    """a condition on the generated inputs, checked with the oracle: expected() runs it with cap = max_happy / 2 and raises
    OverflowError beyond"""
    for name, demands, dist, max_happy in pc.batches(k):
        exp = pc.expected(name, k)
        assert len(exp) == len(demands)
        assert max(h for _, h in exp) <= pc.eff(max_happy) // 2, name
        assert all(0 <= r[-1] <= 16383 for recs, _ in exp for r in recs), name
        assert all(len(d) <= 512 for d in demands)
    sizes = {len(d) for d in pc.tiny_batch()}
    assert sizes == set(range(10))


def test_fixture_children_stay_within_half_of_the_default():
    for name, k in pf.cases():
        ds, firsts, exp = pc.fixture_batch(name, k)
        assert len(ds[0]) <= 512
        for c, f in enumerate(firsts):
            recs, happy = pc.oracle_model(k, ds[0], None, f, cap=pc.eff(pc.FIXTURE_MAX_HAPPY) // 2)
            assert recs == exp[c], (name, k, c)          # the oracle restates the reference binary
