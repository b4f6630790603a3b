"""td_lcm and td_pool2 on the case table of tests/lcm_path_cases.py: both sides of every constant by which csrc/td_lcm.hip
chooses between the level lists and the row-scan loop, between their kernels, chunks, LDS layouts and copy routes.  Every case
is held to its host reference exactly -- pairs in order, total, last_min -- and to the path it is a case for: td_last_stats
word 11 (`lcm_path`) must show exactly the bits the table derives from the case's shape (test_lcm_paths_cpu.py confirms that
derivation and the structural claims of the cases whose edge does not change the path).  Every case is a valid call with a
known answer.  Run with -s to see each case's figures."""
import ctypes

import numpy as np
import pytest

import lcm_path_cases as L
import tick_path_cases as T

pytestmark = pytest.mark.gpu


def _device_matrix(torch, c):
    """the matrix of a sparse or closed-form case, built on the device"""
    n = c["n"]
    if c["input"] == "count":
        return L.count_matrix(n, torch, device="cuda")
    m = torch.full((n, n), c["fill"], dtype=torch.int32, device="cuda")
    r, cc, v = (torch.tensor(a, device="cuda") for a in c["coords"])
    m[r.long(), cc.long()] = v   # unique coordinates (the CPU tier checks it): a deterministic write
    return m


def _lcm_device_out(n, m, args):
    """td_lcm with rows / cols in device memory; cells past n_pairs must stay untouched"""
    import torch
    from taxidispatcher_amd import _ffi
    mask, thr, svo, sv, ss, sb, mp = args
    if not hasattr(m, "data_ptr"):
        m = _ffi.as_i32(m).reshape(n, n)
    rows = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cols = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    k, tot, lm = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
    _ffi.check(_ffi.lib().td_lcm(n, _ffi.addr(m), int(mask), int(thr), int(svo), int(sv), int(ss), int(sb), n if mp is None else int(mp),
                                 _ffi.addr(rows), _ffi.addr(cols), ctypes.byref(k), ctypes.byref(tot), ctypes.byref(lm)))
    return int(tot.value), rows.cpu().numpy(), cols.cpu().numpy(), int(lm.value), int(k.value)


@pytest.mark.parametrize("name", L.LCM_NAMES)
def test_lcm_case(td, name):
    from taxidispatcher_amd import dispatch
    c = L.case(name)
    t_e, r_e, c_e, lm_e = L.reference(name)
    n, args = c["n"], L.lcm_args(c["rule"][0])
    on_device = c["input"] != "dense"
    if on_device:
        import torch
        m = _device_matrix(torch, c)
    else:
        m = c["matrix"]
    if c["out"] == "host":
        tot, rows, cols, lm = dispatch._lcm(n, m, *args)
        path = td.last_stats()["lcm_path"]
    else:
        tot, rows, cols, lm, k = _lcm_device_out(n, m, args)
        path = td.last_stats()["lcm_path"]
        assert (rows[k:] == -7).all() and (cols[k:] == -7).all(), name
        rows, cols = rows[:k], cols[:k]
    if on_device:
        del m
        torch.cuda.empty_cache()
    print(name, "n", n, "pairs", len(rows), "/", len(r_e), "total", tot, "/", t_e, "last_min", lm, "/", lm_e, "path", path, "/", c["bits"])
    assert len(rows) == len(r_e), name
    assert rows.tolist() == r_e and cols.tolist() == c_e, name
    assert (tot, lm) == (t_e, lm_e), name
    assert path == c["bits"], name


@pytest.mark.parametrize("name", L.POOL_NAMES)
def test_pool2_case(td, name):
    c = L.case(name)
    ref = L.reference(name)
    got = td.find_pool(c["frm"], c["to"], c["dist"])
    path = td.last_stats()["lcm_path"]
    print(name, "n", c["n"], "pools", len(got), "/", len(ref), "path", path, "/", c["bits"])
    assert got == ref, name
    assert path == c["bits"], name


def test_count_matrix_on_the_device_is_the_closed_form(td):
    import torch
    for n in (16, 61):
        assert np.array_equal(L.count_matrix(n, torch, device="cuda").cpu().numpy(), L.count_matrix(n))


@pytest.mark.parametrize("name,bits", [("f_table_fill250000", L.LISTS | L.HINTED), ("m_negative", L.LISTS | L.REDONE),
                                       ("m_span255", L.LISTS), ("m_span256", 0)])
def test_tick_hint_bits(td, name, bits):
    """the two bits only td_tick can raise, on cases of tests/tick_path_cases.py whose remainder the general solver answers (a
    distance table: td_assign's line-metric path would clear the word).  The answers are test_gpu_tick_paths.py's business."""
    _, cab, dem, dist, fill, thr, stop, _ = T.case(name)
    assert dist is not None
    got = td.tick(cab, dem, dist, big_cost=fill, drop_time=thr, max_non_lcm=stop)
    path = td.last_stats()["lcm_path"]
    ref = T.reference(name)
    assert got["lcm_rows"].tolist() == list(ref["lcm_rows"]) and got["lcm_cols"].tolist() == list(ref["lcm_cols"])
    assert path & (L.LISTS | L.HINTED | L.REDONE | L.POOL2) == bits, (name, path)
