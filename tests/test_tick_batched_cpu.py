"""CPU tier of the batched position entry points (td_build_assign_batched / td_tick_batched): the ragged packing, the
symbols in the ctypes table and the built library, and no CPU fallback."""

import numpy as np
import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def built():
    entry.build()
    from taxidispatcher_amd import _ffi
    return _ffi


def test_pack_ragged_lists():
    from taxidispatcher_amd import pack_ragged
    cabs = [np.array([3, 1, 4]), [], np.array([1, 5, 9, 2, 6], np.int64), [7]]
    dems = [[2, 7], np.array([1, 8, 2, 8]), [], np.zeros(0)]
    cv, co, dv, do, B, n = pack_ragged(cabs, dems)
    assert (B, n) == (4, 5)
    assert cv.dtype == np.int32 and co.dtype == np.int32 and dv.dtype == np.int32 and do.dtype == np.int32
    assert cv.tolist() == [3, 1, 4, 1, 5, 9, 2, 6, 7] and co.tolist() == [0, 3, 3, 8, 9]
    assert dv.tolist() == [2, 7, 1, 8, 2, 8] and do.tolist() == [0, 2, 6, 6, 6]
    # a ready (values, offsets) pair is handed on
    cv2, co2, dv2, do2, B2, n2 = pack_ragged((cv, co), (dv, do))
    assert np.shares_memory(cv2, cv) and np.shares_memory(co2, co) and (B2, n2) == (4, 5)


def test_pack_ragged_empty_and_errors():
    from taxidispatcher_amd import TdError, pack_ragged
    cv, co, dv, do, B, n = pack_ragged([], [])
    assert (B, n) == (0, 0) and co.tolist() == [0] and do.tolist() == [0] and cv.size == 0
    cv, co, dv, do, B, n = pack_ragged([[]], [[]])
    assert (B, n) == (1, 0)
    with pytest.raises(TdError, match="2 cab lists for 3"):
        pack_ragged([[1], [2]], [[1], [2], [3]])
    with pytest.raises(TdError, match="beyond"):
        pack_ragged((np.arange(4), np.array([0, 5])), (np.arange(4), np.array([0, 4])))
    with pytest.raises(TdError, match="decrease"):
        pack_ragged((np.arange(4), np.array([0, 3, 2])), (np.arange(4), np.array([0, 1, 4])))
    with pytest.raises(TdError, match="start at 0"):
        pack_ragged((np.arange(4), np.array([1, 4])), (np.arange(4), np.array([0, 4])))
    with pytest.raises(TdError, match="integer"):
        pack_ragged([[1.5]], [[1]])


def test_symbols_declared(built):
    lib = built.load()
    for name in ("td_build_assign_batched", "td_tick_batched"):
        assert name in built.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.td_version() == 101


def test_no_cpu_fallback(built):
    """Without a GPU the new calls fail loudly, like test_batched_no_cpu_fallback"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path is exercised on the CPU tier only")
    lib = built.load()
    import taxidispatcher_amd as td
    cabs, dems = [np.array([1, 2, 3])], [np.array([2, 2])]
    with pytest.raises(td.TdError):
        td.build_assign_batched(cabs, dems)
    with pytest.raises(td.TdError):
        td.tick_batched(cabs, dems)
    # not initialised -> ENOINIT from the C ABI itself
    off = np.array([0, 3], np.int32)
    v = np.array([1, 2, 3], np.int32)
    r = np.zeros(3, np.int32)
    t = np.zeros(1, np.int64)
    assert lib.td_build_assign_batched(1, 3, off.ctypes.data, v.ctypes.data, off.ctypes.data, v.ctypes.data, None, 0, 100, -1,
                                       r.ctypes.data, t.ctypes.data, None) == -3
    k = np.zeros(1, np.int32)
    assert lib.td_tick_batched(1, 3, off.ctypes.data, v.ctypes.data, off.ctypes.data, v.ctypes.data, None, 0, 100, -1, 1,
                               r.ctypes.data, r.ctypes.data, k.ctypes.data, k.ctypes.data, None, None, k.ctypes.data, r.ctypes.data,
                               t.ctypes.data, None) == -3
