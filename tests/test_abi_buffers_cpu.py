"""CPU tests of tests/abi_buffers.py: the guard bands notice a single element written in front of or behind the window,
the misalignment is the one asked for, and the window is C-contiguous.  (Host memory only: pinned and device windows are
made by the same code and are exercised by tests/test_gpu_abi_contract.py.)"""
import ctypes

import numpy as np
import pytest

import abi_buffers as ab

SHAPES = [(1,), (7,), (0,), (3, 5), (2, 1028), (4, 300), (3, 2, 8)]
DTYPES = [np.int32, np.int64, np.uint8, np.uint64]


def _poke(address, dtype, value=0):
    """one element written through its raw address, as a kernel or a memcpy of the library would"""
    item = np.dtype(dtype).itemsize
    ctypes.memmove(address, np.array([value], dtype).tobytes(), item)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_window_and_guards(shape, dtype):
    for mis in (0, 1, 3):
        view, check = ab.guarded(shape, dtype, "host", mis)
        item = np.dtype(dtype).itemsize
        assert view.shape == shape and view.dtype == np.dtype(dtype)
        assert view.flags["C_CONTIGUOUS"] and (view.size == 0 or view.flags["WRITEABLE"])
        assert (view == ab.pattern_value(dtype)).all()
        if view.size:
            assert view.ctypes.data % 16 == (mis * item) % 16
            assert ab.ptr(view) == view.ctypes.data
        check()
        # writing the whole window leaves the guards alone
        view[...] = 0
        check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mis", [0, 1])
def test_one_element_outside_is_noticed(dtype, mis):
    item = np.dtype(dtype).itemsize
    for shape in ((5,), (3, 1028)):
        row = shape[-1]
        reach = max(ab.GUARD_MIN, row)
        size = int(np.prod(shape))
        for off in (-1, size, -reach, size + reach - 1):   # the nearest and the farthest element of each guard
            view, check = ab.guarded(shape, dtype, "host", mis)
            _poke(view.ctypes.data + off * item, dtype)
            with pytest.raises(AssertionError, match="BEFORE" if off < 0 else "BEHIND"):
                check()
        # one BYTE is enough, and the last element of the window itself is not a guard
        view, check = ab.guarded(shape, dtype, "host", mis)
        _poke(view.ctypes.data + (size - 1) * item, dtype)
        check()
        ctypes.memmove(view.ctypes.data + size * item + item - 1, b"\x00", 1)
        with pytest.raises(AssertionError, match="BEHIND"):
            check()


def test_misalignment_is_what_was_asked_for():
    v0, _ = ab.guarded((8,), np.int32, "host", 0)
    v1, _ = ab.guarded((8,), np.int32, "host", 1)
    v2, _ = ab.guarded((8, 8), np.int64, "host", 1)
    assert v0.ctypes.data % 16 == 0
    assert v1.ctypes.data % 16 == 4      # 4- but not 16-byte aligned: what a slice of an int32 pool gives
    assert v2.ctypes.data % 16 == 8
    with pytest.raises(AssertionError):
        ab.guarded((8,), np.int32, "host", 16)
    with pytest.raises(ValueError):
        ab.guarded((8,), np.int32, "managed")


def test_guard_is_at_least_one_row():
    view, check = ab.guarded((2, 5000), np.int32, "host")
    _poke(view.ctypes.data + (view.size + 4999) * 4, np.int32)   # a whole row past the end still lands in the guard
    with pytest.raises(AssertionError, match="BEHIND"):
        check()


def test_place_and_scribble():
    rng = np.random.default_rng(0)
    a = rng.integers(-5, 5, (6, 7)).astype(np.int32)
    for mis in (0, 1):
        p = ab.place(a[:, ::2], "host", mis)           # a strided source arrives C-contiguous
        assert p.flags["C_CONTIGUOUS"] and np.array_equal(p, a[:, ::2])
        assert p.ctypes.data % 16 == 4 * mis
        assert np.array_equal(ab.host(p), p) and ab.host(p).ctypes.data != p.ctypes.data
        ab.scribble(p)
        assert (p == ab.pattern_value(np.int32)).all()
    e = ab.place(np.zeros(0, np.int32), "host")
    assert e.size == 0
    assert ab.ptr(None) is None
