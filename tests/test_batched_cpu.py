"""CPU tier of the batched entry points (td_assign_batched / td_lcm_batched): no CPU fallback, and the host-side
packing of a list of differently sized models into one padded slab."""

import numpy as np
import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def built():
    entry.build()
    from taxidispatcher_amd import _ffi
    return _ffi


def test_batched_no_cpu_fallback(built):
    """Without a GPU the batched calls fail loudly, exactly like td_assign (test_abi.py::test_no_cpu_fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path is exercised on the CPU tier only")
    lib = built.load()
    import taxidispatcher_amd as td
    c = np.zeros((3, 4, 4), np.int32)
    with pytest.raises(td.TdError):
        td.assign_batched(c)
    with pytest.raises(td.TdError):
        td.LCM_batched(c, mask=100)
    with pytest.raises(td.TdError):
        td.heuristic_gap(n=4, iters=2, seed=0)
    # not initialised -> ENOINIT from the C ABI itself
    r2c = np.zeros(12, np.int32)
    tot = np.zeros(3, np.int64)
    assert lib.td_assign_batched(3, 4, None, c.ctypes.data, r2c.ctypes.data, tot.ctypes.data, None, None) == -3
    k = np.zeros(3, np.int32)
    lm = np.zeros(3, np.int32)
    assert lib.td_lcm_batched(3, 4, None, c.ctypes.data, 100, -1, 0, 0, -1, 2**62, r2c.ctypes.data, r2c.ctypes.data,
                              k.ctypes.data, tot.ctypes.data, lm.ctypes.data) == -3


def test_batched_symbols_declared(built):
    lib = built.load()
    for name in ("td_assign_batched", "td_lcm_batched"):
        assert name in built.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.td_version() == 101


def test_pack_list_of_models():
    from taxidispatcher_amd.dispatch import pack_batch
    rng = np.random.default_rng(3)
    mats = [rng.integers(-5, 50, (k, k)) for k in (3, 0, 5, 1)]
    slab, ns, batch, n = pack_batch(mats)
    assert batch == 4 and n == 5
    assert slab.dtype == np.int32 and slab.shape == (4, 5, 5) and slab.flags["C_CONTIGUOUS"]
    assert ns.dtype == np.int32 and ns.tolist() == [3, 0, 5, 1]
    for b, m in enumerate(mats):
        k = m.shape[0]
        assert np.array_equal(slab[b, :k, :k], m)
        assert not slab[b, k:, :].any() and not slab[b, :, k:].any()


def test_pack_slab_and_errors():
    from taxidispatcher_amd import TdError
    from taxidispatcher_amd.dispatch import pack_batch
    c = np.arange(2 * 3 * 3, dtype=np.int64).reshape(2, 3, 3)
    slab, ns, batch, n = pack_batch(c, ns=[3, 2])
    assert slab.dtype == np.int32 and np.array_equal(slab, c) and ns.tolist() == [3, 2] and (batch, n) == (2, 3)
    slab, ns, batch, n = pack_batch(c)
    assert ns is None and (batch, n) == (2, 3)
    with pytest.raises(TdError):
        pack_batch(np.zeros((2, 3, 4), np.int32))       # not square
    with pytest.raises(TdError):
        pack_batch(c, ns=[3])                           # ns of the wrong length
    with pytest.raises(TdError):
        pack_batch([np.zeros((2, 3), np.int32)])        # a non-square model in the list
    with pytest.raises(TdError):
        pack_batch([np.zeros((2, 2), np.int32)], ns=[2])
    slab, ns, batch, n = pack_batch([])
    assert (batch, n) == (0, 0) and slab.shape == (0, 0, 0) and ns.size == 0
