"""Buffers for tests of the C ABI's memory contract (tests/test_gpu_abi_contract.py).  TEST INFRASTRUCTURE ONLY.

Every array handed to the library here is a C-contiguous window inside a larger allocation that the test owns: an output
has guard words on both sides, filled like the window itself with the byte 0x5A, so a kernel that stores past the stated
extent of an output lands in memory of the test and is seen by check(); an input sits in host, pinned or device memory at
a chosen alignment (a slice of a pool is aligned to its element size only, not to 16 bytes).  Nothing here hands the
library an undersized or invalid pointer."""
import numpy as np

PATTERN = 0x5A
GUARD_MIN = 256          # elements on each side, or one row of the output when that is longer
KINDS = ("host", "pinned", "device")

_TORCH_DTYPES = {"int32": "int32", "int64": "int64", "uint8": "uint8", "uint64": "int64"}


def pattern_value(dtype):
    """the value an element of `dtype` has when every byte of it is PATTERN"""
    return np.frombuffer(bytes([PATTERN]) * np.dtype(dtype).itemsize, dtype=dtype)[0]


def _raw(nbytes, kind):
    """(numpy uint8 view of the host bytes or None, torch uint8 tensor or None, base address) of a fresh allocation"""
    if kind == "host":
        raw = np.empty(nbytes, np.uint8)
        return raw, None, raw.ctypes.data
    import torch
    if kind == "pinned":
        t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return t.numpy(), t, t.data_ptr()
    if kind == "device":
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        return None, t, t.data_ptr()
    raise ValueError("kind %r is not one of %r" % (kind, KINDS))


def guarded(shape, dtype, kind, misalign=0):
    """-> (view, check).  view: a C-contiguous window of `shape` / `dtype` (numpy array for host and pinned memory, torch
    tensor for device memory) whose base address is 16-byte aligned plus `misalign` ELEMENTS; view and both guard regions
    (at least max(256 elements, one row) each) hold PATTERN in every byte.  check() asserts that both guards still do."""
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    dt = np.dtype(dtype)
    item = dt.itemsize
    size = int(np.prod(shape)) if shape else 1
    row = shape[-1] if shape else 1
    guard = -(-max(GUARD_MIN, row) // 16) * 16           # elements; a multiple of 16 keeps guard * item a multiple of 16
    misalign = int(misalign)
    assert 0 <= misalign < 16
    front = (guard + misalign) * item
    nbytes = front + (size + guard) * item
    host, tens, base = _raw(nbytes + 64, kind)
    skip = (-base) % 64                                   # the front guard starts on a 64-byte boundary
    lo, mid, hi = skip, skip + front, skip + front + size * item
    end = hi + guard * item
    if host is not None:
        host[:] = PATTERN
        view = host[mid:hi].view(dt).reshape(shape)
        address = view.ctypes.data if size else base + mid
    else:
        import torch
        tens.fill_(PATTERN)
        view = tens[mid:hi].view(getattr(torch, _TORCH_DTYPES[dt.name])).reshape(shape)
        address = base + mid
        torch.cuda.synchronize()
    # the case asked for, not silently the aligned one (or the other way round)
    assert address == base + mid and address % 16 == (misalign * item) % 16, (hex(address), misalign, item)
    assert address % item == 0

    def check():
        if host is not None:
            g0, g1 = host[lo:mid], host[hi:end]
        else:
            import torch
            torch.cuda.synchronize()
            g0, g1 = tens[lo:mid].cpu().numpy(), tens[hi:end].cpu().numpy()
        bad0, bad1 = np.nonzero(g0 != PATTERN)[0], np.nonzero(g1 != PATTERN)[0]
        assert bad0.size == 0, "guard BEFORE the output overwritten: %d bytes, the nearest %d bytes in front of it" % (
            bad0.size, g0.size - int(bad0[-1]))
        assert bad1.size == 0, "guard BEHIND the output overwritten: %d bytes, the first %d bytes past its end" % (
            bad1.size, int(bad1[0]))

    return view, check


def place(array, kind, misalign=0):
    """the same data as `array` in host, pinned or device memory, as a window inside a larger allocation (guarded()):
    kind "device" with misalign > 0 is a device view that starts inside its allocation at element alignment only"""
    a = np.ascontiguousarray(array)
    view, _ = guarded(a.shape, a.dtype, kind, misalign)
    if isinstance(view, np.ndarray):
        view[...] = a
    else:
        import torch
        src = a.view(np.int64) if a.dtype == np.uint64 else a
        view.copy_(torch.from_numpy(src))
        torch.cuda.synchronize()   # the library works on a stream of its own: the input is complete before it sees it
    return view


def ptr(x):
    """raw address of a numpy array / torch tensor (None stays None): what goes through the C ABI, no synchronisation"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    # (data_ptr() of an empty tensor is null; the window of an empty output still has its place between the guards)
    return x.untyped_storage().data_ptr() + x.storage_offset() * x.element_size()


def host(x):
    """host numpy copy of a numpy array / torch tensor"""
    if isinstance(x, np.ndarray):
        return x.copy()
    return x.cpu().numpy()


def scribble(x):
    """overwrite every byte of an input window with PATTERN (after a call: the library must not read it again)"""
    if isinstance(x, np.ndarray):
        x.view(np.uint8).reshape(-1)[:] = PATTERN
    else:
        import torch
        x.view(torch.uint8).fill_(PATTERN)
        torch.cuda.synchronize()
