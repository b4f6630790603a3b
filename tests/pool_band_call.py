"""td_pool_n_banded as C sees it, for the GPU tests of the banded finder: max_pools, the slice and the fill behind the records
are visible here, which the Python surface hides."""
import ctypes

import numpy as np


def raw(k, n, cols, dist, first, room, max_pools, out=None, stats=True, happy=True):
    """td_pool_n_banded as C sees it; cols / out: numpy arrays or device tensors"""
    from taxidispatcher_amd import _ffi as f
    lib = f.lib()
    fill = -7
    if out is None:
        out = np.full((max(max_pools, 1) + 2, 2 * k + 1), fill, np.int32)
    m, nh = ctypes.c_int32(-5), ctypes.c_int64(-5)
    st = np.full(4, -5, np.int64)
    S = 0 if dist is None else int(dist.shape[0])
    rc = lib.td_pool_n_banded(k, n, *[f.addr(c) for c in cols], f.addr(dist), S, first[0], first[1], room, max_pools, f.addr(out),
                              ctypes.byref(m), ctypes.byref(nh) if happy else None, f.addr(st) if stats else None)
    host = out if isinstance(out, np.ndarray) else out.cpu().numpy()
    kept = max(m.value, 0)
    return dict(rc=rc, n_pools=m.value, happy=nh.value, stats=tuple(int(v) for v in st), recs=host[:kept].tolist(),
                behind=host[kept:], fill=fill)
