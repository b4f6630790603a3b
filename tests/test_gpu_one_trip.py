"""td_assign's one-trip sequence (TD_ONE_TRIP=1: the two-hop pass over the whole matrix and the end of the solve are
queued behind the block-local start, gated on the device, with one read-back) against the sequence before it
(TD_ONE_TRIP=0: a read-back after phase A and after that pass, memsets, a copy of row_to_col).  Both run in child
processes on the same instances, in the same order, and must hand back the same row_to_col, total, dual bound and
last_stats() bit for bit."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, json, ctypes, hashlib
sys.path.insert(0, %r)
import numpy as np, torch
import taxidispatcher_amd as td
from taxidispatcher_amd import _ffi
td.init(0)
lib = _ffi.lib()
out = {}
g = torch.Generator(device="cuda").manual_seed(23)

def make(name, n):
    if name == "sparse0":   # zero cells mostly outside the diagonal blocks: the pass over the whole matrix has work, rows may be left
        c = torch.randint(1, 60, (n, n), dtype=torch.int32, device="cuda", generator=g)
        cols = (torch.arange(n, device="cuda") * 7919 + 4321) %% n
        for k in range(6):
            c[torch.arange(n, device="cuda"), (cols + k * 2731) %% n] = 0
        return c
    if name == "sparse1":   # one zero cell per row, outside the blocks: the block-local start leaves too many rows for the two-hop pass
        c = torch.randint(1, 60, (n, n), dtype=torch.int32, device="cuda", generator=g)
        c[torch.arange(n, device="cuda"), (torch.arange(n, device="cuda") * 7919 + 4321) %% n] = 0
        return c
    if name == "wide":      # rows too wide for one byte: the width flag of the speculative 1-byte attempt
        return torch.randint(0, 1000, (n, n), dtype=torch.int32, device="cuda", generator=g)
    c = torch.randint(10, 41, (n, n), dtype=torch.int32, device="cuda", generator=g)
    if name == "constrows":   # deferred constant rows (k_place_const)
        c[torch.randperm(n, device="cuda", generator=g)[:n // 8]] = 40
    elif name == "transposed":   # many constant columns: the shape probe asks for the transposed formulation
        c[:, torch.randperm(n, device="cuda", generator=g)[:n // 4]] = 250
    return c

def solve(c, n, dev_out, want_dual, handle=None):
    total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
    r2c = torch.full((n,), -7, dtype=torch.int32, device="cuda") if dev_out else np.full(n, -7, np.int32)
    args = (n, _ffi.addr(c), _ffi.addr(r2c), ctypes.byref(total), ctypes.byref(dual) if want_dual else None)
    _ffi.check(lib.td_solver_assign(handle, *args) if handle is not None else lib.td_assign(*args))
    r = r2c.cpu().numpy() if dev_out else r2c
    assert sorted(r.tolist()) == list(range(n))
    assert int(c[torch.arange(n, device="cuda"), torch.as_tensor(r, device="cuda").long()].sum().item()) == total.value
    if want_dual:
        assert dual.value == total.value
    return [int(total.value), int(dual.value), hashlib.sha1(r.tobytes()).hexdigest(), sorted(td.last_stats().items())]

cases = [("g1", 12288), ("sparse0", 16384), ("g1", 16384), ("wide", 12288), ("constrows", 16384), ("sparse1", 12288),
         ("transposed", 12288), ("g1", 32768)]
for k, (name, n) in enumerate(cases):
    c = make(name, n)
    for dev_out in (True, False):
        for want_dual in (False, True):
            out["%%s_%%d_%%d_%%d" %% (name, n, int(dev_out), int(want_dual))] = solve(c, n, dev_out, want_dual)
    del c
# a td_solver handle, and the families once more in another order in the same process (a ticket left non-zero, a record
# or a cleared word left behind by one call would show in the next)
h = ctypes.c_void_p()
_ffi.check(lib.td_solver_create(ctypes.byref(h)))
for k, (name, n) in enumerate(reversed(cases[:-1])):
    c = make(name, n)
    out["solver_%%s_%%d" %% (name, n)] = solve(c, n, k %% 2 == 0, k %% 3 == 0, h)
    out["again_%%s_%%d" %% (name, n)] = solve(c, n, k %% 2 == 1, k %% 3 == 1)
    del c
lib.td_solver_destroy(h)
print(json.dumps(out))
""" % ROOT


@pytest.mark.gpu
def test_one_trip_sequence_is_bit_identical(td):
    res = {}
    for mode in ("1", "0"):
        env = dict(os.environ, TD_ONE_TRIP=mode)
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        res[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res["1"]) == 8 * 4 + 2 * 7
    for k in res["0"]:
        assert res["1"][k] == res["0"][k], k
