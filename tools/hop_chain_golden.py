"""Solves the instances of tests/test_gpu_hop_chain.py with td_assign and prints (or writes with --out) one JSON object:
for every case and for a device and a host row_to_col, [total, dual bound, sha1 of row_to_col, last_stats()].

tests/golden/hop_chain_parent.json is this script's output at the commit before the two-hop chain was trimmed
(profiles/hop_chain/README.md); the test runs the script in a child process and compares.  The instances are seeded and
made on the device, so the file holds no matrix.

    python tools/hop_chain_golden.py --out tests/golden/hop_chain_parent.json
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (family, n) in the order they are solved; the families are those of tests/test_gpu_one_trip.py
CASES = [("perfjl", 12288), ("perfjl", 16384), ("sparse0", 16384), ("sparse1", 12288), ("constrows", 16384), ("perfjl", 32768)]
# One child process per section (the library reads its switches once).  "maxrows": no local round after round 0 and
# TD_HOP_MAX_ROWS lifted, so that every block enters the two-hop passes with hundreds of free rows, of which a pass looks at
# the first HOP_FMAX = 128 against the first 128 free columns, and the pass over the whole matrix runs on 128 of the rows
# left (perf.jl: about n / 31 zero cells a row, full tables; sparse0: nearly empty tables).
SECTIONS = {"default": ({}, CASES),
            "maxrows": ({"TD_HOP_MAX_ROWS": "100000", "TD_ZS_ROUNDS": "0"}, [("perfjl", 16384), ("sparse0", 16384), ("perfjl", 12288)])}


def make(torch, g, name, n):
    ar = torch.arange(n, device="cuda")
    if name == "sparse0":   # zero cells mostly outside the diagonal blocks: the pass over the whole matrix places rows
        c = torch.randint(1, 60, (n, n), dtype=torch.int32, device="cuda", generator=g)
        cols = (ar * 7919 + 4321) % n
        for k in range(6):
            c[ar, (cols + k * 2731) % n] = 0
        return c
    if name == "sparse1":   # one zero cell per row, outside the blocks: more rows left than TD_HOP_MAX_ROWS
        c = torch.randint(1, 60, (n, n), dtype=torch.int32, device="cuda", generator=g)
        c[ar, (ar * 7919 + 4321) % n] = 0
        return c
    c = torch.randint(10, 41, (n, n), dtype=torch.int32, device="cuda", generator=g)   # perf.jl: U{10..40}
    if name == "constrows":
        c[torch.randperm(n, device="cuda", generator=g)[:n // 8]] = 40
    return c


def solve_section(cases):
    import numpy as np
    import torch
    import taxidispatcher_amd as td
    from taxidispatcher_amd import _ffi
    td.init(0)
    lib = _ffi.lib()
    g = torch.Generator(device="cuda").manual_seed(41)
    out = {}
    for name, n in cases:
        c = make(torch, g, name, n)
        ar = torch.arange(n, device="cuda")
        for dev_out in (True, False):
            total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
            r2c = torch.full((n,), -7, dtype=torch.int32, device="cuda") if dev_out else np.full(n, -7, np.int32)
            _ffi.check(lib.td_assign(n, _ffi.addr(c), _ffi.addr(r2c), ctypes.byref(total), ctypes.byref(dual)))
            r = r2c.cpu().numpy() if dev_out else r2c
            perm = sorted(r.tolist()) == list(range(n))
            cost = int(c[ar, torch.as_tensor(r, device="cuda").long().clamp(0, n - 1)].sum().item())
            out["%s_%d_%s" % (name, n, "dev" if dev_out else "host")] = {
                "total": int(total.value), "dual": int(dual.value), "sha1": hashlib.sha1(r.tobytes()).hexdigest(),
                "stats": sorted([k, int(v)] for k, v in td.last_stats().items() if k not in ("lcm_path", "line_path")), "is_permutation": perm, "cost_of_r2c": cost}
        del c
    return out


def main():
    if "--section" in sys.argv:
        print(json.dumps(solve_section(SECTIONS[sys.argv[sys.argv.index("--section") + 1]][1])))
        return
    out = {}
    for sec, (env, _) in SECTIONS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", sec], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit("section %s: exit status %d" % (sec, r.returncode))
        out[sec] = json.loads(r.stdout.strip().splitlines()[-1])
    # one line per case
    text = "{\n" + ",\n".join(' "%s": {\n' % sec + ",\n".join('  "%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in sorted(out[sec].items()))
                              + "\n }" for sec in sorted(out)) + "\n}"
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    else:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
