"""Solves the instances of tests/test_gpu_hop_fold.py and prints (or writes with --out) one JSON object: for every case and
for a device and a host row_to_col, total, dual bound, sha1 of row_to_col, last_stats(), whether row_to_col is a
permutation and what it costs in the matrix.

tests/golden/hop_fold_parent.json is this script's output at the commit before k_hop_esc was folded into k_hop_table
(profiles/hop_fold/README.md); the test runs the script in a child process and compares.  The
instances are seeded and made on the device, so the file holds no matrix.

    python tools/hop_fold_golden.py --out tests/golden/hop_fold_parent.json
    python tools/hop_fold_golden.py --debug-out profiles/hop_fold/coverage_parent_debug.txt
        (TD_DEBUG's lines on the block-local start per case, and again with TD_HOP_PASSES=1: the line shows the counts in
        front of the last in-block pass, which is then the first)

All sections force 8 diagonal blocks (td_set_blocks(8), TD_BLOCKS_MIN_N=0).  The cases of a section are solved one behind
the other on td_assign's own handle, so "default" is also the sequence n = 12 416, 12 288, 12 416, 12 288, 12 416 on one
handle: the two-hop tables and lists of one solve are what the next one finds.
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

BASE_ENV = {"TD_BLOCKS_MIN_N": "0"}
# (family, n) in the order they are solved; see the docstring of tests/test_gpu_hop_fold.py for what each one covers
SECTIONS = {"default": ({}, [("perfjl", 12416), ("perfjl", 12288), ("perfjl", 12416), ("sparse1", 12288), ("sparse0", 12416)]),
            "maxrows": ({"TD_HOP_MAX_ROWS": "100000", "TD_ZS_ROUNDS": "0"}, [("perfjl", 12416)]),
            "shards": ({}, [("perfjl", 12288)])}
WORLD = 8   # "shards": one diagonal block per shard


def make(torch, g, name, n):
    ar = torch.arange(n, device="cuda")
    if name == "sparse0":   # zero cells mostly outside the diagonal blocks
        c = torch.randint(1, 60, (n, n), dtype=torch.int32, device="cuda", generator=g)
        cols = (ar * 7919 + 4321) % n
        for k in range(6):
            c[ar, (cols + k * 2731) % n] = 0
        return c
    if name == "sparse1":   # one zero cell per row, outside the blocks: more rows left than TD_HOP_MAX_ROWS
        c = torch.randint(1, 60, (n, n), dtype=torch.int32, device="cuda", generator=g)
        c[ar, (ar * 7919 + 4321) % n] = 0
        return c
    return torch.randint(10, 41, (n, n), dtype=torch.int32, device="cuda", generator=g)   # perf.jl: U{10..40}


def record(torch, c, n, r, total, dual, stats):
    ar = torch.arange(n, device="cuda")
    perm = sorted(r.tolist()) == list(range(n))
    cost = int(c[ar, torch.as_tensor(r, device="cuda").long().clamp(0, n - 1)].sum().item())
    return {"total": int(total), "dual": int(dual), "sha1": hashlib.sha1(r.tobytes()).hexdigest(), "stats": stats,
            "is_permutation": perm, "cost_of_r2c": cost}


def solve_section(sec, cases):
    import numpy as np
    import torch
    import taxidispatcher_amd as td
    from taxidispatcher_amd import _ffi
    td.init(0)
    lib = _ffi.lib()
    lib.td_set_blocks(8)
    g = torch.Generator(device="cuda").manual_seed(43)
    out = {}
    for idx, (name, n) in enumerate(cases):
        c = make(torch, g, name, n)
        for dev_out in (True, False):
            key = "%d_%s_%d_%s" % (idx, name, n, "dev" if dev_out else "host")
            sys.stderr.write("== %s/%s\n" % (sec, key))
            sys.stderr.flush()
            total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
            r2c = torch.full((n,), -7, dtype=torch.int32, device="cuda") if dev_out else np.full(n, -7, np.int32)
            _ffi.check(lib.td_assign(n, _ffi.addr(c), _ffi.addr(r2c), ctypes.byref(total), ctypes.byref(dual)))
            r = r2c.cpu().numpy() if dev_out else r2c
            out[key] = record(torch, c, n, r, total.value, dual.value, sorted([k, int(v)] for k, v in td.last_stats().items() if k not in ("lcm_path", "line_path")))
        if sec == "shards":   # the same matrix through the shard API, every shard in this process
            from taxidispatcher_amd import sharded
            sys.stderr.write("== %s/%d_%s_%d_api\n" % (sec, idx, name, n))
            sys.stderr.flush()
            shards = []
            try:
                for k in range(WORLD):
                    row0, nrows, _ = sharded.shard_bounds(n, WORLD, k)
                    shards.append(sharded.HipShard(n, row0, nrows, c[row0:row0 + nrows], share_torch_stream=False))
                r, tot, dual, info = sharded.solve_shards_in_process(shards, blocks=True, fused_round0=True)
            finally:
                for s in shards:
                    s.close()
            r = np.ascontiguousarray(np.asarray(r, dtype=np.int32))
            out["%d_%s_%d_api" % (idx, name, n)] = record(torch, c, n, r, tot, dual, [["left", -1 if info["left"] is None else int(info["left"])], ["path", info["path"]]])
        del c
    return out


def main():
    if "--section" in sys.argv:
        sec = sys.argv[sys.argv.index("--section") + 1]
        print(json.dumps(solve_section(sec, SECTIONS[sec][1])))
        return
    debug = sys.argv[sys.argv.index("--debug-out") + 1] if "--debug-out" in sys.argv else None
    out, log = {}, []
    for sec, (env, _) in SECTIONS.items():
        e = dict(os.environ, **BASE_ENV, **env)
        if debug:
            e["TD_DEBUG"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", sec], env=e, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE if debug else None, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit("section %s: exit status %d\n%s" % (sec, r.returncode, (r.stderr or "")[-3000:]))
        out[sec] = json.loads(r.stdout.strip().splitlines()[-1])
        if debug:
            log += [ln for ln in r.stderr.splitlines() if ln.startswith("== ") or ln.startswith("[td] phase A") or ln.startswith("[td] one trip")]
            # TD_DEBUG prints the counts in front of the LAST in-block pass: the same cases with one pass show the first one's
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", sec], env=dict(e, TD_HOP_PASSES="1"),
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit("section %s, one pass: exit status %d\n%s" % (sec, r.returncode, r.stderr[-3000:]))
            log += [("== TD_HOP_PASSES=1 " + ln[3:]) if ln.startswith("== ") else ln for ln in r.stderr.splitlines()
                    if ln.startswith("== ") or ln.startswith("[td] phase A") or ln.startswith("[td] one trip")]
    if debug:
        with open(debug, "w") as f:
            f.write("\n".join(log) + "\n")
    # one line per case
    text = "{\n" + ",\n".join(' "%s": {\n' % sec + ",\n".join('  "%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in sorted(out[sec].items()))
                              + "\n }" for sec in sorted(out)) + "\n}"
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    elif not debug:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
