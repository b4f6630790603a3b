"""Solves the instances of tests/test_gpu_phase_a_trips.py and prints (or writes with --out) one JSON object: for every case
and for a device and a host row_to_col, total, dual bound, sha1 of row_to_col, last_stats(), whether row_to_col is a
permutation, what it costs in the matrix, and the `[td] phase A` lines TD_DEBUG printed during the solve, parsed (free rows /
columns per block in front of the last in-block two-hop pass, matched, left: the HopCtl words).

tests/golden/phase_a_trips_parent.json is this script's output at the commit before the chain kernels of phase A issued
their flag, gate and count loads together with their first data loads and k_zs_bid took one row per wave
(profiles/phase_a_trips/README.md); the test runs the script in a child process and compares.  The instances are seeded and
made on the device, so the file holds no matrix.

    python tools/phase_a_trips_golden.py --out tests/golden/phase_a_trips_parent.json
    python tools/phase_a_trips_golden.py --debug-out profiles/phase_a_trips/coverage_parent_debug.txt

Every section is a child process of its own (the TD_* settings are read once), forces 8 diagonal blocks
(td_set_blocks(8), TD_BLOCKS_MIN_N=0) and runs with TD_DEBUG=1; the sections run side by side, JOBS at a time.  The cases of
a section are solved one behind the other on td_assign's own handle, so the lists and tables of one n are what the solve of
the next n finds.
"""
import concurrent.futures
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASE_ENV = {"TD_BLOCKS_MIN_N": "0", "TD_DEBUG": "1"}
SEQ = [("perfjl", 12416), ("perfjl", 12288), ("perfjl", 12416)]
# (family, n) in the order they are solved; see the docstring of tests/test_gpu_phase_a_trips.py for what each one covers
SECTIONS = {"passes1": ({"TD_HOP_PASSES": "1"}, SEQ),
            "passes2": ({"TD_HOP_PASSES": "2"}, SEQ),
            "passes3": ({"TD_HOP_PASSES": "3"}, SEQ),
            "rounds0": ({"TD_ZS_ROUNDS": "0"}, [("perfjl", 12288), ("perfjl", 12416)]),
            "rounds1": ({"TD_ZS_ROUNDS": "1"}, [("perfjl", 12288), ("perfjl", 12416)]),
            "rounds2": ({"TD_ZS_ROUNDS": "2"}, [("perfjl", 12288), ("perfjl", 12416)]),
            "maxrows": ({"TD_HOP_MAX_ROWS": "100000", "TD_ZS_ROUNDS": "0"}, [("perfjl", 12416)]),
            "const64": ({}, [("const64", 12288)]),
            "wide": ({}, [("wide", 12416)]),
            "sparse": ({}, [("sparse1", 12288), ("sparse0", 12416)]),
            "shards": ({}, [("perfjl", 12288)]),
            "n16384": ({}, [("perfjl", 16384)])}
WORLD = 8   # "shards": one diagonal block per shard
JOBS = 6    # child processes with the GPU open at a time
PHASE_A = re.compile(r"^\[td\] phase A: (\d+) blocks of (\d+) rows, (\d+) local rounds; .*?:((?: \d+/\d+)+) \| matched (-?\d+), left (-?\d+)")


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
    c = torch.randint(10, 41, (n, n), dtype=torch.int32, device="cuda", generator=g)   # perf.jl: U{10..40}
    if name == "const64":   # 64 constant rows, 8 in every block: they sit the solve out (r2c = -2) and take the columns left
        c[(ar[:64] * 191 + 5) % n] = 25
    if name == "wide":      # one cell that does not fit a byte: the compress pass raises the width flag
        c[5, 7] = 10 ** 6
    return c


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
    g = torch.Generator(device="cuda").manual_seed(47)
    out = {}
    for idx, (name, n) in enumerate(cases):
        c = make(torch, g, name, n)
        for dev_out in (True, False):
            key = "%d_%s_%d_%s" % (idx, name, n, "dev" if dev_out else "host")
            sys.stderr.write("== %s\n" % key)
            sys.stderr.flush()
            total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
            r2c = torch.full((n,), -7, dtype=torch.int32, device="cuda") if dev_out else np.full(n, -7, np.int32)
            _ffi.check(lib.td_assign(n, _ffi.addr(c), _ffi.addr(r2c), ctypes.byref(total), ctypes.byref(dual)))
            r = r2c.cpu().numpy() if dev_out else r2c
            out[key] = record(torch, c, n, r, total.value, dual.value, sorted([k, int(v)] for k, v in td.last_stats().items() if k not in ("lcm_path", "line_path")))
        if sec == "shards":   # the same matrix through the shard API, every shard in this process
            from taxidispatcher_amd import sharded
            sys.stderr.write("== %d_%s_%d_api\n" % (idx, name, n))
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


def phase_a_lines(stderr):
    """{case key: the parsed `[td] phase A` lines printed while it was solved}"""
    got, key = {}, None
    for ln in stderr.splitlines():
        if ln.startswith("== "):
            key = ln[3:].strip()
            got[key] = []
            continue
        m = PHASE_A.match(ln)
        if m and key is not None:
            got[key].append({"blocks": int(m.group(1)), "rpb": int(m.group(2)), "rounds": int(m.group(3)),
                             "free": [[int(x) for x in p.split("/")] for p in m.group(4).split()],
                             "matched": int(m.group(5)), "left": int(m.group(6))})
    return got


def run_section(sec):
    e = dict(os.environ, **BASE_ENV, **SECTIONS[sec][0])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", sec], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        return sec, None, "section %s: exit status %d\n%s" % (sec, r.returncode, (r.stderr or "")[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    pa = phase_a_lines(r.stderr)
    for k, v in res.items():
        v["phase_a"] = pa.get(k, [])
    log = ["== %s/%s" % (sec, ln[3:]) if ln.startswith("== ") else ln for ln in r.stderr.splitlines()
           if ln.startswith("== ") or ln.startswith("[td] phase A") or ln.startswith("[td] one trip")]
    return sec, res, log


def main():
    if "--section" in sys.argv:
        sec = sys.argv[sys.argv.index("--section") + 1]
        print(json.dumps(solve_section(sec, SECTIONS[sec][1])))
        return
    debug = sys.argv[sys.argv.index("--debug-out") + 1] if "--debug-out" in sys.argv else None
    out, logs = {}, {}
    with concurrent.futures.ThreadPoolExecutor(JOBS) as ex:
        for sec, res, log in ex.map(run_section, list(SECTIONS)):
            if res is None:
                sys.exit(log)
            out[sec], logs[sec] = res, log
    if debug:
        with open(debug, "w") as f:
            f.write("\n".join(ln for sec in SECTIONS for ln in logs[sec]) + "\n")
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
