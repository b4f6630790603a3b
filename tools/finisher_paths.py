"""Solves every case of tests/finisher_cases.py with td_assign (line recogniser off) and prints one JSON object: per section
its wall time and, per case, rc, total, dual, finisher_path (td_last_stats word 13), the words of last_stats(), whether
row_to_col is a permutation and what it costs in the matrix, summed in int64 on the host.  It prints no reference:
tests/test_gpu_finisher_paths.py runs this script in a child process and compares with references that need no GPU.

A section is one child process, because the library reads its environment switches once.  The children run one after
another, each under the timeout of its section; at the first child that times out or ends with a non-zero status the script
prints what it has, starts no further child and exits with status 1.

    python tools/finisher_paths.py [--sections a,b] [--out FILE]
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import finisher_cases as fc  # noqa: E402


def solve_case(td, torch, inst):
    """one td_assign call on the instance: the dict the tests read"""
    from taxidispatcher_amd import _ffi
    n = inst["n"]
    if fc.on_device(inst):
        assert inst["k"] == 0
        a, b = fc.positions(inst)
        cost = torch.empty((n, n), dtype=torch.int32, device="cuda")
        td.cost_build(a.astype(np.int32), b.astype(np.int32), None, fill=fc.BIG, threshold=-1, out=cost)
        matrix = None
    else:
        matrix = fc.numpy_matrix(inst)
        cost = _ffi.as_i32(matrix)
    r2c = np.full(n, -7, np.int32)
    total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
    t0 = time.perf_counter()
    rc = _ffi.lib().td_assign(n, _ffi.addr(cost), _ffi.addr(r2c), ctypes.byref(total), ctypes.byref(dual))
    _ffi.lib().td_synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    out = {"rc": int(rc), "total": int(total.value), "dual": int(dual.value), "finisher_path": int(td.finisher_path()),
           "stats": {k: int(v) for k, v in td.last_stats().items()}, "call_ms": round(ms, 1)}
    if rc == 0:
        out["is_permutation"] = sorted(r2c.tolist()) == list(range(n))
        out["cost_of_r2c"] = fc.cost_of(inst, r2c, matrix)
    del cost
    return out


def solve_section(section):
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    td.set_line_metric(False)
    for case in fc.cases_of(section):
        print(json.dumps({"case": case["name"], "result": solve_case(td, torch, case["inst"])}), flush=True)
    td.shutdown()


def run_section(section):
    """(exit status or "timeout", wall seconds, {case: result})"""
    env, timeout = fc.SECTIONS[section]
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", section], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, text=True, timeout=timeout)
        status, text = r.returncode, r.stdout
    except subprocess.TimeoutExpired as e:
        status, text = "timeout", (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout) or ""
    cases = {}
    for line in text.splitlines():
        if line.startswith('{"case"'):
            d = json.loads(line)
            cases[d["case"]] = d["result"]
    return status, time.perf_counter() - t0, cases


def main():
    if "--section" in sys.argv:
        solve_section(sys.argv[sys.argv.index("--section") + 1])
        return 0
    names = list(fc.SECTIONS)
    if "--sections" in sys.argv:
        names = sys.argv[sys.argv.index("--sections") + 1].split(",")
    out, failed = {}, None
    for sec in names:
        status, wall, cases = run_section(sec)
        out[sec] = {"status": status, "wall_s": round(wall, 1), "cases": cases}
        print("section %s: status %s, %.1f s, %d of %d cases" % (sec, status, wall, len(cases), len(fc.cases_of(sec))), file=sys.stderr, flush=True)
        if status != 0:
            failed = sec   # no further child: whatever ended this one may have left the GPU in a bad state
            break
    text = json.dumps(out)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    print(text)
    if failed is not None:
        print("section %s ended abnormally (%s): stopped there" % (failed, out[failed]["status"]), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
