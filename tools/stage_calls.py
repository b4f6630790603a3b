"""One warm call of every entry point behind csrc/td_stage.h, for a HIP API trace and for host-path timing.

    rocprofv3 --hip-trace --stats -d DIR -- python tools/stage_calls.py run [--shape 1000,100,50] > run.json
    python tools/stage_calls.py count DIR/.../*_hip_api_trace.csv --names run.json
    python tools/stage_calls.py time [--shape 1000,100,50] [--reps 9]

run    makes the good calls of tests/stage_refusal_cases.py (every array in host memory, so that every HIP call in the trace is
       the library's), each twice: first the warm-ups, then, between device synchronisations of the caller, the calls that
       count.  The library itself synchronises its stream only, so the trace splits at those marks.  A call the library
       refuses at this shape is left out; the JSON object that run prints names the calls that count and the refused ones.
       Shape "3,4,5" (the default) is the refusal test's; "1000,100,50" is the shape of tools/dispatch_batched_time.py:
       1000 models of 50 .. 100 a side on 50 stands.
count  reads the trace and prints, per entry point, the kernel launches, hipMemcpyAsync, hipMemsetAsync and hipStreamSynchronize
       of the call that counts, as one JSON object.  Two commits are compared by comparing these objects.
time   prints the median wall time of each call in microseconds (after one warm-up), as one JSON object.
td_simb_create is create + 6 td_simb_step + destroy, td_simb_apply is create + begin + apply + destroy.  The calls that take
ragged offsets are made once more with the offset arrays in device memory (the position arrays and the outputs on the host).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

COUNTED = {"hipLaunchKernel": "launch", "hipModuleLaunchKernel": "launch", "hipExtLaunchKernel": "launch", "hipMemcpyAsync": "memcpy",
           "hipMemsetAsync": "memset", "hipStreamSynchronize": "sync"}


def good_ids(cases):
    return [c for c in cases.case_ids() if c.endswith("/good/host")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "count", "time"))
    ap.add_argument("trace", nargs="?")
    ap.add_argument("--shape", default="3,4,5")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--names", help="count: what run printed")
    a = ap.parse_args()
    if a.mode == "count":
        with open(a.names) as f:
            ids = json.load(f)["counted"]
        segs, cur = [], None   # the counted calls between two marks
        with open(a.trace) as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            if r["Function"] == "hipDeviceSynchronize":
                if cur:
                    segs.append(cur)
                cur = {}
            elif cur is not None and r["Function"] in COUNTED:
                k = COUNTED[r["Function"]]
                cur[k] = cur.get(k, 0) + 1
        # the calls that count are the last segments: start-up, the harness's device copies and the warm-ups lie in front of them
        assert len(segs) >= len(ids), "%d segments with library calls for %d calls" % (len(segs), len(ids))
        print(json.dumps({c: dict({"launch": 0, "memcpy": 0, "memset": 0, "sync": 0}, **g) for c, g in zip(ids, segs[-len(ids):])}, indent=1, sort_keys=True))
        return
    import stage_refusal_cases as cases
    import abi_buffers as ab
    import torch
    import taxidispatcher_amd as td
    from taxidispatcher_amd import _ffi
    cases.set_shape(*(int(v) for v in a.shape.split(",")))
    td.init(0)
    lib = _ffi.lib()
    # every good call with host arrays, then the calls that take ragged offsets with the offsets in device memory (placed here,
    # in front of the first mark, so that the harness's own copies are not in a counted segment; outputs stay host windows)
    calls, skipped, keep = [], {}, []
    for c in good_ids(cases):
        calls.append((c.split("/")[0], lambda c=c: cases.run_case(lib, c)["rc"]))
    for name, (names, shapes, call, _, offs, _) in cases.CALLS.items():
        if offs == ("ns",):
            continue
        arrays = {q: dict(cases.IN, **cases.EXTRA_IN)[q] for q in names}
        arrays.update({q: ab.place(arrays[q], "device") for q in offs})
        outs = {q: ab.guarded(shape, dt, "host")[0] for q, (shape, dt) in shapes.items()}
        keep.append((arrays, outs))
        A, O = {q: ab.ptr(v) for q, v in arrays.items()}, {q: ab.ptr(v) for q, v in outs.items()}
        calls.append((name + ", offsets on the device", lambda call=call, A=A, O=O: call(lib, A, O, {"batch": cases.B})))
    ids = []
    for name, f in calls:   # the warm-ups
        if f():
            skipped[name] = cases.last_error(lib)
        else:
            ids.append((name, f))
    out = {}
    torch.cuda.synchronize()
    for name, f in ids:
        times = []
        for _ in range(1 if a.mode == "run" else a.reps):
            t0 = time.perf_counter()
            rc = f()
            times.append(time.perf_counter() - t0)
            assert rc == 0, (name, cases.last_error(lib))
            torch.cuda.synchronize()
        out[name] = round(statistics.median(times) * 1e6, 1)
    td.shutdown()
    print(json.dumps({"counted": [name for name, _ in ids], "skipped": skipped, "median_us": out if a.mode == "time" else None}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
