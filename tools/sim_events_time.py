"""Times the device worlds with the event log off and on (td_sim_log / td_simb_log).

    python tools/sim_events_time.py [--out profiles/sim_events/sim_events_time.json] [--reps 7] [--parent-lib PATH]
    python tools/sim_events_time.py --one-run golden:every_tick      (one run and nothing else: for a kernel trace)

Workloads: `golden`, the committed demand file through td_sim_step, 1300 cabs, 120 ticks; `batch`, tools/sim_batch_time.py's
small_a through td_simb_step, 64 worlds of 150 cabs, 40 ticks.  Settings:
  off          no td_*_log call: the default
  off2         the same again: the spread of this library against itself
  every_tick   every kind on, td_*_events after every tick
  every_10     every kind on, td_*_events after every 10th tick and at the end
  parent_off   --parent-lib: a library built from the parent commit, loaded beside this one, setting `off`
  parent_off2  the same again: the spread of the parent against itself
A run creates its handle, ticks it and destroys it; every call is synchronous, so the host clock around the tick loop ends in
a device synchronise.  All settings alternate within one process (setting after setting, --reps times, after one warm-up
round; every round begins one setting later than the one before, so that no setting always follows the same one); the
median, the smallest and the largest run of a setting are reported, and the records drained and lost.
Everything goes through the raw C ABI, so that two libraries can be driven side by side.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ALL_KINDS = 0xffe
V, I, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64


def declare(lib, with_log):
    lib.td_init.argtypes = [I]
    lib.td_sim_create.argtypes = [I, I, I, I, I32, I, V, V, V, V, V]
    lib.td_sim_step.argtypes = [V, I, V]
    lib.td_sim_destroy.argtypes = [V]
    lib.td_simb_create.argtypes = [I, V, I, I, I, I32, V, V, V, V, V, V]
    lib.td_simb_step.argtypes = [V, I, V]
    lib.td_simb_destroy.argtypes = [V]
    if with_log:
        for name in ("td_sim_log", "td_simb_log"):
            getattr(lib, name).argtypes = [V, ctypes.c_uint32, I64]
        for name in ("td_sim_events", "td_simb_events"):
            getattr(lib, name).argtypes = [V, I64, V, V, V]
    return lib


def ok(rc):
    if rc != 0:
        raise RuntimeError("C ABI call failed: %d" % rc)


def p(a):
    return a.ctypes.data


class Drain:
    """td_*_events into one reusable host buffer"""

    def __init__(self, fn, h, cap):
        self.fn, self.h, self.buf = fn, h, np.empty((cap, 8), np.int32)
        self.n, self.lost = 0, 0

    def __call__(self):
        n, lost = I64(0), I64(0)
        ok(self.fn(self.h, self.buf.shape[0], p(self.buf), ctypes.byref(n), ctypes.byref(lost)))
        self.n += n.value
        self.lost += lost.value


def run_golden(lib, rows, every):
    """every: 0 = logging off, k = every kind on and a drain after every k-th tick; -> (seconds of the tick loop, records, lost)"""
    cols = [np.ascontiguousarray(rows[:, k].astype(np.int32)) for k in (0, 1, 2, 4)]
    h = V()
    ok(lib.td_sim_create(1300, 50, 10, 600, 250000, rows.shape[0], *[p(c) for c in cols], ctypes.byref(h)))
    drain = None
    if every:
        cap = 4 * (1300 + rows.shape[0]) * min(every, 10) + 64
        ok(lib.td_sim_log(h, ALL_KINDS, cap))
        drain = Drain(lib.td_sim_events, h, cap)
    line = np.zeros(9, np.int32)
    t0 = time.perf_counter()
    for t in range(120):
        ok(lib.td_sim_step(h, t, p(line)))
        if every and (t + 1) % every == 0:
            drain()
    if every:
        drain()
    dt = time.perf_counter() - t0
    ok(lib.td_sim_destroy(h))
    return dt, (drain.n if drain else 0), (drain.lost if drain else 0)


def run_batch(lib, packed, ticks, every):
    cabs, off, rid, rfrom, rto, rat = packed
    B = cabs.size
    h = V()
    ok(lib.td_simb_create(B, p(cabs), 12, 4, 16, 250000, p(off), p(rid), p(rfrom), p(rto), p(rat), ctypes.byref(h)))
    drain = None
    if every:
        cap = (4 * (int(cabs.sum()) + int(off[-1])) + 64 * B) * min(every, 10)
        ok(lib.td_simb_log(h, ALL_KINDS, cap))
        drain = Drain(lib.td_simb_events, h, cap)
    line = np.zeros((B, 9), np.int32)
    t0 = time.perf_counter()
    for t in range(ticks):
        ok(lib.td_simb_step(h, t, p(line)))
        if every and (t + 1) % every == 0:
            drain()
    if every:
        drain()
    dt = time.perf_counter() - t0
    ok(lib.td_simb_destroy(h))
    return dt, (drain.n if drain else 0), (drain.lost if drain else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_events", "sim_events_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit (settings parent_off, parent_off2)")
    ap.add_argument("--parent-first", action="store_true", help="load and initialise the parent library before this one")
    ap.add_argument("--one-run", default=None, metavar="WORKLOAD:SETTING", help="one run of golden / batch under off / every_tick / every_10")
    a = ap.parse_args()
    import torch
    import sim_batch_time
    from taxidispatcher_amd import _ffi, simulator
    libs = {}
    for which in (("parent", "new") if a.parent_first else ("new", "parent")):      # the order of loading is part of the experiment
        if which == "new":
            libs["new"] = new = declare(ctypes.CDLL(_ffi.LIB_PATH), True)
            ok(new.td_init(0))
        elif a.parent_lib:
            libs["parent"] = declare(ctypes.CDLL(a.parent_lib), False)
            ok(libs["parent"].td_init(0))
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    tables, fleets, _, b_ticks = sim_batch_time.shape("small_a")
    packed = simulator.pack_worlds(tables, fleets)
    settings = [("off", "new", 0), ("every_tick", "new", 1), ("every_10", "new", 10), ("off2", "new", 0)]
    if a.parent_lib:
        settings += [("parent_off", "parent", 0), ("parent_off2", "parent", 0)]
    work = {"golden": (lambda lib, every: run_golden(lib, rows, every), 120), "batch": (lambda lib, every: run_batch(lib, packed, b_ticks, every), b_ticks)}
    if a.one_run:
        wl, st = a.one_run.split(":")
        every = dict((s, e) for s, _, e in settings)[st]
        dt, n, lost = work[wl][0](new, every)
        print(json.dumps({"workload": wl, "setting": st, "seconds": dt, "records": n, "lost": lost}))
        return
    results = []
    for wl, (fn, ticks) in work.items():
        times = {s: [] for s, _, _ in settings}
        recs = {}
        for rep in range(a.reps + 1):          # round 0 warms every setting up
            for s, which, every in settings[rep % len(settings):] + settings[:rep % len(settings)]:
                dt, n, lost = fn(libs[which], every)
                if rep:
                    times[s].append(dt)
                recs[s] = (n, lost)
        for s, _, _ in settings:
            ts = np.asarray(times[s])
            row = {"workload": wl, "setting": s, "ticks": ticks, "median_ms": float(np.median(ts) * 1e3), "min_ms": float(ts.min() * 1e3),
                   "max_ms": float(ts.max() * 1e3), "ticks_per_s": float(ticks / np.median(ts)), "ms_per_tick": float(np.median(ts) * 1e3 / ticks),
                   "records": recs[s][0], "lost": recs[s][1]}
            print(json.dumps(row), flush=True)
            results.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "parent_lib": bool(a.parent_lib), "parent_first": a.parent_first,
                   "timing": "host clock around the tick loop of synchronous calls; settings alternate in one process; one warm-up round",
                   "results": results}, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
