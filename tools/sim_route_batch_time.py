"""Times routed worlds in a batch (td_simb_route).

    python tools/sim_route_batch_time.py --default-path --parent-lib PATH [--parent-first] [--reps 7] [--out FILE.json]
    python tools/sim_route_batch_time.py --routed [--reps 5] [--only small,large] [--out FILE.json]
    python tools/sim_route_batch_time.py --one-run on|off      (one batched run of the small shape and nothing else: for a kernel trace)

--default-path: section 3.7's shape (64 worlds of 150 cabs on 50 stands, DROP_TIME 10, MAX_NON_LCM 600, a seeded request file per
  world, 40 ticks) through td_simb_step on a default batch and on a (3,2) batch (wait 1, loss 50, plan buffer 24 * 512) that never
  calls td_simb_route, on this library and on one built from the parent commit, both loaded into this process (--parent-first:
  the parent is loaded and initialised first; the order is part of the experiment).  Every setting twice under two names, so
  that each library's spread against itself is in the table.  Settings alternate within the process, --reps times after one
  warm-up round; every round begins one setting later.  Everything goes through the raw C ABI.
--routed: a routed batch against a loop of DeviceSimulator(route=True) handles, and both unrouted, under (3,2) with a plan buffer:
  `small` = the shape above; `large` = 8 worlds of 1000 cabs on the same city, about 100 requests per tick and world (a record
  world of a batch holds at most 512 requests a tick).  A run = create, tick, read the metrics, destroy; each side is warmed up
  once, then the median, smallest and largest of --reps runs.  A refused tick ends the row and is reported with the message.
Host clock around synchronous calls: every tick ends in a device synchronise."""
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
from sim_batch_time import BIG, gen_demand, timed

V, I, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64
CITY = dict(n_stands=50, drop_time=10, max_non_lcm=600, big_cost=BIG)
TICKS = 40
PN, WAIT, LOSS = (3, 2), 1, 50
BUFFER_BATCH, BUFFER_HANDLE = 24 * 512, 24 * 2047      # the smallest plan buffers the two handles take
SHAPES = {"small": dict(B=64, cabs=150, per_tick=46), "large": dict(B=8, cabs=1000, per_tick=100)}


def tables_of(shape):
    s = SHAPES[shape]
    return [gen_demand(CITY["n_stands"], s["per_tick"], TICKS, 4, 10, 100 + b) for b in range(s["B"])], [s["cabs"]] * s["B"]


def declare(lib):
    lib.td_init.argtypes = [I]
    lib.td_simb_create.argtypes = [I, V, I, I, I, I32, V, V, V, V, V, V]
    lib.td_simb_step.argtypes = [V, I, V]
    lib.td_simb_destroy.argtypes = [V]
    lib.td_simb_pooling_n.argtypes = [V, V, V, V, V, I64]
    lib.td_simb_pool_buffer.argtypes = [V, I64]
    lib.td_simb_metrics.argtypes = [V, V]
    return lib


def ok(rc):
    if rc != 0:
        raise RuntimeError("C ABI call failed: %d" % rc)


def run_steps(lib, packed, pn):
    """a batch that never calls td_simb_route: create, TICKS x td_simb_step, metrics, destroy -> (seconds, total_dropped over the worlds)"""
    cabs, off, cols = packed
    B = int(cabs.size)
    t0 = time.perf_counter()
    h = V()
    ok(lib.td_simb_create(B, cabs.ctypes.data, CITY["n_stands"], CITY["drop_time"], CITY["max_non_lcm"], CITY["big_cost"], off.ctypes.data,
                          *[c.ctypes.data for c in cols], ctypes.byref(h)))
    if pn:
        hi, lo, wt, ls = (np.full(B, v, np.int32) for v in (pn[0], pn[1], WAIT, LOSS))
        ok(lib.td_simb_pooling_n(h, hi.ctypes.data, lo.ctypes.data, wt.ctypes.data, ls.ctypes.data, 0))
        ok(lib.td_simb_pool_buffer(h, BUFFER_BATCH))
    line = np.zeros((B, 9), np.int32)
    for t in range(TICKS):
        ok(lib.td_simb_step(h, t, line.ctypes.data))
    m = np.zeros((B, 9), np.int64)
    ok(lib.td_simb_metrics(h, m.ctypes.data))
    ok(lib.td_simb_destroy(h))
    return time.perf_counter() - t0, int(m[:, 0].sum())


def default_path(a):
    from taxidispatcher_amd import _ffi, simulator
    tables, fleets = tables_of("small")
    cabs, off, rid, rfrom, rto, rat = simulator.pack_worlds(tables, fleets)
    packed = (cabs, off, [np.ascontiguousarray(c, np.int32) for c in (rid, rfrom, rto, rat)])
    libs = {}
    for which in (("parent", "new") if a.parent_first else ("new", "parent")):
        libs[which] = declare(ctypes.CDLL(_ffi.LIB_PATH if which == "new" else a.parent_lib))
        ok(libs[which].td_init(0))
    assert hasattr(libs["new"], "td_simb_route") and not hasattr(libs["parent"], "td_simb_route"), "--parent-lib is not the parent's library"
    settings = [(("" if w == "new" else "parent_") + tag + n, w, pn) for tag, pn in (("default", None), ("pool32", PN)) for w in ("new", "parent")
                for n in ("", "_again")]
    times, dropped = {s: [] for s, _, _ in settings}, {}
    for rep in range(a.reps + 1):      # round 0 warms every setting up
        for s, which, pn in settings[rep % len(settings):] + settings[:rep % len(settings)]:
            dt, d = run_steps(libs[which], packed, pn)
            dropped[s] = d
            if rep:
                times[s].append(dt)
    results = []
    for s, which, pn in settings:
        ts = np.asarray(times[s]) * 1e3
        row = {"setting": s, "library": which, "policy": "default" if pn is None else "(3,2), buffer 24 * 512, no td_simb_route", "B": 64, "ticks": TICKS,
               "median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "total_dropped": dropped[s]}
        print(json.dumps(row), flush=True)
        results.append(row)
    return {"what": "default path of a batch against the parent", "parent_first": a.parent_first, "reps": a.reps, "results": results}


def run_batch(td, tables, fleets, route):
    sim = td.DeviceSimulatorBatch(tables, fleets, pool_n=PN, pool_wait=WAIT, pool_loss=LOSS, pool_buffer=BUFFER_BATCH, route=route, **CITY)
    for t in range(TICKS):
        sim.tick(t)
    out = sim.m, (sim.route_metrics() if route else None)
    sim.close()
    return out


def run_loop(td, tables, fleets, route):
    sims = [td.DeviceSimulator(rows, n_cabs=n, pool_n=PN, pool_wait=WAIT, pool_loss=LOSS, pool_buffer=BUFFER_HANDLE, route=route, **CITY)
            for rows, n in zip(tables, fleets)]
    for t in range(TICKS):
        for sim in sims:
            sim.tick(t)
    out = [sim.m for sim in sims], ([sim.route_metrics() for sim in sims] if route else None)
    for sim in sims:
        sim.close()
    return out


def sums(m, rm):
    out = {k: int(sum(x[k] for x in m)) for k in ("total_dropped", "total_pickup_numb", "total_second_passengers")}
    out["max_POOL_MEM_size"] = int(max(x["max_POOL_MEM_size"] for x in m))
    if rm:
        out.update({k: int(sum(x[k] for x in rm)) for k in ("drop_numb", "ride_time", "solo_time")})
        out["max_over_loss"] = int(max(x["max_over_loss"] for x in rm))
    return out


def routed(a, td):
    results = []
    for shape in a.only.split(","):
        tables, fleets = tables_of(shape)
        row = {"shape": shape, "B": len(fleets), "cabs": fleets[0], "ticks": TICKS, "policy": "(3,2), wait %d, loss %d" % (WAIT, LOSS),
               "plan_buffer_batch": BUFFER_BATCH, "plan_buffer_handles": BUFFER_HANDLE,
               "requests_per_world": [int(min(t.shape[0] for t in tables)), int(max(t.shape[0] for t in tables))], **CITY}
        try:
            for route in (False, True):
                tag = "routed" if route else "unrouted"
                run_batch(td, tables, fleets, route), run_loop(td, tables, fleets, route)      # warm-up of both sides
                b_ms, b_lo, b_hi, mb = timed(lambda: run_batch(td, tables, fleets, route), a.reps)
                l_ms, l_lo, l_hi, ml = timed(lambda: run_loop(td, tables, fleets, route), a.reps)
                row[tag] = {"batch_ms": b_ms, "batch_min_ms": b_lo, "batch_max_ms": b_hi, "loop_ms": l_ms, "loop_min_ms": l_lo, "loop_max_ms": l_hi,
                            "loop_over_batch": l_ms / b_ms, "batch": sums(*mb), "loop": sums(*ml)}
        except td.TdError as e:
            row["refused"] = str(e)
        print(json.dumps(row), flush=True)
        results.append(row)
    return {"what": "a routed batch against a loop of routed handles", "reps": a.reps, "results": results}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--default-path", action="store_true")
    ap.add_argument("--routed", action="store_true")
    ap.add_argument("--one-run", default=None, choices=("on", "off"))
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit")
    ap.add_argument("--parent-first", action="store_true", help="load and initialise the parent library before this one")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--only", default="small,large")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if sum([a.default_path, a.routed, a.one_run is not None]) != 1 or (a.default_path and not a.parent_lib):
        ap.error("one of --default-path (with --parent-lib), --routed and --one-run")
    a.reps = a.reps or (7 if a.default_path else 5)
    import torch
    if a.default_path:
        out = default_path(a)
    else:
        import taxidispatcher_amd as td
        td.init(0)
        if a.one_run:
            tables, fleets = tables_of("small")
            run_batch(td, tables, fleets, a.one_run == "on")
            print(json.dumps({"shape": "small", "routes": a.one_run, "ticks": TICKS, "runs": 1}))
            return
        out = routed(a, td)
    out.update(device=torch.cuda.get_device_name(0), timing="host clock around synchronous calls; a run = create, tick, read the metrics, destroy")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
