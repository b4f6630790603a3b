"""Times the route model of the device world (td_sim_route) and restates section 3.15's claim with routes on.

    python tools/sim_route_time.py --default-path --parent-lib PATH [--parent-first] [--reps 7] [--out FILE.json]
    python tools/sim_route_time.py --claim [--reps 3] [--only 600:4,2:on] [--budget 300] [--out FILE.json]

--default-path: the committed 120-tick demand, 1300 cabs, through td_sim_step on a default handle and on a (3,2) handle (wait 0,
  loss 25, plan buffer 2^20) that never calls td_sim_route, on this library and on one built from the parent commit, both
  loaded into this process (--parent-first: the parent is loaded and initialised first; the order is part of the experiment).
  Every setting twice under two names, so that each library's spread against itself is in the table.  Settings alternate
  within the process, setting after setting, --reps times after one warm-up round; every round begins one setting later.
  Everything goes through the raw C ABI, so that two libraries can be driven side by side.
--claim: the rows of section 3.15's table, 1300 and 600 cabs, (3,2) and (4,2) with the plan buffer, routes off and on, one
  DeviceSimulator per run: dropped, picked up, second passengers, the four route counters, mean ride / solo and the tick-loop
  time (the 1300-cab rows --reps times: median, smallest, largest; the 600-cab rows once).  --only CABS:K_HI,K_LO:on|off runs that
  one row once; a run that passes --budget seconds stops after the tick it is in and is reported with the ticks it did.  Every row
  names its slowest tick, that tick's time and its log line (the demand and supply it began with).
Host clock around synchronous calls: the tick loop ends in a device synchronise."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, I, I32, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64
WAIT, LOSS, BUFFER = 0, 25, 1 << 20      # section 3.15's claim rule, section 3.16's smaller buffer


def declare(lib):
    lib.td_init.argtypes = [I]
    lib.td_sim_create.argtypes = [I, I, I, I, I32, I, V, V, V, V, V]
    lib.td_sim_step.argtypes = [V, I, V]
    lib.td_sim_destroy.argtypes = [V]
    lib.td_sim_pooling_n.argtypes = [V, I, I, I, I, I64]
    lib.td_sim_pool_buffer.argtypes = [V, I64]
    lib.td_sim_metrics.argtypes = [V, V]
    return lib


def ok(rc):
    if rc != 0:
        raise RuntimeError("C ABI call failed: %d" % rc)


def run_steps(lib, rows, pn):
    """a handle that never calls td_sim_route: create, 120 x td_sim_step, destroy -> (seconds of the tick loop, total_dropped)"""
    cols = [np.ascontiguousarray(rows[:, k].astype(np.int32)) for k in (0, 1, 2, 4)]
    h = V()
    ok(lib.td_sim_create(1300, 50, 10, 600, 250000, rows.shape[0], *[c.ctypes.data for c in cols], ctypes.byref(h)))
    if pn:
        ok(lib.td_sim_pooling_n(h, pn[0], pn[1], WAIT, LOSS, 0))
        ok(lib.td_sim_pool_buffer(h, BUFFER))
    line = np.zeros(9, np.int32)
    t0 = time.perf_counter()
    for t in range(120):
        ok(lib.td_sim_step(h, t, line.ctypes.data))
    dt = time.perf_counter() - t0
    m = np.zeros(9, np.int64)
    ok(lib.td_sim_metrics(h, m.ctypes.data))
    ok(lib.td_sim_destroy(h))
    return dt, int(m[0])


def default_path(a, rows):
    from taxidispatcher_amd import _ffi
    libs = {}
    for which in (("parent", "new") if a.parent_first else ("new", "parent")):
        libs[which] = declare(ctypes.CDLL(_ffi.LIB_PATH if which == "new" else a.parent_lib))
        ok(libs[which].td_init(0))
    assert hasattr(libs["new"], "td_sim_route") and not hasattr(libs["parent"], "td_sim_route"), "--parent-lib is not the parent's library"
    settings = [(("" if w == "new" else "parent_") + tag + n, w, pn) for tag, pn in (("default", None), ("pool32", (3, 2))) for w in ("new", "parent")
                for n in ("", "_again")]
    times, dropped = {s: [] for s, _, _ in settings}, {}
    for rep in range(a.reps + 1):      # round 0 warms every setting up
        for s, which, pn in settings[rep % len(settings):] + settings[:rep % len(settings)]:
            dt, d = run_steps(libs[which], rows, pn)
            dropped[s] = d
            if rep:
                times[s].append(dt)
    results = []
    for s, which, pn in settings:
        ts = np.asarray(times[s]) * 1e3
        row = {"setting": s, "library": which, "policy": "default" if pn is None else "(3,2), buffer 2^20, no td_sim_route", "ticks": 120,
               "median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "total_dropped": dropped[s]}
        print(json.dumps(row), flush=True)
        results.append(row)
    return {"what": "default path against the parent", "parent_first": a.parent_first, "reps": a.reps, "results": results}


def claim(a, rows):
    import taxidispatcher_amd as td
    td.init(0)
    runs = []
    only = None
    if a.only:
        c, k, r = a.only.split(":")
        only = (int(c), tuple(int(v) for v in k.split(",")), r == "on")
    for cabs in (1300, 600):
        for pn in ((3, 2), (4, 2)):
            for route in (False, True):
                if only and only != (cabs, pn, route):
                    continue
                ts, done, slow = [], 120, (0.0, -1, None)
                for rep in range(a.reps if cabs == 1300 and not only else 1):
                    sim = td.DeviceSimulator(rows, n_cabs=cabs, pool_n=pn, pool_wait=WAIT, pool_loss=LOSS, pool_buffer=BUFFER, route=route)
                    t0 = time.perf_counter()
                    for t in range(120):
                        t1 = time.perf_counter()
                        line = sim.tick(t)
                        slow = max(slow, (time.perf_counter() - t1, t, line))
                        if time.perf_counter() - t0 > a.budget:
                            done = min(done, t + 1)
                            break
                    ts.append(time.perf_counter() - t0)
                    m, rm = sim.m, (sim.route_metrics() if route else None)
                    sim.close()
                rec = {"cabs": cabs, "policy": "(%d,%d)" % pn, "plan_buffer": BUFFER, "routes": route, "dropped": m["total_dropped"],
                       "picked_up": m["total_pickup_numb"], "second_passengers": m["total_second_passengers"], "max_happy_plans_in_a_tick": m["max_POOL_MEM_size"], "max_pools_in_a_tick": m["max_POOL_size"],
                       "tick_loop_s_median": float(np.median(ts)),
                       "tick_loop_s_min": float(min(ts)), "tick_loop_s_max": float(max(ts)), "runs": len(ts), "ticks_done": done,
                       "slowest_tick": slow[1], "slowest_tick_s": slow[0], "slowest_tick_line": slow[2]}
                if route:
                    rec.update(rm, mean_ride=rm["ride_time"] / max(rm["drop_numb"], 1), mean_solo=rm["solo_time"] / max(rm["drop_numb"], 1))
                print(json.dumps(rec), flush=True)
                runs.append(rec)
    return {"what": "section 3.15's rows with routes off and on", "wait": WAIT, "loss": LOSS, "reps_at_1300": a.reps, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--default-path", action="store_true")
    ap.add_argument("--claim", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="a library built from the parent commit")
    ap.add_argument("--parent-first", action="store_true", help="load and initialise the parent library before this one")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--only", default=None, metavar="CABS:K_HI,K_LO:on|off", help="--claim: this one row, once")
    ap.add_argument("--budget", type=float, default=300.0, help="--claim: seconds after which a run stops at the end of its tick")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.default_path == a.claim or (a.default_path and not a.parent_lib):
        ap.error("one of --default-path (with --parent-lib) and --claim")
    a.reps = a.reps or (7 if a.default_path else 3)
    import torch
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    out = default_path(a, rows) if a.default_path else claim(a, rows)
    out.update(device=torch.cuda.get_device_name(0), timing="host clock around the tick loop of synchronous calls")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
