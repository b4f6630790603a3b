"""Times the dispatch policies of the simulator worlds (td_simb_dispatch / td_sim_dispatch).

    python tools/sim_dispatch_policy_time.py [--out profiles/sim_dispatch_policy/sim_dispatch_policy_time.json] [--reps 3]
    python tools/sim_dispatch_policy_time.py --one-run [--default]   (one batched run and nothing else: for a kernel trace;
                                                                      --default: the same worlds without td_simb_dispatch)
    python tools/sim_dispatch_policy_time.py --only committed [--cabs 1300] [--out ...]

1. worlds: 64 worlds of 150 cabs on 50 stands, 40 ticks, 16 demand seeds x the four methods (lcm+opt 16, opt, lcm, split 4) in
   ONE DeviceSimulatorBatch, against a loop of DeviceSimulator handles with the same policies, and against one host Simulator
   per world (HipBackend behind simulator.Simulator(dispatch=...)).  Per method: dropped customers, picked up, pick-up time of
   the batch and of the host worlds (they need not be equal: equal optima may be broken differently by the calls).
2. committed: one DeviceSimulator per policy over --ticks ticks of tests/golden/taxi_demand.txt.gz with Simulator.java's
   constants: the wall time of the tick loop and what the customers got.  A split world refuses a tick whose model has more
   than 1024 cabs or requests; such a policy is reported with the tick and the message instead of figures.
Host clock around synchronous calls; every side is warmed up once, then the median of --reps runs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sim_batch_time import BIG, gen_demand, timed

POLICIES = [("lcm+opt", 16, 4), ("opt", 16, 4), ("lcm", 16, 4), ("split", 16, 4)]
CITY = dict(n_stands=50, drop_time=10, big_cost=BIG)
TICKS, CABS = 40, 150
KEYS = ("total_dropped", "total_pickup_numb", "total_pickup_time", "total_LCM_used", "max_solver_size")


def worlds(seeds):
    """-> (tables, policies): the four methods on each of `seeds` request files, method-minor"""
    tables, pols = [], []
    for s in range(seeds):
        rows = gen_demand(CITY["n_stands"], 46, TICKS, 4, 10, 100 + s)
        for p in POLICIES:
            tables.append(rows)
            pols.append(p)
    return tables, pols


def run_batched(td, tables, pols, default=False):
    kw = dict(max_non_lcm=16) if default else dict(dispatch=[p[0] for p in pols], max_non_lcm=[p[1] for p in pols], parts=[p[2] for p in pols])
    sim = td.DeviceSimulatorBatch(tables, [CABS] * len(tables), **kw, **CITY)
    sim.run(TICKS)
    m = sim.m
    sim.close()
    return m


def run_handles(td, tables, pols):
    out = []
    for rows, p in zip(tables, pols):
        sim = td.DeviceSimulator(rows, n_cabs=CABS, dispatch=p[0], max_non_lcm=p[1], parts=p[2], **CITY)
        sim.run(TICKS)
        out.append(sim.m)
        sim.close()
    return out


def run_host(tables, pols):
    """one host Simulator per world (the module's constants are this city's: 50 stands, DROP_TIME 10)"""
    from taxidispatcher_amd import simulator
    out = []
    for rows, p in zip(tables, pols):
        sim = simulator.Simulator(rows, simulator.HipBackend(), n_cabs=CABS, dispatch=p[0], max_non_lcm=p[1], parts=p[2])
        sim.run(TICKS)
        out.append(sim.m)
    return out


def sums(ms):
    return {k: int(max(m[k] for m in ms)) if k.startswith("max") else int(sum(m[k] for m in ms)) for k in KEYS}


def time_worlds(td, seeds, reps):
    tables, pols = worlds(seeds)
    run_batched(td, tables, pols)
    run_handles(td, tables[:4], pols[:4])
    run_host(tables[:4], pols[:4])
    row = {"B": len(tables), "seeds": seeds, "cabs": CABS, "ticks": TICKS, **CITY}
    row["batched_ms"], row["batched_min_ms"], row["batched_max_ms"], mb = timed(lambda: run_batched(td, tables, pols), reps)
    row["handles_ms"], row["handles_min_ms"], row["handles_max_ms"], mh = timed(lambda: run_handles(td, tables, pols), reps)
    row["host_ms"], row["host_min_ms"], row["host_max_ms"], mo = timed(lambda: run_host(tables, pols), reps)
    row["handles_over_batched"] = row["handles_ms"] / row["batched_ms"]
    row["host_over_batched"] = row["host_ms"] / row["batched_ms"]
    row["policies"] = [{"dispatch": p[0], "max_non_lcm": p[1], "parts": p[2], "batch": sums(mb[q::4]), "handles": sums(mh[q::4]),
                        "host": sums(mo[q::4])} for q, p in enumerate(POLICIES)]
    return row


def committed(td, ticks, cabs, specs):
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    results = []
    for spec in specs.split(","):
        method, _, arg = spec.partition(":")
        kw = dict(dispatch=method)
        if method == "split":
            kw["parts"] = int(arg or 4)
        elif arg:
            kw["max_non_lcm"] = int(arg)
        row = {"policy": spec, "cabs": cabs, "ticks": ticks}
        for rep in range(2):   # the first run warms the library up, the second is timed
            dev = td.DeviceSimulator(rows, n_cabs=cabs, **kw)
            t0 = time.perf_counter()
            try:
                for t in range(ticks):
                    dev.tick(t)
            except td.TdError as e:
                row.update(refused_at_tick=t, message=str(e))
                dev.close()
                break
            row["wall_ms"] = (time.perf_counter() - t0) * 1e3
            m = dev.m
            dev.close()
        else:
            row.update(dropped=m["total_dropped"], picked_up=m["total_pickup_numb"], pickup_time=m["total_pickup_time"],
                       mean_pickup_time=(m["total_pickup_time"] / m["total_pickup_numb"] if m["total_pickup_numb"] else None),
                       second_passengers=m["total_second_passengers"], lcm_ticks=m["total_LCM_used"], max_model=m["max_model_size"],
                       max_solver=m["max_solver_size"])
        print(json.dumps(row), flush=True)
        results.append(row)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_dispatch_policy", "sim_dispatch_policy_time.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=16, help="request files; the batch holds 4 worlds per file")
    ap.add_argument("--one-run", action="store_true", help="run the batch once and exit")
    ap.add_argument("--default", action="store_true", help="with --one-run: the worlds without a dispatch policy")
    ap.add_argument("--only", default="worlds,committed")
    ap.add_argument("--ticks", type=int, default=120)
    ap.add_argument("--cabs", type=int, default=1300)
    ap.add_argument("--policies", default="lcm+opt:600,lcm+opt:16,opt,lcm,split:4")
    a = ap.parse_args()
    import torch
    import taxidispatcher_amd as td
    td.init(0)
    if a.one_run:
        tables, pols = worlds(a.seeds)
        m = run_batched(td, tables, pols, default=a.default)
        print(json.dumps({"B": len(tables), "default": a.default, **sums(m)}))
        return
    only = a.only.split(",")
    info = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": a.reps,
            "timing": "host clock around synchronous calls; every side warmed up once, median of reps (committed: second of two runs)"}
    if "worlds" in only:
        info["worlds"] = time_worlds(td, a.seeds, a.reps)
        print(json.dumps(info["worlds"]), flush=True)
    if "committed" in only:
        info["committed"] = committed(td, a.ticks, a.cabs, a.policies)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(info, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
