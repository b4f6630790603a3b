"""Times pools of up to four in the simulator worlds (td_sim_pooling_n), and writes the table for the
reference README's claim "with 4 passengers in a pool much more is feasible".

    python tools/sim_pool_n_time.py [--out profiles/sim_pool_n/sim_pool_n_time.json] [--seeds 16] [--reps 3]
    python tools/sim_pool_n_time.py --claim [--out profiles/sim_pool_n/claim.json] [--budget 90] [--max-happy 0]

1. the sweep: 64 worlds of 150 cabs on 50 stands, 40 ticks: --seeds demand files x the policies greedy pairs, (2,2), (3,2),
   (4,2) under WAIT / LOSS below.  Three routes: ONE DeviceSimulatorBatch over all of them (td_simb_step per tick, a policy per
   world), a loop of DeviceSimulator handles (td_sim_step per tick and world), and a host Simulator per world on HipBackend
   (find_pool_n and the path calls per tick).  The time of each route over all worlds and the ratios, and per policy the
   dropped customers, second passengers and pick-ups of each route (they need not be equal: td_tick_batched, td_tick and the
   step-by-step calls may break ties between equal optima differently).
2. --claim: the committed 120-tick demand, 1300 cabs and 600 cabs, one DeviceSimulator per policy: the reference's greedy
   pairs, then (2,2), (3,2), (4,2) under CLAIM_WAIT / CLAIM_LOSS.  Dropped, picked up, mean pick-up time, second passengers and
   the tick-loop time; a refused tick (more than 2047 requests before pooling, max_happy, a cost above 16383) ends that
   policy's run and is reported with its tick and the library's message, and so does a run that passes --budget seconds.
   Nothing is tuned until it passes.  --max-happy is the capacity handed to td_sim_pooling_n (0: the pool call's default,
   65536 plans per stage up to 512 requests; 4194304 is the most the library takes) and is written into the result.
Host clock around synchronous calls; the sweep warms every side up once and takes the median of --reps runs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sim_batch_time import BIG, gen_demand, timed

POLICIES = [None, (2, 2), (3, 2), (4, 2)]      # None: the reference's greedy pairs
CITY = dict(n_stands=50, drop_time=10, max_non_lcm=600, big_cost=BIG)
TICKS, CABS = 40, 150
WAIT, LOSS = 1, 50                  # the sweep: a pick-up path of at most one stand, rides at most 50 percent longer
CLAIM_WAIT, CLAIM_LOSS = 0, 25      # the claim: members board at one stand, rides at most 25 percent longer
KEYS = ("total_dropped", "total_pickup_numb", "total_pickup_time", "total_second_passengers", "max_POOL_size", "max_POOL_MEM_size")


def name_of(pn):
    return "greedy pairs" if pn is None else "pool_n (%d,%d)" % pn


def policy_kw(pn, wait, loss, max_happy=0):
    return {} if pn is None else dict(pool_n=pn, pool_wait=wait, pool_loss=loss, max_happy=max_happy)


def run_batch(td, tables):
    """every policy x every demand file in one handle; world order: policy-major"""
    rows = [r for _ in POLICIES for r in tables]
    pns = [pn for pn in POLICIES for _ in tables]
    sim = td.DeviceSimulatorBatch(rows, [CABS] * len(rows), pool_n=pns, pool_wait=WAIT, pool_loss=LOSS, **CITY)
    for t in range(TICKS):
        sim.tick(t)
    m = sim.m
    sim.close()
    return m


def run_device(td, tables):
    out = []
    for pn in POLICIES:
        for rows in tables:
            sim = td.DeviceSimulator(rows, n_cabs=CABS, **CITY, **policy_kw(pn, WAIT, LOSS))
            sim.run(TICKS)
            out.append(sim.m)
            sim.close()
    return out


def run_host(tables):
    """one host Simulator per world (the module's constants are this city's: 50 stands, DROP_TIME 10, MAX_NON_LCM 600)"""
    from taxidispatcher_amd import simulator
    out = []
    for pn in POLICIES:
        for rows in tables:
            kw = policy_kw(pn, WAIT, LOSS)
            kw.pop("max_happy", None)
            sim = simulator.Simulator(rows, simulator.HipBackend(), n_cabs=CABS, **kw)
            sim.run(TICKS)
            out.append(sim.m)
    return out


def sums(ms):
    return {k: int(max(m[k] for m in ms)) if k.startswith("max") else int(sum(m[k] for m in ms)) for k in KEYS}


def sweep(td, seeds, reps):
    tables = [gen_demand(CITY["n_stands"], 46, TICKS, 4, 10, 100 + s) for s in range(seeds)]
    out = {"seeds": seeds, "worlds": seeds * len(POLICIES), "cabs": CABS, "ticks": TICKS, "wait": WAIT, "loss": LOSS, **CITY}
    run_batch(td, tables[:1]), run_device(td, tables[:1]), run_host(tables[:1])
    b_ms, b_lo, b_hi, mb = timed(lambda: run_batch(td, tables), reps)
    d_ms, d_lo, d_hi, md = timed(lambda: run_device(td, tables), reps)
    h_ms, h_lo, h_hi, mh = timed(lambda: run_host(tables), max(1, reps // 3))
    out.update(batch_ms=b_ms, batch_min_ms=b_lo, batch_max_ms=b_hi, handles_ms=d_ms, handles_min_ms=d_lo, handles_max_ms=d_hi, host_ms=h_ms,
               host_min_ms=h_lo, host_max_ms=h_hi, handles_over_batch=d_ms / b_ms, host_over_batch=h_ms / b_ms, host_over_handles=h_ms / d_ms)
    out["policies"] = [{"policy": name_of(pn), "batch": sums(mb[i * seeds:(i + 1) * seeds]), "handles": sums(md[i * seeds:(i + 1) * seeds]),
                        "host": sums(mh[i * seeds:(i + 1) * seeds])} for i, pn in enumerate(POLICIES)]
    print(json.dumps(out), flush=True)
    return out


def claim(td, budget, max_happy):
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    out = {"ticks": 120, "wait": CLAIM_WAIT, "loss": CLAIM_LOSS, "requests": int(rows.shape[0]), "max_happy": max_happy, "runs": []}
    for cabs in (1300, 600):
        for pn in POLICIES:
            sim = td.DeviceSimulator(rows, n_cabs=cabs, **policy_kw(pn, CLAIM_WAIT, CLAIM_LOSS, max_happy))
            rec = {"cabs": cabs, "policy": name_of(pn), "ended": "all 120 ticks"}
            t0 = time.perf_counter()
            done = 0
            for t in range(120):
                try:
                    sim.tick(t)
                except td.TdError as e:
                    rec["ended"] = "tick %d refused: %s" % (t, e)
                    break
                done = t + 1
                if time.perf_counter() - t0 > budget:
                    rec["ended"] = "stopped after tick %d: the run passed %d s" % (t, budget)
                    break
            rec["tick_loop_s"] = time.perf_counter() - t0
            m = sim.m
            rec.update(ticks_done=done, dropped=m["total_dropped"], picked_up=m["total_pickup_numb"], second_passengers=m["total_second_passengers"],
                       mean_pickup_time=(m["total_pickup_time"] / m["total_pickup_numb"] if m["total_pickup_numb"] else None),
                       max_pools_in_a_tick=m["max_POOL_size"], max_happy_plans_in_a_tick=m["max_POOL_MEM_size"], max_model_size=m["max_model_size"])
            sim.close()
            out["runs"].append(rec)
            print(json.dumps(rec), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--claim", action="store_true")
    ap.add_argument("--max-happy", type=int, default=0, help="--claim: the most happy plans of one stage (0: the pool call's default)")
    ap.add_argument("--budget", type=int, default=90, help="--claim: seconds after which a policy's run is stopped and reported as such")
    args = ap.parse_args()
    import taxidispatcher_amd as td
    td.init(0)
    out = claim(td, args.budget, args.max_happy) if args.claim else sweep(td, args.seeds, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
