"""Measurements of td_pool_n_banded and td_sim_pool_buffer on one MI355X (profiles/pool_n_banded/).

    python tools/pool_band_time.py claim --cabs 1300 --pool-n 4,2 --buffer 4194304 [--budget 150] [--save-stage F.npy] [--out F.json]
    python tools/pool_band_time.py price [--stage F.npy] [--out F.json]
    python tools/pool_band_time.py default [--tree DIR] [--out F.json]

claim    one row of the table of DESIGN.md 3.15 with a plan buffer: the committed 120-tick demand, wait 0 / loss 25, first as a
         DeviceSimulator(pool_buffer=) (the tick-loop time, the metrics), then as the host Simulator on a HipBackend that keeps
         td_pool_n_banded's stats of every stage (bands per tick; its metrics must equal the device world's).  A run that passes
         --budget seconds is stopped after a tick and reported as stopped.  --save-stage keeps the request list of the stage
         with the most happy plans that td_pool_n still takes (<= 2^22), for `price`.
price    td_pool_n_banded against td_pool_n on inputs both accept: 600 requests at k = 4 (test_gpu_pool.py's shape) and the
         saved stage; the default buffer (one band: the extra counting pass) and a buffer of about a quarter of the happy
         plans.  Median of 5 warm calls each, host clock, host arrays.
default  what a caller who never asks for a buffer runs: td_pool_n on the 600-request input and the 120-tick loop of a default
         DeviceSimulator, in a fresh process per figure set; --tree times another checkout's package (the parent's)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAIT, LOSS = 0, 25      # the claim's rule (tools/sim_pool_n_time.py)


def random_demand(rng, n, max_wait, losses, stands=50):
    frm = rng.integers(0, stands, n)
    to = np.clip(frm + rng.integers(1, 9, n) * rng.choice([-1, 1], n), 0, stands - 1)
    to = np.where(to == frm, np.where(frm > 0, frm - 1, 1), to)
    return np.stack([np.arange(n), frm, to, rng.integers(0, max_wait + 1, n), rng.choice(losses, n)], 1)


def demand_600():
    """the 600-request input of test_pool_n_random_vs_oracle[4]"""
    rng = np.random.default_rng(44)
    for n, mw, losses in ((4, 9, [90]), (17, 5, [10, 50]), (150, 3, [1, 30])):
        random_demand(rng, n, mw, losses)
    return random_demand(rng, 600, 0, [1, 5, 20])


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def metrics(m):
    return dict(dropped=int(m["total_dropped"]), picked_up=int(m["total_pickup_numb"]), second_passengers=int(m["total_second_passengers"]),
                mean_pickup_time=(m["total_pickup_time"] / m["total_pickup_numb"] if m["total_pickup_numb"] else None),
                max_pools_in_a_tick=int(m["max_POOL_size"]), max_happy_plans_in_a_tick=int(m["max_POOL_MEM_size"]))


def run_ticks(td, sim, budget, after_tick=None):
    """-> (ticks done, how it ended, seconds)"""
    t0 = time.perf_counter()
    done, ended = 0, "all 120 ticks"
    for t in range(120):
        try:
            line = sim.tick(t)
        except td.TdError as e:
            ended = "tick %d refused: %s" % (t, e)
            break
        done = t + 1
        if after_tick:
            after_tick(t, line)
        if time.perf_counter() - t0 > budget:
            ended = "stopped after tick %d: the run passed %d s" % (t, budget)
            break
    return done, ended, time.perf_counter() - t0


def claim(td, args):
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    pn = tuple(int(v) for v in args.pool_n.split(","))
    out = dict(cabs=args.cabs, policy="pool_n (%d,%d)" % pn, wait=WAIT, loss=LOSS, pool_buffer=args.buffer, budget_s=args.budget)
    dev = td.DeviceSimulator(rows, n_cabs=args.cabs, pool_n=pn, pool_wait=WAIT, pool_loss=LOSS, pool_buffer=args.buffer)
    done, ended, secs = run_ticks(td, dev, args.budget)
    out["device"] = dict(ended=ended, ticks_done=done, tick_loop_s=secs, **metrics(dev.m))
    dev.close()
    print(json.dumps(out["device"]), flush=True)

    class Recording(simulator.HipBackend):
        """td_pool_n_banded's stats of every stage, and the largest stage td_pool_n would still take"""
        stages, best = [], (0, None)

        def find_pool_n(self, k, frm, to, wait, loss):
            frm, to, wait, loss = (np.asarray(a, np.int32).reshape(-1) for a in (frm, to, wait, loss))
            rows_k = np.stack([np.arange(frm.size, dtype=np.int32), frm, to, wait, loss], axis=1)
            recs, nh, stats = self.d.find_pool_n_banded(k, rows_k, self.dist, plan_buffer=self.pool_buffer)
            Recording.stages.append((k, int(frm.size), nh) + stats)
            if Recording.best[0] < nh <= 1 << 22:
                Recording.best = (nh, np.concatenate([[[k, 0, 0, 0, 0]], rows_k]))
            return recs, nh

    host = simulator.Simulator(rows, Recording(pool_buffer=args.buffer), n_cabs=args.cabs, pool_n=pn, pool_wait=WAIT, pool_loss=LOSS)
    per_tick = []

    def after(t, line):
        per_tick.append(dict(t=t, stages=Recording.stages[:]))
        del Recording.stages[:]
    h_done, h_ended, h_secs = run_ticks(td, host, args.budget, after)
    bands = [sum(s[3] for s in r["stages"]) for r in per_tick if r["stages"]]
    passes = [sum(s[4] for s in r["stages"]) for r in per_tick if r["stages"]]
    out["host"] = dict(ended=h_ended, ticks_done=h_done, tick_loop_s=h_secs, **metrics(host.m),
                       equals_device=(h_done == done and metrics(host.m) == {k: out["device"][k] for k in metrics(host.m)}),
                       ticks_with_a_stage=len(bands), bands_per_tick_median=statistics.median(bands) if bands else None,
                       bands_per_tick_max=max(bands) if bands else None, passes_per_tick_median=statistics.median(passes) if passes else None,
                       passes_per_tick_max=max(passes) if passes else None,
                       deepest_level=max((s[5] for r in per_tick for s in r["stages"]), default=None),
                       most_keys_in_a_band=max((s[6] for r in per_tick for s in r["stages"]), default=None),
                       largest_stage=max(((s[2], s[0], s[1], r["t"]) for r in per_tick for s in r["stages"]), default=None))
    print(json.dumps(out["host"]), flush=True)
    if args.save_stage and Recording.best[1] is not None:
        np.save(args.save_stage, Recording.best[1])
        out["saved_stage"] = dict(happy=Recording.best[0], k=int(Recording.best[1][0, 0]), n=int(Recording.best[1].shape[0] - 1))
    return out


def price(td, args):
    inputs = [("600 requests, k = 4", 4, demand_600())]
    if args.stage:
        blob = np.load(args.stage)
        inputs.append(("the world's largest accepted stage", int(blob[0, 0]), blob[1:]))
    out = []
    for name, k, d in inputs:
        want, nh = td.find_pool_n(k, d, max_happy=1 << 22)
        base = median_ms(lambda: td.find_pool_n(k, d, max_happy=1 << 22))
        rec = dict(input=name, k=k, n=int(len(d)), happy=nh, pools=int(len(want)), td_pool_n_ms=base)
        for label, room in (("default buffer", 0), ("a quarter of the happy plans", max(24 * len(d), nh // 4 + 1))):
            got, happy, stats = td.find_pool_n_banded(k, d, plan_buffer=room)
            assert got.tolist() == want.tolist() and happy == nh
            ms = median_ms(lambda: td.find_pool_n_banded(k, d, plan_buffer=room))
            rec[label] = dict(plan_buffer=room, stats=stats, ms=ms, over_td_pool_n=ms[0] / base[0])
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return out


def default(td, args):
    from taxidispatcher_amd import simulator
    d = demand_600()
    out = dict(tree=os.path.abspath(args.tree or ROOT))
    out["td_pool_n_600_k4_ms"] = median_ms(lambda: td.find_pool_n(4, d), 9)
    rows = simulator.read_demand(os.path.join(ROOT, "tests", "golden", "taxi_demand.txt.gz"))
    loops = []
    for _ in range(3):
        sim = td.DeviceSimulator(rows)
        t0 = time.perf_counter()
        sim.run(120)
        loops.append(time.perf_counter() - t0)
        dropped = int(sim.m["total_dropped"])
        sim.close()
    out["td_sim_120_ticks_s"] = loops
    out["dropped"] = dropped
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("claim", "price", "default"))
    ap.add_argument("--cabs", type=int, default=1300)
    ap.add_argument("--pool-n", default="4,2")
    ap.add_argument("--buffer", type=int, default=1 << 22)
    ap.add_argument("--budget", type=int, default=150)
    ap.add_argument("--save-stage", default=None)
    ap.add_argument("--stage", default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree or ROOT))
    import taxidispatcher_amd as td
    td.init(0)
    out = dict(claim=claim, price=price, default=default)[args.mode](td, args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
