"""Full 120-tick replay of the reference's simulation input with every path operation on the GPU
(dev tool; prints timing + the printMetrics block).  --world host (default): the Python world model around the GPU path;
--world device: the world in device memory too (DeviceSimulator = td_sim_step, one C-ABI call per tick);
--world device --cabs 900,1100,1300: the committed demand file once per fleet size as ONE batch of worlds
(DeviceSimulatorBatch = td_simb_step, one C-ABI call per tick for all of them), each world's metrics block printed.
--dist FILE.npy: the city as a stand-to-stand distance table (a square integer array saved with numpy.save, [from][to]) for
--world host and --world device, a batch of worlds (--cabs) included: the worlds of a batch share the one table
(td_simb_create_dist); the stands of the demand file must lie inside it.
--events FILE: the run's event log, Simulator.java's simulog.txt, written to FILE (every world: the host world records it
itself, a device world through td_sim_log / td_sim_events, drained after every tick); with --cabs a,b,c one file per world,
FILE with the world's number put before its extension (simulog.0.txt, simulog.1.txt, ...).
--pool none|greedy|optimal and --max-loss X: the pooling policy (default: greedy over every ordered pair, Simulator.java:691;
X > 0 admits the pairs that pass pool_opt_min.py's loss tests, 0 = every pair); with --cabs a,b,c either may be a list a,b,c
with one entry per world, and a single value holds for every world.  An optimal world refuses a tick with more than 2048
requests before pooling (the committed demand file has such ticks at 1300 cabs and fewer).
--dispatch lcm+opt|opt|lcm|split, --max-non-lcm N, --parts P: the dispatch policy (td_sim_dispatch / td_simb_dispatch, or
Simulator(dispatch=...) with --world host); with --cabs a,b,c each may be a list a,b,c with one entry per world, and a single
value holds for every world, e.g. --cabs 400,400,400 --dispatch lcm,opt,split --max-non-lcm 0,16,600 --parts 4.  A split world,
and in a batch an optimum-alone world, refuses a tick whose model has more than 1024 cabs or requests, which the committed
demand reaches at 1300 cabs.
--pool-n K_HI,K_LO (or K), --pool-wait W, --pool-loss L, --max-happy H: pools of up to four (Simulator(pool_n=...) with --world host,
td_sim_pooling_n with --world device) instead of the --pool policy: the cascade of td_pool_n stages K_HI .. K_LO under a pick-up
path of at most W and rides at most L percent longer.  This tool runs one such world; --cabs N with a single N then sets its fleet size (batches
of such worlds: DeviceSimulatorBatch(pool_n=[...]), tools/sim_pool_n_time.py).  A tick with more than 2047 requests before pooling, or a stage with more happy plans than H,
is refused, and the tool says which tick.
--pool-buffer N (with --pool-n): every stage runs through td_pool_n_banded with a plan buffer of N keys (td_sim_pool_buffer /
HipBackend(pool_buffer=N); at least 24 * 2047 = 49128): the same plans, and no tick is refused for its number of happy plans.
--pool-n with --world device --cabs a,b,c: every world of the batch under that cascade (td_simb_pooling_n; a world may have at most
512 requests before pooling in a tick), and --pool-buffer N then sets td_simb_pool_buffer (24 * 512 = 12288 .. 2^22): the pool
rounds run through td_pool_n_banded_batched's kernel and no tick is refused for a world's number of happy plans.
--route (with --pool-n, no --events): a pooled cab drives its plan (Simulator(route=True) / td_sim_route) instead of
being busy for the pool's cost through cheat_a_bit; after the run the four route counters and the mean ride / solo are printed.
With --world device --cabs a,b,c every world of the batch is routed (td_simb_route) and the counters are printed per world."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import taxidispatcher_amd as td
from taxidispatcher_amd import simulator


def parse(argv=None):
    """the command line and the rule of --route, before anything is read or initialised -> (parser, arguments)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", choices=("host", "device"), default="host")
    ap.add_argument("--cabs", default=None, help="comma-separated fleet sizes: one world per size, run as one batch (needs --world device)")
    ap.add_argument("--dist", default=None, metavar="FILE.npy", help="a stand-to-stand distance table (numpy.save of a square integer array)")
    ap.add_argument("--events", default=None, metavar="FILE", help="write the event log (simulog.txt) of the run to FILE")
    ap.add_argument("--pool", default="greedy", metavar="none|greedy|optimal[,...]", help="the pooling policy; a list goes with a --cabs list")
    ap.add_argument("--max-loss", default=None, metavar="X[,...]", help="the candidate rule's max_loss (0: every pair); a list goes with a --cabs list")
    ap.add_argument("--dispatch", default=None, metavar="lcm+opt|opt|lcm|split[,...]", help="the dispatch method; a list goes with a --cabs list")
    ap.add_argument("--max-non-lcm", default=None, metavar="N[,...]", help="max_non_lcm under lcm+opt; a list goes with a --cabs list")
    ap.add_argument("--parts", default="4", metavar="P[,...]", help="the split's number of stand ranges; a list goes with a --cabs list")
    ap.add_argument("--pool-n", default=None, metavar="K_HI,K_LO", help="pools of up to four: the stage sizes, largest first (one world only)")
    ap.add_argument("--pool-wait", type=int, default=0, metavar="W", help="with --pool-n: the longest pick-up path before a member boards")
    ap.add_argument("--pool-loss", type=int, default=0, metavar="L", help="with --pool-n: percent a pooled ride may exceed the direct one")
    ap.add_argument("--max-happy", type=int, default=0, metavar="H", help="with --pool-n: the most happy plans of one stage (0: the pool call's default)")
    ap.add_argument("--pool-buffer", type=int, default=0, metavar="N", help="with --pool-n: the plan buffer of td_pool_n_banded for every stage (0: off)")
    ap.add_argument("--route", action="store_true", help="with --pool-n: a pooled cab drives its plan (no --events)")
    args = ap.parse_args(argv)
    if args.route and (not args.pool_n or args.events):
        ap.error("--route goes with --pool-n and no --events (the event log of routed worlds is not built)")
    return ap, args


def main(argv=None):
    ap, args = parse(argv)
    pool_n, n_cabs_1 = {}, {}

    def print_route(m):
        print("Route counters: dropped off %d, ride time %d, solo time %d, max over loss %s" % (
            m["drop_numb"], m["ride_time"], m["solo_time"], m["max_over_loss"] if m["drop_numb"] else "none"))
        if m["drop_numb"]:
            print("Mean ride / solo: %.3f / %.3f" % (m["ride_time"] / m["drop_numb"], m["solo_time"] / m["drop_numb"]))


    if args.pool_buffer:
        if not args.pool_n:
            ap.error("--pool-buffer goes with --pool-n")
        try:
            if args.cabs and "," in args.cabs:
                simulator.pool_buffer_size(args.pool_buffer, 512, simulator.POOL_BUFFER_BATCH_MAX)
            else:
                simulator.pool_buffer_size(args.pool_buffer)
        except ValueError as e:
            ap.error("--pool-buffer %d: %s" % (args.pool_buffer, e))
    if args.pool_n:
        try:
            sizes = tuple(int(v) for v in args.pool_n.split(","))
            pool_n = dict(pool_n=simulator.pool_n_sizes(sizes[0] if len(sizes) == 1 else sizes), pool_wait=args.pool_wait, pool_loss=args.pool_loss)
            simulator.pool_n_rule(args.pool_wait, args.pool_loss)
        except ValueError as e:
            ap.error("--pool-n %s: %s" % (args.pool_n, e))
        if args.cabs and "," in args.cabs and args.world != "device":
            ap.error("--pool-n with several fleets needs --world device")
        if args.cabs and "," not in args.cabs:
            n_cabs_1, args.cabs = dict(n_cabs=int(args.cabs)), None
    if args.cabs and args.world != "device":
        ap.error("--cabs needs --world device")


    def run_120(sim):
        """sim.run(120); a --pool-n world runs tick by tick, so that a tick past the policy's limits is named when it is refused"""
        if not pool_n:
            return sim.run(120)
        for t in range(120):
            try:
                line = sim.tick(t)
            except td.TdError as e:
                sys.exit("tick %d refused: %s" % (t, e))
            if line is not None:
                sim.log.append(line)
        return sim.log


    policy = {}
    if args.dispatch or args.max_non_lcm is not None:
        n_w = len(args.cabs.split(",")) if args.cabs else 1
        lists = {"dispatch": (args.dispatch or "lcm+opt").split(","), "parts": [int(v) for v in args.parts.split(",")],
                 "max_non_lcm": [int(v) for v in args.max_non_lcm.split(",")] if args.max_non_lcm is not None else [None]}
        for what, vals in lists.items():
            if len(vals) not in (1, n_w):
                ap.error("--%s has %d entries for %d world(s)" % (what.replace("_", "-"), len(vals), n_w))
        for v in lists["dispatch"]:
            if v not in simulator.DISPATCH_MODES:
                ap.error("--dispatch %s: one of %s" % (v, ", ".join(sorted(simulator.DISPATCH_MODES))))
        if args.cabs:
            policy = {k: v * (n_w // len(v)) for k, v in lists.items()}
            if policy["max_non_lcm"][0] is None:
                policy["max_non_lcm"] = None
        else:
            policy = {k: v[0] for k, v in lists.items()}
    n_worlds = len(args.cabs.split(",")) if args.cabs else 1
    pools = args.pool.split(",")
    losses = [float(v) if float(v) > 0 else None for v in args.max_loss.split(",")] if args.max_loss else [None]
    for what, vals in (("--pool", pools), ("--max-loss", losses)):
        if len(vals) not in (1, n_worlds):
            ap.error("%s has %d entries for %d world(s)" % (what, len(vals), n_worlds))
    for v in pools:
        if v not in simulator.POOL_MODES:
            ap.error("--pool %s: one of none, greedy, optimal" % v)
    pools, losses = pools * (n_worlds // len(pools)), losses * (n_worlds // len(losses))
    dist = None
    if args.dist:
        try:
            dist = simulator.check_dist(np.load(args.dist))
        except (OSError, ValueError) as e:
            ap.error("--dist %s: %s" % (args.dist, e))
        simulator.N_STANDS = int(dist.shape[0])      # the host world reads its stand count from the module
    rows = simulator.read_demand("tests/golden/taxi_demand.txt.gz")
    if dist is not None and rows[:, 1:3].max() >= dist.shape[0]:
        ap.error("--dist %s: the demand file uses stand %d, the table has %d stands" % (args.dist, rows[:, 1:3].max(), dist.shape[0]))
    td.init(0)


    def write_events(path, records, world=None):
        with open(path, "w") as f:
            f.writelines(l + "\n" for l in simulator.format_events(records, world=world))
        print("wrote %s" % path)


    def run_logged(sim, ticks):
        """sim.run(ticks) with the event log drained after every tick -> the records, (n, 8)"""
        parts = []
        for t in range(ticks):
            out = sim.tick(t)
            if isinstance(sim, simulator.DeviceSimulatorBatch):
                for b, line in enumerate(out or []):
                    if line is not None:
                        sim.logs[b].append(line)
            elif out is not None:
                sim.log.append(out)
            parts.append(sim.events())
        if sim.events_lost:
            print("event log: %d records lost" % sim.events_lost)
        return np.concatenate(parts)


    if args.world == "device" and args.cabs:
        fleets = [int(v) for v in args.cabs.split(",")]
        sim = simulator.DeviceSimulatorBatch([rows] * len(fleets), fleets, dist=dist, events=True if args.events else None, pool=pools, max_loss=losses,
                                             **policy, **pool_n, **(dict(max_happy=args.max_happy, pool_buffer=args.pool_buffer, route=args.route) if pool_n else {}))
        t0 = time.time()
        if args.events:
            records, logs = run_logged(sim, 120), sim.logs
        elif pool_n:      # tick by tick, so that a tick past the policy's limits is named when it is refused
            logs = sim.logs
            for t in range(120):
                try:
                    out = sim.tick(t)
                except td.TdError as e:
                    sys.exit("tick %d refused: %s" % (t, e))
                for b, line in enumerate(out or []):
                    if line is not None:
                        logs[b].append(line)
        else:
            logs = sim.run(120)
        dt = time.time() - t0
        if args.events:
            stem, ext = os.path.splitext(args.events)
            for b in range(len(fleets)):
                write_events("%s.%d%s" % (stem, b, ext), records, world=b)
        print("120 ticks of %d worlds in %.2f s; worlds and path on the GPU, one td_simb_step call per tick for all worlds" % (len(fleets), dt))
        for b, n in enumerate(fleets):
            print("\n=== world %d: %d cabs, pool %s, max_loss %s, dispatch %s, max_non_lcm %d, parts %d ===" % (b, n, pools[b], losses[b], sim.dispatch[b],
                                                                                                             sim.max_non_lcms[b], sim.parts[b]))
            print("\n".join(logs[b][-2:]))
            print(sim.metrics_text(b, total_simul_time=int(dt)))
            if args.route:
                print_route(sim.route_metrics()[b])
        sys.exit(0)
    if args.world == "device":
        if pool_n:
            pool_n["max_happy"] = args.max_happy
            pool_n["pool_buffer"] = args.pool_buffer
            pool_n["route"] = args.route
        sim = simulator.DeviceSimulator(rows, dist=dist, events=True if args.events else None, pool=pools[0], max_loss=losses[0], **policy, **pool_n,
                                        **n_cabs_1)
        t0 = time.time()
        if args.events:
            records, log = run_logged(sim, 120), sim.log
        else:
            log = run_120(sim)
        dt = time.time() - t0
        if args.events:
            write_events(args.events, records)
        print("120 ticks in %.2f s (reference: 2603 s, README.md:45); world and path on the GPU, one td_sim_step call per tick" % dt)
        print("\n".join(log[-3:]))
        print(sim.metrics_text(total_simul_time=int(dt)))
        if args.route:
            print_route(sim.route_metrics())
        sys.exit(0)
    if pool_n:
        pool_n["route"] = args.route
    sim = simulator.Simulator(rows, backend=simulator.HipBackend(dist, max_happy=args.max_happy, pool_buffer=args.pool_buffer) if pool_n else None, dist=dist, events=bool(args.events), pool=pools[0],
                              max_loss=losses[0], **policy, **pool_n, **({"n_cabs": n_cabs_1["n_cabs"]} if n_cabs_1 else {}))
    t0 = time.time()
    per = {"pool": 0.0, "cost": 0.0, "lcm": 0.0, "solve": 0.0}
    be = sim.be
    def timed(name, fn):
        def w(*a, **k):
            t = time.time(); r = fn(*a, **k); per[name] += time.time() - t; return r
        return w
    be.find_pool = timed("pool", be.find_pool); be.calculate_cost = timed("cost", be.calculate_cost)
    be.lcm = timed("lcm", be.lcm); be.solve = timed("solve", be.solve)
    log = run_120(sim)
    dt = time.time() - t0
    if args.events:
        write_events(args.events, sim.events)
    print("120 ticks in %.2f s (reference: 2603 s, README.md:45); path time on GPU incl. PCIe: %s" % (dt, {k: round(v, 3) for k, v in per.items()}))
    print("\n".join(log[-3:]))
    print(sim.metrics_text(total_simul_time=int(dt)))

    if args.route:
        print_route(sim.route_m)


if __name__ == "__main__":
    main()
