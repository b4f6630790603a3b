"""Tick-loop harness around the assignment path — the caller side of BASELINE config 5.

A from-scratch host harness with the semantics of `Simulator.java` (file:line citations below)
so that the committed run log `simulations/simulog_solv.txt` can be replayed: per tick it builds
the cost matrix, cuts the model with LCM when it is larger than MAX_NON_LCM, applies the pairs,
re-builds the remainder and solves it to optimality.  The three path operations go through a
backend object; the product backend is `HipBackend` (the MI355X library), which also runs the
pool-of-two pre-reduce on the GPU (td_pool2, SURVEY f-3).  World bookkeeping (cab movement,
request intake/drop) is plain host code — it is not on the hot path and is
kept only as far as the golden trace needs it; the numpy pool finder below is the restatement
the oracle-backed replay uses.

Bug-compatible details that the trace depends on are listed in SURVEY.md Appendix A.
"""
import gzip

import numpy as np

HOURS = 2
N_STANDS = 50          # Simulator.java:110
DROP_TIME = 10         # :111
MAX_NON_LCM = 600      # :112
N_CABS = 1300          # :113
BIG_COST = 250000      # :114
CLNT_A_ENDS, CLNT_B_ENDS = 0, 1   # :97-98


# the event log, Simulator.java's simulog.txt: a record is (t, world, kind, method, customer id, cab, aux, 0); a word the kind
# does not use is -1 (method: 0).  The kinds, with the Java line that writes them (include/taxidispatcher_amd.h, TD_EV_*)
(EV_PICKED_UP, EV_CAB_FREE, EV_DROPPED, EV_TEMP_DEMAND, EV_TEMP_DEMAND_ID, EV_POOL, EV_POOL_PAIR, EV_ASSIGNED_PICKED, EV_HEADING,
 EV_ASSIGNED_LCM, EV_POOLED_SECOND) = range(1, 12)
EV_KINDS = tuple(range(1, 12))
EV_LCM, EV_OPT = 1, 2                    # the method word
EV_METHOD = {EV_LCM: "LCM", EV_OPT: "OPT"}

MAX_DIST_STANDS = 4096       # a distance table has at most this many stands (td_sim_create_dist)
MAX_DIST = 0x1fffffff        # and no larger entry: three of them stay below td_pool2's INT_MAX diagonal marker


def check_dist(dist, n_stands=None):
    """A stand-to-stand distance table as the simulator worlds accept it -> a C-contiguous int32 copy.  Square, integers,
    1 .. MAX_DIST_STANDS stands (n_stands, when given), diagonal 0, every other entry in 1 .. MAX_DIST (a zero between two
    stands would start a cab that never arrives: arrival is tested on a later tick).  Symmetry and the triangle
    inequality are not required; dist[a][b] is the way FROM a TO b.  Raises ValueError."""
    d = np.asarray(dist)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("distance table: shape %r is not square" % (d.shape,))
    n = int(d.shape[0])
    if n_stands is not None and n != int(n_stands):
        raise ValueError("distance table: %d x %d for %d stands" % (n, n, int(n_stands)))
    if not 1 <= n <= MAX_DIST_STANDS:
        raise ValueError("distance table: %d stands, outside 1 .. %d" % (n, MAX_DIST_STANDS))
    if d.dtype.kind not in "iu":
        if d.dtype.kind != "f" or not np.array_equal(np.rint(d), d):
            raise ValueError("distance table: entries must be integers")
        d = np.rint(d)
    d = d.astype(np.int64)
    if np.diagonal(d).any():
        raise ValueError("distance table: the diagonal must be 0")
    off = d[~np.eye(n, dtype=bool)]
    if off.size and (off.min() < 1 or off.max() > MAX_DIST):
        raise ValueError("distance table: entries between different stands must lie in 1 .. %d" % MAX_DIST)
    return np.ascontiguousarray(d.astype(np.int32))


POOL_MODES = {"none": 0, "greedy": 1, "optimal": 2}      # TD_POOL_NONE / TD_POOL_GREEDY / TD_POOL_OPTIMAL


def pool_mode(pool):
    """a pooling policy by name -> its TD_POOL_* value (ValueError for anything else)"""
    if pool not in POOL_MODES:
        raise ValueError("pool=%r: one of %s" % (pool, ", ".join(sorted(POOL_MODES))))
    return POOL_MODES[pool]


def pool_n_sizes(pool_n):
    """pool_n as the worlds take it -> None (the pool= policy holds) or (k_hi, k_lo); a bare k means (k, k).  ValueError
    unless 2 <= k_lo <= k_hi <= 4."""
    if pool_n is None:
        return None
    if isinstance(pool_n, (list, tuple, np.ndarray)):
        if len(pool_n) != 2:
            raise ValueError("pool_n=%r: None, k or (k_hi, k_lo)" % (pool_n,))
        hi, lo = pool_n
    else:
        hi = lo = pool_n
    if isinstance(hi, bool) or isinstance(lo, bool) or int(hi) != hi or int(lo) != lo:
        raise ValueError("pool_n=%r: the sizes must be integers" % (pool_n,))
    hi, lo = int(hi), int(lo)
    if not 2 <= lo <= hi <= 4:
        raise ValueError("pool_n=%r: 2 <= k_lo <= k_hi <= 4 is required" % (pool_n,))
    return hi, lo


ROUTE_NONE_SEEN = -(1 << 63)  # route_m["max_over_loss"] before the first drop-off (td_sim_route_metrics: INT64_MIN)
POOL_BUFFER_MIN = 24 * 2047   # td_sim_pool_buffer: the room td_pool_n_banded needs for the largest tick
POOL_BUFFER_BATCH_MIN = 24 * 512   # td_simb_pool_buffer: a world of a batch pools at most 512 requests
POOL_BUFFER_BATCH_MAX = 1 << 22    # ... and a workgroup's slab is at most td_pool_n_batched's largest


def pool_buffer_size(pool_buffer, largest=2047, most=None):
    """pool_buffer of a world -> an int: 0 (off) or at least 24 * largest (2047; a world of a batch: 512) and at most `most`
    (ValueError)"""
    if isinstance(pool_buffer, bool) or not isinstance(pool_buffer, (int, np.integer)):
        raise ValueError("pool_buffer=%r: an integer" % (pool_buffer,))
    if pool_buffer < 0 or 0 < pool_buffer < 24 * largest:
        raise ValueError("pool_buffer=%r: 0, or at least 24 * %d = %d" % (pool_buffer, largest, 24 * largest))
    if most is not None and pool_buffer > most:
        raise ValueError("pool_buffer=%r: at most %d" % (pool_buffer, most))
    return int(pool_buffer)


def pool_n_rule(pool_wait, pool_loss):
    """pool_wait / pool_loss of a pool_n policy -> two ints, each at least 0 (ValueError)"""
    out = []
    for what, v in (("pool_wait", pool_wait), ("pool_loss", pool_loss)):
        if isinstance(v, bool) or int(v) != v or int(v) < 0:
            raise ValueError("%s=%r: an integer, at least 0" % (what, v))
        out.append(int(v))
    return tuple(out)


from .dispatch import DISPATCH_MODES   # the one table: TD_DISPATCH_LCM_OPT / _OPT / _LCM / _SPLIT by name


def dispatch_mode(dispatch):
    """a dispatch method by name -> its TD_DISPATCH_* value (ValueError for anything else, as pool_mode)"""
    if dispatch not in DISPATCH_MODES:
        raise ValueError("dispatch=%r: one of %s" % (dispatch, ", ".join(sorted(DISPATCH_MODES))))
    return DISPATCH_MODES[dispatch]


class HipBackend:
    """cost build / LCM / optimal assignment on the GPU through the C ABI; dist: a stand-to-stand table (None = |a - b|).
    pool / max_loss: the policy find_pool follows when the caller names none ("greedy": dispatch.find_pool, "optimal":
    dispatch.find_pool_optimal; max_loss=None: every ordered pair is a candidate).  max_happy: the most happy plans of one
    find_pool_n stage (0: the default of the pool call underneath).  pool_buffer > 0: every find_pool_n stage is
    td_pool_n_banded with this plan buffer (the specification of td_sim_pool_buffer) and max_happy is not looked at."""

    def __init__(self, dist=None, pool="greedy", max_loss=None, max_happy=0, pool_buffer=0):
        from . import dispatch
        self.d = dispatch
        self.dist = None if dist is None else check_dist(dist)
        pool_mode(pool)
        self.pool, self.max_loss, self.max_happy = pool, max_loss, int(max_happy)
        self.pool_buffer = pool_buffer_size(pool_buffer)

    def calculate_cost(self, cab_to, dem_from):
        return self.d.cost_build(cab_to, dem_from, self.dist, fill=BIG_COST, threshold=DROP_TIME)[1]

    def lcm(self, cost, max_non_lcm=None):
        return self.d.LCM_simulator(cost, max_non_lcm=MAX_NON_LCM if max_non_lcm is None else max_non_lcm, big_cost=BIG_COST)

    def solve(self, cost):
        return self.d.assign(cost)[0]

    def split(self, cab_to, dem_from, parts=4):
        """the split heuristic on the tick's thresholded model (td_dispatch_batched, TD_DISPATCH_SPLIT, a batch of one):
        the request each cab serves within dem_from, or -1"""
        cab_to, dem_from = np.asarray(cab_to, np.int32), np.asarray(dem_from, np.int32)
        res = self.d.dispatch_batched([cab_to], [dem_from], self.dist, big_cost=BIG_COST, drop_time=DROP_TIME, size=N_STANDS, mode="split",
                                      parts=parts)
        return res["row_to_col"][0, :cab_to.size]

    def find_pool(self, frm, to, max_loss=None, optimal=None):
        optimal = self.pool == "optimal" if optimal is None else optimal
        max_loss = self.max_loss if max_loss is None else max_loss
        if optimal:
            return self.d.find_pool_optimal(frm, to, self.dist, max_loss)
        return self.d.find_pool(frm, to, self.dist, max_loss)

    def find_pool_n(self, k, frm, to, wait, loss):
        """pools of k among the requests (td_pool_n: every request may be the first pick-up) -> (records [m, 2k+1] of
        pick-ups, drop-offs, cost in td_pool_n's order, happy plans before de-duplication); up to 512 requests through
        td_pool_n_batched on the one model, above through td_pool_n; with pool_buffer all through td_pool_n_banded"""
        frm, to, wait, loss = (np.asarray(a, np.int32).reshape(-1) for a in (frm, to, wait, loss))
        rows = np.stack([np.arange(frm.size, dtype=np.int32), frm, to, wait, loss], axis=1)
        if self.pool_buffer > 0:
            return self.d.find_pool_n_banded(k, rows, self.dist, plan_buffer=self.pool_buffer)[:2]
        if frm.size <= self.d.POOL_N_BATCHED_NMAX:
            recs, nh = self.d.pool_n_batched(k, [rows], self.dist, max_happy=self.max_happy)
            return np.asarray(recs[0]), int(np.asarray(nh).reshape(-1)[0])
        return self.d.find_pool_n(k, rows, self.dist, max_happy=self.max_happy)


class HipTickBackend(HipBackend):
    """The same path with ONE C-ABI call per tick (td_tick = Simulator.java:163-208 behind one entry point: cost build ->
    LCM -> removal of the matched cabs / requests on the device -> cost build -> optimal assignment); the harness
    only applies the pairs and the solution to its world."""

    def tick(self, cab_to, dem_from):
        return self.d.tick(np.asarray(cab_to, np.int32), np.asarray(dem_from, np.int32), self.dist, big_cost=BIG_COST,
                           drop_time=DROP_TIME, max_non_lcm=MAX_NON_LCM)


class _RealCells:
    """cost[s][c] of a model that stayed on the device, as far as analyzeSolution reads it (Simulator.java:508-511: a
    cell is dist[cab.to][request.from] when that is below DROP_TIME, else big_cost)"""

    def __init__(self, supply, demand, dist=None):
        self.supply, self.demand, self.dist = supply, demand, dist

    def __getitem__(self, s):
        to = self.supply[s][2]
        return _RealRow(to, self.demand, self.dist)


class _RealRow:
    def __init__(self, to, demand, dist=None):
        self.to, self.demand, self.dist = to, demand, dist

    def __getitem__(self, c):
        frm = self.demand[c][1]
        d = abs(self.to - frm) if self.dist is None else int(self.dist[self.to, frm])
        return d if d < DROP_TIME else BIG_COST


def read_demand(path):
    """taxi_demand.txt rows `(id,from,to,time,at)` (Simulator.java:280-304, gendemand.py:19)."""
    op = gzip.open if str(path).endswith(".gz") else open
    rows = []
    with op(path, "rt") as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append([int(v) for v in line[1:-1].split(",")])
    return np.asarray(rows, dtype=np.int64).reshape(-1, 5)


def cheat_a_bit(frm, cost):
    """Simulator.java:469-474"""
    if frm + cost >= N_STANDS:
        return 0 if frm - cost < 0 else frm - cost
    return frm + cost


class Simulator:
    """dist: a stand-to-stand distance table (N_STANDS x N_STANDS, see check_dist; None = the line, |a - b|).  The row is
    always the stand the cab is at or heads to: dist[cab][request].  The backend has to work on the same table
    (HipBackend(dist=...)).  cheat_a_bit stays the reference's stand arithmetic (from +- cost against N_STANDS), which
    means something on a line only; it is kept as it is, bug-compatible, in a table world too.
    pool / max_loss: the pooling policy, the specification of td_sim_pooling.  "greedy" with max_loss=None is
    Simulator.java:691 (every ordered pair, stable cost order) and calls backend.find_pool(frm, to) as it always did; any
    other policy calls backend.find_pool(frm, to, max_loss=..., optimal=...): max_loss > 0 admits the pairs that pass
    pool_opt_min.py:56-64's loss tests, "optimal" takes the most pools, then the least cost, in ascending (cost, custA,
    custB).  "none": findPool and analyzePool do not run, no pool event is written, max_POOL_* stay as they are.
    dispatch / max_non_lcm / parts: the dispatch policy, the specification of td_dispatch_batched's modes inside a world.
    "lcm+opt" with max_non_lcm=None is Simulator.java:163-208 with the module's MAX_NON_LCM, through the calls it always made.
    Any other policy goes step by step through backend.calculate_cost / lcm(cost, max_non_lcm=...) / solve / split:
    "lcm+opt" with its own max_non_lcm; "opt": the LCM never runs; "lcm": the LCM with stop size 0, run to its end, with
    supply always, and the solver never (the line ends after the pairs, total_LCM_used counts the tick); "split":
    backend.split(cab_to, dem_from, parts) on the whole model, applied by analyze_solution (method OPT), max_solver_size takes
    the whole model size.
    pool_n / pool_wait / pool_loss: pools of up to four, the specification of td_sim_pooling_n.  pool_n=None: nothing above
    changes.  pool_n = k or (k_hi, k_lo), 2 <= k_lo <= k_hi <= 4, replaces the pool= policy: find_pool runs a cascade over the
    tick's demand list, stage k = k_hi, k_hi - 1, .., k_lo on the requests no earlier stage pooled (list order kept).  Stage k
    is backend.find_pool_n(k, from, to, wait, loss) = td_pool_n(k, ...) on that list with max_wait = pool_wait and max_loss =
    pool_loss (percent) for every request, every request a possible first pick-up, the world's table or |a - b|; a list
    shorter than k yields nothing.  The tick's plans are the stages' records in stage order, as (pick-ups, drop-offs, cost)
    with indices into the tick's demand list.  analyze_pool: every member of a record but its first pick-up leaves the
    demand; the first pick-up stays and carries field 3 = the id of the second pick-up, field 4 = the pool's size, field 5 =
    the cost; the other members (pick-up order) travel beside it.  Where such a customer is dispatched, _assign_pooled runs
    once per other member in pick-up order, so total_second_passengers and total_pickup_numb grow by one per other member.
    What reaches the request table: on the LCM path (analyze_pairs) d_cab of every member and d_pick of the first pick-up,
    and no pool info; on the OPT path (analyze_solution) those and d_pool_id = the second pick-up's id, d_pool_plan = the
    size, d_pool_cost = the cost, on the first pick-up's row.  The cab stays busy for the cost through cheat_a_bit, as with a
    pair; there is no route model.  max_POOL_size: the most pools of a tick, all stages together; max_POOL_MEM_size: the most
    happy plans before de-duplication of a tick, summed over its stages.  Events: EV_POOL carries the total, one EV_POOL_PAIR
    (customer = the first pick-up, aux = the member) and one EV_POOLED_SECOND per other member.
    route: the route model, the specification of td_sim_route.  False: nothing above changes.  True (needs pool_n; with events:
    ValueError "not built"): a cab dispatched to a customer with a pool record drives the record instead of cheat_a_bit.  Its
    stops are from[p0], .., from[p(k-1)] (picks), to[q0], .., to[q(k-1)] (drops), the path the record's cost prices; c_stops[c]
    holds them as words request index * 2 + (1: drop), -1 behind the list, c_pos[c] counts the stops served.  The route lives
    in the cab and not in the request table, so it is driven on the LCM path as on the OPT path (the reference's asymmetry
    for pool info does not apply to it).  _assign_to_cab_and_go serves stop 0 at t and advances; _go_to_pickup heads to
    from[p0] as before, and the arrival serves stop 0 and advances.  _advance at tick t from the stand just reached: while the
    next stop is at this stand, serve it (a pick sets d_pick[member] = t, a drop d_drop[member] = t: zero-length legs); with a
    stop left the cab starts for its stand (c_from = here, c_to = there, c_start = t, on board), with none it is free here in
    this tick.  Every existing metric is counted where it is counted without routes.  route_m: drop_numb, ride_time = the sum
    of d_drop - d_pick over the dropped-off members, solo_time = the sum of their direct ways, max_over_loss = the largest
    ride * 100 - solo * (100 + pool_loss) seen (ROUTE_NONE_SEEN before the first drop): <= 0 iff every driven ride keeps the loss
    rule."""

    def __init__(self, demand_rows, backend=None, n_cabs=N_CABS, on_solver_instance=None, dist=None, events=False, pool="greedy",
                 max_loss=None, dispatch="lcm+opt", max_non_lcm=None, parts=4, pool_n=None, pool_wait=0, pool_loss=0, route=False):
        pool_mode(pool)
        self.pool_n = pool_n_sizes(pool_n)
        self.pool_wait, self.pool_loss = pool_n_rule(pool_wait, pool_loss)
        self.route = False       # set_route: routes are handed out
        self._has_routes = False # the world has route state (from the first set_route(True) on): cabs mid-route finish theirs
        self._routes = {}        # route: the first pick-up's id -> (the stop words of its record, the record's cost), of this tick
        self._others = {}        # pool_n: the first pick-up's id -> the ids of the pool's other members, of this tick
        dispatch_mode(dispatch)
        if max_non_lcm is not None and int(max_non_lcm) < 0:
            raise ValueError("max_non_lcm=%r is negative" % (max_non_lcm,))
        if dispatch == "split" and not 1 <= int(parts) <= min(32, N_STANDS):
            raise ValueError("parts=%r outside 1 .. min(32, the number of stands)" % (parts,))
        self.dispatch, self.max_non_lcm, self.parts = dispatch, (None if max_non_lcm is None else int(max_non_lcm)), int(parts)
        self.pool, self.max_loss = pool, (None if max_loss is None or not max_loss > 0 else float(max_loss))
        self._events_on = bool(events)
        self.events = []         # events=True: the records of simulog.txt (format_events), in the order the Java writes them
        self.dist = None if dist is None else check_dist(dist, N_STANDS).astype(np.int64)
        self.be = backend if backend is not None else HipBackend(dist)
        self.on_solver_instance = on_solver_instance
        d = np.asarray(demand_rows, dtype=np.int64)
        self.d_id, self.d_from, self.d_to, self.d_time, self.d_at = (d[:, k].copy() for k in range(5))
        nd = d.shape[0]
        self.d_cab = np.full(nd, -1, np.int64)          # cab_assigned (-2 = dropped)
        self.d_pick = np.full(nd, -1, np.int64)
        self.d_pool_id = np.full(nd, -1, np.int64)
        self.d_pool_plan = np.full(nd, -1, np.int64)
        self.d_pool_cost = np.zeros(nd, np.int64)
        self.id2idx = {int(v): i for i, v in enumerate(self.d_id)}
        # initSupply, Simulator.java:565-573
        self.n_cabs = n_cabs
        self.c_from = np.arange(n_cabs, dtype=np.int64) % N_STANDS
        self.c_to = self.c_from.copy()
        self.c_clnt = np.full(n_cabs, -1, np.int64)
        self.c_onboard = np.zeros(n_cabs, np.int64)
        self.c_start = np.full(n_cabs, -1, np.int64)
        self.m = dict(total_dropped=0, total_pickup_time=0, total_pickup_numb=0, total_LCM_used=0,
                      max_model_size=0, max_solver_size=0, max_POOL_MEM_size=0, max_POOL_size=0,
                      total_second_passengers=0)
        self.log = []
        if route:
            self.set_route(True)

    # ---- the route model (route=True)
    def set_route(self, on):
        """td_sim_route between two ticks: True hands routes out from the next tick on (the first time makes the route state),
        False stops handing them out; cabs that are mid-route finish theirs"""
        if on and self.pool_n is None:
            raise ValueError("route=True needs a pool_n policy: pairs have no drop-off order to drive")
        if on and self._events_on:
            raise ValueError("not built: the event log of routed worlds")
        if on and not self._has_routes:
            nd = self.d_id.size
            self.c_stops = np.full((self.n_cabs, 8), -1, np.int64)
            self.c_pos = np.zeros(self.n_cabs, np.int64)
            self.d_drop = np.full(nd, -1, np.int64)
            self.route_m = dict(drop_numb=0, ride_time=0, solo_time=0, max_over_loss=ROUTE_NONE_SEEN)
            self._has_routes = True
        self.route = bool(on)

    def _has_stops(self, c):
        return self.c_pos[c] < 8 and self.c_stops[c, self.c_pos[c]] >= 0

    def _routed(self, cust):
        return self.route and cust[3] != -1 and cust[0] in self._routes

    def _give_route(self, c, cust, method, how):
        """cab c receives the stop list of cust's record (method: EV_LCM / EV_OPT, how: "standing" / "heading"; not used here)"""
        words, _ = self._routes[cust[0]]
        self.c_stops[c, :] = -1
        self.c_stops[c, :len(words)] = words
        self.c_pos[c] = 0

    def _serve(self, t, d, drop):
        if not drop:
            self.d_pick[d] = t
            return
        ride, solo = t - int(self.d_pick[d]), int(self._way(int(self.d_from[d]), int(self.d_to[d])))
        self.d_drop[d] = t
        m = self.route_m
        m["drop_numb"] += 1
        m["ride_time"] += ride
        m["solo_time"] += solo
        m["max_over_loss"] = max(m["max_over_loss"], ride * 100 - solo * (100 + self.pool_loss))

    def _advance(self, t, c, cur):
        pos, nxt = int(self.c_pos[c]), -1
        while pos < 8 and self.c_stops[c, pos] >= 0:
            w = int(self.c_stops[c, pos])
            d, drop = w >> 1, w & 1
            stand = int(self.d_to[d] if drop else self.d_from[d])
            if stand != cur:
                nxt = stand
                break
            self._serve(t, d, drop)
            pos += 1
        self.c_pos[c] = pos
        self.c_from[c] = cur
        if nxt >= 0:
            self.c_to[c] = nxt
            self.c_onboard[c] = 1
            self.c_start[c] = t
        else:                       # the cab is free at this stand in this tick
            self.c_to[c] = cur
            self.c_clnt[c] = -1
            self.c_onboard[c] = 0
            self.c_start[c] = -1

    def _ev(self, t, kind, method=0, customer=-1, cab=-1, aux=-1):
        if self._events_on:
            self.events.append((int(t), 0, kind, method, int(customer), int(cab), int(aux), 0))

    # ---- Simulator.java:220-254
    def _way(self, a, b):
        """the distance from stand(s) a to stand(s) b"""
        return np.abs(a - b) if self.dist is None else self.dist[a, b]

    def check_if_cab_at_destination(self, t):
        moving = np.nonzero((self.c_from != self.c_to) &
                            (self._way(self.c_from, self.c_to) == t - self.c_start))[0]
        for c in moving:
            if self.c_onboard[c] == 0:
                d = self.id2idx.get(int(self.c_clnt[c]))
                if d is None:
                    continue
                self.d_cab[d] = c
                self.d_pick[d] = t
                self._ev(t, EV_PICKED_UP, customer=self.d_id[d], cab=c)                       # :233
                self.m["total_pickup_numb"] += 1
                if self._has_routes and self._has_stops(c):      # the arrival serves stop 0 and advances
                    self._advance(t, c, int(self.d_from[d]))
                    continue
                self.c_from[c] = self.d_from[d]
                self.c_to[c] = self.d_to[d] if self.d_pool_id[d] == -1 else cheat_a_bit(int(self.d_from[d]),
                                                                                       int(self.d_pool_cost[d]))
                self.c_clnt[c] = self.d_id[d]
                self.c_onboard[c] = 1
                self.c_start[c] = t
            elif self._has_routes and self._has_stops(c):    # a cab with stops left: serve the stop, then advance
                self._advance(t, c, int(self.c_to[c]))
            else:
                self.c_from[c] = self.c_to[c]
                self.c_clnt[c] = -1
                self.c_onboard[c] = 0
                self.c_start[c] = -1
                self._ev(t, EV_CAB_FREE, cab=c, aux=self.c_to[c])                             # :251

    @staticmethod
    def _near(stand_flags):
        """near[s] = any flagged stand within distance < DROP_TIME of s"""
        cs = np.concatenate([[0], np.cumsum(stand_flags.astype(np.int64))])
        s = np.arange(N_STANDS)
        lo = np.maximum(0, s - (DROP_TIME - 1))
        hi = np.minimum(N_STANDS - 1, s + (DROP_TIME - 1))
        return (cs[hi + 1] - cs[lo]) > 0

    def _near_cabs(self, cab_flags):
        """createTempDemand's side: near[s] = some flagged stand s' (a cab heads there) has dist[s'][s] < DROP_TIME"""
        if self.dist is None:
            return self._near(cab_flags)
        return (self.dist[np.nonzero(cab_flags)[0], :] < DROP_TIME).any(axis=0)

    def _near_requests(self, req_flags):
        """createTempSupply's side: near[s] = some flagged stand s' (a request starts there) has dist[s][s'] < DROP_TIME"""
        if self.dist is None:
            return self._near(req_flags)
        return (self.dist[:, np.nonzero(req_flags)[0]] < DROP_TIME).any(axis=1)

    # ---- Simulator.java:329-355
    def create_temp_demand(self, t):
        cand = np.nonzero((self.d_cab == -1) & (t >= self.d_at))[0]
        drop = cand[t - self.d_at[cand] >= DROP_TIME]
        self.d_cab[drop] = -2
        self.m["total_dropped"] += int(drop.size)
        for d in drop:
            self._ev(t, EV_DROPPED, customer=self.d_id[d])                                    # :339
        keep = cand[t - self.d_at[cand] < DROP_TIME]
        free_to = np.zeros(N_STANDS, bool)
        free_to[self.c_to[self.c_clnt == -1]] = True
        near = self._near_cabs(free_to)
        keep = keep[near[self.d_from[keep]]]
        self._ev(t, EV_TEMP_DEMAND, aux=keep.size)                                            # :331 / :352, also an empty list
        for d in keep:
            self._ev(t, EV_TEMP_DEMAND_ID, customer=self.d_id[d])                             # :347
        # TempDemand: id, from, to, pool_clnt_id, pool_plan, pool_cost
        return [[int(self.d_id[d]), int(self.d_from[d]), int(self.d_to[d]), -1, -1, 0] for d in keep]

    # ---- Simulator.java:358-372
    def create_temp_supply(self):
        has_req = np.zeros(N_STANDS, bool)
        has_req[self.d_from[self.d_cab == -1]] = True     # ANY unassigned request, no time check
        near = self._near_requests(has_req)
        cabs = np.nonzero((self.c_from == self.c_to) & (self.c_clnt == -1) & near[self.c_to])[0]
        return [[int(c), int(self.c_from[c]), int(self.c_to[c])] for c in cabs]   # Supply: id, from, to

    # ---- Simulator.java:681-758 (every ordered pair is admitted: plan1 = plan2 = true at :691)
    def find_pool(self, temp_demand, t=None):
        n = len(temp_demand)
        if n < 2:
            self._ev(t, EV_POOL, aux=0)                                                       # :742 / :756, no pair
            return []
        frm = np.array([r[1] for r in temp_demand], np.int64)
        to = np.array([r[2] for r in temp_demand], np.int64)
        self.m["max_POOL_MEM_size"] = max(self.m["max_POOL_MEM_size"], n * (n - 1))
        # pool of two on the backend (td_pool2 on the GPU; the tests' comparator restates it on the host)
        if self.pool == "greedy" and self.max_loss is None:
            out = self.be.find_pool(frm, to)
        else:
            out = self.be.find_pool(frm, to, max_loss=self.max_loss, optimal=self.pool == "optimal")
        self.m["max_POOL_size"] = max(self.m["max_POOL_size"], len(out))
        self._ev(t, EV_POOL, aux=len(out))                                                    # :742 / :756
        for p in out:
            self._ev(t, EV_POOL_PAIR, customer=temp_demand[p[0]][0], aux=temp_demand[p[1]][0])   # :746
        return out

    # findPool under pool_n: the cascade; -> [(pick-ups, drop-offs, cost)] with indices into temp_demand, in plan order
    def find_pool_n(self, temp_demand, t=None):
        n = len(temp_demand)
        if n < 2:
            self._ev(t, EV_POOL, aux=0)
            return []
        frm = np.array([r[1] for r in temp_demand], np.int64)
        to = np.array([r[2] for r in temp_demand], np.int64)
        k_hi, k_lo = self.pool_n
        live = np.arange(n)      # the requests no earlier stage pooled, in list order
        out, happy = [], 0
        for k in range(k_hi, k_lo - 1, -1):
            m = int(live.size)
            if m < k:
                continue
            recs, nh = self.be.find_pool_n(k, frm[live], to[live], np.full(m, self.pool_wait, np.int32), np.full(m, self.pool_loss, np.int32))
            happy += int(nh)
            gone = np.zeros(m, bool)
            for r in np.asarray(recs, np.int64).reshape(-1, 2 * k + 1).tolist():
                out.append((tuple(int(live[i]) for i in r[:k]), tuple(int(live[i]) for i in r[k:2 * k]), int(r[2 * k])))
                gone[r[:k]] = True
            live = live[~gone]
        self.m["max_POOL_MEM_size"] = max(self.m["max_POOL_MEM_size"], happy)
        self.m["max_POOL_size"] = max(self.m["max_POOL_size"], len(out))
        self._ev(t, EV_POOL, aux=len(out))
        for picks, _, _ in out:
            for other in picks[1:]:
                self._ev(t, EV_POOL_PAIR, customer=temp_demand[picks[0]][0], aux=temp_demand[other][0])
        return out

    # analyzePool for records: -> (the demand after pooling, {first pick-up's id: the other members' ids in pick-up order})
    @staticmethod
    def analyze_pool_n(pool, temp_demand):
        leaves = {d for picks, _, _ in pool for d in picks[1:]}
        first = {}
        for picks, _, cost in pool:
            first.setdefault(picks[0], (picks[1:], len(picks), cost))
        out, others = [], {}
        for d, r in enumerate(temp_demand):
            if d in leaves:
                continue
            cust = [r[0], r[1], r[2], -1, -1, 0]
            if d in first:
                rest, size, cost = first[d]
                cust[3], cust[4], cust[5] = temp_demand[rest[0]][0], size, cost
                others[r[0]] = tuple(temp_demand[o][0] for o in rest)
            out.append(cust)
        return out, others

    # the customers assigned with a dispatched customer: its pool's other members in pick-up order
    def _pool_members(self, cust):
        if cust[3] == -1:
            return ()
        return self._others.get(cust[0], (cust[3],)) if self.pool_n is not None else (cust[3],)

    # findPool + analyzePool under the world's policy; "none": the demand as it is, in the model's six-field form
    def _pooled(self, temp_demand, t):
        if self.pool_n is not None:
            pool = self.find_pool_n(temp_demand, t)
            out, self._others = self.analyze_pool_n(pool, temp_demand)
            self._routes = {}
            if self.route:       # the stops of each record, under its first pick-up: the path pn_check prices
                idx = lambda p: self.id2idx[temp_demand[p][0]]
                for picks, drops, cost in pool:
                    self._routes.setdefault(temp_demand[picks[0]][0], ([2 * idx(p) for p in picks] + [2 * idx(q) + 1 for q in drops], cost))
            return out
        if self.pool == "none":
            return [[r[0], r[1], r[2], -1, -1, 0] for r in temp_demand]
        return self.analyze_pool(self.find_pool(temp_demand, t), temp_demand)

    # ---- Simulator.java:760-784
    @staticmethod
    def analyze_pool(pool, temp_demand):
        is_b = {p[1] for p in pool}
        a_info = {}
        for a, b, plan, cost in pool:
            a_info.setdefault(a, (b, plan, cost))
        out = []
        for d, r in enumerate(temp_demand):
            if d in is_b:
                continue
            cust = [r[0], r[1], r[2], -1, -1, 0]
            if d in a_info:
                b, plan, cost = a_info[d]
                cust[3], cust[4], cust[5] = temp_demand[b][0], plan, cost
            out.append(cust)
        return out

    def calculate_cost(self, temp_demand, temp_supply):
        n = max(len(temp_demand), len(temp_supply))
        if n == 0:
            return np.zeros((0, 0), np.int32)
        return np.asarray(self.be.calculate_cost(np.array([s[2] for s in temp_supply], np.int32),
                                                 np.array([d[1] for d in temp_demand], np.int32)))

    # ---- Simulator.java:424-490
    def _assign_pooled(self, customer, cab, t=None, method=0):
        d2 = self.id2idx.get(int(customer))
        if d2 is not None:
            self.d_cab[d2] = cab
            self._ev(t, EV_POOLED_SECOND, method, customer=customer, cab=cab)                 # :432-433
            self.m["total_second_passengers"] += 1

    def _assign_to_cab_and_go(self, t, c, cust, method=0):
        if self._routed(cust):       # the cab stands at from[p0]: stop 0 is served at t and the cab advances; no cheat_a_bit
            self._give_route(c, cust, method, "standing")
            self.c_clnt[c] = cust[0]
            self.m["total_pickup_numb"] += 1
            self._advance(t, c, cust[1])
            return
        self.c_from[c] = cust[1]
        self.c_to[c] = cust[2] if cust[3] == -1 else cheat_a_bit(int(self.c_from[c]), cust[5])
        self.c_clnt[c] = cust[0]
        self.c_onboard[c] = 1
        self.c_start[c] = t
        self.m["total_pickup_numb"] += 1
        self._ev(t, EV_ASSIGNED_PICKED, method, customer=cust[0], cab=c, aux=cust[3])          # :448-465

    def _go_to_pickup(self, t, c, cust, method=0):
        if self._routed(cust):       # heads to from[p0] as below; the arrival serves stop 0
            self._give_route(c, cust, method, "heading")
        self.c_to[c] = cust[1]
        self.c_clnt[c] = cust[0]
        self.c_onboard[c] = 0
        self.c_start[c] = t
        self._ev(t, EV_HEADING, method, customer=cust[0], cab=c)                              # :486-487
        self.m["total_pickup_time"] += int(self._way(int(self.c_from[c]), int(self.c_to[c])))

    def _dispatch(self, t, supply, cust, method=0):
        c = supply[0]   # cab id == cab index
        if supply[2] == cust[1]:
            self._assign_to_cab_and_go(t, c, cust, method)
        elif self._way(supply[2], cust[1]) < DROP_TIME:
            self._go_to_pickup(t, c, cust, method)

    # ---- Simulator.java:613-674
    def analyze_pairs(self, t, pairs, temp_demand, temp_supply):
        by_cab = {}
        by_clnt = {}
        for cab, clnt in pairs:
            by_cab.setdefault(cab, clnt)
            by_clnt.setdefault(clnt, cab)
        supply2, demand2 = [], []
        for s, sup in enumerate(temp_supply):
            if s in by_cab:
                self._dispatch(t, sup, temp_demand[by_cab[s]], EV_LCM)
            else:
                supply2.append(list(sup))
        for d, cust in enumerate(temp_demand):
            if d in by_clnt:
                c2 = self.id2idx[cust[0]]
                cab_id = temp_supply[by_clnt[d]][0]
                self.d_cab[c2] = cab_id
                self._ev(t, EV_ASSIGNED_LCM, customer=cust[0], cab=cab_id)                    # :654
                self.d_pick[c2] = t
                for other in self._pool_members(cust):
                    self._assign_pooled(other, cab_id, t, EV_LCM)
                    self.m["total_pickup_numb"] += 1
                # NOTE: pool info is NOT copied into demand[] on the LCM path (only :391-396 does)
            else:
                demand2.append(list(cust))
        return supply2, demand2

    # ---- Simulator.java:375-421
    def analyze_solution(self, t, r2c, cost, temp_demand, temp_supply):
        total = 0
        for s, sup in enumerate(temp_supply):
            c = int(r2c[s]) if s < len(r2c) else -1
            if 0 <= c < len(temp_demand) and cost[s][c] < BIG_COST and sup[1] == sup[2]:
                total += 1
                cust = temp_demand[c]
                d = self.id2idx[cust[0]]
                self.d_cab[d] = sup[0]
                self.d_pick[d] = t
                for other in self._pool_members(cust):
                    self._assign_pooled(other, sup[0], t, EV_OPT)
                    self.m["total_pickup_numb"] += 1
                if cust[3] > -1:
                    self.d_pool_id[d], self.d_pool_plan[d], self.d_pool_cost[d] = cust[3], cust[4], cust[5]
                self._dispatch(t, sup, cust, EV_OPT)
        return total

    # ---- one tick of Simulator.java:151-211 ; returns the simulog_solv line (or None)
    def tick(self, t):
        self.check_if_cab_at_destination(t)
        temp_demand = self.create_temp_demand(t)
        if not temp_demand:
            return None
        temp_supply = self.create_temp_supply()
        line = "t:%d. Initial Count of demand=%d, supply=%d. " % (t, len(temp_demand), len(temp_supply))
        cost = np.zeros((0, 0), np.int32)
        r2c = []
        if temp_supply and (self.dispatch != "lcm+opt" or self.max_non_lcm is not None):
            return self._tick_policy(t, line, temp_demand, temp_supply)
        if temp_supply and hasattr(self.be, "tick"):
            return self._tick_one_call(t, line, temp_demand, temp_supply)
        if temp_supply:
            temp_demand = self._pooled(temp_demand, t)
            cost = self.calculate_cost(temp_demand, temp_supply)
            self.m["max_model_size"] = max(self.m["max_model_size"], cost.shape[0])
            if cost.shape[0] > MAX_NON_LCM:
                pairs, lcm_min_val = self.be.lcm(cost)
                self.m["total_LCM_used"] += 1
                line += "LCM n_pairs=%d" % len(pairs)
                temp_supply, temp_demand = self.analyze_pairs(t, pairs, temp_demand, temp_supply)
                if lcm_min_val == BIG_COST:      # :188 no input for the solver
                    return line
                cost = self.calculate_cost(temp_demand, temp_supply)
                line += ". Sent to solver: demand=%d, supply=%d. " % (len(temp_demand), len(temp_supply))
            self.m["max_solver_size"] = max(self.m["max_solver_size"], cost.shape[0])
            if self.on_solver_instance is not None:
                self.on_solver_instance(t, temp_supply, temp_demand, cost)
            r2c = self.be.solve(cost)
        count = self.analyze_solution(t, r2c, cost, temp_demand, temp_supply)
        return line + "; OPT count=%d" % count

    # ---- the same tick (Simulator.java:163-208) with the whole path behind ONE backend call (td_tick)
    def _tick_one_call(self, t, line, temp_demand, temp_supply):
        temp_demand = self._pooled(temp_demand, t)
        n = max(len(temp_demand), len(temp_supply))
        self.m["max_model_size"] = max(self.m["max_model_size"], n)
        res = self.be.tick([s[2] for s in temp_supply], [d[1] for d in temp_demand])
        if n > MAX_NON_LCM:
            self.m["total_LCM_used"] += 1
            pairs = list(zip(res["lcm_rows"].tolist(), res["lcm_cols"].tolist()))
            line += "LCM n_pairs=%d" % len(pairs)
            kept_supply, kept_demand = self.analyze_pairs(t, pairs, temp_demand, temp_supply)
            # the device's shrink (k_tick_shrink) and analyzePairs' removal must agree
            assert [s[0] for s in kept_supply] == [temp_supply[k][0] for k in res["kept_cabs"].tolist()]
            assert [d[0] for d in kept_demand] == [temp_demand[k][0] for k in res["kept_dems"].tolist()]
            temp_supply, temp_demand = kept_supply, kept_demand
            if not res["solved"]:                # :188 no input for the solver
                return line
            line += ". Sent to solver: demand=%d, supply=%d. " % (len(temp_demand), len(temp_supply))
        self.m["max_solver_size"] = max(self.m["max_solver_size"], res["n_rest"])
        r2c = res["row_to_col"]
        # analyzeSolution reads cost[s][c] < big_cost (:378-383): a real cell of the thresholded model
        count = self.analyze_solution(t, r2c, _RealCells(temp_supply, temp_demand, self.dist), temp_demand, temp_supply)
        return line + "; OPT count=%d" % count

    # ---- the same tick under a dispatch policy of its own (td_dispatch_batched's modes)
    def _tick_policy(self, t, line, temp_demand, temp_supply):
        temp_demand = self._pooled(temp_demand, t)
        n = max(len(temp_demand), len(temp_supply))
        self.m["max_model_size"] = max(self.m["max_model_size"], n)
        mnl = MAX_NON_LCM if self.max_non_lcm is None else self.max_non_lcm
        if self.dispatch == "split":
            self.m["max_solver_size"] = max(self.m["max_solver_size"], n)
            r2c = self.be.split([s[2] for s in temp_supply], [d[1] for d in temp_demand], self.parts)
            count = self.analyze_solution(t, r2c, _RealCells(temp_supply, temp_demand, self.dist), temp_demand, temp_supply)
            return line + "; OPT count=%d" % count
        if self.dispatch == "lcm" or (self.dispatch == "lcm+opt" and n > mnl):
            pairs, lcm_min_val = self.be.lcm(self.calculate_cost(temp_demand, temp_supply), max_non_lcm=0 if self.dispatch == "lcm" else mnl)
            self.m["total_LCM_used"] += 1
            line += "LCM n_pairs=%d" % len(pairs)
            temp_supply, temp_demand = self.analyze_pairs(t, pairs, temp_demand, temp_supply)
            # the LCM alone never solves; :188 no input for the solver; and nobody left over is no model (td_tick's rule)
            if self.dispatch == "lcm" or lcm_min_val == BIG_COST or not (temp_supply or temp_demand):
                return line
            line += ". Sent to solver: demand=%d, supply=%d. " % (len(temp_demand), len(temp_supply))
        cost = self.calculate_cost(temp_demand, temp_supply)
        self.m["max_solver_size"] = max(self.m["max_solver_size"], cost.shape[0])
        if self.on_solver_instance is not None:
            self.on_solver_instance(t, temp_supply, temp_demand, cost)
        count = self.analyze_solution(t, self.be.solve(cost), cost, temp_demand, temp_supply)
        return line + "; OPT count=%d" % count

    # ---- Simulator.java:256-277 printMetrics (wall-clock lines are the caller's: pass them in)
    def metrics_text(self, total_simul_time=0, max_solver_time=0, max_lcm_time=0, max_pool_time=0):
        m = self.m
        lines = ["", "Total customers: %d" % self.d_id.size,
                 "Total dropped customers: %d" % m["total_dropped"],
                 "Total pickedup customers: %d" % m["total_pickup_numb"],
                 "Total customers with assigned cabs: %d" % int((self.d_cab > -1).sum()),
                 "Total simulation time [secs]: %d" % total_simul_time,
                 "Total pickup time: %d" % m["total_pickup_time"]]
        if m["total_pickup_numb"] > 0:
            lines.append("Avg pickup time: %d" % (m["total_pickup_time"] // m["total_pickup_numb"]))
        lines += ["Max model size: %d" % m["max_model_size"], "Max solver size: %d" % m["max_solver_size"],
                  "Max solver time: %d" % max_solver_time, "Max LCM time: %d" % max_lcm_time,
                  "LCM use count: %d" % m["total_LCM_used"], "Max POOL time: %d" % max_pool_time,
                  "Max POOL array size: %d" % m["max_POOL_MEM_size"], "Max POOL size: %d" % m["max_POOL_size"],
                  "Total second customers in POOL: %d" % m["total_second_passengers"]]
        return "\n".join(lines)

    def run(self, t_end=HOURS * 60):
        for t in range(t_end):
            line = self.tick(t)
            if line is not None:
                self.log.append(line)
        return self.log


def event_kinds_mask(events):
    """events: True (every kind) or an iterable of kinds 1 .. 11 -> td_sim_log's bit set; None / False -> 0"""
    if events is None or events is False:
        return 0
    if events is True:
        return sum(1 << k for k in EV_KINDS)
    mask = 0
    for k in events:
        if int(k) not in EV_KINDS:
            raise ValueError("event kind %r outside 1 .. 11" % (k,))
        mask |= 1 << int(k)
    return mask


def format_events(records, world=None):
    """The lines of simulog.txt, byte for byte Simulator.java's strings (without the newline), from event records in log order:
    an (n, 8) array or a sequence of 8-word records.  world: format the records of this world only (a batch's records are
    formatted world by world); None takes every record.  A tempDemand / pool header collects the list records that follow it
    within its tick; a header whose list records were masked out or lost is the bare header, and a list record without its
    header gives no line."""
    lines = []
    open_kind, open_t = 0, None
    for r in np.asarray(records, dtype=np.int64).reshape(-1, 8).tolist():
        t, w, kind, method, cust, cab, aux = r[:7]
        if world is not None and w != world:
            continue
        head = "Time %d. " % t
        if kind in (EV_TEMP_DEMAND_ID, EV_POOL_PAIR):
            if open_kind == kind - 1 and open_t == t:
                lines[-1] += "%d, " % cust if kind == EV_TEMP_DEMAND_ID else "%d(%d), " % (cust, aux)
            continue
        open_kind, open_t = (kind, t) if kind in (EV_TEMP_DEMAND, EV_POOL) else (0, None)
        if kind == EV_PICKED_UP:
            lines.append(head + "Customer %d picked up by Cab %d" % (cust, cab))                    # :233
        elif kind == EV_CAB_FREE:
            lines.append(head + "Cab %d is free at stand %d" % (cab, aux))                          # :251
        elif kind == EV_DROPPED:
            lines.append(head + "Customer %d dropped" % cust)                                       # :339
        elif kind == EV_TEMP_DEMAND:
            lines.append(head + "tempDemand: ")                                                     # :331
        elif kind == EV_POOL:
            lines.append(head + "Customers in pool: ")                                              # :742
        elif kind == EV_ASSIGNED_PICKED:                                                            # :448-463
            lines.append(head + "Customer %d assigned to and picked up by Cab %d" % (cust, cab)
                         + (" (POOL: the other Customer %d)" % aux if aux != -1 else "") + " (method %s)" % EV_METHOD[method])
        elif kind == EV_HEADING:                                                                    # :486-487
            lines.append(head + "Customer %d assigned to Cab %d, cab is heading to the customer (method %s)" % (cust, cab, EV_METHOD[method]))
        elif kind == EV_ASSIGNED_LCM:
            lines.append(head + "Customer %d assigned by LCM to Cab %d" % (cust, cab))              # :654
        elif kind == EV_POOLED_SECOND:                                                              # :432-433
            lines.append(head + "Customer %d assigned in a pool as second passenger to Cab %d (method %s)" % (cust, cab, EV_METHOD[method]))
        else:
            raise ValueError("event record of kind %d" % kind)
    return lines


def _read_pools_n(sim, call, n_req):
    """td_sim_pools_n / td_simb_pools_n -> [(pick-ups, drop-offs, cost)] in plan order"""
    cap = max(n_req // 2, 1)
    recs, size = np.empty((cap, 9), np.int32), np.empty(cap, np.int32)
    k = sim._ct.c_int32(0)
    sim._ffi.check(call(cap, sim._ffi.addr(recs), sim._ffi.addr(size), sim._ct.byref(k)))
    return [(tuple(int(v) for v in recs[i, :size[i]]), tuple(int(v) for v in recs[i, 4:4 + size[i]]), int(recs[i, 8])) for i in range(k.value)]


def _read_pools(sim, call, n_req):
    cap = max(n_req // 2, 1)
    a, b, plan, cost = (np.empty(cap, np.int32) for _ in range(4))
    k = sim._ct.c_int32(0)
    ad = sim._ffi.addr
    sim._ffi.check(call(cap, ad(a), ad(b), ad(plan), ad(cost), sim._ct.byref(k)))
    return [(int(a[i]), int(b[i]), int(plan[i]), int(cost[i])) for i in range(k.value)]


class _DeviceEvents:
    """the event log of a device handle (td_sim_log / td_sim_events or their td_simb twins), shared by both classes"""

    def _events_init(self, log_fn, events_fn, events, capacity, default_capacity):
        self._ev_fn = events_fn
        self.events_lost = 0         # records that did not fit the log, the running total
        self.event_kinds = event_kinds_mask(events)
        self.event_capacity = 0
        if self.event_kinds:
            self.event_capacity = int(default_capacity if capacity is None else capacity)
            self._ffi.check(log_fn(self._h, self.event_kinds, self.event_capacity))

    def events(self, max_records=None):
        """drains the log -> an (n, 8) int32 array of records, oldest first ((0, 8) without logging); `events_lost` grows by
        what did not fit since the last drain.  max_records: take at most so many; more in the log raises TdError and
        leaves the log as it is."""
        ct = self._ct
        n, lost = ct.c_int64(0), ct.c_int64(0)
        if max_records is None:      # ask for the number first: max_records = 0 succeeds only on an empty log
            rc = self._ev_fn(self._h, 0, None, ct.byref(n), ct.byref(lost))
            if rc == 0:
                self.events_lost += lost.value
                return np.zeros((0, 8), np.int32)
            if n.value <= 0:
                self._ffi.check(rc)
            max_records = n.value
        out = np.empty((max(int(max_records), 1), 8), np.int32)
        self._ffi.check(self._ev_fn(self._h, int(max_records), self._ffi.addr(out), ct.byref(n), ct.byref(lost)))
        self.events_lost += lost.value
        return out[:n.value].copy()


class DeviceSimulator(_DeviceEvents):
    """The same world in device memory behind the C ABI (td_sim_*, csrc/td_sim.hip): the cab and request tables never leave
    the GPU, a tick is ONE call (`tick` = td_sim_step: world kernels around td_pool2 and td_tick), and only the counters
    of the log line come back.  `begin` / `model` / `apply` split the tick so that the assignment decisions can come from
    any source.  Log lines, `m` and `metrics_text` are those of `Simulator` with `HipTickBackend`.
    dist: a stand-to-stand distance table as `Simulator` takes it (numpy array-like, or an int32 torch tensor on the device);
    the handle keeps its own copy (td_sim_create_dist).  n_stands then defaults to the table's size.  A host table is
    checked here (check_dist: ValueError); a device tensor is checked for shape and dtype only (ValueError) and its size,
    diagonal and entries by td_sim_create_dist on the device, which raises TdError.
    events: True or an iterable of event kinds (EV_*) switches the event log on (td_sim_log); `events()` drains it,
    `format_events` makes simulog.txt's lines of it.  event_capacity: the records the log holds; the default,
    4 * (n_cabs + n_req) + 64, holds any one tick of the world (a tick writes at most 3 n_cabs + 3.5 n_req + 2 records), so
    a caller that drains after every tick loses nothing.
    pool / max_loss: the pooling policy as `Simulator` takes it (td_sim_pooling); `pools()` reads the plans of the tick last
    begun (td_sim_pools).
    dispatch / parts: the dispatch policy as `Simulator` takes it (td_sim_dispatch, with the world's max_non_lcm); None: the
    world never calls td_sim_dispatch and dispatches as it always did.
    pool_n / pool_wait / pool_loss / max_happy: pools of up to four as `Simulator` takes them (td_sim_pooling_n; max_happy: the
    most happy plans of one stage, 0 = the default of the pool call underneath); `pools_n()` reads the records of the tick
    last begun (td_sim_pools_n), `set_pool_n` changes the policy between two ticks.  None: td_sim_pooling_n is never called.
    pool_buffer: > 0: every stage of a pool_n world is td_pool_n_banded with this plan buffer (td_sim_pool_buffer; at least
    24 * 2047), so no tick is refused for its number of happy plans; `set_pool_buffer` changes it between two ticks, 0 switches
    it off.  0: td_sim_pool_buffer is never called.
    route: True: a pooled cab drives its record as `Simulator(route=True)` specifies (td_sim_route; needs pool_n, and no
    events: ValueError); `set_route` switches it between two ticks (cabs mid-route finish theirs), `route_state()` and
    `route_metrics()` read what it adds.  False: td_sim_route is never called."""

    M_KEYS = ("total_dropped", "total_pickup_time", "total_pickup_numb", "total_LCM_used", "max_model_size", "max_solver_size",
              "max_POOL_MEM_size", "max_POOL_size", "total_second_passengers")
    CAB_KEYS = ("c_from", "c_to", "c_clnt", "c_onboard", "c_start")
    REQ_KEYS = ("d_cab", "d_pick", "d_pool_id", "d_pool_plan", "d_pool_cost")
    ROUTE_M_KEYS = ("drop_numb", "ride_time", "solo_time", "max_over_loss")

    def __init__(self, demand_rows, n_cabs=None, n_stands=None, drop_time=None, max_non_lcm=None, big_cost=None, dist=None, events=None,
                 event_capacity=None, pool="greedy", max_loss=None, dispatch=None, parts=4, pool_n=None, pool_wait=0, pool_loss=0, max_happy=0,
                 pool_buffer=0, route=False):
        import ctypes
        if route and pool_n is None:
            raise ValueError("route=True needs a pool_n policy: pairs have no drop-off order to drive")
        if route and event_kinds_mask(events):
            raise ValueError("not built: the event log of routed worlds")
        mode = pool_mode(pool)
        pool_buffer = pool_buffer_size(pool_buffer)
        if dispatch is not None:
            dispatch_mode(dispatch)
        pool_n_sizes(pool_n)
        pool_n_rule(pool_wait, pool_loss)
        from . import _ffi
        self._ffi, self._ct = _ffi, ctypes
        self._lib = _ffi.lib()
        self._h = None
        d = np.asarray(demand_rows, dtype=np.int64).reshape(-1, 5)
        self.n_req = int(d.shape[0])
        self.n_cabs = int(N_CABS if n_cabs is None else n_cabs)
        if dist is not None:
            if getattr(dist, "is_cuda", False):      # a device table is checked by td_sim_create_dist
                if str(dist.dtype) != "torch.int32" or dist.dim() != 2 or dist.shape[0] != dist.shape[1]:
                    raise ValueError("distance table: a device tensor must be a square int32 table")
            else:
                dist = check_dist(dist)
            if n_stands is not None and int(n_stands) != int(dist.shape[0]):
                raise ValueError("distance table: %d x %d for n_stands=%d" % (dist.shape[0], dist.shape[0], int(n_stands)))
            n_stands = int(dist.shape[0])
        self.n_stands = int(N_STANDS if n_stands is None else n_stands)
        self.drop_time = int(DROP_TIME if drop_time is None else drop_time)
        self.max_non_lcm = int(MAX_NON_LCM if max_non_lcm is None else max_non_lcm)
        self.big_cost = int(BIG_COST if big_cost is None else big_cost)
        cols = [_ffi.as_i32(d[:, k]) for k in (0, 1, 2, 4)]      # id, from, to, at
        h = ctypes.c_void_p()
        _ffi.check(self._lib.td_sim_create_dist(self.n_cabs, self.n_stands, self.drop_time, self.max_non_lcm, self.big_cost, self.n_req,
                                                *[_ffi.addr(c) if self.n_req else None for c in cols], _ffi.addr(dist), ctypes.byref(h)))
        self._h = h
        self._cap = max(self.n_cabs, self.n_req, 1)
        self._info = None
        self.log = []
        self._events_init(self._lib.td_sim_log, self._lib.td_sim_events, events, event_capacity, 4 * (self.n_cabs + self.n_req) + 64)
        self.pool, self.max_loss = pool, max_loss
        if pool != "greedy" or max_loss is not None:      # a default world never calls td_sim_pooling
            _ffi.check(self._lib.td_sim_pooling(self._h, mode, 0.0 if max_loss is None else float(max_loss)))
        self.pool_n = None
        if pool_n is not None:                            # a default world never calls td_sim_pooling_n
            self.set_pool_n(pool_n, pool_wait, pool_loss, max_happy)
        self.pool_buffer = 0
        if pool_buffer:                                   # a default world never calls td_sim_pool_buffer
            self.set_pool_buffer(pool_buffer)
        self.dispatch, self.parts = "lcm+opt", int(parts)
        if dispatch is not None:                          # a default world never calls td_sim_dispatch
            self.set_dispatch(dispatch, self.max_non_lcm, parts)
        self.route = False
        if route:                                         # a default world never calls td_sim_route
            self.set_route(True)

    def set_route(self, on):
        """td_sim_route: hand routes out (or stop handing them out; cabs mid-route finish theirs) from the next begin on"""
        self._ffi.check(self._lib.td_sim_route(self._h, int(bool(on))))
        self.route = bool(on)

    def route_state(self):
        """td_sim_route_state under Simulator's names: d_drop [n_req], c_pos [n_cabs], c_stops [n_cabs, 8]"""
        drop, pos = np.empty(max(self.n_req, 1), np.int32), np.empty(max(self.n_cabs, 1), np.int32)
        stops = np.empty((max(self.n_cabs, 1), 8), np.int32)
        self._ffi.check(self._lib.td_sim_route_state(self._h, *[self._ffi.addr(a) for a in (drop, pos, stops)]))
        return dict(d_drop=drop[:self.n_req], c_pos=pos[:self.n_cabs], c_stops=stops[:self.n_cabs])

    def route_metrics(self):
        """td_sim_route_metrics: Simulator.route_m"""
        out = np.zeros(len(self.ROUTE_M_KEYS), np.int64)
        self._ffi.check(self._lib.td_sim_route_metrics(self._h, self._ffi.addr(out)))
        return {k: int(v) for k, v in zip(self.ROUTE_M_KEYS, out)}

    def set_pool_n(self, pool_n, pool_wait=0, pool_loss=0, max_happy=0):
        """td_sim_pooling_n: pools of k_hi down to k_lo (pool_n = k or (k_hi, k_lo)) under pool_wait / pool_loss, from the next
        begin on; pool_n=None: td_sim_pooling with the handle's pool= policy, back on pairs"""
        if pool_n is None:
            self._ffi.check(self._lib.td_sim_pooling(self._h, pool_mode(self.pool), 0.0 if self.max_loss is None else float(self.max_loss)))
            self.pool_n = None
            return
        hi, lo = pool_n_sizes(pool_n)
        wait, loss = pool_n_rule(pool_wait, pool_loss)
        self._ffi.check(self._lib.td_sim_pooling_n(self._h, hi, lo, wait, loss, int(max_happy)))
        self.pool_n, self.pool_wait, self.pool_loss, self.max_happy = (hi, lo), wait, loss, int(max_happy)

    def set_pool_buffer(self, pool_buffer):
        """td_sim_pool_buffer: the plan buffer of td_pool_n_banded for every stage of a pool_n world, from the next begin on; 0:
        the stages run as they did without it"""
        self._ffi.check(self._lib.td_sim_pool_buffer(self._h, int(pool_buffer)))
        self.pool_buffer = int(pool_buffer)

    def pools_n(self):
        """the plans of the tick last begun under pool_n: a list of (pick-ups, drop-offs, cost), the members indices into that
        tick's demand list before pooling, in plan order (Simulator.find_pool_n's list)"""
        return _read_pools_n(self, lambda *a: self._lib.td_sim_pools_n(self._h, *a), self.n_req)

    def set_dispatch(self, dispatch, max_non_lcm=None, parts=4):
        """td_sim_dispatch: the dispatch method ("lcm+opt", "opt", "lcm", "split"), its max_non_lcm (None: as it is) and the
        split's parts, from the next begin on"""
        mnl = self.max_non_lcm if max_non_lcm is None else int(max_non_lcm)
        self._ffi.check(self._lib.td_sim_dispatch(self._h, dispatch_mode(dispatch), mnl, int(parts)))
        self.dispatch, self.max_non_lcm, self.parts = dispatch, mnl, int(parts)

    def pools(self):
        """the plans of the tick last begun: a list of (custA, custB, plan, cost), indices into that tick's demand list
        before pooling, in plan order; [] when no pooling ran"""
        return _read_pools(self, lambda *a: self._lib.td_sim_pools(self._h, *a), self.n_req)

    def close(self):
        if self._h is not None:
            self._lib.td_sim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the split tick
    def begin(self, t):
        """-> (has_demand, demand before pooling, supply, demand after pooling)"""
        info = np.zeros(4, np.int32)
        self._ffi.check(self._lib.td_sim_begin(self._h, int(t), self._ffi.addr(info)))
        self._t = int(t)
        self._info = tuple(int(v) for v in info)
        return self._info

    def model(self):
        """this tick's model: (cab_to, dem_from), the stands the free cabs stand at / the requests start from"""
        if self._info is None:
            raise self._ffi.TdError("DeviceSimulator.model: no tick has begun")
        cab = np.empty(max(self._info[2], 1), np.int32)
        dem = np.empty(max(self._info[3], 1), np.int32)
        self._ffi.check(self._lib.td_sim_model(self._h, self._ffi.addr(cab), self._ffi.addr(dem)))
        return cab[:self._info[2]], dem[:self._info[3]]

    def apply(self, lcm_rows=(), lcm_cols=(), solved=True, row_to_col=()):
        """the decisions of `dispatch.tick` (or of anything else) -> the line's OPT count (-1: the line has none)"""
        rows, cols, r2c = (self._ffi.as_i32(np.asarray(a).reshape(-1)) for a in (lcm_rows, lcm_cols, row_to_col))
        if rows.size != cols.size:
            raise self._ffi.TdError("lcm_rows and lcm_cols differ in length")
        opt = self._ct.c_int32(0)
        self._ffi.check(self._lib.td_sim_apply(self._h, int(rows.size), self._ffi.addr(rows) if rows.size else None,
                                               self._ffi.addr(cols) if cols.size else None, int(bool(solved)), int(r2c.size),
                                               self._ffi.addr(r2c) if r2c.size else None, self._ct.byref(opt)))
        return opt.value

    @staticmethod
    def format_line(t, line):
        """the simulog_solv line of Simulator.tick / _tick_one_call from td_sim_step's nine counters (None: no line)"""
        has, dem, sup, lcm, pairs, sent, dem2, sup2, opt = (int(v) for v in line)
        if not has:
            return None
        s = "t:%d. Initial Count of demand=%d, supply=%d. " % (t, dem, sup)
        if lcm:
            s += "LCM n_pairs=%d" % pairs
            if not sent:
                return s
            s += ". Sent to solver: demand=%d, supply=%d. " % (dem2, sup2)
        return s + "; OPT count=%d" % opt

    # ---- one tick in one call
    def tick(self, t):
        line = np.zeros(9, np.int32)
        self._ffi.check(self._lib.td_sim_step(self._h, int(t), self._ffi.addr(line)))
        self._info = None
        return self.format_line(int(t), line)

    def run(self, t_end=HOURS * 60):
        for t in range(t_end):
            line = self.tick(t)
            if line is not None:
                self.log.append(line)
        return self.log

    # ---- read-outs
    @property
    def m(self):
        out = np.zeros(len(self.M_KEYS), np.int64)
        self._ffi.check(self._lib.td_sim_metrics(self._h, self._ffi.addr(out)))
        return {k: int(v) for k, v in zip(self.M_KEYS, out)}

    def state(self):
        """the ten state arrays under Simulator's attribute names (c_clnt holds request ids)"""
        arrs = [np.empty(max(self.n_cabs, 1), np.int32) for _ in self.CAB_KEYS] + [np.empty(max(self.n_req, 1), np.int32) for _ in self.REQ_KEYS]
        self._ffi.check(self._lib.td_sim_state(self._h, *[self._ffi.addr(a) for a in arrs]))
        out = {k: a[:self.n_cabs] for k, a in zip(self.CAB_KEYS, arrs[:5])}
        out.update({k: a[:self.n_req] for k, a in zip(self.REQ_KEYS, arrs[5:])})
        return out

    def metrics_text(self, total_simul_time=0, max_solver_time=0, max_lcm_time=0, max_pool_time=0):
        view = Simulator.__new__(Simulator)
        view.m = self.m
        view.d_id = np.empty(self.n_req, np.int64)
        view.d_cab = self.state()["d_cab"]
        return Simulator.metrics_text(view, total_simul_time, max_solver_time, max_lcm_time, max_pool_time)


def pack_worlds(demand_rows_list, n_cabs_list):
    """The host side of td_simb_create: a list of demand tables (rows `(id, from, to, time, at)`, one table per world; a
    table may be empty) and a list of fleet sizes -> (n_cabs[B], req_off[B+1], id, from, to, at), the tables concatenated
    world after world as int32.  Ids must be unique and not negative within a world; two worlds may use the same ids."""
    tables = list(demand_rows_list)
    cabs = [int(c) for c in n_cabs_list]
    if not tables:
        raise ValueError("pack_worlds: a batch needs at least one world")
    if len(tables) != len(cabs):
        raise ValueError("pack_worlds: %d demand tables for %d fleet sizes" % (len(tables), len(cabs)))
    off, parts = [0], []
    for b, rows in enumerate(tables):
        d = np.asarray(rows, dtype=np.int64)
        if d.size == 0:
            d = d.reshape(0, 5)
        if d.ndim != 2 or d.shape[1] != 5:
            raise ValueError("pack_worlds: world %d's demand table has shape %r, not (n, 5)" % (b, d.shape))
        if cabs[b] < 1:
            raise ValueError("pack_worlds: world %d has %d cabs, at least 1 is needed" % (b, cabs[b]))
        ids = d[:, 0]
        if ids.size and ids.min() < 0:
            raise ValueError("pack_worlds: world %d has a negative request id" % b)
        if np.unique(ids).size != ids.size:
            raise ValueError("pack_worlds: request ids must be unique within world %d" % b)
        if d.size and (d.max() > 2**31 - 1 or d.min() < -2**31):
            raise ValueError("pack_worlds: world %d holds a value outside int32" % b)
        parts.append(d)
        off.append(off[-1] + d.shape[0])
    if off[-1] > 2**31 - 1:
        raise ValueError("pack_worlds: %d requests in all, more than int32 offsets address" % off[-1])
    allrows = np.concatenate(parts, axis=0)
    cols = [np.ascontiguousarray(allrows[:, k].astype(np.int32)) for k in (0, 1, 2, 4)]
    return (np.asarray(cabs, np.int32), np.asarray(off, np.int32)) + tuple(cols)


class DeviceSimulatorBatch(_DeviceEvents):
    """B independent worlds behind ONE handle (td_simb_*, csrc/td_simb.hip): the worlds share the city (n_stands, drop_time,
    max_non_lcm, big_cost) and differ in fleet size and request table.  `tick` advances every world by one td_simb_step
    (td_pool2_batched and td_tick_batched on the device lists); `begin` / `model` / `apply` split the tick for decisions
    from any source.  Per world, lines, `m[b]`, `state(b)` and `metrics_text(b)` are those of `DeviceSimulator`.
    dist: ONE stand-to-stand distance table for the whole batch, as `DeviceSimulator` takes it (numpy array-like, or an int32
    torch tensor on the device); the handle keeps its own copy (td_simb_create_dist).  n_stands then defaults to the table's
    size.  A host table is checked here (check_dist), and so are its size against n_stands and the request stands against
    the table: ValueError, before the library is touched.  A device tensor is checked for shape and dtype only; its size,
    diagonal and entries by td_simb_create_dist on the device, which raises TdError.
    events / event_capacity: as `DeviceSimulator` takes them; ONE log for the handle (td_simb_log), a record's second word is
    its world, and within a tick world 0's records come first.  The default capacity, 4 * (all cabs + all requests) + 64 * B,
    holds any one tick of the batch.
    pool / max_loss: the pooling policy, one for the batch or a list with one entry per world (td_simb_pooling; None in a
    max_loss list: every ordered pair in that world); `pools(b)` reads world b's plans of the tick last begun.
    pool_n / pool_wait / pool_loss / max_happy: pools of up to four per world (td_simb_pooling_n): a list with one entry per
    world (k, (k_hi, k_lo), or None: the world keeps its pool= policy) or one value for all; `pools_n(b)` reads world b's
    records, `set_pool_n` changes the policies between two ticks.  A batch that logs events takes such policies with k_hi = 2 only.
    pool_buffer: > 0: every pool round of the pool_n worlds is td_pool_n_banded_batched's kernel with this plan buffer per
    workgroup (td_simb_pool_buffer; 24 * 512 .. 2^22), so no tick is refused for a world's number of happy plans;
    `set_pool_buffer` changes it between two ticks, 0 switches it off.  0: td_simb_pool_buffer is never called.
    route (keyword only): True, or a list with one bool per world: a pooled cab of such a world drives its record as `Simulator(route=True)`
    specifies (td_simb_route); a routed world needs a pool_n policy, and a routed batch takes no events (ValueError, before
    the library is touched).  A world whose routes are off behaves as in a batch without routes.  `set_route` switches the
    worlds between two ticks (cabs mid-route finish theirs); `route_state(b)` and `route_metrics()` read what the routes add,
    per world as `DeviceSimulator` reports them.  False: td_simb_route is never called."""

    M_KEYS, CAB_KEYS, REQ_KEYS = DeviceSimulator.M_KEYS, DeviceSimulator.CAB_KEYS, DeviceSimulator.REQ_KEYS
    ROUTE_M_KEYS = DeviceSimulator.ROUTE_M_KEYS
    format_line = staticmethod(DeviceSimulator.format_line)

    # dispatch / max_non_lcm / parts: the dispatch policy per world (td_simb_dispatch), each a list with one entry per world or one
    # value for all; dispatch=None with a scalar max_non_lcm: the batch never calls td_simb_dispatch and dispatches as it always did
    def __init__(self, demand_rows_list, n_cabs_list, n_stands=None, drop_time=None, max_non_lcm=None, big_cost=None, dist=None,
                 events=None, event_capacity=None, pool="greedy", max_loss=None, dispatch=None, parts=4, pool_n=None, pool_wait=0, pool_loss=0,
                 max_happy=0, pool_buffer=0, **routing):
        import ctypes
        # route= is keyword-only and is taken from **routing: the keywords a batch has had since before it could be routed stay
        # the whole of its named signature (tests/test_sim_route_cpu.py reads it); any other extra keyword is a TypeError
        route = routing.pop("route", False)
        if routing:
            raise TypeError("DeviceSimulatorBatch() got an unexpected keyword argument %r" % sorted(routing)[0])
        pool_buffer = pool_buffer_size(pool_buffer, 512, POOL_BUFFER_BATCH_MAX)
        n_cabs_list = list(n_cabs_list)
        nb = len(n_cabs_list)
        routes = self._route_list(route, nb)
        if any(routes):
            sizes = list(pool_n) if isinstance(pool_n, list) else [pool_n] * nb
            self._check_routes(routes, sizes)
            if event_kinds_mask(events):
                raise ValueError("not built: the event log of routed worlds")
        mnl_list = None
        if isinstance(max_non_lcm, (list, tuple, np.ndarray)):      # a max_non_lcm per world is part of the dispatch policy
            mnl_list = [int(v) for v in max_non_lcm]
            if len(mnl_list) != nb:
                raise ValueError("max_non_lcm: %d entries for %d worlds" % (len(mnl_list), nb))
            max_non_lcm = max(mnl_list) if mnl_list else None
            dispatch = "lcm+opt" if dispatch is None else dispatch
        pools = list(pool) if isinstance(pool, (list, tuple)) else [pool] * nb
        losses = list(max_loss) if isinstance(max_loss, (list, tuple, np.ndarray)) else [max_loss] * nb
        if len(pools) != nb or len(losses) != nb:
            raise ValueError("pool / max_loss: %d / %d entries for %d worlds" % (len(pools), len(losses), nb))
        modes = np.array([pool_mode(p) for p in pools], np.int32)
        from . import _ffi
        self._ffi, self._ct = _ffi, ctypes
        self._h = None
        cabs, off, rid, rfrom, rto, rat = pack_worlds(demand_rows_list, n_cabs_list)
        if dist is not None:
            if getattr(dist, "is_cuda", False):      # a device table is checked by td_simb_create_dist
                if str(dist.dtype) != "torch.int32" or dist.dim() != 2 or dist.shape[0] != dist.shape[1]:
                    raise ValueError("distance table: a device tensor must be a square int32 table")
            else:
                dist = check_dist(dist)
            if n_stands is not None and int(n_stands) != int(dist.shape[0]):
                raise ValueError("distance table: %d x %d for n_stands=%d" % (dist.shape[0], dist.shape[0], int(n_stands)))
            n_stands = int(dist.shape[0])
            for what, col in (("from", rfrom), ("to", rto)):
                bad = np.nonzero((col < 0) | (col >= n_stands))[0]
                if bad.size:
                    b = int(np.searchsorted(off, bad[0], side="right")) - 1
                    raise ValueError("distance table: world %d, request %d: %s stand %d outside the %d x %d table"
                                     % (b, int(bad[0] - off[b]), what, int(col[bad[0]]), n_stands, n_stands))
        self._lib = _ffi.lib()
        self.batch = int(cabs.size)
        self.n_cabs = [int(v) for v in cabs]
        self.req_off = off
        self.n_req = [int(off[b + 1] - off[b]) for b in range(self.batch)]
        self.n_stands = int(N_STANDS if n_stands is None else n_stands)
        self.drop_time = int(DROP_TIME if drop_time is None else drop_time)
        self.max_non_lcm = int(MAX_NON_LCM if max_non_lcm is None else max_non_lcm)
        self.big_cost = int(BIG_COST if big_cost is None else big_cost)
        h = ctypes.c_void_p()
        some = int(off[-1]) > 0
        args = [self.batch, _ffi.addr(cabs), self.n_stands, self.drop_time, self.max_non_lcm, self.big_cost, _ffi.addr(off)]
        args += [_ffi.addr(c) if some else None for c in (rid, rfrom, rto, rat)]
        if dist is None:
            _ffi.check(self._lib.td_simb_create(*args, ctypes.byref(h)))
        else:
            _ffi.check(self._lib.td_simb_create_dist(*args, _ffi.addr(dist), ctypes.byref(h)))
        self._h = h
        self._info = None
        self.logs = [[] for _ in range(self.batch)]
        self._events_init(self._lib.td_simb_log, self._lib.td_simb_events, events, event_capacity,
                          4 * (sum(self.n_cabs) + sum(self.n_req)) + 64 * self.batch)
        self.pool, self.max_loss = pools, losses
        if any(p != "greedy" for p in pools) or any(x is not None for x in losses):      # a default batch never calls td_simb_pooling
            ml = np.array([0.0 if x is None else float(x) for x in losses], np.float64)
            _ffi.check(self._lib.td_simb_pooling(self._h, _ffi.addr(modes), _ffi.addr(ml)))
        self.pool_n = [None] * nb
        if pool_n is not None and not (isinstance(pool_n, list) and all(k is None for k in pool_n)):      # a default batch never calls td_simb_pooling_n
            self.set_pool_n(pool_n, pool_wait, pool_loss, max_happy)
        self.pool_buffer = 0
        if pool_buffer:                                   # a default batch never calls td_simb_pool_buffer
            self.set_pool_buffer(pool_buffer)
        self.dispatch, self.max_non_lcms, self.parts = ["lcm+opt"] * nb, [self.max_non_lcm] * nb, [4] * nb
        if dispatch is not None:                          # a default batch never calls td_simb_dispatch
            self.set_dispatch(dispatch, mnl_list, parts)
        self.route = [False] * nb
        if any(routes):                                   # a batch without routes never calls td_simb_route
            self.set_route(routes)

    @staticmethod
    def _route_list(route, nb):
        routes = [bool(v) for v in route] if isinstance(route, (list, tuple, np.ndarray)) else [bool(route)] * nb
        if len(routes) != nb:
            raise ValueError("route: %d entries for %d worlds" % (len(routes), nb))
        return routes

    @staticmethod
    def _check_routes(routes, sizes):
        for b, on in enumerate(routes):
            if on and (b >= len(sizes) or sizes[b] is None):
                raise ValueError("route: world %d needs a pool_n policy: pairs have no drop-off order to drive" % b)

    def set_route(self, route):
        """td_simb_route: hand routes out in the worlds of `route` (a bool for all, or one per world) from the next begin on;
        a world switched off stops getting routes, its cabs that are mid-route finish theirs"""
        routes = self._route_list(route, self.batch)
        self._check_routes(routes, self.pool_n)
        if any(routes) and self.event_kinds:
            raise ValueError("not built: the event log of routed worlds")
        on = np.array(routes, np.int32)
        self._ffi.check(self._lib.td_simb_route(self._h, self._ffi.addr(on)))
        self.route = routes

    def route_state(self, b):
        """td_simb_route_state of world b under Simulator's names: d_drop [n_req], c_pos [n_cabs], c_stops [n_cabs, 8]"""
        nc, nr = self.n_cabs[b], self.n_req[b]
        drop, pos, stops = np.empty(max(nr, 1), np.int32), np.empty(max(nc, 1), np.int32), np.empty((max(nc, 1), 8), np.int32)
        self._ffi.check(self._lib.td_simb_route_state(self._h, int(b), *[self._ffi.addr(a) for a in (drop, pos, stops)]))
        return dict(d_drop=drop[:nr], c_pos=pos[:nc], c_stops=stops[:nc])

    def route_metrics(self):
        """td_simb_route_metrics: Simulator.route_m of every world"""
        out = np.zeros((self.batch, len(self.ROUTE_M_KEYS)), np.int64)
        self._ffi.check(self._lib.td_simb_route_metrics(self._h, self._ffi.addr(out)))
        return [{k: int(v) for k, v in zip(self.ROUTE_M_KEYS, row)} for row in out]

    def set_dispatch(self, dispatch, max_non_lcm=None, parts=4):
        """td_simb_dispatch: the dispatch method ("lcm+opt", "opt", "lcm", "split"), max_non_lcm (None: as created) and the
        split's parts of every world, from the next begin on; each a list per world, or one value for all worlds"""
        per = lambda v: list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * self.batch
        ds, ms, ps = per(dispatch), per(self.max_non_lcm if max_non_lcm is None else max_non_lcm), per(parts)
        if not len(ds) == len(ms) == len(ps) == self.batch:
            raise ValueError("dispatch / max_non_lcm / parts: %d / %d / %d entries for %d worlds" % (len(ds), len(ms), len(ps), self.batch))
        arrs = [np.array([dispatch_mode(d) for d in ds], np.int32), np.array(ms, np.int32), np.array(ps, np.int32)]
        self._ffi.check(self._lib.td_simb_dispatch(self._h, *[self._ffi.addr(a) for a in arrs]))
        self.dispatch, self.max_non_lcms, self.parts = ds, [int(v) for v in ms], [int(v) for v in ps]

    def set_pool_buffer(self, pool_buffer):
        """td_simb_pool_buffer: the plan buffer per workgroup of every pool round of the pool_n worlds, from the next begin on;
        0: the rounds run as they did without it"""
        self._ffi.check(self._lib.td_simb_pool_buffer(self._h, int(pool_buffer)))
        self.pool_buffer = int(pool_buffer)

    def set_pool_n(self, pool_n, pool_wait=0, pool_loss=0, max_happy=0):
        """td_simb_pooling_n: pools of up to four per world, from the next begin on.  pool_n / pool_wait / pool_loss: a list with
        one entry per world, or one value for all worlds; a pool_n entry of None keeps that world's policy as it is.  pool_n=None
        (not a list): td_simb_pooling with the batch's pool= policies, every world back on pairs."""
        nb = self.batch
        if pool_n is None:
            modes = np.array([pool_mode(p) for p in self.pool], np.int32)
            ml = np.array([0.0 if x is None else float(x) for x in self.max_loss], np.float64)
            self._ffi.check(self._lib.td_simb_pooling(self._h, self._ffi.addr(modes), self._ffi.addr(ml)))
            self.pool_n = [None] * nb
            return
        # a list of length 2 of ints is ONE (k_hi, k_lo) for all worlds only when it is a tuple; a list is per world
        sizes = list(pool_n) if isinstance(pool_n, list) else [pool_n] * nb
        per = lambda v: list(v) if isinstance(v, (list, np.ndarray)) else [v] * nb
        waits, losses = per(pool_wait), per(pool_loss)
        if not len(sizes) == len(waits) == len(losses) == nb:
            raise ValueError("pool_n / pool_wait / pool_loss: %d / %d / %d entries for %d worlds" % (len(sizes), len(waits), len(losses), nb))
        hi, lo, wt, ls = (np.zeros(nb, np.int32) for _ in range(4))
        for b in range(nb):
            k = pool_n_sizes(sizes[b])
            if k is None:
                continue
            hi[b], lo[b] = k
            wt[b], ls[b] = pool_n_rule(waits[b], losses[b])
        self._ffi.check(self._lib.td_simb_pooling_n(self._h, *[self._ffi.addr(a) for a in (hi, lo, wt, ls)], int(max_happy)))
        for b in range(nb):
            if hi[b]:
                self.pool_n[b] = (int(hi[b]), int(lo[b]))

    def pools_n(self, b):
        """world b's records of the tick last begun under pool_n, as DeviceSimulator.pools_n lists them"""
        return _read_pools_n(self, lambda *a: self._lib.td_simb_pools_n(self._h, int(b), *a), self.n_req[b])

    def pools(self, b):
        """world b's plans of the tick last begun, as DeviceSimulator.pools lists them"""
        return _read_pools(self, lambda *a: self._lib.td_simb_pools(self._h, int(b), *a), self.n_req[b])

    def close(self):
        if self._h is not None:
            self._lib.td_simb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the split tick
    def begin(self, t):
        """-> int32 [B, 4]: per world (has_demand, demand before pooling, supply, demand after pooling)"""
        info = np.zeros((self.batch, 4), np.int32)
        self._ffi.check(self._lib.td_simb_begin(self._h, int(t), self._ffi.addr(info)))
        self._info = info
        return info

    def model(self):
        """this tick's models: (cab_off, cab_to, dem_off, dem_from), ragged over the worlds (also after a `tick` that
        td_simb_step refused: the tick is then begun and waits for `apply`)"""
        cab_off, dem_off = np.zeros(self.batch + 1, np.int32), np.zeros(self.batch + 1, np.int32)
        cab, dem = np.empty(max(sum(self.n_cabs), 1), np.int32), np.empty(max(sum(self.n_req), 1), np.int32)
        self._ffi.check(self._lib.td_simb_model(self._h, *[self._ffi.addr(a) for a in (cab_off, cab, dem_off, dem)]))
        return cab_off, cab[:cab_off[-1]], dem_off, dem[:dem_off[-1]]

    def apply(self, decisions):
        """decisions: per world None (nothing to apply) or (lcm_rows, lcm_cols, solved, row_to_col) -> OPT counts [B]"""
        if len(decisions) != self.batch:
            raise self._ffi.TdError("DeviceSimulatorBatch.apply: %d decisions for %d worlds" % (len(decisions), self.batch))
        rows, cols, r2c, solved, p_off, r_off = [], [], [], [], [0], [0]
        for d in decisions:
            a, b, sv, r = ((), (), False, ()) if d is None else d
            a, b, r = (self._ffi.as_i32(np.asarray(x).reshape(-1)) for x in (a, b, r))
            if a.size != b.size:
                raise self._ffi.TdError("lcm_rows and lcm_cols differ in length")
            rows.append(a), cols.append(b), r2c.append(r), solved.append(int(bool(sv)))
            p_off.append(p_off[-1] + a.size), r_off.append(r_off[-1] + r.size)
        rows, cols, r2c = (np.ascontiguousarray(np.concatenate(x).astype(np.int32)) for x in (rows, cols, r2c))
        p_off, r_off, solved = (np.asarray(x, np.int32) for x in (p_off, r_off, solved))
        opt = np.zeros(self.batch, np.int32)
        ad = self._ffi.addr
        self._ffi.check(self._lib.td_simb_apply(self._h, ad(p_off), ad(rows) if rows.size else None, ad(cols) if cols.size else None,
                                                ad(solved), ad(r_off), ad(r2c) if r2c.size else None, ad(opt)))
        return opt

    # ---- one tick of every world in one call
    def tick(self, t):
        """-> the B log lines of tick t (None for a world without demand), or None when no world has one"""
        line = np.zeros((self.batch, 9), np.int32)
        self._ffi.check(self._lib.td_simb_step(self._h, int(t), self._ffi.addr(line)))
        self._info = None
        if not line[:, 0].any():
            return None
        return [self.format_line(int(t), line[b]) for b in range(self.batch)]

    def run(self, t_end=HOURS * 60):
        for t in range(t_end):
            lines = self.tick(t)
            if lines is not None:
                for b, line in enumerate(lines):
                    if line is not None:
                        self.logs[b].append(line)
        return self.logs

    # ---- read-outs
    @property
    def m(self):
        out = np.zeros((self.batch, len(self.M_KEYS)), np.int64)
        self._ffi.check(self._lib.td_simb_metrics(self._h, self._ffi.addr(out)))
        return [{k: int(v) for k, v in zip(self.M_KEYS, row)} for row in out]

    def state(self, b):
        """the ten state arrays of world b under Simulator's attribute names (c_clnt holds request ids)"""
        nc, nr = self.n_cabs[b], self.n_req[b]
        arrs = [np.empty(max(nc, 1), np.int32) for _ in self.CAB_KEYS] + [np.empty(max(nr, 1), np.int32) for _ in self.REQ_KEYS]
        self._ffi.check(self._lib.td_simb_state(self._h, int(b), *[self._ffi.addr(a) for a in arrs]))
        out = {k: a[:nc] for k, a in zip(self.CAB_KEYS, arrs[:5])}
        out.update({k: a[:nr] for k, a in zip(self.REQ_KEYS, arrs[5:])})
        return out

    def metrics_text(self, b, total_simul_time=0, max_solver_time=0, max_lcm_time=0, max_pool_time=0):
        view = Simulator.__new__(Simulator)
        view.m = self.m[b]
        view.d_id = np.empty(self.n_req[b], np.int64)
        view.d_cab = self.state(b)["d_cab"]
        return Simulator.metrics_text(view, total_simul_time, max_solver_time, max_lcm_time, max_pool_time)
