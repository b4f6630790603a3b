"""The case table of tests/test_tick_paths_cpu.py and tests/test_gpu_tick_paths.py: td_tick models that sit on every
constant by which csrc/td_tick.hip and csrc/td_lcm.hip choose an LCM path, a copy route or a slice width, and on every
relation between fill and threshold.  Plain data plus generators: nothing here needs a GPU.

A case is (name, cab_to, dem_from, dist or None, fill, threshold, stop_size, claims).  `claims` are conditions the oracle
alone must confirm (test_tick_paths_cpu.py), so that the table cannot drift into cases that test nothing.  CASE_NAMES is
the static list the tests are parametrised over; case(name) builds a case on first use, reference(name) is the oracle's
tick of it, computed once per process and shared (treat both as read-only)."""
import functools

import numpy as np

from test_gpu_tick_batched import oracle_cost, oracle_tick

BIG = 250000          # Simulator.java's big_cost
I32_MAX = 2**31 - 1

# ---- the constants the table sits on; a case names the one it sits on in the comment beside it
STANDS = 64           # k_lcm_stands (td_lcm.hip): positions 0 .. 63, 1 <= threshold <= 64
LST_MAXN = 2048       # td_lcm.hip LST_MAXN: cabs / requests the stands kernel holds in LDS
LISTS_NMIN = 64       # lcm_impl: level lists for n >= 64, k_lcm_loop below
HINT_THR_MAX = 256    # td_tick.hip: the level range 0 .. threshold - 1 is hinted for 1 <= threshold <= 256
HINT_NMAX = 4096      # lcm_impl: hinted lists (one workgroup per row) for n <= 4096; td_tick's one staged copy of both
                      # position arrays holds while 8 n <= 32768, the same n
LV_MAX = 256          # td_lcm.hip LV_MAX: level lists while max - min of the candidates < 256
SHRINK_T = 1024       # k_tick_shrink: one workgroup of 1024 threads, ceil(n / 1024) rows per thread
TICK_BATCH_NMAX = 2048   # td_batch.hip TICK_NMAX: largest model of td_tick_batched
BATCH_NMAX = 1024        # td_batch.hip BATCH_NMAX: largest remainder td_tick_batched solves

# ---- claims
INSIDE0 = "ends inside value 0"                 # the size stop falls among the value-0 picks: take0 = limit < p0
EXACT0 = "take0 == p0 == limit"                 # the size stop falls on the last value-0 pick
ONE_ABOVE0 = "one pick above value 0"           # limit = p0 + 1
RUNS_OUT = "runs out: lcm_min_val == fill"
ENDS_MATCHED = "first and last cab matched"
ENDS_KEPT = "first and last cab kept"
BOTH_QUEUES = "picks above value 0 from both queues"   # a pick at L >= 1 to a lower stand and one to a higher stand
REAL_GE_FILL = "a real cell >= fill exists"
SPAN255 = "span is exactly 255"
SPAN256 = "span is exactly 256"
NEGATIVE = "a negative candidate exists"
SOLVED = "solved"
NO_SOLVE = "no solve"

_BUILDERS = {}


def _add(name, fn):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = fn


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _uniform(seed, n_s, n_d, S):
    rng = np.random.default_rng(seed)
    return _i32(rng.integers(0, S, n_s)), _i32(rng.integers(0, S, n_d))


def _cover(seed, n_s, n_d):
    """positions over the stands path's whole range, 0 and 63 on both sides"""
    cab, dem = _uniform(seed, n_s, n_d, STANDS)
    cab[1], cab[-2], dem[1], dem[-2] = 0, STANDS - 1, STANDS - 1, 0
    return cab, dem


def _split(seed, n_s, n_d, zero_pairs):
    """cabs on even stands, requests on odd stands, `zero_pairs` requests moved onto even stands: few value-0 picks, the rest
    of the LCM at L >= 1 through both queues of every stand"""
    rng = np.random.default_rng(seed)
    cab = _i32(2 * rng.integers(0, STANDS // 2, n_s))
    dem = _i32(2 * rng.integers(0, STANDS // 2, n_d) + 1)
    dem[rng.permutation(n_d)[:zero_pairs]] -= 1
    return cab, dem


def pick_values(cab, dem, dist, fill, thr):
    """the values of the oracle's LCM picks when only exhaustion stops it (stop_size 0); every shorter LCM is a prefix"""
    ref = oracle_tick(cab, dem, dist, fill, thr, 0)
    _, cost = oracle_cost(cab, dem, dist, fill, thr)
    return cost[ref["lcm_rows"], ref["lcm_cols"]]


def p0_on_stands(cab, dem):
    """value-0 picks of an |a - b| model with threshold >= 1 and fill > 0: per stand min(cabs, requests).  For the shapes
    whose whole pick list would take the oracle too long; test_tick_paths_cpu.py confirms the claim built on it."""
    lo = min(int(cab.min()), int(dem.min()))
    cc, cd = np.bincount(cab - lo), np.bincount(dem - lo)
    m = min(len(cc), len(cd))
    return int(np.minimum(cc[:m], cd[:m]).sum())


# ======================================================================================================================
# stands eligibility and the stands algorithm (dist = None)
# ======================================================================================================================
def _stands_shape(seed, n_s, n_d, stop_of, claims, thr=10):
    def build():
        cab, dem = _cover(seed, n_s, n_d)
        n = max(n_s, n_d)
        return cab, dem, None, BIG, thr, stop_of(n, cab, dem), claims
    return build


_add("s_1x1", lambda: (_i32([5]), _i32([5]), None, BIG, 10, 0, (EXACT0, NO_SOLVE)))   # the smallest model: one pick, nothing left
_add("s_64x64", _stands_shape(1, 64, 64, lambda n, c, d: n - p0_on_stands(c, d) - 1, (ONE_ABOVE0, SOLVED)))
_add("s_65x33", _stands_shape(2, 65, 33, lambda n, c, d: n - p0_on_stands(c, d) // 2, (INSIDE0, SOLVED)))
_add("s_300x200", _stands_shape(3, 300, 200, lambda n, c, d: 120, (SOLVED,)))          # the witness's stands case
_add("s_200x300", _stands_shape(4, 200, 300, lambda n, c, d: 120, (SOLVED,)))


def _s_2048x2048():   # LST_MAXN on both sides; ~20 value-0 picks, then 60 more through the queues
    cab, dem = _split(5, LST_MAXN, LST_MAXN, 20)
    cab[0], dem[7] = 0, STANDS - 1
    return cab, dem, None, BIG, 10, LST_MAXN - (p0_on_stands(cab, dem) + 60), (SOLVED,)


def _s_2048x1():      # LST_MAXN cabs, one request three stands beyond the nearest cab: one pick at L = 3, 2047 cabs and no request left
    cab = _i32(np.random.default_rng(6).integers(0, 61, LST_MAXN))
    return cab, _i32([STANDS - 1]), None, BIG, 10, LST_MAXN - 1, (SOLVED,)


def _s_over(n_s, n_d):   # LST_MAXN + 1 on one side: the matrix path
    def build():
        cab, dem = _cover(7, n_s, n_d)
        return cab, dem, None, BIG, 10, max(n_s, n_d) - 30, (SOLVED,)
    return build


_add("s_2048x2048", _s_2048x2048)
_add("s_2048x1", _s_2048x1)
_add("s_2049x100", _s_over(LST_MAXN + 1, 100))
_add("s_100x2049", _s_over(100, LST_MAXN + 1))


# ---- stand ranges at threshold = STANDS (every cell of a model on 0 .. 63 is a candidate)
def _range(thr, cab64=False, req_m1=False):
    def build():
        cab, dem = _cover(8, 300, 200)
        if cab64:
            cab[150] = STANDS       # one cab one stand beyond the stands path
        if req_m1:
            dem[100] = -1           # one request below it
        if thr == 1:                # every value-0 pick and no more: one pick later the candidates have run out
            return cab, dem, None, BIG, thr, 300 - p0_on_stands(cab, dem), (EXACT0, SOLVED)
        return cab, dem, None, BIG, thr, 120, (SOLVED,)
    return build


_add("r_cover_thr64", _range(STANDS))                  # threshold = 64: the last stands threshold
_add("r_cab64_thr64", _range(STANDS, cab64=True))
_add("r_req-1_thr64", _range(STANDS, req_m1=True))
_add("r_cover_thr65", _range(STANDS + 1))              # threshold = 65: hinted lists
_add("r_cover_thr1", _range(1))                        # threshold = 1: value 0 alone
_add("r_one_stand_50x30", lambda: (_i32([7] * 50), _i32([7] * 30), None, BIG, 10, 30, (INSIDE0, SOLVED)))   # all cells 0
_add("r_one_stand_30x50", lambda: (_i32([7] * 30), _i32([7] * 50), None, BIG, 10, 0, (RUNS_OUT, NO_SOLVE)))


def _r_two_queues():
    """stands with only cabs (10, 20, 30, 40) between stands with only requests (5, 15, 25, 35, 45) and one stand with both:
    at L = 5 every cab stand sees a head in its a - L and in its a + L queue"""
    rng = np.random.default_rng(9)
    cab = _i32(rng.choice([10, 20, 30, 40, 50], 70))
    dem = _i32(rng.choice([5, 15, 25, 35, 45, 50], 60))
    return cab, dem, None, BIG, 10, 20, (BOTH_QUEUES, SOLVED)


_add("r_two_queues", _r_two_queues)


# ---- stop sizes from the oracle's pick list of one model (the Simulator's threshold, 50 stands), p0 = value-0 picks
def _stop(which):
    def build():
        cab, dem = _uniform(10, 90, 70, 50)
        n = 90
        v = pick_values(cab, dem, None, BIG, 10)
        p0 = int((v == 0).sum())
        assert 2 <= p0 < len(v)
        stop, claims = {"n-1": (n - 1, (INSIDE0, SOLVED)), "inside0": (n - p0 // 2, (INSIDE0, SOLVED)),
                        "n-p0": (n - p0, (EXACT0, SOLVED)), "n-p0-1": (n - p0 - 1, (ONE_ABOVE0, SOLVED)),
                        "0": (0, (RUNS_OUT, NO_SOLVE))}[which]
        return cab, dem, None, BIG, 10, stop, claims
    return build


for _w in ("n-1", "inside0", "n-p0", "n-p0-1", "0"):
    _add("stop_" + _w, _stop(_w))


# ======================================================================================================================
# fill against threshold (threshold = 10): the stands rule holds only while every value it takes, 0 .. 9, is below fill
# ======================================================================================================================
FILLS = (11, 10, 9, 1, 0, -3, 254, 255, BIG, I32_MAX)


def _fill_case(model, fill, thr=10):
    def build():
        if model == "stands":      # |a - b| on 50 stands: the stands path for fill >= threshold
            cab, dem = _uniform(11, 300, 200, 50)
            dist, stop = None, 120
        elif model == "small":     # n < LISTS_NMIN: the stands path or k_lcm_loop (20 stands, so that every request finds a cab)
            cab, dem = _uniform(12, 40, 30, 20)
            dist, stop = None, 10
        else:                      # a general table of 0 .. 24: hinted lists
            cab, dem = _uniform(13, 300, 200, 50)
            dist, stop = _i32(np.random.default_rng(14).integers(0, 25, (50, 50))), 120
        # the 300 x 200 models reach their size stop with picks of value 0 and 1 alone, the small one needs every value up to 9:
        # below that fill the candidates run out
        claims = [SOLVED] if fill >= (thr if model == "small" else 2) else [NO_SOLVE, RUNS_OUT]
        if fill < thr or thr < 0:
            claims.append(REAL_GE_FILL)
        return cab, dem, dist, fill, thr, stop, tuple(claims)
    return build


for _m in ("stands", "small", "table"):
    for _f in FILLS:
        _add("f_%s_fill%d" % (_m, _f), _fill_case(_m, _f))
_add("f_table_thr-1_fill12", _fill_case("table", 12, thr=-1))


# ======================================================================================================================
# matrix-path edges
# ======================================================================================================================
def _m_n(n_s):   # LISTS_NMIN: n = 63 -> k_lcm_loop, n = 64 -> hinted lists (200 stands: not a stands model)
    def build():
        cab, dem = _uniform(15, n_s, 40, 200)
        return cab, dem, None, BIG, 10, 50, (SOLVED,)
    return build


_add("m_n63", _m_n(LISTS_NMIN - 1))
_add("m_n64", _m_n(LISTS_NMIN))


def _m_thr(thr, claims):   # HINT_THR_MAX: 256 -> hinted, 257 -> measured; 0 -> no candidate at all
    def build():
        cab, dem = _uniform(16, 300, 200, 400)
        return cab, dem, None, BIG, thr, 120, claims
    return build


_add("m_thr256", _m_thr(HINT_THR_MAX, (SOLVED,)))
_add("m_thr257", _m_thr(HINT_THR_MAX + 1, (SOLVED,)))
_add("m_thr0", _m_thr(0, (RUNS_OUT, NO_SOLVE)))


def _m_span(span, claim):   # LV_MAX: candidate span 255 -> measured lists, 256 -> k_lcm_loop
    def build():
        cab, dem = _uniform(17, 100, 80, 50)
        dist = _i32(np.random.default_rng(18).integers(4, 3 + span, (50, 50)))
        dist[cab[0], dem[0]] = 3
        dist[cab[1], dem[1]] = 3 + span
        return cab, dem, dist, BIG, -1, 40, (claim, SOLVED)
    return build


_add("m_span255", _m_span(LV_MAX - 1, SPAN255))
_add("m_span256", _m_span(LV_MAX, SPAN256))


def _m_negative():   # a candidate below the hinted range 0 .. threshold - 1: the lists are redone with a measured range
    cab, dem = _uniform(19, 300, 200, 50)
    rng = np.random.default_rng(20)
    dist = _i32(rng.integers(0, 25, (50, 50)))
    dist[rng.integers(0, 50, 6), rng.integers(0, 50, 6)] = -2
    return cab, dem, dist, BIG, 10, 120, (NEGATIVE, SOLVED)


_add("m_negative", _m_negative)


def _m_wide(n_s):   # HINT_NMAX: n = 4096 -> hinted lists + one staged copy, n = 4097 -> measured lists + two copies
    def build():
        cab, dem = _uniform(21, n_s, 600, 200)
        return cab, dem, None, BIG, 10, n_s - 48, (SOLVED,)
    return build


_add("m_ns4096", _m_wide(HINT_NMAX))
_add("m_ns4097", _m_wide(HINT_NMAX + 1))


# ======================================================================================================================
# shrink edges: k_tick_shrink's slices of ceil(n / SHRINK_T) rows per thread
# ======================================================================================================================
def _shrink(n_s, ends):
    def build():
        rng = np.random.default_rng(22)   # cabs on stands 0 .. 39, requests on 0 .. 52: some requests only reachable above value 0
        cab, dem = _i32(rng.integers(0, 40, n_s)), _i32(rng.integers(0, 53, 100))
        claims = [SOLVED]
        if ends == "matched":    # cab 0 is the first of its stand; the last cab is the only one of stand 45, where a request waits
            cab[-1], dem[3], dem[50] = 45, 45, cab[0]
            claims.append(ENDS_MATCHED)
        elif ends == "kept":     # both on stand 63, no request within the threshold
            cab[0] = cab[-1] = STANDS - 1
            claims.append(ENDS_KEPT)
        stop = n_s - (p0_on_stands(cab, dem) + 5)
        return cab, dem, None, BIG, 10, stop, tuple(claims)
    return build


_add("k_ns1024", _shrink(SHRINK_T, "matched"))             # 1 row per thread
_add("k_ns1025", _shrink(SHRINK_T + 1, "kept"))            # 2 rows per thread, the last threads without rows
_add("k_ns2047", _shrink(2 * SHRINK_T - 1, "matched"))     # 2 rows per thread, the last thread one row
_add("k_ns2049", _shrink(2 * SHRINK_T + 1, "kept"))        # 3 rows per thread (and beyond LST_MAXN: the matrix path)

CASE_NAMES = tuple(_BUILDERS)

# positions (and the table) resident on the device: one stands-eligible case and one table case
DEVICE_CASES = ("s_300x200", "f_table_fill250000")

# the path witness (test_gpu_tick_paths.py): the first grows td_tick's workspace by less than an int32 matrix, each
# neighbour across one edge by at least one
WITNESS = (("r_cover_thr64", ("r_cab64_thr64", "r_req-1_thr64", "r_cover_thr65")),   # a position at 64 / -1, threshold 65
           ("s_2048x1", ("s_2049x100",)),                                            # n_s = LST_MAXN + 1
           ("f_stands_fill10", ("f_stands_fill9", "f_stands_fill0", "f_stands_fill-3")),   # fill < threshold
           ("f_stands_fill250000", ()))                                              # the Simulator's own tick stays on the stands


@functools.lru_cache(maxsize=None)
def case(name):
    cab, dem, dist, fill, thr, stop, claims = _BUILDERS[name]()
    for a in (cab, dem, dist):
        if a is not None:
            a.setflags(write=False)
    return (name, cab, dem, dist, int(fill), int(thr), int(stop), tuple(claims))


@functools.lru_cache(maxsize=None)
def reference(name):
    _, cab, dem, dist, fill, thr, stop, _ = case(name)
    return oracle_tick(cab, dem, dist, fill, thr, stop)


def stands_eligible(c):
    """td::lcm_stands' gate restated from the constants above: the models whose LCM td_tick takes from the positions"""
    _, cab, dem, dist, fill, thr, stop, _ = c
    n = max(len(cab), len(dem))
    return (dist is None and 1 <= thr <= STANDS and fill >= thr and len(cab) <= LST_MAXN and len(dem) <= LST_MAXN
            and 0 <= stop < n and int(min(cab.min(), dem.min())) >= 0 and int(max(cab.max(), dem.max())) < STANDS)


def batched_ok(c):
    """td_tick_batched's size limits"""
    _, cab, dem, _, _, _, stop, _ = c
    n = max(len(cab), len(dem))
    return n <= TICK_BATCH_NMAX and (stop if 0 <= stop < n else n) <= BATCH_NMAX
