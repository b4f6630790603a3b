"""The case table of tests/test_lcm_shard_cases_cpu.py and tests/test_gpu_lcm_shard_paths.py: inputs of the row-sharded lowest-cost
method (td_lcm_shard_*, the k_lcmsh_* kernels of csrc/td_lcm.hip, driven by taxidispatcher_amd/sharded.py lcm_sharded) that sit
on both sides of every constant those kernels and their launches branch on, of every kind of shard split, of the stop rules and
of the transport key's sentinels.  Plain numpy data and host references: nothing here needs a GPU.

A case is a dict: name, n, the input ("dense": an int32 matrix; "sparse": unique row-major coordinates (r, c, v), every other
cell = `fill`, never a candidate), `rule` (the keyword arguments of lcm_sharded: mask, threshold, stop_value_on, stop_value,
stop_size, sum_below, max_pairs), `splits` (each a list of (row0, nrows) that covers [0, n) in order; empty shards allowed
anywhere) and `claims`: the structural conditions that make it a case for its edge, which the CPU tier confirms from the
references alone.  References, never the code under test: lcm_expected (the oracle under the documented deviation) for dense
models, lcm_path_cases.sparse_greedy for sparse ones; a case taken over from lcm_path_cases keeps the reference it has there."""
import functools
import math

import numpy as np

import lcm_path_cases as L
from test_gpu_widths import lcm_expected

BIG = L.BIG
I32_MIN, I32_MAX = -2**31, 2**31 - 1

# ---- the constants the table sits on, each with the line of csrc/td_lcm.hip (or sharded.py) it restates
SCAN_STEP = 256          # lcm_scan_row: `for (int j0 = lane; j0 < n; j0 += 256)`
SCAN_LOAD = 64           # lcm_scan_row: `v[u] = (j0 + 64 * u < n) ? rp[j0 + 64 * u] : 0`, u < 4
MASK_WORD = 32           # `colmask[c >> 5] >> (c & 31)`; td_lcm_shard_create: `(n + 31) / 32 + 1` words
MIN_THREADS = 1024       # k_lcmsh_min: `<<<1, 1024>>>`, `for (int i = tid; i < nrows; i += 1024)`, `s_red[16]`
GRID_THREADS = 256       # k_lcmsh_colmin / _commit: `<<<(n + 255) / 256, 256>>>`; k_lcmsh_apply: `<<<(nrows + 255) / 256, 256>>>`
ROWS_PER_GROUP = 4       # k_lcmsh_init / _rescan / _rescan_masked: 256 threads = 4 waves, one row each
GROUPS_PER_CU = 8        # `std::min((nrows + 3) / 4, c.n_cu * 8)` workgroups: rows from 32 * n_cu on come from `row += gridDim.x * nw`
KEY_ROW_BIAS = 1         # transport key `(value << 32) | (global_row + 1)`: INT64_MIN / INT64_MAX are never a cell's key
LOCKSTEP_NMAX = 600      # (this module) the kernel-by-kernel comparison with the numpy model runs up to this n
BY_PICK_NMAX = 300       # (this module) above it the per-pick driver runs under a pair cap
BY_PICK_CAP = 200

RULE_KEYS = ("mask", "threshold", "stop_value_on", "stop_value", "stop_size", "sum_below", "max_pairs")


def make_rule(mask, threshold=-1, stop_value_on=0, stop_value=0, stop_size=-1, sum_below=2**62, max_pairs=None):
    return dict(mask=mask, threshold=threshold, stop_value_on=stop_value_on, stop_value=stop_value, stop_size=stop_size,
                sum_below=sum_below, max_pairs=max_pairs)


def simulator_rule(**over):
    """Simulator.java:523-549: cells >= big_cost are never looked at"""
    return make_rule(**dict(dict(mask=BIG, stop_value_on=1, stop_value=BIG, sum_below=BIG), **over))


def oracle_kw(rule):
    """oracle.lcm's arguments of a rule (as RULES of test_gpu_widths.py: the Java scan whenever a stop value is set)"""
    kw = {k: rule[k] for k in RULE_KEYS if k != "max_pairs"}
    kw["java_scan"] = 1 if rule["stop_value_on"] else 0
    if rule["max_pairs"] is not None:
        kw["max_iter"] = rule["max_pairs"]
    return kw


def lcm_args(rule):
    """positional arguments of dispatch._lcm after (n, c)"""
    return (rule["mask"], rule["threshold"], rule["stop_value_on"], rule["stop_value"], rule["stop_size"], rule["sum_below"],
            rule["max_pairs"])


# ======================================================================================================================
# shard splits
# ======================================================================================================================
def shard_bounds(n, world, rank):
    """sharded.shard_bounds restated: a uniform shard height, the trailing shards short or empty"""
    rps = (n + world - 1) // world
    row0 = min(n, rank * rps)
    return row0, max(0, min(rps, n - row0))


def bounds_split(n, world):
    return [shard_bounds(n, world, r) for r in range(world)]


def uneven_world(n):
    """the smallest world >= 3 that does not divide n"""
    return next(w for w in range(3, n + 3) if n % w)


def standard_splits(n):
    """one shard; a world that does not divide n; world = n + 3: one row per shard, three empty shards behind them"""
    return [[(0, n)], bounds_split(n, uneven_world(n)), bounds_split(n, n + 3)]


def covers(split, n):
    """shards in row order, contiguous, from 0 to n"""
    at = 0
    for row0, nrows in split:
        if row0 != at or nrows < 0:
            return False
        at += nrows
    return at == n


# ======================================================================================================================
# the table
# ======================================================================================================================
_BUILDERS = {}


def _add(name, fn):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = fn


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _case(n, inp, rule, splits, claims=(), reuse=None):
    d = dict(n=n, rule=rule, splits=[list(s) for s in splits], claims=tuple(claims), reuse=reuse)
    d.update(inp if isinstance(inp, dict) else {"input": "dense", "matrix": _i32(inp)})
    return d


def _from_cells(n, cells, fill=BIG):
    """dense matrix of {(row, col): value}, every other cell `fill`"""
    m = np.full((n, n), fill, np.int64)
    for (r, c), v in cells.items():
        assert 0 <= r < n and 0 <= c < n, (r, c, n)
        m[r, c] = v
    return m


# ---- the td_lcm table reused: every dense case of lcm_path_cases with n <= 257, under the reference it has there
REUSED_NMAX = 257
REUSED = tuple(m for m in L.LCM_NAMES if m.startswith(("edge_", "quarter_", "narrow_", "span", "lev", "lists_", "loop_")) and
               not m.startswith("loop_n"))       # (loop_n6049 ...: the large sparse models of the loop's LDS edges)


def _reused(name):
    def build():
        c = L.case(name)
        assert c["input"] == "dense" and c["n"] <= REUSED_NMAX, name
        kw = c["rule"][0]
        rule = make_rule(kw["mask"], kw.get("threshold", -1), kw.get("stop_value_on", 0), kw.get("stop_value", 0), kw.get("stop_size", -1),
                         kw.get("sum_below", 2**62), kw.get("max_pairs"))
        return _case(c["n"], c["matrix"], rule, standard_splits(c["n"]), [("reused", name)], reuse=name)
    return build


for _m in REUSED:
    _add("lcm_" + _m, _reused(_m))


# ---- lcm_scan_row: `j0 += 256`, four loads of stride 64.  Row 1 has its only cheap cell in column n - 1 and is the first pick;
# row 9 has the same value there, loses the column to row 1 and re-scans.  Rows 2, 5 and 7 repeat their minimum at columns 0, 64
# and 256 (where n has them): row 2 is taken at 0; row 5, with column 0 gone, moves to the next repeat that is still free, row 7
# to the one after that; a row whose repeats are all gone falls back to a dearer cell near the end of the row.
def _background(rng, n, rows, cols, lo, hi, per_row=3):
    cells = {}
    for r in rows:
        for c in rng.choice(cols, per_row, replace=False):
            cells[(r, int(c))] = int(rng.integers(lo, hi + 1))
    return cells


def _scan(n):
    def build():
        rng = np.random.default_rng(1100 + n)
        rep = [c for c in (0, SCAN_LOAD, SCAN_STEP) if c < n]
        free = [c for c in rep if c != n - 1]      # row 1 takes column n - 1 before anything else
        cells = _background(rng, n, range(12, 32), [c for c in range(6, n - 5) if c not in rep], 30, 60)
        cells[(1, n - 1)] = 1
        for c in range(1, 6):
            cells[(1, c)] = 9                      # dearer cells in front of the row's minimum
        cells[(9, n - 1)], cells[(9, n - 4)] = 1, 22
        for row, val, back_col, back_val in ((2, 3, None, None), (5, 4, n - 2, 20), (7, 6, n - 3, 21)):
            for c in rep:
                cells[(row, c)] = val
            if back_col is not None:
                cells[(row, back_col)] = back_val
        claims = [("first", 1, n - 1), ("last_col", 1), ("rescan", 9, n - 1, n - 4), ("repeat", 2, tuple(rep)), ("takes", 2, 0),
                  ("rescan", 5, 0, free[1] if len(free) > 1 else n - 2), ("rescan", 7, 0, free[2] if len(free) > 2 else n - 3)]
        return _case(n, _from_cells(n, cells), simulator_rule(), standard_splits(n), claims)
    return build


SCAN_NS = (63, 64, 65, 255, 256, 257, 513)
for _n in SCAN_NS:
    _add("scan_n%d" % _n, _scan(_n))


# ---- the column mask's words: a pick in the last column of word 0 (30 at n = 31, else 31) and in the first of word 1 (32) each
# forces the re-scan of a row whose cached column it was.  Every cell is a candidate, so every row is taken.
def _maskword(n):
    def build():
        rng = np.random.default_rng(1200 + n)
        m = rng.integers(10, 41, (n, n))
        claims = []
        for k, e in enumerate(c for c in (MASK_WORD - 2, MASK_WORD - 1, MASK_WORD) if c < n):
            taker, loser = 2 * k, 2 * k + 1
            m[taker, e], m[loser, e] = 1 + k, 5 + k
            claims += [("takes", taker, e), ("rescan", loser, e, None)]
        return _case(n, m, make_rule(100), standard_splits(n) + [[(0, 1), (1, n - 1)]], claims)
    return build


MASKWORD_NS = (31, 32, 33)
for _n in MASKWORD_NS:
    _add("maskword_n%d" % _n, _maskword(_n))


# ---- permutation bands: one candidate per row and column (row i, column (mul * i + 3) mod n), so the round driver takes them all
# in ONE round; the picks' order is by value, then row
def band_cols(n):
    mul = next(m for m in (7, 11, 13, 17, 19, 23) if math.gcd(m, n) == 1)
    return (mul * np.arange(n, dtype=np.int64) + 3) % n


def _sparse_input(n, r, c, v, fill=BIG):
    r, c, v = (np.asarray(a, np.int64) for a in (r, c, v))
    order = np.argsort(r * n + c, kind="stable")
    key = (r * n + c)[order]
    assert (np.diff(key) > 0).all(), "coordinates must be unique"
    return {"input": "sparse", "coords": (_i32(r[order]), _i32(c[order]), _i32(v[order])), "fill": fill}


# ---- k_lcmsh_min: 1024 threads, `i += 1024`, 16 partial minima.  One shard of n rows; the global minimum sits in local rows 0,
# 1024 (the same value as row 0: the same thread's second row, the lower row wins), 1023 and n - 1 in turn; n = 2049 adds a tie
# between rows 1000 and 2024.
def _kmin(n):
    def build():
        cols = band_cols(n)
        vals = np.arange(n, dtype=np.int64) % 7
        special = {0: -8, n - 1: -6}
        if n > MIN_THREADS:
            special[MIN_THREADS] = -8
        if n > MIN_THREADS - 1:
            special.setdefault(MIN_THREADS - 1, -7)
        if n > 2 * MIN_THREADS:
            special[1000], special[1000 + MIN_THREADS] = -5, -5
        for r, v in special.items():
            vals[r] = v
        first = sorted(special, key=lambda r: (special[r], r))
        claims = [("band",), ("rounds", 1), ("picks", 0, tuple((r, int(cols[r])) for r in first)), ("rows", n)]
        splits = [[(0, n)]] + ([[(0, MIN_THREADS), (MIN_THREADS, n - MIN_THREADS)]] if n > MIN_THREADS else [])
        return _case(n, _sparse_input(n, np.arange(n), cols, vals), simulator_rule(), splits, claims)
    return build


KMIN_NS = (MIN_THREADS - 1, MIN_THREADS, MIN_THREADS + 1, 2 * MIN_THREADS + 1)
for _n in KMIN_NS:
    _add("kmin_n%d" % _n, _kmin(_n))


# ---- the 256-thread grids of k_lcmsh_colmin / _commit (one thread per column) and k_lcmsh_apply (one per local row): the
# dominant cell of the whole model in the last column and the last local row, 255 (one workgroup) / 256 (the second one's first
# thread); row 100 caches that column too and re-scans
def _grid(n):
    def build():
        rng = np.random.default_rng(1300 + n)
        cells = _background(rng, n, range(10, 40), list(range(8, n - 1)), 30, 60)
        cells[(n - 1, n - 1)] = 0
        cells[(100, n - 1)], cells[(100, 7)] = 1, 20
        claims = [("first", n - 1, n - 1), ("rescan", 100, n - 1, 7), ("local_row", n - 1)]
        return _case(n, _from_cells(n, cells), simulator_rule(), standard_splits(n)[:2] + [[(0, 1), (1, n - 1)]], claims)
    return build


GRID_NS = (GRID_THREADS, GRID_THREADS + 1)
for _n in GRID_NS:
    _add("grid_n%d" % _n, _grid(_n))


# ---- grid-stride rows: n = 32 n_cu + 64, so the last 64 rows are reached only by `row += gridDim.x * nw` in k_lcmsh_init,
# k_lcmsh_rescan and k_lcmsh_rescan_masked.  A permutation band with values i % 7, except that the first 64 rows' band cells are
# -3 and the stride rows' are -1; stride row 32 n_cu + k also has a cheaper cell (-2) in the band column of row k, which row k
# takes first: every stride row must be scanned at the start (its cached column is row k's) and re-scanned after row k's pick.
STRIDE_TAIL = 64


def stride_n(n_cu):
    return ROWS_PER_GROUP * GROUPS_PER_CU * n_cu + STRIDE_TAIL


@functools.lru_cache(maxsize=2)
def stride_case(n_cu):
    """the grid-stride model for a device of n_cu compute units (the table's own entry is the stand-in n_cu = 2)"""
    n = stride_n(n_cu)
    first = n - STRIDE_TAIL
    cols = band_cols(n)
    i = np.arange(n, dtype=np.int64)
    vals = i % 7
    vals[:STRIDE_TAIL] = -3
    vals[first:] = -1
    k = np.arange(STRIDE_TAIL)
    inp = _sparse_input(n, np.concatenate([i, first + k]), np.concatenate([cols, cols[k]]),
                        np.concatenate([vals, np.full(STRIDE_TAIL, -2)]))
    order = [(int(a), int(cols[a])) for a in k] + [(int(first + a), int(cols[first + a])) for a in k]
    claims = [("rounds", 2), ("picks", 0, tuple(order)), ("rows", n), ("stride", n_cu)]
    claims += [("rescan", first + a, int(cols[a]), int(cols[first + a])) for a in (0, 7, STRIDE_TAIL - 1)]
    d = _case(n, inp, simulator_rule(), [[(0, n)], [(0, first + 8), (first + 8, STRIDE_TAIL - 8)]], claims)
    d["name"] = "stride_ncu%d" % n_cu
    d["n_cu"] = n_cu
    for a in d["coords"]:
        a.setflags(write=False)
    return d


_add("stride_standin", lambda: stride_case(2))


# ---- ties across a shard boundary: the model's smallest value in row 4 (the last row of a shard) and in row 5 (the first row of
# the next shard that has any), in one column (row 4 takes it, row 5 re-scans) or in two (both go in the first round, listed by
# row).  Splits with a one-row and an empty shard in the middle.
TIE_N = 12
TIE_SPLITS = ([(0, TIE_N)], [(0, 5), (5, 7)], [(0, 5), (5, 0), (5, 1), (6, 0), (6, 6)], [(0, 0), (0, 5), (5, 0), (5, 0), (5, 7)],
              bounds_split(TIE_N, TIE_N + 3))


def _tie(same_col):
    def build():
        m = np.random.default_rng(1400 + same_col).integers(1, 41, (TIE_N, TIE_N))
        c2 = 3 if same_col else 7
        m[4, 3] = m[5, c2] = -5
        m[5, 9] = -4 if same_col else m[5, 9]      # where row 5 goes once column 3 is gone
        claims = [("tie", (4, 3), (5, c2)), ("boundary", 4), ("first", 4, 3)]
        claims += [("rescan", 5, 3, 9)] if same_col else [("picks", 0, ((4, 3), (5, 7))), ("dominant", 4, 3), ("dominant", 5, 7)]
        return _case(TIE_N, m, make_rule(100), TIE_SPLITS, claims)
    return build


_add("tie_same_col", _tie(1))
_add("tie_two_cols", _tie(0))


# ---- the stop rules side by side, on one 96 x 96 model with negative values: a third of the cells and the last 26 columns are
# BIG, so at most 70 rows can be taken and a rule that takes all it can runs out of candidates
RULES_N = 96


@functools.lru_cache(maxsize=None)
def rules_matrix():
    rng = np.random.default_rng(1500)
    m = rng.integers(-40, 61, (RULES_N, RULES_N))
    m[rng.random((RULES_N, RULES_N)) < 0.33] = BIG
    m[:, 70:] = BIG
    m[11, 13], m[60, 2] = -40, 60        # both ends of the candidate range are there
    m = _i32(m)
    m.setflags(write=False)
    return m


def _natural(rule):
    return int(lcm_expected(rules_matrix(), oracle_kw(rule))[1].size)


def _rules(maker, *claims):
    def build():
        rule = maker()
        return _case(RULES_N, rules_matrix(), rule, standard_splits(RULES_N), [("rule",)] + list(claims))
    return build


def _sim_sized(delta):
    """the size stop at the natural pick count + delta (never reached / the last pick / one pick early)"""
    natural = _natural(simulator_rule())
    return simulator_rule(stop_size=RULES_N - (natural + delta))


def _capped(delta):
    return make_rule(BIG, threshold=60, sum_below=BIG, max_pairs=_natural(make_rule(BIG, threshold=60, sum_below=BIG)) + delta)


_add("rule_threshold_0", _rules(lambda: make_rule(BIG, threshold=0, sum_below=BIG), ("last_min_above", 0)))
_add("rule_threshold_max", _rules(lambda: make_rule(BIG, threshold=60, sum_below=BIG), ("last_min", BIG)))       # the largest candidate
_add("rule_threshold_max-1", _rules(lambda: make_rule(BIG, threshold=59, sum_below=BIG), ("last_min_in", 60, BIG)))
_add("rule_sim_size_0", _rules(lambda: simulator_rule(stop_size=0), ("last_min", BIG), ("ran_out",)))
_add("rule_sim_size_n-1", _rules(lambda: simulator_rule(stop_size=RULES_N - 1), ("npairs", 1)))
_add("rule_sim_size_natural+1", _rules(lambda: _sim_sized(1), ("last_min", BIG), ("ran_out",)))
_add("rule_sim_size_natural", _rules(lambda: _sim_sized(0), ("size_stop", 0)))
_add("rule_sim_size_natural-1", _rules(lambda: _sim_sized(-1), ("size_stop", -1)))
_add("rule_cap_0", _rules(lambda: make_rule(BIG, threshold=60, sum_below=BIG, max_pairs=0), ("npairs", 0)))
_add("rule_cap_1", _rules(lambda: make_rule(BIG, threshold=60, sum_below=BIG, max_pairs=1), ("npairs", 1)))
_add("rule_cap_natural-1", _rules(lambda: _capped(-1), ("capped",)))
_add("rule_sum_below_-35", _rules(lambda: simulator_rule(sum_below=-35), ("sum_below", -35)))     # inside the picks' range
_add("rule_mask_runs_out", _rules(lambda: make_rule(BIG), ("last_min", BIG), ("ran_out",)))     # no stop value: last_min = mask
_add("rule_live_cell_above_mask", _rules(lambda: make_rule(50), ("last_min_in", 50, BIG), ("deviation",)))


# ---- int32 extremes: mask 2^31 - 1 and no stop value, so every cell is a candidate; -2^31 in global row 0 (value << 32 with a
# zero low word would be INT64_MIN, the "not taken" sentinel: the reason for KEY_ROW_BIAS), in another row of shard 0, in the
# first row of a later shard
EXT_N = 7
EXT_VALUES = (I32_MIN, I32_MIN + 1, -1, 0, I32_MAX - 1)
EXT_SPLITS = ([(0, EXT_N)], [(0, 3), (3, 4)], [(0, 3), (3, 0), (3, 1), (4, 3)], bounds_split(EXT_N, EXT_N + 3))


def _extreme(row, col):
    def build():
        m = np.random.default_rng(1600 + row).choice(np.array(EXT_VALUES[1:], np.int64), (EXT_N, EXT_N))
        m[row, col] = I32_MIN
        return _case(EXT_N, m, make_rule(I32_MAX), EXT_SPLITS, [("first", row, col), ("int32_min", row, col), ("values", EXT_VALUES)])
    return build


_add("ext_min_row0", _extreme(0, 4))
_add("ext_min_row1", _extreme(1, 2))
_add("ext_min_row3", _extreme(3, 5))
# the model the sentinel was found on: with `(value << 32) | global_row` as the key the round driver dropped the pick (0, 1) and
# returned (4, [2, 1], [2, 0], -2147483648)
SENTINEL_BEFORE_FIX = (4, [2, 1], [2, 0], -2147483648)
_add("ext_sentinel_3x3", lambda: _case(3, [[5, I32_MIN, 7], [3, 4, 9], [8, 2, 1]], make_rule(100), [[(0, 3)], [(0, 2), (2, 1)], bounds_split(3, 6)],
                                       [("first", 0, 1), ("int32_min", 0, 1), ("result", (I32_MIN + 4, (0, 2, 1), (1, 2, 0), 3))]))

CASE_NAMES = tuple(_BUILDERS)

# both sides of every edge of the table
EDGES = {
    "scan load 63/64/65 columns": ("scan_n63", "scan_n64", "scan_n65"),
    "scan step 255/256/257 columns": ("scan_n255", "scan_n256", "scan_n257"),
    "scan third step": ("scan_n257", "scan_n513"),
    "mask word 31/32/33": ("maskword_n31", "maskword_n32", "maskword_n33"),
    "k_lcmsh_min 1023/1024/1025 rows": ("kmin_n1023", "kmin_n1024", "kmin_n1025"),
    "k_lcmsh_min third stride": ("kmin_n1025", "kmin_n2049"),
    "grid 256/257": ("grid_n256", "grid_n257"),
    "grid-stride rows": ("grid_n257", "stride_standin"),
    "tie on a boundary": ("tie_same_col", "tie_two_cols"),
    "threshold": ("rule_threshold_0", "rule_threshold_max-1", "rule_threshold_max"),
    "size stop": ("rule_sim_size_0", "rule_sim_size_n-1", "rule_sim_size_natural-1", "rule_sim_size_natural", "rule_sim_size_natural+1"),
    "pair cap": ("rule_cap_0", "rule_cap_1", "rule_cap_natural-1"),
    "sum_below": ("rule_sum_below_-35", "rule_sim_size_0"),
    "last_min": ("rule_mask_runs_out", "rule_live_cell_above_mask"),
    "INT32_MIN row": ("ext_min_row0", "ext_min_row1", "ext_min_row3", "ext_sentinel_3x3"),
}


@functools.lru_cache(maxsize=None)
def case(name):
    d = dict(_BUILDERS[name](), name=name)
    if d.get("matrix") is not None and d["matrix"].flags.writeable:
        d["matrix"].setflags(write=False)
    for a in d.get("coords", ()):
        a.setflags(write=False)
    return d


def dense_matrix(c):
    """the int32 matrix of a case (the CPU tier and the numpy model; a sparse case only where it stays small)"""
    if c["input"] == "dense":
        return c["matrix"]
    assert c["n"] <= L.DENSE_MAX
    m = np.full((c["n"], c["n"]), c["fill"], np.int32)
    r, cc, v = c["coords"]
    m[r, cc] = v
    return m


def _reference_of(c, rule):
    if c["input"] == "dense":
        t, r, cc, lm = lcm_expected(c["matrix"], oracle_kw(rule))
    else:
        t, r, cc, lm = L.sparse_greedy(c["n"], *c["coords"], rule, c["fill"])
    return int(t), np.asarray(r).tolist(), np.asarray(cc).tolist(), int(lm)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(total, rows, cols, last_min) as ints / lists, computed once per process"""
    c = case(name)
    if c["reuse"]:
        return L.reference(c["reuse"])
    return _reference_of(c, c["rule"])


def capped_rule(c, cap):
    """the case's rule under a pair cap (the per-pick driver on the large cases)"""
    mp = c["rule"]["max_pairs"]
    return dict(c["rule"], max_pairs=cap if mp is None else min(mp, cap))


@functools.lru_cache(maxsize=None)
def reference_capped(name, cap):
    c = case(name)
    return _reference_of(c, capped_rule(c, cap))


def stride_reference(c):
    """reference of a stride_case(n_cu) dict (not in the table: its size follows the device)"""
    return _reference_of(c, c["rule"])
