"""The case table of tests/test_lcm_paths_cpu.py and tests/test_gpu_lcm_paths.py: td_lcm and td_pool2 inputs that sit on both
sides of every constant by which csrc/td_lcm.hip chooses a path, a kernel, a chunk or a copy route (DESIGN.md section 3 has the
table).  Plain numpy data, generators and host references: nothing here needs a GPU.

A case is a dict: name, kind ("lcm" / "pool2"), n, the input, the stop rule, where the outputs go, the `lcm_path` bits
(td_last_stats word 11) the call must show, and `claims`: the structural conditions that make it a case for its edge, which the
CPU tier confirms by the references alone so that the table cannot drift into cases that test nothing.

An LCM input is one of
    "dense"   an int32 matrix (n <= DENSE_MAX);
    "sparse"  coordinates (r, c, v), unique and in row-major order, every other cell = `fill` (never a candidate): the GPU test
              builds the matrix on the device, the CPU tier never allocates it beyond DENSE_MAX;
    "count"   the closed-form full matrix of count_model(n).
References, never the code under test: the oracle (with lcm_expected of test_gpu_widths.py) for the dense cases, sparse_greedy
(checked against the oracle on every dense case the oracle can reach) for the sparse ones, count_expected for the closed form,
pool2_reference (checked against OracleBackend.find_pool) for td_pool2.  CASE_NAMES is the static list the tests are
parametrised over; case(name) builds on first use, reference(name) is computed once per process and shared (read-only)."""
import functools

import numpy as np

from oracle import oracle
from test_gpu_widths import RULES, lcm_expected

BIG = 250000
I32_MAX = 2**31 - 1

# ---- the thresholds the table sits on, each with the line of csrc/td_lcm.hip it restates
LISTS_NMIN = 64          # lcm_impl / td_pool2: `if (g_lcm_lists && n >= 64 && n <= 65536)`
NARROW_NMIN = 128        # lcm_impl / td_pool2: `const bool narrow = n >= 128`
NARROW_PITCH = 16        # `const int pitch = ((n + 15) / 16) * 16`
NARROW_TOP = 255         # k_lcm_narrow: `d >= 0 && d < 255` -> exact code, otherwise 255 (lcm_scan_narrow: `code < 255u`)
LV_MAX = 256             # `constexpr int LV_MAX = 256`: lists while `(int64_t)info.vmax - info.vmin < LV_MAX`
BALLOT_LEVELS = 16       # k_lcms_rows / k_lcms_rows4: `if (nlev <= 16)` one ballot per level
ROWS4_NMAX = 4096        # lcm_impl: `if (n <= 4096)` k_lcms_rows4, else k_lcms_rows; td_pool2 always k_lcms_rows
ROWS_BLOCK = 1024        # k_lcms_rows: `jb += 64 * LCH` with LCH = 16
CHUNK = 1024             # k_lcms_greedy: `const int base = sbase + q * 1024`
SKIP_BLOCK = 4096        # k_lcms_greedy: `sbase += 4096`, `__syncthreads_or(any4)`
SCAN_TILE = 8 * 1024     # k_lcms_scan: `base += 1024 * CH` with CH = 8
HASH_SIZE = 16384        # `while (hsz < n && hsz < 16384) hsz <<= 1`
COUNT_MAX = 1 << 28      # `info.count <= (1ll << 28)`
LDS_DEFAULT = 48 * 1024  # `if (shm > 48 * 1024) hipFuncSetAttribute(...)`
LDS_ROWKEYS = 96 * 1024  # `rb_in_lds = ((size_t)n * 8 + shm_mask) <= 96 * 1024`
PINNED_CAP = 1 << 16     # td_core.hip: `c.pinned_cap = 1 << 16`
PINNED_OFF = 8192        # `via_pinned = ... (size_t)8192 + sizeof(int32_t) * 2 * (size_t)n <= c.pinned_cap`
DENSE_MAX = 3000         # (this module) largest n whose matrix the CPU tier builds

# ---- td_last_stats word 11 (include/taxidispatcher_amd.h)
LISTS, ROWS4, NARROW, RB_LDS, HINTED, REDONE, PINNED, POOL2 = 1, 2, 4, 8, 16, 32, 64, 128


def loop_lds(n):
    """k_lcm_loop's dynamic LDS with the row keys in it: 8 n + 4 ceil(n / 32)"""
    return 8 * n + 4 * ((n + 31) // 32)


def greedy_lds(n):
    """k_lcms_greedy's dynamic LDS: 8 hsz + 8 ceil(n / 32)"""
    hsz = 64
    while hsz < n and hsz < HASH_SIZE:
        hsz <<= 1
    return 8 * hsz + 8 * ((n + 31) // 32)


def rows4_quarter(n):
    """k_lcms_rows4: `q = (((n + 3) / 4) + 63) / 64 * 64` columns per wave"""
    return ((n + 3) // 4 + 63) // 64 * 64


def expected_bits(kind, n, count, vmin, vmax, host_out):
    """lcm_impl's / td_pool2's decisions restated from the constants above"""
    bits = POOL2 if kind == "pool2" else 0
    if LISTS_NMIN <= n <= 65536 and 0 < count <= COUNT_MAX and vmax - vmin < LV_MAX:
        bits |= LISTS | (ROWS4 if kind == "lcm" and n <= ROWS4_NMAX else 0)
    else:
        bits |= (NARROW if n >= NARROW_NMIN else 0) | (RB_LDS if loop_lds(n) <= LDS_ROWKEYS else 0)
    if kind == "lcm" and host_out and PINNED_OFF + 8 * n <= PINNED_CAP:
        bits |= PINNED
    return bits


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def rule(name, max_pairs=None, **over):
    """(td_lcm arguments, oracle.lcm arguments) of one of RULES (test_gpu_widths.py), with overrides"""
    kw_gpu, kw_oracle = (dict(d, **over) for d in RULES[name])
    if max_pairs is not None:
        kw_gpu["max_pairs"], kw_oracle["max_iter"] = max_pairs, max_pairs
    return kw_gpu, kw_oracle


def lcm_args(kw_gpu):
    """positional arguments of dispatch._lcm after (n, c)"""
    return (kw_gpu["mask"], kw_gpu.get("threshold", -1), kw_gpu.get("stop_value_on", 0), kw_gpu.get("stop_value", 0),
            kw_gpu.get("stop_size", -1), kw_gpu.get("sum_below", 2**62), kw_gpu.get("max_pairs"))


def candidate_hi(kw_gpu):
    """lcm_impl: `hi = min(cand_limit - 1, mask - 1)`, `min(hi, threshold)` when threshold >= 0"""
    hi = kw_gpu["mask"] - 1
    if kw_gpu.get("stop_value_on", 0):
        hi = min(hi, kw_gpu["stop_value"] - 1)
    if kw_gpu.get("threshold", -1) >= 0:
        hi = min(hi, kw_gpu["threshold"])
    return hi


# ======================================================================================================================
# references
# ======================================================================================================================
def sparse_greedy(n, r, c, v, kw_gpu, fill=BIG):
    """The lowest-cost method on a coordinate list (moved here from test_gpu_parity.py's _sorted_cell_greedy and extended by
    last_min and the stop rules): the candidate cells in (value, row, col) order, each taken when its row and column are free
    -- what repeated first-minimum + masking does (greedy_opt.py:61-82, Simulator.java:523-549).  Every cell outside the list
    is `fill`, which must not be a candidate and must be >= mask, so that once the candidates run out with picks still allowed
    the next minimum the reference reads is the mask / stop value.  Returns (total, rows, cols, last_min)."""
    hi = candidate_hi(kw_gpu)
    mask, sum_below = kw_gpu["mask"], kw_gpu.get("sum_below", 2**62)
    stop_size, cap = kw_gpu.get("stop_size", -1), kw_gpu.get("max_pairs")
    assert fill > hi and fill >= mask
    limit = n if cap is None else min(n, cap)
    if 0 <= stop_size < n:
        limit = min(limit, n - stop_size)
    r, c, v = (np.asarray(a, np.int64) for a in (r, c, v))
    keep = v <= hi
    r, c, v = r[keep], c[keep], v[keep]
    order = np.lexsort((c, r, v))
    r, c, v = r[order], c[order], v[order]
    rt, ct = np.zeros(n, bool), np.zeros(n, bool)
    rows, cols, tot, last = [], [], 0, kw_gpu.get("stop_value", 0)
    for s in range(0, r.size, 8192):
        if len(rows) >= limit:
            break
        rr, cc, vv = r[s:s + 8192], c[s:s + 8192], v[s:s + 8192]
        for k in np.nonzero(~(rt[rr] | ct[cc]))[0]:
            a, b = int(rr[k]), int(cc[k])
            if rt[a] or ct[b]:
                continue
            if len(rows) >= limit:
                break
            rt[a] = ct[b] = True
            rows.append(a)
            cols.append(b)
            last = int(vv[k])
            tot += last if last < sum_below else 0
    if len(rows) < limit:   # the candidates ran out with picks still allowed
        assert kw_gpu.get("stop_value_on", 0) or kw_gpu.get("threshold", -1) >= 0 or len(rows) == n, "heuristic rule: use the oracle"
        last = kw_gpu["stop_value"] if kw_gpu.get("stop_value_on", 0) else mask
    return tot, np.array(rows, np.int32), np.array(cols, np.int32), last


def pool_costs(frm, to, dist):
    """pair costs and plans of Simulator.java:693-699 (k_pool2_cost), int64 [A][B]; dist None: the line |a - b|"""
    frm, to = np.asarray(frm, np.int64), np.asarray(to, np.int64)
    d = (lambda a, b: np.abs(a - b)) if dist is None else (lambda a, b: np.asarray(dist, np.int64)[a, b])
    af, at, bf, bt = frm[:, None], to[:, None], frm[None, :], to[None, :]
    z = np.zeros((frm.size, frm.size), np.int64)
    af, at, bf, bt = af + z, at + z, bf + z, bt + z
    head = d(af, bf)
    cost1 = head + d(bf, at) + d(at, bt)
    cost2 = head + d(bf, bt) + d(bt, at)
    return np.where(cost1 < cost2, cost1, cost2).astype(np.int32), (cost1 < cost2).astype(np.int8)


@functools.lru_cache(maxsize=None)
def case_pool_costs(name):
    c = case(name)
    return pool_costs(c["frm"], c["to"], c["dist"])


def pool2_reference(frm, to, dist=None, by_level=False, costs=None):
    """Simulator.java:681-758 restated (as OracleBackend.find_pool of sim_backend.py, here also for a distance table): every
    ordered pair A != B, stable order by cost (insertion order A-major, then B), a pair kept iff both customers are free;
    ends once n // 2 pairs are kept.  by_level walks the cost values in ascending order instead of sorting all pairs (the
    same order: one value's pairs in row-major order), which ends early on a large n with few levels."""
    cost, plan = pool_costs(frm, to, dist) if costs is None else costs
    n = cost.shape[0]
    off = ~np.eye(n, dtype=bool)
    used, out = np.zeros(n, bool), []

    def walk(a, b):
        for s in range(0, a.size, 8192):
            aa, bb = a[s:s + 8192], b[s:s + 8192]
            for k in np.nonzero(~(used[aa] | used[bb]))[0]:
                ai, bi = int(aa[k]), int(bb[k])
                if used[ai] or used[bi]:
                    continue
                used[ai] = used[bi] = True
                out.append((ai, bi, int(plan[ai, bi]), int(cost[ai, bi])))
            if len(out) >= n // 2:
                return True
        return len(out) >= n // 2

    if by_level:
        flat = np.where(off, cost, -1).ravel()   # pair costs are distances: never negative
        assert int(cost[off].min()) >= 0
        for val in np.unique(flat)[1:]:
            if walk(*np.divmod(np.flatnonzero(flat == val), n)):
                break
    else:
        a, b = np.nonzero(off)
        order = np.argsort(cost[a, b], kind="stable")
        walk(a[order], b[order])
    return out


# ---- the count edge: a full matrix with a closed-form answer
COUNT_M = 3


def count_model(n):
    """zeros on a permutation of all rows and columns but COUNT_M of each; every other cell 1 + ((7 i + 3 j) mod 5).
    Returns (rows without a zero, columns without a zero, zero rows, zero columns)."""
    miss_r = np.array([2, n // 2 + 1, n - 1])
    miss_c = np.array([0, n // 3, n - 2])
    zr = np.setdiff1d(np.arange(n), miss_r)
    zc = np.roll(np.setdiff1d(np.arange(n), miss_c), -(n // 5))
    return miss_r, miss_c, zr, zc


def count_cell(i, j):
    return 1 + (7 * i + 3 * j) % 5


def count_matrix(n, xp=np, **kw):
    """the matrix itself; xp = numpy (small n) or torch with device=... (the GPU test)"""
    _, _, zr, zc = count_model(n)
    i = xp.arange(n, dtype=xp.int32, **kw)[:, None]
    j = xp.arange(n, dtype=xp.int32, **kw)[None, :]
    c = (7 * i + 3 * j) % 5 + 1
    if xp is np:
        c = c.astype(np.int32)
        c[zr, zc] = 0
    else:
        c[xp.as_tensor(zr, **kw), xp.as_tensor(zc, **kw)] = 0
    return c


def count_expected(n, kw_oracle):
    """the zero cells in row order, then the oracle's greedy on the COUNT_M x COUNT_M remainder mapped back (the order by
    (value, row, col) survives taking a submatrix); the rule takes every cell, so last_min is the last pick's value"""
    miss_r, miss_c, zr, zc = count_model(n)
    sub = _i32(count_cell(miss_r[:, None], miss_c[None, :]))
    t, r, c, lm = oracle.lcm(sub, **kw_oracle)
    assert r.size == COUNT_M
    return t, np.concatenate([zr, miss_r[r]]).astype(np.int32), np.concatenate([zc, miss_c[c]]).astype(np.int32), lm


# ======================================================================================================================
# the table
# ======================================================================================================================
_BUILDERS = {}


def _add(name, fn):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = fn


def _sparse_input(n, r, c, v, fill=BIG):
    """unique coordinates in row-major order; of a repeated coordinate the first one given stays"""
    r, c, v = (np.asarray(a, np.int64) for a in (r, c, v))
    assert r.min() >= 0 and c.min() >= 0 and r.max() < n and c.max() < n
    _, first = np.unique(r * n + c, return_index=True)
    return {"input": "sparse", "coords": (_i32(r[first]), _i32(c[first]), _i32(v[first])), "fill": fill}


def _rand_cells(seed, n, per_row, lo, hi):
    rng = np.random.default_rng(seed)
    k = per_row * n
    return np.repeat(np.arange(n), per_row), rng.integers(0, n, k), rng.integers(lo, hi + 1, k)


def _lcm_case(n, inp, rl, bits, claims=(), out="host"):
    d = dict(kind="lcm", n=n, rule=rl, bits=bits, claims=tuple(claims), out=out)
    d.update(inp if isinstance(inp, dict) else {"input": "dense", "matrix": _i32(inp)})
    return d


def _dense(seed, n, lo, hi, ends=True):
    c = np.random.default_rng(seed).integers(lo, hi + 1, (n, n))
    if ends:   # both ends of the range are present
        c[n // 3, n // 2], c[n // 2, n // 3] = lo, hi
    return c


# ---- n = 63 / 64: the loop only / the level lists; rows4 quarter edges 64, 65, 256, 257 (waves 1..3 own no column, one, a chunk)
def _small_n(n, rname):
    def build():
        rl = rule(rname)
        bits = (LISTS | ROWS4 if n >= LISTS_NMIN else RB_LDS) | PINNED
        return _lcm_case(n, _dense(100 + n, n, 1, 14), rl, bits, [("quarters",)] if rname == "heuristic" else [])
    return build


_add("edge_n63", _small_n(63, "greedy_opt"))
_add("edge_n64", _small_n(64, "greedy_opt"))
for _n in (64, 65, 256, 257):
    _add("quarter_n%d" % _n, _small_n(_n, "heuristic"))   # every row and column is taken: a wrong cell in any column shows


# ---- narrow codes: a wide-valued model (the loop) around n = 128 and the pitch of 16.  Row 1 is re-scanned after the first
# pick; its surviving minimum sits at base + 254 (exact code) or base + 255 (code 255: the int32 scan), in the last column,
# behind dearer cells that a saturating code would confuse with it, and the greedy does take it there: the last column is
# dear for every other row, and the size stop is 0, so every row is taken.  Row 2's free columns are all >= base + 255.
def _narrow(n, delta):
    def build():
        rng = np.random.default_rng(200 + n)
        c = rng.integers(3, 2001, (n, n))     # codes below and above 255 everywhere: both scans answer re-scans
        c[:, n - 1] = rng.integers(1500, 2001, n)
        c[0, 5] = 0                           # base = the global first minimum; picked first
        c[1] = rng.integers(300, 2001, n)
        c[1, 5], c[1, n - 1] = 1, delta
        c[2] = rng.integers(NARROW_TOP, 401, n)
        c[2, 5] = 2
        bits = (NARROW if n >= NARROW_NMIN else 0) | RB_LDS | PINNED
        return _lcm_case(n, c, rule("simulator", stop_size=0), bits, [("rescan", 1, delta), ("all255", 2), ("takes", 1, n - 1), ("takes_row", 2)])
    return build


for _n in (127, 128, 129, 143, 144, 145):
    for _d in (NARROW_TOP - 1, NARROW_TOP):
        _add("narrow_n%d_d%d" % (_n, _d), _narrow(_n, _d))


# ---- LV_MAX: candidate range 255 (lists, 256 levels) / 256 (loop), also from a negative minimum
def _span(span, lo):
    def build():
        bits = (LISTS | ROWS4 if span < LV_MAX else RB_LDS) | PINNED
        return _lcm_case(100, _dense(300 + span + (lo < 0), 100, lo, lo + span), rule("simulator"), bits, [("span", span, lo)])
    return build


for _s in (LV_MAX - 1, LV_MAX):
    _add("span%d" % _s, _span(_s, 7))
    _add("span%d_neg" % _s, _span(_s, -100))


# ---- nlev 16 / 17 in k_lcms_rows4 (k_lcms_rows: the n = 4097 cases and td_pool2 below)
def _levels(nlev, lo):
    def build():
        return _lcm_case(200, _dense(400 + nlev + (lo < 0), 200, lo, lo + nlev - 1), rule("heuristic"), LISTS | ROWS4 | PINNED,
                         [("span", nlev - 1, lo)])
    return build


_add("lev16", _levels(BALLOT_LEVELS, 1))
_add("lev17", _levels(BALLOT_LEVELS + 1, 1))
_add("lev16_neg", _levels(BALLOT_LEVELS, -9))
_add("lev17_neg", _levels(BALLOT_LEVELS + 1, -9))


# ---- every stop rule on both paths, pair caps, device outputs
def _tick_like(seed, n):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 50, n), rng.integers(0, 50, n)
    c = np.abs(a[:, None] - b[None, :])
    c[c >= 10] = BIG
    c[:, int(0.7 * n):] = BIG
    return c


_RULE_MODELS = {   # path, rule -> (matrix, rule overrides)
    ("lists", "heuristic"): lambda: (_dense(500, 150, 1, 39), {}),
    ("lists", "greedy_opt"): lambda: (_dense(501, 150, 0, 29), {}),
    ("lists", "simulator"): lambda: (_tick_like(502, 150), dict(stop_size=60)),
    ("loop", "heuristic"): lambda: (_dense(503, 150, -400, 99), {}),
    ("loop", "greedy_opt"): lambda: (_dense(504, 150, -400, 30), {}),
    ("loop", "simulator"): lambda: (np.where(_dense(505, 150, 0, 600) % 7 == 0, BIG, _dense(505, 150, 0, 600)), {}),
}


def _ruled(path, rname, cap=None, out="host"):
    def build():
        c, over = _RULE_MODELS[(path, rname)]()
        base = rule(rname, **over)
        natural = lcm_expected(_i32(c), base[1])[1].size
        mp = None if cap is None else (natural - 1 if cap == "natural-1" else cap)
        bits = (LISTS | ROWS4 if path == "lists" else NARROW | RB_LDS) | (PINNED if out == "host" else 0)
        claims = [("path", path)] + ([("cap", mp, natural)] if cap is not None else [])
        return _lcm_case(150, c, rule(rname, max_pairs=mp, **over), bits, claims, out)
    return build


for _p in ("lists", "loop"):
    for _r in sorted(RULES):
        _add("%s_%s" % (_p, _r), _ruled(_p, _r))
    for _c in (0, 1, "natural-1"):
        _add("%s_greedy_opt_cap_%s" % (_p, _c), _ruled(_p, "greedy_opt", cap=_c))
    _add("%s_simulator_cap_natural-1" % _p, _ruled(_p, "simulator", cap="natural-1"))
    _add("%s_simulator_devout" % _p, _ruled(_p, "simulator", out="device"))
    _add("%s_greedy_opt_devout_cap_1" % _p, _ruled(_p, "greedy_opt", cap=1, out="device"))


# ---- k_lcms_scan: nlev * n = 8192 (one tile) / 8193 (one entry carried into a second tile: the top level of the last row)
def _scan_8192():
    n = SCAN_TILE // BALLOT_LEVELS
    return _lcm_case(n, _dense(600, n, 0, BALLOT_LEVELS - 1), rule("simulator"), LISTS | ROWS4 | PINNED, [("scan", SCAN_TILE)])


def _scan_8193():
    n, nlev = (SCAN_TILE + 1) // 3, 3
    r, c, v = _rand_cells(601, n - 1, 30, 0, nlev - 1)           # nothing in the last row or column ...
    r, c, v = np.concatenate([[n - 1], r]), np.concatenate([[n - 1], c]), np.concatenate([[nlev - 1], v])   # ... but the top level's (n-1, n-1)
    return _lcm_case(n, _sparse_input(n, r, c, v), rule("simulator"), LISTS | ROWS4 | PINNED,
                     [("scan", SCAN_TILE + 1), ("picked", n - 1, n - 1, nlev - 1)])


_add("scan_8192", _scan_8192)
_add("scan_8193", _scan_8193)


# ---- k_lcms_greedy's chunks: list positions 1023 / 1024 (emission across 1024-cell chunks) and 4095 / 4096 (the skip of a
# 4096-cell block without a live cell).  Level 0 takes the first rows, which leaves their cells dead in level 1.
CH_N = 1100


def _chunk_band():
    """level 0 is a permutation band: CH_N pairwise non-conflicting cells, all taken, emitted across two chunks"""
    i = np.arange(CH_N)
    r, c, v = _rand_cells(700, CH_N, 3, 1, 3)
    inp = _sparse_input(CH_N, np.concatenate([i, r]), np.concatenate([(7 * i + 3) % CH_N, c]), np.concatenate([0 * i, v]))
    return _lcm_case(CH_N, inp, rule("greedy_opt"), LISTS | ROWS4 | PINNED,
                     [("pos", 0, CHUNK - 1), ("pos", 0, CHUNK), ("pos", 0, 0), ("pos", 0, CH_N - 1), ("path", "lists")])


def _chunk_dead(n_dead, live_pos):
    """level 0: (i, CH_N - 1 - i) for the first rows; level 1: n_dead cells of those rows (all dead when level 1 starts), then a live
    cell at list position live_pos = n_dead, then cells that the pick kills and one more live cell"""
    def build():
        full, part = divmod(n_dead, CHUNK)
        rows0 = full + (part > 0)
        r = [np.arange(rows0)]
        c = [CH_N - 1 - np.arange(rows0)]
        v = [np.zeros(rows0, np.int64)]
        for i in range(rows0):
            w = CHUNK if i < full else part
            r.append(np.full(w, i)), c.append(1 + np.arange(w)), v.append(np.ones(w, np.int64))
        # the live cell, two cells it kills, a second live cell
        r.append(np.array([rows0, rows0, rows0 + 1, rows0 + 2]))
        c.append(np.array([5, 9, 5, 9]))
        v.append(np.ones(4, np.int64))
        inp = _sparse_input(CH_N, np.concatenate(r), np.concatenate(c), np.concatenate(v))
        claims = [("dead", 1, 0, n_dead), ("pos", 1, live_pos), ("pos", 1, live_pos + 3), ("path", "lists")]
        return _lcm_case(CH_N, inp, rule("greedy_opt"), LISTS | ROWS4 | PINNED, claims)
    return build


_add("chunk_band", _chunk_band)
_add("chunk_dead1024_live1024", _chunk_dead(CHUNK, CHUNK))
_add("chunk_dead1023_live1023", _chunk_dead(CHUNK - 1, CHUNK - 1))
_add("chunk_dead4096_live4096", _chunk_dead(SKIP_BLOCK, SKIP_BLOCK))
_add("chunk_dead4095_live4095", _chunk_dead(SKIP_BLOCK - 1, SKIP_BLOCK - 1))


# ---- large n: sparse models, built on the device by the GPU test
def edge_columns(n):
    """first and last column of every k_lcms_rows4 quarter (n <= ROWS4_NMAX) or k_lcms_rows block, and column n - 1"""
    w = rows4_quarter(n) if n <= ROWS4_NMAX else ROWS_BLOCK
    cols = set()
    for lo in range(0, n, w):
        cols |= {lo, min(lo + w, n) - 1}
    return sorted(cols | {n - 1})


def _big_lists(n, nlev, per_row, seed):
    def build():
        r, c, v = _rand_cells(seed, n, per_row, 0, nlev - 1)
        ec = np.array(edge_columns(n))
        er = np.repeat(np.arange(n), ec.size)
        ecs = np.tile(ec, n)
        ev = (er * 5 + ecs * 3) % nlev
        inp = _sparse_input(n, np.concatenate([er, r]), np.concatenate([ecs, c]), np.concatenate([ev, v]))
        bits = LISTS | (ROWS4 if n <= ROWS4_NMAX else 0) | (PINNED if PINNED_OFF + 8 * n <= PINNED_CAP else 0)
        return _lcm_case(n, inp, rule("simulator"), bits, [("span", nlev - 1, 0), ("edge_columns",), ("lds", "greedy")])
    return build


_add("big_n4093", _big_lists(4093, 17, 31, 800))
_add("big_n4096", _big_lists(4096, 17, 31, 801))
_add("big_n4097_lev16", _big_lists(4097, 16, 31, 802))
_add("big_n4097_lev17", _big_lists(4097, 17, 31, 803))
_add("pinned_n7168", _big_lists(7168, 17, 12, 804))    # 8192 + 8 n = 65536: the pairs ride in the pinned block
_add("pinned_n7169", _big_lists(7169, 17, 12, 805))    # one more: separate copies


def _big_loop(n, seed):   # wide values: the loop; 8 n + 4 ceil(n / 32) on both sides of 49152 and of 98304
    def build():
        r, c, v = _rand_cells(seed, n, 20, 0, 100000)
        bits = NARROW | (RB_LDS if loop_lds(n) <= LDS_ROWKEYS else 0) | (PINNED if PINNED_OFF + 8 * n <= PINNED_CAP else 0)
        return _lcm_case(n, _sparse_input(n, r, c, v), rule("greedy_opt", threshold=100000), bits, [("path", "loop"), ("lds", "loop")])
    return build


_add("loop_n6049", _big_loop(6049, 810))
_add("loop_n6050", _big_loop(6050, 811))
_add("loop_n12098", _big_loop(12098, 812))
_add("loop_n12099", _big_loop(12099, 813))


# ---- n = 16384 / 16385: k_lcms_greedy's tables stop growing; rows 0 and 16384 and columns 0 and 16384 share a slot
HASH_A, HASH_B = 9000, 100
HASH_CELLS = ((0, HASH_A), (5, 0), (7, HASH_SIZE), (HASH_SIZE, HASH_B), (HASH_SIZE, HASH_A))   # level 0, in list order
HASH_TAKEN = ((0, HASH_A), (5, 0), (7, HASH_SIZE), (HASH_SIZE, HASH_B))                        # the last one loses its row and column


def _hash(n):
    def build():
        named = [rc for rc in HASH_CELLS if max(rc) < n]
        r, c, v = _rand_cells(820, n, 5, 1, 5)
        inp = _sparse_input(n, np.concatenate([[a for a, _ in named], r]), np.concatenate([[b for _, b in named], c]),
                            np.concatenate([[0] * len(named), v]))
        return _lcm_case(n, inp, rule("simulator"), LISTS, [("hash", tuple(named))])
    return build


_add("hash_n16384", _hash(HASH_SIZE))
_add("hash_n16385", _hash(HASH_SIZE + 1))


# ---- candidate count 2^28 / 2^28 + 32769: the full matrix, every cell a candidate
def _count(n):
    def build():
        bits = LISTS if n * n <= COUNT_MAX else NARROW
        return dict(kind="lcm", n=n, input="count", rule=rule("heuristic"), bits=bits, claims=(("count", n * n),), out="host")
    return build


_add("count_n16384", _count(16384))
_add("count_n16385", _count(16385))


# ---- td_pool2
def _pool_case(frm, to, dist, bits, claims=()):
    return dict(kind="pool2", n=len(frm), frm=_i32(frm), to=_i32(to), dist=None if dist is None else _i32(dist), bits=bits | POOL2,
                claims=tuple(claims), out="host")


def _pool_line(n, S=50):
    def build():
        rng = np.random.default_rng(900 + n)
        bits = LISTS if n >= LISTS_NMIN else RB_LDS
        return _pool_case(rng.integers(0, S, n), rng.integers(0, S, n), None, bits, [("lds", "greedy")] if n > ROWS4_NMAX else [])
    return build


def _pool_table(n, S=60):
    def build():
        rng = np.random.default_rng(910 + n)
        dist = rng.integers(0, 10**6 + 1, (S, S))
        dist[3, 4] = 10**6
        return _pool_case(rng.integers(0, S, n), rng.integers(0, S, n), dist, (NARROW if n >= NARROW_NMIN else 0) | RB_LDS,
                          [("pool_span_at_least", LV_MAX)])
    return build


@functools.lru_cache(maxsize=None)
def _pool_span_search(span, n=64):
    """from / to on a long line whose pair costs span exactly `span` levels: the first hit of a small search"""
    for S in range(span // 3, span):
        for seed in range(8):
            rng = np.random.default_rng(1000 * S + seed)
            frm, to = rng.integers(0, S, n), rng.integers(0, S, n)
            cost = pool_costs(frm, to, None)[0][~np.eye(n, dtype=bool)]
            if int(cost.max() - cost.min()) == span:
                return frm, to
    raise AssertionError("no model with span %d" % span)


def _pool_span(span):
    def build():
        frm, to = _pool_span_search(span)
        return _pool_case(frm, to, None, LISTS if span < LV_MAX else RB_LDS, [("pool_span", span)])
    return build


for _n in (63, 64, 65):
    _add("pool_line_n%d" % _n, _pool_line(_n))
for _n in (127, 128, 129, 145):
    _add("pool_table_n%d" % _n, _pool_table(_n))
_add("pool_span255", _pool_span(LV_MAX - 1))
_add("pool_span256", _pool_span(LV_MAX))
_add("pool_line_n4097", _pool_line(4097))

CASE_NAMES = tuple(_BUILDERS)
LCM_NAMES = tuple(m for m in CASE_NAMES if not m.startswith("pool_"))
POOL_NAMES = tuple(m for m in CASE_NAMES if m.startswith("pool_"))

# both sides of every edge of the table (test_lcm_paths_cpu.py checks that the path-deciding ones differ in their bits)
EDGES = {
    "n 63/64": ("edge_n63", "edge_n64"),
    "n 127/128": ("narrow_n127_d254", "narrow_n128_d254"),
    "code 254/255": ("narrow_n144_d254", "narrow_n144_d255"),
    "LV_MAX 255/256": ("span255", "span256"),
    "LV_MAX 255/256, vmin < 0": ("span255_neg", "span256_neg"),
    "nlev 16/17 rows4": ("lev16", "lev17"),
    "nlev 16/17 rows": ("big_n4097_lev16", "big_n4097_lev17"),
    "n 4096/4097": ("big_n4096", "big_n4097_lev17"),
    "quarters": ("quarter_n64", "quarter_n65", "quarter_n256", "quarter_n257", "big_n4093", "big_n4096"),
    "positions 1023/1024": ("chunk_dead1023_live1023", "chunk_dead1024_live1024", "chunk_band"),
    "positions 4095/4096": ("chunk_dead4095_live4095", "chunk_dead4096_live4096"),
    "scan tile 8192/8193": ("scan_8192", "scan_8193"),
    "n 16384/16385 tables": ("hash_n16384", "hash_n16385"),
    "count 2^28": ("count_n16384", "count_n16385"),
    "row keys 12098/12099": ("loop_n12098", "loop_n12099"),
    "loop LDS 6049/6050": ("loop_n6049", "loop_n6050"),
    "pinned 7168/7169": ("pinned_n7168", "pinned_n7169"),
    "pool2 n 63/64": ("pool_line_n63", "pool_line_n64"),
    "pool2 n 127/128": ("pool_table_n127", "pool_table_n128"),
    "pool2 LV_MAX": ("pool_span255", "pool_span256"),
    "pool2 n 4097": ("pool_line_n65", "pool_line_n4097"),
}
PATH_DECIDING = ("n 63/64", "n 127/128", "LV_MAX 255/256", "LV_MAX 255/256, vmin < 0", "n 4096/4097", "count 2^28",
                 "row keys 12098/12099", "pinned 7168/7169", "pool2 n 63/64", "pool2 n 127/128", "pool2 LV_MAX")


@functools.lru_cache(maxsize=None)
def case(name):
    d = dict(_BUILDERS[name](), name=name)
    for k in ("matrix", "frm", "to", "dist"):
        if d.get(k) is not None:
            d[k].setflags(write=False)
    for a in d.get("coords", ()):
        a.setflags(write=False)
    return d


def dense_matrix(c):
    """the int32 matrix of a dense or (n <= DENSE_MAX) sparse LCM case"""
    if c["input"] == "dense":
        return c["matrix"]
    assert c["input"] == "sparse" and c["n"] <= DENSE_MAX
    m = np.full((c["n"], c["n"]), c["fill"], np.int32)
    r, cc, v = c["coords"]
    m[r, cc] = v
    return m


def candidates(c):
    """(count, vmin, vmax) of the candidate cells, as k_lcms_minmax measures them"""
    if c["kind"] == "pool2":
        cost = case_pool_costs(c["name"])[0][~np.eye(c["n"], dtype=bool)]
        return int(cost.size), int(cost.min()), int(cost.max())
    hi = candidate_hi(c["rule"][0])
    if c["input"] == "count":
        assert hi >= 5
        return c["n"] ** 2, 0, 5
    v = c["matrix"].ravel() if c["input"] == "dense" else c["coords"][2]
    if c["input"] == "sparse":
        assert c["fill"] > hi
    v = v[v <= hi]
    return int(v.size), int(v.min()), int(v.max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """lcm: (total, rows, cols, last_min) as lists / ints; pool2: the list of (a, b, plan, cost)"""
    c = case(name)
    if c["kind"] == "pool2":
        return pool2_reference(c["frm"], c["to"], c["dist"], by_level=c["n"] > 1000, costs=case_pool_costs(name))
    kw_gpu, kw_oracle = c["rule"]
    if c["input"] == "count":
        t, r, cc, lm = count_expected(c["n"], kw_oracle)
    elif c["input"] == "dense":
        t, r, cc, lm = lcm_expected(c["matrix"], kw_oracle)
    else:
        t, r, cc, lm = sparse_greedy(c["n"], *c["coords"], kw_gpu, c["fill"])
    return int(t), r.tolist(), cc.tolist(), int(lm)
