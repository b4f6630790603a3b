"""The case table of tests/test_finisher_cases_cpu.py, tools/finisher_paths.py and tests/test_gpu_finisher_paths.py: td_assign
inputs that sit on every selection, chunk and LDS edge of sv_finish_t (csrc/td_assign.hip), the chain of finishers that gives
td_assign its exactness on whatever the bidding rounds leave free.  Plain numpy: nothing here needs a GPU.

Three parts.

(a) Instance makers, all solved with the line recogniser off and all with a reference that needs no GPU result:
    L(n, S, seed)      cost |a_i - b_j|, positions uniform in [0, S); the optimum is sum |sort a - sort b|
    LP(n, k, S, seed)  n - k such rows plus k constant rows of BIG, which sit out the rounds (defer_const) and are placed by the
                       finisher's tail; the optimum is the monotone-matching dynamic program over the sorted positions + k BIG
    U(n, hi, seed)     uniform costs 0..hi, n <= ORACLE_NMAX, checked by the CPU oracle
    S picks the cell type through the row range: 255 -> "u8" (1-byte cells), 60000 -> "u16" (2-byte), S4(n) = max(100 n, 150000)
    -> "u32n" (4-byte cells, 32-bit prices; 100 n alone stays below 65535 for n < 656), 5 10^7 -> "u32" (64-bit prices).
    From DEVICE_MIN on the matrix is built on the device by td.cost_build from the same positions.

(b) geometry() / forest_geometry() / expected(): sv_finish_t's arithmetic restated, each rule with the line it restates.
    expected() returns the FP_* flags that must be set (every other flag must be clear), CH and the speculative batch count.
    Where a rule reads a free-row count back from the device, expected() takes it from the statistics of the solve.

(c) SECTIONS and CASES: a section is an environment (one child process, the library reads its switches once); a case names
    its section, its instance, the finisher it stands on and why.  `emulates` marks the rows that run what a REFUSED
    cooperative launch falls back to, emulated by the off switch of that kernel (TD_FOREST=0 / TD_SAPX=0): the same code
    path below the refused launch, at the sizes where the cooperative kernel is the default.

The free rows the bidding rounds (and the speculative batches) left, as measured on the MI355X when the seeds were chosen, are
in the `free` field of each row: (rows at the finisher's entry, rows left to the last finisher); the CPU tier feeds them to
expected() and holds the result against the finisher the row names, the GPU tier uses the counts the solve reports."""
import functools

import numpy as np

BIG = 250000
ORACLE_NMAX = 4096
DEVICE_MIN = 3000          # from this n on the matrix is built on the device (td.cost_build)

# ---- td_last_stats word 13 (include/taxidispatcher_amd.h)
FP_FOREST, FP_FOREST_NONE, FP_FOREST_REFUSED, FP_PSAP, FP_SAPX, FP_SAPX_REFUSED, FP_SAP8_BATCH, FP_SAP8 = (1 << k for k in range(8))
FP_CH_SHIFT, FP_CH_MASK = 8, 0x1F00
FP_SAP512, FP_SAP, FP_NOLDS = 1 << 13, 1 << 14, 1 << 15
FP_BATCH_SHIFT = 16
FP_FLAGS = 0xFFFF & ~FP_CH_MASK
FP_NAMES = {FP_FOREST: "FOREST", FP_FOREST_NONE: "FOREST_NONE", FP_FOREST_REFUSED: "FOREST_REFUSED", FP_PSAP: "PSAP", FP_SAPX: "SAPX",
            FP_SAPX_REFUSED: "SAPX_REFUSED", FP_SAP8_BATCH: "SAP8_BATCH", FP_SAP8: "SAP8", FP_SAP512: "SAP512", FP_SAP: "SAP",
            FP_NOLDS: "NOLDS"}


def flag_names(word):
    return "|".join(v for k, v in FP_NAMES.items() if word & k) or "0"


# ---- cell types: E cells per 16-byte chunk (Tr<CT>::E), bytes per cell, IsLean8<CT>, what last_stats() shows for them
TYPES = {"u8": dict(E=16, bytes=1, lean8=True, narrow=0), "u16": dict(E=8, bytes=2, lean8=False, narrow=0),
         "u32n": dict(E=4, bytes=4, lean8=False, narrow=1), "u32": dict(E=4, bytes=4, lean8=False, narrow=0)}
U8_LIMIT, U16_LIMIT, NP_RANGE = 254, 65534, (1 << 22) - 2      # Tr<CT>::LIMIT: the largest row range (max - min) a type holds

# ---- the constants of sv_finish_t
LDS_STATE_MAX = 150 * 1024   # `const bool lds = st <= 150 * 1024` with st = npad * 2 * sizeof(int)
DYN_LDS_OPT_IN = 48 * 1024   # `if (shm > 48 * 1024) hipFuncSetAttribute(...)`, `if (cshm > 48 * 1024)` with cshm = 2 * sizeof(int) * n
SX_KMAX = 64                 # `constexpr int SX_KMAX = 64`
PS_G = 192                   # `constexpr int PS_G = 192`: searches per speculative batch
FOREST_MAX_N = 32768         # `n <= 32768`
FOREST_PCL_MAX_N = 16384     # `a_pcl = (n <= 16384) ? 1 : 0`, `if (n <= 16384) TD_FO_LAUNCH(64, 1024); else TD_FO_LAUNCH(128, 512);`

# the switches sv_finish_t reads, their defaults and read_tunables' clamps
DEFAULTS = dict(TD_FOREST=1, TD_FOREST_MIN_N=2048, TD_SAPX=1, TD_SAPX_MIN=8, TD_SAPX_ROWS=24, TD_SAP512=1, TD_SAP8=1, TD_PSAP=16,
                TD_PSAP8=1, TD_PSAP_CAP=4096, TD_PSAP_MIN=12, TD_PSAP_WORTH=4, TD_WIDE_U16_N=2048, TD_U16_REDO_FREE=64)
_CLAMPS = dict(TD_FOREST=lambda v: int(v != 0), TD_FOREST_MIN_N=lambda v: max(64, v), TD_SAPX=lambda v: int(v != 0),
               TD_SAPX_MIN=lambda v: max(1, v), TD_SAPX_ROWS=lambda v: max(1, v), TD_SAP512=lambda v: int(v != 0),
               TD_SAP8=lambda v: int(v != 0), TD_PSAP=lambda v: max(0, min(64, v)), TD_PSAP8=lambda v: max(0, min(32, v)),
               TD_PSAP_CAP=lambda v: max(0, v), TD_PSAP_MIN=lambda v: max(1, v), TD_PSAP_WORTH=lambda v: max(1, v),
               TD_WIDE_U16_N=lambda v: max(0, v), TD_U16_REDO_FREE=lambda v: max(0, v))


def tunables(env):
    t = dict(DEFAULTS)
    for k, v in env.items():
        assert k in DEFAULTS, k
        t[k] = _CLAMPS[k](int(v))
    return t


# ======================================================================================================================
# (b) sv_finish_t restated
# ======================================================================================================================
def geometry(kind, n):
    """the sizes sv_finish_t derives from the cell type and n"""
    E, four = TYPES[kind]["E"], TYPES[kind]["bytes"] == 4
    nchunks = (n + E - 1) // E                # sv_compress: `const int nchunks = (n + E - 1) / E`
    npad = nchunks * E
    CH = 1
    while CH * 1024 < nchunks:                # `while (CH * 1024 < nchunks) CH *= 2`
        CH *= 2
    T = (nchunks + CH - 1) // CH
    T = min(1024, max(64, (T + 63) // 64 * 64))
    st = npad * 2 * 4                         # owner[] + pred[]
    lds = st <= LDS_STATE_MAX
    ch5 = 1
    while ch5 * 512 < nchunks:                # `while (ch5 * 512 < nchunks) ch5 *= 2`
        ch5 *= 2
    T5 = (nchunks + ch5 - 1) // ch5
    T5 = min(512, max(64, (T5 + 63) // 64 * 64))
    TX = 128 if four else 256                 # `constexpr int TXsel = (sizeof(CT) == 4) ? TD_SX_TX : 256`
    KX = (nchunks + TX - 1) // TX
    return dict(E=E, nchunks=nchunks, npad=npad, CH=CH, T=T, st=st, lds=lds, shm=st if lds else 0, ch5=ch5, T5=T5, TX=TX, KX=KX,
                last_chunk_cols=n - (nchunks - 1) * E, cshm=2 * 4 * n,
                shm_opt_in=(st if lds else 0) > DYN_LDS_OPT_IN, cshm_opt_in=2 * 4 * n > DYN_LDS_OPT_IN,
                sapx_last_wg_chunks=nchunks - (KX - 1) * TX)


def forest_geometry(n):
    """k_forest's launch: columns per workgroup, threads, grid, the predecessor walk's place, dynamic LDS"""
    small = n <= FOREST_PCL_MAX_N
    CW, TB = (64, 1024) if small else (128, 512)
    n4 = (n + 3) // 4 * 4
    return dict(CW=CW, TB=TB, grid=(n + CW - 1) // CW, a_pcl=int(small), last_slice_cols=n - (n - 1) // CW * CW,
                dyn=max(2 * n4, 6 * n4 if small else 0))


def expected(kind, n, env, free_serial, spec_rows):
    """What sv_finish_t<CT> launches for an unsharded model whose cooperative launches are accepted.
    free_serial: last_stats()["sap_free_rows"], the rows the last finisher found free (k_freelist's count, lowered by every
    k_pcommit; k_forest, k_sapx and the serial searches write back the count they started from).
    spec_rows: last_stats()["parallel_sap_rows"], the rows the speculative batches committed.
    Returns dict(flags, ch, batches_min, batches_exact, kernel): word 13 must equal flags in its flag bits, ch in bits 8..12,
    and hold batches_exact (when not None) or at least batches_min speculative batches."""
    t, g, ty = tunables(env), geometry(kind, n), TYPES[kind]
    E, CH = g["E"], g["CH"]
    assert CH * E <= 64, "beyond the single-workgroup finisher (TD_ERANGE)"
    out = dict(flags=0, ch=0, batches_min=0, batches_exact=0, kernel=None)
    free_entry = free_serial + spec_rows
    # `if constexpr (sizeof(CT) == 4) { if (g_forest && n >= g_forest_min_n && n <= 32768 && tab.count == 1)`
    if ty["bytes"] == 4 and t["TD_FOREST"] and t["TD_FOREST_MIN_N"] <= n <= FOREST_MAX_N:
        if free_entry == 0:
            out.update(flags=FP_FOREST_NONE, kernel="none")
        else:
            fg = forest_geometry(n)
            out.update(flags=FP_FOREST, kernel="k_forest<%s, %d, %d>" % (kind, fg["CW"], fg["TB"]))
        return out
    # `if (g_psap_batches > 0 && CH <= 4 && CH * E <= 16 && lds && n >= 64 && !IsLean8<CT>::value && !sv.tick_sized)`
    nfree_left = -1
    if t["TD_PSAP"] > 0 and CH <= 4 and CH * E <= 16 and g["lds"] and n >= 64 and not ty["lean8"]:
        tb = 512 if (t["TD_SAP512"] and g["T"] <= 512) else 1024          # `const bool tb512 = g_sap512 && T <= 512`
        psap_min = max(t["TD_PSAP_MIN"], 32) if n < 2048 else t["TD_PSAP_MIN"]
        if free_entry >= psap_min and t["TD_PSAP_CAP"] > 0:                 # `while (nfree >= psap_min && launched < g_psap_cap)`
            nb = max(1, min(t["TD_PSAP"], (free_entry + 31) // 32))
            out["flags"] |= FP_PSAP
            out["ch"] = CH
            out["batches_min"] = nb
            out["batches_exact"] = nb if t["TD_PSAP_CAP"] <= nb else None  # one group reaches the cap: no second group
            out["spec_kernel"] = "k_sap<%s, %d, true, %d, SPEC> + k_pcommit" % (kind, CH, tb)
        nfree_left = free_serial
    # `const bool big = KX * TXsel >= g_sapx_min * 256 || (KX * TXsel >= g_sapx_min * 128 && nfree_left >= g_sapx_rows)`
    lean8 = ty["lean8"] and CH == 1 and t["TD_SAP8"]
    span = g["KX"] * g["TX"]
    big = span >= t["TD_SAPX_MIN"] * 256 or (span >= t["TD_SAPX_MIN"] * 128 and nfree_left >= t["TD_SAPX_ROWS"])
    if t["TD_SAPX"] and not lean8 and big and g["KX"] <= SX_KMAX:
        out["flags"] |= FP_SAPX
        out["kernel"] = "k_sapx<%s, %d>" % (kind, g["TX"])
        return out
    nolds = 0 if g["lds"] else FP_NOLDS
    if lean8:                                                                # `if (CH == 1 && g_sap8)`
        if g["lds"] and t["TD_PSAP8"] > 0 and n >= 64:                        # `if (lds && g_psap8_batches > 0 && n >= 64)`
            out["flags"] |= FP_SAP8_BATCH
            out["batches_min"] = out["batches_exact"] = t["TD_PSAP8"]
        out["flags"] |= FP_SAP8 | nolds
        out["ch"] = 1
        out["kernel"] = "k_sap8<%s, false>" % ("true" if g["lds"] else "false")
        return out
    out["ch"] = CH
    if t["TD_SAP512"] and g["ch5"] == CH and g["ch5"] * E <= 16:             # `if (g_sap512 && ch5 == CH && ch5 * E <= 16)`
        out["flags"] |= FP_SAP512 | nolds
        out["kernel"] = "k_sap<%s, %d, %s, 512>" % (kind, CH, "true" if g["lds"] else "false")
        out["threads"] = g["T5"]
        return out
    out["flags"] |= FP_SAP | nolds
    out["kernel"] = "k_sap<%s, %d, %s, 1024>" % (kind, CH, "true" if g["lds"] else "false")
    out["threads"] = g["T"]
    return out


# ======================================================================================================================
# (a) instances and references
# ======================================================================================================================
def S4(n):
    return max(100 * n, 150000)


def kind_of_range(rng_max, wide_prices=False):
    """the cell type solve_orientations ends at for rows whose largest range (max - min) is rng_max"""
    if rng_max <= U8_LIMIT:
        return "u8"
    if rng_max <= U16_LIMIT:
        return "u16"
    return "u32n" if rng_max <= NP_RANGE else "u32"


def _inst(family, n, k, S, seed, m=0):
    return dict(family=family, n=n, k=k, S=S, seed=seed, m=m)


def L(n, S, seed):
    return _inst("L", n, 0, S, seed)


def LP(n, k, S, seed):
    return _inst("LP", n, k, S, seed)


def LN(n, m, S, seed):
    """L with all but m cabs standing on a request of their own (a_i = b_i): the rounds place those at once, the m others push
    chains through them.  The closed form holds as for any positions; the finisher gets hundreds of rows, not thousands (the
    single-workgroup searches of the large tier: L(19204) leaves 5215 rows = 15.7 s, L(16388) 4106 rows = 6.1 s)"""
    return _inst("LN", n, 0, S, seed, m)


def U(n, hi, seed):
    assert n <= ORACLE_NMAX
    return _inst("U", n, 0, hi, seed)


@functools.lru_cache(maxsize=None)
def _positions(family, n, k, S, seed, m):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, S, n - k).astype(np.int64), rng.integers(0, S, n).astype(np.int64)
    if family == "LN":
        a[:n - m] = b[:n - m]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def positions(inst):
    """(a: one position per REAL row, b: one per column)"""
    assert inst["family"] in ("L", "LN", "LP")
    return _positions(inst["family"], inst["n"], inst["k"], inst["S"], inst["seed"], inst["m"])


def on_device(inst):
    return inst["n"] >= DEVICE_MIN


def numpy_matrix(inst):
    """the n x n int32 matrix (n < DEVICE_MIN, or U): real rows first, the k constant rows of BIG behind them"""
    n = inst["n"]
    if inst["family"] == "U":
        return np.random.default_rng(inst["seed"]).integers(0, inst["S"], (n, n), endpoint=True).astype(np.int32)
    a, b = positions(inst)
    c = np.full((n, n), BIG, np.int64)
    c[:n - inst["k"]] = np.abs(a[:, None] - b[None, :])
    return c.astype(np.int32)


def row_ranges(inst):
    """(smallest, largest) range max - min over the rows, from the positions (any n): what picks the cell type"""
    if inst["family"] == "U":
        c = numpy_matrix(inst).astype(np.int64)
        r = c.max(axis=1) - c.min(axis=1)
        return int(r.min()), int(r.max())
    a, b = positions(inst)
    bs = np.sort(b)
    far = np.maximum(np.abs(a - bs[0]), np.abs(a - bs[-1]))
    pos = np.searchsorted(bs, a)
    near = np.minimum(np.abs(a - bs[np.clip(pos, 0, bs.size - 1)]), np.abs(a - bs[np.clip(pos - 1, 0, bs.size - 1)]))
    r = far - near
    lo, hi = int(r.min()), int(r.max())
    return (0 if inst["k"] else lo), hi


def cost_of(inst, r2c, matrix=None):
    """what row_to_col costs, in int64 on the host: from the matrix where one exists here, else from the positions"""
    n = inst["n"]
    r2c = np.clip(np.asarray(r2c, np.int64), 0, n - 1)
    if matrix is not None:
        return int(matrix[np.arange(n), r2c].astype(np.int64).sum())
    a, b = positions(inst)
    real = n - inst["k"]
    return int(np.abs(a - b[r2c[:real]]).sum()) + inst["k"] * BIG


def sorted_matching_total(a, b):
    return int(np.abs(np.sort(a) - np.sort(b)).sum())


def monotone_matching_total(few, many):
    """len(few) points matched to as many of `many` without crossing: dp[i][j] = min(dp[i][j-1], dp[i-1][j-1] + |a_i - b_j|)
    over the sorted positions, a running minimum per row"""
    a_s, b_s = np.sort(np.asarray(few, np.int64)), np.sort(np.asarray(many, np.int64))
    m, k = a_s.size, b_s.size - a_s.size
    assert k >= 0
    prev = np.zeros(k + 1, np.int64)
    for i in range(m):
        prev = np.minimum.accumulate(prev + np.abs(a_s[i] - b_s[i:i + k + 1]))
    return int(prev[k])


def reference_total(inst):
    """the optimum, with no GPU result in it"""
    if inst["family"] == "U":
        from oracle import oracle
        return int(oracle.assign(numpy_matrix(inst))[0])
    a, b = positions(inst)
    if inst["k"] == 0:
        return sorted_matching_total(a, b)
    return monotone_matching_total(a, b) + inst["k"] * BIG


# ======================================================================================================================
# (c) the table
# ======================================================================================================================
_U16 = {"TD_WIDE_U16_N": "0", "TD_U16_REDO_FREE": "0"}     # 2-byte rows stay 2-byte (no redo as 4-byte cells)
# section -> (environment, timeout of its child in seconds).  The timeouts are ten times the wall time measured on the MI355X
# (the docstring of tests/test_gpu_finisher_paths.py has the times), and at least 120 s.
SECTIONS = {
    "default": ({}, 120),
    "psap8_off": ({"TD_PSAP8": "0"}, 120),
    "sap8_off": ({"TD_SAP8": "0"}, 120),
    "sap8_sap512_off": ({"TD_SAP8": "0", "TD_SAP512": "0"}, 120),
    "psap_off": ({"TD_PSAP": "0"}, 120),
    "psap_cap1": ({"TD_PSAP_CAP": "1"}, 120),
    "forest_off": ({"TD_FOREST": "0"}, 120),
    "forest_sap512_off": ({"TD_FOREST": "0", "TD_SAP512": "0"}, 120),
    "forest_off_sapx_rows": ({"TD_FOREST": "0", "TD_SAPX_ROWS": "100000"}, 120),
    "serial": (dict({"TD_FOREST": "0", "TD_SAPX": "0"}, **_U16), 120),
    "serial_large": ({"TD_FOREST": "0", "TD_SAPX": "0"}, 120),
    "sapx_min1": (dict({"TD_SAPX_MIN": "1", "TD_FOREST": "0"}, **_U16), 120),
    "forest_min64": ({"TD_FOREST_MIN_N": "64"}, 120),
}

CASES = {}
_FIN = {"forest": FP_FOREST, "sapx": FP_SAPX, "sap8": FP_SAP8, "sap8+batch": FP_SAP8 | FP_SAP8_BATCH, "sap512": FP_SAP512, "sap": FP_SAP,
        "sap+nolds": FP_SAP | FP_NOLDS}


def _add(name, section, inst, kind, fin, free, stands_on, spec=False, emulates=None):
    """kind: the cell type the instance is solved in (the CPU tier confirms it from the row ranges); fin: the finisher the row
    stands on (a key of _FIN), spec: with generic speculative groups in front (FP_PSAP); free: (rows free at the finisher's
    entry, rows left to the last finisher) as measured on the MI355X with this seed; emulates: the refused cooperative launch
    whose fallback the case runs (None: no such claim)"""
    assert name not in CASES and section in SECTIONS and emulates in (None, "k_forest", "k_sapx", "k_forest+k_sapx")
    CASES[name] = dict(name=name, section=section, inst=inst, kind=kind, flags=_FIN[fin] | (FP_PSAP if spec else 0), free=free,
                       stands_on=stands_on, emulates=emulates)


# ---- 1. k_sap8 (1-byte cells)
_add("sap8_n1024", "default", L(1024, 255, 11024), "u8", "sap8+batch", (252, 214), "nchunks 64: T = 64, the last chunk is full")
_add("sap8_n1025", "default", L(1025, 255, 11025), "u8", "sap8+batch", (249, 216),
     "nchunks 65: T rounds from 64 to 128, the last chunk holds one real column")
_add("sap8_n63", "default", L(63, 255, 10063), "u8", "sap8", (18, 18), "n < 64: no speculative batches")
_add("sap8_n64", "default", L(64, 255, 10064), "u8", "sap8+batch", (13, 11), "n = 64: the first size with speculative batches")
_add("sap8_lp_n200_k17", "default", LP(200, 17, 255, 10200), "u8", "sap8+batch", (32, 20),
     "17 constant rows placed by k_sap8's tail (defer_const)")
_add("sap8_psap8_off_n1024", "psap8_off", L(1024, 255, 11024), "u8", "sap8", (252, 252), "TD_PSAP8=0: k_sap8 alone")
_add("sap8_off_n1024", "sap8_off", L(1024, 255, 11024), "u8", "sap512", (252, 252),
     "TD_SAP8=0: 1-byte cells in the 512-thread k_sap, no speculative batches (IsLean8)")
_add("sap8_sap512_off_n1024", "sap8_sap512_off", L(1024, 255, 11024), "u8", "sap", (252, 252),
     "TD_SAP8=0 TD_SAP512=0: 1-byte cells in the generic k_sap")
# ---- 2. the speculative batches and k_pcommit
_add("psap_n1500", "default", L(1500, 150000, 21500), "u32n", "sap512", (433, 4), "speculative groups, then the 512-thread k_sap", spec=True)
_add("psap_u16_n1500", "default", L(1500, 60000, 21501), "u16", "sap512", (350, 6), "the same in 2-byte cells with 64-bit prices", spec=True)
_add("psap_wide_n1500", "default", L(1500, 5 * 10**7, 21502), "u32", "sap512", (364, 13), "the same in 4-byte cells with 64-bit prices", spec=True)
_add("psap_off_n1500", "psap_off", L(1500, 150000, 21500), "u32n", "sap512", (433, 433), "TD_PSAP=0: no speculative group")
_add("psap_cap1_n1500", "psap_cap1", L(1500, 150000, 21500), "u32n", "sap512", (433, 4), "TD_PSAP_CAP=1: exactly one group", spec=True)
_add("serial_n6144", "serial", L(6144, S4(6144), 26144), "u32n", "sap", (1508, 88),
     "npad * 8 = 2 * 4 * n = 48 KiB exactly: k_sap and k_pcommit without the opt-in", spec=True, emulates="k_forest+k_sapx")
_add("serial_n6148", "serial", L(6148, S4(6148), 26148), "u32n", "sap", (1746, 54), "49184 bytes: both need the dynamic-LDS opt-in",
     spec=True, emulates="k_forest+k_sapx")
# ---- 3. 512-thread against generic k_sap
_add("sap512_n2048", "forest_off", L(2048, S4(2048), 32048), "u32n", "sap512", (564, 31), "nchunks 512: ch5 = CH = 1, 512 threads",
     spec=True, emulates="k_forest")
_add("sap512_n2052", "forest_off", L(2052, S4(2052), 32052), "u32n", "sap", (601, 31),
     "nchunks 513: ch5 = 2 != CH = 1, generic k_sap with T = 576", spec=True, emulates="k_forest")
_add("sap512_off_n2048", "forest_sap512_off", L(2048, S4(2048), 32048), "u32n", "sap", (564, 31), "TD_SAP512=0: generic k_sap with T = 512",
     spec=True, emulates="k_forest")
# ---- 4. CH steps of the generic k_sap
_add("serial_n4096", "serial", L(4096, S4(4096), 44096), "u32n", "sap", (1126, 46), "nchunks 1024: CH = 1", spec=True, emulates="k_forest+k_sapx")
_add("serial_n4100", "serial", L(4100, S4(4100), 44100), "u32n", "sap", (1011, 35), "nchunks 1025: CH = 2", spec=True, emulates="k_forest+k_sapx")
_add("serial_n8192", "serial", L(8192, S4(8192), 48192), "u32n", "sap", (2199, 136), "nchunks 2048: CH = 2", spec=True, emulates="k_forest+k_sapx")
_add("serial_n8196", "serial", L(8196, S4(8196), 48196), "u32n", "sap", (2273, 76), "nchunks 2049: CH = 4", spec=True, emulates="k_forest+k_sapx")
_add("serial_u16_n8192", "serial", L(8192, 60000, 48193), "u16", "sap", (2127, 69), "2-byte cells, nchunks 1024: CH = 1", spec=True,
     emulates="k_sapx")
_add("serial_u16_n8200", "serial", L(8200, 60000, 48200), "u16", "sap", (2144, 55),
     "2-byte cells, nchunks 1025: CH = 2 (the last CH with speculative batches: CH * E = 16)", spec=True, emulates="k_sapx")
# (large tier: LN, see there; the plain L(16388) took 6.1 s and L(19204) 15.7 s in the single workgroup)
_add("serial_n16388", "serial_large", LN(16388, 256, S4(16388), 416388), "u32n", "sap", (240, 240), "CH = 8: no speculative batches (CH > 4)",
     emulates="k_forest+k_sapx")
_add("serial_n19204", "serial_large", LN(19204, 256, S4(19204), 416388), "u32n", "sap+nolds", (246, 246),
     "npad = 19204 > 19200: owner[] / pred[] in global memory", emulates="k_forest+k_sapx")
# ---- 5. k_sapx
_add("sapx_n8192", "forest_off", L(8192, S4(8192), 48192), "u32n", "sapx", (2199, 136), "default thresholds: KX = 16 workgroups", spec=True,
     emulates="k_forest")
_add("sapx_rows_n4100", "forest_off", L(4100, S4(4100), 44100), "u32n", "sapx", (1011, 35),
     "KX * 128 = 1152 in [1024, 2048): k_sapx only with >= 24 rows left", spec=True, emulates="k_forest")
_add("sapx_rows_off_n4100", "forest_off_sapx_rows", L(4100, S4(4100), 44100), "u32n", "sap", (1011, 35),
     "TD_SAPX_ROWS=100000: the same model stays in k_sap", spec=True, emulates="k_forest")
_add("sapx_min1_n1000", "sapx_min1", L(1000, 150000, 51000), "u32n", "sapx", (272, 16),
     "250 chunks: KX = 2, the second workgroup's part is partly empty", spec=True)
_add("sapx_min1_n1024", "sapx_min1", L(1024, 150000, 51024), "u32n", "sapx", (283, 32), "256 chunks: exactly two workgroups", spec=True)
_add("sapx_min1_n1026", "sapx_min1", L(1026, 150000, 51026), "u32n", "sapx", (264, 3),
     "257 chunks: n % 4 != 0 and a third workgroup holding one chunk", spec=True)
_add("sapx_min1_wide_n1026", "sapx_min1", L(1026, 5 * 10**7, 51027), "u32", "sapx", (224, 5), "the same with 64-bit prices and labels", spec=True)
_add("sapx_min1_u16_n2048", "sapx_min1", L(2048, 60000, 52048), "u16", "sapx", (527, 32), "2-byte cells (TX = 256), 256 chunks: KX = 1", spec=True)
_add("sapx_min1_u16_n2056", "sapx_min1", L(2056, 60000, 52056), "u16", "sapx", (517, 13), "257 chunks: KX = 2", spec=True)
# ---- 6. k_forest
for _n, _free in ((64, 15), (65, 16), (66, 13), (67, 18), (127, 28), (128, 24), (129, 33), (1000, 216)):
    _add("forest_n%d" % _n, "forest_min64", L(_n, 150000, 60000 + _n), "u32n", "forest", (_free, _free),
         "%d workgroup(s), last slice of %d column(s), n %% 4 = %d" % ((_n + 63) // 64, _n - (_n - 1) // 64 * 64, _n % 4))
_add("forest_wide_n129", "forest_min64", L(129, 5 * 10**7, 60130), "u32", "forest", (31, 31), "64-bit prices and labels")
_add("forest_n2049", "default", L(2049, S4(2049), 62049), "u32n", "forest", (579, 579),
     "default environment: 33 workgroups, the last slice holds one column")
_add("forest_n16384", "default", L(16384, S4(16384), 616384), "u32n", "forest", (4241, 4241),
     "the last n of <64, 1024> with the predecessor walk in LDS")
_add("forest_n16388", "default", L(16388, S4(16388), 616388), "u32n", "forest", (4086, 4086), "<128, 512>, predecessor walk in global memory")

CASE_NAMES = tuple(CASES)


def cases_of(section):
    return [c for c in CASES.values() if c["section"] == section]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the optimum of a case, computed once per process"""
    return reference_total(CASES[name]["inst"])
