"""GPU tests at the storage-width and value-range boundaries of the solvers (run with -m gpu on an MI355X).

td_assign never solves the int32 matrix it is given: it packs every row into the narrowest cells that hold the row's
range (csrc/td_assign.hip, Tr<CT>::LIMIT) and picks a price width to match.  Each boundary is stood on here with a row
range of exactly L, one step below and one step past it:

    1-byte cells            L = 254            (0xFF pads a row)
    2-byte cells            L = 65 534         (0xFFFF pads a row)
    4-byte cells, 32-bit    L = NP_RANGE = 2^22 - 2
    4-byte cells, 64-bit    L = 2^32 - 2       (2^32 - 1 is refused)
    1-byte cells + escape   real cells 0 .. 253, 254 = the fill value (fused transposing pass, n > 2048)
    packed bid key          refused when (range + 1) * (n + 1) >= 4e12

Every instance has an optimum known by construction (`trap`), with explicit duals, so a size the CPU oracle cannot
reach is still checked exactly; up to n = 3000 the oracle checks it as well.

Teeth.  A too-narrow width stores a row's cells modulo 2^8 / 2^16.  A row range of L + 1 is then read as the pad
code, which only ever makes the row's MAXIMUM cell dearer; an optimum that uses a row's maximum cell can always swap it
for the row's minimum column at no loss (every other row's range is <= L + 1), so no instance can make that reading
change the optimum.  What catches a limit moved by one is the width the statistics report (`check_width`).  From
L + 2 on, the cell wraps and reads CHEAPER than it is: the trap below makes that change the optimum, and the tests
prove so on the "what a too-narrow width would store" matrix (`wrapped`).  The escape-coded cells are the other way
round: a real cell of 254 read as the fill value is dearer, and `escape_model` makes it the only cheap way to serve
its request."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2**31, 2**31 - 1
BIG = 250000
NP_RANGE = 2**22 - 2
U8, U16, U32 = 254, 65534, 2**32 - 2
LADDERS = {"u8": U8, "u16": U16, "np": NP_RANGE, "u32": U32}


# ---------------------------------------------------------------------------------------------------------------------
# the trap: an instance whose optimum is known and which a wrapped cell would change
# ---------------------------------------------------------------------------------------------------------------------
def trap_layout(n, R, r, w, seed, nrows=None):
    """Indices and planted permutation of the trap.  Row r is the boundary row: its minimum (0) sits in column a, its
    maximum (R) in column w.  Row s owns column a and cannot afford anything else; r's optimal choice is column b at
    cost 1; row t owns w and could take b for free.  Read modulo 2^k (R = L + 2), cell (r, w) costs 0: r -> w, t -> b
    beats the true optimum by 1."""
    rng = np.random.default_rng(seed)
    others = [i for i in range(n if nrows is None else nrows) if i != r]
    s, t = (int(x) for x in rng.choice(others, 2, replace=False))
    cols = [j for j in range(n) if j != w]
    a, b = (int(x) for x in rng.choice(cols, 2, replace=False))
    perm = np.full(n, -1, np.int64)
    perm[r], perm[s], perm[t] = b, a, w
    rest_rows = [i for i in range(n) if perm[i] < 0]
    rest_cols = np.array([j for j in range(n) if j not in (a, b, w)], np.int64)
    perm[rest_rows] = rng.permutation(rest_cols)
    return dict(r=r, s=s, t=t, a=a, b=b, w=w, perm=perm)


def trap(n, R, r=None, w=None, seed=0, bases=None, nrows=None):
    """n x n int32 instance (numpy) around trap_layout: every row's range <= R, row r's range exactly R.
    Returns (cost, layout, optimum, u, v): optimum = sum(bases) + 1, perm is the unique optimum, (u, v) closes.
    nrows: the trap's helper rows s and t are taken from the first nrows rows."""
    assert n >= 4 and R >= 2
    r = n - 1 if r is None else r
    w = n - 1 if w is None else w
    g = trap_layout(n, R, r, w, seed, nrows)
    rng = np.random.default_rng(seed + 1)
    A = rng.integers(2, R, (n, n), dtype=np.int64, endpoint=True)   # off the planted cells: 2 .. R
    A[np.arange(n), g["perm"]] = 0
    A[g["r"], g["a"]] = 0
    A[g["r"], g["b"]] = 1
    A[g["r"], g["w"]] = R
    A[g["t"], g["b"]] = 0
    if bases is None:
        bases = rng.integers(I32_MIN, I32_MAX - R, n, dtype=np.int64, endpoint=True)
    bases = np.asarray(bases, np.int64)
    c = A + bases[:, None]
    assert c.min() >= I32_MIN and c.max() <= I32_MAX
    u = bases.copy()
    u[g["r"]] += 1
    u[g["s"]] += 1
    v = np.zeros(n, np.int64)
    v[g["a"]] = -1
    return c.astype(np.int32), g, int(bases.sum()) + 1, u, v


def wrapped(c, bits):
    """what cells of 2^bits would store: every row relative to its minimum, modulo 2^bits, the row minimum added back"""
    c = c.astype(np.int64)
    mn = c.min(axis=1, keepdims=True)
    return ((c - mn) % (1 << bits) + mn).astype(np.int64)


def prove_teeth(c, g, opt, bits):
    """the trap's alternative (r -> w, t -> b) costs less than the optimum under the wrapped reading; for n <= 3000 the
    oracle's optimum of the wrapped matrix differs from the true one"""
    n = c.shape[0]
    cw = wrapped(c, bits)
    alt = g["perm"].copy()
    alt[g["r"]], alt[g["t"]] = g["w"], g["b"]
    assert int(cw[np.arange(n), alt].sum()) < opt
    if n <= 3000 and cw.min() >= I32_MIN and cw.max() <= I32_MAX:
        assert oracle.assign(cw.astype(np.int32))[0] != opt


def row_range(c):
    c = c.astype(np.int64)
    return int((c.max(axis=1) - c.min(axis=1)).max())


def check_width(st, R, n, transposed=False):
    """bytes_per_cell never narrower than the range allows, and the narrow width taken where the design takes it"""
    bpc, npr = st["bytes_per_cell"], st["narrow_price"]
    if R > NP_RANGE:
        assert bpc == 4 and npr == 0, (R, n, st)
    elif R > U16:
        assert bpc == 4 and npr == 1, (R, n, st)
    elif R > U8:
        # 2-byte rows of a wide, hard model of n >= TD_WIDE_U16_N are redone as 4-byte cells with 32-bit prices
        assert bpc == 2 or (n >= 2048 and bpc == 4 and npr == 1), (R, n, st)
    else:
        assert bpc == 1, (R, n, st)
    assert st["transposed"] == (1 if transposed else 0), st


def check_host(td, c, g, opt, u, v, unique=True):
    """td_assign on a host matrix against the optimum by construction (and the oracle up to n = 3000)"""
    n = c.shape[0]
    assert oracle.certificate(c, g["perm"], u, v) == (0, opt, opt)
    r2c, total, dual = td.assign(c, want_dual=True)
    st = dict(td.last_stats())
    assert total == opt, (total, opt, st)
    assert dual == total, (dual, total, st)
    assert sorted(r2c.tolist()) == list(range(n))
    assert int(c[np.arange(n), r2c].astype(np.int64).sum()) == total
    if n <= 3000:
        t_o, r_o, u_o, v_o = oracle.assign(c)
        assert t_o == opt
        if unique:
            assert oracle.is_unique(c, r_o, u_o, v_o)
    if unique:
        assert np.array_equal(r2c, g["perm"]), "unique optimum but per-cab assignment differs"
    return r2c, st


def ladder(L):
    steps = [L - 1, L, L + 1]
    if L in (U8, U16):
        steps.append(L + 2)   # the first range that wraps
    return steps


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2: range ladders for td_assign, host matrices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r,w", [(40, 39, 39),       # shape probe off, last row, last column, n % 16 != 0 (the SENT tail)
                                   (1000, 0, 999),     # row 0, tail column
                                   (2051, 2050, 2050)])  # forest, TD_WIDE_U16_N, last row / column
@pytest.mark.parametrize("name", ["u8", "u16", "np", "u32"])
def test_range_ladder(general_solver, name, n, r, w):
    td = general_solver
    L = LADDERS[name]
    for R in ladder(L):
        if R > U32:   # INT32_MIN .. INT32_MAX in one row: range 2^32 - 1
            c, g, opt, u, v = trap(n, U32, r, w, seed=n, bases=np.full(n, I32_MIN, np.int64))
            c[r, w] = I32_MAX
            assert row_range(c) == 2**32 - 1
            with pytest.raises(td.TdError, match="exceeds 2\\^32-2" if n == 40 else "packed bid key"):
                td.assign(c)
            continue
        if name == "u32" and (R + 1) * (n + 1) >= 4e12:
            c, g, opt, u, v = trap(n, R, r, w, seed=n)
            with pytest.raises(td.TdError, match="packed bid key"):
                td.assign(c)
            continue
        c, g, opt, u, v = trap(n, R, r, w, seed=n + R % 1000)
        assert row_range(c) == R
        r2c, st = check_host(td, c, g, opt, u, v)
        check_width(st, R, n)
        if R == L + 2:
            prove_teeth(c, g, opt, 8 if L == U8 else 16)
        shard_check(c, r2c, opt, {"u8": 1, "u16": 2, "u32": 4}.get(name), L)


def shard_check(c, r2c, opt, width, L):
    """the shard API on the same instance (one in-process shard): compress(width) fits exactly while the range is <= L,
    and the shard solve is bit-identical to td_assign"""
    import torch
    from taxidispatcher_amd import sharded
    n, R = c.shape[0], row_range(c)
    full = torch.from_numpy(c).cuda()
    if width is not None:
        sh = sharded.HipShard(n, 0, n, full, share_torch_stream=False)
        try:
            assert sh.compress(width) == (R <= L), (width, R)
        finally:
            sh.close()
    shards = [sharded.HipShard(n, 0, n, full, share_torch_stream=False)]
    try:
        got, tot, dual, info = sharded.solve_shards_in_process(shards)
    finally:
        for s in shards:
            s.close()
    assert tot == dual == opt, (tot, dual, opt, info)
    assert np.array_equal(got, r2c), "shard solve and td_assign differ"


def test_warm_start_edge(general_solver):
    """TD_WARM_MIN_RANGE = 256: rows of range 255 are never warmed, 256 may be; both 2-byte, both exact (n >= 512)"""
    td = general_solver
    for n in (512, 700):
        for R in (255, 256):
            c, g, opt, u, v = trap(n, R, 0, n - 1, seed=R + n)
            _, st = check_host(td, c, g, opt, u, v)
            check_width(st, R, n)
            if R == 255:
                assert st["warm_rounds"] == 0, st


@pytest.mark.parametrize("R", [253, 254, 255, 256, 65533, 65534, 65535, 65536])
def test_transposed_model_column_ladder(general_solver, R):
    """a model padded with constant columns (the shape probe asks for the transposed problem): the trap sits in a COLUMN,
    whose range is what the transposed solve packs"""
    td = general_solver
    n, pad = 700, 240
    tr, g, opt, u, v = trap(n, R, n - pad - 1, n - 1, seed=R, bases=np.zeros(n, np.int64), nrows=n - pad)
    tr = tr.astype(np.int64)
    tr[n - pad:] = BIG                                   # constant rows of the transposed problem
    opt_t = oracle.assign(tr.astype(np.int32))[0]
    c = np.ascontiguousarray(tr.T).astype(np.int32)     # the caller's matrix: constant trailing columns
    r2c, total, dual = td.assign(c, want_dual=True)
    st = dict(td.last_stats())
    assert total == opt_t == oracle.assign(c)[0] == dual, (total, opt_t, st)
    assert sorted(r2c.tolist()) == list(range(n))
    assert int(c[np.arange(n), r2c].astype(np.int64).sum()) == total
    check_width(st, R, n, transposed=True)
    if R in (256, 65536):
        assert oracle.assign(wrapped(tr, 8 if R == 256 else 16).astype(np.int32))[0] != opt_t


# ---------------------------------------------------------------------------------------------------------------------
# large n: the same traps built on the device, optimum by construction
# ---------------------------------------------------------------------------------------------------------------------
def device_trap(torch, n, R, r, w, seed):
    """trap() on the device (n^2 int32 never on the host): background 2 .. R, small row offsets"""
    g = trap_layout(n, R, r, w, seed)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    c = torch.randint(2, R + 1, (n, n), dtype=torch.int32, device="cuda", generator=gen)
    perm = torch.from_numpy(g["perm"]).cuda()
    ar = torch.arange(n, device="cuda")
    c[ar, perm] = 0
    c[g["r"], g["a"]] = 0
    c[g["r"], g["b"]] = 1
    c[g["r"], g["w"]] = R
    c[g["t"], g["b"]] = 0
    bases = torch.randint(0, I32_MAX - R, (n,), dtype=torch.int32, device="cuda", generator=gen)
    c += bases[:, None]
    u = bases.long().clone()
    u[g["r"]] += 1
    u[g["s"]] += 1
    v = torch.zeros(n, dtype=torch.int64, device="cuda")
    v[g["a"]] = -1
    return c, g, int(bases.long().sum().item()) + 1, u, v


def device_check(torch, td, c, g, opt, u, v, R):
    n = c.shape[0]
    # the certificate of the construction, in row slabs (int64 reduced costs)
    for i0 in range(0, n, 2048):
        red = c[i0:i0 + 2048].long() - u[i0:i0 + 2048, None] - v[None, :]
        assert int(red.min().item()) >= 0
        del red
    mx = max(int((c[i0:i0 + 2048].long().amax(1) - c[i0:i0 + 2048].long().amin(1)).max().item()) for i0 in range(0, n, 2048))
    assert mx == R
    r2c, total, dual = td.assign(c, n, want_dual=True)
    st = dict(td.last_stats())
    assert total == opt == dual, (total, opt, dual, st)
    assert np.array_equal(r2c, g["perm"]), "unique optimum but per-cab assignment differs"
    picked = c[torch.arange(n, device="cuda"), torch.from_numpy(r2c.astype(np.int64)).cuda()]
    assert int(picked.long().sum().item()) == total
    return st


def device_teeth(torch, c, g, opt, bits):
    """the trap's alternative (r -> w, t -> b) under the wrapped reading of 2^bits cells costs less than the optimum"""
    n = c.shape[0]
    rowmin = torch.cat([c[i0:i0 + 2048].long().amin(1) for i0 in range(0, n, 2048)])
    alt = g["perm"].copy()
    alt[g["r"]], alt[g["t"]] = g["w"], g["b"]
    vals = c[torch.arange(n, device="cuda"), torch.from_numpy(alt).cuda()].long()
    assert int((((vals - rowmin) % (1 << bits)) + rowmin).sum().item()) < opt


@pytest.mark.parametrize("n,r,w", [(16384, 0, 16383),    # BID0 compress, block-local start, lazy narrow copy: (0, n-1) is off the diagonal blocks
                                   (12292, 12291, 0)])   # n >= 12 288, not a multiple of 128 (no blocks): BID0 pass alone
def test_range_ladder_large(general_solver, n, r, w):
    import torch
    td = general_solver
    for L in (U8, U16, NP_RANGE):
        for R in ladder(L):
            c, g, opt, u, v = device_trap(torch, n, R, r, w, seed=R % 100003)
            st = device_check(torch, td, c, g, opt, u, v, R)
            check_width(st, R, n)
            if R == L + 2:
                device_teeth(torch, c, g, opt, 8 if L == U8 else 16)
            del c, u, v
            torch.cuda.empty_cache()
    # 2^32 - 2: at this n no row range near 2^32 fits the packed bid key, on either side of the limit
    c = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    c[r, (w + 1) % n] = I32_MIN
    for R in (U32 - 1, U32, U32 + 1):
        c[r, w] = I32_MIN + R
        with pytest.raises(td.TdError, match="packed bid key"):
            td.assign(c, n)
    del c
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 3: escape-coded 1-byte cells of the fused transposing pass
# ---------------------------------------------------------------------------------------------------------------------
def escape_model(n_s, n_d, V, fill, seed, extra=None):
    """cab-major real cost matrix (n_s x n_d) with cells 0 .. 253 or `fill`, plus the escape trap: request J is reachable
    only from cab r at cost V; r's alternative is request J2 at 0, which cab r2 serves at 1.  With V read as `fill`, r
    serves J2 and J goes to a fill cell: the optimum moves."""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 254, (n_s, n_d)).astype(np.int64)
    C[rng.random((n_s, n_d)) < 0.7] = fill
    r, r2, J, J2 = n_s - 1, n_s - 2, n_d - 1, 0
    C[:, J] = fill
    C[:, J2] = fill
    C[r, :] = fill
    C[r2, :] = fill
    C[r, J] = V
    C[r, J2] = 0
    C[r2, J2] = 1
    if extra is not None:
        extra(C, rng)
    return C


def build_inputs(C):
    """positions and an S x S table that make td_cost_build produce exactly C (cab i at i, request j at n_s + j)"""
    n_s, n_d = C.shape
    S = n_s + n_d
    table = np.zeros((S, S), np.int32)
    table[:n_s, n_s:] = C
    return np.arange(n_s, dtype=np.int32), np.arange(n_s, S, dtype=np.int32), table


def solve_both(td, C, fill, want_r2c=False):
    """td_build_assign and td_cost_build + td_assign on the same model, and the oracle"""
    cab, dem, table = build_inputs(C)
    n, r2c, tot, dual = td.build_assign(cab, dem, table, fill=fill, threshold=-1, want_dual=True)
    st = dict(td.last_stats())
    n2, cost = td.cost_build(cab, dem, table, fill=fill, threshold=-1)
    ref, ref_tot, ref_dual = td.assign(cost, n2, want_dual=True)
    st2 = dict(td.last_stats())
    opt = oracle.assign(cost)[0]
    assert n == n2 and tot == ref_tot == dual == ref_dual == opt, (tot, ref_tot, dual, ref_dual, opt, st, st2)
    for p in (r2c, ref):
        assert sorted(p.tolist()) == list(range(n))
        assert int(cost[np.arange(n), p].astype(np.int64).sum()) == opt
    if want_r2c:
        return cost, opt, st, st2, r2c
    return cost, opt, st, st2


def dearer(cost, i, j, fill):
    """the escape misreading: cell (i, j) costs `fill`"""
    c = cost.copy()
    c[i, j] = fill
    return c


@pytest.mark.parametrize("V", [253, 254])
def test_escape_cells_at_the_code_limit(td, V):
    n_s, n_d = 2500, 1500
    C = escape_model(n_s, n_d, V, BIG, seed=V)
    cost, opt, st, st2 = solve_both(td, C, BIG)
    for s in (st, st2):
        assert s["transposed"] == 1, s
        assert s["bytes_per_cell"] == (1 if V == 253 else 4), s   # 254 is the escape code: a real 254 leaves the 1-byte cells
    # teeth: the real cell read as the fill value changes the optimum
    assert oracle.assign(dearer(cost, n_s - 1, n_d - 1, BIG))[0] != opt


def test_escape_real_cell_equal_to_fill(td):
    """real cells equal to the fill value are escape codes, not a reason to leave the 1-byte cells; with r2's own route to
    J2 made dear (100), the optimum serves the trap's request J through such a cell (r -> J2, J at the fill value)"""
    n_s, n_d, fill = 2300, 1200, 300
    r, r2, J = n_s - 1, n_s - 2, n_d - 1

    def dear_r2(C, rng):
        C[r2, 0] = 100
    C = escape_model(n_s, n_d, 253, fill, seed=1, extra=dear_r2)
    cost, opt, st, st2, r2c = solve_both(td, C, fill, want_r2c=True)
    for s in (st, st2):
        assert s["transposed"] == 1 and s["bytes_per_cell"] == 1, s
    served_by = int(np.flatnonzero(r2c == J)[0])
    assert cost[served_by, J] == fill and r2c[r] == 0, (served_by, int(r2c[r]))
    # teeth: the fill-valued real cells of the real columns read as code 254 instead of the fill value move the optimum
    misread = cost.copy()
    real = misread[:, :n_d]
    real[real == fill] = 254
    assert oracle.assign(misread)[0] != opt


def test_escape_negative_real_cell(td):
    """a real cell of -1 lies below the 1-byte cells' base: it must leave them (the 4-byte fused pass or the general
    path); as the trap's cell it is the only cheap way to serve request J"""
    n_s, n_d = 2300, 1200
    C = escape_model(n_s, n_d, -1, BIG, seed=2)
    cost, opt, st, st2 = solve_both(td, C, BIG)
    for s in (st, st2):
        assert s["transposed"] == 1 and s["bytes_per_cell"] == 4, s
    # teeth: -1 stored in one byte is the pad code 255; read as anything but -1 (here: the fill value) the optimum moves
    assert oracle.assign(dearer(cost, n_s - 1, n_d - 1, BIG))[0] != opt


@pytest.mark.parametrize("fill", [254, 255, NP_RANGE, NP_RANGE + 1])
def test_escape_fill_values_at_the_speculative_gate(td, fill):
    """the fused pass is taken speculatively only for 255 <= fill <= NP_RANGE; either side of the gate gives the optimum"""
    n_s, n_d = 2200, 1000
    V = 254 if fill >= 255 else 253
    C = escape_model(n_s, n_d, V, fill, seed=fill % 9973)
    cost, opt, st, st2 = solve_both(td, C, fill)
    if 255 <= fill <= NP_RANGE:
        assert st["transposed"] == 1 and st["bytes_per_cell"] == 4, st   # the real 254 leaves the escape cells
    if fill > 255:
        assert oracle.assign(dearer(cost, n_s - 1, n_d - 1, fill))[0] != opt


# ---------------------------------------------------------------------------------------------------------------------
# 4: the packed bid key at its real edge
# ---------------------------------------------------------------------------------------------------------------------
def test_bid_key_guard_at_its_edge(general_solver):
    td = general_solver
    for n in (930, 931):
        bases = np.full(n, I32_MIN, np.int64)
        c, g, opt, u, v = trap(n, U32, 0, n - 1, seed=n, bases=bases)
        assert row_range(c) == U32
        if n == 930:   # (2^32 - 1) * 931 < 4e12
            _, st = check_host(td, c, g, opt, u, v)
            check_width(st, U32, n)
        else:
            with pytest.raises(td.TdError, match="packed bid key"):
                td.assign(c)
    rng = np.random.default_rng(5)
    c = rng.integers(-1000, 1000, (40, 40)).astype(np.int32)
    c[7, 3], c[7, 30] = I32_MIN, I32_MAX
    with pytest.raises(td.TdError, match="exceeds 2\\^32-2"):
        td.assign(c)


# ---------------------------------------------------------------------------------------------------------------------
# 5: the shard API
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,L", [(1, U8), (2, U16), (4, U32)])
def test_shard_compress_fits_exactly_at_the_limit(general_solver, width, L):
    import torch
    from taxidispatcher_amd import sharded
    td = general_solver
    n = 40
    for R in (L, L + 1):
        if R > U32:   # INT32_MIN .. INT32_MAX in one row
            c, g, opt, u, v = trap(n, U32, n - 1, n - 1, seed=width, bases=np.full(n, I32_MIN, np.int64))
            c[n - 1, n - 1] = I32_MAX
        else:
            c, g, opt, u, v = trap(n, R, n - 1, n - 1, seed=width)
        assert row_range(c) == R
        sh = sharded.HipShard(n, 0, n, torch.from_numpy(c).cuda(), share_torch_stream=False)
        try:
            assert sh.compress(width) == (R == L), (width, R)
        finally:
            sh.close()
        if R > L:
            continue
        shards = [sharded.HipShard(n, 0, n, torch.from_numpy(c).cuda(), share_torch_stream=False)]
        try:
            r2c, tot, dual, info = sharded.solve_shards_in_process(shards)
        finally:
            for s in shards:
                s.close()
        ref, ref_tot = td.assign(c)
        assert tot == dual == ref_tot == opt
        assert np.array_equal(r2c, ref) and np.array_equal(r2c, g["perm"])


# ---------------------------------------------------------------------------------------------------------------------
# 6: batched kernels with the whole int32 range
# ---------------------------------------------------------------------------------------------------------------------
def extreme_model(n, seed):
    """full-int32 cells: INT32_MIN and INT32_MAX in one row, random rows across the whole range"""
    rng = np.random.default_rng(seed)
    c = rng.integers(I32_MIN, I32_MAX, (n, n), dtype=np.int64, endpoint=True)
    if n >= 2:
        i = int(rng.integers(0, n))
        c[i, int(rng.integers(0, n))] = I32_MIN
        c[i, n - 1] = I32_MAX
        c[n - 1, 0] = I32_MAX
        c[0, n - 1] = I32_MIN
    return c.astype(np.int32)


def numpy_dual(c, v):
    c = c.astype(np.int64)
    return int((c - v[None, :]).min(axis=1).sum() + v.sum()) if c.size else 0


@pytest.mark.parametrize("n", [64, 65, 124, 125, 128, 129, 256, 257, 512, 513, 1024])
def test_assign_batched_full_int32_range(td, n):
    B = 2 if n >= 512 else 3
    ns = np.full(B, n, np.int32)
    ns[-1] = max(1, n - 61)   # ragged
    slab = np.full((B, n, n), I32_MAX, np.int32)
    mats = []
    for b in range(B):
        k = int(ns[b])
        m = extreme_model(k, 100 * n + b)
        slab[b, :k, :k] = m
        mats.append(m)
    r2c, total, dual, price = td.assign_batched(slab, ns=ns, want_dual=True, want_prices=True)
    for b, c in enumerate(mats):
        k = c.shape[0]
        assert total[b] == oracle.assign(c)[0], (n, b)
        p = r2c[b, :k]
        assert sorted(p.tolist()) == list(range(k))
        assert int(c.astype(np.int64)[np.arange(k), p].sum()) == total[b]
        assert dual[b] == total[b]
        assert numpy_dual(c, price[b, :k]) == total[b]
        assert (r2c[b, k:] == -1).all()


RULES = {
    "heuristic": (dict(mask=100, threshold=-1), dict(mask=100, threshold=-1)),
    "greedy_opt": (dict(mask=BIG, threshold=10, sum_below=BIG), dict(mask=BIG, threshold=10, sum_below=BIG)),
    "simulator": (dict(mask=BIG, stop_value_on=1, stop_value=BIG, stop_size=4, sum_below=BIG),
                  dict(mask=BIG, stop_value_on=1, stop_value=BIG, stop_size=4, sum_below=BIG, java_scan=1)),
}


def lcm_expected(c, kw_oracle):
    """What td_lcm / td_lcm_batched must return: the reference's greedy (the oracle) under the documented deviation of
    DESIGN.md section 3.  The GPU never picks a masked cell or a cell >= mask; once the smallest live cell is >= mask it
    stops, and last_min is that live cell.  The reference instead takes the first minimum of the WHOLE matrix, masked
    cells (value = mask) included: it goes on picking masked cells, adding the mask to its total, and reports the mask
    as last_min.  Up to the first such pick pairs, total and last_min are the reference's."""
    t_o, r_o, c_o, lm_o = oracle.lcm(c, **kw_oracle)
    if kw_oracle.get("java_scan"):   # cells >= stop_value (= mask) are never candidates there: no deviation possible
        return t_o, r_o, c_o, lm_o
    mask, sum_below = kw_oracle["mask"], kw_oracle.get("sum_below", 2**62)
    n = c.shape[0]
    taken_r, taken_c = np.zeros(n, bool), np.zeros(n, bool)
    p, tot = r_o.size, 0
    for k, (i, j) in enumerate(zip(r_o.tolist(), c_o.tolist())):
        val = mask if (taken_r[i] or taken_c[j]) else int(c[i, j])   # the value the reference reads there
        if val >= mask:
            p = k
            break
        tot += val if val < sum_below else 0
        taken_r[i] = taken_c[j] = True
    live = c[np.ix_(~taken_r, ~taken_c)]
    live_min = int(live.min()) if live.size else None
    if p == r_o.size and not (lm_o == mask and live_min is not None and live_min > mask):
        return t_o, r_o, c_o, lm_o     # the reference never read a masked cell as its minimum
    assert tot == t_o or p < r_o.size
    return tot, r_o[:p], c_o[:p], live_min


@pytest.mark.parametrize("rule,above_mask", [(r, a) for r in sorted(RULES) for a in (False, True)])
def test_lcm_full_int32_range(td, rule, above_mask):
    """INT32_MIN in every model; with above_mask, INT32_MAX as well (the whole int32 range: cells above the mask, where
    the documented deviation applies); otherwise every cell is below the rule's mask value, as in every reference model"""
    from taxidispatcher_amd import dispatch
    kw_gpu, kw_oracle = RULES[rule]
    deviated = 0
    for n in (64, 125, 129, 513):
        B = 3
        ns = np.array([n, n - 1, max(1, n // 2)], np.int32)
        slab = np.full((B, n, n), I32_MIN, np.int32)
        mats = []
        for b in range(B):
            k = int(ns[b])
            m = extreme_model(k, 7 * n + b)
            if not above_mask:
                m = np.minimum(m, kw_gpu["mask"] - 1 - (m & 7)).astype(np.int32)
            if b == 1:   # unreachable cells (below the mask unless the model spans the whole range)
                m[m % 5 == 0] = BIG if above_mask else kw_gpu["mask"] - 1
            slab[b, :k, :k] = m
            mats.append(m)
        total, rows, cols, lm, npairs = td.LCM_batched(slab, ns=ns, **kw_gpu)
        for b, c in enumerate(mats):
            t_e, r_e, c_e, lm_e = lcm_expected(c, kw_oracle)
            t_o, r_o, c_o, lm_o = oracle.lcm(c, **kw_oracle)
            deviated += (t_e, r_e.size, lm_e) != (t_o, r_o.size, lm_o)
            if not above_mask:
                assert (t_e, r_e.tolist(), c_e.tolist(), lm_e) == (t_o, r_o.tolist(), c_o.tolist(), lm_o)
            k = int(npairs[b])
            assert k == r_e.size, (rule, n, b, k, r_e.size)
            assert rows[b, :k].tolist() == r_e.tolist() and cols[b, :k].tolist() == c_e.tolist(), (rule, n, b)
            assert total[b] == t_e and lm[b] == lm_e, (rule, n, b, int(total[b]), t_e, int(lm[b]), lm_e)
            kw = dict(kw_gpu)
            t1, r1, c1, lm1 = dispatch._lcm(c.shape[0], c, kw.get("mask"), kw.get("threshold", -1), kw.get("stop_value_on", 0),
                                            kw.get("stop_value", 0), kw.get("stop_size", -1), kw.get("sum_below", 2**62))
            assert r1.tolist() == r_e.tolist() and c1.tolist() == c_e.tolist() and t1 == t_e and lm1 == lm_e, (rule, n, b)
    if above_mask and rule != "simulator":
        assert deviated > 0   # these models do reach the cells above the mask
