"""The case table of tests/test_line_paths_cpu.py and tests/test_gpu_line_paths.py: td_assign inputs that sit on every branch of
the line-metric attempt (csrc/td_line.hip): the probe's sampling and its fallback branches, the scan bases of k_line_scan and of
k_line_unbal's wg_scan, the 64-bit price width, the certificate's two variants and its last row group, the unbalanced plan's
edges, the transposed retry (DESIGN.md 2.9 has the table of constants).  Plain numpy: nothing here needs a GPU.

A case is a dict: name, n, the positions `a` (cabs, one per REAL row) and `b` (requests, one per REAL column) as int64, `fill`,
`dummy_rows` / `dummy_cols` (indices of the constant rows / columns of the n x n matrix), `perturb` (None or (row, col, value):
one cell overwritten), `via` (how the matrix reaches the library: "host" array, "device" tensor, "device_off4" a device tensor
one int32 behind a 16-byte boundary), `bits` (the `line_path` word, td_last_stats word 12, the call must show), `refused`,
`stats` (line_metric, line_dummies, transposed) and `claims`: the structural conditions that make it a case for its edge, which
the CPU tier confirms from the references alone, so that the table cannot drift into cases that test nothing.

A bug on this path is slow, not wrong: the answer is used only when k_line_cert accepts it, anything else falls through to the
general solver with the same total.  So every case that is not marked refused must be ACCEPTED, with exactly its bits.

References, never the code under test: the sorted matching for a balanced model, order_preserving_total (a dynamic program by
rows, independent of the kernel's prefix-min-by-shift formulation) plus k * fill for an unbalanced one, the oracle on the
perturbed matrix for the refused cases.  probe_model / expected_bits restate k_line_probe's and line_finish's decisions from the
constants below, reading rows and columns through a Model (positions, not a matrix), so they serve every n.
CASE_NAMES is the static list the tests are parametrised over; case(name) builds on first use, reference(name) is computed
once per process and shared."""
import functools

import numpy as np

from oracle import oracle
from test_line_math import certificate_holds, unbalanced_plan

BIG = 250000
I32_MAX = 2**31 - 1

# ---- the thresholds the table sits on, each with the line of csrc/td_line.hip it restates
PROBE_T = 1024           # k_line_probe<<<1, 1024>>>: `if (t < n)`, `if (t < nsamp)` tests see the first 1024 cells / samples
PROBE_SAMPLES = 1024     # k_line_probe: `const int step = n > 1024 ? n / 1024 : 1`
SCAN_BASE = 1024 * 16    # k_line_scan: `for (int base = 0; base < n; base += T * CH)` with CH = 16
WG_SCAN_BASE = 1024 * 8  # wg_scan: `for (int base = 0; base < len; base += T * CH)` with CH = 8
PRICE32 = 1 << 30        # k_line_scan: `out |= price < -(1ll << 30) || price > (1ll << 30)`; k_line_unbal: `if (pr < -(1ll << 30)) wide = 1`
LINE_KMAX = 256          # `constexpr int LINE_KMAX = 256`; k_line_probe: `kdummy >= 1 && kdummy <= LINE_KMAX && n - kdummy >= 2`
CERT_R = 4               # line_finish: `constexpr int R = 4` rows per workgroup sweep, `std::min(r0 + r, nrows - 1)`
CERT_VEC = 4             # line_finish: `const bool vec = (n % 4 == 0) && (((uintptr_t)d_cost & 15) == 0)`
C1_SEARCH = 64           # k_line_probe (constant last column): `if (t < 64) { const int j = 1 + t;` the transposed probe's second column
DENSE_MAX = 3000         # (this module) largest n whose matrix the CPU tier builds
DEVICE_MIN = 8192        # (this module) from this n on the GPU tier builds the matrix on the device

# ---- td_last_stats word 12 (include/taxidispatcher_amd.h)
PROBE, BALANCED, TRANSPOSE, UNBAL, QROW2, I2SEARCH, I2COLQ, REV, VEC, WIDE, ACCEPTED = (1 << k for k in range(11))


# ======================================================================================================================
# the matrix: by positions (any n) and dense (numpy, torch)
# ======================================================================================================================
class Model:
    """rows, columns and cells of the n x n matrix of a case, computed from the positions: what the probe reads, at any n"""

    def __init__(self, c, transposed=False):
        n = c["n"]
        self.n, self.fill, self.perturb = n, int(c["fill"]), c["perturb"]
        A, rd = _expand(n, c["a"], c["dummy_rows"])
        B, cd = _expand(n, c["b"], c["dummy_cols"])
        if transposed:
            A, rd, B, cd = B, cd, A, rd
            if self.perturb is not None:
                self.perturb = (self.perturb[1], self.perturb[0], self.perturb[2])
        self.A, self.rd, self.B, self.cd = A, rd, B, cd

    def row(self, i):
        r = np.where(self.cd | self.rd[i], self.fill, np.abs(self.A[i] - self.B))
        if self.perturb is not None and self.perturb[0] == i:
            r[self.perturb[1]] = self.perturb[2]
        return r

    def col(self, j):
        r = np.where(self.rd | self.cd[j], self.fill, np.abs(self.A - self.B[j]))
        if self.perturb is not None and self.perturb[1] == j:
            r[self.perturb[0]] = self.perturb[2]
        return r

    def cell(self, i, j):
        return int(self.row(i)[j])


def _expand(n, pos, dummies):
    """positions of the real lines spread over n lines, and the mask of the constant ones"""
    mask = np.zeros(n, bool)
    mask[list(dummies)] = True
    full = np.zeros(n, np.int64)
    assert int((~mask).sum()) == len(pos)
    full[~mask] = pos
    return full, mask


def numpy_matrix(c):
    """|a_i - b_j| in int64, the constant lines, the perturbed cell, then the cast to int32 (n <= DENSE_MAX on the CPU tier)"""
    m = Model(c)
    M = np.abs(m.A[:, None] - m.B[None, :])
    M[m.rd, :] = m.fill
    M[:, m.cd] = m.fill
    if c["perturb"] is not None:
        M[c["perturb"][0], c["perturb"][1]] = c["perturb"][2]
    assert int(M.min()) >= 0 and int(M.max()) <= I32_MAX
    return M.astype(np.int32)


def torch_matrix(c, torch, out=None, rows_per_block=2048):
    """the same on the device: int64 differences in blocks of rows (the int64 form of a whole large matrix is never held),
    cast to int32 into `out` (an n x n int32 device tensor; made here when None)"""
    m = Model(c)
    n = m.n
    if out is None:
        out = torch.empty((n, n), dtype=torch.int32, device="cuda")
    A, B = torch.as_tensor(m.A, device="cuda"), torch.as_tensor(m.B, device="cuda")
    rd, cd = torch.as_tensor(m.rd, device="cuda"), torch.as_tensor(m.cd, device="cuda")
    for r0 in range(0, n, rows_per_block):
        r1 = min(n, r0 + rows_per_block)
        blk = (A[r0:r1, None] - B[None, :]).abs()
        blk[rd[r0:r1], :] = m.fill
        blk[:, cd] = m.fill
        out[r0:r1] = blk.to(torch.int32)
    if c["perturb"] is not None:
        out[c["perturb"][0], c["perturb"][1]] = c["perturb"][2]
    return out


# ======================================================================================================================
# k_line_probe and line_finish restated
# ======================================================================================================================
def _span_ok(x, y, D):
    return (x + y == D) | (np.abs(x - y) == D)


def probe_model(m):
    """k_line_probe on a Model: dict(mode, q, rq, i2, path, rev, k).  One workgroup of PROBE_T threads: the `t < n` tests see the
    first PROBE_T cells, the sampled-row loops every sample."""
    n, p, i1 = m.n, 0, 0
    step = n // PROBE_SAMPLES if n > PROBE_SAMPLES else 1
    nsamp = (n + step - 1) // step
    samp = np.arange(nsamp) * step
    first = min(n, PROBE_T)
    r0, r1 = m.row(0), m.row(1)
    u0, w0 = int(r0[0]), int(r1[0])
    Ea, Eb = u0 + w0, abs(u0 - w0)
    B0, B1 = m.cell(n - 1, 0), int(r0[n - 1])
    out = dict(mode=0, q=-1, rq=0, i2=-1, path=0, rev=0, k=0, step=step, nsamp=nsamp)
    bad_a = bool((~_span_ok(r0[:first], r1[:first], Ea)).any())
    bad_b = bool((~_span_ok(r0[:first], r1[:first], Eb)).any())
    rows_dummy = bool((m.row(n - 1)[:first] == B0).all())
    colp, col_last = m.col(p), m.col(n - 1)
    cols_dummy = bool((col_last[samp[:PROBE_T]] == B1).all())
    if cols_dummy:
        real = np.flatnonzero(colp[:first] != B1)
        if real.size == 0 or rows_dummy:
            return out
        r = int(real[0])
        rr = m.row(r)
        diff = np.flatnonzero(rr[1:min(n, 1 + C1_SEARCH)] != rr[0])
        c1 = 1 + int(diff[0]) if diff.size else 1
        out["c1"] = c1
        ur, wr = int(rr[0]), int(rr[c1])
        x, y = colp[:first], m.col(c1)[:first]
        bad_c, bad_d = bool((~_span_ok(x, y, ur + wr)).any()), bool((~_span_ok(x, y, abs(ur - wr))).any())
        out["mode"] = 0 if (bad_c and bad_d) else 2
        return out
    if bad_a and bad_b:
        return out
    cols_ok = not (bool((~_span_ok(r0, r1, Ea)).any()) and bool((~_span_ok(r0, r1, Eb)).any()))
    d = np.abs(r0 - u0)
    q = int(np.argmax(d)) if d.max() != 0 else -1      # ties: the smallest index (better())
    rq = 0
    if cols_ok and q < 0:
        rq = 1 if rows_dummy else n // 2
        row = m.row(rq)
        d = np.abs(row - row[p])
        q = int(np.argmax(d)) if d.max() != 0 else -1
        out["path"] |= QROW2
    out["q"], out["rq"] = q, rq
    i2 = -1
    if cols_ok and q >= 0:
        colq = m.col(q)
        if w0 != u0 or r1[q] != r0[q]:
            i2 = 1
        else:
            for attempt, colv in enumerate((colp, colq)):
                if i2 >= 0:
                    break
                dummy = rows_dummy & (colp[samp] == B0) & (colq[samp] == B0)
                d = np.where(dummy, 0, np.abs(colv[samp] - colv[i1]))
                if d.max() != 0:
                    i2 = int(samp[int(np.argmax(d))])
                out["path"] |= I2COLQ if attempt else I2SEARCH
            if i2 >= 0:
                ra, rb = m.row(i1), m.row(i2)
                Fa, Fb = int(colp[i1] + colp[i2]), abs(int(colp[i1] - colp[i2]))
                cols_ok = not (bool((~_span_ok(ra, rb, Fa)).any()) and bool((~_span_ok(ra, rb, Fb)).any()))
    out["i2"] = i2
    if cols_ok and q >= 0 and i2 >= 0:
        x0, y0 = int(colp[rq]), int(colq[rq])
        x, y = colp[samp], colq[samp]
        keep = ~(rows_dummy & (x == B0) & (y == B0))
        bad_a = bool((~_span_ok(x, y, x0 + y0))[keep].any())
        bad_b = bool((~_span_ok(x, y, abs(x0 - y0)))[keep].any())
        mode = int(not (bad_a and bad_b))
        if mode and rows_dummy:
            k = int(((colp == B0) & (colq == B0)).sum())
            out["k"] = k
            mode = 3 if (1 <= k <= LINE_KMAX and n - k >= 2) else 0
        out["mode"] = mode
        K1 = int(colp[i1]) ** 2 - int(colq[i1]) ** 2
        K2 = int(colp[i2]) ** 2 - int(colq[i2]) ** 2
        out["rev"] = int(K2 < K1)
    return out


def plan(m, pr):
    """The plan k_line_keys .. k_line_scan / k_line_unbal make after verdict pr["mode"] in (1, 3), from the positions:
    (sig, tau, prices by column or None).  Row keys from columns (0, q), column keys from rows (0, i2), negated when rev; the
    radix sort is stable, so is the argsort.  Prices: balanced the exclusive prefix sums of f (O(n), any n); unbalanced
    test_line_math.unbalanced_plan on the sorted positions (n <= DENSE_MAX: it builds the sorted matrix)."""
    n = m.n
    colp, colq = m.col(0), m.col(pr["q"])
    rk = colp ** 2 - colq ** 2
    ck = m.row(0) ** 2 - m.row(pr["i2"]) ** 2
    if pr["rev"]:
        ck = -ck
    tau = np.argsort(ck, kind="stable")
    if pr["mode"] == 1:
        sig = np.argsort(rk, kind="stable")
        As = m.A[sig[:-1]]
        f = np.abs(As - m.B[tau[1:]]) - np.abs(As - m.B[tau[:-1]])
        v = np.zeros(n, np.int64)
        v[tau[1:]] = np.cumsum(f)
        r2c = np.empty(n, np.int64)
        r2c[sig] = tau
        return r2c, v
    const = (colp == m.fill) & (colq == m.fill)
    real = np.flatnonzero(~const)
    sig = np.concatenate([real[np.argsort(rk[real], kind="stable")], np.flatnonzero(const)])
    if n > DENSE_MAX:
        return None, None
    _, r2c_s, v_s, _ = unbalanced_plan(m.A[sig[:real.size]], m.B[tau])
    r2c, v = np.empty(n, np.int64), np.empty(n, np.int64)
    r2c[sig] = tau[r2c_s]
    v[tau] = v_s
    return r2c, v


def span(c):
    """the distance between the outermost positions: no price of either plan leaves +-span (a price is a sum of adjacent
    differences f, |f| <= the gap between two neighbouring requests, each gap counted once)"""
    lo = min(int(c["a"].min()), int(c["b"].min()))
    return max(int(c["a"].max()), int(c["b"].max())) - lo


def finished_probe(c):
    """the probe on the caller's matrix and, after verdict 2, on the transpose: (bits so far, the Model the attempt goes on
    with, its verdict, whether that matrix is 16-byte aligned)"""
    bits = PROBE
    m = Model(c)
    pr = probe_model(m)
    aligned = c["via"] != "device_off4"
    if pr["mode"] == 2:
        bits |= TRANSPOSE
        m = Model(c, transposed=True)
        pr = probe_model(m)
        aligned = True          # the library's own transposed copy
    return bits, m, pr, aligned


def expected_bits(c):
    """td_assign's line attempt restated: (bits, the Model that is finished, its probe verdict, (row_to_col, prices) of the
    plan or Nones).  The ACCEPTED bit is set when the attempt reaches line_finish on an unperturbed model: a true line metric
    must certify."""
    bits, m, pr, aligned = finished_probe(c)
    if pr["mode"] not in (1, 3):
        return bits, m, pr, (None, None)
    bits |= (BALANCED if pr["mode"] == 1 else UNBAL) | pr["path"] | (REV if pr["rev"] else 0)
    if c["n"] % CERT_VEC == 0 and aligned:
        bits |= VEC
    r2c, v = plan(m, pr)
    if v is None:
        assert span(c) <= PRICE32     # the bound of span(): no price can be wide
        wide = False
    elif pr["mode"] == 1:
        wide = bool((v < -PRICE32).any() or (v > PRICE32).any())
    else:
        wide = bool((v < -PRICE32).any())
    bits |= WIDE if wide else 0
    if c["perturb"] is None:
        bits |= ACCEPTED
    return bits, m, pr, (r2c, v)


# ======================================================================================================================
# references
# ======================================================================================================================
def sorted_matching_total(a, b):
    return int(np.abs(np.sort(a) - np.sort(b)).sum())


def order_preserving_total(few, many):
    """m = len(few) points matched to m of the m + k points of `many` without crossing: row by row, prev[d] = the cheapest way
    to have matched the rows so far with the last one shifted by at most d"""
    a_s, b_s = np.sort(np.asarray(few, np.int64)), np.sort(np.asarray(many, np.int64))
    m, k = a_s.size, b_s.size - a_s.size
    assert k >= 0
    prev = np.zeros(k + 1, np.int64)
    for i in range(m):
        prev = np.minimum.accumulate(prev + np.abs(a_s[i] - b_s[i:i + k + 1]))
    return int(prev[k])


def model_total(c):
    """the optimum of an unperturbed case from its positions"""
    a, b = c["a"], c["b"]
    k = abs(a.size - b.size)
    if k == 0:
        return sorted_matching_total(a, b)
    few, many = (a, b) if a.size < b.size else (b, a)
    return order_preserving_total(few, many) + k * int(c["fill"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """the optimal total: from the positions, or the oracle's on the perturbed matrix"""
    c = case(name)
    if c["perturb"] is not None:
        assert c["n"] <= 1028
        return int(oracle.assign(numpy_matrix(c))[0])
    return model_total(c)


# ======================================================================================================================
# the table
# ======================================================================================================================
_BUILDERS = {}


def _add(name, fn):
    assert name not in _BUILDERS, name
    _BUILDERS[name] = fn


def _case(a, b, core, claims=(), fill=BIG, dummy_rows=None, dummy_cols=None, via=None, perturb=None, refused=False, rev=None,
          eighth=None):
    """`core`: the bits the case states, but for REV where rev is None: generic positions leave the direction of the two key
    orders to chance, there the bit is the probe model's (the rev_on / rev_off cases state it)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    n = max(a.size, b.size)
    dr = tuple(range(a.size, n)) if dummy_rows is None else tuple(dummy_rows)
    dc = tuple(range(b.size, n)) if dummy_cols is None else tuple(dummy_cols)
    assert len(dr) == n - a.size and len(dc) == n - b.size
    if via is None:
        via = "device" if n >= DEVICE_MIN else "host"
    c = dict(n=n, a=a, b=b, fill=fill, dummy_rows=dr, dummy_cols=dc, via=via, perturb=perturb, refused=refused,
             claims=tuple(claims), eighth=eighth)
    if rev is None:
        _, _, pr, _ = finished_probe(c)
        rev = bool(pr["rev"]) and pr["mode"] in (1, 3)
    c["bits"] = core | (REV if rev else 0)
    accepted = bool(c["bits"] & ACCEPTED)
    assert accepted != refused
    c["stats"] = dict(line_metric=int(accepted), line_dummies=(len(dr) + len(dc)) if accepted else 0,
                      transposed=int(accepted and len(dc) > 0))
    return c


def _generic(seed, na, nb, S=None):
    """distinct cab stands and distinct request stands among S = 10 n"""
    n = max(na, nb)
    rng = np.random.default_rng(seed)
    S = 10 * n if S is None else S
    return rng.permutation(S)[:na].astype(np.int64), rng.permutation(S)[:nb].astype(np.int64)


def _vec(n):
    return VEC if n % CERT_VEC == 0 else 0


# ---- balanced, generic positions: the probe's sampling (n = 1025 .. 2049), the ragged last row group of the certificate
# (n % 4 = 1, 2, 3), the 16-byte variant from a host array, a device tensor and a device tensor 4 bytes off, and the second
# trip through k_line_scan's base loop (n = 16385; 16384 is test_gpu_line.py's)
def _balanced(n, seed, via=None):
    def build():
        a, b = _generic(seed, n, n)
        step = n // PROBE_SAMPLES if n > PROBE_SAMPLES else 1
        claims = [("sampling", step, (n + step - 1) // step), ("scan_trips", (n + SCAN_BASE - 1) // SCAN_BASE),
                  ("last_group_rows", n - (n - 1) // CERT_R * CERT_R)]
        core = PROBE | BALANCED | (_vec(n) if via != "device_off4" else 0) | ACCEPTED
        return _case(a, b, core, claims, via=via, eighth=lambda: _balanced(max(2, n // 8), seed)())
    return build


for _n in (1025, 1026, 1027, 2047, 2048, 2049, 16383, 16385):
    _add("balanced_n%d" % _n, _balanced(_n, 100 + _n))
_add("vec_host_n1028", _balanced(1028, 1128, "host"))
_add("vec_device_n1028", _balanced(1028, 1128, "device"))
_add("vec_off4_n1028", _balanced(1028, 1128, "device_off4"))


# ---- the probe's fallback branches (random positions never produce them), at one loop trip and at nsamp > blockDim
def _blind_row0(n, k):
    """every request at distance d of cab 0, on both sides: row 0 sees one distance, q comes from row n / 2 (row 1 when there
    are constant rows)"""
    def build():
        rng = np.random.default_rng(200 + n + k)
        d = 7 * n
        a = rng.permutation(10 * n)[:n - k].astype(np.int64) + d
        b = np.where(rng.integers(0, 2, n) == 1, a[0] + d, a[0] - d)
        b[0], b[n - 1] = a[0] - d, a[0] + d
        core = PROBE | (UNBAL if k else BALANCED) | QROW2 | _vec(n) | ACCEPTED
        return _case(a, b, core, [("blind_row0", 1 if k else n // 2)])
    return build


def _rows01_same(n):
    def build():
        a, b = _generic(300 + n, n, n)
        a[1] = a[0]
        step = n // PROBE_SAMPLES if n > PROBE_SAMPLES else 1
        return _case(a, b, PROBE | BALANCED | I2SEARCH | _vec(n) | ACCEPTED, [("rows01_same",), ("sampling", step, (n + step - 1) // step)])
    return build


def _rows01_same_colp_blind(n):
    """every cab at distance d of request 0: column 0 cannot tell any two rows apart, the search finds i2 on column q"""
    def build():
        rng = np.random.default_rng(400 + n)
        d = 20 * n
        b = rng.permutation(10 * n)[:n].astype(np.int64) + d
        side = rng.integers(0, 2, n)
        side[:2] = 0
        side[2:2 + (n + 1) // 2] = 1
        a = np.where(side == 1, b[0] + d, b[0] - d)
        return _case(a, b, PROBE | BALANCED | I2SEARCH | I2COLQ | _vec(n) | ACCEPTED, [("colp_blind",)])
    return build


def _rev(n, on):
    def build():
        a, b = _generic(500 + n, n, n)
        a, b = np.sort(a), np.sort(b)
        if on:
            b = b[::-1].copy()
        return _case(a, b, PROBE | BALANCED | _vec(n) | ACCEPTED, [("rev", on)], rev=on)
    return build


for _n in (64, 1025):
    _add("blind_row0_n%d" % _n, _blind_row0(_n, 0))
    _add("blind_row0_dummies3_n%d" % _n, _blind_row0(_n, 3))
    _add("rows01_same_n%d" % _n, _rows01_same(_n))
    _add("rows01_same_colp_blind_n%d" % _n, _rows01_same_colp_blind(_n))
    _add("rev_on_n%d" % _n, _rev(_n, True))
    _add("rev_off_n%d" % _n, _rev(_n, False))
_add("rows01_same_n2049", _rows01_same(2049))


# ---- 64-bit prices: the requests span more than 2^30 and every cab lies beyond them; the mirror image is the control
WIDE_LO, WIDE_HI = 2**31 - 1002, 2**31 - 2      # the far cluster, both ends inclusive


def _wide(m, k, mirror):
    def build():
        rng = np.random.default_rng(600 + m + k + 50 * mirror)
        far_n, wide_n = (m + k, m) if mirror else (m, m + k)
        far = rng.integers(WIDE_LO, WIDE_HI + 1, far_n)
        wide = rng.integers(0, WIDE_LO, wide_n)
        wide[0], wide[1] = 0, WIDE_LO - 1        # the span is there whatever the seed
        a, b = (wide, far) if mirror else (far, wide)
        n = m + k
        core = PROBE | (UNBAL if k else BALANCED) | _vec(n) | (0 if mirror else WIDE) | ACCEPTED
        return _case(a, b, core, [("wide", not mirror), ("last_group_rows", n - (n - 1) // CERT_R * CERT_R)], fill=I32_MAX)
    return build


for _n in (1025, 1026, 1027):
    _add("wide_balanced_n%d" % _n, _wide(_n, 0, False))
_add("wide_balanced_control_n1026", _wide(1026, 0, True))
_add("wide_unbalanced_m509_k3", _wide(509, 3, False))
_add("wide_unbalanced_m1025_k3", _wide(1025, 3, False))
_add("wide_unbalanced_control_m509_k3", _wide(509, 3, True))


# ---- certificate reach: one cell lowered to 0 where no span test of the probe reads it; the optimum moves, so only
# k_line_cert can (and must) refuse.  The seed of each case is the first one of its sequence for which the claim holds.
def _reach(n, where, seed):
    def build():
        a, b = _generic(seed, n, n)
        i, j = {"last_last": (n - 1, n - 1), "last_row": (n - 1, 5), "last_col": (7, n - 1)}[where]
        return _case(a, b, PROBE | BALANCED | _vec(n), [("reach", i, j)], perturb=(i, j, 0), refused=True)
    return build


REACH_SEEDS = {(1025, "last_last"): 700, (1025, "last_row"): 751, (1025, "last_col"): 702,
               (1028, "last_last"): 703, (1028, "last_row"): 704, (1028, "last_col"): 715}
for (_n, _w), _s in REACH_SEEDS.items():
    _add("reach_n%d_%s" % (_n, _w), _reach(_n, _w, _s))


# ---- the unbalanced plan: its scans' base of 8192 (m real rows: OpSum over m, OpMinArg over m + 1, OpClamp over m - 1 both
# ways), the small edges against the oracle, n - k = 2 / 1, k = LINE_KMAX / + 1, constant lines that are not the trailing ones
def _unbal(m, k, seed, side="cabs", claims=()):
    def build():
        n = m + k
        a, b = _generic(seed, m, n) if side == "cabs" else _generic(seed, n, m)
        scans = [("wg_scan_trips", nm, ln, (ln + WG_SCAN_BASE - 1) // WG_SCAN_BASE) for nm, ln in (("sum", m), ("minarg", m + 1), ("clamp", m - 1))]
        ok = k <= LINE_KMAX and m >= 2
        core = PROBE | ((UNBAL | _vec(n) | ACCEPTED | (TRANSPOSE if side == "requests" else 0)) if ok else 0)
        return _case(a, b, core, list(claims) + (scans if ok else [("probe_refuses",)]), refused=not ok,
                     eighth=lambda: _unbal(max(2, m // 8), k, seed, side)())
    return build


for _m in (8191, 8192, 8193):
    for _k in (1, 2):
        _add("unbal_m%d_k%d" % (_m, _k), _unbal(_m, _k, 800 + _m + _k))
for _k in (1, 2):
    _add("unbal_requests_m8193_k%d" % _k, _unbal(8193, _k, 820 + _k, "requests"))
for _m in (2, 3, 63, 64, 65, 1023, 1024, 1025):
    for _k in (1, 3):
        _add("unbal_m%d_k%d" % (_m, _k), _unbal(_m, _k, 840 + _m + _k))
_add("unbal_m2_k2", _unbal(2, 2, 860))
_add("unbal_m2_k256", _unbal(2, LINE_KMAX, 861, claims=[("kmax",)]))
_add("unbal_m1_k2_refused", _unbal(1, 2, 862))
_add("unbal_m1_k257_refused", _unbal(1, LINE_KMAX + 1, 863))


def _scattered(side):
    def build():
        n = 130
        lines = (2, 40, 41, 100, n - 1) if side == "cabs" else (70, 90, 100, n - 1)
        k = len(lines)
        a, b = _generic(870 + k, n - k, n) if side == "cabs" else _generic(870 + k, n, n - k)
        core = PROBE | UNBAL | ACCEPTED | (TRANSPOSE if side == "requests" else 0) | _vec(n)
        kw = dict(dummy_rows=lines) if side == "cabs" else dict(dummy_cols=lines)
        return _case(a, b, core, [("scattered", side, lines)], **kw)
    return build


_add("dummies_scattered_rows", _scattered("cabs"))
_add("dummies_scattered_cols", _scattered("requests"))

CASE_NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    d = dict(_BUILDERS[name](), name=name)
    d["a"].setflags(write=False)
    d["b"].setflags(write=False)
    return d
