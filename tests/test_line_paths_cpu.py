"""CPU tier of the line-path suite: every case of tests/line_path_cases.py is confirmed from the references alone, without a
GPU and without the library: its structural claims hold, its `line_path` bits follow from the claims and the constants (the probe
and the finish restated in numpy), the numpy plan certifies on the numpy matrix with the reference's total (n <= DENSE_MAX), and
above that the two references agree on a 1/8-size model of the same construction.  So a tie-heavy case is known to be certifiable
before the GPU is asked to accept it, and the table cannot drift into cases that test nothing."""
import numpy as np
import pytest

from oracle import oracle

import line_path_cases as L
from test_line_math import certificate_holds


def _check_claim(c, claim, m, pr):
    n, a, b, kind = c["n"], c["a"], c["b"], claim[0]
    if kind == "sampling":        # the probe's row step and sample count; more samples than threads from n = 1025 on
        step, nsamp = claim[1:]
        assert (pr["step"], pr["nsamp"]) == (step, nsamp)
        assert step == (1 if n < 2 * L.PROBE_SAMPLES else n // L.PROBE_SAMPLES)
        if L.PROBE_SAMPLES < n < 2 * L.PROBE_SAMPLES:
            assert step == 1 and nsamp > L.PROBE_T
    elif kind == "scan_trips":    # trips through k_line_scan's base loop
        assert claim[1] == (1 if n <= L.SCAN_BASE else 2)
    elif kind == "last_group_rows":   # real rows of the certificate's last group of CERT_R; the rest are clamped copies
        assert claim[1] == (n % L.CERT_R or L.CERT_R)
    elif kind == "blind_row0":
        d = np.abs(a[0] - b)
        assert (d == d[0]).all() and {int(x) for x in b - a[0]} == {-int(d[0]), int(d[0])}
        assert a[1] != a[0] and a[min(n // 2, a.size - 1)] != a[0] and a[-1] != a[0]
        assert pr["rq"] == claim[1] and pr["path"] & L.QROW2
    elif kind == "rows01_same":
        assert a[0] == a[1] and len(set(a.tolist())) == n - 1 and len(set(b.tolist())) == n
        assert pr["path"] == L.I2SEARCH and a[pr["i2"]] != a[0]
    elif kind == "colp_blind":
        d = np.abs(a - b[0])
        assert (d == d[0]).all() and a[0] == a[1] and int((a != a[0]).sum()) >= n // 2
        assert len(set(b.tolist())) == n and b[-1] != b[0]
        assert pr["path"] == L.I2SEARCH | L.I2COLQ and a[pr["i2"]] != a[0]
    elif kind == "rev":
        # K(i) = (b_q - b_p)(2 a_i - b_p - b_q): the row keys run against the positions when b_q < b_p, and the column keys,
        # (a_i2 - a_i1)(2 b_j - ..) up to sign, must then be negated
        assert (np.diff(a) > 0).all() and (np.diff(b) * (-1 if claim[1] else 1) > 0).all()
        sign = (int(b[pr["q"]]) - int(b[0])) * (int(a[pr["i2"]]) - int(a[0]))
        assert sign != 0 and (sign < 0) == claim[1] == bool(pr["rev"])
    elif kind == "wide":
        far, wide = (a, b) if claim[1] else (b, a)
        assert far.min() >= L.WIDE_LO and far.max() <= L.WIDE_HI and wide.min() == 0 and wide.max() == L.WIDE_LO - 1
        assert L.span(c) > L.PRICE32
    elif kind == "reach":
        i, j = claim[1:]
        clean = dict(c, perturb=None)
        _, m0, pr0, _ = L.expected_bits(clean)
        # the probe reads the same anchors with and without the wrong cell, and none of its span tests reads it: rows 0 (= rq)
        # and i2 over all columns, columns 0 and q over the sampled rows
        assert (pr["mode"], pr["q"], pr["i2"], pr["rq"], pr["rev"]) == (1, pr0["q"], pr0["i2"], 0, pr0["rev"])
        assert i not in (0, pr["i2"]) and j not in (0, pr["q"])
        assert i == n - 1 or j == n - 1       # the last row group (rows clamped by min(r0 + r, nrows - 1)) or the last column
        assert L.reference(c["name"]) < L.model_total(clean)     # the optimum moves: the sorted matching is no longer optimal
    elif kind == "wg_scan_trips":
        _, what, ln, trips = claim
        m_real = min(a.size, b.size)
        assert ln == {"sum": m_real, "minarg": m_real + 1, "clamp": m_real - 1}[what]
        assert trips == (ln + L.WG_SCAN_BASE - 1) // L.WG_SCAN_BASE
    elif kind == "probe_refuses":
        assert pr["mode"] == 0 and (min(a.size, b.size) < 2 or abs(a.size - b.size) > L.LINE_KMAX)
    elif kind == "kmax":
        assert abs(a.size - b.size) == L.LINE_KMAX and min(a.size, b.size) == 2
    elif kind == "scattered":
        _, side, lines = claim
        assert lines[-1] == n - 1 and 0 not in lines and 1 not in lines and list(lines) != list(range(n - len(lines), n))
        if side == "requests":
            assert min(lines) > L.C1_SEARCH and c["dummy_cols"] == tuple(lines)
        else:
            assert c["dummy_rows"] == tuple(lines)
    else:
        raise AssertionError("unknown claim %r" % (claim,))


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_case_claims_bits_and_plan(name):
    c = L.case(name)
    n = c["n"]
    bits, m, pr, (r2c, v) = L.expected_bits(c)
    assert c["claims"], name
    for claim in c["claims"]:
        _check_claim(c, claim, m, pr)
    assert bits == c["bits"], (name, bits, c["bits"])
    assert bool(bits & L.ACCEPTED) != c["refused"]
    assert c["via"] != "host" or n < L.DEVICE_MIN
    ref = L.reference(name)
    if not (bits & (L.BALANCED | L.UNBAL)):      # refused by the probe: nothing to certify; the optimum is the general solver's
        assert c["refused"] and ref == int(oracle.assign(L.numpy_matrix(c))[0])
        return
    if n <= L.DENSE_MAX:
        M = L.numpy_matrix(c)
        if bits & L.TRANSPOSE:
            M = np.ascontiguousarray(M.T)
        assert sorted(r2c.tolist()) == list(range(n))
        total = int(M[np.arange(n), r2c].astype(np.int64).sum())
        wide = bool((v < -L.PRICE32).any() or (v > L.PRICE32).any())
        assert wide == bool(bits & L.WIDE) and (wide or int(np.abs(v).max()) <= L.span(c))
        if c["perturb"] is None:
            assert certificate_holds(M, r2c, v), name     # a true line metric: the plan the kernels make must certify
            assert total == ref, name
        else:
            assert not certificate_holds(M, r2c, v) and total > ref, name
    else:
        # too large for a matrix here: the same construction at 1/8 of the size, the position reference against the oracle
        small = c["eighth"]()
        assert small["n"] <= L.DENSE_MAX and (small["a"].size < small["b"].size) == (c["a"].size < c["b"].size)
        assert L.model_total(small) == int(oracle.assign(L.numpy_matrix(small))[0])
        assert L.span(c) <= L.PRICE32 and not (bits & L.WIDE)


@pytest.mark.parametrize("name", [x for x in L.CASE_NAMES if L.case(x)["n"] <= 130 and L.case(x)["perturb"] is None])
def test_small_cases_against_the_oracle(name):
    c = L.case(name)
    assert L.reference(name) == int(oracle.assign(L.numpy_matrix(c))[0])


def test_references_agree_on_random_models():
    """order_preserving_total against the oracle and against unbalanced_plan's prefix-min scans"""
    from test_line_math import unbalanced_plan
    rng = np.random.default_rng(5)
    for _ in range(100):
        m, k = int(rng.integers(2, 40)), int(rng.integers(1, 6))
        a, b = rng.integers(0, 300, m), rng.integers(0, 300, m + k)
        c = dict(n=m + k, a=a, b=b, fill=L.BIG, dummy_rows=tuple(range(m, m + k)), dummy_cols=(), perturb=None)
        dp = L.order_preserving_total(a, b)
        assert dp == unbalanced_plan(np.sort(a), np.sort(b))[3]
        assert dp + k * L.BIG == int(oracle.assign(L.numpy_matrix(c))[0])


def test_the_table_covers_both_sides_of_every_edge():
    bits = {x: L.case(x)["bits"] for x in L.CASE_NAMES}
    assert bits["rev_on_n64"] ^ bits["rev_off_n64"] == L.REV == bits["rev_on_n1025"] ^ bits["rev_off_n1025"]
    assert bits["vec_host_n1028"] == bits["vec_device_n1028"] == bits["vec_off4_n1028"] | L.VEC
    for w in ("wide_balanced_n1025", "wide_balanced_n1026", "wide_balanced_n1027", "wide_unbalanced_m509_k3", "wide_unbalanced_m1025_k3"):
        assert bits[w] & L.WIDE
    assert not (bits["wide_balanced_control_n1026"] | bits["wide_unbalanced_control_m509_k3"]) & L.WIDE
    seen = 0
    for x in L.CASE_NAMES:
        seen |= bits[x]
    assert seen == 2 * L.ACCEPTED - 1        # every bit of the word is shown by some case
    assert {L.case(x)["n"] for x in L.CASE_NAMES} >= {1025, 2047, 2048, 2049, 16383, 16385}
    # the numpy and the position forms of the matrix are one matrix
    for x in ("dummies_scattered_rows", "dummies_scattered_cols", "reach_n1025_last_col", "unbal_m3_k3"):
        c = L.case(x)
        M, m = L.numpy_matrix(c), L.Model(c)
        for i in (0, 1, 7 % c["n"], c["n"] - 1):
            assert (M[i] == m.row(i)).all() and (M[:, i] == m.col(i)).all()
