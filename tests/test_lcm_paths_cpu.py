"""CPU tier of the td_lcm / td_pool2 path table (tests/lcm_path_cases.py): every case's claims hold by the references alone, the
`lcm_path` bits a case expects follow from its measured shape and the named constants, and the references agree with each
other where more than one can answer.  What the kernels make of the cases: test_gpu_lcm_paths.py."""
import numpy as np
import pytest

import lcm_path_cases as L
from oracle import oracle
from sim_backend import OracleBackend


def _level_lists(c):
    """the level-list model of an LCM case with a matrix: for every candidate value, its cells in row-major order"""
    m = L.dense_matrix(c)
    hi = L.candidate_hi(c["rule"][0])
    return {int(v): list(zip(*map(np.ndarray.tolist, np.nonzero(m == v)))) for v in np.unique(m[m <= hi])}, m


def _pick_positions(c, ref):
    """(value, position in that value's list) of every pick of the reference"""
    lists, m = _level_lists(c)
    index = {v: {rc: k for k, rc in enumerate(cells)} for v, cells in lists.items()}
    return [(int(m[r, cc]), index[int(m[r, cc])][(r, cc)]) for r, cc in zip(ref[1], ref[2])], lists


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_bits_follow_from_shape_and_constants(name):
    c = L.case(name)
    count, vmin, vmax = L.candidates(c)
    assert c["bits"] == L.expected_bits(c["kind"], c["n"], count, vmin, vmax, c["out"] == "host"), (name, count, vmin, vmax)
    if c["kind"] == "lcm" and c["input"] == "sparse":
        assert count <= 300000            # the Python walk of the reference stays in seconds
        r, cc, _ = c["coords"]
        key = r.astype(np.int64) * c["n"] + cc
        assert (np.diff(key) > 0).all()   # unique, row-major: the device build is deterministic
    if c["kind"] == "lcm" and c["input"] != "count" and c["n"] > L.DENSE_MAX:
        assert c["input"] == "sparse"     # nothing on this tier allocates a matrix that large


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_claims_hold_by_the_reference(name):
    c = L.case(name)
    ref = L.reference(name)
    n = c["n"]
    count, vmin, vmax = L.candidates(c)
    for claim in c["claims"]:
        what = claim[0]
        if what == "quarters":
            q = L.rows4_quarter(n)
            owned = [max(0, min(n, (w + 1) * q) - w * q) for w in range(4)]
            assert owned == {64: [64, 0, 0, 0], 65: [64, 1, 0, 0], 256: [64, 64, 64, 64], 257: [128, 128, 1, 0]}[n]
            assert set(ref[2]) >= {0, n - 1}                       # picks in the first and the last column
        elif what == "rescan":
            _, row, delta = claim
            m = c["matrix"].astype(np.int64)
            base = int(m.min())
            first_col = int(np.argmin(m[row]))
            k = ref[1].index(row) if row in ref[1] else len(ref[1])
            earlier = [(r, cc) for r, cc in zip(ref[1][:k], ref[2][:k])]
            assert any(cc == first_col and r != row for r, cc in earlier)       # its first minimum's column went to another row
            assert (ref[1][0], ref[2][0]) == (0, first_col) and m[0, first_col] == base
            free = np.ones(n, bool)
            free[first_col] = False
            assert int(m[row][free].min()) - base == delta                      # what the re-scan must find
            assert int(np.flatnonzero(free & (m[row] == base + delta))[0]) == n - 1   # in the last column (the padded chunk)
            assert (m[row][free][:-1] > base + L.NARROW_TOP).all()              # behind cells a saturated code would equal
        elif what == "all255":
            m = c["matrix"].astype(np.int64)
            base, row = int(m.min()), claim[1]
            free = np.ones(n, bool)
            free[int(np.argmin(m[row]))] = False
            assert (m[row][free] >= base + L.NARROW_TOP).all() and int(np.argmin(m[row])) == ref[2][0]
        elif what == "takes":
            assert (claim[1], claim[2]) in list(zip(ref[1], ref[2]))
        elif what == "takes_row":
            assert claim[1] in ref[1]
        elif what == "span":
            assert (vmax - vmin, vmin) == (claim[1], claim[2])
        elif what == "path":
            assert bool(c["bits"] & L.LISTS) == (claim[1] == "lists")
        elif what == "cap":
            _, mp, natural = claim
            assert natural >= 2 and mp in (0, 1, natural - 1) and len(ref[1]) == mp
        elif what == "scan":
            assert (vmax - vmin + 1) * n == claim[1]
        elif what == "picked":
            _, r, cc, v = claim
            assert (r, cc) in list(zip(ref[1], ref[2])) and L.dense_matrix(c)[r, cc] == v == vmax
        elif what in ("pos", "dead"):
            picks, lists = _pick_positions(c, ref)
            if what == "pos":
                assert (claim[1], claim[2]) in picks, (name, claim)
            else:   # no cell of the block is live when the walk reaches it: its row or column went to an earlier pick
                _, val, lo, hi = claim
                before = [k for k, (v, p) in enumerate(picks) if (v, p) < (val, lo)]
                rows, cols = {ref[1][k] for k in before}, {ref[2][k] for k in before}
                assert len(lists[val]) > hi
                assert all(r in rows or cc in cols for r, cc in lists[val][lo:hi])
                assert not any(v == val and lo <= p < hi for v, p in picks)
        elif what == "edge_columns":
            r, cc, v = c["coords"]
            cand = set(cc[v <= L.candidate_hi(c["rule"][0])].tolist())
            assert set(L.edge_columns(n)) <= cand and n - 1 in ref[2]
            if n <= L.ROWS4_NMAX:
                q = L.rows4_quarter(n)
                assert q == 1024 and (n - 3 * q) % 64 == {4093: 61, 4096: 0}[n]   # the last wave: a partial chunk / full chunks
        elif what == "lds":
            if claim[1] == "greedy":   # 4097 is the first n whose walk needs more LDS than the default
                assert (L.greedy_lds(n) > L.LDS_DEFAULT) == (n > L.ROWS4_NMAX)
                assert L.greedy_lds(4096) <= L.LDS_DEFAULT < L.greedy_lds(4097)
            else:
                assert (L.loop_lds(n) > L.LDS_DEFAULT) == (n >= 6050) and (L.loop_lds(n) > L.LDS_ROWKEYS) == (n >= 12099)
        elif what == "hash":
            named = claim[1]
            r, cc, v = c["coords"]
            level0 = list(zip(r[v == 0].tolist(), cc[v == 0].tolist()))
            assert level0 == list(named) and len(level0) <= L.CHUNK     # one level list, inside one chunk
            taken = [rc for rc in L.HASH_TAKEN if max(rc) < n]
            assert list(zip(ref[1], ref[2]))[:len(taken)] == taken
            if n > L.HASH_SIZE:   # rows 0 / 16384 and columns 0 / 16384 share a slot without a true conflict; column HASH_A is one
                m = L.HASH_SIZE - 1
                (r0, c0), (r1, c1), (r2, c2), (r3, c3), (r4, c4) = named
                assert r0 != r3 and r0 & m == r3 & m and c0 != c3
                assert c1 != c2 and c1 & m == c2 & m and r1 != r2
                assert c4 == c0 and r4 == r3 and (r4, c4) not in zip(ref[1], ref[2])
            else:
                assert len(named) == 2
        elif what == "count":
            assert count == claim[1] == n * n and (count <= L.COUNT_MAX) == (n <= 16384)
            assert L.loop_lds(n) > L.LDS_ROWKEYS
        elif what == "pool_span":
            assert vmax - vmin == claim[1]
        elif what == "pool_span_at_least":
            assert vmax - vmin >= claim[1] and vmax > 10**6
        else:
            raise AssertionError("unknown claim %r" % (claim,))
    if c["kind"] == "pool2":
        assert len(ref) == n // 2 and len({x for a, b, _, _ in ref for x in (a, b)}) == 2 * (n // 2)
    elif c["out"] == "host":
        assert (L.PINNED_OFF + 8 * n <= L.PINNED_CAP) == bool(c["bits"] & L.PINNED)


def test_both_sides_of_every_edge_are_in_the_table():
    for edge, names in L.EDGES.items():
        assert len(names) >= 2 and set(names) <= set(L.CASE_NAMES), edge
    for edge in L.PATH_DECIDING:
        a, b = L.EDGES[edge][:2]
        assert L.case(a)["bits"] != L.case(b)["bits"], edge
    n_of = lambda m: L.case(m)["n"]
    assert {n_of(m) for m in L.LCM_NAMES} >= {63, 64, 65, 127, 128, 129, 143, 144, 145, 256, 257, 4093, 4096, 4097, 6049, 6050,
                                              7168, 7169, 12098, 12099, 16384, 16385}
    assert {n_of(m) for m in L.POOL_NAMES} >= {63, 64, 65, 127, 128, 129, 145, 4097}
    assert any(n_of(m) % 2 for m in L.POOL_NAMES)
    for path in ("lists", "loop"):   # per path: every rule, a cap of 0, of 1 and one below the natural count, device outputs
        mine = [L.case(m) for m in L.LCM_NAMES if ("path", path) in L.case(m)["claims"]]
        rules = [c["rule"][0] for c in mine]
        assert any(r["mask"] == 100 for r in rules) and any(r.get("stop_value_on") for r in rules) and any(r.get("threshold", -1) >= 0 for r in rules)
        caps = [cl for c in mine for cl in c["claims"] if cl[0] == "cap"]
        assert {cl[1] for cl in caps} >= {0, 1} and any(cl[1] == cl[2] - 1 and cl[1] > 1 for cl in caps)
        assert any(c["out"] == "device" for c in mine) and any(c["out"] == "host" for c in mine)


def _oracle_reachable(name):
    """the cases on which sparse_greedy can be held against the oracle: n within the oracle's reach, and a model that
    sparse_greedy's contract covers (no cell between the candidates and the mask; under the heuristic rule every cell a candidate)"""
    c = L.case(name)
    if c["input"] == "count" or c["n"] > 1300:
        return False
    kw_gpu = c["rule"][0]
    m = L.dense_matrix(c)
    rest = m[m > L.candidate_hi(kw_gpu)]
    if rest.size and int(rest.min()) < kw_gpu["mask"]:
        return False
    return bool(kw_gpu.get("stop_value_on") or kw_gpu.get("threshold", -1) >= 0 or not rest.size)


@pytest.mark.parametrize("name", [m for m in L.LCM_NAMES if _oracle_reachable(m)])
def test_sparse_greedy_agrees_with_the_oracle(name):
    """sparse_greedy (the reference of the large sparse cases) on every case the oracle can reach, under that case's own rule"""
    c = L.case(name)
    kw_gpu, kw_oracle = c["rule"]
    m = L.dense_matrix(c)
    hi = L.candidate_hi(kw_gpu)
    r, cc = np.nonzero(m <= hi)
    rest = m[m > hi]
    fill = int(rest.min()) if rest.size else max(L.BIG, kw_gpu["mask"])
    got = L.sparse_greedy(c["n"], r, cc, m[r, cc], kw_gpu, fill)
    t, ro, co, lm = oracle.lcm(m, **kw_oracle)
    assert (got[0], got[1].tolist(), got[2].tolist(), got[3]) == (t, ro.tolist(), co.tolist(), lm), name
    assert (t, ro.tolist(), co.tolist(), lm) == L.reference(name)


def test_sparse_greedy_is_checked_on_every_rule_and_ending():
    names = [m for m in L.LCM_NAMES if _oracle_reachable(m)]
    assert len(names) >= 30
    rules = [L.case(m)["rule"][0] for m in names]
    assert any(r["mask"] == 100 for r in rules) and any(r.get("stop_value_on") for r in rules) and any(r.get("threshold", -1) >= 0 for r in rules)
    ends = {(len(L.reference(m)[1]) > 0, L.reference(m)[3] in (L.BIG, 100)) for m in names}
    assert ends >= {(True, True), (True, False)}   # ran out of candidates / stopped on a pick


def test_count_closed_form_agrees_with_the_oracle():
    kw_gpu, kw_oracle = L.rule("heuristic")
    for n in (16, 40, 61):
        m = L.count_matrix(n)
        miss_r, miss_c, zr, zc = L.count_model(n)
        assert (m == 0).sum() == n - L.COUNT_M and not (m[miss_r] == 0).any() and not (m[:, miss_c] == 0).any()
        assert sorted(zc.tolist() + miss_c.tolist()) == list(range(n)) and (np.diff(zr) > 0).all()
        i, j = np.nonzero(m)
        assert (m[i, j] == L.count_cell(i, j)).all()
        t, r, c, lm = oracle.lcm(m, **kw_oracle)
        e = L.count_expected(n, kw_oracle)
        assert (t, r.tolist(), c.tolist(), lm) == (e[0], e[1].tolist(), e[2].tolist(), e[3])
    for n in (16384, 16385):   # the large cases: from the description alone
        miss_r, miss_c, zr, zc = L.count_model(n)
        assert len(set(zc.tolist())) == zr.size == n - L.COUNT_M and not set(zc.tolist()) & set(miss_c.tolist())
        ref = L.reference("count_n%d" % n)
        assert len(ref[1]) == n and sorted(ref[1]) == sorted(ref[2]) == list(range(n)) and ref[0] == ref[3] + sum(
            int(L.count_cell(r, c)) for r, c in zip(ref[1][-3:-1], ref[2][-3:-1]))


def test_pool2_reference_agrees_with_the_simulator_restatement():
    for name in ("pool_line_n63", "pool_line_n64", "pool_line_n65", "pool_span255", "pool_span256"):
        c = L.case(name)
        assert L.reference(name) == OracleBackend().find_pool(c["frm"], c["to"]), name
    for name in ("pool_line_n65", "pool_span255", "pool_table_n127"):   # both walks of the reference give one order
        c = L.case(name)
        assert L.pool2_reference(c["frm"], c["to"], c["dist"], by_level=True) == L.reference(name), name
    c = L.case("pool_line_n4097")
    cost = L.case_pool_costs("pool_line_n4097")[0]
    ref = L.reference("pool_line_n4097")
    assert len(ref) == 4097 // 2 and [x[3] for x in ref] == sorted(x[3] for x in ref)
    assert all(cost[a, b] == k for a, b, _, k in ref)


def test_reference_is_shared_and_read_only():
    assert L.reference("edge_n64") is L.reference("edge_n64") and L.case("edge_n64") is L.case("edge_n64")
    with pytest.raises(ValueError):
        L.case("edge_n64")["matrix"][0, 0] = 1
    with pytest.raises(ValueError):
        L.case("scan_8193")["coords"][2][0] = 1
