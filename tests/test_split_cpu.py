"""CPU tier of td_split_batched: the host restatement of split.py:61-119 (tests/split_model.py) against brute force, the
checker's own teeth, the symbol in the ctypes table and the built library, and no CPU fallback."""
import numpy as np
import pytest

import __graft_entry__ as entry
import split_model as M


@pytest.fixture(scope="module")
def built():
    entry.build()
    from taxidispatcher_amd import _ffi
    return _ffi


def _cases(rng, size, count, kmax=6):
    for _ in range(count):
        ns, nd = (int(x) for x in rng.integers(0, kmax + 1, 2))
        yield rng.integers(0, size, ns).tolist(), rng.integers(0, size, nd).tolist()


def test_ranges_follow_the_reference_loop():
    assert M.ranges(20, 4) == [(0, 5), (5, 10), (10, 15), (15, 20)]
    assert M.ranges(22, 4) == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 25)]   # five ranges, stand 21 in the fifth
    assert M.ranges(4, 4) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert M.ranges(7, 1) == [(0, 7)]
    assert len(M.ranges(63, 32)) == 63   # the most ranges parts <= 32 can give


@pytest.mark.parametrize("size,parts", [(22, 4), (4, 4), (9, 1), (20, 4)])
def test_restatement_against_brute_force(size, parts):
    rng = np.random.default_rng(1000 * size + parts)
    sym = rng.integers(0, 30, (size, size))
    sym = sym + sym.T
    asym = rng.integers(0, 50, (size, size))
    for dist in (None, sym, asym):
        for cab, dem in _cases(rng, size, 25):
            out = M.solve_split_host(cab, dem, size, parts, dist, M.FILL)
            M.check_case(cab, dem, size, parts, dist, M.FILL, out, opt=M.opt_brute)
            M.check_case(cab, dem, size, parts, dist, M.FILL, out, opt=M.opt_oracle)


def test_restatement_fifth_range():
    """size 22 in 4 parts: stands 20 and 21 make the fifth range, so a cab and a request there meet in stage 0"""
    out = M.solve_split_host([21, 3], [20, 16], 22, 4)
    assert out["cab_req"] == [0, 1] and out["cab_stage"] == [0, 1] and out["total"] == 1 + 13 and out["n_rest"] == (1, 1)
    M.check_case([21, 3], [20, 16], 22, 4, None, M.FILL, out, opt=M.opt_brute)
    out = M.solve_split_host([], [1], 22, 4)
    assert out["total"] == 0 and out["n_rest"] == (0, 0)


def test_one_part_is_the_unsplit_optimum():
    rng = np.random.default_rng(5)
    for cab, dem in _cases(rng, 12, 20):
        out = M.solve_split_host(cab, dem, 12, 1)
        assert out["total"] == M.opt_brute(cab, dem, None, M.FILL)
        assert out["rest_total"] == 0


def test_checker_rejects_wrong_outputs():
    cab, dem = [1, 2, 8, 9, 14], [0, 3, 7, 16, 17, 18]
    good = M.solve_split_host(cab, dem, 20, 4)
    M.check_case(cab, dem, 20, 4, None, M.FILL, good)

    def broken(**kw):
        out = {k: (list(v) if isinstance(v, list) else v) for k, v in good.items()}
        out.update(kw)
        with pytest.raises(AssertionError):
            M.check_case(cab, dem, 20, 4, None, M.FILL, out)

    broken(total=good["total"] + 1)
    broken(rest_total=good["rest_total"] - 1)
    broken(dual_gap=1)
    broken(n_rest=(good["n_rest"][0] + 1, good["n_rest"][1]))
    req, stage = list(good["cab_req"]), list(good["cab_stage"])
    i = stage.index(0)
    broken(cab_req=req[:i] + [-1] + req[i + 1:], cab_stage=stage[:i] + [-1] + stage[i + 1:])   # a region's smaller side not matched
    broken(cab_stage=[1 if s == 0 else s for s in stage])                                       # region pairs claimed by the fifth solve
    j = next(k for k in range(len(req)) if k != i and req[k] != -1)
    broken(cab_req=req[:j] + [req[i]] + req[j + 1:])                                            # a request served twice


def test_symbol_declared(built):
    lib = built.load()
    assert "td_split_batched" in built.SIGNATURES
    assert getattr(lib, "td_split_batched") is not None
    assert lib.td_version() == 101
    import taxidispatcher_amd as td
    for name in ("split_batched", "solve_split", "split_gap"):
        assert name in td.__all__ and callable(getattr(td, name))


def test_solve_split_empty_side_is_none():
    import taxidispatcher_amd as td
    assert td.solve_split(None, [], [(0, 1, 2)], 10) is None
    assert td.solve_split(None, [(0, 1, 2)], [], 10) is None


def test_no_cpu_fallback(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the failure path is exercised on the CPU tier only")
    lib = built.load()
    import taxidispatcher_amd as td
    with pytest.raises(td.TdError):
        td.split_batched([np.array([1, 2, 3])], [np.array([2, 2])], 10)
    off = np.array([0, 3], np.int32)
    v = np.array([1, 2, 3], np.int32)
    r = np.zeros(3, np.int32)
    t = np.zeros(1, np.int64)
    assert lib.td_split_batched(1, 3, off.ctypes.data, v.ctypes.data, off.ctypes.data, v.ctypes.data, None, 0, 10, 4, 100,
                                r.ctypes.data, None, t.ctypes.data, None, None, None) == -3
