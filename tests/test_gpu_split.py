"""td_split_batched / split_batched / solve_split / split_gap on the GPU.  Every result goes through the checker of
tests/split_model.py (exact: a region's sum, the derived rest lists, the fifth solve's sum, the total, dual_gap == 0)."""
import numpy as np
import pytest

import split_model as M

pytestmark = pytest.mark.gpu

FILL = M.FILL
PATTERN32, PATTERN64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _random_cases(rng, size, count, kmax, kmin=0):
    cabs, dems = [], []
    for _ in range(count):
        ns, nd = (int(x) for x in rng.integers(kmin, kmax + 1, 2))
        cabs.append(rng.integers(0, size, ns).astype(np.int32))
        dems.append(rng.integers(0, size, nd).astype(np.int32))
    return cabs, dems


def _run_checked(td, cabs, dems, size, parts, dist=None, fill=FILL):
    res = td.split_batched(cabs, dems, size, parts, dist, fill)
    M.check_batch(cabs, dems, size, parts, dist, fill, res)
    return res


def test_region_shapes_in_one_batch(td):
    size, parts = 20, 4   # ranges of 5 stands
    cabs = [[1, 2, 3, 6, 10, 14],          # r0: 3 cabs / 1 request, r1: 1 / 3, r2: 2 / 2, r3: empty
            [],                            # no cabs
            [0, 4, 17, 15],                # r0: cabs only, r1: requests only, r2: empty, r3: equal
            [],                            # neither
            [15, 16, 17],                  # everything in one range
            [3, 8],                        # no requests
            [19, 0]]                       # the two ends
    dems = [[4, 5, 7, 9, 11, 13],
            [1, 2],
            [5, 9, 16, 19],
            [],
            [19, 18, 15, 16],
            [],
            [0, 19]]
    res = _run_checked(td, cabs, dems, size, parts)
    assert res["n_rest"].tolist() == [[2, 2], [0, 0], [2, 2], [0, 0], [0, 1], [0, 0], [0, 0]]
    assert res["total"].tolist()[1] == 0 and res["total"].tolist()[3] == 0 and res["total"].tolist()[5] == 0
    assert res["cab_stage"][res["cab_off"][2]:res["cab_off"][3]].tolist() == [1, 1, 0, 0]
    assert res["cab_req"][res["cab_off"][5]:res["cab_off"][6]].tolist() == [-1, -1]
    assert res["cab_req"][res["cab_off"][6]:].tolist() == [1, 0] and res["total"][6] == 0


@pytest.mark.parametrize("size,parts", [(20, 4), (22, 4), (4, 4), (20, 1), (64, 32), (63, 32)])
def test_range_rule(td, size, parts):
    rng = np.random.default_rng(100 * size + parts)
    cabs, dems = _random_cases(rng, size, 40, 12)
    cabs[0] = np.array([size - 1, 0, size - 1], np.int32)   # the last stand: in the short extra range when there is one
    dems[0] = np.array([size - 1, size - 1], np.int32)
    _run_checked(td, cabs, dems, size, parts)


@pytest.mark.parametrize("n", [64, 65, 128, 129, 256, 257, 512, 513])
def test_solver_template_edges(td, n):
    rng = np.random.default_rng(n)
    size = 4000
    cabs = [rng.integers(0, size, n).astype(np.int32), rng.integers(0, size, n - 3).astype(np.int32), rng.integers(0, size, 5).astype(np.int32)]
    dems = [rng.integers(0, size, n).astype(np.int32), rng.integers(0, size, n).astype(np.int32), rng.integers(0, size, n).astype(np.int32)]
    _run_checked(td, cabs, dems, size, 4)


def test_size_limit(td):
    rng = np.random.default_rng(1024)
    size = 4000
    cabs = [rng.integers(0, size // 2, 1024).astype(np.int32)]      # ranges 0 and 1 hold cabs only,
    dems = [rng.integers(size // 2, size, 1024).astype(np.int32)]   # ranges 2 and 3 requests only: the fifth model is the case
    res = _run_checked(td, cabs, dems, size, 4)
    assert res["n_rest"].tolist() == [[1024, 1024]] and (res["cab_stage"] == 1).all()
    assert res["total"][0] == res["rest_total"][0] == int(dems[0].sum()) - int(cabs[0].sum())
    with pytest.raises(td.TdError, match="1024"):
        td.split_batched([np.zeros(1025, np.int32)], [np.zeros(3, np.int32)], size, 4)
    rc, outs = _raw(td, [np.zeros(3, np.int32)], [np.zeros(1025, np.int32)], None, 0, size, 4, FILL, False)
    assert rc == -1 and _untouched(outs)


@pytest.mark.parametrize("S", [20, 300])   # 1.6 KB: staged in LDS beside the model arrays; 360 KB: read through L2
@pytest.mark.parametrize("kind", ["line", "symmetric", "asymmetric"])
def test_distance_source(td, S, kind):
    rng = np.random.default_rng(S + len(kind))
    if kind == "line":
        dist = None
    else:
        dist = rng.integers(0, 200, (S, S)).astype(np.int32)
        if kind == "symmetric":
            dist = (dist + dist.T).astype(np.int32)
        else:
            dist[np.arange(S), np.arange(S)] = 0
    cabs, dems = _random_cases(rng, S, 30, 16)
    res = _run_checked(td, cabs, dems, S, 4, dist)
    if kind == "asymmetric":   # the row is the cab's stand: the transposed table does not verify
        with pytest.raises(AssertionError):
            M.check_batch(cabs, dems, S, 4, dist.T, FILL, res)


def test_input_forms_and_determinism(td):
    import torch
    rng = np.random.default_rng(7)
    cabs, dems = _random_cases(rng, 40, 60, 20)
    dist = rng.integers(0, 90, (40, 40)).astype(np.int32)
    a = _run_checked(td, cabs, dems, 40, 4, dist)
    b = td.split_batched(cabs, dems, 40, 4, dist)
    cv, co, dv, do, _, _ = td.pack_ragged(cabs, dems)
    dev = [torch.from_numpy(x).cuda() for x in (cv, co, dv, do)]
    c = td.split_batched((dev[0], dev[1]), (dev[2], dev[3]), 40, 4, torch.from_numpy(dist).cuda())
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k


def test_grid_stride(td):
    rng = np.random.default_rng(3000)
    cabs, dems = _random_cases(rng, 20, 3000, 8)
    _run_checked(td, cabs, dems, 20, 4)


def _raw(td, cabs, dems, dist, S, size, parts, fill, device_outputs):
    """the C call with pre-filled outputs -> (rc, outputs as numpy)"""
    import torch
    lib = td._ffi.lib()
    cv, co, dv, do, batch, n = td.pack_ragged(cabs, dems)
    nc = int(co[-1])
    shapes = [((max(nc, 1),), np.int32), ((max(nc, 1),), np.int32), ((batch,), np.int64), ((batch,), np.int64), ((2 * batch,), np.int32),
              ((batch,), np.int64)]
    outs = [np.full(s, PATTERN32 if t == np.int32 else PATTERN64, t) for s, t in shapes]
    if device_outputs:
        outs = [torch.from_numpy(o).cuda() for o in outs]
    d = None if dist is None else np.ascontiguousarray(dist, np.int32)
    rc = lib.td_split_batched(batch, n, td._ffi.addr(co), td._ffi.addr(cv), td._ffi.addr(do), td._ffi.addr(dv),
                              None if d is None else d.ctypes.data, S, size, parts, fill, *[td._ffi.addr(o) for o in outs])
    return rc, [o.cpu().numpy() if device_outputs else o for o in outs]


def _untouched(outs):
    return all((o == (PATTERN32 if o.dtype == np.int32 else PATTERN64)).all() for o in outs)


@pytest.mark.parametrize("device_outputs", [False, True])
def test_refusals_leave_outputs_unwritten(td, device_outputs):
    rng = np.random.default_rng(11)
    cabs, dems = _random_cases(rng, 20, 12, 9, kmin=2)
    table = rng.integers(0, 100, (20, 20)).astype(np.int32)
    rc, outs = _raw(td, cabs, dems, None, 0, 20, 4, FILL, device_outputs)
    assert rc == 0 and not _untouched(outs)
    res = {"cab_req": outs[0], "cab_stage": outs[1], "total": outs[2], "rest_total": outs[3], "n_rest": outs[4].reshape(-1, 2),
           "dual_gap": outs[5], "cab_off": np.concatenate([[0], np.cumsum([len(c) for c in cabs])])}
    M.check_batch(cabs, dems, 20, 4, None, FILL, res)

    def refused(cabs, dems, dist, S, size, parts, fill):
        rc, outs = _raw(td, cabs, dems, dist, S, size, parts, fill, device_outputs)
        assert rc == -1, rc
        assert _untouched(outs)

    at_size = [c.copy() for c in cabs]
    at_size[5][1] = 20
    refused(at_size, dems, None, 0, 20, 4, FILL)            # a position at size
    negative = [d.copy() for d in dems]
    negative[7][0] = -1
    refused(cabs, negative, None, 0, 20, 4, FILL)           # a negative position
    refused(cabs, negative, table, 20, 20, 4, FILL)
    same_range = [np.array([6, 7], np.int32)], [np.array([8], np.int32)]
    used2 = table.copy()
    used2[7, 8] = FILL
    refused(same_range[0], same_range[1], used2, 20, 20, 4, FILL)   # a region model's cell equal to fill
    cross = [np.array([1], np.int32)], [np.array([18], np.int32)]
    used3 = table.copy()
    used3[1, 18] = FILL
    refused(cross[0], cross[1], used3, 20, 20, 4, FILL)     # a fifth model's cell equal to fill
    refused(cabs, dems, None, 0, 3, 4, FILL)                # size < parts
    refused(cabs, dems, table[:19, :19], 19, 20, 4, FILL)   # S < size
    refused(cabs, dems, None, 0, 20, 0, FILL)               # parts < 1
    refused(cabs, dems, None, 0, 20, 33, FILL)              # parts > 32
    refused(cabs, dems, None, 0, 20, 4, 19)                 # the line's longest distance is not below fill
    # an entry equal to fill that no model uses is no reason to refuse
    unused = table.copy()
    unused[18, 1] = FILL
    rc, outs = _raw(td, cross[0], cross[1], unused, 20, 20, 4, FILL, device_outputs)
    assert rc == 0 and outs[2][0] == table[1, 18]


def test_gap_ordering(td):
    opt, split, lcm, gap_split, gap_lcm = td.split_gap(20, 10, 200, seed=1)
    assert opt.shape == split.shape == lcm.shape == (200,)
    assert (opt <= split).all() and (opt <= lcm).all()
    assert gap_split >= 0 and gap_lcm >= 0


def test_single_case_shape(td):
    """procedure.py:32-51's example: 3 cabs, 4 customers on 10 stands"""
    n_stands = 10
    dist = np.abs(np.arange(n_stands)[:, None] - np.arange(n_stands)[None, :]).astype(np.int32)
    demand = [(0, 0, 2), (1, 0, 5), (2, 3, 1), (3, 5, 1)]
    cabs = [(0, 3, 3), (1, 3, 1), (2, 0, 5)]
    got = td.solve_split(dist, demand, cabs, n_stands)
    cab_to, dem_from = [c[2] for c in cabs], [d[1] for d in demand]
    res = _run_checked(td, [cab_to], [dem_from], n_stands, 4, dist)
    assert got == int(res["total"][0]) == M.solve_split_host(cab_to, dem_from, n_stands, 4, dist)["total"] == 1
    assert td.solve_split(None, demand, cabs, n_stands) == 1
