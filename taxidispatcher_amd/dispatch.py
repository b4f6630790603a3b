"""Host-side mirror of the reference's Python interface for the assignment hot path.

Same function names, argument meaning and return shapes as the reference scripts, so a user
of `procedure.py` / `greedy_opt.py` / `simulate.py` / `solver.py` can switch the import and keep
the calling code.  Every function runs on the MI355X through the C ABI (`_ffi`); nothing here
computes an assignment, a cost matrix or an LCM on the CPU.

Reference map (file:line in boguszjelinski/taxidispatcher):
    calculate_cost        greedy_opt.py:86-99, simulate.py:17-33 (drop_time), Simulator.java:493-520
    calculate_cost_by_id  procedure.py:6-12
    solve                 greedy_opt.py:102-118 / simulate.py:36-53  -> (n, x, cost)
    procedure_solve       procedure.py:5-29                           -> x
    build_assign          the same API #1 without handing the matrix back (td_build_assign)
    solve_cost            solver.py:11-27                             -> x
    LCM                   greedy_opt.py:61-82 / simulate.py:76-98
    LCM_heuristic         heuristic.py:24-33
    LCM_simulator         Simulator.java:523-549
    count_sum             greedy_opt.py:21-29
    filter_out            greedy_opt.py:32-37 (by id) / simulate.py:64-69 (by position)
    combined              greedy_opt.py:136-160
    assign_batched        the optimum of many small models per call (heuristic.py:20-40, split.py:61-120)
    LCM_batched           LCM of many small models per call (heuristic.py:24-33 per scenario)
    heuristic_gap         heuristic.py:20-40 as two calls
    build_assign_batched  build_assign of many ragged position models per call (split.py's regions, zones of one tick)
    tick_batched          tick() of many ragged position models per call (Simulator.java:163-208 per zone / per seed)
    match_batched         maximum-weight matching of many general graphs per call (the optimum behind pool_opt_min.py)
    split_batched         split.py:61-119 as a whole, for many cases per call (td_split_batched)
    dispatch_batched      many models per call, a dispatch method per model: LCM + optimum, optimum, LCM, split (td_dispatch_batched)
    solve_split           split.py:61-119 for one case, the reference's call shape  -> total
    split_gap             split.py's main (optimum, split total, LCM) as library calls
    pool2_batched         greedy (pool_opt_min.py:81-102) or optimal (:114-122) pools of two of many ragged models per call
    find_pool_optimal     find_pool's format, optimal pools
    pool_gap              pool_opt_min.py as two calls
    find_pool_n_banded    pool_n.c (pools of 2..4) of one model in a bounded plan buffer, any number of happy plans
    pool_n_batched        pool_n.c (pools of 2..4) of many models of at most 512 requests per call
    find_pool_fanout      findpool.c as two calls: the 8 children as one batch, then the merge
"""
import ctypes

import numpy as np

from . import _ffi

BIG_COST = 250000  # greedy_opt.py:5, simulate.py:12, Simulator.java:115


# ----------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------
def _records(rows):
    """(id, from, to) iterables -> three int32 arrays."""
    rows = list(rows)
    if not rows:
        z = np.zeros(0, np.int32)
        return z, z, z
    a = _ffi.as_i32(rows).reshape(len(rows), -1)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1]), np.ascontiguousarray(a[:, 2])


def _require_i32(t, what):
    """device tensors go to the kernels as they are: they must be int32 (numpy inputs are converted)"""
    if hasattr(t, "data_ptr") and str(getattr(t, "dtype", "")) != "torch.int32":
        raise _ffi.TdError("%s: a torch tensor handed to the library must be int32, got %s" % (what, t.dtype))


def _dist_arg(distances):
    """distances: None (=> |a-b|), an S x S array-like, or a (device_ptr, S) tuple."""
    if distances is None:
        return None, 0, None
    if isinstance(distances, tuple):
        return distances[0], int(distances[1]), None
    if hasattr(distances, "data_ptr") and getattr(distances, "is_cuda", False):
        _require_i32(distances, "distances")
        if distances.dim() != 2 or distances.shape[0] != distances.shape[1]:
            raise _ffi.TdError("distances must be a square S x S table")
        return _ffi.addr(distances), int(distances.shape[0]), distances   # addr() fences torch's stream
    d = _ffi.as_i32(distances)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise _ffi.TdError("distances must be a square S x S table")
    return d.ctypes.data, int(d.shape[0]), d


def cost_build(cab_to, dem_from, distances=None, fill=BIG_COST, threshold=-1, cab_id=None, dem_id=None,
               by_id=False, out=None, sync=True):
    """Thin wrapper over td_cost_build. Returns (n, cost) with cost an int32 n x n numpy array,
    or writes into `out` (numpy array or torch CUDA tensor) and returns (n, out).
    sync=False: a device `out` is NOT waited for — only for callers whose next use of it is another call of this
    library (same stream, e.g. a tick loop: cost_build -> LCM -> assign)."""
    lib = _ffi.lib()
    cab_to = _ffi.as_i32(cab_to)
    dem_from = _ffi.as_i32(dem_from)
    n_s, n_d = int(cab_to.size), int(dem_from.size)
    n = max(n_s, n_d)
    cab_id = None if cab_id is None else _ffi.as_i32(cab_id)
    dem_id = None if dem_id is None else _ffi.as_i32(dem_id)
    dptr, S, keep = _dist_arg(distances)
    if out is None:
        out = np.empty((n, n), np.int32)
    if n:
        _ffi.check(lib.td_cost_build(_ffi.addr(cab_to), _ffi.addr(cab_id), n_s, _ffi.addr(dem_from),
                                     _ffi.addr(dem_id), n_d, dptr, S, int(fill), int(threshold), int(bool(by_id)),
                                     _ffi.addr(out)))
        if sync and getattr(out, "is_cuda", False):
            # device output: written asynchronously on the library's stream; torch works on its own
            _ffi.check(lib.td_synchronize())
    del keep
    return n, out


def assign(cost, n=None, want_dual=False):
    """Thin wrapper over td_assign. cost: n x n int32 (numpy or torch CUDA tensor).
    Returns (row_to_col int32[n], total[, dual_bound])."""
    lib = _ffi.lib()
    if isinstance(cost, np.ndarray) or not hasattr(cost, "data_ptr"):
        cost = _ffi.as_i32(cost)
    else:
        _require_i32(cost, "cost")
    if n is None:
        n = int(cost.shape[0])
    r2c = np.empty(n, np.int32)
    total = ctypes.c_int64(0)
    dual = ctypes.c_int64(0)
    _ffi.check(lib.td_assign(n, _ffi.addr(cost), _ffi.addr(r2c), ctypes.byref(total),
                             ctypes.byref(dual) if want_dual else None))
    if want_dual:
        return r2c, int(total.value), int(dual.value)
    return r2c, int(total.value)


def set_line_metric(on):
    """Switch td_assign's line-metric attempt (sorted matching + certificate pass, td_line.hip) on or off;
    returns the previous setting. On by default."""
    return bool(_ffi.lib().td_set_line_metric(1 if on else 0))


def build_assign(cab_to, dem_from, distances=None, fill=BIG_COST, threshold=-1, want_dual=False):
    """td_build_assign: cost build + optimal assignment in one call (the reference's solve(distances, demand, cabs),
    procedure.py:5-29 / greedy_opt.py:102-118 / simulate.py:36-53, without handing the matrix back).  A model padded
    with dummy requests never exists as an int32 matrix on the device.  Returns (n, row_to_col int32[n], total[, dual])."""
    lib = _ffi.lib()
    cab = cab_to if hasattr(cab_to, "data_ptr") else _ffi.as_i32(cab_to)
    dem = dem_from if hasattr(dem_from, "data_ptr") else _ffi.as_i32(dem_from)
    n_s, n_d = int(cab.shape[0]), int(dem.shape[0])
    n = max(n_s, n_d)
    dptr, S, keep = _dist_arg(distances)
    r2c = np.empty(n, np.int32)
    total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
    _ffi.check(lib.td_build_assign(_ffi.addr(cab) if n_s else None, n_s, _ffi.addr(dem) if n_d else None, n_d, dptr, S, int(fill),
                                   int(threshold), _ffi.addr(r2c) if n else None, ctypes.byref(total),
                                   ctypes.byref(dual) if want_dual else None))
    del keep
    if want_dual:
        return n, r2c, int(total.value), int(dual.value)
    return n, r2c, int(total.value)


class Solver:
    """A handle-scoped solver (td_solver_*): its own grow-only workspace on the GPU, same calls and answers as assign() /
    build_assign().  Several can live in one process, each keeping the workspace of its own models; calls stay synchronous and
    one at a time per process, whichever handle they go to (the stream, the pinned read-back block and last_stats() belong to
    the library context, not to the handle)."""

    def __init__(self):
        self.lib = _ffi.lib()
        h = ctypes.c_void_p()
        _ffi.check(self.lib.td_solver_create(ctypes.byref(h)))
        self.h = h

    def assign(self, cost, n=None, want_dual=False):
        if isinstance(cost, np.ndarray) or not hasattr(cost, "data_ptr"):
            cost = _ffi.as_i32(cost)
        else:
            _require_i32(cost, "cost")
        if n is None:
            n = int(cost.shape[0])
        r2c = np.empty(n, np.int32)
        total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
        _ffi.check(self.lib.td_solver_assign(self.h, n, _ffi.addr(cost), _ffi.addr(r2c), ctypes.byref(total),
                                             ctypes.byref(dual) if want_dual else None))
        return (r2c, int(total.value), int(dual.value)) if want_dual else (r2c, int(total.value))

    def build_assign(self, cab_to, dem_from, distances=None, fill=BIG_COST, threshold=-1, want_dual=False):
        cab = cab_to if hasattr(cab_to, "data_ptr") else _ffi.as_i32(cab_to)
        dem = dem_from if hasattr(dem_from, "data_ptr") else _ffi.as_i32(dem_from)
        n_s, n_d = int(cab.shape[0]), int(dem.shape[0])
        n = max(n_s, n_d)
        dptr, S, keep = _dist_arg(distances)
        r2c = np.empty(n, np.int32)
        total, dual = ctypes.c_int64(0), ctypes.c_int64(0)
        _ffi.check(self.lib.td_solver_build_assign(self.h, _ffi.addr(cab) if n_s else None, n_s, _ffi.addr(dem) if n_d else None, n_d, dptr, S,
                                                   int(fill), int(threshold), _ffi.addr(r2c) if n else None, ctypes.byref(total),
                                                   ctypes.byref(dual) if want_dual else None))
        del keep
        return (n, r2c, int(total.value), int(dual.value)) if want_dual else (n, r2c, int(total.value))

    def close(self):
        if self.h:
            self.lib.td_solver_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def expand_x(n, row_to_col):
    """row_to_col -> the reference's n*n 0/1 vector, index n*cab + cust (solver.py:36-39)."""
    x = np.zeros(n * n, np.uint8)
    if n:
        _ffi.check(_ffi.lib().td_expand_x(n, _ffi.addr(_ffi.as_i32(row_to_col)), _ffi.addr(x)))
    return x


def last_stats():
    out = (ctypes.c_int64 * 16)()
    _ffi.check(_ffi.lib().td_last_stats(out, 16))
    d = {"bid_rounds": out[0], "warm_rounds": out[1], "sap_free_rows": out[2], "sap_steps": out[3], "bytes_per_cell": out[4],
         "parallel_sap_rows": out[5], "narrow_price": out[6], "transposed": out[7], "line_metric": out[8], "line_dummies": out[9], "forest_levels": out[10],
         "lcm_path": out[11],    # td_lcm / td_pool2's word, defined right after such a call (the header lists its bits)
         "line_path": out[12]}   # what td_assign's line-metric attempt did, accepted or refused (the header lists its bits)
    return d


def finisher_path():
    """td_last_stats word 13: which finishers the last td_assign launched for the rows its bidding rounds left free, as a bit
    set (the TD_FP_* bits of the header).  Not a key of last_stats(): recorded comparisons of that dict stay valid."""
    out = (ctypes.c_int64 * 16)()
    _ffi.check(_ffi.lib().td_last_stats(out, 16))
    return int(out[13])


def match_path():
    """td_last_stats word 14: what the last match_batched / pool2_batched launched, as a bit set (the TD_MP_* bits of the
    header): 1 solver state in LDS, 2 in workspace slices, 4 a pool call, 8 the greedy launched, 16 k_pool_match launched,
    32 per-model policy arrays given; bits 8..23 the chunks launched (saturating).  Not a key of last_stats(): recorded
    comparisons of that dict stay valid."""
    out = (ctypes.c_int64 * 16)()
    _ffi.check(_ffi.lib().td_last_stats(out, 16))
    return int(out[14])


# ----------------------------------------------------------------------------------------
# reference-shaped API
# ----------------------------------------------------------------------------------------
def calculate_cost(distances, demand, cabs, big_cost=BIG_COST, drop_time=None):
    """greedy_opt.py:86-99. With drop_time (simulate.py:27: DROP_TIME=10) a cell is written only
    if distance < drop_time. n == 0 -> (0, 0) as simulate.py:21."""
    _, _, c_to = _records(cabs)
    _, d_frm, _ = _records(demand)
    if max(c_to.size, d_frm.size) == 0:
        return 0, 0
    return cost_build(c_to, d_frm, distances, fill=big_cost, threshold=-1 if drop_time is None else drop_time)


def calculate_cost_by_id(distances, demand, cabs):
    """procedure.py:6-12: fill n*n, cells addressed by the records' ids."""
    c_id, _, c_to = _records(cabs)
    d_id, d_frm, _ = _records(demand)
    n = max(c_to.size, d_frm.size)
    if n == 0:
        return 0, np.zeros((0, 0), np.int32)
    return cost_build(c_to, d_frm, distances, fill=n * n, threshold=-1, cab_id=c_id, dem_id=d_id, by_id=True)


def solve_cost(n, cost):
    """solver.py:11-27 solve(n, cost) -> x ; n == 0 -> (0, []) (solver.py:12)."""
    if n == 0:
        return 0, []
    r2c, _ = assign(cost, n)
    return expand_x(n, r2c)


def procedure_solve(distances, demand, cabs):
    """procedure.py:5-29 solve(distances, demand, cabs) -> x (length n*n, x[n*cab+cust] == 1)."""
    c_id, _, c_to = _records(cabs)
    d_id, d_frm, _ = _records(demand)
    n = max(c_to.size, d_frm.size)
    if n == 0:
        return np.zeros(0, np.uint8)
    ids_ok = (distances is not None and c_id.size and d_id.size and c_id.min() >= 0 and d_id.min() >= 0 and c_id.max() < n and d_id.max() < n
              and np.unique(c_id).size == c_id.size and np.unique(d_id).size == d_id.size)
    if not ids_ok:   # (ids outside 0..n-1 or repeated: the scatter of procedure.py:12 decides, build the matrix the same way)
        n, cost = calculate_cost_by_id(distances, demand, cabs)
        r2c, _ = assign(cost, n)
        return expand_x(n, r2c)
    # procedure.py:9-12 addresses the cells by the records' ids: the same matrix as the positional rule over arrays ORDERED BY ID
    # (a missing id is a stand outside the table: td_cost_build never indexes outside it, the cell stays at the fill value)
    to_by_id = np.full(n, -1, np.int32)
    frm_by_id = np.full(n, -1, np.int32)
    to_by_id[c_id] = c_to
    frm_by_id[d_id] = d_frm
    _, r2c, _ = build_assign(to_by_id, frm_by_id, distances, fill=n * n, threshold=-1)
    return expand_x(n, r2c)


def solve(distances, demand, cabs, big_cost=BIG_COST, drop_time=None):
    """greedy_opt.py:102-118 / simulate.py:36-53 -> (n, x, cost); n == 0 -> (0, [], 0)."""
    n, cost = calculate_cost(distances, demand, cabs, big_cost, drop_time)
    if n == 0:
        return 0, [], 0
    r2c, _ = assign(cost, n)
    return n, expand_x(n, r2c), cost


def _lcm(n, c, mask, threshold, stop_value_on, stop_value, stop_size, sum_below, max_pairs=None):
    lib = _ffi.lib()
    if not hasattr(c, "data_ptr"):
        c = _ffi.as_i32(c).reshape(n, n)
    rows = np.empty(max(n, 1), np.int32)
    cols = np.empty(max(n, 1), np.int32)
    k = ctypes.c_int32(0)
    tot = ctypes.c_int64(0)
    lm = ctypes.c_int32(0)
    _ffi.check(lib.td_lcm(n, _ffi.addr(c), int(mask), int(threshold), int(stop_value_on), int(stop_value),
                          int(stop_size), int(sum_below), n if max_pairs is None else int(max_pairs), _ffi.addr(rows), _ffi.addr(cols), ctypes.byref(k),
                          ctypes.byref(tot), ctypes.byref(lm)))
    return int(tot.value), rows[:k.value].copy(), cols[:k.value].copy(), int(lm.value)


def LCM(n, c, threshold=10, big_cost=BIG_COST, with_pairs=False):
    """greedy_opt.py:61-82 (THRESHOLD=10) / simulate.py:76-98 (THRESHOLD=20, with_pairs=True).
    `c` is the cab-major n x n cost (what np.array(matrix(cost).T) is in the reference).
    Returns (total_cost, allocated_supply, allocated_demand[, allocated])."""
    total, rows, cols, _ = _lcm(n, c, big_cost, threshold, 0, 0, -1, big_cost)
    if with_pairs:
        return total, list(map(int, rows)), list(map(int, cols)), list(zip(map(int, rows), map(int, cols)))
    return total, list(map(int, rows)), list(map(int, cols))


def LCM_heuristic(n, c):
    """heuristic.py:24-33: n iterations, every taken cell summed, mask value 100."""
    total, rows, cols, _ = _lcm(n, c, 100, -1, 0, 0, -1, 2**62)
    return total, list(map(int, rows)), list(map(int, cols))


def LCM_simulator(cost, max_non_lcm=600, big_cost=BIG_COST, as_arrays=False):
    """Simulator.java:523-549 -> (pairs [(cab, request)], LCM_min_val); as_arrays=True: (rows, cols, LCM_min_val)
    as int32 arrays (a tick loop that only indexes with them skips ~700 Python tuples per tick)."""
    cost_a = cost if hasattr(cost, "data_ptr") else _ffi.as_i32(cost)
    n = int(cost_a.shape[0])
    _, rows, cols, lm = _lcm(n, cost_a, big_cost, -1, 1, big_cost, max_non_lcm, big_cost)
    if as_arrays:
        return rows, cols, lm
    return list(zip(map(int, rows), map(int, cols))), lm


def tick(cab_to, dem_from, distances=None, big_cost=BIG_COST, drop_time=10, max_non_lcm=600):
    """One dispatcher tick in one C-ABI call (td_tick): calculate_cost -> LCM down to max_non_lcm rows ->
    removal of the matched cabs / requests on the device -> calculate_cost -> optimal assignment
    (Simulator.java:163-208,493-549,613-674; greedy_opt.py:32-37).  cab_to / dem_from: the stands the free cabs
    stand at / the requests start from.  Returns a dict: lcm_rows, lcm_cols (int32 arrays, the reference's pick
    order), lcm_min_val, kept_cabs, kept_dems (positions handed to the solver, in order), n_rest, row_to_col
    (int32[n_rest], indices into kept_cabs -> kept_dems; >= len(kept_dems) or a cab index >= len(kept_cabs): dummy),
    total (the remainder's optimum, dummy cells count big_cost), solved (False when the LCM ran and ended on big_cost:
    like Simulator.java:188-189 the tick then has no input for the solver; row_to_col is empty and total 0)."""
    lib = _ffi.lib()
    cab = cab_to if hasattr(cab_to, "data_ptr") else _ffi.as_i32(cab_to)
    dem = dem_from if hasattr(dem_from, "data_ptr") else _ffi.as_i32(dem_from)
    n_s, n_d = int(cab.shape[0]), int(dem.shape[0])
    n = max(n_s, n_d)
    dptr, S, keep = _dist_arg(distances)
    rows = np.empty(max(n, 1), np.int32)
    cols = np.empty(max(n, 1), np.int32)
    kc = np.empty(max(n_s, 1), np.int32)
    kd = np.empty(max(n_d, 1), np.int32)
    r2c = np.empty(max(n, 1), np.int32)
    k, lm, n2, tot = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    _ffi.check(lib.td_tick(_ffi.addr(cab) if n_s else None, n_s, _ffi.addr(dem) if n_d else None, n_d, dptr, S, int(big_cost),
                           -1 if drop_time is None else int(drop_time), -1 if max_non_lcm is None else int(max_non_lcm),
                           _ffi.addr(rows), _ffi.addr(cols), ctypes.byref(k), ctypes.byref(lm), _ffi.addr(kc), _ffi.addr(kd),
                           ctypes.byref(n2), _ffi.addr(r2c), ctypes.byref(tot)))
    del keep
    kk = k.value
    lcm_ran = max_non_lcm is not None and 0 <= int(max_non_lcm) < n
    solved = n2.value > 0 and not (lcm_ran and lm.value == int(big_cost))
    return {"lcm_rows": rows[:kk], "lcm_cols": cols[:kk], "lcm_min_val": lm.value, "kept_cabs": kc[:n_s - kk],
            "kept_dems": kd[:n_d - kk], "n_rest": n2.value, "row_to_col": r2c[:n2.value if solved else 0], "total": tot.value,
            "solved": solved}


def find_pool(frm, to, distances=None, max_loss=None):
    """Simulator.java:681-758 findPool on the GPU: requests given by their from/to stands ->
    list of (custA, custB, plan, cost) in the order the reference keeps them.  max_loss=None: every ordered pair is a
    candidate (td_pool2); else pool_opt_min.py:56-64's loss tests decide (td_pool2_loss), and fewer than n // 2 plans, or
    none, may come back."""
    lib = _ffi.lib()
    frm, to = _ffi.as_i32(frm), _ffi.as_i32(to)
    n = int(frm.size)
    if n < 2:
        return []
    dptr, S, keep = _dist_arg(distances)
    a = np.empty(n // 2 + 1, np.int32)
    b = np.empty(n // 2 + 1, np.int32)
    plan = np.empty(n // 2 + 1, np.int32)
    cost = np.empty(n // 2 + 1, np.int32)
    k = ctypes.c_int32(0)
    if max_loss is None:
        _ffi.check(lib.td_pool2(n, _ffi.addr(frm), _ffi.addr(to), dptr, S, _ffi.addr(a), _ffi.addr(b), _ffi.addr(plan),
                                _ffi.addr(cost), ctypes.byref(k)))
    else:
        _ffi.check(lib.td_pool2_loss(n, _ffi.addr(frm), _ffi.addr(to), dptr, S, float(max_loss), _ffi.addr(a), _ffi.addr(b),
                                     _ffi.addr(plan), _ffi.addr(cost), ctypes.byref(k)))
    del keep
    return [(int(a[i]), int(b[i]), int(plan[i]), int(cost[i])) for i in range(k.value)]


def find_pool_n(k, demand, distances=None, child=None, children=8, max_happy=0):
    """pool_n.c on the GPU.  demand: rows (id, from, to, max_wait, max_loss) like the reference's
    demand file (pool_n.c:18,29-54; the id column is not used, requests are addressed by position).
    child = t: only the first-pick-up slice findpool.c gives its child t of `children`
    (pool_n.c:243-246); None: all requests as first pick-up.  Returns (int32 array [m, 2k+1] of
    pick-ups, drop-offs, cost in the reference's output order, number of happy plans)."""
    lib = _ffi.lib()
    if not 2 <= int(k) <= 4:
        raise _ffi.TdError("pool size %d (2..4)" % int(k))
    d = _ffi.as_i32(np.asarray(demand).reshape(len(demand), -1))
    n = int(d.shape[0])
    frm, to, wait, loss = (np.ascontiguousarray(d[:, c]) for c in (1, 2, 3, 4))
    if child is None:
        first0, first1 = 0, n
    else:
        step = n // children + 1
        first0 = step * child
        first1 = min(n, first0 + step)
    dptr, S, keep = _dist_arg(distances)
    cap = max(1, n // k + 1)
    out = np.zeros((cap, 2 * k + 1), np.int32)
    m = ctypes.c_int32(0)
    nh = ctypes.c_int64(0)
    _ffi.check(lib.td_pool_n(int(k), n, _ffi.addr(frm), _ffi.addr(to), _ffi.addr(wait), _ffi.addr(loss), dptr, S, int(first0),
                             int(first1), int(max_happy), cap, _ffi.addr(out), ctypes.byref(m), ctypes.byref(nh)))
    del keep
    return out[:m.value].copy(), int(nh.value)


def find_pool_n_banded(k, demand, distances=None, child=None, children=8, plan_buffer=0):
    """td_pool_n_banded: find_pool_n's answer with at most plan_buffer plan keys held at once (0: 4 Mi; at least 24 * len(demand)),
    whatever the number of happy plans.  demand / distances / child / children as find_pool_n takes them.  Returns (records,
    number of happy plans, stats): stats = (bands, enumeration passes, the deepest level a band was cut at, the most keys of
    one band)."""
    lib = _ffi.lib()
    if not 2 <= int(k) <= 4:
        raise _ffi.TdError("pool size %d (2..4)" % int(k))
    d = _ffi.as_i32(np.asarray(demand).reshape(len(demand), -1))
    n = int(d.shape[0])
    frm, to, wait, loss = (np.ascontiguousarray(d[:, c]) for c in (1, 2, 3, 4))
    if child is None:
        first0, first1 = 0, n
    else:
        step = n // children + 1
        first0 = step * child
        first1 = min(n, first0 + step)
    dptr, S, keep = _dist_arg(distances)
    cap = max(1, n // k + 1)
    out = np.zeros((cap, 2 * k + 1), np.int32)
    m = ctypes.c_int32(0)
    nh = ctypes.c_int64(0)
    stats = np.zeros(4, np.int64)
    _ffi.check(lib.td_pool_n_banded(int(k), n, _ffi.addr(frm), _ffi.addr(to), _ffi.addr(wait), _ffi.addr(loss), dptr, S, int(first0),
                                    int(first1), int(plan_buffer), cap, _ffi.addr(out), ctypes.byref(m), ctypes.byref(nh), _ffi.addr(stats)))
    del keep
    return out[:m.value].copy(), int(nh.value), tuple(int(v) for v in stats)


def merge_pools(k, n_requests, lists):
    """findpool.c:73-98,166-172: the children's lists (in child order) merged into one list of pools
    that share no request; sorted by cost first for 4-passenger pools only, as the reference does."""
    lib = _ffi.lib()
    parts = [np.asarray(x, np.int32).reshape(-1, 2 * k + 1) for x in lists]
    allp = np.ascontiguousarray(np.concatenate(parts, 0)) if parts else np.zeros((0, 2 * k + 1), np.int32)
    cap = max(1, n_requests // k + 1)
    out = np.zeros((cap, 2 * k + 1), np.int32)
    m = ctypes.c_int32(0)
    _ffi.check(lib.td_pool_merge(int(k), int(n_requests), int(allp.shape[0]), _ffi.addr(allp) if allp.size else None,
                                 1 if k == 4 else 0, cap, _ffi.addr(out), ctypes.byref(m)))
    return out[:m.value].copy()


POOL_N_BATCHED_NMAX = 512   # largest model of pool_n_batched


def pack_pool_n(demands, firsts=None):
    """pool_n_batched's packing: a list of demand row arrays (id, from, to, max_wait, max_loss) -> (off int32[B + 1], from,
    to, max_wait, max_loss int32[all requests], first int32[B, 2] or None, batch, n = the largest model).  firsts: per model
    None (every request may be the first pick-up) or a (first0, first1) slice."""
    rows = [_ffi.as_i32(np.asarray(d).reshape(len(d), -1)) if len(d) else np.zeros((0, 5), np.int32) for d in demands]
    for b, d in enumerate(rows):
        if d.shape[1] < 5:
            raise _ffi.TdError("model %d: demand rows are (id, from, to, max_wait, max_loss)" % b)
    batch = len(rows)
    sizes = np.array([d.shape[0] for d in rows], np.int64)
    off = np.zeros(batch + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    allr = np.concatenate(rows, 0) if batch else np.zeros((0, 5), np.int32)
    frm, to, wait, loss = (np.ascontiguousarray(allr[:, c]) for c in (1, 2, 3, 4))
    first = None
    if firsts is not None:
        if len(firsts) != batch:
            raise _ffi.TdError("%d first-pick-up slices for %d models" % (len(firsts), batch))
        first = np.zeros((batch, 2), np.int32)
        for b, f in enumerate(firsts):
            first[b] = (0, sizes[b]) if f is None else (int(f[0]), int(f[1]))
    return off, frm, to, wait, loss, first, batch, int(sizes.max()) if batch else 0


def pool_n_batched(k, demands, distances=None, firsts=None, max_happy=0):
    """td_pool_n_batched: pool_n.c for B models in one call, one shared distance table (None: |a - b|).  demands: a list of
    row arrays (id, from, to, max_wait, max_loss) as find_pool_n takes, each of at most 512 requests; firsts: per model None or
    its first-pick-up slice (first0, first1).  Returns (a list of int32 arrays [m_b, 2k+1] of pick-ups, drop-offs, cost in the
    reference's output order, request indices being positions within the model; int64[B] happy plans per model)."""
    lib = _ffi.lib()
    if not 2 <= int(k) <= 4:
        raise _ffi.TdError("pool size %d (2..4)" % int(k))
    off, frm, to, wait, loss, first, batch, n = pack_pool_n(demands, firsts)
    dptr, S, keep = _dist_arg(distances)
    per = n // int(k)
    pools = _out((batch, per, 2 * int(k) + 1), np.int32)
    m, nh = _out((batch,), np.int32), _out((batch,), np.int64)
    _ffi.check(lib.td_pool_n_batched(int(k), batch, n, _ffi.addr(off), _ffi.addr(frm), _ffi.addr(to), _ffi.addr(wait), _ffi.addr(loss),
                                     dptr, S, _ffi.addr(first), int(max_happy), _ffi.addr(pools), _ffi.addr(m), _ffi.addr(nh), None))
    del keep
    return [pools[b, :int(m[b])].copy() for b in range(batch)], nh


def pool_n_banded_batched(k, demands, distances=None, firsts=None, plan_buffer=0, stats=False):
    """td_pool_n_banded_batched: pool_n_batched's arguments and answer with at most plan_buffer plan keys held per workgroup
    (0: 65536; at least 24 * the largest model, at most 2^22), whatever a model's number of happy plans.  Returns (records per
    model, int64[B] happy plans per model), and with stats=True a third value: int64[B, 4], per model (bands, enumeration
    passes, the deepest level a band was cut at, the most keys of one band)."""
    lib = _ffi.lib()
    if not 2 <= int(k) <= 4:
        raise _ffi.TdError("pool size %d (2..4)" % int(k))
    off, frm, to, wait, loss, first, batch, n = pack_pool_n(demands, firsts)
    dptr, S, keep = _dist_arg(distances)
    per = n // int(k)
    pools = _out((batch, per, 2 * int(k) + 1), np.int32)
    m, nh, st = _out((batch,), np.int32), _out((batch,), np.int64), _out((batch, 4), np.int64)
    _ffi.check(lib.td_pool_n_banded_batched(int(k), batch, n, _ffi.addr(off), _ffi.addr(frm), _ffi.addr(to), _ffi.addr(wait), _ffi.addr(loss),
                                            dptr, S, _ffi.addr(first), int(plan_buffer), _ffi.addr(pools), _ffi.addr(m), _ffi.addr(nh), None,
                                            _ffi.addr(st) if stats else None))
    del keep
    lists = [pools[b, :int(m[b])].copy() for b in range(batch)]
    return (lists, nh, st) if stats else (lists, nh)


def find_pool_fanout(k, demand, distances=None, children=8, plan_buffer=None):
    """findpool.c as two calls: its `children` first-pick-up slices (pool_n.c:243-246) as one batch of `children` models of
    the same demand, then the merge (findpool.c:73-98,166-172).  Returns the merged int32 array [m, 2k+1].  plan_buffer: the
    children go through pool_n_banded_batched with this buffer (0: its default) instead of pool_n_batched."""
    d = np.asarray(demand).reshape(len(demand), -1)
    n = int(d.shape[0])
    step = n // children + 1
    firsts = [(step * c, min(n, step * c + step)) for c in range(children)]
    if plan_buffer is None:
        lists, _ = pool_n_batched(k, [d] * children, distances, firsts)
    else:
        lists, _ = pool_n_banded_batched(k, [d] * children, distances, firsts, plan_buffer)
    return merge_pools(k, n, lists)


def count_sum(nn, cost, res, big_cost=BIG_COST):
    """greedy_opt.py:21-29 with positional lists: because cost[taxi][trip] IS
    dist[supply[taxi].to][demand[trip].from] for every real cell, the sum over x==1 cells with
    cost < big_cost equals the reference's sum of dist[...] terms. `res` is x (n*n) or row_to_col."""
    res = np.asarray(res)
    if nn == 1:
        # x = [1] and row_to_col = [0] have the same size: with one row the only assignment is column 0
        r2c = np.zeros(1, np.int32)
    elif res.size == nn * nn:
        r2c = np.full(nn, -1, np.int32)
        ii, jj = np.nonzero(res.reshape(nn, nn) == 1)
        r2c[ii] = jj
    else:
        r2c = _ffi.as_i32(res)
    s = ctypes.c_int64(0)
    k = ctypes.c_int32(0)
    if not hasattr(cost, "data_ptr"):
        cost = _ffi.as_i32(cost)
    _ffi.check(_ffi.lib().td_count_sum(nn, _ffi.addr(cost), _ffi.addr(r2c), int(big_cost), ctypes.byref(s),
                                       ctypes.byref(k)))
    return int(s.value)


def filter_out(input, allocated, element=None):
    """element given: greedy_opt.py:32-37 (drop rows whose row[element] is in `allocated`);
    element None: simulate.py:64-69 (drop by position). Host list bookkeeping, O(n)."""
    alloc = set(int(a) for a in allocated)
    if element is None:
        output = [row for i, row in enumerate(input) if i not in alloc]
    else:
        output = [row for row in input if row[element] not in alloc]
    return len(output), output


def combined(distances, demand, cabs, threshold=10, big_cost=BIG_COST):
    """greedy_opt.py:136-160: optimal solve, then LCM(threshold) + optimal on the remainder.
    Returns (nn, res, n2, res2 + lcm) — the four numbers the reference appends to its log."""
    nn, x, cost_table = solve(distances, demand, cabs, big_cost)
    if nn == 0:
        return 0, 0, 0, 0
    res = count_sum(nn, cost_table, x, big_cost)
    lcm, allocated_cabs, allocated_cust = LCM(nn, cost_table, threshold, big_cost)
    # ids equal positions in rand_list (greedy_opt.py:47-50) but filter by the records' own id
    cabs = list(cabs)
    demand = list(demand)
    cab_ids = [cabs[i][0] for i in allocated_cabs if i < len(cabs)]
    cust_ids = [demand[i][0] for i in allocated_cust if i < len(demand)]
    _, rest_demand = filter_out(demand, cust_ids, 0)
    _, rest_cabs = filter_out(cabs, cab_ids, 0)
    n2, x2, cost_table2 = solve(distances, rest_demand, rest_cabs, big_cost)
    res2 = count_sum(n2, cost_table2, x2, big_cost) if n2 else 0
    return nn, res, n2, res2 + lcm


# ----------------------------------------------------------------------------------------
# many small models per call (td_assign_batched / td_lcm_batched)
# ----------------------------------------------------------------------------------------
BATCH_NMAX = 1024   # largest model of a batched call; a larger one is one assign() call


def pack_batch(costs, ns=None):
    """Batched input -> (cost, ns, batch, n).  `costs` is a (B, n, n) int32 array-like or torch CUDA int32 tensor
    (handed on as it is), or a list of 2-D square arrays of different sizes: those are packed into a zero-padded
    (B, n, n) slab with n = the largest size and ns = their sizes.  `ns` given with a list is refused."""
    if isinstance(costs, (list, tuple)) and (len(costs) == 0 or np.ndim(costs[0]) == 2):
        if ns is not None:
            raise _ffi.TdError("ns is derived from the list of models; do not pass it as well")
        mats = [_ffi.as_i32(c) for c in costs]
        for k, m in enumerate(mats):
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise _ffi.TdError("model %d is not a square matrix: shape %s" % (k, m.shape))
        sizes = np.array([m.shape[0] for m in mats], np.int32)
        n = int(sizes.max()) if len(mats) else 0
        slab = np.zeros((len(mats), n, n), np.int32)
        for k, m in enumerate(mats):
            slab[k, :m.shape[0], :m.shape[0]] = m
        return slab, sizes, len(mats), n
    if hasattr(costs, "data_ptr") and not isinstance(costs, np.ndarray):
        _require_i32(costs, "costs")
        cost = costs
    else:
        cost = _ffi.as_i32(costs)
    if cost.ndim != 3 or cost.shape[1] != cost.shape[2]:
        raise _ffi.TdError("costs must be a (B, n, n) batch of square models, got shape %s" % (tuple(cost.shape),))
    batch, n = int(cost.shape[0]), int(cost.shape[1])
    if ns is not None:
        ns = ns if hasattr(ns, "data_ptr") and not isinstance(ns, np.ndarray) else _ffi.as_i32(ns).reshape(-1)
        if int(ns.shape[0]) != batch:
            raise _ffi.TdError("ns has %d entries for a batch of %d" % (int(ns.shape[0]), batch))
    return cost, ns, batch, n


def assign_batched(costs, ns=None, want_dual=False, want_prices=False):
    """td_assign_batched: the optimum of B independent square models (n <= 1024) in one call (heuristic.py:20-40's 1000
    scenarios, split.py:61-120's regions).  costs: see pack_batch; ns (int32[B]): model b is the top-left ns[b] x ns[b]
    block of its slab.  Returns (row_to_col int32[B, n] (-1 beyond ns[b]), total int64[B][, dual_bound int64[B]]
    [, col_price int64[B, n]])."""
    lib = _ffi.lib()
    cost, ns, batch, n = pack_batch(costs, ns)
    r2c = np.empty((batch, n), np.int32)
    total = np.empty(batch, np.int64)
    dual = np.empty(batch, np.int64) if want_dual else None
    price = np.empty((batch, n), np.int64) if want_prices else None
    _ffi.check(lib.td_assign_batched(batch, n, _ffi.addr(ns), _ffi.addr(cost) if batch * n else None, _ffi.addr(r2c),
                                     _ffi.addr(total), _ffi.addr(dual), _ffi.addr(price)))
    out = (r2c, total)
    if want_dual:
        out += (dual,)
    if want_prices:
        out += (price,)
    return out


def LCM_batched(costs, ns=None, mask=BIG_COST, threshold=-1, stop_value_on=0, stop_value=0, stop_size=-1, sum_below=2**62):
    """td_lcm_batched: td_lcm's greedy (same parameters as _lcm / td_lcm) on every model of a batch.  costs / ns: as
    assign_batched.  Returns (total int64[B], rows int32[B, n], cols int32[B, n], last_min int32[B], n_pairs int32[B]);
    model b's pairs are rows[b, :n_pairs[b]], cols[b, :n_pairs[b]] in pick order."""
    lib = _ffi.lib()
    cost, ns, batch, n = pack_batch(costs, ns)
    rows = np.full((batch, n), -1, np.int32)
    cols = np.full((batch, n), -1, np.int32)
    k = np.empty(batch, np.int32)
    total = np.empty(batch, np.int64)
    lm = np.empty(batch, np.int32)
    _ffi.check(lib.td_lcm_batched(batch, n, _ffi.addr(ns), _ffi.addr(cost) if batch * n else None, int(mask), int(threshold),
                                  int(stop_value_on), int(stop_value), int(stop_size), int(sum_below), _ffi.addr(rows),
                                  _ffi.addr(cols), _ffi.addr(k), _ffi.addr(total), _ffi.addr(lm)))
    return total, rows, cols, lm, k


def heuristic_gap(n=100, iters=1000, seed=None):
    """heuristic.py:20-40 as two library calls: `iters` models of n x n costs U{1..39}, LCM with mask 100 and n picks
    (every taken cell summed), then the optimum of each.  Returns (lcm_totals int64[iters], optima int64[iters],
    mean gap in % = mean of 100 * (lcm - opt) / opt).  Raises when an optimum exceeds its LCM total (heuristic.py:40's
    "!!!" detector: the solver failed)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 40, (iters, n, n)).astype(np.int32)
    lcm_tot = LCM_batched(c, mask=100, threshold=-1)[0]
    _, opt = assign_batched(c)
    bad = np.nonzero(opt > lcm_tot)[0]
    if bad.size:
        raise _ffi.TdError("optimum above the LCM total in %d scenarios (first: %d: %d > %d)"
                           % (bad.size, int(bad[0]), int(opt[bad[0]]), int(lcm_tot[bad[0]])))
    return lcm_tot, opt, float(np.mean(100.0 * (lcm_tot - opt) / opt))


# ----------------------------------------------------------------------------------------
# many dispatch models from their positions per call (td_build_assign_batched / td_tick_batched)
# ----------------------------------------------------------------------------------------
TICK_BATCH_NMAX = 2048   # largest model of tick_batched (Simulator.java's 1300 x 900 tick); its remainder is <= BATCH_NMAX


def _ragged(side, what):
    """one side of pack_ragged -> (values, offsets, host offsets int64)"""
    if isinstance(side, tuple):
        if len(side) != 2:
            raise _ffi.TdError("%s: a ready ragged input is a (values, offsets) pair" % what)
        vals, offs = side
        if hasattr(vals, "data_ptr") and not isinstance(vals, np.ndarray):
            _require_i32(vals, what + " values")
            n_vals = int(vals.numel())
        else:
            vals = _ffi.as_i32(vals).reshape(-1)
            n_vals = int(vals.size)
        if hasattr(offs, "data_ptr") and not isinstance(offs, np.ndarray):
            _require_i32(offs, what + " offsets")
            h = offs.detach().cpu().numpy().astype(np.int64).reshape(-1)
        else:
            offs = _ffi.as_i32(offs).reshape(-1)
            h = offs.astype(np.int64)
        if h.size == 0 or h[0] != 0:
            raise _ffi.TdError("%s: offsets must start at 0" % what)
        if (np.diff(h) < 0).any():
            raise _ffi.TdError("%s: offsets decrease" % what)
        if h[-1] > n_vals:
            raise _ffi.TdError("%s: offset %d beyond the %d values" % (what, int(h[-1]), n_vals))
        return vals, offs, h
    models = [_ffi.as_i32(m).reshape(-1) for m in side]
    h = np.zeros(len(models) + 1, np.int64)
    h[1:] = np.cumsum([m.size for m in models])
    if h[-1] > 2**31 - 1:
        raise _ffi.TdError("%s: more than 2^31 - 1 positions" % what)
    vals = np.ascontiguousarray(np.concatenate(models)) if models else np.zeros(0, np.int32)
    return vals.astype(np.int32, copy=False), h.astype(np.int32), h


def pack_ragged(cab_tos, dem_froms):
    """Ragged batch of dispatch models -> (cab_values, cab_offsets, dem_values, dem_offsets, batch, n).  Each side is a list
    of 1-D position arrays (one per model), or a ready (values, offsets) tuple (numpy, or torch CUDA int32 tensors handed on as
    they are; offsets int32[B+1] from 0, never decreasing, the last one within the values).  n = the largest max(n_s, n_d)."""
    cv, co, ch = _ragged(cab_tos, "cab_tos")
    dv, do, dh = _ragged(dem_froms, "dem_froms")
    if ch.size != dh.size:
        raise _ffi.TdError("%d cab lists for %d request lists" % (ch.size - 1, dh.size - 1))
    batch = int(ch.size - 1)
    n = int(np.maximum(np.diff(ch), np.diff(dh)).max()) if batch else 0
    return cv, co, dv, do, batch, n


def _out(shape, dtype):
    """an output of `shape` whose address is never null (an empty model list still hands the C ABI an array)"""
    size = int(np.prod(shape))
    return np.empty(max(size, 1), dtype)[:size].reshape(shape)


def build_assign_batched(cab_tos, dem_froms, distances=None, fill=BIG_COST, threshold=-1, want_dual=False):
    """td_build_assign_batched: build_assign of B ragged dispatch models in one call, one shared distance table (None: |a - b|);
    no cost matrix is written.  cab_tos / dem_froms: see pack_ragged.  Returns (row_to_col int32[B, n] (-1 beyond a model's
    max(n_s, n_d)), total int64[B][, dual_bound int64[B]])."""
    lib = _ffi.lib()
    cv, co, dv, do, batch, n = pack_ragged(cab_tos, dem_froms)
    dptr, S, keep = _dist_arg(distances)
    r2c = _out((batch, n), np.int32)
    total = _out((batch,), np.int64)
    dual = _out((batch,), np.int64) if want_dual else None
    _ffi.check(lib.td_build_assign_batched(batch, n, _ffi.addr(co), _ffi.addr(cv), _ffi.addr(do), _ffi.addr(dv), dptr, S, int(fill),
                                           int(threshold), _ffi.addr(r2c), _ffi.addr(total), _ffi.addr(dual)))
    del keep
    return (r2c, total, dual) if want_dual else (r2c, total)


def tick_batched(cab_tos, dem_froms, distances=None, big_cost=BIG_COST, drop_time=10, max_non_lcm=600):
    """td_tick_batched: tick() of B ragged dispatch models in one call (two launches), one shared distance table.
    cab_tos / dem_froms: see pack_ragged.  Returns a list of B dicts with tick()'s keys and meanings (lcm_min_val is
    big_cost where the LCM did not run), plus dual_bound (== total certifies the remainder's optimum; 0 without a solve)."""
    lib = _ffi.lib()
    cv, co, dv, do, batch, n = pack_ragged(cab_tos, dem_froms)
    ch = np.asarray(co.detach().cpu().numpy() if hasattr(co, "detach") else co, np.int64)
    dh = np.asarray(do.detach().cpu().numpy() if hasattr(do, "detach") else do, np.int64)
    dptr, S, keep = _dist_arg(distances)
    rows, cols, kc, kd, r2c = (_out((batch, n), np.int32) for _ in range(5))
    k, lm, n2 = (_out((batch,), np.int32) for _ in range(3))
    total, dual = _out((batch,), np.int64), _out((batch,), np.int64)
    stop = -1 if max_non_lcm is None else int(max_non_lcm)
    _ffi.check(lib.td_tick_batched(batch, n, _ffi.addr(co), _ffi.addr(cv), _ffi.addr(do), _ffi.addr(dv), dptr, S, int(big_cost),
                                   -1 if drop_time is None else int(drop_time), stop, _ffi.addr(rows), _ffi.addr(cols), _ffi.addr(k),
                                   _ffi.addr(lm), _ffi.addr(kc), _ffi.addr(kd), _ffi.addr(n2), _ffi.addr(r2c), _ffi.addr(total),
                                   _ffi.addr(dual)))
    del keep
    out = []
    for b in range(batch):
        n_s, n_d = int(ch[b + 1] - ch[b]), int(dh[b + 1] - dh[b])
        kk, nr = int(k[b]), int(n2[b])
        lcm_ran = 0 <= stop < max(n_s, n_d)
        solved = nr > 0 and not (lcm_ran and int(lm[b]) == int(big_cost))
        out.append({"lcm_rows": rows[b, :kk], "lcm_cols": cols[b, :kk], "lcm_min_val": int(lm[b]), "kept_cabs": kc[b, :n_s - kk],
                    "kept_dems": kd[b, :n_d - kk], "n_rest": nr, "row_to_col": r2c[b, :nr if solved else 0], "total": int(total[b]),
                    "solved": solved, "dual_bound": int(dual[b])})
    return out


# ----------------------------------------------------------------------------------------
# the split heuristic as a whole (td_split_batched)
# ----------------------------------------------------------------------------------------
def split_batched(cab_tos, dem_froms, size, parts=4, distances=None, fill=BIG_COST):
    """td_split_batched: split.py:61-119 of B ragged cases in one call: the stand ranges of `size` stands in `parts` parts
    (size / parts stands each, a short extra range when parts does not divide size) solved as region models, then one solve
    per case over whoever the regions left over.  cab_tos / dem_froms: see pack_ragged; one shared distance table (None:
    |a - b|).  Returns a dict: cab_req int32[all cabs] (the index within the case's request list of the request a cab serves,
    or -1; case c's cabs at cab_off[c] : cab_off[c + 1]), cab_stage (0 region, 1 fifth solve, -1 not served), total int64[B],
    rest_total int64[B] (the fifth solve's part), n_rest int32[B, 2] (rest cabs, rest requests), dual_gap int64[B] (0 certifies
    every model of the case), cab_off int64[B + 1]."""
    lib = _ffi.lib()
    cv, co, dv, do, batch, n = pack_ragged(cab_tos, dem_froms)
    ch = np.asarray(co.detach().cpu().numpy() if hasattr(co, "detach") else co, np.int64)
    dptr, S, keep = _dist_arg(distances)
    nc = int(ch[-1])
    req, stage = _out((nc,), np.int32), _out((nc,), np.int32)
    total, rest, gap = (_out((batch,), np.int64) for _ in range(3))
    n_rest = _out((batch, 2), np.int32)
    _ffi.check(lib.td_split_batched(batch, n, _ffi.addr(co), _ffi.addr(cv), _ffi.addr(do), _ffi.addr(dv), dptr, S, int(size), int(parts),
                                    int(fill), _ffi.addr(req), _ffi.addr(stage), _ffi.addr(total), _ffi.addr(rest), _ffi.addr(n_rest),
                                    _ffi.addr(gap)))
    del keep
    return {"cab_req": req, "cab_stage": stage, "total": total, "rest_total": rest, "n_rest": n_rest, "dual_gap": gap, "cab_off": ch}


# ----------------------------------------------------------------------------------------
# many dispatch models per call, a dispatch method per model (td_dispatch_batched)
# ----------------------------------------------------------------------------------------
DISPATCH_MODES = {"lcm+opt": 0, "opt": 1, "lcm": 2, "split": 3}   # TD_DISPATCH_LCM_OPT / _OPT / _LCM / _SPLIT: the one table


def dispatch_mode(m):
    """a dispatch method as the C ABI's number: a name of DISPATCH_MODES, or the number itself"""
    if isinstance(m, str):
        if m not in DISPATCH_MODES:
            raise _ffi.TdError("dispatch method %r is none of %s" % (m, sorted(DISPATCH_MODES)))
        return DISPATCH_MODES[m]
    return int(m)


def _policy(v, batch, what, conv=int):
    """one policy argument of dispatch_batched -> None, a torch CUDA int32 tensor handed on as it is, or int32[batch]"""
    if v is None:
        return None
    if hasattr(v, "data_ptr") and not isinstance(v, np.ndarray):
        _require_i32(v, what)
        if int(v.numel()) != batch:
            raise _ffi.TdError("%s has %d entries for %d models" % (what, int(v.numel()), batch))
        return v
    if isinstance(v, (str, int, np.integer)):
        return np.full(max(batch, 1), conv(v), np.int32)[:batch]
    a = np.ascontiguousarray([conv(x) for x in v], np.int32).reshape(-1)
    if a.size != batch:
        raise _ffi.TdError("%s has %d entries for %d models" % (what, a.size, batch))
    return a


def dispatch_batched(cab_tos, dem_froms, distances=None, big_cost=BIG_COST, drop_time=10, size=None, mode=None, max_non_lcm=None,
                     parts=None, n=None):
    """td_dispatch_batched: B ragged dispatch models in one call, a dispatch method per model.  cab_tos / dem_froms: see
    pack_ragged; one shared distance table (None: |a - b|).  mode: "lcm+opt" (tick_batched with the model's own max_non_lcm),
    "opt", "lcm" (the LCM to its end, never a solve) or "split" (split.py:61-119 on the cells below drop_time, parts ranges over
    `size` stands; size defaults to the table's), or their numbers; mode / max_non_lcm / parts are a scalar for all models, a
    list per model, a torch CUDA int32 tensor, or None (lcm+opt / the LCM never runs / 4).  n: the output stride (default: the
    largest model).  Returns a dict of td_tick_batched's arrays: lcm_rows, lcm_cols, kept_cabs, kept_dems, row_to_col
    int32[B, n]; n_pairs, lcm_min_val, n_rest int32[B]; total, dual_bound int64[B]; for a split model row_to_col[b, i] is the
    request cab i serves (or -1) and dual_bound == total certifies every model solved for it."""
    lib = _ffi.lib()
    cv, co, dv, do, batch, nmax = pack_ragged(cab_tos, dem_froms)
    n = nmax if n is None else int(n)
    dptr, S, keep = _dist_arg(distances)
    if size is None:
        size = S
    md = _policy(mode, batch, "mode", dispatch_mode)
    st = _policy(max_non_lcm, batch, "max_non_lcm")
    pt = _policy(parts, batch, "parts")
    rows, cols, kc, kd, r2c = (_out((batch, n), np.int32) for _ in range(5))
    k, lm, n2 = (_out((batch,), np.int32) for _ in range(3))
    total, dual = _out((batch,), np.int64), _out((batch,), np.int64)
    _ffi.check(lib.td_dispatch_batched(batch, n, _ffi.addr(co), _ffi.addr(cv), _ffi.addr(do), _ffi.addr(dv), dptr, S, int(big_cost),
                                       -1 if drop_time is None else int(drop_time), int(size), _ffi.addr(md), _ffi.addr(st),
                                       _ffi.addr(pt), _ffi.addr(rows), _ffi.addr(cols), _ffi.addr(k), _ffi.addr(lm), _ffi.addr(kc),
                                       _ffi.addr(kd), _ffi.addr(n2), _ffi.addr(r2c), _ffi.addr(total), _ffi.addr(dual)))
    del keep
    return {"lcm_rows": rows, "lcm_cols": cols, "n_pairs": k, "lcm_min_val": lm, "kept_cabs": kc, "kept_dems": kd, "n_rest": n2,
            "row_to_col": r2c, "total": total, "dual_bound": dual}


def solve_split(distances, demand, cabs, size, parts=4):
    """split.py:61-119 for one case in the reference's call shape: demand / cabs are (id, from, to) records, a cab stands at
    its `to`, a request at its `from`.  Returns the split total, or None when either list is empty (split.py:62-64)."""
    demand, cabs = list(demand), list(cabs)
    if not demand or not cabs:
        return None
    _, d_frm, _ = _records(demand)
    _, _, c_to = _records(cabs)
    return int(split_batched([c_to], [d_frm], size, parts, distances)["total"][0])


def _rand_positions(rng, numb, size, cases, column):
    """rand_list (split.py:41-52) for `cases` lists: numb draws of (from, to) in [0, size), a record with from == to is dropped;
    returns the kept records' `column` (0 = from, 1 = to) per list"""
    ft = rng.integers(0, size, (cases, numb, 2))
    keep = ft[:, :, 0] != ft[:, :, 1]
    return [ft[c, keep[c], column].astype(np.int32) for c in range(cases)]


def split_gap(n_stands=20, n_size=10, cases=1000, seed=None, parts=4):
    """split.py's main as library calls, for `cases` random cases on the line of n_stands stands: the unsplit optimum
    (build_assign_batched), the split total (split_batched) and split.py:161-175's LCM (LCM_batched over chunks of cases whose
    cost slab stays below 256 MiB), each summed over real cells only.  Returns (optima, split_totals, lcm_totals int64[cases],
    split gap, LCM gap), a gap being 100 * (sum x - sum opt) / sum opt.  Raises when a split total is below its optimum."""
    rng = np.random.default_rng(seed)
    dems = _rand_positions(rng, n_size, n_stands, cases, 0)
    cabs = _rand_positions(rng, n_size, n_stands, cases, 1)
    n_s = np.array([c.size for c in cabs], np.int64)
    n_d = np.array([d.size for d in dems], np.int64)
    nb = np.maximum(n_s, n_d)
    _, padded = build_assign_batched(cabs, dems)
    opt = np.where((n_s > 0) & (n_d > 0), padded - np.abs(n_s - n_d) * BIG_COST, 0)   # dummy cells count fill in td_build_assign
    split = split_batched(cabs, dems, n_stands, parts)["total"].astype(np.int64)
    bad = np.nonzero(split < opt)[0]
    if bad.size:
        raise _ffi.TdError("split total below the optimum in %d cases (first: %d: %d < %d)"
                           % (bad.size, int(bad[0]), int(split[bad[0]]), int(opt[bad[0]])))
    n = int(nb.max()) if cases else 0
    lcm = np.zeros(cases, np.int64)
    chunk = max(1, (256 * 2**20 - 1) // max(1, 4 * n * n))
    for lo in range(0, cases if n else 0, chunk):
        hi = min(cases, lo + chunk)
        pc = np.zeros((hi - lo, n), np.int32)
        pd = np.zeros((hi - lo, n), np.int32)
        for k in range(lo, hi):
            pc[k - lo, :n_s[k]] = cabs[k]
            pd[k - lo, :n_d[k]] = dems[k]
        real = (np.arange(n)[None, :, None] < n_s[lo:hi, None, None]) & (np.arange(n)[None, None, :] < n_d[lo:hi, None, None])
        slab = np.where(real, np.abs(pc[:, :, None] - pd[:, None, :]), BIG_COST).astype(np.int32)
        lcm[lo:hi] = LCM_batched(slab, nb[lo:hi].astype(np.int32), mask=BIG_COST, threshold=-1, sum_below=BIG_COST)[0]
    so = float(opt.sum())
    gaps = tuple(100.0 * (float(x.sum()) - so) / so if so else 0.0 for x in (split, lcm))
    return opt, split, lcm, gaps[0], gaps[1]


# ----------------------------------------------------------------------------------------
# maximum-weight matching of many general graphs, optimal pools of two (td_match_batched / td_pool2_batched)
# ----------------------------------------------------------------------------------------
MATCH_NMAX = 2048   # largest model of match_batched / pool2_batched


def match_batched(weights, ns=None, want_dual=False):
    """td_match_batched: the maximum-weight matching of B general graphs (n <= 2048) in one call.  weights: see pack_batch
    (edge {i, j} weighs max(W[i][j], W[j][i]); <= 0 is no edge).  Returns (mate int32[B, n] (-1: unmatched or beyond ns[b]),
    total int64[B], dual_bound int64[B]) -- dual_bound == total certifies the maximum -- and with want_dual the certificate
    (y int64[B, n], blossom_parent int32[B, 2n], z int64[B, n]) in doubled units (see the header)."""
    lib = _ffi.lib()
    w, ns, batch, n = pack_batch(weights, ns)
    mate = _out((batch, n), np.int32)
    total, bound = _out((batch,), np.int64), _out((batch,), np.int64)
    y = _out((batch, n), np.int64) if want_dual else None
    par = _out((batch, 2 * n), np.int32) if want_dual else None
    z = _out((batch, n), np.int64) if want_dual else None
    _ffi.check(lib.td_match_batched(batch, n, _ffi.addr(ns), _ffi.addr(w) if batch * n else None, _ffi.addr(mate), _ffi.addr(total),
                                    _ffi.addr(bound), _ffi.addr(y), _ffi.addr(par), _ffi.addr(z)))
    return (mate, total, bound, (y, par, z)) if want_dual else (mate, total, bound)


def pool2_batched(froms, tos, distances=None, max_loss=None, optimal=True, n=None):
    """td_pool2_batched: pools of two for B ragged models in one call, one shared distance table (None: |a - b|).
    froms / tos: ragged lists as in pack_ragged (the same model sizes on both sides).  max_loss=None: every ordered pair is a
    candidate (Simulator.java:691); else pool_opt_min.py:58-64's loss tests.  optimal=False: the reference's greedy in its
    keep order; optimal=True: the most pools, then the least total cost, in ascending (cost, custA, custB).
    max_loss and optimal may also be lists with one entry per model (None in a max_loss list: every ordered pair for that
    model): td_pool2_batched_v, the same launches whatever the mix; model b comes out exactly as a uniform call on it alone.
    Returns (cust_a, cust_b, plan, cost: int32[B, n // 2], n_pools int32[B], total int64[B]); model b's pools are the first
    n_pools[b] entries of its rows; customer indices are positions within the model.
    n: the stride of the pair-cost slab and of the outputs (default: the longest model); refused when below the longest model
    or above MATCH_NMAX.  A larger n answers the same, with fewer models per 256 MiB chunk."""
    lib = _ffi.lib()
    fv, fo, fh = _ragged(froms, "froms")
    tv, _, th = _ragged(tos, "tos")
    if not np.array_equal(fh, th):
        raise _ffi.TdError("froms and tos must describe the same models (equal offsets)")
    batch = int(fh.size - 1)
    longest = int(np.diff(fh).max()) if batch else 0
    if n is None:
        n = longest
    elif int(n) < longest or int(n) > MATCH_NMAX:
        raise _ffi.TdError("n = %d: below the longest model (%d customers) or above %d" % (int(n), longest, MATCH_NMAX))
    n = int(n)
    dptr, S, keep = _dist_arg(distances)
    half = n // 2
    a, b, plan, cost = (_out((batch, half), np.int32) for _ in range(4))
    k, total = _out((batch,), np.int32), _out((batch,), np.int64)
    ml_list = isinstance(max_loss, (list, tuple, np.ndarray))
    opt_list = isinstance(optimal, (list, tuple, np.ndarray))
    if ml_list or opt_list:
        mlv = optv = None
        if max_loss is not None:
            mlv = np.array([0.0 if x is None else float(x) for x in (max_loss if ml_list else [max_loss] * batch)], np.float64)
        if opt_list or optimal:
            optv = np.array([int(x) for x in (optimal if opt_list else [1] * batch)], np.int32)
        for v, what in ((mlv, "max_loss"), (optv, "optimal")):
            if v is not None and v.size != batch:
                raise _ffi.TdError("%s has %d entries for %d models" % (what, v.size, batch))
        _ffi.check(lib.td_pool2_batched_v(batch, n, _ffi.addr(fo), _ffi.addr(fv), _ffi.addr(tv), dptr, S, _ffi.addr(mlv), _ffi.addr(optv),
                                          _ffi.addr(a), _ffi.addr(b), _ffi.addr(plan), _ffi.addr(cost), _ffi.addr(k), _ffi.addr(total)))
    else:
        ml = 0.0 if max_loss is None else float(max_loss)
        _ffi.check(lib.td_pool2_batched(batch, n, _ffi.addr(fo), _ffi.addr(fv), _ffi.addr(tv), dptr, S, ml, 1 if optimal else 0,
                                        _ffi.addr(a), _ffi.addr(b), _ffi.addr(plan), _ffi.addr(cost), _ffi.addr(k), _ffi.addr(total)))
    del keep
    return a, b, plan, cost, k, total


def find_pool_optimal(frm, to, distances=None, max_loss=None):
    """The optimal pools of two of one model in find_pool's format: a list of (custA, custB, plan, cost), the most pools and
    among those the least total cost, in ascending (cost, custA, custB); drops in where find_pool is used."""
    frm, to = _ffi.as_i32(frm).reshape(-1), _ffi.as_i32(to).reshape(-1)
    a, b, plan, cost, k, _ = pool2_batched([frm], [to], distances, max_loss, optimal=True)
    return [(int(a[0, i]), int(b[0, i]), int(plan[0, i]), int(cost[0, i])) for i in range(int(k[0]))]


def pool_gap(n=100, iters=5, seed=None, max_loss=1.01):
    """pool_opt_min.py as two library calls: one n x n table U{1..39}, then per iteration n customers (from, to uniform over
    the n stands, from == to removed), the greedy and the optimum of every iteration.  Returns (greedy_totals, optimal_totals,
    greedy_counts, optimal_counts, mean gap in % = mean of 100 * (greedy - opt) / opt over the iterations with equal counts,
    :124-125; nan when there is none).  Raises when an optimum has fewer pools than the greedy, or at equal counts a larger
    total (the solver failed).  Two quirks of the reference are not reproduced: its removal loop skips the element after a
    removed one (:38-43), and it carries the shrunken customer count into the next iteration (:45)."""
    rng = np.random.default_rng(seed)
    table = rng.integers(1, 40, (n, n)).astype(np.int32)
    froms, tos = [], []
    for _ in range(iters):
        d = rng.integers(0, n, (n, 2)).astype(np.int32)
        d = d[d[:, 0] != d[:, 1]]
        froms.append(np.ascontiguousarray(d[:, 0]))
        tos.append(np.ascontiguousarray(d[:, 1]))
    gk, gt = pool2_batched(froms, tos, table, max_loss, optimal=False)[4:]
    ok, ot = pool2_batched(froms, tos, table, max_loss, optimal=True)[4:]
    bad = np.nonzero((ok < gk) | ((ok == gk) & (ot > gt)))[0]
    if bad.size:
        i = int(bad[0])
        raise _ffi.TdError("optimal pooling worse than the greedy in %d iterations (first: %d: %d pools / %d against %d / %d)"
                           % (bad.size, i, int(ok[i]), int(ot[i]), int(gk[i]), int(gt[i])))
    eq = (ok == gk) & (ot > 0)
    gap = float(np.mean(100.0 * (gt[eq] - ot[eq]) / ot[eq])) if eq.any() else float("nan")
    return gt, ot, gk, ok, gap
