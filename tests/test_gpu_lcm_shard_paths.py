"""The row-sharded lowest-cost method (td_lcm_shard_*, the k_lcmsh_* kernels of csrc/td_lcm.hip) on the case table of
tests/lcm_shard_cases.py, all shards of a split driven in this process (no process group):
  * end to end: every case and split through the round driver of taxidispatcher_amd/sharded.py, and through the per-pick
    driver, held exactly to the case's host reference -- pairs in order, total, last_min -- and to td_lcm on the same matrix;
  * kernel by kernel: the round loop re-implemented here with a numpy shard model (tests/shard_model.py) beside every device
    shard; after every round_colmin and round_apply the device vector must equal the model's, element for element, per shard
    and before any reduction, and in a second pass local_min() must agree in all three words after every take.  A wrong
    kernel is named by the first vector that differs, not by a pair list that is wrong many rounds later.
test_lcm_shard_cases_cpu.py confirms the references, the claims of the cases and the model itself.  Run with -s to see each
case's figures and wall time."""
import time

import numpy as np
import pytest

import lcm_shard_cases as S
from shard_model import ModelLcmShard

pytestmark = pytest.mark.gpu

INT64_MAX = 2**63 - 1
PICK_SHARDS_MAX = 16      # the per-pick passes take a split of more shards than this (one row each) only up to n = PICK_ROWS_NMAX:
PICK_ROWS_NMAX = 65       # every pick costs one host round trip per shard


def _matrix(c):
    """the case's matrix: host numpy (the shards stage their rows), or, for the large sparse cases, built on the device (the
    shards read the rows in place)"""
    if c["input"] == "dense" or c["n"] <= S.LOCKSTEP_NMAX:
        return S.dense_matrix(c)
    import torch
    n = c["n"]
    m = torch.full((n, n), c["fill"], dtype=torch.int32, device="cuda")
    r, cc, v = (torch.tensor(a, device="cuda") for a in c["coords"])
    m[r.long(), cc.long()] = v   # unique coordinates (the CPU tier checks it): a deterministic write
    return m


def _open(c, split, m):
    """one HipLcmShard per (row0, nrows) of the split; the caller closes them"""
    from taxidispatcher_amd import sharded
    r = c["rule"]
    shards = []
    try:
        for row0, nrows in split:
            rows = m[row0:row0 + nrows]
            shards.append(sharded.HipLcmShard(c["n"], row0, nrows, np.ascontiguousarray(rows) if isinstance(rows, np.ndarray) else rows,
                                              r["stop_value_on"], r["stop_value"]))
    except BaseException:
        _close(shards)
        raise
    return shards


def _close(shards):
    for s in shards:
        s.close()


def _per_pick(c, split):
    return len(split) <= PICK_SHARDS_MAX or c["n"] <= PICK_ROWS_NMAX


def _end_to_end(td, c, ref, ref_capped, m):
    """both drivers on every split, td_lcm on the same matrix; prints the figures"""
    from taxidispatcher_amd import dispatch, sharded
    n, rule, name = c["n"], c["rule"], c["name"]
    rounds_claim = [cl[1] for cl in c["claims"] if cl[0] == "rounds"]
    t0 = time.perf_counter()
    for split in c["splits"]:
        shards = _open(c, split, m)
        try:
            got = sharded.lcm_sharded(shards, None, n, **rule)
            rounds = sharded.lcm_sharded.last_rounds
        finally:
            _close(shards)
        print(name, "n", n, "shards", len(split), "round driver: pairs", len(got[1]), "/", len(ref[1]), "total", got[0], "/", ref[0], "last_min",
              got[3], "/", ref[3], "rounds", rounds)
        assert len(got[1]) == len(ref[1]), (name, len(split))
        assert got == ref, (name, "rounds", len(split))
        if rounds_claim:   # a pure permutation band goes in ONE round; the stride model's second round is its re-scanned rows
            assert rounds == rounds_claim[0], (name, len(split), rounds)
        if not _per_pick(c, split):
            continue
        capped = n > S.BY_PICK_NMAX
        shards = _open(c, split, m)
        try:
            got = sharded.lcm_sharded(shards, None, n, by_pick=True, **(S.capped_rule(c, S.BY_PICK_CAP) if capped else rule))
        finally:
            _close(shards)
        want = ref_capped if capped else ref
        print(name, "n", n, "shards", len(split), "per pick%s: pairs" % (" (capped)" if capped else ""), len(got[1]), "/", len(want[1]), "total",
              got[0], "/", want[0], "last_min", got[3], "/", want[3])
        assert got == want, (name, "by pick", len(split))
    tot, rows, cols, lm = dispatch._lcm(n, m, *S.lcm_args(rule))
    assert (int(tot), rows.tolist(), cols.tolist(), int(lm)) == ref, (name, "td_lcm")
    print(name, "wall %.2f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("name", S.CASE_NAMES)
def test_end_to_end(td, name):
    c = S.case(name)
    capped = S.reference_capped(name, S.BY_PICK_CAP) if c["n"] > S.BY_PICK_NMAX else None
    _end_to_end(td, c, S.reference(name), capped, _matrix(c))


def test_end_to_end_grid_stride_rows(td):
    """k_lcmsh_init, k_lcmsh_rescan and k_lcmsh_rescan_masked launch min((nrows + 3) / 4, 8 n_cu) workgroups of four waves: the
    rows from 32 n_cu on are reached only by the grid stride.  The model of lcm_shard_cases.stride_case at THIS device's n_cu
    (n = 32 n_cu + 64, built on the device): every stride row must be scanned at the start and re-scanned after an earlier
    row's pick, in one shard over all rows and with a shard boundary eight rows into the stride rows."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = S.stride_case(n_cu)
    assert c["n"] == 32 * n_cu + 64 and c["n"] > S.BY_PICK_NMAX
    ref = S.stride_reference(c)
    capped = S._reference_of(c, S.capped_rule(c, S.BY_PICK_CAP))
    assert len(capped[1]) == S.BY_PICK_CAP >= 2 * S.STRIDE_TAIL     # the capped per-pick pass still takes every re-scanned stride row
    m = _matrix(c)
    try:
        _end_to_end(td, c, ref, capped, m)
    finally:
        del m
        torch.cuda.empty_cache()


# ======================================================================================================================
# kernel by kernel, in lockstep with the numpy model
# ======================================================================================================================
class _Vectors:
    """int64 vectors of length n in host memory (numpy) or device memory (torch), as the shard calls take them"""

    def __init__(self, mem, n):
        self.mem, self.n = mem, n
        if mem == "device":
            import torch
            self.torch = torch

    def empty(self):
        # filled with a value no kernel writes, so that a cell a kernel leaves out shows
        if self.mem == "host":
            return np.full(self.n, -7, np.int64)
        return self.torch.full((self.n,), -7, dtype=self.torch.int64, device="cuda")

    def put(self, a):
        return a.copy() if self.mem == "host" else self.torch.from_numpy(a).cuda()

    def get(self, v):
        return v.copy() if self.mem == "host" else v.cpu().numpy()


def _same(dev, mod, where):
    if not np.array_equal(dev, mod):
        k = int(np.flatnonzero(dev != mod)[0])
        raise AssertionError("%s: %d of %d elements differ, the first at column %d: device %d (%#x), model %d (%#x)" % (
            where, int((dev != mod).sum()), dev.size, k, int(dev[k]), int(dev[k]) & (2**64 - 1), int(mod[k]), int(mod[k]) & (2**64 - 1)))


def _limits(rule):
    """lcm_sharded's candidate limit and round limit"""
    cand_limit = int(rule["stop_value"]) if rule["stop_value_on"] else INT64_MAX
    limit = min(cand_limit, int(rule["mask"]))
    if rule["threshold"] >= 0:
        limit = min(limit, int(rule["threshold"]) + 1)
    return cand_limit, limit


def _lockstep_rounds(c, split, m, mem):
    """the round loop of lcm_sharded, every device vector compared with the model's; returns (rounds, picks {col: key})"""
    n, name = c["n"], c["name"]
    cand_limit, limit = _limits(c["rule"])
    r = c["rule"]
    models = [ModelLcmShard(n, row0, nrows, m[row0:row0 + nrows], r["stop_value_on"], r["stop_value"]) for row0, nrows in split]
    vec = _Vectors(mem, n)
    none_min, none_max = ModelLcmShard.NONE_MIN, ModelLcmShard.NONE_MAX
    shards = _open(c, split, m)
    try:
        def col_minima(lim, rnd):
            colmin = np.full(n, none_min, np.int64)
            for k, (sh, mo) in enumerate(zip(shards, models)):
                dv, mv = vec.empty(), np.empty(n, np.int64)
                sh.round_colmin(lim, dv)
                mo.round_colmin(lim, mv)
                _same(vec.get(dv), mv, "%s, %d shards, %s vectors, round %d, round_colmin of shard %d (rows %d..%d)" % (
                    name, len(split), mem, rnd, k, sh.row0, sh.row0 + sh.nrows - 1))
                colmin = np.minimum(colmin, mv)
            return colmin

        rounds, picks = 0, {}
        while True:
            colmin = col_minima(limit, rounds)
            taken = np.full(n, none_max, np.int64)
            cm_dev = vec.put(colmin)
            for k, (sh, mo) in enumerate(zip(shards, models)):
                dv, mv = vec.empty(), np.empty(n, np.int64)
                sh.round_apply(limit, cm_dev, dv)
                mo.round_apply(limit, colmin, mv)
                _same(vec.get(dv), mv, "%s, %d shards, %s vectors, round %d, round_apply of shard %d (rows %d..%d)" % (
                    name, len(split), mem, rounds, k, sh.row0, sh.row0 + sh.nrows - 1))
                taken = np.maximum(taken, mv)
            if not (taken != none_max).any():
                break
            rounds += 1
            tk_dev = vec.put(taken)
            for sh, mo in zip(shards, models):
                sh.round_commit(tk_dev)
                mo.round_commit(taken)
            for col in np.flatnonzero(taken != none_max):
                assert int(col) not in picks
                picks[int(col)] = int(taken[col])
            assert rounds <= n, name
        col_minima(cand_limit, rounds)     # the look the driver takes for last_min (and what round_commit's re-scan left behind)
    finally:
        _close(shards)
    return rounds, picks


def _lockstep_picks(c, split, m):
    """the per-pick loop of lcm_sharded: after every take, local_min() of every device shard == the model's, all three words"""
    n, name, rule = c["n"], c["name"], c["rule"]
    models = [ModelLcmShard(n, row0, nrows, m[row0:row0 + nrows], rule["stop_value_on"], rule["stop_value"]) for row0, nrows in split]
    iters = n if rule["max_pairs"] is None else min(n, rule["max_pairs"])
    size, taken = n, []
    shards = _open(c, split, m)
    try:
        for step in range(iters + 1):      # (one look more than picks: what the last take left behind)
            best = (INT64_MAX, -1, -1)
            for k, (sh, mo) in enumerate(zip(shards, models)):
                dv, mv = sh.local_min(), mo.local_min()
                assert dv == mv, "%s, %d shards, after %d takes, local_min of shard %d (rows %d..%d): device %r, model %r" % (
                    name, len(split), step, k, sh.row0, sh.row0 + sh.nrows - 1, dv, mv)
                best = min(best, mv)
            v, row, col = best
            if step == iters or v == INT64_MAX or (rule["threshold"] >= 0 and v > rule["threshold"]) or (
                    rule["stop_value_on"] and v >= rule["stop_value"]) or v >= rule["mask"]:
                break
            taken.append((row, col))
            size -= 1
            for sh, mo in zip(shards, models):
                sh.take(row, col)
                mo.take(row, col)
            if rule["stop_size"] >= 0 and size == rule["stop_size"]:
                break
    finally:
        _close(shards)
    return taken


LOCKSTEP_NAMES = tuple(name for name in S.CASE_NAMES if not name.startswith("kmin_"))


@pytest.mark.parametrize("mem", ["device", "host"])
@pytest.mark.parametrize("name", LOCKSTEP_NAMES)
def test_rounds_kernel_by_kernel(td, name, mem):
    """round_colmin (k_lcmsh_colmin), round_apply (k_lcmsh_fill64, k_lcmsh_apply) and round_commit (k_lcmsh_commit,
    k_lcmsh_rescan_masked, seen through the next round's vectors) against the numpy model, the vectors in device or in host
    memory.  The picks of all rounds are the reference's pairs wherever the rule takes all it can reach."""
    c = S.case(name)
    assert c["n"] <= S.LOCKSTEP_NMAX
    m = S.dense_matrix(c)
    ref = S.reference(name)
    rule = c["rule"]
    t0 = time.perf_counter()
    for split in c["splits"]:
        rounds, picks = _lockstep_rounds(c, split, m, mem)
        got = sorted(((key >> 32), (key & 0xFFFFFFFF) - S.KEY_ROW_BIAS, col) for col, key in picks.items())
        print(name, "n", c["n"], "shards", len(split), mem, "vectors: rounds", rounds, "picks", len(got), "reference pairs", len(ref[1]))
        assert all(int(m[row, col]) == v for v, row, col in got), name
        # the stop rules that cut the sorted picks short are the host's; up to there the picks are the reference's, in order
        assert [(row, col) for _, row, col in got][:len(ref[1])] == list(zip(ref[1], ref[2])), (name, len(split))
        if rule["max_pairs"] is None and rule["stop_size"] < 0:
            assert len(got) == len(ref[1]), (name, len(split))
    print(name, mem, "wall %.2f s" % (time.perf_counter() - t0))


@pytest.mark.parametrize("name", LOCKSTEP_NAMES)
def test_picks_kernel_by_kernel(td, name):
    """local_min (k_lcmsh_min) after every take (k_lcmsh_mark, k_lcmsh_rescan) against the numpy model, per shard"""
    c = S.case(name)
    m = S.dense_matrix(c)
    ref = S.reference(name)
    t0 = time.perf_counter()
    for split in c["splits"]:
        if not _per_pick(c, split):
            continue
        taken = _lockstep_picks(c, split, m)
        assert taken == list(zip(ref[1], ref[2])), (name, len(split))
    print(name, "n", c["n"], "picks", len(ref[1]), "wall %.2f s" % (time.perf_counter() - t0))


def test_lockstep_covers_the_table():
    """every case up to LOCKSTEP_NMAX runs kernel by kernel; the k_lcmsh_min cases (n >= 1023) run end to end only"""
    for name in S.CASE_NAMES:
        assert (name in LOCKSTEP_NAMES) == (S.case(name)["n"] <= S.LOCKSTEP_NMAX), name
