"""td_pool_n_banded restated on the host: the happy plans of pool_n.c enumerated in numpy, their keys, and the
band loop over them: count by cost, cut at the first digit that fits, scan the band with the used requests carried along.
The CPU tests check it against oracle.pool_n; the GPU tests compare td_pool_n_banded's records AND its stats with it."""
import bisect
import itertools

import numpy as np

SEQ_BITS = 50
END = (1 << 64) - 1
DEFAULT_BUFFER = 1 << 22


def random_demand(rng, n, max_wait, losses, stands=50):
    """tests/test_gpu_pool.py's generator, draw for draw"""
    frm = rng.integers(0, stands, n)
    to = np.clip(frm + rng.integers(1, 9, n) * rng.choice([-1, 1], n), 0, stands - 1)
    to = np.where(to == frm, np.where(frm > 0, frm - 1, 1), to)
    return np.stack([np.arange(n), frm, to, rng.integers(0, max_wait + 1, n), rng.choice(losses, n)], 1)


def same_stand(n=12, stand=3):
    """n requests from a stand to itself, wait 0, loss 0: every plan is happy at cost 0"""
    z = np.zeros(n, np.int64)
    return np.stack([np.arange(n), z + stand, z + stand, z, z], 1)


def inputs():
    """the named inputs of the band tests: name -> (demand rows, distance table or None)"""
    rng = np.random.default_rng(7)
    out = {"same12": (same_stand(), None)}
    for name, (n, mw, losses, stands) in (("r24", (24, 9, [90], 6)), ("r40", (40, 6, [30, 90], 10)), ("r64", (64, 4, [50], 12))):
        out[name] = (random_demand(rng, n, mw, losses, stands), None)
    return out


def table_case(k):
    """the asymmetric 30-stand table case of test_gpu_pool.py::test_pool_n_random_vs_oracle[k], with the generator in the state
    that test leaves it in"""
    rng = np.random.default_rng(40 + k)
    for n, mw, losses in ((4, 9, [90]), (17, 5, [10, 50]), (150, 3, [1, 30]), (600, 1 if k == 4 else 2, [1, 5, 20])):
        if n < k:
            continue
        random_demand(rng, n, mw if k < 4 or n < 600 else 0, losses)
    S = 30
    dist = rng.integers(0, 12, (S, S)).astype(np.int32)
    np.fill_diagonal(dist, 0)
    return random_demand(rng, 80, 6, [20, 60], stands=S), dist


def _d(dist, a, b):
    return np.abs(a - b) if dist is None else dist[a, b].astype(np.int64)


def happy_plans(k, d, dist=None, first0=0, first1=None):
    """pool_n.c's happy plans of the first-pick-up slice in KEY order -> (cost, p [m, 4] with 0 behind the pool's size, qi), all
    int64.  The pick-up sequences grow one member at a time under the wait rule, then every drop-off order is tested with the
    reference's arithmetic (double, 1 + loss / 100.0)."""
    d = np.asarray(d, np.int64)
    n = d.shape[0]
    frm, to, wait, loss = (d[:, c] for c in (1, 2, 3, 4))
    first1 = n if first1 is None else min(first1, n)
    first0 = max(first0, 0)
    dist = None if dist is None else np.asarray(dist, np.int64)
    p0 = np.arange(first0, max(first0, first1))
    p0 = p0[wait[p0] >= 0]
    seqs, path = p0[:, None], np.zeros(p0.size, np.int64)
    for _ in range(1, k):
        cand = np.repeat(seqs, n, axis=0)
        nxt = np.tile(np.arange(n), seqs.shape[0])
        length = np.repeat(path, n) + _d(dist, frm[cand[:, -1]], frm[nxt])
        ok = (length <= wait[nxt]) & (cand != nxt[:, None]).all(axis=1)
        seqs, path = np.concatenate([cand[ok], nxt[ok, None]], axis=1), length[ok]
    m = seqs.shape[0]
    pick = [_d(dist, frm[seqs[:, i]], frm[seqs[:, i + 1]]) for i in range(k - 1)]
    direct = _d(dist, frm, to).astype(np.float64) * (1 + loss / 100.0)
    costs, ps, qis = [], [], []
    for qi, q in enumerate(itertools.permutations(range(k))):      # lexicographic: pn_perm's order
        first = _d(dist, frm[seqs[:, k - 1]], to[seqs[:, q[0]]])
        drop = np.zeros(m, np.int64)
        happy = np.ones(m, bool)
        for j in range(k):
            if j > 0:
                drop = drop + _d(dist, to[seqs[:, q[j - 1]]], to[seqs[:, q[j]]])
            c = first + drop
            for ph in range(q[j], k - 1):
                c = c + pick[ph]
            happy &= ~(c.astype(np.float64) > direct[seqs[:, q[j]]])
        cost = sum(pick) + first + drop
        costs.append(cost[happy]), ps.append(seqs[happy]), qis.append(np.full(int(happy.sum()), qi, np.int64))
    cost, p, qi = np.concatenate(costs), np.concatenate(ps), np.concatenate(qis)
    p = np.concatenate([p, np.zeros((p.shape[0], 4 - k), np.int64)], axis=1)
    order = np.lexsort((qi, p[:, 3], p[:, 2], p[:, 1], p[:, 0], cost))
    return cost[order], p[order], qi[order]


def keys_of(n, cost, p, qi):
    """td_pool_core.h's key as Python ints"""
    out = []
    for c, row, q in zip(cost.tolist(), p.tolist(), qi.tolist()):
        out.append((c << SEQ_BITS) | ((((row[0] * n + row[1]) * n + row[2]) * n + row[3]) * 24 + q))
    return out


def scan_all(k, cost, p, qi):
    """the reference's sequential de-duplication over the whole list -> records"""
    used, recs = set(), []
    perms = list(itertools.permutations(range(k)))
    for c, row, q in zip(cost.tolist(), p.tolist(), qi.tolist()):
        mem = row[:k]
        if any(x in used for x in mem):
            continue
        used.update(mem)
        recs.append(mem + [mem[j] for j in perms[q]] + [c])
    return recs


CHUNK = 1024      # k_band_greedy: keys per chunk


def banded(k, n, cost, p, qi, plan_buffer=0, max_pools=None, trace=None):
    """the host loop of td_pool_n_banded on the plan list -> (records, n_happy, (bands, passes, deepest level, most keys)).
    trace: a list that gets one dict per band: lo, hi, level (the digit it was cut at), expect (its keys), first_bins (the size
    of the first non-empty bin at each level it passed through), prefix (the key of the digits fixed above the cut), kept (the
    positions of the kept plans among the band's keys in ascending order), kills_later (per kept plan: a key of a LATER chunk
    of 1024 of the same band shares a request with it, so k_band_greedy must carry the bitmap from chunk to chunk), rows
    (the band's keys as indices into the plan list)."""
    room = DEFAULT_BUFFER if plan_buffer <= 0 else int(plan_buffer)
    assert room >= 24 * n
    perms = list(itertools.permutations(range(k)))
    max_pools = n // k if max_pools is None else min(max_pools, n // k)
    key = keys_of(n, cost, p, qi)      # ascending
    digits = [cost, p[:, 0], p[:, 1], p[:, 2], p[:, 3]]
    weight = [1 << SEQ_BITS, n ** 3 * 24, n ** 2 * 24, n * 24, 24]
    used = np.zeros(max(n, 1), bool)
    recs, lo = [], 0
    bands = passes = deepest = most = 0
    m = cost.size
    pos = np.arange(m)
    above = np.ones(m, bool)      # key >= lo: the list is sorted, so a position
    while True:
        live = above & ~used[p[:, :k]].any(axis=1) if m else np.zeros(0, bool)
        passes += 1
        if not live.any() or n - int(used.sum()) < k or len(recs) >= max_pools:
            break
        level, prefix, sel, bins = 0, 0, live, 1 << 14
        first_bins = []
        while True:
            vals = digits[level][sel]
            hist = np.bincount(vals, minlength=bins)
            b0 = int(vals.min())
            first_bins.append(int(hist[b0]))
            if hist[b0] <= room:
                expect, b1 = 0, b0
                while b1 < bins and expect + int(hist[b1]) <= room:
                    expect += int(hist[b1])
                    b1 += 1
                if level == 0:      # a run to the last bin ends above every key
                    hi = END if b1 == bins else b1 << SEQ_BITS
                else:
                    hi = prefix + b1 * weight[level]
                break
            assert level < k - 1, "one value of the last digit but one holds more than 24 n plans"
            prefix += b0 * weight[level]
            sel = sel & (digits[level] == b0)
            level += 1
            bins = n
            passes += 1
        deepest = max(deepest, level)
        band = np.nonzero(live & (pos < bisect.bisect_left(key, hi)))[0]
        assert len(band) == expect, (len(band), expect)
        passes += 1
        most = max(most, expect)
        kept_at = []
        for at, i in enumerate(band.tolist()):
            if n - int(used.sum()) < k or len(recs) >= max_pools:
                break
            mem = p[i, :k].tolist()
            if used[mem].any():
                continue
            used[mem] = True
            kept_at.append(at)
            recs.append(mem + [mem[j] for j in perms[int(qi[i])]] + [int(cost[i])])
        bands += 1
        if trace is not None:
            kills = []
            for at in kept_at:
                later = band[(at // CHUNK + 1) * CHUNK:]
                kills.append(bool(np.isin(p[later, :k], p[band[at], :k]).any()))
            trace.append(dict(lo=lo, hi=hi, level=level, expect=expect, first_bins=first_bins, prefix=prefix, kept=kept_at,
                              kills_later=kills, rows=band))
        if hi == END:      # nothing lies above: no further count
            break
        lo = hi
        above = pos >= bisect.bisect_left(key, lo)
    return recs, int(m), (bands, passes, deepest, most)
