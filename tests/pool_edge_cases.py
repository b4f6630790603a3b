"""The case generators of tests/test_pool_edges_cpu.py and tests/test_gpu_pool_edges.py: td_pool_n instances and td_pool_merge
record lists that sit on the rules and constants of csrc/td_pool.hip -- the double-precision happiness rule at equality, the
wait rule at equality, the 256-thread grid edge, the top of the 64-bit plan key, the 14-bit cost limit, and the 1024-plan
chunks of the greedy de-duplication.  Plain numpy data plus host comparators: nothing here needs a GPU.

Every generator asserts on the CPU that its cases reach the condition they are named for (with the oracle and the pure
Python restatements below), so a later edit cannot quietly empty a test.  Generators are computed once per process and
shared (treat what they return as read-only); reference(case) is the oracle's answer, cached the same way.

Comparators:  td_pool_n -> oracle.pool_n (C, IEEE double, the restatement of pool_n.c);  the happiness sweep additionally
-> py_happy_count with happy_rule (Python floats are IEEE doubles);  td_pool_merge -> merge_scan (a sequential scan)."""
import collections
import functools
import itertools

import numpy as np

from oracle import oracle

PN_MAXN = 2047        # td_pool.hip PN_MAXN: 4 * 11 bits of pick-ups + 5 bits of drop-off order in the 50-bit sequence number
PN_MAXCOST = 16383    # td_pool.hip PN_MAXCOST: 14 bits of cost above the sequence number
CHUNK = 1024          # k_pooln_greedy: plans per chunk (one workgroup of 1024 threads)
ENUM_BLOCK = 256      # k_pooln_enum / k_pooln_enum4: threads per workgroup along the second / third pick-up
HAPPY_MIN, HAPPY_MAX = CHUNK + 1, 200000   # a multi-chunk greedy; the oracle's default plan capacity
HUGE_LOSS = 1000000   # percent: a passenger with a positive direct ride who accepts every plan of these instances

# (direct, loss) with direct * (100 + loss) / 100 an integer T while the double product falls just below T: a ride of
# exactly T is unhappy in the reference and happy in exact arithmetic
KNOWN_MISROUNDED = {(25, 16): 29, (45, 40): 63, (50, 16): 58, (50, 82): 91}

PoolCase = collections.namedtuple("PoolCase", "name k frm to wait loss dist first0 first1 info")
MergeCase = collections.namedtuple("MergeCase", "name k n_requests recs sort_by_cost max_pools claim")


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _case(name, k, frm, to, wait, loss, dist=None, first=None, **info):
    frm, to, wait, loss = map(_i32, (frm, to, wait, loss))
    n = int(frm.size)
    assert to.size == wait.size == loss.size == n
    f0, f1 = (0, n) if first is None else first
    return PoolCase(name, k, frm, to, wait, loss, None if dist is None else _i32(dist), f0, f1, info)


_REF = {}


def reference(case, cap=HAPPY_MAX):
    """the oracle's (records as lists, n_happy) of a case, computed once"""
    key = (case.name, case.k)
    if key not in _REF:
        recs, nh = oracle.pool_n(case.k, case.frm, case.to, case.wait, case.loss, case.dist, case.first0, case.first1, cap=cap)
        _REF[key] = (recs.tolist(), nh)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------
# pure Python restatements (tiny instances only)
# ------------------------------------------------------------------------------------------------------------------
def happy_rule(c, direct, loss):
    """pool_n.c:118-119: a ride of length c is refused iff  c > direct * (1 + loss / 100.0)  in double arithmetic.
    Python floats are IEEE doubles and int * float converts the int first, as C does."""
    return not (float(c) > direct * (1 + loss / 100.0))


def happy_rule_exact(c, direct, loss):
    """the same rule in exact integer arithmetic: what a kernel would compute that is NOT the reference's rule"""
    return not (c * 100 > direct * (100 + loss))


def py_plans(case):
    """every plan of a tiny instance that passes the wait rule, in the reference's enumeration order:
    (pick-ups p, drop-off order q, [(passenger, ride length)] in drop-off order, cost)"""
    k, n = case.k, int(case.frm.size)
    f, t, w = case.frm.tolist(), case.to.tolist(), case.wait.tolist()
    if case.dist is None:
        def D(a, b):
            return abs(a - b)
    else:
        tab = case.dist.tolist()

        def D(a, b):
            return tab[a][b]
    perms = list(itertools.permutations(range(k)))
    for p in itertools.permutations(range(n), k):
        if not case.first0 <= p[0] < case.first1 or 0 > w[p[0]]:
            continue
        legs = [D(f[p[l - 1]], f[p[l]]) for l in range(1, k)]
        if any(sum(legs[:l]) > w[p[l]] for l in range(1, k)):
            continue
        for q in perms:
            ride = D(f[p[-1]], t[p[q[0]]])
            rides = []
            for d in range(k):
                if d:
                    ride += D(t[p[q[d - 1]]], t[p[q[d]]])
                rides.append((p[q[d]], sum(legs[q[d]:]) + ride))
            yield p, q, rides, sum(legs) + ride


def py_happy_count(case, rule=happy_rule):
    """the number of happy plans of a tiny instance under `rule`"""
    f, t, loss = case.frm.tolist(), case.to.tolist(), case.loss.tolist()
    direct = [abs(a - b) if case.dist is None else int(case.dist[a, b]) for a, b in zip(f, t)]
    return sum(all(rule(c, direct[x], loss[x]) for x, c in rides) for _, _, rides, _ in py_plans(case))


def rides_of(case, x):
    """the ride lengths passenger x meets in plans whose other passengers are all happy: the plans x alone decides"""
    f, t, loss = case.frm.tolist(), case.to.tolist(), case.loss.tolist()
    direct = [abs(a - b) if case.dist is None else int(case.dist[a, b]) for a, b in zip(f, t)]
    out = set()
    for _, _, rides, _ in py_plans(case):
        if all(happy_rule(c, direct[y], loss[y]) for y, c in rides if y != x):
            out.update(c for y, c in rides if y == x)
    return out


# ------------------------------------------------------------------------------------------------------------------
# happy_ties: the happiness rule at, one above and one below  direct * (100 + loss) / 100
# ------------------------------------------------------------------------------------------------------------------
def integer_pairs(max_direct, max_loss):
    return [(d, l) for d in range(1, max_direct + 1) for l in range(max_loss + 1) if d * l % 100 == 0]


def _tie_table(k, d, l):
    """Four requests on a general table; request 0 (X: direct d, loss l) is always the first pick-up (waits are 0 and only
    the legs INTO its pick-up stand cost something), the others accept everything.  X's ride is T when Y is dropped
    first, T + 1 when Z is, T - 1 when W is (W's direct ride is 0: it is happy only as the first drop-off)."""
    T = d * (100 + l) // 100
    P, DX, DY, DZ, DW = (0, 1, 2, 3), 4, 5, 6, 7
    dist = np.ones((8, 8), np.int32)
    np.fill_diagonal(dist, 0)
    for i in P:
        for j in P:
            dist[i, j] = 0 if (j != 0 or i == j) else 5
        dist[i, DX], dist[i, DY], dist[i, DZ], dist[i, DW] = d, 1, 1, 0
    dist[DY, DX], dist[DZ, DX], dist[DW, DX] = T - 1, T, T - 1
    return _case("tie_table_d%d_l%d" % (d, l), k, P, (DX, DY, DZ, DW), (0, 0, 0, 0), (l, HUGE_LOSS, HUGE_LOSS, HUGE_LOSS), dist,
                 direct=d, loss_x=l, T=T, want=(T - 1, T, T + 1))


def _tie_line(k, d, l):
    """The same on the line |a - b|: X rides from B to B + d, the others board one stand further (X's wait 0 keeps it first)
    and leave h stands before it, so X rides d + 2h.  Every walk from B to B + d has the parity of d: the line reaches T
    itself when the allowed excess T - d is even, and T - 1 and T + 1 when it is odd."""
    T = d * (100 + l) // 100
    e, B = T - d, 50
    hs = (e // 2, e // 2 + 1, max(e // 2 - 1, 0))
    want = (T,) if e % 2 == 0 else (T - 1, T + 1)
    return _case("tie_line_d%d_l%d" % (d, l), k, (B, B + 1, B + 1, B + 1), (B + d,) + tuple(B + 1 - h for h in hs), (0, 1, 1, 1),
                 (l, HUGE_LOSS, HUGE_LOSS, HUGE_LOSS), None, direct=d, loss_x=l, T=T, want=want)


def misrounded_pairs(max_direct, max_loss):
    """the integer-product pairs at which the double rule refuses a ride of exactly T"""
    return [(d, l) for d, l in integer_pairs(max_direct, max_loss) if not happy_rule(d * (100 + l) // 100, d, l)]


@functools.lru_cache(maxsize=None)
def happy_ties(k):
    """-> list of PoolCase.  The sweep: every (direct <= 60, loss <= 100) pair with an integer product, on the table and on
    the line; then table cases up to direct 400 / loss 300: every pair there the double rule misrounds, and as many more
    that it does not (the largest directs first)."""
    small = integer_pairs(60, 100)
    cases = [mk(k, d, l) for d, l in small for mk in (_tie_table, _tie_line)]
    big_bad = [p for p in misrounded_pairs(400, 300) if p not in set(small)]
    big_bad = big_bad[::max(1, len(big_bad) // 120)]          # at most about 120 of them, spread over the whole range
    big_ok = [p for p in integer_pairs(400, 300)[::-1] if p[0] > 60 and happy_rule(p[0] * (100 + p[1]) // 100, *p)]
    big_ok = big_ok[::max(1, len(big_ok) // max(1, len(big_bad)))][:len(big_bad)]
    cases += [_tie_table(k, d, l) for d, l in big_bad + big_ok]
    # ---- CPU conditions
    assert any(d > 300 for d, _ in big_bad + big_ok) and any(l > 200 for _, l in big_bad + big_ok)
    differ = agree = 0
    seen = set()
    for c in cases:
        i = c.info
        got = rides_of(c, 0)
        assert set(i["want"]) <= got, (c.name, i["want"], sorted(got))
        if i["T"] in got:
            seen.add((i["direct"], i["loss_x"]))
            if happy_rule(i["T"], i["direct"], i["loss_x"]):
                agree += 1
            else:
                assert happy_rule_exact(i["T"], i["direct"], i["loss_x"])
                differ += 1
    for (d, l), T in KNOWN_MISROUNDED.items():
        assert (d, l) in seen and d * (100 + l) == 100 * T
        assert not happy_rule(T, d, l) and happy_rule_exact(T, d, l) and happy_rule(T - 1, d, l)
    assert differ >= len(KNOWN_MISROUNDED) and agree >= differ, (differ, agree)
    return cases


# ------------------------------------------------------------------------------------------------------------------
# wait_edges: the wait rule at equality, at WAIT = 0 on one stand, with a negative WAIT
# ------------------------------------------------------------------------------------------------------------------
def _line_table(S=64):
    a = np.arange(S)
    return np.abs(a[:, None] - a[None, :]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def wait_edges(k):
    """-> list of PoolCase; info["pair"] names the variant a case is compared with by the CPU condition"""
    B, cum = 10, (0, 3, 7, 12)[:k]
    cases = []
    for level in range(1, k):
        for tab in (False, True):
            for longer in (False, True):
                # requests 0..k-1 stand at B + cum with WAIT == the path to them in index order; two bystanders with a long WAIT
                frm = [B + c for c in cum] + [B + 1, B + 30]
                wait = list(cum) + [100, 100]
                wait[level] -= 1 if longer else 0
                name = "wait_l%d_%s_%s" % (level, "table" if tab else "line", "longer" if longer else "equal")
                cases.append(_case(name, k, frm, [f + 4 for f in frm], wait, [1000] * (k + 2), _line_table() if tab else None,
                                   pair=name.replace("longer", "equal"), relation="fewer" if longer else None))
    n = k + 2
    to = [21 + i for i in range(n)]
    loss = [0, 50, 100, 200, 400, 1000][:n]
    cases.append(_case("wait0_one_stand", k, [20] * n, to, [0] * n, loss, pair=None, relation=None))
    neg = [0] * n
    neg[1] = -1
    cases.append(_case("wait_negative", k, [20] * n, to, neg, loss, pair="wait0_one_stand", relation="fewer", absent=1))
    keep = [i for i in range(n) if i != 1]
    cases.append(_case("wait_negative_removed", k, [20] * (n - 1), [to[i] for i in keep], [0] * (n - 1), [loss[i] for i in keep],
                       pair="wait_negative", relation="same"))
    # ---- CPU conditions
    by_name = {c.name: c for c in cases}
    for c in cases:
        recs, nh = reference(c)
        assert nh == py_happy_count(c), c.name
        if c.info["pair"]:
            other = reference(by_name[c.info["pair"]])[1]
            assert (nh < other) if c.info["relation"] == "fewer" else (nh == other), (c.name, nh, other)
        if "absent" in c.info:   # first pick-up in one candidate plan, later pick-up in another: refused in both
            assert nh > 0 and all(c.info["absent"] not in r[:k] for r in recs)
    assert reference(by_name["wait0_one_stand"])[1] > 0
    return cases


# ------------------------------------------------------------------------------------------------------------------
# grid_edges: one request below, at and above the 256-thread workgroup edge
# ------------------------------------------------------------------------------------------------------------------
GRID_WAIT = {2: 3, 3: 2, 4: 1}    # largest WAIT of the random part: keeps the happy plans inside HAPPY_MIN .. HAPPY_MAX


def _random_demand(rng, n, max_wait, losses, stands=50):
    frm = rng.integers(0, stands, n)
    to = np.clip(frm + rng.integers(1, 9, n) * rng.choice([-1, 1], n), 0, stands - 1)
    to = np.where(to == frm, np.where(frm > 0, frm - 1, 1), to)
    return frm, to, rng.integers(0, max_wait + 1, n), rng.choice(losses, n)


@functools.lru_cache(maxsize=None)
def grid_edges(k):
    """-> list of PoolCase: n = 255, 256, 257 (random requests on stands 0..49; the last 2k requests ride together from
    stand 60 to stand 62, apart from everybody else, so that the highest request numbers end up in kept pools), n = k and
    n = k - 1"""
    cases = []
    for n in (ENUM_BLOCK - 1, ENUM_BLOCK, ENUM_BLOCK + 1):
        frm, to, wait, loss = _random_demand(np.random.default_rng(100 * k + n), n, GRID_WAIT[k], [10, 50])
        frm[-2 * k:], to[-2 * k:], wait[-2 * k:], loss[-2 * k:] = 60, 62, 0, 100
        cases.append(_case("grid_n%d" % n, k, frm, to, wait, loss, multi_chunk=True, top=[r for r in (254, 255, 256) if r < n]))
    frm, to, wait, loss = np.full(k, 5), 6 + np.arange(k), np.zeros(k, int), np.full(k, 400)   # one stand: every order passes
    cases.append(_case("grid_n_eq_k", k, frm, to, wait, loss, multi_chunk=False, top=[]))
    cases.append(_case("grid_n_below_k", k, frm[:-1], to[:-1], wait[:-1], loss[:-1], multi_chunk=False, top=[], empty=True))
    # ---- CPU conditions
    for c in cases:
        recs, nh = reference(c)
        if c.info["multi_chunk"]:
            assert HAPPY_MIN <= nh <= HAPPY_MAX, (c.name, nh)
            kept = {x for r in recs for x in r[:k]}
            assert set(c.info["top"]) <= kept and c.info["top"], (c.name, sorted(kept)[-8:])
        elif c.info.get("empty"):
            assert nh == 0 and recs == []
        else:
            assert nh >= 1 and len(recs) == 1 and sorted(recs[0][:k]) == list(range(k)), (c.name, nh, recs)
    return cases


# ------------------------------------------------------------------------------------------------------------------
# top_of_key: n = PN_MAXN, the last first-pick-up slice, every base-n digit of the sequence number near its top
# ------------------------------------------------------------------------------------------------------------------
TOP_CLUSTER = {2: 100, 3: 12, 4: 12}   # poolable requests (k = 2 needs about a hundred for more than 1024 happy plans)


@functools.lru_cache(maxsize=None)
def top_of_key(k):
    """-> one PoolCase with n = 2047 and first pick-ups [2040, 2047).  Fillers stand on stands 0..49 with WAIT 0 and the
    cluster on stand 100, so no filler can follow a cluster member (the path to it would be at least 51)."""
    n = PN_MAXN
    rng = np.random.default_rng(2047 + k)
    frm, to, wait, loss = _random_demand(rng, n, 0, [10, 50])
    must = [0, 1, 1023, 1024] + list(range(2040, 2047))
    rest = [i for i in rng.permutation(n).tolist() if i not in set(must)]
    cluster = sorted(must + rest[:TOP_CLUSTER[k] - len(must)])
    for i in cluster:
        frm[i], wait[i], loss[i] = 100, 0, 100
        to[i] = 103 + i % 3
    # the cheapest rides: 2040.. together (pick-ups all >= 2040), then the next slice members with requests 0 and 1
    for i in range(2040, 2040 + k):
        to[i] = 101
    for i in [2040 + k, 0, 1, 2041 + k][:k]:
        to[i] = 102
    c = _case("top_of_key", k, frm, to, wait, loss, first=(2040, 2047), cluster=cluster)
    # ---- CPU conditions
    recs, nh = reference(c)
    assert HAPPY_MIN <= nh <= HAPPY_MAX, nh
    assert all(set(r[:k]) <= set(cluster) for r in recs)
    assert any(min(r[:k]) >= 2040 for r in recs), recs
    assert any(0 in r[:k] for r in recs), recs
    return [c]


# ------------------------------------------------------------------------------------------------------------------
# cost_limit: the 14 bits of cost in the plan key
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cost_limit():
    """-> (fits, too_large): k = 2 on a general table with exactly two happy plans, a cheap one (C, D) and one (A, B) of cost
    16383 / 16384.  Every other leg of the table is far longer than any WAIT."""
    out = []
    for last in (6383, 6384):
        dist = np.full((8, 8), 1000000, np.int32)
        np.fill_diagonal(dist, 0)
        dist[0, 1] = dist[2, 3] = 20000                       # direct rides of A: 0 -> 1 and B: 2 -> 3
        dist[0, 2], dist[2, 1], dist[1, 3] = 5000, 5000, last  # pick up A, pick up B, drop A, drop B
        dist[4, 5] = dist[6, 7] = 100                         # C: 4 -> 5, D: 6 -> 7
        dist[4, 6], dist[6, 5], dist[5, 7] = 10, 20, 30
        c = _case("cost_%d" % (10000 + last), 2, (0, 2, 4, 6), (1, 3, 5, 7), (0, 5000, 0, 10), (0, 0, 0, 0), dist, cost=10000 + last)
        recs, nh = reference(c)
        assert nh == 2 == py_happy_count(c) and recs == [[2, 3, 2, 3, 60], [0, 1, 0, 1, 10000 + last]], (recs, nh)
        out.append(c)
    assert out[0].info["cost"] == PN_MAXCOST and out[1].info["cost"] == PN_MAXCOST + 1
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# td_pool_merge: the sequential scan and crafted record lists
# ------------------------------------------------------------------------------------------------------------------
def merge_scan(k, recs, sort_by_cost, max_pools):
    """The comparator of td_pool_merge: optional stable sort by the last field, keep a record iff none of its first k
    fields was used by an earlier kept record, truncate to max_pools.  -> (kept records as lists, their positions in the
    sorted order)"""
    recs = np.asarray(recs, np.int64).reshape(-1, 2 * k + 1)
    order = np.argsort(recs[:, 2 * k], kind="stable") if sort_by_cost else np.arange(recs.shape[0])
    used, kept, pos = set(), [], []
    for rank, i in enumerate(order.tolist()):
        c = recs[i, :k].tolist()
        if any(x in used for x in c):
            continue
        used.update(c)
        kept.append(recs[i].tolist())
        pos.append(rank)
    return kept[:max(max_pools, 0)], pos[:max(max_pools, 0)]


MERGE_SIZES = (1023, 1024, 1025, 2048, 2049, 3073)


def _records(k, reqs, costs):
    reqs = np.asarray(reqs, np.int64).reshape(-1, k)
    drops = reqs[:, ::-1]                                     # any permutation of the pick-ups: the merge only copies it
    return _i32(np.concatenate([reqs, drops, np.asarray(costs, np.int64).reshape(-1, 1)], 1))


def _subsets(rng, n_in, k, n_requests):
    return np.stack([rng.choice(n_requests, k, replace=False) for _ in range(n_in)])


DENSE_REQUESTS, DENSE_TAIL = 64, 32


def _dense(k, rng, n_in, sort_by_cost, hold_back):
    """Random k-subsets of 64 requests (of the first 64 - k, so that at least one block is left to share out); the last 32 places of the first chunk OF THE SORTED ORDER then get records that
    share out, k at a time, the requests the scan has left free before them (each takes over the cost of the record it
    replaces, so the order stands): after the first chunk fewer than k requests are free.  hold_back: the last of those
    records goes to the very end of the list instead, so exactly k requests are free after the first chunk and the one
    record that can still use them sits in the last chunk."""
    recs = _records(k, _subsets(rng, n_in, k, DENSE_REQUESTS - k), rng.integers(0, 8, n_in))
    order = np.argsort(recs[:, 2 * k], kind="stable") if sort_by_cost else np.arange(n_in)
    head = min(n_in, CHUNK) - DENSE_TAIL
    used = {x for r in merge_scan(k, recs[order[:head]], 0, n_in)[0] for x in r[:k]}
    free = [x for x in rng.permutation(DENSE_REQUESTS).tolist() if x not in used]
    blocks = [free[i:i + k] for i in range(0, len(free) - k + 1, k)]
    assert 1 <= len(blocks) <= DENSE_TAIL
    places = order[head:head + len(blocks)].tolist()
    if hold_back:
        places[-1] = int(order[-1])
        assert n_in > CHUNK
    for place, block in zip(places, blocks):
        recs[place, :k], recs[place, k:2 * k] = block, block[::-1]
    return recs


@functools.lru_cache(maxsize=None)
def merge_cases(k):
    """-> list of MergeCase.  claim: "chunks" (kept records in at least two 1024-chunks of the sorted order), "first chunk"
    (n_in > 1024, every kept record in the first chunk and fewer than k requests left), "some" (a non-empty result)."""
    rng = np.random.default_rng(500 + k)
    cases = []

    def add(name, n_requests, recs, sort_by_cost, claim, max_pools=None):
        cases.append(MergeCase(name, k, n_requests, recs, sort_by_cost, n_requests // k + 1 if max_pools is None else max_pools, claim))

    for n_in in MERGE_SIZES:
        # one record behind a chunk edge may or may not be kept; from a full second chunk on the claim is "chunks"
        claim = "chunks" if n_in >= 2 * CHUNK else "some"
        chain = _records(k, (np.arange(n_in)[:, None] + np.arange(k)[None, :]) % PN_MAXN, rng.integers(0, 8, n_in))
        sparse = _records(k, _subsets(rng, n_in, k, PN_MAXN), rng.integers(0, 8, n_in))
        for s in (0, 1):
            add("chain_%d_s%d" % (n_in, s), PN_MAXN, chain, s, claim)
            dense = _dense(k, rng, n_in, s, False)
            add("dense_%d_s%d" % (n_in, s), DENSE_REQUESTS, dense, s, "first chunk" if n_in > CHUNK else "some")
            if n_in > CHUNK:   # exactly k requests left after the first chunk: the last record must still be kept
                add("dense_k_left_%d_s%d" % (n_in, s), DENSE_REQUESTS, _dense(k, rng, n_in, s, True), s, "chunks")
            add("sparse_%d_s%d" % (n_in, s), PN_MAXN, sparse, s, claim)
        if n_in == 2049:
            add("dense_wide_%d" % n_in, PN_MAXN, dense, 1, "some")      # the same records: no early break by request count
            add("equal_costs_%d" % n_in, PN_MAXN, _records(k, sparse[:, :k], np.full(n_in, 7)), 1, claim)
            add("descending_%d" % n_in, PN_MAXN, _records(k, sparse[:, :k], n_in - np.arange(n_in)), 1, claim)
            for nm, recs in (("chain", chain), ("sparse", sparse)):
                for s in (0, 1):
                    first = sum(p < CHUNK for p in merge_scan(k, recs, s, PN_MAXN)[1])
                    for extra in (0, 1):   # the cut at, and one record behind, the first chunk's edge
                        add("%s_cut%d_s%d" % (nm, extra, s), PN_MAXN, recs, s, "chunks" if extra else "some", first + extra)
    # the chunk edge: records 0..1021 all want requests 0..k-1 (record 0 gets them); 1022, 1023, 1024.. are fresh
    fresh = lambda j: np.arange(k) + k * (j + 1)              # noqa: E731
    for dead in (False, True):
        reqs = np.tile(np.arange(k), (CHUNK + 6, 1))
        for j, i in enumerate(range(CHUNK - 2, CHUNK + 6)):
            reqs[i] = fresh(j)
        if dead:
            reqs[CHUNK - 1, 0] = reqs[CHUNK - 2, 0]           # 1023 shares only with 1022 (kept): 1023 is dropped ..
        reqs[CHUNK, k - 1] = reqs[CHUNK - 1, k - 1]           # .. and 1024 shares only with 1023: kept iff 1023 was dropped
        for s in (0, 1):
            add("edge_%s_s%d" % ("dead" if dead else "kept", s), PN_MAXN, _records(k, reqs, np.arange(CHUNK + 6)), s, "chunks")
    # ---- CPU conditions
    by_name = {c.name: c for c in cases}
    assert len(by_name) == len(cases)
    for c in cases:
        kept, pos = merge_scan(c.k, c.recs, c.sort_by_cost, c.max_pools)
        assert kept, c.name
        assert c.recs[:, :k].min() >= 0 and c.recs[:, :k].max() < c.n_requests
        if c.claim == "chunks":
            assert len({p // CHUNK for p in pos}) >= 2, c.name
        elif c.claim == "first chunk":
            assert c.recs.shape[0] > CHUNK and max(pos) < CHUNK and c.n_requests - k * len(kept) < k, c.name
    full = {c.name: merge_scan(k, c.recs, c.sort_by_cost, c.max_pools) for c in cases}
    for s in (0, 1):
        kept_pos = full["edge_kept_s%d" % s][1]
        assert CHUNK - 1 in kept_pos and CHUNK not in kept_pos and CHUNK + 1 in kept_pos
        dead_pos = full["edge_dead_s%d" % s][1]
        assert CHUNK - 2 in dead_pos and CHUNK - 1 not in dead_pos and CHUNK in dead_pos
        for nm in ("chain", "sparse"):   # the cut lands at the chunk edge / keeps exactly one record of the second chunk
            assert max(full["%s_cut0_s%d" % (nm, s)][1]) < CHUNK <= max(full["%s_cut1_s%d" % (nm, s)][1])
            assert sum(p >= CHUNK for p in full["%s_cut1_s%d" % (nm, s)][1]) == 1
    n = 2049   # equal costs keep the input order; strictly descending costs reverse it
    assert full["equal_costs_%d" % n][0] == [r[:2 * k] + [7] for r in merge_scan(k, by_name["sparse_%d_s0" % n].recs, 0, PN_MAXN)[0]]
    rev = by_name["descending_%d" % n].recs[::-1]
    assert full["descending_%d" % n][0] == merge_scan(k, rev, 0, PN_MAXN)[0]
    return cases


def bad_id_inputs(k):
    """-> [(label, record, id, records)]: 1025 records with valid ids except ONE id outside [0, 2047), in the first, a middle
    or the last record: -1, n_requests and 2^30 (td_pool_merge must refuse them; never hand them to a library without
    that check: the greedy would index its tables with the id)"""
    base = _records(k, (np.arange(CHUNK + 1)[:, None] + np.arange(k)[None, :]) % PN_MAXN, np.zeros(CHUNK + 1))
    out = []
    for rec, field in ((0, 0), (CHUNK // 2, k - 1), (CHUNK, 1)):
        for bad in (-1, PN_MAXN, 2**30):
            r = base.copy()
            r[rec, field] = bad
            out.append(("rec%d_id%d" % (rec, bad), rec, bad, r))
    return out
