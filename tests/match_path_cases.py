"""The case table of tests/test_match_paths_cpu.py, tests/test_gpu_match_paths.py and
tests/golden/pool_opt/make_match_paths_golden.py: models that sit on every control path of the blossom solver
(csrc/td_match_core.h), on the state placement edge of state_plan and on the chunk seams and range edges of
pool2_batched_impl (csrc/td_match.hip).  Plain numpy: nothing here needs a GPU, networkx or a compiler.

Four parts.

(a) MATCH_CASES: matching models, each with a name, a maker, the claims it must satisfy and the reason it exists.  A claim
    is a threshold that matters to the lane split of the device build (64 lanes): `trace` claims are minima of the path
    counters of the host build (tdm::Trace, printed by tools/match_proto.cpp built with -DTDM_TRACE, in TRACE_FIELDS' order),
    `final` claims are minima of the final blossom structure (structure(): the most leaves of a blossom left standing, the
    deepest nesting of a vertex), which the device exports too.  The expected totals are networkx's
    (tests/golden/pool_opt/match_paths.json); the unions also know theirs without it: a disjoint union's optimum is the
    sum of its components', r x the sum of the committed networkx totals of the fifteen graphs.

(b) The placement rule of state_plan and the chunk size of pool2_batched_impl restated, each with the line it restates, and
    the placement cases: one-edge models at both candidate edges, the r = PLACEMENT_R union padded to the edge and past it.

(c) SEAMS / POLICIES / seam_models() / v_wrapper_case(): pool batches that end exactly at, one past and one past twice the
    chunk, at a stride where the chunk divides 256 MiB exactly (2048) and one where it does not (1449).

(d) Range edges of the pool weights: span_case(), negative_case(), limit_cell_case(), with references that keep the
    candidate mask apart from the cost (tests/pool_opt_data.py marks a non-candidate with -1, which a negative cost is not).
"""
import hashlib

import numpy as np

import pool_opt_data as D

# ======================================================================================================================
# (a) matching cases
# ======================================================================================================================
# tdm::Trace's fields as tools/match_proto.cpp prints them (its TRACE_FIELDS)
TRACE_FIELDS = ("blossom_formed leaves_max aug_blossom aug_fwd aug_back aug_nested expand_end expand_end_nested expand_T relabel_fwd "
                "relabel_back relabel_steps_max sub_vertex_T sub_blossom_T reach_in_T delta1 delta2 delta3 delta4 substage_max "
                "augmentations").split()
# the rarely walked paths: each must be walked by at least two cases of the table
RARE_PATHS = ("sub_blossom_T", "expand_end_nested", "relabel_fwd", "relabel_back", "aug_nested")
WAVE = 64   # lanes of the device build: a case counts for the lane split only when its vertex ids pass one wave (n > 64)

BLOSSOM_NAMES = sorted(D.BLOSSOM_CASES)
UNION_SEED = 20240
PLACEMENT_R = 9


def union(r, seed=UNION_SEED, pad_to=None):
    """r copies of the fifteen networkx blossom graphs as one graph: the copies are disjoint, the vertex ids a seeded
    permutation (so every component's vertices and blossoms are spread over all lanes and several loop trips), the weight
    of an edge in the upper or the lower triangle by turns.  pad_to: isolated vertices 0 .. pad_to - size - 1 below the
    union, which then sits at the top vertex ids."""
    edges = []
    base = 0
    for _ in range(r):
        for name in BLOSSOM_NAMES:
            es = D.BLOSSOM_CASES[name]
            edges += [(base + a - 1, base + b - 1, w) for a, b, w in es]
            base += max(max(a, b) for a, b, _ in es)
    perm = np.random.default_rng(seed + r).permutation(base)
    n = base if pad_to is None else pad_to
    assert n >= base
    W = np.zeros((n, n), np.int32)
    for k, (a, b, w) in enumerate(edges):
        i, j = sorted((int(perm[a]) + n - base, int(perm[b]) + n - base))
        if k & 1:
            i, j = j, i
        W[i, j] = w
    return W


UNION_SIZE = sum(max(max(a, b) for a, b, _ in es) for es in D.BLOSSOM_CASES.values())   # 118 vertices per copy


def odd_cycle(k, pendant_at):
    """an odd cycle of k vertices, every edge of weight 10, and a vertex k hung on `pendant_at` with weight 8: the cycle is
    matched up pair by pair, the last free vertex grows both ways round and shrinks ALL k vertices into one blossom, and
    the pendant edge then augments through it (the optimum is (k - 1) / 2 * 10 + 8)"""
    assert k % 2 == 1
    W = np.zeros((k + 1, k + 1), np.int32)
    for i in range(k):
        j = (i + 1) % k
        W[min(i, j), max(i, j)] = 10
    W[pendant_at, k] = 8
    return W


def triangle_chain(depth, pendant_at):
    """vertex 0 and `depth` pairs (2k - 1, 2k) of weight `base`; pair k hangs on pair k - 1 (pair 1 on vertex 0) by two edges
    of weight base - k.  The pairs match first; then level after level closes a triangle [the blossom so far, 2k - 1, 2k]:
    `depth` blossoms nested `depth` deep, 2 depth + 1 leaves in the outermost.  base = 8 depth^2 + 20 keeps every dual
    positive until the last vertex 2 depth + 1, hung on `pendant_at` with weight base - 2 depth^2, augments through them."""
    n = 2 * depth + 2
    base = 8 * depth * depth + 20
    W = np.zeros((n, n), np.int32)
    W[0, 1] = W[0, 2] = base - 1
    W[1, 2] = base
    for k in range(2, depth + 1):
        a, b = 2 * k - 1, 2 * k
        W[a - 2, a] = W[b - 2, b] = base - k
        W[a, b] = base
    W[pendant_at, n - 1] = base - 2 * depth * depth
    return W


def case(name, make, why, trace=None, final=None, total=None):
    return dict(name=name, make=make, why=why, trace=trace or {}, final=final or {}, total=total)


UNION_TOTAL = 1137   # the sum of the fifteen committed networkx totals (tests/golden/pool_opt/golden.json, "blossom")
_UNION_TRACE = dict(sub_blossom_T=1, expand_end_nested=1, relabel_fwd=1, relabel_back=1, reach_in_T=1, delta1=1, delta2=1, delta3=1,
                    delta4=1, sub_vertex_T=1, expand_T=1, expand_end=1, aug_nested=1)

MATCH_CASES = [
    case("union_r1", lambda: union(1), "every 'nasty' expansion of the networkx graphs with ids spread over 118 vertices",
         trace=_UNION_TRACE, total=UNION_TOTAL),
    case("union_r2", lambda: union(2), "the same over 236 vertices: four trips of every lane-split loop",
         trace=_UNION_TRACE, total=2 * UNION_TOTAL),
    case("union_r4", lambda: union(4), "the same over 472 vertices: eight trips",
         trace=_UNION_TRACE, total=4 * UNION_TOTAL),
    case("cycle65", lambda: odd_cycle(65, 1), "one blossom of 65 leaves: the leaf loop's ballot takes a second round",
         trace=dict(leaves_max=65, aug_back=1), final=dict(leaves=65), total=32 * 10 + 8),
    case("cycle129", lambda: odd_cycle(129, 64), "129 leaves: a third ballot round, the augmenting walk the other way round",
         trace=dict(leaves_max=129, aug_fwd=1), final=dict(leaves=129), total=64 * 10 + 8),
    case("cycle199", lambda: odd_cycle(199, 100), "199 leaves: four ballot rounds, the last one partly filled",
         trace=dict(leaves_max=199), final=dict(leaves=199), total=99 * 10 + 8),
    case("chain41", lambda: triangle_chain(41, 1), "41 blossoms nested 41 deep, 83 leaves; the augmentation enters at the innermost",
         trace=dict(leaves_max=83, aug_nested=40, blossom_formed=41), final=dict(leaves=83, depth=41)),
    case("chain100", lambda: triangle_chain(100, 100), "100 deep, 201 leaves; the augmentation enters half way down",
         trace=dict(leaves_max=201, aug_nested=50, blossom_formed=100, aug_fwd=1, aug_back=1), final=dict(leaves=201, depth=100)),
    case("family_sparse300", lambda: D.family("sparse", 300), "committed family model: a 253-leaf blossom at formation, a 72-step relabel walk",
         trace=dict(leaves_max=129, relabel_steps_max=65, aug_nested=1, expand_T=1), final=dict(leaves=129)),
    case("family_ties257", lambda: D.family("ties", 257), "committed family model: all 257 vertices in one blossom, nested 127 deep at the end",
         trace=dict(leaves_max=129, aug_nested=1, expand_end_nested=1), final=dict(leaves=129, depth=64)),
    case("family_near_max255", lambda: D.family("near_max", 255), "the one committed model that walks sub_blossom_T; weights near 2^31",
         trace=dict(sub_blossom_T=1, sub_vertex_T=1, expand_end_nested=1, relabel_fwd=1, relabel_back=1), final=dict(leaves=129, depth=64)),
    case("family_pool256", lambda: D.family("pool", 256), "committed family model: 48 delta-4 expansions, 214 descents into child blossoms",
         trace=dict(leaves_max=129, expand_T=10, aug_nested=100, sub_vertex_T=1, delta4=10)),
]


def structure(parent, n):
    """(the most leaves of a blossom, the deepest nesting of a vertex) from parent pointers over 2n node ids (vertices 0..n-1,
    blossoms n..2n-1, -1 = top level)"""
    par = np.asarray(parent, np.int64)
    leaves = np.zeros(2 * n + 1, np.int64)
    depth = np.zeros(n, np.int64)
    cur = par[:n].copy()
    idx = np.arange(n)
    for _ in range(2 * n + 1):
        live = cur >= 0
        if not live.any():
            break
        np.add.at(leaves, cur[live], 1)
        depth[idx[live]] += 1
        cur[live] = par[cur[live]]
    return (int(leaves.max()) if n else 0), (int(depth.max()) if n else 0)


def digest(mate, y, parent, z):
    """SHA-256 of a model's (mate, y, blossom_parent, z), each over the model's own n (2n for the parents, blossom ids
    n..2n-1), as little-endian int64"""
    h = hashlib.sha256()
    for a in (mate, y, parent, z):
        h.update(np.ascontiguousarray(np.asarray(a, np.int64)).astype("<i8").tobytes())
    return h.hexdigest()


def digest_parts(mate, y, parent, z):
    """the four arrays hashed one by one, to name the first that differs"""
    return [digest(a, [], [], []) for a in (mate, y, parent, z)]


def own_ids(parent_row, stride, m):
    """a model's 2m parent pointers from a row exported at stride `stride` (blossom ids stride + k -> m + k)"""
    par = np.asarray(parent_row, np.int64)
    conv = lambda a: np.where(a >= stride, a - stride + m, a)
    return np.concatenate([conv(par[:m]), conv(par[stride:stride + m])])


# ======================================================================================================================
# (b) state placement and chunk size restated
# ======================================================================================================================
NMAX = 2048                      # `constexpr int MATCH_NMAX = 2048`
LDS_CAP = 160 * 1024             # `cap = std::min<size_t>((size_t)v, 160 * 1024) - 1024`
LDS_RESERVE = 1024
LDS_FALLBACK = 64 * 1024         # `v = 64 * 1024` when the attribute cannot be read
SLAB_BYTES = 256 << 20           # `((size_t)256 << 20) / (sizeof(int32_t) * NN)`
WS_BYTES = 512 << 20             # `((size_t)512 << 20) / *per`
POOL_KMAX = 1 << 33              # `constexpr int64_t POOL_KMAX = (int64_t)1 << 33`
INT_MAX, INT_MIN = 2**31 - 1, -2**31
TD_ERANGE = -4

MP_LDS, MP_WS, MP_POOL, MP_GREEDY, MP_MATCH, MP_PER_MODEL = 1, 2, 4, 8, 16, 32   # td_last_stats word 14
MP_CHUNK_SHIFT, MP_CHUNK_MAX = 8, 0xFFFF


def state_bytes(n):
    """`bytes(n) = n * (2 * 2 * 8 + 6 * 4 + 2 * 4 + 11 * 2 * 4) + 64` (td_match_core.h): 152 n + 64"""
    return n * (2 * 2 * 8 + 6 * 4 + 2 * 4 + 11 * 2 * 4) + 64


def align256(x):
    """td_stage.h's align256"""
    return (x + 255) // 256 * 256


def lds_budget(max_shared):
    """`cap = std::min<size_t>((size_t)v, 160 * 1024) - 1024` (td::lds_budget)"""
    return min(max_shared, LDS_CAP) - LDS_RESERVE


def in_lds(nmax, max_shared):
    """`*per = align256(tdm::bytes(std::max(nmax, 1))); *lds = *per <= lds_budget();` (state_plan)"""
    return align256(state_bytes(max(nmax, 1))) <= lds_budget(max_shared)


def ws_grid(batch, nmax):
    """`*grid = max(1, min(min(batch, 1 << 20), (512 << 20) / *per))` (state_plan, workspace placement)"""
    return max(1, min(min(batch, 1 << 20), WS_BYTES // align256(state_bytes(max(nmax, 1)))))


def placement_edge(max_shared):
    """the largest n whose state lies in LDS"""
    n = 1
    while in_lds(n + 1, max_shared):
        n += 1
    return n


# the budgets a device may report -> the edge: the state is in LDS at n_edge and in the workspace at n_edge + 1
PLACEMENT_BUDGETS = {LDS_FALLBACK: 424, LDS_CAP: 1070}


def one_edge(ns):
    """an ns-vertex model with the single edge {0, ns - 1} of weight 7: placement depends on ns alone"""
    W = np.zeros((ns, ns), np.int32)
    W[0, ns - 1] = 7
    return W


def placement_r(ns):
    """copies of the union in an ns-vertex placement model: 9 (1062 vertices) at the 160 KiB edge, 3 (354) at the 64 KiB one"""
    return PLACEMENT_R if ns >= PLACEMENT_R * UNION_SIZE else 3


def placement_union(ns):
    """the r = 9 union (1062 vertices; total 9 * 1137 = 10 233) at the top vertex ids of an ns-vertex model, isolated vertices
    below it (r = 3 at the 64 KiB edge).  Measured: the host build solves the 1070- and the 1071-vertex model in about 1 s
    each; the MI355X takes 2.8 s for the two (state in LDS, then in a workspace slice) with their numpy certificate checks."""
    return union(placement_r(ns), pad_to=ns)


def placement_union_total(ns):
    return placement_r(ns) * UNION_TOTAL


def chunk_of(n, batch):
    """`chunk = max(1, min(B, (256 << 20) / (sizeof(int32_t) * max(n * n, 1))))` (pool2_batched_impl)"""
    return max(1, min(batch, SLAB_BYTES // (4 * max(n * n, 1))))


def chunks_launched(n, batch):
    """`for (b0 = 0; b0 < batch; b0 += chunk)`: ceil(batch / chunk)"""
    c = chunk_of(n, batch)
    return -(-batch // c)


def expected_pool_path(n, batch, longest, optimal, per_model, max_shared):
    """word 14 after a pool call: `run_match = opt_v || optimal`, `run_greedy = opt_v || !optimal`; the placement bits only
    with run_match (state_plan is then asked for the longest model)"""
    run_match, run_greedy = per_model or bool(optimal), per_model or not optimal
    w = MP_POOL | (MP_PER_MODEL if per_model else 0) | (MP_GREEDY if run_greedy else 0)
    if run_match:
        w |= MP_MATCH | (MP_LDS if in_lds(longest, max_shared) else MP_WS)
    return w | min(chunks_launched(n, batch), MP_CHUNK_MAX) << MP_CHUNK_SHIFT


# ======================================================================================================================
# (c) chunk seams
# ======================================================================================================================
# stride -> the chunk it gives: 2048 divides 256 MiB exactly (16 MiB blocks), 4 * 1449^2 = 8 398 404 does not
SEAMS = {2048: 16, 1449: 31}
SEAM_MAX_CUSTOMERS = 40
SEAM_TABLE_MAX_LOSS = 1.01
SEAM_SEED = 9001   # chosen so that the optimum of each of the eight seam models differs from its greedy (the CPU tier asserts it)


def seam_batches(stride):
    c = SEAMS[stride]
    return [c, c + 1, 2 * c + 1]


def seam_models(stride, with_table):
    """the 2 chunk + 1 models of a stride (a shorter batch is a prefix): 0..40 customers each; the four models on either side
    of the two seams are the largest and differ from each other (40, 39, 38 and 37 customers, own seeds)"""
    c = SEAMS[stride]
    S = 100 if with_table else 50
    rng = np.random.default_rng(7000 + stride + (1 if with_table else 0))
    sizes = rng.integers(0, SEAM_MAX_CUSTOMERS - 3, 2 * c + 1)
    sizes[0] = 0   # an empty model at the head of the first chunk
    for k, m in ((c - 1, 40), (c, 39), (2 * c - 1, 38), (2 * c, 37)):
        sizes[k] = m
    return [D.pool_model(int(m), SEAM_SEED + 131 * stride + 7 * k + (1 if with_table else 0), S) for k, m in enumerate(sizes)]


def seam_key(stride, with_table):
    return "seam%d_%s" % (stride, "table" if with_table else "line")


def seam_table(with_table):
    return (D.pool_table(), SEAM_TABLE_MAX_LOSS) if with_table else (None, None)


def seam_policy(kind, stride, batch):
    """(optimal argument of pool2_batched, per-model list of 0 / 1): "greedy", "optimal", or "mix": a per-model list that
    changes kind exactly at every seam (greedy below the first, optimal to the second, greedy after)"""
    c = SEAMS[stride]
    if kind == "greedy":
        return False, [0] * batch
    if kind == "optimal":
        return True, [1] * batch
    v = [(b // c) & 1 for b in range(batch)]
    return v, v


POLICIES = ("greedy", "optimal", "mix")


def v_wrapper_case():
    """one per-model batch through the plain wrapper (no n=): model 0 has 2048 customers and is greedy, so the stride is 2048
    and the 32 small optimal models behind it keep their solver state in the workspace (state_plan sees the longest model of
    the call); 33 models, chunk 16: three chunks.  Every pair is a candidate (|a - b| over 50 stands)."""
    models = [D.pool_model(NMAX, 424242, 50)] + seam_models(2048, False)[1:]
    return models, [0] + [1] * (len(models) - 1)


V_WRAPPER_KEY = seam_key(2048, False)   # its small models are that seam's models 1..32


# ======================================================================================================================
# (d) range edges of the pool weights
# ======================================================================================================================
def pair_costs_masked(frm, to, table):
    """every ordered pair A != B is a candidate (max_loss None): (c int64, candidate mask, plan1), with no sentinel in c"""
    cand = ~np.eye(len(frm), dtype=bool)
    f, t = np.asarray(frm, np.int64), np.asarray(to, np.int64)
    T = np.asarray(table, np.int64)
    Af, At, Bf, Bt = f[:, None], t[:, None], f[None, :], t[None, :]
    c1 = T[Af, Bf] + T[Bf, At] + T[At, Bt]
    c2 = T[Af, Bf] + T[Bf, Bt] + T[Bt, At]
    return np.minimum(c1, c2), cand, c1 < c2


def greedy_masked(c, cand):
    """pool_opt_data.greedy with the mask apart: candidates stably sorted by cost (A-major), kept iff both are unused"""
    A, B = np.nonzero(cand)
    cost = c[A, B]
    used = np.zeros(c.shape[0], bool)
    out = []
    for k in np.argsort(cost, kind="stable"):
        a, b = int(A[k]), int(B[k])
        if not used[a] and not used[b]:
            used[a] = used[b] = True
            out.append((a, b, int(cost[k])))
            if 2 * len(out) + 1 >= c.shape[0]:   # at most one customer is left: nothing more can be kept
                break
    return out


def span_of(c, cand):
    """`span = (mx > 0 ? mx : 0) + (mn < 0 ? -mn : 0)` (k_pool_costs)"""
    mx, mn = int(c[cand].max()), int(c[cand].min())
    return max(mx, 0) + max(-mn, 0)


def lex_weights_masked(c, cand):
    """(K, W) as k_pool_costs / PoolW make them: K = floor(m / 2) * span + 1, W = K - c on candidates (Python integers)"""
    m = c.shape[0]
    K = (m // 2) * span_of(c, cand) + 1
    W = np.zeros((m, m), object)
    W[cand] = [K - int(x) for x in c[cand]]
    return K, W


def accepted(m, span):
    """`if (opt && kk + span >= POOL_KMAX)` refuses: accepted iff floor(m / 2) * span + 1 + span < 2^33"""
    return (m // 2) * span + 1 + span < POOL_KMAX


SPAN_M = 64
SPAN_MAX = 260301048   # the largest span a 64-customer model may have: 33 * span + 1 < 2^33
# 2^33 - 1 = 7 * 23 * 89 * 599479, so 33 * span + 1 never equals 2^33; with 44 customers 23 * span + 1 does, at
# span = 373 475 417: the one place where `>=` and `>` in the range check differ.  That span is refused, one below is accepted.
EXACT_M = 44
EXACT_SPAN = (2**33 - 1) // 23
# (customers, largest accepted span): span + 1 is refused
SPAN_EDGES = {"span_max": (SPAN_M, SPAN_MAX), "span_exact": (EXACT_M, EXACT_SPAN - 1)}


def span_case(span, m=SPAN_M):
    """m (64) customers on a 12-stand table: customers 0 and 1 both ride 0 -> 1 and d(0, 1) = span, d(0, 0) = d(1, 1) = 0, so the
    ordered pairs (0, 1) and (1, 0) cost exactly `span`; every other entry is U{1..39}, so every other pair costs at most
    117 and the candidate costs span [3.., span]: K = 32 span + 1.  Returns (frm, to, table)."""
    rng = np.random.default_rng(606)
    S = 12
    table = rng.integers(1, 40, (S, S)).astype(np.int64)
    table[0, 0] = table[1, 1] = 0
    table[0, 1] = span
    table[1, 0] = 1
    frm = np.concatenate([[0, 0], rng.integers(2, S, m - 2)]).astype(np.int32)
    to = np.concatenate([[1, 1], rng.integers(2, S, m - 2)]).astype(np.int32)
    return frm, to, table.astype(np.int32)


def negative_case():
    """48 customers on a 9-stand table with entries in [-10, 39]: candidate costs of both signs (c_max > 0 > c_min), so span
    adds both, and the optimum keeps pools of both signs (11 below zero, 13 above: the CPU tier asserts both kinds), so
    k_pool_finish's sort key crosses the sign change.  Returns (frm, to, table)."""
    rng = np.random.default_rng(707)
    S = 9
    table = rng.integers(-10, 40, (S, S)).astype(np.int32)
    frm, to = rng.integers(0, S, 48).astype(np.int32), rng.integers(0, S, 48).astype(np.int32)
    return frm, to, table


def limit_cell_case(value):
    """two customers riding 0 -> 1 with d(0, 1) = value and zeros elsewhere: both ordered pairs cost exactly `value`"""
    table = np.zeros((2, 2), np.int64)
    table[0, 1] = value
    return np.zeros(2, np.int32), np.ones(2, np.int32), table.astype(np.int32)


# value -> accepted by the greedy (`if (cc >= INT_MAX || cc <= INT_MIN)` refuses)
LIMIT_CELLS = {INT_MAX - 1: True, INT_MAX: False, INT_MIN + 1: True, INT_MIN: False}
