"""Shared data of the matching / optimal-pool tests (no GPU, no networkx): the seeded model families that the golden
generator (tests/golden/pool_opt/make_pool_opt_golden.py) and the GPU tests build alike, networkx's blossom test graphs,
and pool_opt_min.py's candidate rule, greedy and objective restated with numpy."""
import numpy as np

SIZES = [0, 1, 2, 3, 5, 31, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300]
FAMILIES = ["ties", "wide", "sparse", "near_max", "nonpos", "pool"]

# networkx's test_matching.py blossom graphs (weighted edge lists, vertices from 1 as there)
BLOSSOM_CASES = {
    "s_blossom": [(1, 2, 8), (1, 3, 9), (2, 3, 10), (3, 4, 7)],
    "s_blossom_augment": [(1, 2, 8), (1, 3, 9), (2, 3, 10), (3, 4, 7), (1, 6, 5), (4, 5, 6)],
    "s_t_blossom": [(1, 2, 9), (1, 3, 8), (2, 3, 10), (1, 4, 5), (4, 5, 4), (1, 6, 3)],
    "s_t_blossom_relabel": [(1, 2, 9), (1, 3, 8), (2, 3, 10), (1, 4, 5), (4, 5, 3), (1, 6, 4)],
    "s_t_blossom_moved": [(1, 2, 9), (1, 3, 8), (2, 3, 10), (1, 4, 5), (4, 5, 3), (3, 6, 4)],
    "nested_s_blossom": [(1, 2, 9), (1, 3, 9), (2, 3, 10), (2, 4, 8), (3, 5, 8), (4, 5, 10), (5, 6, 6)],
    "nested_s_blossom_relabel": [(1, 2, 10), (1, 7, 10), (2, 3, 12), (3, 4, 20), (3, 5, 20), (4, 5, 25), (5, 6, 10), (6, 7, 10),
                                 (7, 8, 8)],
    "nested_s_blossom_expand": [(1, 2, 8), (1, 3, 8), (2, 3, 10), (2, 4, 12), (3, 5, 12), (4, 5, 14), (4, 6, 12), (5, 7, 12),
                                (6, 7, 14), (7, 8, 12)],
    "s_blossom_relabel_expand": [(1, 2, 23), (1, 5, 22), (1, 6, 15), (2, 3, 25), (3, 4, 22), (4, 5, 25), (4, 8, 14), (5, 7, 13)],
    "nested_s_blossom_relabel_expand": [(1, 2, 19), (1, 3, 20), (1, 8, 8), (2, 3, 25), (2, 4, 18), (3, 5, 18), (4, 5, 13),
                                        (4, 7, 7), (5, 6, 7)],
    "nasty_blossom1": [(1, 2, 45), (1, 5, 45), (2, 3, 50), (3, 4, 45), (4, 5, 50), (1, 6, 30), (3, 9, 35), (4, 8, 35), (5, 7, 26),
                       (9, 10, 5)],
    "nasty_blossom2": [(1, 2, 45), (1, 5, 45), (2, 3, 50), (3, 4, 45), (4, 5, 50), (1, 6, 30), (3, 9, 35), (4, 8, 26), (5, 7, 40),
                       (9, 10, 5)],
    "nasty_blossom_least_slack": [(1, 2, 45), (1, 5, 45), (2, 3, 50), (3, 4, 45), (4, 5, 50), (1, 6, 30), (3, 9, 35), (4, 8, 28),
                                  (5, 7, 26), (9, 10, 5)],
    "nasty_blossom_augmenting": [(1, 2, 45), (1, 7, 45), (2, 3, 50), (3, 4, 45), (4, 5, 95), (4, 6, 94), (5, 6, 94), (6, 7, 50),
                                 (1, 8, 30), (3, 11, 35), (5, 9, 36), (7, 10, 26), (11, 12, 5)],
    "nasty_blossom_expand_recursively": [(1, 2, 40), (1, 3, 40), (2, 3, 60), (2, 4, 55), (3, 5, 55), (4, 5, 50), (1, 8, 15),
                                         (5, 7, 30), (7, 6, 10), (8, 10, 10), (4, 9, 30)],
}


def blossom_matrix(edges):
    """edge list (1-based) -> weight matrix (0-based; one direction filled, the other 0)"""
    n = max(max(a, b) for a, b, _ in edges)
    W = np.zeros((n, n), np.int32)
    for a, b, w in edges:
        W[a - 1, b - 1] = w
    return W


def family(fam, n, seed=None):
    """a seeded dense n x n weight matrix of one family"""
    rng = np.random.default_rng(FAMILIES.index(fam) * 10007 + n if seed is None else seed)
    if fam == "ties":
        W = rng.integers(1, 6, (n, n))
    elif fam == "wide":
        W = rng.integers(1, 10**6 + 1, (n, n))
    elif fam == "sparse":   # 90 % of the cells <= 0 (no edge)
        W = np.where(rng.random((n, n)) < 0.9, -rng.integers(0, 5, (n, n)), rng.integers(1, 1000, (n, n)))
    elif fam == "near_max":
        W = 2**31 - 1 - rng.integers(0, 1000, (n, n))
    elif fam == "nonpos":
        W = -rng.integers(0, 100, (n, n))
    elif fam == "pool":     # K - w with w a pool cost (three U{1..39} legs), K = floor(n/2) * max w + 1
        K = (n // 2) * 117 + 1
        W = K - rng.integers(3, 118, (n, n))
    else:
        raise ValueError(fam)
    return np.asarray(W, np.int64).astype(np.int32)


def pool_model(m, seed, S):
    """m customers with from / to uniform over S stands"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, S, m).astype(np.int32), rng.integers(0, S, m).astype(np.int32)


def pool_table(S=100, seed=7):
    """pool_opt_min.py:29's table: S x S, U{1..39}"""
    return np.random.default_rng(seed).integers(1, 40, (S, S)).astype(np.int32)


# the pool models with golden (count, total): (name, m, seed, table?, max_loss)
POOL_CASES = [("gated%d" % m, m, 100 + m, True, 1.01) for m in (0, 1, 2, 3, 5, 31, 64, 100, 128, 200, 300)] + \
             [("every%d" % m, m, 200 + m, False, None) for m in (0, 1, 2, 3, 5, 31, 64, 100, 128, 200, 300)]


def pair_costs(frm, to, table=None, max_loss=None):
    """pool_opt_min.py:51-79 with numpy: (c, plan1) where c[A, B] = min(cost1, cost2) when the ordered pair (A, B) is a
    candidate, else -1 (int64), and plan1[A, B] = cost1 < cost2.  max_loss None or <= 0: every ordered pair is one."""
    f = np.asarray(frm, np.int64)
    t = np.asarray(to, np.int64)
    if table is None:
        d = lambda a, b: np.abs(a - b)
    else:
        T = np.asarray(table, np.int64)
        d = lambda a, b: T[a, b]
    Af, At, Bf, Bt = f[:, None], t[:, None], f[None, :], t[None, :]
    ab, bfat, atbt, bfbt, btat, aa = d(Af, Bf), d(Bf, At), d(At, Bt), d(Bf, Bt), d(Bt, At), d(Af, At)
    c1, c2 = ab + bfat + atbt, ab + bfbt + btat
    cand = ~np.eye(f.size, dtype=bool)
    if max_loss is not None and max_loss > 0:
        p1 = ((bfat + atbt) < bfbt * max_loss) & ((ab + bfat) < aa * max_loss)
        p2 = c2 < aa * max_loss
        cand &= p1 | p2
    return np.where(cand, np.minimum(c1, c2), -1), c1 < c2


def greedy(c):
    """:81-102: candidates stably sorted by cost (A-major insertion order), kept iff they share no customer with an earlier
    kept one -> list of (custA, custB, cost)"""
    A, B = np.nonzero(c >= 0)
    cost = c[A, B]
    used = np.zeros(c.shape[0], bool)
    out = []
    for k in np.argsort(cost, kind="stable"):
        a, b = int(A[k]), int(B[k])
        if not used[a] and not used[b]:
            used[a] = used[b] = True
            out.append((a, b, int(cost[k])))
    return out


def lex_weights(c):
    """(K, W): the matching weights of the lexicographic objective, W[A][B] = K - c[A][B] for a candidate, 0 otherwise"""
    m = c.shape[0]
    cand = c >= 0
    if not cand.any():
        return 1, np.zeros((m, m), np.int64)
    mx, mn = int(c[cand].max()), int(c[cand].min())
    K = (m // 2) * (max(mx, 0) + max(-mn, 0)) + 1
    return K, np.where(cand, K - c, 0)
