"""Numpy checker of a maximum-weight matching certificate as td_match_batched exports it (doubled units).

For a model with weight matrix W (n x n; edge {i, j} has weight max(W[i][j], W[j][i]) and exists iff that is > 0), the
mates, the vertex duals y, the blossom family as parent pointers over the 2n node ids (vertices 0..n-1, blossoms
n..2n-1, -1 = top level) and the blossom duals z (z[k] belongs to blossom n + k), it re-verifies outside the library:
  * the mates form a matching of existing edges and `total` is its weight,
  * y >= 0, z >= 0, y_i = 0 for every unmatched i,
  * 2 w_ij <= y_i + y_j + sum of z_B over the blossoms holding both i and j, for every edge,
  * every blossom with z_B > 0 is full (odd size, (|B| - 1) / 2 matched pairs inside),
  * (sum y + sum z_B * floor(|B| / 2)) / 2 == total == bound.
Weak duality then makes `total` the maximum.  No GPU and no networkx needed.
"""
import numpy as np


def edge_weights(W):
    W = np.asarray(W, np.int64)
    w = np.maximum(W, W.T)
    np.fill_diagonal(w, 0)
    return w


def check(W, mate, total, bound, y, parent, z):
    """Raises AssertionError with the first violated condition."""
    w = edge_weights(W)
    n = w.shape[0]
    mate = np.asarray(mate, np.int64)[:n]
    y = np.asarray(y, np.int64)[:n]
    parent = np.asarray(parent, np.int64)
    z = np.asarray(z, np.int64)[:n]
    par = np.concatenate([parent[:n], parent[n:2 * n]]) if n else parent[:0]
    idx = np.arange(n)
    m = mate >= 0
    assert ((mate >= -1) & (mate < n)).all(), "mate out of range"
    assert (mate[mate[m]] == idx[m]).all(), "mates not symmetric"
    assert (w[idx[m], mate[m]] > 0).all(), "a matched pair is not an edge"
    tot = int(w[idx[m], mate[m]].sum()) // 2
    assert tot == int(total), ("total", tot, int(total))
    assert (y >= 0).all(), "negative vertex dual"
    assert (z >= 0).all(), "negative blossom dual"
    assert (y[~m] == 0).all(), "unmatched vertex with a positive dual"
    # A[v, k]: vertex v lies in blossom n + k
    A = np.zeros((n, n), bool)
    cur = par[:n].copy() if n else np.zeros(0, np.int64)
    for _ in range(2 * n + 1):
        live = cur >= 0
        if not live.any():
            break
        assert (cur[live] >= n).all() and (cur[live] < 2 * n).all(), "parent is not a blossom id"
        A[idx[live], cur[live] - n] = True
        cur[live] = par[cur[live]]
    else:
        raise AssertionError("parent pointers form a cycle")
    size = A.sum(axis=0)
    used = z > 0
    assert (size[used] % 2 == 1).all(), "a blossom with z > 0 has an even size"
    inside = A[m] & A[mate[m]]          # vertex v and its mate both in blossom k
    pairs = inside.sum(axis=0) // 2
    assert (pairs[used] == (size[used] - 1) // 2).all(), "a blossom with z > 0 is not full"
    Af = A.astype(np.float64)
    zs = np.rint((Af * z.astype(np.float64)) @ Af.T).astype(np.int64)   # exact: every term < 2^53
    slack = y[:, None] + y[None, :] + zs - 2 * w
    e = w > 0
    assert (slack[e] >= 0).all(), "an edge violates its dual constraint"
    b2 = int(y.sum()) + int((z * (size // 2)).sum())
    assert b2 % 2 == 0 and b2 // 2 == tot == int(bound), ("dual objective", b2, tot, int(bound))
