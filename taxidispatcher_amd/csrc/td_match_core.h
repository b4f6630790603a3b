// td_match_core.h — maximum-weight matching of one general graph (n <= 2048 vertices), primal-dual weighted blossom
// method in Galil's O(n^3) form (the structure of networkx's max_weight_matching), exact int64 arithmetic.
//
// One code path for the host (W = 1: a plain serial build, checked against networkx by tools/match_proto.cpp) and the
// device (W = 64: ONE wave per model).  On the device every lane runs the control logic (queue, augment, shrink,
// expand) on the same shared state and writes the same values, so no lane ever waits for another; the lanes split
// the O(n) loops between them: the row scan of a newly S-labelled vertex, the four delta reductions, the dual update,
// the least-slack rebuild of a new blossom and the leaf relabelling.  A phase whose lanes wrote different cells ends
// with wsync() before any lane reads another lane's cell.
//
// Conventions (networkx / mwmatching): every weight counts twice, y_v starts at max w, slack(v, w) = y_v + y_w - 2 w_vw;
// a blossom dual `dual[b]` is half of the doubled z_B (z_B = 2 dual[b] in the exported certificate).  An edge {v, w}
// exists iff wt(v, w) > 0.  A tight edge is one of slack 0 (no allowedge table: an edge with an S end, once tight,
// stays tight for the rest of the stage, so recomputing the slack gives the same answer).  Edges are packed as
// E(v, w) = v << 12 | w.  A blossom's children form a ring: nxt / prv, ced[x] = the edge from a vertex of x to a vertex
// of nxt[x], head[b] = the child holding the base.  Blossom ids are n .. 2n - 1.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define TDM_HD __host__ __device__ __forceinline__
#else
#define TDM_HD inline
#endif

namespace tdm {

#if defined(__HIP_DEVICE_COMPILE__)
constexpr int W = 64;
#else
constexpr int W = 1;
#endif
constexpr int NMAX = 2048;
constexpr uint64_t NONE = ~0ull;
constexpr uint64_t M24 = (1ull << 24) - 1;
enum { ERR_CAP = 1, ERR_STATE = 2, ERR_CERT = 4, ERR_RANGE = 8 };

TDM_HD int lane()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return threadIdx.x & 63;
#else
    return 0;
#endif
}
TDM_HD uint64_t ballot(bool p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(p);
#else
    return p ? 1ull : 0ull;
#endif
}
TDM_HD int popc(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(m);
#else
    return __builtin_popcountll(m);
#endif
}
TDM_HD uint64_t below(uint64_t m) { return m & ((1ull << lane()) - 1ull); }   // bits of the lanes below this one
TDM_HD uint64_t wmin(uint64_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = __shfl_xor(k, o);
        k = t < k ? t : k;
    }
#endif
    return k;
}
TDM_HD int64_t wsum(int64_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
#endif
    return s;
}
TDM_HD int wor(int s)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s |= __shfl_xor(s, o);
#endif
    return s;
}
TDM_HD void wsync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();   // one-wave workgroup: a memory fence between lane-owned writes and cross-lane reads
#endif
}
TDM_HD void add_i32(int32_t *p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

TDM_HD int E(int v, int w) { return v << 12 | w; }
TDM_HD int E0(int e) { return e >> 12; }
TDM_HD int E1(int e) { return e & 4095; }
TDM_HD int flip(int e) { return (e & 4095) << 12 | e >> 12; }
TDM_HD uint64_t pack(int64_t v, int idx) { return (uint64_t)v << 24 | (uint64_t)(uint32_t)idx; }

// Path counters of the host build (tools/match_proto.cpp's test build defines TDM_TRACE; td_match.hip never does, and
// without the macro the hooks expand to nothing): which control paths a solve walked, how often, how far.
#ifdef TDM_TRACE
struct Trace {
    long long blossom_formed, leaves_max;                                    // add_blossom: count, most leaves at formation
    long long aug_blossom, aug_fwd, aug_back, aug_nested;                    // augment_blossom: items, walk direction, child blossoms
    long long expand_end, expand_end_nested;                                 // end-of-stage expansions, zero-dual sub-blossoms freed with them
    long long expand_T, relabel_fwd, relabel_back, relabel_steps_max;        // delta-4 expansions, the relabel walk's direction and length
    long long sub_vertex_T, sub_blossom_T;                                   // a reached child of an expanded T-blossom becomes T
    long long reach_in_T;                                                    // scan: a vertex inside a T-blossom marked reached
    long long delta1, delta2, delta3, delta4, substage_max, augmentations;   // run: the delta choice, the longest stage
};
inline Trace g_trace{};
#define TDM_COUNT(f) (++tdm::g_trace.f)
#define TDM_MAX(f, v) (tdm::g_trace.f = (long long)(v) > tdm::g_trace.f ? (long long)(v) : tdm::g_trace.f)
#else
#define TDM_COUNT(f) ((void)0)
#define TDM_MAX(f, v) ((void)0)
#endif

// per-model state: n vertices, 2n nodes; carve() lays it out in `bytes(n)` bytes (LDS or a workspace slice)
struct St {
    int32_t *mate, *inb, *pathb, *freeb, *stk, *tmp;              // n
    int32_t *queue;                                                // 2n
    int32_t *label, *lend, *par, *base, *best, *nxt, *prv, *ced, *head, *stamp, *cnt;   // 2n
    int64_t *dual, *cum;                                           // 2n
};
TDM_HD size_t bytes(int n) { return (size_t)n * (2 * 2 * 8 + 6 * 4 + 2 * 4 + 11 * 2 * 4) + 64; }
TDM_HD St carve(void *mem, int n)
{
    St s;
    int64_t *q = (int64_t *)mem;
    s.dual = q;
    s.cum = q + 2 * n;
    int32_t *p = (int32_t *)(q + 4 * n);
    s.mate = p;
    s.inb = p + n;
    s.pathb = p + 2 * n;
    s.freeb = p + 3 * n;
    s.stk = p + 4 * n;
    s.tmp = p + 5 * n;
    s.queue = p + 6 * n;
    p += 8 * n;
    s.label = p;
    s.lend = p + 2 * n;
    s.par = p + 4 * n;
    s.base = p + 6 * n;
    s.best = p + 8 * n;
    s.nxt = p + 10 * n;
    s.prv = p + 12 * n;
    s.ced = p + 14 * n;
    s.head = p + 16 * n;
    s.stamp = p + 18 * n;
    s.cnt = p + 20 * n;
    return s;
}

// WT: int64_t operator()(int i, int j) const -> the weight of edge {i, j} (symmetric; <= 0: no edge)
template <class WT>
struct Match {
    St s;
    const WT wt;
    int n, qh, qt, nfree, err;

    TDM_HD Match(const St &st, const WT &w, int nv) : s(st), wt(w), n(nv), qh(0), qt(0), nfree(0), err(0) {}

    TDM_HD int64_t slack(int v, int w) const { return s.dual[v] + s.dual[w] - 2 * wt(v, w); }
    TDM_HD int64_t slackc(int e) const { return slack(E0(e), E1(e)); }

    TDM_HD void push(int v)
    {
        if (qt >= 2 * n) {
            err |= ERR_STATE;
            return;
        }
        s.queue[qt++] = v;
    }

    // every leaf of top-level blossom b joins the queue (vertex order)
    TDM_HD void queue_leaves(int b)
    {
        if (b < n) {
            push(b);
            return;
        }
        for (int u0 = 0; u0 < n; u0 += W) {
            const int u = u0 + lane();
            const bool p = u < n && s.inb[u] == b;
            const uint64_t m = ballot(p);
            if (qt + popc(m) > 2 * n) {
                err |= ERR_STATE;
                return;
            }
            if (p) s.queue[qt + popc(below(m))] = u;
            qt += popc(m);
        }
        wsync();
    }

    TDM_HD void assign_label(int w, int t, int v)
    {
        for (int it = 0; it < 2; it++) {
            const int b = s.inb[w];
            const int e = v >= 0 ? E(v, w) : -1;
            s.label[w] = s.label[b] = t;
            s.lend[w] = s.lend[b] = e;
            s.best[w] = s.best[b] = -1;
            if (t == 1) {
                queue_leaves(b);
                return;
            }
            const int bs = s.base[b];   // a T-blossom's base is matched: its mate becomes S
            if (bs < 0 || s.mate[bs] < 0) {
                err |= ERR_STATE;
                return;
            }
            w = s.mate[bs];
            v = bs;
            t = 1;
        }
    }

    // trace back from v and w: the base of the new blossom, or -1 when the two roots differ (augmenting path)
    TDM_HD int scan_blossom(int v, int w)
    {
        int np = 0, base = -1;
        while (v != -1) {
            int b = s.inb[v];
            if (s.label[b] & 4) {
                base = s.base[b];
                break;
            }
            if (np >= n) {
                err |= ERR_CAP;
                break;
            }
            s.pathb[np++] = b;
            s.label[b] = 5;
            if (s.lend[b] == -1) {
                v = -1;
            } else {
                v = E0(s.lend[b]);
                b = s.inb[v];
                v = E0(s.lend[b]);
            }
            if (w != -1) {
                const int t = v;
                v = w;
                w = t;
            }
        }
        for (int k = 0; k < np; k++) s.label[s.pathb[k]] = 1;
        return base;
    }

    TDM_HD void add_blossom(int base, int v, int w)
    {
        const int bb = s.inb[base], bv = s.inb[v], bw = s.inb[w];
        if (nfree <= 0) {
            err |= ERR_STATE;
            return;
        }
        const int b = s.freeb[--nfree];
        s.base[b] = base;
        s.par[b] = -1;
        s.par[bb] = b;
        int x = bv, succ = bw, e = E(v, w), g = 0;
        for (;; g++) {   // v's side: from bv back to the base child
            s.nxt[x] = succ;
            s.ced[x] = e;
            s.prv[succ] = x;
            if (x == bb) break;
            if (g > 2 * n) {
                err |= ERR_CAP;
                return;
            }
            s.par[x] = b;
            e = s.lend[x];
            succ = x;
            x = s.inb[E0(e)];
        }
        for (x = bw, g = 0; x != bb; g++) {   // w's side
            if (g > 2 * n) {
                err |= ERR_CAP;
                return;
            }
            s.par[x] = b;
            const int ex = s.lend[x], y = s.inb[E0(ex)];
            s.nxt[x] = y;
            s.ced[x] = flip(ex);
            s.prv[y] = x;
            x = y;
        }
        s.head[b] = bb;
        s.label[b] = 1;
        s.lend[b] = s.lend[bb];
        s.dual[b] = 0;
        // leaves move into b; the T ones join the queue; tmp = the leaf list
        int nl = 0;
        for (int u0 = 0; u0 < n; u0 += W) {
            const int u = u0 + lane();
            bool in = false, wasT = false;
            if (u < n) {
                const int ib = s.inb[u];
                in = s.par[ib] == b;
                wasT = in && s.label[ib] == 2;
            }
            const uint64_t mq = ballot(wasT), ml = ballot(in);
            if (qt + popc(mq) > 2 * n) {
                err |= ERR_STATE;
                return;
            }
            if (wasT) s.queue[qt + popc(below(mq))] = u;
            if (in) {
                s.tmp[nl + popc(below(ml))] = u;
                s.inb[u] = b;
            }
            qt += popc(mq);
            nl += popc(ml);
        }
        TDM_COUNT(blossom_formed);
        TDM_MAX(leaves_max, nl);
        x = bb;
        g = 0;
        do {
            s.best[x] = -1;
            x = s.nxt[x];
        } while (x != bb && ++g <= 2 * n);
        wsync();
        // least-slack edge from b to another S-blossom, over every leaf
        uint64_t key = NONE;
        for (int w0 = 0; w0 < n; w0 += W) {
            const int ww = w0 + lane();
            if (ww < n) {
                const int bx = s.inb[ww];
                if (bx != b && s.label[bx] == 1)
                    for (int k = 0; k < nl; k++) {
                        const int u = s.tmp[k];
                        if (wt(u, ww) > 0) {
                            const uint64_t kk = pack(slack(u, ww), E(u, ww));
                            key = kk < key ? kk : key;
                        }
                    }
            }
        }
        key = wmin(key);
        s.best[b] = key == NONE ? -1 : (int)(key & M24);
    }

    TDM_HD void free_blossom(int x)
    {
        s.label[x] = 0;
        s.lend[x] = -1;
        s.best[x] = -1;
        s.par[x] = -1;
        s.base[x] = -1;
        s.head[x] = -1;
        s.dual[x] = 0;
        s.freeb[nfree++] = x;
    }

    // the blossoms under b (b itself included) flip their matching so that vertex v becomes b's base
    TDM_HD void augment_blossom(int b0, int v0)
    {
        int sp = 0;
        s.stk[sp++] = b0 << 12 | v0;
        while (sp > 0) {
            const int it = s.stk[--sp], b = it >> 12, v = it & 4095;
            int t = v, g = 0;
            while (s.par[t] != b) {
                t = s.par[t];
                if (t < 0 || ++g > 2 * n) {
                    err |= ERR_STATE;
                    return;
                }
            }
            TDM_COUNT(aug_blossom);
            if (t >= n) {
                s.stk[sp++] = t << 12 | v;
                TDM_COUNT(aug_nested);
            }
            int i = 0;
            for (int x = s.head[b]; x != t; x = s.nxt[x])
                if (++i > 2 * n) {
                    err |= ERR_STATE;
                    return;
                }
            const bool fwd = i & 1;
            if (i > 0) {
                if (fwd) TDM_COUNT(aug_fwd);
                else TDM_COUNT(aug_back);
            }
            for (int tc = t, g2 = 0; tc != s.head[b];) {
                if (++g2 > n) {
                    err |= ERR_CAP;
                    return;
                }
                int t1, t2, wv, xv;
                if (fwd) {
                    t1 = s.nxt[tc];
                    const int e = s.ced[t1];
                    wv = E0(e);
                    xv = E1(e);
                    t2 = s.nxt[t1];
                } else {
                    t1 = s.prv[tc];
                    const int e = s.ced[s.prv[t1]];
                    xv = E0(e);
                    wv = E1(e);
                    t2 = s.prv[t1];
                }
                if (sp + 2 > n) {
                    err |= ERR_CAP;
                    return;
                }
                if (t1 >= n) s.stk[sp++] = t1 << 12 | wv;
                if (t2 >= n) s.stk[sp++] = t2 << 12 | xv;
                s.mate[wv] = xv;
                s.mate[xv] = wv;
                tc = t2;
            }
            s.head[b] = t;
            s.base[b] = v;
        }
    }

    TDM_HD void augment_matching(int v, int w)
    {
        TDM_COUNT(augmentations);
        for (int side = 0; side < 2; side++) {
            int sv = side ? w : v, j = side ? v : w;
            for (int g = 0;; g++) {
                if (g > n) {
                    err |= ERR_CAP;
                    return;
                }
                const int bs = s.inb[sv];
                if (bs >= n) augment_blossom(bs, sv);
                s.mate[sv] = j;
                if (s.lend[bs] == -1) break;
                const int t = E0(s.lend[bs]), bt = s.inb[t], e = s.lend[bt];
                sv = E0(e);
                j = E1(e);
                if (bt >= n) augment_blossom(bt, j);
                s.mate[j] = sv;
            }
        }
    }

    TDM_HD int step(int x, bool fwd) const { return fwd ? s.nxt[x] : s.prv[x]; }

    TDM_HD void expand_blossom(int b, bool endstage)
    {
        // children become top-level (at the end of a stage, zero-dual sub-blossoms are expanded as well)
        int sp = 0;
        s.stk[sp++] = b;
        if (endstage) TDM_COUNT(expand_end);
        while (sp > 0) {
            const int x = s.stk[--sp];
            int c = s.head[x], g = 0;
            do {
                s.par[c] = -1;
                if (endstage && c >= n && s.dual[c] == 0) {
                    if (sp >= n) {
                        err |= ERR_CAP;
                        return;
                    }
                    s.stk[sp++] = c;
                }
                c = s.nxt[c];
            } while (c != s.head[x] && ++g <= 2 * n);
            if (x != b) {
                free_blossom(x);
                TDM_COUNT(expand_end_nested);
            }
        }
        for (int u0 = 0; u0 < n; u0 += W) {
            const int u = u0 + lane();
            if (u < n && s.inb[u] == b) {
                int x = u;
                for (int g = 0; s.par[x] != -1 && g <= 2 * n; g++) x = s.par[x];
                s.inb[u] = x;
            }
        }
        wsync();
        if (!endstage && s.label[b] == 2) {   // relabel the sub-blossoms of an expanded T-blossom
            const int entry = s.inb[E1(s.lend[b])];
            int j = 0;
            for (int x = s.head[b]; x != entry; x = s.nxt[x])
                if (++j > 2 * n) {
                    err |= ERR_STATE;
                    return;
                }
            const bool fwd = j & 1;
            TDM_COUNT(expand_T);
            TDM_MAX(relabel_steps_max, j);
            if (j > 0) {
                if (fwd) TDM_COUNT(relabel_fwd);
                else TDM_COUNT(relabel_back);
            }
            int v = E0(s.lend[b]), w = E1(s.lend[b]), tc = entry, g = 0;
            while (tc != s.head[b] && !err) {
                const int q = fwd ? E1(s.ced[tc]) : E0(s.ced[s.prv[tc]]);
                s.label[w] = 0;
                s.label[q] = 0;
                assign_label(w, 2, v);
                const int t1 = step(tc, fwd);
                if (fwd) {
                    v = E0(s.ced[t1]);
                    w = E1(s.ced[t1]);
                } else {
                    w = E0(s.ced[s.prv[t1]]);
                    v = E1(s.ced[s.prv[t1]]);
                }
                tc = step(t1, fwd);
                if (++g > 2 * n) err |= ERR_CAP;
            }
            const int bw = tc;
            s.label[w] = s.label[bw] = 2;
            s.lend[w] = s.lend[bw] = E(v, w);
            s.best[bw] = -1;
            g = 0;
            for (int x = step(bw, fwd); x != entry && !err; x = step(x, fwd)) {
                if (++g > 2 * n) {
                    err |= ERR_CAP;
                    break;
                }
                if (s.label[x] == 1) continue;   // got S through a neighbour already
                int rv = -1;
                if (x < n) {
                    rv = s.label[x] != 0 ? x : -1;
                } else {
                    uint64_t k = NONE;
                    for (int u0 = 0; u0 < n; u0 += W) {
                        const int u = u0 + lane();
                        if (u < n && s.inb[u] == x && s.label[u] != 0) k = k < (uint64_t)u ? k : (uint64_t)u;
                    }
                    k = wmin(k);
                    rv = k == NONE ? -1 : (int)k;
                }
                if (rv >= 0) {   // a vertex reached from outside: the sub-blossom becomes T
                    if (x < n) TDM_COUNT(sub_vertex_T);
                    else TDM_COUNT(sub_blossom_T);
                    s.label[rv] = 0;
                    s.label[s.mate[s.base[x]]] = 0;
                    assign_label(rv, 2, E0(s.lend[rv]));
                }
            }
        }
        free_blossom(b);
    }

    // scan the row of S-vertex v; returns true after an augmentation
    TDM_HD bool scan(int v)
    {
        for (int w0 = 0; w0 < n; w0 += W) {
            const int w = w0 + lane();
            bool tight = false;
            if (w < n && w != v && s.inb[w] != s.inb[v]) {
                const int64_t wv = wt(v, w);
                tight = wv > 0 && s.dual[v] + s.dual[w] - 2 * wv <= 0;
            }
            uint64_t m = ballot(tight);
            while (m && !err) {
                const int k = __builtin_ctzll(m);
                m &= m - 1;
                const int ww = w0 + k, bw = s.inb[ww];
                if (bw == s.inb[v]) continue;
                if (s.label[bw] == 0) {
                    assign_label(ww, 2, v);
                } else if (s.label[bw] == 1) {
                    const int base = scan_blossom(v, ww);
                    if (base >= 0) {
                        add_blossom(base, v, ww);
                    } else {
                        augment_matching(v, ww);
                        return true;
                    }
                } else if (s.label[ww] == 0) {   // inside a T-blossom: mark it reached
                    s.label[ww] = 2;
                    s.lend[ww] = E(v, ww);
                    TDM_COUNT(reach_in_T);
                }
            }
        }
        // edges that are not tight, with the labels as they are now
        const int bv = s.inb[v];
        uint64_t key = NONE;
        for (int w0 = 0; w0 < n; w0 += W) {
            const int w = w0 + lane();
            if (w < n && w != v) {
                const int bw = s.inb[w];
                const int64_t wv = wt(v, w);
                if (wv > 0 && bw != bv) {
                    const int64_t sl = s.dual[v] + s.dual[w] - 2 * wv;
                    if (sl > 0) {
                        if (s.label[bw] == 1) {
                            const uint64_t kk = pack(sl, E(v, w));
                            key = kk < key ? kk : key;
                        } else if (s.label[w] == 0) {
                            const int be = s.best[w];
                            if (be < 0 || sl < slackc(be)) s.best[w] = E(v, w);
                        }
                    }
                }
            }
        }
        key = wmin(key);
        wsync();
        if (key != NONE) {
            const int be = s.best[bv];
            if (be < 0 || (int64_t)(key >> 24) < slackc(be)) s.best[bv] = (int)(key & M24);
        }
        return false;
    }

    // the whole solve; returns the error word (0 = done)
    TDM_HD int run()
    {
        const int n2 = 2 * n;
        int64_t maxw = 0;
        for (int i = 0; i < n; i++)
            for (int j = i + 1 + lane(); j < n; j += W) {
                const int64_t x = wt(i, j);
                maxw = x > maxw ? x : maxw;
            }
        maxw = (int64_t)~wmin(~(uint64_t)maxw);   // the max as the min of the complements (maxw >= 0)
        for (int x = lane(); x < n2; x += W) {
            const bool v = x < n;
            if (v) {
                s.mate[x] = -1;
                s.inb[x] = x;
            }
            s.par[x] = -1;
            s.base[x] = v ? x : -1;
            s.dual[x] = v ? maxw : 0;
            s.head[x] = -1;
            if (!v) s.freeb[x - n] = n2 - 1 - (x - n);
        }
        nfree = n;
        wsync();
        if (maxw <= 0) return 0;
        if (maxw >= ((int64_t)1 << 34)) return ERR_RANGE;
        for (int stage = 0; stage <= n + 1; stage++) {
            if (stage == n + 1) return ERR_CAP;
            for (int x = lane(); x < n2; x += W) {
                s.label[x] = 0;
                s.lend[x] = -1;
                s.best[x] = -1;
            }
            wsync();
            qh = qt = 0;
            for (int u0 = 0; u0 < n; u0 += W) {   // top-level blossoms with a free base: S, their leaves queued
                const int u = u0 + lane();
                bool p = false;
                if (u < n) {
                    const int b = s.inb[u];
                    p = s.mate[s.base[b]] < 0;
                    if (p) s.label[b] = 1;
                    if (p && s.mate[u] < 0) s.label[u] = 1;
                }
                const uint64_t m = ballot(p);
                if (p) s.queue[qt + popc(below(m))] = u;
                qt += popc(m);
            }
            wsync();
            bool aug = false;
            for (int sub = 0;; sub++) {
                if (sub > 4 * n + 8) return err | ERR_CAP;
                TDM_MAX(substage_max, sub);
                while (qh < qt && !aug && !err) aug = scan(s.queue[qh++]);
                if (err) return err;
                if (aug) break;
                // delta: 1 = min vertex dual, 2 = S-to-free edge, 3 = S-to-S edge (half), 4 = T-blossom dual
                uint64_t k1 = NONE, k2 = NONE, k3 = NONE, k4 = NONE;
                for (int x = lane(); x < n2; x += W) {
                    if (x < n) {
                        const uint64_t a = pack(s.dual[x], x);
                        k1 = a < k1 ? a : k1;
                        if (s.label[s.inb[x]] == 0 && s.best[x] >= 0) {
                            const uint64_t c = pack(slackc(s.best[x]), x);
                            k2 = c < k2 ? c : k2;
                        }
                    }
                    if (s.par[x] == -1 && s.base[x] >= 0) {
                        if (s.label[x] == 1 && s.best[x] >= 0) {
                            const uint64_t c = pack(slackc(s.best[x]), x);
                            k3 = c < k3 ? c : k3;
                        }
                        if (x >= n && s.label[x] == 2) {
                            const uint64_t c = pack(s.dual[x], x);
                            k4 = c < k4 ? c : k4;
                        }
                    }
                }
                k1 = wmin(k1);
                k2 = wmin(k2);
                k3 = wmin(k3);
                k4 = wmin(k4);
                int type = 1, arg = (int)(k1 & M24);
                int64_t delta = (int64_t)(k1 >> 24);
                if (k2 != NONE && (int64_t)(k2 >> 24) < delta) {
                    type = 2;
                    delta = (int64_t)(k2 >> 24);
                    arg = (int)(k2 & M24);
                }
                if (k3 != NONE) {
                    const int64_t sl = (int64_t)(k3 >> 24);
                    if (sl & 1) return err | ERR_STATE;   // integer weights keep S-S slacks even
                    if (sl / 2 < delta) {
                        type = 3;
                        delta = sl / 2;
                        arg = (int)(k3 & M24);
                    }
                }
                if (k4 != NONE && (int64_t)(k4 >> 24) < delta) {
                    type = 4;
                    delta = (int64_t)(k4 >> 24);
                    arg = (int)(k4 & M24);
                }
                if (delta < 0) return err | ERR_STATE;
                if (type == 1) TDM_COUNT(delta1);
                else if (type == 2) TDM_COUNT(delta2);
                else if (type == 3) TDM_COUNT(delta3);
                else TDM_COUNT(delta4);
                for (int x = lane(); x < n2; x += W) {
                    if (x < n) {
                        const int lb = s.label[s.inb[x]];
                        if (lb == 1) s.dual[x] -= delta;
                        else if (lb == 2) s.dual[x] += delta;
                    } else if (s.par[x] == -1 && s.base[x] >= 0) {
                        if (s.label[x] == 1) s.dual[x] += delta;
                        else if (s.label[x] == 2) s.dual[x] -= delta;
                    }
                }
                wsync();
                if (type == 1) break;
                qh = qt = 0;
                if (type == 2) {
                    const int e = s.best[arg];
                    int i = E0(e), j = E1(e);
                    if (s.label[s.inb[i]] == 0) i = j;
                    push(i);
                } else if (type == 3) {
                    push(E0(s.best[arg]));
                } else {
                    expand_blossom(arg, false);
                }
                if (err) return err;
            }
            if (!aug) break;
            for (int b = n; b < n2 && !err; b++)
                if (s.par[b] == -1 && s.base[b] >= 0 && s.label[b] == 1 && s.dual[b] == 0) expand_blossom(b, true);
            if (err) return err;
        }
        return err;
    }

    // certificate from the final state: every edge satisfies 2w <= y_i + y_j + sum z over the blossoms holding both,
    // matched edges are tight, y, z >= 0, unmatched y = 0; total = matched weight, bound = dual objective.  Leaves the
    // leaf count of blossom x in cnt[x].  Returns ERR_CERT on a violation.
    TDM_HD int certify(int64_t &total, int64_t &bound)
    {
        const int n2 = 2 * n;
        int bad = 0;
        for (int x = lane(); x < n2; x += W) {
            s.stamp[x] = -1;
            s.cnt[x] = 0;
        }
        wsync();
        int64_t tot = 0, ysum = 0;
        for (int u = lane(); u < n; u += W) {
            const int m = s.mate[u];
            if (m >= 0) {
                if (m >= n || s.mate[m] != u || wt(u, m) <= 0) bad = 1;
                else if (u < m) tot += wt(u, m);
            } else if (s.dual[u] != 0) {
                bad = 1;
            }
            if (s.dual[u] < 0) bad = 1;
            ysum += s.dual[u];
            int g = 0;
            for (int x = s.par[u]; x != -1 && g <= n2; x = s.par[x], g++) add_i32(&s.cnt[x], 1);
        }
        wsync();
        int64_t zsum = 0;
        for (int x = n + lane(); x < n2; x += W)
            if (s.base[x] >= 0) {
                if (s.dual[x] < 0) bad = 1;
                zsum += 2 * s.dual[x] * (s.cnt[x] / 2);
            }
        for (int i = 0; i < n; i++) {
            // i's ancestors: stamp = i, cum = sum of z over the node and its ancestors (z = 2 dual)
            int d = 0;
            for (int x = s.par[i]; x != -1 && d < n; x = s.par[x]) s.tmp[d++] = x;
            int64_t c = 0;
            for (int k = d - 1; k >= 0; k--) {
                const int x = s.tmp[k];
                c += 2 * s.dual[x];
                if (lane() == 0) {
                    s.stamp[x] = i;
                    s.cum[x] = c;
                }
            }
            wsync();
            for (int j = i + 1 + lane(); j < n; j += W) {
                const int64_t w = wt(i, j);
                if (w <= 0) continue;
                int x = s.par[j], g = 0;
                while (x != -1 && s.stamp[x] != i && g++ <= n2) x = s.par[x];
                const int64_t sl = s.dual[i] + s.dual[j] + (x == -1 ? 0 : s.cum[x]) - 2 * w;
                if (sl < 0 || (s.mate[i] == j && sl != 0)) bad = 1;
            }
            wsync();
        }
        tot = wsum(tot);
        const int64_t b2 = wsum(ysum) + wsum(zsum);
        total = tot;
        bound = b2 >> 1;
        return wor(bad) ? ERR_CERT : 0;
    }
};

}  // namespace tdm
