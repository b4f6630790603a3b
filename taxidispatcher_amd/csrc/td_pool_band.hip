// td_pool_band.hip — td_pool_n_banded: td_pool_n's answer with a plan buffer of a fixed size.
//
// td_pool_n stores every happy plan as a key, sorts them all and runs the greedy de-duplication once: its buffer must hold the
// whole list.  The key of td_pool_core.h (cost, p0, p1, p2, p3, drop-off order) is a mixed-radix number whose ascending order IS
// the reference's stable sort, and the sequential scan keeps a plan iff no EARLIER kept plan shares a request with it.  So the
// scan may run over consecutive key intervals ("bands") [lo, hi) in ascending order with the set of used requests carried
// from one band to the next, and a plan with a used member never has to be stored: the scan would skip it.
//
// Host loop (td_pool_n_banded): state = lo and the device bitmap used[n].
//   1. count   one enumeration pass histograms the live happy plans with key >= lo by cost (64-bit counters)
//   2. choose  the longest run of costs from the lowest non-empty one whose sum fits the buffer; where one cost alone does not
//              fit, the same pass histograms the next digit (p0, p1, ..) inside that prefix, until a value fits: one value of
//              digit p_{k-2} holds at most (n - k + 1) k! <= 24 n plans, and plan_buffer >= 24 n is required
//   3. enum    the same walk appends the live happy plans of [lo, hi) as keys; their number must be what the histogram said
//   4. scan    radix sort, then the chunked greedy with the bitmap loaded from and stored back to device memory; the kept plans
//              go straight to the records behind those of the earlier bands
//   5. lo = hi; count again (the requests just used remove plans)
//
// Kernels: k_band_enum<K, COUNT> (K = 2, 3: one thread per (p0, p1), the request table in LDS) and k_band_enum4<COUNT> (one
// thread per (p0, p1, p2)) are k_pooln_enum<K> / k_pooln_enum4's walks with the filter added: grid shape and the
// workgroup-uniform exits are theirs, a used p0 (or, for four, p1) lets the whole workgroup leave, the bitmap is staged in LDS
// for the per-lane tests.  Histogram and append are aggregated per wave: ballot, then one atomic per wave and distinct bin.
#include <hipcub/hipcub.hpp>

#include "td_common.h"
#include "td_pool_core.h"

using namespace td;

namespace {

constexpr int PB_BINS = PN_MAXCOST + 1;        // histogram bins: a cost (level 0) or a request (levels 1 ..), n <= PN_MAXN < PB_BINS
constexpr int PB_WORDS = (PN_MAXN + 32) / 32;  // the used bitmap
constexpr unsigned long long PB_END = ~0ull;   // above every key: the largest is (PN_MAXCOST << 50) | (seq < 2^50)

struct BandCtl {
    unsigned long long count;   // keys appended by the band pass
    unsigned long long bad;     // happy plans whose cost does not fit the key: counted for n_happy, never a bin or a key
    int err;                    // 1: there is such a plan
    int kept;                   // records written so far, all bands
    int n_used;                 // requests used so far
    int pad;
};

// what a pass filters by and where its plans go
struct BandArgs {
    unsigned long long klo, khi;        // the key interval [klo, khi)
    int level;                          // COUNT: the digit to histogram: 0 the cost, l >= 1 pick-up p[l - 1]
    unsigned long long cap;             // band pass: room in keys
    unsigned long long *keys;
    unsigned long long *hist;           // PB_BINS counters
    const unsigned int *used;           // PB_WORDS words
    BandCtl *ctl;
};

__device__ __forceinline__ bool pb_bit(const unsigned int *u, int x) { return (u[x >> 5] >> (x & 31)) & 1u; }

// One happy-or-not plan per lane of the wave that is here.  COUNT: histogram the lanes inside the interval, one atomic per
// distinct bin of the wave; else append their keys, one atomic per wave.
template <bool COUNT>
__device__ __forceinline__ void pb_sink(bool happy, int cost, const int *p, unsigned long long seq, const BandArgs &a, int lane)
{
    bool in = happy;
    if (happy && (cost > PN_MAXCOST || cost < 0)) {   // never a bin or a key
        atomicOr(&a.ctl->err, 1);
        if (COUNT) atomicAdd(&a.ctl->bad, 1ull);
        in = false;
    }
    const unsigned long long key = ((unsigned long long)(in ? cost : 0) << PN_SEQ_BITS) | seq;
    in = in && key >= a.klo && key < a.khi;
    unsigned long long m = __ballot(in);
    if (!m) return;
    if (COUNT) {
        const int bin = a.level == 0 ? cost : a.level == 1 ? p[0] : a.level == 2 ? p[1] : p[2];   // no indexed p[]: it stays in registers
        while (m) {
            const int leader = __ffsll((long long)m) - 1;
            const int b = __shfl(bin, leader);
            const unsigned long long same = __ballot(in && bin == b);
            if (lane == leader) atomicAdd(&a.hist[b], (unsigned long long)__popcll(same));
            m &= ~same;
        }
    } else {
        unsigned long long base = 0;
        const int leader = __ffsll((long long)m) - 1;
        if (lane == leader) base = atomicAdd(&a.ctl->count, (unsigned long long)__popcll(m));
        base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), leader) << 32) |
               (unsigned long long)(uint32_t)__shfl((int)(uint32_t)base, leader);
        if (in) {
            const unsigned long long idx = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (idx < a.cap) a.keys[idx] = key;
        }
    }
}

template <int K, bool COUNT>
__global__ __launch_bounds__(256) void k_band_enum(int n, const int32_t *__restrict__ from, const int32_t *__restrict__ to,
                                                   const int32_t *__restrict__ wait, const int32_t *__restrict__ loss,
                                                   const int32_t *__restrict__ dist, int S, int first0, int first1, BandArgs a)
{
    static_assert(K == 2 || K == 3, "pools of four have k_band_enum4");
    extern __shared__ int32_t sm[];
    int32_t *sf = sm, *st = sm + n, *sw = sm + 2 * n, *sl = sm + 3 * n;
    unsigned int *su = reinterpret_cast<unsigned int *>(sm + 4 * n);
    int p[4] = {0, 0, 0, 0};
    p[0] = first0 + blockIdx.y;
    if (p[0] >= first1 || pb_bit(a.used, p[0])) return;   // uniform: before the barrier
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        sf[i] = from[i];
        st[i] = to[i];
        sw[i] = wait[i];
        sl[i] = loss[i];
    }
    for (int i = threadIdx.x; i < PB_WORDS; i += blockDim.x) su[i] = a.used[i];
    __syncthreads();
    if (0 > sw[p[0]]) return;   // (pool_n.c:177 at level 0)
    constexpr int NP = K == 2 ? 2 : 6;
    const unsigned long long nn = (unsigned long long)n;
    const int lane = threadIdx.x & 63;
    const int p1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (p1 >= n || p1 == p[0] || pb_bit(su, p1)) return;
    p[1] = p1;
    const int d01 = pn_d(dist, S, sf[p[0]], sf[p1]);
    if (d01 > sw[p1]) return;           // pool_n.c:177-178
    auto emit = [&](int p2) {
        p[2] = p2;
        for (int qi = 0; qi < NP; qi++) {
            int q[4];
            pn_perm(K, qi, q);
            int cost = 0;
            const bool happy = pn_check<K>(p, q, sf, st, sl, dist, S, &cost);
            const unsigned long long seq = (((unsigned long long)p[0] * nn + p[1]) * nn + p2) * nn * 24ull + (unsigned long long)qi;
            pb_sink<COUNT>(happy, cost, p, seq, a, lane);
        }
    };
    if constexpr (K == 2) {
        emit(0);
    } else {
        for (int p2 = 0; p2 < n; p2++) {
            if (p2 == p[0] || p2 == p1 || pb_bit(su, p2)) continue;
            if (d01 + pn_d(dist, S, sf[p1], sf[p2]) > sw[p2]) continue;
            emit(p2);
        }
    }
}

template <bool COUNT>
__global__ __launch_bounds__(256) void k_band_enum4(int n, const int32_t *__restrict__ from, const int32_t *__restrict__ to,
                                                    const int32_t *__restrict__ wait, const int32_t *__restrict__ loss,
                                                    const int32_t *__restrict__ dist, int S, int first0, int first1, BandArgs a)
{
    __shared__ unsigned int su[PB_WORDS];
    int p[4];
    p[0] = first0 + blockIdx.z;
    p[1] = blockIdx.y;
    // uniform over the workgroup, all before the barrier
    if (p[0] >= first1 || p[1] == p[0] || 0 > wait[p[0]]) return;
    if (pb_bit(a.used, p[0]) || pb_bit(a.used, p[1])) return;
    const int d01 = pn_d(dist, S, from[p[0]], from[p[1]]);
    if (d01 > wait[p[1]]) return;   // pool_n.c:177-178
    for (int i = threadIdx.x; i < PB_WORDS; i += blockDim.x) su[i] = a.used[i];
    __syncthreads();
    const int p2 = blockIdx.x * blockDim.x + threadIdx.x;
    if (p2 >= n || p2 == p[0] || p2 == p[1] || pb_bit(su, p2)) return;
    const int d012 = d01 + pn_d(dist, S, from[p[1]], from[p2]);
    if (d012 > wait[p2]) return;
    p[2] = p2;
    const unsigned long long nn = (unsigned long long)n;
    const int lane = threadIdx.x & 63;
    const int f2 = from[p2];
    for (int p3 = 0; p3 < n; p3++) {
        if (p3 == p[0] || p3 == p[1] || p3 == p2 || pb_bit(su, p3)) continue;
        if (d012 + pn_d(dist, S, f2, from[p3]) > wait[p3]) continue;
        p[3] = p3;
        for (int qi = 0; qi < 24; qi++) {
            int q[4];
            pn_perm(4, qi, q);
            int cost = 0;
            const bool happy = pn_check<4>(p, q, from, to, loss, dist, S, &cost);
            const unsigned long long seq = ((((unsigned long long)p[0] * nn + p[1]) * nn + p2) * nn + p3) * 24ull + (unsigned long long)qi;
            pb_sink<COUNT>(happy, cost, p, seq, a, lane);
        }
    }
}

// k_pooln_greedy's chunked scan over one band's sorted keys, ONE workgroup: the used bitmap and the counts come from device
// memory and go back there, and a kept plan's record is written at once, behind the ctl->kept records of the earlier bands.
__global__ __launch_bounds__(1024) void k_band_greedy(int k, int n, unsigned long long count, const unsigned long long *__restrict__ keys,
                                                      int max_kept, int32_t *__restrict__ out, unsigned int *__restrict__ g_used,
                                                      BandCtl *__restrict__ ctl)
{
    extern __shared__ int sm[];
    int *owner = sm;                                                  // n: smallest live plan of the chunk claiming the request
    unsigned int *used = reinterpret_cast<unsigned int *>(sm + n);   // PB_WORDS
    __shared__ int s_live, s_nkept, s_nused, s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < n; i += 1024) owner[i] = INT_MAX;
    for (int i = tid; i < PB_WORDS; i += 1024) used[i] = g_used[i];
    if (tid == 0) {
        s_nkept = ctl->kept;
        s_nused = ctl->n_used;
    }
    __syncthreads();
    for (unsigned long long base = 0; base < count; base += 1024ull) {
        if (s_nused + k > n || s_nkept >= max_kept) break;   // no k unused requests left / output full
        const unsigned long long i = base + (unsigned long long)tid;
        int c[4] = {0, 0, 0, 0};
        unsigned long long key = 0;
        bool alive = false, taken = false;
        if (i < count) {
            key = keys[i];
            pn_key_requests(n, key, c);
            alive = true;
        }
        for (;;) {
            // a plan dies when one of its requests is used
            if (alive && !taken) {
                for (int a = 0; a < k; a++)
                    if (pb_bit(used, c[a])) alive = false;
            }
            const bool live = alive && !taken;
            if (tid == 0) s_live = 0;
            __syncthreads();
            if (live) {
                s_live = 1;
                for (int a = 0; a < k; a++) atomicMin(&owner[c[a]], tid);
            }
            __syncthreads();
            if (!s_live) break;
            bool win = live;
            if (live)
                for (int a = 0; a < k; a++) win = win && (owner[c[a]] == tid);
            __syncthreads();
            if (live)
                for (int a = 0; a < k; a++) owner[c[a]] = INT_MAX;
            if (win) {
                taken = true;
                for (int a = 0; a < k; a++) atomicOr(&used[c[a] >> 5], 1u << (c[a] & 31));
            }
            __syncthreads();
        }
        // ordered compaction of the chunk's taken plans, as records
        const unsigned long long m = __ballot(taken);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int off = s_nkept, tot = 0;
        for (int q = 0; q < 16; q++) {
            if (q < w) off += s_w[q];
            tot += s_w[q];
        }
        if (taken && off + before < max_kept) {
            int32_t *o = out + (size_t)(off + before) * (size_t)(2 * k + 1);
            int q[4];
            pn_perm(k, (int)((key & PN_SEQ_MASK) % 24ull), q);
            for (int a = 0; a < k; a++) {
                o[a] = c[a];
                o[k + a] = c[q[a]];
            }
            o[2 * k] = (int32_t)(key >> PN_SEQ_BITS);
        }
        __syncthreads();
        if (tid == 0) {
            s_nkept += tot;
            s_nused += tot * k;
        }
        __syncthreads();
    }
    for (int i = tid; i < PB_WORDS; i += 1024) g_used[i] = used[i];
    if (tid == 0) {
        ctl->kept = min(s_nkept, max_kept);
        ctl->n_used = s_nused;
    }
}

struct BandWs {
    Buf keys, keys2, tmp, ctl, out, in;
    void *pin = nullptr;   // pinned: BandCtl and the histogram as the host reads them (the context's block is smaller)
};
BandWs g_bw;

// the device block behind g_bw.ctl: BandCtl, the bitmap, the histogram; the host reads ctl and histogram in one copy
struct BandDev {
    unsigned int *used;
    BandCtl *ctl;
    unsigned long long *hist;
};
constexpr size_t PB_USED_BYTES = 256, PB_HEAD_BYTES = sizeof(BandCtl) + sizeof(unsigned long long) * PB_BINS;
static_assert(sizeof(unsigned int) * PB_WORDS <= PB_USED_BYTES && sizeof(BandCtl) % 8 == 0, "the block's layout");

struct Pass {
    int k, n, S, first0, first1;
    const int32_t *arr[4], *dist;
};

// one enumeration pass over the first pick-ups the interval allows; count: a histogram of `bins` bins comes home with the ctl
template <bool COUNT>
int band_pass(const Pass &ps, const BandDev &d, BandArgs a, int bins, BandCtl *h_ctl, const unsigned long long **h_hist)
{
    Ctx &c = ctx();
    const int k = ps.k, n = ps.n;
    int f0 = ps.first0, f1 = ps.first1;
    // inside one cost the interval bounds the first pick-up: the grid shrinks to it
    if (a.khi != PB_END && (a.klo >> PN_SEQ_BITS) == ((a.khi - 1) >> PN_SEQ_BITS)) {
        const unsigned long long w1 = (unsigned long long)n * n * n * 24ull;
        f0 = (int)std::max<unsigned long long>((unsigned long long)f0, (a.klo & PN_SEQ_MASK) / w1);
        f1 = (int)std::min<unsigned long long>((unsigned long long)f1, ((a.khi - 1) & PN_SEQ_MASK) / w1 + 1ull);
    }
    if (COUNT) TD_HIP(hipMemsetAsync(d.hist, 0, sizeof(unsigned long long) * (size_t)bins, c.stream));
    else TD_HIP(hipMemsetAsync(&d.ctl->count, 0, sizeof(unsigned long long), c.stream));
    if (f1 > f0) {
        ProfScope pscope(TD_K_LCM);
        const size_t shm = sizeof(int32_t) * 4 * (size_t)n + sizeof(unsigned int) * PB_WORDS;
        const dim3 g((n + 255) / 256, f1 - f0);
#define TD_PB(KV) \
    k_band_enum<KV, COUNT><<<g, 256, shm, c.stream>>>(n, ps.arr[0], ps.arr[1], ps.arr[2], ps.arr[3], ps.dist, ps.S, f0, f1, a)
        if (k == 2) TD_PB(2);
        else if (k == 3) TD_PB(3);
        else   // n <= PN_MAXN: both grid dimensions fit
            k_band_enum4<COUNT><<<dim3((n + 255) / 256, n, f1 - f0), 256, 0, c.stream>>>(n, ps.arr[0], ps.arr[1], ps.arr[2], ps.arr[3], ps.dist,
                                                                                          ps.S, f0, f1, a);
#undef TD_PB
        TD_HIP(hipGetLastError());
    }
    const size_t bytes = sizeof(BandCtl) + (COUNT ? sizeof(unsigned long long) * (size_t)bins : 0);
    TD_HIP(hipMemcpyAsync(g_bw.pin, d.ctl, bytes, hipMemcpyDeviceToHost, c.stream));
    TD_HIP(hipStreamSynchronize(c.stream));
    *h_ctl = *(const BandCtl *)g_bw.pin;
    if (h_hist) *h_hist = (const unsigned long long *)((const char *)g_bw.pin + sizeof(BandCtl));
    return TD_OK;
}

}  // namespace

void td::pool_band_release_workspace()
{
    Buf *bs[] = {&g_bw.keys, &g_bw.keys2, &g_bw.tmp, &g_bw.ctl, &g_bw.out, &g_bw.in};
    for (Buf *b : bs) buf_free(*b);
    if (g_bw.pin) (void)hipHostFree(g_bw.pin);
    g_bw.pin = nullptr;
}

extern "C" int td_pool_n_banded(int k, int n, const int32_t *from, const int32_t *to, const int32_t *max_wait,
                                const int32_t *max_loss, const int32_t *dist, int S, int first0, int first1,
                                int64_t plan_buffer, int max_pools, int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *stats)
{
    TD_REQUIRE_INIT();
    Ctx &c = ctx();
    if (k < 2 || k > 4) return fail(TD_EINVAL, "pool size %d (2..4)", k);
    if (n < 0 || n > PN_MAXN) return fail(TD_EINVAL, "n=%d (at most %d requests; the reference's MAX_DEMAND is 2000)", n, PN_MAXN);
    if (!n_pools || (max_pools > 0 && !pools)) return fail(TD_EINVAL, "null output");
    if (dist && S <= 0) return fail(TD_EINVAL, "dist given but S=%d", S);
    if (plan_buffer <= 0) plan_buffer = 1 << 22;
    plan_buffer = std::min<int64_t>(plan_buffer, (int64_t)1 << 30);   // the sort counts in int; no list of n <= 2047 needs more per band
    if (plan_buffer < (int64_t)24 * n)
        return fail(TD_EINVAL, "td_pool_n_banded: plan_buffer = %lld below 24 * n = %lld", (long long)plan_buffer, 24ll * n);
    *n_pools = 0;
    if (n_happy) *n_happy = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    first0 = std::max(first0, 0);
    first1 = std::min(first1, n);
    if (n < k || first1 <= first0 || max_pools <= 0) return TD_OK;
    if (!from || !to || !max_wait || !max_loss) return fail(TD_EINVAL, "null request array");
    if (!g_bw.pin) TD_HIP(hipHostMalloc(&g_bw.pin, PB_HEAD_BYTES, hipHostMallocDefault));
    max_pools = std::min(max_pools, n / k);   // pools share no request
    int rc;
    // stage the four request arrays (and the table)
    if ((rc = ensure(g_bw.in, sizeof(int32_t) * 4 * (size_t)n))) return rc;
    const int32_t *src[4] = {from, to, max_wait, max_loss};
    Pass ps{k, n, S, first0, first1, {nullptr, nullptr, nullptr, nullptr}, nullptr};
    for (int q = 0; q < 4; q++) {
        if (is_device_ptr(src[q])) ps.arr[q] = src[q];
        else {
            int32_t *dst = (int32_t *)g_bw.in.p + (size_t)q * n;
            TD_HIP(hipMemcpyAsync(dst, src[q], sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c.stream));
            ps.arr[q] = dst;
        }
    }
    const void *d_dist = nullptr;
    if (dist && (rc = to_device(dist, sizeof(int32_t) * (size_t)S * S, c.stage_c, &d_dist))) return rc;
    ps.dist = (const int32_t *)d_dist;
    if ((rc = ensure(g_bw.keys, sizeof(unsigned long long) * (size_t)plan_buffer))) return rc;
    if ((rc = ensure(g_bw.keys2, sizeof(unsigned long long) * (size_t)plan_buffer))) return rc;
    if ((rc = ensure(g_bw.ctl, PB_USED_BYTES + PB_HEAD_BYTES))) return rc;
    BandDev d;
    d.used = (unsigned int *)g_bw.ctl.p;
    d.ctl = (BandCtl *)((char *)g_bw.ctl.p + PB_USED_BYTES);
    d.hist = (unsigned long long *)(d.ctl + 1);
    TD_HIP(hipMemsetAsync(g_bw.ctl.p, 0, PB_USED_BYTES + sizeof(BandCtl), c.stream));   // nothing used, nothing kept
    const size_t ob = sizeof(int32_t) * (size_t)max_pools * (size_t)(2 * k + 1);
    int32_t *d_out = pools;
    if (!is_device_ptr(pools)) {
        if ((rc = ensure(g_bw.out, ob))) return rc;
        d_out = (int32_t *)g_bw.out.p;
    }
    // digit weights of the sequence number: p0, p1, p2, p3
    const unsigned long long nn = (unsigned long long)n;
    const unsigned long long wgt[5] = {0, nn * nn * nn * 24ull, nn * nn * 24ull, nn * 24ull, 24ull};
    const unsigned long long room = (unsigned long long)plan_buffer;
    unsigned long long lo = 0;
    int64_t bands = 0, passes = 0, deepest = 0, most = 0;
    int kept = 0;
    BandArgs a{0, PB_END, 0, room, (unsigned long long *)g_bw.keys.p, d.hist, d.used, d.ctl};
    for (bool first = true;; first = false) {
        // 1. the live happy plans from lo on, by cost
        BandCtl h;
        const unsigned long long *hist = nullptr;
        a.klo = lo, a.khi = PB_END, a.level = 0;
        if ((rc = band_pass<true>(ps, d, a, PB_BINS, &h, &hist))) return rc;
        passes++;
        unsigned long long sum = 0;
        for (int b = 0; b < PB_BINS; b++) sum += hist[b];
        if (first) {
            if (n_happy) *n_happy = (int64_t)sum;
            if (n_happy) *n_happy += (int64_t)h.bad;
            if (h.err) return fail(TD_ERANGE, "td_pool_n_banded: a plan cost does not fit 14 bits");
        }
        kept = h.kept;
        if (sum == 0 || n - h.n_used < k || kept >= max_pools) break;
        // 2. the band: the longest run from the lowest non-empty value that fits, one digit deeper where a single value does not
        int level = 0, bins = PB_BINS;
        unsigned long long prefix = 0, hi = PB_END, expect = 0;   // prefix: the key of the digits fixed so far
        for (;;) {
            int b0 = 0;
            while (b0 < bins && hist[b0] == 0) b0++;
            if (b0 == bins) return fail(TD_EINTERNAL, "td_pool_n_banded: an empty histogram at level %d", level);
            if (hist[b0] <= room) {
                int b1 = b0;
                while (b1 < bins && expect + hist[b1] <= room) expect += hist[b1++];
                if (level == 0) hi = b1 == PB_BINS ? PB_END : (unsigned long long)b1 << PN_SEQ_BITS;
                else hi = prefix + (unsigned long long)b1 * wgt[level];
                break;
            }
            if (level == k - 1)
                return fail(TD_EINTERNAL, "td_pool_n_banded: %llu plans behind one value of the last digit but one", hist[b0]);
            prefix += level == 0 ? (unsigned long long)b0 << PN_SEQ_BITS : (unsigned long long)b0 * wgt[level];
            level++;
            a.klo = std::max(lo, prefix), a.khi = prefix + nn * wgt[level], a.level = level, bins = n;
            if ((rc = band_pass<true>(ps, d, a, bins, &h, &hist))) return rc;
            passes++;
        }
        deepest = std::max<int64_t>(deepest, level);
        // 3. its keys
        a.klo = lo, a.khi = hi, a.level = 0;
        if ((rc = band_pass<false>(ps, d, a, 0, &h, nullptr))) return rc;
        passes++;
        if (h.count != expect)
            return fail(TD_EINTERNAL, "td_pool_n_banded: %llu keys in a band, %llu by its histogram", h.count, expect);
        most = std::max<int64_t>(most, (int64_t)expect);
        // 4. sort and scan
        size_t bytes = 0;
        unsigned long long *k_in = (unsigned long long *)g_bw.keys.p, *k_out = (unsigned long long *)g_bw.keys2.p;
        TD_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, k_in, k_out, (int)expect, 0, 64, c.stream));
        if ((rc = ensure(g_bw.tmp, bytes + 256))) return rc;
        TD_HIP(hipcub::DeviceRadixSort::SortKeys(g_bw.tmp.p, bytes, k_in, k_out, (int)expect, 0, 64, c.stream));
        const size_t shm = sizeof(int) * (size_t)n + sizeof(unsigned int) * PB_WORDS;
        k_band_greedy<<<1, 1024, shm, c.stream>>>(k, n, expect, k_out, max_pools, d_out, d.used, d.ctl);
        TD_HIP(hipGetLastError());
        bands++;
        // 5.
        if (hi == PB_END) {   // nothing lies above: the next count would be empty
            TD_HIP(hipMemcpyAsync(g_bw.pin, d.ctl, sizeof(BandCtl), hipMemcpyDeviceToHost, c.stream));
            TD_HIP(hipStreamSynchronize(c.stream));
            kept = ((const BandCtl *)g_bw.pin)->kept;
            break;
        }
        lo = hi;
    }
    if (kept > 0 && d_out != pools) {
        TD_HIP(hipMemcpyAsync(pools, d_out, sizeof(int32_t) * (size_t)kept * (size_t)(2 * k + 1), hipMemcpyDeviceToHost, c.stream));
        TD_HIP(hipStreamSynchronize(c.stream));
    }
    *n_pools = kept;
    if (stats) stats[0] = bands, stats[1] = passes, stats[2] = deepest, stats[3] = most;
    return TD_OK;
}
