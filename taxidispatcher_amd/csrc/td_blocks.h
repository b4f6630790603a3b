// td_blocks.h — included by td_assign.hip (inside its anonymous namespace, after k_assign / build_free_list).
//
// BLOCK-LOCAL START of a solve with 1-byte cells ("phase A") and the TWO-HOP AUGMENTATION on tight
// cells.  Both exist for the row-sharded solve of SURVEY §8e (N = 65 536 over 8 GPUs): every exchange step between
// ranks costs tens of microseconds, and the plain sequence (one MAX all-reduce of the bid keys per bidding round,
// twelve rounds, a serial finisher on rank 0) spends more time in exchanges and in the serial tail than in the
// streaming passes that actually shard.
//
// Phase A needs NO exchange.  The matrix is cut into V diagonal blocks: block b = rows [b*rpb, (b+1)*rpb) x columns
// [b*rpb, (b+1)*rpb) (rpb = n / V; a rank owns whole blocks).  Inside its block a row may only take a column whose
// reduced cell is 0 at price 0 ("zero cell").  Such a pair is tight whatever happens elsewhere (reduced cells and
// prices are >= 0, so 0 is the row's minimum), no price moves, and nobody outside the block looks at the block's
// columns — so ANY matching on the zero cells of the diagonal blocks is a valid starting state of the auction
// (complementary slackness exact, all prices 0), found without a word exchanged:
//   round 0      the 1-byte compress pass writes every row's first zero cell of its own column slice in the row's
//                rotated order (k_compress_reg<.., BID0> with zs_rpb > 0), k_zs_assign resolves the columns;
//   rounds 1..R  k_zs_bid (one wave per free row, 1/V of the row is read) + k_zs_assign: a free column is
//                preferred, else the row takes an owned zero column and the evicted row bids again (the tie eviction
//                of k_bid, restricted to the block);
//   two hops     k_hop_*: what the rounds leave free (a few dozen rows per block) is matched through paths
//                free row i -> tight column j -> its owner r' -> FREE column j' tight for r'.  On tie-heavy
//                instances (perf.jl: n / 31 zero cells per row) nearly every (i, j') pair is connected this way.
// After phase A the ranks exchange their owner slices ONCE (all-gather) and the ordinary global rounds and the
// finisher take whatever is still free — on the perf.jl instance nothing.
//
// The two-hop kernels are written for general prices (tight = reduced cost 0 against the row's dual), windowed to a
// block's columns only in phase A, where the zero-cell rule stands in for the row minimum.
//   k_hop_lists  per block: the free rows / free columns (block-relative, ordered), at most HOP_FMAX of each used
//   k_hop_table  per free row i (one workgroup): tab[i][b] = the smallest r' such that col(r') is tight for i and
//                free column b is tight for r' (c[r'][j'] + p[j'] equals c[r'][col(r')] + p[col(r')], the row's dual by
//                complementary slackness; tested for the rows r' the free row reaches: nobody reads anyone else's).
//                atomicMin in LDS, or per (row, segment) straight into the table: independent of scheduling
//   k_hop_match  per block (one workgroup, the walk in one wave): rows in order take the first free column in their
//                rotated order whose r' is still unused; then i -> col(r'), r' -> j' is rewired.  Deterministic.
// Nothing here changes a price, so every pair it creates is tight and the finishers' invariant holds.

// HOP_FMAX (free rows / columns of a block the two-hop pass looks at) and HOP_BMAX (blocks per shard) are defined
// with the tunables at the top of td_assign.hip.

struct HopCtl {                 // device words of the pass (one per shard)
    int nfr[HOP_BMAX], nfc[HOP_BMAX];   // free rows / columns per local block (true counts)
    int left;                           // free rows the pass left (over all local blocks)
    int matched;
    int pad[2];
};

__device__ __forceinline__ uint32_t zs_zero_bytes(uint32_t w)   // 0x80 in every byte of w that is zero (exact, no borrow)
{
    return ~(((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w | 0x7F7F7F7Fu);
}

// The kernels of the chain behind the compress pass start on cold lines (the kernel before them ran on other XCDs), so
// what they cost is the number of DEPENDENT global round trips, not the bytes.  Each of them therefore issues the width
// flag, its gate and its counts TOGETHER with the first data loads whose addresses depend on kernel arguments and ids
// only, and tests them afterwards.  Such a load is in bounds whatever flag, gate and counts say (indices are clamped),
// no store and no atomic stands in front of the tests, and a load whose address comes from a loaded value stays behind
// that value's test.  Left to itself the compiler moves a load whose value is used on one side of a branch only back
// behind the branch (and waits for the flag first): an empty `asm volatile` that names ALL the values of the group as
// operands ("s" scalar, "v" vector register) stands between the loads and the tests, so every load is issued in front
// of it and the one wait is there.  Where a loop stands between a flag load and its test the flag is read with a relaxed
// atomic load, which stays where it is written and waits only at its use.

// ---- phase A, rounds >= 1: one WAVE per free row, zero cells of the row's own column slice only
// ob[j] = 1 once column j has an owner (phase A never changes a price: all are 0)
// A wave takes one row (nrows / 4 workgroups, one trip); its r2c word is loaded with the width flag, in front.  The lanes
// stride over the cpb = rpb / 16 chunks of the slice, two chunks a lane and trip with all four loads issued together (an
// index past the end is clamped to the last chunk: the same candidate twice).  No LDS, no barrier: the minimum is the
// shuffle ladder's, lane 0 issues the atomicMax.  The key a row writes is a pure function of the row, the round, cc and ob
// (the smallest `owned << 24 | rotated position` over the slice), so any partition of the rows over waves and of the
// chunks over lanes gives the keys of one workgroup per row.  (Two consecutive rows per wave in half as many workgroups,
// their r2c words loaded together: 8.1 / 6.2 / 5.4 / 4.7 us for the four rounds of a g1 step against 7.0 / 4.4 / 4.4 / 4.5.)
__global__ __launch_bounds__(256) void k_zs_bid(int nrows, int row0, int nchunks, int rpb, const uint8_t *__restrict__ cc,
                                                const uint8_t *__restrict__ ob, const int *__restrict__ r2c,
                                                unsigned long long *__restrict__ bid, const int *__restrict__ ctl, int round,
                                                int tie_evict)
{
    const int lane = threadIdx.x & 63;
    const int lrow = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int flag = ctl[CTL_FLAG], col = r2c[min(lrow, nrows - 1)];
    asm volatile("" :: "s"(flag), "s"(col));
    if (flag || lrow >= nrows || col != -1) return;   // uniform
    const int cpb = rpb >> 4;
    const size_t pitch = (size_t)nchunks * 16;
    const int row = row0 + lrow;
    const int c0 = (row / rpb) * cpb;   // first chunk of the row's column slice
    const uint32_t hsh = ((uint32_t)row + 1u) * 0x9E3779B1u + (uint32_t)round * 0x85EBCA6Bu;
    const int rot = (int)(((uint64_t)(hsh ^ (hsh >> 15)) * (uint64_t)cpb) >> 32);
    const uint8_t *rp = cc + (size_t)lrow * pitch;
    int best = INT_MAX;   // owned << 24 | rotated cell position
    for (int t0 = lane; t0 < cpb; t0 += 128) {
        int t[2] = {t0, min(t0 + 64, cpb - 1)};
        uint4 cv[2], ov[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            int ch = t[u] + rot;
            if (ch >= cpb) ch -= cpb;
            ch += c0;
            cv[u] = *reinterpret_cast<const uint4 *>(rp + (size_t)ch * 16);
            ov[u] = *reinterpret_cast<const uint4 *>(ob + (size_t)ch * 16);
        }
        // (else a word of ob is loaded again behind the test of its cells: a second round trip)
        asm volatile("" :: "v"(cv[0].x), "v"(cv[0].y), "v"(cv[0].z), "v"(cv[0].w), "v"(ov[0].x), "v"(ov[0].y), "v"(ov[0].z), "v"(ov[0].w),
                     "v"(cv[1].x), "v"(cv[1].y), "v"(cv[1].z), "v"(cv[1].w), "v"(ov[1].x), "v"(ov[1].y), "v"(ov[1].z), "v"(ov[1].w));
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const uint32_t cw[4] = {cv[u].x, cv[u].y, cv[u].z, cv[u].w}, ow[4] = {ov[u].x, ov[u].y, ov[u].z, ov[u].w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t z = zs_zero_bytes(cw[q]);
                if (!z) continue;
                const uint32_t zf = z & zs_zero_bytes(ow[q]);   // zero cell in a free column
                const uint32_t pick = zf ? zf : z;
                const int cand = (zf ? 0 : (1 << 24)) | (t[u] * 16 + q * 4 + (__builtin_ctz(pick) >> 3));
                best = min(best, cand);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    if (lane == 0 && best != INT_MAX) {
        const bool owned = (best >> 24) != 0;
        const int pos = best & 0xFFFFFF;
        int ch = (pos >> 4) + rot;
        if (ch >= cpb) ch -= cpb;
        const int j = (c0 + ch) * 16 + (pos & 15);
        if (!owned || tie_evict) atomicMax(&bid[j], (unsigned long long)(row + 1));   // price 0: the key is the row
    }
}

// ---- phase A: resolve the bids on the columns [col_lo, col_hi) of this shard's blocks (prices stay 0)
// the flag, the bid and the column's owner are one round trip
__global__ __launch_bounds__(256) void k_zs_assign(int col_lo, int col_hi, int nrows, int row0, unsigned long long *__restrict__ bid,
                                                   int32_t *__restrict__ pk, int *__restrict__ owner, int *__restrict__ r2c,
                                                   uint8_t *__restrict__ ob, const int *__restrict__ ctl)
{
    const int j = col_lo + blockIdx.x * blockDim.x + threadIdx.x;
    const int jc = min(j, col_hi - 1);
    int flag = ctl[CTL_FLAG];
    unsigned long long k = bid[jc];
    int old = owner[jc];
    asm volatile("" :: "s"(flag), "v"(k), "v"(old));
    if (flag || j >= col_hi || !k) return;
    const int row = (int)(k & ((1ull << ROW_BITS) - 1)) - 1;
    if (old >= row0 && old < row0 + nrows) r2c[old - row0] = -1;
    owner[j] = row;
    if (row >= row0 && row < row0 + nrows) r2c[row - row0] = j;
    pk[j] = 1;   // price 0, owned
    ob[j] = 1;
    bid[j] = 0ull;
}

// ---- two hops: free rows / columns of every local block (block-relative indices, ascending)
// gate_max > 0 (one block only: the pass over the whole matrix queued without a read-back): the pass runs only if
// 0 < HopCtl::left <= gate_max; otherwise the block's counts are set to 0, which makes the pass's other kernels exit,
// and `left` keeps the value the previous pass left
// tab_preset != nullptr: the table rows of the block's free rows are set to HOP_NONE, for a k_hop_table<.., SPLIT> whose
// workgroups take their minima straight into the table
constexpr int HOP_NONE = INT_MAX;   // table entry "no candidate" as k_hop_table<.., SPLIT> leaves it (the other layout writes -1)
__global__ __launch_bounds__(1024) void k_hop_lists(int rpb, int ncols_blk, int col_lo, const int *__restrict__ r2c,
                                                    const int *__restrict__ owner, int *__restrict__ frl, int *__restrict__ fcl,
                                                    HopCtl *__restrict__ hc, const int *__restrict__ ctl, int gate_max = 0,
                                                    int *__restrict__ tab_preset = nullptr)
{
    // in-block call: one round trip for the flag and both arrays' slices (the counting half of both lists only loads).
    // Gated call: the flag and the gate are one round trip and the slices come behind the open gate: it is shut on the
    // instances that leave many rows, and one workgroup counting the whole r2c and owner for nothing cost 16 us at
    // n = 65 536 (k_hop_lists 4.8 -> 21.0 us).  Every thread reads the gate itself: its value is used in front of the first
    // barrier, thread 0 stores `left` behind it
    const int lb = blockIdx.x;
    const int flag = __hip_atomic_load(&ctl[CTL_FLAG], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gate_max > 0) {
        const int left = __hip_atomic_load(&hc->left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" :: "v"(flag), "v"(left));
        if (flag) return;
        if (!(left > 0 && left <= gate_max)) {
            if (threadIdx.x == 0) hc->nfr[lb] = 0, hc->nfc[lb] = 0;
            return;
        }
    }
    const int *rs = r2c + (size_t)lb * rpb, *os = owner + col_lo + (size_t)lb * ncols_blk;
    int cntr, cntc;
    if (rpb == ncols_blk) free_list_count2(rpb, rs, -1, os, -1, cntr, cntc);
    else cntr = free_list_count(rpb, rs, -1), cntc = free_list_count(ncols_blk, os, -1);
    asm volatile("" :: "v"(cntr), "v"(cntc));
    if (flag) return;
    int nfr, nfc;
    build_free_list2(rpb, rs, frl + (size_t)lb * rpb, -1, cntr, ncols_blk, os, fcl + (size_t)lb * ncols_blk, -1, cntc, nfr, nfc);
    if (threadIdx.x == 0) {
        hc->nfr[lb] = nfr;
        hc->nfc[lb] = nfc;
        if (lb == 0) hc->left = 0, hc->matched = 0;
    }
    if (tab_preset) {
        int4 *t4 = reinterpret_cast<int4 *>(tab_preset + (size_t)lb * HOP_FMAX * HOP_FMAX);
        for (int k = threadIdx.x; k < min(nfr, HOP_FMAX) * (HOP_FMAX / 4); k += 1024) t4[k] = make_int4(HOP_NONE, HOP_NONE, HOP_NONE, HOP_NONE);
    }
}

// ---- two hops: per free row the table row tab[b] = smallest r' (global id) with col(r') tight for the row and free
// column b tight for r'.  window_zero = 1: only the block's column slice is read and "tight" means a zero cell at
// price 0 (phase A); 0: the whole row, tight against the row's minimum of c + p.
// The row is taken in segments of 256 chunks (one per thread): the tight cells of a segment go to a list in LDS first
// (a thread-private walk over its 16 cells with three dependent loads behind every hit cost 16 serialised load chains
// per wave: 19 us for a 2048-column slice), then all 256 threads take list entries and keep those whose owner r' is a row
// of the block in a second list, then one thread per (r', free column) pair tests the column against the row's dual and
// takes atomicMin into the table row: the gathers of all pairs are independent of one another.  (A kernel of its own that
// made a 128-bit mask of tight free columns for EVERY assigned row, one wave a row, cost 9.6 + 4.9 + 9.6 us per step at
// n = 16 384 and 71 us in the first pass at n = 65 536; a pass reads the masks of a few dozen rows.)  A segment holds at most
// 256 * E (RAW: 256 * 4 * 4) candidates: the lists cannot overflow, the result does not depend on the order of the appends.
// SPLIT (window_zero only): one workgroup per (free row, segment), blockIdx.x = (lb * HOP_FMAX + a) * nseg + segment, and
// the minima go straight into the table row, which k_hop_lists has preset to HOP_NONE.  The pass over the whole matrix
// has few free rows and several segments a row (RAW: n / 4096); one workgroup per row left all but a handful of CUs
// idle while it walked its segments one behind the other.  atomicMin: the table does not depend on the order.
template <typename CT, bool RAW = false, bool SPLIT = false>
__global__ __launch_bounds__(256) void k_hop_table(int n, int nrows, int row0, int nchunks, int rpb, int ncols_blk, int col_lo,
                                                   int max_rows, int window_zero, const CT *__restrict__ cc,
                                                   const typename Tr<CT>::PT *__restrict__ pk, const int *__restrict__ owner,
                                                   const int *__restrict__ frl, const int *__restrict__ fcl,
                                                   const HopCtl *__restrict__ hc, int *__restrict__ tab,
                                                   const int *__restrict__ ctl, const int32_t *__restrict__ rowmin = nullptr,
                                                   int nseg = 1)
{
    using PT = typename Tr<CT>::PT;
    constexpr int E = RAW ? 4 : Tr<CT>::E;   // cells per 16 bytes (RAW: the int32 matrix itself, nchunks = n / 4, and a cell is c - rowmin[row]: the value the narrow copy holds, for a solve whose compress pass stored the diagonal slices only, k_compress_reg diag_only)
    __shared__ int s_tab[HOP_FMAX];
    constexpr int CHT = RAW ? 4 : 1;   // 16-byte pieces per thread and segment (RAW: 4 cells a piece, the same 4096-entry list as 1-byte cells)
    __shared__ int s_cand[256 * E * CHT];
    __shared__ int s_hr[256 * E * CHT], s_hj[256 * E * CHT];   // the candidates owned by a row r' of the block: r' (local), its column
    __shared__ int s_fc[HOP_FMAX];                             // the block's free columns, the first HOP_FMAX
    __shared__ int s_ncand, s_nhit;
    __shared__ long long s_v[4];
    constexpr int HU = 4;
    const int seg = SPLIT ? (int)blockIdx.x % nseg : 0, ba = SPLIT ? (int)blockIdx.x / nseg : (int)blockIdx.x;
    const int lb = ba / HOP_FMAX, a = ba % HOP_FMAX;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // one round trip: flag, counts, the free row's list entry and the free columns (list indices clamped into the block's
    // lists: entries at or past the counts are stale words nobody uses)
    int flag = ctl[CTL_FLAG];
    int nfr = hc->nfr[lb], nfc_all = hc->nfc[lb];
    int fr_a = frl[(size_t)lb * rpb + min(a, rpb - 1)];
    int fc_t = fcl[(size_t)lb * ncols_blk + min(tid & (HOP_FMAX - 1), ncols_blk - 1)];
    asm volatile("" :: "s"(flag), "s"(nfr), "s"(nfc_all), "s"(fr_a), "v"(fc_t));
    if (flag) return;
    if (nfr > max_rows || a >= min(nfr, HOP_FMAX)) return;
    const int lrow = lb * rpb + fr_a;
    const size_t pitch = (size_t)nchunks * E;
    const unsigned char *rp = reinterpret_cast<const unsigned char *>(cc) + (size_t)lrow * pitch * (RAW ? 4 : sizeof(CT));
    const int32_t mn = RAW ? rowmin[lrow] : 0;
    auto cells = [&](const uint4 &raw, uint32_t *c) {
        if constexpr (RAW) {
            c[0] = (uint32_t)((int32_t)raw.x - mn), c[1] = (uint32_t)((int32_t)raw.y - mn);
            c[2] = (uint32_t)((int32_t)raw.z - mn), c[3] = (uint32_t)((int32_t)raw.w - mn);
        } else
            unpack<CT>(raw, c);
    };
    // a cell of an assigned row r' (local id) as the row's dual sees it
    auto ecell = [&](int rl, int col) -> long long {
        if constexpr (RAW) return (long long)(uint32_t)(reinterpret_cast<const int32_t *>(cc)[(size_t)rl * pitch + col] - rowmin[rl]);
        else return (long long)(uint32_t)cc[(size_t)rl * pitch + col];
    };
    const int nfc = min(nfc_all, HOP_FMAX);
    const int cb = col_lo + lb * ncols_blk;
    if (tid < nfc) s_fc[tid] = fc_t;
    int *tab_row = tab + ((size_t)lb * HOP_FMAX + a) * HOP_FMAX;
    if (!SPLIT && tid < HOP_FMAX) s_tab[tid] = INT_MAX;
    if (tid == 0) s_ncand = 0, s_nhit = 0;
    // the row's columns in question: its block's slice (phase A) or all of them
    const int ch_lo = window_zero ? (col_lo + lb * ncols_blk) / E : 0;
    const int ch_n = window_zero ? (ncols_blk + E - 1) / E : nchunks;
    long long v = 0;
    if (!window_zero) {
        long long mv = LLONG_MAX;
        for (int t = tid; t < ch_n; t += 256) {
            uint32_t c[E];
            cells(*reinterpret_cast<const uint4 *>(rp + (size_t)(ch_lo + t) * 16), c);
            PT pv[E];
            const int j0 = (ch_lo + t) * E;
            if constexpr (sizeof(PT) == 4) {
                const int4 *pp = reinterpret_cast<const int4 *>(pk + j0);
#pragma unroll
                for (int q = 0; q < E / 4; q++) {
                    const int4 x = pp[q];
                    pv[4 * q + 0] = x.x, pv[4 * q + 1] = x.y, pv[4 * q + 2] = x.z, pv[4 * q + 3] = x.w;
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; e++) pv[e] = pk[j0 + e];
            }
#pragma unroll
            for (int e = 0; e < E; e++)
                if (j0 + e < n) mv = min(mv, (long long)c[e] + (long long)(pv[e] >> 1));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long ov = __shfl_xor(mv, o);
            mv = ov < mv ? ov : mv;
        }
        if (lane == 0) s_v[w] = mv;
        __syncthreads();
        v = min(min(s_v[0], s_v[1]), min(s_v[2], s_v[3]));
    }
    __syncthreads();
    for (int t0 = SPLIT ? seg * 256 * CHT : 0; t0 < (SPLIT ? min(ch_n, (seg + 1) * 256 * CHT) : ch_n); t0 += 256 * CHT) {
        uint4 raws[CHT];
#pragma unroll
        for (int u = 0; u < CHT; u++) {
            const int t = t0 + u * 256 + tid;
            if (t < ch_n) raws[u] = *reinterpret_cast<const uint4 *>(rp + (size_t)(ch_lo + t) * 16);
        }
#pragma unroll
        for (int u = 0; u < CHT; u++) {
        const int t = t0 + u * 256 + tid;
        if (t < ch_n) {
            const uint4 raw = raws[u];
            bool any = true;
            if constexpr (!RAW && sizeof(CT) == 1 && std::is_same<CT, uint8_t>::value)   // (a zero cell is a zero byte)
                if (window_zero) any = (zs_zero_bytes(raw.x) | zs_zero_bytes(raw.y) | zs_zero_bytes(raw.z) | zs_zero_bytes(raw.w)) != 0;
            if (any) {
                uint32_t c[E];
                cells(raw, c);
                PT pv[E];
                const int j0 = (ch_lo + t) * E;
                if constexpr (sizeof(PT) == 4) {
                    const int4 *pp = reinterpret_cast<const int4 *>(pk + j0);
#pragma unroll
                    for (int q = 0; q < E / 4; q++) {
                        const int4 x = pp[q];
                        pv[4 * q + 0] = x.x, pv[4 * q + 1] = x.y, pv[4 * q + 2] = x.z, pv[4 * q + 3] = x.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < E; e++) pv[e] = pk[j0 + e];
                }
#pragma unroll
                for (int e = 0; e < E; e++) {
                    const bool tight = j0 + e < n && (long long)c[e] + (long long)(pv[e] >> 1) == v && (!window_zero || c[e] == 0);
                    if (tight) s_cand[atomicAdd(&s_ncand, 1)] = j0 + e;
                }
            }
        }
        }
        __syncthreads();
        const int nc = s_ncand;
        for (int k = tid; k < nc; k += 256) {
            const int j = s_cand[k], r = owner[j];
            if (r < row0 || r >= row0 + nrows) continue;   // a free column (then the rounds take it), or a row of another shard
            if ((r - row0) / rpb != lb) continue;          // (two hops inside the block)
            const int h = atomicAdd(&s_nhit, 1);
            s_hr[h] = r - row0, s_hj[h] = j;
        }
        __syncthreads();
        // one thread per (r', free column b) pair, HU pairs of a thread in flight: b is tight for r' iff c[r'][b] + p[b] equals
        // c[r'][col(r')] + p[col(r')], the row's dual by complementary slackness (col(r') is the candidate column itself)
        const int np = s_nhit * nfc;
        int *dst = SPLIT ? tab_row : s_tab;
        for (int p0 = 0; p0 < np; p0 += 256 * HU) {
            long long du[HU], dx[HU];
            int rg[HU], bb[HU];
            bool live[HU];
#pragma unroll
            for (int q = 0; q < HU; q++) {
                const int p = min(p0 + q * 256 + tid, np - 1);
                const int h = p / nfc, b = p - h * nfc;
                const int rl = s_hr[h], j = s_hj[h], jb = cb + s_fc[b];
                rg[q] = rl + row0, bb[q] = b;
                // (an entry that is no larger already cannot change: no gathers for the pair.  Entries only go down, so a stale
                // read costs gathers, never a result; a row r' is reached by several free rows once a block has more free rows
                // than a row has tight cells per free row, n = 65 536: 2.6 tests per (r', column) without this)
                live[q] = SPLIT || s_tab[b] > rg[q];
                du[q] = dx[q] = 0;
                if (live[q]) {
                    du[q] = ecell(rl, j) + (long long)(pk[j] >> 1);
                    dx[q] = ecell(rl, jb) + (long long)(pk[jb] >> 1);
                }
            }
#pragma unroll
            for (int q = 0; q < HU; q++)
                if (live[q] && p0 + q * 256 + tid < np && du[q] == dx[q]) atomicMin(&dst[bb[q]], rg[q]);
        }
        __syncthreads();
        if (tid == 0) s_ncand = 0, s_nhit = 0;
        __syncthreads();
    }
    if (!SPLIT && tid < HOP_FMAX) tab_row[tid] = s_tab[tid] == INT_MAX ? -1 : s_tab[tid];
}

// ---- two hops: one workgroup per block takes the table rows in order (deterministic greedy) and rewires
// The walk over the free rows is a serial chain, so it runs in ONE wave and touches nothing but LDS and registers:
//   - all HOP_MATCH_T threads stage the block's table rows, the rotated starts and the used-row bits in LDS (one barrier);
//   - wave 0 walks: lane l holds the table entries of free columns l and l + 64.  Two ballots give the 128-bit set of
//     columns whose r' is still unused, the used columns are two scalar words, and "the first column at or after the
//     row's rotated start, cyclically" is a few scalar bit operations: the same column as the minimum over the keys
//     t = (column - st) mod nc that the workgroup-wide version took through LDS and two barriers per row.  Table
//     entries are read two rows ahead and the used-row bits one row ahead; a bit read one row early misses exactly the
//     previous winner, which is compared by value.  The winner goes to s_win[], nothing is loaded from global memory;
//   - after one more barrier thread a rewires match a.  The pairs of different matches share no row and no column (a
//     free row, an r' and a free column are each used once, col(r') is r''s alone), so these loads and stores need no
//     order among themselves; inside the walk the load of col(r') was a global round trip per matched row.
// The flag, the counts, the thread's free row and the table rows of the first 32 free rows are loaded in one group in front
// of the tests ("The kernels of the chain" above); further table rows are staged four 16-byte loads a thread at a time.
// Every in-block pass is still a launch triple of its own: running the passes after the first inside this kernel (one
// workgroup per block rebuilding its lists and its table rows) was specified and not built, see DESIGN 7.1.
// dynamic LDS: HOP_FMAX * HOP_FMAX table entries, then one bit per row of the block.
constexpr int HOP_MATCH_T = 256;
template <typename PT>
__global__ __launch_bounds__(HOP_MATCH_T) void k_hop_match(int nrows, int row0, int rpb, int ncols_blk, int col_lo, int max_rows,
                                                           PT *__restrict__ pk, int *__restrict__ owner, int *__restrict__ r2c,
                                                           uint8_t *__restrict__ ob, const int *__restrict__ frl,
                                                           const int *__restrict__ fcl, HopCtl *__restrict__ hc,
                                                           const int *__restrict__ tab, int *__restrict__ ctl)
{
    extern __shared__ uint32_t s_hop_dyn[];
    __shared__ int s_st[HOP_FMAX];        // rotated start of free row a
    __shared__ int s_win[HOP_FMAX][2];    // match of free row a: r' (-1: none), free column index
    // one round trip: flag, counts, this thread's free row and the first HOP_TAB_U quads a thread stages (the table rows of
    // 32 free rows; a block's table is HOP_FMAX * HOP_FMAX words whatever its counts say, the list index is clamped)
    constexpr int HOP_TAB_U = 4;
    const int lb = blockIdx.x;
    const int tid = threadIdx.x;
    const int *fr = frl + (size_t)lb * rpb, *fc = fcl + (size_t)lb * ncols_blk;
    const int4 *src = reinterpret_cast<const int4 *>(tab + (size_t)lb * HOP_FMAX * HOP_FMAX);
    int flag = ctl[CTL_FLAG];
    int nfr = hc->nfr[lb], nfc_all = hc->nfc[lb];
    int fr_t = fr[min(tid & (HOP_FMAX - 1), rpb - 1)];
    int4 x0[HOP_TAB_U];
#pragma unroll
    for (int q = 0; q < HOP_TAB_U; q++) x0[q] = src[tid + q * HOP_MATCH_T];
    asm volatile("" :: "s"(flag), "s"(nfr), "s"(nfc_all), "v"(fr_t), "v"(x0[0].x), "v"(x0[0].y), "v"(x0[0].z), "v"(x0[0].w),
                 "v"(x0[1].x), "v"(x0[1].y), "v"(x0[1].z), "v"(x0[1].w), "v"(x0[2].x), "v"(x0[2].y), "v"(x0[2].z), "v"(x0[2].w),
                 "v"(x0[3].x), "v"(x0[3].y), "v"(x0[3].z), "v"(x0[3].w));
    static_assert(HOP_TAB_U == 4, "the operand list above");
    if (flag) return;
    if (nfr == 0) return;
    if (nfr > max_rows) {
        if (tid == 0) atomicAdd(&hc->left, nfr);
        return;
    }
    const int na = min(nfr, HOP_FMAX), nc = min(nfc_all, HOP_FMAX);
    int *s_tab = reinterpret_cast<int *>(s_hop_dyn);
    uint32_t *s_usedr = s_hop_dyn + HOP_FMAX * HOP_FMAX;
    const int blk_row0 = row0 + lb * rpb;
    const int my_i = tid < na ? blk_row0 + fr_t : 0;   // free row `tid` of the block
    {
        int4 *dst = reinterpret_cast<int4 *>(s_tab);
        auto norm = [&](int r, int col) { return (r == HOP_NONE || col >= nc) ? -1 : r; };   // -1: no candidate
        auto stage = [&](int k, const int4 &x) {
            const int col = (k * 4) & (HOP_FMAX - 1);
            dst[k] = make_int4(norm(x.x, col), norm(x.y, col + 1), norm(x.z, col + 2), norm(x.w, col + 3));
        };
        const int nq = na * (HOP_FMAX / 4);
#pragma unroll
        for (int q = 0; q < HOP_TAB_U; q++)
            if (tid + q * HOP_MATCH_T < nq) stage(tid + q * HOP_MATCH_T, x0[q]);
        for (int k0 = tid + HOP_TAB_U * HOP_MATCH_T; k0 < nq; k0 += HOP_TAB_U * HOP_MATCH_T) {   // (na > 32: four loads in flight)
            int4 x[HOP_TAB_U];
#pragma unroll
            for (int q = 0; q < HOP_TAB_U; q++) x[q] = src[min(k0 + q * HOP_MATCH_T, nq - 1)];
#pragma unroll
            for (int q = 0; q < HOP_TAB_U; q++)
                if (k0 + q * HOP_MATCH_T < nq) stage(k0 + q * HOP_MATCH_T, x[q]);
        }
        for (int k = tid; k < (rpb + 31) / 32; k += HOP_MATCH_T) s_usedr[k] = 0u;
        if (tid < na) {
            const uint32_t hsh = ((uint32_t)my_i + 1u) * 0x9E3779B1u;
            s_st[tid] = nc ? (int)(((uint64_t)(hsh ^ (hsh >> 15)) * (uint64_t)nc) >> 32) : 0;
        }
    }
    __syncthreads();
    if (tid < 64) {
        const int lane = tid;
        // (no branch around an LDS read: the compiler waits for every read it has to put behind a branch before it goes on,
        // seven LDS round trips a row; the reads of a row are issued together and used one row later)
        auto entry = [&](int a, int col) -> int {   // r' of (free row a, free column col < HOP_FMAX), -1: none
            const int r = s_tab[min(a, HOP_FMAX - 1) * HOP_FMAX + col];
            return a < na ? r : -1;
        };
        auto used = [&](int r) -> bool {   // (a missing entry counts as used)
            const int rb = max(r - blk_row0, 0);
            const uint32_t word = s_usedr[rb >> 5];
            return r < 0 || ((word >> (rb & 31)) & 1u);
        };
        unsigned long long usedc0 = 0ull, usedc1 = 0ull;
        int done = 0, r_prev = -1;
        int ra0 = entry(0, lane), ra1 = entry(0, lane + 64);   // this row's entries
        int rb0 = entry(1, lane), rb1 = entry(1, lane + 64);   // the next row's
        bool ua0 = used(ra0), ua1 = used(ra1);
        int st = s_st[0];
        for (int a = 0; a < na; a++) {
            // reads for the rows to come: issued in front of this row's write to s_usedr
            const int rc0 = entry(a + 2, lane), rc1 = entry(a + 2, lane + 64);
            const bool ub0 = used(rb0), ub1 = used(rb1);
            const int st_nx = s_st[min(a + 1, HOP_FMAX - 1)];
            const unsigned long long m0 = __ballot(!ua0 && ra0 != r_prev) & ~usedc0;
            const unsigned long long m1 = __ballot(!ua1 && ra1 != r_prev) & ~usedc1;
            int rw = -1, cw = 0;
            if (m0 | m1) {
                const unsigned long long h0 = st < 64 ? m0 & (~0ull << st) : 0ull;
                const unsigned long long h1 = st < 64 ? m1 : m1 & (~0ull << (st - 64));
                if (h0 | h1) cw = h0 ? __builtin_ctzll(h0) : 64 + __builtin_ctzll(h1);
                else cw = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
                rw = __builtin_amdgcn_readlane(cw < 64 ? ra0 : ra1, cw & 63);   // (cw is wave-uniform)
                if (cw < 64) usedc0 |= 1ull << cw;
                else usedc1 |= 1ull << (cw - 64);
                r_prev = rw;
                done++;
            }
            if (lane == 0) {
                s_win[a][0] = rw, s_win[a][1] = cw;
                if (rw >= 0) {
                    const int rb = rw - blk_row0;
                    atomicOr(&s_usedr[rb >> 5], 1u << (rb & 31));   // (no value comes back: nothing to wait for)
                }
            }
            // one wave: LDS takes its accesses in program order, the fence keeps the compiler to it
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            ra0 = rb0, ra1 = rb1, ua0 = ub0, ua1 = ub1;
            rb0 = rc0, rb1 = rc1;
            st = st_nx;
        }
        if (lane == 0) {
            atomicAdd(&hc->left, nfr - done);
            atomicAdd(&hc->matched, done);
        }
    }
    __syncthreads();
    if (tid < na && s_win[tid][0] >= 0) {
        const int r = s_win[tid][0], i_g = my_i;
        const int rl = r - row0, il = i_g - row0;
        const int j = r2c[rl], jp = col_lo + lb * ncols_blk + fc[s_win[tid][1]];
        r2c[il] = j;
        owner[j] = i_g;
        r2c[rl] = jp;
        owner[jp] = r;
        pk[jp] = pk[jp] | (PT)1;
        if (ob) ob[jp] = 1;
    }
}

