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
//   rounds 1..R  k_zs_bid (one workgroup per free row, 1/V of the row is read) + k_zs_assign: a free column is
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

// ---- phase A, rounds >= 1: one workgroup per free row, zero cells of the row's own column slice only
// ob[j] = 1 once column j has an owner (phase A never changes a price: all are 0)
__global__ __launch_bounds__(256) void k_zs_bid(int nrows, int row0, int nchunks, int rpb, const uint8_t *__restrict__ cc,
                                                const uint8_t *__restrict__ ob, const int *__restrict__ r2c,
                                                unsigned long long *__restrict__ bid, const int *__restrict__ ctl, int round,
                                                int tie_evict)
{
    __shared__ int s_best[4];
    if (ctl[CTL_FLAG]) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int cpb = rpb >> 4;
    const size_t pitch = (size_t)nchunks * 16;
    for (int lrow = blockIdx.x; lrow < nrows; lrow += gridDim.x) {
        if (r2c[lrow] != -1) continue;   // uniform
        const int row = row0 + lrow;
        const int c0 = (row / rpb) * cpb;   // first chunk of the row's column slice
        const uint32_t hsh = ((uint32_t)row + 1u) * 0x9E3779B1u + (uint32_t)round * 0x85EBCA6Bu;
        const int rot = (int)(((uint64_t)(hsh ^ (hsh >> 15)) * (uint64_t)cpb) >> 32);
        const uint8_t *rp = cc + (size_t)lrow * pitch;
        int best = INT_MAX;   // owned << 24 | rotated cell position
        for (int t = tid; t < cpb; t += 256) {
            int ch = t + rot;
            if (ch >= cpb) ch -= cpb;
            ch += c0;
            const uint4 cv = *reinterpret_cast<const uint4 *>(rp + (size_t)ch * 16);
            const uint4 ov = *reinterpret_cast<const uint4 *>(ob + (size_t)ch * 16);
            const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, ow[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t z = zs_zero_bytes(cw[k]);
                if (!z) continue;
                const uint32_t zf = z & zs_zero_bytes(ow[k]);   // zero cell in a free column
                const uint32_t pick = zf ? zf : z;
                const int cand = (zf ? 0 : (1 << 24)) | (t * 16 + k * 4 + (__builtin_ctz(pick) >> 3));
                best = min(best, cand);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
        if (lane == 0) s_best[w] = best;
        __syncthreads();
        if (tid == 0) {
            best = min(min(s_best[0], s_best[1]), min(s_best[2], s_best[3]));
            if (best != INT_MAX) {
                const bool owned = (best >> 24) != 0;
                const int pos = best & 0xFFFFFF;
                int ch = (pos >> 4) + rot;
                if (ch >= cpb) ch -= cpb;
                const int j = (c0 + ch) * 16 + (pos & 15);
                if (!owned || tie_evict) atomicMax(&bid[j], (unsigned long long)(row + 1));   // price 0: the key is the row
            }
        }
        __syncthreads();
    }
}

// ---- phase A: resolve the bids on the columns [col_lo, col_hi) of this shard's blocks (prices stay 0)
__global__ __launch_bounds__(256) void k_zs_assign(int col_lo, int col_hi, int nrows, int row0, unsigned long long *__restrict__ bid,
                                                   int32_t *__restrict__ pk, int *__restrict__ owner, int *__restrict__ r2c,
                                                   uint8_t *__restrict__ ob, const int *__restrict__ ctl)
{
    if (ctl[CTL_FLAG]) return;
    const int j = col_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= col_hi) return;
    const unsigned long long k = bid[j];
    if (!k) return;
    const int row = (int)(k & ((1ull << ROW_BITS) - 1)) - 1;
    const int old = owner[j];
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
    if (ctl[CTL_FLAG]) return;
    const int lb = blockIdx.x;
    if (gate_max > 0) {
        __shared__ int s_go;
        if (threadIdx.x == 0) {
            const int left = hc->left;
            s_go = left > 0 && left <= gate_max;
        }
        __syncthreads();
        if (!s_go) {
            if (threadIdx.x == 0) hc->nfr[lb] = 0, hc->nfc[lb] = 0;
            return;
        }
    }
    const int nfr = build_free_list(rpb, r2c + (size_t)lb * rpb, frl + (size_t)lb * rpb, -1);
    const int nfc = build_free_list(ncols_blk, owner + col_lo + (size_t)lb * ncols_blk, fcl + (size_t)lb * ncols_blk, -1);
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
    if (ctl[CTL_FLAG]) return;
    const int seg = SPLIT ? (int)blockIdx.x % nseg : 0, ba = SPLIT ? (int)blockIdx.x / nseg : (int)blockIdx.x;
    const int lb = ba / HOP_FMAX, a = ba % HOP_FMAX;
    const int nfr = hc->nfr[lb];
    if (nfr > max_rows || a >= min(nfr, HOP_FMAX)) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lrow = lb * rpb + frl[(size_t)lb * rpb + a];
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
    const int nfc = min(hc->nfc[lb], HOP_FMAX);
    const int cb = col_lo + lb * ncols_blk;
    if (tid < nfc) s_fc[tid] = fcl[(size_t)lb * ncols_blk + tid];
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
    if (ctl[CTL_FLAG]) return;
    const int lb = blockIdx.x;
    const int nfr = hc->nfr[lb];
    const int tid = threadIdx.x;
    if (nfr == 0) return;
    if (nfr > max_rows) {
        if (tid == 0) atomicAdd(&hc->left, nfr);
        return;
    }
    const int na = min(nfr, HOP_FMAX), nc = min(hc->nfc[lb], HOP_FMAX);
    int *s_tab = reinterpret_cast<int *>(s_hop_dyn);
    uint32_t *s_usedr = s_hop_dyn + HOP_FMAX * HOP_FMAX;
    const int *fr = frl + (size_t)lb * rpb, *fc = fcl + (size_t)lb * ncols_blk;
    const int blk_row0 = row0 + lb * rpb;
    const int my_i = tid < na ? blk_row0 + fr[tid] : 0;   // free row `tid` of the block
    {
        const int4 *src = reinterpret_cast<const int4 *>(tab + (size_t)lb * HOP_FMAX * HOP_FMAX);
        int4 *dst = reinterpret_cast<int4 *>(s_tab);
        auto norm = [&](int r, int col) { return (r == HOP_NONE || col >= nc) ? -1 : r; };   // -1: no candidate
        for (int k = tid; k < na * (HOP_FMAX / 4); k += HOP_MATCH_T) {
            const int4 x = src[k];
            const int col = (k * 4) & (HOP_FMAX - 1);
            dst[k] = make_int4(norm(x.x, col), norm(x.y, col + 1), norm(x.z, col + 2), norm(x.w, col + 3));
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

