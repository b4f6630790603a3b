// td_common.h — shared host-side context for the gfx950 assignment library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>

#include "taxidispatcher_amd.h"

namespace td {

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
};

struct Ctx {
    bool inited = false;
    int device = -1;
    int n_cu = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    char err[512] = {0};
    // grow-only device workspace, reused across calls (no hipMalloc on the hot path)
    Buf stage_a, stage_b, stage_c, stage_d, stage_out;  // host<->device staging
    Buf cc;                                             // narrow code matrix of td_lcm / td_pool2
    Buf misc;                                           // small scratch (td_count_sum)
    Buf lcm_a, lcm_b, lcm_c, lcm_d;
    void *pinned = nullptr;  // small pinned host block for result read-back
    size_t pinned_cap = 0;
    // pinned bounce ring for SMALL host inputs (position arrays): a pageable hipMemcpyAsync blocks the host for
    // ~10 us per call, a host memcpy into this ring + an async copy from it does not
    void *pin_in = nullptr;
    size_t pin_in_cap = 0, pin_in_off = 0;
    // profiling
    bool prof = false;
    double prof_ms[TD_K_COUNT] = {0};
    int64_t prof_n[TD_K_COUNT] = {0};
    struct Pending {
        hipEvent_t a, b;
        int k;
    };
    Pending pend[4096];
    int n_pend = 0;
    hipEvent_t ev_pool[8192];
    int n_ev = 0, ev_next = 0;
    hipEvent_t ev_built = nullptr;   // end of the last no-wait builder call on the library's own stream (td_core.hip: builder_end)
    int64_t stats[16] = {0};
};

Ctx &ctx();
int fail(int code, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);
int ensure(Buf &b, size_t bytes);
// releases a workspace buffer (no-op when empty); with ensure() the only place that moves td_workspace_bytes' counter
void buf_free(Buf &b);
bool is_device_ptr(const void *p);
// returns a device pointer holding `bytes` of src (src itself when already on the device)
int to_device(const void *src, size_t bytes, Buf &stage, const void **out);
// a slot of the pinned input ring for `bytes` of host input (the ring wraps after a stream synchronisation); *slot = nullptr
// when there is no ring or the input is empty or larger than PIN_IN_MAX: the caller copies from its own array
constexpr size_t PIN_IN_MAX = 32768;
int pin_in_slot(size_t bytes, void **slot);
// queues the copy of a HOST array to the device, through the ring when it fits
int copy_in(void *dst, const void *src, size_t bytes);
// td_line.hip: sorted matching + certificate pass for line-metric matrices (tried first by td_assign)
//   line_probe_launch  queues the O(n) probe; *skip_dev = device word that is non-zero unless the probe refuses;
//                      clear_words non-null: the probe also zeroes clear_words[0 .. nclear) (td_assign's control words)
//   line_probe_wait    waits for the probe alone (its call number in the pinned verdict block, not the stream; the probe runs behind
//                      whatever the caller queued in front of td_assign, a no-wait cost build included) and returns its verdict:
//                      0 refused, 1 plausible, 2 constant trailing columns (retry on the transpose),
//                      3 plausible with *k constant rows (the unbalanced model)
//   line_finish        keys, sort, prices, certificate pass; *accepted = 1: *r2c_dev / *total are proven optimal;
//                      *path = the LP_QROW2 .. LP_WIDE bits of the probe and of this finish, accepted or not
// td_last_stats word 12 (line_path): what the last td_assign's line attempt did (the public header lists the bits)
enum { LP_PROBE = 1, LP_BALANCED = 2, LP_TRANSPOSE = 4, LP_UNBAL = 8, LP_QROW2 = 16, LP_I2SEARCH = 32, LP_I2COLQ = 64, LP_REV = 128,
       LP_VEC = 256, LP_WIDE = 512, LP_ACCEPTED = 1024 };
// td_last_stats word 13 (finisher_path): which finishers the last td_assign's sv_finish_t launched (the public header lists the bits)
enum { FP_FOREST = 1, FP_FOREST_NONE = 2, FP_FOREST_REFUSED = 4, FP_PSAP = 8, FP_SAPX = 16, FP_SAPX_REFUSED = 32, FP_SAP8_BATCH = 64,
       FP_SAP8 = 128, FP_CH_SHIFT = 8 /* bits 8..12: CH */, FP_SAP512 = 1 << 13, FP_SAP = 1 << 14, FP_NOLDS = 1 << 15,
       FP_BATCH_SHIFT = 16 /* bits 16..31: speculative batches launched */ };
int line_probe_launch(int n, const int32_t *d_cost, const long long **skip_dev, int *clear_words = nullptr, int nclear = 0);
int line_probe_wait(int *mode, int *k, int *suspicious = nullptr /* the 1-byte attempt is void: the probe made the queued pass a no-op */,
                    int *shape3 = nullptr /* int[4]: estimated constant columns / rows, row 0 too wide for one byte, value of the last column */);
int line_finish(int n, int k, const int32_t *d_cost, const int32_t **r2c_dev, int64_t *total, int *accepted, int *path);
void line_release_workspace();
// td_assign.hip: cost build + optimal assignment from DEVICE position arrays in the default workspace (td_tick's remainder);
// a model padded with dummy requests never exists as an int32 matrix (its cells are made inside the fused compress pass)
int build_assign_device(const int32_t *d_cab, int n_s, const int32_t *d_dem, int n_d, const int32_t *d_dist, int S, int32_t fill,
                        int32_t threshold, bool tick, int32_t *row_to_col, int64_t *total, int64_t *dual_bound);
// td_lcm.hip: td_lcm with the candidate cells' value range given by the caller (no min / max pass, no host round trip);
// a wrong hint is detected on the device and the call is redone with the measured range
int lcm_hinted(int n, const int32_t *cost, int32_t mask, int32_t threshold, int stop_value_on, int32_t stop_value, int stop_size,
               int64_t sum_below, int max_pairs, int32_t *rows, int32_t *cols, int32_t *n_pairs, int64_t *total, int32_t *last_min,
               int hint_vmin, int hint_vmax);
// td_core.hip: td_cost_build for device-resident library buffers: no wait for the stream, as the public entry points with
// device arrays, and no ordering of the default stream behind it (td_tick: nobody outside the library sees the buffer)
int cost_build_async(const int32_t *cab_to, int n_s, const int32_t *dem_from, int n_d, const int32_t *dist, int S, int32_t fill,
                     int32_t threshold, int32_t *cost);
// td_lcm.hip: td_tick's LCM of a thresholded |a - b| model on <= 64 stands straight from the position arrays (no matrix);
// *ok = 0: not such a model, nothing done
int lcm_stands(int n_s, int n_d, const int32_t *d_cab_to, const int32_t *d_dem_from, int32_t fill, int32_t threshold, int stop_size,
               int32_t *rows, int32_t *cols, int32_t *n_pairs, int32_t *last_min, int *ok);
// td_batch.hip: frees the batched entry points' result buffer (td_shutdown)
void batch_release_workspace();
// td_batch.hip: td_pool2_batched's greedy, the LCM with symmetric masking over B pair-cost blocks (slab stride n, ns[b] <= n
// <= 2048, INT_MAX = no candidate); pairs at b * (n / 2) in pick order.  Queued on the library stream.
void pool2_greedy_launch(int batch, int n, const int32_t *d_ns, const int32_t *d_cost, int32_t *rows, int32_t *cols, int32_t *n_pairs);
// td_match.hip: frees td_match_batched / td_pool2_batched's workspace (td_shutdown)
void match_release_workspace();
// td_pool.hip: frees td_pool_n / td_pool_merge's workspace (td_shutdown)
void pool_release_workspace();
// td_pool_band.hip: frees td_pool_n_banded's workspace (td_shutdown)
void pool_band_release_workspace();
// td_pool_batch.hip: frees td_pool_n_batched's key slab and staging (td_shutdown)
void pool_batch_release_workspace();
// td_pool_batch.hip: td_pool_n_batched's core on device arrays with a size per model, for the worlds of td_simb_pooling_n
int pool_n_worlds(int k, int batch, int n, const int32_t *off, const int32_t *cnt, const int32_t *k_hi, const int32_t *k_lo,
                  const int32_t *from, const int32_t *to, const int32_t *wait, const int32_t *loss, const int32_t *dist, int S,
                  int64_t max_happy, int32_t *pools, int32_t *n_pools, long long *n_happy, long long *total, int *over_model,
                  long long *over_count);
// td_pool_batch.hip: the same with td_pool_n_banded_batched's kernel (plan_buffer keys per workgroup, no refusal for the plan count)
int pool_n_worlds_banded(int k, int batch, int n, const int32_t *off, const int32_t *cnt, const int32_t *k_hi, const int32_t *k_lo,
                         const int32_t *from, const int32_t *to, const int32_t *wait, const int32_t *loss, const int32_t *dist, int S,
                         int64_t plan_buffer, int32_t *pools, int32_t *n_pools, long long *n_happy, long long *total);
void prof_begin(int k);
void prof_end(int k);
void prof_flush();

#define TD_HIP(call)                                       \
    do {                                                   \
        hipError_t _e = (call);                            \
        if (_e != hipSuccess) return td::hip_fail(_e, #call); \
    } while (0)

#define TD_REQUIRE_INIT()                                                   \
    do {                                                                    \
        if (!td::ctx().inited) return td::fail(TD_ENOINIT, "td_init() has not been called"); \
    } while (0)

struct ProfScope {
    int k;
    explicit ProfScope(int k_) : k(k_) { prof_begin(k); }
    ~ProfScope() { prof_end(k); }
};

__host__ __device__ inline uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

}  // namespace td
