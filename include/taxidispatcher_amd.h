/*
 * taxidispatcher_amd.h — C ABI of the MI355X (gfx950) cab<->request assignment path.
 *
 * This is the drop-in boundary for ONE hot path of boguszjelinski/taxidispatcher:
 *     cost-matrix build  ->  (optional) LCM greedy pre-reduce  ->  optimal N x N assignment
 * i.e. what the reference hands to cvxopt.glpk.ilp.  Nothing native exists in the reference
 * for this path (its three C files are pool finders), so each entry point cites the
 * reference *function* it replaces; the Python binding a maintainer would add is shown in
 * INTEGRATION.md and shipped in taxidispatcher_amd/_ffi.py.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `void*` stream is a hipStream_t.
 *   - every data pointer may be a HOST pointer or a DEVICE pointer of the active device;
 *     the library detects which (hipPointerGetAttributes) and stages host buffers itself.
 *   - caller owns every buffer; the library keeps no pointer past return (the shard handles td_shard_* /
 *     td_lcm_shard_* excepted: they read their cost_rows until they are destroyed).  A pointer need only be
 *     aligned to its element size; outputs are written within their stated capacity and nowhere else.
 *   - return 0 on success, a negative TD_E* code on failure; td_last_error() gives the text.
 *     No exceptions cross the ABI.
 *   - single-threaded like the reference (one solve at a time per process); calls are
 *     synchronous unless the name ends in _async.
 *   - cost matrices are row-major int32, row = cab (supply), column = request (demand),
 *     exactly the reference's `cost[cab][cust]` / linear index n*cab+cust
 *     (solver.py:13, greedy_opt.py:22-24, Simulator.java:378-380).
 */
#ifndef TAXIDISPATCHER_AMD_H
#define TAXIDISPATCHER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define TD_API __attribute__((visibility("default")))
#else
#define TD_API
#endif

#define TD_OK 0
#define TD_EINVAL (-1)   /* bad argument */
#define TD_EHIP (-2)     /* a HIP runtime call failed */
#define TD_ENOINIT (-3)  /* td_init not called */
#define TD_ERANGE (-4)   /* cost range would overflow the solver's integer arithmetic */
#define TD_EINTERNAL (-5)

/* ---- life cycle -------------------------------------------------------------------- */
TD_API int td_init(int device);            /* select GPU, create stream + workspace */
TD_API void td_shutdown(void);
TD_API const char *td_last_error(void);
/* Stream rule: every entry point enqueues on ONE stream (the library's own unless td_set_stream
 * gave it the caller's). Device INPUTS must be complete in that stream's order, device OUTPUTS of
 * the asynchronous entry points (td_cost_build, td_gen_uniform with a device destination) are
 * ready in that stream's order: a caller working on another stream either shares its stream
 * with td_set_stream or fences with its own synchronisation / td_synchronize. Entry points that
 * return values to the host (td_assign, td_lcm, td_pool2, td_count_sum) return after their
 * results are complete.
 * The builders (td_cost_build, td_cost_build_rows, td_gen_uniform) do NOT wait for the stream
 * when the destination and every array argument they were given (positions, ids, the distance
 * table) are device memory: the call returns with its kernels queued, and the next entry point
 * (td_assign, td_lcm, ...) queues behind them without a host round trip in between. Launch
 * errors are still reported by the call, execution errors by the next call that synchronises.
 * If ANY of those pointers is host memory (a pinned host pointer counts as host) the call waits:
 * a host destination is complete on return, a host array may be reused or freed on return.
 * Lifetime: the device inputs of a call that did not wait must stay valid and unmodified, and
 * its output must not be written by anyone else, until the library's stream has passed the
 * call: that is td_synchronize or any entry point that returns values to the host.
 * While the library runs on its own stream, a builder that does not wait also makes the default
 * (null) stream wait for it on the device: work queued on the default stream after the call sees
 * the whole output. Work on any other stream needs the fence above. */
TD_API int td_set_stream(void *hip_stream); /* run on the caller's stream (NULL -> library stream) */
TD_API int td_synchronize(void);
/* Device bytes currently held in the library's grow-only workspaces (the default solver, handles, shards, staging and
 * result buffers).  Callable at any time, before td_init and after td_shutdown too.  After a *_destroy it is back at the
 * value from before the matching *_create; after td_shutdown it is 0, PROVIDED every td_solver, td_shard and td_lcm_shard
 * handle was destroyed first: td_shutdown does not release what a handle owns, and the shard *_destroy calls refuse to run
 * once the library is shut down.  Pinned host blocks are not counted. */
TD_API int td_workspace_bytes(int64_t *bytes);
TD_API int td_version(void);

/* ---- a-2 cost-matrix build ---------------------------------------------------------
 * Replaces calculate_cost: greedy_opt.py:86-99 (fill=big_cost, threshold<0),
 * simulate.py:17-33 (threshold=DROP_TIME), Simulator.java:493-520 (same + id != -1, pass
 * ids as NULL when all valid), and — with ids — procedure.py:6-12 (cells addressed by id,
 * fill = n*n).
 *   n = max(n_s, n_d);  cost is n*n int32, pre-filled with `fill`;
 *   cost[c][d] = dist[cab_to[c]*S + dem_from[d]]   (dist == NULL  =>  |cab_to[c]-dem_from[d]|)
 *   written only when threshold < 0 or value < threshold.
 *   cab_id / dem_id: NULL => positional.  Non-NULL => a pair is skipped when either id is -1
 *   (Simulator.java:508); with by_id != 0 the cell written is cost[cab_id[c]][dem_id[d]]
 *   (procedure.py:12).
 * One GPU thread per (cab, request) pair quad; position arrays read coalesced.
 */
TD_API int td_cost_build(const int32_t *cab_to, const int32_t *cab_id, int n_s,
                  const int32_t *dem_from, const int32_t *dem_id, int n_d,
                  const int32_t *dist, int S, int32_t fill, int32_t threshold, int by_id,
                  int32_t *cost /* n*n */);

/* Row window of the same matrix: writes rows [row0, row0 + nrows) of the n x n model into
 * cost_rows (nrows * n int32).  This is how a row shard builds its block in place from the
 * replicated position arrays: every rank passes the full cab_to / dem_from (<= 256 KiB
 * each) and its own window; no communication.  With by_id the window applies to the cab ids. */
TD_API int td_cost_build_rows(const int32_t *cab_to, const int32_t *cab_id, int n_s,
                       const int32_t *dem_from, const int32_t *dem_id, int n_d,
                       const int32_t *dist, int S, int32_t fill, int32_t threshold, int by_id,
                       int row0, int nrows, int32_t *cost_rows /* nrows*n */);

/* ---- a-4 optimal assignment --------------------------------------------------------
 * Replaces solve(n, cost) at solver.py:11-27 (and the ilp call at procedure.py:27,
 * greedy_opt.py:117, simulate.py:52, heuristic.py:37): min sum c[i][j] x[i][j], every row
 * and column used exactly once.  Output is row_to_col[n] (x[n*i + row_to_col[i]] == 1);
 * td_expand_x gives the reference's n*n 0/1 vector.
 *   total       optimal objective (exact integer, equals GLPK's optimum)
 *   dual_bound  may be NULL; else an LP-duality lower bound computed on the device from the
 *               final prices: dual_bound == total certifies optimality.
 * One solver per process: td_assign works in ONE grow-only device workspace owned by the library
 * (no hipMalloc after the first call of a size), like the reference, which solves one model at a
 * time per process (Simulator.java:195-205 waits for its child).  Calls are serialised by the
 * caller; consecutive calls of any sizes are independent (tests/test_gpu_parity.py::
 * test_workspace_reuse_across_sizes).  Row shards (td_shard_*) each own a workspace, so several
 * shards may live in one process.
 */
TD_API int td_assign(int n, const int32_t *cost, int32_t *row_to_col, int64_t *total,
              int64_t *dual_bound);
/* Line-metric instances.  The reference's distance table is a line (greedy_opt.py:122-127: dist[i][j] = |i - j|),
 * so its square cost matrices are |a_i - b_j|: sorted by a and b they are Monge and the sorted matching is
 * optimal.  td_assign tries that matching first (O(n) anchor reads, one sort of 2n keys) and keeps it only
 * when ONE pass over the matrix proves it optimal on the actual cells (row minima of c[i][j] - v[j] all on
 * the matched cells; exact 64-bit integers); every other matrix goes to the general solver unchanged.
 * td_set_line_metric(0) switches the attempt off (1 = on, the default; env TD_LINE=0 does the same);
 * returns the previous setting. */
TD_API int td_set_line_metric(int on);

/* ---- handle-scoped solvers --------------------------------------------------------------------------
 * td_assign / td_build_assign solve in the library's default workspace.  A td_solver owns a workspace of its own (grow-only,
 * released by td_solver_destroy), so one process can keep several — e.g. one sized for N = 65 536 and one for ticks — without
 * one call regrowing what the other needs.  Same arguments, results and errors as td_assign / td_build_assign.  A handle
 * owns its workspace and nothing else: the stream, the pinned read-back block and td_last_stats belong to the library
 * context, so calls are synchronous and ONE AT A TIME PER PROCESS, whichever handles they go to (the reference is
 * strictly single-threaded).  Handles are not a way to solve from two threads at once. */
typedef struct td_solver td_solver;
TD_API int td_solver_create(td_solver **out);
TD_API int td_solver_destroy(td_solver *h);
TD_API int td_solver_assign(td_solver *h, int n, const int32_t *cost, int32_t *row_to_col, int64_t *total, int64_t *dual_bound);
TD_API int td_solver_build_assign(td_solver *h, const int32_t *cab_to, int n_s, const int32_t *dem_from, int n_d, const int32_t *dist, int S,
                                  int32_t fill, int32_t threshold, int32_t *row_to_col, int64_t *total, int64_t *dual_bound);

/* ---- API #1 of the reference in ONE call: cost build + optimal assignment --------------------------------------
 * What procedure.py:5-29, greedy_opt.py:102-118 and simulate.py:36-53 expose: solve(distances, demand, cabs) builds the cost
 * matrix (td_cost_build's positional rule: cost[i][j] = dist[cab_to[i]][dem_from[j]] if below `threshold`, else `fill`;
 * rows / columns beyond n_s / n_d are `fill`; dist == NULL => |a - b|) and solves it.  Same row_to_col, total and
 * dual bound as td_cost_build + td_assign — but a model padded with dummy requests (n_s - n_d beyond the shape rule's
 * margin, fill >= 255: every Simulator.java / simulate.py tick) never exists as an int32 matrix: the fused transposing
 * compress pass makes each cell from the position arrays straight into its 1- / 4-byte working copy, and the total is
 * summed from the position arrays again (csrc/td_assign.hip: CellSrc).  Other shapes are built into a library buffer
 * and solved by td_assign.  Arrays may be host or device memory; td_tick's remainder goes through the same path. */
TD_API int td_build_assign(const int32_t *cab_to, int n_s, const int32_t *dem_from, int n_d, const int32_t *dist, int S, int32_t fill,
                           int32_t threshold, int32_t *row_to_col, int64_t *total, int64_t *dual_bound);

/* n*n bytes of 0/1 in the reference's order i = n*cab + cust (solver.py:36-39) */
TD_API int td_expand_x(int n, const int32_t *row_to_col, uint8_t *x);

/* ---- a-5 LCM greedy pre-reduce -----------------------------------------------------
 * Replaces LCM: greedy_opt.py:61-82, simulate.py:76-98, heuristic.py:24-33,
 * Simulator.java:523-549.  Repeatedly takes the first minimum in row-major order and masks
 * its row and column.
 *   threshold >= 0 : stop before taking a cell  > threshold     (greedy_opt.py:68-69)
 *   stop_value_on  : stop before taking a cell == stop_value, and cells >= stop_value are
 *                    never candidates                              (Simulator.java:529-538)
 *   stop_size >= 0 : stop after taking when n - pairs == stop_size (Simulator.java:544-545)
 *   sum_below      : a taken cell is summed only if value < sum_below (greedy_opt.py:74)
 *   max_pairs      : capacity of rows[] / cols[] (n is always enough)
 * Outputs pairs in the order the reference takes them.
 */
TD_API int td_lcm(int n, const int32_t *cost, int32_t mask, int32_t threshold, int stop_value_on,
           int32_t stop_value, int stop_size, int64_t sum_below, int max_pairs,
           int32_t *rows, int32_t *cols, int32_t *n_pairs, int64_t *total, int32_t *last_min);

/* ---- a-4 / a-5 for MANY small models in one call (heuristic.py:20-40, split.py:61-120) -------------------------------
 * B independent square models of size up to n (n <= 1024), model b's cells at cost + b*n*n, row-major,
 * row = cab, column = request.  ns (int32[B], may be NULL = every model is n x n): model b is the top-left
 * ns[b] x ns[b] block of its slab (0 <= ns[b] <= n); cells outside it are never read.
 * One workgroup per model (csrc/td_batch.hip): no launch, copy or host synchronisation per model, which is what a
 * td_assign / td_lcm call per model pays.  Cells are indexed with 64-bit arithmetic (B*n*n may exceed 2^31).
 * Arrays may be host or device memory; calls are synchronous.  TD_EINVAL: n > 1024 (a large model is one td_assign
 * call), batch < 0, ns[b] outside [0, n].
 *
 * td_assign_batched: the optimum of every model.  Outputs per model: row_to_col[b*n + i] (i < ns[b]; -1 for
 * i >= ns[b]), total[b], dual_bound[b] (may be NULL), col_price[b*n + j] (int64, may be NULL; 0 for j >= ns[b]):
 * column potentials v with sum_i min_j (c_ij - v_j) + sum_j v_j == dual_bound[b], recomputed from the cells;
 * dual_bound == total certifies optimality.  TD_EINTERNAL if a model hit a defensive loop cap.
 * When to use which (measured on MI355X): up to n = 256 the batched call wins (1000 models of 100 x 100:
 * 1.3 ms against 371 ms for a loop of td_solver_assign); at n = 1024 one td_assign per model is faster for heavily tied
 * costs (U{1..39}: 0.24 against 0.9 ms per model) while uniform costs still gain 7x batched.  Crossover: n ~ 512. */
TD_API int td_assign_batched(int batch, int n, const int32_t *ns, const int32_t *cost, int32_t *row_to_col,
                             int64_t *total, int64_t *dual_bound, int64_t *col_price);

/* td_lcm's semantics and parameters applied to every model of the batch (same slab layout / ns as above;
 * stop_size counts against ns[b]; at most ns[b] picks).  rows / cols: int32[B*n] (model b's pairs at b*n, in pick
 * order), n_pairs / last_min: int32[B], total: int64[B]. */
TD_API int td_lcm_batched(int batch, int n, const int32_t *ns, const int32_t *cost, int32_t mask, int32_t threshold,
                          int stop_value_on, int32_t stop_value, int stop_size, int64_t sum_below,
                          int32_t *rows, int32_t *cols, int32_t *n_pairs, int64_t *total, int32_t *last_min);

/* ---- many dispatch models from their POSITIONS in one call (split.py's regions, zones / cities of one tick, sweeps) ----
 * B ragged dispatch models: model b = cabs cab_to[cab_off[b] .. cab_off[b+1]), requests dem_from[dem_off[b] .. dem_off[b+1]);
 * one shared distance table (S x S, or NULL = |a - b|).  n_s(b), n_d(b) are those counts and n(b) = max(n_s, n_d).
 * Model b's cells follow td_cost_build's positional rule: dist[cab][dem] when threshold < 0 or it is below threshold, else
 * fill; a stand outside [0, S) of a table, and rows / columns beyond n_s / n_d, are fill.  No cost matrix is ever written:
 * one workgroup per model makes its cells from the positions (the table staged in LDS when it fits, else read through L2).
 *   n: the caller's output stride; every n(b) <= n.  Offsets: int32[B+1], from 0, never decreasing.  Per-model outputs are
 *   [B*n] with model b's entries at b*n; scalars [B].  Arrays may be host or device memory (outputs too); calls are
 *   synchronous; batch == 0 is a no-op.
 * td_build_assign_batched: model b = td_build_assign of its positions: row_to_col[b*n + i] (i < n(b); -1 beyond),
 *   total[b] (dummy cells count fill), dual_bound[b] (may be NULL; recomputed from the cells: == total certifies the model).
 *   TD_EINVAL: n > 1024.
 * td_tick_batched: model b = td_tick on the same arguments: the LCM of Simulator.java:523-549 down to stop_size rows (stop on
 *   fill; skipped when stop_size < 0 or >= n(b)), the shrink, the remainder's optimum.  lcm_rows / lcm_cols: the pairs in
 *   the reference's pick order, n_pairs[b] of them; lcm_last_min[b] (fill when the LCM did not run); kept_cabs / kept_dems
 *   (may be NULL): indices into model b's own lists, in order; n_rest[b] = the larger count; row_to_col (over the kept lists;
 *   -1 for i >= n_rest[b]), total, dual_bound (may be NULL): the remainder's optimum.  When the LCM ran and ended on fill (Simulator.java:188-189)
 *   the model has no solve: row_to_col is -1, total and dual_bound are 0 (defined here, unlike td_tick).  stop_size < 0
 *   equals td_build_assign_batched plus empty pair lists.  TD_EINVAL: n > 2048, or a model whose remainder has more than
 *   1024 rows (min(n(b), stop_size) when the LCM runs, else n(b)).
 * Both: TD_EINVAL for S <= 0 with a table, invalid offsets, null required outputs; TD_EINTERNAL if a model hit a
 * defensive loop cap.  Two launches per tick call (LCM + shrink, then the solve), one per build call, whatever B is.
 * When to use which: many models of up to a few hundred stands per side: these calls; a single large model,
 * or 1300 x 900 ticks, where the per-model td_tick loop can win: see the measured crossover. */
TD_API int td_build_assign_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to,
                                   const int32_t *dem_off, const int32_t *dem_from, const int32_t *dist, int S,
                                   int32_t fill, int32_t threshold, int32_t *row_to_col, int64_t *total,
                                   int64_t *dual_bound);
TD_API int td_tick_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to,
                           const int32_t *dem_off, const int32_t *dem_from, const int32_t *dist, int S,
                           int32_t fill, int32_t threshold, int stop_size,
                           int32_t *lcm_rows, int32_t *lcm_cols, int32_t *n_pairs, int32_t *lcm_last_min,
                           int32_t *kept_cabs, int32_t *kept_dems, int32_t *n_rest, int32_t *row_to_col,
                           int64_t *total, int64_t *dual_bound);

/* ---- the split heuristic of MANY cases in one call (split.py:61-119 as a whole) -----------------------------------------
 * B ragged cases as above (offsets, positions, one shared table or NULL = |a - b|, host or device memory, synchronous,
 * batch == 0 is a no-op); n bounds every case's max(n_s, n_d), n <= 1024 (the fifth model can be a whole case).  Cells are
 * dist[cab_to][dem_from], no threshold.
 *   Ranges: split_size = size / parts; range r is stands [r*split_size, (r+1)*split_size) for every r*split_size < size, so a
 *   size that parts does not divide gives more than parts ranges, the last one short (the reference's `while start<size`).
 *   A cab belongs to the range of its cab_to, a request to that of its dem_from; order within a region is the case's order.
 *   Region with cabs and requests: the optimum of its square model padded with fill.  A pair on a real cell is served; with
 *   more cabs than requests the cabs on dummy columns go to the rest, with more requests the requests on dummy rows do.
 *   Region with requests only / without requests: all of them / all its cabs go to the rest.
 *   Fifth solve: the optimum over the rest cabs and rest requests, each in the case's order; only real cells are summed.
 *   A case with no cabs or no requests has no solve at all (split.py:62-64): total 0, every cab -1, n_rest 0 / 0.
 * Outputs: cab_req[cab_off[c] + i]: the index, within case c's request list, of the request cab i serves, or -1;
 *   cab_stage (same shape, may be NULL): 0 served inside its region, 1 by the fifth solve, -1 not served; total[c]: the split
 *   total; rest_total[c] (may be NULL): the fifth solve's part of it; n_rest[2c], n_rest[2c + 1] (may be NULL): the sizes of
 *   the rest lists; dual_gap[c] (may be NULL): the sum over every model solved for the case of total - dual_bound as the
 *   solver's dual pass reports them: 0 certifies every model of the case.  Which cab of a region stays over is the solver's
 *   choice among equal optima, so totals of two different solvers need not agree; a region's own sum always does.
 * Five launches whatever B is (partition, the region models, collection, the fifth models, sums: csrc/td_batch.hip), no
 * host read-back between them, one synchronisation at the end.
 * TD_EINVAL, with every output left unwritten: n > 1024 or a case larger than n, bad offsets, parts outside [1, 32],
 *   size < parts, S < size with a table, a position outside [0, size), a table entry used as a cell outside [0, fill),
 *   fill < 1, on the line size - 1 >= fill, null cab_req / total or inputs.  Positions and table entries are checked on the
 *   device.  TD_EINTERNAL (outputs unwritten as well) if a model hit a defensive loop cap.
 * When to use which (measured on MI355X): the whole heuristic is one call wherever the two-call route
 * (two td_build_assign_batched calls with a host pass that cuts the lists and collects the unserved) was measured: 1000 cases of
 * 10 per side on 20 stands 0.97 against 23.3 ms, 1000 cases of 400 / 400 on 4000 stands 9.2 against 39.4 ms.  No shape was found
 * where the two calls win; regions alone, with nothing left over to solve, remain td_build_assign_batched. */
TD_API int td_split_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to,
                            const int32_t *dem_off, const int32_t *dem_from, const int32_t *dist, int S,
                            int size, int parts, int32_t fill, int32_t *cab_req, int32_t *cab_stage,
                            int64_t *total, int64_t *rest_total, int32_t *n_rest, int64_t *dual_gap);

/* ---- MANY dispatch models in one call, a dispatch method per model ---------------------------------------------------------
 * td_tick_batched's inputs and output layout (ragged lists behind offsets, host or device memory, synchronous, batch == 0 is
 * a no-op, n = the output stride <= 2048), plus a policy per model: mode[b], stop_size[b], parts[b], each int32[B], host or
 * device memory, each may be NULL (mode 0 everywhere; the LCM never runs; 4 parts).  size = the number of stands the split's
 * ranges are cut over (read for split models only).
 *   TD_DISPATCH_LCM_OPT  model b is what td_tick_batched makes of it with stop_size[b], every output.
 *   TD_DISPATCH_OPT      the LCM never runs: td_tick_batched with stop_size < 0.
 *   TD_DISPATCH_LCM      the LCM of Simulator.java:523-549 with stop size 0, run to its end (no candidate below fill left, or
 *                        every row taken); the model is never solved, whatever the last minimum was.  Pairs, n_pairs and
 *                        lcm_last_min as td_tick_batched; kept lists = who is in no pair; n_rest = the larger kept count;
 *                        row_to_col -1, total and dual_bound 0.
 *   TD_DISPATCH_SPLIT    split.py:61-119 (td_split_batched's ranges of parts[b] over size, region optima, collection of the
 *                        left-overs, the fifth solve) on the model's thresholded cells: a cell is dist below threshold, else
 *                        fill (threshold < 0: dist).  A cab is served only on a real cell below fill: a pair on a thresholded
 *                        cell leaves its cab and its request to the rest (after the fifth solve: unserved), and only cells
 *                        below fill are summed.  n_pairs 0, lcm_last_min fill, n_rest = max(n_s, n_d), kept lists = the whole
 *                        model in order, row_to_col[b*n + i] = the request cab i serves within the model's request list or -1
 *                        (td_split_batched's cab_req; -1 for i >= n_s), total = the split total, dual_bound = total minus the
 *                        case's dual gap: dual_bound == total certifies every model solved for the case.  With threshold < 0
 *                        row_to_col and total equal td_split_batched's cab_req and total bit for bit.
 * Launches (csrc/td_batch.hip): the tick's two take every model that is not split, the split's five take the split models
 * and run only when there is one: 2 without a split model, 7 with one, whatever B and the mix.
 * TD_EINVAL, with every output left unwritten: td_tick_batched's rules; with a split model td_split_batched's (S < size with a
 * table, fill < 1, on the line size - 1 >= fill, a position of a split model outside [0, size), a table entry used as its
 * cell outside [0, fill)); a mode outside 0 .. 3; a split model with more than 1024 cabs or requests; parts[b] outside
 * [1, 32] or size < parts[b] for a split model; a TD_DISPATCH_OPT / _LCM_OPT model whose remainder (by its own stop_size)
 * has more than 1024 rows.  TD_EINTERNAL if a model hit a defensive loop cap. */
#define TD_DISPATCH_LCM_OPT 0
#define TD_DISPATCH_OPT 1
#define TD_DISPATCH_LCM 2
#define TD_DISPATCH_SPLIT 3
TD_API int td_dispatch_batched(int batch, int n, const int32_t *cab_off, const int32_t *cab_to,
                               const int32_t *dem_off, const int32_t *dem_from, const int32_t *dist, int S,
                               int32_t fill, int32_t threshold, int size, const int32_t *mode,
                               const int32_t *stop_size, const int32_t *parts,
                               int32_t *lcm_rows, int32_t *lcm_cols, int32_t *n_pairs, int32_t *lcm_last_min,
                               int32_t *kept_cabs, int32_t *kept_dems, int32_t *n_rest, int32_t *row_to_col,
                               int64_t *total, int64_t *dual_bound);

/* Row-sharded LCM: rank r owns cost rows [row0, row0 + nrows).  Per pick every shard
 * reports its smallest live cell {value, global row, column} (value = INT64_MAX: none), the caller
 * takes the minimum in the reference's order (value, row, column) over all shards — one all-gather of
 * 24 bytes per rank — applies td_lcm's stop rules and tells every shard the pick.  Pairs, total and
 * last_min equal td_lcm's.  Host driver: taxidispatcher_amd/sharded.py lcm_sharded. */
typedef struct td_lcm_shard td_lcm_shard;
TD_API int td_lcm_shard_create(int n, int row0, int nrows, const int32_t *cost_rows, int stop_value_on,
                               int32_t stop_value, td_lcm_shard **out);
TD_API int td_lcm_shard_destroy(td_lcm_shard *s);
TD_API int td_lcm_shard_local_min(td_lcm_shard *s, int64_t *out3);
TD_API int td_lcm_shard_take(td_lcm_shard *s, int row, int col);
/* The same result in ROUNDS of locally dominant cells instead of one exchange per pick (Simulator.java:523-549 takes up
 * to 700 picks per tick): a live cell that is the first minimum of its row AND of its column under the order (value, row,
 * column) is taken by the sequential greedy before anything else of its row or column, so all of them are taken at once.
 * Per round: round_colmin (per column the smallest live cell below `limit` of this shard's rows, INT64_MAX = none) -> MIN
 * all-reduce of the n keys -> round_apply (taken[c] = the key of a row whose first minimum is its column's minimum,
 * INT64_MIN = none) -> MAX all-reduce -> round_commit (mask the taken columns everywhere, retire the taken rows, re-scan the
 * rows that lost their cached column).  A key is (value << 32) | (global row + 1) as a SIGNED int64, ordered like (value,
 * row): value = key >> 32, row = (key & 0xFFFFFFFF) - 1.  Its low word is 1 .. 2^31, so neither sentinel is the key of a
 * cell, whatever int32 value the cell holds (-2^31 in row 0 included).  The picks sorted by (value, row, column) are
 * td_lcm's pair list; the stop rules are applied to that order by the host driver (sharded.py lcm_sharded).  Vectors
 * may be host or device memory. */
TD_API int td_lcm_shard_round_colmin(td_lcm_shard *s, int64_t limit, int64_t *colmin);
TD_API int td_lcm_shard_round_apply(td_lcm_shard *s, int64_t limit, const int64_t *colmin, int64_t *taken);
TD_API int td_lcm_shard_round_commit(td_lcm_shard *s, const int64_t *taken);

/* ---- one dispatcher tick in ONE call (BASELINE configs[4]) ---------------------------------
 * Replaces, for one time step, Simulator.java:163-208 after createTempDemand / createTempSupply:
 * calculate_cost (:493-520; simulate.py:17-33) -> LCM down to `stop_size` rows (:523-549, stops on big_cost or
 * when MAX_NON_LCM rows are left; skipped when stop_size < 0 or >= n) -> removal of the matched cabs and requests
 * (analyzePairs :613-674, filter_out greedy_opt.py:32-37 / simulate.py:64-69: a compaction kernel, the pair list
 * never leaves the device for it) -> calculate_cost of the remainder -> optimal assignment (solver.py:26).
 *   cab_to[n_s], dem_from[n_d], dist (S x S or NULL = |a-b|): host or device; fill = big_cost; threshold = DROP_TIME
 *   (< 0: none).  Outputs (HOST arrays): the LCM pairs in the reference's order (capacity max(n_s, n_d)), *n_pairs,
 *   *lcm_last_min (LCM_min_val, Simulator.java:188), kept_cabs / kept_dems (may be NULL: positions of the cabs /
 *   requests left for the solver, in order), *n_rest = max of their counts, row_to_col[n_rest] and the total of
 *   the remainder's optimal assignment (dummy cells count fill, like td_assign).  An empty model returns 0 pairs,
 *   n_rest 0.  When the LCM ran and ended on `fill` (*lcm_last_min == fill) the tick has no input for the solver,
 *   as in Simulator.java:188-189: the pairs, the kept lists and *n_rest are reported, row_to_col is left untouched and
 *   *total is 0.  row_to_col indexes the kept lists: ask for kept_cabs / kept_dems whenever it is used.
 *   The cost matrices are library buffers in HBM (td_tick_release_workspace frees them). */
TD_API int td_tick(const int32_t *cab_to, int n_s, const int32_t *dem_from, int n_d, const int32_t *dist, int S, int32_t fill,
                   int32_t threshold, int stop_size, int32_t *lcm_rows, int32_t *lcm_cols, int32_t *n_pairs,
                   int32_t *lcm_last_min, int32_t *kept_cabs, int32_t *kept_dems, int32_t *n_rest, int32_t *row_to_col,
                   int64_t *total);
TD_API void td_tick_release_workspace(void);

/* ---- a simulator world in device memory (Simulator.java:151-211, the whole tick loop) -----------------
 * The handle owns the request table (id, from, to, at, cab_assigned, picked_at, pool_id, pool_plan, pool_cost) and the
 * fleet (from, to, client, on_board, time_started) in HBM; they never leave the device.  Cab i starts at stand
 * i % n_stands (initSupply :565-573); distances are |a - b| on n_stands stands (td_sim_create) or a stand-to-stand table
 * (td_sim_create_dist, below).  A tick is
 *   td_sim_begin   checkIfCabAtDestination (:220-254), createTempDemand incl. the drop (:329-355), createTempSupply
 *                  (:358-372), findPool (td_pool2 on the device lists) and analyzePool (:760-784; skipped without supply).
 *                  info = {has_demand, demand before pooling, supply, demand after pooling}; has_demand == 0: the tick
 *                  is over (Simulator.java:160), no td_sim_apply follows.
 *   td_sim_model   the tick's model: cab_to[supply], dem_from[demand after pooling], host or device destination.
 *   td_sim_apply   the decisions, from any source: the LCM pairs (indices into the model; read only when the model is
 *                  larger than max_non_lcm: analyzePairs :613-674, which also leaves the kept cabs / requests in order) and,
 *                  when `solved`, row_to_col[n_r2c] over the kept lists (the whole model when no LCM ran):
 *                  analyzeSolution :375-421.  *opt_count = the line's "OPT count", -1 when the LCM ran and solved == 0
 *                  (:188-189, the line has none).  A cab and a request occur in at most one pair, a request in at most
 *                  one row_to_col cell (what td_tick returns); a pair outside the model is TD_EINVAL and applies nothing.
 *   td_sim_step    begin + td_tick(the world's table or NULL, fill big_cost, threshold drop_time, stop_size max_non_lcm) on
 *                  the device lists + apply.  line = {has line, demand, supply, LCM ran, pairs, sent to solver, demand and supply
 *                  of the remainder, OPT count or -1}.
 * Per tick only the counters and the small lists (pairs, kept lists, row_to_col) cross PCIe.  Request ids must be unique
 * and not negative, stands lie in 0 .. n_stands - 1 (at most 2^18 stands), arrival times are not negative: td_sim_create
 * checks it.  Input arrays may be host or device memory.  All calls are synchronous, on the library's one stream.
 * Sequencing: ticks run forward (td_sim_begin with t <= the last begun tick is TD_EINVAL, and so is a begin while a tick
 * with demand waits for its apply); td_sim_model / td_sim_apply need a begun tick with has_demand == 1.  Handles are
 * independent worlds; td_workspace_bytes counts their memory until td_sim_destroy.
 * td_sim_create_dist: the same world on a distance table dist[n_stands * n_stands], row-major, dist[from][to] = the ticks a cab
 * needs from stand `from` to stand `to`; host or device memory; NULL is td_sim_create.  The handle COPIES the table (the caller
 * may free or overwrite it after the call) and keeps the copy and two neighbour bit matrices built from it (2 * n_stands *
 * ceil(n_stands / 32) words) until td_sim_destroy; td_workspace_bytes counts them.  The row is always the stand the cab is at
 * or heads to, as Simulator.java reads dist[][]: a cab arrives when dist[from][to] == t - time_started; a request enters the
 * temp demand iff some client-less cab has dist[cab.to][request.from] < drop_time, a standing client-less cab the temp supply
 * iff some unassigned request has dist[cab.to][request.from] < drop_time; td_pool2 and td_tick get the table; a cab goes to a
 * pick-up iff dist[cab.to][request.from] < drop_time and total_pickup_time grows by dist[cab.from][request.from].  The pooled
 * cab's destination stays the reference's stand arithmetic (from +- pool cost against n_stands, :469-474), which means
 * something on a line only; it is kept as it is.  Symmetry and the triangle inequality are not required.  TD_EINVAL (no
 * handle): n_stands > 4096, a diagonal entry other than 0, any other entry outside 1 .. 0x1fffffff (a 0 between two stands
 * would start a cab that never arrives; three entries must stay below td_pool2's INT_MAX marker).  The entries are checked on
 * the device, on the handle's copy: a refused table has the handle allocated and freed again inside the call, so
 * td_workspace_bytes is back at its earlier value when the call returns.  Every other td_sim_* call works on such a world unchanged.
 * td_sim_state: any pointer may be NULL; cab arrays [n_cabs] (client = the request id, -1 none), request arrays [n_req].
 * td_sim_metrics: Simulator.m in its order: total_dropped, total_pickup_time, total_pickup_numb, total_LCM_used,
 * max_model_size, max_solver_size, max_POOL_MEM_size, max_POOL_size, total_second_passengers. */
typedef struct td_sim td_sim;
#define TD_SIM_N_METRICS 9
TD_API int td_sim_create(int n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost, int n_req,
                         const int32_t *req_id, const int32_t *req_from, const int32_t *req_to, const int32_t *req_at,
                         td_sim **out);
TD_API int td_sim_create_dist(int n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost, int n_req,
                              const int32_t *req_id, const int32_t *req_from, const int32_t *req_to, const int32_t *req_at,
                              const int32_t *dist /* n_stands x n_stands, [from][to]; host or device; NULL: td_sim_create */,
                              td_sim **out);
TD_API int td_sim_destroy(td_sim *s);
TD_API int td_sim_begin(td_sim *s, int t, int32_t info[4]);
TD_API int td_sim_model(td_sim *s, int32_t *cab_to, int32_t *dem_from);
TD_API int td_sim_apply(td_sim *s, int n_pairs, const int32_t *lcm_rows, const int32_t *lcm_cols, int solved, int n_r2c,
                        const int32_t *row_to_col, int32_t *opt_count);
TD_API int td_sim_step(td_sim *s, int t, int32_t line[9]);
TD_API int td_sim_state(td_sim *s, int32_t *c_from, int32_t *c_to, int32_t *c_clnt, int32_t *c_onboard, int32_t *c_start,
                        int32_t *d_cab, int32_t *d_pick, int32_t *d_pool_id, int32_t *d_pool_plan, int32_t *d_pool_cost);
TD_API int td_sim_metrics(td_sim *s, int64_t out[TD_SIM_N_METRICS]);

/* ---- the event log of a world: Simulator.java's second file, simulog.txt (csrc/td_sim_world.h) ----------
 * A record is 8 int32 words {t, world, kind, method, customer, cab, aux, 0}: world = 0 in td_sim; customer = a request ID;
 * cab = the cab number (world-local in td_simb); method = 0 none, 1 LCM, 2 OPT; a word the kind does not use is -1 (method:
 * 0).  Kinds and the Java line that writes them:
 *    1 PICKED_UP       :233      customer, cab             7 POOL_PAIR       :746      customer = custA, aux = custB (ids)
 *    2 CAB_FREE        :251      cab, aux = stand          8 ASSIGNED_PICKED :448-465  customer, cab, method, aux = the pooled
 *    3 DROPPED         :339      customer                                               other customer's id or -1
 *    4 TEMP_DEMAND     :331/352  aux = entries; every      9 HEADING         :486-487  customer, cab, method
 *                                tick and world           10 ASSIGNED_LCM    :654      customer, cab
 *    5 TEMP_DEMAND_ID  :347      customer, list order     11 POOLED_SECOND   :432-433  customer = the second passenger, cab,
 *    6 POOL            :742/756  aux = plans kept; once                                 method
 *                                where findPool ran (demand and supply both non-empty)
 * Order: ticks as they ran; within a tick world 0's records, then world 1's ...; within a tick and world the order in which
 * Simulator.java writes: 1 / 2 by cab; every 3 by request, 4, its 5s; 6, its 7s in plan order; analyzePairs' cab loop (8 / 9,
 * LCM) in supply order; its request loop (10, then that request's 11, LCM) in demand order; analyzeSolution in supply order
 * (a cab's 11 first, then its 8 / 9, OPT).  The device delivers this order; nothing is sorted.
 *   td_sim_log     kinds: bit k set = kind k is recorded; capacity = records the log holds.  Allocates the log and its staging
 *                  (td_workspace_bytes counts them until td_sim_destroy or td_sim_log(s, 0, 0), which switches logging off,
 *                  frees them and discards what is buffered); a second call replaces the log.  Neither the log nor the handle
 *                  grows afterwards.  TD_EINVAL: bits outside 1 .. 11, kinds != 0 with capacity outside 1 .. 2^31 - 1, a call
 *                  while a tick with demand waits for its apply.  Logging is off until this call and then costs nothing: a
 *                  tick launches the kernels it always launched, in instantiations without logging code.
 *   td_sim_events  copies every buffered record, oldest first, to records (host or device memory), sets *n, sets *lost (may
 *                  be NULL) to the records that did not fit since the last successful call, and empties the log.  More than
 *                  max_records buffered: TD_EINVAL, *n = the number buffered, nothing is copied or removed.  Without logging
 *                  *n = 0, *lost = 0.  A full log drops further records and counts them; what it keeps is a prefix of the
 *                  full sequence.  After any td_sim_* call returns the log holds every record of the work done so far (begin,
 *                  apply and step alike; a drain between td_simb_begin and td_simb_apply delivers begin's records of every
 *                  world, the apply's follow world by world).  Logging never changes the world.
 * td_simb_log / td_simb_events: the same for a batch; the log is one for the handle. */
#define TD_EV_PICKED_UP 1
#define TD_EV_CAB_FREE 2
#define TD_EV_DROPPED 3
#define TD_EV_TEMP_DEMAND 4
#define TD_EV_TEMP_DEMAND_ID 5
#define TD_EV_POOL 6
#define TD_EV_POOL_PAIR 7
#define TD_EV_ASSIGNED_PICKED 8
#define TD_EV_HEADING 9
#define TD_EV_ASSIGNED_LCM 10
#define TD_EV_POOLED_SECOND 11
#define TD_EV_ALL 0xffeu
#define TD_EV_WORDS 8
TD_API int td_sim_log(td_sim *s, uint32_t kinds, int64_t capacity);
TD_API int td_sim_events(td_sim *s, int64_t max_records, int32_t *records, int64_t *n, int64_t *lost);

/* ---- B simulator worlds behind ONE handle (a sweep over fleet sizes / request files of one city) -----------------------
 * td_simb is td_sim with a world dimension: B independent worlds in device memory, advanced one tick at a time by one call
 * for all of them; the number of launches and read-backs of a call does not depend on B (csrc/td_simb.hip).
 * The worlds share the city: n_stands, drop_time, max_non_lcm, big_cost and the distances, |a - b| (td_simb_create) or ONE
 * stand-to-stand table for the whole batch (td_simb_create_dist, below); world b has its own n_cabs[b] and
 * its own request table, the slice [req_off[b], req_off[b + 1]) of the concatenated request arrays (it may be empty).
 * Per world, info, line, opt_count, the state arrays and the metrics mean exactly what they mean in td_sim_*; cab numbers,
 * pair indices and row_to_col indices are world-local.  Ragged arrays are packed world after world behind offsets [B + 1]
 * that start at 0 and never decrease.  Input arrays may be host or device memory, and so may the outputs of td_simb_model and
 * td_simb_state; info, line, opt_count and the metrics are host arrays.  All calls are synchronous.
 *   td_simb_create  TD_EINVAL: batch outside 1 .. 65535, n_cabs[b] outside 1 .. 2048, max_non_lcm > 1024 (so that a
 *                   remainder always fits td_tick_batched), n_stands > 2^18, bad offsets, and per world td_sim_create's rules
 *                   for the requests (ids unique within a world and not negative, stands inside the line, times not negative).
 *   td_simb_begin   begins tick t in every world; info[4 b ..] = world b's td_sim_begin info.  A world without demand has
 *                   info = {0,0,0,0} and empty segments in td_simb_model / td_simb_apply (its solved[b] is ignored, its
 *                   opt_count[b] is 0).  If no world has demand the tick is over and no apply follows.
 *   td_simb_model   every world's model: cab_off / cab_to, dem_off / dem_from (demand after pooling; a world without supply
 *                   was not pooled and lists its demand as it is).
 *   td_simb_apply   every world's decisions in one call: world b's pairs lcm_rows / lcm_cols[pair_off[b] .. pair_off[b + 1])
 *                   are read only when its model is larger than max_non_lcm, its row_to_col[r2c_off[b] .. r2c_off[b + 1]) only
 *                   when solved[b]; opt_count[b] as td_sim_apply's.  A pair outside its own world's model is TD_EINVAL,
 *                   applies nothing in ANY world, and the tick keeps waiting for its apply.
 *   td_simb_step    begin + td_pool2_batched's greedy (inside begin) + td_tick_batched(the batch's table or NULL, fill big_cost, threshold
 *                   drop_time, stop_size max_non_lcm) on the device lists + apply; line[9 b ..] = world b's td_sim_step line.
 *                   Its decisions are those two calls' decisions; td_tick and td_tick_batched may break ties between equal
 *                   optima differently, so a world need not take td_sim_step's course.  A world with supply and more than 2048
 *                   requests before pooling in a tick: TD_EINVAL (the message names the world and the count), nothing is
 *                   applied, the tick stays begun and can be finished through td_simb_model / td_simb_apply (td_simb_begin
 *                   pools such a tick world by world with td_pool2).
 *   td_simb_state   td_sim_state of world `world` (TD_EINVAL outside 0 .. B - 1); td_simb_metrics: [B * TD_SIM_N_METRICS].
 * Sequencing is td_sim's for the handle as a whole: time runs forward, a begin while a tick with demand waits for its apply is
 * TD_EINVAL, td_simb_model / td_simb_apply need a begun tick.  A handle does not grow after create (the strided outputs of the
 * two batched calls are part of it, sized from the limits above); td_workspace_bytes counts it until td_simb_destroy.
 * td_simb_create_dist: the same batch on a distance table dist[n_stands * n_stands], row-major, dist[from][to], host or device
 * memory, shared by all worlds of the batch; NULL is td_simb_create.  The table contract is td_sim_create_dist's: the handle
 * COPIES the table (the caller may free or overwrite it after the call) and keeps the copy, two neighbour bit matrices
 * (2 * n_stands * ceil(n_stands / 32) words) and two near bitsets per world (2 * B * ceil(n_stands / 32) words) until
 * td_simb_destroy; td_workspace_bytes counts them.  The row is always the stand the cab is at or heads to (arrival, the two
 * near tests, pick-up, total_pickup_time exactly as td_sim_create_dist states them); td_pool2_batched, td_tick_batched and the
 * per-world td_pool2 of a tick beyond 2048 requests get the table; the pooled cab's destination stays the reference's stand
 * arithmetic.  TD_EINVAL (no handle): td_simb_create's limits, n_stands > 4096, a diagonal entry other than 0, any other entry
 * outside 1 .. 0x1fffffff.  The entries are checked on the device, on the handle's copy: a refused table has the handle
 * allocated and freed again inside the call, so td_workspace_bytes is back at its earlier value when the call returns.  Every
 * other td_simb_* call works on such a handle unchanged; a tick launches two kernels more, whatever B is.
 * When to use which on a table (measured on one MI355X, 64 worlds of 150 cabs on 50 stands): the table batch
 * costs 3 percent over the line batch on the same |a - b| city and is 13.6 to 16.7 times faster than a loop over
 * td_sim_create_dist handles; for a few worlds of about 1000 cabs and more the advice above holds, a loop over td_sim handles.
 * When to use which (measured on one MI355X): many worlds of up to a few hundred cabs: one td_simb handle
 * (64 worlds of 150 cabs: 21 times faster than a loop over td_sim handles); a few worlds of about 1000 cabs and more, where
 * a tick is no longer launch latency and the batched calls give each model one workgroup: a loop over td_sim handles (8
 * worlds of 900 .. 1300 cabs: the loop is 6.4 times faster). */
typedef struct td_simb td_simb;
TD_API int td_simb_create(int batch, const int32_t *n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost,
                          const int32_t *req_off, const int32_t *req_id, const int32_t *req_from, const int32_t *req_to,
                          const int32_t *req_at, td_simb **out);
TD_API int td_simb_create_dist(int batch, const int32_t *n_cabs, int n_stands, int drop_time, int max_non_lcm, int32_t big_cost,
                               const int32_t *req_off, const int32_t *req_id, const int32_t *req_from, const int32_t *req_to,
                               const int32_t *req_at,
                               const int32_t *dist /* n_stands x n_stands, [from][to]; host or device; NULL: td_simb_create */,
                               td_simb **out);
TD_API int td_simb_destroy(td_simb *s);
TD_API int td_simb_begin(td_simb *s, int t, int32_t *info);
TD_API int td_simb_model(td_simb *s, int32_t *cab_off, int32_t *cab_to, int32_t *dem_off, int32_t *dem_from);
TD_API int td_simb_apply(td_simb *s, const int32_t *pair_off, const int32_t *lcm_rows, const int32_t *lcm_cols,
                         const int32_t *solved, const int32_t *r2c_off, const int32_t *row_to_col, int32_t *opt_count);
TD_API int td_simb_step(td_simb *s, int t, int32_t *line);
TD_API int td_simb_state(td_simb *s, int world, int32_t *c_from, int32_t *c_to, int32_t *c_clnt, int32_t *c_onboard,
                         int32_t *c_start, int32_t *d_cab, int32_t *d_pick, int32_t *d_pool_id, int32_t *d_pool_plan,
                         int32_t *d_pool_cost);
TD_API int td_simb_metrics(td_simb *s, int64_t *out);
/* ---- the pooling policy of a world -----------------------------------------------------------------------
 * Until *_pooling is called a world pools as Simulator.java:691 does: the greedy over every ordered pair (TD_POOL_GREEDY,
 * max_loss <= 0), through the calls and kernels it always used.  td_sim_pooling sets one world's policy, td_simb_pooling
 * every world's (mode [B], NULL = greedy everywhere; max_loss [B] doubles, NULL = every ordered pair everywhere; host or
 * device memory).  It takes effect from the next begin, allocates nothing (the batch's per-world flag is part of the handle
 * since create) and nothing per tick.  TD_EINVAL: a mode outside 0 .. 2, a NaN max_loss, a call while a tick with demand
 * waits for its apply; the policy is then unchanged.
 *   TD_POOL_NONE     findPool and analyzePool do not run: the demand after pooling is the demand (copied in list order), no
 *                    TD_EV_POOL / TD_EV_POOL_PAIR record, max_POOL_MEM_size and max_POOL_size untouched.  In a batch the world
 *                    is left out of the pool lists the way a world without supply is.
 *   TD_POOL_GREEDY   td_sim: td_pool2_loss (td_pool2 when max_loss <= 0).  td_simb: td_pool2_batched_v on the device lists,
 *                    ONE call for all policies of the batch; in a tick where some world has more than 2048 requests, world by
 *                    world through td_pool2_loss with that world's max_loss.
 *   TD_POOL_OPTIMAL  the lexicographic optimum of td_pool2_batched(optimal = 1) under max_loss: the most pools, then the least
 *                    cost, each pool in its cheaper candidate direction, listed in ascending (cost, custA, custB), which is the
 *                    plan order of the event log.  td_sim runs the same device code on its one model.  More than 2048 requests
 *                    before pooling in a tick of such a world (with supply): TD_EINVAL from begin, the message names the world
 *                    and the count; the handle is left as a failing td_pool2 inside begin leaves it: the tick counts as begun
 *                    (last tick = t, waiting for its apply), nothing of it was pooled, and it cannot be completed.
 * max_POOL_MEM_size stays n (n - 1) under a rule as well: it counts the pairs examined, not the pairs admitted.
 * max_POOL_size, total_second_passengers and the event records follow from the plans as they always did; analyzePool, the
 * apply kernels, td_tick and td_tick_batched do not know the policy.
 * td_sim_pools / td_simb_pools: the plans of the tick last begun (of world `world`), in plan order: cust_a[i] picks up
 * cust_b[i], indices into that tick's demand list before pooling, plan and cost as td_pool2 states them; host or device
 * destinations.  *n = 0 when no pooling ran (no demand, no supply, fewer than two requests, TD_POOL_NONE).  More plans than
 * max_pools: TD_EINVAL with *n set, nothing copied.  The plans are read where the pool call left them for the event log. */
#define TD_POOL_NONE 0
#define TD_POOL_GREEDY 1
#define TD_POOL_OPTIMAL 2
TD_API int td_sim_pooling(td_sim *s, int mode, double max_loss);
TD_API int td_simb_pooling(td_simb *s, const int32_t *mode /* [B], NULL = greedy */, const double *max_loss /* [B], NULL = every pair */);
TD_API int td_sim_pools(td_sim *s, int max_pools, int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n);
TD_API int td_simb_pools(td_simb *s, int world, int max_pools, int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n);

/* ---- pools of up to four in a world ---------------------------------------------------------------------------
 * td_sim_pooling_n replaces the world's pair policy from the next begin on (the specification: Simulator(pool_n=, pool_wait=,
 * pool_loss=)); a later td_sim_pooling puts the world back on a pair policy.  findPool is then a cascade over the tick's
 * demand list: stage k = k_hi, k_hi - 1, .., k_lo runs on the requests no earlier stage pooled, in list order, and is exactly
 * td_pool_n(k, ...) on that list with max_wait and max_loss_pct for every request, every request a possible first pick-up, the
 * world's table or |a - b|; a list shorter than k yields nothing.  The tick's plans are the stages' records in stage order.
 * analyzePool: every member of a record but its first pick-up leaves the demand and is assigned with it (one second
 * passenger and one pick-up counted per such member); the first pick-up stays, carries the cost, and its cab is kept busy for
 * the cost as with a pair.  There is no route model.  td_sim_state on the OPT path: d_pool_id = the second pick-up's id,
 * d_pool_plan = the pool's size, d_pool_cost = the cost (the LCM path copies no pool info, as with pairs).
 * max_POOL_size: the most plans of a tick, all stages; max_POOL_MEM_size: the most happy plans of a tick, summed over its stages.
 * The first call allocates the wider partner columns and the stage lists for the handle; nothing is allocated per tick.
 * TD_EINVAL, the policy unchanged: sizes outside 2 <= k_lo <= k_hi <= 4, a negative wait or loss, max_happy above 2^22
 * (td_pool_n_batched's limit; <= 0: the default of the call underneath), a call while a tick with demand waits for its apply,
 * k_hi > 2 on a handle that logs.
 * Limits per tick, from the calls underneath: up to 512 requests before pooling a stage is td_pool_n_batched's device code on
 * the one model, up to 2047 td_pool_n with the whole list as first pick-ups (inputs and records stay on the device either
 * way); more than 2047: TD_EINVAL from begin.  More happy plans in a stage than max_happy, or a plan cost above 16383:
 * TD_ERANGE from begin.  After any of these the handle is left as TD_POOL_OPTIMAL's paragraph above states it.
 * td_sim_pools_n: the plans of the tick last begun in plan order (stage order, then td_pool_n's order): a record is 9 ints,
 * 4 pick-ups, 4 drop-offs (-1 behind the pool's size), the cost; members are indices into that tick's demand list before
 * pooling; size[i] is 2 .. 4; host or device destinations.  More plans than max_pools: TD_EINVAL with *n set, nothing copied.
 * td_sim_pools on a world under this policy is TD_EINVAL (the message names td_sim_pools_n), and td_sim_pools_n on a pair
 * world likewise.
 * The event log is cut on purpose: the apply stages own two staging slots per thread and a pool of four needs four, so
 * td_sim_log with a non-zero mask on a world with k_hi > 2 is TD_EINVAL ("not built").  With k_hi == 2 the log works: a pool
 * is a pair, and the records are the specification's.
 * td_simb_pooling_n gives every world of a batch its own such policy: four arrays [B], host or device; k_hi[b] == 0: world b
 * keeps the policy it has (a pair policy of td_simb_pooling, or an earlier one of this call).  td_simb_pooling puts every
 * world back on a pair policy.  The pool call sees every world of the policy at once: round k = 4, 3, 2 is ONE launch of
 * td_pool_n_batched's workgroup-per-model core over the worlds whose cascade has a stage of k (a world of another policy,
 * without supply or with fewer than two requests is an empty model), then one launch for the records and marks and one
 * compaction pass for all worlds: at most three rounds a tick, whatever B is.  A world with more than 512 requests before
 * pooling in a tick: TD_EINVAL from begin, the message names the world and the count; max_happy and the cost limit as above,
 * the message names the world.  td_simb_pools_n(world) / td_simb_pools(world) refuse a world of the other kind.
 * The event log of a batch follows the single world's rule: td_simb_log with a non-zero mask while some world has k_hi > 2, and
 * td_simb_pooling_n that gives a world k_hi > 2 on a batch that logs, are TD_EINVAL ("not built"); with k_hi == 2 in every
 * record world the log works and a world's records are the specification's.  A pair world above 2048 requests before pooling
 * is pooled world by world as in a batch of pair worlds, whatever the record worlds beside it do. */
TD_API int td_sim_pooling_n(td_sim *s, int k_hi, int k_lo, int max_wait, int max_loss_pct, int64_t max_happy);
TD_API int td_simb_pooling_n(td_simb *s, const int32_t *k_hi, const int32_t *k_lo, const int32_t *max_wait, const int32_t *max_loss_pct,
                             int64_t max_happy);
TD_API int td_sim_pools_n(td_sim *s, int max_pools, int32_t *records /* max_pools x 9 */, int32_t *size, int32_t *n);
/* td_sim_pool_buffer: with plan_buffer > 0 every stage of a world under td_sim_pooling_n is
 * td_pool_n_banded(k, ..., plan_buffer, ...) on the device lists, whatever the list's size up to 2047: the same records, and
 * begin no longer returns TD_ERANGE for the number of happy plans (max_happy is not looked at; the cost limit stays).
 * max_POOL_MEM_size stays the sum of the stages' true happy counts.  0 restores the calls above.  TD_EINVAL, nothing changed:
 * a NULL handle, a negative value, a value below 24 * 2047 (the room td_pool_n_banded needs for the largest tick), a call
 * while a tick waits for its apply.  The setting survives td_sim_pooling and td_sim_pooling_n and takes effect at the next
 * begin; a handle that never calls it launches exactly what it did before the call existed. */
TD_API int td_sim_pool_buffer(td_sim *s, int64_t plan_buffer);
/* td_simb_pool_buffer: the same for a batch of worlds.  With plan_buffer > 0 every round k = 4, 3, 2 of a tick
 * is ONE launch of td_pool_n_banded_batched's core over the worlds instead of td_pool_n_batched's: the same records, still at
 * most three pool launches a tick, begin is no longer TD_ERANGE for a world's number of happy plans (max_happy is not looked
 * at; the cost limit and the 512 requests of a world stay), max_POOL_MEM_size stays the sum of the true happy counts.  0
 * restores td_pool_n_batched's core.  TD_EINVAL, the handle unchanged: a NULL handle, a negative value, a value in
 * 1 .. 24 * 512 - 1, a value above 2^22, a call while a tick waits for its apply.  The setting survives td_simb_pooling and
 * td_simb_pooling_n and takes effect at the next begin; a batch that never calls it launches exactly what it did before. */
TD_API int td_simb_pool_buffer(td_simb *s, int64_t plan_buffer);
TD_API int td_simb_pools_n(td_simb *s, int world, int max_pools, int32_t *records /* max_pools x 9 */, int32_t *size, int32_t *n);

/* ---- the route model of a world -----------------------------------------------------------------------------------
 * Without it a pooled cab is busy for the pool's cost through cheat_a_bit and ends at a stand nobody asked for.  With
 * td_sim_route(s, 1) a cab that is dispatched to a customer with a pool record drives the record (the specification:
 * Simulator(route=True)): its stops are the pick-ups in order, then the drop-offs in order, which is the path the record's
 * cost prices.  Standing at the first pick-up it serves stop 0 at the dispatch tick and advances; otherwise it heads there as
 * before and the arrival serves stop 0.  Advancing serves every stop at the stand just reached (a pick-up sets d_pick, a
 * drop-off sets d_drop), then starts for the next stop's stand; with no stop left the cab is free at this stand in this tick.
 * The route lives in the cab, so the LCM path drives a pool as the OPT path does.  Every existing metric is counted where it
 * was.  A customer without a record behaves as before.
 * td_sim_route: on != 0 takes effect from the next begin; the first such call allocates the route storage (8 stop words and a
 * position per cab, the drop-off tick per request, one record column per list, four counters; td_workspace_bytes counts it,
 * td_sim_destroy returns it) and nothing is allocated per tick.  on == 0 stops handing out routes; cabs that are mid-route
 * finish theirs.  TD_EINVAL, nothing changed: a call while a tick waits for its apply, on != 0 on a handle without a
 * td_sim_pooling_n policy or on a handle that logs.  While routes are on td_sim_pooling (back to pairs) is TD_EINVAL, and
 * td_sim_log with a non-zero mask is TD_EINVAL ("not built") on any handle that has route storage.
 * td_sim_route_state: d_drop [n_req] (-1 until dropped off), the position [n_cabs] = the stops of the cab's list already
 * served, the stop words [8 * n_cabs]: request index * 2 + (1: drop-off, 0: pick-up), -1 behind the list; a finished list stays
 * until the cab gets the next one.  Host or device destinations, NULL to skip.  td_sim_route_metrics: drop_numb, ride_time =
 * the sum of d_drop - d_pick over the dropped-off members, solo_time = the sum of their direct ways, max_over_loss = the
 * largest ride * 100 - solo * (100 + max_loss_pct) seen (INT64_MIN before the first drop-off; <= 0 iff every driven ride
 * keeps the loss rule).  Both are TD_EINVAL on a handle that never had routes.  td_sim_state and td_sim_metrics keep their
 * layouts.  A handle that never calls td_sim_route launches the kernels it launched before.
 *
 * A batch routes every world or some of them.  td_simb_route: on[b] != 0 hands out routes in world b from
 * the next begin on (on [B]: host or device); the first call with a world on allocates the route storage of the whole batch
 * (8 stop words and a position per cab of all fleets, the drop-off tick per request, one record column per list, four
 * counters per world, on [B]; td_workspace_bytes counts it, td_simb_destroy returns it) and queues one init launch.
 * on[b] == 0 stops handing out routes in world b; its cabs that are mid-route finish theirs.  A world whose routes are off
 * behaves exactly as in a batch without routes, whatever its neighbours do, and a routed batch queues the kernels of the
 * same batch unrouted, in the same order.  All zeros on a handle that never had routes is TD_OK and allocates nothing.
 * TD_EINVAL, nothing changed: a null handle or on, a call while a tick waits for its apply, on[b] != 0 for a world without
 * a td_simb_pooling_n policy (k_hi[b] == 0: pairs have no drop-off order; the message names the world), a world on in a
 * handle that logs.  While a world's routes are on td_simb_pooling is TD_EINVAL, as is a td_simb_pooling_n call that leaves
 * that world pooling pairs, and td_simb_log with a non-zero mask is TD_EINVAL ("not built") on a handle that has route storage.
 * td_simb_route_state: world `world`'s segment only, as td_sim_route_state of a one-world handle reports it: r_drop [the
 * world's requests], c_pos [its cabs], c_stops [8 * its cabs] with the request index counted from where the world's table
 * begins (-1 stays -1).  Host or device destinations, NULL to skip.  td_simb_route_metrics: TD_SIM_N_ROUTE_METRICS words per
 * world, world after world; a world that never dropped anyone off reports 0, 0, 0, INT64_MIN.  Both are TD_EINVAL on a
 * handle without route storage ("no routes") and for a world outside 0 .. B - 1. */
#define TD_SIM_N_ROUTE_METRICS 4
TD_API int td_sim_route(td_sim *s, int on);
TD_API int td_sim_route_state(td_sim *s, int32_t *r_drop, int32_t *c_pos, int32_t *c_stops /* 8 * n_cabs */);
TD_API int td_sim_route_metrics(td_sim *s, int64_t out[TD_SIM_N_ROUTE_METRICS]);
TD_API int td_simb_route(td_simb *s, const int32_t *on /* [B] */);
TD_API int td_simb_route_state(td_simb *s, int world, int32_t *r_drop, int32_t *c_pos, int32_t *c_stops /* 8 * n_cabs of the world */);
TD_API int td_simb_route_metrics(td_simb *s, int64_t *out /* B * TD_SIM_N_ROUTE_METRICS */);

/* ---- the dispatch policy of a world ------------------------------------------------------------------------------
 * Until *_dispatch is called a world dispatches as Simulator.java:163-208 does, "the LCM down to max_non_lcm, then the
 * optimum", with the max_non_lcm it was created with, through the calls and kernels it always used.  td_sim_dispatch sets one
 * world's method (TD_DISPATCH_*, above), its max_non_lcm and, for the split, the number of parts over the n_stands stands;
 * td_simb_dispatch every world's (mode, max_non_lcm, parts: int32[B] each, host or device memory; NULL = lcm+opt everywhere /
 * the max_non_lcm the handle was created with / 4).  It takes effect from the next begin and allocates nothing, then or per
 * tick (the batch's per-world rule is part of the handle since create).  TD_EINVAL, the policy unchanged: a mode outside
 * 0 .. 3, a negative max_non_lcm, a max_non_lcm above 1024 in a batch, parts outside 1 .. min(32, n_stands) for a split world,
 * a call while a tick with demand waits for its apply.
 * "The LCM ran" is then the world's rule, wherever it is evaluated (the apply kernels, the kept lists, the event log, the
 * line, total_LCM_used): TD_DISPATCH_LCM_OPT: the model is larger than the world's max_non_lcm; TD_DISPATCH_LCM: always,
 * with supply; TD_DISPATCH_OPT and TD_DISPATCH_SPLIT: never.
 *   td_sim_step    LCM_OPT: td_tick with the world's max_non_lcm.  OPT: td_tick with stop_size -1.  LCM: td_tick with stop_size
 *                  0, applied without a solution: line = {1, d, s, 1, k, 0, d - k, s - k, -1}.  SPLIT: td_dispatch_batched's
 *                  device code on the one model (cells below drop_time, parts ranges over n_stands), applied as a solution
 *                  over the whole model: decisions are logged with the method word of the optimum, max_solver_size takes the
 *                  whole model size, line = {1, d, s, 0, 0, 0, d, s, OPT count} as for OPT.  A split model with more than
 *                  1024 cabs or requests: TD_EINVAL, the message names the tick and the counts; the tick stays begun and is
 *                  finished through td_sim_model / td_sim_apply.  td_dispatch_batched's refusals apply (a table entry used as
 *                  a cell must lie below big_cost).
 *   td_simb_step   when some world's policy is not the handle's own (lcm+opt with the created max_non_lcm): ONE
 *                  td_dispatch_batched on the device lists with the policy arrays (2 launches, 7 when a world splits) instead of
 *                  td_tick_batched; else td_tick_batched exactly as before.  A split world's or an optimum-alone world's model
 *                  with more than 1024 cabs or requests: TD_EINVAL, the message names the world and the counts; the tick stays
 *                  begun and is finished through td_simb_model / td_simb_apply.  The lines are td_sim_step's per world.
 *   td_sim_apply   with decisions from elsewhere follows the same rule: pairs are read only where the LCM ran under the world's
 *                  policy, `solved` is ignored in a TD_DISPATCH_LCM world (nothing is solved there), row_to_col is over the
 *                  whole model in OPT and SPLIT worlds (the request of each cab). */
TD_API int td_sim_dispatch(td_sim *s, int mode, int max_non_lcm, int parts);
TD_API int td_simb_dispatch(td_simb *s, const int32_t *mode, const int32_t *max_non_lcm, const int32_t *parts); /* [B] each, NULL = as created / 4 */

/* the batch's event log: td_sim_log / td_sim_events above with a world word; ONE log for the handle, within a tick world 0's
 * records first; the number of launches the log adds to a tick (three kernels, two fills) does not depend on B */
TD_API int td_simb_log(td_simb *s, uint32_t kinds, int64_t capacity);
TD_API int td_simb_events(td_simb *s, int64_t max_records, int32_t *records, int64_t *n, int64_t *lost);

/* ---- f-3 pool of two (the step right before the path in every tick) -------------------
 * Replaces findPool: Simulator.java:681-758 (and pool.c:64-131): every ordered pair (A, B) of
 * requests is a candidate with cost = min(plan1, plan2) (:693-717); plans are taken in STABLE
 * order of cost (insertion order A-major, then B) and kept iff neither customer is in an earlier
 * kept plan (:729-739).  Implemented as the lowest-cost method with symmetric masking on the
 * n x n pair-cost matrix (same kernels as td_lcm).  Outputs up to n/2 plans in the reference's
 * order: cust_a[i] picks up cust_b[i]; plan[i] = 1 (CLNT_B_ENDS) iff cost1 < cost2 else 0.
 */
TD_API int td_pool2(int n, const int32_t *from, const int32_t *to, const int32_t *dist, int S,
                    int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n_pairs);
/* td_pool2_loss: td_pool2 under the reference's own candidate rule (pool_opt_min.py:56-64, Simulator.java's unread
 * max_loss = 1.01).  max_loss <= 0 (or NaN) is td_pool2, call for call.  max_loss > 0: the ordered pair (A, B) is a
 * candidate iff plan 1 or plan 2 passes its loss test, compared in double (the one definition, csrc/td_pool_rule.h, is
 * td_pool2_batched's); a refused pair carries the diagonal's INT_MAX marker in the pair-cost matrix and the greedy ends
 * where the candidates do, so fewer than n / 2 plans, or none, may come back.  plan and cost are those of the pair whether
 * or not its cheaper plan passed.  The model is spread over the device exactly as td_pool2's (same kernels, same paths,
 * same lcm_path stats word, no n beyond td_pool2's); for n <= 2048 the result equals td_pool2_batched(batch = 1,
 * optimal = 0, max_loss).  Errors are td_pool2's. */
TD_API int td_pool2_loss(int n, const int32_t *from, const int32_t *to, const int32_t *dist, int S, double max_loss,
                         int32_t *cust_a, int32_t *cust_b, int32_t *plan, int32_t *cost, int32_t *n_pairs);

/* ---- maximum-weight matching of MANY general graphs, and optimal pools of two (pool_opt_min.py, pool_optimum.py) -------
 * One workgroup (one wave) per model runs the primal-dual weighted blossom method (Edmonds; Galil's O(n^3) form) in exact
 * int64 arithmetic (csrc/td_match.hip, csrc/td_match_core.h); no launch or host synchronisation per model.  Arrays may be
 * host or device memory (outputs too); calls are synchronous; batch == 0 is a no-op; cells are indexed in 64 bits.
 *
 * td_match_batched: the slab layout of td_assign_batched (model b = the top-left ns[b] x ns[b] block of slab b; ns may be
 *   NULL = every model is n x n), n <= 2048.  Edge {i, j} (i != j) has weight max(W[i][j], W[j][i]); a weight <= 0 is no
 *   edge; the diagonal is never read.  Outputs: mate[b*n + i] = the partner of i or -1; total[b] = the matched weight;
 *   dual_bound[b] (may be NULL) = the dual objective, recomputed on the device after every pair of the model was checked
 *   against the duals: dual_bound == total certifies the maximum.  Optional duals, in doubled units (NULL = not wanted):
 *   dual_vertex[b*n + i] = y_i; blossom_parent[b*2n + id] = the parent blossom of node id (vertices 0..n-1, blossoms
 *   n..2n-1; -1 = top level; an id with no vertex under it is unused); dual_blossom[b*n + k] = z of blossom n + k.  They
 *   satisfy 2 w_ij <= y_i + y_j + sum of z_B over the blossoms holding i and j, y, z >= 0, y_i = 0 for unmatched i, every
 *   blossom with z_B > 0 is full, and dual_bound = (sum y + sum z_B * floor(|B| / 2)) / 2.
 *   TD_EINVAL: n > 2048, batch < 0, ns[b] outside [0, n]; TD_EINTERNAL: a defensive loop cap or a violated pair.
 *
 * td_pool2_batched: B ragged pool models, customers from[off[b] .. off[b+1]) -> to[...] (positions within the model are the
 *   customer indices), one shared table (dist S x S, or NULL = |a - b|).  n: the output stride, every model size <= n <= 2048;
 *   model b's pools sit at b*(n/2): cust_a picks up cust_b, plan = 1 (CLNT_B_ENDS) iff cost1 < cost2, cost = min(cost1, cost2);
 *   n_pools[b], total[b] = the sum of the listed costs.  Candidates (pool_opt_min.py:56-64): with max_loss > 0 the ordered
 *   pair (A, B) is one iff plan 1 or plan 2 passes its loss test (compared in double); with max_loss <= 0 every ordered pair
 *   is (Simulator.java:691, td_pool2).
 *     optimal = 0: the greedy (stable sort by cost, A-major then B; keep a pair iff it shares no customer with an earlier kept
 *       one), in the reference's keep order; with max_loss <= 0 it equals td_pool2 model by model.
 *     optimal = 1: the lexicographic optimum, the most pools and among those the least total cost, each pool in its cheaper
 *       candidate direction (the smaller cust_a on a tie), listed in ascending (cost, cust_a, cust_b).
 *   TD_EINVAL: n > 2048, batch < 0, bad offsets, a model larger than n, a stand outside the table, null outputs; TD_ERANGE:
 *   a pair cost outside int32, or (optimal = 1 only) pool weights K - cost, K = floor(m/2) * cost span + 1, of 2^33 or more;
 *   TD_EINTERNAL as above.
 *
 * td_pool2_batched_v: td_pool2_batched with a policy per model.  max_loss [batch] doubles (NULL = every ordered pair
 *   everywhere), optimal [batch] int32, each 0 or 1 (NULL = greedy everywhere; any other entry is TD_EINVAL before anything
 *   is written); host or device memory.  Model b is exactly td_pool2_batched with the scalars max_loss[b], optimal[b] on that
 *   model alone; the TD_ERANGE weight check applies to the optimal models only.  The launches of a call do not depend on the
 *   batch or on the mix: with an optimal array both the greedy and the matching kernel run and each sees the models of the
 *   other kind as empty.  td_pool2_batched is the uniform case of the same code. */
TD_API int td_match_batched(int batch, int n, const int32_t *ns, const int32_t *weight, int32_t *mate, int64_t *total,
                            int64_t *dual_bound, int64_t *dual_vertex, int32_t *blossom_parent, int64_t *dual_blossom);
TD_API int td_pool2_batched(int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to, const int32_t *dist,
                            int S, double max_loss, int optimal, int32_t *cust_a, int32_t *cust_b, int32_t *plan,
                            int32_t *cost, int32_t *n_pools, int64_t *total);
TD_API int td_pool2_batched_v(int batch, int n, const int32_t *off, const int32_t *from, const int32_t *to, const int32_t *dist,
                              int S, const double *max_loss, const int32_t *optimal, int32_t *cust_a, int32_t *cust_b,
                              int32_t *plan, int32_t *cost, int32_t *n_pools, int64_t *total);

/* ---- f-4 pools of up to 4 passengers ---------------------------------------------------
 * Replaces pool_n.c:101-207 (findPool / drop_customers / removeDuplicates; Pool.java:32-113 is the
 * same enumeration) for ONE first-pick-up slice [first0, first1) — the unit findpool.c:138-141 hands
 * to each of its 8 children (child t: first0 = t * (n/8 + 1), pool_n.c:243-246) — and the merge of
 * the children's lists (findpool.c:73-98,166-172).
 *   requests i = 0..n-1: from[i], to[i], max_wait[i] (pick-up path up to i may not be longer),
 *   max_loss[i] (percent a pooled ride may exceed the direct one);  dist: S x S or NULL => |a-b|.
 *   pools: max_pools records of 2k+1 ints (k pick-ups, k drop-offs, cost) in the reference's output
 *   order (stable by cost, de-duplicated); a max_pools below the length of that list keeps its first
 *   max_pools records (td_pool_merge alike) and nothing is written behind them;  n_happy: happy plans
 *   before de-duplication;  max_happy:
 *   capacity of the plan buffer (<= 0: 4 Mi plans; TD_ERANGE when exceeded — the reference's
 *   pool[10000] simply overflows there).
 *   k = 2, 3 or 4 passengers (TD_EINVAL otherwise: with k = 1 the reference's duplicate test compares its 4 padded slots
 *   and keeps a single pool, which is not reproduced).
 *   td_pool_n: n <= 2047 (TD_EINVAL above); TD_ERANGE when a happy plan costs more than 16383 (n_happy is still set).
 *   td_pool_merge: n_requests <= 2047 (TD_EINVAL above).  Precondition on pools_in (host or device memory): the first k
 *   fields of every record, the requests, lie in [0, n_requests).  It is checked on the device before the de-duplication
 *   runs: an input with a request outside that range is refused with TD_EINVAL, td_last_error() names the first such record
 *   and the id, *n_out = 0 and nothing is written to pools_out.
 */
TD_API int td_pool_n(int k, int n, const int32_t *from, const int32_t *to, const int32_t *max_wait,
                     const int32_t *max_loss, const int32_t *dist, int S, int first0, int first1,
                     int64_t max_happy, int max_pools, int32_t *pools, int32_t *n_pools, int64_t *n_happy);
TD_API int td_pool_merge(int k, int n_requests, int n_in, const int32_t *pools_in /* n_in * (2k+1) */,
                         int sort_by_cost, int max_pools, int32_t *pools_out, int32_t *n_out);

/* ---- f-4 in a bounded plan buffer --------------------------------------
 * td_pool_n_banded: td_pool_n's arguments, rules and answer (host or device arrays, the first-pick-up slice, k = 2..4,
 *   n <= 2047, the empty cases, TD_ERANGE for a plan cost above 16383 with n_happy still set): pools[0 .. n_pools) and n_pools
 *   are, record for record, what td_pool_n returns on the same input with room for every happy plan, and n_happy is the true
 *   number of happy plans.  It never fails for the number of happy plans.
 *   plan_buffer: the most plan keys the call holds at once (<= 0: 4 Mi).  The keys' ascending order is the reference's stable
 *   sort and the de-duplication only reads them in that order, so it runs over consecutive key intervals ("bands"), each
 *   enumerated, sorted and scanned on its own with the set of used requests carried along; a plan with a used request is
 *   never stored.  A band is the longest run of costs that fits; where one cost alone does not fit it is cut at the first
 *   pick-up, then the second, and so on: one value of the last digit but one holds at most (n - k + 1) k! <= 24 n plans, so
 *   the only new refusal is plan_buffer < 24 n (TD_EINVAL, the message has both numbers, no output written).  Workspace
 *   grows with plan_buffer (two key arrays and the sort's scratch), not with the plan count; time grows with the bands:
 *   every band costs one counting pass per level it is cut at and one enumeration pass.
 *   stats (may be NULL): [0] bands, [1] enumeration passes in all, counting passes included, [2] the deepest level a band was
 *   cut at (0: at a cost, l: at pick-up l - 1; at most k - 1), [3] the most keys held in one band.  All 0 in the empty cases.
 */
TD_API int td_pool_n_banded(int k, int n, const int32_t *from, const int32_t *to, const int32_t *max_wait,
                            const int32_t *max_loss, const int32_t *dist, int S, int first0, int first1,
                            int64_t plan_buffer, int max_pools, int32_t *pools, int32_t *n_pools,
                            int64_t *n_happy, int64_t stats[4] /* may be NULL */);

/* ---- f-4 for MANY models per call ------------------------------------------------------
 * td_pool_n_batched: B ragged models, model b = requests [off[b], off[b+1]) of the concatenated from / to / max_wait /
 *   max_loss arrays (request indices in the output are positions within the model), one shared table (dist S x S, or NULL
 *   = |a - b|).  n: the output stride, every model size n_b <= n <= 512 (a larger model stays td_pool_n over slices).
 *   Arrays may be host or device memory (outputs too); the call is synchronous; batch == 0 is a no-op.  One workgroup per
 *   model enumerates, selects and writes the records (csrc/td_pool_batch.hip): no launch, sort or host synchronisation per
 *   model.
 *   Model b is exactly td_pool_n(k, n_b, ..., first0, first1, ...) on its own requests: the same wait rule (the level-0 test
 *   0 > max_wait[p0] included), the same happiness test in double with 1 + loss / 100.0, the same cost, the same order
 *   (stable by cost, the reference's enumeration order among equal costs) and the same de-duplication.  first == NULL:
 *   every request may be the first pick-up; else first[2b], first[2b+1] is model b's first-pick-up slice, clamped to
 *   [0, n_b] as td_pool_n clamps it: findpool.c's 8 children are 8 models of one batch (the same demand, 8 slices).  An
 *   empty slice or n_b < k gives 0 pools and 0 happy plans.
 *   pools: records of 2k+1 ints (pick-ups, drop-offs, cost), model b's from b * (n / k) * (2k + 1); a model keeps at most
 *   n_b / k pools, so nothing is truncated; nothing is written behind a model's n_pools[b] records; may be NULL when
 *   n / k == 0.  n_pools[B];  n_happy[B] (may be NULL): happy plans before de-duplication;  total[B] (may be NULL): the sum
 *   of the listed costs.
 *   max_happy: the most happy plans one model may have (<= 0: 65536; at most 2^22).  Plan storage is (workgroups in flight)
 *   x max_happy 8-byte keys, workgroups in flight = min(1024, 1 GiB / (8 max_happy)) whatever the batch: grow-only, counted
 *   by td_workspace_bytes, released by td_shutdown; inputs and results are staged in one block that grows in 4 MiB steps.
 *   TD_EINVAL, every output unwritten: k outside 2..4, batch < 0, n outside [0, 512], off[0] != 0, a decreasing offset, a
 *   model larger than n, a null required array, dist with S <= 0, max_happy > 2^22, and, with a table, a from / to outside
 *   [0, S) (checked on the device; td_last_error() names the first such model).  TD_ERANGE when some model has more than
 *   max_happy happy plans (the message names the first such model and its count; n_happy[] is still written for every
 *   model, nothing else is), or when a happy plan's cost is negative or above 16383 (td_pool_n's limit; nothing is written).
 *   When to use which: td_pool_n_batched for many models of at most 512 requests each.  Measured on one MI355X (host clock,
 *   host arrays): 1000 models x 100 requests take 3.80 / 4.13 / 8.90 ms at k = 2 / 3 / 4 against 104 / 163 / 833 ms for a loop
 *   of td_pool_n (27x / 39x / 94x); 1000 x 40: 29x / 36x / 70x; 64 x 256: 9.8x / 5.1x / 3.4x; findpool.c's 8 children of the
 *   committed fixture demands (40..400 requests) as one batch: 2.1x .. 11.2x.  No measured shape has the loop ahead.  td_pool_n remains the call for one model,
 *   for any model above 512 requests and for more than 2^22 happy plans per slice.
 */
TD_API int td_pool_n_batched(int k, int batch, int n, const int32_t *off,
                             const int32_t *from, const int32_t *to, const int32_t *max_wait, const int32_t *max_loss,
                             const int32_t *dist, int S, const int32_t *first /* [2*batch] or NULL */,
                             int64_t max_happy, int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *total);

/* ---- f-4 for MANY models per call in a bounded plan slab ----------------
 * td_pool_n_banded_batched: td_pool_n_batched's arguments, layout, staging and rules (host or device memory for every array,
 *   batch == 0 a no-op, a refused call writes no output), with td_pool_n_banded's band loop run inside the workgroup: model
 *   b's records, n_pools[b] and total[b] are what td_pool_n_batched writes for model b with room for every plan, n_happy[b]
 *   is the true number of happy plans, and the call is never refused for the number of happy plans.  One launch; no host
 *   round trip, sort call or launch per band or per model.
 *   plan_buffer: the most plan keys a workgroup holds at once (<= 0: 65536; at most 2^22).  Plan storage is (workgroups in
 *   flight) x plan_buffer 8-byte keys, workgroups in flight = min(1024, 1 GiB / (8 plan_buffer)), plus 128 KiB of cost
 *   counters per workgroup in flight; grow-only, counted by td_workspace_bytes, released by td_shutdown.
 *   stats (may be NULL): [4 * batch], model b's four numbers at 4 b as td_pool_n_banded defines them: bands, enumeration
 *   passes in all, the deepest level a band was cut at, the most keys held in one band.  All 0 for an empty model.
 *   TD_EINVAL, every output unwritten: td_pool_n_batched's refusals (k, batch, n, the offsets, a model larger than n, a null
 *   required array, dist with S <= 0, a stand outside the table), plan_buffer above 2^22, and plan_buffer below 24 x the
 *   requests of some model (the message names the first such model and both numbers).  TD_ERANGE: a happy plan's cost is
 *   negative or above 16383.
 *   When to use which, measured on one MI355X (host clock, host arrays): lists that fit are answered faster by
 *   td_pool_n_batched (one walk instead of at least two): 1000 x 100: 1.08 / 1.13 / 1.71 times its time at k = 2 / 3 / 4,
 *   64 x 256: 1.23 / 1.91 / 2.82.  64 models of 256 requests with 0.6 / 1.1 million plans each (k = 3 / 4), buffer 65 536:
 *   1.25 / 3.82 times td_pool_n_batched(max_happy = 2^22) on its 32 workgroups, and 7.2 / 2.7 times faster than a loop of
 *   td_pool_n_banded.  So: td_pool_n_batched while every list fits a max_happy up to 2^22; this call when some model may not
 *   fit or the slab must stay small; td_pool_n_banded for one model.
 */
TD_API int td_pool_n_banded_batched(int k, int batch, int n, const int32_t *off,
                                    const int32_t *from, const int32_t *to, const int32_t *max_wait, const int32_t *max_loss,
                                    const int32_t *dist, int S, const int32_t *first /* [2*batch] or NULL */,
                                    int64_t plan_buffer, int32_t *pools, int32_t *n_pools, int64_t *n_happy, int64_t *total,
                                    int64_t *stats /* [4*batch] or NULL */);

/* ---- a-7 objective evaluation  (greedy_opt.py:21-29 count_sum) ---------------------- */
TD_API int td_count_sum(int n, const int32_t *cost, const int32_t *row_to_col, int64_t big_cost,
                 int64_t *sum, int32_t *n_real);

/* ---- a-10 synthetic instances (bench / tests) --------------------------------------
 * perf.jl:5  t = rand(lo:hi, n, n)  as a counter-based hash so that host oracle, one GPU
 * and each row shard generate identical cells: cell(i,j) = lo + mulhi32(hi32(splitmix64(
 * seed*0x100000001B3 + i*n + j)), hi-lo+1).  Writes rows [row0, row0+nrows).
 */
TD_API int td_gen_uniform(int n, uint64_t seed, int32_t lo, int32_t hi, int row0, int nrows,
                   int32_t *cost /* nrows*n */);

/* ---- multi-GPU: row-sharded solve ---------------------------------------
 * One process per GPU.  Rank r owns cost rows [row0, row0+nrows) x all n columns; prices and
 * column owners are replicated.  The exchange step between ranks (one MAX all-reduce of the
 * packed 64-bit bid keys per bidding round) is done by the CALLER with torch.distributed /
 * RCCL on the key buffer, or by the library itself (td_shard_rounds below).  Host driver:
 * taxidispatcher_amd/sharded.py.
 *   td_shard_compress   narrow working copy of the local rows (1, 2 or 4 bytes per cell); every
 *                       rank must end up with the same width (caller reduces `fits` with MIN)
 *   td_shard_const_rows constant rows (dummy cabs of a padded model, greedy_opt.py:88-90) sit out the solve as in
 *                       td_assign: after td_shard_compress, before td_shard_begin, every rank marks its constant
 *                       rows in a zeroed device mask of n ints (set = 0), the caller SUM-all-reduces the mask and
 *                       gives it back (set = 1); the finisher's rank then hands those rows the left-over columns
 *   td_shard_options    flags bit 0 = "this caller runs td_shard_const_rows in every solve": a wide shard's 1-byte
 *                       compress pass may then initialise the state, defer the constant rows and write round 0's
 *                       bids itself, as td_assign does (same keys; td_shard_bid(0) only hands them over)
 *   td_shard_bid        one Jacobi bidding round over the local free rows; writes keys[j] =
 *                       (price << 20 | global_row + 1) with atomicMax, 0 = no bid
 *   td_shard_apply      applies the globally reduced keys (identical on every rank) and zeroes them
 *   td_shard_finish     augmenting-path finisher on the calling rank; shard_ptrs[k] is the base of
 *                       shard k's compressed rows as visible from this device (own memory, peer
 *                       memory mapped with td_ipc_open over xGMI, or a gathered copy)
 *   td_shard_owner      get (set=0) / set (set=1) the replicated owner[] (n ints)
 *   td_shard_total      this shard's part of the total (and of the dual bound); caller sums
 */
typedef struct td_shard td_shard;
TD_API int td_shard_create(int n, int row0, int nrows, const int32_t *cost_rows, td_shard **out);
TD_API int td_shard_destroy(td_shard *s);
TD_API int td_shard_compress(td_shard *s, int bytes_per_cell, int *fits);
/* largest row cost range (max - min) this shard has seen so far; the caller reduces it with MAX over
 * the ranks and hands the result to td_shard_begin, which applies td_assign's TD_ERANGE guard
 * ((range + 1) * (n + 1) must stay below 4e12: the packed bid key holds price << 20 | row) */
TD_API int td_shard_range(td_shard *s, int64_t *range);
TD_API int td_shard_begin(td_shard *s, int64_t global_range /* < 0: use this shard's own */);
TD_API int td_shard_keys_len(td_shard *s);
TD_API int td_shard_bid(td_shard *s, int round, uint64_t *keys);
TD_API int td_shard_apply(td_shard *s, int round, uint64_t *keys);
TD_API int td_shard_cc(td_shard *s, void **ptr, uint64_t *bytes);
/* All bidding rounds in ONE call: per round  td_shard_bid -> RCCL MAX all-reduce of the keys -> td_shard_apply,
 * enqueued back to back on the library's stream (no host work between the rounds).  The communicator is
 * the library's own: rank 0 makes a 128-byte id (td_comm_unique_id), the caller broadcasts it with whatever
 * it has (torch.distributed), every rank calls td_comm_init.  librccl.so is dlopen'ed on first use. */
TD_API int td_comm_unique_id(void *id128);
TD_API int td_comm_init(int world, int rank, const void *id128);
TD_API int td_comm_destroy(void);
TD_API int td_shard_rounds(td_shard *s, int rounds, uint64_t *keys);
TD_API int td_shard_finish(td_shard *s, int world, const void *const *shard_ptrs, int rows_per_shard);
TD_API int td_shard_owner(td_shard *s, int32_t *owner, int set);
TD_API int td_shard_price(td_shard *s, int64_t *price /* n, device */, int set);
TD_API int td_shard_total(td_shard *s, int64_t *partial_total, int64_t *partial_dual);
/* the same into three int64 words of DEVICE memory, no host round trip: {partial total, partial dual bound, error / void-attempt
 * flags}; the caller SUM-all-reduces them and reads them once (word 2 != 0: an error on some rank) */
TD_API int td_shard_total_dev(td_shard *s, int64_t *out3 /* device */, int want_dual);
TD_API int td_shard_const_rows(td_shard *s, int32_t *mask_full, int set);
TD_API int td_shard_options(td_shard *s, int flags);
TD_API int td_shard_row_to_col(td_shard *s, int32_t *r2c_local);
/* BLOCK-LOCAL START of the sharded solve (csrc/td_blocks.h; what SURVEY 8e's "one exchange per round" costs at
 * N = 65 536 over 8 GPUs is the exchanges, not the rounds).  With td_shard_options(flags = 3) the 1-byte compress
 * pass of a shard that owns whole diagonal blocks (n / 8 rows x the same columns) writes, for every row, a bid for
 * the first ZERO cell of the row's own column slice; td_shard_phase_a then runs a few bidding rounds and a two-hop
 * augmentation pass on the zero cells of those blocks — no price moves, every pair is tight, nothing is exchanged.
 * The ranks then meet ONCE: td_shard_state_export writes this rank's segment (td_shard_state_words int32 words of
 * device memory: fits / ran / free rows left / constant rows / range, the owners of its column slice, the
 * constant-row flags of its rows), the caller all-gathers the segments in rank order, td_shard_state_import fills in
 * the other slices (owners, owned bits, the replicated constant-row mask of td_shard_const_rows) and returns
 * summary[0..5] = {all ranks fit, all ran phase A, free rows left in total, constant rows, largest row range, rank 0's segment
 * word 6 (free for the caller: solve_sharded carries the line-metric attempt's plausibility word there)}.
 * The ordinary rounds (td_shard_bid / _apply / _rounds) and td_shard_finish take what is still free; when
 * summary[2] == 0 the solve is complete, except that td_shard_place_const is still due when summary[3] > 0 (the constant
 * rows sat out phase A).  flags bit 2 (flags = 7): the compress pass stores the 1-byte cells of the
 * diagonal slices only (all that phase A reads: 1/8 of the narrow copy); the library writes the other cells by itself
 * the first time a call needs whole rows (td_shard_bid / _rounds, td_shard_cc — where the pointers td_shard_finish reads
 * through come from —, the dual bound of td_shard_total) — never, when phase A leaves nothing.  td_assign starts the same way for n >= 12 288 (td_set_blocks),
 * so a sharded run and td_assign with the same block count stay bit-identical. */
TD_API int td_shard_compress_spec(td_shard *s);   /* the 1-byte compress pass without waiting for its width flag (it travels in the segment) */
TD_API int td_shard_blocks_pending(td_shard *s);
TD_API int td_shard_phase_a(td_shard *s);
TD_API int td_shard_state_words(td_shard *s, int rows_per_shard);
TD_API int td_shard_state_export(td_shard *s, int rows_per_shard, int fits, int32_t *seg /* device */);
TD_API int td_shard_state_import(td_shard *s, int world, int rank, int rows_per_shard, const int32_t *all /* device */,
                                 int64_t *summary6 /* host, 6 words */);
/* summary[2] == 0 with constant rows in the model: every rank places them itself from the replicated owner[] and mask
 * (k-th constant row <- k-th column nobody owns, what td_shard_finish does on its rank) — no finisher, no exchange */
TD_API int td_shard_place_const(td_shard *s);
/* diagonal blocks td_assign starts in: 0 = never, > 0 = that many (n must be a multiple of 16 * blocks, n >= 12 288),
 * -1 = by size (8 from n = 12 288 on, where the 1-byte compress pass can write the bids).  Returns the previous setting. */
TD_API int td_set_blocks(int blocks);
/* The sorted matching of td_assign's line-metric path (cost = |a_i - b_j|, perf.jl's G2 family) over ROW SHARDS.
 * Replaces the same call as td_assign (simulator.py:199 / munkres.c solve / greedy_opt.py:95), for matrices one
 * GPU cannot hold.  `ws` is td_line_shard_ws_words(n) 64-bit words of device memory owned by the caller.  Every
 * rank runs phases 0, 1, 2, 3 in order and after EACH phase SUM-all-reduces ws[*seg_off .. *seg_off + *seg_len)
 * with the other ranks (the segments are written disjointly and zero elsewhere, so the sum is the exchange; with
 * one rank there is nothing to do).  phase 0: anchors from the rank that owns row 0; 1: row keys; 2: replicated
 * sort, local matched cells and neighbours; 3: replicated prices, certificate pass over the local rows.
 * td_line_shard_result (after phase 3's exchange): *accepted = 1 when every rank's rows certify the matching
 * (then it is optimal, whatever the matrix was), *total its cost, row_to_col[0..nrows) (host or device) the
 * columns of the local rows.  *accepted = 0: use the general sharded solve (td_shard_*). */
TD_API int64_t td_line_shard_ws_words(int n);
TD_API int td_line_shard_phase(int phase, int n, int row0, int nrows, const int32_t *cost_rows, int64_t *ws, int64_t *seg_off,
                               int64_t *seg_len);
TD_API int td_line_shard_result(int n, int row0, int nrows, const int64_t *ws, int32_t *row_to_col, int64_t *total, int32_t *accepted);
TD_API int td_ipc_export(const void *dev_ptr, void *handle64);
TD_API int td_ipc_open(const void *handle64, void **dev_ptr);
TD_API int td_ipc_close(void *dev_ptr);
TD_API int td_memcpy(void *dst, const void *src, uint64_t bytes);

/* ---- profiling hooks used by bench.py ---------------------------------------------- */
#define TD_K_COST_BUILD 0
#define TD_K_GEN 1
#define TD_K_COMPRESS 2
#define TD_K_BID 3
#define TD_K_ASSIGN 4
#define TD_K_SAP 5
#define TD_K_FINAL 6
#define TD_K_LCM 7
#define TD_K_LINE 8   /* line-metric recogniser: anchors, keys, sort, prices */
#define TD_K_CERT 9   /* ... and its certificate pass over the int32 matrix */
#define TD_K_COUNT 10
TD_API int td_profile_enable(int on);                      /* HIP-event timing per kernel class */
TD_API int td_profile_get(int kernel, double *total_ms, int64_t *launches);
TD_API int td_profile_reset(void);
/* counters of the last td_assign: [0]=bid rounds, [1]=rounds of the eps > 0 price warm start,
 * [2]=free rows left to the serial finisher, [3]=its dijkstra steps, [4]=cost storage bytes per cell,
 * [5]=augmentations committed by the parallel finisher, [6]=1 when 4-byte cells were solved with 32-bit prices and labels,
 * [7]=1 when the transposed formulation was solved
 * (many constant columns, see DESIGN.md "rectangular models"),
 * [8]=1 when the matrix was recognised as a line metric: sorted matching, proven by the certificate pass
 * (then [0..6] are 0 except [4]=4, [7]=1 when it was the transpose that was recognised (constant trailing columns),
 * [9] = number of constant rows of the unbalanced model; see DESIGN.md "line-metric instances").
 * [11] = lcm_path, the path the last td_lcm / td_pool2 took, as a bit set (DESIGN.md section 3 has the thresholds):
 *     1  level lists (otherwise the row-scan loop)        2  lists built with one workgroup per row (n <= 4096)
 *     4  loop: narrow byte copy made (n >= 128)           8  loop: row keys held in LDS
 *    16  lists: value range hinted by the caller (td_tick)
 *    32  redone with the measured range after a wrong hint (the other bits are those of the second run)
 *    64  pairs returned through the pinned block          128  called as td_pool2
 *   Word [11] is set to 0 when td_lcm / td_pool2 is entered and filled in before it returns; it is defined only right
 *   after such a call.  Other calls may clear it (td_assign zeroes all 16 words on its line-metric path).
 * [12] = line_path, what the last td_assign's line-metric attempt did, as a bit set (DESIGN.md 2.9 has the constants):
 *     1  the probe was launched                           2  verdict 1 (balanced) on the matrix that was finished
 *     4  the caller's matrix got verdict 2 (constant trailing columns) and the attempt went on on the transpose
 *     8  verdict 3: the unbalanced plan (constant rows)  16  q was taken from the second row asked (row 0 saw no difference)
 *    32  rows 0 and 1 coincide: i2 came from the search over the sampled rows
 *    64  ... and that search found it only on column q  128  column keys negated
 *   256  certificate pass with 16-byte loads            512  64-bit prices (a price left +-2^30)
 *  1024  accepted (always equal to word [8])
 *   Word [12] is set to 0 when td_assign is entered, filled in as the attempt proceeds and kept when the general solver
 *   takes over, so a refusal can be read too.  After a transposed retry bits 2, 8 and 16..512 describe the probe and the
 *   finish on the transpose.  The sharded entry points (td_line_shard_*) do not set it.
 * [13] = finisher_path, which finishers the last td_assign launched for the rows the bidding rounds left free, as a bit set
 *   (FP_* below; DESIGN.md section 2, step 4 has the selection):
 *     1  FP_FOREST          k_forest launched              2  FP_FOREST_NONE    k_forest's turn, but 0 rows were free
 *     4  FP_FOREST_REFUSED  its cooperative launch returned an error (the finishers below took over)
 *     8  FP_PSAP            at least one group of speculative k_sap batches with k_pcommit
 *    16  FP_SAPX            k_sapx launched               32  FP_SAPX_REFUSED   its cooperative launch returned an error
 *    64  FP_SAP8_BATCH      k_sap8's speculative batches 128  FP_SAP8           k_sap8
 *   bits 8..12              CH, the 16-byte chunks per thread of the single-workgroup search that was launched (1 .. 16)
 *  8192  FP_SAP512          the 512-thread k_sap       16384  FP_SAP            the generic (1024-thread) k_sap
 * 32768  FP_NOLDS           that search kept owner[] / pred[] in global memory (npad * 8 bytes > 150 KiB)
 *   bits 16..31             speculative batches launched (k_sap in SPEC mode or k_sap8, each with its k_pcommit)
 *   Word [13] is set to 0 when td_assign is entered and again before the finisher of each cell width's attempt, so it
 *   describes the attempt that delivered the answer (0: the rounds left no row, or the line-metric path answered).
 * [14] = match_path, what the last td_match_batched / td_pool2_batched / td_pool2_batched_v launched, as a bit set (MP_* below;
 *   DESIGN.md 3.5 has the placement rule and the chunk size):
 *     1  MP_LDS        the solver's per-model state (align256(152 n + 64) bytes, n the longest model) lay in LDS
 *     2  MP_WS         ... in slices of the library workspace, one per workgroup (it did not fit the LDS budget)
 *     4  MP_POOL       entered as a pool call (td_pool2_batched / td_pool2_batched_v)
 *     8  MP_GREEDY     the greedy was launched           16  MP_MATCH   k_pool_match (the optimum) was launched
 *    32  MP_PER_MODEL  per-model policy arrays were given (td_pool2_batched_v)
 *   bits 8..23         chunks launched, saturating at 65535 (pool calls: ceil(batch / chunk); td_match_batched: 1)
 *   Bits 1 and 2 are set by td_match_batched always and by a pool call only with MP_MATCH.  Word [14] is set to 0 when one of
 *   the three is entered and filled in before it returns, refused calls included once the launches were made (TD_ERANGE,
 *   TD_EINTERNAL); an argument error or a batch of 0 leaves it 0.  It is defined only right after such a call. */
#define TD_FP_FOREST 1
#define TD_FP_FOREST_NONE 2
#define TD_FP_FOREST_REFUSED 4
#define TD_FP_PSAP 8
#define TD_FP_SAPX 16
#define TD_FP_SAPX_REFUSED 32
#define TD_FP_SAP8_BATCH 64
#define TD_FP_SAP8 128
#define TD_FP_CH_SHIFT 8
#define TD_FP_CH_MASK 0x1f00
#define TD_FP_SAP512 8192
#define TD_FP_SAP 16384
#define TD_FP_NOLDS 32768
#define TD_FP_BATCH_SHIFT 16
#define TD_MP_LDS 1
#define TD_MP_WS 2
#define TD_MP_POOL 4
#define TD_MP_GREEDY 8
#define TD_MP_MATCH 16
#define TD_MP_PER_MODEL 32
#define TD_MP_CHUNK_SHIFT 8
#define TD_MP_CHUNK_MAX 0xffff
TD_API int td_last_stats(int64_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif
