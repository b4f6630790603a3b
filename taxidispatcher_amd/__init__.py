"""taxidispatcher_amd — MI355X (gfx950) cab<->request assignment path.

cost-matrix build -> LCM greedy pre-reduce -> optimal N x N assignment as hand-written HIP
kernels behind a C ABI (include/taxidispatcher_amd.h).  See DESIGN.md / INTEGRATION.md.
"""
from . import _ffi
from ._ffi import TdError, init, shutdown
from .dispatch import (BIG_COST, DISPATCH_MODES, LCM, Solver, LCM_batched, LCM_heuristic, LCM_simulator, assign, assign_batched, build_assign, build_assign_batched, calculate_cost, calculate_cost_by_id,
                       combined, cost_build, count_sum, dispatch_batched, expand_x, filter_out, find_pool, find_pool_fanout, find_pool_n, find_pool_n_banded, find_pool_optimal, finisher_path, heuristic_gap, last_stats,
                       match_batched, match_path, merge_pools, pack_pool_n, pack_ragged, pool2_batched, pool_gap, pool_n_banded_batched, pool_n_batched, procedure_solve, set_line_metric, solve, solve_cost, solve_split, split_batched, split_gap,
                       tick, tick_batched)
from .simulator import DeviceSimulator, DeviceSimulatorBatch, format_events

__all__ = ["TdError", "init", "shutdown", "BIG_COST", "DISPATCH_MODES", "DeviceSimulator", "DeviceSimulatorBatch", "format_events", "LCM", "Solver", "LCM_batched", "LCM_heuristic", "LCM_simulator", "assign",
           "assign_batched", "build_assign", "build_assign_batched",
           "calculate_cost", "calculate_cost_by_id", "combined", "cost_build", "count_sum", "dispatch_batched", "expand_x", "filter_out", "find_pool",
           "find_pool_fanout", "find_pool_n", "find_pool_n_banded", "find_pool_optimal", "heuristic_gap", "match_batched", "merge_pools", "pool2_batched", "pool_gap", "pool_n_banded_batched", "pool_n_batched", "last_stats", "finisher_path", "match_path", "pack_pool_n", "pack_ragged", "procedure_solve", "set_line_metric", "solve",
           "solve_cost", "solve_split", "split_batched", "split_gap", "tick", "tick_batched"]
