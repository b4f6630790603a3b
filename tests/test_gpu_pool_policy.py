"""Pooling policies on the device: td_pool2_loss, td_pool2_batched_v, td_sim_pooling / td_simb_pooling, td_sim_pools /
td_simb_pools.

1. td_pool2_loss against pool_opt_data's pair_costs + greedy (plan from plan1) on both greedy paths (level lists, narrow
   row scan), on models without a candidate and with exactly one, against td_pool2 and td_pool2_batched;
2. td_pool2_batched_v: every model of a mixed batch equals the scalar call on itself;
3. worlds in lock-step with the specification (simulator.Simulator(pool=, max_loss=)): the plans flow device -> host, are
   checked there against the CPU (the optimum against a certified matching or exhaustive search, never against the pool
   call under test alone), the decisions are the oracle's on both sides;
4. a mixed batch against its worlds alone, the default policy against an untouched handle, the event log's plan order;
5. the C-ABI contract of the four new world entry points."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import abi_buffers as ab
import match_cert
import pool_opt_data as po
import sim_backend
import sim_pool_policy as spp
import sim_worlds as sw

pytestmark = pytest.mark.gpu

TD_EINVAL = -1
LP_LISTS, LP_NARROW, LP_POOL2 = 1, 4, 128
BIG = sw.BIG_COST


# ---- 1. td_pool2_loss ------------------------------------------------------------------------------------------------------
def reference(frm, to, table, max_loss):
    c, plan1 = po.pair_costs(frm, to, table, max_loss)
    return spp.greedy_plans(c, plan1), c


def model(kind, n):
    """(frm, to, table): `line` = 50 stands, |a - b|; `table` = pool_table(), 100 stands, U{1..39}"""
    if kind == "line":
        return po.pool_model(n, 900 + n, 50) + (None,)
    return po.pool_model(n, 700 + n, 100) + (po.pool_table(),)


@pytest.mark.parametrize("max_loss", [1.01, 2.0])
@pytest.mark.parametrize("kind", ["line", "table"])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129])
def test_pool2_loss_equals_the_restatement(td, n, kind, max_loss):
    frm, to, table = model(kind, n)
    want, c = reference(frm, to, table, max_loss)
    got = td.find_pool(frm, to, table, max_loss=max_loss)
    path = td.last_stats()["lcm_path"]
    assert got == want
    assert path & LP_POOL2
    if n >= 64 and (c >= 0).any():      # pool costs span fewer than 256 values here: the level lists
        assert path & LP_LISTS, path
    else:
        assert not path & LP_LISTS, path


def wide_table(S=40, seed=11):
    t = np.random.default_rng(seed).integers(1, 0x1fffffff + 1, (S, S)).astype(np.int32)
    t[0, 1] = 0x1fffffff
    return t


@pytest.mark.parametrize("n", [128, 129])
def test_pool2_loss_on_the_narrow_row_scan_path(td, n):
    table = wide_table()
    frm, to = po.pool_model(n, 300 + n, table.shape[0])
    want, c = reference(frm, to, table, 2.0)
    assert 0 < len(want) and (c >= 0).sum() < n * (n - 1)      # the rule refuses some pairs and admits some
    got = td.find_pool(frm, to, table, max_loss=2.0)
    path = td.last_stats()["lcm_path"]
    assert got == want
    assert path & LP_NARROW and not path & LP_LISTS, path


def test_both_greedy_paths_were_taken(td):
    """the level lists at n = 128 on pool_table(), the narrow row scan at n = 128 on the wide table, under the same rule"""
    frm, to, table = model("table", 128)
    assert td.find_pool(frm, to, table, max_loss=2.0) == reference(frm, to, table, 2.0)[0]
    lists = td.last_stats()["lcm_path"]
    frm, to = po.pool_model(128, 428, 40)
    assert td.find_pool(frm, to, wide_table(), max_loss=2.0) == reference(frm, to, wide_table(), 2.0)[0]
    rows = td.last_stats()["lcm_path"]
    assert lists & LP_LISTS and not lists & LP_NARROW and rows & LP_NARROW and not rows & LP_LISTS


@pytest.mark.parametrize("n", [5, 70, 130])
def test_a_model_without_a_candidate_gives_no_plan(td, n):
    stand = np.arange(n, dtype=np.int32) % 50
    want, c = reference(stand, stand, None, 1.01)
    assert want == [] and not (c >= 0).any()
    assert td.find_pool(stand, stand, None, max_loss=1.01) == []
    assert not td.last_stats()["lcm_path"] & LP_LISTS      # k_lcms_minmax counts 0 cells: the row-scan path, base word INT_MAX
    table = po.pool_table()
    assert td.find_pool(stand, stand, table, max_loss=1.01) == reference(stand, stand, table, 1.01)[0]


@pytest.mark.parametrize("n", [5, 66, 130])
def test_a_model_with_exactly_one_candidate_pair(td, n):
    frm = np.full(n, 40, np.int32)
    to = frm.copy()
    frm[n // 2], to[n // 2] = 0, 10      # A: 0 -> 10
    frm[n - 1], to[n - 1] = 2, 8         # B: 2 -> 8 rides inside A's trip; nobody else travels
    want, c = reference(frm, to, None, 1.01)
    assert (c >= 0).sum() == 1 and want == [(n // 2, n - 1, 0, 10)]
    assert td.find_pool(frm, to, None, max_loss=1.01) == want


@pytest.mark.parametrize("n", [3, 65, 129])
def test_max_loss_zero_is_td_pool2(td, n):
    for kind in ("line", "table"):
        frm, to, table = model(kind, n)
        every = td.find_pool(frm, to, table)
        assert len(every) == n // 2
        assert td.find_pool(frm, to, table, max_loss=0.0) == every
        assert td.find_pool(frm, to, table, max_loss=-1.0) == every


@pytest.mark.parametrize("max_loss", [1.01, 2.0])
def test_pool2_loss_equals_the_batched_greedy_at_129(td, max_loss):
    for kind in ("line", "table"):
        frm, to, table = model(kind, 129)
        a, b, plan, cost, k, _ = td.pool2_batched([frm], [to], table, max_loss, optimal=False)
        batched = [(int(a[0, i]), int(b[0, i]), int(plan[0, i]), int(cost[0, i])) for i in range(int(k[0]))]
        assert td.find_pool(frm, to, table, max_loss=max_loss) == batched


# ---- 2. td_pool2_batched_v -------------------------------------------------------------------------------------------------
V_SIZES = [0, 1, 2, 3, 31, 64, 65, 100, 129]
V_OPT = [1, 0, 1, 0, 1, 0, 1, 0, 1]
V_LOSS = [1.01, None, None, 2.0, 1.01, 1.01, None, 2.0, 2.0]


def v_models():
    ms = [po.pool_model(m, 500 + m, 100) for m in V_SIZES]
    return [f for f, _ in ms], [t for _, t in ms]


def pools_of(out, b=0):
    a, c, plan, cost, k, total = out
    return [(int(a[b, i]), int(c[b, i]), int(plan[b, i]), int(cost[b, i])) for i in range(int(k[b]))], int(total[b])


@pytest.mark.parametrize("table", [False, True])
def test_batched_v_every_model_equals_the_scalar_call_on_itself(td, table):
    froms, tos = v_models()
    tab = po.pool_table() if table else None
    mixed = td.pool2_batched(froms, tos, tab, max_loss=V_LOSS, optimal=V_OPT)
    kinds = set()
    for b in range(len(V_SIZES)):
        alone = td.pool2_batched([froms[b]], [tos[b]], tab, V_LOSS[b], optimal=bool(V_OPT[b]))
        assert pools_of(mixed, b) == pools_of(alone), b
        kinds.add((V_OPT[b], len(pools_of(alone)[0]) > 0))
    assert kinds >= {(0, True), (1, True)}      # both kinds produced pools in the mixed call
    # one kind everywhere, given as arrays: the uniform calls
    for opt in (0, 1):
        got = td.pool2_batched(froms, tos, tab, max_loss=[1.01] * 9, optimal=[opt] * 9)
        want = td.pool2_batched(froms, tos, tab, 1.01, optimal=bool(opt))
        for b in range(9):
            assert pools_of(got, b) == pools_of(want, b), (opt, b)


def raw_v(td, froms, tos, max_loss, optimal, fill=None):
    """td_pool2_batched_v on the raw ABI (max_loss / optimal: arrays or None = NULL) -> (rc, outputs)"""
    from taxidispatcher_amd import _ffi
    lib = _ffi.lib()
    off = np.concatenate([[0], np.cumsum([len(f) for f in froms])]).astype(np.int32)
    fv, tv = np.concatenate(froms).astype(np.int32), np.concatenate(tos).astype(np.int32)
    batch, n = len(froms), max(len(f) for f in froms)
    outs = [np.zeros((batch, n // 2), np.int32) for _ in range(4)] + [np.zeros(batch, np.int32), np.zeros(batch, np.int64)]
    if fill is not None:
        for o in outs:
            o[...] = fill
    rc = lib.td_pool2_batched_v(batch, n, off.ctypes.data, fv.ctypes.data, tv.ctypes.data, None, 0,
                                None if max_loss is None else max_loss.ctypes.data, None if optimal is None else optimal.ctypes.data,
                                *[o.ctypes.data for o in outs])
    return rc, outs


def test_batched_v_null_arrays_are_the_scalar_defaults(td):
    froms, tos = v_models()
    rc, outs = raw_v(td, froms, tos, None, None)
    assert rc == 0
    want = td.pool2_batched(froms, tos, None, None, optimal=False)
    for b in range(9):
        assert pools_of(outs, b) == pools_of(want, b), b
    # one array given, the other NULL
    rc, outs = raw_v(td, froms, tos, np.full(9, 1.01), None)
    want = td.pool2_batched(froms, tos, None, 1.01, optimal=False)
    assert rc == 0 and all(pools_of(outs, b) == pools_of(want, b) for b in range(9))
    rc, outs = raw_v(td, froms, tos, None, np.ones(9, np.int32))
    want = td.pool2_batched(froms, tos, None, None, optimal=True)
    assert rc == 0 and all(pools_of(outs, b) == pools_of(want, b) for b in range(9))


def test_batched_v_refuses_an_optimal_flag_of_two(td):
    froms, tos = v_models()
    opt = np.array(V_OPT, np.int32)
    opt[5] = 2
    rc, outs = raw_v(td, froms, tos, None, opt, fill=-77)
    assert rc == TD_EINVAL
    assert all((o == -77).all() for o in outs)


# ---- 3. worlds in lock-step with the specification ---------------------------------------------------------------------------
class FedBackend(sim_backend.OracleTickBackend):
    """find_pool hands back the plans read from the device (and remembers the model it was asked about); tick is the
    oracle's and remembers its arguments and result"""

    def __init__(self):
        self.plans, self.asked, self.last = [], None, None

    def find_pool(self, frm, to, max_loss=None, optimal=False):
        self.asked = (np.asarray(frm), np.asarray(to), max_loss, optimal)
        return list(self.plans)

    def tick(self, cab_to, dem_from):
        res = super().tick(cab_to, dem_from)
        self.last = (list(cab_to), list(dem_from), res)
        return res


def certified_weight(td, frm, to, max_loss):
    """the maximum matching weight of the model's lex_weights: exhaustive search for small models, else td.match_batched's
    matching with its dual certificate re-verified by match_cert (numpy)"""
    c, _ = po.pair_costs(frm, to, None, max_loss)
    if len(frm) <= 12:
        return spp.exhaustive_weight(c)
    _, W = po.lex_weights(c)
    W = W.astype(np.int32)
    mate, total, bound, (y, par, z) = td.match_batched([W], want_dual=True)
    match_cert.check(W, mate[0], total[0], bound[0], y[0], par[0], z[0])
    return int(total[0])


def world_kw(w):
    return dict(n_cabs=w["cabs"], n_stands=w["stands"], drop_time=w["drop_time"], max_non_lcm=w["max_non_lcm"], big_cost=BIG)


def assert_same_state(got, host, where):
    for k, v in sw.state_of(host).items():
        assert np.array_equal(got[k], v), (where, k, np.nonzero(got[k] != v)[0][:8].tolist())


@pytest.mark.parametrize("pool,max_loss", spp.POLICIES)
@pytest.mark.parametrize("name", ["small", "mid"])
def test_a_world_in_lock_step_with_the_specification(td, name, pool, max_loss, monkeypatch):
    from taxidispatcher_amd import simulator
    w = sw.WORLDS[name]
    sw.patch_constants(monkeypatch, w)
    rows = sw.gen_demand(**w)
    be = FedBackend()
    host = simulator.Simulator(rows, be, n_cabs=w["cabs"], pool=pool, max_loss=max_loss)
    dev = td.DeviceSimulator(rows, pool=pool, max_loss=max_loss, **world_kw(w))
    n_plans = n_checked = 0
    for t in range(w["ticks"]):
        info = dev.begin(t)                                                    # 1
        be.plans = dev.pools()                                                 # 2
        be.asked = be.last = None
        want = host.tick(t)                                                    # 4 (3 inside: the host asks for the plans of its own model)
        if pool == "none" or info[2] == 0 or info[1] < 2:
            assert be.plans == [] and be.asked is None, t
        else:
            frm, to, ml, optimal = be.asked
            assert len(frm) == info[1] and ml == max_loss and optimal == (pool == "optimal"), t
            cert = certified_weight(td, frm, to, ml) if optimal else None
            spp.check_plans(frm, to, ml, optimal, be.plans, cert)              # 3
            n_plans += len(be.plans)
            n_checked += 1
        if not info[0]:
            line = None
        elif info[2] == 0:
            assert be.last is None, t
            line = dev.format_line(t, [1, info[1], 0, 0, 0, 0, 0, 0, dev.apply()])
        else:
            cab_to, dem_from, res = be.last
            got_cab, got_dem = dev.model()                                     # 5
            assert got_cab.tolist() == cab_to and got_dem.tolist() == dem_from and info[3] == len(dem_from), t
            opt = dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])      # 6
            lcm = max(info[2], info[3]) > w["max_non_lcm"]
            line = dev.format_line(t, [1, info[1], info[2], lcm, len(res["lcm_rows"]), lcm and res["solved"], len(res["kept_dems"]),
                                       len(res["kept_cabs"]), opt])
        assert line == want, t                                                 # 7
        assert dev.m == host.m, t
        assert_same_state(dev.state(), host, (name, pool, max_loss, t))
    if pool == "none":
        assert host.m["total_second_passengers"] == 0 and host.m["max_POOL_MEM_size"] == 0
    else:
        assert n_checked > 10 and n_plans > 0 and host.m["total_second_passengers"] > 0
    dev.close()


# ---- 4. a batch --------------------------------------------------------------------------------------------------------------
SEEDS = (2, 12)


def batch_worlds():
    """8 worlds on `small`'s city: two demand seeds x the four policies"""
    w = sw.WORLDS["small"]
    rows, pools, losses = [], [], []
    for seed in SEEDS:
        for pool, ml in spp.POLICIES:
            rows.append(sw.gen_demand(**dict(w, seed=seed)))
            pools.append(pool)
            losses.append(ml)
    return w, rows, pools, losses


def batch_kw(w):
    return dict(n_stands=w["stands"], drop_time=w["drop_time"], max_non_lcm=w["max_non_lcm"], big_cost=BIG)


def test_a_mixed_batch_equals_its_worlds_alone(td):
    w, rows, pools, losses = batch_worlds()
    B = len(rows)
    dev = td.DeviceSimulatorBatch(rows, [w["cabs"]] * B, pool=pools, max_loss=losses, **batch_kw(w))
    alone = [td.DeviceSimulatorBatch([rows[b]], [w["cabs"]], pool=pools[b], max_loss=losses[b], **batch_kw(w)) for b in range(B)]
    for t in range(w["ticks"]):
        lines = dev.tick(t)
        for b in range(B):
            one = alone[b].tick(t)
            assert (None if lines is None else lines[b]) == (None if one is None else one[0]), (t, b)
            assert dev.pools(b) == alone[b].pools(0), (t, b)
    m = dev.m
    for b in range(B):
        assert m[b] == alone[b].m[0], b
        got, want = dev.state(b), alone[b].state(0)
        for k in want:
            assert np.array_equal(got[k], want[k]), (b, k)
        alone[b].close()
    seconds = [x["total_second_passengers"] for x in m]
    for s in range(len(SEEDS)):
        none, greedy, opt_every, opt_ruled = seconds[4 * s:4 * s + 4]
        assert none == 0 and greedy > 0 and opt_every > 0 and opt_ruled > 0
        assert m[4 * s]["max_POOL_MEM_size"] == 0 and m[4 * s]["max_POOL_size"] == 0
        assert all(m[4 * s + q]["max_POOL_MEM_size"] > 0 and m[4 * s + q]["max_POOL_size"] > 0 for q in (1, 2, 3))
    dev.close()


def test_the_default_policy_world_equals_an_untouched_handle(td):
    w = sw.WORLDS["small"]
    rows = sw.gen_demand(**w)
    set_b = td.DeviceSimulatorBatch([rows, rows], [w["cabs"]] * 2, pool=["greedy", "optimal"], max_loss=[None, 1.01], **batch_kw(w))
    plain_b = td.DeviceSimulatorBatch([rows], [w["cabs"]], **batch_kw(w))
    set_1 = td.DeviceSimulator(rows, pool="greedy", max_loss=0.0, **world_kw(w))      # td_sim_pooling(TD_POOL_GREEDY, 0.0) is called
    plain_1 = td.DeviceSimulator(rows, **world_kw(w))
    for t in range(w["ticks"]):
        a, b = set_b.tick(t), plain_b.tick(t)
        assert (None if a is None else a[0]) == (None if b is None else b[0]), t
        assert set_b.pools(0) == plain_b.pools(0), t
        assert set_1.tick(t) == plain_1.tick(t), t
        assert set_1.pools() == plain_1.pools(), t
    assert set_b.m[0] == plain_b.m[0] and set_1.m == plain_1.m
    for k, v in plain_b.state(0).items():
        assert np.array_equal(set_b.state(0)[k], v), k
    for k, v in plain_1.state().items():
        assert np.array_equal(set_1.state()[k], v), k
    for d in (set_b, plain_b, set_1, plain_1):
        d.close()


def test_the_event_log_lists_an_optimal_worlds_pairs_in_pools_order(td, monkeypatch):
    w = sw.WORLDS["small"]
    sw.patch_constants(monkeypatch, w)
    rows = sw.gen_demand(**w)
    dev = td.DeviceSimulatorBatch([rows, rows], [w["cabs"]] * 2, pool=["optimal", "none"], max_loss=[1.01, None], events=True, **batch_kw(w))
    oracle = sim_backend.OracleTickBackend()
    pairs_seen = 0
    for t in range(w["ticks"]):
        info = dev.begin(t)
        ev = dev.events()                # begin's records of every world
        assert (ev[:, 0] == t).all()
        for b in (0, 1):
            e = ev[ev[:, 1] == b]
            ids = e[e[:, 2] == 5][:, 4].tolist()
            heads, pairs = e[e[:, 2] == 6], e[e[:, 2] == 7]
            plans = dev.pools(b)
            if b == 1 or not (info[b][0] and info[b][2]):
                assert len(heads) == 0 and len(pairs) == 0 and plans == [], (t, b)
                continue
            assert len(ids) == info[b][1] and len(heads) == 1 and heads[0][6] == len(plans), (t, b)
            assert [(int(p[4]), int(p[6])) for p in pairs] == [(ids[a], ids[c]) for a, c, _, _ in plans], (t, b)
            assert [p[3] for p in plans] == sorted(p[3] for p in plans), (t, b)
            pairs_seen += len(plans)
        if not info[:, 0].any():
            continue
        cab_off, cab_to, dem_off, dem_from = dev.model()
        dec = []
        for b in (0, 1):
            if not info[b][0] or not info[b][2]:
                dec.append(None)
                continue
            r = oracle.tick(cab_to[cab_off[b]:cab_off[b + 1]], dem_from[dem_off[b]:dem_off[b + 1]])
            dec.append((r["lcm_rows"], r["lcm_cols"], r["solved"], r["row_to_col"]))
        dev.apply(dec)
        rest = dev.events()
        assert not np.isin(rest[:, 2], (6, 7)).any(), t
    assert pairs_seen > 20 and dev.events_lost == 0
    dev.close()


# ---- 5. the contract -----------------------------------------------------------------------------------------------------------
def lib_of(td):
    from taxidispatcher_amd import _ffi
    return _ffi.lib()


def begun_with_plans(td, batch):
    """a world (or a batch of one) on `small` under greedy 1.01, begun at the first tick with at least two plans, waiting for
    its apply -> (handle object, tick, plans)"""
    w = sw.WORLDS["small"]
    rows = sw.gen_demand(**w)
    if batch:
        dev = td.DeviceSimulatorBatch([rows], [w["cabs"]], pool="greedy", max_loss=1.01, **batch_kw(w))
    else:
        dev = td.DeviceSimulator(rows, pool="greedy", max_loss=1.01, **world_kw(w))
    for t in range(w["ticks"]):
        dev.begin(t)
        plans = dev.pools(0) if batch else dev.pools()
        if len(plans) >= 2:
            return dev, t, plans
        info = np.asarray(dev._info).reshape(-1, 4)[0]
        if info[0]:
            if batch:
                dev.apply([None if not info[2] else ((), (), False, ())])
            else:
                dev.apply((), (), False, ())
    raise AssertionError("no tick with two plans")


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("kind", ["host", "device"])
def test_pools_outputs_in_host_and_device_memory(td, batch, kind):
    lib = lib_of(td)
    dev, t, plans = begun_with_plans(td, batch)
    k = len(plans)
    bufs = [ab.guarded(k, np.int32, kind, misalign=q) for q in range(4)]
    n = ctypes.c_int32(-1)
    args = [dev._h] + ([0] if batch else []) + [k] + [ab.ptr(v) for v, _ in bufs] + [ctypes.byref(n)]
    assert (lib.td_simb_pools if batch else lib.td_sim_pools)(*args) == 0
    assert n.value == k
    got = [ab.host(v).tolist() for v, _ in bufs]
    assert list(zip(*got)) == plans
    for _, check in bufs:
        check()
    dev.close()


@pytest.mark.parametrize("batch", [False, True])
def test_pools_with_max_pools_too_small(td, batch):
    lib = lib_of(td)
    dev, t, plans = begun_with_plans(td, batch)
    k = len(plans)
    bufs = [ab.guarded(k, np.int32, "host") for _ in range(4)]
    n = ctypes.c_int32(-1)
    fn = lib.td_simb_pools if batch else lib.td_sim_pools
    head = [dev._h] + ([0] if batch else [])
    assert fn(*head, k - 1, *[ab.ptr(v) for v, _ in bufs], ctypes.byref(n)) == TD_EINVAL
    assert n.value == k
    assert all((v == ab.pattern_value(np.int32)).all() for v, _ in bufs)
    assert fn(*head, -1, *[ab.ptr(v) for v, _ in bufs], ctypes.byref(n)) == TD_EINVAL
    if batch:
        assert fn(dev._h, 1, k, *[ab.ptr(v) for v, _ in bufs], ctypes.byref(n)) == TD_EINVAL      # world outside the batch
    assert fn(*head, k, *[ab.ptr(v) for v, _ in bufs], ctypes.byref(n)) == 0 and n.value == k
    dev.close()


@pytest.mark.parametrize("batch", [False, True])
def test_pooling_is_refused_while_a_tick_waits_and_for_bad_arguments(td, batch):
    lib = lib_of(td)
    dev, t, plans = begun_with_plans(td, batch)
    mode, loss = np.array([2], np.int32), np.array([1.5], np.float64)

    def pooling(m, x):
        if batch:
            mode[0], loss[0] = m, x
            return lib.td_simb_pooling(dev._h, mode.ctypes.data, loss.ctypes.data)
        return lib.td_sim_pooling(dev._h, int(m), float(x))
    assert pooling(2, 1.5) == TD_EINVAL                 # the tick waits for its apply
    assert b"waits" in lib.td_last_error()
    if batch:
        dev.apply([((), (), False, ())])
    else:
        dev.apply((), (), False, ())
    assert pooling(3, 1.5) == TD_EINVAL and pooling(-1, 1.5) == TD_EINVAL and pooling(1, math.nan) == TD_EINVAL
    # refused calls changed nothing: the next tick still pools under greedy 1.01
    dev.begin(t + 1)
    got = dev.pools(0) if batch else dev.pools()
    w = sw.WORLDS["small"]
    twin = td.DeviceSimulator(sw.gen_demand(**w), pool="greedy", max_loss=1.01, **world_kw(w))
    for u in range(t + 2):
        info = twin.begin(u)
        want = twin.pools()
        if info[0]:
            twin.apply((), (), False, ())
    assert got == want
    twin.close()
    dev.close()


def test_workspace_bytes_return_after_destroy(td):
    lib = lib_of(td)

    def ws():
        v = ctypes.c_int64(-1)
        assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
        return v.value
    w, rows, pools, losses = batch_worlds()

    def make():
        return (td.DeviceSimulatorBatch(rows, [w["cabs"]] * len(rows), pool=pools, max_loss=losses, **batch_kw(w)),
                td.DeviceSimulator(rows[3], pool="optimal", max_loss=1.01, **world_kw(w)))
    for d in make():      # the library's own grow-only buffers reach their size for these worlds
        d.run(10)
        d.close()
    before = ws()
    plain = td.DeviceSimulatorBatch(rows, [w["cabs"]] * len(rows), **batch_kw(w))
    plain_held = ws() - before
    plain.close()
    assert ws() == before
    devs = make()
    held = ws() - before
    for d in devs:
        d.run(10)
    assert ws() - before == held      # td_*_pooling allocated nothing, and nothing per tick
    devs[1].close()
    assert ws() - before == plain_held      # a batch under policies holds what an untouched batch holds
    devs[0].close()
    assert ws() == before


@pytest.mark.parametrize("batch", [False, True])
def test_an_optimal_world_past_2048_requests_is_refused_by_begin(td, batch):
    """a refusal, not a fault: one cab at stand 0 and 2049 requests 0 -> 1 in tick 0; the optimum of a tick is ONE model of
    the batched finder, which holds 2048 customers"""
    n = 2049
    rows = np.stack([np.arange(n), np.zeros(n, np.int64), np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1)
    kw = dict(n_stands=2, drop_time=3, max_non_lcm=4, big_cost=BIG)
    from taxidispatcher_amd import TdError
    if batch:
        dev = td.DeviceSimulatorBatch([rows[:5], rows], [1, 1], pool=["optimal", "optimal"], max_loss=[None, 1.01], **kw)
    else:
        dev = td.DeviceSimulator(rows, n_cabs=1, pool="optimal", **kw)
    with pytest.raises(TdError) as e:
        dev.begin(0)
    assert "2049" in str(e.value) and ("world 1" if batch else "world 0") in str(e.value) and "error -1" in str(e.value)
    with pytest.raises(TdError):      # the handle is as a failing td_pool2 inside begin leaves it: the tick counts as begun
        dev.begin(1)
    dev.close()
    # the same tick under the greedy rule is served (the device-wide finder has no such limit)
    if batch:
        ok = td.DeviceSimulatorBatch([rows[:5], rows], [1, 1], pool=["optimal", "greedy"], max_loss=[None, 1.01], **kw)
        info = ok.begin(0)
        assert info[1].tolist()[:3] == [1, n, 1] and len(ok.pools(0)) == 2
        assert ok.pools(1) == [(2 * i, 2 * i + 1, 0, 1) for i in range(n // 2)]      # equal customers: every pair passes, cost 1, A-major order
    else:
        ok = td.DeviceSimulator(rows, n_cabs=1, pool="greedy", max_loss=1.01, **kw)
        info = ok.begin(0)
        assert info[:3] == (1, n, 1)
        assert ok.pools() == [(2 * i, 2 * i + 1, 0, 1) for i in range(n // 2)]
    ok.close()
