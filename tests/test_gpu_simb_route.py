"""Routed worlds in a batch: td_simb_route / td_simb_route_state / td_simb_route_metrics, DeviceSimulatorBatch(route=...).

Every world of a batch equals a DeviceSimulator(route=...) handle on the same inputs and policy, tick by tick (the comparator
of tests/test_gpu_simb_pool_n.py; helpers in simb_route_worlds.py).

1. the hand-made worlds of sim_route_worlds in batches: six worlds of one city in one batch, in both orders; the LCM world
   beside a copy of itself with routes off; the world that leaves the line and the one on a table, each beside an empty world;
2. family A under mixed policies, some record worlds routed, one not, a pair world, through td_simb_step and through begin /
   model / apply;
3. on -> 0 in one world with cabs mid-route, the other world keeps its routes;
4. a routed cab in the second workgroup of its fleet, the fleet off a multiple of 1024 in the concatenated table;
5. a banded batch;
6. every refusal, and the workspace bytes;
7. td_simb_route_state's destinations."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_worlds as sbw
import sim_route_worlds as R
import simb_route_worlds as B

pytestmark = pytest.mark.gpu

TD_EINVAL = B.TD_EINVAL
CITY = sbw.CITY_A
lib_of, err, i32 = B.lib_of, B.err, B.i32


def hand_world(name, route=True):
    w = R.HAND[name]
    return B.world(w["rows"], w["cabs"], w["pool_n"], w["wait"], w["loss"], route=route)


def hand_batch(td, names, routes, ticks, dist=None):
    """the hand-made worlds `names` (None: an empty world of three cabs) as one batch through td_simb_step, each against its handle
    after every tick, and a routed one against the ticks written out by hand"""
    city = R.HAND[next(n for n in names if n)]
    worlds = [hand_world(n, r) if n else B.world(B.EMPTY_ROWS, 3) for n, r in zip(names, routes)]
    dev = B.batch_of(td, worlds, city, dist=dist)
    alone = [B.handle_of(td, w, city, dist=dist) for w in worlds]
    for t in range(ticks):
        lines = B.batch_tick(td, dev, city, t, "step")
        m, rm = dev.m, dev.route_metrics()
        for b, (name, one) in enumerate(zip(names, alone)):
            want, _ = B.handle_tick(td, one, city, t, dist)
            assert lines[b] == want, (t, b)
            B.assert_world_is_handle(dev, b, one, (names, t), m, rm)
            if not routes[b]:
                B.assert_no_routes(dev, b, (names, t))
                continue
            w, st, rs = R.HAND[name], dev.state(b), dev.route_state(b)
            for i, (tp, tdrop) in enumerate(zip(w["d_pick"], w["d_drop"])):
                assert t < tp or st["d_pick"][i] == tp, (name, t, i)
                assert rs["d_drop"][i] == (tdrop if t >= tdrop else -1), (name, t, i)
            c = w["cab"]
            cab = tuple(int(st[k][c]) for k in ("c_from", "c_to", "c_clnt", "c_onboard", "c_start"))
            if t >= w["free_t"]:
                assert cab == (w["free_at"], w["free_at"], -1, 0, -1) and rs["c_pos"][c] == 2 * len(w["d_pick"]), (name, t, cab)
            else:
                assert cab[2] != -1, (name, t, cab)      # busy from the dispatch in tick 0 until the hand-written free tick
            assert rm[b]["drop_numb"] == sum(tdrop <= t for tdrop in w["d_drop"]) and rm[b]["max_over_loss"] <= 0, (name, t, rm[b])
    out = [(dev.state(b), dev.route_state(b)) for b in range(dev.batch)]
    for one in alone:
        one.close()
    dev.close()
    return out


# ---- 0. the surface ---------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_null_arguments_refused(td):
    lib = lib_of()
    out = np.zeros(4, np.int64)
    assert lib.td_simb_route(None, i32(1).ctypes.data) == TD_EINVAL and "null handle" in err()
    assert lib.td_simb_route_state(None, 0, None, None, None) == TD_EINVAL and "null handle" in err()
    assert lib.td_simb_route_metrics(None, out.ctypes.data) == TD_EINVAL


# ---- 1. the hand-made worlds in batches ---------------------------------------------------------------------------------------------
SIX = ("standing", "heading", "same_from", "drop_at_next", "last_two", "four")


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_six_hand_made_worlds_in_one_batch(td, order):
    """one city, a pool_n, wait and loss per world; in both orders a world with index > 0 uses record 0 of its own slab and
    position 0 of its own demand list (every world pools its requests 0 and 1 into its record 0)"""
    names = SIX if order == "forward" else SIX[::-1]
    assert len({tuple(R.HAND[n][k] for k in ("stands", "drop_time", "max_non_lcm")) for n in names}) == 1
    assert len({(R.HAND[n]["pool_n"], R.HAND[n]["wait"]) for n in names}) > 2
    hand_batch(td, names, [True] * 6, max(R.HAND[n]["free_t"] for n in names) + 2)


def test_the_lcm_world_beside_itself_with_routes_off(td):
    """the off copy shows the unrouted outcome: the cab forgets the pool at the pick-up and the second member is never picked up"""
    w = R.HAND["lcm_heading"]
    out = hand_batch(td, ("lcm_heading", "lcm_heading"), [True, False], w["free_t"] + 2)
    (on_st, on_rs), (off_st, off_rs) = out
    assert on_st["d_pick"].tolist() == w["d_pick"] and on_rs["d_drop"].tolist() == w["d_drop"]
    assert off_st["d_pick"][1] == -1 and off_st["d_cab"][1] == w["cab"] and off_st["d_pick"][0] == w["d_pick"][0]


@pytest.mark.parametrize("name", ["off_line", "ring6"])
def test_a_hand_made_world_beside_an_empty_world(td, name):
    w = R.HAND[name]
    out = hand_batch(td, (None, name), [False, True], w["free_t"] + 2, dist=w.get("dist"))
    st, rs = out[1]
    assert st["d_pick"].tolist() == w["d_pick"] and rs["d_drop"].tolist() == w["d_drop"]


# ---- 2. family A, mixed ---------------------------------------------------------------------------------------------------------------
# world order: A1, A7, A40, A90, Aempty.  An entry: (pool, max_loss, pool_n, wait, loss, route)
P42, P33 = ("greedy", None, (4, 2), 1, 50), ("greedy", None, (3, 3), 1, 50)
MIXES = (
    # a record world with routes off, (4, 2) and (3, 3) routed under different losses, a pair world, the empty world routed
    (("greedy", None, (2, 2), 2, 100, False), P42 + (True,), ("greedy", None, (3, 3), 1, 40, True), ("greedy", 1.5, None, 0, 0, False),
     ("greedy", None, (2, 2), 0, 0, True)),
    # a pair world that does not pool, the two policies the other way round, the large fleet routed
    (("none", None, None, 0, 0, False), P33 + (True,), P42 + (True,), ("greedy", None, (2, 2), 2, 100, True), ("greedy", None, None, 0, 0, False)),
)


@pytest.mark.parametrize("way", ["step", "split"])
@pytest.mark.parametrize("which", [0, 1])
def test_a_mixed_batch_equals_a_handle_per_world(td, which, way):
    city, runs = sbw.family("A")
    worlds = [B.world(run["rows"], run["world"]["cabs"], p[2], p[3], p[4], p[5], p[0], p[1]) for (_, run), p in zip(runs, MIXES[which])]
    routed = [w["route"] for w in worlds]
    losses = {w["loss"] for w in worlds if w["route"] and len(w["rows"])}
    assert len(losses) > 1 and any(w["pn"] and not w["route"] for w in worlds) == (which == 0)
    dev, plain = B.batch_of(td, worlds, city), B.batch_of(td, worlds, city, route=False)
    assert dev.route == routed and plain.route == [False] * 5
    alone = [B.handle_of(td, w, city) for w in worlds]
    given = {True: 0, False: 0}      # routed dispatches seen in ticks where the world's LCM ran / did not
    for t in range(city["ticks"]):
        lines, unrouted = B.batch_tick(td, dev, city, t, way), B.batch_tick(td, plain, city, t, way)
        m, rm, pm = dev.m, dev.route_metrics(), plain.m
        for b, one in enumerate(alone):
            before = one.route_state()["c_stops"] if routed[b] else None
            want, lcm = B.handle_tick(td, one, city, t)
            assert lines[b] == want, (t, b)
            B.assert_world_is_handle(dev, b, one, (which, way, t), m, rm)
            if routed[b]:
                given[lcm] += int((one.route_state()["c_stops"] != before).any(axis=1).sum())
            else:      # a world without routes: untouched by its neighbours' routes, and equal to the batch without any
                B.assert_no_routes(dev, b, (which, way, t))
                assert unrouted[b] == lines[b] and pm[b] == m[b], (t, b)
                sbw.assert_same_state(dev, b, plain.state(b), ("plain", t))
        assert lines[-1] is None, t      # the world without requests
    # what keeps the comparison from passing vacuously, on the handles
    for b, one in enumerate(alone):
        if routed[b]:
            rmo = one.route_metrics()
            assert rmo["max_over_loss"] <= 0 and (rmo["drop_numb"] > 0) == (len(worlds[b]["rows"]) > 0), (b, rmo)
    assert given[True] > 0 and given[False] > 0, given
    for one in alone:
        one.close()
    dev.close(), plain.close()


# ---- 3. on -> 0 in one world ------------------------------------------------------------------------------------------------------------
def test_off_in_one_world_lets_its_cabs_finish_and_leaves_the_other_alone(td):
    city, runs = sbw.family("A")
    by = dict(runs)
    worlds = [B.world(by["A40"]["rows"], 40, (4, 2), 1, 50, True), B.world(by["A7"]["rows"], 7, (3, 3), 1, 40, True)]
    dev = B.batch_of(td, worlds, city)
    alone = [B.handle_of(td, w, city) for w in worlds]
    at_switch, mid, drops = None, 0, []
    for t in range(24):
        if t == 8:
            rs = dev.route_state(0)
            mid = int(B.has_stops(rs).sum())      # from c_pos and c_stops: cabs of world 0 with stops left
            at_switch = rs["c_stops"].copy()
            dev.set_route([False, True])
            alone[0].set_route(False)
            alone[0].had_routes = True      # the handle keeps its route state: compared on
        lines = B.batch_tick(td, dev, city, t, "step")
        for b, one in enumerate(alone):
            want, _ = B.handle_tick(td, one, city, t)
            assert lines[b] == want, (t, b)
            B.assert_world_is_handle(dev, b, one, t)
        drops.append([x["drop_numb"] for x in dev.route_metrics()])
    assert mid > 0
    rs = dev.route_state(0)
    assert np.array_equal(rs["c_stops"], at_switch)      # no list was handed out in world 0 after the switch
    assert not B.has_stops(rs).any() and drops[23][0] > drops[7][0]      # and its cabs finished theirs
    assert drops[23][1] > drops[7][1] and dev.route == [False, True]      # the other world went on
    for one in alone:
        one.close()
    dev.close()


# ---- 4. a fleet's second workgroup ------------------------------------------------------------------------------------------------------
def test_a_routed_cab_in_the_second_workgroup_of_its_fleet(td):
    """CITY_W: 50 stands, 1030 cabs, cab c starts at stand c % 50: the 21 cabs at stand 24 are rows 24, 74, .., 1024.  50 requests
    24 -> 30 make 25 pools of two; every cheapest assignment uses all 21 cabs that stand at 24, so row 1024 drives a route.  A
    world of five cabs before it puts the fleet at row 5 of the concatenated table."""
    city = sbw.CITY_W
    rows = np.asarray([(i, 24, 30, 0, 0) for i in range(50)], np.int64)
    small = R.req((1, 3), (2, 3))
    worlds = [B.world(small, 5, 2, 1, 100, True), B.world(rows, 1030, 2, 0, 0, True)]
    dev = B.batch_of(td, worlds, city)
    alone = [B.handle_of(td, w, city) for w in worlds]
    for t in range(8):
        lines = B.batch_tick(td, dev, city, t, "step")
        for b, one in enumerate(alone):
            want, _ = B.handle_tick(td, one, city, t)
            assert lines[b] == want, (t, b)
            B.assert_world_is_handle(dev, b, one, t)
        if t == 0:
            got = np.nonzero((dev.route_state(1)["c_stops"] >= 0).any(axis=1))[0]
            assert len(got) == 25 and got.max() >= 1024, got      # the cab index read back
    rm = dev.route_metrics()
    assert rm[1]["drop_numb"] == 50 and rm[1]["ride_time"] == rm[1]["solo_time"] == 300 and rm[0]["drop_numb"] == 2
    for one in alone:
        one.close()
    dev.close()


# ---- 5. a banded batch ----------------------------------------------------------------------------------------------------------------
def test_a_banded_batch(td):
    """the smallest plan buffer a batch takes (24 * 512) against handles under the smallest theirs take (24 * 2047)"""
    city, runs = sbw.family("A")
    by = dict(runs)
    worlds = [B.world(by["A7"]["rows"], 7, (4, 2), 1, 50, True), B.world(by["A40"]["rows"], 40, (4, 2), 1, 40, True)]
    dev = B.batch_of(td, worlds, city, pool_buffer=24 * 512)
    alone = [B.handle_of(td, w, city, pool_buffer=24 * 2047) for w in worlds]
    for t in range(16):
        lines = B.batch_tick(td, dev, city, t, "step")
        for b, one in enumerate(alone):
            want, _ = B.handle_tick(td, one, city, t)
            assert lines[b] == want, (t, b)
            B.assert_world_is_handle(dev, b, one, t)
    assert all(one.route_metrics()["drop_numb"] > 0 for one in alone)
    for one in alone:
        one.close()
    dev.close()


# ---- 6. refusals and the workspace ------------------------------------------------------------------------------------------------------
def a_batch(td, pn, **kw):
    city, runs = sbw.family("A")
    by = dict(runs)
    return td.DeviceSimulatorBatch([by["A7"]["rows"], by["A40"]["rows"]], [7, 40], pool_n=pn, pool_wait=1, pool_loss=50, **B.kw_of(city), **kw)


def test_refusals(td):
    lib = lib_of()
    route = lambda h, *on: lib.td_simb_route(h, i32(*on).ctypes.data)
    out, buf = np.zeros(8, np.int64), np.zeros(8 * 40, np.int32)
    dev = a_batch(td, [(3, 2), None])
    assert lib.td_simb_route(dev._h, None) == TD_EINVAL and "null on" in err()
    assert route(dev._h, 0, 0) == 0      # all zeros on a handle that never had routes: nothing happens
    assert lib.td_simb_route_state(dev._h, 0, None, None, buf.ctypes.data) == TD_EINVAL and "no routes" in err()
    assert lib.td_simb_route_metrics(dev._h, out.ctypes.data) == TD_EINVAL and "no routes" in err()
    assert route(dev._h, 1, 1) == TD_EINVAL and "world 1 pools pairs" in err()      # pairs have no drop-off order
    assert lib.td_simb_route_metrics(dev._h, out.ctypes.data) == TD_EINVAL      # the refusal allocated nothing
    assert route(dev._h, 1, 0) == 0
    assert lib.td_simb_log(dev._h, 0xffe, 4096) == TD_EINVAL and "not built: the event log of routed worlds" in err()
    assert lib.td_simb_log(dev._h, 0, 0) == 0      # an empty mask is no log
    z = i32(0, 0)
    assert lib.td_simb_pooling(dev._h, None, None) == TD_EINVAL and "world 0's routes are on" in err()
    assert lib.td_simb_route_metrics(dev._h, None) == TD_EINVAL
    for world in (-1, 2):
        assert lib.td_simb_route_state(dev._h, world, None, None, buf.ctypes.data) == TD_EINVAL and "world %d outside 0 .. 1" % world in err()
    t = next(t for t in range(CITY["ticks"]) if dev.begin(t)[:, 0].any())
    assert route(dev._h, 0, 0) == TD_EINVAL and "waits for td_simb_apply" in err()      # only between ticks
    assert route(dev._h, 1, 0) == TD_EINVAL and "waits for td_simb_apply" in err()
    dev.apply([None, None])
    assert route(dev._h, 0, 0) == 0 and lib.td_simb_pooling(dev._h, None, None) == 0      # off: pairs are allowed again
    assert route(dev._h, 1, 0) == TD_EINVAL and "world 0 pools pairs" in err()      # and routes refused on the pair policy
    assert lib.td_simb_log(dev._h, 0xffe, 4096) == TD_EINVAL and "not built" in err()      # the handle keeps its route storage
    # a world without a policy keeps pooling pairs under td_simb_pooling_n's k_hi = 0 ("keep"): it cannot have routes on, so the
    # refusal of a td_simb_pooling_n call that leaves a routed world on pairs is not reachable through the C ABI
    assert lib.td_simb_pooling_n(dev._h, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0) == 0
    dev.close()
    logs = a_batch(td, [(2, 2), (2, 2)], events=True)
    assert route(logs._h, 0, 1) == TD_EINVAL and "not built" in err()      # a handle that logs
    assert route(logs._h, 0, 0) == 0
    logs.close()


def test_workspace_bytes_count_the_route_storage(td):
    base = B.ws()
    dev = a_batch(td, [(3, 2), (3, 2)])
    plain = B.ws()
    dev.set_route(False)
    assert B.ws() == plain      # all zeros allocates nothing
    dev.set_route([False, True])
    grown = B.ws() - plain
    nc, nr = 47, sum(dev.n_req)
    # 8 stop words and a position per cab, the drop-off tick per request, two record columns, four 64-bit counters per world, on [B]
    assert grown >= 4 * (9 * nc + 3 * nr + 2) + 32 * 2
    dev.set_route(False)
    dev.set_route(True)
    assert B.ws() - plain == grown      # allocated once
    dev.close()
    assert B.ws() == base


# ---- 7. td_simb_route_state's destinations ------------------------------------------------------------------------------------------------
def test_route_state_destinations(td):
    import torch
    lib = lib_of()
    dev = a_batch(td, [(3, 2), (4, 2)], route=True)
    for t in range(6):
        dev.tick(t)
    want = dev.route_state(1)
    assert (want["c_stops"] >= 0).any() and want["c_stops"].max() < 2 * dev.n_req[1]      # world-local request indices
    assert lib.td_simb_route_state(dev._h, 1, None, None, None) == 0      # every destination skipped
    pos = np.full(40, -7, np.int32)
    assert lib.td_simb_route_state(dev._h, 1, None, pos.ctypes.data, None) == 0 and np.array_equal(pos, want["c_pos"])
    drop = torch.full((dev.n_req[1],), -7, dtype=torch.int32, device="cuda")
    stops = torch.full((40, 8), -7, dtype=torch.int32, device="cuda")
    assert lib.td_simb_route_state(dev._h, 1, drop.data_ptr(), None, stops.data_ptr()) == 0      # device destinations
    torch.cuda.synchronize()
    assert np.array_equal(drop.cpu().numpy(), want["d_drop"]) and np.array_equal(stops.cpu().numpy(), want["c_stops"])
    assert lib.td_simb_route_state(dev._h, 2, None, pos.ctypes.data, None) == TD_EINVAL and "world 2 outside" in err()
    assert np.array_equal(pos, want["c_pos"])      # a refusal writes nothing
    dev.close()
