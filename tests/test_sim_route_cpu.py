"""The route model in the host specification, Simulator(route=True): the specification of td_sim_route.  CPU only: the oracle's
tick and oracle.pool_n as the stage's pool finder.  Hand-made worlds with the pick-up and drop-off ticks written out by hand
(sim_route_worlds.HAND), then family A's fleets with the three invariants checked after every tick and the cases they reach
asserted by count, so that a change of seed or rule cannot empty the tests that run the same worlds on the device."""
import os
import re

import numpy as np
import pytest

import sim_batch_worlds as sbw
import sim_route_worlds as R

CITY = sbw.CITY_A   # 12 stands, drop_time 4, max_non_lcm 16, 30 ticks
NAMES = ("A1", "A7", "A40", "A90")
SIZES = ((4, 2), (3, 3))
WAIT, LOSS = 1, 50
EV_LCM, EV_OPT = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- hand-made worlds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.HAND))
def test_a_hand_made_world(name):
    w = R.HAND[name]
    run = R.hand_run(name)
    sim, tr = run["sim"], run["sim"].route_trace
    assert sim.d_pick.tolist() == w["d_pick"] and sim.d_drop.tolist() == w["d_drop"]
    # one routed dispatch, on the path and in the way the world was made for
    assert tr["dispatches"] == {(EV_LCM if w["path"] == "lcm" else EV_OPT, w["how"]): 1}
    t0 = w["d_pick"][int(np.argmin(w["d_pick"]))]
    assert [f[:5] for f in tr["freed"]] == [(w["cab"], t0, w["cost"], w["free_t"], w["free_at"])] and w["free_t"] == t0 + w["cost"]
    assert (tr["zero_pick"], tr["zero_drop"], tr["same_tick_free"]) == (w.get("zero_pick", 0), w.get("zero_drop", 0), w.get("same_tick_free", 0))
    k = len(w["d_pick"])
    assert sim.c_pos[w["cab"]] == 2 * k and (sim.c_stops[w["cab"], :2 * k] >= 0).all() and (sim.c_stops[w["cab"], 2 * k:] == -1).all()
    # the cab tick by tick: busy with the first pick-up as its client until the free tick, then free at the last drop-off's stand
    for rec in run["ticks"]:
        st, c = rec["state"], w["cab"]
        if rec["t"] < w["free_t"]:
            assert st["c_clnt"][c] != -1, rec["t"]
        else:
            assert (st["c_from"][c], st["c_to"][c], st["c_clnt"][c], st["c_onboard"][c], st["c_start"][c]) == (w["free_at"], w["free_at"], -1, 0, -1)
    m = sim.route_m
    solo = sum(int(sim._way(int(f), int(t))) for f, t in zip(sim.d_from, sim.d_to))
    assert m["drop_numb"] == k and m["ride_time"] == sum(d - p for p, d in zip(w["d_pick"], w["d_drop"])) and m["solo_time"] == solo
    # the existing metrics are counted where they were: every member a pick-up, every member but the first a second passenger
    assert sim.m["total_pickup_numb"] == k and sim.m["total_second_passengers"] == k - 1 and sim.m["total_dropped"] == 0


@pytest.mark.parametrize("name", sorted(R.HAND))
def test_without_routes_the_same_world_runs_as_before(name):
    """route=False: the members but the first are never picked up, nobody is dropped off, and the run has no route state"""
    w = R.HAND[name]
    off = R.hand_run(name, route=False)["sim"]
    first = int(np.argmin(w["d_pick"]))
    assert [p for i, p in enumerate(off.d_pick.tolist()) if i != first] == [-1] * (len(w["d_pick"]) - 1)
    assert not hasattr(off, "d_drop") and not hasattr(off, "route_m")
    assert off.m == R.hand_run(name)["sim"].m      # the metrics do not see the route


def test_off_the_line_the_cab_ends_elsewhere_without_routes():
    """the pool costs 7 from stand 5 on a line of 10: cheat_a_bit clamps to stand 0, the cab is busy for 5 ticks and ends where
    nobody asked to go; with routes it is busy for the cost and ends at the last drop-off"""
    w = R.HAND["off_line"]
    off, on = R.hand_run("off_line", route=False), R.hand_run("off_line")
    free_off = next(r["t"] for r in off["ticks"] if r["t"] > 0 and r["state"]["c_clnt"][5] == -1)
    assert free_off == 5 and off["ticks"][-1]["state"]["c_from"][5] == 0
    assert on["ticks"][-1]["state"]["c_from"][5] == 8 and w["free_t"] == 7
    assert on["sim"].route_m["max_over_loss"] == 0      # r0 rides 6 for a direct way of 4 under a loss of 50 percent: exactly the limit


def test_on_the_lcm_path_the_pool_is_forgotten_without_routes():
    off, on = R.hand_run("lcm_heading", route=False), R.hand_run("lcm_heading")
    # without routes the heading cab drives the first passenger's own trip 3 -> 6 and is free at t = 5 all the same; r1 counts as
    # a second passenger and is never picked up.  With routes r1 rides 4 -> 5 on the way
    assert off["sim"].d_pick.tolist() == [2, -1] and on["sim"].d_pick.tolist() == [2, 3] and on["sim"].d_drop.tolist() == [5, 4]
    assert off["sim"].m == on["sim"].m and on["sim"].m["total_LCM_used"] == 1 and (on["sim"].d_pool_id == -1).all()


# ---- family A -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cover():
    """every fleet under both size pairs; spec_run checks the three invariants after every tick"""
    city, runs = sbw.family("A")
    out = {}
    for name, run in runs:
        if name not in NAMES:
            continue
        for pn in SIZES:
            out[name, pn] = R.spec_run(run["rows"], run["world"]["cabs"], CITY, CITY["ticks"], pn, WAIT, LOSS)
    return out


# summed over the four fleets and the two size pairs: routed dispatches by (path, standing / heading), zero-length pick and
# drop legs, cabs freed by a zero-length last leg, finished routes, dropped-off members
COVER_COUNTS = {"lcm standing": 297, "lcm heading": 80, "opt standing": 49, "opt heading": 51, "zero_pick": 567, "zero_drop": 489,
                "same_tick_free": 179, "freed": 393, "drop_numb": 1210}


def test_the_fleets_reach_every_case(cover):
    tot = dict.fromkeys(COVER_COUNTS, 0)
    for (name, pn), run in cover.items():
        tr = run["sim"].route_trace
        for (method, how), n in tr["dispatches"].items():
            tot["%s %s" % ("lcm" if method == EV_LCM else "opt", how)] += n
        for k in ("zero_pick", "zero_drop", "same_tick_free"):
            tot[k] += tr[k]
        tot["freed"] += len(tr["freed"])
        tot["drop_numb"] += run["sim"].route_m["drop_numb"]
    print(tot)
    for k, v in tot.items():
        assert v > 0, k
    assert tot == COVER_COUNTS


def test_the_invariants_hold_at_the_end_too(cover):
    for (name, pn), run in cover.items():
        sim = run["sim"]
        R.check_invariants(sim, CITY["ticks"])
        m = sim.route_m
        assert m["max_over_loss"] <= 0 and m["ride_time"] >= m["solo_time"] > 0, (name, pn, m)
        # a member is dropped off only after it was assigned; some routes are still being driven when the run ends
        assert (sim.d_cab[sim.d_drop >= 0] >= 0).all()
        assert m["drop_numb"] <= sim.m["total_pickup_numb"], (name, pn)


# ---- the surface ------------------------------------------------------------------------------------------------------------------
def test_keyword_refusals():
    from taxidispatcher_amd import simulator as S
    rows = np.zeros((0, 5), np.int64)
    with pytest.raises(ValueError, match="pool_n"):
        S.Simulator(rows, backend=object(), n_cabs=3, route=True)
    with pytest.raises(ValueError, match="pool_n"):
        S.Simulator(rows, backend=object(), n_cabs=3, route=True, pool="optimal")
    with pytest.raises(ValueError, match="not built"):
        S.Simulator(rows, backend=object(), n_cabs=3, route=True, pool_n=2, events=True)
    with pytest.raises(ValueError, match="pool_n"):
        S.DeviceSimulator(rows, n_cabs=3, route=True)
    with pytest.raises(ValueError, match="not built"):
        S.DeviceSimulator(rows, n_cabs=3, route=True, pool_n=2, events=True)
    sim = S.Simulator(rows, backend=object(), n_cabs=3, route=True, pool_n=(4, 2))
    assert sim.route_m == dict(drop_numb=0, ride_time=0, solo_time=0, max_over_loss=S.ROUTE_NONE_SEEN) and S.ROUTE_NONE_SEEN == -2**63
    assert sim.c_stops.shape == (3, 8) and (sim.c_stops == -1).all() and (sim.c_pos == 0).all()
    import inspect
    assert "route" not in inspect.signature(S.DeviceSimulatorBatch.__init__).parameters      # cut on purpose


def test_the_header_and_the_ffi_agree_on_the_new_calls():
    import ctypes
    from taxidispatcher_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "taxidispatcher_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in ("td_sim_route", "td_sim_route_state", "td_sim_route_metrics"):
        m = re.search(r"TD_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _ffi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            assert a is (ctypes.c_void_p if "*" in p or "[" in p else ctypes.c_int), (name, p, a)
    assert "#define TD_SIM_N_ROUTE_METRICS 4" in hdr


def test_the_calls_are_built_and_exported():
    import __graft_entry__ as entry
    entry.build()
    from taxidispatcher_amd import _ffi
    lib = _ffi.load()
    assert lib.td_sim_route is not None and lib.td_sim_route_state is not None and lib.td_sim_route_metrics is not None
