"""CPU tier of the distance-table simulator (Simulator(dist=...)) on the oracle backend: a table filled with |a - b| is the
line world; the worlds of sim_dist_worlds.py reach every branch the device world (tests/test_gpu_sim_dist.py) is compared
on, the two directions of the near test included; a hand-checked one-way pair; what an invalid table raises."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_dist_worlds as sd
import sim_worlds as sw


@pytest.mark.parametrize("name", ["tiny", "small", "mid65"])
def test_line_table_is_the_line_world(name):
    ref = sw.oracle_run(name)
    w = ref["world"]
    got = sd.run_world(ref["rows"], sd.line(w["stands"]), w)
    assert got["log"] == ref["log"]
    for a, b in zip(got["ticks"], ref["ticks"]):
        assert a["line"] == b["line"] and a["m"] == b["m"], a["t"]
        assert (a["n_dem"], a["n_sup"], a["cab_to"], a["dem_from"]) == (b["n_dem"], b["n_sup"], b["cab_to"], b["dem_from"]), a["t"]
        for k, v in b["state"].items():
            assert np.array_equal(a["state"][k], v), (a["t"], k)


def test_tables_and_generator():
    assert sd.grid(3, 2).tolist()[0] == [0, 1, 2, 1, 2, 3] and sd.ring(4).tolist()[1] == [3, 0, 1, 2]
    for name in sd.WORLDS:
        D, w = sd.table(name), sd.world(name)
        from taxidispatcher_amd import simulator
        assert simulator.check_dist(D).shape == (w["stands"], w["stands"])
        if name != "ring2100p":
            a, b = sd.gen_demand(D, **w), sd.gen_demand(D, **w)
            assert a.shape == b.shape and (a == b).all() and a.shape[0] > 0
            assert (a[:, 0] == range(a.shape[0])).all() and (a[:, 1] != a[:, 2]).all()
            assert (D[a[:, 1], a[:, 2]] <= w["span"]).all() and (a[:, 4] - a[:, 3]).max() < w["max_wait"]
    P = sd.table("ring2100p")
    assert (P + P.T)[~np.eye(2100, dtype=bool)].min() == 2100 == (P + P.T).max()      # still a one-way ring


def test_worlds_reach_every_branch_and_both_directions():
    tot = {}
    for name in sd.WORLDS:
        run = sd.oracle_run(name)
        print(name, run["cover"])
        for k, v in run["cover"].items():
            if k == "cheat":
                for q in range(3):
                    tot["cheat%d" % q] = tot.get("cheat%d" % q, 0) + v[q]
            else:
                tot[k] = tot.get(k, 0) + v
    for k in ("no_lcm", "lcm_ends_on_big", "lcm_then_solver", "assign_and_go", "go_to_pickup", "arrive_empty", "arrive_loaded", "cheat0",
              "cheat1", "cheat2", "second_passengers", "drops", "pool_info_copied", "dir_dem", "dir_sup"):
        assert tot[k] > 0, (k, tot)
    big = sd.oracle_run("ring2100p")["cover"]
    assert big["hi_dem"] > 0 and big["hi_sup"] > 0      # stands behind the first 64 x 32 bits of the flag words


ONE_WAY = np.array([[0, 1, 9], [9, 0, 9], [9, 9, 0]], np.int32)
PAIR_WORLD = dict(stands=3, drop_time=3, max_non_lcm=4, cabs=1, ticks=12)
PAIR_ROWS = np.array([[0, 1, 2, 0, 0]], np.int64)


def test_one_way_pair():
    """one cab at stand 0, one request 1 -> 2 at t = 0, d[0][1] = 1 but d[1][0] = 9, drop_time 3"""
    run = sd.run_world(PAIR_ROWS, ONE_WAY, PAIR_WORLD)
    t0, t1 = run["ticks"][0], run["ticks"][1]
    assert (t0["n_dem"], t0["n_sup"], t0["cab_to"], t0["dem_from"]) == (1, 1, [0], [1])
    assert t0["line"] == "t:0. Initial Count of demand=1, supply=1. ; OPT count=1"
    assert run["cover"]["go_to_pickup"] == 1 and run["cover"]["assign_and_go"] == 0
    st = t0["state"]                                       # on the way to the pick-up: one tick, dist[0][1]
    assert (st["c_from"][0], st["c_to"][0], st["c_onboard"][0], st["c_start"][0], st["d_cab"][0]) == (0, 1, 0, 0, 0)
    assert t0["m"]["total_pickup_time"] == 1 and t0["m"]["total_pickup_numb"] == 0
    st = t1["state"]                                       # picked up exactly at t = 1
    assert (st["c_from"][0], st["c_to"][0], st["c_onboard"][0], st["c_start"][0], st["d_pick"][0]) == (1, 2, 1, 1, 1)
    assert t1["m"]["total_pickup_numb"] == 1
    trip = int(ONE_WAY[1, 2])
    for tk in run["ticks"][1:]:                            # the trip takes d[1][2] ticks
        loaded = tk["t"] < 1 + trip
        assert tk["state"]["c_onboard"][0] == (1 if loaded else 0), tk["t"]
        assert tk["state"]["c_from"][0] == (1 if loaded else 2), tk["t"]
    assert run["cover"]["arrive_empty"] == 1 and run["cover"]["arrive_loaded"] == 1 and run["ticks"][-1]["m"]["total_dropped"] == 0


def test_one_way_pair_transposed():
    run = sd.run_world(PAIR_ROWS, ONE_WAY.T.copy(), PAIR_WORLD)
    assert run["ticks"][0]["line"] is None and run["ticks"][0]["n_dem"] == 0 and run["ticks"][0]["res"] is None
    assert run["log"] == []
    for tk in run["ticks"]:
        assert tk["m"]["total_dropped"] == (1 if tk["t"] >= 3 else 0), tk["t"]
        assert tk["state"]["d_cab"][0] == (-2 if tk["t"] >= 3 else -1), tk["t"]
        assert tk["state"]["c_to"][0] == 0 and tk["state"]["c_clnt"][0] == -1


def bad_tables():
    ok = sd.line(5)

    def put(i, j, v):
        d = ok.astype(np.int64)
        d[i, j] = v
        return d
    return {"non-square": ok[:4], "wrong size": sd.line(6), "negative": put(1, 3, -1), "diagonal": put(2, 2, 1), "zero": put(3, 1, 0),
            "too large": put(0, 4, 0x20000000), "not 2-d": ok[0]}


@pytest.mark.parametrize("what", list(bad_tables()))
def test_invalid_table_raises(what, monkeypatch):
    from taxidispatcher_amd import simulator
    monkeypatch.setattr(simulator, "N_STANDS", 5)
    rows = np.array([[0, 1, 2, 0, 0]], np.int64)
    with pytest.raises(ValueError):
        simulator.Simulator(rows, sd.OracleDistTickBackend(sd.line(5)), n_cabs=2, dist=bad_tables()[what])
    good = sd.line(5).astype(np.int64)
    good[0, 4] = 0x1fffffff                                 # the largest entry a table may hold
    assert simulator.Simulator(rows, sd.OracleDistTickBackend(good), n_cabs=2, dist=good).dist[0, 4] == 0x1fffffff
    with pytest.raises(ValueError):
        simulator.check_dist(np.zeros((4097, 4097), np.int8))
