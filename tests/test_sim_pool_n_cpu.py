"""Pools of up to four in the host specification, Simulator(pool_n=, pool_wait=, pool_loss=): the specification of
td_sim_pooling_n.  CPU only: the oracle's tick and oracle.pool_n as the stage's pool finder.  The coverage the small worlds
give is asserted here by count, so that a change of seed or rule cannot empty the tests that run the same worlds on the device."""
import numpy as np
import pytest

import sim_batch_worlds as sbw
import sim_pool_n_worlds as W

CITY = sbw.CITY_A   # 12 stands, drop_time 4, max_non_lcm 16, 30 ticks
NAMES = ("A1", "A7", "A40", "A90")


@pytest.fixture(scope="module")
def worlds():
    city, runs = sbw.family("A")
    return {name: run for name, run in runs}


@pytest.fixture(scope="module")
def cover(worlds):
    """every fleet under every size pair, each tick checked (check_tick: the cascade restated, the invariants) -> the counts"""
    out = {}
    for name in NAMES:
        for pn in W.SIZES:
            run = W.spec_run(worlds[name]["rows"], worlds[name]["world"]["cabs"], CITY, CITY["ticks"], pn)
            c = dict(three_sizes=0, short_stage=0, lcm_pools=0, opt_pools=0, lost_pools=0, no_supply=0, pools=0, seconds=0, max_happy=0, max_pools=0)
            for rec in run["ticks"]:
                happy, short = W.check_tick(rec, pn)
                c["short_stage"] += short
                c["max_happy"], c["max_pools"] = max(c["max_happy"], happy), max(c["max_pools"], len(rec["plans"]))
                c["three_sizes"] += {len(p[0]) for p in rec["plans"]} == {2, 3, 4}
                for k in ("lcm_pools", "opt_pools", "lost_pools", "seconds"):
                    c[k] += rec[k]
                c["pools"] += len(rec["plans"])
                c["no_supply"] += rec["line"] is not None and "supply=0." in rec["line"]
            out[name, pn] = (c, run)
    return out


def test_metrics_follow_the_cascade(cover):
    """max_POOL_size: the most pools of a tick, all stages; max_POOL_MEM_size: the most happy plans of a tick, summed over its
    stages; total_second_passengers: size - 1 per dispatched pool"""
    for (name, pn), (c, run) in cover.items():
        assert run["m"]["max_POOL_size"] == c["max_pools"] and run["m"]["max_POOL_MEM_size"] == c["max_happy"], (name, pn)
        assert run["m"]["total_second_passengers"] == c["seconds"], (name, pn)
        assert c["max_happy"] <= 65536, (name, pn)      # td_pool_n_batched's default max_happy holds every stage of these worlds


# summed over the four fleets and the five size pairs, under sim_pool_n_worlds' rule (WAIT, LOSS): ticks with pools of all three
# sizes in one cascade; stages whose list was shorter than their k; pools dispatched on the LCM path; on the OPT path; pools
# whose first pick-up found no cab; ticks with demand and no supply; pools found; second passengers
COVER_COUNTS = dict(three_sizes=43, short_stage=13, lcm_pools=1019, opt_pools=311, lost_pools=783, no_supply=6, pools=2113, seconds=2223)


def test_the_worlds_reach_every_case(cover):
    tot = {k: sum(c[k] for c, _ in cover.values()) for k in ("three_sizes", "short_stage", "lcm_pools", "opt_pools", "lost_pools", "no_supply",
                                                             "pools", "seconds")}
    print(tot)
    for k, v in tot.items():
        assert v > 0, k
    assert tot == COVER_COUNTS
    # all three sizes in one cascade needs (4, 2); a pool of each size is dispatched on each path somewhere
    assert all(c["three_sizes"] == 0 for (name, pn), (c, _) in cover.items() if pn != (4, 2))
    assert all(cover[name, (4, 2)][0]["three_sizes"] > 0 for name in NAMES)


def test_a_lost_pool_returns_next_tick(cover):
    """a pool whose first pick-up finds no cab: its members stay assigned to nobody, and those still waiting are in the next
    tick's demand again"""
    seen = 0
    for (name, pn), (c, run) in cover.items():
        sim = run["sim"]
        for rec, nxt in zip(run["ticks"], run["ticks"][1:]):
            if not rec["plans"] or nxt["ids"] is None:
                continue
            for picks, _, _ in rec["plans"]:
                first = sim.id2idx[rec["ids"][picks[0]]]
                if rec["state"]["d_cab"][first] != -1:
                    continue
                members = [sim.id2idx[rec["ids"][d]] for d in picks]
                assert all(rec["state"]["d_cab"][m] == -1 for m in members), (name, pn, rec["t"])
                back = [m for m in members if nxt["t"] - sim.d_at[m] < CITY["drop_time"]]
                # createTempDemand admits a waiting request only near a free cab: the members it admits are requests like any other
                seen += sum(int(sim.d_id[m]) in nxt["ids"] for m in back)
    assert seen > 0


def test_pool_info_reaches_the_table_on_the_opt_path_only(cover):
    for (name, pn), (c, run) in cover.items():
        st = run["state"]
        rows = np.nonzero(st["d_pool_id"] != -1)[0]
        assert set(st["d_pool_plan"][rows].tolist()) <= set(range(pn[1], pn[0] + 1)), (name, pn)
        assert (st["d_pool_plan"][st["d_pool_id"] == -1] == -1).all()
        if c["opt_pools"] == 0:
            assert rows.size == 0, (name, pn)
        # an OPT pool's row is written in the tick it is dispatched: never more rows than OPT pools
        assert rows.size <= c["opt_pools"], (name, pn)
    assert any(c["lcm_pools"] > 0 and c["opt_pools"] == 0 for c, _ in cover.values())


@pytest.mark.parametrize("name", NAMES)
def test_pool_n_none_changes_nothing(worlds, name):
    """pool_n=None: line for line, metric for metric and row for row the run without the keyword"""
    from taxidispatcher_amd import simulator
    import sim_backend
    import sim_worlds as sw
    run = worlds[name]
    with pytest.MonkeyPatch.context() as mp:
        sw.patch_constants(mp, CITY)
        for kw in ({"pool_n": None}, {"pool_n": None, "pool_wait": 3, "pool_loss": 40}):
            sim = simulator.Simulator(run["rows"], sim_backend.OracleTickBackend(), n_cabs=run["world"]["cabs"], events=True, **kw)
            ref = simulator.Simulator(run["rows"], sim_backend.OracleTickBackend(), n_cabs=run["world"]["cabs"], events=True)
            assert sim.run(CITY["ticks"]) == ref.run(CITY["ticks"]) == run["log"]
            assert sim.m == ref.m == run["ticks"][-1]["m"] and sim.events == ref.events
            for k, v in run["ticks"][-1]["state"].items():
                assert np.array_equal(sw.state_of(sim)[k], v), k


def test_events_of_the_specification(worlds):
    """EV_POOL carries the total pool count, one EV_POOL_PAIR (customer = the first pick-up, aux = the member) and one
    EV_POOLED_SECOND per other member"""
    from taxidispatcher_amd import simulator as S
    run = W.spec_run(worlds["A40"]["rows"], 40, CITY, CITY["ticks"], (4, 2), events=True)
    ev = np.asarray(run["events"], np.int64).reshape(-1, 8)
    for rec in run["ticks"]:
        mine = ev[ev[:, 0] == rec["t"]]
        heads = mine[mine[:, 2] == S.EV_POOL]
        if rec["dem"] is None:
            assert heads.shape[0] == 0
            continue
        assert heads.shape[0] == 1 and heads[0, 6] == len(rec["plans"])
        pairs = [(int(r[4]), int(r[6])) for r in mine[mine[:, 2] == S.EV_POOL_PAIR]]
        assert pairs == [(rec["ids"][p[0]], rec["ids"][d]) for p, _, _ in rec["plans"] for d in p[1:]]
        assert (mine[:, 2] == S.EV_POOLED_SECOND).sum() == rec["second_delta"]
    assert (ev[:, 2] == S.EV_POOLED_SECOND).sum() == run["m"]["total_second_passengers"] > 0


def test_keyword_refusals():
    from taxidispatcher_amd import simulator
    rows = np.zeros((0, 5), np.int64)
    for kw in ({"pool_n": 1}, {"pool_n": 5}, {"pool_n": (2, 3)}, {"pool_n": (4, 1)}, {"pool_n": (5, 2)}, {"pool_n": (4, 3, 2)}, {"pool_n": 2.5},
               {"pool_n": "4"}, {"pool_n": 3, "pool_wait": -1}, {"pool_n": 3, "pool_loss": -1}, {"pool_n": 3, "pool_wait": 1.5}):
        with pytest.raises((ValueError, TypeError)):
            simulator.Simulator(rows, backend=object(), n_cabs=3, **kw)
    assert simulator.pool_n_sizes(3) == (3, 3) and simulator.pool_n_sizes((4, 2)) == (4, 2) and simulator.pool_n_sizes(None) is None
    # the pair policy's names are what they were
    assert simulator.POOL_MODES == {"none": 0, "greedy": 1, "optimal": 2}
    with pytest.raises(ValueError):
        simulator.pool_mode("n")


def test_a_short_list_and_an_empty_tick():
    """fewer than two requests: findPool as today (no pool, the header with 0); a stage list shorter than its k: no pools"""
    from taxidispatcher_amd import simulator
    sim = simulator.Simulator(np.zeros((0, 5), np.int64), backend=W.PoolNOracleBackend(), n_cabs=3, pool_n=(4, 2), events=True)
    assert sim.find_pool_n([[7, 1, 2, -1, -1, 0]], 0) == [] and sim.events[-1][2] == simulator.EV_POOL and sim.events[-1][6] == 0
    # three requests on one stand going the same way: no pool of four, one of three
    dem = [[i, 2, 4, -1, -1, 0] for i in range(3)]
    plans = sim.find_pool_n(dem, 1)
    assert [len(p[0]) for p in plans] == [3] and sim.m["max_POOL_size"] == 1
    out, others = sim.analyze_pool_n(plans, dem)
    first = plans[0][0][0]
    assert [c[0] for c in out] == [first] and out[0][3:] == [plans[0][0][1], 3, plans[0][2]] and others == {first: plans[0][0][1:]}
