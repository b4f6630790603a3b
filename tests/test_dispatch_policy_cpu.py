"""The dispatch policies of the host specification (simulator.Simulator(dispatch=, max_non_lcm=, parts=)) on the oracle, and
the coverage the small worlds give the split: asserted here, without a GPU, so that a change of seed cannot empty the tests
that run the same worlds on the device."""
import numpy as np
import pytest

import sim_batch_worlds as sbw
import sim_dispatch_policy as P

CITY = sbw.CITY_A   # 12 stands, drop_time 4, max_non_lcm 16, 30 ticks
NAMES = ("A1", "A7", "A40", "A90")


@pytest.fixture(scope="module")
def worlds():
    city, runs = sbw.family("A")
    return {name: run for name, run in runs}


def _run(worlds, name, **policy):
    run = worlds[name]
    return P.policy_run(run["rows"], run["world"]["cabs"], CITY, CITY["ticks"], **policy)


@pytest.mark.parametrize("name", NAMES)
def test_default_keywords_reproduce_the_run(worlds, name):
    """a Simulator without a dispatch keyword, and one with the defaults spelt out, take the course they took before"""
    for kw in ({}, {"dispatch": "lcm+opt", "max_non_lcm": None, "parts": 4}):
        got = _run(worlds, name, **kw)
        assert got["log"] == worlds[name]["log"]
        assert got["m"] == worlds[name]["ticks"][-1]["m"]
        for k, v in worlds[name]["ticks"][-1]["state"].items():
            assert np.array_equal(got["state"][k], v), k
    # the same stop size as a policy of the world's own goes step by step and ends in the same place
    own = _run(worlds, name, max_non_lcm=CITY["max_non_lcm"])
    assert own["log"] == worlds[name]["log"] and own["m"] == worlds[name]["ticks"][-1]["m"]


@pytest.mark.parametrize("name", NAMES)
def test_a_stop_size_above_every_model_is_the_optimum_alone(worlds, name):
    top = max(max(rec["n_sup"], rec["n_dem"]) for rec in worlds[name]["ticks"])
    a, b = _run(worlds, name, dispatch="lcm+opt", max_non_lcm=top), _run(worlds, name, dispatch="opt")
    assert a["lines"] == b["lines"] and a["m"] == b["m"] and a["m"]["total_LCM_used"] == 0
    assert all("LCM" not in line for line in b["log"])
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k]), k


@pytest.mark.parametrize("name", NAMES)
def test_the_lcm_alone_never_solves(worlds, name):
    got = _run(worlds, name, dispatch="lcm")
    assert got["backend"].solves == 0
    with_supply = [line for line in got["log"] if "supply=0." not in line]
    assert with_supply and all("OPT count" not in line and "LCM n_pairs=" in line and "Sent to solver" not in line for line in with_supply)
    assert got["m"]["total_LCM_used"] == len(with_supply) and got["m"]["max_solver_size"] == 0


def _split_cover(worlds):
    out = {}
    for name in NAMES:
        # 12 stands: parts 4 gives ranges of 3 stands, parts 5 ranges of 2 stands, 6 of them; inside such a range every distance
        # is below drop_time 4, so a region pair the threshold refuses needs wider ranges: parts 2, ranges of 6 stands
        for parts in (4, 5, 2):
            got = _run(worlds, name, dispatch="split", parts=parts)
            cov = got["backend"].cover
            rec = {k: sum(c[k] > 0 for c in cov) for k in ("fifth_serves", "cabs_only", "requests_only", "more_cabs", "more_requests",
                                                           "refused_pair")}
            rec.update(ticks=len(cov), no_supply=got["no_supply"], served=sum(c["served"] for c in cov))
            out[name, parts] = (rec, got)
    return out


def test_split_worlds_stay_consistent_and_cover_the_branches(worlds):
    """every split decision passes check_split_model inside the backend; the lines are the optimum's lines; and between them
    the worlds reach every branch of the split"""
    out = _split_cover(worlds)
    for (name, parts), (rec, got) in out.items():
        assert got["m"]["total_LCM_used"] == 0 and all("LCM" not in line and "OPT count=" in line for line in got["log"]), (name, parts)
        served = sum(int(line.split("OPT count=")[1]) for line in got["log"])
        assert served == rec["served"], (name, parts)
        top = max(max(rec_["n_sup"], rec_["n_dem"]) for rec_ in worlds[name]["ticks"])
        assert 0 < got["m"]["max_solver_size"] <= max(got["m"]["max_model_size"], top)
    tot = lambda k: sum(rec[k] for rec, _ in out.values())
    for k in ("fifth_serves", "cabs_only", "requests_only", "more_cabs", "more_requests", "refused_pair", "no_supply"):
        assert tot(k) > 0, k
    got = {k: tot(k) for k in COVER_COUNTS}
    print(got)
    assert got == COVER_COUNTS
    assert out["A40", 2][0]["refused_pair"] == 1   # the one tick with a region pair the threshold refuses


# the ticks (summed over the four worlds and parts 4, 5, 2) in which a split decision has: a fifth solve that serves somebody;
# a region with cabs only; with requests only; with more cabs than requests; with more requests than cabs; a region pair
# refused by the threshold; and the ticks with waiting requests and no supply.  From sim_batch_worlds.FAMILY_A's seeds.
COVER_COUNTS = dict(fifth_serves=51, cabs_only=92, requests_only=96, more_cabs=176, more_requests=131, refused_pair=1, no_supply=75)


def test_policy_arguments_are_checked():
    from taxidispatcher_amd import simulator
    rows = np.zeros((0, 5), np.int64)
    for kw in ({"dispatch": "greedy"}, {"max_non_lcm": -1}, {"dispatch": "split", "parts": 0}, {"dispatch": "split", "parts": 33}):
        with pytest.raises(ValueError):
            simulator.Simulator(rows, backend=object(), n_cabs=3, **kw)
    assert simulator.dispatch_mode("split") == 3 and simulator.DISPATCH_MODES == {"lcm+opt": 0, "opt": 1, "lcm": 2, "split": 3}
