"""CPU tier: the small worlds of sim_worlds.py on the oracle backend reach every branch of the tick that the device world
(tests/test_gpu_sim_device.py) is compared on; this guards the inputs, not the device code."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim_worlds as sw


def test_generator_is_seeded_and_in_range():
    for name, w in sw.WORLDS.items():
        a, b = sw.gen_demand(**w), sw.gen_demand(**w)
        assert a.shape == b.shape and (a == b).all() and a.shape[0] > 0, name
        assert (a[:, 0] == range(a.shape[0])).all()                          # unique ids
        assert a[:, 1:3].min() >= 0 and a[:, 1:3].max() < w["stands"] and (a[:, 1] != a[:, 2]).all()
        assert (a[:, 4] >= a[:, 3]).all() and (a[:, 4] - a[:, 3]).max() < w["max_wait"]


def test_first_four_worlds_reach_every_branch():
    tot = {}
    for name in sw.FIRST_FOUR:
        run = sw.oracle_run(name)
        print(name, run["cover"])
        for k, v in run["cover"].items():
            if k == "cheat":
                for q in range(3):
                    tot["cheat%d" % q] = tot.get("cheat%d" % q, 0) + v[q]
            else:
                tot[k] = tot.get(k, 0) + v
    for k in ("empty_ticks", "no_lcm", "lcm_ends_on_big", "lcm_then_solver", "assign_and_go", "go_to_pickup", "cheat0", "cheat1",
              "cheat2", "arrive_empty", "arrive_loaded", "second_passengers", "drops", "pool_info_copied"):
        assert tot[k] >= 1, (k, tot)


@pytest.mark.parametrize("name,supply", [("wide1024", 1024), ("wide1025", 1025)])
def test_wide_worlds_fill_a_workgroup(name, supply):
    run = sw.oracle_run(name)
    t0 = run["ticks"][0]
    assert t0["n_sup"] == supply and t0["line"] is not None and "LCM n_pairs=" in t0["line"]
    assert all(tk["line"] is not None and "LCM" in tk["line"] for tk in run["ticks"])
