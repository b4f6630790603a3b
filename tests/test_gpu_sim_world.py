"""One set of world kernels (csrc/td_sim_world.h), two drivers: a td_sim handle and a td_simb handle of ONE world run in
lockstep through begin / model / apply on the same decisions, the CPU oracle run's (as test_trace_driven_against_the_oracle
takes them).  After every tick the info words, the model lists, the OPT count, the ten state arrays and the nine metrics of
the two handles are equal: exact integer equality, no tick and no world left out.
The two handles are compared with each other only; that either equals the CPU world model is what the trace-driven tests of
test_gpu_sim_device.py, test_gpu_sim_dist.py and test_gpu_sim_batch.py assert.

Worlds: `tiny`, `wide1025` (the chunk edge of the 1024-thread passes; its model goes through the LCM) and `grid3x2`, the
smallest world on a distance table."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_worlds as sb
import sim_dist_worlds as sd
import sim_worlds as sw

pytestmark = pytest.mark.gpu


def the_run(name):
    """-> (oracle run, distance table or None)"""
    return (sd.oracle_run(name), sd.table(name)) if name in sd.WORLDS else (sw.oracle_run(name), None)


@pytest.mark.parametrize("name", ["tiny", "wide1025", "grid3x2"])
def test_one_world_equals_a_batch_of_one(td, name):
    run, D = the_run(name)
    w = run["world"]
    kw = dict(n_stands=w["stands"], drop_time=w["drop_time"], max_non_lcm=w["max_non_lcm"], big_cost=sw.BIG_COST, dist=D)
    one = td.DeviceSimulator(run["rows"], n_cabs=w["cabs"], **kw)
    bat = td.DeviceSimulatorBatch([run["rows"]], [w["cabs"]], **kw)
    assert len(run["ticks"]) == w["ticks"] and any(rec["res"] is not None for rec in run["ticks"])
    for rec in run["ticks"]:
        t = rec["t"]
        info = one.begin(t)
        assert info == tuple(bat.begin(t)[0].tolist()), t
        assert info[0] == (rec["n_dem"] > 0), t
        if info[0]:
            cab_to, dem_from = one.model()
            cab_off, b_cab_to, dem_off, b_dem_from = bat.model()
            assert cab_off.tolist() == [0, len(cab_to)] and dem_off.tolist() == [0, len(dem_from)], t
            assert np.array_equal(cab_to, b_cab_to) and np.array_equal(dem_from, b_dem_from), t
            dec = sb.decisions_of(rec)
            opt = one.apply() if dec is None else one.apply(*dec)
            assert opt == int(bat.apply([dec])[0]), t
        assert one.m == bat.m[0], t
        a, b = one.state(), bat.state(0)
        assert a.keys() == b.keys() and len(a) == 10
        for k in a:
            assert np.array_equal(a[k], b[k]), (t, k, np.nonzero(a[k] != b[k])[0][:8].tolist())
    one.close()
    bat.close()
