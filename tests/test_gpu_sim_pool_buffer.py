"""td_sim_pool_buffer: a world under td_sim_pooling_n whose stages run through td_pool_n_banded.  The world of
test_gpu_sim_pool_n.py::test_max_happy_is_refused_by_begin_with_the_count, with one happy plan too many for its max_happy, is
still refused without the call and runs to its end with it, equal tick by tick to a world with room and to the host Simulator
on HipBackend(pool_buffer=...); the call's refusals and life cycle."""
import numpy as np
import pytest

import sim_pool_n_worlds as W
import test_gpu_sim_pool_n as T

pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ERANGE = -1, -4
ROOM = 24 * 2047
CITY = dict(stands=12, drop_time=4, max_non_lcm=16)
TICKS = 12


def tight_world():
    """40 requests of tick 0 on 9 stands, 12 cabs, pools of four under wait 0 / loss 50: -> (rows, the cascade's plans, its
    happy plans)"""
    rng = np.random.default_rng(9)
    n = 40
    frm = rng.integers(0, 9, n)
    rows = np.stack([np.arange(n), frm, frm + rng.integers(1, 4, n), np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1).astype(np.int64)
    want, happy, _ = W.cascade(4, 4, rows[:, 1], rows[:, 2], 0, 50)
    assert happy > 1000 and want
    return rows, want, happy


def test_a_world_past_its_max_happy_runs_with_the_buffer(td):
    from taxidispatcher_amd import simulator
    rows, want, happy = tight_world()
    lib = T.lib_of()
    info = np.zeros(4, np.int32)
    # without the call: refused, as before
    tight = T.device_world(td, rows, 12, CITY, (4, 4), wait=0, loss=50, max_happy=happy - 1)
    assert lib.td_sim_begin(tight._h, 0, info.ctypes.data) == TD_ERANGE and str(happy) in T.err()
    tight.close()
    # the specification on the banded finder, recorded once
    run = W.spec_run(rows, 12, CITY, TICKS, (4, 4), wait=0, loss=50, backend=simulator.HipBackend(max_happy=happy - 1, pool_buffer=ROOM))
    assert run["ticks"][0]["plans"] == want and run["m"]["max_POOL_MEM_size"] == happy
    assert run["m"]["total_second_passengers"] > 0 and sum(r["line"] is not None for r in run["ticks"]) >= 2
    banded = T.device_world(td, rows, 12, CITY, (4, 4), wait=0, loss=50, max_happy=happy - 1, pool_buffer=ROOM)
    roomy = T.device_world(td, rows, 12, CITY, (4, 4), wait=0, loss=50)
    assert banded.pool_buffer == ROOM and roomy.pool_buffer == 0
    for rec in run["ticks"]:
        t = rec["t"]
        for name, dev in (("banded", banded), ("roomy", roomy)):
            assert dev.tick(t) == rec["line"], (name, t)
            assert dev.pools_n() == rec["plans"], (name, t)
            T.assert_same(dev, rec, (name, t))
    assert banded.m["max_POOL_MEM_size"] == happy      # the true count, not what a band held
    banded.close(), roomy.close()


def test_a_cascade_through_the_buffer_equals_the_calls_it_replaces(td):
    """(4, 2) under the family rule on a family-A fleet: three stages a tick, each a td_pool_n_batched model without the buffer
    and a td_pool_n_banded call with it"""
    import sim_batch_worlds as sbw
    city, runs = sbw.family("A")
    world = dict(runs)["A40"]
    rows, cabs = world["rows"], world["world"]["cabs"]
    a = T.device_world(td, rows, cabs, city, (4, 2))
    b = T.device_world(td, rows, cabs, city, (4, 2), pool_buffer=ROOM)
    pooled = 0
    for t in range(city["ticks"]):
        assert a.tick(t) == b.tick(t), t
        assert a.pools_n() == b.pools_n(), t
        pooled += len(a.pools_n())
        assert a.m == b.m, t
        sa, sb = a.state(), b.state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (t, k)
    assert pooled > 10 and {len(p[0]) for p in b.pools_n()} <= {2, 3, 4}
    a.close(), b.close()


def test_refusals_and_life_cycle(td):
    rows, want, happy = tight_world()
    lib = T.lib_of()
    info = np.zeros(4, np.int32)
    assert lib.td_sim_pool_buffer(None, ROOM) == TD_EINVAL and "null handle" in T.err()
    dev = T.device_world(td, rows, 12, CITY, (4, 4), wait=0, loss=50, max_happy=happy - 1)
    for bad in (ROOM - 1, 1, -1):
        assert lib.td_sim_pool_buffer(dev._h, bad) == TD_EINVAL and str(bad) in T.err() and str(ROOM) in T.err(), bad
    with pytest.raises(ValueError):
        T.device_world(td, rows, 12, CITY, (4, 4), pool_buffer=ROOM - 1)
    with pytest.raises(td.TdError):
        dev.set_pool_buffer(ROOM - 1)
    assert dev.pool_buffer == 0
    # a refusal left the world without a buffer: begin is still refused for the count
    assert lib.td_sim_begin(dev._h, 0, info.ctypes.data) == TD_ERANGE and str(happy) in T.err()
    # ... and the tick counts as begun: the setting cannot change under it
    assert lib.td_sim_pool_buffer(dev._h, ROOM) == TD_EINVAL and "still waits for td_sim_apply" in T.err()
    dev.close()
    # on, off, on: each holds from the next begin; the setting survives td_sim_pooling_n and td_sim_pooling
    dev = T.device_world(td, rows, 12, CITY, (4, 4), wait=0, loss=50, max_happy=happy - 1)
    dev.set_pool_buffer(ROOM)
    dev.set_pool_buffer(0)
    assert lib.td_sim_begin(dev._h, 0, info.ctypes.data) == TD_ERANGE
    dev.close()
    dev = T.device_world(td, rows, 12, CITY, (4, 4), wait=0, loss=50, max_happy=happy - 1)
    dev.set_pool_buffer(ROOM)
    dev.set_pool_n(None)                                   # pairs ...
    dev.set_pool_n((4, 4), 0, 50, max_happy=happy - 1)     # ... and back: the buffer is still set
    assert dev.begin(0)[1] == len(rows) and dev.pools_n() == want and dev.m["max_POOL_MEM_size"] == happy
    dev.close()
    # the buffer set before the policy
    dev = td.DeviceSimulator(rows, n_cabs=12, n_stands=CITY["stands"], drop_time=CITY["drop_time"], max_non_lcm=CITY["max_non_lcm"],
                             big_cost=T.BIG, pool_buffer=ROOM)
    dev.set_pool_n((4, 4), 0, 50, max_happy=happy - 1)
    assert dev.begin(0)[1] == len(rows) and dev.pools_n() == want
    dev.close()
