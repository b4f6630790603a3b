"""td_simb_pool_buffer: the pool rounds of a batch of worlds through td_pool_n_banded_batched's kernel.  Family A's fleets in one
batch under (4, 2), (3, 3), (2, 2) and a pair world equal the same batch without the buffer after every tick; a batch with one
happy plan too many for its max_happy is still refused without the call and runs to its end with it; the call's refusals and
life cycle."""
import numpy as np
import pytest

import sim_batch_worlds as sbw
import test_gpu_sim_pool_buffer as SPB
import test_gpu_simb_pool_n as TB

pytestmark = pytest.mark.gpu

TD_EINVAL, TD_ERANGE = -1, -4
ROOM = 24 * 512
# world order: A1, A7, A40, A90, Aempty
POLICIES = (TB.P42, TB.P33, TB.P22, TB.GREEDY, TB.NONE)


def same_worlds(a, b, policies, where):
    """state, metrics and plans of every world of two batches"""
    assert a.m == b.m, where
    for w, p in enumerate(policies):
        sa, sb_ = a.state(w), b.state(w)
        for key in sa:
            assert np.array_equal(sa[key], sb_[key]), (where, w, key)


@pytest.mark.parametrize("way", ["step", "split"])
def test_a_batch_through_the_buffer_equals_the_batch_without(td, way):
    """both batches dispatch through td_tick_batched, so equal optima are tie-broken alike"""
    city, runs = sbw.family("A")
    plain, banded = TB.batch_of(td, runs, POLICIES), TB.batch_of(td, runs, POLICIES, pool_buffer=ROOM)
    assert plain.pool_buffer == 0 and banded.pool_buffer == ROOM
    sizes = [set() for _ in runs]
    pooled = 0
    for t in range(city["ticks"]):
        if way == "step":
            la, lb = plain.tick(t), banded.tick(t)
        else:
            la, lb = sbw.split_tick(td, plain, city, t), sbw.split_tick(td, banded, city, t)
        assert la == lb, t
        if la is not None:
            for w, p in enumerate(POLICIES[:-1]):
                if la[w] is None:
                    continue
                plans = TB.plans_of(plain, p, w)
                assert TB.plans_of(banded, p, w) == plans, (t, w)
                if p[2] is not None:
                    sizes[w] |= {len(x[0]) for x in plans}
                    pooled += len(plans)
        same_worlds(plain, banded, POLICIES, (way, t))
    assert sizes[0] == {2, 3, 4} and sizes[1] == {3} and sizes[2] == {2} and pooled > 30, (sizes, pooled)
    plain.close(), banded.close()


def tight_batch(td, happy_limit, **kw):
    """the world of test_gpu_sim_pool_buffer.py (40 requests at tick 0, pools of four under wait 0 / loss 50) beside a pair world"""
    rows, want, happy = SPB.tight_world()
    other = rows[:25].copy()
    city = SPB.CITY
    dev = td.DeviceSimulatorBatch([other, rows], [9, 12], n_stands=city["stands"], drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"],
                                  big_cost=TB.BIG, pool_n=[None, (4, 4)], pool_wait=0, pool_loss=50, max_happy=happy_limit(happy), **kw)
    return dev, rows, want, happy


def test_a_batch_past_its_max_happy_runs_with_the_buffer(td):
    lib = TB.lib_of()
    info = np.zeros((2, 4), np.int32)
    tight, rows, want, happy = tight_batch(td, lambda h: h - 1)
    assert lib.td_simb_begin(tight._h, 0, info.ctypes.data) == TD_ERANGE and "world 1" in TB.err() and str(happy) in TB.err()
    tight.close()
    banded, _, _, _ = tight_batch(td, lambda h: h - 1, pool_buffer=ROOM)
    roomy, _, _, _ = tight_batch(td, lambda h: 0)
    assert ROOM < happy      # the first tick's list does not fit one band
    for t in range(SPB.TICKS):
        assert banded.tick(t) == roomy.tick(t), t
        if t == 0:
            assert banded.pools_n(1) == want == roomy.pools_n(1)
            assert banded.pools(0) == roomy.pools(0) and len(roomy.pools(0)) > 0
        same_worlds(banded, roomy, (None, None), t)
    assert banded.m[1]["max_POOL_MEM_size"] == happy      # the true count, not what a band held
    assert banded.m[1]["total_second_passengers"] > 0
    banded.close(), roomy.close()


def test_refusals_and_life_cycle(td):
    lib = TB.lib_of()
    info = np.zeros((2, 4), np.int32)
    assert lib.td_simb_pool_buffer(None, ROOM) == TD_EINVAL and "null handle" in TB.err()
    dev, rows, want, happy = tight_batch(td, lambda h: h - 1)
    for bad in (-1, 1, ROOM - 1, (1 << 22) + 1):
        assert lib.td_simb_pool_buffer(dev._h, bad) == TD_EINVAL and str(bad) in TB.err() and str(ROOM) in TB.err(), bad
    with pytest.raises(ValueError):
        tight_batch(td, lambda h: 0, pool_buffer=ROOM - 1)
    with pytest.raises(td.TdError):
        dev.set_pool_buffer(ROOM - 1)
    assert dev.pool_buffer == 0
    # the refusals left the batch without a buffer: begin is still refused for the count
    assert lib.td_simb_begin(dev._h, 0, info.ctypes.data) == TD_ERANGE and str(happy) in TB.err()
    dev.close()
    # on, then off: 0 holds from the next begin
    dev, _, _, _ = tight_batch(td, lambda h: h - 1, pool_buffer=1 << 22)
    dev.set_pool_buffer(0)
    assert dev.pool_buffer == 0 and lib.td_simb_begin(dev._h, 0, info.ctypes.data) == TD_ERANGE
    dev.close()
    # a call while a tick waits for its apply; then between two ticks; the setting survives td_simb_pooling_n and td_simb_pooling
    dev, _, _, _ = tight_batch(td, lambda h: h - 1, pool_buffer=ROOM)
    twin, _, _, _ = tight_batch(td, lambda h: 0)
    got = dev.begin(0)
    assert np.array_equal(got, twin.begin(0)) and got[1][1] == len(rows) and dev.pools_n(1) == want
    assert lib.td_simb_pool_buffer(dev._h, 0) == TD_EINVAL and "still waits for td_simb_apply" in TB.err()
    assert lib.td_simb_pool_buffer(dev._h, 1 << 22) == TD_EINVAL
    assert dev.pools(0) == twin.pools(0) and len(dev.pools(0)) > 0      # the pair world beside it pooled as it always does
    for d in (dev, twin):
        d.model()
        d.apply([None if not (got[b][0] and got[b][2]) else ((), (), False, np.arange(0)) for b in range(2)])
    dev.set_pool_buffer(65536)
    dev.set_pool_n(None)
    dev.set_pool_n([None, (4, 4)], 0, 50, max_happy=1)      # max_happy is not looked at under the buffer
    twin.set_pool_n([None, (4, 4)], 0, 50)
    assert dev.pool_buffer == 65536
    for t in range(1, SPB.TICKS):
        assert dev.tick(t) == twin.tick(t), t
        same_worlds(dev, twin, (None, None), t)
    dev.close(), twin.close()
