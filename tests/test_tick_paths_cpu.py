"""CPU tier of the td_tick path table (tests/tick_path_cases.py): every case's claims hold by the oracle alone, and the
cases named for an edge lie on the side of it their names say.  What td_tick makes of them: test_gpu_tick_paths.py."""
import numpy as np
import pytest

import tick_path_cases as T
from test_gpu_tick_batched import oracle_cost, oracle_tick

I32_MIN = -2**31


def _limit(c):
    _, cab, dem, _, _, _, stop, _ = c
    return max(len(cab), len(dem)) - stop


def _pick_values(c, ref):
    _, cab, dem, dist, fill, thr, _, _ = c
    _, cost = oracle_cost(cab, dem, dist, fill, thr)
    return cost[ref["lcm_rows"], ref["lcm_cols"]], cost[:len(cab), :len(dem)]


def _one_more_pick(c):
    """the oracle's LCM with the size stop one pick later"""
    _, cab, dem, dist, fill, thr, stop, _ = c
    assert stop >= 1
    more = oracle_tick(cab, dem, dist, fill, thr, stop - 1)
    return _pick_values(c, more)[0]


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_claims_hold_by_the_oracle(name):
    c = T.case(name)
    _, cab, dem, dist, fill, thr, stop, claims = c
    ref = T.reference(name)
    n = max(len(cab), len(dem))
    assert 0 <= stop < n                                    # the LCM runs in every case of the table
    assert (T.SOLVED in claims) != (T.NO_SOLVE in claims)   # every case says which
    v, real = _pick_values(c, ref)
    k, limit = len(v), _limit(c)
    for claim in claims:
        if claim == T.INSIDE0:
            assert k == limit and (v == 0).all()
            assert _one_more_pick(c)[-1] == 0               # p0 > limit
        elif claim == T.EXACT0:
            assert k == limit and (v == 0).all()
            if stop >= 1:
                more = _one_more_pick(c)
                assert len(more) == k or more[-1] > 0       # p0 == limit
        elif claim == T.ONE_ABOVE0:
            assert k == limit and (v[:-1] == 0).all() and v[-1] > 0
        elif claim == T.RUNS_OUT:
            assert k < limit and ref["lcm_min_val"] == fill and not ref["solved"]
        elif claim == T.ENDS_MATCHED:
            assert 0 in ref["lcm_rows"] and len(cab) - 1 in ref["lcm_rows"]
        elif claim == T.ENDS_KEPT:
            assert 0 in ref["kept_cabs"] and len(cab) - 1 in ref["kept_cabs"]
        elif claim == T.BOTH_QUEUES:
            up = cab[ref["lcm_rows"]] < dem[ref["lcm_cols"]]
            down = cab[ref["lcm_rows"]] > dem[ref["lcm_cols"]]
            assert (v[up] > 0).any() and (v[down] > 0).any()
        elif claim == T.REAL_GE_FILL:
            _, raw = oracle_cost(cab, dem, dist, I32_MIN, thr)   # a fill no distance equals: what is left is real
            raw = raw[:len(cab), :len(dem)]
            assert (raw[raw != I32_MIN] >= fill).any()
        elif claim in (T.SPAN255, T.SPAN256):
            cand = real[real < fill]
            assert int(cand.max()) - int(cand.min()) == (255 if claim == T.SPAN255 else 256)
        elif claim == T.NEGATIVE:
            assert (real[real < fill] < 0).any()
        elif claim == T.SOLVED:
            assert ref["solved"] and ref["n_rest"] > 0
        elif claim == T.NO_SOLVE:
            assert not ref["solved"]
        else:
            raise AssertionError("unknown claim %r" % (claim,))


def test_cases_lie_on_their_edges():
    shape = lambda name: (len(T.case(name)[1]), len(T.case(name)[2]))
    assert {shape(m) for m in T.CASE_NAMES} >= {(1, 1), (64, 64), (65, 33), (300, 200), (200, 300), (2048, 2048), (2048, 1),
                                                (2049, 100), (100, 2049), (40, 30), (63, 40), (64, 40), (4096, 600), (4097, 600),
                                                (1024, 100), (1025, 100), (2047, 100)}
    eligible = {m for m in T.CASE_NAMES if T.stands_eligible(T.case(m))}
    assert {"s_1x1", "s_64x64", "s_65x33", "s_300x200", "s_200x300", "s_2048x2048", "s_2048x1", "r_cover_thr64", "r_cover_thr1",
            "r_one_stand_50x30", "r_one_stand_30x50", "r_two_queues", "k_ns1024", "k_ns1025", "k_ns2047"} <= eligible
    assert not eligible & {"s_2049x100", "s_100x2049", "r_cab64_thr64", "r_req-1_thr64", "r_cover_thr65", "k_ns2049", "m_n63", "m_n64"}
    for model in ("stands", "small"):
        for fill in T.FILLS:
            assert (("f_%s_fill%d" % (model, fill)) in eligible) == (fill >= 10), (model, fill)
    assert not any(m.startswith(("f_table", "m_")) for m in eligible)
    # positions at the ends of the stands range
    for m in ("s_300x200", "r_cover_thr64", "r_cover_thr65", "r_cover_thr1"):
        _, cab, dem, *_ = T.case(m)
        assert cab.min() == dem.min() == 0 and cab.max() == dem.max() == T.STANDS - 1
    assert T.case("r_cab64_thr64")[1].max() == T.STANDS and T.case("r_req-1_thr64")[2].min() == -1
    # the witness: a stands-eligible case with more cabs than requests, neighbours that are not eligible
    for base, others in T.WITNESS:
        assert base in eligible and shape(base)[0] > shape(base)[1]
        assert not eligible & set(others)
    # the device-memory cases: one of each kind
    assert [T.case(m)[3] is None for m in T.DEVICE_CASES] == [True, False] and T.DEVICE_CASES[0] in eligible
    # td_tick_batched takes most of the table
    assert sum(T.batched_ok(T.case(m)) for m in T.CASE_NAMES) >= len(T.CASE_NAMES) - 12


def test_reference_is_shared_and_read_only():
    a, b = T.reference("s_65x33"), T.reference("s_65x33")
    assert a is b and T.case("s_65x33") is T.case("s_65x33")
    with pytest.raises(ValueError):
        T.case("s_65x33")[1][0] = 1
