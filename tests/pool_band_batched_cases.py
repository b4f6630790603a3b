"""What tests/test_gpu_pool_band_batched.py and tests/test_pool_band_batched_cpu.py share: the part of the td_pool_n_banded
corpus (pool_band_cases.py) that td_pool_n_banded_batched can take, the small model that rides between two copies of a case,
and the mixed batch in which a workgroup takes a second model.  Plain numpy data: nothing here needs a GPU."""
import functools

import numpy as np

import pool_band_cases as C
import pool_band_model as M

NMAX = 512                                # the largest model of the batched calls
CORPUS_COUNTS = {2: 22, 3: 23, 4: 20}     # the cases of all_cases() with at most 512 requests and max_pools None, by k


@functools.lru_cache(maxsize=None)
def corpus():
    """-> k -> list of BandCase: every case of pool_band_cases.all_cases() with at most 512 requests and no max_pools (the
    batched call keeps n_b // k pools, never fewer).  Generators repeat a case under two names; both stay, as the counts say."""
    out = {k: [] for k in C.KS}
    for cases in C.all_cases().values():
        for bc in cases:
            if int(bc.case.frm.size) <= NMAX and bc.max_pools is None:
                out[bc.case.k].append(bc)
    return out


def filler(k, room):
    """the different small model between the two copies of a case: min(7, room // 24) requests on one stand, every plan happy at
    cost 0 -> (demand rows, its records, its happy count, its stats under `room`)"""
    d = M.same_stand(min(7, room // 24), stand=0)
    cost, p, qi = M.happy_plans(k, d)
    recs, nh, stats = M.banded(k, len(d), cost, p, qi, room)
    return d, recs, nh, stats


def answer(k, d, dist, room, first=None):
    """the host model's (records, happy count, stats) of one demand under `room`"""
    if len(d) == 0:
        return [], 0, (0, 0, 0, 0)
    f0, f1 = (0, len(d)) if first is None else first
    cost, p, qi = M.happy_plans(k, d, dist, f0, f1)
    if len(d) < k or min(f1, len(d)) <= max(f0, 0):
        return [], 0, (0, 0, 0, 0)
    return M.banded(k, len(d), cost, p, qi, room)


SECOND_B = 70
SECOND_ROOM = 1 << 22      # 32 workgroups in flight: every workgroup takes a second and a third model


# the models that leave one band under 2^22 keys.  Pools of two have at most 512 * 511 * 2 plans, so they never do: their
# batch of 70 holds the other kinds, and small_room_batch() below gives a workgroup a second model behind a multi-band one.
# "bands": c plain and c dear members on one stand (pool_band_cases.cluster): P(c, k) k! plans at cost 0, which fit, and more
#          than 2^22 with those at cost 1, so the first band is cost 0 alone and the second starts from a bitmap that is not empty
#          (k = 4, c = 16: 1 048 320 + 5 013 120; k = 3, c = 64: 1 499 904 + 4 596 480)
# "deep":  one stand, every plan at cost 0 and more than 2^22 of them: cut at the first pick-up
#          (k = 4: 22 requests, 4 213 440 plans; k = 3: 90 requests, 4 229 280)
SECOND_BIG = {4: dict(bands=16, deep=22), 3: dict(bands=64, deep=90)}


@functools.lru_cache(maxsize=None)
def second_model_batch(k):
    """-> (demands, firsts, kinds): 70 models of six kinds in turn -- empty, fewer than k requests, an empty slice, one band,
    several bands, a deep cut -- so that each of the 32 workgroups meets other kinds behind the model it finished"""
    rng = np.random.default_rng(170 + k)
    ds, firsts, kinds = [], [], []
    for b in range(SECOND_B):
        kind = ("empty", "below_k", "empty_slice", "one_band", "bands", "deep")[b % 6]
        first = None
        if kind == "empty":
            d = np.zeros((0, 5), np.int64)
        elif kind == "below_k":
            d = M.random_demand(rng, k - 1, 9, [90], 6)
        elif kind == "empty_slice":
            d, first = M.random_demand(rng, 20, 9, [90], 6), (7, 7)
        elif kind == "one_band" or k == 2:
            d = M.random_demand(rng, 24 + b % 5, 9, [90], 6)
            first = (3, 20) if kind == "bands" else None
        elif kind == "bands":
            c = SECOND_BIG[k]["bands"]
            d = C.rows(C.cluster(2 * c + 2, range(2 * c), k, dear=range(c, 2 * c)))
        else:
            d = M.same_stand(SECOND_BIG[k]["deep"])
        ds.append(d), firsts.append(first), kinds.append(kind)
    return ds, firsts, kinds


SMALL_B = 1030      # six models more than workgroups in flight at a small room
SMALL_ROOM = {2: 336, 3: 659, 4: 2159}      # CUT_TABLE's rooms: the same-stand model below is cut deep and leaves several bands


@functools.lru_cache(maxsize=None)
def small_room_batch(k):
    """-> (demands, firsts, expected per model as (records, happy, stats)): 1030 models of at most 14 requests under
    SMALL_ROOM[k], four distinct ones in turn, so the workgroups 0 .. 5 take a second model: behind the same-stand model of
    pool_band_cases.CUT_TABLE (several bands, the deepest cut of its k) comes a random one, an empty one, and the same again"""
    rng = np.random.default_rng(270 + k)
    room = SMALL_ROOM[k]
    distinct = [(M.same_stand(14 if k == 2 else 12), None), (M.random_demand(rng, 13, 9, [90], 4), None), (np.zeros((0, 5), np.int64), None),
                (M.random_demand(rng, 14, 9, [90], 3), (2, 9))]
    exp = [answer(k, d, None, room, f) for d, f in distinct]
    assert exp[0][2] == C.CUT_TABLE[(14 if k == 2 else 12, k, room)]
    order = [(b + (b >= 1024)) % 4 for b in range(SMALL_B)]      # a workgroup's second model is the kind behind its first
    return [distinct[i][0] for i in order], [distinct[i][1] for i in order], [exp[i] for i in order]
