"""Pools of up to four in the simulator worlds (Simulator(pool_n=, pool_wait=, pool_loss=), td_sim_pooling_n): the oracle
backend whose find_pool_n is oracle.pool_n, the cascade restated on oracle.pool_n, and the recorded specification run that the
CPU tests check for coverage and invariants and the GPU tests compare a device world with, tick by tick."""
import copy

import numpy as np
import pytest

import sim_backend
import sim_worlds as sw
from oracle import oracle

SIZES = ((2, 2), (3, 3), (4, 4), (4, 2), (3, 2))
# one rule for every test on family A (12 stands, trips of up to 3 stands): a pick-up path of at most 1 stand before a member
# boards, a pooled ride at most 50 percent longer than the direct one.  test_sim_pool_n_cpu.py asserts what it reaches; no
# stage of these worlds has more happy plans than td_pool_n_batched's default max_happy (65536).
WAIT, LOSS = 1, 50


WIDE = dict(stands=50, drop_time=10, max_non_lcm=600)


def one_tick_world(n, seed=3):
    """n requests that all arrive at tick 0, a cab at every stand: the first tick's demand list is the table"""
    rng = np.random.default_rng(seed)
    frm = rng.integers(0, WIDE["stands"], n)
    to = (frm + rng.integers(1, 5, n)) % WIDE["stands"]
    return np.stack([np.arange(n), frm, to, np.zeros(n, np.int64), np.zeros(n, np.int64)], axis=1).astype(np.int64)


class PoolNOracleBackend(sim_backend.OracleTickBackend):
    """the oracle's tick, and oracle.pool_n as the pool finder of a stage"""

    def __init__(self, dist=None):
        self.dist = dist

    def find_pool_n(self, k, frm, to, wait, loss):
        return oracle.pool_n(k, frm, to, wait, loss, self.dist)


def cascade(k_hi, k_lo, frm, to, wait, loss, dist=None):
    """the specification's cascade restated: -> ([(pick-ups, drop-offs, cost)] over the tick's list, happy plans of all stages,
    stages whose list was shorter than their k)"""
    frm, to = np.asarray(frm, np.int32), np.asarray(to, np.int32)
    live = list(range(frm.size))
    plans, happy, short = [], 0, 0
    if frm.size < 2:
        return plans, happy, short
    for k in range(k_hi, k_lo - 1, -1):
        if len(live) < k:
            short += 1
            continue
        m = len(live)
        recs, nh = oracle.pool_n(k, frm[live], to[live], np.full(m, wait, np.int32), np.full(m, loss, np.int32), dist)
        happy += nh
        gone = set()
        for r in recs.tolist():
            plans.append((tuple(live[i] for i in r[:k]), tuple(live[i] for i in r[k:2 * k]), r[2 * k]))
            gone.update(r[:k])
        live = [d for j, d in enumerate(live) if j not in gone]
    return plans, happy, short


def spec_run(rows, cabs, city, ticks, pool_n, wait=WAIT, loss=LOSS, backend=None, dist=None, events=False, **kw):
    """Simulator(pool_n=...) on `backend` (default: PoolNOracleBackend) with the city's constants patched in, recorded per tick:
    t, line, state, m, dem (from / to of the demand before pooling), plans, after (ids of the demand after pooling), others,
    lcm_pools / opt_pools (pools dispatched on either path), lost_pools (pools whose first pick-up found no cab), n_sup"""
    from taxidispatcher_amd import simulator
    with pytest.MonkeyPatch.context() as mp:
        sw.patch_constants(mp, city)
        be = PoolNOracleBackend(dist) if backend is None else backend
        sim = simulator.Simulator(rows, be, n_cabs=cabs, pool_n=pool_n, pool_wait=wait, pool_loss=loss, dist=dist, events=events, **kw)
        cur = {}
        real_find, real_pooled, real_pairs, real_sol, real_sup = sim.find_pool_n, sim._pooled, sim.analyze_pairs, sim.analyze_solution, sim.create_temp_supply

        def find(temp_demand, t=None):
            out = real_find(temp_demand, t)
            cur.update(dem=([r[1] for r in temp_demand], [r[2] for r in temp_demand]), ids=[r[0] for r in temp_demand], plans=list(out))
            return out

        def pooled(temp_demand, t):
            out = real_pooled(temp_demand, t)
            cur.update(after=[list(c) for c in out], others=dict(sim._others))
            return out

        def moved(call, key):
            def wrapped(t, dec, cost_or_dem, *rest):
                temp_demand = rest[0] if key == "opt_pools" else cost_or_dem
                firsts = [c for c in temp_demand if c[3] > -1]
                before = {c[0]: int(sim.d_cab[sim.id2idx[c[0]]]) for c in firsts}
                out = call(t, dec, cost_or_dem, *rest)
                took = [c for c in firsts if before[c[0]] == -1 and sim.d_cab[sim.id2idx[c[0]]] > -1]
                cur[key] = cur.get(key, 0) + len(took)
                cur["seconds"] = cur.get("seconds", 0) + sum(c[4] - 1 for c in took)
                return out
            return wrapped

        def supply():
            out = real_sup()
            cur["n_sup"] = len(out)
            return out
        sim.find_pool_n, sim._pooled, sim.create_temp_supply = find, pooled, supply
        sim.analyze_pairs, sim.analyze_solution = moved(real_pairs, "lcm_pools"), moved(real_sol, "opt_pools")
        recs = []
        for t in range(ticks):
            cur.clear()
            second0 = sim.m["total_second_passengers"]
            line = sim.tick(t)
            if line is not None:
                sim.log.append(line)
            plans = cur.get("plans", [])
            rec = dict(t=t, line=line, state=sw.state_of(sim), m=copy.deepcopy(sim.m), dem=cur.get("dem"), ids=cur.get("ids"), plans=plans,
                       after=cur.get("after"), others=cur.get("others", {}), lcm_pools=cur.get("lcm_pools", 0), opt_pools=cur.get("opt_pools", 0),
                       n_sup=cur.get("n_sup", 0), seconds=cur.get("seconds", 0), second_delta=sim.m["total_second_passengers"] - second0)
            rec["lost_pools"] = len(plans) - rec["lcm_pools"] - rec["opt_pools"]
            recs.append(rec)
        return dict(ticks=recs, log=list(sim.log), m=dict(sim.m), state=sw.state_of(sim), events=list(sim.events), sim=sim)


def check_tick(rec, pool_n, wait=WAIT, loss=LOSS, dist=None):
    """the invariants of one recorded tick, and the plan list against the restated cascade; -> the cascade's (happy, short)"""
    if rec["dem"] is None:      # no demand, or no supply: findPool did not run
        assert rec["plans"] == [] and rec["second_delta"] == 0
        return 0, 0
    frm, to = rec["dem"]
    want, happy, short = cascade(pool_n[0], pool_n[1], frm, to, wait, loss, dist)
    assert rec["plans"] == want, rec["t"]
    members = [d for picks, _, _ in rec["plans"] for d in picks]
    assert len(members) == len(set(members)), ("a request in two pools", rec["t"])
    for picks, drops, cost in rec["plans"]:
        assert pool_n[1] <= len(picks) <= pool_n[0] and sorted(picks) == sorted(drops) and cost >= 0
    # every removed member belongs to a pool whose first pick-up is still in the demand, and carries (second pick-up, size, cost)
    after = {c[0]: c for c in rec["after"]}
    ids = rec["ids"]
    removed = set(ids) - set(after)
    assert removed == {ids[d] for picks, _, _ in rec["plans"] for d in picks[1:]}
    for picks, _, cost in rec["plans"]:
        first = after[ids[picks[0]]]
        assert first[3:] == [ids[picks[1]], len(picks), cost]
        assert rec["others"][first[0]] == tuple(ids[d] for d in picks[1:])
    assert [c[0] for c in rec["after"]] == [i for i in ids if i not in removed]      # list order kept
    assert rec["second_delta"] == rec["seconds"]      # total_second_passengers: size - 1 per dispatched pool
    return happy, short
