"""The event log of the device worlds (td_sim_log / td_sim_events, td_simb_log / td_simb_events) against the host world
model's records (Simulator(events=True), tests/test_sim_events_cpu.py): every word, in order.

4. trace-driven: the CPU run's decisions through begin / apply, the log drained after every tick;
5. td_sim_step in lockstep with Simulator + HipTickBackend, on the line, on a table and on the committed input;
6. batches: family A (line) and family D (table) through the existing lockstep helpers;
7. the contract of the four calls."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_batch_dist_worlds as sbd
import sim_batch_worlds as sb
import sim_dist_worlds as sd
import sim_event_cases as ec
import sim_worlds as sw

GOLD = os.path.join(HERE, "golden")
pytestmark = pytest.mark.gpu
TD_EINVAL = -1
FILL = 0x5a5a5a5a
CB = 1024      # the workgroup of every compaction pass


def device_world(td, w, rows, **kw):
    return td.DeviceSimulator(rows, n_cabs=w["cabs"], n_stands=w["stands"], drop_time=w["drop_time"], max_non_lcm=w["max_non_lcm"],
                              big_cost=sw.BIG_COST, **kw)


def same(got, want, where):
    got, want = np.asarray(got).reshape(-1, 8), np.asarray(want).reshape(-1, 8)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (where, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def apply_rec(dev, rec):
    """one recorded tick through begin / apply -> the log line (test_gpu_sim_device's rule)"""
    t = rec["t"]
    info = dev.begin(t)
    if rec["n_dem"] == 0:
        assert info == (0, 0, 0, 0), t
        return None
    assert info[:3] == (1, rec["n_dem"], rec["n_sup"]), t
    res = rec["res"]
    if res is None:
        return dev.format_line(t, [1, rec["n_dem"], 0, 0, 0, 0, 0, 0, dev.apply()])
    opt = dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
    lcm = max(info[2], info[3]) > dev.max_non_lcm
    return dev.format_line(t, [1, rec["n_dem"], rec["n_sup"], lcm, len(res["lcm_rows"]), lcm and res["solved"], len(res["kept_dems"]),
                               len(res["kept_cabs"]), opt])


def run_of(name):
    return ec.hand_run() if name == "hand" else ec.event_run(name)


# ---- 4. trace-driven, one world
@pytest.mark.parametrize("name", ["hand"] + list(sw.WORLDS))
def test_trace_driven_records_equal_the_host_world(td, name):
    run = run_of(name)
    if name in sw.WIDE:      # the reach of the case: a staged list (the supply of the pairs stage) at / one past a workgroup
        assert max(rec["n_sup"] for rec in run["ticks"]) == sw.WORLDS[name]["cabs"] in (CB, CB + 1)
        assert any(rec["n_sup"] + rec["n_d2"] > CB and len((rec["res"] or {"lcm_rows": []})["lcm_rows"]) > 0 for rec in run["ticks"])
        assert max(rec["ev"].shape[0] for rec in run["ticks"]) > CB      # and a tick whose scatter crosses a workgroup boundary
    dev = device_world(td, run["world"], run["rows"], events=True)
    for rec in run["ticks"]:
        line = apply_rec(dev, rec)
        same(dev.events(), rec["ev"], (name, rec["t"]))
        assert line == rec["line"] and dev.m == rec["m"], rec["t"]
        got = dev.state()
        assert all(np.array_equal(got[k], v) for k, v in rec["state"].items()), rec["t"]
    assert dev.events_lost == 0 and dev.events().shape == (0, 8)
    dev.close()


def test_hand_made_world_text_from_the_device(td):
    run = ec.hand_run()
    dev = device_world(td, ec.HAND, ec.HAND_ROWS, events=True)
    for rec in run["ticks"]:
        apply_rec(dev, rec)
    assert td.format_events(dev.events()) == ec.HAND_LINES       # (g) several ticks without a drain come back in tick order
    dev.close()


# ---- 5. the step path
def lockstep_step(td, rows, w, ticks, mp=None, dist=None):
    from taxidispatcher_amd import simulator
    if mp is not None:
        sw.patch_constants(mp, w)
    host = simulator.Simulator(rows, simulator.HipTickBackend(dist=dist), n_cabs=w["cabs"], dist=dist, events=True)
    dev = device_world(td, w, rows, events=True, **({} if dist is None else dict(dist=dist)))
    most = 0
    for t in range(ticks):
        n0 = len(host.events)
        a, b = host.tick(t), dev.tick(t)
        assert a == b, t
        want = ec.as_records(host.events[n0:])
        same(dev.events(), want, t)
        most = max(most, want.shape[0])
    assert dev.m == host.m
    dev.close()
    return host, most


@pytest.mark.parametrize("name", ["tiny", "mid65"])
def test_step_in_lockstep_with_the_product_path(td, name, monkeypatch):
    w = sw.WORLDS[name]
    host, _ = lockstep_step(td, sw.gen_demand(**w), w, w["ticks"], monkeypatch)
    assert len(host.events) > 0 and host.m["total_pickup_numb"] > 0


def test_step_on_a_table_world(td, monkeypatch):
    name = "ring12"
    w, D = sd.world(name), sd.table(name)
    host, _ = lockstep_step(td, sd.gen_demand(D, **w), w, w["ticks"], monkeypatch, dist=D)
    ev = ec.as_records(host.events)
    assert all(ec.count(ev, k) > 0 for k in ec.ALL_KINDS)


def test_step_on_the_committed_input_crosses_a_workgroup(td):
    """ticks 0 .. 19 of the committed demand file: 1300 cabs, and ticks that deliver more than 1024 records, so the scatter
    of one tick crosses a workgroup boundary"""
    from taxidispatcher_amd import simulator
    rows = simulator.read_demand(os.path.join(GOLD, "taxi_demand.txt.gz"))
    w = dict(stands=simulator.N_STANDS, cabs=simulator.N_CABS, drop_time=simulator.DROP_TIME, max_non_lcm=simulator.MAX_NON_LCM)
    host, most = lockstep_step(td, rows, w, 20)
    assert most > CB and host.m["total_LCM_used"] > 0


# ---- 6. batches
def batch_lockstep(td, mp, which):
    """the family through its existing lockstep helper, with events switched on in the hosts and in the batch"""
    from taxidispatcher_amd import simulator

    class EventSimulator(simulator.Simulator):
        def __init__(self, *a, **kw):
            kw.setdefault("events", True)
            super().__init__(*a, **kw)
    real_batch = td.DeviceSimulatorBatch
    mp.setattr(simulator, "Simulator", EventSimulator)
    mp.setattr(td, "DeviceSimulatorBatch", lambda *a, **kw: real_batch(*a, events=True, event_capacity=1 << 19, **kw))
    if which == "A":
        city, runs = sb.family("A")
        dev, hosts = sb.lockstep(td, mp, city, [r["rows"] for _, r in runs], [r["world"]["cabs"] for _, r in runs], city["ticks"])
        hosts = [hosts[b] for b in range(len(runs))]
    else:
        city, D, runs = sbd.family("D")
        dev, hosts = sbd.lockstep(td, mp, city, D, [r["rows"] for _, r in runs], [r["world"]["cabs"] for _, r in runs], city["ticks"])
    return city, runs, dev, hosts


@pytest.mark.parametrize("which", ["A", "D"])
def test_batch_records_equal_each_host_world(td, monkeypatch, which):
    city, runs, dev, hosts = batch_lockstep(td, monkeypatch, which)
    B = len(runs)
    ev = dev.events()                # every tick of the run in one drain
    assert dev.events_lost == 0 and ev.shape[0] > 0
    # ticks in the order they ran, within a tick the worlds ascending
    key = ev[:, 0].astype(np.int64) * B + ev[:, 1]
    assert (np.diff(key) >= 0).all() and ev[:, 0].max() == city["ticks"] - 1
    quiet = 0
    for b, host in enumerate(hosts):
        want = ec.as_records(host.events)
        got = ev[ev[:, 1] == b].copy()
        got[:, 1] = 0
        same(got, want, (which, b))
        assert td.format_events(ev, world=b) == td.format_events(want)
        # a world without demand in a tick contributes its arrivals, its drops and record 4 only
        for t in range(city["ticks"]):
            mine = want[want[:, 0] == t]
            hdr = mine[mine[:, 2] == ec.TEMP_DEMAND]
            assert hdr.shape[0] == 1
            if hdr[0, 6] == 0:
                quiet += 1
                assert set(mine[:, 2].tolist()) <= {ec.PICKED_UP, ec.CAB_FREE, ec.DROPPED, ec.TEMP_DEMAND}, (b, t)
    assert quiet > city["ticks"]      # the world without requests, and ticks without demand in the others
    assert ec.as_records(hosts[-1].events).shape[0] == city["ticks"]          # the empty request table: record 4 alone, every tick
    assert any(h.m["total_LCM_used"] > 0 for h in hosts) and any(h.m["total_dropped"] > 0 for h in hosts)
    dev.close()


def test_batch_drained_between_begin_and_apply(td):
    """trace-driven family A: a drain after begin delivers begin's records of every world, the drain after apply the rest,
    world by world; together they are each host world's records of the tick"""
    city, runs = sb.family("A")
    hosts = [ec.event_run("simbA_" + name, rows=r["rows"], world=r["world"]) for name, r in runs[:-1]]
    dev = td.DeviceSimulatorBatch([r["rows"] for _, r in runs[:-1]], [r["world"]["cabs"] for _, r in runs[:-1]], n_stands=city["stands"],
                                  drop_time=city["drop_time"], max_non_lcm=city["max_non_lcm"], big_cost=sw.BIG_COST, events=True)
    begin_kinds = (ec.PICKED_UP, ec.CAB_FREE, ec.DROPPED, ec.TEMP_DEMAND, ec.TEMP_DEMAND_ID, ec.POOL, ec.POOL_PAIR)
    for t in range(city["ticks"]):
        recs = [h["ticks"][t] for h in hosts]
        info = dev.begin(t)
        first = dev.events()
        second = np.zeros((0, 8), np.int32)
        if info[:, 0].any():
            dev.apply([sb.decisions_of(rec) for rec in recs])
            second = dev.events()
        for b, rec in enumerate(recs):
            want = rec["ev"].copy()
            want[:, 1] = b
            isb = np.isin(want[:, 2], begin_kinds)
            same(first[first[:, 1] == b], want[isb], (t, b, "begin"))
            same(second[second[:, 1] == b], want[~isb], (t, b, "apply"))
    assert dev.m == [h["m"] for h in hosts]
    dev.close()


# ---- 7. contract
def raw(td):
    from taxidispatcher_amd import _ffi
    return _ffi.lib(), _ffi


def drain(lib, h, max_records, out_addr):
    n, lost = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = lib.td_sim_events(h, max_records, out_addr, ctypes.byref(n), ctypes.byref(lost))
    return rc, n.value, lost.value


def hand_ticks(dev, upto):
    run = ec.hand_run()
    for rec in run["ticks"][:upto]:
        apply_rec(dev, rec)
    return np.concatenate([rec["ev"] for rec in run["ticks"][:upto]])


@pytest.mark.parametrize("dest", ["host", "device", "host+4", "device+4"])
def test_full_log_keeps_a_prefix_and_counts_the_rest(td, dest):
    import torch
    lib, _ffi = raw(td)
    cap = 5                                # tick 1 of the hand-made world alone writes 13 records
    dev = device_world(td, ec.HAND, ec.HAND_ROWS, events=True, event_capacity=cap)
    full = hand_ticks(dev, 2)               # ticks 0 and 1: 1 + 13 records; the log ends inside tick 1's tempDemand list
    assert full.shape[0] == 14
    words = 8 * 8 + 2
    if dest.startswith("device"):
        buf = torch.full((words,), FILL, dtype=torch.int32, device="cuda")
    else:
        buf = np.full(words, FILL, np.int32)
    off = 0
    if dest.endswith("+4"):                      # a destination aligned to 4 bytes only
        off = 1 if _ffi.addr(buf) % 8 == 0 else 2
        assert (_ffi.addr(buf) + 4 * off) % 8 == 4
    rc, n, lost = drain(lib, dev._h, 8, _ffi.addr(buf) + 4 * off)
    got = buf.cpu().numpy() if dest.startswith("device") else buf
    assert (rc, n, lost) == (0, cap, full.shape[0] - cap)
    same(got[off:off + 8 * cap], full[:cap], dest)
    assert (got[:off] == FILL).all() and (got[off + 8 * cap:] == FILL).all()       # nothing behind n * 8 words
    assert drain(lib, dev._h, 8, _ffi.addr(buf)) == (0, 0, 0)                     # emptied, and the count of lost records with it
    full2 = hand_ticks_from(dev, 2, 3)       # the log takes records again
    same(dev.events(), full2, "after the drain")
    assert dev.events_lost == 0
    dev.close()


def hand_ticks_from(dev, lo, hi):
    run = ec.hand_run()
    for rec in run["ticks"][lo:hi]:
        apply_rec(dev, rec)
    return np.concatenate([rec["ev"] for rec in run["ticks"][lo:hi]])


def test_max_records_too_small_consumes_nothing(td):
    lib, _ffi = raw(td)
    dev = device_world(td, ec.HAND, ec.HAND_ROWS, events=True)
    full = hand_ticks(dev, 3)
    buf = np.full(8 * full.shape[0], FILL, np.int32)
    rc, n, _ = drain(lib, dev._h, full.shape[0] - 1, buf.ctypes.data)
    assert rc == TD_EINVAL and n == full.shape[0] and (buf == FILL).all()
    with pytest.raises(td.TdError):
        dev.events(max_records=1)
    assert drain(lib, dev._h, -1, buf.ctypes.data)[0] == TD_EINVAL
    same(dev.events(max_records=full.shape[0]), full, "the next call returns everything")
    dev.close()


@pytest.mark.parametrize("kinds", [(ec.TEMP_DEMAND, ec.POOL, ec.ASSIGNED_LCM), (ec.PICKED_UP, ec.CAB_FREE, ec.DROPPED, ec.TEMP_DEMAND_ID, ec.POOL_PAIR,
                                                                               ec.ASSIGNED_PICKED, ec.HEADING, ec.POOLED_SECOND)])
def test_a_kinds_subset_is_the_full_log_filtered(td, kinds):
    run = ec.event_run("tiny")
    dev = device_world(td, run["world"], run["rows"], events=kinds)
    for rec in run["ticks"]:
        apply_rec(dev, rec)
        same(dev.events(), rec["ev"][np.isin(rec["ev"][:, 2], kinds)], rec["t"])
    dev.close()


def test_logging_changes_nothing_in_the_world(td):
    run = ec.event_run("small")
    on, off = device_world(td, run["world"], run["rows"], events=True, event_capacity=16), device_world(td, run["world"], run["rows"])
    for t in range(run["world"]["ticks"]):      # the step path; the log overflows after a few ticks and stays full
        assert on.tick(t) == off.tick(t), t
        assert on.m == off.m, t
        a, b = on.state(), off.state()
        assert all(np.array_equal(a[k], b[k]) for k in a), t
    assert on.events().shape == (16, 8) and on.events_lost > 0 and off.events().shape == (0, 8) and off.events_lost == 0
    on.close()
    off.close()


def test_workspace_bytes_count_the_log(td):
    lib, _ffi = raw(td)

    def ws():
        v = ctypes.c_int64(-1)
        assert lib.td_workspace_bytes(ctypes.byref(v)) == 0
        return v.value
    run = ec.event_run("small")
    base = ws()
    dev = device_world(td, run["world"], run["rows"])
    plain = ws()
    assert lib.td_sim_log(dev._h, 0xffe, 1000) == 0
    assert ws() - plain >= 32 * 1000
    assert lib.td_sim_log(dev._h, 0xffe, 10) == 0              # again with other arguments: the log is replaced
    assert 0 < ws() - plain < 32 * 1000
    assert lib.td_sim_log(dev._h, 0, 0) == 0 and ws() == plain
    assert lib.td_sim_log(dev._h, 2, 10) == 0 and ws() > plain
    dev.close()
    assert ws() == base                                        # destroy frees the log with the handle
    city, runs = sb.family("A")
    batch = sb.device_batch(td, city, runs)
    plain = ws()
    assert lib.td_simb_log(batch._h, 0xffe, 1000) == 0 and ws() - plain >= 32 * 1000
    assert lib.td_simb_log(batch._h, 0, 0) == 0 and ws() == plain
    batch.close()


def test_argument_rules(td):
    lib, _ffi = raw(td)
    dev = device_world(td, ec.HAND, ec.HAND_ROWS)
    city, runs = sb.family("A")
    batch = sb.device_batch(td, city, runs)
    buf = np.full(64, FILL, np.int32)
    n, lost = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for log, events, h in ((lib.td_sim_log, lib.td_sim_events, dev._h), (lib.td_simb_log, lib.td_simb_events, batch._h)):
        assert log(None, 2, 10) == TD_EINVAL
        assert log(h, 1, 10) == TD_EINVAL and log(h, 1 << 12, 10) == TD_EINVAL and log(h, 0x80000002, 10) == TD_EINVAL     # bits outside 1 .. 11
        assert log(h, 2, 0) == TD_EINVAL and log(h, 2, -1) == TD_EINVAL
        assert events(None, 8, buf.ctypes.data, ctypes.byref(n), ctypes.byref(lost)) == TD_EINVAL
        assert events(h, 8, buf.ctypes.data, None, ctypes.byref(lost)) == TD_EINVAL
        # a handle without logging: n = 0, lost = 0, nothing written
        assert events(h, 8, buf.ctypes.data, ctypes.byref(n), ctypes.byref(lost)) == 0 and (n.value, lost.value) == (0, 0)
        assert events(h, 0, None, ctypes.byref(n), None) == 0 and n.value == 0
        assert (buf == FILL).all()
    # a call while a tick with demand waits for its apply
    assert dev.begin(0) == (0, 0, 0, 0) and lib.td_sim_log(dev._h, 0xffe, 64) == 0      # tick 0 has no demand: nothing waits
    assert dev.begin(1)[0] == 1
    assert lib.td_sim_log(dev._h, 0xffe, 64) == TD_EINVAL and lib.td_sim_log(dev._h, 0, 0) == TD_EINVAL
    rec = ec.hand_run()["ticks"][1]
    res = rec["res"]
    dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
    assert lib.td_sim_log(dev._h, 0xffe, 64) == 0
    info = batch.begin(0)
    assert info[:, 0].any() and lib.td_simb_log(batch._h, 0xffe, 64) == TD_EINVAL
    with pytest.raises(ValueError):
        device_world(td, ec.HAND, ec.HAND_ROWS, events=[12])
    dev.close()
    batch.close()
