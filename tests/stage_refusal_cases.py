"""The calls of tests/test_gpu_stage_refusals.py and tools/stage_refusals_golden.py.  TEST INFRASTRUCTURE ONLY.

Every entry point that stages ragged offsets (or per-model sizes) is called with batch = 3, n = 4 and positions on a 5-stand
line: once with good inputs and once per bad array, with the bad array in host and in device memory.  run(lib) returns
{case id: record}; a record holds the return code, the whole td_last_error text, for every output window whether it still
holds abi_buffers' pattern, and for a call that succeeded the entries of every output that the header defines.  The guards
of every window are asserted where the call is made.  The fixture tests/golden/stage_refusals_parent.json is run()'s result
at the commit before the staging helpers were gathered in csrc/td_stage.h."""
import ctypes

import numpy as np

import abi_buffers as ab

B, N, S = 3, 4, 5   # the shape of the test (set_shape below)
BIG, THR = 250000, 10
P = ab.ptr
KINDS = (("host", 0), ("device", 0))
BAD_OFFSETS = {"first_not_0": [1, 2, 3, 4], "decreasing": [0, 3, 2, 4], "too_long": [0, 5, 5, 5]}
BAD_NS = {"ns": [4, 5, -1]}
I32, I64 = np.int32, np.int64


def i32(x):
    return np.ascontiguousarray(np.asarray(x, I32))


def _offsets(counts):
    return i32(np.concatenate([[0], np.cumsum(counts)]))


def _inputs():
    rng = np.random.default_rng(20)
    small = (B, N, S) == (3, 4, 5)
    n_cab = [4, 2, 3] if small else rng.integers(N // 2, N + 1, B)
    n_dem = [3, 4, 1] if small else rng.integers(N // 2, N + 1, B)
    T = int(np.sum(n_cab))   # cabs, customers and requests of all models
    a = {"cab_off": _offsets(n_cab), "dem_off": _offsets(n_dem), "cab_to": i32(rng.integers(0, S, T)), "dem_from": i32(rng.integers(0, S, T if small else int(np.sum(n_dem)))),
         "off": _offsets(n_cab), "from": i32(rng.integers(0, S, T)), "max_wait": i32(rng.integers(0, 6, T)), "max_loss": i32(rng.choice([30, 60, 90], T)),
         "table": i32(np.abs(np.arange(S)[:, None] - np.arange(S)[None, :])), "ns": i32([4, 3, 0] if small else n_cab),
         "cost": i32(rng.integers(1, 40, (B, N, N))), "mode": i32(np.resize([0, 3, 1], B)), "stop": i32(np.full(B, 2)), "parts": i32(np.full(B, 2)),
         "ml_v": np.ascontiguousarray(np.resize([0.0, 50.0, 0.0], B)), "opt_v": i32(np.resize([1, 0, 1], B)),
         "n_cabs": i32(n_cab), "req_off": _offsets(n_cab), "req_id": i32(np.arange(T) + 100), "req_at": i32(np.zeros(T)),
         "zeros4": i32(np.zeros(B + 1)), "zeros3": i32(np.zeros(B)), "dec": i32(np.zeros(16))}
    a["to"] = i32((a["from"] + 1 + rng.integers(0, S - 1, T)) % S)
    w = rng.integers(1, 40, (B, N, N))
    a["weight"] = i32(w + w.transpose(0, 2, 1))
    return a


IN = TICK_OUT = POOL2_OUT = CALLS = EXTRA_IN = None   # set_shape() makes them


def _outputs():
    global TICK_OUT, POOL2_OUT
    TICK_OUT = {"rows": ((B, N), I32), "cols": ((B, N), I32), "k": ((B,), I32), "lm": ((B,), I32), "kc": ((B, N), I32), "kd": ((B, N), I32),
                "n2": ((B,), I32), "r2c": ((B, N), I32), "tot": ((B,), I64), "dual": ((B,), I64)}
    POOL2_OUT = {"a": ((B, N // 2), I32), "b": ((B, N // 2), I32), "plan": ((B, N // 2), I32), "pcost": ((B, N // 2), I32), "k": ((B,), I32),
                 "tot": ((B,), I64)}


def _rows(o, names, count):
    """the first count[b] entries of row b of every array in names"""
    return {q: [o[q][b, :int(count[b])].tolist() for b in range(B)] for q in names}


def _tick_defined(o):
    d = {q: o[q].tolist() for q in ("k", "lm", "n2", "tot", "dual")}
    d.update(_rows(o, ("rows", "cols"), o["k"]))
    d.update(_rows(o, ("r2c",), o["n2"]))
    ns, nd = np.diff(IN["cab_off"]), np.diff(IN["dem_off"])
    d.update(_rows(o, ("kc",), ns - o["k"]))
    d.update(_rows(o, ("kd",), nd - o["k"]))
    return d


def _pool2_defined(o):
    d = {q: o[q].tolist() for q in ("k", "tot")}
    d.update(_rows(o, ("a", "b", "plan", "pcost"), o["k"]))
    return d


def _pooln_defined(o):
    d = {q: o[q].tolist() for q in ("k", "nh", "tot")}
    d.update(_rows(o, ("pools",), o["k"] * 5))
    return d


def _all(o):
    return {q: v.tolist() for q, v in o.items()}


def _pos(A):
    return A["cab_off"], A["cab_to"], A["dem_off"], A["dem_from"]


# name -> (input names, output shapes, call(lib, A, O, x) with addresses A / O and scalars x, defined entries, offset arrays, extra cases)
def _calls():
    return {
        "td_build_assign_batched": (
            ("cab_off", "cab_to", "dem_off", "dem_from"), {"r2c": ((B, N), I32), "tot": ((B,), I64), "dual": ((B,), I64)},
            lambda lib, A, O, x: lib.td_build_assign_batched(x["batch"], N, *_pos(A), None, 0, BIG, THR, O["r2c"], O["tot"], O["dual"]),
            _all, ("cab_off", "dem_off"), {}),
        "td_tick_batched": (
            ("cab_off", "cab_to", "dem_off", "dem_from"), TICK_OUT,
            lambda lib, A, O, x: lib.td_tick_batched(x["batch"], N, *_pos(A), None, 0, BIG, THR, 2, *(O[q] for q in TICK_OUT)),
            _tick_defined, ("cab_off", "dem_off"), {}),
        "td_split_batched": (
            ("cab_off", "cab_to", "dem_off", "dem_from", "table"),
            {"req": ((len(IN["cab_to"]),), I32), "stage": ((len(IN["cab_to"]),), I32), "tot": ((B,), I64), "rest": ((B,), I64), "n_rest": ((2 * B,), I32), "gap": ((B,), I64)},
            lambda lib, A, O, x: lib.td_split_batched(x["batch"], N, *_pos(A), A["table"] if x.get("table") else None, S if x.get("table") else 0, S,
                                                      x.get("parts", 2), x.get("fill", BIG), *(O[q] for q in ("req", "stage", "tot", "rest", "n_rest", "gap"))),
            _all, ("cab_off", "dem_off"), {"two_rules": {"table": 1, "parts": 0, "fill": 0}}),
        "td_dispatch_batched": (
            ("cab_off", "cab_to", "dem_off", "dem_from", "table", "mode", "stop", "parts", "parts0", "mode3"), TICK_OUT,
            lambda lib, A, O, x: lib.td_dispatch_batched(x["batch"], N, *_pos(A), A["table"] if x.get("table") else None, S if x.get("table") else 0,
                                                         x.get("fill", BIG), THR, S, A[x.get("mode", "mode")], A["stop"], A[x.get("parts", "parts")],
                                                         *(O[q] for q in TICK_OUT)),
            _tick_defined, ("cab_off", "dem_off"), {"two_rules": {"table": 1, "mode": "mode3", "parts": "parts0", "fill": 0}}),
        "td_pool2_batched": (
            ("off", "from", "to"), POOL2_OUT,
            lambda lib, A, O, x: lib.td_pool2_batched(x["batch"], N, A["off"], A["from"], A["to"], None, 0, 0.0, 1, *(O[q] for q in POOL2_OUT)),
            _pool2_defined, ("off",), {}),
        "td_pool2_batched_v": (
            ("off", "from", "to", "ml_v", "opt_v"), POOL2_OUT,
            lambda lib, A, O, x: lib.td_pool2_batched_v(x["batch"], N, A["off"], A["from"], A["to"], None, 0, A["ml_v"], A["opt_v"], *(O[q] for q in POOL2_OUT)),
            _pool2_defined, ("off",), {}),
        "td_pool_n_batched": (
            ("off", "from", "to", "max_wait", "max_loss"), {"pools": ((B, (N // 2) * 5), I32), "k": ((B,), I32), "nh": ((B,), I64), "tot": ((B,), I64)},
            lambda lib, A, O, x: lib.td_pool_n_batched(2, x["batch"], N, A["off"], A["from"], A["to"], A["max_wait"], A["max_loss"], None, 0, None, 0,
                                                       O["pools"], O["k"], O["nh"], O["tot"]),
            _pooln_defined, ("off",), {}),
        "td_assign_batched": (
            ("ns", "cost"), {"r2c": ((B, N), I32), "tot": ((B,), I64), "dual": ((B,), I64), "price": ((B, N), I64)},
            lambda lib, A, O, x: lib.td_assign_batched(x["batch"], N, A["ns"], A["cost"], O["r2c"], O["tot"], O["dual"], O["price"]),
            _all, ("ns",), {}),
        "td_lcm_batched": (
            ("ns", "cost"), {"rows": ((B, N), I32), "cols": ((B, N), I32), "k": ((B,), I32), "tot": ((B,), I64), "lm": ((B,), I32)},
            lambda lib, A, O, x: lib.td_lcm_batched(x["batch"], N, A["ns"], A["cost"], 100, -1, 0, 0, -1, 2**62, *(O[q] for q in ("rows", "cols", "k", "tot", "lm"))),
            lambda o: dict({q: o[q].tolist() for q in ("k", "tot", "lm")}, **_rows(o, ("rows", "cols"), o["k"])), ("ns",), {}),
        "td_match_batched": (
            ("ns", "weight"), {"mate": ((B, N), I32), "tot": ((B,), I64), "dual": ((B,), I64), "dv": ((B, N), I64), "bp": ((B, 2 * N), I32), "db": ((B, N), I64)},
            lambda lib, A, O, x: lib.td_match_batched(x["batch"], N, A["ns"], A["weight"], *(O[q] for q in ("mate", "tot", "dual", "dv", "bp", "db"))),
            lambda o: {q: o[q].tolist() for q in ("mate", "tot", "dual")}, ("ns",), {}),
    }


def set_shape(b, n, s):
    """the test's shape is (3, 4, 5); tools/stage_calls.py also makes the good calls at a workload shape, where the models have
    random sizes in [n / 2, n]"""
    global B, N, S, IN, CALLS, EXTRA_IN
    B, N, S = b, n, s
    IN = _inputs()
    _outputs()
    CALLS = _calls()
    EXTRA_IN = {"parts0": i32(np.zeros(B)), "mode3": i32(np.full(B, 3))}


set_shape(3, 4, 5)


def last_error(lib):
    e = lib.td_last_error()
    return e.decode() if isinstance(e, bytes) else str(e)


def _record(lib, rc, outs):
    pat = {q: bool((ab.host(v).view(np.uint8) == ab.PATTERN).all()) for q, (v, _) in outs.items()}
    for _, chk in outs.values():
        chk()
    return {"rc": int(rc), "error": last_error(lib) if rc else "", "untouched": pat}


def _one(lib, name, kind, override, scalars):
    names, shapes, call, defined, _, _ = CALLS[name]
    arrays = {q: dict(IN, **EXTRA_IN)[q] for q in names}
    arrays.update(override)
    placed = {q: ab.place(v, *kind) if q in override else v for q, v in arrays.items()}   # alive until the call has returned
    outs = {q: ab.guarded(shape, dt, *kind) for q, (shape, dt) in shapes.items()}
    x = dict({"batch": B}, **scalars)
    rc = call(lib, {q: P(v) for q, v in placed.items()}, {q: P(v) for q, (v, _) in outs.items()}, x)
    rec = _record(lib, rc, outs)
    if rc == 0:
        rec["outputs"] = defined({q: ab.host(v) for q, (v, _) in outs.items()})
    return rec


def _simb_create(lib, dist, kind, req_off):
    """-> (rc, handle); req_off in `kind` memory"""
    h = ctypes.c_void_p()
    off = ab.place(req_off, *kind)
    args = [B, P(IN["n_cabs"]), S, 2, 100, BIG, P(off), P(IN["req_id"]), P(IN["from"]), P(IN["to"]), P(IN["req_at"])]
    rc = lib.td_simb_create_dist(*args, P(IN["table"]), ctypes.byref(h)) if dist else lib.td_simb_create(*args, ctypes.byref(h))
    return rc, h


def _simb_create_case(lib, dist, kind, req_off, steps):
    rc, h = _simb_create(lib, dist, kind, req_off)
    rec = {"rc": int(rc), "error": last_error(lib) if rc else "", "untouched": {}}
    if rc == 0 and steps:   # the whole layout at work: a few ticks of every world
        lines = []
        for t in range(steps):
            line = np.zeros(9 * B, I32)
            assert lib.td_simb_step(h, t, P(line)) == 0, last_error(lib)
            lines.append(line.tolist())
        rec["outputs"] = {"lines": lines}
    if rc == 0:
        assert lib.td_simb_destroy(h) == 0
    return rec


def _simb_apply_case(lib, kind, override):
    rc, h = _simb_create(lib, False, ("host", 0), IN["req_off"])
    assert rc == 0, last_error(lib)
    info = np.zeros(4 * B, I32)
    assert lib.td_simb_begin(h, 0, P(info)) == 0, last_error(lib)
    arrays = {"pair_off": IN["zeros4"], "r2c_off": IN["zeros4"]}
    arrays.update(override)
    placed = {q: ab.place(v, *kind) if q in override else v for q, v in arrays.items()}
    opt, chk = ab.guarded((B,), I32, "host")   # opt_count is a host array
    rc = lib.td_simb_apply(h, P(placed["pair_off"]), P(IN["dec"]), P(IN["dec"]), P(IN["zeros3"]), P(placed["r2c_off"]), P(IN["dec"]), P(opt))
    rec = _record(lib, rc, {"opt_count": (opt, chk)})
    if rc == 0:
        rec["outputs"] = {"info": info.tolist(), "opt_count": opt.tolist()}
    assert lib.td_simb_destroy(h) == 0
    return rec


def case_ids():
    ids = []
    for name, (_, _, _, _, offs, extra) in CALLS.items():
        ids += ["%s/good/%s" % (name, k[0]) for k in KINDS] + ["%s/batch0" % name]
        bad = BAD_NS if offs == ("ns",) else BAD_OFFSETS
        ids += ["%s/%s/%s/%s" % (name, q, b, k[0]) for q in offs for b in bad for k in KINDS]
        ids += ["%s/%s" % (name, e) for e in extra]
    for name in ("td_simb_create", "td_simb_create_dist"):
        ids += ["%s/good/%s" % (name, k[0]) for k in KINDS] + ["%s/req_off/%s/%s" % (name, b, k[0]) for b in BAD_OFFSETS for k in KINDS]
    ids += ["td_simb_apply/good/%s" % k[0] for k in KINDS]
    ids += ["td_simb_apply/%s/%s/%s" % (q, b, k[0]) for q in ("pair_off", "r2c_off") for b in BAD_OFFSETS for k in KINDS]
    return ids


def run_case(lib, cid):
    part = cid.split("/")
    name = part[0]
    kind = (part[-1], 0) if part[-1] in ("host", "device") else ("host", 0)
    if name in ("td_simb_create", "td_simb_create_dist"):
        good = part[1] == "good"
        return _simb_create_case(lib, name.endswith("dist"), kind, IN["req_off"] if good else i32(BAD_OFFSETS[part[2]]), 6 if good else 0)
    if name == "td_simb_apply":
        return _simb_apply_case(lib, kind, {} if part[1] == "good" else {part[1]: i32(BAD_OFFSETS[part[2]])})
    if part[1] == "good":
        return _one(lib, name, kind, {}, {})
    if part[1] == "batch0":   # no model: null arrays are fine
        names, shapes, call, _, _, _ = CALLS[name]
        rc = call(lib, {q: None for q in names}, {q: None for q in shapes}, {"batch": 0})
        return {"rc": int(rc), "error": last_error(lib) if rc else "", "untouched": {}}
    if len(part) == 2:
        return _one(lib, name, kind, {}, CALLS[name][5][part[1]])
    bad = BAD_NS if part[1] == "ns" else BAD_OFFSETS
    return _one(lib, name, kind, {part[1]: i32(bad[part[2]])}, {})


def run(lib):
    return {cid: run_case(lib, cid) for cid in case_ids()}
