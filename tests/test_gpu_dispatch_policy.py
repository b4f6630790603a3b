"""td_dispatch_batched / dispatch_batched on the GPU: a dispatch method per model (the tick, the optimum alone, the LCM alone,
the split heuristic on thresholded cells).  The split and the LCM are checked against tests/sim_dispatch_policy.py's
restatements, the two tick modes against td_tick_batched, the split without a threshold against td_split_batched bit for bit.
And the policy of a device world (td_sim_dispatch, DeviceSimulator(dispatch=...)): td_sim_step, the same tick driven through
begin / model / apply, and the host specification fed the verified decisions agree after every tick; the same for a policy per
world of a batch (td_simb_dispatch, DeviceSimulatorBatch(dispatch=[...]))."""
import numpy as np
import pytest

import sim_dispatch_policy as P

pytestmark = pytest.mark.gpu

FILL = P.FILL
PATTERN32, PATTERN64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
LCM_OPT, OPT, LCM, SPLIT = 0, 1, 2, 3
NAMES = ["lcm_rows", "lcm_cols", "n_pairs", "lcm_min_val", "kept_cabs", "kept_dems", "n_rest", "row_to_col", "total", "dual_bound"]
PER_MODEL = {"lcm_rows", "lcm_cols", "kept_cabs", "kept_dems", "row_to_col"}


def _random_cases(rng, size, count, kmax, kmin=0):
    cabs, dems = [], []
    for _ in range(count):
        ns, nd = (int(x) for x in rng.integers(kmin, kmax + 1, 2))
        cabs.append(rng.integers(0, size, ns).astype(np.int32))
        dems.append(rng.integers(0, size, nd).astype(np.int32))
    return cabs, dems


def _table(rng, S, top):
    """an asymmetric table with entries in 1 .. top - 1 and a zero diagonal"""
    d = rng.integers(1, top, (S, S)).astype(np.int32)
    d[np.arange(S), np.arange(S)] = 0
    return d


def _outs(batch, n, device):
    """the ten outputs pre-filled with a pattern: a refused call must leave it everywhere"""
    outs = {}
    for k in NAMES:
        t = np.int64 if k in ("total", "dual_bound") else np.int32
        outs[k] = np.full((batch, n) if k in PER_MODEL else (batch,), PATTERN64 if t == np.int64 else PATTERN32, t)
    if device:
        import torch
        outs = {k: torch.from_numpy(v).cuda() for k, v in outs.items()}
    return outs


def _i32(v, batch):
    if v is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (batch,)))


def raw_dispatch(td, cabs, dems, dist=None, fill=FILL, thr=-1, size=0, mode=None, stop=None, parts=None, n=None, device=False):
    """the C call on pre-filled outputs -> (rc, outputs as numpy)"""
    lib = td._ffi.lib()
    cv, co, dv, do, batch, nmax = td.pack_ragged(cabs, dems)
    n = nmax if n is None else n
    d = None if dist is None else np.ascontiguousarray(dist, np.int32)
    S = 0 if d is None else int(d.shape[0])
    md, st, pt = _i32(mode, batch), _i32(stop, batch), _i32(parts, batch)
    outs = _outs(batch, n, device)
    A = td._ffi.addr
    rc = lib.td_dispatch_batched(batch, n, A(co), A(cv), A(do), A(dv), A(d), S, fill, thr, size, A(md), A(st), A(pt),
                                 *[A(outs[k]) for k in NAMES])
    return rc, {k: (v.cpu().numpy() if device else v) for k, v in outs.items()}


def raw_tick(td, cabs, dems, dist, fill, thr, stop, n=None):
    lib = td._ffi.lib()
    cv, co, dv, do, batch, nmax = td.pack_ragged(cabs, dems)
    n = nmax if n is None else n
    d = None if dist is None else np.ascontiguousarray(dist, np.int32)
    outs = _outs(batch, n, False)
    A = td._ffi.addr
    rc = lib.td_tick_batched(batch, n, A(co), A(cv), A(do), A(dv), A(d), 0 if d is None else int(d.shape[0]), fill, thr, stop,
                             *[A(outs[k]) for k in NAMES])
    assert rc == 0, td._ffi.load().td_last_error()
    return outs


def ok(td, rc_outs):
    rc, outs = rc_outs
    assert rc == 0, td._ffi.load().td_last_error()
    return outs


def same_model(a, ba, b, bb, ns, nd, what):
    """model ba of result a equals model bb of result b on every output (a list up to its length: a call with host outputs
    does not define what lies beyond)"""
    k = int(a["n_pairs"][ba])
    upto = {"lcm_rows": k, "lcm_cols": k, "kept_cabs": ns - k, "kept_dems": nd - k}
    for key in NAMES:
        x, y = a[key][ba], b[key][bb]
        if key in upto:
            x, y = x[:upto[key]], y[:upto[key]]
        assert np.array_equal(x, y), "%s: %s of model %d / %d: %s != %s" % (what, key, ba, bb, x, y)


def untouched(outs):
    return all((o == (PATTERN64 if o.dtype == np.int64 else PATTERN32)).all() for o in outs.values())


# ---- 1. all split, no threshold: td_split_batched bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["line", "table"])
def test_split_without_threshold_is_split_batched(td, kind):
    rng = np.random.default_rng(20 + len(kind))
    size = 20
    dist = None if kind == "line" else _table(rng, size, 60)
    cabs, dems = _random_cases(rng, size, 20, 10)
    cabs[3], dems[4] = np.zeros(0, np.int32), np.zeros(0, np.int32)
    n = max(max(len(c), len(d)) for c, d in zip(cabs, dems))
    off = np.concatenate([[0], np.cumsum([len(c) for c in cabs])])
    ref = {p: td.split_batched(cabs, dems, size, p, dist) for p in (3, 4, 5)}   # 3: 6 stands, a short fourth range of 2

    def against(res, b, p):
        ns, nd = len(cabs[b]), len(dems[b])
        assert np.array_equal(res["row_to_col"][b, :ns], ref[p]["cab_req"][off[b]:off[b + 1]]), (b, p)
        assert (res["row_to_col"][b, ns:] == -1).all()
        assert res["total"][b] == ref[p]["total"][b] and res["dual_bound"][b] == ref[p]["total"][b] - ref[p]["dual_gap"][b]
        assert res["n_pairs"][b] == 0 and res["lcm_min_val"][b] == FILL and res["n_rest"][b] == max(ns, nd)
        assert res["kept_cabs"][b, :ns].tolist() == list(range(ns)) and res["kept_dems"][b, :nd].tolist() == list(range(nd))

    for p in (4, 3):
        res = ok(td, raw_dispatch(td, cabs, dems, dist, size=size, mode=SPLIT, parts=p))
        for b in range(20):
            against(res, b, p)
    none = ok(td, raw_dispatch(td, cabs, dems, dist, size=size, mode=SPLIT))   # parts == NULL: 4 parts
    for b in range(20):
        against(none, b, 4)
    mixed = [(3, 4, 5)[b % 3] for b in range(20)]
    res = ok(td, raw_dispatch(td, cabs, dems, dist, size=size, mode=SPLIT, parts=mixed))
    for b in range(20):
        against(res, b, mixed[b])
    assert n <= 10


# ---- 2. mode 0 with a stop size per model: td_tick_batched per distinct stop size ----------------------------------------------
@pytest.mark.parametrize("kind,thr", [("line", 6), ("table", 25), ("line", -1)])
def test_tick_mode_with_a_stop_size_per_model(td, kind, thr):
    rng = np.random.default_rng(31 + thr)
    size = 20
    dist = None if kind == "line" else _table(rng, size, 60)
    cabs, dems = _random_cases(rng, size, 24, 9, kmin=1)
    nb = [max(len(c), len(d)) for c, d in zip(cabs, dems)]
    stops = [(-1, 0, 1, nb[b] - 1, nb[b], nb[b] + 1)[b % 6] for b in range(24)]
    n = max(nb) + 1   # a stride above every model
    for mode in (None, LCM_OPT):
        res = ok(td, raw_dispatch(td, cabs, dems, dist, thr=thr, mode=mode, stop=stops, n=n))
        for s in sorted(set(stops)):
            ref = raw_tick(td, cabs, dems, dist, FILL, thr, s, n)
            for b in range(24):
                if stops[b] == s:
                    same_model(res, b, ref, b, len(cabs[b]), len(dems[b]), "stop size %d" % s)
    # TD_DISPATCH_OPT and a NULL stop_size: the stop_size < 0 case
    ref = raw_tick(td, cabs, dems, dist, FILL, thr, -1, n)
    for kw in ({"mode": OPT, "stop": stops}, {"mode": OPT}, {}):
        res = ok(td, raw_dispatch(td, cabs, dems, dist, thr=thr, n=n, **kw))
        for b in range(24):
            same_model(res, b, ref, b, len(cabs[b]), len(dems[b]), "the optimum alone %r" % (kw,))


# ---- 3. the split on thresholded cells --------------------------------------------------------------------------------------
def _check_split(res, cabs, dems, size, parts, dist, thr, which=None):
    cover = []
    for b in (range(len(cabs)) if which is None else which):
        p = parts[b] if isinstance(parts, (list, tuple)) else parts
        cover.append(P.check_split_model(cabs[b], dems[b], size, p, dist, FILL, thr, res["row_to_col"][b], res["total"][b],
                                         res["dual_bound"][b]))
        ns, nd = len(cabs[b]), len(dems[b])
        assert (res["row_to_col"][b, ns:] == -1).all()
        assert res["n_pairs"][b] == 0 and res["lcm_min_val"][b] == FILL and res["n_rest"][b] == max(ns, nd)
        assert res["kept_cabs"][b, :ns].tolist() == list(range(ns)) and res["kept_dems"][b, :nd].tolist() == list(range(nd))
    return cover


@pytest.mark.parametrize("kind", ["line", "table"])
def test_split_on_thresholded_cells(td, kind):
    rng = np.random.default_rng(47 + len(kind))
    size = 20
    dist = None if kind == "line" else _table(rng, size, 30)
    top = size - 1 if dist is None else int(dist.max())
    cabs, dems = _random_cases(rng, size, 30, 10, kmin=1)
    cabs[0], dems[0] = np.array([1, 2, 3], np.int32), np.zeros(0, np.int32)    # an empty side
    cabs[1], dems[1] = np.zeros(0, np.int32), np.array([7], np.int32)
    cabs[2], dems[2] = np.array([2, 2, 11], np.int32), np.array([2, 13, 2, 19], np.int32)   # distance-0 cells
    parts = [(4, 5, 3)[b % 3] for b in range(30)]
    for thr in (0, 1, top, top + 1):
        res = ok(td, raw_dispatch(td, cabs, dems, dist, thr=thr, size=size, mode=SPLIT, parts=parts))
        cover = _check_split(res, cabs, dems, size, parts, dist, thr)
        if thr == 0:   # every cell is refused: nobody is served
            assert (res["row_to_col"] == -1).all() and (res["total"] == 0).all()
        if thr == 1:   # only the cells of distance 0 are left
            assert res["row_to_col"][2, :3].tolist() in ([0, 2, -1], [2, 0, -1]) and res["total"][2] == 0
        if thr == 1:
            assert sum(c["refused_pair"] for c in cover) > 0
        if thr == top + 1:   # no cell is refused: the call without a threshold
            free = ok(td, raw_dispatch(td, cabs, dems, dist, thr=-1, size=size, mode=SPLIT, parts=parts))
            for b in range(30):
                same_model(res, b, free, b, len(cabs[b]), len(dems[b]), "a threshold above every distance")
            assert sum(c["fifth_serves"] for c in cover) > 0 and sum(c["cabs_only"] for c in cover) > 0


# ---- 4. the LCM alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,thr", [("line", 5), ("table", 20), ("line", -1)])
def test_lcm_alone(td, kind, thr):
    rng = np.random.default_rng(59 + thr)
    size = 20
    dist = None if kind == "line" else _table(rng, size, 40)
    cabs, dems = _random_cases(rng, size, 12, 9, kmin=1)
    cabs[0], dems[0] = np.arange(8, dtype=np.int32), np.arange(8, dtype=np.int32)[::-1].copy()   # square
    cabs[1], dems[1] = np.array([4, 4, 9], np.int32), np.array([5, 3, 4, 4, 10, 18], np.int32)   # n_s < n_d
    cabs[2], dems[2] = np.array([5, 3, 4, 4, 10, 18], np.int32), np.array([4, 4, 9], np.int32)   # n_s > n_d
    cabs[3], dems[3] = np.array([0, 1], np.int32), np.array([19, 18, 17], np.int32)              # with thr 5: the first minimum is fill
    cabs[4], dems[4] = np.zeros(0, np.int32), np.array([3], np.int32)                            # no supply
    cabs[5], dems[5] = np.array([3], np.int32), np.zeros(0, np.int32)
    n = max(max(len(c), len(d)) for c, d in zip(cabs, dems))
    # a stop_size entry is not read in this mode
    res = ok(td, raw_dispatch(td, cabs, dems, dist, thr=thr, mode=LCM, stop=[3] * 12))
    for b in range(12):
        P.check_lcm_model(cabs[b], dems[b], dist, FILL, thr, res, b, n)
    if kind == "line" and thr == 5:
        assert res["n_pairs"][3] == 0 and res["lcm_min_val"][3] == FILL
    if kind == "line" and thr == -1:
        assert res["n_pairs"][0] == 8 and res["n_pairs"][1] == 3 and res["n_pairs"][2] == 3   # every row taken / no candidate left
        assert res["lcm_min_val"][1] == FILL and res["lcm_min_val"][0] < FILL


# ---- 5. the four modes in one batch -----------------------------------------------------------------------------------------
def _uniform(td, cabs, dems, dist, thr, size, stop, parts, n):
    return {m: ok(td, raw_dispatch(td, cabs, dems, dist, thr=thr, size=size, mode=m, stop=stop, parts=parts, n=n)) for m in range(4)}


@pytest.mark.parametrize("kind", ["line", "table"])
def test_mixed_batch(td, kind):
    rng = np.random.default_rng(71 + len(kind))
    size = 20
    dist = None if kind == "line" else _table(rng, size, 40)
    thr = 7 if dist is None else 22
    cabs, dems = _random_cases(rng, size, 41, 10)
    modes = [(SPLIT, LCM_OPT, LCM, OPT)[b % 4] for b in range(41)]
    stop = [int(x) for x in rng.integers(0, 6, 41)]
    parts = [(4, 5)[(b // 4) % 2] for b in range(41)]
    n = 12
    uni = _uniform(td, cabs, dems, dist, thr, size, stop, parts, n)
    for device in (False, True):
        res = ok(td, raw_dispatch(td, cabs, dems, dist, thr=thr, size=size, mode=modes, stop=stop, parts=parts, n=n, device=device))
        for b in range(41):
            same_model(res, b, uni[modes[b]], b, len(cabs[b]), len(dems[b]), "mode %d" % modes[b])
    _check_split(uni[SPLIT], cabs, dems, size, parts, dist, thr)
    for b in range(41):
        P.check_lcm_model(cabs[b], dems[b], dist, FILL, thr, uni[LCM], b, n)
        assert uni[OPT]["dual_bound"][b] == uni[OPT]["total"][b] and uni[LCM_OPT]["dual_bound"][b] == uni[LCM_OPT]["total"][b]


def test_mixed_batch_past_the_split_grid(td):
    """2050 models: above the split kernels' grid of 2048 workgroups, so a workgroup takes a second case of another mode"""
    rng = np.random.default_rng(2050)
    size, B, thr, n = 12, 2050, 5, 4
    cabs, dems = _random_cases(rng, size, B, 4)
    modes = [(SPLIT, LCM_OPT, LCM, OPT)[b % 4] for b in range(B)]
    stop = [int(x) for x in rng.integers(0, 4, B)]
    parts = [(4, 3)[(b // 4) % 2] for b in range(B)]
    uni = _uniform(td, cabs, dems, None, thr, size, stop, parts, n)
    res = ok(td, raw_dispatch(td, cabs, dems, None, thr=thr, size=size, mode=modes, stop=stop, parts=parts, n=n))
    for b in range(B):
        same_model(res, b, uni[modes[b]], b, len(cabs[b]), len(dems[b]), "mode %d" % modes[b])
    _check_split(res, cabs, dems, size, parts, None, thr, which=[0, 4, 8, 2044, 2048])


def test_split_at_the_thread_count_boundary(td):
    """one model of 64 and one of 65 per side in one split batch (64 threads up to 64 per side, 256 above), and each alone"""
    rng = np.random.default_rng(6465)
    size, thr = 200, 30
    cabs = [rng.integers(0, size, k).astype(np.int32) for k in (64, 65)]
    dems = [rng.integers(0, size, k).astype(np.int32) for k in (64, 65)]
    res = ok(td, raw_dispatch(td, cabs, dems, None, thr=thr, size=size, mode=SPLIT, parts=4))
    _check_split(res, cabs, dems, size, 4, None, thr)
    for b in range(2):
        one = ok(td, raw_dispatch(td, cabs[b:b + 1], dems[b:b + 1], None, thr=thr, size=size, mode=SPLIT, parts=4))
        _check_split(one, cabs[b:b + 1], dems[b:b + 1], size, 4, None, thr)
        assert one["total"][0] == res["total"][b]


# ---- 6. refusals leave every output unwritten ---------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_refusals_leave_outputs_unwritten(td, device):
    rng = np.random.default_rng(83)
    size = 20
    cabs, dems = _random_cases(rng, size, 8, 9, kmin=2)
    table = _table(rng, size, 60)
    modes = [(SPLIT, LCM_OPT, LCM, OPT)[b % 4] for b in range(8)]
    rc, outs = raw_dispatch(td, cabs, dems, None, thr=6, size=size, mode=modes, stop=2, parts=4, device=device)
    assert rc == 0 and not untouched(outs)

    def refused(cabs=cabs, dems=dems, dist=None, size=size, mode=modes, stop=2, parts=4, fill=FILL, match=None):
        rc, outs = raw_dispatch(td, cabs, dems, dist, fill=fill, thr=6, size=size, mode=mode, stop=stop, parts=parts, device=device)
        assert rc == -1, rc
        assert untouched(outs)
        if match:
            assert match in td._ffi.load().td_last_error().decode()

    refused(mode=[SPLIT, 4] + modes[2:], match="mode[1] = 4")
    refused(mode=[-1] + modes[1:], match="mode[0] = -1")
    big = [np.zeros(1025, np.int32)], [np.zeros(3, np.int32)]
    refused(big[0], big[1], mode=SPLIT, match="1025")                       # a split model of 1025 cabs
    refused(big[1], big[0], mode=SPLIT, match="1025")                       # ... of 1025 requests
    assert raw_dispatch(td, big[0], big[1], None, thr=6, size=size, mode=LCM, device=device)[0] == 0   # the LCM alone takes it
    refused(parts=[4, 4, 4, 4, 0, 4, 4, 4], match="parts[4] = 0")
    refused(parts=[33] + [4] * 7, match="parts[0] = 33")
    assert raw_dispatch(td, cabs, dems, None, thr=6, size=size, mode=modes, stop=2, parts=[4, 0, 33, -5] * 2, device=device)[0] == 0
    refused(size=3, match="size = 3")                                       # size < parts
    refused(big[0], big[0], mode=OPT, match="1025 rows")                    # a remainder above 1024
    refused(big[0], big[0], mode=LCM_OPT, stop=1025, match="1025 rows")
    refused(big[0], big[0], mode=LCM_OPT, stop=None, match="1025 rows")
    assert raw_dispatch(td, big[0], big[0], None, thr=6, size=size, mode=LCM_OPT, stop=1024, device=device)[0] == 0
    # td_split_batched's rules, for a batch with a split model only
    refused(dist=table[:19, :19], match="S = 19")
    refused(fill=19, match="fill")
    assert raw_dispatch(td, cabs, dems, None, fill=19, thr=6, size=size, mode=[m if m != SPLIT else OPT for m in modes], stop=2,
                        device=device)[0] == 0
    at_size = [c.copy() for c in cabs]
    at_size[4][1] = size                                                    # model 4 is a split model: a position at size,
    refused(cabs=at_size, match="position")                                 # found on the device before any output is written
    used = table.copy()
    used[6, 8] = FILL
    refused([np.array([6, 7], np.int32)], [np.array([8], np.int32)], dist=used, mode=SPLIT, match="table entry")
    # td_tick_batched's rules
    lib, A = td._ffi.lib(), td._ffi.addr
    cv, co, dv, do, batch, n = td.pack_ragged(cabs, dems)
    outs = _outs(batch, n - 1, False)
    assert lib.td_dispatch_batched(batch, n - 1, A(co), A(cv), A(do), A(dv), None, 0, FILL, 6, size, None, None, None,
                                   *[A(outs[k]) for k in NAMES]) == -1 and untouched(outs)    # a model above the stride
    outs = _outs(batch, n, False)
    args = [A(outs[k]) for k in NAMES]
    args[7] = None
    assert lib.td_dispatch_batched(batch, n, A(co), A(cv), A(do), A(dv), None, 0, FILL, 6, size, None, None, None, *args) == -1
    assert untouched(outs)                                                  # a null required output
    args = [A(outs[k]) for k in NAMES]
    assert lib.td_dispatch_batched(batch, n, None, A(cv), A(do), A(dv), None, 0, FILL, 6, size, None, None, None, *args) == -1
    assert lib.td_dispatch_batched(batch, n, A(co), None, A(do), A(dv), None, 0, FILL, 6, size, None, None, None, *args) == -1
    assert lib.td_dispatch_batched(batch, n, A(co), A(cv), A(do), None, None, 0, FILL, 6, size, None, None, None, *args) == -1
    assert lib.td_dispatch_batched(-1, n, A(co), A(cv), A(do), A(dv), None, 0, FILL, 6, size, None, None, None, *args) == -1
    assert lib.td_dispatch_batched(batch, 2049, A(co), A(cv), A(do), A(dv), None, 0, FILL, 6, size, None, None, None, *args) == -1
    assert untouched(outs)                                                  # null inputs, a negative batch, a stride above 2048
    args[4] = args[5] = args[9] = None                                      # kept lists and dual_bound may be null
    assert lib.td_dispatch_batched(batch, n, A(co), A(cv), A(do), A(dv), None, 0, FILL, 6, size, A(_i32(modes, batch)), None, None,
                                   *args) == 0
    assert not (outs["row_to_col"] == PATTERN32).any() and (outs["kept_cabs"] == PATTERN32).all()
    assert (outs["dual_bound"] == PATTERN64).all()
    assert lib.td_dispatch_batched(0, 0, None, None, None, None, None, 0, FILL, 6, size, None, None, None, *([None] * 10)) == 0


# ---- the Python call ----------------------------------------------------------------------------------------------------------
def test_dispatch_batched_python(td):
    import torch
    rng = np.random.default_rng(97)
    size = 20
    cabs, dems = _random_cases(rng, size, 10, 8)
    names = ["split", "lcm+opt", "lcm", "opt"]
    modes = [names[b % 4] for b in range(10)]
    res = td.dispatch_batched(cabs, dems, None, drop_time=6, size=size, mode=modes, max_non_lcm=2, parts=5)
    raw = ok(td, raw_dispatch(td, cabs, dems, None, thr=6, size=size, mode=[td.DISPATCH_MODES[m] for m in modes], stop=2, parts=5))
    n = raw["row_to_col"].shape[1]
    for b in range(10):
        ns, nd, k = len(cabs[b]), len(dems[b]), int(raw["n_pairs"][b])
        for key in NAMES:
            if key not in PER_MODEL:
                assert res[key][b] == raw[key][b], (key, b)
        assert np.array_equal(res["row_to_col"][b], raw["row_to_col"][b]) and res["row_to_col"].shape == (10, n)
        assert np.array_equal(res["lcm_rows"][b, :k], raw["lcm_rows"][b, :k]) and np.array_equal(res["kept_cabs"][b, :ns - k], raw["kept_cabs"][b, :ns - k])
        assert np.array_equal(res["kept_dems"][b, :nd - k], raw["kept_dems"][b, :nd - k])
    dev = td.dispatch_batched(cabs, dems, None, drop_time=6, size=size, mode=torch.tensor([td.DISPATCH_MODES[m] for m in modes], dtype=torch.int32).cuda(),
                              max_non_lcm=torch.full((10,), 2, dtype=torch.int32).cuda(), parts=torch.full((10,), 5, dtype=torch.int32).cuda())
    for key in ("row_to_col", "total", "dual_bound", "n_pairs", "n_rest"):
        assert np.array_equal(dev[key], res[key]), key
    with pytest.raises(td.TdError, match="none of"):
        td.dispatch_batched(cabs, dems, None, size=size, mode="greedy")
    with pytest.raises(td.TdError, match="entries"):
        td.dispatch_batched(cabs, dems, None, size=size, mode=[0, 1])


# ---- 7. the policy of a device world (td_sim_dispatch, DeviceSimulator(dispatch=...)) ----------------------------------------
import sim_batch_worlds as sbw
import sim_worlds as sw

CITY = sbw.CITY_A
# parts 2: ranges of 6 stands, wider than drop_time 4, so a region pair can be refused by the threshold inside a simulation
POLICIES = [("lcm+opt", 16, 4), ("lcm+opt", 0, 4), ("opt", 16, 4), ("lcm", 16, 4), ("split", 16, 4), ("split", 16, 5), ("split", 16, 2)]


def _device(td, run, policy=None, **kw):
    if policy is not None:
        kw.update(dispatch=policy[0], max_non_lcm=policy[1], parts=policy[2])
    else:
        kw.update(max_non_lcm=CITY["max_non_lcm"])
    return td.DeviceSimulator(run["rows"], n_cabs=run["world"]["cabs"], n_stands=CITY["stands"], drop_time=CITY["drop_time"],
                              big_cost=sw.BIG_COST, **kw)


def _decide(td, policy, cab_to, dem_from):
    """the calls td_sim_step makes under the policy, on the model the world hands out -> tick()'s dict, verified against the
    restatements: LCM pairs, the solver's total against the oracle's optimum, the split by check_split_model"""
    from oracle import oracle
    mode, mnl, parts = policy
    fill, thr, n_s, n_d = sw.BIG_COST, CITY["drop_time"], len(cab_to), len(dem_from)
    if mode == "split":
        res = td.dispatch_batched([cab_to], [dem_from], None, big_cost=fill, drop_time=thr, size=CITY["stands"], mode="split", parts=parts)
        cover = P.check_split_model(cab_to, dem_from, CITY["stands"], parts, None, fill, thr, res["row_to_col"][0], res["total"][0],
                                    res["dual_bound"][0])
        return dict(lcm_rows=[], lcm_cols=[], solved=True, row_to_col=res["row_to_col"][0, :max(n_s, n_d)], lcm_min_val=fill, cover=cover)
    stop = {"lcm+opt": mnl, "opt": None, "lcm": 0}[mode]
    res = td.tick(np.asarray(cab_to, np.int32), np.asarray(dem_from, np.int32), None, big_cost=fill, drop_time=thr, max_non_lcm=stop)
    ran = stop is not None and max(n_s, n_d) > stop
    if mode == "lcm":
        rows, cols, lm = P.lcm_to_end(cab_to, dem_from, None, fill, thr)
        assert (res["lcm_rows"].tolist(), res["lcm_cols"].tolist(), res["lcm_min_val"]) == (rows, cols, lm)
        return dict(res, solved=False, row_to_col=[])
    if ran:
        cost = oracle.cost_build(cab_to, dem_from, None, fill, thr)[1]
        _, rows, cols, lm = oracle.lcm(cost, mask=fill, stop_value_on=1, stop_value=fill, stop_size=stop, sum_below=fill, java_scan=1)
        assert (res["lcm_rows"].tolist(), res["lcm_cols"].tolist(), res["lcm_min_val"]) == (rows.tolist(), cols.tolist(), lm)
    else:
        assert len(res["lcm_rows"]) == 0
    if res["solved"]:
        kc, kd = np.asarray(cab_to)[res["kept_cabs"]], np.asarray(dem_from)[res["kept_dems"]]
        assert res["total"] == P.opt_thr(kc, kd, None, fill, thr)
    return res


class ReplayBackend:
    """the host specification's backend: the decisions are the device calls' (set per tick), pooling is the library's"""

    def __init__(self, td):
        from taxidispatcher_amd import simulator
        self.hip, self.dec = simulator.HipBackend(), None

    def calculate_cost(self, cab_to, dem_from):
        return self.hip.calculate_cost(cab_to, dem_from)

    def find_pool(self, frm, to):
        return self.hip.find_pool(frm, to)

    def lcm(self, cost, max_non_lcm=None):
        return list(zip(self.dec["lcm_rows"].tolist(), self.dec["lcm_cols"].tolist())), self.dec["lcm_min_val"]

    def solve(self, cost):
        assert self.dec["solved"]
        return self.dec["row_to_col"]

    def split(self, cab_to, dem_from, parts=4):
        return self.dec["row_to_col"]


@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: "%s-%d-%d" % p)
@pytest.mark.parametrize("name", ["A7", "A40"])
def test_a_world_under_a_policy(td, monkeypatch, name, policy):
    """handle X runs td_sim_step under the policy; handle Y is driven by begin -> model -> the same calls -> apply; the host
    specification is fed Y's (verified) decisions: after every tick the three agree in state, metrics and line; and the event
    log of X is the specification's"""
    from taxidispatcher_amd import simulator
    run = dict(sbw.family("A")[1])[name]
    sw.patch_constants(monkeypatch, CITY)
    mode, mnl, parts = policy
    X, Y = _device(td, run, policy, events=True), _device(td, run, policy)
    be = ReplayBackend(td)
    host = simulator.Simulator(run["rows"], be, n_cabs=run["world"]["cabs"], dispatch=mode, max_non_lcm=mnl, parts=parts, events=True)
    cover, lcm_ticks = [], 0
    for t in range(CITY["ticks"]):
        has, n_dem, n_sup, n_d2 = Y.begin(t)
        y_line = None
        if has:
            ln = [1, n_dem, n_sup, 0, 0, 0, 0, 0, 0]
            if n_sup:
                cab_to, dem_from = Y.model()
                be.dec = dec = _decide(td, policy, cab_to.copy(), dem_from.copy())
                cover.append(dec.get("cover"))
                lcm = mode == "lcm" or (mode == "lcm+opt" and max(n_sup, n_d2) > mnl)
                lcm_ticks += lcm
                k = len(dec["lcm_rows"]) if lcm else 0
                ln[3:8] = [lcm, k, lcm and dec["solved"], n_d2 - k, n_sup - k]
                ln[8] = Y.apply(dec["lcm_rows"], dec["lcm_cols"], dec["solved"], dec["row_to_col"])
            else:
                ln[8] = Y.apply()
            y_line = Y.format_line(t, ln)
        x_line, h_line = X.tick(t), host.tick(t)
        if h_line is not None:
            host.log.append(h_line)
        assert x_line == y_line == h_line, (t, x_line, y_line, h_line)
        assert X.m == Y.m == host.m, t
        want = sw.state_of(host)
        for dev in (X, Y):
            got = dev.state()
            for k, v in want.items():
                assert np.array_equal(got[k], v), (t, k)
    assert td.format_events(X.events()) == td.format_events(host.events)
    m = X.m
    assert m["total_LCM_used"] == lcm_ticks
    if mode == "lcm":
        assert lcm_ticks > 0 and m["max_solver_size"] == 0 and all("OPT" not in line for line in host.log)
    if mode in ("opt", "split"):
        assert lcm_ticks == 0 and m["max_solver_size"] == m["max_model_size"] > 0
    if mode == "split":
        assert sum(c["served"] for c in cover) > 0 and sum(c["fifth_serves"] for c in cover) > 0
    if policy == ("lcm+opt", 0, 4):
        assert lcm_ticks > 0


# ---- 8. the default path -------------------------------------------------------------------------------------------------------
def test_a_world_that_sets_the_default_policy_takes_the_default_course(td):
    run = dict(sbw.family("A")[1])["A40"]
    import ctypes
    plain, same = _device(td, run), _device(td, run)
    lib = td._ffi.lib()
    before, after = ctypes.c_int64(-1), ctypes.c_int64(-2)
    assert lib.td_workspace_bytes(ctypes.byref(before)) == 0
    same.set_dispatch("lcm+opt", CITY["max_non_lcm"], 4)
    assert lib.td_workspace_bytes(ctypes.byref(after)) == 0 and before.value == after.value   # the call allocates nothing
    for t in range(CITY["ticks"]):
        assert plain.tick(t) == same.tick(t), t
        assert plain.m == same.m
        a, b = plain.state(), same.state()
        assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- 9. the contract of td_sim_dispatch ----------------------------------------------------------------------------------------
def test_td_sim_dispatch_contract(td):
    lib = td._ffi.lib()
    run = dict(sbw.family("A")[1])["A40"]
    dev, plain = _device(td, run), _device(td, run)
    err = lambda: td._ffi.load().td_last_error().decode()
    assert lib.td_sim_dispatch(None, 0, 16, 4) == -1 and "null handle" in err()
    for args, word in (((4, 16, 4), "mode = 4"), ((-1, 16, 4), "mode = -1"), ((0, -1, 4), "max_non_lcm = -1"), ((3, 16, 0), "parts = 0"),
                       ((3, 16, 33), "parts = 33"), ((3, 16, 13), "parts = 13")):      # 13 parts over 12 stands
        assert lib.td_sim_dispatch(dev._h, *args) == -1 and word in err(), args
    assert lib.td_sim_dispatch(dev._h, 2, 16, 99) == 0 and lib.td_sim_dispatch(dev._h, 0, 16, 0) == 0   # parts are read for the split only
    # a refused call changed nothing: the world still takes the default course
    for t in range(3):
        assert dev.tick(t) == plain.tick(t)
    t = 3
    while not (dev.begin(t)[0] and dev._info[2] > 0):   # a tick with demand and supply: it waits for its apply
        if dev._info[0]:
            dev.apply()
        t += 1
    assert t < CITY["ticks"] - 2
    assert lib.td_sim_dispatch(dev._h, 1, 16, 4) == -1 and "waits for td_sim_apply" in err()
    cab_to, dem_from = dev.model()
    res = td.tick(cab_to, dem_from, None, big_cost=sw.BIG_COST, drop_time=CITY["drop_time"], max_non_lcm=CITY["max_non_lcm"])
    dev.apply(res["lcm_rows"], res["lcm_cols"], res["solved"], res["row_to_col"])
    dev.set_dispatch("lcm")                                                # between two ticks the policy is taken
    lines = [dev.tick(u) for u in range(t + 1, CITY["ticks"])]
    assert dev.dispatch == "lcm" and any(lines) and all("OPT count" not in line for line in lines if line and "supply=0." not in line)


def test_a_split_world_above_1024_per_side_is_refused_by_the_step(td):
    """1100 cabs and 1100 requests at one stand: the step names the counts, the tick stays begun and is finished by hand"""
    n = 1100
    rows = np.array([(i, 0, 1, 0, 0) for i in range(n)], np.int64)
    dev = td.DeviceSimulator(rows, n_cabs=n, n_stands=1 + 1, drop_time=2, max_non_lcm=16, big_cost=sw.BIG_COST, pool="none", dispatch="split",
                             parts=2)
    with pytest.raises(td.TdError, match="1100 cabs and 1100 requests, more than 1024"):
        dev.tick(0)
    lib = td._ffi.lib()
    assert lib.td_sim_dispatch(dev._h, 1, 16, 4) == -1                      # the tick still waits for its apply
    info = np.zeros(4, np.int32)
    assert lib.td_sim_begin(dev._h, 1, td._ffi.addr(info)) == -1
    dev._info = (1, n, n, n)
    cab_to, dem_from = dev.model()
    assert cab_to.size == n and dem_from.size == n
    served = np.where(cab_to == 0, 1, 0)
    r2c = np.full(n, -1, np.int32)
    at0 = np.nonzero(cab_to == 0)[0]
    r2c[at0] = np.arange(at0.size)                                          # a cab standing at stand 0 takes a request there
    assert dev.apply(row_to_col=r2c) == at0.size == n // 2 and served.sum() == at0.size
    assert dev.m["max_solver_size"] == n and dev.m["total_LCM_used"] == 0


# ---- 7b. a policy per world of a batch (td_simb_dispatch, DeviceSimulatorBatch(dispatch=[...])) -------------------------------
# family A's four fleets and its empty world; between the two lists: the four modes, max_non_lcm 0 and 16, parts 4, 5 and 2
BATCH_POLICIES = {
    "first": [("lcm+opt", 0, 4), ("split", 16, 5), ("lcm", 16, 4), ("opt", 16, 4), ("split", 16, 4)],
    "second": [("split", 16, 4), ("lcm+opt", 16, 4), ("split", 16, 2), ("lcm", 0, 4), ("opt", 16, 4)],
}


def _batch(td, runs, policies=None, **kw):
    if policies is not None:
        kw.update(dispatch=[p[0] for p in policies], max_non_lcm=[p[1] for p in policies], parts=[p[2] for p in policies])
    else:
        kw.update(max_non_lcm=CITY["max_non_lcm"])
    return td.DeviceSimulatorBatch([r["rows"] for _, r in runs], [r["world"]["cabs"] for _, r in runs], n_stands=CITY["stands"],
                                   drop_time=CITY["drop_time"], big_cost=sw.BIG_COST, **kw)


class BatchReplayBackend(ReplayBackend):
    """ReplayBackend whose pooling is the batch's (td_pool2_batched's greedy on one model)"""

    def __init__(self, td):
        ReplayBackend.__init__(self, td)
        self.calls = sbw.BatchedCallsBackend(td, CITY)

    def find_pool(self, frm, to):
        return self.calls.find_pool(frm, to)


def _verify(policy, cab_to, dem_from, dec):
    """one world's decision of a dispatch_batched call against the restatements (as _decide does for td_sim's calls)"""
    from oracle import oracle
    mode, mnl, parts = policy
    fill, thr = sw.BIG_COST, CITY["drop_time"]
    if mode == "split":
        return P.check_split_model(cab_to, dem_from, CITY["stands"], parts, None, fill, thr, dec["row_to_col"], dec["total"], dec["dual_bound"])
    if mode == "lcm":
        rows, cols, lm = P.lcm_to_end(cab_to, dem_from, None, fill, thr)
        assert (list(dec["lcm_rows"]), list(dec["lcm_cols"]), dec["lcm_min_val"]) == (rows, cols, lm)
        return None
    if dec["lcm"]:
        cost = oracle.cost_build(cab_to, dem_from, None, fill, thr)[1]
        _, rows, cols, lm = oracle.lcm(cost, mask=fill, stop_value_on=1, stop_value=fill, stop_size=mnl, sum_below=fill, java_scan=1)
        assert (list(dec["lcm_rows"]), list(dec["lcm_cols"]), dec["lcm_min_val"]) == (rows.tolist(), cols.tolist(), lm)
    if dec["solved"]:
        assert dec["total"] == dec["dual_bound"] == P.opt_thr(np.asarray(cab_to)[dec["kept_cabs"]], np.asarray(dem_from)[dec["kept_dems"]], None,
                                                              fill, thr)
    return None


@pytest.mark.parametrize("which", sorted(BATCH_POLICIES))
def test_a_batch_under_a_policy_per_world(td, monkeypatch, which):
    """handle X runs td_simb_step under the policy list; handle Y, the same worlds, is driven by begin -> model ->
    dispatch_batched (the same batch, n and policy arrays) -> apply; a host Simulator per world replays Y's verified decisions:
    state, metrics and line of the three agree after every tick, and X's event log is the specification's, world by world"""
    from taxidispatcher_amd import simulator
    policies = BATCH_POLICIES[which]
    runs = sbw.family("A")[1]
    B = len(runs)
    assert B == len(policies) == 5
    sw.patch_constants(monkeypatch, CITY)
    X, Y = _batch(td, runs, policies, events=True, event_capacity=1 << 19), _batch(td, runs, policies)
    bes = [BatchReplayBackend(td) for _ in range(B)]
    hosts = [simulator.Simulator(r["rows"], bes[b], n_cabs=r["world"]["cabs"], dispatch=policies[b][0], max_non_lcm=policies[b][1],
                                 parts=policies[b][2], events=True) for b, (_, r) in enumerate(runs)]
    modes, mnls, parts = ([p[k] for p in policies] for k in range(3))
    rule = [m if d == "lcm+opt" else -1 if d == "lcm" else 1 << 30 for d, m in zip(modes, mnls)]
    cover, lcm_ticks = [], [0] * B
    for t in range(CITY["ticks"]):
        info = Y.begin(t)
        y_lines = [None] * B
        if info[:, 0].any():
            cab_off, cab_to, dem_off, dem_from = Y.model()
            cabs = [cab_to[cab_off[b]:cab_off[b + 1]] for b in range(B)]
            dems = [dem_from[dem_off[b]:dem_off[b + 1]] if info[b, 2] else dem_from[:0] for b in range(B)]   # no supply: no model
            n = max(1, max(max(len(c), len(d)) for c, d in zip(cabs, dems)))
            res = td.dispatch_batched(cabs, dems, None, big_cost=sw.BIG_COST, drop_time=CITY["drop_time"], size=CITY["stands"], mode=modes,
                                      max_non_lcm=mnls, parts=parts, n=n)
            decisions = []
            for b in range(B):
                n_s, n_d = int(info[b, 2]), int(info[b, 3])
                if not info[b, 0] or not n_s:
                    decisions.append(None)
                    continue
                lcm = max(n_s, n_d) > rule[b]
                lcm_ticks[b] += lcm
                k = int(res["n_pairs"][b]) if lcm else 0
                nr, lm = int(res["n_rest"][b]), int(res["lcm_min_val"][b])
                solved = modes[b] != "lcm" and nr > 0 and not (lcm and lm == sw.BIG_COST)
                dec = dict(lcm=lcm, lcm_rows=res["lcm_rows"][b, :k], lcm_cols=res["lcm_cols"][b, :k], lcm_min_val=lm, solved=solved,
                           row_to_col=res["row_to_col"][b, :nr] if solved else res["row_to_col"][b, :0], total=int(res["total"][b]),
                           dual_bound=int(res["dual_bound"][b]), kept_cabs=res["kept_cabs"][b, :n_s - k], kept_dems=res["kept_dems"][b, :n_d - k])
                cover.append(_verify(policies[b], cabs[b], dems[b], dec))
                bes[b].dec = dec
                decisions.append((dec["lcm_rows"], dec["lcm_cols"], solved, dec["row_to_col"]))
            opt = Y.apply(decisions)
            for b in range(B):
                n_s, n_d = int(info[b, 2]), int(info[b, 3])
                d = decisions[b]
                lcm = n_s > 0 and max(n_s, n_d) > rule[b]
                k = len(d[0]) if lcm else 0
                y_lines[b] = Y.format_line(t, [info[b, 0], info[b, 1], n_s, lcm, k, lcm and d[2], n_d - k if n_s else 0, n_s - k, opt[b]])
        x_lines = X.tick(t) or [None] * B
        xm, ym = X.m, Y.m
        for b in range(B):
            h_line = hosts[b].tick(t)
            assert x_lines[b] == y_lines[b] == h_line, (t, b, x_lines[b], y_lines[b], h_line)
            assert xm[b] == ym[b] == hosts[b].m, (t, b)
            want = sw.state_of(hosts[b])
            for dev in (X, Y):
                got = dev.state(b)
                for key, v in want.items():
                    assert np.array_equal(got[key], v), (t, b, key)
    ev = X.events()
    assert X.events_lost == 0
    for b in range(B):
        assert td.format_events(ev, world=b) == td.format_events(hosts[b].events), b
        assert X.m[b]["total_LCM_used"] == lcm_ticks[b]
        if modes[b] in ("opt", "split"):
            assert lcm_ticks[b] == 0
    assert sum(lcm_ticks) > 0
    split = [c for c in cover if c is not None]
    assert sum(c["served"] for c in split) > 0 and sum(c["fifth_serves"] for c in split) > 0


def test_a_batch_that_sets_the_default_policy_takes_the_default_course(td):
    import ctypes
    runs = sbw.family("A")[1]
    plain, same = _batch(td, runs), _batch(td, runs)
    lib = td._ffi.lib()
    before, after = ctypes.c_int64(-1), ctypes.c_int64(-2)
    assert lib.td_workspace_bytes(ctypes.byref(before)) == 0
    same.set_dispatch("lcm+opt", CITY["max_non_lcm"], 4)
    assert lib.td_workspace_bytes(ctypes.byref(after)) == 0 and before.value == after.value   # the call allocates nothing
    for t in range(CITY["ticks"]):
        assert plain.tick(t) == same.tick(t), t
        assert plain.m == same.m
        for b in range(len(runs)):
            a, c = plain.state(b), same.state(b)
            assert all(np.array_equal(a[k], c[k]) for k in a)


def test_td_simb_dispatch_contract(td):
    lib, A = td._ffi.lib(), td._ffi.addr
    runs = sbw.family("A")[1]
    dev, plain = _batch(td, runs), _batch(td, runs)
    B = dev.batch
    err = lambda: td._ffi.load().td_last_error().decode()
    i32 = lambda v: np.asarray(v, np.int32)
    assert lib.td_simb_dispatch(None, None, None, None) == -1 and "null handle" in err()
    for mode, mnl, parts, word in (([0, 4, 0, 0, 0], None, None, "mode[1] = 4"), ([-1, 0, 0, 0, 0], None, None, "mode[0] = -1"),
                                   (None, [16, 16, -1, 16, 16], None, "max_non_lcm[2] = -1"), (None, [16, 1025, 16, 16, 16], None, "1025 > 1024"),
                                   ([3] * 5, None, [4, 4, 0, 4, 4], "parts[2] = 0"), ([3] * 5, None, [33, 4, 4, 4, 4], "parts[0] = 33"),
                                   ([3] * 5, None, [4, 4, 4, 4, 13], "parts[4] = 13")):      # 13 parts over 12 stands
        args = [None if v is None else i32(v) for v in (mode, mnl, parts)]
        assert lib.td_simb_dispatch(dev._h, *[A(a) for a in args]) == -1 and word in err(), word
    assert lib.td_simb_dispatch(dev._h, A(i32([0, 1, 2, 0, 1])), None, A(i32([0, 99, -3, 0, 0]))) == 0   # parts are read for the split only
    assert lib.td_simb_dispatch(dev._h, None, None, None) == 0                                          # NULL: as created
    for t in range(3):   # the refused calls changed nothing, the last one restored the default
        assert dev.tick(t) == plain.tick(t)
    t = 3
    while not (dev.begin(t)[:, 2] > 0).any():   # a tick in which some world has demand and supply: it waits for its apply
        if dev._info[:, 0].any():
            dev.apply([None] * B)
        t += 1
    assert lib.td_simb_dispatch(dev._h, None, None, None) == -1 and "waits for td_simb_apply" in err()
    dev.apply([None] * B)
    import torch
    assert lib.td_simb_dispatch(dev._h, A(torch.tensor([2] * B, dtype=torch.int32).cuda()), None, None) == 0   # device memory
    lines = [ln for u in range(t + 1, CITY["ticks"]) for ln in (dev.tick(u) or []) if ln]
    assert lines and all("OPT count" not in ln for ln in lines if "supply=0." not in ln)


@pytest.mark.parametrize("mode", ["split", "opt"])
def test_a_batch_refuses_a_model_above_1024_in_its_step(td, mode):
    """world 1 has 1100 cabs and 1100 requests at one stand: the step names the world and the counts, the tick stays begun and
    is finished through model / apply"""
    n = 1100
    rows = np.array([(i, 0, 1, 0, 0) for i in range(n)], np.int64)
    small = np.array([(0, 1, 0, 0, 0)], np.int64)
    dev = td.DeviceSimulatorBatch([small, rows], [2, n], n_stands=2, drop_time=2, max_non_lcm=16, big_cost=sw.BIG_COST, pool="none",
                                  dispatch=["lcm", mode], parts=2)
    with pytest.raises(td.TdError, match="world 1's .* model has 1100 cabs and 1100 requests in tick 0, more than 1024"):
        dev.tick(0)
    lib = td._ffi.lib()
    assert lib.td_simb_dispatch(dev._h, None, None, None) == -1            # the tick still waits for its apply
    cab_off, cab_to, dem_off, dem_from = dev.model()
    assert cab_off.tolist() == [0, 2, 2 + n] and dem_off.tolist() == [0, 1, 1 + n]
    c1 = cab_to[2:]
    r2c = np.full(n, -1, np.int32)
    at0 = np.nonzero(c1 == 0)[0]
    r2c[at0] = np.arange(at0.size)                                          # a cab standing at stand 0 takes a request there
    opt = dev.apply([([0 if cab_to[0] == 1 else 1], [0], True, []), ([], [], True, r2c)])   # world 0: the LCM alone, `solved` is ignored
    assert opt.tolist() == [-1, n // 2]
    m = dev.m
    assert m[1]["max_solver_size"] == n and m[1]["total_LCM_used"] == 0 and m[0]["total_LCM_used"] == 1 and m[0]["max_solver_size"] == 0
