"""td_pool_n_banded_batched on the GPU: the band loop inside the workgroup against the host model of td_pool_n_banded
(pool_band_model.banded: records AND stats), the oracle, td_pool_n_batched and the reference binary's fixtures; the refusal it
removes; a workgroup's second model; the contract of the C call."""
import numpy as np
import pytest

import pool_band_batched_cases as B
import pool_band_cases as C
import pool_band_model as M
import pool_fixtures as pf
import pool_n_batched_cases as pc
from oracle import oracle

pytestmark = pytest.mark.gpu

GUARD = -77
TD_EINVAL, TD_ERANGE = -1, -4


def ffi():
    from taxidispatcher_amd import _ffi
    return _ffi


def err():
    return ffi().lib().td_last_error().decode()


def call(td, k, demands, dist=None, firsts=None, plan_buffer=0, n=None, want=True, off=None):
    """the raw C call on host arrays, every output pre-filled with GUARD -> dict(rc, pools [B, n // k, 2k+1], m, nh, tot, stats)"""
    f = ffi()
    off_, frm, to, wait, loss, first, batch, nmax = td.pack_pool_n(demands, firsts)
    off_ = off_ if off is None else np.ascontiguousarray(off, np.int32)
    n = nmax if n is None else n
    d = None if dist is None else np.ascontiguousarray(dist, np.int32)
    kk = max(k, 1)
    pools = np.full((batch, max(n, 0) // kk, 2 * kk + 1), GUARD, np.int32)
    m = np.full(batch, GUARD, np.int32)
    nh, tot, st = np.full(batch, GUARD, np.int64), np.full(batch, GUARD, np.int64), np.full((batch, 4), GUARD, np.int64)
    rc = f.lib().td_pool_n_banded_batched(k, batch, n, f.addr(off_), f.addr(frm), f.addr(to), f.addr(wait), f.addr(loss), f.addr(d),
                                          0 if d is None else d.shape[0], f.addr(first), plan_buffer, f.addr(pools) if pools.size else None,
                                          f.addr(m), f.addr(nh) if want else None, f.addr(tot) if want else None, f.addr(st) if want else None)
    return dict(rc=rc, pools=pools, m=m, nh=nh, tot=tot, stats=st)


def untouched(got):
    return all((got[key] == GUARD).all() for key in ("pools", "m", "nh", "tot", "stats"))


def assert_model(got, b, recs, nh, stats, what):
    m = int(got["m"][b])
    assert got["pools"][b, :m].tolist() == recs, (what, b)
    assert m == len(recs) and (got["pools"][b, m:] == GUARD).all(), (what, b)      # nothing behind a model's records
    assert int(got["nh"][b]) == nh and int(got["tot"][b]) == sum(r[-1] for r in recs), (what, b)
    if stats is not None:
        assert tuple(got["stats"][b].tolist()) == tuple(stats), (what, b, got["stats"][b].tolist(), stats)


# ---- the edge corpus of td_pool_n_banded, each case twice in a batch of three ---------------------------------------------------
@pytest.mark.parametrize("k", C.KS)
def test_the_edge_corpus(td, k):
    """a room equal to a bin and one below at every level, the k = 2 second band, bitmap words 31 / 32 / 63 / 64, the slice under
    a deep cut, n = 255 / 256 / 257: records == the oracle's, n_happy and all four stats == the host model's, for both copies"""
    cases = B.corpus()[k]
    assert len(cases) == B.CORPUS_COUNTS[k]
    for bc in cases:
        c, s = bc.case, C.solve(bc)
        d = C.rows(c)
        fd, frecs, fnh, fstats = B.filler(k, bc.room)
        assert 1 <= len(fd) <= bc.room // 24 and len(fd) != len(d)
        got = call(td, k, [d, fd, d], c.dist, [(c.first0, c.first1), None, (c.first0, c.first1)], bc.room)
        assert got["rc"] == 0, (bc.name, err())
        for b in (0, 2):
            assert_model(got, b, s.exp, s.nh, s.stats, bc.name)
        assert_model(got, 1, frecs, fnh, fstats, bc.name + " filler")


# ---- the named inputs: one batch per k under three buffers ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def named():
    """k -> (demands, the table, per model: the oracle's records, its happy count, the plans in key order); every model under
    table_case(k)'s table, which the stands of the other inputs fit"""
    out = {}
    for k in C.KS:
        td_, dist = M.table_case(k)
        ds = [d for d, _ in M.inputs().values()] + [td_]
        assert max(int(d[:, 1:3].max()) for d in ds) < dist.shape[0]
        per = []
        for d in ds:
            exp, nh = oracle.pool_n(k, d[:, 1], d[:, 2], d[:, 3], d[:, 4], dist, cap=3000000)
            per.append((exp.tolist(), nh, M.happy_plans(k, d, dist)))
        out[k] = (ds, dist, per)
    return out


@pytest.mark.parametrize("k", C.KS)
def test_the_named_inputs_as_one_batch(td, named, k):
    ds, dist, per = named[k]
    n_max = max(len(d) for d in ds)
    assert n_max == 80
    ref, ref_nh = td.pool_n_batched(k, ds, dist, max_happy=1 << 22)
    for room in (24 * n_max, 8192, 0):
        got = call(td, k, ds, dist, None, room)
        assert got["rc"] == 0, err()
        for b, (d, (exp, nh, (cost, p, qi))) in enumerate(zip(ds, per)):
            stats = M.banded(k, len(d), cost, p, qi, room or 65536)[2]
            print(k, room, b, stats)
            assert_model(got, b, exp, nh, stats, (k, room))
            assert ref[b].tolist() == exp and int(ref_nh[b]) == nh
        if room and k == 4:
            assert got["stats"][:, 0].max() >= 2 and got["stats"][:, 3].max() <= room


# ---- the reference binary's fixtures ------------------------------------------------------------------------------------------------
def test_the_reference_fixtures_with_the_smallest_buffer(td):
    for name, k in pf.cases():
        ds, firsts, exp = pc.fixture_batch(name, k)
        n = len(ds[0])
        assert n <= 400
        got = call(td, k, ds, None, firsts, 24 * n)
        assert got["rc"] == 0, (name, k, err())
        for c in range(8):
            assert got["pools"][c, :got["m"][c]].tolist() == exp[c], (name, k, c)
            assert got["tot"][c] == sum(r[-1] for r in exp[c]) and got["stats"][c, 3] <= 24 * n
        assert td.find_pool_fanout(k, ds[0], plan_buffer=24 * n).tolist() == pf.merge_restatement(k, exp), (name, k)


# ---- the refusal is gone ------------------------------------------------------------------------------------------------------------
def test_the_refusal_it_removes(td):
    """test_gpu_pool_n_batched.py::test_capacity_edge's batch: model 1 has one plan more than max_happy"""
    k, d = 4, pc.edge_model()
    small = pc.mixed_batch()[2], pc.mixed_batch()[6]
    ds = [small[0], d, small[1]]
    exp = [pc.oracle_model(k, x, cap=65536) for x in ds]
    happy = exp[1][1]
    assert 1000 < happy < 32768
    with pytest.raises(ffi().TdError) as e:
        td.pool_n_batched(k, ds, max_happy=happy - 1)
    assert "error %d" % TD_ERANGE in str(e.value) and "model 1" in str(e.value) and str(happy) in str(e.value)
    n = max(len(x) for x in ds)
    got = call(td, k, ds, plan_buffer=24 * n)
    assert got["rc"] == 0, err()
    for b, (recs, nh) in enumerate(exp):
        assert_model(got, b, recs, nh, None, "refusal gone")
    assert got["stats"][1, 0] >= 1 and got["stats"][1, 3] <= 24 * n
    # ... and under a buffer the list does not fit either: 24 x the 64 requests of the largest other model is refused for model 1,
    # so the smallest legal buffer of the batch is the one above
    assert call(td, k, ds, plan_buffer=24 * 64)["rc"] == TD_EINVAL and "model 1" in err()


# ---- a workgroup's second model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", C.KS)
def test_a_workgroups_second_model_under_the_largest_buffer(td, k):
    """plan_buffer = 2^22: 32 workgroups for 70 models of mixed kinds; every model equals the same model alone.  A bitmap, lo, a
    queue count or a histogram that a model leaves behind shows in the next one."""
    ds, firsts, kinds = B.second_model_batch(k)
    assert len(ds) == B.SECOND_B > 2 * 32
    got = call(td, k, ds, None, firsts, B.SECOND_ROOM, n=max(len(d) for d in ds))
    assert got["rc"] == 0, err()
    alone = {}
    for b, (d, f, kind) in enumerate(zip(ds, firsts, kinds)):
        key = (d.tobytes(), f)
        if key not in alone:
            one = call(td, k, [d], None, [f], B.SECOND_ROOM)
            assert one["rc"] == 0, (b, err())
            alone[key] = one
        one = alone[key]
        m = int(one["m"][0])
        assert got["m"][b] == m and got["pools"][b, :m].tolist() == one["pools"][0, :m].tolist(), (k, b, kind)
        assert (got["pools"][b, m:] == GUARD).all()
        for key2 in ("nh", "tot", "stats"):
            assert got[key2][b].tolist() == one[key2][0].tolist(), (k, b, kind, key2)
        st = one["stats"][0].tolist()
        if kind in ("empty", "below_k", "empty_slice"):
            assert m == 0 and one["nh"][0] == 0 and st == [0, 0, 0, 0]
        elif kind == "one_band" or k == 2:
            assert st[0] == 1 and st[1] == 2 and st[3] == one["nh"][0] > 0, (kind, st)
        elif kind == "bands":
            assert st[0] == 2 and st[2] == 0 and one["nh"][0] > B.SECOND_ROOM >= st[3], (kind, st)
        else:
            assert st[2] == 1 and one["nh"][0] > B.SECOND_ROOM >= st[3], (kind, st)
            assert one["pools"][0, :m, :k].reshape(-1).tolist() == list(range(m * k)) and m == len(d) // k


@pytest.mark.parametrize("k", C.KS)
def test_a_second_model_behind_a_model_of_several_bands(td, k):
    """1030 models under a small room (1024 workgroups in flight): workgroups 0 .. 5 take a second model, of another kind than
    their first; every model against the host model's records, happy count and stats"""
    ds, firsts, exp = B.small_room_batch(k)
    got = call(td, k, ds, None, [f if f is not None else (0, len(d)) for d, f in zip(ds, firsts)], B.SMALL_ROOM[k])
    assert got["rc"] == 0, err()
    assert exp[0][2][0] >= 2 and exp[0][2][2] == (1 if k == 2 else k - 1)
    for b in list(range(8)) + list(range(1016, B.SMALL_B)):
        assert_model(got, b, *exp[b], ("small room", k))
    # the rest at once: equal to the first of their kind
    for b in range(8, 1016):
        assert got["m"][b] == got["m"][b % 4] and got["pools"][b].tolist() == got["pools"][b % 4].tolist(), b
        assert got["nh"][b] == got["nh"][b % 4] and got["stats"][b].tolist() == got["stats"][b % 4].tolist(), b


# ---- the contract of the C call ---------------------------------------------------------------------------------------------------
def test_device_pointers_equal_host_arrays(td, named):
    import torch
    f = ffi()
    k = 3
    ds, dist, per = named[k]
    firsts = [None, (3, 20)] + [None] * (len(ds) - 2)
    room = 24 * 80
    host = call(td, k, ds, dist, firsts, room)
    assert host["rc"] == 0
    off, frm, to, wait, loss, first, batch, n = td.pack_pool_n(ds, firsts)
    dev = [torch.from_numpy(a).cuda() for a in (off, frm, to, wait, loss, first.reshape(-1), np.ascontiguousarray(dist, np.int32))]
    pools = torch.full((batch, n // k, 2 * k + 1), GUARD, dtype=torch.int32, device="cuda")
    m = torch.full((batch,), GUARD, dtype=torch.int32, device="cuda")
    nh, tot = (torch.full((batch,), GUARD, dtype=torch.int64, device="cuda") for _ in range(2))
    st = torch.full((batch, 4), GUARD, dtype=torch.int64, device="cuda")
    rc = f.lib().td_pool_n_banded_batched(k, batch, n, *[f.addr(t) for t in dev[:5]], f.addr(dev[6]), dist.shape[0], f.addr(dev[5]), room,
                                          f.addr(pools), f.addr(m), f.addr(nh), f.addr(tot), f.addr(st))
    assert rc == 0, err()
    for a, t in ((host["pools"], pools), (host["m"], m), (host["nh"], nh), (host["tot"], tot), (host["stats"], st)):
        assert a.tolist() == t.cpu().numpy().tolist()
    for b in (0, 2, 3, 4):
        assert_model(host, b, per[b][0], per[b][1], None, "host")
    exp1, nh1 = oracle.pool_n(k, *[ds[1][:, c] for c in (1, 2, 3, 4)], dist, 3, 20, cap=3000000)
    assert_model(host, 1, exp1.tolist(), nh1, None, "the slice")
    # without the optional outputs
    bare = call(td, k, ds, dist, firsts, room, want=False)
    assert bare["rc"] == 0 and bare["pools"].tolist() == host["pools"].tolist() and bare["m"].tolist() == host["m"].tolist()
    assert (bare["nh"] == GUARD).all() and (bare["tot"] == GUARD).all() and (bare["stats"] == GUARD).all()


def test_batch_zero_writes_nothing(td):
    f = ffi()
    g, g64 = np.full(4, GUARD, np.int32), np.full(4, GUARD, np.int64)
    off = np.zeros(1, np.int32)
    assert f.lib().td_pool_n_banded_batched(3, 0, 9, f.addr(off), None, None, None, None, None, 0, None, 0, f.addr(g), f.addr(g), f.addr(g64),
                                            f.addr(g64), f.addr(g64)) == 0
    assert (g == GUARD).all() and (g64 == GUARD).all()
    lists, nh, st = td.pool_n_banded_batched(3, [], stats=True)
    assert lists == [] and nh.size == 0 and st.shape == (0, 4)


def test_refusals_leave_the_outputs_alone(td):
    rng = np.random.default_rng(77)
    ds = [pc.random_demand(rng, m, 3, [10, 30]) for m in (20, 7, 33)]
    good = [0, 20, 27, 60]

    def refused(got, code, what):
        assert got["rc"] == code, (what, got["rc"], err())
        assert untouched(got), what

    assert call(td, 2, ds, n=33, off=good)["rc"] == 0
    for k in (1, 5):
        refused(call(td, k, ds, n=33), TD_EINVAL, ("k", k))
    refused(call(td, 2, ds, n=33, off=[1, 20, 27, 60]), TD_EINVAL, "off[0] = 1")
    refused(call(td, 2, ds, n=33, off=[0, 27, 20, 60]), TD_EINVAL, "a decreasing offset")
    refused(call(td, 2, ds, n=513), TD_EINVAL, "n = 513")
    refused(call(td, 2, ds, n=-1), TD_EINVAL, "n = -1")
    refused(call(td, 2, ds, n=32), TD_EINVAL, "a model of 33 with n = 32")
    refused(call(td, 2, ds, n=33, plan_buffer=(1 << 22) + 1), TD_EINVAL, "plan_buffer above 2^22")
    assert "plan_buffer" in err()
    refused(call(td, 2, ds, n=33, plan_buffer=24 * 33 - 1), TD_EINVAL, "plan_buffer below 24 n")
    assert "model 2" in err() and str(24 * 33 - 1) in err() and str(24 * 33) in err()
    refused(call(td, 2, ds, n=33, plan_buffer=24 * 20 - 1), TD_EINVAL, "plan_buffer below 24 n of the first model")
    assert "model 0" in err() and str(24 * 20 - 1) in err() and str(24 * 20) in err()
    assert call(td, 2, ds, n=33, plan_buffer=24 * 33)["rc"] == 0
    f = ffi()
    off, frm, to, wait, loss, _, batch, n = td.pack_pool_n(ds)
    g, g64 = np.full(64 * 5, GUARD, np.int32), np.full(16, GUARD, np.int64)
    lib = f.lib()
    args = [f.addr(frm), f.addr(to), f.addr(wait), f.addr(loss)]
    assert lib.td_pool_n_banded_batched(2, -1, n, f.addr(off), *args, None, 0, None, 0, f.addr(g), f.addr(g), None, None, f.addr(g64)) == TD_EINVAL
    assert lib.td_pool_n_banded_batched(2, batch, n, None, *args, None, 0, None, 0, f.addr(g), f.addr(g), None, None, f.addr(g64)) == TD_EINVAL
    assert lib.td_pool_n_banded_batched(2, batch, n, f.addr(off), None, *args[1:], None, 0, None, 0, f.addr(g), f.addr(g), None, None,
                                        f.addr(g64)) == TD_EINVAL
    assert lib.td_pool_n_banded_batched(2, batch, n, f.addr(off), *args, None, 0, None, 0, f.addr(g), None, None, None, f.addr(g64)) == TD_EINVAL
    assert lib.td_pool_n_banded_batched(2, batch, n, f.addr(off), *args, None, 0, None, 0, None, f.addr(g), None, None, f.addr(g64)) == TD_EINVAL
    table = np.zeros((1, 1), np.int32)
    assert lib.td_pool_n_banded_batched(2, batch, n, f.addr(off), *args, f.addr(table), 0, None, 0, f.addr(g), f.addr(g), None, None,
                                        f.addr(g64)) == TD_EINVAL
    assert (g == GUARD).all() and (g64 == GUARD).all()
    dist, tds = pc.table_batch()
    bad = [x.copy() for x in tds[:3]]
    bad[1][40, 2] = pc.TABLE_S                                  # a drop-off stand = S
    refused(call(td, 3, bad, dist), TD_EINVAL, "stand = S")
    assert "model 1" in err()
    # a happy pair with cost 20000 on |a - b|: 0 -> 10000 and 10000 -> 20000, both patient and tolerant
    far = np.array([[0, 0, 10000, 20000, 1000], [1, 10000, 20000, 20000, 1000]])
    refused(call(td, 2, [ds[1], far]), TD_ERANGE, "cost 20000")
    assert "14 bits" in err()
    # the cost counters are clean behind a refusal: the next call answers as the first did
    again = call(td, 2, ds, n=33, off=good)
    first = call(td, 2, ds, n=33, plan_buffer=24 * 33)
    assert again["rc"] == 0 and again["pools"].tolist() == first["pools"].tolist() and again["nh"].tolist() == first["nh"].tolist()


def test_a_second_call_on_other_data(td, named):
    """slab, counters and staging are the library's between calls: another batch right behind, and the first again"""
    a = named[4]
    b = named[2]
    for k, (ds, dist, per) in ((4, a), (2, b), (4, a), (2, b)):
        lists, nh, st = td.pool_n_banded_batched(k, ds, dist, plan_buffer=24 * 80, stats=True)
        for i, (exp, h, _) in enumerate(per):
            assert lists[i].tolist() == exp and int(nh[i]) == h, (k, i)
        assert st.shape == (len(ds), 4) and (st[:, 3] <= 24 * 80).all()
