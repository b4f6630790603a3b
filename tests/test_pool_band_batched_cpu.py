"""What td_pool_n_banded_batched and td_simb_pool_buffer need checked without a GPU: the corpus the GPU test runs and its three
counts, the batches in which a workgroup takes a second model, DeviceSimulatorBatch's pool_buffer validation, and the new
calls' prototypes in the header and in _ffi.SIGNATURES."""
import os
import re

import pytest

import pool_band_batched_cases as B
import pool_band_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_corpus_filter_and_its_three_counts():
    corpus = B.corpus()
    assert {k: len(v) for k, v in corpus.items()} == B.CORPUS_COUNTS == {2: 22, 3: 23, 4: 20}
    everything = [bc for cases in C.all_cases().values() for bc in cases]
    kept = [bc for k in C.KS for bc in corpus[k]]
    assert all(bc.max_pools is None and bc.case.frm.size <= 512 and bc.room >= 24 * bc.case.frm.size for bc in kept)
    left = [bc for bc in everything if not any(bc is x for x in kept)]
    assert left and all(bc.max_pools is not None or bc.case.frm.size > 512 for bc in left)
    assert len(kept) + len(left) == len(everything)
    # what the GPU test is there for is inside the filter
    names = {bc.name for bc in kept}
    for k in C.KS:
        assert {"bitmap_first_n%d_k%d" % (n, k) for n in C.BITMAP_N} <= names
        assert {"band_grid_n%d_k%d" % (n, k) for n in (255, 256, 257)} <= names
    assert {"slice_deep_k3", "slice_deep_k4", "k2_same40", "level0_exact", "level0_below"} <= names
    assert {"same%d_k%d_room%d" % key for key in C.CUT_TABLE} <= names


@pytest.mark.parametrize("k", C.KS)
def test_the_filler_is_a_different_small_model(k):
    for room in sorted({bc.room for bc in B.corpus()[k]}):
        d, recs, nh, stats = B.filler(k, room)
        assert 1 <= len(d) <= room // 24 and len(d) <= 7
        assert len(recs) == len(d) // k and nh > 0 and stats[3] <= room


@pytest.mark.parametrize("k", C.KS)
def test_the_second_model_batches(k):
    ds, firsts, kinds = B.second_model_batch(k)
    assert len(ds) == len(firsts) == len(kinds) == 70 and set(kinds) == {"empty", "below_k", "empty_slice", "one_band", "bands", "deep"}
    assert max(len(d) for d in ds) <= 512
    # 32 workgroups deal the models grid-stride: every workgroup's second model is of another kind than its first
    assert all(kinds[b] != kinds[b + 32] for b in range(32))
    small, sf, exp = B.small_room_batch(k)
    assert len(small) == len(sf) == len(exp) == B.SMALL_B > 1024 and max(len(d) for d in small) <= B.SMALL_ROOM[k] // 24
    assert exp[0][2][0] >= 2 and exp[0][2][2] == (1 if k == 2 else k - 1)      # several bands, the deepest cut
    assert all(small[b] is not small[b - 1024] for b in range(1024, B.SMALL_B))
    assert exp[2] == ([], 0, (0, 0, 0, 0)) and exp[1][1] > 0 and exp[3][1] > 0


def test_the_batch_pool_buffer_validation():
    from taxidispatcher_amd import simulator as S
    size = lambda v: S.pool_buffer_size(v, 512, S.POOL_BUFFER_BATCH_MAX)
    assert S.POOL_BUFFER_BATCH_MIN == 24 * 512 and S.POOL_BUFFER_BATCH_MAX == 1 << 22
    assert size(0) == 0 and size(24 * 512) == 24 * 512 and size(1 << 22) == 1 << 22 and size(65536) == 65536
    for bad in (-1, 1, 24 * 512 - 1, (1 << 22) + 1, True, 3.0, "65536", None):
        with pytest.raises(ValueError):
            size(bad)
    # the single world's rule is as it was
    assert S.pool_buffer_size(24 * 2047) == 24 * 2047 and S.pool_buffer_size(1 << 30) == 1 << 30
    with pytest.raises(ValueError) as e:
        S.pool_buffer_size(24 * 2047 - 1)
    assert "24 * 2047" in str(e.value)
    # the batch refuses before anything touches the library
    for bad in (100, -5, (1 << 22) + 1):
        with pytest.raises(ValueError):
            S.DeviceSimulatorBatch([[]], [1], pool_buffer=bad)


def test_the_header_and_the_ffi_agree_on_the_new_calls():
    import ctypes
    from taxidispatcher_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "taxidispatcher_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in ("td_pool_n_banded_batched", "td_simb_pool_buffer"):
        m = re.search(r"TD_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _ffi.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            if "*" in p:
                assert a in (_ffi.c_i32p, ctypes.c_void_p) or isinstance(a, type(ctypes.POINTER(ctypes.c_int))), (name, p, a)
            else:
                assert a is ctype[p.split()[0]], (name, p, a)
    assert len(_ffi.SIGNATURES["td_pool_n_banded_batched"][1]) == len(_ffi.SIGNATURES["td_pool_n_batched"][1]) + 1
