"""td_assign's line-metric attempt (csrc/td_line.hip) on the case table of tests/line_path_cases.py: every branch of the probe,
both sides of the scan bases of k_line_scan and wg_scan, 64-bit prices, both certificate variants and the certificate's last row
group and column, the unbalanced plan's edges and the transposed retry.  A bug on this path is slow, not wrong -- a refused
certificate falls through to the general solver with the same total -- so every case is held to its reference AND to the path it
is a case for: td_last_stats word 12 (`line_path`) must show exactly the bits the table states (test_line_paths_cpu.py confirms
them, and the cases' structural claims, from the references alone).  Run with -s to see each case's figures."""
import numpy as np
import pytest

import line_path_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture()
def line_on(td):
    was = td.set_line_metric(True)
    yield td
    td.set_line_metric(was)


def _matrix(c):
    """(what td.assign gets, the buffer that owns it or None)"""
    if c["via"] == "host":
        return L.numpy_matrix(c), None
    import torch
    n = c["n"]
    if c["via"] == "device":
        return L.torch_matrix(c, torch), None
    buf = torch.empty(n * n + 4, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    m = buf[1:1 + n * n].view(n, n)
    L.torch_matrix(c, torch, out=m)
    assert m.data_ptr() % 16 == 4 and m.is_contiguous()
    return m, buf


@pytest.mark.parametrize("name", L.CASE_NAMES)
def test_line_case(line_on, name):
    td = line_on
    c = L.case(name)
    n, ref = c["n"], L.reference(name)
    m, buf = _matrix(c)
    r2c, total, dual = td.assign(m, want_dual=True)
    st = td.last_stats()
    if c["via"] == "host":
        cells = int(m[np.arange(n), r2c].astype(np.int64).sum())
    else:
        import torch
        cells = int(m[torch.arange(n, device="cuda"), torch.as_tensor(r2c, device="cuda").long()].sum(dtype=torch.int64).item())
        del m, buf
        torch.cuda.empty_cache()
    print(name, "n", n, "total", total, "dual", dual, "cells", cells, "ref", ref, "line_path", st["line_path"], "/", c["bits"],
          {k: st[k] for k in ("line_metric", "line_dummies", "transposed")})
    assert sorted(r2c.tolist()) == list(range(n)), name
    assert cells == total == dual == ref, name
    assert st["line_path"] == c["bits"], (name, st["line_path"], c["bits"])
    assert st["line_metric"] == c["stats"]["line_metric"] == (st["line_path"] & L.ACCEPTED) // L.ACCEPTED, name
    assert st["line_dummies"] == c["stats"]["line_dummies"], name
    if not c["refused"]:      # (after a refusal the general solver decides for itself which formulation it solves)
        assert st["transposed"] == c["stats"]["transposed"], name
    else:
        assert st["line_path"] & L.PROBE and not st["line_path"] & L.ACCEPTED, name


def test_line_path_word_is_cleared_and_kept(line_on):
    """word 12 is zeroed when td_assign is entered (attempt off: it stays 0) and survives the general solver after a refusal"""
    td = line_on
    rng = np.random.default_rng(3)
    cost = rng.integers(0, 1000, (80, 80)).astype(np.int32)
    c = L.case("rev_on_n64")
    td.assign(L.numpy_matrix(c))
    assert td.last_stats()["line_path"] == c["bits"]
    td.assign(cost)
    assert td.last_stats()["line_path"] == L.PROBE and td.last_stats()["line_metric"] == 0
    td.assign(L.numpy_matrix(c))
    td.set_line_metric(False)
    td.assign(L.numpy_matrix(c))
    assert td.last_stats()["line_path"] == 0 and td.last_stats()["line_metric"] == 0
    td.set_line_metric(True)
