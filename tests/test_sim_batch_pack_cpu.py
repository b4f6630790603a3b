"""simulator.pack_worlds: the host side of td_simb_create (demand tables and fleet sizes -> concatenated int32 arrays and
offsets).  No GPU."""
import numpy as np
import pytest

from taxidispatcher_amd import simulator


def rows(*r):
    return np.array(r, np.int64).reshape(-1, 5)


def test_tables_are_concatenated_world_after_world():
    a = rows((5, 0, 1, 0, 0), (6, 2, 3, 1, 4))
    c = rows((5, 4, 0, 2, 2))                       # the id 5 again: ids are unique per world, not across worlds
    cabs, off, rid, rfrom, rto, rat = simulator.pack_worlds([a, np.zeros((0, 5), np.int64), c], [3, 1, 2000])
    assert cabs.dtype == off.dtype == rid.dtype == rat.dtype == np.int32
    assert cabs.tolist() == [3, 1, 2000] and off.tolist() == [0, 2, 2, 3]      # an empty table in the middle
    assert rid.tolist() == [5, 6, 5] and rfrom.tolist() == [0, 2, 4] and rto.tolist() == [1, 3, 0]
    assert rat.tolist() == [0, 4, 2]                # column 4 (at), not column 3 (time)
    assert all(x.flags["C_CONTIGUOUS"] for x in (cabs, off, rid, rfrom, rto, rat))


def test_a_single_world_and_an_empty_list_table():
    cabs, off, rid, rfrom, rto, rat = simulator.pack_worlds([rows((1, 0, 1, 0, 0))], [7])
    assert cabs.tolist() == [7] and off.tolist() == [0, 1] and rid.tolist() == [1]
    cabs, off, rid, _, _, _ = simulator.pack_worlds([[]], [1])                # a plain empty list is an empty table
    assert off.tolist() == [0, 0] and rid.size == 0 and rid.dtype == np.int32


@pytest.mark.parametrize("tables, cabs, msg", [
    ([], [], "at least one world"),
    ([rows((1, 0, 1, 0, 0))], [1, 2], "1 demand tables for 2 fleet sizes"),
    ([rows((1, 0, 1, 0, 0)), rows((2, 0, 1, 0, 0), (2, 1, 2, 0, 0))], [1, 1], "unique within world 1"),
    ([rows((-1, 0, 1, 0, 0))], [1], "world 0 has a negative request id"),
    ([rows((1, 0, 1, 0, 0))], [0], "world 0 has 0 cabs"),
    ([np.zeros((2, 4), np.int64)], [1], "shape (2, 4), not (n, 5)"),
    ([rows((1, 0, 2**31, 0, 0))], [1], "outside int32"),
])
def test_error_messages(tables, cabs, msg):
    with pytest.raises(ValueError) as e:
        simulator.pack_worlds(tables, cabs)
    assert msg in str(e.value)
