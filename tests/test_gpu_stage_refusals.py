"""Replays tests/golden/stage_refusals_parent.json (tools/stage_refusals_golden.py at the commit before csrc/td_stage.h): every
entry point that stages ragged offsets or per-model sizes, with batch = 3 and n = 4, refuses the same inputs with the same
return code and the same td_last_error text, leaves the same output windows untouched (guards included: they are asserted
where the call is made), accepts batch = 0 with null arrays, and a good call returns bit-identical outputs."""
import json
import os

import pytest

import stage_refusal_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_refusals_parent.json")
with open(GOLDEN) as f:
    PARENT = json.load(f)


def test_the_fixture_has_every_case():
    assert sorted(PARENT) == sorted(cases.case_ids())


@pytest.mark.parametrize("cid", cases.case_ids())
def test_as_at_the_parent(td, cid):
    from taxidispatcher_amd import _ffi
    got = json.loads(json.dumps(cases.run_case(_ffi.lib(), cid)))
    want = PARENT[cid]
    assert (got["rc"], got["error"]) == (want["rc"], want["error"])
    assert got["untouched"] == want["untouched"]
    assert got.get("outputs") == want.get("outputs")
    if cid.endswith("/batch0"):
        assert got["rc"] == 0
