"""Runs every case of tests/stage_refusal_cases.py on GPU 0 and prints (or writes with --out) one JSON object
{case id: record}: return code, td_last_error text, which output windows were left untouched, and the defined outputs of the
calls that succeed.

tests/golden/stage_refusals_parent.json is this script's output at the commit before the staging helpers of the batched
calls and the world handles moved into csrc/td_stage.h; tests/test_gpu_stage_refusals.py replays it.

    python tools/stage_refusals_golden.py --out tests/golden/stage_refusals_parent.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import taxidispatcher_amd as td
    from taxidispatcher_amd import _ffi
    import stage_refusal_cases as cases
    td.init(0)
    text = json.dumps(cases.run(_ffi.lib()), indent=1, sort_keys=True)
    td.shutdown()
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
