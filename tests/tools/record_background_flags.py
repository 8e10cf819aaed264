"""Writes tests/background_flags_recorded.json: which blocks the host proof of the library SOLSTRALE_BUILD_DIR names flags (sol_background_blocks)
in the cases of tests/test_background_blocks.py::test_host_flags_match_the_recorded_parent - per case the number of blocks, the number flagged
and a SHA-1 of np.packbits(flags). Run on a box without a GPU, against a build of the commit whose behaviour is to be pinned
(build(out_dir=...) at that commit); never against the tree under test."""
import json
import os
import sys
sys.path.insert(0, "tests/tools"); import _paths  # noqa: E401,F401
import test_background_blocks as t

assert os.environ.get("SOLSTRALE_BUILD_DIR"), "name the recorded library's build directory in SOLSTRALE_BUILD_DIR"
cases = t.flag_records()
flagging = sum(1 for v in cases.values() if v[1] > 0)
assert flagging >= 60, flagging
with open(t.RECORD, "w") as f:
    json.dump({"cases": cases}, f, separators=(",", ":"))
    f.write("\n")
print(f"{len(cases)} cases, {flagging} with flagged blocks", file=sys.stderr)
