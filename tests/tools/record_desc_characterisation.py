"""Writes tests/desc_characterisation.json: what the library SOLSTRALE_BUILD_DIR names answers to the mutated descriptors of
tests/test_desc_mutations.py::test_refusals_are_the_recorded_ones. Run on a box without a GPU, against a build of the commit whose
behaviour is to be pinned (python solstrale-rust_amd/build.py at that commit, or build(out_dir=...)); never against the tree under test."""
import json
import os
import sys
sys.path.insert(0, "tests/tools"); import _paths  # noqa: E401,F401
import test_desc_mutations as t
from solstrale_amd import _abi

assert os.environ.get("SOLSTRALE_BUILD_DIR"), "name the recorded library's build directory in SOLSTRALE_BUILD_DIR"
texts, per_scene = [], {}
for name, sc in t._scenes().items():
    rows = t._characterise(_abi.load_hip(), sc, t._recorded_groups(sc, name))
    for row in rows:
        for pair in row:
            if pair[1] not in texts:
                texts.append(pair[1])
            pair[1] = texts.index(pair[1])
    per_scene[name] = rows
with open(t.RECORD, "w") as f:
    json.dump({"texts": texts, "scenes": per_scene}, f, separators=(",", ":"))
    f.write("\n")
