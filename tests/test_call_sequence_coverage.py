"""So that the next extension of the C ABI is not forgotten by the call-sequence campaigns: every exported function of include/solstrale_hip.h
whose first parameter is a SolScene* is either called by one of the two campaigns - tests/test_gpu_call_sequences.py (the render path's surface,
named inside its Handle class) or tests/test_gpu_call_sequences_ext.py (everything since: the keys of its CALLS table and what its ALSO table lists
inside a composite call) - or listed in EXCLUDED below with the reason. No GPU: the header and the two files are read as text."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

EXCLUDED = {
    "sol_comm_init": "needs the other ranks of a communicator: tests/test_gpu_gather.py",
    "sol_read_image": "reads what a gather over several handles assembled: tests/test_gpu_gather.py, tests/test_gpu_local_devices.py",
    "sol_env_sampling": "needs a scene with an environment map, which the campaigns' scenes lack: tests/test_env_importance.py",
    "sol_env_tables": "reads the tables of sol_env_sampling: tests/test_env_importance.py",
    "sol_env_eval": "evaluates the tables of sol_env_sampling: tests/test_env_importance.py",
    "sol_light_eval": "a function-level probe of the light tree: tests/test_gpu_light_sampling.py",
    "sol_scene_background_flags": "a moved handle's proof is sound, not the fresh handle's flag for flag - there is no yardstick: tests/test_gpu_set_camera.py",
    "sol_scene_set_triangles_ms": "timings: nothing to compare",
    "sol_scene_triangle_records": "pre-split triangles make several records a caller's triangle, in each build's own order: tests/test_gpu_set_triangles.py",
}


def scene_entry_points():
    """Every function the device header declares whose first parameter is a SolScene* (const or not), the way tests/test_abi.py reads the header."""
    text = open(os.path.join(ROOT, "include", "solstrale_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"static inline[^{;]*\{.*?\n\}", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sol_[a-z0-9_]+)\s*\(\s*(?:const\s+)?SolScene\s*\*\s*[a-z_]+\s*[,)]", text)))


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "solstrale_hip.h")).read(), flags=re.S)
    return set(re.findall(r"\b(sol_[a-z0-9_]+)\s*\(", text))


def names_in(node):
    """every sol_* name a piece of syntax holds: as an attribute (L.sol_render) or inside a string ("sol_render", f"sol_bloom(..")"""
    found = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Attribute) and n.attr.startswith("sol_"):
            found.add(n.attr)
        elif isinstance(n, ast.Constant) and isinstance(n.value, str):
            found |= set(re.findall(r"\bsol_[a-z0-9_]+\b", n.value))
    return found


def old_campaign_calls():
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_call_sequences.py")).read())
    handle = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Handle"]
    assert len(handle) == 1
    return names_in(handle[0])


def _literal_dict(tree, name):
    found = [n.value for n in tree.body if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in n.targets)]
    assert len(found) == 1 and isinstance(found[0], ast.Dict), name
    keys = [k.value for k in found[0].keys if isinstance(k, ast.Constant) and isinstance(k.value, str)]
    assert len(keys) == len(found[0].keys) == len(set(keys)), f"{name}: literal, distinct entry point names"
    return dict(zip(keys, found[0].values))


def new_campaign_calls():
    """The keys of CALLS - one per distinct call - and, for the composite calls among them, the names ALSO lists under their key."""
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_call_sequences_ext.py")).read())
    calls, also = _literal_dict(tree, "CALLS"), _literal_dict(tree, "ALSO")
    assert set(also) <= set(calls), "ALSO: every key is a key of CALLS"
    names = set(calls)
    for key, inside in also.items():
        listed = ast.literal_eval(inside)
        assert listed and all(isinstance(n, str) for n in listed) and not set(listed) & set(calls), key
        names |= set(listed)
    return names


def test_every_entry_point_that_takes_a_scene_is_in_a_campaign_or_excluded_by_name():
    entry_points = scene_entry_points()
    assert len(entry_points) >= 115 and {"sol_render", "sol_scene_info", "sol_lightmap_chart_levels_dev", "sol_scene_set_primitives"} <= set(entry_points)
    called = old_campaign_calls() | new_campaign_calls()
    missing = [n for n in entry_points if n not in called and n not in EXCLUDED]
    assert not missing, f"neither campaign calls {missing}, and tests/test_call_sequence_coverage.py does not exclude them"


def test_the_exclusions_are_entry_points_no_campaign_calls():
    called = old_campaign_calls() | new_campaign_calls()
    assert not sorted(set(EXCLUDED) & called), "excluded, but called by a campaign"
    assert not sorted(set(EXCLUDED) - set(scene_entry_points())), "excluded, but not an entry point of the header that takes a scene"
    assert all(isinstance(r, str) and len(r) > 10 for r in EXCLUDED.values())


def test_the_new_campaign_s_table_names_declared_functions_only():
    unknown = sorted(new_campaign_calls() - declared())
    assert not unknown, f"CALLS names {unknown}, which include/solstrale_hip.h does not declare"
    assert len(new_campaign_calls() - old_campaign_calls()) >= 60  # (the surface the older file does not reach)
