"""The `dfs_index` contract (include/solstrale_hip.h; DESIGN.md 4, the tie rule and rule 8): the device breaks ties between equal hits by
`dfs_index` and recognises the flat primitive a ray leaves by it, the float oracle by its walk of the caller's tree and by the primitive
reference. The two agree only when every record the tree reaches carries its number in the tree's pre-order walk (the last visit's, for a
shared sub-tree), and the three descriptor entry points - sol_scene_create, sol_world_tree_check_ex, sol_background_blocks - refuse
any other numbering. Before they did, a raw-API descriptor with every Cornell quad at 0 rendered 34 664 of 40 000 pixels away from the
oracle (geometry vanished for every secondary ray: a hit on any quad counted as leaving it), and a reversed numbering flipped every tie.

CPU half: every scene the suite builds passes; duplicated, swapped, shifted, tagged and first-visit numberings are refused by all three
entry points, and so is a seeded campaign of single-record changes. GPU half: descriptors the check accepts but the host never emits - the
primitive tables in another order, a shared sub-tree with a tie - render bit for bit as their host-made twins and within 1e-5 of the
oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dfs_util as du
import orc
import parity_util as pu
from random_scenes import needle_scene, random_scene
from ref_cases import CASES
from solstrale_amd import AlbedoShader, DeviceError, DeviceScene, RenderConfig, _abi, scenes

N_MUTATIONS = int(os.environ.get("SOL_TEST_MUTATIONS", "600"))  # (as in test_desc_mutations: SOL_TEST_MUTATIONS scales the campaign)
SEED_SHIFT = int(os.environ.get("SOL_TEST_MUTATION_SEED", "0"))
CAMPAIGN_SEED = 0xDF5
MESSAGE = re.compile(rb"dfs_index: (sphere|quad|triangle|medium) (\d+) carries (\d+), the world tree's depth-first order gives it (\d+)")
TREE_CHECK_V1_BYTES = 48  # (SOL_TREE_CHECK_V1_BYTES: SolTreeCheck's first layout, through leaf_area)
BASES = ["cornell", "test_scene", "obj_box", "needles"]
KIND_OF_NAME = {v.encode(): k for k, v in du.KIND_NAMES.items()}


def _rc(w=24, h=16, spp=1, shader=None):
    return RenderConfig(w, h, spp, shader) if shader else RenderConfig(w, h, spp)


PRODUCERS = {
    "c1_cornell": lambda: scenes.cornell_box(_rc()),
    "c2_cornell_spheres": lambda: scenes.cornell_spheres(_rc(), n_spheres=300),
    "c3_sponza": lambda: scenes.sponza_like(_rc(), n_triangles=6000, texture_size=16),
    "c3_sponza_heterogeneous": lambda: scenes.sponza_like(_rc(), texture_size=16, mesh="heterogeneous"),  # (its full 262 267: the layout needs them)
    "c5_statue": lambda: scenes.statue_like(_rc(), n_triangles=6000),
    "test_scene": lambda: scenes.create_test_scene(_rc()),
    "test_scene_environment": lambda: scenes.create_test_scene_with_environment(_rc(), size=(16, 8)),
    "bvh_test_scene_flat": lambda: scenes.new_bvh_test_scene(_rc(), False, 40),
    "bvh_test_scene_nested": lambda: scenes.new_bvh_test_scene(_rc(), True, 40),
}
PRODUCERS.update({f"ref_{name}": (lambda f=f: f(1)) for name, f, *_ in CASES})
PRODUCERS.update({f"random_{s}": (lambda s=s: random_scene(s)) for s in range(6)})
PRODUCERS.update({f"needles_{s}": (lambda s=s: needle_scene(s)) for s in range(3)})
PRODUCERS.update({f"obj_{f}": (lambda f=f: scenes.create_obj_with_box(_rc(), f)) for f in ("box.obj", "boxWithMat.obj")})
PRODUCERS.update({f"obj_{f}": (lambda f=f: scenes.create_obj_with_triangle(_rc(), f)) for f in ("triWithNormalMap.obj", "triWithHeightMap.obj")})


def _codes(lib, sc):
    """(sol_scene_create, sol_world_tree_check_ex, sol_background_blocks); a created scene is destroyed at once."""
    h = C.c_void_p()
    rc = lib.sol_scene_create(sc.desc_ptr, 0, C.byref(h))
    if rc == _abi.SOL_OK:
        lib.sol_scene_destroy(h)
    err = lib.sol_last_error() if rc != _abi.SOL_OK else b""
    chk = _abi.SolTreeCheck()
    rc_chk = lib.sol_world_tree_check_ex(sc.desc_ptr, 0, C.byref(chk), C.sizeof(chk))
    nb = ((sc.desc.width + 7) // 8) * ((sc.desc.height + 7) // 8)
    flags = (C.c_uint8 * nb)()
    n = C.c_uint32()
    rc_bg = lib.sol_background_blocks(sc.desc_ptr, 0, flags, nb, C.byref(n))
    return (rc, rc_chk, rc_bg), err, chk


def _accepted(codes):
    """Accepted by the validation: created (a GPU), or refused only for want of one (SOL_EDEVICE), and both diagnostics OK."""
    return codes[0] in (_abi.SOL_OK, _abi.SOL_EDEVICE) and codes[1] == _abi.SOL_OK and codes[2] == _abi.SOL_OK


def _assert_refused(lib, sc, what):
    """All three entry points return SOL_EINVAL, each naming a record whose number is wrong, with the value found and the one expected."""
    want = du.tree_numbering(sc.desc)
    calls = (lambda: lib.sol_scene_create(sc.desc_ptr, 0, C.byref(C.c_void_p())),
             lambda: lib.sol_world_tree_check_ex(sc.desc_ptr, 0, C.byref(_abi.SolTreeCheck()), C.sizeof(_abi.SolTreeCheck)),
             lambda: lib.sol_background_blocks(sc.desc_ptr, 0, None, 0, C.byref(C.c_uint32())))
    for name, call in zip(("sol_scene_create", "sol_world_tree_check_ex", "sol_background_blocks"), calls):
        rc = call()
        err = lib.sol_last_error()
        assert rc == _abi.SOL_EINVAL, (what, name, rc, err)
        m = MESSAGE.search(err)
        assert m, (what, name, err)
        kind, index, have, expected = KIND_OF_NAME[m.group(1)], int(m.group(2)), int(m.group(3)), int(m.group(4))
        assert du.get_dfs(sc.desc, kind, index) == have and want[(kind, index)] == expected != have, (what, name, err)


@pytest.fixture(scope="module")
def lib():
    return _abi.load_hip()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", list(PRODUCERS))
def test_every_in_tree_producer_passes(lib, name):
    """Every scene factory the suite and bench.py use numbers its records as the check wants (the host's Flattener, through SceneBuilder,
    the OBJ loader, nested Bvh, mediums and their boundaries): the check refuses no real scene. The restatement in dfs_util agrees."""
    sc = PRODUCERS[name]()
    want = du.tree_numbering(sc.desc)
    assert want and all(du.get_dfs(sc.desc, k, i) == v for (k, i), v in want.items())
    codes, err, _ = _codes(lib, sc)
    assert _accepted(codes), (codes, err)


def _base_scenes():
    rc = _rc()
    return {"cornell": scenes.cornell_box(rc), "test_scene": scenes.create_test_scene(rc), "obj_box": scenes.create_obj_with_box(rc, "box.obj"),
            "needles": needle_scene(1, 24, 16, 1)}


@pytest.fixture(scope="module")
def bases():
    return _base_scenes()


def _refusal_cases(desc, rng):
    """(label, {(kind, index): new value}) per kind of wrong numbering, on records the walk reaches."""
    want = du.tree_numbering(desc)
    recs = sorted(want, key=lambda r: want[r])
    a, b = (recs[i] for i in rng.choice(len(recs), 2, replace=False))
    one = recs[int(rng.integers(len(recs)))]
    cases = [("duplicate", {b: want[a]}),
             ("swap", {a: want[b], b: want[a]}),
             ("bit_31", {one: want[one] | 0x80000000}),
             ("unknown", {one: 0xFFFFFFFF}),
             ("shifted", {r: want[r] + 1 for r in recs}),
             ("first_and_last", {recs[0]: want[recs[-1]], recs[-1]: want[recs[0]]})]
    for m in range(desc.n_mediums):
        if (_abi.REF_MEDIUM, m) in want:
            first = next(r for r in recs if want[r] == want[(_abi.REF_MEDIUM, m)] + 1)  # the boundary's first primitive
            cases.append((f"medium_{m}_with_its_boundary", {(_abi.REF_MEDIUM, m): want[first], first: want[(_abi.REF_MEDIUM, m)]}))
    return cases


@pytest.mark.parametrize("name", BASES)
def test_wrong_numberings_are_refused_by_every_entry_point(lib, bases, name):
    sc = bases[name]
    rng = np.random.default_rng(7)
    cases = _refusal_cases(sc.desc, rng)
    assert name != "test_scene" or any(c[0].startswith("medium") for c in cases)
    for label, change in cases:
        old = {r: du.get_dfs(sc.desc, *r) for r in change}
        for r, v in change.items():
            du.set_dfs(sc.desc, *r, v)
        try:
            _assert_refused(lib, sc, label)
        finally:
            for r, v in old.items():
                du.set_dfs(sc.desc, *r, v)
        codes, err, _ = _codes(lib, sc)
        assert _accepted(codes), (label, codes, err)  # (nothing of the refused descriptor stays behind)


def test_a_shared_subtree_is_numbered_by_its_last_visit(lib):
    """A sub-tree referenced from two nodes is walked twice; the float oracle lets the later of two equal hits win, so its records carry the
    number of their LAST visit (dfs_util.shared_subtree_scene; the GPU test below renders it against the oracle). First-visit numbering,
    otherwise unique and in range, is refused."""
    last = du.shared_subtree_scene(_rc(32, 24))
    assert du.visit_order(last.desc) == [(_abi.REF_QUAD, last.red_quad), (_abi.REF_QUAD, 1 - last.red_quad), (_abi.REF_SPHERE, 0),
                                         (_abi.REF_QUAD, last.red_quad)]
    codes, err, chk = _codes(lib, last)
    assert _accepted(codes), (codes, err)
    assert chk.leaf_mismatches == 0 and chk.box_violations == 0
    _assert_refused(lib, du.shared_subtree_scene(_rc(32, 24), rule="first"), "first visit")


def test_a_long_chain_of_shared_subtrees_is_checked_in_linear_time(lib):
    """Sixty nodes, each referencing the next one twice: the walk visits the quad at the bottom 2^60 times. The check must neither follow
    the visits one by one nor wrap its counts: the numbers run past 2^31 and the descriptor is refused, at once."""
    sc = du.shared_subtree_scene(_rc(32, 24))
    d = sc.desc
    depth = 60
    nodes = (_abi.SolBvhNode * (depth + 1))()
    for i in range(depth):
        nodes[i] = _abi.SolBvhNode(d.nodes[0].bbox, du.ref(_abi.REF_NODE, i + 1), du.ref(_abi.REF_NODE, i + 1))
    nodes[depth] = _abi.SolBvhNode(d.nodes[0].bbox, du.ref(_abi.REF_QUAD, 0), du.ref(_abi.REF_SPHERE, 0))
    sc._keep.append(nodes)
    d.nodes, d.n_nodes, d.root = C.cast(nodes, C.POINTER(_abi.SolBvhNode)), depth + 1, du.ref(_abi.REF_NODE, 0)
    for call in (lambda: lib.sol_world_tree_check_ex(sc.desc_ptr, 0, C.byref(_abi.SolTreeCheck()), C.sizeof(_abi.SolTreeCheck)),
                 lambda: lib.sol_background_blocks(sc.desc_ptr, 0, None, 0, C.byref(C.c_uint32())),
                 lambda: lib.sol_scene_create(sc.desc_ptr, 0, C.byref(C.c_void_p()))):
        assert call() == _abi.SOL_EINVAL
        assert b"beyond 2^31" in lib.sol_last_error(), lib.sol_last_error()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", BASES)
def test_seeded_dfs_only_campaign(lib, bases, name):
    """Single-record changes of dfs_index alone (seeded; its own stream, so test_desc_mutations' campaign stays as it was): a reachable
    record takes another reachable record's value, a random u32, or its own value +- 1 - never its own. Every one is refused by all three
    entry points, and the untouched descriptor is accepted afterwards."""
    sc = bases[name]
    want = du.tree_numbering(sc.desc)
    recs = sorted(want)
    rng = np.random.default_rng(CAMPAIGN_SEED + BASES.index(name) + 1000 * SEED_SHIFT)
    for _ in range(max(50, N_MUTATIONS // 4)):
        r = recs[int(rng.integers(len(recs)))]
        old = want[r]
        how = int(rng.integers(3))
        if how == 0:
            other = recs[int(rng.integers(len(recs)))]
            new = want[other] if other != r else old + 1
        elif how == 1:
            new = int(rng.integers(0, 1 << 32))
        else:
            new = old + 1 if rng.integers(2) or old == 0 else old - 1
        if new == old:
            new = old ^ 1
        new &= 0xFFFFFFFF
        du.set_dfs(sc.desc, *r, new)
        try:
            _assert_refused(lib, sc, f"{du.KIND_NAMES[r[0]]} {r[1]}: {old} -> {new}")
        finally:
            du.set_dfs(sc.desc, *r, old)
    codes, err, _ = _codes(lib, sc)
    assert _accepted(codes), (codes, err)


@pytest.mark.parametrize("size", [TREE_CHECK_V1_BYTES, C.sizeof(_abi.SolTreeCheck)])
def test_a_refused_tree_check_writes_zeros(lib, bases, size):
    """sol_world_tree_check_ex copies its result to the caller also when it refuses: zeros, never the stack's leftovers (the first layout's
    size and the full one; a null descriptor is refused before anything is computed, a misnumbered one after the tree is resolved)."""
    sc = bases["cornell"]
    q = (_abi.REF_QUAD, 0)
    old = du.get_dfs(sc.desc, *q)
    for desc in (None, sc.desc_ptr):
        buf = (C.c_uint8 * size)(*([0xA5] * size))
        du.set_dfs(sc.desc, *q, old + 7)
        try:
            rc = lib.sol_world_tree_check_ex(desc, 0, buf, size)
        finally:
            du.set_dfs(sc.desc, *q, old)
        assert rc == _abi.SOL_EINVAL and bytes(buf) == bytes(size), (desc is None, rc, bytes(buf))


# ---- GPU: what the check accepts but the host never emits ------------------------------------------------------------------------

def _render(scene, spp, world_tree):
    with DeviceScene(scene, world_tree=world_tree) as ds:
        ds.render(0, spp, pu.SEED)
        return ds.read()


def _assert_oracle(img, scene, spp):
    ref, _ = orc.render(scene, 0, spp, pu.SEED, real=orc.ORC_F32)
    res = pu.compare(img, ref, spp)
    assert np.isfinite(img).all() and res["bad_pixels"] == 0 and res["max_rel"] <= pu.REL_TOL and res["rmse_mean_good"] < 1e-5, res
    return ref


SHUFFLED = {
    "c1_cornell": lambda: scenes.cornell_box(_rc(96, 96, 8)),
    "test_scene": lambda: scenes.create_test_scene(_rc(128, 64, 8)),  # mediums, three kinds of light, an image texture
    "random_5": lambda: random_scene(5, 96, 72, 8),  # blend materials, a constant medium, quad and triangle lights
    "c3_sponza": lambda: scenes.sponza_like(_rc(128, 72, 4), n_triangles=20000, texture_size=64),
}


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", list(SHUFFLED))
def test_record_order_is_not_dfs_order(name):
    """The sphere, quad and triangle tables shuffled, every node, light and medium-boundary reference remapped, dfs_index travelling with
    its record: the same world listed in another order. The device frame must be the unshuffled one bit for bit, for the reference's
    topology and for the device-built tree, and match the oracle - the renderer uses dfs_index, never an array position, where order
    matters."""
    sc = SHUFFLED[name]()
    spp = sc.render_config.samples_per_pixel
    mixed = du.shuffled(sc, seed=list(SHUFFLED).index(name) + 1)
    d, m = sc.desc, mixed.desc
    assert any(du.get_dfs(d, k, i) != du.get_dfs(m, k, i) for (k, i) in du.tree_numbering(d))  # (the order did change)
    assert all(du.get_dfs(m, k, i) == v for (k, i), v in du.tree_numbering(m).items())
    for tree in (_abi.TREE_REF, _abi.TREE_DEVICE):
        a, b = _render(sc, spp, tree), _render(mixed, spp, tree)
        assert np.array_equal(a, b), (tree, int((a != b).any(axis=-1).sum()))
    _assert_oracle(b, mixed, spp)


@pytest.mark.gpu
def test_a_shared_subtree_decides_its_tie_by_its_last_visit():
    """dfs_util.shared_subtree_scene: red quad A under a sub-tree walked before and after the coincident white quad B. The oracle lets the
    later hit win (A's second visit), and so does the device with A numbered by that visit: device and oracle agree and red shows wherever
    the quads are seen - through the Albedo shader and the path tracer. (Before the check, A numbered by its first visit was accepted and
    1 210 of 6 144 pixels differed from the oracle; now it is refused.)"""
    spp = 4
    sc = du.shared_subtree_scene(_rc(96, 64, spp, AlbedoShader()))
    img = _render(sc, spp, _abi.TREE_AUTO)
    ref = _assert_oracle(img, sc, spp)
    red, white = np.array([1., 0., 0.]) * spp, np.array([.9, .9, .9]) * spp
    inside = np.abs(ref - red).max(axis=-1) < 1e-5
    assert inside.sum() > 1000 and np.allclose(img[inside], red, atol=1e-5)
    assert not (np.abs(img - white).max(axis=-1) < 1e-5).any()
    path = du.shared_subtree_scene(_rc(96, 64, 8))
    for tree in (_abi.TREE_REF, _abi.TREE_DEVICE):
        _assert_oracle(_render(path, 8, tree), path, 8)
    with pytest.raises(DeviceError, match="dfs_index"):
        DeviceScene(du.shared_subtree_scene(_rc(96, 64, spp, AlbedoShader()), rule="first"))
