"""sol_scene_set_primitives: a live handle gets new places for its spheres and quads - the lights among them - and its triangles,
any kinds in one call. After the move every output - frame, auxiliary planes, camera rays, closest hits, the sphere and quad records read back
through sol_scene_primitive_records, the light tables and the light tree - is byte-identical to a handle freshly created from D'
(tests/primitive_util.py: every moved primitive made again by its CPU constructor, every node box the union of its children's); the closest hits
are also the float oracle's on D', bit for bit - the probe for a refitted box that fails to contain its primitive. Sequences do not accumulate,
the order with sol_scene_set_camera does not matter, options, modes and the partition are kept, a refused call leaves the handle - and what the
next partial move refits over - as it was, and the background blocks proved over the refitted tree are sound.

No pixel and no ray is left out and equality is over all bytes: the scenes have no ties that depend on the tree, because a moved handle keeps
creation's dfs_index numbers and the fresh handle of D' carries the same numbers (the tie rule).

Frames are 128x96 at 16 spp."""
import ctypes as C

import numpy as np
import pytest

import orc
import parity_util as pu
import primitive_util as prim
from solstrale_amd import CameraConfig, DeviceError, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, background_blocks, quad_from_corner, scenes
from test_gpu_set_triangles import _mesh_scene

pytestmark = pytest.mark.gpu

SEED = pu.SEED
SPP = 16
RC = RenderConfig(128, 96, SPP, PathTracingShader(8))
MOVES = ("identity", "light", "jitter_spheres", "all", "each", "scale")
KINDS = ("triangles", "spheres", "quads")
HIT = _abi.SOL_RAY_HIT


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _three_lights():
    """A sphere light and two quad lights of different size over a floor with a few spheres on it."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    world = [b.Quad((-4., 0., -4.), (8., 0., 0.), (0., 0., 8.), grey), b.Quad((-4., 0., -4.), (8., 0., 0.), (0., 5., 0.), grey)]
    world += [b.Sphere((-2. + 1.3 * k, .5 + .1 * k, .3 * k - 1.), .5 + .05 * k, b.Lambertian(b.SolidColor(.3 + .1 * k, .5, .7 - .1 * k))) for k in range(4)]
    world.append(b.Sphere((2.5, 3.2, 1.), .4, b.DiffuseLight(12., 10., 8.)))
    world.append(b.Quad((-3., 4., -1.), (1.5, 0., 0.), (0., 0., 1.5), b.DiffuseLight(6., 7., 9.)))
    world.append(b.Quad((0., 4.5, -2.), (.5, 0., 0.), (0., .1, .6), b.DiffuseLight(20., 18., 15.)))
    return b.finish(b.Bvh(world), CameraConfig(45., 0., (0., 3., 10.), (0., 1.5, 0.), (0., 1., 0.)), (.05, .06, .1), RC)


class _WithOutsideLight:
    """The Cornell box with one more quad light that is in lights[] and in the quad array but under no node of the world: it lights the box through
    its front opening, no ray ever hits it, and it has a device record that is no part of the root's box."""

    def __init__(self):
        self._scene = scenes.cornell_box(RC)
        d0 = self._scene.desc
        self.render_config = self._scene.render_config
        self.desc = _abi.SolSceneDesc.from_buffer_copy(d0)
        self._quads = (_abi.SolQuad * (d0.n_quads + 1))()
        C.memmove(self._quads, d0.quads, C.sizeof(_abi.SolQuad) * d0.n_quads)
        lamp = d0.quads[_abi.ref_index(d0.lights[0])]
        extra = self._quads[d0.n_quads]
        extra.material, extra.dfs_index = lamp.material, 0x0FFFFFF0
        quad_from_corner((200., 100., -300.), (150., 0., 0.), (0., 120., 30.), out=extra)
        self._lights = (C.c_uint32 * (d0.n_lights + 1))(*[d0.lights[i] for i in range(d0.n_lights)], (_abi.REF_QUAD << 28) | d0.n_quads)
        self.desc.quads, self.desc.n_quads = C.cast(self._quads, C.POINTER(_abi.SolQuad)), d0.n_quads + 1
        self.desc.lights, self.desc.n_lights = C.cast(self._lights, C.POINTER(C.c_uint32)), d0.n_lights + 1
        self.desc_ptr = C.pointer(self.desc)
        self.width, self.height = int(d0.width), int(d0.height)


def _two_spheres():
    b = SceneBuilder()
    world = [b.Sphere((0., 0., 0.), 1.5, b.Lambertian(b.SolidColor(.6, .6, .6))), b.Sphere((1., 4., 1.), 1., b.DiffuseLight(8., 8., 8.))]
    return b.finish(b.Bvh(world), CameraConfig(40., 0., (0., 2., 12.), (0., 1.5, 0.), (0., 1., 0.)), (.2, .3, .5), RC)


def _sphere_chain(n=120):
    """A Bvh nested n levels deep, a sphere per level: under SOL_BVH=ref the 7-wide tree has many levels - one refit launch each - and its
    searches use the spill stack."""
    b = SceneBuilder()
    m = b.Lambertian(b.SolidColor(.8, .8, .8))
    ids = [b.Sphere((float(x), 0.3 * (x % 3), 0.), 0.45, m) for x in range(n)]
    inner = b.Bvh(ids[:2])
    for k in range(2, n):
        inner = b.Bvh([inner, ids[k]]) if k % 2 else b.Bvh([ids[k], inner])
    light = b.Sphere((0., 1e4, 0.), 3e3, b.DiffuseLight(3, 3, 3))
    return b.finish(b.Bvh([inner, light]), CameraConfig(12., 0., (-30., 0.4, 0.3), (50., 0.3, 0.), (0, 1, 0)), (.1, .1, .1), RC)


_LENS = CameraConfig(40., 0.25, (0., 4., 10.), (0., 1., 0.), (0., 1., 0.))
# name -> (maker, creation arguments, environment variables, light sampling mode)
_SCENES = {
    "cornell": (lambda: scenes.cornell_box(RC), {}, {}, None),
    "cornell_ref": (lambda: scenes.cornell_box(RC), dict(world_tree=_abi.TREE_REF), {}, None),
    "cornell_sah16": (lambda: scenes.cornell_box(RC), dict(world_tree=_abi.TREE_SAH16), {}, None),
    "spheres300": (lambda: scenes.cornell_spheres(RC, 300), {}, {}, None),
    "mesh": (_mesh_scene, {}, {}, None),
    "lights_uniform": (_three_lights, {}, {}, "uniform"),
    "lights_tree": (_three_lights, {}, {}, "tree"),
    "lights_power": (_three_lights, {}, {}, "power"),
    "outside": (_WithOutsideLight, {}, {}, None),
    "thinlens": (lambda: _mesh_scene(camera=_LENS), {}, {}, None),
    "environment": (lambda: _mesh_scene(environment=True), {}, {}, None),
    "twospheres": (_two_spheres, {}, {}, None),
    "chain": (_sphere_chain, {}, {"SOL_BVH": "ref"}, None),
}
_cache = {}


def _base(name):
    """Scenes that differ only in how the handle is created share the description, D' and the oracle's answers."""
    return name.split("_")[0]


def _scene(name):
    if _base(name) not in _cache:
        sc = _SCENES[name][0]()
        _cache[_base(name)] = (sc, prim.rows_of(sc.desc))
    return _cache[_base(name)]


def _plan(name, move):
    """The calls of a move: a list of dict(kind -> rows), and the rows the handle holds after the last one."""
    sc, rows = _scene(name)
    if move == "identity":
        return [dict(rows)], rows
    if move == "light":
        new, kinds = prim.light_moved(sc.desc, rows)
        return [{k: new[k] for k in kinds}], new
    if move == "jitter_spheres":
        new = dict(rows, spheres=prim.jitter(rows, 5)["spheres"])
        return [dict(spheres=new["spheres"])], new
    if move == "all":
        new = prim.jitter(rows, 7)
        return [dict(new)], new
    if move == "each":
        new = prim.jitter(rows, 9)
        return [{k: new[k]} for k in KINDS], new
    if move == "scale":
        new = prim.scale(rows, 1.5)
        return [dict(new)], new
    raise ValueError(move)


def _moved(name, move):
    key = (_base(name), move)
    if key not in _cache:
        calls, new = _plan(name, move)
        _cache[key] = (calls, new, prim.MovedScene(_scene(name)[0], **new))
    return _cache[key]


def _open(name, sc, dynamic, monkeypatch, **more):
    _, create, env, mode = _SCENES[name]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    ds = DeviceScene(sc, dynamic_primitives=dynamic, **create, **more)
    if mode:
        ds.light_sampling(mode)
    return ds


def _random_rays(rows, n=4097, seed=11):
    rng = np.random.default_rng(seed)
    p = prim.targets_of(rows)  # (the far light of the chain is no target)
    lo, hi = p.min(axis=0) - 1., p.max(axis=0) + 1.
    r = np.empty((n, 8), dtype=np.float32)
    r[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    r[:, 3] = 0.001
    aim = p[rng.integers(0, len(p), n)] + rng.normal(size=(n, 3)) * 0.05   # most rays pass near a corner: boxes are grazed
    r[:, 4:7] = np.where(rng.random((n, 1)) < 0.7, aim - r[:, 0:3], rng.normal(size=(n, 3)))
    r[:, 7] = np.inf
    return r


def _outputs(ds, rays):
    ds.clear()
    ds.clear_aux()
    ds.render(0, SPP, SEED)
    frame = ds.read()
    ds.render_aux(0, SPP, SEED)
    albedo, normal = ds.read_aux()
    cam = ds.camera_rays(0, 0, ds.width, ds.height, 3, SEED).cpu().numpy()
    hits = ds.closest_hits(np.concatenate([cam.reshape(-1, 8), rays]))
    return dict(frame=frame, albedo=albedo, normal=normal, camera_rays=cam, t=hits["t"].copy(), status=hits["status"].copy(),
                dfs_index=hits["dfs_index"].copy(), material=hits["material"].copy())


def _records(ds):
    """The sphere and quad records by the caller's index (the device order is each tree's own)."""
    out = {}
    for kind in ("sphere", "quad"):
        rec, of = ds.primitive_records(kind)
        assert sorted(of.tolist()) == list(range(len(of)))
        out[kind] = rec[np.argsort(of)]
    return out


def _light_tables(ds):
    """Mode 2's q, C and W and the light tree's boxes (the handle is left in the power mode: call it last)."""
    ds.light_sampling("power")
    q, cdf, total = ds.light_tables()
    nodes, first, _ = ds.light_tree()
    return dict(q=q, cdf=cdf, total=np.float64(total), tree=nodes, first_leaf=np.uint32(first))


def _same(got, want, what):
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k, int((g.view(np.uint8) != w.view(np.uint8)).sum()))


def _oracle_hits(sc, rays):
    lib = orc.load()
    n = len(rays)
    status, t, mat = np.zeros(n, np.uint32), np.full(n, np.inf, np.float32), np.zeros(n, np.uint32)
    o, d, tt, mm = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(), C.c_uint32()
    for i, r in enumerate(rays):
        o[:], d[:] = [float(x) for x in r[0:3]], [float(x) for x in r[4:7]]
        if lib.orc_closest_hit(sc.desc_ptr, orc.ORC_F32, o, d, C.byref(tt), C.byref(mm)):
            status[i], t[i], mat[i] = HIT, np.float32(tt.value), mm.value
    return status, t, mat


def _apply(ds, calls, **kw):
    for call in calls:
        ds.set_primitives(**call, **kw)


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", list(_SCENES))
def test_a_moved_handle_is_a_fresh_handle_of_the_moved_description(name, move, monkeypatch):
    sc, rows = _scene(name)
    calls, new, moved = _moved(name, move)
    rays = _random_rays(new)
    with _open(name, moved, False, monkeypatch) as fresh:
        want = _outputs(fresh, rays)
        want_info, want_rec, want_tables = fresh.info(), _records(fresh), _light_tables(fresh)
    with _open(name, sc, True, monkeypatch) as ds:
        info = ds.info()
        if name == "spheres300":
            assert info["stack_bound"] >= 2 * 3 + 2, info   # at least three levels of wide nodes (2 dwords a level + 2)
        if name == "chain":
            assert info["tree_name"] == "ref" and info["stack_bound"] > info["lds_stack"], info
        ds.render(0, SPP, SEED)  # (sums, a table and costs of the old geometry are there to be dropped)
        _apply(ds, calls)
        got = _outputs(ds, rays)
        _same(got, want, (name, move))
        assert ds.info()["strict_triangles"] == want_info["strict_triangles"]
        _same(_records(ds), want_rec, (name, move, "records"))
        _same(_light_tables(ds), want_tables, (name, move, "light tables"))
    # the float oracle on D': every camera ray of the frame and the random rays
    all_rays = np.concatenate([want["camera_rays"].reshape(-1, 8), rays])
    okey = (_base(name), move, "oracle")
    if okey not in _cache:
        _cache[okey] = _oracle_hits(moved, all_rays)
    status, t, mat = _cache[okey]
    assert 0.02 < (status == HIT).mean() <= 1.0
    assert (got["status"] == status).all(), int((got["status"] != status).sum())
    assert got["t"].view(np.uint32).tobytes() == t.view(np.uint32).tobytes(), int((got["t"].view(np.uint32) != t.view(np.uint32)).sum())
    assert (got["material"][status == HIT] == mat[status == HIT]).all()


def test_records_are_the_cpu_constructors_casts(monkeypatch):
    """Device records against sol_sphere_from_center / sol_quad_from_corner directly, as float casts of the CPU functions' f64 fields (the cast
    is numpy's here, not the library's)."""
    from solstrale_amd import sphere_from_center
    sc, rows = _scene("lights_uniform")
    calls, new, _ = _moved("lights_uniform", "all")
    with _open("lights_uniform", sc, True, monkeypatch) as ds:
        _apply(ds, calls)
        rec = _records(ds)
    f32 = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32)
    for i, r in enumerate(rec["sphere"]):
        s = sphere_from_center(new["spheres"][i, :3], new["spheres"][i, 3])
        assert r["c"].tobytes() == f32(s.center[:]).tobytes() and r["radius"] == abs(np.float32(s.radius))
        assert r["dfs"] == sc.desc.spheres[i].dfs_index and r["mat"] == sc.desc.spheres[i].material and not r["pad"].any()
    for i, r in enumerate(rec["quad"]):
        q = quad_from_corner(*new["quads"][i])
        for f, src in (("n", q.normal), ("q", q.q), ("w", q.w), ("u", q.u), ("v", q.v)):
            assert r[f].tobytes() == f32(src[:]).tobytes(), (i, f)
        assert r["d"] == np.float32(q.d) and r["area"] == np.float32(q.area) and r["pad"] == 0
        assert r["dfs"] == sc.desc.quads[i].dfs_index and r["mat"] == sc.desc.quads[i].material


def test_the_host_route_and_the_device_route_give_the_same_bytes(monkeypatch):
    import torch
    sc, rows = _scene("mesh")
    calls, new, moved = _moved("mesh", "all")
    rays = _random_rays(new, 257)
    with _open("mesh", sc, True, monkeypatch) as ds:
        _apply(ds, calls)
        want, want_rec = _outputs(ds, rays), _records(ds)
        ds.set_primitives(**prim.scale(rows, 1.2))
        dev = f"cuda:{ds.device}"
        ds.set_primitives(**{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in new.items()})
        _same(_outputs(ds, rays), want, "device route")
        _same(_records(ds), want_rec, "device route records")
        with pytest.raises(ValueError, match="one call"):
            ds.set_primitives(spheres=new["spheres"], quads=torch.from_numpy(new["quads"]).to(dev))


# ---- sequences, order, partition, sessions, neutrality ------------------------------------------------------------------------------------
def test_a_sequence_returns_to_where_it_started(monkeypatch):
    """A -> B -> A equals fresh A: nothing accumulates in the boxes or the records."""
    sc, rows = _scene("spheres300")
    calls_a, new_a, moved_a = _moved("spheres300", "all")
    rays = _random_rays(new_a, 513)
    with _open("spheres300", moved_a, False, monkeypatch) as fresh:
        want = _outputs(fresh, rays)
    with _open("spheres300", sc, True, monkeypatch) as ds:
        for move in ("all", "scale", "all"):
            _apply(ds, _moved("spheres300", move)[0])
            ds.render(0, SPP, SEED)
        _same(_outputs(ds, rays), want, "sequence")


def test_the_order_with_set_camera_does_not_matter(monkeypatch):
    cam_b = CameraConfig(50., 0., (6., 5., 7.), (0., 1., 0.), (0., 1., 0.))
    sc, rows = _scene("mesh")
    calls, new, moved = _moved("mesh", "all")
    rays = _random_rays(new, 513)
    with _open("mesh", moved, False, monkeypatch) as fresh:
        fresh.set_camera(cam_b)
        want = _outputs(fresh, rays)
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_camera(cam_b)
        _apply(ds, calls)
        _same(_outputs(ds, rays), want, "camera first")
    with _open("mesh", sc, True, monkeypatch) as ds:
        _apply(ds, calls)
        ds.set_camera(cam_b)
        _same(_outputs(ds, rays), want, "camera last")


def test_the_partition_survives_a_move(monkeypatch):
    """Rank 1 of 2."""
    sc, rows = _scene("spheres300")
    calls, new, moved = _moved("spheres300", "all")
    with _open("spheres300", moved, False, monkeypatch) as fresh:
        fresh.set_partition(1, 2)
        fresh.render(0, SPP, SEED)
        want, want_crc = fresh.read(), fresh.info()["partition_crc"]
    with _open("spheres300", sc, True, monkeypatch) as ds:
        ds.set_partition(1, 2)
        ds.render(0, SPP, SEED)
        with pytest.raises(DeviceError) as e:
            ds.set_primitives(spheres=new["spheres"], reprobe=True)
        assert e.value.code == _abi.SOL_EINVAL and "world" in e.value.msg
        _apply(ds, calls)
        ds.render(0, SPP, SEED)
        assert ds.info()["partition_crc"] == want_crc and ds.read().tobytes() == want.tobytes()


def test_sums_and_sessions_are_reset_and_adaptive_rounds_are_the_fresh_handles(monkeypatch):
    sc, rows = _scene("cornell")
    calls, new, moved = _moved("cornell", "light")

    def rounds(ds):
        ds.adaptive_begin(16, 16, 32, 0.05)
        n = ds.adaptive_run(SEED)
        return n, ds.read(), ds.adaptive_counts()

    with _open("cornell", moved, False, monkeypatch) as fresh:
        want = rounds(fresh)
    with _open("cornell", sc, True, monkeypatch) as ds:
        ds.render(0, SPP, SEED)
        ds.render_aux(0, SPP, SEED)
        ds.adaptive_begin(16, 16, 32, 0.05)
        assert ds.adaptive_round(SEED) > 0
        _apply(ds, calls)
        assert not ds.read().any() and not ds.read_aux()[0].any() and ds.resolve_aux()[2] == 0
        with pytest.raises(DeviceError) as e:
            ds.adaptive_round(SEED)
        assert e.value.code == _abi.SOL_EINVAL and "no adaptive session" in e.value.msg
        got = rounds(ds)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and (got[2] == want[2]).all()


@pytest.mark.parametrize("name", ["spheres300", "mesh"])
def test_the_option_alone_changes_no_byte(name, monkeypatch):
    sc, rows = _scene(name)
    rays = _random_rays(rows, 513)
    with _open(name, sc, False, monkeypatch) as plain:
        want, want_rec = _outputs(plain, rays), _records(plain)
        want_flags = plain.background_flags()
    with _open(name, sc, True, monkeypatch) as ds:
        _same(_outputs(ds, rays), want, "option on, never moved")
        _same(_records(ds), want_rec, "records")
        assert (ds.background_flags() == want_flags).all()


def test_a_handle_with_dynamic_triangles_alone_moves_triangles_only(monkeypatch):
    sc, rows = _scene("mesh")
    calls, new, _ = _moved("mesh", "all")
    moved = prim.MovedScene(sc, triangles=new["triangles"])
    rays = _random_rays(rows, 513)
    with _open("mesh", moved, False, monkeypatch) as fresh:
        want = _outputs(fresh, rays)
    with DeviceScene(sc, dynamic_triangles=True) as ds:
        for kind in ("spheres", "quads"):
            with pytest.raises(DeviceError) as e:
                ds.set_primitives(**{kind: new[kind]})
            assert e.value.code == _abi.SOL_EINVAL and "dynamic_primitives" in e.value.msg
        with pytest.raises(DeviceError) as e:
            ds.set_primitives(triangles=new["triangles"], spheres=new["spheres"])
        assert e.value.code == _abi.SOL_EINVAL and "dynamic_primitives" in e.value.msg
        ds.set_primitives(triangles=new["triangles"])
        _same(_outputs(ds, rays), want, "a triangles-only set")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_move_leaves_the_handle_as_it_was(monkeypatch):
    """After EACH refusal the sums are untouched and the next outputs (frame, auxiliary planes, camera rays, hits, records) are an untouched twin's."""
    sc, rows = _scene("mesh")
    calls, new, _ = _moved("mesh", "all")
    rays = _random_rays(new, 513)
    with _open("mesh", sc, True, monkeypatch) as twin:
        _apply(twin, calls)
        want, want_rec = _outputs(twin, rays), _records(twin)
        want_flags = twin.background_flags()
    nan_centre = new["spheres"].copy()
    nan_centre[0, 1] = np.nan
    inf_radius = new["spheres"].copy()
    inf_radius[0, 3] = np.inf
    far_quad = new["quads"].copy()
    far_quad[1, 0, 2] = 1e12
    big = prim.scale(new, 8.0)
    with _open("mesh", sc, True, monkeypatch) as ds:
        _apply(ds, calls)
        for call, code, word in ((dict(spheres=nan_centre), _abi.SOL_EINVAL, "finite"), (dict(spheres=inf_radius, quads=new["quads"]), _abi.SOL_EINVAL, "finite"),
                                 (dict(quads=far_quad), _abi.SOL_EINVAL, "2^38"), (dict(spheres=new["spheres"][:0]), _abi.SOL_EINVAL, "rows"),
                                 (dict(quads=np.concatenate([new["quads"], new["quads"][:1]])), _abi.SOL_EINVAL, "rows"), (dict(big), _abi.SOL_ERANGE, "re-create")):
            ds.clear()
            ds.render(0, SPP, SEED)
            sums = ds.read()
            with pytest.raises(DeviceError) as e:
                ds.set_primitives(**call)
            assert e.value.code == code and word in e.value.msg, (code, e.value.code, e.value.msg)
            assert ds.read().tobytes() == sums.tobytes()  # no sums cleared
            assert (ds.background_flags() == want_flags).all()
            _same(_outputs(ds, rays), want, ("after the refusal", word))
            _same(_records(ds), want_rec, ("records after the refusal", word))
    # a scene with a constant medium (queries refuse it too: frame and auxiliary planes)
    med = scenes.create_test_scene(RC)
    assert med.desc.n_mediums > 0

    def frames(d):
        d.clear()
        d.clear_aux()
        d.render(0, SPP, SEED)
        d.render_aux(0, SPP, SEED)
        return dict(zip(("frame", "albedo", "normal"), (d.read(),) + tuple(d.read_aux())))

    with DeviceScene(med, dynamic_primitives=True) as twin:
        want = frames(twin)
    with DeviceScene(med, dynamic_primitives=True) as ds:
        ds.render(0, SPP, SEED)
        sums = ds.read()
        with pytest.raises(DeviceError) as e:
            ds.set_primitives(spheres=prim.rows_of(med.desc)["spheres"])
        assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        assert ds.read().tobytes() == sums.tobytes()
        _same(frames(ds), want, "medium")


def test_a_refused_triangle_move_does_not_reach_the_next_spheres_only_move(monkeypatch):
    """The partial-update trap: the refused call's triangle boxes must not be what the next call refits over, nor its share of S."""
    sc, rows = _scene("mesh")
    calls, new, _ = _moved("mesh", "all")
    moved = prim.MovedScene(sc, spheres=new["spheres"])  # old triangles, new spheres
    rays = _random_rays(rows, 513)
    with _open("mesh", moved, False, monkeypatch) as fresh:
        want, want_rec = _outputs(fresh, rays), _records(fresh)
    with _open("mesh", sc, True, monkeypatch) as ds:
        with pytest.raises(DeviceError) as e:
            ds.set_primitives(triangles=prim.scale(rows, 8.0)["triangles"])
        assert e.value.code == _abi.SOL_ERANGE
        ds.set_primitives(spheres=new["spheres"])
        _same(_outputs(ds, rays), want, "old triangles, new spheres")
        _same(_records(ds), want_rec, "records")


def test_a_refused_spheres_move_does_not_reach_the_next_quads_only_move(monkeypatch):
    sc, rows = _scene("spheres300")
    calls, new, _ = _moved("spheres300", "all")
    moved = prim.MovedScene(sc, quads=new["quads"])  # old spheres, new quads
    rays = _random_rays(rows, 513)
    with _open("spheres300", moved, False, monkeypatch) as fresh:
        want, want_rec = _outputs(fresh, rays), _records(fresh)
    with _open("spheres300", sc, True, monkeypatch) as ds:
        with pytest.raises(DeviceError) as e:
            ds.set_primitives(spheres=prim.scale(rows, 8.0)["spheres"])
        assert e.value.code == _abi.SOL_ERANGE
        bad = new["spheres"].copy()
        bad[7, 3] = np.nan
        with pytest.raises(DeviceError) as e:
            ds.set_primitives(spheres=bad)
        assert e.value.code == _abi.SOL_EINVAL
        ds.set_primitives(quads=new["quads"])
        _same(_outputs(ds, rays), want, "old spheres, new quads")
        _same(_records(ds), want_rec, "records")


def test_argument_errors_with_a_handle(monkeypatch):
    sc, rows = _scene("twospheres")
    with _open("twospheres", sc, True, monkeypatch) as ds:
        lib, S, U = ds.lib, _abi.SolPrimitiveSet, _abi.SolGeometryUpdate
        s = np.ascontiguousarray(rows["spheres"])
        good = S(size=C.sizeof(S), spheres=s.ctypes.data, n_spheres=2)
        assert lib.sol_scene_set_primitives(ds.h, None, None) == _abi.SOL_EINVAL and b"null set" in lib.sol_last_error()
        assert lib.sol_scene_set_primitives(ds.h, C.byref(S(size=C.sizeof(S))), None) == _abi.SOL_EINVAL and b"all three" in lib.sol_last_error()
        assert lib.sol_scene_set_primitives(ds.h, C.byref(S(size=C.sizeof(S), spheres=s.ctypes.data, n_spheres=3)), None) == _abi.SOL_EINVAL
        assert lib.sol_scene_set_primitives(ds.h, C.byref(S(size=C.sizeof(S), flags=_abi.SOL_PRIMS_DEVICE, spheres=8, n_spheres=2)), None) == _abi.SOL_EINVAL
        assert b"aligned" in lib.sol_last_error()
        assert lib.sol_scene_set_primitives(ds.h, C.byref(good), C.byref(U(size=8, flags=_abi.SOL_GEOM_NO_BACKGROUND_PROOF))) == _abi.SOL_OK
        assert not ds.background_flags().any()
        assert lib.sol_scene_set_primitives(ds.h, C.byref(good), None) == _abi.SOL_OK
        ds.kernel_timing(True)
        assert lib.sol_scene_set_primitives(ds.h, C.byref(good), None) == _abi.SOL_OK
        ms = ds.set_triangles_ms()
        assert all(v >= 0. for v in ms.values()), ms


# ---- background blocks over the refitted tree ---------------------------------------------------------------------------------------------------
def test_background_blocks_of_a_moved_scene_are_sound_and_not_all_lost(monkeypatch):
    sc, rows = _scene("twospheres")
    new = prim.jitter(rows, 3, 0.2)
    moved = prim.MovedScene(sc, **new)
    assert background_blocks(moved, 0).mean() >= 0.2 and background_blocks(sc, 0).mean() >= 0.2   # the host proof (checked on the CPU first)
    with _open("twospheres", sc, True, monkeypatch) as ds:
        ds.set_primitives(spheres=new["spheres"])
        flags = ds.background_flags()
        assert flags.mean() >= 0.1, flags.mean()
        mask = np.repeat(np.repeat(flags, 8, axis=0), 8, axis=1)[:sc.height, :sc.width]
        hits_elsewhere = 0
        for sample in range(4):
            rays = ds.camera_rays(0, 0, sc.width, sc.height, sample, SEED).cpu().numpy().reshape(-1, 8)
            status = ds.closest_hits(rays)["status"].reshape(sc.height, sc.width)
            assert (status[mask] == _abi.SOL_RAY_MISS).all(), (sample, int((status[mask] != _abi.SOL_RAY_MISS).sum()))
            hits_elsewhere += int((status[~mask] == HIT).sum())
        assert hits_elsewhere > 0
        ds.set_primitives(spheres=new["spheres"], background_proof=False)
        assert not ds.background_flags().any()
