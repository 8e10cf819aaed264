"""sol_scene_set_triangles: a live handle gets new vertices for its triangles. After the move every output - frame, auxiliary
planes, camera rays, closest hits - is byte-identical to a handle freshly created from D' (tests/geometry_util.py: every triangle made again
by sol_triangle_from_vertices, every node box the union of its children's); the closest hits are also the float oracle's on D', bit for bit -
the probe for a refitted box that fails to contain its primitive; the device's triangle records are those a creation from D' uploads (read
back through sol_scene_triangle_records, the read-back route of the library: sol_debug_path shows hits, not records). Sequences do not
accumulate, the order with sol_scene_set_camera does not matter, options, modes and the partition are kept, refusals leave the handle as
it was, and the background blocks proved over the refitted tree are sound.

Frames are 128x96 at 16 spp."""
import ctypes as C

import numpy as np
import pytest

import geometry_util as gu
import orc
import parity_util as pu
from solstrale_amd import (CameraConfig, DeviceError, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, background_blocks,
                           triangle_from_vertices)

pytestmark = pytest.mark.gpu

SEED = pu.SEED
SPP = 16
RC = RenderConfig(128, 96, SPP, PathTracingShader(8))
MOVES = ("identity", "sine", "translate", "scale")
HIT = _abi.SOL_RAY_HIT
INF = np.float32(np.inf)


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _grid_mesh(cells=24, size=3.0, centre=(0., 1.2, 0.), bump=0.35):
    """cells x cells x 2 triangles of a wavy sheet, float64 [n, 3, 3], and per-vertex texture coordinates [n, 3, 2]."""
    k = np.arange(cells + 1) / cells
    x, z = np.meshgrid(k, k, indexing="ij")
    p = np.stack([(x - .5) * size + centre[0], centre[1] + bump * np.sin(5. * x) * np.cos(4. * z), (z - .5) * size + centre[2]], axis=-1)
    uv = np.stack([x, z], axis=-1)
    tri = lambda g: np.concatenate([np.stack([g[:-1, :-1], g[1:, :-1], g[1:, 1:]], axis=2).reshape(-1, 3, g.shape[-1]),
                                    np.stack([g[:-1, :-1], g[1:, 1:], g[:-1, 1:]], axis=2).reshape(-1, 3, g.shape[-1])])
    return tri(p), tri(uv).astype(np.float32)


_CAM = CameraConfig(40., 0., (0., 4., 10.), (0., 1., 0.), (0., 1., 0.))


def _mesh_scene(rc=RC, camera=_CAM, environment=False, emissive=0, floor=True, cells=24):
    """(a) the grid mesh over a floor quad, with a sphere and a quad light in ONE Bvh list (mixed-kind leaves). emissive: so many triangle
    lights hover above the mesh (they move with it)."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    red = b.Lambertian(b.SolidColor(.7, .3, .25))
    verts, uvs = _grid_mesh(cells)
    first, n = b.triangles(verts, red, uvs)
    world = list(range(first, first + n))
    if floor:
        world.append(b.Quad((-3., 0., -3.), (6., 0., 0.), (0., 0., 6.), grey))
    world.append(b.Sphere((2.2, .7, 1.), .7, grey))
    world.append(b.Quad((-1., 5., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(9., 9., 9.)))
    for k in range(emissive):
        x = -1.2 + 2.4 * k / max(emissive - 1, 1)
        world.append(b.Triangle((x, 2.4, -.4), (x + .5 + .1 * k, 2.5, 0.), (x, 2.6, .5), b.DiffuseLight(4. + 3. * k, 6., 8. - k)))
    if environment:
        h, w = 32, 64
        yy, xx = np.meshgrid(np.linspace(0., 1., h), np.linspace(0., 1., w), indexing="ij")
        b.environment(np.stack([.2 + .6 * xx, .3 + .4 * yy, .8 - .5 * xx * yy], axis=-1).astype(np.float32), 1.5)
    return b.finish(b.Bvh(world), camera, (.2, .3, .5), rc)


def _split_scene():
    """(c) two large triangles (a floor) among the small ones of the mesh: the device build pre-splits the large ones (split_percent = 100)."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    verts, uvs = _grid_mesh(16)
    first, n = b.triangles(verts, grey, uvs)
    world = list(range(first, first + n))
    world += [b.Triangle((-6., 0., -6.), (6., 0., 6.), (6., 0.3, -6.), grey), b.Triangle((-6., 0., -6.), (-6., 0.2, 6.), (6., 0., 6.), grey),
              b.Triangle((-5., 0.1, 4.), (5., 3., -5.), (5., 0.1, 4.5), grey)]
    world.append(b.Quad((-1., 6., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(9., 9., 9.)))
    return b.finish(b.Bvh(world), _CAM, (.2, .3, .5), RC)


def _needle_scene():
    from test_fp32_contract import strip_light_scene
    return strip_light_scene(300, RC)


def _random_needle_scene():
    """(d) needle_scene of the random scene generator: 20-60 needles of aspect 40-2000 in every vertex order, textured, metal and dielectric
    materials, real texture coordinates, some of them lights."""
    import random_scenes
    return random_scenes.needle_scene(3, RC.width, RC.height, SPP)


def _two_triangles():
    """(f) a world of two triangles, one of them the light."""
    b = SceneBuilder()
    world = [b.Triangle((-2., 0., -1.), (2., 0., -1.), (0., 2.5, -1.5), b.Lambertian(b.SolidColor(.6, .6, .6))),
             b.Triangle((-1., 3., 1.), (1., 3., 1.), (0., 3.2, -1.), b.DiffuseLight(8., 8., 8.))]
    return b.finish(b.Bvh(world), CameraConfig(40., 0., (0., 2., 9.), (0., 1.5, 0.), (0., 1., 0.)), (.2, .3, .5), RC)


def _triangle_chain(n=120):
    """(i) a Bvh nested n levels deep, a triangle per level (the sphere chain of the deep-tree tests, in triangles): under SOL_BVH=ref the
    7-wide tree has many levels - one refit launch each - and its searches use the spill stack."""
    b = SceneBuilder()
    m = b.Lambertian(b.SolidColor(.8, .8, .8))
    ids = [b.Triangle((float(x), 0.3 * (x % 3) - .4, -.4), (float(x) + .2, 0.3 * (x % 3) + .5, 0.), (float(x) - .1, 0.3 * (x % 3) - .4, .45), m) for x in range(n)]
    inner = b.Bvh(ids[:2])
    for k in range(2, n):
        inner = b.Bvh([inner, ids[k]]) if k % 2 else b.Bvh([ids[k], inner])
    light = b.Sphere((0., 1e4, 0.), 3e3, b.DiffuseLight(3, 3, 3))
    cam = CameraConfig(12., 0., (-30., 0.4, 0.3), (50., 0.3, 0.), (0, 1, 0))
    return b.finish(b.Bvh([inner, light]), cam, (.1, .1, .1), RC)


# name -> (maker, creation arguments, environment variables, light sampling mode)
_SCENES = {
    "mesh": (_mesh_scene, {}, {}, None),
    "mesh_ref": (_mesh_scene, dict(world_tree=_abi.TREE_REF), {}, None),
    "mesh_sah16": (_mesh_scene, dict(world_tree=_abi.TREE_SAH16), {}, None),
    "split": (_split_scene, dict(split_percent=100), {}, None),
    "needle_scene": (_random_needle_scene, {}, {}, None),
    "strip_light": (_needle_scene, {}, {}, None),  # (an extra: two needle triangles that are the light)
    "emissive_uniform": (lambda: _mesh_scene(emissive=5), {}, {}, "uniform"),
    "emissive_tree": (lambda: _mesh_scene(emissive=5), {}, {}, "tree"),
    "emissive_power": (lambda: _mesh_scene(emissive=5), {}, {}, "power"),
    "two_triangles": (_two_triangles, {}, {}, None),
    "environment": (lambda: _mesh_scene(environment=True), {}, {}, None),
    "thin_lens": (lambda: _mesh_scene(camera=CameraConfig(40., 0.25, (0., 4., 10.), (0., 1., 0.), (0., 1., 0.))), {}, {}, None),
    "chain_ref": (_triangle_chain, {}, {"SOL_BVH": "ref"}, None),
}
_cache = {}


def _base(name):
    """Scenes that differ only in how the handle is created share the description, D' and the oracle's answers."""
    return name.split("_")[0] if name.startswith(("mesh", "emissive")) else name


def _scene(name):
    if _base(name) not in _cache:
        _cache[_base(name)] = _SCENES[name][0]()
    return _cache[_base(name)]


def _moved(name, kind):
    """(new vertices, D') of scene `name` under move `kind`; cached, with the oracle's hits once they are asked for."""
    key = (_base(name), kind)
    if key not in _cache:
        sc = _scene(name)
        v = gu.move(gu.vertices_of(sc.desc), kind)
        _cache[key] = (v, gu.MovedScene(sc, v))
    return _cache[key]


def _open(name, sc, dynamic, monkeypatch):
    _, create, env, mode = _SCENES[name]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    ds = DeviceScene(sc, dynamic_triangles=dynamic, **create)
    if mode:
        ds.light_sampling(mode)
    return ds


def _random_rays(sc, n=4097, seed=11):
    rng = np.random.default_rng(seed)
    p = gu.vertices_of(sc.desc).reshape(-1, 3)
    lo, hi = np.maximum(p.min(axis=0) - 1., -60.), np.minimum(p.max(axis=0) + 1., 60.)
    r = np.empty((n, 8), dtype=np.float32)
    r[:, 0:3] = rng.uniform(lo, hi, (n, 3))
    r[:, 3] = 0.001
    aim = p[rng.integers(0, len(p), n)] + rng.normal(size=(n, 3)) * 0.05   # most rays pass near a vertex: boxes are grazed
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


def _same(got, want, what):
    for k in want:
        g, w = got[k], want[k]
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


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MOVES)
@pytest.mark.parametrize("name", list(_SCENES))
def test_a_moved_handle_is_a_fresh_handle_of_the_moved_description(name, kind, monkeypatch):
    sc = _scene(name)
    v, moved = _moved(name, kind)
    rays = _random_rays(moved)
    with _open(name, moved, False, monkeypatch) as fresh:
        want = _outputs(fresh, rays)
        want_info = fresh.info()
        ft, fs, fof = fresh.triangle_records()
    with _open(name, sc, True, monkeypatch) as ds:
        info = ds.info()
        if name == "split":
            assert info["split_references"] > 0
        if name == "chain_ref":
            assert info["tree_name"] == "ref" and info["stack_bound"] > info["lds_stack"], info
        ds.render(0, SPP, SEED)  # (sums, a table and costs of the old geometry are there to be dropped)
        ds.set_triangles(v)
        got = _outputs(ds, rays)
        _same(got, want, (name, kind))
        assert ds.info()["strict_triangles"] == want_info["strict_triangles"]
        # records, by caller triangle (the leaf order is each tree's own; every copy of a pre-split triangle is the same record)
        dt, dsh, dof = ds.triangle_records()
        fresh_of = {int(i): k for k, i in enumerate(fof)}
        assert set(int(i) for i in dof) == set(fresh_of)
        pick = np.array([fresh_of[int(i)] for i in dof])
        assert dt.tobytes() == ft[pick].tobytes(), int((dt.view(np.uint8).reshape(len(dt), -1) != ft[pick].view(np.uint8).reshape(len(dt), -1)).any(axis=1).sum())
        assert dsh.tobytes() == fs[pick].tobytes(), int((dsh.view(np.uint8).reshape(len(dt), -1) != fs[pick].view(np.uint8).reshape(len(dt), -1)).any(axis=1).sum())
    # the float oracle on D': every camera ray of the frame and the random rays
    all_rays = np.concatenate([want["camera_rays"].reshape(-1, 8), rays])
    okey = (_base(name), kind, "oracle")
    if okey not in _cache:
        _cache[okey] = _oracle_hits(moved, all_rays)
    status, t, mat = _cache[okey]
    assert 0.02 < (status == HIT).mean() < 1.0
    assert (got["status"] == status).all(), int((got["status"] != status).sum())
    assert got["t"].view(np.uint32).tobytes() == t.view(np.uint32).tobytes(), int((got["t"].view(np.uint32) != t.view(np.uint32)).sum())
    assert (got["material"][status == HIT] == mat[status == HIT]).all()


def test_records_are_the_cpu_functions(monkeypatch):
    """Device records against sol_triangle_from_vertices directly: v0 / edges of the rotated frame, normal, tangents, uvs, area - as float
    casts of the CPU function's f64 fields (the cast and the rotation are numpy's here, not the library's)."""
    sc = _scene("mesh")
    v, moved = _moved("mesh", "sine")
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_triangles(v)
        tris, shade, of = ds.triangle_records()
    f32 = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32)
    assert len(of) >= sc.desc.n_triangles
    for r in range(len(of)):
        t = triangle_from_vertices(v[of[r]], np.array([sc.desc.triangles[int(of[r])].uv0[:], sc.desc.triangles[int(of[r])].uv1[:], sc.desc.triangles[int(of[r])].uv2[:]]))
        a, b = np.array(t.v0v1[:]), np.array(t.v0v2[:])
        c = b - a
        l01, l02, l12 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2], (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        k = 2 if l01 > max(l12, l02) else (1 if l02 > l12 else 0)
        p0 = np.array(t.v0[:])
        v0, e1, e2 = [(p0, a, b), (p0 + a, b - a, -a), (p0 + b, -b, a - b)][k]
        assert tris["v0"][r].tobytes() == f32(v0).tobytes() and tris["e1"][r].tobytes() == f32(e1).tobytes() and tris["e2"][r].tobytes() == f32(e2).tobytes(), r
        assert tris["area"][r] == np.float32(t.area) and tris["dfs"][r] == sc.desc.triangles[int(of[r])].dfs_index
        assert shade["n"][r].tobytes() == f32(t.normal[:]).tobytes() and shade["t"][r].tobytes() == f32(t.tangent[:]).tobytes()
        assert shade["b"][r].tobytes() == f32(t.bi_tangent[:]).tobytes()
        uv = [t.uv0, t.uv1, t.uv2]
        assert (shade["u0"][r], shade["v0"][r], shade["u1"][r], shade["v1"][r]) == (uv[k][0], uv[k][1], uv[(k + 1) % 3][0], uv[(k + 1) % 3][1])
        assert (shade["u2"][r], shade["v2"][r]) == (uv[(k + 2) % 3][0], uv[(k + 2) % 3][1])
        assert tris["mat"][r] == shade["mat"][r] == sc.desc.triangles[int(of[r])].material


def test_the_device_route_takes_a_tensor_without_a_copy(monkeypatch):
    import torch
    sc = _scene("mesh")
    v, moved = _moved("mesh", "sine")
    rays = _random_rays(moved, 257)
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_triangles(v)
        want = _outputs(ds, rays)
        ds.set_triangles(gu.move(v, "translate"))
        ds.set_triangles(torch.from_numpy(v).to(f"cuda:{ds.device}"))
        _same(_outputs(ds, rays), want, "device route")


# ---- sequences, order, partition, sessions, neutrality ------------------------------------------------------------------------------------
def test_a_sequence_returns_to_where_it_started(monkeypatch):
    """A -> B -> C -> A equals fresh A: nothing accumulates in the boxes or the records."""
    sc = _scene("mesh")
    va, moved_a = _moved("mesh", "sine")
    rays = _random_rays(moved_a, 513)
    with _open("mesh", moved_a, False, monkeypatch) as fresh:
        want = _outputs(fresh, rays)
    with _open("mesh", sc, True, monkeypatch) as ds:
        for kind in ("sine", "scale", "translate", "sine"):
            ds.set_triangles(_moved("mesh", kind)[0])
            ds.render(0, SPP, SEED)
        _same(_outputs(ds, rays), want, "sequence")


def test_the_order_with_set_camera_does_not_matter(monkeypatch):
    cam_b = CameraConfig(50., 0., (6., 5., 7.), (0., 1., 0.), (0., 1., 0.))
    sc = _scene("mesh")
    v, moved = _moved("mesh", "sine")
    rays = _random_rays(moved, 513)
    with _open("mesh", moved, False, monkeypatch) as fresh:
        fresh.set_camera(cam_b)
        want = _outputs(fresh, rays)
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_camera(cam_b)
        ds.set_triangles(v)
        _same(_outputs(ds, rays), want, "camera first")
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_triangles(v)
        ds.set_camera(cam_b)
        _same(_outputs(ds, rays), want, "camera last")


def test_the_partition_survives_a_move(monkeypatch):
    sc = _scene("mesh")
    v, moved = _moved("mesh", "sine")
    with _open("mesh", moved, False, monkeypatch) as fresh:
        fresh.set_partition(1, 2)
        fresh.render(0, SPP, SEED)
        want, want_crc = fresh.read(), fresh.info()["partition_crc"]
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_partition(1, 2)
        ds.render(0, SPP, SEED)
        with pytest.raises(DeviceError) as e:
            ds.set_triangles(v, reprobe=True)
        assert e.value.code == _abi.SOL_EINVAL and "world" in e.value.msg
        ds.set_triangles(v)
        ds.render(0, SPP, SEED)
        assert ds.info()["partition_crc"] == want_crc and ds.read().tobytes() == want.tobytes()


def test_sums_and_sessions_are_reset_and_adaptive_rounds_are_the_fresh_handles(monkeypatch):
    sc = _scene("mesh")
    v, moved = _moved("mesh", "sine")

    def rounds(ds):
        ds.adaptive_begin(16, 16, 32, 0.05)
        n = ds.adaptive_run(SEED)
        return n, ds.read(), ds.adaptive_counts()

    with _open("mesh", moved, False, monkeypatch) as fresh:
        want = rounds(fresh)
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.render(0, SPP, SEED)
        ds.render_aux(0, SPP, SEED)
        ds.adaptive_begin(16, 16, 32, 0.05)
        assert ds.adaptive_round(SEED) > 0
        ds.set_triangles(v)
        assert not ds.read().any() and not ds.read_aux()[0].any() and ds.resolve_aux()[2] == 0
        with pytest.raises(DeviceError) as e:
            ds.adaptive_round(SEED)
        assert e.value.code == _abi.SOL_EINVAL and "no adaptive session" in e.value.msg
        got = rounds(ds)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and (got[2] == want[2]).all()


def test_the_option_alone_changes_no_byte(monkeypatch):
    sc = _scene("mesh")
    rays = _random_rays(sc, 513)
    with _open("mesh", sc, False, monkeypatch) as plain:
        want = _outputs(plain, rays)
        want_flags = plain.background_flags()
    with _open("mesh", sc, True, monkeypatch) as ds:
        _same(_outputs(ds, rays), want, "option on, never moved")
        assert (ds.background_flags() == want_flags).all()


def test_the_mesh_becomes_needles_and_is_plain_again(monkeypatch):
    """(d) strict_triangles 0 -> 1 -> 0: squashed to a hundredth along z the mesh's triangles are 100:1 needles - the fatter pad and the
    consistency rule come on as a creation would turn them on, and go again."""
    sc = _scene("mesh")
    v0 = gu.vertices_of(sc.desc)
    squashed = v0.copy()
    squashed[..., 2] *= 0.01
    rays = _random_rays(sc, 513)
    with _open("mesh", sc, True, monkeypatch) as ds:
        assert not ds.info()["strict_triangles"]
        for v, strict in ((squashed, True), (v0, False)):
            moved = gu.MovedScene(sc, v)
            with _open("mesh", moved, False, monkeypatch) as fresh:
                assert fresh.info()["strict_triangles"] == strict
                want = _outputs(fresh, rays)
            ds.set_triangles(v)
            assert ds.info()["strict_triangles"] == strict
            _same(_outputs(ds, rays), want, ("needles", strict))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_move_leaves_the_handle_as_it_was(monkeypatch):
    """After EACH refusal the sums are untouched and the next outputs (frame, auxiliary planes, camera rays, hits) are an untouched twin's."""
    from solstrale_amd import scenes
    sc = _scene("mesh")
    v = gu.vertices_of(sc.desc)
    rays = _random_rays(sc, 513)
    with _open("mesh", sc, True, monkeypatch) as twin:
        twin.set_triangles(_moved("mesh", "sine")[0])
        want = _outputs(twin, rays)
        want_flags = twin.background_flags()
    with _open("mesh", sc, True, monkeypatch) as ds:
        ds.set_triangles(_moved("mesh", "sine")[0])
        bad = v.copy()
        bad[17, 1, 2] = np.nan
        inf = v.copy()
        inf[3, 0, 0] = np.inf
        far = v.copy()
        far[5, 2, 1] = 1e12
        for verts, code, word in ((bad, _abi.SOL_EINVAL, "finite"), (inf, _abi.SOL_EINVAL, "finite"), (far, _abi.SOL_EINVAL, "2^38"),
                                  (v[:-1], _abi.SOL_EINVAL, "rows"), (gu.move(v, "scale", 8.0), _abi.SOL_ERANGE, "re-create")):
            ds.clear()
            ds.render(0, SPP, SEED)
            sums = ds.read()
            with pytest.raises(DeviceError) as e:
                ds.set_triangles(verts)
            assert e.value.code == code and word in e.value.msg, (code, e.value.code, e.value.msg)
            assert ds.read().tobytes() == sums.tobytes()  # no sums cleared
            assert (ds.background_flags() == want_flags).all()
            _same(_outputs(ds, rays), want, ("after the refusal", word))
    # a handle created without the option: refused, and still the plain twin
    with _open("mesh", sc, False, monkeypatch) as twin:
        want = _outputs(twin, rays)
    with _open("mesh", sc, False, monkeypatch) as plain:
        plain.render(0, SPP, SEED)
        sums = plain.read()
        with pytest.raises(DeviceError) as e:
            plain.set_triangles(v)
        assert e.value.code == _abi.SOL_EINVAL and "dynamic_triangles" in e.value.msg
        assert plain.read().tobytes() == sums.tobytes()
        _same(_outputs(plain, rays), want, "no option")
    # a scene with a constant medium (queries refuse it too: frame and auxiliary planes)
    med = scenes.create_test_scene(RC)
    assert med.desc.n_mediums > 0

    def frames(d):
        d.clear()
        d.clear_aux()
        d.render(0, SPP, SEED)
        d.render_aux(0, SPP, SEED)
        return dict(zip(("frame", "albedo", "normal"), (d.read(),) + tuple(d.read_aux())))

    with DeviceScene(med, dynamic_triangles=True) as twin:
        want = frames(twin)
    with DeviceScene(med, dynamic_triangles=True) as ds:
        ds.render(0, SPP, SEED)
        sums = ds.read()
        with pytest.raises(DeviceError) as e:
            ds.set_triangles(gu.vertices_of(med.desc))
        assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        assert ds.read().tobytes() == sums.tobytes()
        _same(frames(ds), want, "medium")


def test_argument_errors_with_a_handle(monkeypatch):
    sc = _scene("two_triangles")
    v = gu.vertices_of(sc.desc)
    with _open("two_triangles", sc, True, monkeypatch) as ds:
        lib, good = ds.lib, C.sizeof(_abi.SolGeometryUpdate)
        assert lib.sol_scene_set_triangles(ds.h, None, 2, None) == _abi.SOL_EINVAL
        for upd in (_abi.SolGeometryUpdate(size=4), _abi.SolGeometryUpdate(size=4097), _abi.SolGeometryUpdate(size=good, flags=4),
                    _abi.SolGeometryUpdate(size=good, reserved=(C.c_uint32 * 2)(0, 1))):
            assert lib.sol_scene_set_triangles(ds.h, v.ctypes.data, 2, C.byref(upd)) == _abi.SOL_EINVAL
        assert lib.sol_scene_set_triangles_dev(ds.h, C.c_void_p(8), 2, None) == _abi.SOL_EINVAL and b"aligned" in lib.sol_last_error()
        assert lib.sol_scene_set_triangles(ds.h, v.ctypes.data, 2, C.byref(_abi.SolGeometryUpdate(size=8, flags=_abi.SOL_GEOM_NO_BACKGROUND_PROOF))) == _abi.SOL_OK
        assert not ds.background_flags().any()
        assert lib.sol_scene_set_triangles(ds.h, v.ctypes.data, 2, None) == _abi.SOL_OK


# ---- background blocks over the refitted tree ---------------------------------------------------------------------------------------------------
def _sky_scene():
    """The mesh alone in the sky (no floor), small in the frame: under half of the frame before and after the move."""
    return _mesh_scene(floor=False, cells=12, camera=CameraConfig(40., 0., (0., 3., 14.), (0., 1.5, 0.), (0., 1., 0.)))


def test_background_blocks_of_a_moved_scene_are_sound_and_not_all_lost(monkeypatch):
    sc = _sky_scene()
    v = gu.move(gu.vertices_of(sc.desc), "sine")
    moved = gu.MovedScene(sc, v)
    host = background_blocks(moved, 0)
    assert host.mean() >= 0.2, host.mean()       # the host proof over D' (checked on the CPU first)
    assert background_blocks(sc, 0).mean() >= 0.2
    with DeviceScene(sc, dynamic_triangles=True) as ds:
        for sample in range(4):  # the mesh covers under half of the frame before the move ...
            rays = ds.camera_rays(0, 0, sc.width, sc.height, sample, SEED).cpu().numpy().reshape(-1, 8)
            assert 0.0 < (ds.closest_hits(rays)["status"] == HIT).mean() < 0.5
        ds.set_triangles(v)
        flags = ds.background_flags()
        assert flags.mean() >= 0.1, flags.mean()  # the refit tree's looser boxes may lose some, never all
        mask = np.repeat(np.repeat(flags, 8, axis=0), 8, axis=1)[:sc.height, :sc.width]
        hits_elsewhere = 0
        for sample in range(4):
            rays = ds.camera_rays(0, 0, sc.width, sc.height, sample, SEED).cpu().numpy().reshape(-1, 8)
            status = ds.closest_hits(rays)["status"].reshape(sc.height, sc.width)
            assert (status[mask] == _abi.SOL_RAY_MISS).all(), (sample, int((status[mask] != _abi.SOL_RAY_MISS).sum()))
            hits_elsewhere += int((status[~mask] == HIT).sum())
            assert (status == HIT).mean() < 0.5  # ... and after it
        assert hits_elsewhere > 0
        ds.set_triangles(v, background_proof=False)
        assert not ds.background_flags().any()
