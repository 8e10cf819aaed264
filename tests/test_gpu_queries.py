"""Ray queries on the device (sol_query / sol_query_dev / sol_camera_rays) against three independent yardsticks: the float
oracle's own closest hit (bit for bit), the device's path diagnostics and counters, and the queries' own invariants - batch shape,
interval, validity, neutrality towards renders."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import orc
import parity_util as pu
from solstrale_amd import CameraConfig, DeviceError, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = np.float32(np.inf)
HIT, MISS, INVALID = _abi.SOL_RAY_HIT, _abi.SOL_RAY_MISS, _abi.SOL_RAY_INVALID


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _cornell():
    return scenes.cornell_box(RenderConfig(64, 64, 1))


def _random_mixed():
    """The first seeded random scene of the parity tests' generator without a constant medium (queries refuse those): spheres, quads,
    triangles and boxes in one world, so mixed leaves."""
    import random_scenes
    for seed in range(48):
        sc = random_scenes.random_scene(seed)
        if sc.desc.n_mediums == 0 and sc.desc.n_spheres and sc.desc.n_quads and sc.desc.n_triangles:
            return sc
    raise AssertionError("no medium-free mixed scene among the seeds")


def _needles():
    from test_fp32_contract import strip_light_scene
    return strip_light_scene(300, RenderConfig(96, 64, 1, PathTracingShader(8)))


def _deep_chain():
    """The sphere chain of the deep-tree tests, 120 levels: collapsed from the reference's own topology (SOL_BVH=ref) the 7-wide tree is 20
    levels deep, 42 dwords of stack - past the 32 of the LDS stack, so the query kernel built with the spill tail runs."""
    from test_gpu_parity import _sphere_chain
    b = SceneBuilder()
    inner = _sphere_chain(b, 120)
    light = b.Sphere((0., 1e4, 0.), 3e3, b.DiffuseLight(3, 3, 3))
    cam = CameraConfig(12., 0., (-30., 0.4, 0.3), (50., 0.3, 0.), (0, 1, 0))
    return b.finish(b.Bvh([inner, light]), cam, (.1, .1, .1), RenderConfig(64, 64, 1))


def _quad_stack():
    """Five parallel unit-spaced quads across the -z axis (and a light off the axis)."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    world = [b.Quad((-1., -1., -float(k)), (2., 0., 0.), (0., 2., 0.), grey) for k in range(1, 6)]
    world.append(b.Quad((-1., 5., -4.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(5., 5., 5.)))
    cam = CameraConfig(40., 0., (0., 0., 3.), (0., 0., -1.), (0., 1., 0.))
    return b.finish(b.Bvh(world), cam, (0., 0., 0.), RenderConfig(32, 32, 1))


# ---- rays ------------------------------------------------------------------------------------------------------------------
def _world_box(sc):
    d = sc.desc
    assert _abi.ref_kind(d.root) == _abi.REF_NODE
    v = d.nodes[_abi.ref_index(d.root)].bbox.v
    lo, hi = np.array([v[0], v[2], v[4]]), np.array([v[1], v[3], v[5]])
    if (hi - lo).max() > 1e3:  # (a far light - a sphere of radius 3000 ten thousand units up - would make every random ray start in empty space)
        lo, hi = np.maximum(lo, -50.), np.minimum(hi, 50.)
    return lo, hi


def _targets(sc):
    """Vertices, edge midpoints and centres of the scene's primitives (f64)."""
    d, pts = sc.desc, []
    for i in range(d.n_triangles):
        t = d.triangles[i]
        a = np.array(t.v0[:]); b = a + np.array(t.v0v1[:]); c = a + np.array(t.v0v2[:])
        pts += [a, b, c, (a + b) / 2, (b + c) / 2, (a + c) / 2, (a + b + c) / 3]
    for i in range(d.n_quads):
        q = d.quads[i]
        o = np.array(q.q[:]); u = np.array(q.u[:]); v = np.array(q.v[:])
        pts += [o, o + u, o + v, o + u + v, o + u / 2, o + v / 2, o + u + v / 2, o + v + u / 2, o + (u + v) / 2]
    for i in range(d.n_spheres):
        pts.append(np.array(d.spheres[i].center[:]))
    return np.array(pts)


def _as_rays(o, d, tmin=0.001, tmax=np.inf):
    n = len(o)
    r = np.empty((n, 8), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def ray_mix(sc, ds, seed, per_class=256):
    """A seeded mix, tmin = 0.001, tmax = inf: camera rays; uniform random rays from inside the world box; rays aimed at vertices, edges and
    primitive centres; axis-aligned rays with both signed zeros."""
    rng = np.random.default_rng(seed)
    lo, hi = _world_box(sc)
    cam = ds.camera_rays(0, 0, sc.width, sc.height, 3, pu.SEED).cpu().numpy().reshape(-1, 8)
    cam = cam[rng.choice(len(cam), per_class, replace=False)]
    o = rng.uniform(lo, hi, (per_class, 3))
    uniform = _as_rays(o, rng.normal(size=(per_class, 3)) * rng.uniform(0.1, 20., (per_class, 1)))
    tg = _targets(sc)
    tg = tg[rng.integers(0, len(tg), per_class)]
    o = np.where(rng.random((per_class, 1)) < 0.5, rng.uniform(lo, hi, (per_class, 3)), np.array(sc.desc.camera.origin[:])[None, :])
    aimed = _as_rays(o, tg - o)
    o = rng.uniform(lo, hi, (per_class, 3))
    d = np.where(rng.random((per_class, 3)) < 0.5, 0.0, -0.0)
    axis = rng.integers(0, 3, per_class)
    d[np.arange(per_class), axis] = rng.choice([-1.0, 1.0, 2.5, -0.25], per_class)
    axial = _as_rays(o, d)
    rays = np.concatenate([cam, uniform, aimed, axial])
    assert np.signbit(axial[:, 4:7][axial[:, 4:7] == 0]).any() and not np.signbit(axial[:, 4:7][axial[:, 4:7] == 0]).all()
    return np.ascontiguousarray(rays[rng.permutation(len(rays))])


def oracle_hits(sc, rays):
    """orc_closest_hit in the float instantiation, ray by ray: (status, t cast back to float, material)."""
    lib = orc.load()
    n = len(rays)
    status, t, mat = np.zeros(n, np.uint32), np.full(n, np.inf, np.float32), np.zeros(n, np.uint32)
    o, d, tt, mm = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(), C.c_uint32()
    for i, r in enumerate(rays):
        assert r[3] == np.float32(0.001) and r[7] == INF  # (the oracle searches RAY_INTERVAL)
        o[:], d[:] = [float(x) for x in r[0:3]], [float(x) for x in r[4:7]]
        if lib.orc_closest_hit(sc.desc_ptr, orc.ORC_F32, o, d, C.byref(tt), C.byref(mm)):
            status[i], t[i], mat[i] = HIT, np.float32(tt.value), mm.value
    return status, t, mat


def both_modes(ds, rays):
    """closest_hits, after checking that occluded answers SOL_RAY_HIT exactly where it reports a hit (and INVALID where it does)."""
    hits = ds.closest_hits(rays)
    occ = ds.occluded(rays)
    assert occ.dtype == np.uint32 and (occ == np.where(hits["status"] == HIT, HIT, np.where(hits["status"] == INVALID, INVALID, MISS))).all()
    return hits


def check_misses(hits):
    m = hits["status"] == MISS
    assert (hits["t"][m] == INF).all()
    for f in ("u", "v", "kind", "dfs_index", "material", "reserved"):
        assert (hits[f][m] == 0).all(), f
    assert (hits["reserved"] == 0).all()


# ---- bit-exact against the float oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,env,expect", [(_cornell, {}, {}), (_random_mixed, {}, {}), (_needles, {}, {"strict_triangles": True}),
                                             (_deep_chain, {"SOL_BVH": "ref"}, {"spill": True})],
                         ids=["cornell", "random_mixed", "needles_strict", "deep_chain_spill"])
def test_closest_hits_equal_the_float_oracle_bit_for_bit(make, env, expect, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = make()
    d = sc.desc
    assert d.n_mediums == 0 and d.n_spheres + d.n_quads + d.n_triangles <= 2000
    with DeviceScene(sc) as ds:
        info = ds.info()
        if "strict_triangles" in expect:
            assert info["strict_triangles"]
        if "spill" in expect:
            assert info["stack_bound"] > info["lds_stack"], info
        rays = ray_mix(sc, ds, 7)
        assert len(rays) <= 2048
        hits = both_modes(ds, rays)
    status, t, mat = oracle_hits(sc, rays)
    check_misses(hits)
    assert 0.1 < (status == HIT).mean() < 1.0  # (the mix exercises both answers)
    bad = np.nonzero(hits["status"] != status)[0]
    assert bad.size == 0, (bad[:8], rays[bad[:8]], hits[bad[:8]], t[bad[:8]])
    bad = np.nonzero(hits["t"].view(np.uint32) != t.view(np.uint32))[0]
    assert bad.size == 0, (bad[:8], rays[bad[:8]], hits[bad[:8]], t[bad[:8]])
    h = status == HIT
    assert (hits["material"][h] == mat[h]).all()
    # kind and dfs_index name a primitive of the description that carries this material
    for k in np.nonzero(h)[0][:256]:
        kind, dfs = int(hits["kind"][k]), int(hits["dfs_index"][k])
        arr, n = {_abi.REF_SPHERE: (d.spheres, d.n_spheres), _abi.REF_QUAD: (d.quads, d.n_quads), _abi.REF_TRIANGLE: (d.triangles, d.n_triangles)}[kind]
        assert any(arr[i].dfs_index == dfs and arr[i].material == int(hits["material"][k]) for i in range(n)), (k, kind, dfs)


# ---- device against device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_cornell, _random_mixed], ids=["cornell", "random_mixed"])
def test_row_0_of_debug_path_is_camera_rays_then_closest_hits(make):
    sc = make()
    rng = np.random.default_rng(11)
    with DeviceScene(sc) as ds:
        for _ in range(32):
            x, y, s = int(rng.integers(0, sc.width)), int(rng.integers(0, sc.height)), int(rng.integers(0, 64))
            rows, _colour = ds.debug_path(x, y, s, pu.SEED)
            ray = ds.camera_rays(x, y, x + 1, y + 1, s, pu.SEED).cpu().numpy().reshape(1, 8)
            hit = ds.closest_hits(ray)[0]
            r0 = rows[0]
            assert ray[0, 3] == np.float32(0.001) and ray[0, 7] == INF
            assert r0[0:3].tobytes() == ray[0, 0:3].tobytes() and r0[3:6].tobytes() == ray[0, 4:7].tobytes(), (x, y, s)
            ref_bits, dfs_bits = int(r0[7:8].view(np.uint32)[0]), int(r0[8:9].view(np.uint32)[0])
            if _abi.ref_kind(ref_bits) == _abi.REF_NONE:
                assert hit["status"] == MISS, (x, y, s, hit)
            else:
                assert hit["status"] == HIT and hit["t"].tobytes() == r0[6:7].tobytes(), (x, y, s, hit, r0)
                assert hit["kind"] == _abi.ref_kind(ref_bits) and hit["dfs_index"] == dfs_bits, (x, y, s, hit, r0)


def test_primary_hit_count_of_a_counted_render_equals_the_hits_over_its_camera_rays():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        ds.render(0, 1, pu.SEED, counted=True)
        st = _abi.SolPathStats()
        st.size = C.sizeof(st)
        ds._chk(ds.lib.sol_path_stats(ds.h, C.byref(st)))
        assert st.samples == 64 * 64
        rays = ds.camera_rays(0, 0, 64, 64, 0, pu.SEED)
        assert tuple(rays.shape) == (64, 64, 8)
        hits = ds.hits_to_numpy(ds.closest_hits(rays.reshape(-1, 8)))
    assert int((hits["status"] == HIT).sum()) == int(st.primary_hits) and 0 < st.primary_hits


# ---- batch shapes ------------------------------------------------------------------------------------------------------------------
def test_batch_shape_and_order_do_not_change_a_ray_s_answer():
    """n = 1, 63, 64, 65, 255, 257 and 4097 cross wave, workgroup and grid-stride boundaries: each batch gives the bytes of the same prefix of
    one large batch, and a permuted batch the permuted bytes - in both modes."""
    sc = _random_mixed()
    with DeviceScene(sc) as ds:
        rays = np.concatenate([ray_mix(sc, ds, 21, 512), ray_mix(sc, ds, 22, 513)])[:4097]
        assert len(rays) == 4097
        whole = both_modes(ds, rays)
        assert 0 < (whole["status"] == HIT).sum() < len(rays)
        for n in (1, 63, 64, 65, 255, 257, 4097):
            part = both_modes(ds, rays[:n])
            assert part.tobytes() == whole[:n].tobytes(), n
        perm = np.random.default_rng(5).permutation(len(rays))
        assert both_modes(ds, rays[perm]).tobytes() == whole[perm].tobytes()
        assert len(ds.closest_hits(rays[:0])) == 0 and len(ds.occluded(rays[:0])) == 0  # n == 0 succeeds and does nothing


# ---- interval ----------------------------------------------------------------------------------------------------------------------
def test_the_interval_is_the_search_s_own():
    sc = _quad_stack()
    with DeviceScene(sc) as ds:
        ray = _as_rays(np.array([[0.1, 0.2, 0.5]]), np.array([[0., 0., -2.]]))  # |d| = 2: t counts in units of it
        ts = []
        for _ in range(5):
            h = both_modes(ds, ray)[0]
            assert h["status"] == HIT and h["kind"] == _abi.REF_QUAD
            ts.append(h["t"])
            ray[0, 3] = np.nextafter(h["t"], INF)
        assert all(a < b for a, b in zip(ts, ts[1:])) and ts[0] == np.float32(0.75) and ts[4] == np.float32(2.75), ts
        assert both_modes(ds, ray)[0]["status"] == MISS
        ray[0, 3] = 0.001
        for tmax, want in ((0.5 * ts[0], MISS), (2.0 * ts[0], HIT), (ts[0], HIT), (np.nextafter(ts[0], np.float32(0)), MISS)):
            ray[0, 7] = tmax
            h = both_modes(ds, ray)[0]
            assert h["status"] == want and (want == MISS or h["t"] == ts[0]), (tmax, h)
        # finite upper ends on a whole batch: a hit is kept exactly when it lies inside
        rays = ray_mix(sc, ds, 31, 64)
        open_ = ds.closest_hits(rays)
        rays[:, 7] = 3.0
        cut = both_modes(ds, rays)
        inside = (open_["status"] == HIT) & (open_["t"] <= 3.0)
        assert (cut["status"] == np.where(inside, HIT, MISS)).all() and cut[inside].tobytes() == open_[inside].tobytes()


def test_finite_upper_ends_in_a_scene_with_needles():
    sc = _needles()
    with DeviceScene(sc) as ds:
        rays = ray_mix(sc, ds, 33, 128)
        open_ = ds.closest_hits(rays)
        rays[:, 7] = np.float32(np.median(open_["t"][open_["status"] == HIT]))
        cut = both_modes(ds, rays)
        inside = (open_["status"] == HIT) & (open_["t"] <= rays[:, 7])
        assert inside.any() and (~inside & (open_["status"] == HIT)).any()
        assert (cut["status"] == np.where(inside, HIT, MISS)).all() and cut[inside].tobytes() == open_[inside].tobytes()


# ---- invalid rays ------------------------------------------------------------------------------------------------------------------
def test_invalid_rays_are_answered_invalid_and_leave_their_neighbours_alone():
    sc = _random_mixed()
    nan = np.float32(np.nan)
    classes = [(4, nan), (5, INF), (6, -INF), ("zero", 0), (0, nan), (3, np.float32(-0.5)), ("tmin>tmax", 0), (7, nan), (1, INF), (3, INF), (7, -INF)]
    with DeviceScene(sc) as ds:
        valid = ray_mix(sc, ds, 41, 64)
        rng = np.random.default_rng(42)
        mixed, is_valid = [], []
        for k, r in enumerate(valid):
            mixed.append(r); is_valid.append(True)
            if k % 3 == 0:
                col, val = classes[int(rng.integers(0, len(classes)))] if k >= 3 * len(classes) else classes[k // 3]
                b = valid[int(rng.integers(0, len(valid)))].copy()
                if col == "zero":
                    b[4:7] = [0.0, -0.0, 0.0]
                elif col == "tmin>tmax":
                    b[3], b[7] = 2.0, 1.0
                else:
                    b[col] = val
                mixed.append(b); is_valid.append(False)
        mixed, is_valid = np.array(mixed, dtype=np.float32), np.array(is_valid)
        assert (~is_valid).sum() >= len(classes)
        alone = ds.closest_hits(valid)
        hits = both_modes(ds, mixed)
    assert (hits["status"][~is_valid] == INVALID).all()
    assert hits[is_valid].tobytes() == alone.tobytes()
    inv = hits[~is_valid]
    for f in ("t", "u", "v", "kind", "dfs_index", "material", "reserved"):
        assert (inv[f].view(np.uint32) == 0).all(), f


# ---- neutrality --------------------------------------------------------------------------------------------------------------------
def test_a_query_between_renders_changes_no_frame():
    sc = scenes.cornell_box(RenderConfig(64, 64, 32))
    with DeviceScene(sc) as ds:
        ds.render(0, 32, pu.SEED)
        want = ds.read()
        ds.clear()
        ds.render(0, 16, pu.SEED)
        rays = ray_mix(sc, ds, 51, 64)
        both_modes(ds, rays)
        ds.render(16, 16, pu.SEED)
        assert ds.read().tobytes() == want.tobytes()
        # inside an adaptive session with threshold 0 (every block runs to max_samples)
        ds.adaptive_begin(16, 16, 32, 0.0)
        assert ds.adaptive_round(pu.SEED) > 0
        both_modes(ds, rays)
        assert ds.adaptive_round(pu.SEED) == 0
        assert ds.read().tobytes() == want.tobytes() and (ds.adaptive_counts() == 32).all()


def test_refusals():
    with DeviceScene(scenes.create_test_scene(RenderConfig(32, 32, 1))) as ds:  # (a constant medium)
        ray = _as_rays(np.zeros((1, 3)), np.ones((1, 3)))
        for f in (ds.closest_hits, ds.occluded):
            with pytest.raises(DeviceError) as e:
                f(ray)
            assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        assert tuple(ds.camera_rays(0, 0, 4, 2, 0, 1).shape) == (2, 4, 8)  # (camera rays need no search)
    with DeviceScene(_cornell()) as ds:
        lib, ray, out = ds.lib, _as_rays(np.zeros((1, 3)), np.ones((1, 3))), np.zeros(8, np.uint32)
        assert lib.sol_query(ds.h, 2, ray.ctypes.data, 1, out.ctypes.data) == _abi.SOL_EINVAL and b"mode" in lib.sol_last_error()
        assert lib.sol_query(ds.h, 0, None, 1, out.ctypes.data) == _abi.SOL_EINVAL and b"null" in lib.sol_last_error()
        assert lib.sol_query(ds.h, 0, ray.ctypes.data, 1, None) == _abi.SOL_EINVAL
        assert lib.sol_query_dev(ds.h, 0, None, 1, None) == _abi.SOL_EINVAL
        assert lib.sol_query(None, 0, ray.ctypes.data, 1, out.ctypes.data) == _abi.SOL_EINVAL
        assert lib.sol_query(ds.h, 0, ray.ctypes.data, (1 << 31) + 1, out.ctypes.data) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
        assert lib.sol_query(ds.h, 0, None, 0, None) == _abi.SOL_OK
        for rect in ((0, 0, 0, 1), (3, 0, 3, 4), (0, 0, 65, 1), (0, 5, 4, 5), (0, 0, 4, 65), (70, 0, 80, 4)):
            with pytest.raises(DeviceError) as e:
                ds.camera_rays(*rect, 0, 1)
            assert e.value.code == _abi.SOL_EINVAL, rect
        assert (out == 0).all()


# ---- device-pointer route ----------------------------------------------------------------------------------------------------------
def test_device_tensors_give_the_host_route_s_answers():
    import torch
    sc = _random_mixed()
    with DeviceScene(sc) as ds:
        rays = ray_mix(sc, ds, 61, 300)
        rays[::7, 7] = 4.0
        rays[5, 4:7] = 0.0  # an invalid one
        host_hits, host_occ = ds.closest_hits(rays), ds.occluded(rays)
        dev = torch.from_numpy(rays).cuda()
        dh, do = ds.closest_hits(dev), ds.occluded(dev)
        assert dh.is_cuda and do.is_cuda and tuple(dh.shape) == (len(rays), 8) and tuple(do.shape) == (len(rays),)
        assert ds.hits_to_numpy(dh).tobytes() == host_hits.tobytes()
        assert do.cpu().numpy().view(np.uint32).tobytes() == host_occ.tobytes()
        with pytest.raises(ValueError):
            ds.closest_hits(dev[:, :7])
        with pytest.raises(ValueError):
            ds.closest_hits(dev.double())
    assert zlib.crc32(host_hits.tobytes()) != 0
