"""Irradiance queries on the device (sol_irradiance / sol_irradiance_dev / sol_irradiance_rays). The anchor is the identity
with the radiance queries: sol_irradiance_rays writes the ray and key a sample starts with, sol_radiance over them is that sample's
contribution bit for bit, and the sums are the render's association of those. Around it: the generator against the float oracle, sums that
are exact by construction, an occluder whose blocked directions the CPU predicts, batch shapes, refusals and neutrality. Frames are 32 x 32."""
import ctypes as C
import zlib

import numpy as np
import pytest

import irradiance_util as iu
import orc
import parity_util as pu
from parity_util import env_two_lights as _env_two_lights
from solstrale_amd import (AlbedoShader, CameraConfig, DeviceError, DeviceScene, NormalShader, PathTracingShader, RenderConfig, SceneBuilder, _abi,
                           scenes)

pytestmark = pytest.mark.gpu
SEED = pu.SEED
INF = np.float32(np.inf)
NAN = np.float32(np.nan)
MODES = ("cosine", "sphere")
RC = RenderConfig(32, 32, 1)
# (column, value) per class of invalid row, as tests/test_gpu_queries.py enumerates them; "zero": a zero normal, "tmin>tmax"
INVALID_CLASSES = [(4, NAN), (5, INF), (6, -INF), ("zero", 0), (0, NAN), (3, np.float32(-0.5)), ("tmin>tmax", 0), (7, NAN), (1, INF), (3, INF), (7, -INF)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- scenes and points -------------------------------------------------------------------------------------------------------------------
def _cornell(rc=RC):
    return scenes.cornell_box(rc)


def _random_mixed():
    """The first medium-free seeded random scene with spheres, quads and triangles (tests/test_gpu_queries.py picks the same), at 32 x 32."""
    import random_scenes
    for seed in range(48):
        sc = random_scenes.random_scene(seed, width=32, height=32)
        if sc.desc.n_mediums == 0 and sc.desc.n_spheres and sc.desc.n_quads and sc.desc.n_triangles:
            return sc
    raise AssertionError("no medium-free mixed scene among the seeds")


def _needles():
    from test_fp32_contract import strip_light_scene
    return strip_light_scene(300, RenderConfig(32, 32, 1, PathTracingShader(8)))


def _deep_chain():
    """tests/test_gpu_queries.py's 120-level sphere chain: under SOL_BVH=ref its searches run past the LDS stack."""
    from test_gpu_parity import _sphere_chain
    b = SceneBuilder()
    inner = _sphere_chain(b, 120)
    light = b.Sphere((0., 1e4, 0.), 3e3, b.DiffuseLight(3, 3, 3))
    cam = CameraConfig(12., 0., (-30., 0.4, 0.3), (50., 0.3, 0.), (0, 1, 0))
    return b.finish(b.Bvh([inner, light]), cam, (.1, .1, .1), RC)


def surface_points(sc, ds, count, seed=1, hover=0.0):
    """`count` points on the scene's surfaces: where the camera rays of a sample hit (of as many samples as it takes), with the normal the
    auxiliary plane holds for that sample and pixel, scaled so that it is not unit length; tmin = 0.001, tmax = inf. Rows of (position, tmin,
    normal, tmax). hover > 0: every other point is lifted that far off its surface and looks back at it (the normal turned round), so that its
    paths meet geometry at once also in an open scene."""
    pos, nrm = [], []
    for s in range(8):
        rays = ds.camera_rays(0, 0, sc.width, sc.height, s, SEED).cpu().numpy().reshape(-1, 8)
        hits = ds.closest_hits(rays)
        ds.clear_aux()
        ds.render_aux(s, 1, SEED)
        normal = ds.read_aux()[1].reshape(-1, 3)
        ds.clear_aux()
        ok = np.nonzero((hits["status"] == _abi.SOL_RAY_HIT) & (np.abs(normal).sum(axis=1) > 0.5) & np.isfinite(normal).all(axis=1))[0]
        pos.append(rays[ok, 0:3] + hits["t"][ok, None] * rays[ok, 4:7])
        nrm.append(normal[ok])
        if sum(len(x) for x in pos) >= count:
            break
    pos, nrm = np.concatenate(pos), np.concatenate(nrm)
    assert len(pos) >= count, (len(pos), count)
    rng = np.random.default_rng(seed)
    ok = rng.permutation(len(pos))[:count]
    p = np.empty((count, 8), dtype=np.float32)
    p[:, 0:3], p[:, 3], p[:, 7] = pos[ok], 0.001, INF
    p[:, 4:7] = nrm[ok] * rng.uniform(0.25, 4.0, (count, 1)).astype(np.float32)
    if hover > 0.0:
        unit = nrm[ok][::2] / np.sqrt((nrm[ok][::2] ** 2).sum(axis=1, keepdims=True))
        p[::2, 0:3] += hover * unit
        p[::2, 4:7] = -p[::2, 4:7]
    return p


def with_invalid_rows(points, seed=2):
    """`points` with one invalid row of every class spliced in; returns (rows, is_valid)."""
    rng = np.random.default_rng(seed)
    rows, valid = list(points), [True] * len(points)
    for col, val in INVALID_CLASSES:
        b = points[int(rng.integers(0, len(points)))].copy()
        if col == "zero":
            b[4:7] = [0.0, -0.0, 0.0]
        elif col == "tmin>tmax":
            b[3], b[7] = 2.0, 1.0
        else:
            b[col] = val
        at = int(rng.integers(0, len(rows) + 1))
        rows.insert(at, b)
        valid.insert(at, False)
    return np.array(rows, dtype=np.float32), np.array(valid)


def _render_association(per_sample):
    """per_sample: [k, n, 3] float32 contributions of samples first .. first + k - 1. Chunk sums of up to 16 samples counted from the first one,
    each 0 + c + c + .. in sample order, then the chunks in order on top of 0 - sol_radiance's association, restated in numpy float32."""
    k, n = per_sample.shape[0], per_sample.shape[1]
    total = np.zeros((n, 3), dtype=np.float32)
    for c0 in range(0, k, 16):
        chunk = np.zeros((n, 3), dtype=np.float32)
        for j in range(c0, min(c0 + 16, k)):
            chunk = chunk + per_sample[j]
        total = total + chunk
    assert total.dtype == np.float32
    return total


def assert_identity(ds, points, is_valid=None, ks=(1, 17), first=5, key_base=7, modes=MODES, distinct=False):
    """irradiance(points, samples = k, first_sample = first) against the association over radiance(*irradiance_rays(points, s), samples = 1,
    first_sample = s), bit for bit, in both modes."""
    is_valid = np.ones(len(points), bool) if is_valid is None else is_valid
    for mode in modes:
        per = []
        for s in range(first, first + max(ks)):
            rays, keys = ds.irradiance_rays(points, s, seed=SEED, key_base=key_base, mode=mode)
            rows = ds.radiance(rays, samples=1, first_sample=s, seed=SEED, keys=keys).cpu().numpy()
            cnt = np.ascontiguousarray(rows[:, 3]).view(np.uint32)
            assert (cnt[is_valid] == 1).all() and (cnt[~is_valid] == 0).all(), (mode, s)
            per.append(np.ascontiguousarray(rows[:, :3]))
        per = np.stack(per)
        assert np.isfinite(per).all()
        assert np.abs(per).sum() > 0  # (something arrives somewhere)
        if distinct:
            assert len({p.tobytes() for p in per}) == len(per)  # (every sample is another path)
        for k in ks:
            rgb, cnt = ds.irradiance(points, samples=k, first_sample=first, seed=SEED, key_base=key_base, mode=mode)
            want = _render_association(per[:k])
            assert np.array_equal(_bits(rgb), _bits(want)), (mode, k, int((_bits(rgb) != _bits(want)).any(axis=1).sum()), len(points))
            assert (cnt[is_valid] == k).all() and (cnt[~is_valid] == 0).all() and (_bits(rgb[~is_valid]) == 0).all(), (mode, k)
    return per


# ---- 1. the identity with the radiance queries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_cornell, _random_mixed], ids=["cornell", "random_mixed"])
def test_irradiance_is_the_association_over_radiance_of_its_own_rays(make):
    sc = make()
    assert sc.desc.n_mediums == 0
    with DeviceScene(sc) as ds:
        points, is_valid = with_invalid_rows(surface_points(sc, ds, 300))
        assert len(points) == 300 + len(INVALID_CLASSES)
        assert_identity(ds, points, is_valid, ks=(1, 15, 16, 17, 48), distinct=True)


def _variation(name):
    """name -> (scene, environment variables, env_sampling mode, light_sampling mode, what the handle must report)."""
    import test_env_importance as te
    pt = lambda depth: RenderConfig(32, 32, 1, PathTracingShader(depth))
    return {
        "default": (lambda: _cornell(), {}, None, None, {}),
        "env_importance": (lambda: te._lambertian_scene(pt(6)), {}, "importance", None, {}),
        "light_tree": (lambda: scenes.many_lights(64, "quads", pt(50)), {}, None, "tree", {}),
        "light_power": (lambda: scenes.mixed_power_lights(64, pt(6)), {}, None, "power", {}),
        "env_and_tree": (lambda: _env_two_lights(pt(8)), {}, "importance", "tree", {}),
        "needles_strict": (_needles, {}, None, None, {"strict_triangles": True}),
        "deep_chain_spill": (_deep_chain, {"SOL_BVH": "ref"}, None, None, {"spill": True}),
        "albedo": (lambda: _cornell(RenderConfig(32, 32, 1, AlbedoShader())), {}, None, None, {}),
        "normal": (lambda: _cornell(RenderConfig(32, 32, 1, NormalShader())), {}, None, None, {}),
    }[name]


@pytest.mark.parametrize("name", ["default", "env_importance", "light_tree", "light_power", "env_and_tree", "needles_strict", "deep_chain_spill", "albedo",
                                  "normal"])
def test_the_identity_holds_in_every_estimator_kernel_and_shader(name, monkeypatch):
    make, env, env_mode, light_mode, expect = _variation(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = make()
    assert sc.desc.n_mediums == 0
    with DeviceScene(sc) as ds:
        info = ds.info()
        if "strict_triangles" in expect:
            assert info["strict_triangles"]
        if "spill" in expect:
            assert info["stack_bound"] > info["lds_stack"], info
        points = surface_points(sc, ds, 24, hover=0.5)
        plain = ds.irradiance(points, samples=4, seed=SEED)[0]
        if env_mode:
            ds.env_sampling(env_mode)
        if light_mode:
            ds.light_sampling(light_mode)
        assert_identity(ds, points)
        if env_mode or light_mode == "power":  # (the tree alone gives the uniform frames: DESIGN.md 14)
            assert ds.irradiance(points, samples=4, seed=SEED)[0].tobytes() != plain.tobytes()  # the query follows the handle's mode


# ---- 2. the generator ---------------------------------------------------------------------------------------------------------------------
def _generator_points(n=200, seed=3):
    """Points at random places with random normals of random length; among them normals along each axis, both signs, and ones with
    |x| > 0.9 of their length (onb_new's other helper axis)."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 8), dtype=np.float32)
    p[:, 0:3], p[:, 3], p[:, 7] = rng.uniform(-5, 5, (n, 3)), 0.001, INF
    nrm = rng.normal(size=(n, 3)) * rng.uniform(0.01, 100.0, (n, 1))
    nrm[:6] = np.concatenate([np.eye(3), -np.eye(3)]) * rng.uniform(0.5, 2.0, (6, 1))
    nrm[6:12] = np.array([1.0, 0.0, 0.0]) * rng.choice([-3.0, 3.0], (6, 1)) + rng.uniform(-0.4, 0.4, (6, 3))
    p[:, 4:7] = nrm
    return p


def _sphere_restated(seed, key, sample, first_draw):
    """random_in_unit_sphere from the stream of (seed, key, sample) at counter first_draw, restated from the oracle's orc_rng_bits in numpy
    float32: rounds of three draws, each 2 u - 1 with u = (bits >> 8) / 2^24, until x x + y y + z z < 1. Returns (point, rounds)."""
    lib = orc.load()
    for rounds in range(1, 81):
        c = first_draw + 3 * (rounds - 1)
        u = np.array([lib.orc_rng_bits(seed, key, sample, c + j) >> 8 for j in range(3)], dtype=np.float32) * np.float32(1.0 / 16777216.0)
        p = u * np.float32(2.0) + np.float32(-1.0)
        if p[0] * p[0] + p[1] * p[1] + p[2] * p[2] < np.float32(1.0):
            return p, rounds
    raise AssertionError("80 rejections")


def test_the_directions_are_the_float_oracle_s_generator():
    """COSINE at first_draw = 0: within 1e-5 per component (the project's parity tolerance) of the oracle's random_cosine_direction through
    the normal's basis in float64, counter 2 afterwards. SPHERE: unit within 1e-5, the oracle's accepted point normalised, counter first_draw
    + 3 x rounds - read off function 8 (which draws the sphere point from counter 2 on, after its cosine direction) and, from counter 0 and
    another one, restated from orc_rng_bits."""
    sc = _cornell()
    points = _generator_points()
    n = len(points)
    sample, key_base, seed = 11, 500, SEED
    keys = key_base + np.arange(n)
    with DeviceScene(sc) as ds:
        rays, kout = ds.irradiance_rays(points, sample, seed=seed, key_base=key_base, mode="cosine")
        rays, kout = rays.cpu().numpy(), kout.cpu().numpy().view(np.uint32)
        local = iu.local_cosine_directions(seed, keys, [sample])[:, 0]
        want = np.stack([iu.world_directions(points[i, 4:7], local[i]) for i in range(n)])
        err = np.abs(rays[:, 4:7].astype(np.float64) - want).max()
        print(f"cosine directions against the CPU prediction: max abs error per component {err:.3e} over {n} points")
        assert err <= 1e-5
        assert np.array_equal(_bits(rays[:, 0:4]), _bits(points[:, 0:4])) and np.array_equal(_bits(rays[:, 7]), _bits(points[:, 7]))
        assert (kout[:, 0] == keys).all() and (kout[:, 1] == 2).all()
        cosn = (rays[:, 4:7].astype(np.float64) * points[:, 4:7]).sum(axis=1)
        assert (cosn >= 0).all()  # the hemisphere about the normal

        # SPHERE from counter 2: function 8's own sphere point
        rays, kout = ds.irradiance_rays(points, sample, seed=seed, key_base=key_base, first_draw=2, mode="sphere")
        rays, kout = rays.cpu().numpy(), kout.cpu().numpy().view(np.uint32)
        p, after = iu.sphere_draws_after_the_cosine(seed, keys, [sample])
        p, after = p[:, 0].astype(np.float64), after[:, 0]
        assert ((after - 2) % 3 == 0).all() and (after > 5).any()  # (some points took more than one round)
        d = rays[:, 4:7].astype(np.float64)
        err_unit, err_dir = np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max(), np.abs(d - p / np.sqrt((p * p).sum(axis=1))[:, None]).max()
        print(f"sphere directions: max |length - 1| {err_unit:.3e}, max abs error per component {err_dir:.3e}")
        assert err_unit <= 1e-5 and err_dir <= 1e-5
        assert (kout[:, 1] == after).all() and (kout[:, 0] == keys).all()

        # SPHERE from counter 0 and from counter 7, explicit keys: restated from the generator's bits
        for first_draw in (0, 7):
            k = np.stack([keys[:24] * 3 + 1, np.full(24, first_draw)], axis=1).astype(np.uint32)
            rays, kout = ds.irradiance_rays(points[:24], sample, seed=seed, keys=k, key_base=99, first_draw=1, mode="sphere")
            rays, kout = rays.cpu().numpy(), kout.cpu().numpy().view(np.uint32)
            for i in range(24):
                q, rounds = _sphere_restated(seed, int(k[i, 0]), sample, first_draw)
                q = q.astype(np.float64)
                assert kout[i].tolist() == [int(k[i, 0]), first_draw + 3 * rounds], (i, kout[i], rounds)
                assert np.abs(rays[i, 4:7] - q / np.sqrt((q * q).sum())).max() <= 1e-5


def test_first_draw_and_keys_shift_the_streams_as_they_do_for_radiance():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        points = surface_points(sc, ds, 4)
        rows = np.repeat(points[:1], 4, axis=0)
        keys = np.array([[11, 2], [12, 2], [11, 2], [11, 4]], dtype=np.uint32)
        for mode in MODES:
            rays, kout = ds.irradiance_rays(rows, 3, seed=SEED, keys=keys, mode=mode)
            rays, kout = rays.cpu().numpy(), kout.cpu().numpy().view(np.uint32)
            assert rays[0].tobytes() == rays[2].tobytes() and rays[0].tobytes() != rays[1].tobytes() and rays[0].tobytes() != rays[3].tobytes()
            if mode == "cosine":
                assert (kout[:, 1] == keys[:, 1] + 2).all()  # two draws from wherever the stream was entered
            again, kagain = ds.irradiance_rays(rows[:2], 3, seed=SEED, key_base=11, first_draw=2, mode=mode)
            assert again.cpu().numpy().tobytes() == rays[:2].tobytes() and kagain.cpu().numpy().view(np.uint32).tobytes() == kout[:2].tobytes()
            rgb, cnt = ds.irradiance(rows, samples=16, seed=SEED, keys=keys, mode=mode)
            assert (cnt == 16).all() and np.isfinite(rgb).all()
            assert rgb[0].tobytes() == rgb[2].tobytes() and rgb[0].tobytes() != rgb[1].tobytes() and rgb[0].tobytes() != rgb[3].tobytes()
            same, _ = ds.irradiance(rows[:2], samples=16, seed=SEED, key_base=11, first_draw=2, mode=mode)
            assert same.tobytes() == rgb[:2].tobytes()
            wrap, _ = ds.irradiance(rows[:2], samples=16, seed=SEED, key_base=0xFFFFFFFF, first_draw=2, mode=mode)
            zero, _ = ds.irradiance(rows[:1], samples=16, seed=SEED, key_base=0, first_draw=2, mode=mode)
            assert wrap[1].tobytes() == zero[0].tobytes()  # key_base + i wraps
        cos, _ = ds.irradiance(rows, samples=16, seed=SEED, keys=keys, mode="cosine")
        assert cos.tobytes() != rgb.tobytes()  # (the mode is read)


# ---- 3. sums that are exact by construction ------------------------------------------------------------------------------------------------
BACKGROUND = (0.5, 0.25, 2.0)  # powers of two below 3: 48 of them add up without rounding, in any order


def _far_geometry():
    b = SceneBuilder()
    world = [b.Sphere((0., 0., -10.), 1., b.Lambertian(b.SolidColor(.5, .5, .5))), b.Sphere((0., 30., 0.), 1., b.DiffuseLight(4., 4., 4.))]
    return b.finish(b.Bvh(world), CameraConfig(40., 0., (0., 0., 3.), (0., 0., -1.), (0., 1., 0.)), BACKGROUND, RC)


def test_a_point_that_sees_nothing_within_its_interval_sums_the_background_exactly():
    """Every direction misses inside [tmin, tmax] - tmax = 2 is shorter than the distance to any geometry (at least 8 from these points) -, so
    every sample is the background: sum == samples x background bit for bit, 48 samples, both modes, through the partial buffer."""
    sc = _far_geometry()
    points = np.array([[0., 0., 0., 0., 0., 0., -1., 2.], [1., -1., 0.5, 0.001, 0.3, 2., 0.1, 2.], [0., 0., 0., 0., 1., 0., 0., 1.]], dtype=np.float32)
    points = np.concatenate([points, [[0., 0., 0., 0., 0., 0., 0., 2.]]]).astype(np.float32)  # and an invalid one
    bg = np.array(BACKGROUND, dtype=np.float32)
    with DeviceScene(sc) as ds:
        for mode in MODES:
            for samples in (48, 7):
                rgb, cnt = ds.irradiance(points, samples=samples, first_sample=2, seed=SEED, mode=mode)
                assert cnt.tolist() == [samples] * 3 + [0], (mode, cnt)
                assert np.array_equal(_bits(rgb[:3]), _bits(np.tile(np.float32(samples) * bg, (3, 1)))), (mode, rgb)
                assert (_bits(rgb[3]) == 0).all()


# ---- 4. the occluder ----------------------------------------------------------------------------------------------------------------------
def _occluder_scene():
    """Background (1, 1, 1); a black Lambertian sphere of radius R centred D along the normal of the point at the origin; the mandatory light,
    a sphere of radius 0.01 a hundred units behind the point's plane (it fills 2.5e-9 of the sphere of directions and emits (1, 1, 1))."""
    w = iu.onb(iu.OCC_NORMAL)[2]
    b = SceneBuilder()
    world = [b.Sphere(tuple(iu.OCC_D * w), iu.OCC_R, b.Lambertian(b.SolidColor(0., 0., 0.))), b.Sphere(tuple(-100. * w), 0.01, b.DiffuseLight(1., 1., 1.))]
    return b.finish(b.Bvh(world), CameraConfig(40., 0., (0., 0., 9.), (0., 0., 0.), (0., 1., 0.)), (1., 1., 1.), RC)


def test_the_occluder_blocks_the_directions_the_cpu_predicts():
    """64 points x 1024 samples. A free direction adds exactly (1, 1, 1), a blocked one exactly 0 (the sphere's albedo is 0): every sum is an
    integer count of free directions, equal in the three channels. COSINE: per point the count is the CPU's (tests/irradiance_util.py) - the
    directions it is sure of, plus at most the borderline ones; at most 0.5 % are borderline in all. SPHERE: the cone fills (1 - 0.8) / 2 of
    the sphere; the free total lies within 5 sqrt(N p (1 - p)) of N (1 - p)."""
    sc = _occluder_scene()
    n, samples = iu.OCC_POINTS, iu.OCC_SAMPLES
    points = np.zeros((n, 8), dtype=np.float32)
    points[:, 4:7], points[:, 7] = iu.OCC_NORMAL, INF
    blocked, borderline = iu.occluder_prediction()
    assert borderline.sum() <= 0.005 * blocked.size
    sure_free = (~blocked & ~borderline).sum(axis=1)
    with DeviceScene(sc) as ds:
        rgb, cnt = ds.irradiance(points, samples=samples, seed=iu.OCC_SEED, key_base=iu.OCC_KEY_BASE, mode="cosine")
        assert (cnt == samples).all()
        assert (rgb == np.rint(rgb)).all() and (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 0] == rgb[:, 2]).all()
        free = rgb[:, 0].astype(np.int64)
        off = int(((free < sure_free) | (free > sure_free + borderline.sum(axis=1))).sum())
        print(f"cosine: free {int(free.sum())} of {n * samples}; predicted {int(sure_free.sum())} + up to {int(borderline.sum())} borderline; points off: {off}")
        assert off == 0, (free, sure_free, borderline.sum(axis=1))
        assert (free[borderline.sum(axis=1) == 0] == sure_free[borderline.sum(axis=1) == 0]).all()

        rgb, cnt = ds.irradiance(points, samples=samples, seed=iu.OCC_SEED, key_base=iu.OCC_KEY_BASE, mode="sphere")
        assert (cnt == samples).all()
        assert (rgb == np.rint(rgb)).all() and (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 0] == rgb[:, 2]).all()
        big_n, p = n * samples, (1.0 - 0.8) / 2.0
        free = float(rgb[:, 0].astype(np.float64).sum())
        print(f"sphere: free {free:.0f} of {big_n}; expected {big_n * (1 - p):.0f} +- {np.sqrt(big_n * p * (1 - p)):.0f}")
        assert abs(free - big_n * (1 - p)) <= 5 * np.sqrt(big_n * p * (1 - p))


# ---- 5. shapes ----------------------------------------------------------------------------------------------------------------------------
def test_batch_shape_order_and_route_do_not_change_a_point_s_answer(monkeypatch):
    """n = 1, 63, 64, 65, 257 and a permutation: answers follow the rows. Device tensors give the host route's bits. A partial buffer bounded to
    128 rows (SOL_RADIANCE_ROWS) - slices of 64 points, windows of two chunks - gives the default bound's bits."""
    import torch
    sc = _cornell()
    rng = np.random.default_rng(9)
    with DeviceScene(sc) as ds:
        points, is_valid = with_invalid_rows(surface_points(sc, ds, 257 - len(INVALID_CLASSES)))
        assert len(points) == 257
        keys = np.stack([rng.integers(0, 2 ** 32, 257), 2 * rng.integers(0, 8, 257)], axis=1).astype(np.uint32)
        perm = rng.permutation(257)
        want = {}
        for mode in MODES:
            for samples in (2, 17, 40):  # one chunk (the kernel answers), two and three (the resolve kernel; three: two windows under the small bound)
                whole, cnt = ds.irradiance(points, samples=samples, first_sample=3, seed=SEED, keys=keys, mode=mode)
                want[mode, samples, "keys"] = (whole, cnt)
                want[mode, samples, None] = ds.irradiance(points, samples=samples, first_sample=3, seed=SEED, key_base=40, mode=mode)
                assert (cnt[is_valid] == samples).all() and (cnt[~is_valid] == 0).all() and len({r.tobytes() for r in whole}) > 1  # (not one constant: the permutation below means something)
                for n in (1, 63, 64, 65, 257):
                    part, c = ds.irradiance(points[:n], samples=samples, first_sample=3, seed=SEED, keys=keys[:n], mode=mode)
                    assert part.tobytes() == whole[:n].tobytes() and (c == cnt[:n]).all(), (mode, samples, n)
                shuffled, c = ds.irradiance(points[perm], samples=samples, first_sample=3, seed=SEED, keys=keys[perm], mode=mode)
                assert shuffled.tobytes() == whole[perm].tobytes() and (c == cnt[perm]).all()
                dev = ds.irradiance(torch.from_numpy(points).cuda(), samples=samples, first_sample=3, seed=SEED, keys=torch.from_numpy(keys.view(np.int32)).cuda(),
                                    mode=mode)
                assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (257, 4)
                dev = dev.cpu().numpy()
                assert np.ascontiguousarray(dev[:, :3]).tobytes() == whole.tobytes() and (np.ascontiguousarray(dev[:, 3]).view(np.uint32) == cnt).all()
        with pytest.raises(ValueError):
            ds.irradiance(torch.from_numpy(points).cuda()[:, :7])
        with pytest.raises(ValueError):
            ds.irradiance(points, mode="ambient")
        with pytest.raises(ValueError):
            ds.irradiance_rays(points[:, :7], 0)
    monkeypatch.setenv("SOL_RADIANCE_ROWS", "128")
    with DeviceScene(sc) as ds:
        for (mode, samples, k), (rgb, cnt) in want.items():
            got, c = ds.irradiance(points, samples=samples, first_sample=3, seed=SEED, keys=keys if k else None, key_base=40, mode=mode)
            assert got.tobytes() == rgb.tobytes() and (c == cnt).all(), (mode, samples, k)


# ---- 6. refusals and neutrality -------------------------------------------------------------------------------------------------------------
def test_refusals():
    point = np.array([[0., 0., 0., 0.001, 0., 1., 0., np.inf]], dtype=np.float32)
    CFG = _abi.SolIrradianceConfig
    cfg = lambda **kw: CFG(**{**dict(size=C.sizeof(CFG), samples=1), **kw})
    with DeviceScene(scenes.create_test_scene(RC)) as ds:  # (a constant medium)
        for f in (lambda: ds.irradiance(point), lambda: ds.irradiance(point, mode="sphere"), lambda: ds.irradiance_rays(point, 0)):
            with pytest.raises(DeviceError) as e:
                f()
            assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        assert ds.lib.sol_irradiance(ds.h, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK  # n == 0 succeeds on any scene
        assert ds.lib.sol_irradiance_dev(ds.h, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK
        assert ds.lib.sol_irradiance_rays(ds.h, None, None, 0, C.byref(cfg()), None, None) == _abi.SOL_OK
    with DeviceScene(_cornell()) as ds:
        lib, out, kout = ds.lib, np.full(8, 7, np.uint32), np.full(2, 7, np.uint32)
        calls = {
            "sol_irradiance": lambda c, pts=point.ctypes.data, n=1, o=out.ctypes.data: lib.sol_irradiance(ds.h, pts, None, n, C.byref(c) if c is not None else None, o),
            "sol_irradiance_dev": lambda c, pts=point.ctypes.data, n=1, o=out.ctypes.data: lib.sol_irradiance_dev(ds.h, pts, None, n, C.byref(c) if c is not None else None, o),
            "sol_irradiance_rays": lambda c, pts=point.ctypes.data, n=1, o=out.ctypes.data: lib.sol_irradiance_rays(ds.h, pts, None, n, C.byref(c) if c is not None else None, o,
                                                                                                             kout.ctypes.data),
        }
        for name, call in calls.items():
            for c, word in ((cfg(samples=0), b"samples"), (cfg(size=24), b"size"), (cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample"),
                            (cfg(mode=2), b"mode"), (None, b"null configuration")):
                assert call(c) == _abi.SOL_EINVAL and word in lib.sol_last_error(), (name, word, lib.sol_last_error())
            assert call(cfg(), n=(1 << 31) + 1) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
            assert call(cfg(), pts=None) == _abi.SOL_EINVAL and b"null point" in lib.sol_last_error()
            assert call(cfg(), o=None) == _abi.SOL_EINVAL and b"null output" in lib.sol_last_error()
            assert call(cfg(), pts=None, n=0, o=None) == _abi.SOL_OK  # n == 0 succeeds and touches nothing
        assert lib.sol_irradiance_rays(ds.h, point.ctypes.data, None, 1, C.byref(cfg()), out.ctypes.data, None) == _abi.SOL_EINVAL
        assert calls["sol_irradiance_rays"](cfg(samples=2)) == _abi.SOL_EINVAL and b"samples" in lib.sol_last_error()
        assert lib.sol_irradiance(None, point.ctypes.data, None, 1, C.byref(cfg()), out.ctypes.data) == _abi.SOL_EINVAL and b"null scene" in lib.sol_last_error()
        assert (out == 7).all() and (kout == 7).all()
        assert calls["sol_irradiance"](cfg(first_sample=0xFFFFFFEF, samples=1)) == _abi.SOL_OK  # the last sample there is
        assert out[3] == 1


def _path_stats(ds):
    st = _abi.SolPathStats()
    st.size = C.sizeof(st)
    ds._chk(ds.lib.sol_path_stats(ds.h, C.byref(st)))
    return st


def test_irradiance_queries_between_renders_change_no_frame_plane_or_statistic():
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))

    def sequence(ds, query):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        query()
        ds.render(8, 8, SEED)
        query()
        ds.render_aux(0, 4, SEED)
        query()
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds))

    with DeviceScene(sc) as ds:
        points = surface_points(sc, ds, 64)

        def query():
            ds.irradiance(points, samples=1, seed=SEED)
            ds.irradiance(points, samples=40, first_sample=3, seed=SEED, key_base=5, mode="sphere")
            ds.irradiance_rays(points, 2, seed=SEED)

        want = sequence(ds, lambda: None)
        assert sequence(ds, query) == want and want[3]["rays"] > 0
        # inside an adaptive session with threshold 0 (every block runs to max_samples)
        ds.clear()
        ds.render(0, 32, SEED)
        frame = ds.read()
        ds.adaptive_begin(16, 16, 32, 0.0)
        assert ds.adaptive_round(SEED) > 0
        query()
        assert ds.adaptive_round(SEED) == 0
        assert ds.read().tobytes() == frame.tobytes() and (ds.adaptive_counts() == 32).all()


def test_radiance_and_irradiance_queries_share_scratch_and_keep_their_own_bits():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        points = surface_points(sc, ds, 130)
        rays = points.copy()  # (as rays: from the surface along the normal)
        rad = lambda: ds.radiance(rays, samples=40, first_sample=1, seed=SEED, key_base=3)[0].tobytes()
        irr = lambda: ds.irradiance(points, samples=40, first_sample=1, seed=SEED, key_base=3)[0].tobytes()
        small = lambda: ds.irradiance(points[:5], samples=17, seed=SEED, mode="sphere")[0].tobytes()
    with DeviceScene(sc) as ds:
        alone_rad = rad()
    with DeviceScene(sc) as ds:
        alone_irr = irr()
    assert alone_rad != alone_irr
    with DeviceScene(sc) as ds:
        assert irr() == alone_irr and rad() == alone_rad and small() and irr() == alone_irr and rad() == alone_rad
    with DeviceScene(sc) as ds:
        assert rad() == alone_rad and irr() == alone_irr
