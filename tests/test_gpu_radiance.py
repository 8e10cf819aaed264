"""Radiance queries on the device (sol_radiance / sol_radiance_dev / sol_camera_ray_keys) against three yardsticks: the render
itself (bit for bit over its own camera rays), the float oracle (for rays the handle's camera never made) and the queries' own invariants -
the summation order, interval, keys, batch shape, validity, refusals, neutrality towards renders. No scene here holds a constant medium but
the one of the refusal case."""
import ctypes as C
import zlib

import numpy as np
import pytest

import orc
import parity_util as pu
from parity_util import env_two_lights as _env_two_lights
from solstrale_amd import (AlbedoShader, CameraConfig, DeviceError, DeviceScene, NormalShader, PathTracingShader, RenderConfig, SceneBuilder, _abi,
                           camera_record, scenes)
from test_gpu_queries import _as_rays, _cornell, _deep_chain, _needles, _random_mixed, _world_box, ray_mix

pytestmark = pytest.mark.gpu
SEED = pu.SEED
INF = np.float32(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _camera_batch(ds, sc, s, seed=SEED):
    """The rays and keys of the whole frame for (s, seed): [n, 8] float32 and [n, 2] int32 device tensors, row-major."""
    rays = ds.camera_rays(0, 0, sc.width, sc.height, s, seed).reshape(-1, 8).contiguous()
    keys = ds.camera_ray_keys(0, 0, sc.width, sc.height, s, seed).reshape(-1, 2).contiguous()
    return rays, keys


def assert_render_identity(ds, sc, s, seed=SEED):
    """radiance over the frame's camera rays and keys, one sample, against clear; render(s, 1); read - on the float bits. Returns the keys."""
    rays, keys = _camera_batch(ds, sc, s, seed)
    rows = ds.radiance(rays, samples=1, first_sample=s, seed=seed, keys=keys).cpu().numpy()
    ds.clear()
    ds.render(s, 1, seed)
    want = ds.read().reshape(-1, 3)
    got = np.ascontiguousarray(rows[:, :3])
    assert np.array_equal(_bits(got), _bits(want)), (s, int((_bits(got) != _bits(want)).any(axis=1).sum()), len(want))
    assert (np.ascontiguousarray(rows[:, 3]).view(np.uint32) == 1).all()  # (every camera ray is valid)
    assert np.isfinite(want).all() and np.abs(want).sum() > 0  # (a Normal frame has negative components)
    return keys.cpu().numpy()


# ---- 1. the render identity, bit for bit ------------------------------------------------------------------------------------------------
def _lens_scene():
    """A thin lens at 64 x 32: the lens disc is drawn by rejection, so first_draw differs from pixel to pixel. The reference's thin-lens scene,
    scenes.create_test_scene, holds a constant medium, which a radiance query refuses (test_refusals; its keys are checked in
    test_keys_of_the_reference_s_thin_lens_scene): the identity is checked on the medium-free thin-lens scene of tests/test_gpu_set_camera.py."""
    from test_gpu_set_camera import _lens_balls
    sc = _lens_balls(RenderConfig(64, 32, 1, PathTracingShader(8)))
    assert sc.desc.camera.lens_radius > 0 and sc.desc.n_mediums == 0
    return sc


def test_keys_of_the_reference_s_thin_lens_scene():
    """scenes.create_test_scene at 64 x 32: pixel = row * W + x, first_draw = 2 + twice the rejection rounds - more than one value."""
    sc = scenes.create_test_scene(RenderConfig(64, 32, 1))
    with DeviceScene(sc) as ds:
        keys = ds.camera_ray_keys(0, 0, 64, 32, 3, SEED).cpu().numpy().reshape(-1, 2)
        part = ds.camera_ray_keys(5, 7, 9, 10, 3, SEED).cpu().numpy()
    assert (keys[:, 0] == np.arange(64 * 32)).all()
    assert len(np.unique(keys[:, 1])) > 1 and (keys[:, 1] >= 4).all() and (keys[:, 1] % 2 == 0).all()
    assert np.array_equal(part, keys.reshape(32, 64, 2)[7:10, 5:9])


@pytest.mark.parametrize("make,env,expect", [(_cornell, {}, {}), (_random_mixed, {}, {}), (_needles, {}, {"strict_triangles": True}),
                                             (_deep_chain, {"SOL_BVH": "ref"}, {"spill": True}), (_lens_scene, {}, {"lens": True})],
                         ids=["cornell", "random_mixed", "needles_strict", "deep_chain_spill", "thin_lens"])
def test_radiance_over_the_camera_rays_is_the_render_bit_for_bit(make, env, expect, monkeypatch):
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
        for s in (0, 37):
            keys = assert_render_identity(ds, sc, s)
            assert (keys[:, 0] == np.arange(sc.width * sc.height)).all()
            if "lens" in expect:
                assert sc.desc.camera.lens_radius > 0 and len(np.unique(keys[:, 1])) > 1
            if sc.desc.camera.lens_radius > 0:  # (the seeded random scene has a thin lens too)
                assert (keys[:, 1] >= 4).all() and (keys[:, 1] % 2 == 0).all()
            else:
                assert (keys[:, 1] == 2).all()


# ---- 2. the oracle, for rays the handle's camera never made -----------------------------------------------------------------------------
class _WithCamera:
    """`scene` with another camera in its description: a copy of the descriptor, as parity_util.WindowScene copies one."""

    def __init__(self, scene, cam):
        self._parent = scene
        self.desc = _abi.SolSceneDesc()
        C.memmove(C.byref(self.desc), C.byref(scene.desc), C.sizeof(_abi.SolSceneDesc))
        self.desc.camera = camera_record(scene.width, scene.height, cam)
        self.desc_ptr = C.pointer(self.desc)
        self.width, self.height = scene.width, scene.height


def _second_camera(sc, name):
    if name == "cornell":
        return CameraConfig(65., 0., (150., 300., 100.), (420., 120., 520.), (0., 1., 0.))
    lo, hi = _world_box(sc)
    return CameraConfig(70., 0., tuple(lo + 0.3 * (hi - lo)), tuple(lo + (hi - lo) * np.array([0.9, 0.4, 0.8])), (0., 1., 0.))


@pytest.mark.parametrize("make", [_cornell, _random_mixed], ids=["cornell", "random_mixed"])
def test_rays_of_another_camera_match_the_float_oracle(make, request):
    """The allowance is the one tests/test_gpu_parity.py gives sol_render on these scenes (assert_parity, max_bad = 0): no pixel outside
    1e-5 relative, max_rel <= 1e-5, the RMSE of the pixels inside below 1e-5."""
    sc = make()
    cam2 = _second_camera(sc, request.node.callspec.id)
    rec1 = _abi.SolCamera.from_buffer_copy(sc.desc.camera)
    other = _WithCamera(sc, cam2)
    with DeviceScene(sc) as ds:
        for s in (0, 5):
            ds.set_camera(cam2)
            rays, keys = _camera_batch(ds, sc, s)
            ds.set_camera(rec1)
            back = ds.camera_rays(0, 0, sc.width, sc.height, s, SEED).reshape(-1, 8)
            assert not np.array_equal(back.cpu().numpy(), rays.cpu().numpy())  # (the handle looks through its first camera again)
            rows = ds.radiance(rays, samples=1, first_sample=s, seed=SEED, keys=keys).cpu().numpy()
            img = np.ascontiguousarray(rows[:, :3]).reshape(sc.height, sc.width, 3)
            ref, _ = orc.render(other, s, 1, SEED, real=orc.ORC_F32)
            res = pu.compare(img, ref, 1)
            print(request.node.callspec.id, s, res)
            assert np.isfinite(img).all() and img.sum() > 0
            assert res["bad_pixels"] == 0 and res["max_rel"] <= pu.REL_TOL and res["rmse_mean_good"] < 1e-5, res


# ---- 3. several samples -----------------------------------------------------------------------------------------------------------------
def _render_association(per_sample):
    """per_sample: [k, n, 3] float32 colours of samples first .. first + k - 1. Chunk sums of up to 16 samples counted from the first one,
    each 0 + c + c + .. in sample order, then the chunks in order on top of 0: sol_resolve_kernel's association, in numpy float32."""
    k, n = per_sample.shape[0], per_sample.shape[1]
    total = np.zeros((n, 3), dtype=np.float32)
    for c0 in range(0, k, 16):
        chunk = np.zeros((n, 3), dtype=np.float32)
        for j in range(c0, min(c0 + 16, k)):
            chunk = chunk + per_sample[j]
        total = total + chunk
    assert total.dtype == np.float32
    return total


def test_several_samples_are_added_in_the_render_s_order():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        rays = ray_mix(sc, ds, 71, 75)
        assert rays.shape == (300, 8)
        per = []
        for s in range(5, 5 + 48):
            rgb, cnt = ds.radiance(rays, samples=1, first_sample=s, seed=SEED, key_base=7)
            assert (cnt == 1).all()
            per.append(rgb)
        per = np.stack(per)
        assert len({p.tobytes() for p in per}) == 48  # (every sample is another path)
        for k in (1, 15, 16, 17, 48):
            rgb, cnt = ds.radiance(rays, samples=k, first_sample=5, seed=SEED, key_base=7)
            want = _render_association(per[:k])
            assert np.array_equal(_bits(rgb), _bits(want)), (k, int((_bits(rgb) != _bits(want)).any(axis=1).sum()))
            assert (cnt == k).all()


def test_thirty_two_samples_over_one_frame_s_camera_rays():
    """The rays and keys of Cornell's pinhole frame for sample 0, queried with samples = 32. A render of 32 samples makes new camera rays for
    every sample (the pixel jitter), so this is NOT the 32-sample frame: the yardstick is the float32 sum, in the render's association (two
    chunks of 16, each added in sample order), of 32 single-sample queries of the same rays and keys."""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        rays, keys = _camera_batch(ds, sc, 0)
        per = np.stack([np.ascontiguousarray(ds.radiance(rays, samples=1, first_sample=s, seed=SEED, keys=keys).cpu().numpy()[:, :3]) for s in range(32)])
        rows = ds.radiance(rays, samples=32, first_sample=0, seed=SEED, keys=keys).cpu().numpy()
        ds.clear()
        ds.render(0, 1, SEED)
        assert np.array_equal(_bits(per[0]), _bits(ds.read().reshape(-1, 3)))  # (sample 0 of it is the render's)
    assert np.array_equal(_bits(rows[:, :3]), _bits(_render_association(per)))
    assert (np.ascontiguousarray(rows[:, 3]).view(np.uint32) == 32).all()


# ---- 4. interval and keys ---------------------------------------------------------------------------------------------------------------
BACKGROUND = (0.1, 0.2, 0.3)


def _light_stack():
    """test_gpu_queries._quad_stack with each of the five quads a DiffuseLight of its own power-of-two colour, facing +z."""
    b = SceneBuilder()
    world = [b.Quad((-1., -1., -float(k)), (2., 0., 0.), (0., 2., 0.), b.DiffuseLight(2.0 ** k, 2.0 ** -k, 2.0 ** (k - 3))) for k in range(1, 6)]
    cam = CameraConfig(40., 0., (0., 0., 3.), (0., 0., -1.), (0., 1., 0.))
    return b.finish(b.Bvh(world), cam, BACKGROUND, RenderConfig(32, 32, 1))


def test_the_first_search_runs_over_the_ray_s_own_interval():
    sc = _light_stack()
    with DeviceScene(sc) as ds:
        ray = _as_rays(np.array([[0.1, 0.2, 0.5]]), np.array([[0., 0., -2.]]))  # |d| = 2: quad k lies at t = (k + 0.5) / 2
        for k in range(1, 6):
            t_k = np.float32((k + 0.5) / 2)
            hit = ds.closest_hits(ray)[0]
            assert hit["status"] == _abi.SOL_RAY_HIT and hit["t"] == t_k, (k, hit)
            rgb, cnt = ds.radiance(ray, samples=1, seed=SEED)
            assert rgb[0].tolist() == [2.0 ** k, 2.0 ** -k, 2.0 ** (k - 3)] and cnt[0] == 1, (k, rgb)
            ray[0, 3] = np.nextafter(t_k, INF)  # just past quad k: the next answer is quad k + 1's emission
        rgb, _ = ds.radiance(ray, samples=1, seed=SEED)
        assert np.array_equal(_bits(rgb[0]), _bits(np.array(BACKGROUND, dtype=np.float32)))  # behind the last quad
        ray[0, 3], ray[0, 7] = 0.0, 0.5  # tmax short of the first quad
        rgb, cnt = ds.radiance(ray, samples=3, seed=SEED)
        bg = np.array(BACKGROUND, dtype=np.float32)
        assert np.array_equal(_bits(rgb[0]), _bits((np.zeros(3, np.float32) + bg) + bg + bg)) and cnt[0] == 3
        ray[0, 7] = 0.75  # the interval is closed: tmax on the first quad hits it
        assert ds.radiance(ray, samples=1, seed=SEED)[0][0].tolist() == [2.0, 0.5, 0.25]


def test_the_key_names_the_random_stream():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        one = _as_rays(np.array([[278., 278., -100.]]), np.array([[0.1, -0.4, 1.0]]))  # onto the Lambertian floor
        rays = np.repeat(one, 4, axis=0)
        keys = np.array([[11, 2], [12, 2], [11, 2], [11, 4]], dtype=np.uint32)
        rgb, cnt = ds.radiance(rays, samples=16, seed=SEED, keys=keys)
        assert (cnt == 16).all() and np.isfinite(rgb).all()
        assert not np.array_equal(_bits(rgb[0]), _bits(rgb[1]))  # another pixel key: another stream
        assert np.array_equal(_bits(rgb[0]), _bits(rgb[2]))      # the same key: the same bits
        assert not np.array_equal(_bits(rgb[0]), _bits(rgb[3]))  # another first draw: the stream read from another place
        # keys = None is (key_base + i, first_draw)
        again, _ = ds.radiance(rays[:2], samples=16, seed=SEED, key_base=11, first_draw=2)
        assert np.array_equal(_bits(again), _bits(rgb[:2]))
        wrap, _ = ds.radiance(rays[:2], samples=16, seed=SEED, key_base=0xFFFFFFFF, first_draw=2)
        zero, _ = ds.radiance(rays[:1], samples=16, seed=SEED, key_base=0, first_draw=2)
        assert np.array_equal(_bits(wrap[1]), _bits(zero[0]))  # key_base + i wraps


def test_batch_shape_and_order_do_not_change_a_ray_s_answer():
    """n = 1, 63, 64, 65, 255, 257 and 4097 cross wave, workgroup and reservation boundaries: each batch gives the rows of the same prefix of
    one large batch, and a permuted batch with its keys permuted alongside the permuted rows."""
    sc = _random_mixed()
    rng = np.random.default_rng(9)
    with DeviceScene(sc) as ds:
        rays = np.concatenate([ray_mix(sc, ds, 21, 512), ray_mix(sc, ds, 22, 513)])[:4097]
        keys = np.stack([rng.integers(0, 2 ** 32, len(rays)), 2 * rng.integers(0, 8, len(rays))], axis=1).astype(np.uint32)
        whole, cnt = ds.radiance(rays, samples=2, first_sample=3, seed=SEED, keys=keys)
        assert (cnt == 2).all() and len({r.tobytes() for r in whole}) > 100
        for n in (1, 63, 64, 65, 255, 257, 4097):
            part, c = ds.radiance(rays[:n], samples=2, first_sample=3, seed=SEED, keys=keys[:n])
            assert part.tobytes() == whole[:n].tobytes() and (c == 2).all(), n
        perm = rng.permutation(len(rays))
        shuffled, _ = ds.radiance(rays[perm], samples=2, first_sample=3, seed=SEED, keys=keys[perm])
        assert shuffled.tobytes() == whole[perm].tobytes()
        many, c = ds.radiance(rays[:257], samples=17, first_sample=3, seed=SEED, keys=keys[:257])  # (the same through the partial buffer)
        shuffled, _ = ds.radiance(rays[perm[:257]], samples=17, first_sample=3, seed=SEED, keys=keys[perm[:257]])
        sel = np.nonzero(perm[:257] < 257)[0]
        assert (c == 17).all() and shuffled[sel].tobytes() == many[perm[:257][sel]].tobytes()


def test_a_small_partial_buffer_splits_the_call_and_changes_no_bit(monkeypatch):
    """SOL_RADIANCE_ROWS bounds the partial buffer (default 2^24 rows). With 128 rows a call of 257 rays and more than one chunk is split
    into slices of 64 rays, and beyond two chunks per ray into windows of two chunks whose sums the resolve kernel carries on: the rows
    are those of a handle with the default bound. One chunk goes straight to the output either way."""
    sc = _cornell()
    rng = np.random.default_rng(13)
    with DeviceScene(sc) as ds:
        rays = ray_mix(sc, ds, 81, 65)[:257]
        rays[100, 4:7] = 0.0  # an invalid one, in the second slice
        keys = np.stack([rng.integers(0, 2 ** 32, len(rays)), np.full(len(rays), 2)], axis=1).astype(np.uint32)
        cases = [(s, k) for s in (1, 17, 32, 33, 80) for k in (keys, None)]
        want = [ds.radiance(rays, samples=s, first_sample=3, seed=SEED, keys=k, key_base=40) for s, k in cases]
    monkeypatch.setenv("SOL_RADIANCE_ROWS", "128")
    with DeviceScene(sc) as ds:
        for (s, k), (rgb, cnt) in zip(cases, want):
            got, c = ds.radiance(rays, samples=s, first_sample=3, seed=SEED, keys=k, key_base=40)
            assert got.tobytes() == rgb.tobytes() and (c == cnt).all(), s
            assert c[100] == 0 and (np.delete(c, 100) == s).all()
        import torch
        dev = ds.radiance(torch.from_numpy(rays).cuda(), samples=80, first_sample=3, seed=SEED, key_base=40).cpu().numpy()
        assert np.ascontiguousarray(dev[:, :3]).tobytes() == want[-1][0].tobytes()


# ---- 5. modes ---------------------------------------------------------------------------------------------------------------------------
def _mode_cases():
    import test_env_importance as te
    return {
        "env_importance": (lambda: te._lambertian_scene(RenderConfig(64, 48, 1, PathTracingShader(6))), "importance", None),
        "light_tree": (lambda: scenes.many_lights(64, "quads", RenderConfig(48, 48, 1, PathTracingShader(50))), None, "tree"),
        "light_power": (lambda: scenes.mixed_power_lights(64, RenderConfig(64, 64, 1, PathTracingShader(6))), None, "power"),
        "env_and_tree": (lambda: _env_two_lights(RenderConfig(64, 48, 1, PathTracingShader(8))), "importance", "tree"),
    }


@pytest.mark.parametrize("name", ["env_importance", "light_tree", "light_power", "env_and_tree"])
def test_the_render_identity_holds_in_every_sampling_mode(name):
    make, env, light = _mode_cases()[name]
    sc = make()
    assert sc.desc.n_mediums == 0
    with DeviceScene(sc) as ds:
        rays, keys = _camera_batch(ds, sc, 1)
        plain = ds.radiance(rays, samples=1, first_sample=1, seed=SEED, keys=keys).cpu().numpy()
        if env:
            ds.env_sampling(env)
        if light:
            ds.light_sampling(light)
        for s in (1, 20):
            assert_render_identity(ds, sc, s)
        moded = ds.radiance(rays, samples=1, first_sample=1, seed=SEED, keys=keys).cpu().numpy()
        if name != "light_tree":  # (the tree alone gives the uniform frames: DESIGN.md 14)
            assert moded.tobytes() != plain.tobytes()  # the query follows the handle's mode
        if env:
            ds.env_sampling(None)
        if light:
            ds.light_sampling(None)
        assert ds.radiance(rays, samples=1, first_sample=1, seed=SEED, keys=keys).cpu().numpy().tobytes() == plain.tobytes()


@pytest.mark.parametrize("shader", [AlbedoShader(), NormalShader()], ids=["albedo", "normal"])
def test_the_render_identity_holds_under_the_albedo_and_normal_shaders(shader):
    sc = scenes.cornell_box(RenderConfig(64, 64, 1, shader))
    with DeviceScene(sc) as ds:
        for s in (0, 9):
            assert_render_identity(ds, sc, s)


# ---- 6. validity, refusals, neutrality, device route ------------------------------------------------------------------------------------
def test_invalid_rays_answer_zero_and_leave_their_neighbours_alone():
    sc = _random_mixed()
    nan = np.float32(np.nan)
    # (the classes tests/test_gpu_queries.py enumerates)
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
        keys = np.stack([np.arange(len(mixed)), np.full(len(mixed), 2)], axis=1).astype(np.uint32)
        for samples in (1, 20):  # the kernel's own answer, and the resolve kernel's
            alone, cnt_alone = ds.radiance(valid, samples=samples, seed=SEED, keys=keys[is_valid])
            rgb, cnt = ds.radiance(mixed, samples=samples, seed=SEED, keys=keys)
            assert (cnt[~is_valid] == 0).all() and (_bits(rgb[~is_valid]) == 0).all()
            assert (cnt[is_valid] == samples).all() and (cnt_alone == samples).all()
            assert rgb[is_valid].tobytes() == alone.tobytes()


def test_refusals():
    ray = _as_rays(np.zeros((1, 3)), np.ones((1, 3)))
    with DeviceScene(scenes.create_test_scene(RenderConfig(32, 32, 1))) as ds:  # (a constant medium)
        with pytest.raises(DeviceError) as e:
            ds.radiance(ray)
        assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        assert tuple(ds.camera_ray_keys(0, 0, 4, 2, 0, 1).shape) == (2, 4, 2)  # (keys need no search)
        cfg1 = _abi.SolRadianceConfig(size=C.sizeof(_abi.SolRadianceConfig), samples=1)
        assert ds.lib.sol_radiance(ds.h, None, None, 0, C.byref(cfg1), None) == _abi.SOL_OK  # n == 0 succeeds on any scene
    with DeviceScene(_cornell()) as ds:
        lib, out = ds.lib, np.full(4, 7, np.uint32)
        cfg = lambda **kw: _abi.SolRadianceConfig(**{**dict(size=C.sizeof(_abi.SolRadianceConfig), samples=1), **kw})
        call = lambda c, rays=ray.ctypes.data, n=1, o=out.ctypes.data: lib.sol_radiance(ds.h, rays, None, n, C.byref(c) if c is not None else None, o)
        for c, word in ((cfg(samples=0), b"samples"), (cfg(size=24), b"size"), (cfg(reserved=1), b"reserved"),
                        (cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample"), (None, b"null configuration")):
            assert call(c) == _abi.SOL_EINVAL and word in lib.sol_last_error(), (word, lib.sol_last_error())
        assert call(cfg(), n=(1 << 31) + 1) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
        assert call(cfg(), rays=None) == _abi.SOL_EINVAL and b"null" in lib.sol_last_error()
        assert call(cfg(), o=None) == _abi.SOL_EINVAL
        assert lib.sol_radiance_dev(ds.h, None, None, 1, C.byref(cfg()), None) == _abi.SOL_EINVAL
        assert (out == 7).all()
        assert call(cfg(), rays=None, n=0, o=None) == _abi.SOL_OK  # n == 0 succeeds and touches nothing
        assert lib.sol_radiance_dev(ds.h, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK
        assert call(cfg(first_sample=0xFFFFFFEF, samples=1)) == _abi.SOL_OK  # the last sample there is
        for rect in ((0, 0, 0, 1), (3, 0, 3, 4), (0, 0, 65, 1), (0, 5, 4, 5), (0, 0, 4, 65), (70, 0, 80, 4)):
            with pytest.raises(DeviceError) as e:
                ds.camera_ray_keys(*rect, 0, 1)
            assert e.value.code == _abi.SOL_EINVAL, rect


def test_radiance_queries_between_renders_change_no_frame_plane_or_statistic():
    sc = scenes.cornell_box(RenderConfig(64, 64, 16))

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
        rays = ray_mix(sc, ds, 51, 64)

        def query():
            ds.radiance(rays, samples=1, seed=SEED)
            ds.radiance(rays, samples=40, first_sample=3, seed=SEED, key_base=5)

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


def _path_stats(ds):
    st = _abi.SolPathStats()
    st.size = C.sizeof(st)
    ds._chk(ds.lib.sol_path_stats(ds.h, C.byref(st)))
    return st


def test_device_tensors_give_the_host_route_s_rows():
    import torch
    sc = _random_mixed()
    with DeviceScene(sc) as ds:
        rays = ray_mix(sc, ds, 61, 300)
        rays[::7, 7] = 4.0
        rays[5, 4:7] = 0.0  # an invalid one
        keys = np.stack([np.arange(len(rays)) * 3, np.full(len(rays), 2)], axis=1).astype(np.uint32)
        dev, dkeys = torch.from_numpy(rays).cuda(), torch.from_numpy(keys.view(np.int32)).cuda()
        for samples, k, dk in ((1, keys, dkeys), (33, keys, dkeys), (5, None, None)):
            rgb, cnt = ds.radiance(rays, samples=samples, seed=SEED, keys=k, key_base=9)
            rows = ds.radiance(dev, samples=samples, seed=SEED, keys=dk, key_base=9)
            assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == (len(rays), 4)
            rows = rows.cpu().numpy()
            assert np.ascontiguousarray(rows[:, :3]).tobytes() == rgb.tobytes()
            assert (np.ascontiguousarray(rows[:, 3]).view(np.uint32) == cnt).all() and cnt[5] == 0 and cnt[4] == samples
        with pytest.raises(ValueError):
            ds.radiance(dev[:, :7])
        with pytest.raises(ValueError):
            ds.radiance(dev, keys=dkeys[:-1])
        with pytest.raises(ValueError):
            ds.radiance(dev.double())


def test_the_render_identity_holds_after_a_light_was_moved():
    import primitive_util as prim
    from test_gpu_set_primitives import _three_lights
    sc = _three_lights()
    rows = prim.rows_of(sc.desc)
    new, kinds = prim.light_moved(sc.desc, rows)
    assert kinds
    with DeviceScene(sc, dynamic_primitives=True) as ds:
        rays, keys = _camera_batch(ds, sc, 2)
        before = ds.radiance(rays, samples=1, first_sample=2, seed=SEED, keys=keys).cpu().numpy()
        ds.set_primitives(**{k: new[k] for k in kinds})
        assert_render_identity(ds, sc, 2)
        after = ds.radiance(rays, samples=1, first_sample=2, seed=SEED, keys=keys).cpu().numpy()
        assert after.tobytes() != before.tobytes()  # (the query sees the moved lights)
