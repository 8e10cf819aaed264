"""Irradiance moments on the device (sol_irradiance_moments / sol_irradiance_moments_dev). The anchor is the identity with what the
call replaces: per sample, sol_irradiance_rays writes the ray and key and sol_radiance over them answers the sample's colour c_s; the six sums are
sol_radiance's association of c_s and of fl(c_s x c_s), restated in numpy float32 (tests/lightmap_filter_var_ref.py, moments_of_samples) - bit for
bit - and (r, g, b, samples) is sol_irradiance's answer to the same call. Around it: every estimator kernel, batch shapes, keys, both routes, a
stream of the caller's, the splits of the partial buffer in child processes of their own, refusals and neutrality. Frames are 32 x 32."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import lightmap_filter_var_ref as vr
from solstrale_amd import MOMENTS_DTYPE, DeviceError, DeviceScene, RenderConfig, _abi, moments_to_numpy, scenes
from test_gpu_irradiance import INVALID_CLASSES, MODES, RC, SEED, _cornell, _path_stats, _random_mixed, _variation, surface_points, with_invalid_rows
from test_gpu_irradiance_sh import per_sample

pytestmark = pytest.mark.gpu


def _words(rows):
    return np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 8)


def assert_moments_identity(ds, points, is_valid=None, ks=(1, 17), first=5, key_base=7, modes=MODES):
    """irradiance_moments(points, samples = k, first_sample = first) against the association of c_s and fl(c_s x c_s) over the per-sample round
    trip, and its first four words against irradiance() for the same call: bit for bit."""
    is_valid = np.ones(len(points), bool) if is_valid is None else is_valid
    for mode in modes:
        cols, _ = per_sample(ds, points, range(first, first + max(ks)), key_base=key_base, mode=mode, is_valid=is_valid)
        assert np.isfinite(cols).all() and np.abs(cols).sum() > 0  # (something arrives somewhere)
        for k in ks:
            got = ds.irradiance_moments(points, samples=k, first_sample=first, seed=SEED, key_base=key_base, mode=mode)
            assert got.dtype == MOMENTS_DTYPE and got.shape == (len(points),)
            want = vr.moments_of_samples(cols[:k], valid=is_valid)
            off = int((_words(got) != _words(want)).any(axis=1).sum())
            assert off == 0, (mode, k, off, len(points))
            assert (_words(got)[~is_valid] == 0).all() and (got["samples"][is_valid] == k).all() and (got["reserved"] == 0).all(), (mode, k)
            rgb, cnt = ds.irradiance(points, samples=k, first_sample=first, seed=SEED, key_base=key_base, mode=mode)
            assert got["sum"].tobytes() == rgb.tobytes() and (got["samples"] == cnt).all(), (mode, k, "sol_irradiance's answer")
            assert (got["sum2"][is_valid] >= 0).all() and (got["sum2"][is_valid].sum(axis=1) > 0).any()


# ---- 1. the identity, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_cornell, _random_mixed], ids=["cornell", "random_mixed"])
def test_the_six_sums_are_the_association_over_the_per_sample_round_trip(make):
    sc = make()
    assert sc.desc.n_mediums == 0
    with DeviceScene(sc) as ds:
        points, is_valid = with_invalid_rows(surface_points(sc, ds, 300))
        assert len(points) == 300 + len(INVALID_CLASSES)
        assert_moments_identity(ds, points, is_valid, ks=(1, 15, 16, 17, 48))


@pytest.mark.parametrize("name", ["env_importance", "light_tree", "light_power", "needles_strict", "deep_chain_spill"])
def test_the_identity_holds_in_every_estimator_kernel(name, monkeypatch):
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
        if env_mode:
            ds.env_sampling(env_mode)
        if light_mode:
            ds.light_sampling(light_mode)
        assert_moments_identity(ds, points)


# ---- 2. shapes ------------------------------------------------------------------------------------------------------------------------------
CASES = [(mode, samples, use_keys) for mode in MODES for samples in (2, 40) for use_keys in (True, False)]  # 40: three chunks, the last one short


def _shape_inputs(ds, sc):
    rng = np.random.default_rng(9)
    points, is_valid = with_invalid_rows(surface_points(sc, ds, 257 - len(INVALID_CLASSES)))
    keys = np.stack([rng.integers(0, 2 ** 32, 257), 3 * rng.integers(0, 2, 257)], axis=1).astype(np.uint32)  # first_draw 0 and 3
    return points, is_valid, keys


def _answer(ds, points, keys, case, first_draw=0):
    mode, samples, use_keys = case
    return ds.irradiance_moments(points, samples=samples, first_sample=3, seed=SEED, keys=keys if use_keys else None, key_base=40, first_draw=first_draw, mode=mode)


CHILD = """
import sys
import numpy as np
from solstrale_amd import DeviceScene, RenderConfig, scenes
a = np.load(sys.argv[1])
out = {}
with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
    for k in range(int(a["n"])):
        mode, samples, use_keys = str(a[f"mode{k}"]), int(a[f"samples{k}"]), bool(a[f"keys{k}"])
        out[f"rows{k}"] = ds.irradiance_moments(a["points"], samples=samples, first_sample=3, seed=int(a["seed"]), keys=a["keys"] if use_keys else None, key_base=40,
                                                mode=mode).view(np.uint32).reshape(-1, 8)
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def shapes():
    """The 257 rows, their keys and the default bound's answers to CASES: computed once, shared by the tests below and left unchanged."""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        points, is_valid, keys = _shape_inputs(ds, sc)
        want = {case: _answer(ds, points, keys, case) for case in CASES}
    return points, is_valid, keys, want


def test_batch_shape_order_keys_and_route_do_not_change_a_point_s_answer(shapes):
    """n = 1, 63, 64, 65, 257 and a permutation: answers follow the rows. Keys carry first_draw 0 and 3; without keys key_base and first_draw shift the
    streams. Device tensors - also on a stream of the caller's - give the host route's bits."""
    import torch
    points, is_valid, keys, want = shapes
    assert len(points) == 257
    perm = np.random.default_rng(10).permutation(257)
    with DeviceScene(_cornell()) as ds:
        for case in CASES:
            whole = want[case]
            assert (whole["samples"][is_valid] == case[1]).all() and (_words(whole)[~is_valid] == 0).all() and len({r.tobytes() for r in whole}) > 1
            for n in (1, 63, 64, 65):
                part = _answer(ds, points[:n], keys[:n], case)
                assert part.tobytes() == whole[:n].tobytes(), (case, n)
            if case[2]:
                assert _answer(ds, points[perm], keys[perm], case).tobytes() == whole[perm].tobytes(), (case, "a permutation")
                continue
            # without keys row i draws from key_base + i: the permuted call differs, and a window of the rows with its own key_base does not
            mode, samples, _ = case
            tail = ds.irradiance_moments(points[100:], samples=samples, first_sample=3, seed=SEED, key_base=140, mode=mode)
            assert tail.tobytes() == whole[100:].tobytes(), case
            shifted = _answer(ds, points, None, case, first_draw=3)
            assert shifted.tobytes() != whole.tobytes() and (shifted["samples"] == whole["samples"]).all()
            k3 = np.stack([40 + np.arange(257), np.full(257, 3)], axis=1).astype(np.uint32)
            assert ds.irradiance_moments(points, samples=samples, first_sample=3, seed=SEED, keys=k3, mode=mode).tobytes() == shifted.tobytes(), case
        stream = torch.cuda.Stream()
        for own in (False, True):
            if own:
                ds.set_stream(stream.cuda_stream)
            try:
                for case in CASES[::3]:
                    dev = ds.irradiance_moments(torch.from_numpy(points).cuda(), samples=case[1], first_sample=3, seed=SEED,
                                                keys=torch.from_numpy(keys.view(np.int32)).cuda() if case[2] else None, key_base=40, mode=case[0])
                    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (257, 8)
                    assert moments_to_numpy(dev).tobytes() == want[case].tobytes(), (case, own)
                    if own:
                        assert _answer(ds, points, keys, case).tobytes() == want[case].tobytes(), (case, "host route on the caller's stream")
            finally:
                ds.set_stream(0)
        with pytest.raises(ValueError):
            ds.irradiance_moments(torch.from_numpy(points).cuda()[:, :7])
        with pytest.raises(ValueError):
            ds.irradiance_moments(points, mode="ambient")


@pytest.mark.parametrize("rows", ["2048", "128"])
def test_the_partial_buffer_s_bound_does_not_change_a_point_s_answer(rows, shapes, tmp_path):
    """SOL_RADIANCE_ROWS is read at creation: each bound runs in a fresh child process of its own. 2048 rows: 257 points x 40 samples go in slices of
    64 points and windows of two chunks and one, the sums carried in `out`; 128 rows is below the floor of one group x one chunk."""
    points, _, keys, want = shapes
    arrays = {"n": len(CASES), "points": points, "keys": keys, "seed": SEED}
    for k, (mode, samples, use_keys) in enumerate(CASES):
        arrays.update({f"mode{k}": mode, f"samples{k}": samples, f"keys{k}": use_keys})
    np.savez(tmp_path / "in.npz", **arrays)
    env = {**os.environ, "SOL_RADIANCE_ROWS": rows, "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    for k, case in enumerate(CASES):
        assert (got[f"rows{k}"] == _words(want[case])).all(), (rows, case)


# ---- 3. refusals and neutrality ----------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_handle():
    point = np.array([[0., 0., 0., 0.001, 0., 1., 0., np.inf]], dtype=np.float32)
    CFG = _abi.SolIrradianceConfig
    cfg = lambda **kw: CFG(**{**dict(size=C.sizeof(CFG), samples=1), **kw})
    with DeviceScene(scenes.create_test_scene(RC)) as ds:  # (a constant medium)
        for f in (lambda: ds.irradiance_moments(point), lambda: ds.irradiance_moments(point, mode="sphere")):
            with pytest.raises(DeviceError) as e:
                f()
            assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        assert ds.lib.sol_irradiance_moments(ds.h, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK  # n == 0 succeeds on any scene
        assert ds.lib.sol_irradiance_moments_dev(ds.h, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK
    with DeviceScene(_cornell()) as ds:
        lib, out = ds.lib, np.full(8, 7, np.uint32)
        for name, fn in (("sol_irradiance_moments", lib.sol_irradiance_moments), ("sol_irradiance_moments_dev", lib.sol_irradiance_moments_dev)):
            call = lambda c, pts=point.ctypes.data, n=1, o=out.ctypes.data: fn(ds.h, pts, None, n, C.byref(c) if c is not None else None, o)
            for c, word in ((cfg(samples=0), b"samples"), (cfg(size=24), b"size"), (cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample"),
                            (cfg(mode=2), b"mode"), (None, b"null configuration")):
                assert call(c) == _abi.SOL_EINVAL and word in lib.sol_last_error() and name.encode() + b":" in lib.sol_last_error(), (name, word, lib.sol_last_error())
            assert call(cfg(), n=(1 << 31) + 1) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
            assert call(cfg(), pts=None) == _abi.SOL_EINVAL and b"null point" in lib.sol_last_error()
            assert call(cfg(), o=None) == _abi.SOL_EINVAL and b"null output" in lib.sol_last_error()
            assert call(cfg(), pts=None, n=0, o=None) == _abi.SOL_OK  # n == 0 succeeds and touches nothing
        assert (out == 7).all()
        assert lib.sol_irradiance_moments(ds.h, point.ctypes.data, None, 1, C.byref(cfg(first_sample=0xFFFFFFEF, samples=1)), out.ctypes.data) == _abi.SOL_OK
        assert out[3] == 1 and out[7] == 0  # the last sample there is


def test_moments_queries_between_renders_change_no_frame_plane_statistic_or_other_query():
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))

    def sequence(ds, points, query):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        query()
        ds.render(8, 8, SEED)
        query()
        ds.render_aux(0, 4, SEED)
        query()
        irr = ds.irradiance(points, samples=20, first_sample=1, seed=SEED, key_base=3)[0]
        query()
        sh = ds.irradiance_sh(points, samples=20, first_sample=1, seed=SEED, key_base=3)[0]
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(irr.tobytes()), zlib.crc32(sh.tobytes()))

    with DeviceScene(sc) as ds:
        points = surface_points(sc, ds, 64)

        def query():
            ds.irradiance_moments(points, samples=1, seed=SEED)
            ds.irradiance_moments(points, samples=40, first_sample=3, seed=SEED, key_base=5, mode="sphere")

        want = sequence(ds, points, lambda: None)
        assert sequence(ds, points, query) == want and want[3]["rays"] > 0
