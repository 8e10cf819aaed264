"""Directional distance moments on the device (sol_visibility_oct, sol_volume_build_depth, sol_volume_sample_depth). The anchor
is the identity with the ray queries: sol_irradiance_rays writes the ray of a sample, sol_query answers it, and a map's four sums per texel are
sol_radiance's association of the lobe-weighted answers, restated in numpy float32 (tests/depth_ref.py) and compared word for word. Around it:
batch shapes, invalid rows between guard rows, the splits of a bounded partial buffer, both projection kernels, the routes, build and sample
against the restatement, the chain in a scene with a wall, refusals on a handle and neutrality. Frames are at most 64 x 64."""
import ctypes as C
import zlib

import numpy as np
import pytest

import depth_ref as dr
import parity_util as pu
import volume_ref as vr
from solstrale_amd import CameraConfig, DeviceError, DeviceScene, RenderConfig, SceneBuilder, VolumeGrid, _abi, scenes
from test_gpu_irradiance import INVALID_CLASSES, _cornell, _deep_chain, _needles, _path_stats, _random_mixed, with_invalid_rows
from test_gpu_visibility import hit_points, per_sample_answers
from test_gpu_volume import FLAG_IDS, FLAGS, assert_words_equal, grid_of, points, probes, random_sums  # noqa: F401  (points, probes: module fixtures)

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F, U = np.float32, np.uint32
INF, NAN = F(np.inf), F(np.nan)
RC = RenderConfig(32, 32, 1)
HIT, MISS, INVALID = _abi.SOL_RAY_HIT, _abi.SOL_RAY_MISS, _abi.SOL_RAY_INVALID
G = 64  # guard rows on either side of an output


def restate(res, sharpness, status, t, dirs, k, is_valid=None):
    return dr.accumulate(res, sharpness, dirs[:k], t[:k], status[:k] == HIT, status[:k] != INVALID, is_valid)


def assert_maps_equal(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.view(U).reshape(got.shape[0], -1), want.view(U).reshape(want.shape[0], -1)
    if (g != w).any():
        bad = np.nonzero((g != w).any(axis=1))[0]
        tex = np.nonzero(g[bad[0]] != w[bad[0]])[0]
        raise AssertionError((what, len(bad), len(g), bad[:5], tex[:8], got.reshape(len(g), -1)[bad[0], tex[:8]], want.reshape(len(g), -1)[bad[0], tex[:8]]))


# ---- 1. the identity with the ray queries, bit for bit --------------------------------------------------------------------------------------
KS = (1, 15, 16, 17, 48)
FIRST = 5
COMBOS = (("cosine", False, 0), ("cosine", True, 3), ("sphere", False, 3), ("sphere", True, 0))
# (res, sharpness_log2): a Latin square - every res with every sharpness over the three rows; row (combo + k) % 3 runs for a given combo and k, so every
# pair meets both modes, keys and key_base, both first_draws, and sample counts on either side of a chunk
PAIRS = (((4, 0), (8, 5), (16, 6)), ((4, 5), (8, 6), (16, 0)), ((4, 6), (8, 0), (16, 5)))


@pytest.mark.parametrize("make, env, expect", [(_cornell, {}, {}), (_random_mixed, {}, {}), (_needles, {}, {"strict_triangles": True}),
                                               (_deep_chain, {"SOL_BVH": "ref"}, {"spill": True})],
                         ids=["cornell", "random_mixed", "needles_strict", "deep_chain_spill"])
def test_visibility_oct_is_the_association_over_the_ray_queries_of_its_own_rays(make, env, expect, monkeypatch):
    """200 camera-ray hit points; half of them get a finite radius, the upper quartile of the first sample's hit distances, as
    tests/test_gpu_visibility.py does. The share of hits among all samples must lie in (5 %, 95 %)."""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = make()
    rng = np.random.default_rng(11)
    with DeviceScene(sc) as ds:
        info = ds.info()
        if "strict_triangles" in expect:
            assert info["strict_triangles"]
        if "spill" in expect:
            assert info["stack_bound"] > info["lds_stack"], info
        n = 200
        pts = hit_points(sc, ds, n)
        probe = np.concatenate([per_sample_answers(ds, pts[::2], FIRST, 1, key_base=7, mode=m)[1][0] for m in ("cosine", "sphere")])
        radius = F(np.quantile(probe[np.isfinite(probe)], 0.75)) if np.isfinite(probe).any() else F(1.0)
        pts[::2, 7] = radius
        keys = np.stack([rng.integers(0, 2 ** 32, n), np.zeros(n)], axis=1).astype(U)
        dev_points = torch.from_numpy(pts).cuda()
        n_hits = n_all = 0
        seen = set()
        for ci, (mode, with_keys, first_draw) in enumerate(COMBOS):
            keys[:, 1] = first_draw
            dev_keys = torch.from_numpy(keys.view(np.int32)).cuda() if with_keys else None
            kw = dict(keys=dev_keys, key_base=7, first_draw=0 if with_keys else first_draw, mode=mode)
            status, t, dirs = per_sample_answers(ds, dev_points, FIRST, max(KS), **kw)
            assert (status != INVALID).all()
            n_hits, n_all = n_hits + int((status == HIT).sum()), n_all + status.size
            for ki, k in enumerate(KS):
                for res, sharp in PAIRS[(ci + ki) % 3]:
                    got = ds.visibility_oct(dev_points, res=res, sharpness_log2=sharp, samples=k, first_sample=FIRST, seed=SEED, **kw).cpu().numpy()
                    assert got.shape == (n, res * res, 4)
                    assert_maps_equal(got, restate(res, sharp, status, t, dirs, k), (mode, with_keys, first_draw, k, res, sharp))
                    seen.add((res, sharp))
        assert len(seen) == 9
        share = n_hits / n_all
        print(f"hits: {n_hits} of {n_all} samples ({100 * share:.1f} %), finite radius {radius:.4f}")
        assert 0.05 < share < 0.95, share


# ---- 2. shapes and routes --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_case():
    """257 hit points of the Cornell box, every other one with a finite radius, and their maps at 33 samples by the restatement's inputs"""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        pts = hit_points(sc, ds, 257)
        pts[::2, 7] = 200.0  # (the box is 555 wide)
        status, t, dirs = per_sample_answers(ds, pts, 2, 33, key_base=40, first_draw=2, mode="sphere")
    return sc, pts, (status, t, dirs)


def test_batch_shape_order_and_keys_do_not_change_a_point_s_map(cornell_case):
    sc, pts, (status, t, dirs) = cornell_case
    rng = np.random.default_rng(9)
    big = len(pts)
    perm = rng.permutation(big)
    keys = np.stack([40 + np.arange(big), np.full(big, 2)], axis=1).astype(U)
    with DeviceScene(sc) as ds:
        for res, sharp, samples in ((4, 5, 33), (8, 5, 17), (16, 2, 33)):
            kw = dict(res=res, sharpness_log2=sharp, samples=samples, first_sample=2, seed=SEED, mode="sphere")
            whole = ds.visibility_oct(pts, key_base=40, first_draw=2, **kw)
            assert_maps_equal(whole, restate(res, sharp, status, t, dirs, samples), (res, "the restatement"))
            assert_maps_equal(ds.visibility_oct(pts, keys=keys, key_base=9, first_draw=5, **kw), whole, (res, "keys"))
            for n in (1, 63, 64, 65, 257):
                assert_maps_equal(ds.visibility_oct(pts[:n], keys=keys[:n], **kw), whole[:n], (res, n))
                assert_maps_equal(ds.visibility_oct(pts[:n], key_base=40, first_draw=2, **kw), whole[:n], (res, n, "key_base"))
            assert_maps_equal(ds.visibility_oct(pts[perm], keys=keys[perm], **kw), whole[perm], (res, "permutation"))
        with pytest.raises(ValueError):
            ds.visibility_oct(pts[:, :7])
        with pytest.raises(ValueError):
            ds.visibility_oct(pts, mode="ambient")
        with pytest.raises(DeviceError) as e:
            ds.visibility_oct(pts, res=5)
        assert e.value.code == _abi.SOL_EINVAL and "res" in e.value.msg


@pytest.mark.parametrize("project", ["wave", "plain"])
def test_invalid_rows_answer_zero_words_between_untouched_guard_rows(project, monkeypatch):
    """Every class of invalid row among valid ones; the output sits between guard rows that must keep their pattern (device route, both
    projection kernels - the plain one is the developer override SOL_DEPTH_PROJECT=plain)."""
    import torch
    if project == "plain":
        monkeypatch.setenv("SOL_DEPTH_PROJECT", "plain")
    sc = _cornell()
    rng = np.random.default_rng(5)
    with DeviceScene(sc) as ds:
        clean = hit_points(sc, ds, 150)
        rows, is_valid = with_invalid_rows(clean)
        n = len(rows)
        assert n == 150 + len(INVALID_CLASSES) and (~is_valid).sum() == len(INVALID_CLASSES)
        keys = np.stack([rng.integers(0, 2 ** 32, n), rng.integers(0, 8, n)], axis=1).astype(U)
        d_rows, d_keys = torch.from_numpy(rows).cuda(), torch.from_numpy(keys.view(np.int32)).cuda()
        for res, samples in ((4, 16), (8, 48), (16, 17)):
            texels = res * res
            status, t, dirs = per_sample_answers(ds, rows[is_valid], 1, samples, keys=keys[is_valid], mode="cosine")
            want = np.zeros((n, texels, 4), dtype=F)
            want[is_valid] = restate(res, 3, status, t, dirs, samples)
            buf = torch.full((G + n * texels + G, 4), 7.5, dtype=torch.float32, device="cuda")
            cfg = ds._irradiance_config(samples, 1, SEED, 0, 0, "cosine")
            oct_cfg = ds._oct_config(res, 3)
            torch.cuda.synchronize()
            ds._chk(ds.lib.sol_visibility_oct_dev(ds.h, C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_keys.data_ptr()), n, C.byref(cfg), C.byref(oct_cfg),
                                                  C.c_void_p(buf.data_ptr() + G * 16)))
            ds.sync()
            got = buf.cpu().numpy()
            assert (got[:G] == 7.5).all() and (got[G + n * texels:] == 7.5).all(), (project, res)
            body = got[G:G + n * texels].reshape(n, texels, 4)
            assert body[~is_valid].tobytes() == bytes(16 * texels * len(INVALID_CLASSES))
            assert_maps_equal(body, want, (project, res, samples))
            assert_maps_equal(ds.visibility_oct(rows, res=res, sharpness_log2=3, samples=samples, first_sample=1, seed=SEED, keys=keys, mode="cosine"), want,
                              (project, res, "host route"))


def test_a_normal_whose_squared_length_underflows_adds_nothing_and_the_call_returns():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        pts = hit_points(sc, ds, 70)
        pts[33, 4:7] = [1e-30, 0.0, 0.0]
        for mode in ("cosine", "sphere"):
            status, t, dirs = per_sample_answers(ds, pts, 2, 48, key_base=1, mode=mode)
            if mode == "cosine":
                assert (status[:, 33] == INVALID).all() and (np.delete(status, 33, axis=1) != INVALID).all()
            for samples in (16, 48):
                got = ds.visibility_oct(pts, res=8, sharpness_log2=5, samples=samples, first_sample=2, seed=SEED, key_base=1, mode=mode)
                assert_maps_equal(got, restate(8, 5, status, t, dirs, samples), (mode, samples))
                if mode == "cosine":
                    assert got[33].tobytes() == bytes(64 * 16)  # no ray was made: every sum is +0


@pytest.mark.parametrize("project", ["wave", "plain"])
def test_a_bounded_partial_buffer_and_both_projection_kernels_give_the_default_s_bits(project, monkeypatch):
    """SOL_RADIANCE_ROWS = 128 words is less than one group of points over one chunk: 300 points x 80 samples (five chunks) run as five slices of 64
    points, each in five windows of one chunk which the projection kernel carries on in `out`. SOL_RADIANCE_ROWS = 2048 words is two such units
    (wave projection only): 40 samples (three chunks, the last one short) run in slices of 64 points, each in a window of two chunks and one of
    the short chunk alone."""
    sc = _cornell()
    calls = [dict(res=4, sharpness_log2=5, mode="sphere"), dict(res=8, sharpness_log2=6, mode="cosine"), dict(res=16, sharpness_log2=0, mode="sphere")]
    with DeviceScene(sc) as ds:
        pts = hit_points(sc, ds, 300)
        pts[::2, 7] = 150.0
        want = [ds.visibility_oct(pts, samples=80, first_sample=3, seed=SEED, key_base=40, **kw) for kw in calls]
        assert all((w[..., 2] > 0).any() and (w[..., 1] > 0).any() for w in want)
        if project == "wave":
            want40 = ds.visibility_oct(pts, samples=40, first_sample=3, seed=SEED, key_base=40, **calls[1])
            assert (want40[..., 2] > 0).any() and (want40[..., 1] > 0).any()
    monkeypatch.setenv("SOL_RADIANCE_ROWS", "128")
    if project == "plain":
        monkeypatch.setenv("SOL_DEPTH_PROJECT", "plain")
    with DeviceScene(sc) as ds:
        for kw, w in zip(calls, want):
            assert_maps_equal(ds.visibility_oct(pts, samples=80, first_sample=3, seed=SEED, key_base=40, **kw), w, (project, kw))
    if project == "wave":
        monkeypatch.setenv("SOL_RADIANCE_ROWS", "2048")
        with DeviceScene(sc) as ds:
            assert_maps_equal(ds.visibility_oct(pts, samples=40, first_sample=3, seed=SEED, key_base=40, **calls[1]), want40, (project, 40, calls[1]))


def test_device_tensors_host_arrays_and_another_stream_give_the_same_bytes(cornell_case):
    import torch
    sc, pts, _ = cornell_case
    rng = np.random.default_rng(3)
    n = len(pts)
    keys = np.stack([rng.integers(0, 2 ** 32, n), 2 * rng.integers(0, 8, n)], axis=1).astype(U)
    with DeviceScene(sc) as ds:
        dev_points, dev_keys = torch.from_numpy(pts).cuda(), torch.from_numpy(keys.view(np.int32)).cuda()
        stream = torch.cuda.Stream()
        for samples, res in ((7, 4), (40, 8), (20, 16)):
            for with_keys in (True, False):
                kw = dict(res=res, sharpness_log2=4, samples=samples, first_sample=3, seed=SEED, key_base=12)
                host = ds.visibility_oct(pts, keys=keys if with_keys else None, **kw)
                assert isinstance(host, np.ndarray) and host.dtype == F and host.shape == (n, res * res, 4)
                dev = ds.visibility_oct(dev_points, keys=dev_keys if with_keys else None, **kw)
                assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (n, res * res, 4)
                assert_maps_equal(dev.cpu().numpy(), host, (samples, with_keys))
                torch.cuda.synchronize()
                ds.set_stream(stream.cuda_stream)
                try:
                    other = ds.visibility_oct(dev_points, keys=dev_keys if with_keys else None, **kw)
                    on_host = ds.visibility_oct(pts, keys=keys if with_keys else None, **kw)
                    built = ds.volume_build_depth(VolumeGrid((0, 0, 0), 1.0, (n, 1, 1)), other, 150.0, res=res)
                finally:
                    ds.set_stream(0)
                assert_maps_equal(other.cpu().numpy(), host, (samples, with_keys, "stream"))
                assert_maps_equal(on_host, host, (samples, with_keys, "stream, host route"))
                assert_maps_equal(built.cpu().numpy(), dr.build_depth(host, 150.0), (samples, with_keys, "stream, build"))


# ---- 3. build and sample ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (nothing is traced: any handle serves)
        yield d


def random_oct_sums(n, res, seed):
    """[n, res * res, 4] sums as a gather leaves them, with every class of texel sol_volume_build_depth must judge"""
    rng = np.random.default_rng(seed)
    shape = (n, res * res)
    w = rng.uniform(0.0, 40.0, shape) * (rng.random(shape) < 0.9)  # a tenth of the texels saw nothing
    share = rng.uniform(0, 1, shape)
    mean_t = rng.uniform(0.2, 1.5, shape)
    sums = np.stack([w, w * share, w * (1 - share) * mean_t, w * (1 - share) * mean_t ** 2 * rng.uniform(1.0, 1.5, shape)], axis=-1).astype(F)
    flat = sums.reshape(-1, 4)
    pick = rng.permutation(len(flat))
    k = max(len(flat) // 40, 1)
    flat[pick[0 * k:1 * k], rng.integers(0, 4, k)] = NAN
    flat[pick[1 * k:2 * k], rng.integers(0, 4, k)] = rng.choice([INF, -INF], k)
    flat[pick[2 * k:3 * k], 0] = F(-0.0)
    flat[pick[3 * k:4 * k], 0] = F(-1.0)
    return sums


@pytest.mark.parametrize("res", [4, 8, 16])
def test_volume_build_depth_equals_the_restatement_on_every_class_of_texel(ds, res):
    import torch
    grid = grid_of(counts=(5, 3, 2))
    sums = random_oct_sums(grid.n_probes, res, 20 + res)
    assert (sums[..., 0] == 0).any() and np.isnan(sums).any() and np.isinf(sums).any()
    for radius in (2.0, 0.37):
        want = dr.build_depth(sums, radius)
        assert (want == np.array([radius, F(radius) * F(radius)], dtype=F)).all(axis=-1).sum() > grid.n_probes  # texels without information
        host = ds.volume_build_depth(grid, sums, radius, res=res)
        assert isinstance(host, np.ndarray) and host.shape == (grid.n_probes, res * res, 2)
        assert_maps_equal(host, want, (res, radius, "host"))
        buf = torch.full((G + sums.size // 4 + G, 2), 7.5, dtype=torch.float32, device="cuda")
        d_sums = torch.from_numpy(sums).cuda()
        torch.cuda.synchronize()
        ds._chk(ds.lib.sol_volume_build_depth_dev(ds.h, C.byref(grid.record()), C.c_void_p(d_sums.data_ptr()), C.byref(ds._oct_config(res)), float(radius),
                                                  C.c_void_p(buf.data_ptr() + G * 8)))
        ds.sync()
        got = buf.cpu().numpy()
        assert (got[:G] == 7.5).all() and (got[-G:] == 7.5).all()
        assert_maps_equal(got[G:-G].reshape(want.shape), want, (res, radius, "device"))
        assert_maps_equal(ds.volume_build_depth(grid, d_sums, radius, res=res).cpu().numpy(), want, (res, radius, "device, python"))
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(DeviceError) as e:
            ds.volume_build_depth(grid, sums, radius, res=res)
        assert e.value.code == _abi.SOL_EINVAL and "radius" in e.value.msg


def random_depth(n_probes, res, seed, radius=2.0):
    rng = np.random.default_rng(seed)
    shape = (n_probes, res * res)
    mean = rng.uniform(0.05, 1.5, shape)
    depth = np.stack([mean, mean ** 2 * rng.uniform(1.0, 1.6, shape)], axis=-1).astype(F)
    empty = rng.random(shape) < 0.1
    depth[empty] = (radius, radius * radius)
    return depth


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_volume_sample_depth_equals_the_restatement_word_for_word(ds, probes, points, flags):  # noqa: F811
    """The 9 x 7 x 5 grid and the 4097 points of tests/test_gpu_volume.py (inside, outside, on planes, lines and probes, invalid rows), both routes.
    With SOL_VOLUME_CHEBYSHEV off it is sol_volume_sample, word for word."""
    import torch
    d_points, d_probes = torch.from_numpy(points).cuda(), torch.from_numpy(probes).cuda()
    for res, bias in ((8, 0.25), (4, 0.0), (16, 0.1)) if flags == (True, True) else ((8, 0.25),):
        grid = grid_of(flags, bias)
        depth = random_depth(grid.n_probes, res, 30 + res)
        want = dr.volume_sample_depth(grid, probes, depth, res, points)
        assert ((want.view(U)[:, 3] > 0).sum() > 3500) and (want.view(U)[:, 3] == 0).sum() >= 40
        buf = torch.full((G + len(points) + G, 4), 7.5, dtype=torch.float32, device="cuda")
        d_depth = torch.from_numpy(depth).cuda()
        torch.cuda.synchronize()
        ds._chk(ds.lib.sol_volume_sample_depth_dev(ds.h, C.byref(grid.record()), C.c_void_p(d_probes.data_ptr()), C.c_void_p(d_depth.data_ptr()),
                                                   C.byref(ds._oct_config(res)), C.c_void_p(d_points.data_ptr()), len(points), C.c_void_p(buf.data_ptr() + G * 16)))
        ds.sync()
        got = buf.cpu().numpy()
        assert (got[:G] == 7.5).all() and (got[-G:] == 7.5).all()
        assert_words_equal(got[G:-G], want, (flags, res, "device"))
        assert_words_equal(ds.volume_sample(grid, d_probes, d_points, depth=d_depth, res=res).cpu().numpy(), want, (flags, res, "device, python"))
        rgb, samples = ds.volume_sample(grid, probes, points, depth=depth, res=res)
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), want, (flags, res, "host"))
        iso = ds.volume_sample(grid, d_probes, d_points).cpu().numpy()
        if not flags[1]:
            assert_words_equal(got[G:-G], iso, (flags, "sol_volume_sample"))
        else:
            assert (got[G:-G].view(U) != iso.view(U)).any()  # (the maps are read)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_a_grid_with_a_one_probe_axis(ds, flags):
    rng = np.random.default_rng(41)
    grid = grid_of(flags, 0.1, counts=(6, 1, 4))
    sh, vis = random_sums(grid.n_probes, 42)
    rows = vr.volume_build(sh, vis, radius=2.0)
    depth = random_depth(grid.n_probes, 8, 43)
    at = vr.probe_positions(grid)
    lo, size = at[0].astype(np.float64), (at[-1] - at[0]).astype(np.float64)
    pos = lo + rng.uniform(-0.3, 1.3, (700, 3)) * np.where(size > 0, size, 1.0)
    pts = vr.point_rows(pos.astype(F), vr.unit_normals(rng, 700))
    want = dr.volume_sample_depth(grid, rows, depth, 8, pts)
    rgb, samples = ds.volume_sample(grid, rows, pts, depth=depth, res=8)
    assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), want, flags)
    assert (samples > 0).sum() > 500


# ---- 4. the chain, in a scene with a wall ------------------------------------------------------------------------------------------------------
def _box_with_a_wall():
    """A closed grey box x in [-2, 2], y in [0, 2], z in [-1.5, 1.5], black background, split at x = 0 by an opaque quad wall; a quad light under
    the ceiling of the half x > 0, facing down."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(0.7, 0.7, 0.7))
    world = [b.Quad((-2.0, 0.0, -1.5), (4.0, 0.0, 0.0), (0.0, 0.0, 3.0), grey),   # floor
             b.Quad((-2.0, 2.0, -1.5), (4.0, 0.0, 0.0), (0.0, 0.0, 3.0), grey),   # ceiling
             b.Quad((-2.0, 0.0, -1.5), (0.0, 2.0, 0.0), (0.0, 0.0, 3.0), grey),   # x = -2
             b.Quad((2.0, 0.0, -1.5), (0.0, 2.0, 0.0), (0.0, 0.0, 3.0), grey),    # x = +2
             b.Quad((-2.0, 0.0, -1.5), (4.0, 0.0, 0.0), (0.0, 2.0, 0.0), grey),   # z = -1.5
             b.Quad((-2.0, 0.0, 1.5), (4.0, 0.0, 0.0), (0.0, 2.0, 0.0), grey),    # z = +1.5
             b.Quad((0.0, 0.0, -1.5), (0.0, 2.0, 0.0), (0.0, 0.0, 3.0), grey),    # the wall
             b.Quad((0.5, 1.98, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), b.DiffuseLight(12, 12, 12))]
    cam = CameraConfig(60.0, 0.0, (1.0, 1.0, 1.4), (1.0, 0.5, 0.0), (0, 1, 0))
    return b.finish(b.Bvh(world), cam, (0.0, 0.0, 0.0), RC)


def test_in_a_scene_with_a_wall_depth_maps_leak_less_than_the_isotropic_moments():
    """A 4 x 3 x 3 grid straddles the wall, its probes half a spacing from it; 256 samples. Over 48 floor points of the dark half within one spacing
    of the wall, with the irradiance at 1024 samples as ground truth, the sum of |answer - truth| must be smaller with depth maps than with the
    isotropic moments built from the same seed; over the lit half's mirror points it must not be larger by more than the isotropic error itself.
    The ratios are printed (profiles/volume_depth.txt records them); none is fixed in advance."""
    import torch
    sc = _box_with_a_wall()
    grid = VolumeGrid((-1.5, 0.4, -1.0), (1.0, 0.6, 1.0), (4, 3, 3), normal_bias=0.05)
    assert np.abs(vr.probe_positions(grid)[:, 0]).min() >= 0.25 * 1.0
    radius, res, sharp = 6.0, 8, 5
    xs, zs = np.meshgrid(np.linspace(-0.95, -0.05, 8), np.linspace(-1.2, 1.2, 6))
    dark = np.stack([xs.ravel(), np.zeros(48), zs.ravel()], axis=1)
    lit = dark * np.array([-1.0, 1.0, 1.0])
    floor = vr.point_rows(np.concatenate([dark, lit]).astype(F), [(0, 1, 0)])
    with DeviceScene(sc) as ds:
        d_floor = torch.from_numpy(floor).cuda()
        at = ds.volume_points(grid, tmax=radius)
        sh = ds.irradiance_sh(ds.volume_points(grid), samples=256, seed=SEED, mode="sphere")
        vis = ds.visibility(at, samples=256, seed=SEED, mode="sphere", distances=True)
        sums = ds.visibility_oct(at, res=res, sharpness_log2=sharp, samples=256, seed=SEED, mode="sphere")
        built = ds.volume_build(grid, sh, vis, radius)
        depth = ds.volume_build_depth(grid, sums, radius, res=res, sharpness_log2=sharp)
        iso = ds.volume_sample(grid, built, d_floor).cpu().numpy()
        got = ds.volume_sample(grid, built, d_floor, depth=depth, res=res).cpu().numpy()
        rgb, cnt = ds.irradiance(floor, samples=1024, seed=SEED + 1, mode="cosine")
        # the device's chain is the restatement's chain on the device's own sums
        assert_maps_equal(depth.cpu().numpy(), dr.build_depth(sums.cpu().numpy(), radius), "depth maps")
        assert_words_equal(got, dr.volume_sample_depth(grid, built.cpu().numpy(), depth.cpu().numpy(), res, floor), "floor")
    assert (cnt == 1024).all()
    truth = np.pi * rgb.astype(np.float64) / 1024.0
    err_iso = np.abs(iso[:, :3] - truth).sum(axis=1)
    err_depth = np.abs(got[:, :3] - truth).sum(axis=1)
    dark_iso, dark_depth, lit_iso, lit_depth = err_iso[:48].sum(), err_depth[:48].sum(), err_iso[48:].sum(), err_depth[48:].sum()
    print(f"dark half: sum |answer - truth| isotropic {dark_iso:.4f}, depth maps {dark_depth:.4f} (ratio {dark_depth / dark_iso:.4f}); "
          f"lit half: isotropic {lit_iso:.4f}, depth maps {lit_depth:.4f} (ratio {lit_depth / lit_iso:.4f}); truth sums dark {truth[:48].sum():.4f} lit {truth[48:].sum():.4f}")
    assert dark_iso > 0 and dark_depth < dark_iso
    assert lit_depth <= 2.0 * lit_iso


# ---- 5. refusals on a handle, neutrality ---------------------------------------------------------------------------------------------------------
def test_refusals_on_a_handle_and_a_scene_with_a_medium(points):  # noqa: F811
    point = np.array([[0., 0., 0., 0.001, 0., 1., 0., np.inf]], dtype=F)
    medium = scenes.create_test_scene(RC)
    assert medium.desc.n_mediums > 0
    with DeviceScene(medium) as ds:
        with pytest.raises(DeviceError) as e:
            ds.visibility_oct(point)
        assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        cfg, oct_cfg = ds._irradiance_config(1, 0, 0, 0, 0, "sphere"), ds._oct_config(8, 5)
        for fn in (ds.lib.sol_visibility_oct, ds.lib.sol_visibility_oct_dev):
            assert fn(ds.h, None, None, 0, C.byref(cfg), C.byref(oct_cfg), None) == _abi.SOL_OK  # n == 0 succeeds on any scene
            assert fn(ds.h, point.ctypes.data, None, 1, C.byref(cfg), C.byref(ds._oct_config(8, 7)), None) == _abi.SOL_EINVAL
            assert b"sharpness_log2" in ds.lib.sol_last_error()  # the configuration is judged in front of the medium
        # build and sample trace nothing: the scene's medium does not matter
        grid = grid_of((True, True), 0.25)
        sh, vis = random_sums(grid.n_probes, 61)
        rows = vr.volume_build(sh, vis, 2.0)
        sums = random_oct_sums(grid.n_probes, 8, 62)
        depth = ds.volume_build_depth(grid, sums, 2.0)
        assert_maps_equal(depth, dr.build_depth(sums, 2.0), "depth maps on a scene with a medium")
        rgb, samples = ds.volume_sample(grid, rows, points[:300], depth=depth)
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), dr.volume_sample_depth(grid, rows, depth, 8, points[:300]), "a scene with a medium")
    with DeviceScene(_cornell()) as ds:
        lib, out = ds.lib, np.full(64 * 4, 7, U)
        cfg, oct_cfg = ds._irradiance_config(1, 0, 0, 0, 0, "sphere"), ds._oct_config(8, 5)
        for fn in (lib.sol_visibility_oct, lib.sol_visibility_oct_dev):
            assert fn(ds.h, None, None, 1, C.byref(cfg), C.byref(oct_cfg), out.ctypes.data) == _abi.SOL_EINVAL and b"null point" in lib.sol_last_error()
            assert fn(ds.h, point.ctypes.data, None, 1, C.byref(cfg), C.byref(oct_cfg), None) == _abi.SOL_EINVAL and b"null output" in lib.sol_last_error()
            assert fn(ds.h, point.ctypes.data, None, 1, C.byref(cfg), None, out.ctypes.data) == _abi.SOL_EINVAL and b"null SolOctConfig" in lib.sol_last_error()
        assert (out == 7).all()


def test_the_new_calls_between_renders_change_no_frame_plane_or_statistic(points):  # noqa: F811
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    grid = grid_of((True, True), 0.25)
    sh, vis = random_sums(grid.n_probes, 51)
    rows = vr.volume_build(sh, vis, 2.0)

    def sequence(ds, between):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        between()
        ds.render(8, 8, SEED)
        between()
        ds.render_aux(0, 4, SEED)
        between()
        vis_rows = ds.visibility_to_numpy(ds.visibility(ds.camera_rays(0, 0, 8, 8, 1, SEED).reshape(-1, 8), samples=20, seed=SEED))
        between()
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(vis_rows.tobytes()))

    with DeviceScene(sc) as ds:
        pts = hit_points(sc, ds, 64)
        d_points, d_rows = torch.from_numpy(points).cuda(), torch.from_numpy(rows).cuda()

        def depth_calls():
            ds.visibility_oct(pts, res=4, samples=1, seed=SEED)
            at = ds.volume_points(grid, tmax=2.0)
            sums = ds.visibility_oct(at, res=8, samples=40, first_sample=3, seed=SEED, key_base=5)
            depth = ds.volume_build_depth(grid, sums, 2.0)
            ds.volume_sample(grid, d_rows, d_points, depth=depth)
            ds.volume_sample(grid, rows, points[:100], depth=depth.cpu().numpy())

        want = sequence(ds, lambda: None)
        assert sequence(ds, depth_calls) == want and want[3]["rays"] > 0
