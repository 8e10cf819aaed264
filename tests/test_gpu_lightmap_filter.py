"""Lightmap filtering on the device (sol_lightmap_filter). The yardstick is tests/lightmap_filter_ref.py, the rule restated in numpy
float32: every answer is compared word for word (a NaN with a NaN), on the host route and the device route. Around it: atlases smaller than a tap
footprint and steps beyond the atlas, every channel grouping, every class of row that is not live between guard rows, sigmas of +inf and 1e-6, both
pass shapes in child processes of their own, a permutation, a stream of the caller's, a scene with a medium, neutrality - and the chain
points -> irradiance -> filter against a 1024-sample truth. Atlases are at most 256 x 256."""
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import lightmap_filter_ref as fr
import lightmap_ref as lr
import parity_util as pu
from solstrale_amd import CameraConfig, DeviceScene, RenderConfig, SceneBuilder, _abi, scenes

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F = np.float32
INF = float("inf")
RC = RenderConfig(32, 32, 1)


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (the atlas of a filter call is the caller's: any handle serves)
        yield d


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    g, w = got.view(np.uint32).reshape(got.shape[0], -1), want.view(np.uint32).reshape(want.shape[0], -1)
    differ = (g != w) & ~(np.isnan(got.reshape(g.shape)) & np.isnan(want.reshape(g.shape)))
    if differ.any():
        bad = np.nonzero(differ.any(axis=1))[0]
        raise AssertionError((what, len(bad), len(g), bad[:5], got[bad[:3]], want[bad[:3]]))


@functools.lru_cache(maxsize=None)
def atlas(W, H, perm_seed=None):
    """(points, texels, sigma_position) of the test mesh in a W x H atlas, by the rasteriser's restatement with conservative claims: a jittered grid
    mesh over the middle of the atlas with holes (every seventh triangle is missing), and a second chart, higher and tilted, that overlaps its
    corner. sigma_position: two texels' world size."""
    V, T, N = lr.grid_mesh(6, 4)
    keep = np.arange(len(V)) % 7 != 3
    V, T, N = V[keep], T[keep], N[keep]
    T = (T * F(0.8) + F(0.05)).astype(F)
    V2, T2, N2 = lr.grid_mesh(3, 9)
    T2 = (T2 * F(0.4) + F(0.58)).astype(F)
    V2 = (V2 * F(0.5) + np.asarray((3.0, 0.5, 0.0), dtype=F)).astype(F)
    N2 = (N2 + np.asarray((0.5, 0.0, 0.0), dtype=F)).astype(F)
    V, T, N = np.concatenate([V, V2]), np.concatenate([T, T2]), np.concatenate([N, N2])
    if perm_seed is not None:
        perm = np.random.default_rng(perm_seed).permutation(len(V))
        V, T, N = V[perm], T[perm], N[perm]
    points, texels = lr.lightmap_points(V, T, W, H, normals=N, conservative=True)
    return points, texels, 2.0 * 4.0 / (0.8 * max(W, 1))


def rows_of(n, channels, words, seed):
    """n rows of `words` words: `channels` floats of mixed magnitude and sign, then words that are counts, not floats."""
    rng = np.random.default_rng(seed)
    values = (rng.normal(size=(n, words)) * rng.choice([0.05, 1.0, 30.0], (n, 1))).astype(F)
    if words > channels:
        values[:, channels:] = (np.arange(n * (words - channels), dtype=np.uint32) + np.uint32(0x7F800001)).reshape(n, -1).view(F)  # (NaN bit patterns behind the channels)
    return values


def check_both_routes(ds, values, points, texels, W, H, what, **kw):
    import torch
    want = fr.lightmap_filter(values, points, texels, W, H, **kw)
    got = ds.lightmap_filter(values, points, texels, W, H, **kw)
    assert_words_equal(got, want, (what, "host"))
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (values, points, texels.view(np.int32).reshape(-1, 4))]
    got = ds.lightmap_filter(d[0], d[1], d[2], W, H, **kw)
    assert got.shape == d[0].shape and got.is_cuda
    assert_words_equal(got.cpu().numpy(), want, (what, "device"))
    return want


# ---- 1. the rule against the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", [(1, 1), (300, 1), (5, 3), (64, 4), (65, 5)])
def test_small_and_odd_atlases_at_every_iteration_count(ds, W, H):
    points, texels, sigma = atlas(W, H)
    values = rows_of(W * H, 3, 4, W)
    for iterations in (1, 2, 3, 8):
        want = check_both_routes(ds, values, points, texels, W, H, (W, H, iterations), sigma_position=sigma, iterations=iterations)
        live = fr.live_texels(values, points, texels, 3)
        assert_words_equal(want[~live], values[~live], "rows that are not live")
        assert_words_equal(want[:, 3:], values[:, 3:], "the trailing word")


def test_steps_beyond_the_atlas(ds):
    W, H = 130, 67
    points, texels, sigma = atlas(W, H)
    values = rows_of(W * H, 3, 4, 1)
    live = fr.live_texels(values, points, texels, 3)
    assert 0.3 < live.mean() < 0.9 and (texels["flags"] == 2).sum() > 20, "holes, and conservative texels"
    want = check_both_routes(ds, values, points, texels, W, H, "130 x 67 x 8", sigma_position=sigma, iterations=8)
    assert (want[live, :3] != values[live, :3]).any(axis=1).mean() > 0.9


@pytest.mark.parametrize("channels, words", [(1, 1), (3, 4), (4, 4), (5, 6), (27, 28), (32, 32), (2, 5)])
def test_every_channel_grouping(ds, channels, words):
    W, H = 70, 37
    points, texels, sigma = atlas(W, H)
    values = rows_of(W * H, channels, words, channels)
    check_both_routes(ds, values, points, texels, W, H, (channels, words), sigma_position=sigma, iterations=3, channels=channels, value_scale=0.5)


def test_sigmas_of_infinity_and_of_the_smallest_value(ds):
    W, H = 48, 40
    points, texels, sigma = atlas(W, H)
    values = np.abs(rows_of(W * H, 3, 3, 6))
    for k, name in enumerate(("sigma_position", "sigma_plane", "sigma_value")):
        for s in (INF, 1e-6):
            kw = dict(sigma_position=sigma, sigma_plane=sigma, sigma_value=0.25)
            kw[name] = s
            check_both_routes(ds, values, points, texels, W, H, (name, s), iterations=4, normal_power_log2=k, **kw)
    check_both_routes(ds, values, points, texels, W, H, "all off", sigma_position=INF, sigma_plane=INF, sigma_value=INF, normal_power_log2=0, iterations=2)
    check_both_routes(ds, values, points, texels, W, H, "sharpest normals", sigma_position=sigma, normal_power_log2=7, iterations=2)


def test_every_class_of_row_that_is_not_live_between_guard_rows(ds):
    import torch
    W, H, G = 33, 21, 64
    points, texels, sigma = (a.copy() if hasattr(a, "copy") else a for a in atlas(W, H))
    values = rows_of(W * H, 3, 4, 8)
    live = np.nonzero(fr.live_texels(values, points, texels, 3))[0]
    pick = live[np.linspace(0, len(live) - 1, 12).astype(int)]
    texels["triangle"][pick[0]] = lr.NONE                                   # unowned, a valid row
    texels["triangle"][pick[1]], values[pick[1], :3] = lr.NONE, np.nan      # unowned, NaNs in the row
    points[pick[2], 0], points[pick[3], 2] = np.nan, -np.inf                # a position word
    points[pick[4], 4], points[pick[5], 6] = np.inf, np.nan                 # a normal word
    values[pick[6], 0], values[pick[7], 2] = np.nan, np.inf                 # a value word
    points[pick[8]] = 0                                                     # owned with zero words: live, a normal that weighs every tap 0
    points[pick[9]], values[pick[9]] = 0, 0
    points[pick[10], 3], points[pick[11], 7] = np.nan, np.nan               # tmin and tmax are not guides: still live
    want = check_both_routes(ds, values, points, texels, W, H, "bad rows", sigma_position=sigma, iterations=3)
    assert_words_equal(want[pick[:8]], values[pick[:8]], "rows that are not live come back as they went in")
    assert np.isfinite(want[np.setdiff1d(live, pick[:8]), :3]).all(), "and were no tap of a neighbour"
    assert (want[pick[10], :3] != values[pick[10], :3]).any()
    # the device route between guard rows
    n = W * H
    d_points, d_texels, d_values = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (points, texels.view(np.int32).reshape(-1, 4), values))
    out = torch.full((n + 2 * G, 4), 7.0, dtype=torch.float32, device="cuda")
    cfg = _abi.SolLightmapFilterConfig(size=64, width=W, height=H, iterations=3, normal_power_log2=5, channels=3, stride_bytes=16, sigma_position=sigma,
                                       sigma_plane=sigma, sigma_value=0.25, value_scale=1.0)
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_lightmap_filter_dev(ds.h, C.byref(cfg), C.c_void_p(d_points.data_ptr()), C.c_void_p(d_texels.data_ptr()), C.c_void_p(d_values.data_ptr()),
                                            C.c_void_p(out[G:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n:] == 7).all()
    assert_words_equal(out[G:G + n].cpu().numpy(), want, "guarded rows")
    assert_words_equal(d_values.cpu().numpy(), values, "the input is not written")


CHILD = """
import sys
import numpy as np
from solstrale_amd import LIGHTMAP_TEXEL_DTYPE, DeviceScene, RenderConfig, scenes
import torch
a = np.load(sys.argv[1])
out = {}
with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
    for k in range(int(a["n"])):
        v, p, t = a[f"values{k}"], a[f"points{k}"], a[f"texels{k}"]
        W, H, it, ch, sigma = (a[f"args{k}"][j] for j in range(5))
        kw = dict(sigma_position=float(sigma), iterations=int(it), channels=int(ch))
        out[f"host{k}"] = ds.lightmap_filter(v, p, t.view(LIGHTMAP_TEXEL_DTYPE).reshape(-1), int(W), int(H), **kw)
        d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v, p, t.view(np.int32).reshape(-1, 4))]
        out[f"device{k}"] = ds.lightmap_filter(d[0], d[1], d[2], int(W), int(H), **kw).cpu().numpy()
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("shape", ["plain", "staged", "fold"])
def test_every_pass_shape_answers_the_same_words(shape, tmp_path):
    """SOL_LIGHTMAP_FILTER is read at creation: each shape runs in a fresh child process of its own. Steps 1 and 2 are the staged kernel's, 4 and 8
    the plain one's in either shape; tiles at the atlas's edge, an atlas below one tile, and channel groups beyond the first."""
    cases = [(70, 37, 4, 3, 4), (70, 37, 2, 27, 28), (5, 3, 2, 3, 4), (16, 16, 1, 5, 5), (33, 17, 3, 32, 32)]
    arrays, wants = {"n": len(cases)}, []
    for k, (W, H, it, ch, words) in enumerate(cases):
        points, texels, sigma = atlas(W, H)
        values = rows_of(W * H, ch, words, 20 + k)
        arrays.update({f"values{k}": values, f"points{k}": points, f"texels{k}": texels.view(np.uint32).reshape(-1, 4),
                       f"args{k}": np.asarray([W, H, it, ch, sigma], dtype=np.float64)})
        wants.append(fr.lightmap_filter(values, points, texels, W, H, sigma_position=sigma, iterations=it, channels=ch))
    np.savez(tmp_path / "in.npz", **arrays)
    env = {**os.environ, "SOL_LIGHTMAP_FILTER": shape, "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    for k, want in enumerate(wants):
        assert_words_equal(got[f"host{k}"], want, (shape, cases[k], "host"))
        assert_words_equal(got[f"device{k}"], want, (shape, cases[k], "device"))


def test_a_permutation_of_the_triangles_changes_only_texels_that_change_hands(ds):
    """The filter reads no triangle index: wherever the permuted mesh gives a texel the same point row, and all its taps too, the answer is the same
    word. Compared through the restatement on both meshes, and the two against each other where the rows agree everywhere."""
    W, H = 61, 40
    base_p, base_t, sigma = atlas(W, H)
    perm_p, perm_t, _ = atlas(W, H, perm_seed=8)
    values = rows_of(W * H, 3, 4, 3)
    a = check_both_routes(ds, values, base_p, base_t, W, H, "base", sigma_position=sigma, iterations=1)
    b = check_both_routes(ds, values, perm_p, perm_t, W, H, "permuted", sigma_position=sigma, iterations=1)
    same = (base_p.view(np.uint32) == perm_p.view(np.uint32)).all(axis=1) & ((base_t["triangle"] == lr.NONE) == (perm_t["triangle"] == lr.NONE))
    reach = 2  # one pass of step 1: taps up to two texels away (a texel on a shared edge may change hands, and its row with it)
    padded = np.pad(~same.reshape(H, W), reach)
    near = np.zeros((H, W), dtype=bool)
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            near |= padded[dy:dy + H, dx:dx + W]
    far = ~near.reshape(-1)
    assert far.sum() > 200, "enough rows whose whole footprint the permutation left alone to make the comparison mean something"
    assert_words_equal(b[far], a[far], "rows under the permutation")


def test_a_stream_of_the_callers(ds):
    import torch
    W, H = 50, 41
    points, texels, sigma = atlas(W, H)
    values = rows_of(W * H, 3, 4, 12)
    want = fr.lightmap_filter(values, points, texels, W, H, sigma_position=sigma, iterations=3)
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)
    try:
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (values, points, texels.view(np.int32).reshape(-1, 4))]
        assert_words_equal(ds.lightmap_filter(d[0], d[1], d[2], W, H, sigma_position=sigma, iterations=3).cpu().numpy(), want, "device route on the caller's stream")
        assert_words_equal(ds.lightmap_filter(values, points, texels, W, H, sigma_position=sigma, iterations=3), want, "host route on the caller's stream")
    finally:
        ds.set_stream(0)


def test_a_scene_with_a_constant_medium_is_served():
    W, H = 24, 20
    points, texels, sigma = atlas(W, H)
    values = rows_of(W * H, 3, 4, 2)
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    with DeviceScene(sc) as ds:
        check_both_routes(ds, values, points, texels, W, H, "a scene with a medium", sigma_position=sigma, iterations=2)


# ---- 2. neutrality ----------------------------------------------------------------------------------------------------------------------------
def _path_stats(ds):
    st = _abi.SolPathStats()
    st.size = C.sizeof(st)
    ds._chk(ds.lib.sol_path_stats(ds.h, C.byref(st)))
    return st


def test_filter_calls_between_renders_change_no_frame_plane_or_statistic():
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    W, H = 40, 24
    points, texels, sigma = atlas(W, H)
    values = rows_of(W * H, 27, 28, 4)

    def sequence(ds, between):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        between()
        ds.render(8, 8, SEED)
        between()
        ds.render_aux(0, 4, SEED)
        between()
        radiance = ds.radiance(ds.camera_rays(0, 0, 8, 8, 0, SEED).reshape(-1, 8), samples=3, seed=SEED).cpu().numpy()
        between()
        vis = ds.visibility_to_numpy(ds.visibility(ds.camera_rays(0, 0, 8, 8, 1, SEED).reshape(-1, 8), samples=20, seed=SEED))
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(radiance.tobytes()), zlib.crc32(vis.tobytes()))

    with DeviceScene(sc) as ds:
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (values, points, texels.view(np.int32).reshape(-1, 4))]

        def filters():
            ds.lightmap_filter(d[0], d[1], d[2], W, H, sigma_position=sigma, iterations=4, channels=27)
            ds.lightmap_filter(values[:, :4], points, texels, W, H, sigma_position=sigma, iterations=1)

        want = sequence(ds, lambda: None)
        assert sequence(ds, filters) == want and want[3]["rays"] > 0


# ---- 3. the chain -----------------------------------------------------------------------------------------------------------------------------
def floor_under_a_light():
    """A triangle floor (the jittered grid mesh, its lightmap chart in the middle three quarters of the atlas) under a quad light."""
    V, T, N = lr.grid_mesh(8, 2)
    V, T, N = (np.ascontiguousarray(a[:, [0, 2, 1]]) for a in (V, T, N))  # (wound so that the geometric normals point up, at the light)
    T = np.ascontiguousarray(T * F(0.75) + F(0.125), dtype=F)
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(0.7, 0.7, 0.7))
    first, n = b.triangles(V.astype(np.float64), grey, uvs=T)
    light = b.Quad((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), b.DiffuseLight(8, 8, 8))
    cam = CameraConfig(40.0, 0.0, (0.0, 6.0, 6.0), (0.0, 0.0, 0.0), (0, 1, 0))
    return b.finish(b.Bvh(list(range(first, first + n)) + [light]), cam, (0.0, 0.0, 0.0), RC), V, T, N


def test_the_filtered_bake_is_nearer_the_truth_than_the_unfiltered_one():
    """points -> irradiance (4 samples) -> filter on device memory, against the 1024-sample gather of another seed. The filtered atlas's mean squared
    error must be below the unfiltered one's - the condition a denoiser exists for -, and the chain must stay brighter under the light than in the
    corners. The ratio is measured, not fixed here (profiles/lightmap_filter.txt, DESIGN.md 26: on an MI355X an MSE of 18.17 unfiltered and 13.79
    filtered, a ratio of 1.32, with the untuned defaults); so is the error the filter adds when it is fed the 1024-sample atlas (0.076), which is
    reported and not asserted."""
    import torch
    W = H = 64
    low, high = 4, 1024
    sc, V, T, N = floor_under_a_light()
    sigma = 2.0 * 4.0 / (0.75 * W)  # two texels of a floor 4 units wide over three quarters of the atlas
    with DeviceScene(sc) as ds:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        points, texels = ds.lightmap_points(dV, dT, W, H, normals=dN)
        noisy = ds.irradiance(points, samples=low, seed=SEED)
        truth = ds.irradiance(points, samples=high, seed=SEED + 977)
        filtered = ds.lightmap_filter(noisy, points, texels, W, H, sigma_position=sigma, value_scale=np.pi / low)
        refiltered = ds.lightmap_filter(truth, points, texels, W, H, sigma_position=sigma, value_scale=np.pi / high)
        p, t = points.cpu().numpy(), texels.cpu().numpy().view(lr.TEXEL_DTYPE).reshape(-1)
        assert_words_equal(filtered.cpu().numpy(), fr.lightmap_filter(noisy.cpu().numpy(), p, t, W, H, sigma_position=sigma, value_scale=np.pi / low), "the chain")
    owned = t["triangle"] != lr.NONE
    assert 0.5 * W * H < owned.sum() < 0.65 * W * H
    e_truth = truth.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / high)
    e_noisy = noisy.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / low)
    e_filtered = filtered.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / low)
    e_refiltered = refiltered.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / high)
    mse_noisy, mse_filtered = ((e_noisy - e_truth) ** 2).mean(), ((e_filtered - e_truth) ** 2).mean()
    mse_added = ((e_refiltered - e_truth) ** 2).mean()
    print(f"lightmap filter chain 64 x 64: MSE against the {high}-sample truth: unfiltered {mse_noisy:.6g}, filtered {mse_filtered:.6g}, "
          f"ratio {mse_noisy / mse_filtered:.3f}; the filter over the {high}-sample atlas adds {mse_added:.6g} (mean irradiance {e_truth.mean():.4g})")
    assert mse_filtered < mse_noisy
    assert (filtered.cpu().numpy()[:, 3].view(np.uint32) == noisy.cpu().numpy()[:, 3].view(np.uint32)).all(), "the samples word is carried"
    lum = filtered.cpu().numpy()[:, :3].sum(axis=1).reshape(H, W)
    under = lum[24:40, 24:40].mean()
    corners = np.mean([lum[8:16, 8:16].mean(), lum[8:16, 48:56].mean(), lum[48:56, 8:16].mean(), lum[48:56, 48:56].mean()])
    assert under > 2.0 * corners > 0.0
