"""Irradiance volumes on the device (sol_volume_points / sol_volume_build / sol_volume_sample). The yardstick is tests/volume_ref.py,
the rule restated in numpy float32: point rows, probes and sampled rows are compared word for word, on the host route and the device route.
Around it: guard rows, every class of skipped probe and invalid row, all four flag combinations, a one-probe axis, batch sizes around the wave
and the block, a permutation, a stream of the caller's, the whole bake end to end, neutrality, and a scene with a constant medium. Grids have at
most 9 x 7 x 5 probes, calls at most 4097 points."""
import ctypes as C
import zlib

import numpy as np
import pytest

import parity_util as pu
import volume_ref as vr
from solstrale_amd import DeviceScene, RenderConfig, VolumeGrid, _abi, scenes, volume_probes_to_numpy
from test_gpu_irradiance import _path_stats
from test_gpu_lightmap import floor_under_a_light

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F, U = np.float32, np.uint32
INF, NAN = F(np.inf), F(np.nan)
RC = RenderConfig(32, 32, 1)
G = 64  # guard rows on either side of an output
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
FLAG_IDS = ["plain", "backface", "chebyshev", "both"]
ORIGIN, SPACING, COUNTS = (-1.0, 0.5, 2.0), (0.5, 0.75, 1.25), (9, 7, 5)


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (nothing is traced: any handle serves)
        yield d


def grid_of(flags=(True, True), bias=0.0, counts=COUNTS, spacing=SPACING):
    return VolumeGrid(ORIGIN, spacing, counts, backface=flags[0], chebyshev=flags[1], normal_bias=bias)


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape[0] == want.shape[0], (what, got.shape, want.shape)
    g, w = got.view(U).reshape(got.shape[0], -1), want.view(U).reshape(want.shape[0], -1)
    if g.shape != w.shape or (g != w).any():
        bad = np.nonzero((g != w).any(axis=1))[0]
        raise AssertionError((what, len(bad), len(g), bad[:5], got[bad[:3]], want[bad[:3]]))


def random_sums(n, seed):
    """[n, 28] SolSh9 rows and [n, 8] SolVisibility rows as gathers leave them, with every class of row sol_volume_build must judge"""
    rng = np.random.default_rng(seed)
    samples = rng.integers(1, 200, n).astype(U)
    sh = np.zeros((n, 28), dtype=F)
    sh[:, :27] = (rng.normal(size=(n, 27)) * 0.3 * samples[:, None]).astype(F)
    sh[:, 0:3] = (rng.uniform(1.0, 3.0, (n, 3)) * samples[:, None]).astype(F)  # (a bright constant term: most probes answer something positive)
    sh.view(U)[:, 27] = samples
    vis = np.zeros((n, 8), dtype=F)
    hits = (samples * rng.uniform(0, 1, n)).astype(U)
    mean_t = rng.uniform(0.2, 1.5, n)
    vis[:, 0:3] = rng.normal(size=(n, 3)).astype(F)
    vis[:, 4] = (hits * mean_t).astype(F)
    vis[:, 5] = (hits * mean_t ** 2 * rng.uniform(1.0, 1.5, n)).astype(F)
    vis.view(U)[:, 3], vis.view(U)[:, 6], vis.view(U)[:, 7] = samples - hits, hits, samples
    k = max(n // 16, 1)
    pick = rng.permutation(n)
    sh.view(U)[pick[0 * k:1 * k], 27] = 0                                   # probes without samples
    sh[pick[1 * k:2 * k], rng.integers(0, 27, k)] = NAN                     # a NaN among the sums
    sh[pick[2 * k:3 * k], rng.integers(0, 27, k)] = rng.choice([INF, -INF], k)  # an infinity
    vis.view(U)[pick[3 * k:4 * k], 7] = 0                                   # a visibility row without samples
    vis[pick[4 * k:5 * k], 4] = INF                                         # sums of distances that are not finite
    vis[pick[5 * k:6 * k], 5] = NAN
    return sh, vis


@pytest.fixture(scope="module")
def probes():
    """the probes of the 9 x 7 x 5 grid, by the restatement: about a fifth invalid, most of the rest with moments"""
    sh, vis = random_sums(9 * 7 * 5, 11)
    rows = vr.volume_build(sh, vis, radius=2.0)
    flags = rows.view(U)[:, 29]
    assert 20 < (flags == 0).sum() < 80 and (flags == 3).sum() > 150 and (flags == 1).sum() > 20
    return rows


@pytest.fixture(scope="module")
def points():
    """4097 point rows: inside the grid, on its planes, lines and probes, outside every face, every class of invalid row; normals of any length"""
    rng = np.random.default_rng(12)
    grid = grid_of()
    at = vr.probe_positions(grid)
    lo, size = at[0].astype(np.float64), (at[-1] - at[0]).astype(np.float64)
    pos = [lo + rng.uniform(0, 1, (2600, 3)) * size]
    snapped = lo + rng.uniform(0, 1, (600, 3)) * size            # on planes and lines: one or two coordinates are a probe's, on the bits
    onto = at[rng.integers(0, len(at), 600)]
    mask = rng.integers(1, 7, 600)[:, None] >> np.arange(3)[None, :] & 1
    pos.append(np.where(mask == 1, onto, snapped))
    pos.append(at[rng.integers(0, len(at), 200)])                # on probes: l2 == 0
    for axis in range(3):                                        # outside every face
        for side in (-1, 2):
            p = lo + rng.uniform(-0.2, 1.2, (60, 3)) * size
            p[:, axis] = lo[axis] + (side + rng.uniform(-1, 1, 60) * 0.9) * size[axis] if side == 2 else lo[axis] - rng.uniform(0.01, 3, 60) * size[axis]
            pos.append(p)
    pos = np.concatenate(pos)
    pos = np.concatenate([pos, lo + rng.uniform(-0.5, 1.5, (4097 - len(pos), 3)) * size]).astype(F)
    normals = vr.unit_normals(rng, 4097) * (10.0 ** rng.uniform(-3, 3, (4097, 1))).astype(F)  # non-unit normals
    rows = vr.point_rows(pos, normals)
    rows[:, 3], rows[:, 7] = rng.uniform(0, 1, 4097).astype(F), NAN  # (tmin and tmax are not read)
    bad = rng.permutation(4097)[:40]
    for k, x in enumerate(bad):                                  # every class of invalid row
        if k < 18:
            rows[x, (0, 1, 2, 4, 5, 6)[k % 6]] = (NAN, INF, -INF)[k // 6]
        elif k < 24:
            rows[x, 4:7] = 0
        elif k < 32:
            rows[x, 4:7] = vr.unit_normals(rng, 1)[0] * F(1e-25 if k < 28 else 1e-20)  # a squared length that is zero, or subnormal
        else:
            rows[x, 4:7] = vr.unit_normals(rng, 1)[0] * F(1e25)   # one that overflows
    rows = rows[rng.permutation(4097)]
    ok = vr.volume_sample(grid_of((False, False)), vr.probes_of_values(np.ones((9 * 7 * 5, 3))), rows).view(U)[:, 3] != 0
    assert (~ok).sum() == 40
    return rows


# ---- 1. points ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 1, 3), (9, 7, 5)], ids=lambda c: "x".join(map(str, c)))
def test_volume_points_equal_the_restatement_and_stay_inside_their_rows(ds, counts):
    import torch
    spacing = tuple(s if c > 1 else float("nan") for s, c in zip(SPACING, counts))  # (the spacing of a one-probe axis is never read)
    grid = grid_of(counts=counts, spacing=spacing)
    n = grid.n_probes
    for kw in (dict(), dict(tmin=0.25, tmax=7.5), dict(tmin=0.0, tmax=0.0)):
        want = vr.volume_points(grid, **kw)
        assert want.shape == (n, 8) and np.isfinite(want[:, :7]).all()
        assert_words_equal(ds.volume_points(grid, host=True, **kw), want, (counts, kw, "host"))
        assert_words_equal(ds.volume_points(grid, **kw).cpu().numpy(), want, (counts, kw, "device"))
    out = torch.full((n + 2 * G, 8), 7.0, dtype=torch.float32, device="cuda")
    rec = grid.record()
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_volume_points_dev(ds.h, C.byref(rec), 1e-3, float("inf"), C.c_void_p(out[G:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n:] == 7).all()
    assert_words_equal(out[G:G + n].cpu().numpy(), vr.volume_points(grid), (counts, "guarded"))
    # the rows are valid gather points, and a sample AT a probe finds it with weight one: the baker and the sampler agree on the position
    got = ds.volume_sample(grid_of((False, False), counts=counts, spacing=spacing), vr.probes_of_values(np.arange(3 * n).reshape(n, 3) + 1.0), want)
    assert (got[1] == 1).all() and np.allclose(got[0], np.arange(3 * n).reshape(n, 3) + 1.0, rtol=1e-6)


# ---- 2. build -------------------------------------------------------------------------------------------------------------------------------
def test_volume_build_equals_the_restatement_on_every_class_of_row(ds):
    import torch
    grid = grid_of()
    n = grid.n_probes
    sh, vis = random_sums(n, 21)
    d_sh, d_vis = torch.from_numpy(sh).cuda(), torch.from_numpy(vis).cuda()
    for what, v, d_v, radius in (("moments", vis, d_vis, 2.0), ("no visibility", None, None, 2.0), ("no radius", vis, d_vis, None), ("radius 0", vis, d_vis, 0.0),
                                 ("radius inf", vis, d_vis, float("inf")), ("radius NaN", vis, d_vis, float("nan")), ("radius < 0", vis, d_vis, -1.0)):
        want = vr.volume_build(sh, v, radius=0.0 if radius is None else radius)
        flags = want.view(U)[:, 29]
        assert ((flags & 2) != 0).any() == (what == "moments") and (flags == 0).sum() >= 3 * (n // 16)
        got = ds.volume_build(grid, sh, v, radius)
        assert got.dtype == vr.PROBE_DTYPE and got.shape == (n,)
        assert_words_equal(got, want, (what, "host"))
        assert_words_equal(ds.volume_build(grid, d_sh, d_v, radius).cpu().numpy(), want, (what, "device"))
    want = vr.volume_build(sh, vis, radius=2.0)
    # the pair irradiance_sh returns on its host route, and a structured visibility array
    pair = (sh[:, :27].reshape(n, 9, 3), sh.view(U)[:, 27].copy())
    assert_words_equal(ds.volume_build(grid, pair, vis.view(DeviceScene.VISIBILITY_DTYPE).reshape(-1), 2.0), want, "host, as the gathers return them")
    # every class is there and judged as stated
    w = want.view(U)
    dead = (sh.view(U)[:, 27] == 0) | ~np.isfinite(sh[:, :27]).all(axis=1)
    assert dead.sum() == 3 * (n // 16) and (w[dead] == 0).all() and ((w[~dead, 29] & 1) == 1).all() and (w[~dead, 30] == sh.view(U)[~dead, 27]).all()
    no_moments = ~dead & ((vis.view(U)[:, 7] == 0) | ~np.isfinite(vis[:, 4]) | ~np.isfinite(vis[:, 5]))
    assert no_moments.sum() > 0 and (w[no_moments, 29] == 1).all() and (w[no_moments, 27:29] == 0).all() and (w[~dead & ~no_moments, 29] == 3).all()
    # guard rows around the output of the device route
    out = torch.full((n + 2 * G, 32), 7.0, dtype=torch.float32, device="cuda")
    rec = grid.record()
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_volume_build_dev(ds.h, C.byref(rec), C.c_void_p(d_sh.data_ptr()), C.c_void_p(d_vis.data_ptr()), 2.0, C.c_void_p(out[G:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n:] == 7).all()
    assert_words_equal(out[G:G + n].cpu().numpy(), want, "guarded")
    assert_words_equal(volume_probes_to_numpy(out[G:G + n].contiguous()), want, "as a structured array")


# ---- 3. sample ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_volume_sample_equals_the_restatement_word_for_word(ds, probes, points, flags):
    import torch
    d_probes, d_points = torch.from_numpy(probes).cuda(), torch.from_numpy(points).cuda()
    for bias in (0.0, 0.25):
        grid = grid_of(flags, bias)
        want = vr.volume_sample(grid, probes, points)
        count = want.view(U)[:, 3]
        assert (count <= 8).all() and (count == 8).sum() > 300 and (count == 0).sum() >= 40 and len(set(count)) >= 8
        assert np.isfinite(want[:, :3]).all() and (want[:, :3] >= 0).all()
        rgb, samples = ds.volume_sample(grid, probes, points)
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), want, (flags, bias, "host"))
        got = ds.volume_sample(grid, d_probes, d_points)
        assert_words_equal(got.cpu().numpy(), want, (flags, bias, "device"))
        # batch sizes around the wave and the block; the answer of a point does not depend on its neighbours
        for n in (1, 63, 64, 65):
            assert_words_equal(ds.volume_sample(grid, d_probes, d_points[:n].contiguous()).cpu().numpy(), want[:n], (flags, bias, n))
        rgb, samples = ds.volume_sample(grid, volume_probes_to_numpy(d_probes), points[:65])
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), want[:65], (flags, bias, "host, 65"))
        perm = np.random.default_rng(5).permutation(len(points))
        moved = ds.volume_sample(grid, d_probes, torch.from_numpy(points[perm]).cuda())
        assert_words_equal(moved.cpu().numpy(), want[perm], (flags, bias, "permuted"))
    # the flags do something on this data
    plain = vr.volume_sample(grid_of((False, False), 0.25), probes, points)
    assert flags == (False, False) or (want.view(U) != plain.view(U)).any(axis=1).mean() > 0.3
    # guard rows around the output, and an empty call that touches nothing
    out = torch.full((len(points) + 2 * G, 4), 7.0, dtype=torch.float32, device="cuda")
    rec = grid.record()
    torch.cuda.synchronize()
    for n in (0, len(points)):
        ds._chk(ds.lib.sol_volume_sample_dev(ds.h, C.byref(rec), C.c_void_p(d_probes.data_ptr()), C.c_void_p(d_points.data_ptr()), n, C.c_void_p(out[G:].data_ptr())))
        ds.sync()
        assert (out[:G] == 7).all() and (out[G + n:] == 7).all()
    assert_words_equal(out[G:G + len(points)].cpu().numpy(), want, (flags, "guarded"))
    empty = ds.volume_sample(grid, d_probes, d_points[:0].contiguous())
    assert tuple(empty.shape) == (0, 4)
    # a contiguous view that starts 4 bytes into an allocation is refused where it is handed over: the kernels move 16-byte words
    shifted = torch.zeros(65 * 8 + 1, dtype=torch.float32, device="cuda")[1:].view(65, 8)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        ds.volume_sample(grid, d_probes, shifted)


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_a_grid_with_a_one_probe_axis(ds, flags):
    import torch
    rng = np.random.default_rng(31)
    counts, spacing = (2, 1, 3), (SPACING[0], float("nan"), SPACING[2])
    sh, vis = random_sums(6, 32)
    sh.view(U)[:, 27] = np.maximum(sh.view(U)[:, 27], 1)  # (six probes: keep them all)
    sh[~np.isfinite(sh)] = 1.0
    probes = vr.volume_build(sh, vis, radius=2.0)
    assert (probes.view(U)[:, 29] & 1).all()
    at = vr.probe_positions(grid_of(counts=counts, spacing=spacing))
    lo, size = at[0].astype(np.float64), (at[-1] - at[0]).astype(np.float64) + (0, 2.0, 0)
    pos = np.concatenate([lo + rng.uniform(-0.5, 1.5, (500, 3)) * size - (0, 1.0, 0), at]).astype(F)
    rows = vr.point_rows(pos, vr.unit_normals(rng, len(pos)))
    for bias in (0.0, 0.25):
        grid = grid_of(flags, bias, counts, spacing)
        want = vr.volume_sample(grid, probes, rows)
        assert want.view(U)[:, 3].max() == 4 and (flags[1] or (want.view(U)[:, 3] >= 1).all())  # never the second layer along y
        rgb, samples = ds.volume_sample(grid, probes, rows)
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), want, (flags, bias, "host"))
        got = ds.volume_sample(grid, torch.from_numpy(probes).cuda(), torch.from_numpy(rows).cuda())
        assert_words_equal(got.cpu().numpy(), want, (flags, bias, "device"))


def test_a_stream_of_the_callers(ds, probes, points):
    import torch
    grid = grid_of((True, True), 0.25)
    sh, vis = random_sums(grid.n_probes, 41)
    want_probes = vr.volume_build(sh, vis, radius=1.5)
    want = vr.volume_sample(grid, want_probes, points)
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)
    try:
        assert_words_equal(ds.volume_points(grid).cpu().numpy(), vr.volume_points(grid), "points on the caller's stream")
        built = ds.volume_build(grid, torch.from_numpy(sh).cuda(), torch.from_numpy(vis).cuda(), 1.5)
        assert_words_equal(built.cpu().numpy(), want_probes, "probes on the caller's stream")
        got = ds.volume_sample(grid, built, torch.from_numpy(points).cuda())
        assert_words_equal(got.cpu().numpy(), want, "samples on the caller's stream")
        rgb, samples = ds.volume_sample(grid, ds.volume_build(grid, sh, vis, 1.5), points)
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), want, "host routes on the caller's stream")
    finally:
        ds.set_stream(0)


# ---- 4. the whole chain -----------------------------------------------------------------------------------------------------------------------
def test_points_then_gathers_then_build_then_sample_is_the_chain_of_the_restatement():
    import torch
    sc, V, T, N = floor_under_a_light()  # the floor spans x, z in [-2, 2] near y = 0; the light is the quad x, z in [-1, 1] at y = 2
    grid = VolumeGrid((-2.0, 0.3, -2.0), (1.0, 0.5, 1.0), (5, 3, 5), normal_bias=0.05)
    radius = 4.0
    g = np.linspace(-1.9, 1.9, 20)
    x, z = np.meshgrid(g, g)
    h = 0.1 * np.sin(3.0 * (x + 2) / 4) * np.cos(2.0 * (z + 2) / 4)  # (the floor's height field: the points lie on it up to the mesh's facets)
    floor = vr.point_rows(np.stack([x, h, z], axis=-1).reshape(-1, 3), [(0, 1, 0)])
    with DeviceScene(sc) as ds:
        sh = ds.irradiance_sh(ds.volume_points(grid), samples=256, seed=SEED, mode="sphere")
        vis = ds.visibility(ds.volume_points(grid, tmax=radius), samples=256, seed=SEED, mode="sphere", distances=True)
        built = ds.volume_build(grid, sh, vis, radius)
        out = ds.volume_sample(grid, built, torch.from_numpy(floor).cuda())
        baked = ds.lightmap_dilate(out, torch.zeros((400, 4), dtype=torch.int32, device="cuda"), 20, 20, passes=0)  # (every texel owned: the rows pass as they are)
    sh, vis, built, out = (a.cpu().numpy() for a in (sh, vis, built, out))
    assert (sh.view(U)[:, 27] == 256).all() and (vis.view(U)[:, 7] == 256).all()
    want_probes = vr.volume_build(sh, vis, radius)
    assert_words_equal(built, want_probes, "the probes from the device's own sums")
    assert (want_probes.view(U)[:, 29] == 3).all()
    want = vr.volume_sample(grid, want_probes, floor)
    assert_words_equal(out, want, "the floor from the device's own probes")
    assert_words_equal(baked.cpu().numpy(), want, "sampled rows are rows lightmap_dilate takes")
    assert (want.view(U)[:, 3] >= 1).all()
    lum = want[:, :3].sum(axis=1).reshape(20, 20)
    under = lum[8:12, 8:12].mean()  # below the light's centre
    corners = np.mean([lum[:3, :3].mean(), lum[:3, -3:].mean(), lum[-3:, :3].mean(), lum[-3:, -3:].mean()])
    assert under > 1.5 * corners > 0.0, (under, corners)


# ---- 5. neutrality ----------------------------------------------------------------------------------------------------------------------------
def test_volume_calls_between_renders_change_no_frame_plane_or_statistic(points):
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    grid = grid_of((True, True), 0.25)
    sh, vis = random_sums(grid.n_probes, 51)

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
        vis_rows = ds.visibility_to_numpy(ds.visibility(ds.camera_rays(0, 0, 8, 8, 1, SEED).reshape(-1, 8), samples=20, seed=SEED))
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(radiance.tobytes()), zlib.crc32(vis_rows.tobytes()))

    with DeviceScene(sc) as ds:
        d_sh, d_vis, d_points = torch.from_numpy(sh).cuda(), torch.from_numpy(vis).cuda(), torch.from_numpy(points).cuda()

        def volume():
            at = ds.volume_points(grid)
            built = ds.volume_build(grid, ds.irradiance_sh(at, samples=2, seed=SEED, mode="sphere"), d_vis, 2.0)
            ds.volume_sample(grid, built, d_points)
            ds.volume_sample(grid, ds.volume_build(grid, sh, vis, 2.0), points[:100])
            ds.volume_sample(grid, ds.volume_build(grid, d_sh), ds.volume_points(grid, host=True))

        want = sequence(ds, lambda: None)
        assert sequence(ds, volume) == want and want[3]["rays"] > 0


def test_a_scene_with_a_constant_medium_is_served(points):
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    grid = grid_of((True, True), 0.25)
    sh, vis = random_sums(grid.n_probes, 61)
    with DeviceScene(sc) as ds:
        assert_words_equal(ds.volume_points(grid, host=True), vr.volume_points(grid), "points on a scene with a medium")
        built = ds.volume_build(grid, sh, vis, 2.0)
        assert_words_equal(built, vr.volume_build(sh, vis, 2.0), "probes on a scene with a medium")
        rgb, samples = ds.volume_sample(grid, built, points[:300])
        assert_words_equal(np.concatenate([rgb, samples.view(F)[:, None]], axis=1), vr.volume_sample(grid, probes_rows(built), points[:300]), "samples on a scene with a medium")


def probes_rows(built):
    return np.ascontiguousarray(built).view(F).reshape(-1, 32)
