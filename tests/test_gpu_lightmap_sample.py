"""Lightmap lookups on the device (sol_lightmap_coords / sol_lightmap_sample). The yardstick is tests/lightmap_sample_ref.py, the rule
restated in numpy float32: every answer is compared word for word, NaN for NaN, over every row - bilinear and nearest, with and without the
dilation's plane, with and without the chart guard, on the host route and the device route. Around it: guard words, a stream of the caller's, the
hits of a camera turned into surface rows and checked geometrically, the whole chain from a bake to a view, and neutrality. Atlases are at most
130 x 67, rows a few hundred."""
import ctypes as C
import zlib

import numpy as np
import pytest

import lightmap_ref as lr
import lightmap_sample_ref as sr
import parity_util as pu
from solstrale_amd import (CameraConfig, DeviceScene, RenderConfig, SceneBuilder, _abi, lightmap_mesh, lightmap_texels_to_numpy, lightmap_triangle_table,
                           scenes)
from test_gpu_irradiance import _path_stats
from test_lightmap_sample_abi import invalid_rows

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F = np.float32
EPS = float(np.finfo(F).eps) / 2
INF, NAN = F(np.inf), F(np.nan)
RC = RenderConfig(32, 32, 1)
ATLASES = [(1, 1), (5, 3), (300, 1), (64, 64), (130, 67)]
CHANNELS = [(1, 1), (3, 4), (27, 28), (2, 5)]  # (channels, words of a row)


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (the geometry of a lookup is the caller's: any handle serves)
        yield d


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape[0] == want.shape[0], (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(got.shape[0], -1), want.view(np.uint32).reshape(want.shape[0], -1)
    if g.shape != w.shape or (g != w).any():
        bad = np.nonzero((g != w).any(axis=1))[0]
        raise AssertionError((what, len(bad), len(g), bad[:5], got[bad[:3]], want[bad[:3]]))


def texels_tensor(texels):
    import torch
    return torch.from_numpy(np.ascontiguousarray(texels).view(np.int32).reshape(-1, 4)).cuda()


# ---- the mesh and the rows every lookup test shares ------------------------------------------------------------------------------------------
HOLE = (6, 6)  # the 2 x 2 block of grid cells from here on is left out of the rasterisation: the hole
HOLE_CORNER = (2 + 2 * (7 * 8 + 7), 2 + 2 * (7 * 8 + 7) + 2)  # the two triangles of the hole's last cell: no dilation of four passes reaches them


def lookup_mesh():
    """(vertices, uvs, rasterised): two overlapping charts in front (the lowest index wins their texels), the jittered 8 x 8 grid mesh over all of
    [0, 1]^2, then a triangle whose UVs lie far outside, one with a UV word that is not finite and one with a vertex word that is not finite.
    rasterised: the UVs ownership is made from - the grid's top right 2 x 2 cells degenerate, so that the atlas has a hole the rows still reach."""
    over = np.asarray([[(0.1, 0.1), (0.9, 0.15), (0.4, 0.8)], [(0.3, 0.05), (0.95, 0.6), (0.2, 0.9)]], dtype=F)
    V, T, _ = lr.grid_mesh(8, 3)
    extra = np.asarray([[(1e30, 0.5), (0.5, 1e30), (-1e30, -1e30)], [(0.2, 0.2), (NAN, 0.3), (0.3, 0.8)], [(0.6, 0.2), (0.8, 0.3), (0.7, 0.5)]], dtype=F)
    uvs = np.concatenate([over, T, extra])
    over_v = lr.lift(over)
    over_v[0, :, 1], over_v[1, :, 1] = 1.0, 2.0
    vertices = np.concatenate([over_v, V, lr.lift(np.nan_to_num(np.clip(extra, -8, 8)))])
    vertices[-1, 2, 0] = INF
    rasterised = uvs.copy()
    for y in range(HOLE[1], 8):
        for x in range(HOLE[0], 8):
            rasterised[2 + 2 * (y * 8 + x): 2 + 2 * (y * 8 + x) + 2] = 0.0
    return vertices, uvs, rasterised


def lookup_rows(uvs, texel_rows, n=257, seed=21):
    """n surface rows: random points of every triangle (the hole's, the far one's and the bad ones' too), every border vertex of the grid (u or v
    exactly 0 or 1), texel rows of a conservative rasterisation, and one row of every invalid class between good rows."""
    rng = np.random.default_rng(seed)
    nt = len(uvs)
    at = np.argwhere(np.isin(uvs[2:-3], (0.0, 1.0)).any(axis=2))  # (grid triangle, corner) on the border of [0, 1]^2
    corner = np.zeros(len(at), dtype=sr.TEXEL_DTYPE)
    corner["triangle"], corner["flags"] = at[:, 0] + 2, 1
    corner["b1"], corner["b2"] = (at[:, 1] == 1), (at[:, 1] == 2)
    corner = corner[rng.permutation(len(corner))[:48]]
    names, bad = invalid_rows(nt, nt - 2, None)
    tex = texel_rows[rng.permutation(len(texel_rows))[:40]]
    n_random = n - len(corner) - len(bad) - len(tex)
    b = rng.dirichlet((1.0, 1.0, 1.0), n_random).astype(F)
    rand = np.zeros(n_random, dtype=sr.TEXEL_DTYPE)
    rand["triangle"], rand["b1"], rand["b2"], rand["flags"] = rng.integers(0, nt, n_random), b[:, 1], b[:, 2], rng.integers(1, 3, n_random)
    rand["triangle"][:24] = rng.integers(HOLE_CORNER[0], HOLE_CORNER[1], 24)  # (well inside the hole)
    rows = np.concatenate([rand, corner, tex])
    rows = rows[rng.permutation(len(rows))]
    where = np.sort(rng.permutation(len(rows) - 2)[:len(bad)] + 1)
    rows = np.insert(rows, where, bad)  # each between good rows
    assert len(rows) == n
    return rows


class Atlas:
    """One atlas of the shared mesh: ownership (conservative), and per dilation the plane and per channel layout the dilated values with taps that
    are not finite put in afterwards."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.vertices, self.uvs, rasterised = lookup_mesh()
        self.points, self.texels = lr.lightmap_points(self.vertices, rasterised, W, H, conservative=True)
        self.rows = lookup_rows(self.uvs, self.texels[self.texels["flags"] != 0] if (self.texels["flags"] != 0).any() else self.texels)
        self.values, self.pass_of = {}, {}
        rng = np.random.default_rng(W * 1000 + H)
        for channels, words in CHANNELS:
            raw = (rng.normal(size=(W * H, words)) * rng.choice([1e-3, 1.0, 1e4], (W * H, 1))).astype(F)
            raw[:, channels:] = np.arange(W * H * (words - channels), dtype=np.uint32).reshape(W * H, -1).view(F)
            for passes in (0, 1, 4):
                out, pass_of = lr.lightmap_dilate(raw, self.texels, W, H, passes=passes, channels=channels)
                out = out.copy()
                spoil = rng.random(W * H) < 0.06
                out[spoil, rng.integers(0, channels, int(spoil.sum()))] = rng.choice([INF, -INF, NAN], int(spoil.sum()))
                self.values[(channels, passes)], self.pass_of[passes] = out, pass_of
            self.values[(channels, None)] = self.values[(channels, 0)]


_atlases = {}


def atlas(W, H):
    if (W, H) not in _atlases:
        _atlases[(W, H)] = Atlas(W, H)
    return _atlases[(W, H)]


# ---- 1. the lookup ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_the_lookup_equals_the_restatement_word_for_word(ds, W, H):
    import torch
    A = atlas(W, H)
    d_uvs, d_texels, d_rows = torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), texels_tensor(A.rows)
    seen = set()
    for channels, words in CHANNELS:
        for passes in (None, 0, 1, 4):
            values = A.values[(channels, passes)]
            pass_of = None if passes is None else A.pass_of[passes]
            d_values = torch.from_numpy(values).cuda()
            d_pass = None if pass_of is None else torch.from_numpy(pass_of).cuda()
            for nearest in (False, True):
                tag = (W, H, channels, passes, "nearest" if nearest else "bilinear")
                want = sr.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                got = ds.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                assert got.shape == (len(A.rows), channels + 1)
                assert_words_equal(got, want, tag + ("host",))
                got = ds.lightmap_sample(d_values, d_rows, d_uvs, d_texels, W, H, channels=channels, pass_of=d_pass, nearest=nearest)
                assert_words_equal(got.cpu().numpy(), want, tag + ("device",))
                count = want[:, channels].view(np.uint32)
                assert np.isfinite(want[:, :channels]).all() and (count <= (1 if nearest else 4)).all()
                seen |= set(np.unique(count))
    if (W, H) == (64, 64):  # the cases the rows are made for are there
        assert seen == {0, 1, 2, 3, 4}
        want, taps = sr.lightmap_sample(A.values[(3, 4)], A.rows, A.uvs, A.texels, W, H, pass_of=A.pass_of[4], return_taps=True)
        hole = (A.rows["triangle"] >= HOLE_CORNER[0]) & (A.rows["triangle"] < HOLE_CORNER[1]) & (A.rows["flags"] != 0) & sr.finite(A.rows["b1"])
        assert hole.sum() >= 24 and (~taps[hole].any(axis=1)).sum() >= 12  # valid rows with all four taps uncovered, even after four passes
        far = A.rows["triangle"] == len(A.uvs) - 3
        assert far.any() and (want[far].view(np.uint32) == 0).all()  # UVs of 1e30: no tap
        assert (A.texels["flags"] == 2).any() and (A.rows["flags"] == 2).any()


@pytest.mark.parametrize("channels, words", [(3, 4), (27, 28)], ids=["radiance_rows", "sh9_rows"])
def test_row_counts_around_a_wave_a_permutation_and_guard_words(ds, channels, words):
    import torch
    W, H, G = 130, 67, 64
    A = atlas(W, H)
    values, pass_of = A.values[(channels, 1)], A.pass_of[1]
    want = sr.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, channels=channels, pass_of=pass_of)
    d_uvs, d_texels, d_values, d_pass = torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), torch.from_numpy(values).cuda(), torch.from_numpy(pass_of).cuda()
    for n in (1, 63, 64, 65, 257):
        got = ds.lightmap_sample(d_values, texels_tensor(A.rows[:n]), d_uvs, d_texels, W, H, channels=channels, pass_of=d_pass)
        assert_words_equal(got.cpu().numpy(), want[:n], (channels, n, "device"))
        assert_words_equal(ds.lightmap_sample(values, A.rows[:n], A.uvs, A.texels, W, H, channels=channels, pass_of=pass_of), want[:n], (channels, n, "host"))
    perm = np.random.default_rng(5).permutation(len(A.rows))
    got = ds.lightmap_sample(d_values, texels_tensor(A.rows[perm]), d_uvs, d_texels, W, H, channels=channels, pass_of=d_pass)
    assert_words_equal(got.cpu().numpy(), want[perm], (channels, "permuted"))
    # guard words before and after out (the raw call)
    n = len(A.rows)
    out = torch.full((2 * G + n * (channels + 1),), 7.0, dtype=torch.float32, device="cuda")
    d_rows = texels_tensor(A.rows)
    cfg = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=channels, stride_bytes=4 * words, flags=0, chart_radius=float("inf"))
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_lightmap_sample_dev(ds.h, C.byref(cfg), C.c_void_p(d_uvs.data_ptr()), len(A.uvs), C.c_void_p(d_texels.data_ptr()), C.c_void_p(d_pass.data_ptr()),
                                            C.c_void_p(d_values.data_ptr()), None, None, C.c_void_p(d_rows.data_ptr()), n, C.c_void_p(out[G:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n * (channels + 1):] == 7).all()
    assert_words_equal(out[G:G + n * (channels + 1)].cpu().numpy().reshape(n, channels + 1), want, (channels, "guarded"))
    # n == 0 writes nothing
    ds._chk(ds.lib.sol_lightmap_sample_dev(ds.h, C.byref(cfg), C.c_void_p(d_uvs.data_ptr()), len(A.uvs), C.c_void_p(d_texels.data_ptr()), None,
                                            C.c_void_p(d_values.data_ptr()), None, None, C.c_void_p(d_rows.data_ptr()), 0, C.c_void_p(out.data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all()


def test_a_stream_of_the_callers(ds):
    import torch
    W, H = 64, 64
    A = atlas(W, H)
    values, pass_of = A.values[(3, 4)], A.pass_of[4]
    want = sr.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, pass_of=pass_of)
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)
    try:
        got = ds.lightmap_sample(torch.from_numpy(values).cuda(), texels_tensor(A.rows), torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), W, H,
                                 pass_of=torch.from_numpy(pass_of).cuda())
        assert_words_equal(got.cpu().numpy(), want, "device route on the caller's stream")
        assert_words_equal(ds.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, pass_of=pass_of), want, "host route on the caller's stream")
    finally:
        ds.set_stream(0)


# ---- 2. the chart guard -----------------------------------------------------------------------------------------------------------------------
def two_charts(W=16, H=8):
    """The left half of the atlas is a bright chart at x = 0 in the world, the right half a dark one 100 units away: adjacent, no gutter."""
    uvs = np.asarray([[(0.0, 0.0), (0.5, 0.0), (0.5, 1.0)], [(0.0, 0.0), (0.5, 1.0), (0.0, 1.0)],
                      [(0.5, 0.0), (1.0, 0.0), (1.0, 1.0)], [(0.5, 0.0), (1.0, 1.0), (0.5, 1.0)]], dtype=F)
    vertices = lr.lift(uvs)
    vertices[2:, :, 0] += F(100.0)
    points, texels = lr.lightmap_points(vertices, uvs, W, H)
    assert (texels["triangle"] != lr.NONE).all()
    values = np.zeros((W * H, 4), dtype=F)
    values[texels["triangle"] < 2, :3] = 1.0
    return uvs, vertices, points, texels, values


def test_the_chart_guard_keeps_a_neighbouring_chart_out(ds):
    import torch
    W, H = 16, 8
    uvs, vertices, points, texels, values = two_charts(W, H)
    rng = np.random.default_rng(31)
    n = 200
    rows = np.zeros(n, dtype=sr.TEXEL_DTYPE)  # points of the dark chart, the first half of them within a third of a texel of the shared border
    rows["triangle"], rows["flags"] = 3, 1  # corners (0.5, 0), (1, 1), (0.5, 1): u = 0.5 + 0.5 b1, v = b1 + b2
    s, t = rng.uniform(0, 1, n), rng.uniform(0.1, 0.9, n)
    s[:n // 2] = rng.uniform(0.0, 0.02, n // 2)  # s * 8 texels from the border
    rows["b1"], rows["b2"] = s.astype(F), ((1 - s) * t).astype(F)
    dev = [torch.from_numpy(a).cuda() for a in (values, uvs, vertices, points)]
    d_rows, d_texels = texels_tensor(rows), texels_tensor(texels)
    answers = {}
    for radius in (None, 5.0, float("inf"), 1e-6):
        kw = {} if radius is None else dict(chart_radius=radius, vertices=vertices, points=points)
        want = sr.lightmap_sample(values, rows, uvs, texels, W, H, **{**kw, "chart_radius": np.inf if radius is None else radius})
        assert_words_equal(ds.lightmap_sample(values, rows, uvs, texels, W, H, **kw), want, ("host", radius))
        dkw = {} if radius is None else dict(chart_radius=radius, vertices=dev[2], points=dev[3])
        assert_words_equal(ds.lightmap_sample(dev[0], d_rows, dev[1], d_texels, W, H, **dkw).cpu().numpy(), want, ("device", radius))
        want_n = sr.lightmap_sample(values, rows, uvs, texels, W, H, nearest=True, **{**kw, "chart_radius": np.inf if radius is None else radius})
        assert_words_equal(ds.lightmap_sample(dev[0], d_rows, dev[1], d_texels, W, H, nearest=True, **dkw).cpu().numpy(), want_n, ("nearest", radius))
        answers[radius] = want
    border = np.arange(n) < n // 2
    assert (answers[None][border, 0] > 0).all()                       # without the guard the bright chart bleeds into the dark one
    assert (answers[5.0][:, :3] == 0).all()                            # with it the dark chart is exactly dark
    assert (answers[5.0][:, 3].view(np.uint32) >= 1).all() and (answers[5.0][border, 3].view(np.uint32) <= 2).all()
    assert_words_equal(answers[float("inf")], answers[None], "+inf is no guard")
    assert (answers[1e-6].view(np.uint32) == 0).all()                  # no owned texel lies within 1e-6 of these points
    # the dilated-tap exception: the bright chart's texels lose their owner but stay covered - no point row, so the guard cannot refuse them
    filled = texels.copy()
    was_bright = texels["triangle"] < 2
    filled["triangle"][was_bright], filled["flags"][was_bright] = lr.NONE, 0
    pass_of = np.where(was_bright, 1, 0).astype(np.uint8).reshape(H, W)
    want = sr.lightmap_sample(values, rows, uvs, filled, W, H, pass_of=pass_of, chart_radius=5.0, vertices=vertices, points=points)
    got = ds.lightmap_sample(dev[0], d_rows, dev[1], texels_tensor(filled), W, H, pass_of=torch.from_numpy(pass_of).cuda(), chart_radius=5.0, vertices=dev[2],
                             points=dev[3])
    assert_words_equal(got.cpu().numpy(), want, "dilated taps under the guard")
    assert_words_equal(ds.lightmap_sample(values, rows, uvs, filled, W, H, pass_of=pass_of, chart_radius=5.0, vertices=vertices, points=points), want,
                       "dilated taps under the guard, host")
    assert (want[border, 0] > 0).all()
    tiny = sr.lightmap_sample(values, rows, uvs, filled, W, H, pass_of=pass_of, chart_radius=1e-6, vertices=vertices, points=points)
    got = ds.lightmap_sample(dev[0], d_rows, dev[1], texels_tensor(filled), W, H, pass_of=torch.from_numpy(pass_of).cuda(), chart_radius=1e-6, vertices=dev[2],
                             points=dev[3])
    assert_words_equal(got.cpu().numpy(), tiny, "only the dilated taps are left")
    assert (tiny[border, 0] == 1).all() and (tiny[~border & (s > 0.3)].view(np.uint32) == 0).all()
    # a vertex word that is not finite makes the row invalid under the guard only
    broken = vertices.copy()
    broken[3, 1, 2] = NAN  # (the rows' triangle)
    want = sr.lightmap_sample(values, rows, uvs, texels, W, H, chart_radius=5.0, vertices=broken, points=points)
    assert (want.view(np.uint32) == 0).all()
    assert_words_equal(ds.lightmap_sample(dev[0], d_rows, dev[1], d_texels, W, H, chart_radius=5.0, vertices=torch.from_numpy(broken).cuda(), points=dev[3]).cpu().numpy(),
                       want, "a vertex word that is not finite")


# ---- 3. coords --------------------------------------------------------------------------------------------------------------------------------
def floor_under_a_light():
    """The scene of tests/test_gpu_lightmap.py, built afresh: a triangle floor (the jittered grid mesh, its lightmap chart in the middle three
    quarters of the atlas) under a quad light. Returns the scene and the floor as the DESCRIPTION lists it (the flattener's order): vertices,
    uvs, and the same in float64."""
    V, T, N = lr.grid_mesh(8, 2)
    V, T = (np.ascontiguousarray(a[:, [0, 2, 1]]) for a in (V, T))  # (wound so that the geometric normals point up, at the light)
    T = np.ascontiguousarray(T * F(0.75) + F(0.125), dtype=F)
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(0.7, 0.7, 0.7))
    first, n = b.triangles(V.astype(np.float64), grey, uvs=T)
    light = b.Quad((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), b.DiffuseLight(8, 8, 8))
    cam = CameraConfig(40.0, 0.0, (0.0, 6.0, 6.0), (0.0, 0.0, 0.0), (0, 1, 0))
    sc = b.finish(b.Bvh(list(range(first, first + n)) + [light]), cam, (0.0, 0.0, 0.0), RC)
    assert sc.desc.n_triangles == n == 128
    mesh_v, mesh_t = lightmap_mesh(sc, 0, n)
    assert sorted(map(bytes, mesh_t)) == sorted(map(bytes, T))  # the same triangles, in the flattener's order
    return sc, mesh_v, mesh_t


def test_coords_of_camera_hits_equal_the_restatement_and_lie_on_the_ray():
    """The geometric check pins the (u, v) convention. The device solves o + t d = v0 + u e1 + v e2 in fp32 by Moeller-Trumbore: t, u and v are
    quotients of triple products. A triple product of vectors a, b, c computed in fp32 is off by at most about 4 EPS |a| |b| |c| (two roundings per
    cross-product component, three more in the dot product, to first order), and the determinant is |d| 2A cos(theta), A the triangle's area and
    theta the angle between ray and normal. With D = |o| + t |d| + max |vertex| bounding every vector's length, the error of u moves the point
    by |e1| du <= 4 EPS D |e1| |e2| / (2A cos(theta)) = 4 EPS D kappa / cos(theta), kappa = 1 / sin(the corner's angle); the same for v, and for t
    along the ray; numerator and determinant each err, so twice that: 3 x 2 x 4 = 24 EPS D kappa / cos(theta). The record's fp32 cast, the ray's
    own fp32 words and the conversion's (1 - u) - v add a few EPS D. kappa is taken as the largest of the triangle's three corners (the record
    starts at one of them). The bound used is 32 EPS D kappa / cos(theta)."""
    import torch
    sc, V, T = floor_under_a_light()
    n_tri = len(V)
    table = lightmap_triangle_table(sc, 0, n_tri)
    assert set(np.unique(table[table != sr.NONE] >> 30)) == {0, 1, 2}  # every rotation occurs among the jittered triangles
    with DeviceScene(sc) as ds:
        rays = ds.camera_rays(0, 0, 32, 32, 0, SEED).reshape(-1, 8)
        d_hits = ds.closest_hits(rays)
        hits = ds.hits_to_numpy(d_hits)
        is_tri = (hits["status"] == 1) & (hits["kind"] == sr.REF_TRIANGLE)
        n_quad, n_miss = int(((hits["status"] == 1) & (hits["kind"] == sr.REF_QUAD)).sum()), int((hits["status"] == 0).sum())
        print(f"coords: {int(is_tri.sum())} floor hits, {n_quad} light hits, {n_miss} misses of {len(hits)} rays")
        assert is_tri.sum() > 200 and n_quad > 0 and n_miss > 0
        holes = table.copy()
        holes[::5] = sr.NONE
        for name, tab in (("whole", table), ("some without lightmap", holes), ("short", table[:len(table) // 2]), ("empty", table[:0])):
            want = sr.lightmap_coords(hits, tab)
            assert_words_equal(lightmap_texels_to_numpy(ds.lightmap_coords(d_hits, tab)), want, (name, "device"))
            assert_words_equal(ds.lightmap_coords(hits, tab), want, (name, "host"))
        assert_words_equal(lightmap_texels_to_numpy(ds.lightmap_coords(d_hits, torch.from_numpy(table.view(np.int32)).cuda())), sr.lightmap_coords(hits, table),
                           "a table on the device")
        assert (sr.lightmap_coords(hits, holes)["flags"][is_tri] == 0).sum() > 20 and (sr.lightmap_coords(hits, table[:64])["flags"][is_tri] == 0).sum() > 20
        rows = sr.lightmap_coords(hits, table)
        assert (rows["flags"] == is_tri).all()
        # a guarded output and n == 0
        out = torch.full((len(hits) + 16, 4), 7, dtype=torch.int32, device="cuda")
        d_table = torch.from_numpy(table.view(np.int32)).cuda()
        torch.cuda.synchronize()
        ds._chk(ds.lib.sol_lightmap_coords_dev(ds.h, C.c_void_p(d_hits.data_ptr()), len(hits), C.c_void_p(d_table.data_ptr()), len(table), C.c_void_p(out[8:].data_ptr())))
        ds._chk(ds.lib.sol_lightmap_coords_dev(ds.h, C.c_void_p(d_hits.data_ptr()), 0, C.c_void_p(d_table.data_ptr()), len(table), C.c_void_p(out.data_ptr())))
        ds.sync()
        assert (out[:8] == 7).all() and (out[8 + len(hits):] == 7).all()
        assert_words_equal(lightmap_texels_to_numpy(out[8:8 + len(hits)].contiguous()), rows, "guarded coords")
    r = rays.cpu().numpy().astype(np.float64)[is_tri]
    h, c = hits[is_tri], rows[is_tri]
    tri = np.zeros((n_tri, 3, 3))
    for k in range(n_tri):
        t = sc.desc.triangles[k]
        tri[k, 0] = t.v0[:]
        tri[k, 1], tri[k, 2] = tri[k, 0] + np.asarray(t.v0v1[:]), tri[k, 0] + np.asarray(t.v0v2[:])
    P = tri[c["triangle"]]
    b1, b2 = c["b1"].astype(np.float64)[:, None], c["b2"].astype(np.float64)[:, None]
    on_triangle = P[:, 0] + b1 * (P[:, 1] - P[:, 0]) + b2 * (P[:, 2] - P[:, 0])
    on_ray = r[:, 0:3] + h["t"].astype(np.float64)[:, None] * r[:, 4:7]
    e = [P[:, 1] - P[:, 0], P[:, 2] - P[:, 1], P[:, 0] - P[:, 2]]
    normal = np.cross(e[0], -e[2])
    area2 = np.linalg.norm(normal, axis=1)
    length = [np.linalg.norm(x, axis=1) for x in e]
    kappa = np.max([length[0] * length[2], length[0] * length[1], length[1] * length[2]], axis=0) / area2
    cos_theta = np.abs((normal * r[:, 4:7]).sum(axis=1)) / (area2 * np.linalg.norm(r[:, 4:7], axis=1))
    D = np.linalg.norm(r[:, 0:3], axis=1) + h["t"] * np.linalg.norm(r[:, 4:7], axis=1) + np.abs(tri).max()
    bound = 32 * EPS * D * kappa / cos_theta
    gap = np.linalg.norm(on_triangle - on_ray, axis=1)
    print(f"coords: {len(gap)} triangle hits, largest gap / bound {np.max(gap / bound):.3f}, bound {bound.min():.2e} .. {bound.max():.2e}")
    assert (gap <= bound).all()
    assert bound.max() < 1e-3  # (against a wrong convention the check has teeth: a point of another corner's frame is a triangle's size away)
    wrong = P[:, 0] + h["u"].astype(np.float64)[:, None] * (P[:, 1] - P[:, 0]) + h["v"].astype(np.float64)[:, None] * (P[:, 2] - P[:, 0])
    rotated = (table[h["dfs_index"]] >> 30) != 0
    assert rotated.sum() > 100 and (np.linalg.norm(wrong - on_ray, axis=1)[rotated] > 1e-2).mean() > 0.9  # the raw (u, v) are NOT the description's frame


# ---- 4. the chain -----------------------------------------------------------------------------------------------------------------------------
def test_bake_then_view_is_the_four_calls_and_shows_the_light():
    import torch
    W = H = 32
    sc, V, T = floor_under_a_light()
    table = lightmap_triangle_table(sc, 0, len(V))
    with DeviceScene(sc) as ds:
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        points, texels = ds.lightmap_points(dV, dT, W, H)
        rows = ds.irradiance(points, samples=17, seed=SEED)
        baked, pass_of = ds.lightmap_dilate(rows, texels, W, H, passes=2, return_pass_of=True)
        # nearest, at the device's own texel rows: the baked rows' words
        own = torch.nonzero(texels[:, 3] == 1)[:, 0]
        assert 0.5 * W * H < len(own) < 0.65 * W * H
        got = ds.lightmap_sample(baked, texels[own].contiguous(), dT, texels, W, H, pass_of=pass_of, nearest=True)
        assert_words_equal(got[:, :3].cpu().numpy(), baked[own][:, :3].cpu().numpy(), "nearest at the texel rows")
        assert (got[:, 3].view(torch.int32) == 1).all()
        # the view, and the four calls by hand
        view = ds.lightmap_view(baked, dT, texels, W, H, table, 0, 0, 32, 32, sample=0, seed=SEED, pass_of=pass_of)
        assert tuple(view.shape) == (32, 32, 4)
        rays = ds.camera_rays(0, 0, 32, 32, 0, SEED)
        hits = ds.closest_hits(rays.reshape(-1, 8))
        coords = ds.lightmap_coords(hits, table)
        by_hand = ds.lightmap_sample(baked, coords, dT, texels, W, H, pass_of=pass_of)
        assert_words_equal(view.reshape(-1, 4).cpu().numpy(), by_hand.cpu().numpy(), "lightmap_view against the four calls")
        # and against the restatement over the device's hits
        h = ds.hits_to_numpy(hits)
        want = sr.lightmap_sample(baked.cpu().numpy(), sr.lightmap_coords(h, table), T, lightmap_texels_to_numpy(texels), W, H, pass_of=pass_of.cpu().numpy())
        assert_words_equal(by_hand.cpu().numpy(), want, "the view against the restatement")
    v = view.cpu().numpy()
    count = v[..., 3].view(np.uint32).reshape(-1)
    floor = (h["status"] == 1) & (h["kind"] == sr.REF_TRIANGLE)
    assert (count[~floor] == 0).all() and (v.reshape(-1, 4)[~floor] == 0).all()  # a miss, and a pixel on the light
    assert (h["status"] == 0).any() and ((h["kind"] == sr.REF_QUAD) & (h["status"] == 1)).any()
    assert (count[floor] >= 1).all() and (count[floor] == 4).mean() > 0.9  # two passes of dilation cover every tap of the chart
    # brighter under the light than near the floor's corners: by where the pixel's hit lies on the floor
    r = rays.reshape(-1, 8).cpu().numpy().astype(np.float64)
    at = r[:, 0:3] + h["t"].astype(np.float64)[:, None] * r[:, 4:7]
    lum = v.reshape(-1, 4)[:, :3].sum(axis=1)
    under = floor & (np.abs(at[:, 0]) < 0.5) & (np.abs(at[:, 2]) < 0.5)
    corners = floor & (np.abs(at[:, 0]) > 1.4) & (np.abs(at[:, 2]) > 1.4)
    assert under.sum() > 10 and corners.sum() > 10
    assert lum[under].mean() > 2.0 * lum[corners].mean() > 0.0


# ---- 5. neutrality and media ------------------------------------------------------------------------------------------------------------------
def test_lookups_between_renders_change_no_frame_plane_or_statistic():
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    A = atlas(64, 64)

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
        dev = [torch.from_numpy(A.values[(3, 1)]).cuda(), texels_tensor(A.rows), torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels)]
        table = np.arange(40, dtype=np.uint32)

        def lookups():
            ds.lightmap_sample(*dev, 64, 64, pass_of=torch.from_numpy(A.pass_of[1]).cuda())
            ds.lightmap_sample(A.values[(27, None)], A.rows, A.uvs, A.texels, 64, 64, channels=27, nearest=True)
            hits = ds.closest_hits(ds.camera_rays(0, 0, 8, 8, 0, SEED).reshape(-1, 8))
            ds.lightmap_coords(hits, table)
            ds.lightmap_coords(ds.hits_to_numpy(hits), table)

        want = sequence(ds, lambda: None)
        assert sequence(ds, lookups) == want and want[3]["rays"] > 0


def test_a_scene_with_a_constant_medium_is_served():
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    A = atlas(64, 64)
    hits = np.zeros(5, dtype=sr.HIT_DTYPE)
    hits["status"], hits["kind"], hits["u"], hits["v"], hits["dfs_index"] = 1, [4, 4, 3, 4, 4], 0.25, 0.5, [0, 1, 2, 3, 9]
    hits["status"][1] = 0
    table = np.asarray([3, 4 | 1 << 30, 5, 6 | 2 << 30], dtype=np.uint32)
    with DeviceScene(sc) as ds:
        want = sr.lightmap_sample(A.values[(3, 1)], A.rows, A.uvs, A.texels, 64, 64, pass_of=A.pass_of[1])
        assert_words_equal(ds.lightmap_sample(A.values[(3, 1)], A.rows, A.uvs, A.texels, 64, 64, pass_of=A.pass_of[1]), want, "a lookup on a scene with a medium")
        assert_words_equal(ds.lightmap_coords(hits, table), sr.lightmap_coords(hits, table), "coords on a scene with a medium")
