"""Directional lightmaps on the device (sol_lightmap_sh / sol_lightmap_normals). The yardstick is tests/lightmap_sh_ref.py, the rule
restated in numpy float32: every answer is compared word for word, NaN for NaN, over every row - evaluation, evaluation with the clamp and
coefficient mode, bilinear and nearest, with and without the dilation's plane, strides of 112 and 128 bytes, on the host route and the device
route; coefficient mode also against the device's own lightmap_sample(channels=27). The rows are those of tests/test_gpu_lightmap_sample.py (a
mesh with a hole, overlapping charts, conservative texels, UVs of exactly 0 and 1 and of 1e30, one row of every invalid class between good rows),
so valid and invalid rows share octets and waves. Around it: row counts at the edges of an octet, a wave and a workgroup, guard words, a stream
of the caller's, the chart guard, the normals of a camera's hits, the chain from a bake to a normal-mapped view, neutrality, a scene with a medium.
Atlases are at most 130 x 67, rows a few hundred."""
import ctypes as C
import zlib

import numpy as np
import pytest

import lightmap_ref as lr
import lightmap_sample_ref as sr
import lightmap_sh_ref as shr
import parity_util as pu
from solstrale_amd import DeviceScene, RenderConfig, _abi, lightmap_texels_to_numpy, lightmap_triangle_table, scenes
from test_gpu_irradiance import _path_stats
from test_gpu_lightmap_sample import assert_words_equal, floor_under_a_light, lookup_mesh, lookup_rows, texels_tensor, two_charts
from test_lightmap_sh_abi import BAD_NORMALS

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F = np.float32
INF, NAN = F(np.inf), F(np.nan)
RC = RenderConfig(32, 32, 1)
ATLASES = [(1, 1), (5, 3), (300, 1), (64, 64), (130, 67)]
WORDS = (28, 32)  # strides of 112 and 128 bytes
MODES = [("evaluation", {}), ("clamped", dict(clamp=True)), ("coefficients", dict(coefficients=True))]
SCALE = 4 * np.pi / 64


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (the geometry of a lookup is the caller's: any handle serves)
        yield d


def row_normals(n, seed):
    """n rows (x, y, z, unused): unit and unnormalised normals, and one of every bad class between good ones."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    out = np.zeros((n, 4), dtype=F)
    out[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    out[n // 3:, :3] *= rng.choice([0.25, 3.0, 1e3, 1e-3], (n - n // 3, 1)).astype(F)
    out[:, 3] = rng.choice([F(0), F(7), NAN, INF], n)  # (not looked at)
    where = np.sort(rng.permutation(n)[:len(BAD_NORMALS)])
    for at, (_, bad) in zip(where, BAD_NORMALS):
        out[at, :3] = bad
    return out


class ShAtlas:
    """One atlas of the shared mesh with SolSh9 rows: ownership (conservative), and per stride and dilation the dilated values with words that are
    not finite put in afterwards - in words 0, 13 and 26 (three different lanes of an octet) and, which must change nothing, in word 27."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.vertices, self.uvs, rasterised = lookup_mesh()
        self.points, self.texels = lr.lightmap_points(self.vertices, rasterised, W, H, conservative=True)
        self.rows = lookup_rows(self.uvs, self.texels[self.texels["flags"] != 0] if (self.texels["flags"] != 0).any() else self.texels)
        self.normals = row_normals(len(self.rows), W + H)
        self.values, self.pass_of = {}, {}
        rng = np.random.default_rng(W * 1000 + H)
        for words in WORDS:
            raw = (rng.normal(size=(W * H, words)) * rng.choice([1e-3, 1.0, 1e4], (W * H, 1))).astype(F)
            raw[:, 27:] = np.arange(W * H * (words - 27), dtype=np.uint32).reshape(W * H, -1).view(F)
            for passes in (0, 1, 4):
                out, pass_of = lr.lightmap_dilate(raw, self.texels, W, H, passes=passes, channels=27)
                out = out.copy()
                for word in (0, 13, 26):
                    spoil = rng.random(W * H) < 0.03
                    out[spoil, word] = rng.choice([INF, -INF, NAN], int(spoil.sum()))
                out[rng.random(W * H) < 0.3, 27] = NAN  # the sample count's word: the tap stays live
                if words > 28:
                    out[:, 28:] = NAN  # beyond the row: never read
                self.values[(words, passes)], self.pass_of[passes] = out, pass_of
            self.values[(words, None)] = self.values[(words, 0)]


_atlases = {}


def atlas(W, H):
    if (W, H) not in _atlases:
        _atlases[(W, H)] = ShAtlas(W, H)
    return _atlases[(W, H)]


# ---- 1. the lookup and the evaluation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_every_mode_equals_the_restatement_word_for_word(ds, W, H):
    import torch
    A = atlas(W, H)
    d_uvs, d_texels, d_rows, d_normals = torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), texels_tensor(A.rows), torch.from_numpy(A.normals).cuda()
    seen, zeroed = set(), 0
    for words in WORDS:
        for passes in (None, 0, 1, 4):
            values = A.values[(words, passes)]
            pass_of = None if passes is None else A.pass_of[passes]
            d_values = torch.from_numpy(values).cuda()
            d_pass = None if pass_of is None else torch.from_numpy(pass_of).cuda()
            for nearest in (False, True):
                lookup = sr.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, channels=27, pass_of=pass_of, nearest=nearest)
                for mode, kw in MODES:
                    tag = (W, H, words, passes, "nearest" if nearest else "bilinear", mode)
                    nh, nd = (None, None) if mode == "coefficients" else (A.normals, d_normals)
                    want = shr.lightmap_sh(values, A.rows, nh, A.uvs, A.texels, W, H, scale=SCALE, pass_of=pass_of, nearest=nearest, **kw)
                    got = ds.lightmap_sh(values, A.rows, nh, A.uvs, A.texels, W, H, scale=SCALE, pass_of=pass_of, nearest=nearest, **kw)
                    assert got.shape == (len(A.rows), 28 if mode == "coefficients" else 4)
                    assert_words_equal(got, want, tag + ("host",))
                    got = ds.lightmap_sh(d_values, d_rows, nd, d_uvs, d_texels, W, H, scale=SCALE, pass_of=d_pass, nearest=nearest, **kw)
                    assert_words_equal(got.cpu().numpy(), want, tag + ("device",))
                    if mode == "coefficients":
                        assert_words_equal(want, lookup, tag + ("the restatement of the lookup",))
                        own = ds.lightmap_sample(d_values, d_rows, d_uvs, d_texels, W, H, channels=27, pass_of=d_pass, nearest=nearest)
                        assert_words_equal(got.cpu().numpy(), own.cpu().numpy(), tag + ("the device's own lightmap_sample",))
                        seen |= set(np.unique(want[:, 27].view(np.uint32)))
                    else:
                        count = lookup[:, 27].view(np.uint32)
                        assert (want[:, 3].view(np.uint32) <= count).all()
                        zeroed += int(((want[:, 3].view(np.uint32) == 0) & (count > 0)).sum())  # a bad normal on a row the lookup serves
                        if mode == "clamped":
                            assert not (want[:, :3] < 0).any() and not np.isnan(want[:, :3]).any()
    if (W, H) == (64, 64):  # the cases the rows and values are made for are there
        assert seen == {0, 1, 2, 3, 4} and zeroed > 0
        values, pass_of = A.values[(28, 4)], A.pass_of[4]
        want, taps = sr.lightmap_sample(values, A.rows, A.uvs, A.texels, W, H, channels=27, pass_of=pass_of, return_taps=True)
        clean = np.where(np.isnan(values[:, 27:28]), F(0), values[:, 27:28])
        again = sr.lightmap_sample(np.concatenate([values[:, :27], clean], axis=1), A.rows, A.uvs, A.texels, W, H, channels=27, pass_of=pass_of)
        assert np.isnan(values[:, 27]).any() and (want[:, 27].view(np.uint32) == again[:, 27].view(np.uint32)).all()  # NaN in word 27 kills no tap
        for word in (0, 13, 26):
            only = values.copy()
            only[:, [w for w in (0, 13, 26) if w != word]] = F(1)
            other = sr.lightmap_sample(only, A.rows, A.uvs, A.texels, W, H, channels=27, pass_of=pass_of)
            full = sr.lightmap_sample(np.where(np.isfinite(only), only, F(1)), A.rows, A.uvs, A.texels, W, H, channels=27, pass_of=pass_of)
            assert (other[:, 27].view(np.uint32) < full[:, 27].view(np.uint32)).any(), word  # a bad word 0, 13 or 26 alone takes taps out
        far = A.rows["triangle"] == len(A.uvs) - 3
        assert far.any() and (want[far].view(np.uint32) == 0).all()  # UVs of 1e30: no tap
        assert (A.texels["flags"] == 2).any() and (A.rows["flags"] == 2).any()


@pytest.mark.parametrize("mode, kw", MODES, ids=[m for m, _ in MODES])
def test_row_counts_around_an_octet_a_wave_and_a_workgroup_a_permutation_and_guard_words(ds, mode, kw):
    import torch
    W, H, G = 130, 67, 64
    A = atlas(W, H)
    values, pass_of = A.values[(28, 1)], A.pass_of[1]
    coefficients = mode == "coefficients"
    out_words = 28 if coefficients else 4
    want = shr.lightmap_sh(values, A.rows, None if coefficients else A.normals, A.uvs, A.texels, W, H, scale=SCALE, pass_of=pass_of, **kw)
    d_uvs, d_texels, d_values, d_pass = torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), torch.from_numpy(values).cuda(), torch.from_numpy(pass_of).cuda()
    d_normals = None if coefficients else torch.from_numpy(A.normals).cuda()
    for n in (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257):
        got = ds.lightmap_sh(d_values, texels_tensor(A.rows[:n]), None if coefficients else d_normals[:n].contiguous(), d_uvs, d_texels, W, H, scale=SCALE,
                             pass_of=d_pass, **kw)
        assert_words_equal(got.cpu().numpy(), want[:n], (mode, n, "device"))
    for n in (1, 9, 257):
        got = ds.lightmap_sh(values, A.rows[:n], None if coefficients else A.normals[:n], A.uvs, A.texels, W, H, scale=SCALE, pass_of=pass_of, **kw)
        assert_words_equal(got, want[:n], (mode, n, "host"))
    perm = np.random.default_rng(5).permutation(len(A.rows))
    got = ds.lightmap_sh(d_values, texels_tensor(A.rows[perm]), None if coefficients else torch.from_numpy(A.normals[perm]).cuda(), d_uvs, d_texels, W, H,
                         scale=SCALE, pass_of=d_pass, **kw)
    assert_words_equal(got.cpu().numpy(), want[perm], (mode, "permuted"))
    # guard words before and after out (the raw call)
    n = len(A.rows)
    out = torch.full((2 * G + n * out_words,), 7.0, dtype=torch.float32, device="cuda")
    d_rows = texels_tensor(A.rows)
    flags = _abi.SOL_LIGHTMAP_SH_COEFFICIENTS if coefficients else _abi.SOL_LIGHTMAP_SH_CLAMP if mode == "clamped" else 0
    cfg = _abi.SolLightmapShConfig(size=32, width=W, height=H, stride_bytes=112, flags=flags, chart_radius=float("inf"), scale=SCALE)
    args = (C.c_void_p(d_uvs.data_ptr()), len(A.uvs), C.c_void_p(d_texels.data_ptr()), C.c_void_p(d_pass.data_ptr()), C.c_void_p(d_values.data_ptr()), None, None,
            C.c_void_p(d_rows.data_ptr()), None if coefficients else C.c_void_p(d_normals.data_ptr()))
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_lightmap_sh_dev(ds.h, C.byref(cfg), *args, n, C.c_void_p(out[G:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n * out_words:] == 7).all()
    assert_words_equal(out[G:G + n * out_words].cpu().numpy().reshape(n, out_words), want, (mode, "guarded"))
    for short in (1, 9):  # the rows behind the last one of a call stay as they were
        out.fill_(7.0)
        torch.cuda.synchronize()
        ds._chk(ds.lib.sol_lightmap_sh_dev(ds.h, C.byref(cfg), *args, short, C.c_void_p(out[G:].data_ptr())))
        ds.sync()
        assert (out[:G] == 7).all() and (out[G + short * out_words:] == 7).all()
    # n == 0 writes nothing
    ds._chk(ds.lib.sol_lightmap_sh_dev(ds.h, C.byref(cfg), *args, 0, C.c_void_p(out.data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all()


def test_a_stream_of_the_callers(ds):
    import torch
    W, H = 64, 64
    A = atlas(W, H)
    values, pass_of = A.values[(32, 4)], A.pass_of[4]
    want = shr.lightmap_sh(values, A.rows, A.normals, A.uvs, A.texels, W, H, scale=SCALE, pass_of=pass_of)
    want_n = shr.lightmap_normals(A.rows, A.vertices)
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)
    try:
        got = ds.lightmap_sh(torch.from_numpy(values).cuda(), texels_tensor(A.rows), torch.from_numpy(A.normals).cuda(), torch.from_numpy(A.uvs).cuda(),
                             texels_tensor(A.texels), W, H, scale=SCALE, pass_of=torch.from_numpy(pass_of).cuda())
        assert_words_equal(got.cpu().numpy(), want, "device route on the caller's stream")
        assert_words_equal(ds.lightmap_sh(values, A.rows, A.normals, A.uvs, A.texels, W, H, scale=SCALE, pass_of=pass_of), want, "host route on the caller's stream")
        assert_words_equal(ds.lightmap_normals(texels_tensor(A.rows), torch.from_numpy(A.vertices).cuda()).cpu().numpy(), want_n, "normals, device route")
        assert_words_equal(ds.lightmap_normals(A.rows, A.vertices), want_n, "normals, host route")
    finally:
        ds.set_stream(0)


# ---- 2. the chart guard -----------------------------------------------------------------------------------------------------------------------
def test_the_chart_guard_keeps_a_neighbouring_chart_out(ds):
    import torch
    W, H = 16, 8
    uvs, vertices, points, texels, rgb = two_charts(W, H)
    values = np.zeros((W * H, 28), dtype=F)
    values[:, 0:3] = rgb[:, :3]  # the constant term alone: bright chart 1, dark chart 0
    rng = np.random.default_rng(31)
    n = 200
    rows = np.zeros(n, dtype=sr.TEXEL_DTYPE)  # points of the dark chart, the first half of them within a third of a texel of the shared border
    rows["triangle"], rows["flags"] = 3, 1
    s, t = rng.uniform(0, 1, n), rng.uniform(0.1, 0.9, n)
    s[:n // 2] = rng.uniform(0.0, 0.02, n // 2)
    rows["b1"], rows["b2"] = s.astype(F), ((1 - s) * t).astype(F)
    normals = np.zeros((n, 4), dtype=F)  # (every normal usable: this test is about the taps)
    d = rng.normal(size=(n, 3))
    normals[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    dev = [torch.from_numpy(a).cuda() for a in (values, uvs, vertices, points, normals)]
    d_rows, d_texels = texels_tensor(rows), texels_tensor(texels)
    answers = {}
    for radius in (None, 5.0, float("inf"), 1e-6):
        kw = {} if radius is None else dict(chart_radius=radius, vertices=vertices, points=points)
        dkw = {} if radius is None else dict(chart_radius=radius, vertices=dev[2], points=dev[3])
        ref_kw = {**kw, "chart_radius": np.inf if radius is None else radius}
        for mode, mkw in MODES:
            for nearest in (False, True):
                nh, nd = (None, None) if mode == "coefficients" else (normals, dev[4])
                want = shr.lightmap_sh(values, rows, nh, uvs, texels, W, H, nearest=nearest, **ref_kw, **mkw)
                assert_words_equal(ds.lightmap_sh(values, rows, nh, uvs, texels, W, H, nearest=nearest, **kw, **mkw), want, ("host", radius, mode, nearest))
                assert_words_equal(ds.lightmap_sh(dev[0], d_rows, nd, dev[1], d_texels, W, H, nearest=nearest, **dkw, **mkw).cpu().numpy(), want,
                                   ("device", radius, mode, nearest))
                if mode == "evaluation" and not nearest:
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
    d_pass = torch.from_numpy(pass_of).cuda()
    for radius in (5.0, 1e-6):
        want = shr.lightmap_sh(values, rows, normals, uvs, filled, W, H, pass_of=pass_of, chart_radius=radius, vertices=vertices, points=points)
        got = ds.lightmap_sh(dev[0], d_rows, dev[4], dev[1], texels_tensor(filled), W, H, pass_of=d_pass, chart_radius=radius, vertices=dev[2], points=dev[3])
        assert_words_equal(got.cpu().numpy(), want, ("dilated taps under the guard", radius))
        assert_words_equal(ds.lightmap_sh(values, rows, normals, uvs, filled, W, H, pass_of=pass_of, chart_radius=radius, vertices=vertices, points=points), want,
                           ("dilated taps under the guard, host", radius))
        assert (want[border, 0] > 0).all()
        if radius == 1e-6:  # only the dilated taps are left
            assert (want[~border & (s > 0.3)].view(np.uint32) == 0).all()
    # a vertex word that is not finite makes the row invalid under the guard only
    broken = vertices.copy()
    broken[3, 1, 2] = NAN  # (the rows' triangle)
    want = shr.lightmap_sh(values, rows, normals, uvs, texels, W, H, chart_radius=5.0, vertices=broken, points=points)
    assert (want.view(np.uint32) == 0).all()
    got = ds.lightmap_sh(dev[0], d_rows, dev[4], dev[1], d_texels, W, H, chart_radius=5.0, vertices=torch.from_numpy(broken).cuda(), points=dev[3])
    assert_words_equal(got.cpu().numpy(), want, "a vertex word that is not finite")


# ---- 3. normals -------------------------------------------------------------------------------------------------------------------------------
def floor_normals(V, seed=9):
    """per-vertex normals for the floor's triangles: near up, some without length, one with a word that is not finite"""
    rng = np.random.default_rng(seed)
    N = np.zeros_like(V)
    N[..., 1] = 1
    N += rng.normal(scale=0.2, size=N.shape).astype(F)
    N[::7] = 0
    N[3, 1, 0] = INF
    return N


def test_normals_of_a_cameras_hits_equal_the_restatement_on_both_routes():
    import torch
    sc, V, T = floor_under_a_light()
    table = lightmap_triangle_table(sc, 0, len(V))
    assert set(np.unique(table[table != sr.NONE] >> 30)) == {0, 1, 2}  # every rotation occurs among the jittered triangles
    N = floor_normals(V)
    with DeviceScene(sc) as ds:
        d_coords = ds.lightmap_coords(ds.closest_hits(ds.camera_rays(0, 0, 32, 32, 0, SEED).reshape(-1, 8)), table)
        coords = lightmap_texels_to_numpy(d_coords)
        assert (coords["flags"] != 0).sum() > 200 and (coords["flags"] == 0).any()
        dV, dN = torch.from_numpy(V).cuda(), torch.from_numpy(N).cuda()
        for name, nh, nd in (("geometric", None, None), ("vertex normals", N, dN)):
            want = shr.lightmap_normals(coords, V, nh)
            assert_words_equal(ds.lightmap_normals(d_coords, dV, nd).cpu().numpy(), want, (name, "device"))
            assert_words_equal(ds.lightmap_normals(coords, V, nh), want, (name, "host"))
            hit = coords["flags"] != 0
            assert (want[~hit].view(np.uint32) == 0).all() and (want[:, 3].view(np.uint32) == 0).all()
            served = hit & (coords["triangle"] != 3) if nh is not None else hit
            length = np.linalg.norm(want[served, :3].astype(np.float64), axis=1)
            assert (np.abs(length - 1) < 4e-7).all() and (want[served, 1] > 0.5).all()  # unit, and up: the floor faces the light
            if nh is not None:
                assert (want[hit & (coords["triangle"] == 3)].view(np.uint32) == 0).all()  # (its normal word that is not finite)
        # every invalid row, a guarded output and n == 0
        from test_lightmap_sample_abi import invalid_rows
        names, bad = invalid_rows(len(V), 0, None)
        third = np.zeros(1, dtype=sr.TEXEL_DTYPE)
        third[0] = (3, 0.25, 0.5, 1)  # the triangle whose vertex normals hold a word that is not finite
        rows = np.concatenate([coords[:3], bad[:-1], third, coords[3:6]])  # (the last class is about UVs: not this call's)
        want = shr.lightmap_normals(rows, V)
        assert (want[3:-4].view(np.uint32) == 0).all() and (want[-4, :3] != 0).any()
        with_normals = shr.lightmap_normals(rows, V, N)
        assert (with_normals[3:-3].view(np.uint32) == 0).all()
        assert_words_equal(ds.lightmap_normals(texels_tensor(rows), dV, dN).cpu().numpy(), with_normals, "invalid rows, vertex normals")
        out = torch.full((len(rows) + 16, 4), 7.0, dtype=torch.float32, device="cuda")
        d_rows = texels_tensor(rows)
        torch.cuda.synchronize()
        ds._chk(ds.lib.sol_lightmap_normals_dev(ds.h, C.c_void_p(d_rows.data_ptr()), len(rows), C.c_void_p(dV.data_ptr()), None, len(V), C.c_void_p(out[8:].data_ptr())))
        ds._chk(ds.lib.sol_lightmap_normals_dev(ds.h, C.c_void_p(d_rows.data_ptr()), 0, C.c_void_p(dV.data_ptr()), None, len(V), C.c_void_p(out.data_ptr())))
        ds.sync()
        assert (out[:8] == 7).all() and (out[8 + len(rows):] == 7).all()
        assert_words_equal(out[8:8 + len(rows)].cpu().numpy(), want, "guarded normals")


# ---- 4. the chain -----------------------------------------------------------------------------------------------------------------------------
def tilted_normals(rays, hits, toward):
    """[n, 4] normals tilted 45 degrees from straight up toward (or away from) the light's side: the horizontal direction from the pixel's hit
    to the light's centre above the origin."""
    r = rays.reshape(-1, 8).astype(np.float64)
    with np.errstate(all="ignore"):
        at = r[:, 0:3] + hits["t"].astype(np.float64)[:, None] * r[:, 4:7]
    with np.errstate(all="ignore"):  # (a miss has no hit point: its normal is NaN, its row invalid anyway)
        side = -at[:, [0, 2]]
        dist = np.linalg.norm(side, axis=1)
        side = side / np.maximum(dist, 1e-9)[:, None] * (1.0 if toward else -1.0)
    n = np.zeros((len(r), 4), dtype=F)
    n[:, 0], n[:, 1], n[:, 2] = side[:, 0] * np.sqrt(0.5), np.sqrt(0.5), side[:, 1] * np.sqrt(0.5)
    return n, dist


def bake_and_view(ds, sc, V, T, samples=64, W=32, H=32):
    """the chain on the floor under a light; returns what the test and tests/tools/lightmap_sh_bench.py look at"""
    import torch
    table = lightmap_triangle_table(sc, 0, len(V))
    dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    points, texels = ds.lightmap_points(dV, dT, W, H)
    rows = ds.irradiance_sh(points, samples=samples, seed=SEED, mode="sphere")
    baked, pass_of = ds.lightmap_dilate(rows, texels, W, H, passes=2, channels=27, return_pass_of=True)
    scale = 4 * np.pi / samples
    rays = ds.camera_rays(0, 0, 32, 32, 0, SEED)
    hits = ds.closest_hits(rays.reshape(-1, 8))
    h = ds.hits_to_numpy(hits)
    floor = (h["status"] == 1) & (h["kind"] == sr.REF_TRIANGLE)
    views = {}
    for name, toward in (("toward", True), ("away", False)):
        n, dist = tilted_normals(rays.cpu().numpy(), h, toward)
        views[name] = ds.lightmap_view_sh(baked, dT, texels, W, H, table, dV, 0, 0, 32, 32, scale, sample=0, seed=SEED, pass_of=pass_of, clamp=True,
                                          perturb=torch.from_numpy(n.reshape(32, 32, 4)).cuda()).cpu().numpy()
    lit = floor & (dist > 0.5) & (dist < 2.0)  # where there is a side to tilt to, around the light's footprint
    lum = {k: float(v.reshape(-1, 4)[lit, :3].sum(axis=1).mean()) for k, v in views.items()}
    return dict(table=table, dV=dV, dT=dT, texels=texels, baked=baked, pass_of=pass_of, scale=scale, rays=rays, hits=hits, h=h, floor=floor, lit=lit, lum=lum,
                views=views)


def test_bake_then_view_is_the_five_calls_and_a_normal_map_turns_the_light():
    import torch
    W = H = 32
    sc, V, T = floor_under_a_light()
    with DeviceScene(sc) as ds:
        b = bake_and_view(ds, sc, V, T)
        baked, texels, pass_of, dT, dV, table, scale = b["baked"], b["texels"], b["pass_of"], b["dT"], b["dV"], b["table"], b["scale"]
        assert tuple(baked.shape) == (W * H, 28)
        # the view with the surface's own normals, and the five calls by hand
        view = ds.lightmap_view_sh(baked, dT, texels, W, H, table, dV, 0, 0, 32, 32, scale, sample=0, seed=SEED, pass_of=pass_of)
        assert tuple(view.shape) == (32, 32, 4)
        coords = ds.lightmap_coords(b["hits"], table)
        normals = ds.lightmap_normals(coords, dV)
        by_hand = ds.lightmap_sh(baked, coords, normals, dT, texels, W, H, scale=scale, pass_of=pass_of)
        assert_words_equal(view.reshape(-1, 4).cpu().numpy(), by_hand.cpu().numpy(), "lightmap_view_sh against the five calls")
        # and against the restatement over the device's hits
        h = b["h"]
        rows = sr.lightmap_coords(h, table)
        want_n = shr.lightmap_normals(rows, V)
        assert_words_equal(normals.cpu().numpy(), want_n, "the view's normals against the restatement")
        host = dict(values=baked.cpu().numpy(), texels=lightmap_texels_to_numpy(texels), pass_of=pass_of.cpu().numpy())
        want = shr.lightmap_sh(host["values"], rows, want_n, T, host["texels"], W, H, scale=scale, pass_of=host["pass_of"])
        assert_words_equal(by_hand.cpu().numpy(), want, "the view against the restatement")
        for name, toward in (("toward", True), ("away", False)):  # the normal-mapped views too
            n, _ = tilted_normals(b["rays"].cpu().numpy(), h, toward)
            want_t = shr.lightmap_sh(host["values"], rows, n, T, host["texels"], W, H, scale=scale, pass_of=host["pass_of"], clamp=True)
            assert_words_equal(b["views"][name].reshape(-1, 4), want_t, ("perturbed", name))
        coeff = ds.lightmap_view_sh(baked, dT, texels, W, H, table, dV, 0, 0, 32, 32, scale, sample=0, seed=SEED, pass_of=pass_of, coefficients=True)
        assert_words_equal(coeff.reshape(-1, 28).cpu().numpy(), ds.lightmap_view(baked, dT, texels, W, H, table, 0, 0, 32, 32, sample=0, seed=SEED, pass_of=pass_of,
                                                                                   channels=27).reshape(-1, 28).cpu().numpy(), "the coefficient view")
    v = view.cpu().numpy().reshape(-1, 4)
    count, floor = v[:, 3].view(np.uint32), b["floor"]
    assert (count[~floor] == 0).all() and (v[~floor] == 0).all()  # a miss, and a pixel on the light
    assert (h["status"] == 0).any() and ((h["kind"] == sr.REF_QUAD) & (h["status"] == 1)).any()
    assert (count[floor] >= 1).all() and (count[floor] == 4).mean() > 0.9
    # the floor faces the light: its own normals see it, and a normal tilted toward the light's side sees more of it than one tilted away
    assert v[floor, :3].sum(axis=1).mean() > 0
    lum = b["lum"]
    print(f"lightmap_view_sh: {int(b['lit'].sum())} lit pixels, mean toward {lum['toward']:.4f}, away {lum['away']:.4f}, ratio {lum['toward'] / max(lum['away'], 1e-30):.3f}")
    assert b["lit"].sum() > 100
    assert lum["toward"] > lum["away"]


# ---- 5. neutrality and media ------------------------------------------------------------------------------------------------------------------
def test_sh_lookups_between_renders_change_no_frame_plane_or_statistic():
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
        dev = [torch.from_numpy(A.values[(28, 1)]).cuda(), texels_tensor(A.rows), torch.from_numpy(A.normals).cuda(), torch.from_numpy(A.uvs).cuda(),
               texels_tensor(A.texels)]
        d_vertices = torch.from_numpy(A.vertices).cuda()

        def lookups():
            ds.lightmap_sh(*dev, 64, 64, scale=SCALE, pass_of=torch.from_numpy(A.pass_of[1]).cuda())
            ds.lightmap_sh(A.values[(32, None)], A.rows, None, A.uvs, A.texels, 64, 64, nearest=True, coefficients=True)
            ds.lightmap_sh(A.values[(28, None)], A.rows, A.normals, A.uvs, A.texels, 64, 64, clamp=True)
            ds.lightmap_normals(dev[1], d_vertices)
            ds.lightmap_normals(A.rows, A.vertices)

        want = sequence(ds, lambda: None)
        assert sequence(ds, lookups) == want and want[3]["rays"] > 0


def test_a_scene_with_a_constant_medium_is_served():
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    A = atlas(64, 64)
    with DeviceScene(sc) as ds:
        want = shr.lightmap_sh(A.values[(28, 1)], A.rows, A.normals, A.uvs, A.texels, 64, 64, scale=SCALE, pass_of=A.pass_of[1])
        assert_words_equal(ds.lightmap_sh(A.values[(28, 1)], A.rows, A.normals, A.uvs, A.texels, 64, 64, scale=SCALE, pass_of=A.pass_of[1]), want,
                           "an SH lookup on a scene with a medium")
        assert_words_equal(ds.lightmap_normals(A.rows, A.vertices), shr.lightmap_normals(A.rows, A.vertices), "normals on a scene with a medium")
