"""Lightmap mip chains on the device (sol_lightmap_mips / sol_lightmap_sample_lod / sol_lightmap_lod). The yardstick is
tests/lightmap_mips_ref.py, the rule restated in numpy float32: every word of a chain, of its cover plane, of a lookup and of a level of detail is
compared, NaN for NaN, on the host route and the device route. Around it: the level-only path in a child process, guard words, the two identities
against the device's own lightmap_sample, the chart guard, the view, neutrality and a scene with a medium. The mesh, the atlases and the floor scene
are those of tests/test_gpu_lightmap_sample.py. Atlases are at most 257 x 129, rows a few hundred."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import lightmap_mips_ref as mr
import lightmap_sample_ref as sr
import parity_util as pu
from solstrale_amd import DeviceScene, RenderConfig, lightmap_mip_layout, lightmap_texels_to_numpy, lightmap_triangle_table, pixel_spread, scenes
from test_gpu_irradiance import _path_stats
from test_gpu_lightmap_sample import CHANNELS, atlas, floor_under_a_light, texels_tensor, two_charts
from test_lightmap_mips_abi import invalid_lod_rows

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F = np.float32
INF, NAN = F(np.inf), F(np.nan)
RC = RenderConfig(32, 32, 1)
# odd sizes at several levels; 64 x 64 is exactly the tail kernel's largest input, 65 x 64 one texel larger: the hand-over from the level kernel
ATLASES = [(1, 1), (2, 2), (3, 3), (5, 3), (300, 1), (64, 64), (65, 64), (130, 67), (257, 129)]


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (the geometry of a chain is the caller's: any handle serves)
        yield d


def check(got, want, what):
    """Every word (or byte) of `got` is that of `want`, NaN for NaN; arrays of any shape, also empty ones."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.size == 0:
        return
    word = np.uint32 if got.dtype.itemsize == 4 else np.uint8
    g, w = got.view(word).reshape(got.shape[0], -1), want.view(word).reshape(want.shape[0], -1)
    if (g != w).any():
        bad = np.nonzero((g != w).any(axis=1))[0]
        raise AssertionError((what, len(bad), len(g), bad[:5], got[bad[:3]], want[bad[:3]]))


def spoiled(A, channels, passes):
    """The atlas's values (they carry non-finite words already) with one more: the only covered source of some level-1 texel, where there is one -
    its three neighbours are uncovered, so the destination must come out uncovered."""
    values = A.values[(channels, passes)].copy()
    W, H = A.W, A.H
    covered = (A.pass_of[passes].reshape(-1) != 255) if passes is not None else (A.texels["triangle"] != sr.NONE)
    c = np.zeros((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), dtype=bool)
    c[:H, :W] = covered.reshape(H, W)
    alone = (c[0::2, 0::2].astype(int) + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) == 1
    found = False
    if alone.any():
        j, i = np.argwhere(alone)[len(np.argwhere(alone)) // 2]
        for dj in (0, 1):
            for di in (0, 1):
                if c[2 * j + dj, 2 * i + di]:
                    values[(2 * j + dj) * W + 2 * i + di, channels - 1] = NAN
                    found = True
    return values, found


_chains = {}


def chain(A, channels, passes):
    """(values, pass_of, the restatement's full chain and cover) of one atlas, channel layout and dilation - computed once"""
    key = (A.W, A.H, channels, passes)
    if key not in _chains:
        values, found = spoiled(A, channels, passes)
        pass_of = None if passes is None else A.pass_of[passes]
        mips, cover = mr.lightmap_mips(values, A.texels, A.W, A.H, channels=channels, pass_of=pass_of)
        if found and len(cover):
            assert (cover[:((A.W + 1) // 2) * ((A.H + 1) // 2)] == 255).any()
        _chains[key] = (values, pass_of, mips, cover)
    return _chains[key]


# ---- 1. the chain -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_the_chain_equals_the_restatement_word_for_word(ds, W, H):
    import torch
    A = atlas(W, H)
    d_texels = texels_tensor(A.texels)
    full = lightmap_mip_layout(W, H)
    lone = False
    for channels, words in CHANNELS:
        for passes in (None, 0, 1, 4):
            values, pass_of, want_mips, want_cover = chain(A, channels, passes)
            lone |= spoiled(A, channels, passes)[1]
            assert want_mips.shape == (full["rows"], words) and set(np.unique(want_cover)) <= {0, 255}
            d_values = torch.from_numpy(values).cuda()
            d_pass = None if pass_of is None else torch.from_numpy(pass_of).cuda()
            for levels in sorted({1, min(2, full["levels"]), None}, key=lambda x: x or 99):
                rows = lightmap_mip_layout(W, H, levels)["rows"]  # (a shorter chain is the full one's beginning)
                tag = (W, H, channels, passes, levels)
                mips, cover = ds.lightmap_mips(d_values, d_texels, W, H, channels=channels, pass_of=d_pass, levels=levels)
                assert tuple(mips.shape) == (rows, words) and tuple(cover.shape) == (rows,)
                check(mips.cpu().numpy(), want_mips[:rows], tag + ("device", "mips"))
                check(cover.cpu().numpy(), want_cover[:rows], tag + ("device", "cover"))
                if passes in (None, 1):
                    mips, cover = ds.lightmap_mips(values, A.texels, W, H, channels=channels, pass_of=pass_of, levels=levels)
                    check(mips, want_mips[:rows], tag + ("host", "mips"))
                    check(cover, want_cover[:rows], tag + ("host", "cover"))
            check(d_values.cpu().numpy(), values, "the input is not written")
            if full["levels"] > 1 and (want_cover == 0).any():  # covered rows are finite, uncovered rows zero, the words behind the channels copied
                assert np.isfinite(want_mips[want_cover == 0][:, :channels]).all() and (want_mips[want_cover == 255].view(np.uint32) == 0).all()
    if (W, H) == (64, 64):
        assert lone  # a covered texel whose three neighbours are not, made non-finite
        assert full["levels"] == 7 and (chain(A, 3, 4)[3] == 255).any() and chain(A, 3, 4)[3][-1] == 0


CHILD = """
import sys
import numpy as np
from solstrale_amd import LIGHTMAP_TEXEL_DTYPE, DeviceScene, RenderConfig, scenes
import torch
a = np.load(sys.argv[1])
out = {}
with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
    for k in range(int(a["n"])):
        v, t, p = a[f"values{k}"], a[f"texels{k}"], a[f"pass{k}"]
        W, H, ch = (int(x) for x in a[f"args{k}"])
        out[f"hm{k}"], out[f"hc{k}"] = ds.lightmap_mips(v, t.view(LIGHTMAP_TEXEL_DTYPE).reshape(-1), W, H, channels=ch, pass_of=p)
        m, c = ds.lightmap_mips(torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32).reshape(-1, 4)).cuda(), W, H, channels=ch, pass_of=torch.from_numpy(p).cuda())
        out[f"dm{k}"], out[f"dc{k}"] = m.cpu().numpy(), c.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def test_the_level_only_path_answers_the_default_paths_bytes(ds, tmp_path):
    """SOL_LIGHTMAP_MIPS=levels in a fresh child process: a launch per level down to 1 x 1. The default path (this process) hands the small levels to
    the tail kernel for rows of at most 12 words; both must answer the restatement's bytes."""
    cases = [(64, 64, 3, 4), (65, 64, 3, 4), (130, 67, 1, 1), (130, 67, 2, 5), (257, 129, 3, 4), (5, 3, 3, 4), (130, 67, 27, 28)]
    arrays = {"n": len(cases)}
    for k, (W, H, ch, words) in enumerate(cases):
        values, pass_of, _, _ = chain(atlas(W, H), ch, 1)
        arrays.update({f"values{k}": values, f"texels{k}": atlas(W, H).texels.view(np.uint32).reshape(-1, 4), f"pass{k}": pass_of,
                       f"args{k}": np.asarray([W, H, ch])})
    np.savez(tmp_path / "in.npz", **arrays)
    env = {**os.environ, "SOL_LIGHTMAP_MIPS": "levels", "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    for k, (W, H, ch, words) in enumerate(cases):
        values, pass_of, want_mips, want_cover = chain(atlas(W, H), ch, 1)
        mips, cover = ds.lightmap_mips(values, atlas(W, H).texels, W, H, channels=ch, pass_of=pass_of)  # the default path, here
        for route in ("h", "d"):
            assert got[f"{route}m{k}"].tobytes() == mips.tobytes() == want_mips.tobytes(), (cases[k], route)
            assert got[f"{route}c{k}"].tobytes() == cover.tobytes() == want_cover.tobytes(), (cases[k], route)


@pytest.mark.parametrize("W, H, channels, words", [(130, 67, 3, 4), (65, 64, 2, 5), (64, 64, 27, 28)], ids=["vector_rows", "word_rows", "sh9_rows"])
def test_guard_words_behind_both_buffers(ds, W, H, channels, words):
    import torch
    G = 64
    A = atlas(W, H)
    values, pass_of, want_mips, want_cover = chain(A, channels, 1)
    rows = len(want_cover)
    d_values, d_texels, d_pass = torch.from_numpy(values).cuda(), texels_tensor(A.texels), torch.from_numpy(pass_of).cuda()
    mips = torch.full((2 * G + rows * words,), 7.0, dtype=torch.float32, device="cuda")
    cover = torch.full((2 * G + rows,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_lightmap_mips_dev(ds.h, C.c_void_p(d_texels.data_ptr()), C.c_void_p(d_pass.data_ptr()), W, H, C.c_void_p(d_values.data_ptr()), channels,
                                         4 * words, 0, C.c_void_p(mips[G:].data_ptr()), C.c_void_p(cover[G:].data_ptr())))
    ds.sync()
    assert (mips[:G] == 7).all() and (mips[G + rows * words:] == 7).all() and (cover[:G] == 7).all() and (cover[G + rows:] == 7).all()
    check(mips[G:G + rows * words].cpu().numpy().reshape(rows, words), want_mips, "guarded mips")
    check(cover[G:G + rows].cpu().numpy(), want_cover, "guarded cover")
    # one level writes nothing
    ds._chk(ds.lib.sol_lightmap_mips_dev(ds.h, C.c_void_p(d_texels.data_ptr()), None, W, H, C.c_void_p(d_values.data_ptr()), channels, 4 * words, 1,
                                         C.c_void_p(mips.data_ptr()), C.c_void_p(cover.data_ptr())))
    ds.sync()
    assert (mips[:G] == 7).all() and (cover[:G] == 7).all()


# ---- 2. the lookup ----------------------------------------------------------------------------------------------------------------------------
def lods_for(n, levels, seed=3):
    pool = np.asarray([-1.0, -0.0, 0.0, 0.5, 1.0, 1.25, levels - 1, levels - 0.5, levels + 2, NAN, INF, -INF, 2.0, 2.75, 0.001], dtype=F)
    rng = np.random.default_rng(seed)
    out = pool[np.arange(n) % len(pool)]
    extra = rng.random(n) < 0.3
    out[extra] = rng.uniform(0, levels, int(extra.sum())).astype(F)
    return out[rng.permutation(n)]


LOOKUPS = [(1, 1, 3, 4), (5, 3, 3, 4), (300, 1, 3, 4), (64, 64, 3, 4), (130, 67, 3, 4), (130, 67, 1, 1), (130, 67, 27, 28), (130, 67, 2, 5)]


@pytest.mark.parametrize("W, H, channels, words", LOOKUPS, ids=[f"{w}x{h}x{c}" for w, h, c, _ in LOOKUPS])
def test_the_trilinear_lookup_equals_the_restatement_word_for_word(ds, W, H, channels, words):
    import torch
    A = atlas(W, H)
    d_uvs, d_texels, d_rows = torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), texels_tensor(A.rows)
    full = lightmap_mip_layout(W, H)["levels"]
    seen = set()
    for passes in (None, 4):
        values, pass_of, mips, cover = chain(A, channels, passes)
        d_values, d_mips, d_cover = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (values, mips, cover))
        d_pass = None if pass_of is None else torch.from_numpy(pass_of).cuda()
        for levels in sorted({1, min(2, full), full}):
            rows = lightmap_mip_layout(W, H, levels)["rows"]
            lods = lods_for(len(A.rows), levels)
            kw = dict(channels=channels, levels=levels)
            want = mr.lightmap_sample_lod(values, mips[:rows], cover[:rows], lods, A.rows, A.uvs, A.texels, W, H, pass_of=pass_of, **kw)
            tag = (W, H, channels, passes, levels)
            got = ds.lightmap_sample_lod(d_values, d_mips[:rows], d_cover[:rows], torch.from_numpy(lods).cuda(), d_rows, d_uvs, d_texels, W, H, pass_of=d_pass, **kw)
            assert tuple(got.shape) == (len(A.rows), channels + 1)
            check(got.cpu().numpy(), want, tag + ("device",))
            check(ds.lightmap_sample_lod(values, mips[:rows], cover[:rows], lods, A.rows, A.uvs, A.texels, W, H, pass_of=pass_of, **kw), want,
                               tag + ("host",))
            assert np.isfinite(want[:, :channels]).all()
            seen |= set(np.unique(want[:, channels].view(np.uint32)))
            if levels == full and channels == 3:
                for n in (1, 63, 64, 65):
                    got = ds.lightmap_sample_lod(d_values, d_mips, d_cover, torch.from_numpy(lods[:n]).cuda(), texels_tensor(A.rows[:n]), d_uvs, d_texels, W, H,
                                                 pass_of=d_pass, **kw)
                    check(got.cpu().numpy(), want[:n], tag + (n,))
    if (W, H) in ((64, 64), (130, 67)):
        assert seen >= {0, 1, 2, 3, 4, 5, 6, 7, 8}


@pytest.mark.parametrize("W, H", [(64, 64), (130, 67)], ids=["64x64", "130x67"])
def test_the_two_identities_against_the_devices_own_lookup(ds, W, H):
    import torch
    A = atlas(W, H)
    d_uvs, d_texels, d_rows = torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels), texels_tensor(A.rows)
    n = len(A.rows)
    lay = lightmap_mip_layout(W, H)
    for channels, passes in ((3, 1), (27, None)):
        values, pass_of, _, _ = chain(A, channels, passes)
        d_values = torch.from_numpy(values).cuda()
        d_pass = None if pass_of is None else torch.from_numpy(pass_of).cuda()
        d_mips, d_cover = ds.lightmap_mips(d_values, d_texels, W, H, channels=channels, pass_of=d_pass)
        plain = ds.lightmap_sample(d_values, d_rows, d_uvs, d_texels, W, H, channels=channels, pass_of=d_pass).cpu().numpy()
        # 1. lod <= 0, or one level: sol_lightmap_sample's words
        for lod in (-2.5, -0.0, 0.0, NAN, -INF):
            got = ds.lightmap_sample_lod(d_values, d_mips, d_cover, torch.full((n,), float(lod), device="cuda"), d_rows, d_uvs, d_texels, W, H, channels=channels,
                                         pass_of=d_pass)
            check(got.cpu().numpy(), plain, ("lod <= 0", channels, lod))
        got = ds.lightmap_sample_lod(d_values, None, None, torch.full((n,), 3.5, device="cuda"), d_rows, d_uvs, d_texels, W, H, channels=channels, pass_of=d_pass,
                                     levels=1)
        check(got.cpu().numpy(), plain, ("one level", channels))
        # 2. powers of two, an integral lod: sol_lightmap_sample over the level with its cover as pass_of
        if (W, H) == (64, 64):
            for l in range(1, lay["levels"]):
                lo, hi, wl, hl = lay["offsets"][l], lay["offsets"][l] + lay["widths"][l] * lay["heights"][l], lay["widths"][l], lay["heights"][l]
                none = torch.full((hi - lo, 4), -1, dtype=torch.int32, device="cuda")
                level = ds.lightmap_sample(d_mips[lo:hi].contiguous(), d_rows, d_uvs, none, wl, hl, channels=channels,
                                           pass_of=d_cover[lo:hi].contiguous().reshape(hl, wl)).cpu().numpy()
                for lod in ((float(l),) if l < lay["levels"] - 1 else (float(l), l + 0.5, 99.0, float("inf"))):
                    got = ds.lightmap_sample_lod(d_values, d_mips, d_cover, torch.full((n,), lod, device="cuda"), d_rows, d_uvs, d_texels, W, H, channels=channels,
                                                 pass_of=d_pass)
                    check(got.cpu().numpy(), level, ("level", channels, l, lod))


def test_the_chart_guard_acts_at_level_zero_only(ds):
    import torch
    W, H = 16, 8
    uvs, vertices, points, texels, values = two_charts(W, H)
    rng = np.random.default_rng(31)
    n = 200
    rows = np.zeros(n, dtype=sr.TEXEL_DTYPE)  # points of the dark chart, half of them within a third of a texel of the shared border
    rows["triangle"], rows["flags"] = 3, 1
    s, t = rng.uniform(0, 1, n), rng.uniform(0.1, 0.9, n)
    s[:n // 2] = rng.uniform(0.0, 0.02, n // 2)
    rows["b1"], rows["b2"] = s.astype(F), ((1 - s) * t).astype(F)
    mips, cover = mr.lightmap_mips(values, texels, W, H)
    dev = [torch.from_numpy(a).cuda() for a in (values, mips, cover, uvs, vertices, points)]
    d_rows, d_texels = texels_tensor(rows), texels_tensor(texels)
    border = np.arange(n) < n // 2
    for lod in (0.0, 0.5, 1.0):
        lods = np.full(n, lod, dtype=F)
        answers = {}
        for radius in (None, 5.0):
            kw = {} if radius is None else dict(chart_radius=radius, vertices=vertices, points=points)
            dkw = {} if radius is None else dict(chart_radius=radius, vertices=dev[4], points=dev[5])
            want = mr.lightmap_sample_lod(values, mips, cover, lods, rows, uvs, texels, W, H, **{**kw, "chart_radius": np.inf if radius is None else radius})
            check(ds.lightmap_sample_lod(values, mips, cover, lods, rows, uvs, texels, W, H, **kw), want, ("host", lod, radius))
            got = ds.lightmap_sample_lod(dev[0], dev[1], dev[2], torch.from_numpy(lods).cuda(), d_rows, dev[3], d_texels, W, H, **dkw)
            check(got.cpu().numpy(), want, ("device", lod, radius))
            answers[radius] = want
        if lod == 0.0:  # the guard keeps the bright chart out, exactly as sol_lightmap_sample does
            assert (answers[None][border, 0] > 0).all() and (answers[5.0][:, :3] == 0).all()
            check(answers[5.0], ds.lightmap_sample(values, rows, uvs, texels, W, H, chart_radius=5.0, vertices=vertices, points=points), "level 0")
        if lod == 1.0:  # a coarser texel has no point row: the guard changes nothing there, and the charts mix (no chart ids)
            check(answers[5.0], answers[None], "level 1")
            assert (answers[5.0][border, 0] > 0).all()
    broken = vertices.copy()
    broken[3, 1, 2] = NAN  # a vertex word that is not finite makes the row invalid under the guard, at every lod
    got = ds.lightmap_sample_lod(values, mips, cover, np.full(n, 1.0, dtype=F), rows, uvs, texels, W, H, chart_radius=5.0, vertices=broken, points=points)
    assert (got.view(np.uint32) == 0).all()


# ---- 3. the level of detail -------------------------------------------------------------------------------------------------------------------
def test_the_lod_of_camera_hits_equals_the_restatement():
    import torch
    sc, V, T = floor_under_a_light()
    table = lightmap_triangle_table(sc, 0, len(V))
    assert set(np.unique(table[table != sr.NONE] >> 30)) == {0, 1, 2}  # every rotation occurs among the jittered triangles
    W = H = 256
    with DeviceScene(sc) as ds:
        rays = ds.camera_rays(0, 0, 32, 32, 0, SEED).reshape(-1, 8)
        d_hits = ds.closest_hits(rays)
        d_coords = ds.lightmap_coords(d_hits, table)
        hits, coords, r = ds.hits_to_numpy(d_hits), lightmap_texels_to_numpy(d_coords), rays.cpu().numpy()
        floor = coords["flags"] != 0
        assert floor.sum() > 200 and (~floor).sum() > 20
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        spread = pixel_spread(40.0, 32)
        for s, bias in ((spread, 0.0), (spread, -1.5), (spread / 64, 0.25), (spread * 8, 2.0)):
            want = mr.lightmap_lod(r, hits, coords, V, T, W, H, s, bias)
            got = ds.lightmap_lod(rays, d_hits, d_coords, dV, dT, W, H, s, bias)
            assert got.dtype == torch.float32 and tuple(got.shape) == (1024,)
            check(got.cpu().numpy(), want, ("device", s, bias))
            check(ds.lightmap_lod(r, hits, coords, V, T, W, H, s, bias), want, ("host", s, bias))
            assert (want[~floor] == 0).all() and np.isfinite(want).all()
        want = mr.lightmap_lod(r, hits, coords, V, T, W, H, spread)
        # the meaning of the number: half the base-2 logarithm of q, in float64 from the same hits - plog2 lies below log2 by at most 0.0861 (the
        # chord of log2 over a binade), its half by 0.0431; the fp32 roundings of q's dozen operations move log2(q) by some 1e-5
        r64, P = r.astype(np.float64)[floor], V.astype(np.float64)[coords["triangle"][floor]]
        U = T.astype(np.float64)[coords["triangle"][floor]] * W
        N = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        nn, D = (N * N).sum(axis=1), r64[:, 4:7]
        c2 = np.maximum((D * N).sum(axis=1) ** 2 / ((D * D).sum(axis=1) * nn), 1 / 64)
        a = np.abs((U[:, 1, 0] - U[:, 0, 0]) * (U[:, 2, 1] - U[:, 0, 1]) - (U[:, 1, 1] - U[:, 0, 1]) * (U[:, 2, 0] - U[:, 0, 0]))
        q = (spread * hits["t"][floor].astype(np.float64)) ** 2 * (a / np.sqrt(nn)) / c2
        ideal = np.where(q > 1, 0.5 * np.log2(np.maximum(q, 1)), 0.0)
        print(f"lod: {int(floor.sum())} floor hits, lambda {want[floor].min():.3f} .. {want[floor].max():.3f}, "
              f"largest shortfall against log2 {np.max(ideal - want[floor]):.4f}")
        assert (want[floor] <= ideal + 1e-4).all() and (ideal - want[floor] <= 0.0431 + 1e-4).all() and (want[floor] > 0).mean() > 0.9
        for n in (1, 63, 64, 65):
            got = ds.lightmap_lod(rays[:n].contiguous(), d_hits[:n].contiguous(), d_coords[:n].contiguous(), dV, dT, W, H, spread)
            check(got.cpu().numpy(), want[:n], n)
        # a row of every invalid class, between good rows
        cases = invalid_lod_rows()
        good = np.nonzero(floor)[0][:len(cases) + 1]
        for k, (name, (br, bh, bc, bv, bt)) in enumerate(cases.items()):
            rr, hh, cc = r[good].copy(), hits[good].copy(), coords[good].copy()
            VV, TT = np.concatenate([V, bv]), np.concatenate([T, bt])
            bc = bc.copy()
            if bc["triangle"][0] == 0:
                bc["triangle"] = len(V)  # (the case's own triangle, behind the mesh)
            elif bc["triangle"][0] == 1:
                bc["triangle"] = len(VV)  # (beyond the mesh)
            rr[k + 1:k + 2], hh[k + 1:k + 2], cc[k + 1:k + 2] = br, bh.astype(hh.dtype), bc
            want = mr.lightmap_lod(rr, hh, cc, VV, TT, W, H, spread, 1.0)
            assert want[k + 1] == 0 and (np.delete(want, k + 1) > 1).all(), name
            check(ds.lightmap_lod(rr, hh, cc, VV, TT, W, H, spread, 1.0), want, (name, "host"))
            got = ds.lightmap_lod(torch.from_numpy(rr).cuda(), torch.from_numpy(hh.view(np.int32).reshape(-1, 8)).cuda(), texels_tensor(cc),
                                  torch.from_numpy(VV).cuda(), torch.from_numpy(TT).cuda(), W, H, spread, 1.0)
            check(got.cpu().numpy(), want, (name, "device"))


# ---- 4. the view ------------------------------------------------------------------------------------------------------------------------------
def test_the_view_is_the_five_calls_and_a_far_checkerboard_flickers_less():
    import torch
    W = H = 2048  # (at 256 the floor's lods are 0.1 .. 1.1: three levels finer and every pixel of the floor covers more than four texels)
    sc, V, T = floor_under_a_light()
    table = lightmap_triangle_table(sc, 0, len(V))
    spread = pixel_spread(40.0, 32)
    with DeviceScene(sc) as ds:
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        points, texels = ds.lightmap_points(dV, dT, W, H)
        ij = torch.arange(W * H, device="cuda")
        board = (((ij % W) + (ij // W)) % 2).to(torch.float32)  # a one-texel checkerboard
        values = torch.stack([board, board, board, torch.ones_like(board)], dim=1).contiguous()
        baked, pass_of = ds.lightmap_dilate(values, texels, W, H, passes=2, return_pass_of=True)
        mips, cover = ds.lightmap_mips(baked, texels, W, H, pass_of=pass_of)
        view = ds.lightmap_view_lod(baked, mips, cover, dT, texels, W, H, table, dV, 0, 0, 32, 32, spread, sample=0, seed=SEED, pass_of=pass_of)
        assert tuple(view.shape) == (32, 32, 4)
        rays = ds.camera_rays(0, 0, 32, 32, 0, SEED).reshape(-1, 8)
        hits = ds.closest_hits(rays)
        coords = ds.lightmap_coords(hits, table)
        lods = ds.lightmap_lod(rays, hits, coords, dV, dT, W, H, spread)
        by_hand = ds.lightmap_sample_lod(baked, mips, cover, lods, coords, dT, texels, W, H, pass_of=pass_of)
        check(view.reshape(-1, 4).cpu().numpy(), by_hand.cpu().numpy(), "lightmap_view_lod against the five calls")
        h, c, t_np, po = ds.hits_to_numpy(hits), lightmap_texels_to_numpy(coords), lightmap_texels_to_numpy(texels), pass_of.cpu().numpy()
        want_lods = mr.lightmap_lod(rays.cpu().numpy(), h, c, V, T, W, H, spread)
        want = mr.lightmap_sample_lod(baked.cpu().numpy(), mips.cpu().numpy(), cover.cpu().numpy(), want_lods, c, T, t_np, W, H, pass_of=po)
        check(by_hand.cpu().numpy(), want, "the view against the restatement")
        # spread tiny: every lod is 0 and the view is lightmap_view
        plain = ds.lightmap_view(baked, dT, texels, W, H, table, 0, 0, 32, 32, sample=0, seed=SEED, pass_of=pass_of)
        tiny = ds.lightmap_view_lod(baked, mips, cover, dT, texels, W, H, table, dV, 0, 0, 32, 32, 1e-9, sample=0, seed=SEED, pass_of=pass_of)
        check(tiny.reshape(-1, 4).cpu().numpy(), plain.reshape(-1, 4).cpu().numpy(), "a tiny spread against lightmap_view")
    floor = (c["flags"] != 0).reshape(32, 32)
    assert floor.sum() > 200 and want_lods[floor.reshape(-1)].min() > 2  # far enough: more than four texels under every pixel
    v, p = view.cpu().numpy()[..., 0], plain.cpu().numpy()[..., 0]

    def flicker(img):  # the sum of absolute differences of neighbouring floor pixels
        across = np.abs(np.diff(img, axis=1))[floor[:, 1:] & floor[:, :-1]].sum()
        down = np.abs(np.diff(img, axis=0))[floor[1:] & floor[:-1]].sum()
        return float(across + down)

    print(f"view: flicker {flicker(v):.3f} with the chain, {flicker(p):.3f} without")
    assert flicker(v) < flicker(p)


# ---- 5. neutrality and media ------------------------------------------------------------------------------------------------------------------
def test_the_new_calls_between_renders_change_no_frame_plane_or_statistic():
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    A = atlas(64, 64)
    values, pass_of, mips, cover = chain(A, 3, 1)

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
        d_values, d_texels, d_rows, d_uvs = torch.from_numpy(values).cuda(), texels_tensor(A.texels), texels_tensor(A.rows), torch.from_numpy(A.uvs).cuda()
        d_pass, d_vertices = torch.from_numpy(pass_of).cuda(), torch.from_numpy(A.vertices).cuda()
        lods = lods_for(len(A.rows), 7)
        table = np.arange(40, dtype=np.uint32)

        def calls():
            m, c = ds.lightmap_mips(d_values, d_texels, 64, 64, pass_of=d_pass)
            ds.lightmap_mips(values, A.texels, 64, 64, pass_of=pass_of, levels=3)
            ds.lightmap_sample_lod(d_values, m, c, torch.from_numpy(lods).cuda(), d_rows, d_uvs, d_texels, 64, 64, pass_of=d_pass)
            ds.lightmap_sample_lod(values, mips, cover, lods, A.rows, A.uvs, A.texels, 64, 64, pass_of=pass_of)
            rays = ds.camera_rays(0, 0, 8, 8, 0, SEED).reshape(-1, 8)
            hits = ds.closest_hits(rays)
            coords = ds.lightmap_coords(hits, table)
            ds.lightmap_lod(rays, hits, coords, d_vertices, d_uvs, 64, 64, 0.01)
            ds.lightmap_lod(rays.cpu().numpy(), ds.hits_to_numpy(hits), lightmap_texels_to_numpy(coords), A.vertices, A.uvs, 64, 64, 0.01, 0.5)

        want = sequence(ds, lambda: None)
        assert sequence(ds, calls) == want and want[3]["rays"] > 0


def test_a_scene_with_a_constant_medium_is_served():
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    A = atlas(64, 64)
    values, pass_of, mips, cover = chain(A, 3, 1)
    lods = lods_for(len(A.rows), 7)
    r, h, c, v, t = invalid_lod_rows()["a miss"]
    h = h.copy()
    h["status"] = 1
    with DeviceScene(sc) as ds:
        got_mips, got_cover = ds.lightmap_mips(values, A.texels, 64, 64, pass_of=pass_of)
        check(got_mips, mips, "a chain on a scene with a medium")
        check(got_cover, cover, "its cover")
        want = mr.lightmap_sample_lod(values, mips, cover, lods, A.rows, A.uvs, A.texels, 64, 64, pass_of=pass_of)
        check(ds.lightmap_sample_lod(values, mips, cover, lods, A.rows, A.uvs, A.texels, 64, 64, pass_of=pass_of), want, "a lookup on such a scene")
        check(ds.lightmap_lod(r, h, c, v, t, 256, 256, 0.02), mr.lightmap_lod(r, h, c, v, t, 256, 256, 0.02), "a level of detail on such a scene")
