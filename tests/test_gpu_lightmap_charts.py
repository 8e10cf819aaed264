"""Lightmap charts on the device (sol_lightmap_charts / sol_lightmap_dilate_charts / sol_lightmap_sample_charts / sol_lightmap_chart_levels,
DESIGN.md 32). The yardstick is tests/lightmap_charts_ref.py, the rule restated in numpy: every label, every word of a dilated atlas, of its
pass_of and chart planes, of a lookup and of the level counts is compared on the host route and the device route. Around it: the masked-hash path
in a child process, guard words, the one-chart identities against the device's own lightmap_dilate and lightmap_sample, the bleed across a
one-texel gutter that the old chain shows and the new one does not (restated without a device in
tests/test_lightmap_charts_abi.py::test_the_old_chain_bleeds_across_a_one_texel_gutter_and_the_new_chain_does_not), a chain whose level count
comes from chart_levels, the view, neutrality and a scene with a medium. The mesh, the atlases and the rows are those of
tests/test_gpu_lightmap_sample.py. Atlases are at most 130 x 67, meshes at most 4096 triangles."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import lightmap_charts_ref as cr
import lightmap_mips_ref as mr
import lightmap_ref as lr
import lightmap_sample_ref as sr
import parity_util as pu
from solstrale_amd import DeviceScene, RenderConfig, lightmap_texels_to_numpy, lightmap_triangle_table, scenes
from test_gpu_irradiance import _path_stats
from test_gpu_lightmap_sample import ATLASES, CHANNELS, assert_words_equal, atlas, floor_under_a_light, lookup_mesh, texels_tensor, two_charts
from test_lightmap_charts_abi import bleed_fixture, four_chart_grid, two_chart_plane
from test_lightmap_sample_abi import invalid_rows

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F = np.float32
NONE = cr.NONE
RC = RenderConfig(32, 32, 1)


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (the geometry of a chart is the caller's: any handle serves)
        yield d


def words(x):
    """a device tensor or an array as uint32 words on the host"""
    x = x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


# ---- 1. the labels ----------------------------------------------------------------------------------------------------------------------------
def label_cases():
    """name -> (uvs, vertices or None)"""
    rng = np.random.default_rng(17)
    cases = {}
    V12, T12, _ = lr.grid_mesh(12, 5)
    for n in (0, 1, 2, 63, 64, 65, 257):
        cases[f"n{n}"] = (T12[:n], V12[:n] if n % 2 else None)
    vertices, uvs, _ = lookup_mesh()
    cases["lookup_mesh"], cases["lookup_mesh_uv_only"] = (uvs, vertices), (uvs, None)
    V8, T8, _ = lr.grid_mesh(8, 3)
    cases["grid"] = (T8, V8)
    V4, T4 = four_chart_grid()
    cases["four_charts"], cases["four_charts_uv_only"] = (T4, V4), (T4, None)
    uv2, v2 = two_charts()[:2]
    cases["two_charts_uv_only"], cases["two_charts"] = (uv2, None), (uv2, v2)
    fan = np.zeros((1000, 3, 2), dtype=F)
    fan[:, 0], fan[:, 1] = (0.25, 0.5), (0.75, 0.5)
    fan[:, 2, 0], fan[:, 2, 1] = np.linspace(0.0, 1.0, 1000), np.where(np.arange(1000) % 2, 0.9, 0.1)
    cases["fan"] = (fan, None)
    p = np.stack([np.arange(4098) / 4098.0, np.arange(4098) % 2], axis=1).astype(F)  # a strip: triangle k is points k, k + 1, k + 2
    strip = np.stack([p[:-2], p[1:-1], p[2:]], axis=1)
    cases["strip"], cases["strip_reversed"], cases["strip_permuted"] = (strip, None), (strip[::-1].copy(), None), (strip[rng.permutation(4096)], None)
    k = np.arange(300)
    base = np.stack([(k % 20) * 0.05, (k // 20) * 0.05], axis=1)[:, None, :]
    cases["disjoint"] = ((base + np.asarray([(0.01, 0.01), (0.03, 0.01), (0.01, 0.03)])[None]).astype(F), None)
    dup = np.concatenate([T8[:10], T8[:10], T8[40:44], T8[:10][:, ::-1]])
    cases["duplicates"] = (dup, lr.lift(dup))
    return cases


EXPECTED_CHARTS = {"n0": 0, "grid": 1, "four_charts": 4, "four_charts_uv_only": 4, "two_charts_uv_only": 1, "two_charts": 2, "fan": 1, "strip": 1,
                   "strip_reversed": 1, "strip_permuted": 1, "disjoint": 300, "lookup_mesh": 4, "lookup_mesh_uv_only": 5}
_label_refs = {}


def label_ref(name):
    if name not in _label_refs:
        uvs, vertices = label_cases()[name]
        _label_refs[name] = cr.lightmap_charts(uvs, vertices)
    return _label_refs[name]


@pytest.mark.parametrize("name", list(label_cases()))
def test_labels_equal_the_restatement_word_for_word(ds, name):
    import torch
    uvs, vertices = label_cases()[name]
    want, want_n = label_ref(name)
    if name in EXPECTED_CHARTS:
        assert want_n == EXPECTED_CHARTS[name]
    got, n = ds.lightmap_charts(uvs, vertices)
    assert got.dtype == np.uint32 and n == want_n and (got == want).all(), (name, "host", n, want_n, np.nonzero(got != want)[0][:8])
    d_uvs = torch.from_numpy(np.ascontiguousarray(uvs)).cuda()
    d_vertices = None if vertices is None else torch.from_numpy(np.ascontiguousarray(vertices)).cuda()
    got, n = ds.lightmap_charts(d_uvs, d_vertices)
    assert n == want_n and (words(got) == want).all(), (name, "device", n, want_n)


def test_guard_words_behind_the_labels_and_the_count(ds):
    import torch
    vertices, uvs, _ = lookup_mesh()
    want, want_n = label_ref("lookup_mesh")
    n, G = len(uvs), 64
    d_uvs, d_vertices = torch.from_numpy(uvs).cuda(), torch.from_numpy(vertices).cuda()
    out = torch.full((G + n + G,), 7, dtype=torch.int32, device="cuda")
    count = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_lightmap_charts_dev(ds.h, C.c_void_p(d_uvs.data_ptr()), C.c_void_p(d_vertices.data_ptr()), n, C.c_void_p(out[G:].data_ptr()),
                                           C.c_void_p(count[1:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n:] == 7).all() and count.tolist() == [7, want_n, 7]
    assert (words(out[G:G + n].contiguous()) == want).all()
    assert (words(d_uvs) == words(uvs)).all() and (words(d_vertices) == words(vertices)).all()  # the inputs are not written


CHILD = r"""
import sys
import numpy as np
import torch
from solstrale_amd import DeviceScene, RenderConfig, scenes
a = np.load(sys.argv[1])
out = {}
with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
    for k in range(int(a["n"])):
        uvs = a[f"uvs{k}"]
        vertices = a[f"vertices{k}"] if f"vertices{k}" in a else None
        out[f"h{k}"], hn = ds.lightmap_charts(uvs, vertices)
        d, dn = ds.lightmap_charts(torch.from_numpy(uvs).cuda(), None if vertices is None else torch.from_numpy(vertices).cuda())
        out[f"d{k}"], out[f"n{k}"] = d.cpu().numpy().view(np.uint32), np.asarray([hn, dn])
np.savez(sys.argv[2], **out)
"""


def test_the_masked_hash_path_answers_the_same_labels(ds, tmp_path):
    """SOL_LIGHTMAP_CHARTS=collide in a fresh child process: the hash keeps 4 bits, so every run of equal hashes holds many different keys and the
    match has to tell them apart by the full key. The labels are the restatement's, as the default path's (this process) are."""
    names = ["lookup_mesh", "four_charts", "two_charts", "fan", "strip_permuted", "disjoint", "duplicates", "n65"]
    cases = label_cases()
    arrays = {"n": len(names)}
    for k, name in enumerate(names):
        uvs, vertices = cases[name]
        arrays[f"uvs{k}"] = np.ascontiguousarray(uvs)
        if vertices is not None:
            arrays[f"vertices{k}"] = np.ascontiguousarray(vertices)
    np.savez(tmp_path / "in.npz", **arrays)
    env = {**os.environ, "SOL_LIGHTMAP_CHARTS": "collide", "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    for k, name in enumerate(names):
        want, want_n = label_ref(name)
        here, here_n = ds.lightmap_charts(*cases[name])  # the default path
        assert (got[f"h{k}"] == want).all() and (got[f"d{k}"] == want).all() and (here == want).all(), name
        assert got[f"n{k}"].tolist() == [want_n, want_n] and here_n == want_n, name


# ---- 2. the dilation --------------------------------------------------------------------------------------------------------------------------
class Charted:
    """The atlas of the lookup tests with the mesh's real labels: raw values per channel layout, and per number of passes the restatement's
    dilated values, pass_of and chart plane."""

    def __init__(self, W, H):
        A = atlas(W, H)
        self.A, self.W, self.H = A, W, H
        self.chart_of, self.n_charts = label_ref("lookup_mesh")
        self.texels = A.texels.copy()
        rng = np.random.default_rng(W * 77 + H)
        if W * H >= 15:  # some owned texels whose triangle is out of range or has no chart: they count as uncovered
            owned = np.nonzero(self.texels["triangle"] != NONE)[0]
            pick = owned[rng.permutation(len(owned))[:max(2, len(owned) // 20)]]
            self.texels["triangle"][pick[::2]] = len(self.chart_of) + 5
            self.texels["triangle"][pick[1::2]] = len(self.chart_of) - 2  # the triangle with a UV word that is not finite
            assert self.chart_of[len(self.chart_of) - 2] == NONE
        self.raw, self.ref = {}, {}
        for channels, nwords in CHANNELS:
            raw = (rng.normal(size=(W * H, nwords)) * rng.choice([1e-3, 1.0, 1e4], (W * H, 1))).astype(F)
            raw[:, channels:] = np.arange(W * H * (nwords - channels), dtype=np.uint32).reshape(W * H, -1).view(F)
            self.raw[channels] = raw
            for passes in (0, 1, 4):
                self.ref[(channels, passes)] = cr.lightmap_dilate_charts(raw, self.texels, self.chart_of, W, H, passes=passes, channels=channels)


_charted = {}


def charted(W, H):
    if (W, H) not in _charted:
        _charted[(W, H)] = Charted(W, H)
    return _charted[(W, H)]


@pytest.mark.parametrize("W, H", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_the_dilation_equals_the_restatement_byte_for_byte(ds, W, H):
    import torch
    Q = charted(W, H)
    d_texels, d_chart = texels_tensor(Q.texels), i32(Q.chart_of)
    planes = set()
    for channels, nwords in CHANNELS:
        raw = Q.raw[channels]
        d_raw = torch.from_numpy(raw).cuda()
        for passes in (0, 1, 4):
            want, want_pass, want_plane = Q.ref[(channels, passes)]
            tag = (W, H, channels, passes)
            out, pass_of, plane = ds.lightmap_dilate_charts(raw, Q.texels, Q.chart_of, W, H, passes=passes, channels=channels)
            assert out.tobytes() == want.tobytes() and pass_of.tobytes() == want_pass.tobytes() and plane.tobytes() == want_plane.tobytes(), tag + ("host",)
            out, pass_of, plane = ds.lightmap_dilate_charts(d_raw, d_texels, d_chart, W, H, passes=passes, channels=channels)
            assert (words(out) == words(want)).all() and (words(plane) == want_plane).all(), tag + ("device",)
            assert pass_of.cpu().numpy().tobytes() == want_pass.tobytes(), tag + ("device",)
            assert (words(d_raw) == words(raw)).all()  # the input is not written
            planes |= set(np.unique(want_plane).tolist())
            assert ((want_plane == NONE) == (want_pass == 255)).all()
    if (W, H) == (64, 64):  # the cases the atlas is made for are there: every chart that owns texels, and texels nothing reached
        assert planes == {0, 1, 2, NONE}
        bad = (Q.texels["triangle"] != NONE) & (Q.texels["triangle"] >= len(Q.chart_of) - 2)
        assert bad.sum() >= 2 and (Q.ref[(3, 0)][2].reshape(-1)[bad] == NONE).all()


@pytest.mark.parametrize("W, H", [(64, 64), (130, 67)], ids=["64x64", "130x67"])
def test_with_one_chart_the_dilation_is_the_devices_own_lightmap_dilate(ds, W, H):
    import torch
    A = atlas(W, H)
    one = np.zeros(len(A.uvs), dtype=np.uint32)  # every triangle in one chart
    rng = np.random.default_rng(3)
    for channels, nwords in CHANNELS:
        raw = rng.normal(size=(W * H, nwords)).astype(F)
        for passes in (0, 1, 4):
            want, want_pass = ds.lightmap_dilate(raw, A.texels, W, H, passes=passes, channels=channels, return_pass_of=True)
            out, pass_of, plane = ds.lightmap_dilate_charts(raw, A.texels, one, W, H, passes=passes, channels=channels)
            assert out.tobytes() == want.tobytes() and pass_of.tobytes() == want_pass.tobytes(), (W, H, channels, passes, "host")
            assert ((plane == 0) == (pass_of != 255)).all() and ((plane == NONE) == (pass_of == 255)).all()
            d_want, d_want_pass = ds.lightmap_dilate(torch.from_numpy(raw).cuda(), texels_tensor(A.texels), W, H, passes=passes, channels=channels, return_pass_of=True)
            out, pass_of, plane = ds.lightmap_dilate_charts(torch.from_numpy(raw).cuda(), texels_tensor(A.texels), i32(one), W, H, passes=passes, channels=channels)
            assert torch.equal(out.view(torch.int32), d_want.view(torch.int32)) and torch.equal(pass_of, d_want_pass), (W, H, channels, passes, "device")


# ---- 3. the lookup ----------------------------------------------------------------------------------------------------------------------------
def spoiled(Q, channels, passes):
    """the restatement's dilated atlas with some taps made not finite, as the lookup tests do"""
    out, pass_of, plane = Q.ref[(channels, passes)]
    rng = np.random.default_rng(Q.W * 31 + Q.H + channels + passes)
    out = out.copy()
    spoil = rng.random(Q.W * Q.H) < 0.06
    out[spoil, rng.integers(0, channels, int(spoil.sum()))] = rng.choice([np.inf, -np.inf, np.nan], int(spoil.sum())).astype(F)
    return out, pass_of, plane


@pytest.mark.parametrize("W, H", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_the_lookup_equals_the_restatement_word_for_word(ds, W, H):
    import torch
    Q = charted(W, H)
    A = Q.A
    d_uvs, d_texels, d_rows, d_chart = torch.from_numpy(A.uvs).cuda(), texels_tensor(Q.texels), texels_tensor(A.rows), i32(Q.chart_of)
    refused = 0
    for channels, nwords in CHANNELS:
        for passes in (None, 0, 1, 4):
            values, pass_of, plane = spoiled(Q, channels, passes or 0)
            if passes is None:
                pass_of = None
            d_values, d_plane = torch.from_numpy(values).cuda(), i32(plane)
            d_pass = None if pass_of is None else torch.from_numpy(pass_of).cuda()
            for nearest in (False, True):
                tag = (W, H, channels, passes, "nearest" if nearest else "bilinear")
                want = cr.lightmap_sample_charts(values, A.rows, A.uvs, Q.texels, Q.chart_of, plane, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                got = ds.lightmap_sample_charts(values, A.rows, A.uvs, Q.texels, Q.chart_of, plane, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                assert got.shape == (len(A.rows), channels + 1)
                assert_words_equal(got, want, tag + ("host",))
                got = ds.lightmap_sample_charts(d_values, d_rows, d_uvs, d_texels, d_chart, d_plane, W, H, channels=channels, pass_of=d_pass, nearest=nearest)
                assert_words_equal(got.cpu().numpy(), want, tag + ("device",))
                plain = sr.lightmap_sample(values, A.rows, A.uvs, Q.texels, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                refused += int((plain[:, channels].view(np.uint32) > want[:, channels].view(np.uint32)).sum())
    if (W, H) == (64, 64):
        assert refused > 50  # the guard does something on this atlas: taps of another chart were live before


@pytest.mark.parametrize("channels, nwords", [(3, 4), (27, 28)], ids=["radiance_rows", "sh9_rows"])
def test_row_counts_around_a_wave_a_permutation_and_guard_words(ds, channels, nwords):
    import torch
    W, H, G = 130, 67, 64
    Q = charted(W, H)
    A = Q.A
    values, pass_of, plane = spoiled(Q, channels, 1)
    want = cr.lightmap_sample_charts(values, A.rows, A.uvs, Q.texels, Q.chart_of, plane, W, H, channels=channels, pass_of=pass_of)
    dev = dict(uvs=torch.from_numpy(A.uvs).cuda(), texels=texels_tensor(Q.texels), chart_of_triangle=i32(Q.chart_of), chart_plane=i32(plane))
    d_values, d_pass = torch.from_numpy(values).cuda(), torch.from_numpy(pass_of).cuda()
    for n in (1, 63, 64, 65, 257):
        got = ds.lightmap_sample_charts(d_values, texels_tensor(A.rows[:n]), dev["uvs"], dev["texels"], dev["chart_of_triangle"], dev["chart_plane"], W, H,
                                        channels=channels, pass_of=d_pass)
        assert_words_equal(got.cpu().numpy(), want[:n], (channels, n, "device"))
    perm = np.random.default_rng(2).permutation(len(A.rows))
    got = ds.lightmap_sample_charts(values, A.rows[perm], A.uvs, Q.texels, Q.chart_of, plane, W, H, channels=channels, pass_of=pass_of)
    assert_words_equal(got, want[perm], (channels, "a permutation"))
    from solstrale_amd import _abi
    n = len(A.rows)
    cfg = _abi.SolLightmapSampleConfig(size=C.sizeof(_abi.SolLightmapSampleConfig), width=W, height=H, channels=channels, stride_bytes=4 * nwords, flags=0,
                                       chart_radius=float("inf"))
    out = torch.full((G + n * (channels + 1) + G,), 7.0, dtype=torch.float32, device="cuda")
    d_rows = texels_tensor(A.rows)
    torch.cuda.synchronize()
    ds._chk(ds.lib.sol_lightmap_sample_charts_dev(ds.h, C.byref(cfg), C.c_void_p(dev["uvs"].data_ptr()), len(A.uvs), C.c_void_p(dev["texels"].data_ptr()),
                                                  C.c_void_p(d_pass.data_ptr()), C.c_void_p(d_values.data_ptr()), C.c_void_p(dev["chart_of_triangle"].data_ptr()),
                                                  C.c_void_p(dev["chart_plane"].data_ptr()), C.c_void_p(d_rows.data_ptr()), n, C.c_void_p(out[G:].data_ptr())))
    ds.sync()
    assert (out[:G] == 7).all() and (out[G + n * (channels + 1):] == 7).all()
    assert_words_equal(out[G:G + n * (channels + 1)].reshape(n, channels + 1).cpu().numpy(), want, (channels, "guarded"))


@pytest.mark.parametrize("W, H", [(64, 64), (130, 67)], ids=["64x64", "130x67"])
def test_with_one_chart_the_lookup_is_the_devices_own_lightmap_sample(ds, W, H):
    import torch
    A = atlas(W, H)
    one = np.zeros(len(A.uvs), dtype=np.uint32)
    for channels, nwords in CHANNELS:
        raw = A.values[(channels, 0)]  # (with taps that are not finite)
        for passes in (0, 1, 4):
            out, pass_of, plane = ds.lightmap_dilate_charts(raw, A.texels, one, W, H, passes=passes, channels=channels)
            for nearest in (False, True):
                want = ds.lightmap_sample(out, A.rows, A.uvs, A.texels, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                got = ds.lightmap_sample_charts(out, A.rows, A.uvs, A.texels, one, plane, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                assert_words_equal(got, want, (W, H, channels, passes, nearest, "host"))
            d = [torch.from_numpy(out).cuda(), texels_tensor(A.rows), torch.from_numpy(A.uvs).cuda(), texels_tensor(A.texels)]
            want = ds.lightmap_sample(*d, W, H, channels=channels, pass_of=torch.from_numpy(pass_of).cuda())
            got = ds.lightmap_sample_charts(*d, i32(one), i32(plane), W, H, channels=channels, pass_of=torch.from_numpy(pass_of).cuda())
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (W, H, channels, passes, "device")


def test_every_class_of_invalid_row_and_a_row_without_chart_answer_zeros(ds):
    W = H = 16
    T = np.asarray([[(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)], [(0.9, 0.1), (0.9, 0.9), (np.nan, 0.9)], [(0.2, 0.2), (0.8, 0.3), (0.3, 0.8)]], dtype=F)
    chart_of = np.asarray([0, 0, NONE], dtype=np.uint32)  # triangle 2 is finite and has no chart: the caller's labels say so
    texels = np.zeros(W * H, dtype=sr.TEXEL_DTYPE)
    texels["flags"] = 1
    values, plane = np.ones((W * H, 4), dtype=F), np.zeros((H, W), dtype=np.uint32)
    names, rows = invalid_rows(len(T), 1)
    good = np.zeros(1, dtype=sr.TEXEL_DTYPE)
    good[0] = (0, 0.25, 0.25, 1)
    no_chart = good.copy()
    no_chart["triangle"] = 2
    rows = np.concatenate([good, rows, no_chart, good])
    for nearest in (False, True):
        want = cr.lightmap_sample_charts(values, rows, T, texels, chart_of, plane, W, H, nearest=nearest)
        assert (want[[0, -1], :3] == 1.0).all() and (want[1:-1].view(np.uint32) == 0).all(), names
        got = ds.lightmap_sample_charts(values, rows, T, texels, chart_of, plane, W, H, nearest=nearest)
        assert_words_equal(got, want, ("invalid rows", nearest, "host"))
        import torch
        got = ds.lightmap_sample_charts(torch.from_numpy(values).cuda(), texels_tensor(rows), torch.from_numpy(T).cuda(), texels_tensor(texels), i32(chart_of),
                                        i32(plane), W, H, nearest=nearest)
        assert_words_equal(got.cpu().numpy(), want, ("invalid rows", nearest, "device"))


def test_label_arrays_of_another_width_are_refused_by_name(ds):
    W = H = 4
    texels = np.zeros(W * H, dtype=sr.TEXEL_DTYPE)
    values, rows, uvs = np.zeros((W * H, 4), dtype=F), np.zeros(1, dtype=sr.TEXEL_DTYPE), np.zeros((2, 3, 2), dtype=F)
    wide, plane = np.zeros(2, dtype=np.int64), np.zeros((H, W), dtype=np.uint32)  # (numpy's default integer: twice the words)
    with pytest.raises(ValueError, match="chart_of_triangle"):
        ds.lightmap_dilate_charts(values, texels, wide, W, H)
    with pytest.raises(ValueError, match="chart_of_triangle"):
        ds.lightmap_sample_charts(values, rows, uvs, texels, wide, plane, W, H)
    with pytest.raises(ValueError, match="chart_plane"):
        ds.lightmap_sample_charts(values, rows, uvs, texels, wide.astype(np.uint32), plane.astype(np.float32), W, H)
    with pytest.raises(ValueError, match="chart_plane"):
        ds.lightmap_chart_levels(plane.astype(np.int64), W, H)
    out, pass_of, got = ds.lightmap_dilate_charts(values, texels, wide.astype(np.int32), W, H)  # int32 holds the same words
    assert (got == 0).all() and (pass_of == 0).all()


# ---- 4. the bleed -----------------------------------------------------------------------------------------------------------------------------
def test_the_old_chain_bleeds_across_a_one_texel_gutter_and_the_new_chain_does_not(ds):
    """tests/test_lightmap_charts_abi.py shows the same with the restatements alone: d texels from the border, d in (0.02, 0.18), the old chain
    mixes the gutter's 0.5 in with weight 0.5 - d."""
    import torch
    W, H = 16, 8
    uvs, texels, values, dark, bright = bleed_fixture(W, H)
    for device in (False, True):
        up = (lambda a: texels_tensor(a) if a.dtype == sr.TEXEL_DTYPE else torch.from_numpy(a).cuda()) if device else (lambda a: a)
        host = (lambda t: t.cpu().numpy()) if device else (lambda a: a)
        old, old_pass = ds.lightmap_dilate(up(values), up(texels), W, H, passes=1, return_pass_of=True)
        old_dark = host(ds.lightmap_sample(old, up(dark), up(uvs), up(texels), W, H, pass_of=old_pass))
        old_bright = host(ds.lightmap_sample(old, up(bright), up(uvs), up(texels), W, H, pass_of=old_pass))
        assert (old_dark[:, :3] > 0.0).all() and (old_bright[:, :3] < 1.0).all()
        assert (old_dark[:, :3] > 0.15).all() and (old_dark[:, :3] < 0.25).all() and (old_bright[:, :3] > 0.75).all() and (old_bright[:, :3] < 0.85).all()
        chart_of, n = ds.lightmap_charts(up(uvs))
        assert n == 2 and words(chart_of).tolist() == [0, 0, 1, 1]
        new, pass_of, plane = ds.lightmap_dilate_charts(up(values), up(texels), chart_of, W, H, passes=1)
        new_dark = host(ds.lightmap_sample_charts(new, up(dark), up(uvs), up(texels), chart_of, plane, W, H, pass_of=pass_of))
        new_bright = host(ds.lightmap_sample_charts(new, up(bright), up(uvs), up(texels), chart_of, plane, W, H, pass_of=pass_of))
        assert (new_dark[:, :3] == 0.0).all() and (new_dark[:, 3].view(np.uint32) >= 1).all(), device
        assert (new_bright[:, :3] == 1.0).all() and (new_bright[:, 3].view(np.uint32) >= 1).all(), device


# ---- 5. the levels ----------------------------------------------------------------------------------------------------------------------------
def check_levels(ds, plane, W, H, pass_of, tag):
    import torch
    want = cr.lightmap_chart_levels(plane, W, H, pass_of)
    got = ds.lightmap_chart_levels(plane, W, H, pass_of)
    assert got[0] == want[0] and (got[1] == want[1]).all() and (got[2] == want[2]).all(), (tag, "host", got, want)
    got = ds.lightmap_chart_levels(i32(plane), W, H, None if pass_of is None else torch.from_numpy(pass_of).cuda())
    assert got[0] == want[0] and (got[1] == want[1]).all() and (got[2] == want[2]).all(), (tag, "device", got, want)
    return want


@pytest.mark.parametrize("W, H", ATLASES, ids=[f"{w}x{h}" for w, h in ATLASES])
def test_the_levels_equal_the_restatement(ds, W, H):
    Q = charted(W, H)
    seen = set()
    for passes in (0, 1, 4):
        _, pass_of, plane = Q.ref[(3, passes)]
        for po in (None, pass_of):
            want = check_levels(ds, plane, W, H, po, (W, H, passes, po is not None))
            seen.add(want[0])
            full = mr.mip_layout(W, H)[0]
            assert 1 <= want[0] <= full and not want[1][full:].any() and not want[2][full:].any() and want[1][0] == want[2][0] == 0
    hidden = Q.ref[(3, 4)][1].copy()  # pass_of decides: with the dilated texels taken out again the plane is the undilated one's
    hidden[hidden != 0] = 255
    got, undilated = check_levels(ds, Q.ref[(3, 4)][2], W, H, hidden, "hidden"), cr.lightmap_chart_levels(Q.ref[(3, 0)][2], W, H)
    assert got[0] == undilated[0] and (got[1] == undilated[1]).all() and (got[2] == undilated[2]).all()


def test_the_two_hand_derived_level_counts(ds):
    _, _, plane = two_chart_plane(32, 32, (0, 8), (16, 24))
    levels, mt, mw = check_levels(ds, plane, 32, 32, None, "32x32")
    assert levels == 4 and mt.tolist() == [0, 0, 0, 0, 0, 1] + [0] * 9 and mw.tolist() == [0, 0, 0, 0, 1, 1] + [0] * 9
    _, _, plane = two_chart_plane(16, 8, (0, 6), (7, 16))
    levels, mt, mw = check_levels(ds, plane, 16, 8, None, "16x8")
    assert levels == 1 and mw[1] == 3
    one = np.zeros((1, 1), dtype=np.uint32)
    assert check_levels(ds, one, 1, 1, None, "1x1")[0] == 1


def test_a_chain_cut_at_chart_levels_mixes_no_charts(ds):
    """The four-chart grid in a 64 x 64 atlas, each chart shrunk towards its own quadrant's centre so that gutters open between them: the levels
    chart_levels answers, handed to lightmap_mips, give a chain in which no covered texel has sources of two charts - checked from the planes."""
    W = H = 64
    V, T = four_chart_grid()
    chart_of, n = cr.lightmap_charts(T)
    assert n == 4
    T = T.copy()
    for c, (cx, cy) in enumerate(((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75))):
        centre = np.asarray((cx, cy), dtype=F)
        T[chart_of == c] = ((T[chart_of == c] - centre) * F(0.6) + centre).astype(F)
    got_chart, got_n = ds.lightmap_charts(T)
    assert got_n == 4 and (got_chart == cr.lightmap_charts(T)[0]).all()
    points, texels = ds.lightmap_points(V, T, W, H)
    values = np.zeros((W * H, 4), dtype=F)
    values[:, :3] = np.random.default_rng(4).uniform(0.1, 1.0, (W * H, 3))
    out, pass_of, plane = ds.lightmap_dilate_charts(values, texels, got_chart, W, H, passes=1)
    levels, mt, mw = ds.lightmap_chart_levels(plane, W, H, pass_of)
    assert 2 <= levels < mr.mip_layout(W, H)[0], levels  # gutters of at least nine texels: some levels are safe, the last ones are not
    mips, cover = ds.lightmap_mips(out, texels, W, H, pass_of=pass_of, levels=levels)
    planes = cr.chart_level_planes(plane, W, H, pass_of)
    n_levels, ws, hs, offsets, total = mr.mip_layout(W, H, levels)
    assert len(cover) == total
    for l in range(1, levels):
        covered = cover[offsets[l]:offsets[l] + ws[l] * hs[l]].reshape(hs[l], ws[l]) == 0
        assert covered.any() and (planes[l][covered] != cr.MIXED).all() and (planes[l][covered] != NONE).all(), l
    assert (planes[levels] == cr.MIXED).any() or mw[levels] > 0  # and one level more would mix


# ---- 6. the view, neutrality and media --------------------------------------------------------------------------------------------------------
def test_the_view_is_its_four_calls():
    import torch
    W = H = 32
    sc, V, T = floor_under_a_light()
    table = lightmap_triangle_table(sc, 0, len(V))
    with DeviceScene(sc) as ds:
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        chart_of, n = ds.lightmap_charts(dT, dV)
        assert n == 1
        points, texels = ds.lightmap_points(dV, dT, W, H)
        rows = ds.irradiance(points, samples=5, seed=SEED)
        baked, pass_of, plane = ds.lightmap_dilate_charts(rows, texels, chart_of, W, H, passes=2)
        view = ds.lightmap_view_charts(baked, dT, texels, chart_of, plane, W, H, table, 0, 0, 32, 32, sample=0, seed=SEED, pass_of=pass_of)
        assert tuple(view.shape) == (32, 32, 4)
        hits = ds.closest_hits(ds.camera_rays(0, 0, 32, 32, 0, SEED).reshape(-1, 8))
        coords = ds.lightmap_coords(hits, table)
        by_hand = ds.lightmap_sample_charts(baked, coords, dT, texels, chart_of, plane, W, H, pass_of=pass_of)
        assert_words_equal(view.reshape(-1, 4).cpu().numpy(), by_hand.cpu().numpy(), "lightmap_view_charts against the four calls")
        old = ds.lightmap_view(ds.lightmap_dilate(rows, texels, W, H, passes=2), dT, texels, W, H, table, 0, 0, 32, 32, sample=0, seed=SEED, pass_of=pass_of)
        assert torch.equal(view.view(torch.int32), old.view(torch.int32))  # one chart: lightmap_view's words
        assert (view[..., 3].view(torch.int32) > 0).any()


def test_chart_calls_between_renders_change_no_frame_plane_or_statistic():
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    Q = charted(64, 64)
    A = Q.A

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
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(radiance.tobytes()))

    with DeviceScene(sc) as ds:
        def calls():
            chart_of, n = ds.lightmap_charts(torch.from_numpy(A.uvs).cuda(), torch.from_numpy(A.vertices).cuda())
            out, pass_of, plane = ds.lightmap_dilate_charts(torch.from_numpy(Q.raw[3]).cuda(), texels_tensor(Q.texels), chart_of, 64, 64, passes=2)
            ds.lightmap_sample_charts(out, texels_tensor(A.rows), torch.from_numpy(A.uvs).cuda(), texels_tensor(Q.texels), chart_of, plane, 64, 64, pass_of=pass_of)
            ds.lightmap_chart_levels(plane, 64, 64, pass_of)
            ds.lightmap_charts(A.uvs)
            ds.lightmap_chart_levels(Q.ref[(3, 1)][2], 64, 64)

        want = sequence(ds, lambda: None)
        assert sequence(ds, calls) == want and want[3]["rays"] > 0


def test_a_scene_with_a_constant_medium_is_served():
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    Q = charted(64, 64)
    A = Q.A
    with DeviceScene(sc) as ds:
        chart_of, n = ds.lightmap_charts(A.uvs, A.vertices)
        assert (chart_of == Q.chart_of).all() and n == Q.n_charts
        want, want_pass, want_plane = Q.ref[(3, 1)]
        out, pass_of, plane = ds.lightmap_dilate_charts(Q.raw[3], Q.texels, chart_of, 64, 64, passes=1)
        assert out.tobytes() == want.tobytes() and pass_of.tobytes() == want_pass.tobytes() and plane.tobytes() == want_plane.tobytes()
        got = ds.lightmap_sample_charts(out, A.rows, A.uvs, Q.texels, chart_of, plane, 64, 64, pass_of=pass_of)
        assert_words_equal(got, cr.lightmap_sample_charts(want, A.rows, A.uvs, Q.texels, Q.chart_of, want_plane, 64, 64, pass_of=want_pass), "a medium scene")
        assert ds.lightmap_chart_levels(plane, 64, 64, pass_of)[0] == cr.lightmap_chart_levels(want_plane, 64, 64, want_pass)[0]
