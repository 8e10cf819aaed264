"""Lightmap unwrap on the device (lightmap_unwrap / sol_lightmap_unwrap) against the restatement of tests/lightmap_unwrap_ref.py,
word for word: UVs, labels and every word of the result, over triangle counts around a wave and a workgroup, the known meshes, many shelves
with equal rectangles, single charts of 16 x 16 and 65 x 64 texels, three gutters and both overflow cases; the host route against the device
route, a stream that is not the default, the masked hash in a child process, guard words behind the three outputs, neutrality towards a live
scene, and the closed loop with the calls that were here before: lightmap_charts finds the unwrap's charts, and a bake that starts from a
scene's mesh and ends in lightmap_view_charts has a tap under every pixel that sees a live triangle."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import lightmap_charts_ref as cr
import lightmap_ref as lr
import lightmap_unwrap_ref as ur
import parity_util as pu
from solstrale_amd import DeviceScene, RenderConfig, _abi, lightmap_mesh, lightmap_texels_to_numpy, lightmap_triangle_table, lightmap_unwrap, lightmap_unwrap_fit, scenes
from test_gpu_lightmap_sample import assert_words_equal

pytestmark = pytest.mark.gpu

SEED = pu.SEED
F = np.float32
NONE = ur.NONE


def words(x):
    """a device tensor or an array as uint32 words on the host"""
    x = x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint32)


def same_words(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.tobytes() != want.tobytes():
        assert_words_equal(got, want, what)
        raise AssertionError(what)


def result_words(r):
    return [r.n_charts, r.live_triangles, r.used_width, r.used_height, r.overflow, 0, r.content_texels & 0xFFFFFFFF, r.content_texels >> 32]


def cases():
    """name -> (vertices, width, height, texels_per_unit, keywords)"""
    big = ur.grid(46, seed=4, bump=1.2)  # 4232 triangles
    c = {}
    for n in (0, 1, 63, 64, 65, 257, 4097):
        c[f"n{n}"] = (big[:n], 512, 512, 24.0, dict(crease_cos=0.97))
    c["cube"] = (ur.cube(), 64, 64, 8.0, {})
    c["fin"] = (ur.fin(), 64, 64, 9.0, {})
    c["bumped"] = (ur.grid(8, bump=0.5), 128, 128, 8.0, {})
    c["bumped_creased"] = (ur.grid(8, bump=0.5), 128, 128, 8.0, dict(crease_cos=0.95))
    c["dead"] = (ur.with_dead(ur.grid(9))[0], 128, 128, 11.0, {})
    c["shelves"] = (ur.disjoint(3000), 64, 16384, 8.0, {})  # a few sizes of rectangle, thousands of ties, hundreds of shelves
    c["chart16"] = (ur.grid(4, size=1.0) * F(13) + F(0.5), 64, 64, 1.0, {})  # 0.5 .. 13.5 each way: 14 texels and the two guards
    c["chart65x64"] = (ur.grid(5, size=1.0) * F([61.5, 1, 62.5]) + F(0.25), 128, 128, 1.0, {})  # (class y: the atlas x is the mesh's z)
    for g in (0, 1, 5):
        c[f"gutter{g}"] = (np.concatenate([ur.cube(), ur.disjoint(40) + F([3, 0, 3])]), 96, 256, 8.0, dict(gutter=g))
    c["too_wide"] = (ur.cube(), 8, 128, 8.0, {})
    c["too_high"] = (ur.cube(), 26, 38, 8.0, {})
    return c


CASES = cases()
_REF = {}


def ref(name):
    """the restatement of a case, computed once: (uvs, labels, the result's eight words)"""
    if name not in _REF:
        v, W, H, tpu, kw = CASES[name]
        uvs, ch, res = ur.lightmap_unwrap(v, W, H, tpu, **kw)
        _REF[name] = (uvs, ch, ur.result_words(res).tolist())
    return _REF[name]


def test_the_cases_are_what_they_are_meant_to_be():
    assert ref("cube")[2][0] == 6 and ref("fin")[2][0] == 2 and ref("bumped")[2][0] == 1 and ref("bumped_creased")[2][0] > 1
    assert ref("shelves")[2][:2] == [3000, 3000] and ref("shelves")[2][3] > 2000 and ref("shelves")[2][4] == 0
    d = ur.lightmap_unwrap(*CASES["chart16"][:4], detail=True)[3]
    assert (d["cw"].tolist(), d["ch"].tolist()) == ([16], [16])
    d = ur.lightmap_unwrap(*CASES["chart65x64"][:4], detail=True)[3]
    assert (d["cw"].tolist(), d["ch"].tolist()) == ([65], [64])
    assert ref("too_wide")[2][4] == 1 and ref("too_high")[2][4] == 2 and ref("dead")[2][1] == 162 - 3
    assert all(ref(f"gutter{g}")[2][4] == 0 for g in (0, 1, 5)) and ref("n4097")[2][0] > 100


@pytest.mark.parametrize("name", list(CASES))
def test_both_routes_equal_the_restatement_word_for_word(name):
    import torch
    v, W, H, tpu, kw = CASES[name]
    want_uvs, want_ch, want_res = ref(name)
    uvs, ch, res = lightmap_unwrap(v, W, H, tpu, **kw)  # the host route
    assert result_words(res) == want_res, (name, "host", res, want_res)
    same_words(uvs.reshape(-1, 6), want_uvs.reshape(-1, 6), (name, "host uvs"))
    assert (ch == want_ch).all(), (name, "host labels")
    d_uvs, d_ch, d_res = lightmap_unwrap(torch.from_numpy(np.ascontiguousarray(v)).cuda(), W, H, tpu, **kw)  # the device route
    assert result_words(d_res) == want_res, (name, "device", d_res, want_res)
    same_words(d_uvs.cpu().numpy().reshape(-1, 6), want_uvs.reshape(-1, 6), (name, "device uvs"))
    assert (words(d_ch) == want_ch).all(), (name, "device labels")


def test_a_stream_that_is_not_the_default_and_two_calls_in_a_row():
    import torch
    v, W, H, tpu, kw = CASES["gutter1"]
    want_uvs, want_ch, want_res = ref("gutter1")
    d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert torch.cuda.current_stream().cuda_stream == stream.cuda_stream != 0
        first = lightmap_unwrap(d_v, W, H, tpu, **kw)
        second = lightmap_unwrap(d_v, W, H, tpu, **kw)
    for uvs, ch, res in (first, second):
        assert result_words(res) == want_res
        assert_words_equal(uvs.cpu().numpy().reshape(-1, 6), want_uvs.reshape(-1, 6), "stream")
        assert (words(ch) == want_ch).all()


def test_guard_words_behind_all_three_outputs():
    import torch
    lib = _abi.load_hip()
    v, W, H, tpu, kw = CASES["dead"]
    want_uvs, want_ch, want_res = ref("dead")
    n, G = len(v), 64
    d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    uvs = torch.full((G + n * 6 + G,), 7.0, dtype=torch.float32, device="cuda")
    ch = torch.full((G + n + G,), 7, dtype=torch.int32, device="cuda")
    res = torch.full((G + 8 + G,), 7, dtype=torch.int32, device="cuda")
    cfg = _abi.SolUnwrapConfig(size=C.sizeof(_abi.SolUnwrapConfig), width=W, height=H, gutter=2, texels_per_unit=tpu, crease_cos=-1.0)
    torch.cuda.synchronize()
    rc = lib.sol_lightmap_unwrap_dev(0, None, C.byref(cfg), C.c_void_p(d_v.data_ptr()), n, C.c_void_p(uvs[G:].data_ptr()), C.c_void_p(ch[G:].data_ptr()),
                                     C.c_void_p(res[G:].data_ptr()))
    assert rc == 0, lib.sol_last_error()
    for t in (uvs, ch, res):
        assert (t[:G] == 7).all() and (t[-G:] == 7).all()
    assert words(res[G:G + 8].contiguous()).tolist() == want_res
    assert (words(ch[G:G + n].contiguous()) == want_ch).all() and (words(uvs[G:G + n * 6].contiguous()) == words(want_uvs).reshape(-1)).all()
    assert (words(d_v) == words(v)).all()  # the input is not written


CHILD = r"""
import sys
import numpy as np
import torch
from solstrale_amd import lightmap_unwrap
a = np.load(sys.argv[1])
out = {}
for k in range(int(a["n"])):
    v, (W, H, g), (tpu, cc) = a[f"v{k}"], a[f"i{k}"], a[f"f{k}"]
    for tag, x in (("h", v), ("d", torch.from_numpy(v).cuda())):
        uvs, ch, res = lightmap_unwrap(x, int(W), int(H), float(tpu), gutter=int(g), crease_cos=float(cc))
        if tag == "d":
            uvs, ch = uvs.cpu().numpy(), ch.cpu().numpy().view(np.uint32)
        out[f"{tag}uv{k}"], out[f"{tag}ch{k}"], out[f"{tag}res{k}"] = uvs, ch, np.asarray(list(res), dtype=np.uint64)
np.savez(sys.argv[2], **out)
"""


def test_the_masked_hash_path_answers_the_same_words(tmp_path):
    """SOL_LIGHTMAP_UNWRAP=collide in a fresh child process: the hash keeps 4 bits, so every run of equal hashes holds many different edges and the
    match has to tell them apart by the full key."""
    names = ["cube", "fin", "bumped_creased", "dead", "n257", "gutter1"]
    arrays = {"n": len(names)}
    for k, name in enumerate(names):
        v, W, H, tpu, kw = CASES[name]
        arrays[f"v{k}"] = np.ascontiguousarray(v)
        arrays[f"i{k}"], arrays[f"f{k}"] = np.asarray([W, H, kw.get("gutter", 2)]), np.asarray([tpu, kw.get("crease_cos", -1.0)])
    np.savez(tmp_path / "in.npz", **arrays)
    env = {**os.environ, "SOL_LIGHTMAP_UNWRAP": "collide", "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    for k, name in enumerate(names):
        want_uvs, want_ch, want_res = ref(name)
        for tag in ("h", "d"):
            res = got[f"{tag}res{k}"].tolist()
            assert res[:5] == want_res[:5] and res[5] == want_res[6] | (want_res[7] << 32), (name, tag)
            assert (got[f"{tag}ch{k}"] == want_ch).all() and (words(got[f"{tag}uv{k}"]) == words(want_uvs)).all(), (name, tag)


def test_a_call_between_two_renders_changes_no_frame():
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    v, W, H, tpu, kw = CASES["gutter1"]
    d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()

    def sequence(ds, between):
        ds.clear()
        ds.render(0, 8, SEED, counted=True)
        between()
        ds.render(8, 8, SEED)
        between()
        return zlib.crc32(ds.read().tobytes()), ds.stats()

    def calls():
        lightmap_unwrap(d_v, W, H, tpu, **kw)
        lightmap_unwrap(v, W, H, tpu, **kw)

    with DeviceScene(sc) as ds:
        want = sequence(ds, lambda: None)
        assert sequence(ds, calls) == want and want[1]["rays"] > 0


# ---- the closed loop with the calls that were here before -----------------------------------------------------------------------------------
def test_lightmap_charts_finds_the_charts_of_the_unwrap():
    import torch
    with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
        for name in ("cube", "bumped_creased", "gutter0", "n4097"):
            v, W, H, tpu, kw = CASES[name]
            d_v = torch.from_numpy(np.ascontiguousarray(v)).cuda()
            uvs, ch, res = lightmap_unwrap(d_v, W, H, tpu, **kw)
            back, n = ds.lightmap_charts(uvs, d_v)
            assert res.overflow == 0 and n == res.n_charts and torch.equal(back, ch), name


def test_a_bake_that_starts_from_a_scenes_mesh():
    """lightmap_mesh -> lightmap_unwrap -> lightmap_points(conservative) -> irradiance -> lightmap_dilate_charts -> lightmap_view_charts at 64 x 48
    pixels. The rasteriser, the dilation and the lookup equal their numpy restatements over the unwrap's UVs (the gather's rows are the device's:
    its own tests pin them), and every pixel whose hit is a live triangle has a tap."""
    import torch
    import lightmap_sample_ref as sr
    W, H = 256, 160
    sc = scenes.sponza_like(RenderConfig(64, 48, 1), n_triangles=600, texture_size=64, n_materials=4)
    nt = int(sc.desc.n_triangles)
    V, _ = lightmap_mesh(sc, 0, nt)
    table = lightmap_triangle_table(sc, 0, nt)
    want_uvs, want_ch, want_res = ur.lightmap_unwrap(V, W, H, 2.0)
    assert want_res["overflow"] == 0 and want_res["n_charts"] > 20
    with DeviceScene(sc) as ds:
        dV = torch.from_numpy(V).cuda()
        uvs, ch, res = lightmap_unwrap(dV, W, H, 2.0)
        assert result_words(res) == ur.result_words(want_res).tolist() and (words(ch) == want_ch).all()
        assert_words_equal(uvs.cpu().numpy().reshape(-1, 6), want_uvs.reshape(-1, 6), "uvs")
        points, texels = ds.lightmap_points(dV, uvs, W, H, conservative=True)
        want_points, want_texels = lr.lightmap_points(V, want_uvs, W, H, conservative=True)
        got_texels = lightmap_texels_to_numpy(texels)
        assert got_texels.tobytes() == want_texels.tobytes() and (words(points) == words(want_points).reshape(words(points).shape)).all()
        rows = ds.irradiance(points, samples=4, seed=SEED)
        baked, pass_of, plane = ds.lightmap_dilate_charts(rows, texels, ch, W, H, passes=2)
        want_baked, want_pass, want_plane = cr.lightmap_dilate_charts(rows.cpu().numpy(), want_texels, want_ch, W, H, passes=2)
        assert (words(baked) == words(want_baked).reshape(words(baked).shape)).all()
        assert (pass_of.cpu().numpy().reshape(-1) == want_pass.reshape(-1)).all() and (words(plane).reshape(-1) == want_plane.reshape(-1)).all()
        view = ds.lightmap_view_charts(baked, uvs, texels, ch, plane, W, H, table, 0, 0, 64, 48, sample=0, seed=SEED, pass_of=pass_of)
        hits = ds.closest_hits(ds.camera_rays(0, 0, 64, 48, 0, SEED).reshape(-1, 8))
        coords = lightmap_texels_to_numpy(ds.lightmap_coords(hits, table))
        want_view = cr.lightmap_sample_charts(want_baked, coords, want_uvs, want_texels, want_ch, want_plane, W, H, pass_of=want_pass)
        assert_words_equal(view.reshape(-1, 4).cpu().numpy(), want_view, "the view against the numpy chain")
        live = (coords["triangle"] != sr.NONE) & (coords["flags"] != 0)
        live[live] = want_ch[coords["triangle"][live]] != NONE
        taps = words(view.reshape(-1, 4))[:, 3]
        assert live.sum() > 1000 and (taps[live] > 0).all(), (int(live.sum()), int((taps[live] == 0).sum()))


def test_the_fit_is_the_densest_probe_and_one_step_denser_overflows():
    import torch
    v = np.concatenate([ur.cube(), ur.grid(6, bump=0.4) + F([2, 0, 0])])
    d_v = torch.from_numpy(v).cuda()
    fit = lightmap_unwrap_fit(d_v, 128, 96, gutter=1, steps=8)
    assert fit.result.overflow == 0 and fit.result.n_charts == 7 and fit.result.used_height <= 96 and fit.result.used_width <= 128
    assert 0 < fit.texels_per_unit < fit.overflow_at
    want_uvs, want_ch, want_res = ur.lightmap_unwrap(v, 128, 96, fit.texels_per_unit, gutter=1)
    assert result_words(fit.result) == ur.result_words(want_res).tolist() and (words(fit.chart_of_triangle) == want_ch).all()
    assert_words_equal(fit.uvs.cpu().numpy().reshape(-1, 6), want_uvs.reshape(-1, 6), "fit")
    denser = lightmap_unwrap(d_v, 128, 96, fit.overflow_at, gutter=1)[2]
    assert denser.overflow != 0 and ur.lightmap_unwrap(v, 128, 96, fit.overflow_at, gutter=1)[2]["overflow"] == denser.overflow
