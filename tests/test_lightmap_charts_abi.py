"""Lightmap charts (sol_lightmap_charts / sol_lightmap_dilate_charts / sol_lightmap_sample_charts / sol_lightmap_chart_levels), the
part that needs no GPU: the eight entry points are exported, declared and documented, the header is C99, the kernels are gfx950 code of the
library, every refusal of every call answers SOL_EINVAL in the stated order and in front of the device check with nothing written - and the
restatement the GPU tests compare against (tests/lightmap_charts_ref.py) has the rule's own properties: dense labels in mesh order, invariant
under what does not change an edge, the one-chart identities against tests/lightmap_ref.py and tests/lightmap_sample_ref.py, the bleed that
motivates the feature and its absence from the new chain, and the two hand-derived level counts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import lightmap_charts_ref as cr
import lightmap_ref as lr
import lightmap_sample_ref as sr
from solstrale_amd import CHART_NONE, DeviceScene, _abi, device_count
from test_lightmap_mips_abi import _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_charts_dev", "sol_lightmap_charts", "sol_lightmap_dilate_charts_dev", "sol_lightmap_dilate_charts",
                "sol_lightmap_sample_charts_dev", "sol_lightmap_sample_charts", "sol_lightmap_chart_levels_dev", "sol_lightmap_chart_levels")
KERNELS = (b"sol_lightmap_charts_hash_kernel", b"sol_lightmap_charts_match_kernel", b"sol_lightmap_charts_flatten_kernel", b"sol_lightmap_charts_ids_kernel",
           b"sol_lightmap_dilate_charts_begin_kernel", b"sol_lightmap_dilate_charts_pass_kernel", b"sol_lightmap_sample_charts_kernel",
           b"sol_lightmap_chart_level_kernel", b"sol_lightmap_chart_windows_kernel", b"sol_lightmap_chart_answer_kernel")
CFG = _abi.SolLightmapSampleConfig
F = np.float32
INF, NAN = float("inf"), float("nan")
NONE = cr.NONE


def test_the_entry_points_are_exported_declared_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene,", text), name
        assert re.search(r"\b" + name + r"\b", guide), name
    assert len(lib.sol_lightmap_charts.argtypes) == len(lib.sol_lightmap_charts_dev.argtypes) == 6
    assert len(lib.sol_lightmap_dilate_charts.argtypes) == len(lib.sol_lightmap_dilate_charts_dev.argtypes) == 13
    assert len(lib.sol_lightmap_sample_charts.argtypes) == len(lib.sol_lightmap_sample_charts_dev.argtypes) == 12
    assert len(lib.sol_lightmap_chart_levels.argtypes) == len(lib.sol_lightmap_chart_levels_dev.argtypes) == 8
    assert re.search(r"#define SOL_CHART_NONE 0xFFFFFFFFu", text) and CHART_NONE == NONE == 0xFFFFFFFF
    assert re.search(r"#define SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES \(1u << 30\)", text) and cr.MAX_TRIANGLES == 1 << 30
    assert "SOL_CHART_NONE" in guide and "SOL_LIGHTMAP_CHARTS=collide" in text
    for method in ("lightmap_charts", "lightmap_dilate_charts", "lightmap_sample_charts", "lightmap_chart_levels", "lightmap_view_charts"):
        assert callable(getattr(DeviceScene, method))


def test_the_header_is_c99(tmp_path):
    src = tmp_path / "charts.c"
    src.write_text('#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   '  int (*f[8])(void) = {(int (*)(void))sol_lightmap_charts_dev, (int (*)(void))sol_lightmap_charts, (int (*)(void))sol_lightmap_dilate_charts_dev,\n'
                   '    (int (*)(void))sol_lightmap_dilate_charts, (int (*)(void))sol_lightmap_sample_charts_dev, (int (*)(void))sol_lightmap_sample_charts,\n'
                   '    (int (*)(void))sol_lightmap_chart_levels_dev, (int (*)(void))sol_lightmap_chart_levels};\n'
                   '  printf("%u %u %d", (unsigned)SOL_CHART_NONE, (unsigned)SOL_LIGHTMAP_CHARTS_MAX_TRIANGLES, f[0] != 0);\n  return 0;\n}\n')
    exe = tmp_path / "charts"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + os.path.dirname(_abi.HIP_LIB), "-lsolstrale_hip", "-Wl,-rpath," + os.path.dirname(_abi.HIP_LIB)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == [str(0xFFFFFFFF), str(1 << 30), "1"]


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    names = set(re.findall(rb"_Z\d+(sol_[a-z0-9_]+_kernel)[A-Za-z0-9_]*\.kd", data))
    for k in KERNELS:
        assert k in names, k


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_lightmap_charts_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    uvs, vertices, chart_of, n_charts = (C.c_float * 12)(), (C.c_float * 18)(), (C.c_uint32 * 2)(), (C.c_uint32 * 1)(7)
    good = dict(scene=stand_in, uvs=uvs, vertices=vertices, n=2, chart_of=chart_of, n_charts=n_charts)
    steps = [(dict(scene=None), b"null scene"), (dict(n=(1 << 30) + 1), b"at most 2^30"), (dict(uvs=None), b"null UV"), (dict(chart_of=None), b"null label output"),
             (dict(n_charts=None), b"null chart count")]

    def call(name, a):
        return getattr(lib, name)(a["scene"], a["uvs"], a["vertices"], a["n"], a["chart_of"], a["n_charts"])

    _walk(steps, good, call, ("sol_lightmap_charts", "sol_lightmap_charts_dev"))
    assert bytes(chart_of) == bytes(8) and n_charts[0] == 7  # nothing was written
    assert call("sol_lightmap_charts", {**good, "n": 0, "uvs": None, "vertices": None, "chart_of": None}) == _abi.SOL_OK and n_charts[0] == 0  # no triangle: no device
    if device_count() == 0:
        for name in ("sol_lightmap_charts", "sol_lightmap_charts_dev"):
            assert call(name, good) == _abi.SOL_EDEVICE
            assert call(name, {**good, "vertices": None}) == _abi.SOL_EDEVICE
        assert call("sol_lightmap_charts_dev", {**good, "n": 0}) == _abi.SOL_EDEVICE  # (its count is a device word)


def test_every_refusal_of_lightmap_dilate_charts_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    texels, values, chart_of = (C.c_uint32 * 64)(), (C.c_float * 64)(), (C.c_uint32 * 2)()
    out, pass_of, plane = (C.c_float * 64)(), (C.c_uint8 * 16)(), (C.c_uint32 * 16)()
    good = dict(scene=stand_in, texels=texels, w=4, h=4, values=values, ch=3, stride=16, passes=1, chart_of=chart_of, nt=2, out=out, pass_of=pass_of, plane=plane)
    steps = [(dict(scene=None), b"null scene"), (dict(texels=None), b"null texel"), (dict(values=None), b"null value"), (dict(out=None), b"null output"),
             (dict(pass_of=None), b"null pass_of output"), (dict(plane=None), b"null plane output"), (dict(w=0), b"atlas"), (dict(h=16385), b"atlas"),
             (dict(ch=0), b"channels"), (dict(ch=33), b"channels"), (dict(stride=10), b"stride"), (dict(stride=8), b"stride"), (dict(passes=255), b"passes"),
             (dict(out=values), b"out may not be values"), (dict(chart_of=None), b"null chart_of_triangle"), (dict(nt=(1 << 30) + 1), b"at most 2^30")]

    def call(name, a):
        return getattr(lib, name)(a["scene"], a["texels"], a["w"], a["h"], a["values"], a["ch"], a["stride"], a["passes"], a["chart_of"], a["nt"], a["out"],
                                  a["pass_of"], a["plane"])

    def combine(broken, later):  # (a null value pointer is no alias of a null output)
        return not ("values" in broken and "out" in later)

    _walk(steps, good, call, ("sol_lightmap_dilate_charts", "sol_lightmap_dilate_charts_dev"), combine)
    if device_count() == 0:
        for name in ("sol_lightmap_dilate_charts", "sol_lightmap_dilate_charts_dev"):
            assert call(name, good) == _abi.SOL_EDEVICE
            assert call(name, {**good, "nt": 0, "chart_of": None, "passes": 0}) == _abi.SOL_EDEVICE  # no triangle needs no pointer
    assert bytes(out) == bytes(256) and bytes(pass_of) == bytes(16) and bytes(plane) == bytes(64) and bytes(values) == bytes(256)  # nothing was written


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, channels=3, stride_bytes=16, flags=0, chart_radius=INF)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_every_refusal_of_lightmap_sample_charts_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    uvs, texels, pass_of, values = (C.c_float * 12)(), (C.c_uint32 * 64)(), (C.c_uint8 * 16)(), (C.c_float * 64)()
    chart_of, plane, coords, out = (C.c_uint32 * 2)(), (C.c_uint32 * 16)(), (C.c_uint32 * 8)(), (C.c_float * 8)()
    good = dict(scene=stand_in, c={}, uvs=uvs, nt=2, texels=texels, values=values, chart_of=chart_of, plane=plane, coords=coords, n=2, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=40)), b"size"),
             (dict(c=dict(reserved=1)), b"reserved"), (dict(c=dict(flags=2)), b"unknown bits"), (dict(c=dict(width=0)), b"atlas"),
             (dict(c=dict(height=16385)), b"atlas"), (dict(c=dict(channels=33)), b"channels"), (dict(c=dict(stride_bytes=8)), b"stride"),
             (dict(c=dict(chart_radius=NAN)), b"chart_radius"), (dict(c=dict(chart_radius=0.5)), b"chart_radius"), (dict(c=dict(chart_radius=-INF)), b"chart_radius"),
             (dict(nt=(1 << 30) + 1), b"at most 2^30"), (dict(n=(1 << 31) + 1), b"at most 2^31)"), (dict(uvs=None), b"null UV"),
             (dict(chart_of=None), b"null chart_of_triangle"), (dict(texels=None), b"null texel"), (dict(values=None), b"null value"),
             (dict(plane=None), b"null plane"), (dict(coords=None), b"null coordinate"), (dict(out=None), b"null output"),
             (dict(out=values), b"out may not be values"), (dict(out=coords), b"out may not be coords")]

    def call(name, a):
        cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
        return getattr(lib, name)(a["scene"], cfg, a["uvs"], a["nt"], a["texels"], pass_of, a["values"], a["chart_of"], a["plane"], a["coords"], a["n"], a["out"])

    _walk(steps, good, call, ("sol_lightmap_sample_charts", "sol_lightmap_sample_charts_dev"))
    for name in ("sol_lightmap_sample_charts", "sol_lightmap_sample_charts_dev"):
        assert call(name, {**good, "n": 0}) == _abi.SOL_OK  # no row: nothing to run, no device looked for
        assert call(name, {**good, "n": 0, "nt": 0, "uvs": None, "chart_of": None, "c": dict(flags=1)}) == _abi.SOL_OK
        if device_count() == 0:
            assert call(name, good) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(32) and bytes(values) == bytes(256) and bytes(plane) == bytes(64)  # nothing was written


def test_every_refusal_of_lightmap_chart_levels_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    plane, pass_of = (C.c_uint32 * 16)(), (C.c_uint8 * 16)()
    levels, mixed_texels, mixed_windows = (C.c_uint32 * 1)(9), (C.c_uint32 * 15)(*([9] * 15)), (C.c_uint32 * 15)(*([9] * 15))
    good = dict(scene=stand_in, plane=plane, pass_of=pass_of, w=4, h=4, levels=levels, mt=mixed_texels, mw=mixed_windows)
    steps = [(dict(scene=None), b"null scene"), (dict(w=0), b"atlas"), (dict(h=16385), b"atlas"), (dict(plane=None), b"null plane"),
             (dict(levels=None), b"null levels"), (dict(mt=None), b"null mixed_texels"), (dict(mw=None), b"null mixed_windows")]

    def call(name, a):
        return getattr(lib, name)(a["scene"], a["plane"], a["pass_of"], a["w"], a["h"], a["levels"], a["mt"], a["mw"])

    _walk(steps, good, call, ("sol_lightmap_chart_levels", "sol_lightmap_chart_levels_dev"))
    assert levels[0] == 9 and list(mixed_texels) == [9] * 15 and list(mixed_windows) == [9] * 15  # nothing was written
    if device_count() == 0:
        for name in ("sol_lightmap_chart_levels", "sol_lightmap_chart_levels_dev"):
            assert call(name, good) == _abi.SOL_EDEVICE
            assert call(name, {**good, "pass_of": None}) == _abi.SOL_EDEVICE
        assert call("sol_lightmap_chart_levels_dev", {**good, "w": 1, "h": 1}) == _abi.SOL_EDEVICE  # (its answers are device words)
    assert call("sol_lightmap_chart_levels", {**good, "w": 1, "h": 1}) == _abi.SOL_OK  # a 1 x 1 plane: level 0 alone, no device looked for
    assert levels[0] == 1 and list(mixed_texels) == [0] * 15 and list(mixed_windows) == [0] * 15


# ---- the restatement's own properties: labels -----------------------------------------------------------------------------------------------
def _partition(chart):
    """the partition a label array stands for: a set of frozensets of triangle indices, and the triangles without chart"""
    chart = np.asarray(chart)
    return {frozenset(np.nonzero(chart == c)[0].tolist()) for c in np.unique(chart) if c != NONE}, set(np.nonzero(chart == NONE)[0].tolist())


def _dense_in_mesh_order(chart, n_charts):
    live = chart[chart != NONE]
    assert set(live.tolist()) == set(range(n_charts))
    first = [int(np.nonzero(chart == c)[0][0]) for c in range(n_charts)]
    assert first == sorted(first)  # chart c's lowest triangle comes before chart c + 1's


def four_chart_grid():
    """The jittered 8 x 8 grid cut into four: the UVs of the cells of row 4 and of column 4 nudged by an ulp, so that no edge between them and
    the rows below / the columns left of them is equal any more. Returns (vertices, uvs)."""
    V, T, _ = lr.grid_mesh(8, 3)
    T = T.copy()
    for y in range(8):
        for x in range(8):
            cell = slice(2 * (y * 8 + x), 2 * (y * 8 + x) + 2)
            if x >= 4:
                T[cell, :, 0] = np.nextafter(T[cell, :, 0], F(2))
            if y >= 4:
                T[cell, :, 1] = np.nextafter(T[cell, :, 1], F(2))
    return V, T


def test_labels_are_dense_in_mesh_order_and_invariant_under_what_keeps_the_edges():
    V, T, _ = lr.grid_mesh(8, 3)
    chart, n = cr.lightmap_charts(T)
    assert n == 1 and (chart == 0).all() and chart.dtype == np.uint32
    V4, T4 = four_chart_grid()
    chart4, n4 = cr.lightmap_charts(T4)
    assert n4 == 4
    _dense_in_mesh_order(chart4, n4)
    cells = chart4.reshape(8, 8, 2)
    assert (cells[:4, :4] == 0).all() and (cells[:4, 4:] == 1).all() and (cells[4:, :4] == 2).all() and (cells[4:, 4:] == 3).all()
    assert cr.lightmap_charts(T4, V4)[1] == 4 and cr.lightmap_charts(T, V)[1] == 1
    # the corner order of a triangle and the sign of a zero change no edge
    rng = np.random.default_rng(5)
    flipped = T4.copy()
    which = rng.random(len(T4)) < 0.5
    flipped[which] = flipped[which][:, ::-1]
    assert (cr.lightmap_charts(flipped)[0] == chart4).all()
    signed = T4.copy()
    zeros = signed == 0
    assert zeros.any()
    signed[zeros] = F(-0.0)
    assert np.signbit(signed[zeros]).all() and (cr.lightmap_charts(signed)[0] == chart4).all()
    # a permutation of the triangles permutes the partition and renumbers the ids by the new lowest indices
    perm = rng.permutation(len(T4))
    chart_p, n_p = cr.lightmap_charts(T4[perm], V4[perm])
    assert n_p == 4
    _dense_in_mesh_order(chart_p, n_p)
    inverse = np.argsort(perm)
    want = {frozenset(inverse[list(s)].tolist()) for s in _partition(chart4)[0]}
    assert _partition(chart_p)[0] == want
    # a triangle with a word that is not finite has no chart and joins nothing; ids stay dense around it
    bad = T4.copy()
    bad[0, 1, 0] = NAN
    chart_b, n_b = cr.lightmap_charts(bad)
    assert chart_b[0] == NONE and n_b == 4 and chart_b[1] == 0
    bad_v = V4.copy()
    bad_v[3, 2, 1] = INF
    assert cr.lightmap_charts(T4, bad_v)[0][3] == NONE and cr.lightmap_charts(T4)[0][3] == 0


def test_a_shared_corner_joins_nothing_and_a_shared_edge_joins_all_its_triangles():
    a = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5)]
    corner = [(0.5, 0.0), (1.0, 0.0), (1.0, 0.5)]  # shares the corner (0.5, 0) with a
    edge = [(0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]    # shares the edge (0.5, 0) - (0, 0.5) with a
    chart, n = cr.lightmap_charts(np.asarray([a, corner], dtype=F))
    assert n == 2 and chart.tolist() == [0, 1]
    chart, n = cr.lightmap_charts(np.asarray([a, corner, edge], dtype=F))
    assert n == 2 and chart.tolist() == [0, 1, 0]
    fan = np.asarray([[(0.2, 0.2), (0.8, 0.8), (0.1 * k, 1.0 - 0.1 * k)] for k in range(5)], dtype=F)  # five triangles on one edge
    assert cr.lightmap_charts(fan)[0].tolist() == [0] * 5
    assert cr.lightmap_charts(np.asarray([a, a, a], dtype=F))[0].tolist() == [0, 0, 0]  # exact duplicates
    # with vertices an edge is shared only where the positions agree too
    uvs = np.asarray([a, edge], dtype=F)
    pos = lr.lift(uvs)
    assert cr.lightmap_charts(uvs, pos)[1] == 1
    pos[1, :, 1] += F(1.0)
    assert cr.lightmap_charts(uvs, pos)[1] == 2
    assert cr.lightmap_charts(np.zeros((0, 3, 2), dtype=F))[1] == 0


# ---- the restatement's own properties: the one-chart identities ---------------------------------------------------------------------------
def test_with_one_chart_the_dilation_and_the_lookup_are_the_parents():
    W, H = 37, 22
    V, T, N = lr.grid_mesh(8, 1)
    T = (T * F(0.7) + F(0.1)).astype(F)  # a border the dilation has to fill
    points, texels = lr.lightmap_points(V, T, W, H, normals=N, conservative=True)
    chart_of, n = cr.lightmap_charts(T)
    assert n == 1 and (texels["triangle"] == NONE).any()
    rng = np.random.default_rng(9)
    rows = np.zeros(400, dtype=sr.TEXEL_DTYPE)
    b = rng.dirichlet((1.0, 1.0, 1.0), len(rows)).astype(F)
    rows["triangle"], rows["b1"], rows["b2"], rows["flags"] = rng.integers(0, len(T), len(rows)), b[:, 1], b[:, 2], 1
    for channels, words in ((3, 4), (2, 5)):
        values = rng.normal(size=(W * H, words)).astype(F)
        for passes in (0, 1, 4):
            want, want_pass = lr.lightmap_dilate(values, texels, W, H, passes=passes, channels=channels)
            out, pass_of, plane = cr.lightmap_dilate_charts(values, texels, chart_of, W, H, passes=passes, channels=channels)
            assert out.tobytes() == want.tobytes() and pass_of.tobytes() == want_pass.tobytes()
            assert ((plane == 0) == (pass_of != 255)).all() and ((plane == NONE) == (pass_of == 255)).all()
            for nearest in (False, True):
                a = cr.lightmap_sample_charts(out, rows, T, texels, chart_of, plane, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                b_ = sr.lightmap_sample(out, rows, T, texels, W, H, channels=channels, pass_of=pass_of, nearest=nearest)
                assert a.tobytes() == b_.tobytes()


# ---- the bleed: what the feature is for -------------------------------------------------------------------------------------------------------
def bleed_fixture(W=16, H=8):
    """A bright chart over texel columns 0..5 and a dark one over columns 7..15 of a 16 x 8 atlas: a gutter of one texel, column 6. Returns
    (uvs, texels, values, dark rows, bright rows): rows within a fifth of a texel of their chart's border towards the gutter."""
    a, b = F(6.0 / 16.0), F(7.0 / 16.0)
    uvs = np.asarray([[(0.0, 0.0), (a, 0.0), (a, 1.0)], [(0.0, 0.0), (a, 1.0), (0.0, 1.0)],
                      [(b, 0.0), (1.0, 0.0), (1.0, 1.0)], [(b, 0.0), (1.0, 1.0), (b, 1.0)]], dtype=F)
    points, texels = lr.lightmap_points(lr.lift(uvs), uvs, W, H)
    col = np.arange(W * H) % W
    assert (texels["triangle"][col <= 5] < 2).all() and (texels["triangle"][col == 6] == NONE).all() and (texels["triangle"][col >= 7] >= 2).all()
    assert (texels["triangle"][col >= 7] != NONE).all()
    values = np.zeros((W * H, 4), dtype=F)
    values[texels["triangle"] < 2, :3] = 1.0
    rng = np.random.default_rng(41)
    n = 64
    delta, v = rng.uniform(0.02, 0.18, n), rng.uniform(0.1, 0.9, n)  # texels from the border; the row's v
    dark = np.zeros(n, dtype=sr.TEXEL_DTYPE)  # triangle 3: u = 7/16 + (9/16) b1, v = b1 + b2
    dark["triangle"], dark["flags"], dark["b1"] = 3, 1, delta / 9.0
    dark["b2"] = v - dark["b1"]
    bright = np.zeros(n, dtype=sr.TEXEL_DTYPE)  # triangle 0: u = (6/16) (b1 + b2), v = b2; b0 = delta / 6
    bright["triangle"], bright["flags"], bright["b2"] = 0, 1, v
    bright["b1"] = 1.0 - delta / 6.0 - v
    return uvs, texels, values, dark, bright


def test_the_old_chain_bleeds_across_a_one_texel_gutter_and_the_new_chain_does_not():
    W, H = 16, 8
    uvs, texels, values, dark, bright = bleed_fixture(W, H)
    old, old_pass = lr.lightmap_dilate(values, texels, W, H, passes=1)
    assert (old.reshape(H, W, 4)[:, 6, 0] == 0.5).all()  # the gutter: three bright and three dark neighbours
    old_dark = sr.lightmap_sample(old, dark, uvs, texels, W, H, pass_of=old_pass)
    old_bright = sr.lightmap_sample(old, bright, uvs, texels, W, H, pass_of=old_pass)
    # d texels from the border, d in (0.02, 0.18): a dark row mixes the gutter's 0.5 in with weight 0.5 - d, a bright one with weight 0.5 - d too
    assert (old_dark[:, :3] > 0.15).all() and (old_dark[:, :3] < 0.25).all()      # (0.5 - d) / 2 instead of 0
    assert (old_bright[:, :3] > 0.75).all() and (old_bright[:, :3] < 0.85).all()  # 1 - (0.5 - d) / 2 instead of 1
    chart_of, n = cr.lightmap_charts(uvs)
    assert n == 2 and chart_of.tolist() == [0, 0, 1, 1]
    new, pass_of, plane = cr.lightmap_dilate_charts(values, texels, chart_of, W, H, passes=1)
    assert (new.reshape(H, W, 4)[:, 6, 0] == 1.0).all() and (plane[:, 6] == 0).all() and (pass_of[:, 6] == 1).all()  # the tie goes to the lower id, unmixed
    new_dark = cr.lightmap_sample_charts(new, dark, uvs, texels, chart_of, plane, W, H, pass_of=pass_of)
    new_bright = cr.lightmap_sample_charts(new, bright, uvs, texels, chart_of, plane, W, H, pass_of=pass_of)
    assert (new_dark[:, :3] == 0.0).all() and (new_dark[:, 3].view(np.uint32) >= 1).all()
    assert (new_bright[:, :3] == 1.0).all() and (new_bright[:, 3].view(np.uint32) >= 1).all()


# ---- the levels -----------------------------------------------------------------------------------------------------------------------------
def two_chart_plane(W, H, cols_a, cols_b):
    """(uvs, texels, plane): two charts over the texel columns [cols_a), [cols_b) of every row, ownership by tests/lightmap_ref.py, not dilated"""
    quads = []
    for c0, c1 in (cols_a, cols_b):
        u0, u1 = F(c0 / W), F(c1 / W)
        quads += [[(u0, 0.0), (u1, 0.0), (u1, 1.0)], [(u0, 0.0), (u1, 1.0), (u0, 1.0)]]
    uvs = np.asarray(quads, dtype=F)
    points, texels = lr.lightmap_points(lr.lift(uvs), uvs, W, H)
    col = np.arange(W * H) % W
    in_a, in_b = (col >= cols_a[0]) & (col < cols_a[1]), (col >= cols_b[0]) & (col < cols_b[1])
    assert (texels["triangle"][in_a] < 2).all() and (texels["triangle"][in_b] // 2 == 1).all() and (texels["triangle"][~in_a & ~in_b] == NONE).all()
    chart_of, n = cr.lightmap_charts(uvs)
    assert n == 2
    out, pass_of, plane = cr.lightmap_dilate_charts(np.zeros((W * H, 4), dtype=F), texels, chart_of, W, H, passes=0)
    return uvs, texels, plane


def test_the_two_hand_derived_level_counts():
    """32 x 32, charts over columns 0..7 and 16..23: level 1 holds them in columns 0..3 and 8..11, level 2 in 0..1 and 4..5, level 3 (4 wide) in
    columns 0 and 2 - no window of two columns holds both. Level 4 is 2 x 2: column 0 is the first chart, column 1 (sources 2 and 3) the second,
    and its one window holds both: levels = 4. Level 5, 1 x 1, is MIXED."""
    _, _, plane = two_chart_plane(32, 32, (0, 8), (16, 24))
    levels, mixed_texels, mixed_windows = cr.lightmap_chart_levels(plane, 32, 32)
    assert levels == 4
    assert mixed_texels.tolist() == [0, 0, 0, 0, 0, 1] + [0] * 9 and mixed_windows.tolist() == [0, 0, 0, 0, 1, 1] + [0] * 9
    # 16 x 8, columns 0..5 and 7..15: level 1's column 2 is the first chart, column 3 (sources 6 and 7) the second: a window holds both at once
    _, _, plane = two_chart_plane(16, 8, (0, 6), (7, 16))
    levels, mixed_texels, mixed_windows = cr.lightmap_chart_levels(plane, 16, 8)
    assert levels == 1 and mixed_texels[1] == 0 and mixed_windows[1] == 3  # (level 1 is 8 x 4: the windows (2, j), j = 0, 1, 2)


def test_levels_of_one_chart_of_nothing_and_of_pass_of():
    W, H = 37, 22
    plane = np.zeros((H, W), dtype=np.uint32)
    levels, mt, mw = cr.lightmap_chart_levels(plane, W, H)
    assert levels == 7 and not mt.any() and not mw.any()  # one chart: every level is safe
    assert cr.lightmap_chart_levels(np.full((H, W), NONE, dtype=np.uint32), W, H)[0] == 7
    levels, mt, mw = cr.lightmap_chart_levels(np.zeros((1, 1), dtype=np.uint32), 1, 1)
    assert levels == 1 and not mt.any() and not mw.any()  # a 1 x 1 plane: level 0 alone
    plane = np.zeros((H, W), dtype=np.uint32)
    plane[:, 20:] = 1  # two abutting charts: level 1's columns 9 and 10 hold one each, and the windows over them both
    levels, mt, mw = cr.lightmap_chart_levels(plane, W, H)
    assert levels == 1 and mt[1] == 0 and mw[1] > 0
    pass_of = np.zeros((H, W), dtype=np.uint8)
    pass_of[:, 20:] = 255  # the second chart is not covered: not live
    assert cr.lightmap_chart_levels(plane, W, H, pass_of)[0] == 7
