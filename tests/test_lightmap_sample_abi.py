"""Lightmap lookups (sol_lightmap_coords / sol_lightmap_sample), the part that needs no GPU: the four entry points are exported,
declared and documented, SolLightmapSampleConfig (32 bytes) has the same size and offsets from gcc and from ctypes, every refusal answers
SOL_EINVAL in the stated order and in front of the device check with nothing written, the kernels are gfx950 code of the library - and the
restatement the GPU tests compare against (tests/lightmap_sample_ref.py) has the rule's own properties, each within a bound derived here from the
roundings the rule performs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lightmap_ref as lr
import lightmap_sample_ref as sr
from solstrale_amd import LIGHTMAP_TEXEL_DTYPE, DeviceScene, _abi, device_count, lightmap_triangle_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_coords_dev", "sol_lightmap_coords", "sol_lightmap_sample_dev", "sol_lightmap_sample")
CFG = _abi.SolLightmapSampleConfig
CFG_OFFSETS = {"size": 0, "width": 4, "height": 8, "channels": 12, "stride_bytes": 16, "flags": 20, "chart_radius": 24, "reserved": 28}
F = np.float32
EPS = float(np.finfo(F).eps) / 2  # the relative error of one rounding
INF, NAN = float("inf"), float("nan")
GRID_SEED = 1


def test_the_four_entry_points_are_exported_declared_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene,", text), name
        assert getattr(lib, name).argtypes is not None
        assert re.search(r"\b" + name + r"\b", guide), name
    assert len(lib.sol_lightmap_coords.argtypes) == len(lib.sol_lightmap_coords_dev.argtypes) == 6
    assert len(lib.sol_lightmap_sample.argtypes) == len(lib.sol_lightmap_sample_dev.argtypes) == 12
    assert _abi.SOL_LIGHTMAP_SAMPLE_NEAREST == 1 and re.search(r"#define SOL_LIGHTMAP_SAMPLE_NEAREST 1u", text)
    assert _abi.SOL_LIGHTMAP_TABLE_ROTATION_SHIFT == sr.ROTATION_SHIFT == 30 and re.search(r"#define SOL_LIGHTMAP_TABLE_ROTATION_SHIFT 30u", text)
    assert _abi.SOL_LIGHTMAP_TABLE_TRIANGLE_MASK == sr.TRIANGLE_MASK and re.search(r"#define SOL_LIGHTMAP_TABLE_TRIANGLE_MASK 0x3FFFFFFFu", text)
    for method in ("lightmap_coords", "lightmap_sample", "lightmap_view"):
        assert callable(getattr(DeviceScene, method))
    assert sr.HIT_DTYPE == DeviceScene.RAY_HIT_DTYPE and sr.TEXEL_DTYPE == LIGHTMAP_TEXEL_DTYPE


def test_the_config_agrees_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(CFG) == 32
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == CFG_OFFSETS
    fields = ", ".join(f"(unsigned)offsetof(SolLightmapSampleConfig, {n})" for n in CFG_OFFSETS)
    count = 1 + len(CFG_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolLightmapSampleConfig), {fields});\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32] + list(CFG_OFFSETS.values())


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, channels=3, stride_bytes=16, flags=0, chart_radius=INF, reserved=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_every_refusal_of_lightmap_sample_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of the device check reads the handle. Each bad argument is
    paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    uvs, vertices, texels, pass_of = (C.c_float * 12)(), (C.c_float * 18)(), (C.c_uint32 * 64)(), (C.c_uint8 * 16)()
    values, points, coords, out = (C.c_float * 64)(), (C.c_float * 128)(), (C.c_uint32 * 8)(), (C.c_float * 8)()
    good = dict(scene=stand_in, c={}, uvs=uvs, nt=2, texels=texels, values=values, vertices=None, points=None, coords=coords, n=2, out=out)
    # (what to break - "c": fields of the configuration -, the word sol_last_error must hold), in the header's order
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=28)), b"size"),
             (dict(c=dict(reserved=1)), b"reserved"), (dict(c=dict(flags=2)), b"flags"), (dict(c=dict(width=0)), b"atlas"),
             (dict(c=dict(height=16385)), b"atlas"), (dict(c=dict(channels=0)), b"channels (1 .. 32)"),
             (dict(c=dict(channels=33, stride_bytes=256)), b"channels (1 .. 32)"), (dict(c=dict(stride_bytes=18)), b"stride"),
             (dict(c=dict(stride_bytes=8)), b"stride"), (dict(c=dict(chart_radius=NAN)), b"chart_radius"), (dict(c=dict(chart_radius=0.0)), b"chart_radius"),
             (dict(c=dict(chart_radius=-1.0)), b"chart_radius"), (dict(vertices=vertices), b"go together"), (dict(points=points), b"go together"),
             (dict(c=dict(chart_radius=0.5)), b"needs the guard arrays"), (dict(nt=(1 << 31) - 1), b"2^31 - 2"), (dict(n=(1 << 31) + 1), b"at most 2^31)"),
             (dict(uvs=None), b"null UV"), (dict(texels=None), b"null texel"), (dict(values=None), b"null value"), (dict(coords=None), b"null coordinate"),
             (dict(out=None), b"null output"), (dict(out=values), b"out may not be values"), (dict(out=coords), b"out may not be coords")]
    for name in ("sol_lightmap_sample", "sol_lightmap_sample_dev"):
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
            return fn(a["scene"], cfg, a["uvs"], a["nt"], a["texels"], pass_of, a["values"], a["vertices"], a["points"], a["coords"], a["n"], a["out"])

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:  # the earlier refusal is the one named
                if (set(later) - {"c"}) & (set(broken) - {"c"}) or set(later.get("c", {})) & set(broken.get("c", {})):
                    continue  # (two values for one argument cannot be combined)
                if {"vertices", "points"} & set(broken) and {"vertices", "points"} & set(later):
                    continue  # (both given is no fault)
                args = {**good, **later, **broken, "c": {**later.get("c", {}), **broken.get("c", {})}}
                assert call(args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        # a finite radius with both arrays is no fault; n == 0 succeeds before the device is looked for; n_triangles == 0 needs no UV pointer
        assert call({**good, "n": 0}) == _abi.SOL_OK
        assert call({**good, "n": 0, "nt": 0, "uvs": None, "vertices": vertices, "points": points, "c": dict(chart_radius=0.5)}) == _abi.SOL_OK
        if device_count() == 0:
            assert call({**good, "vertices": vertices, "points": points, "c": dict(chart_radius=0.5)}) == _abi.SOL_EDEVICE
            assert call({**good, "c": dict(flags=1)}) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(32) and bytes(values) == bytes(256) and bytes(coords) == bytes(32)  # nothing was written


def test_every_refusal_of_lightmap_coords_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    hits, table, out = (C.c_uint32 * 16)(), (C.c_uint32 * 4)(), (C.c_uint32 * 8)()
    good = dict(scene=stand_in, hits=hits, n=2, table=table, n_dfs=4, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(n=(1 << 31) + 1), b"hits in one call"), (dict(n_dfs=(1 << 31) + 1), b"a table of"),
             (dict(table=None), b"null table"), (dict(hits=None), b"null hit"), (dict(out=None), b"null output"), (dict(out=hits), b"out may not be hits")]
    for name in ("sol_lightmap_coords", "sol_lightmap_coords_dev"):
        fn = getattr(lib, name)

        def call(a):
            return fn(a["scene"], a["hits"], a["n"], a["table"], a["n_dfs"], a["out"])

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:
                if set(later) & set(broken):
                    continue
                assert call({**good, **later, **broken}) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        assert call({**good, "n": 0}) == _abi.SOL_OK
        if device_count() == 0:
            assert call({**good, "n_dfs": 0, "table": None}) == _abi.SOL_EDEVICE  # an empty table needs no pointer
    assert bytes(out) == bytes(32)  # nothing was written


def test_the_kernels_are_gfx950_code_of_the_library_and_the_radiance_family_is_as_it_was():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for kernel in (b"sol_lightmap_coords_kernel", b"sol_lightmap_sample_kernel"):
        assert kernel in data, kernel
    # the instances of the radiance family, by their mangled names' kernel descriptors: none of the new kernels matches sol_radiance_*
    names = set(re.findall(rb"_Z\d+(sol_[a-z0-9_]+_kernel)[A-Za-z0-9_]*\.kd", data))
    assert b"sol_lightmap_coords_kernel" in names and b"sol_lightmap_sample_kernel" in names
    assert not [n for n in names if n.startswith(b"sol_radiance") and b"lightmap" in n]
    assert len(set(re.findall(rb"_Z\d+sol_lightmap_(?:coords|sample)_kernel[A-Za-z0-9_]*\.kd", data))) == 2  # one shape each


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------------
def _grid_atlas(W=64, H=64):
    V, T, N = lr.grid_mesh(16, GRID_SEED)
    points, texels = lr.lightmap_points(V, T, W, H, normals=N)
    return V, T, points, texels


def _random_rows(rng, n_triangles, n):
    """n surface rows inside random triangles"""
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
    rows = np.zeros(n, dtype=sr.TEXEL_DTYPE)
    rows["triangle"], rows["b1"], rows["b2"], rows["flags"] = rng.integers(0, n_triangles, n), b[:, 1], b[:, 2], 1
    return rows


def test_a_constant_atlas_answers_the_constant():
    """sum = c * w_a + c * w_b + .. and wsum = w_a + w_b + ..: each of the at most four products is rounded once (relative error EPS), each of the
    at most three effective additions of either chain once (the first, onto 0, is exact), and so is the division. To first order the quotient
    is off by at most (1 + 3 + 3 + 1) EPS relative; 9 EPS covers the second-order terms."""
    V, T, points, texels = _grid_atlas()
    rng = np.random.default_rng(11)
    rows = _random_rows(rng, len(V), 4000)
    for c in (1.0, 0.3, 1234.5678, -7e-5):
        values = np.full((64 * 64, 4), F(c), dtype=F)
        out = sr.lightmap_sample(values, rows, T, texels, 64, 64)
        count = out[:, 3].view(np.uint32)
        assert (count >= 1).all() and (count == 4).mean() > 0.8  # the mesh tiles the atlas: only taps beyond the border are missing
        assert (np.abs(out[:, :3].astype(np.float64) - float(F(c))) <= 9 * EPS * abs(float(F(c)))).all()


def test_nearest_at_the_texel_rows_returns_the_texels_own_words():
    V, T, points, texels = _grid_atlas()
    rng = np.random.default_rng(12)
    values = rng.normal(size=(64 * 64, 4)).astype(F)
    values[:, 3] = np.arange(64 * 64, dtype=np.uint32).view(F)
    own = texels["flags"] == 1
    assert own.all()  # (the jittered grid tiles the atlas, tests/test_lightmap_abi.py)
    out = sr.lightmap_sample(values, texels[own], T, texels, 64, 64, nearest=True)
    assert (out[:, :3].view(np.uint32) == values[own][:, :3].view(np.uint32)).all() and (out[:, 3].view(np.uint32) == 1).all()
    # and bilinear there: the centre tap has all the weight up to the rounding of the interpolated UV, so the answer is near the texel's value
    out = sr.lightmap_sample(values, texels[own], T, texels, 64, 64)
    assert (out[:, 3].view(np.uint32) >= 1).all()


def test_an_affine_atlas_is_reproduced_inside_a_chart():
    """value(i, j) = a + b * (i + 0.5) / W + c * (j + 0.5) / H, stored in float32. Bilinear interpolation reproduces an affine function exactly in
    real arithmetic: with all four taps live the answer is a + b * u + c * v at the row's own (u, v). The bound, with M = |a| + |b| + |c| the
    largest magnitude involved: the stored values are rounded once (EPS M); the rule's u and v carry 5 roundings each (three products, two
    additions of numbers of magnitude at most 1: 5 EPS, times |b| or |c|, together at most 5 EPS M); x = u * W - 0.5 carries two more roundings
    of a number up to W, an absolute 2 EPS W in texels or 2 EPS in u (2 EPS M); fx = x - floor(x) is exact; the weights' own roundings (1 - fx and
    the product) enter sum and wsum alike and only shift the average among four taps that differ by M / 32 at most (below EPS M); the products
    and the two chains and the division add (1 + 3 + 3 + 1) EPS M as for a constant atlas. Total below (1 + 5 + 2 + 1 + 8) EPS M = 17 EPS M;
    20 EPS M covers the second-order terms and the float64 evaluation of the expectation."""
    W = H = 64
    V, T, points, texels = _grid_atlas(W, H)
    a, b, c = 0.75, 2.5, -1.25
    M = abs(a) + abs(b) + abs(c)
    j, i = np.divmod(np.arange(W * H), W)
    values = np.zeros((W * H, 4), dtype=F)
    for ch, scale in enumerate((1.0, 2.0, -0.5)):
        values[:, ch] = (scale * (a + b * (i + 0.5) / W + c * (j + 0.5) / H)).astype(F)
    rng = np.random.default_rng(13)
    rows = _random_rows(rng, len(V), 6000)
    out, taps = sr.lightmap_sample(values, rows, T, texels, W, H, return_taps=True)
    inner = taps.all(axis=1)
    assert inner.mean() > 0.9
    uv = T.astype(np.float64)[rows["triangle"]]
    b1, b2 = rows["b1"].astype(np.float64), rows["b2"].astype(np.float64)
    b0 = 1.0 - b1 - b2
    u = uv[:, 0, 0] * b0 + uv[:, 1, 0] * b1 + uv[:, 2, 0] * b2
    v = uv[:, 0, 1] * b0 + uv[:, 1, 1] * b1 + uv[:, 2, 1] * b2
    for ch, scale in enumerate((1.0, 2.0, -0.5)):
        want = scale * (a + b * u + c * v)
        assert (np.abs(out[inner, ch].astype(np.float64) - want[inner]) <= 20 * EPS * M * abs(scale)).all()


def test_the_count_is_the_number_of_live_taps_and_dead_rows_answer_zeros():
    W, H = 20, 12
    rng = np.random.default_rng(14)
    T = np.asarray([[(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], [(1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]], dtype=F)
    texels = np.zeros(W * H, dtype=sr.TEXEL_DTYPE)
    owned = rng.random(W * H) < 0.6
    texels["triangle"] = np.where(owned, 0, sr.NONE)
    texels["flags"] = owned
    values = rng.normal(size=(W * H, 5)).astype(F)
    values[rng.random(W * H) < 0.1, 1] = np.inf
    values[rng.random(W * H) < 0.1, 0] = np.nan
    values[:, 2:] = np.nan  # (beyond the two channels: never read)
    rows = _random_rows(rng, 2, 3000)
    out, taps = sr.lightmap_sample(values, rows, T, texels, W, H, channels=2, return_taps=True)
    count = out[:, 2].view(np.uint32)
    assert set(np.unique(count)) == {0, 1, 2, 3, 4}
    some = taps.any(axis=1)
    assert (count[some] == taps.sum(axis=1)[some]).all()  # (random rows: no live tap has weight zero)
    assert (out[~some].view(np.uint32) == 0).all() and np.isfinite(out[:, :2]).all()
    # the liveness of the restatement against an independent evaluation in float64 / integers
    uv = T.astype(np.float64)[rows["triangle"]]
    b1, b2 = rows["b1"].astype(np.float64), rows["b2"].astype(np.float64)
    x = (uv[:, 0, 0] * (1 - b1 - b2) + uv[:, 1, 0] * b1 + uv[:, 2, 0] * b2) * W - 0.5
    y = (uv[:, 0, 1] * (1 - b1 - b2) + uv[:, 1, 1] * b1 + uv[:, 2, 1] * b2) * H - 0.5
    clear = (np.abs(x - np.round(x)) > 1e-4) & (np.abs(y - np.round(y)) > 1e-4)  # (away from where rounding decides the tap)
    want = np.zeros(len(rows), dtype=np.int64)
    good = (owned & np.isfinite(values[:, :2]).all(axis=1)).reshape(H, W)
    for k in range(4):
        i, j = np.floor(x).astype(int) + (k & 1), np.floor(y).astype(int) + (k >> 1)
        inside = (i >= 0) & (j >= 0) & (i < W) & (j < H)
        want += inside & good[np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)]
    assert clear.mean() > 0.99 and (count[clear] == want[clear]).all()
    # all four taps dead: an atlas without an owner
    texels["triangle"], texels["flags"] = sr.NONE, 0
    assert (sr.lightmap_sample(values, rows, T, texels, W, H, channels=2).view(np.uint32) == 0).all()
    # pass_of decides coverage where it is given
    pass_of = np.where(rng.random(W * H) < 0.5, 255, 1).astype(np.uint8)
    out, taps = sr.lightmap_sample(np.ones((W * H, 2), F), rows, T, texels, W, H, channels=2, pass_of=pass_of, return_taps=True)
    assert taps.any() and (out[:, 2].view(np.uint32) == taps.sum(axis=1)).all()


def invalid_rows(n_triangles, bad_uv_triangle, bad_vertex_triangle=None):
    """One surface row per class of invalid row (name, row); the classes that need a triangle with a non-finite word name that triangle."""
    cases = [("flags == 0", (0, 0.25, 0.25, 0)), ("no triangle", (sr.NONE, 0.25, 0.25, 1)), ("triangle == n_triangles", (n_triangles, 0.25, 0.25, 1)),
             ("triangle far beyond", (0x7FFFFFFF, 0.25, 0.25, 1)), ("b1 NaN", (0, NAN, 0.25, 1)), ("b1 inf", (0, INF, 0.25, 2)), ("b2 -inf", (0, 0.25, -INF, 1)),
             ("b2 NaN", (0, 0.25, NAN, 1)), ("a UV word that is not finite", (bad_uv_triangle, 0.25, 0.25, 1))]
    if bad_vertex_triangle is not None:
        cases.append(("a vertex word that is not finite", (bad_vertex_triangle, 0.25, 0.25, 1)))
    rows = np.zeros(len(cases), dtype=sr.TEXEL_DTYPE)
    for k, (_, r) in enumerate(cases):
        rows[k] = r
    return [c[0] for c in cases], rows


def test_every_class_of_invalid_row_answers_zeros():
    W = H = 16
    T = np.asarray([[(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)], [(0.9, 0.1), (0.9, 0.9), (NAN, 0.9)], [(0.2, 0.2), (0.8, 0.3), (0.3, 0.8)]], dtype=F)
    V = lr.lift(np.nan_to_num(T))
    V[2, 1, 1] = INF
    texels = np.zeros(W * H, dtype=sr.TEXEL_DTYPE)
    texels["flags"] = 1
    values = np.ones((W * H, 4), dtype=F)
    points = np.zeros((W * H, 8), dtype=F)
    names, rows = invalid_rows(len(T), 1, 2)
    good = np.zeros(1, dtype=sr.TEXEL_DTYPE)
    good[0] = (0, 0.25, 0.25, 1)
    for nearest in (False, True):
        out = sr.lightmap_sample(values, np.concatenate([good, rows, good]), T, texels, W, H, nearest=nearest, chart_radius=100.0, vertices=V, points=points)
        assert (out[[0, -1], :3] == 1).all() and (out[[0, -1], 3].view(np.uint32) >= 1).all()
        for k, name in enumerate(names):
            assert (out[1 + k].view(np.uint32) == 0).all(), name
        # without the guard the vertex words are not looked at: triangle 2's row is good
        out = sr.lightmap_sample(values, rows, T, texels, W, H, nearest=nearest)
        assert (out[:-1].view(np.uint32) == 0).all() and (out[-1, :3] == 1).all()


def test_the_coords_of_the_restatement_follow_the_record_rotation():
    """A hit's (u, v) weigh the edges of the rotated record: the row's (b1, b2) must name the same point in the triangle's own order."""
    rng = np.random.default_rng(15)
    P = rng.normal(size=(3, 3))
    hits = np.zeros(8, dtype=sr.HIT_DTYPE)
    hits["status"], hits["kind"] = sr.RAY_HIT, sr.REF_TRIANGLE
    hits["u"], hits["v"] = 0.25, 0.5
    hits["dfs_index"] = [0, 1, 2, 3, 4, 0, 0, 0]
    hits["status"][5], hits["kind"][6], hits["dfs_index"][7] = 0, 3, 9
    table = np.asarray([7, 7 | 1 << 30, 7 | 2 << 30, sr.NONE, 7 | 3 << 30], dtype=np.uint32)
    rows = sr.lightmap_coords(hits, table)
    assert (rows["triangle"][:3] == 7).all() and (rows["flags"][:3] == 1).all()
    assert (rows[3:].view(np.uint32).reshape(-1, 4) == (sr.NONE, 0, 0, 0)).all()
    for k in range(3):
        rec = (P[k], P[(k + 1) % 3], P[(k + 2) % 3])  # record k starts at corner k
        at_record = rec[0] + 0.25 * (rec[1] - rec[0]) + 0.5 * (rec[2] - rec[0])
        b1, b2 = float(rows["b1"][k]), float(rows["b2"][k])
        assert np.allclose(P[0] * (1 - b1 - b2) + P[1] * b1 + P[2] * b2, at_record, atol=1e-6)


def test_the_triangle_table_names_every_triangle_by_its_dfs_index_with_its_rotation():
    from solstrale_amd import CameraConfig, RenderConfig, SceneBuilder
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(0.7, 0.7, 0.7))
    tri = np.asarray([[(0, 0, 0), (1, 0, 0), (0, 1, 0)],      # longest edge v1v2: rotation 0
                      [(0, 0, 2), (3, 1, 2), (9, 0, 2)],      # longest edge v2v0: rotation 1
                      [(0, 0, 4), (9, 0, 4), (4, 1, 4)]], dtype=np.float64)  # longest edge v0v1: rotation 2
    first, n = b.triangles(tri, grey)
    light = b.Sphere((0.0, 9.0, 0.0), 1.0, b.DiffuseLight(4, 4, 4))
    sc = b.finish(b.Bvh([light] + list(range(first, first + n))), CameraConfig(40.0, 0.0, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0)), (0.0, 0.0, 0.0),
                  RenderConfig(8, 8, 1))
    assert sc.desc.n_triangles == 3
    table = lightmap_triangle_table(sc, 0, 3)
    rotation_of_v0 = {0.0: 0, 2.0: 1, 4.0: 2}
    seen = set()
    for k in range(3):
        t = sc.desc.triangles[k]
        entry = int(table[t.dfs_index])
        assert entry & sr.TRIANGLE_MASK == k and entry >> 30 == rotation_of_v0[t.v0[2]]
        seen.add(t.dfs_index)
    assert (np.delete(table, sorted(seen)) == sr.NONE).all() and len(table) == max(seen) + 1
    part = lightmap_triangle_table(sc, 1, 2)  # a sub-range: triangle 1 is lightmap triangle 0
    assert int(part[sc.desc.triangles[1].dfs_index]) & sr.TRIANGLE_MASK == 0 and (part != sr.NONE).sum() == 2
    with pytest.raises(ValueError):
        lightmap_triangle_table(sc, 2, 2)
