"""Lightmap mip chains (sol_lightmap_mip_layout / sol_lightmap_mips / sol_lightmap_sample_lod / sol_lightmap_lod), the part that needs
no GPU: the entry points are exported, declared and documented, SolLightmapLodConfig (40 bytes) has the same size and offsets from gcc and from
ctypes, every refusal of every call answers SOL_EINVAL in the stated order and in front of the device check with nothing written, the layout
agrees between C, Python and the restatement, the kernels are gfx950 code of the library - and the restatement the GPU tests compare against
(tests/lightmap_mips_ref.py) has the rule's own properties."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import lightmap_mips_ref as mr
import lightmap_ref as lr
import lightmap_sample_ref as sr
from solstrale_amd import DeviceScene, _abi, device_count, lightmap_mip_layout, pixel_spread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_mips_dev", "sol_lightmap_mips", "sol_lightmap_sample_lod_dev", "sol_lightmap_sample_lod", "sol_lightmap_lod_dev",
                "sol_lightmap_lod")
CFG = _abi.SolLightmapLodConfig
CFG_OFFSETS = {"size": 0, "width": 4, "height": 8, "channels": 12, "stride_bytes": 16, "flags": 20, "chart_radius": 24, "levels": 28, "reserved": 32}
F = np.float32
EPS = float(np.finfo(F).eps) / 2  # the relative error of one rounding: 2^-24
INF, NAN = float("inf"), float("nan")
LAYOUT_SIZES = [(1, 1), (2, 2), (3, 3), (5, 3), (300, 1), (130, 67), (16384, 16384)]


def test_the_entry_points_are_exported_declared_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene,", text), name
        assert re.search(r"\b" + name + r"\b", guide), name
    assert hasattr(lib, "sol_lightmap_mip_layout") and "sol_lightmap_mip_layout" in _abi.HIP_SYMBOLS
    assert re.search(r"\bint sol_lightmap_mip_layout\(uint32_t width,", text) and "sol_lightmap_mip_layout" in guide
    assert len(lib.sol_lightmap_mips.argtypes) == len(lib.sol_lightmap_mips_dev.argtypes) == 11
    assert len(lib.sol_lightmap_sample_lod.argtypes) == len(lib.sol_lightmap_sample_lod_dev.argtypes) == 15
    assert len(lib.sol_lightmap_lod.argtypes) == len(lib.sol_lightmap_lod_dev.argtypes) == 13
    assert _abi.SOL_LIGHTMAP_MAX_LEVELS == 15 and re.search(r"#define SOL_LIGHTMAP_MAX_LEVELS 15u", text)
    for method in ("lightmap_mips", "lightmap_sample_lod", "lightmap_lod", "lightmap_view_lod"):
        assert callable(getattr(DeviceScene, method))
    assert "levels up to" in text and "gutter" in text  # the chart caveat is stated where the caller reads it
    assert abs(pixel_spread(90.0, 100) - 0.02) < 1e-12 and pixel_spread(40.0, 1080) > 0


def test_the_config_agrees_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(CFG) == 40
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == CFG_OFFSETS
    fields = ", ".join(f"(unsigned)offsetof(SolLightmapLodConfig, {n})" for n in CFG_OFFSETS)
    count = 1 + len(CFG_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolLightmapLodConfig), {fields});\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [40] + list(CFG_OFFSETS.values())


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    names = set(re.findall(rb"_Z\d+(sol_[a-z0-9_]+_kernel)[A-Za-z0-9_]*\.kd", data))
    for k in (b"sol_lightmap_mips_level_kernel", b"sol_lightmap_mips_tail_kernel", b"sol_lightmap_sample_lod_kernel", b"sol_lightmap_lod_kernel"):
        assert k in names, k


# ---- the layout ---------------------------------------------------------------------------------------------------------------------------
def _c_layout(W, H, levels):
    lib = _abi.load_hip()
    n, total = C.c_uint32(99), C.c_uint64(99)
    w, h, at = (C.c_uint32 * 15)(), (C.c_uint32 * 15)(), (C.c_uint64 * 15)()
    rc = lib.sol_lightmap_mip_layout(W, H, levels, C.byref(n), w, h, at, C.byref(total))
    return rc, n.value, list(w), list(h), list(at), total.value


def test_the_layout_agrees_between_c_python_and_the_restatement():
    lib = _abi.load_hip()
    for W, H in LAYOUT_SIZES:
        full = mr.mip_layout(W, H)[0]
        assert full == max(W - 1, H - 1).bit_length() + 1
        for levels in sorted({0, 1, 2, full}):
            if levels > full:
                continue
            rc, n, w, h, at, total = _c_layout(W, H, levels)
            assert rc == _abi.SOL_OK
            py = lightmap_mip_layout(W, H, levels or None)
            ref = mr.mip_layout(W, H, levels or None)
            assert (n, w[:n], h[:n], at[:n], total) == (py["levels"], py["widths"], py["heights"], py["offsets"], py["rows"]) == ref
            assert w[n:] == [0] * (15 - n) and h[n:] == [0] * (15 - n) and at[n:] == [0] * (15 - n)
            assert (w[0], h[0], at[0]) == (W, H, 0) and (n == 1 or at[1] == 0)
            for l in range(1, n):  # a ceiling: no source texel is dropped; packed without a gap
                assert w[l] == -(-w[l - 1] // 2) and h[l] == -(-h[l - 1] // 2)
                assert at[l] == sum(w[k] * h[k] for k in range(1, l))
            assert total == sum(w[k] * h[k] for k in range(1, n))
            if levels == 0:
                assert (w[n - 1], h[n - 1]) == (1, 1) and (n == 1 or (w[n - 2], h[n - 2]) != (1, 1))
        assert lib.sol_lightmap_mip_layout(W, H, full + 1, None, None, None, None, None) == _abi.SOL_EINVAL and b"levels" in lib.sol_last_error()
        assert lib.sol_lightmap_mip_layout(W, H, 0, None, None, None, None, None) == _abi.SOL_OK  # every out pointer may be null
    assert mr.mip_layout(16384, 16384)[0] == 15 and mr.mip_layout(1, 1) == (1, [1], [1], [0], 0)
    for W, H in ((0, 4), (4, 0), (16385, 1), (1, 16385)):
        assert lib.sol_lightmap_mip_layout(W, H, 0, None, None, None, None, None) == _abi.SOL_EINVAL and b"atlas" in lib.sol_last_error()


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------
def _walk(steps, good, call, names, combine=lambda broken, later: True):
    lib = _abi.load_hip()
    err = lib.sol_last_error
    for name in names:
        for k, (broken, word) in enumerate(steps):
            assert call(name, {**good, **broken, "c": {**good.get("c", {}), **broken.get("c", {})}}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:  # the earlier refusal is the one named
                if (set(later) - {"c"}) & (set(broken) - {"c"}) or set(later.get("c", {})) & set(broken.get("c", {})) or not combine(broken, later):
                    continue
                args = {**good, **later, **broken, "c": {**good.get("c", {}), **later.get("c", {}), **broken.get("c", {})}}
                assert call(name, args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())


def test_every_refusal_of_lightmap_mips_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    texels, pass_of, values = (C.c_uint32 * 64)(), (C.c_uint8 * 16)(), (C.c_float * 64)()
    mips, cover = (C.c_float * 32)(), (C.c_uint8 * 8)()
    good = dict(scene=stand_in, texels=texels, pass_of=pass_of, w=4, h=4, values=values, ch=3, stride=16, levels=0, mips=mips, cover=cover)
    steps = [(dict(scene=None), b"null scene"), (dict(w=0), b"atlas"), (dict(h=16385), b"atlas"), (dict(ch=0), b"channels"), (dict(ch=33), b"channels"),
             (dict(stride=10), b"stride"), (dict(stride=8), b"stride"), (dict(levels=4), b"levels"), (dict(texels=None), b"null texel"),
             (dict(values=None), b"null value"), (dict(mips=None), b"null chain"), (dict(cover=None), b"null cover"),
             (dict(mips=values), b"mips_out may not be values"), (dict(mips=texels), b"mips_out may not be texels"),
             (dict(cover=values), b"cover_out may not be values"), (dict(cover=pass_of), b"cover_out may not be pass_of")]

    def call(name, a):
        return getattr(lib, name)(a["scene"], a["texels"], a["pass_of"], a["w"], a["h"], a["values"], a["ch"], a["stride"], a["levels"], a["mips"], a["cover"])

    def combine(broken, later):  # (a null value pointer is no alias of a null output)
        return not ({"values", "texels"} & set(broken) and {"mips", "cover"} & set(later))

    _walk(steps, good, call, ("sol_lightmap_mips", "sol_lightmap_mips_dev"), combine)
    for name in ("sol_lightmap_mips", "sol_lightmap_mips_dev"):
        assert call(name, {**good, "levels": 1, "mips": None, "cover": None}) == _abi.SOL_OK  # one level: nothing to make, no device looked for
        assert call(name, {**good, "w": 1, "h": 1, "mips": None, "cover": None}) == _abi.SOL_OK
        if device_count() == 0:
            assert call(name, good) == _abi.SOL_EDEVICE
            assert call(name, {**good, "pass_of": None, "levels": 3}) == _abi.SOL_EDEVICE
    assert bytes(mips) == bytes(128) and bytes(cover) == bytes(8) and bytes(values) == bytes(256) and err() is not None  # nothing was written


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, channels=3, stride_bytes=16, flags=0, chart_radius=INF, levels=0)
    for k, v in kw.items():
        if k == "reserved":
            c.reserved[1] = v
        else:
            setattr(c, k, v)
    return c


def test_every_refusal_of_lightmap_sample_lod_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    uvs, vertices, texels, pass_of = (C.c_float * 12)(), (C.c_float * 18)(), (C.c_uint32 * 64)(), (C.c_uint8 * 16)()
    values, mips, cover, points = (C.c_float * 64)(), (C.c_float * 32)(), (C.c_uint8 * 8)(), (C.c_float * 128)()
    coords, lods, out = (C.c_uint32 * 8)(), (C.c_float * 2)(), (C.c_float * 8)()
    good = dict(scene=stand_in, c={}, uvs=uvs, nt=2, texels=texels, values=values, mips=mips, cover=cover, vertices=None, points=None, coords=coords, lods=lods,
                n=2, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=32)), b"size"),
             (dict(c=dict(reserved=1)), b"reserved"), (dict(c=dict(flags=1)), b"unknown bits"), (dict(c=dict(width=0)), b"atlas"),
             (dict(c=dict(height=16385)), b"atlas"), (dict(c=dict(channels=33)), b"channels"), (dict(c=dict(stride_bytes=8)), b"stride"),
             (dict(c=dict(chart_radius=NAN)), b"chart_radius"), (dict(c=dict(chart_radius=-1.0)), b"chart_radius"), (dict(vertices=vertices), b"go together"),
             (dict(points=points), b"go together"), (dict(c=dict(chart_radius=0.5)), b"needs the guard arrays"), (dict(c=dict(levels=4)), b"levels"),
             (dict(nt=(1 << 31) - 1), b"2^31 - 2"), (dict(n=(1 << 31) + 1), b"at most 2^31)"), (dict(uvs=None), b"null UV"), (dict(texels=None), b"null texel"),
             (dict(values=None), b"null value"), (dict(coords=None), b"null coordinate"), (dict(lods=None), b"null lod"), (dict(out=None), b"null output"),
             (dict(mips=None), b"null chain"), (dict(cover=None), b"null cover"), (dict(out=values), b"out may not be values"),
             (dict(out=coords), b"out may not be coords"), (dict(out=lods), b"out may not be lods"), (dict(out=mips), b"out may not be mips")]

    def call(name, a):
        cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
        return getattr(lib, name)(a["scene"], cfg, a["uvs"], a["nt"], a["texels"], pass_of, a["values"], a["mips"], a["cover"], a["vertices"], a["points"],
                                  a["coords"], a["lods"], a["n"], a["out"])

    def combine(broken, later):
        if {"vertices", "points"} & set(broken) and {"vertices", "points"} & set(later):
            return False  # (both given is no fault)
        if {"width", "height"} & set(broken.get("c", {})) or {"width", "height"} & set(later.get("c", {})):
            return "levels" not in later.get("c", {}) and "levels" not in broken.get("c", {})
        return True

    _walk(steps, good, call, ("sol_lightmap_sample_lod", "sol_lightmap_sample_lod_dev"), combine)
    for name in ("sol_lightmap_sample_lod", "sol_lightmap_sample_lod_dev"):
        assert call(name, {**good, "n": 0}) == _abi.SOL_OK
        assert call(name, {**good, "n": 0, "mips": None, "cover": None, "c": dict(levels=1)}) == _abi.SOL_OK  # one level needs no chain
        assert call(name, {**good, "n": 0, "nt": 0, "uvs": None, "vertices": vertices, "points": points, "c": dict(chart_radius=0.5)}) == _abi.SOL_OK
        if device_count() == 0:
            assert call(name, good) == _abi.SOL_EDEVICE
            assert call(name, {**good, "mips": None, "cover": None, "c": dict(levels=1)}) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(32) and bytes(values) == bytes(256) and bytes(mips) == bytes(128) and bytes(lods) == bytes(8)  # nothing was written


def test_every_refusal_of_lightmap_lod_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    rays, hits, coords, vertices, uvs, out = (C.c_float * 16)(), (C.c_uint32 * 16)(), (C.c_uint32 * 8)(), (C.c_float * 18)(), (C.c_float * 12)(), (C.c_float * 2)()
    good = dict(scene=stand_in, rays=rays, hits=hits, coords=coords, n=2, vertices=vertices, uvs=uvs, nt=2, w=4, h=4, spread=0.01, bias=0.0, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(w=0), b"atlas"), (dict(h=16385), b"atlas"), (dict(spread=0.0), b"spread"), (dict(spread=-1.0), b"spread"),
             (dict(spread=INF), b"spread"), (dict(spread=NAN), b"spread"), (dict(bias=INF), b"bias"), (dict(bias=NAN), b"bias"),
             (dict(nt=(1 << 31) - 1), b"2^31 - 2"), (dict(n=(1 << 31) + 1), b"at most 2^31)"), (dict(vertices=None), b"null vertex"), (dict(uvs=None), b"null UV"),
             (dict(rays=None), b"null ray"), (dict(hits=None), b"null hit"), (dict(coords=None), b"null coordinate"), (dict(out=None), b"null output"),
             (dict(out=rays), b"out may not be rays"), (dict(out=hits), b"out may not be hits"), (dict(out=coords), b"out may not be coords")]

    def call(name, a):
        return getattr(lib, name)(a["scene"], a["rays"], a["hits"], a["coords"], a["n"], a["vertices"], a["uvs"], a["nt"], a["w"], a["h"], a["spread"], a["bias"],
                                  a["out"])

    _walk(steps, good, call, ("sol_lightmap_lod", "sol_lightmap_lod_dev"))
    for name in ("sol_lightmap_lod", "sol_lightmap_lod_dev"):
        assert call(name, {**good, "n": 0}) == _abi.SOL_OK
        assert call(name, {**good, "n": 0, "bias": -3.5}) == _abi.SOL_OK
        if device_count() == 0:
            assert call(name, good) == _abi.SOL_EDEVICE
            assert call(name, {**good, "nt": 0, "vertices": None, "uvs": None}) == _abi.SOL_EDEVICE  # no triangle needs no pointer
    assert bytes(out) == bytes(8) and bytes(rays) == bytes(64) and bytes(hits) == bytes(64) and bytes(coords) == bytes(32)  # nothing was written


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------------
def _grid_atlas(W, H, seed=1):
    V, T, N = lr.grid_mesh(8, seed)
    points, texels = lr.lightmap_points(V, T, W, H, normals=N)
    return V, T, points, texels


def _random_rows(rng, n_triangles, n):
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
    rows = np.zeros(n, dtype=sr.TEXEL_DTYPE)
    rows["triangle"], rows["b1"], rows["b2"], rows["flags"] = rng.integers(0, n_triangles, n), b[:, 1], b[:, 2], 1
    return rows


def test_a_constant_atlas_answers_the_constant_at_every_level_and_lod():
    """A power of two k: a sum of c <= 4 copies, c k, is exact and (c k) / c is k, so every level holds k. In a lookup, scaling by a power of two
    commutes with every rounding: sum = sum_t (w_t k) carries the roundings of wsum = sum_t w_t times k, and sum / wsum = k exactly. The blend
    (k g) + (k f) with g = 1 - f is k (g + f), and g + f = 1 exactly where 1 - f was exact - it is for the lods used here, multiples of 1/8.
    For another constant x every level's mean errs by one rounding per added tap and one of the division, 4 EPS |x| a level to first order; a
    lookup adds at most 4 products, 3 sums, 3 sums of weights and a division, 11 EPS, and a blend 3 more: the bound used is
    (4 l_max + 14) EPS |x| (1 + 32 EPS) over levels up to l_max."""
    W, H = 37, 22
    V, T, points, texels = _grid_atlas(W, H)
    rng = np.random.default_rng(7)
    rows = _random_rows(rng, len(V), 600)
    lods = rng.choice(np.arange(0, 8 * 7) / 8.0, 600).astype(F)
    texels = texels.copy()
    texels["triangle"][rng.random(W * H) < 0.2] = sr.NONE  # holes: the constant must not be diluted by them
    n_levels = mr.mip_layout(W, H)[0]
    for x, exact in ((0.25, True), (-8.0, True), (0.7, False), (1234.567, False)):
        values = np.full((W * H, 4), x, dtype=F)
        values[:, 3] = np.uint32(5).view(F)
        mips, cover = mr.lightmap_mips(values, texels, W, H)
        got = mr.lightmap_sample_lod(values, mips, cover, lods, rows, T, texels, W, H)
        count = got[:, 3].view(np.uint32)
        assert (count > 0).mean() > 0.9 and set(np.unique(count)) <= set(range(9))
        hit = count > 0
        bound = 0.0 if exact else (4 * (n_levels - 1) + 14) * EPS * abs(x) * (1 + 32 * EPS)
        assert np.abs(got[hit, :3].astype(np.float64) - float(F(x))).max() <= bound, (x, np.abs(got[hit, :3].astype(np.float64) - float(F(x))).max(), bound)
        assert np.abs(mips[cover == 0, :3].astype(np.float64) - float(F(x))).max() <= bound
        assert (mips[cover == 0, 3].view(np.uint32) == 5).all() and (mips[cover == 255].view(np.uint32) == 0).all()  # the words behind the channels
        assert (got[~hit].view(np.uint32) == 0).all()
    assert cover[-1] == 0  # the last level is one covered texel


def test_an_uncovered_or_nan_texel_never_reaches_a_coarser_level_or_a_lookup():
    W, H = 33, 18
    V, T, points, texels = _grid_atlas(W, H, seed=2)
    rng = np.random.default_rng(9)
    owned = texels["triangle"] != sr.NONE
    values = np.ones((W * H, 3), dtype=F)
    values[~owned] = 1e30  # poison where nothing is covered
    poison = owned & (rng.random(W * H) < 0.15)
    values[poison, rng.integers(0, 3, int(poison.sum()))] = rng.choice([np.inf, -np.inf, np.nan], int(poison.sum()))
    mips, cover = mr.lightmap_mips(values, texels, W, H, channels=3)
    assert set(np.unique(cover)) == {0, 255}
    assert (mips[cover == 0] == 1.0).all() and (mips[cover == 255].view(np.uint32) == 0).all()
    # a destination is covered exactly when one of its level-0 texels is live
    n, ws, hs, at, total = mr.mip_layout(W, H)
    live0 = (owned & np.isfinite(values).all(axis=1)).reshape(H, W)
    for l in range(1, n):
        want = np.zeros((hs[l], ws[l]), dtype=bool)
        for j in range(H):
            for i in range(W):
                want[j >> l, i >> l] |= live0[j, i]
        assert ((cover[at[l]:at[l] + ws[l] * hs[l]] == 0).reshape(hs[l], ws[l]) == want).all(), l
    rows = _random_rows(rng, len(V), 500)
    lods = rng.uniform(-1, n, 500).astype(F)
    got = mr.lightmap_sample_lod(values, mips, cover, lods, rows, T, texels, W, H)
    hit = got[:, 3].view(np.uint32) > 0
    assert hit.mean() > 0.9 and np.abs(got[hit, :3] - 1.0).max() <= 14 * EPS and (got[~hit].view(np.uint32) == 0).all()
    # a sum that overflows leaves an uncovered zero row, and the level above does not see it
    big = np.full((4, 1), 3e38, dtype=F)
    t4 = np.zeros(4, dtype=sr.TEXEL_DTYPE)
    m, c = mr.lightmap_mips(big, t4, 2, 2, channels=1)
    assert c.tolist() == [255] and m.view(np.uint32).tolist() == [[0]]
    m, c = mr.lightmap_mips(np.concatenate([big, big]).reshape(8, 1), np.zeros(8, dtype=sr.TEXEL_DTYPE), 4, 2, channels=1)
    assert c.tolist() == [255, 255, 255]


def test_lod_at_most_zero_is_the_plain_lookup_and_integral_lods_are_lookups_of_the_level():
    W, H = 64, 64  # powers of two, square: W_l = W 2^-l exactly at every level (a size held at 1 while the other still halves is no such level)
    V, T, points, texels = _grid_atlas(W, H, seed=3)
    rng = np.random.default_rng(11)
    rows = _random_rows(rng, len(V), 800)
    values = rng.normal(size=(W * H, 4)).astype(F)
    values[rng.random(W * H) < 0.05, 1] = np.nan
    pass_of = np.where(texels["triangle"] != sr.NONE, 0, rng.choice([1, 255], W * H)).astype(np.uint8)
    for po in (None, pass_of):
        mips, cover = mr.lightmap_mips(values, texels, W, H, pass_of=po)
        plain = sr.lightmap_sample(values, rows, T, texels, W, H, pass_of=po)
        for lod in (-3.0, -0.0, 0.0, NAN, -INF):
            got = mr.lightmap_sample_lod(values, mips, cover, np.full(800, lod, dtype=F), rows, T, texels, W, H, pass_of=po)
            assert (got.view(np.uint32) == plain.view(np.uint32)).all(), lod
        got = mr.lightmap_sample_lod(values, None, None, np.full(800, 2.5, dtype=F), rows, T, texels, W, H, pass_of=po, levels=1)
        assert (got.view(np.uint32) == plain.view(np.uint32)).all()
        n, ws, hs, at, total = mr.mip_layout(W, H)
        none = np.zeros(1, dtype=sr.TEXEL_DTYPE)
        for l in range(1, n):
            lo, hi = at[l], at[l] + ws[l] * hs[l]
            level = sr.lightmap_sample(mips[lo:hi], rows, T, np.resize(none, hi - lo), ws[l], hs[l], pass_of=cover[lo:hi])
            for lod in ((float(l),) if l < n - 1 else (float(l), l + 0.5, 99.0, INF)):
                got = mr.lightmap_sample_lod(values, mips, cover, np.full(800, lod, dtype=F), rows, T, texels, W, H, pass_of=po)
                assert (got.view(np.uint32) == level.view(np.uint32)).all(), (l, lod)


def test_the_count_word_in_each_of_the_five_blend_cases():
    """A 4 x 4 atlas of one chart over all of [0, 1]^2; the rows look at its middle, u = v = 0.5: level 0's four taps are texels (1..2, 1..2), level
    1's (0..1, 0..1) - all of level 1."""
    W = H = 4
    T = np.asarray([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], dtype=F)
    row = np.zeros(1, dtype=sr.TEXEL_DTYPE)
    row["triangle"], row["b1"], row["b2"], row["flags"] = 0, 0.0, 0.5, 1  # (u, v) = (0.5, 0.5)
    texels = np.zeros(16, dtype=sr.TEXEL_DTYPE)
    values = np.arange(16, dtype=F).reshape(16, 1) + 1
    mips, cover = mr.lightmap_mips(values, texels, W, H, channels=1)
    assert cover.tolist() == [0] * 5

    def look(lod, values=values, mips=mips, cover=cover, row=row):
        return mr.lightmap_sample_lod(values, mips, cover, np.asarray([lod], dtype=F), row, T, texels, W, H, channels=1)[0]

    centre0 = F(np.mean([6, 7, 10, 11]))
    level1 = mr.lightmap_mips(values, texels, W, H, channels=1)[0][:4, 0]
    centre1 = F(level1.mean())
    one = look(1.0)  # 1. f == 0: the level alone
    assert one[0] == centre1 and one[1:].view(np.uint32)[0] == 4
    both = look(0.25)  # 2. both levels
    assert both[0] == F(F(centre0 * F(0.75)) + F(centre1 * F(0.25))) and both[1:].view(np.uint32)[0] == 8
    gone = cover.copy()
    gone[:4] = 255
    only_a = look(0.25, cover=gone)  # 3. the coarser level has no live tap
    assert only_a[0] == centre0 and only_a[1:].view(np.uint32)[0] == 4
    nans = values.copy()
    nans[[5, 6, 9, 10]] = np.nan
    only_b = look(0.25, values=nans)  # 4. the finer level has none (the chain is the clean atlas's)
    assert only_b[0] == centre1 and only_b[1:].view(np.uint32)[0] == 4
    neither = look(0.25, values=nans, cover=gone)  # 5. neither
    assert neither.view(np.uint32).tolist() == [0, 0]
    bad = row.copy()
    bad["flags"] = 0
    assert look(0.25, row=bad).view(np.uint32).tolist() == [0, 0]  # an invalid row
    three = nans.copy()
    three[[6, 9, 10]] = values[[6, 9, 10]]  # one tap of level 0 is NaN: 3 + 4
    assert look(0.5, values=three)[1:].view(np.uint32)[0] == 7


def test_plog2_is_exact_at_powers_of_two_monotone_and_continuous():
    k = np.arange(-126, 128)
    assert (mr.plog2(np.ldexp(F(1), k).astype(F)) == k.astype(F)).all()
    q = np.sort(np.concatenate([np.exp(np.random.default_rng(1).uniform(-20, 40, 20000)).astype(F), np.ldexp(F(1), np.arange(-10, 30)).astype(F)]))
    p = mr.plog2(q)
    assert (np.diff(p) >= 0).all()
    assert np.abs(p.astype(np.float64) - np.log2(q.astype(np.float64))).max() < 0.0861  # the chord lies below log2 by at most 0.08607
    below = np.nextafter(np.ldexp(F(1), np.arange(-5, 20)).astype(F), F(0))
    assert np.abs(mr.plog2(below) - np.arange(-5, 20)).max() < 1e-6  # continuous across an exponent step
    assert mr.plog2(F(3.0)) == F(1.5) and mr.plog2(F(np.inf)) == F(128)


def _one_hit(t=4.0, d=(0.0, -1.0, 0.0), tri_scale=1.0, uv_scale=1.0):
    rays = np.asarray([[0, 4, 0, 1e-3, d[0], d[1], d[2], np.inf]], dtype=F)
    hits = np.zeros(1, dtype=sr.HIT_DTYPE)
    hits["t"], hits["status"], hits["kind"] = t, 1, sr.REF_TRIANGLE
    coords = np.zeros(1, dtype=sr.TEXEL_DTYPE)
    coords["flags"], coords["b1"], coords["b2"] = 1, 0.25, 0.25
    V = (np.asarray([[(0, 0, 0), (0, 0, 1), (1, 0, 0)]], dtype=F) * F(tri_scale))  # normal +y, doubled area tri_scale^2
    T = (np.asarray([[(0, 0), (0, 1), (1, 0)]], dtype=F) * F(uv_scale))
    return rays, hits, coords, V, T


def test_lightmap_lod_follows_the_distance_the_angle_and_every_invalid_class():
    W = H = 256
    rays, hits, coords, V, T = _one_hit()
    # head on, a unit triangle over the whole atlas: q = (s t)^2 W H, lambda = log2(s t W) at powers of two
    spread = 2.0 ** -6
    got = mr.lightmap_lod(rays, hits, coords, V, T, W, H, spread)
    assert got[0] == F(np.log2(spread * 4 * 256))  # 4: exactly
    # doubling t quadruples q exactly: the exponent moves by 2 and the mantissa bits stay, so plog2 moves by 2 and lambda by exactly 1 - wherever
    # (float)e + m is a representable sum for both. It is when q has few mantissa bits: head on, q = 16 t^2.
    for t in (3.0, 5.0, 6.5, 12.0, 1.0625):
        a = mr.lightmap_lod(*_one_hit(t)[:3], V, T, W, H, spread)
        b = mr.lightmap_lod(*_one_hit(2 * t)[:3], V, T, W, H, spread)
        assert a[0] == F(0.5) * mr.plog2(F(16 * t * t)) > 0 and b[0] == a[0] + F(1), (t, a, b)
    # With a full mantissa the sum (float)e + m is rounded, by at most half an ulp of a number below 32 (q < 2^32), 2^-20, for either t: the two
    # plog2 differ from 2 by at most 2^-19 and the lambdas, their exact halves, from 1 by at most 2^-20 - and by nothing where e and e + 2 lie in
    # one binade.
    rng = np.random.default_rng(4)
    exact = 0
    for _ in range(50):
        d = rng.normal(size=3)
        d[1] = -abs(d[1]) - 0.5
        t = float(rng.uniform(1, 30))
        a = mr.lightmap_lod(*_one_hit(t, d)[:3], V, T, W, H, 0.01)
        b = mr.lightmap_lod(*_one_hit(2 * F(t), d)[:3], V, T, W, H, 0.01)
        assert 0 < a[0] < 15 and abs((float(b[0]) - float(a[0])) - 1.0) <= 2.0 ** -20, (a, b)
        exact += b[0] == a[0] + F(1)
    assert exact >= 10
    # the cosine floor: below a cosine of 1/8 the answer stops growing
    head = mr.lightmap_lod(*_one_hit(4.0, (0, -1, 0))[:3], V, T, W, H, spread)[0]
    graze = [mr.lightmap_lod(*_one_hit(4.0, (np.sqrt(1 - c * c), -c, 0))[:3], V, T, W, H, spread)[0] for c in (0.5, 0.25, 0.125, 0.05, 0.001)]
    assert head < graze[0] < graze[1] < graze[2] and abs(graze[2] - (head + 3)) < 1e-3 and graze[3] == graze[4] and abs(graze[4] - (head + 3)) < 1e-3
    # q <= 1: the bias alone, and nothing below 0
    assert mr.lightmap_lod(rays, hits, coords, V, T, W, H, 1e-6, 0.75)[0] == F(0.75) and mr.lightmap_lod(rays, hits, coords, V, T, W, H, 1e-6, -0.5)[0] == 0
    assert mr.lightmap_lod(rays, hits, coords, V, T, W, H, spread, -20.0)[0] == 0
    # every invalid class answers 0
    for name, (r, h, c, v, t) in invalid_lod_rows().items():
        assert mr.lightmap_lod(r, h, c, v, t, W, H, spread, 1.0)[0] == 0, name
    assert mr.lightmap_lod(rays, hits, coords, V, T, W, H, spread, 1.0)[0] > 1


def invalid_lod_rows():
    """name -> (rays, hits, coords, vertices, uvs) of one row that must answer 0 - shared with the GPU test"""
    out = {}

    def case(name, edit):
        r, h, c, v, t = (a.copy() for a in _one_hit())
        edit(r, h, c, v, t)
        out[name] = (r, h, c, v, t)

    case("a miss", lambda r, h, c, v, t: h.__setitem__("status", 0))
    case("flags == 0", lambda r, h, c, v, t: c.__setitem__("flags", 0))
    case("no triangle", lambda r, h, c, v, t: c.__setitem__("triangle", sr.NONE))
    case("a triangle beyond the mesh", lambda r, h, c, v, t: c.__setitem__("triangle", 1))
    case("t == 0", lambda r, h, c, v, t: h.__setitem__("t", 0.0))
    case("t < 0", lambda r, h, c, v, t: h.__setitem__("t", -1.0))
    case("t NaN", lambda r, h, c, v, t: h.__setitem__("t", np.nan))
    case("t inf", lambda r, h, c, v, t: h.__setitem__("t", np.inf))
    case("a direction word not finite", lambda r, h, c, v, t: r.__setitem__((0, 5), np.nan))
    case("an origin word not finite", lambda r, h, c, v, t: r.__setitem__((0, 0), np.inf))
    case("a vertex word not finite", lambda r, h, c, v, t: v.__setitem__((0, 2, 1), np.nan))
    case("a UV word not finite", lambda r, h, c, v, t: t.__setitem__((0, 1, 0), np.inf))
    case("no world area", lambda r, h, c, v, t: v.__setitem__((0, 2), v[0, 1]))
    case("no texel-space area", lambda r, h, c, v, t: t.__setitem__((0, 2), t[0, 1]))
    return out
