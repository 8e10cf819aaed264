"""Directional lightmaps (sol_lightmap_sh / sol_lightmap_normals), the part that needs no GPU: the four entry points are exported,
declared and documented, SolLightmapShConfig (32 bytes) has the same size and offsets from gcc and from ctypes, every refusal of both calls
answers SOL_EINVAL in the stated order and in front of the device check with nothing written, the kernels are gfx950 code of the library - and
the restatement the GPU tests compare against (tests/lightmap_sh_ref.py) has the rule's own properties, each within a bound derived here from the
roundings the rule performs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import lightmap_ref as lr
import lightmap_sample_ref as sr
import lightmap_sh_ref as shr
from solstrale_amd import DeviceScene, _abi, device_count, sh9, sh9_irradiance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_sh_dev", "sol_lightmap_sh", "sol_lightmap_normals_dev", "sol_lightmap_normals")
CFG = _abi.SolLightmapShConfig
CFG_OFFSETS = {"size": 0, "width": 4, "height": 8, "stride_bytes": 12, "flags": 16, "chart_radius": 20, "scale": 24, "reserved": 28}
F = np.float32
EPS = float(np.finfo(F).eps) / 2  # the relative error of one rounding: 2^-24
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
    assert len(lib.sol_lightmap_sh.argtypes) == len(lib.sol_lightmap_sh_dev.argtypes) == 13
    assert len(lib.sol_lightmap_normals.argtypes) == len(lib.sol_lightmap_normals_dev.argtypes) == 7
    for name, value in (("NEAREST", 1), ("COEFFICIENTS", 2), ("CLAMP", 4)):
        assert getattr(_abi, "SOL_LIGHTMAP_SH_" + name) == value and re.search(rf"#define SOL_LIGHTMAP_SH_{name} {value}u", text)
    for method in ("lightmap_sh", "lightmap_normals", "lightmap_view_sh"):
        assert callable(getattr(DeviceScene, method))


def test_the_config_agrees_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(CFG) == 32
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == CFG_OFFSETS
    fields = ", ".join(f"(unsigned)offsetof(SolLightmapShConfig, {n})" for n in CFG_OFFSETS)
    count = 1 + len(CFG_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolLightmapShConfig), {fields});\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32] + list(CFG_OFFSETS.values())


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, stride_bytes=112, flags=0, chart_radius=INF, scale=1.0, reserved=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_every_refusal_of_lightmap_sh_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of the device check reads the handle. Each bad argument is
    paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    uvs, vertices, texels, pass_of = (C.c_float * 12)(), (C.c_float * 18)(), (C.c_uint32 * 64)(), (C.c_uint8 * 16)()
    values, points, coords, normals, out = (C.c_float * (16 * 28))(), (C.c_float * 128)(), (C.c_uint32 * 8)(), (C.c_float * 8)(), (C.c_float * 56)()
    good = dict(scene=stand_in, c={}, uvs=uvs, nt=2, texels=texels, values=values, vertices=None, points=None, coords=coords, normals=normals, n=2, out=out)
    # (what to break - "c": fields of the configuration -, the word sol_last_error must hold), in the header's order
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=28)), b"size"),
             (dict(c=dict(reserved=1)), b"reserved"), (dict(c=dict(flags=8)), b"unknown bits"), (dict(c=dict(flags=6)), b"SOL_LIGHTMAP_SH_CLAMP with"),
             (dict(c=dict(width=0)), b"atlas"), (dict(c=dict(height=16385)), b"atlas"), (dict(c=dict(stride_bytes=96)), b"stride"),
             (dict(c=dict(stride_bytes=116)), b"stride"), (dict(c=dict(chart_radius=NAN)), b"chart_radius"), (dict(c=dict(chart_radius=0.0)), b"chart_radius"),
             (dict(c=dict(chart_radius=-1.0)), b"chart_radius"), (dict(vertices=vertices), b"go together"), (dict(points=points), b"go together"),
             (dict(c=dict(chart_radius=0.5)), b"needs the guard arrays"), (dict(c=dict(scale=INF)), b"scale"), (dict(c=dict(scale=NAN)), b"scale"),
             (dict(nt=(1 << 31) - 1), b"2^31 - 2"), (dict(n=(1 << 31) + 1), b"at most 2^31)"), (dict(uvs=None), b"null UV"), (dict(texels=None), b"null texel"),
             (dict(values=None), b"null value"), (dict(coords=None), b"null coordinate"), (dict(normals=None), b"null normals"),
             (dict(out=None), b"null output"), (dict(out=values), b"out may not be values"), (dict(out=coords), b"out may not be coords"),
             (dict(out=normals), b"out may not be normals")]
    for name in ("sol_lightmap_sh", "sol_lightmap_sh_dev"):
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
            return fn(a["scene"], cfg, a["uvs"], a["nt"], a["texels"], pass_of, a["values"], a["vertices"], a["points"], a["coords"], a["normals"], a["n"],
                      a["out"])

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
        # coefficient mode reads no normal and looks at no scale; a finite radius with both arrays is no fault; n == 0 succeeds before the device is
        # looked for; n_triangles == 0 needs no UV pointer
        assert call({**good, "n": 0}) == _abi.SOL_OK
        assert call({**good, "n": 0, "normals": None, "c": dict(flags=2, scale=NAN)}) == _abi.SOL_OK
        assert call({**good, "n": 0, "normals": None, "c": dict(flags=3, scale=INF, stride_bytes=128)}) == _abi.SOL_OK
        assert call({**good, "n": 0, "nt": 0, "uvs": None, "vertices": vertices, "points": points, "c": dict(chart_radius=0.5, flags=5)}) == _abi.SOL_OK
        assert call({**good, "n": 0, "c": dict(flags=2), "out": normals}) == _abi.SOL_EINVAL and b"out may not be normals" in err()
        if device_count() == 0:
            assert call({**good, "vertices": vertices, "points": points, "c": dict(chart_radius=0.5)}) == _abi.SOL_EDEVICE
            assert call({**good, "c": dict(flags=5, scale=-2.0)}) == _abi.SOL_EDEVICE
            assert call({**good, "normals": None, "c": dict(flags=2)}) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(224) and bytes(values) == bytes(16 * 112) and bytes(coords) == bytes(32) and bytes(normals) == bytes(32)  # nothing was written


def test_every_refusal_of_lightmap_normals_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    coords, vertices, vertex_normals, out = (C.c_uint32 * 8)(), (C.c_float * 18)(), (C.c_float * 18)(), (C.c_float * 8)()
    good = dict(scene=stand_in, coords=coords, n=2, vertices=vertices, nt=2, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(nt=(1 << 31) - 1), b"2^31 - 2"), (dict(n=(1 << 31) + 1), b"at most 2^31)"),
             (dict(vertices=None), b"null vertex"), (dict(coords=None), b"null coordinate"), (dict(out=None), b"null output"),
             (dict(out=coords), b"out may not be coords")]
    for name in ("sol_lightmap_normals", "sol_lightmap_normals_dev"):
        fn = getattr(lib, name)
        for vn in (None, vertex_normals):
            def call(a):
                return fn(a["scene"], a["coords"], a["n"], a["vertices"], vn, a["nt"], a["out"])

            for k, (broken, word) in enumerate(steps):
                assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
                assert word in err() and name.encode() + b":" in err(), (name, word, err())
                for later, _ in steps[k + 1:]:
                    if set(later) & set(broken):
                        continue
                    assert call({**good, **later, **broken}) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
            assert call({**good, "n": 0}) == _abi.SOL_OK
            if device_count() == 0:
                assert call({**good, "nt": 0, "vertices": None}) == _abi.SOL_EDEVICE  # no triangle needs no pointer
                assert call(good) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(32) and bytes(coords) == bytes(32)  # nothing was written


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    names = set(re.findall(rb"_Z\d+(sol_[a-z0-9_]+_kernel)[A-Za-z0-9_]*\.kd", data))
    assert b"sol_lightmap_sh_kernel" in names and b"sol_lightmap_normals_kernel" in names
    assert len(set(re.findall(rb"_Z\d+sol_lightmap_(?:sh|normals)_kernel[A-Za-z0-9_]*\.kd", data))) == 2  # one shape each


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------------
def _grid_atlas(W=64, H=64):
    V, T, N = lr.grid_mesh(16, GRID_SEED)
    points, texels = lr.lightmap_points(V, T, W, H, normals=N)
    return V, T, N, points, texels


def _random_rows(rng, n_triangles, n):
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
    rows = np.zeros(n, dtype=sr.TEXEL_DTYPE)
    rows["triangle"], rows["b1"], rows["b2"], rows["flags"] = rng.integers(0, n_triangles, n), b[:, 1], b[:, 2], 1
    return rows


def _unit_normals(rng, n):
    d = rng.normal(size=(n, 3))
    out = np.zeros((n, 4), dtype=F)
    out[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    out[:, 3] = 7.0  # (unused)
    return out


def _sh_values(rng, W, H, words=28):
    values = rng.normal(size=(W * H, words)).astype(F)
    values[:, 27] = np.arange(W * H, dtype=np.uint32).view(F)  # (the sample count: not a value)
    return values


def test_the_constants_of_the_restatement_are_the_fp32_roundings():
    assert [float(a).hex() for a in shr.A[:2] + shr.A[4:5]] == [float(F(x)).hex() for x in (np.pi, 2 * np.pi / 3, np.pi / 4)]
    text = open(os.path.join(ROOT, "solstrale-rust_amd", "csrc", "sol_lightmap_sh.h")).read()
    for name, a in (("A0", shr.A[0]), ("A1", shr.A[1]), ("A2", shr.A[4])):
        literal = re.search(rf"#define SOL_LSH_{name} ([0-9.]+)f", text).group(1)
        assert F(literal) == a, (name, literal)  # (numpy parses the decimal with one rounding, as the compiler does)
    d = np.random.default_rng(3).normal(size=(50, 3)).astype(F)
    ours = np.stack(shr.basis(d[:, 0], d[:, 1], d[:, 2]), axis=1)
    assert (ours.view(np.uint32) == sh9(d).view(np.uint32)).all()  # the basis the bake projects onto


def test_coefficient_mode_is_the_27_channel_lookup_word_for_word():
    V, T, N, points, texels = _grid_atlas()
    rng = np.random.default_rng(41)
    rows = _random_rows(rng, len(V), 3000)
    values = _sh_values(rng, 64, 64)
    values[rng.random(64 * 64) < 0.05, 13] = np.inf
    for nearest in (False, True):
        got = shr.lightmap_sh(values, rows, None, T, texels, 64, 64, nearest=nearest, coefficients=True, scale=NAN)
        want = sr.lightmap_sample(values, rows, T, texels, 64, 64, channels=27, nearest=nearest)
        assert got.shape == (3000, 28) and (got.view(np.uint32) == want.view(np.uint32)).all()
        assert set(np.unique(got[:, 27].view(np.uint32))) >= ({0, 1} if nearest else {3, 4})


def test_evaluation_equals_scale_times_sh9_irradiance_within_the_roundings_counted():
    """E is sum_k A_k Y_k L_k times scale. Against float64 over the same fp32 basis and the same fp32 L, the device's chain rounds: the constant
    A_k once (against the exact pi), B_k = A_k * Y_k once, t_k = B_k * L once, each of the nine additions once, the scale once - 13 roundings on the
    way of any one term, each relative to a partial sum that is at most S = sum_k |A_k Y_k L_k|; 16 EPS scale S covers them and the second order."""
    V, T, N, points, texels = _grid_atlas()
    rng = np.random.default_rng(42)
    n = 4000
    rows = _random_rows(rng, len(V), n)
    values = _sh_values(rng, 64, 64) * F(3.0)
    values[:, 27] = 0
    normals = _unit_normals(rng, n)
    normals[n // 2:, :3] *= rng.uniform(0.2, 5.0, (n - n // 2, 1)).astype(F)  # not normalised: taken as they come
    a64 = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    for scale in (1.0, 4 * np.pi / 64, -0.5):
        got = shr.lightmap_sh(values, rows, normals, T, texels, 64, 64, scale=scale)
        coeff = shr.lightmap_sh(values, rows, None, T, texels, 64, 64, coefficients=True)
        L = coeff[:, :27].astype(np.float64).reshape(n, 9, 3)
        count = coeff[:, 27].view(np.uint32)
        assert (got[:, 3].view(np.uint32) == count).all() and (count >= 1).all()
        y = sh9(normals[:, :3]).astype(np.float64)
        want = float(F(scale)) * np.einsum("nk,nkc->nc", y * a64, L)
        for row in (0, n - 1):  # the same through the package's own sh9_irradiance, a row at a time
            assert np.allclose(float(F(scale)) * sh9_irradiance(L[row], normals[row:row + 1, :3])[0], want[row], rtol=1e-12, atol=0)
        S = np.einsum("nk,nkc->nc", np.abs(y * a64), np.abs(L))
        err = np.abs(got[:, :3].astype(np.float64) - want)
        bound = 16 * EPS * abs(float(F(scale))) * S
        print(f"evaluation: scale {scale:.4g}: largest error / bound {np.max(err / bound):.3f}")
        assert (err <= bound).all()


def test_an_atlas_of_the_constant_term_alone_is_the_same_for_every_normal():
    """L_0 = c, every other coefficient 0: the lookup of a constant answers c up to its own roundings (9 EPS, tests/test_lightmap_sample_abi.py), and
    E = ((A_0 * k_0) * L_0 + 0 + ..) * scale whatever the normal - the terms of k >= 1 are products with an exact zero. Word for word for nearest
    rows (L_0 is c exactly); for bilinear rows every normal gives the SAME words, near A_0 k_0 c scale."""
    V, T, N, points, texels = _grid_atlas()
    rng = np.random.default_rng(43)
    n = 2000
    rows = _random_rows(rng, len(V), n)
    c, scale = (0.75, 2.5, 1e-3), 1.7
    values = np.zeros((64 * 64, 28), dtype=F)
    values[:, 0:3] = np.asarray(c, dtype=F)
    values[:, 27] = NAN  # word 27 is no value: never judged
    want = ((shr.A[0] * shr.K[0]) * np.asarray(c, dtype=F)) * F(scale)
    first = None
    for k in range(3):
        normals = _unit_normals(rng, n) * F((1.0, 3.0, 0.01)[k])
        got = shr.lightmap_sh(values, rows, normals, T, texels, 64, 64, scale=scale, nearest=True)
        assert (got[:, 3].view(np.uint32) == 1).all() and (got[:, :3].view(np.uint32) == want.view(np.uint32)).all()
        got = shr.lightmap_sh(values, rows, normals, T, texels, 64, 64, scale=scale)
        assert (np.abs(got[:, :3].astype(np.float64) - want.astype(np.float64)) <= (9 + 3) * EPS * np.abs(want.astype(np.float64))).all()
        first = got if first is None else first
        assert (got.view(np.uint32) == first.view(np.uint32)).all()


def test_the_clamp_zeroes_negatives_and_nan():
    V, T, N, points, texels = _grid_atlas()
    rng = np.random.default_rng(44)
    n = 2000
    rows = _random_rows(rng, len(V), n)
    values = _sh_values(rng, 64, 64)
    values[:, 3:6] = F(3e38)
    values[:, 9:12] = F(-3e38)  # k = 1 and k = 3: B reaches 3 for a normal of length 3, so the two terms overflow and meet as +inf and -inf
    normals = _unit_normals(rng, n) * F(3.0)
    plain = shr.lightmap_sh(values, rows, normals, T, texels, 64, 64, scale=4.0)
    clamped = shr.lightmap_sh(values, rows, normals, T, texels, 64, 64, scale=4.0, clamp=True)
    E = plain[:, :3]
    assert np.isnan(E).any() and (E < 0).any() and (E > 0).any()
    keep = E > 0
    assert (clamped[:, :3][keep].view(np.uint32) == E[keep].view(np.uint32)).all() and (clamped[:, :3][~keep].view(np.uint32) == 0).all()
    assert (clamped[:, 3].view(np.uint32) == plain[:, 3].view(np.uint32)).all()


BAD_NORMALS = [("zero", (0.0, 0.0, 0.0)), ("negative zero", (-0.0, 0.0, -0.0)), ("subnormal words", (1e-40, 0.0, 0.0)), ("a subnormal length", (1e-19, 1e-20, 0.0)),
               ("a length that underflows", (1e-30, 1e-30, 1e-30)), ("a length that overflows", (2e19, 2e19, 0.0)), ("+inf", (INF, 0.0, 0.0)),
               ("-inf", (0.0, -INF, 1.0)), ("NaN", (0.0, 1.0, NAN)), ("NaN first", (NAN, 1.0, 0.0))]


def test_every_class_of_bad_normal_answers_zeros():
    V, T, N, points, texels = _grid_atlas()
    rng = np.random.default_rng(45)
    values = _sh_values(rng, 64, 64)
    rows = _random_rows(rng, len(V), len(BAD_NORMALS) + 2)
    normals = _unit_normals(rng, len(rows))
    for k, (_, nrm) in enumerate(BAD_NORMALS):
        normals[1 + k, :3] = nrm
    normals[:, 3] = NAN  # the fourth word is not looked at
    for nearest in (False, True):
        got = shr.lightmap_sh(values, rows, normals, T, texels, 64, 64, nearest=nearest)
        assert (got[[0, -1], 3].view(np.uint32) >= 1).all() and (got[[0, -1], :3] != 0).all()
        for k, (name, _) in enumerate(BAD_NORMALS):
            assert (got[1 + k].view(np.uint32) == 0).all(), name
    # the smallest normal length is served: 2^-63 squared is 2^-126
    normals[1, :3] = (2.0 ** -63, 0.0, 0.0)
    assert shr.lightmap_sh(values, rows, normals, T, texels, 64, 64)[1, 3].view(np.uint32) >= 1


def test_the_normals_of_the_texel_rows_are_the_point_rows_normals():
    for W, H in ((64, 64), (37, 19)):
        V, T, N = lr.grid_mesh(16, GRID_SEED)
        N = N.copy()
        N[5] = 0.0           # vertex normals without length: the geometric normal serves
        N[6, 0] = (0, 0, 1)
        N[6, 1] = (0, 0, -1)  # they cancel somewhere inside the triangle
        for normals in (None, N):
            points, texels = lr.lightmap_points(V, T, W, H, normals=normals, conservative=True)
            own = texels["flags"] != 0
            assert own.sum() > 0.9 * W * H
            got = shr.lightmap_normals(texels, V, normals)
            assert (got[own, :3].view(np.uint32) == points[own, 4:7].view(np.uint32)).all() and (got[:, 3].view(np.uint32) == 0).all()
            assert (got[~own].view(np.uint32) == 0).all()
    # conservative texels (renormalised weights), on a mesh with gaps
    V, T, N = lr.grid_mesh(16, GRID_SEED)
    V, T, N = V[::3], T[::3], N[::3]
    points, texels = lr.lightmap_points(V, T, 64, 64, normals=N, conservative=True)
    own = texels["flags"] != 0
    assert (texels["flags"] == 2).sum() > 100 and (~own).sum() > 100
    got = shr.lightmap_normals(texels, V, N)
    assert (got[own, :3].view(np.uint32) == points[own, 4:7].view(np.uint32)).all() and (got[~own].view(np.uint32) == 0).all()
    # what answers zeros
    rows = np.zeros(8, dtype=sr.TEXEL_DTYPE)
    rows["b1"], rows["b2"], rows["flags"] = 0.25, 0.25, 1
    rows["triangle"] = [0, 1, 2, 3, sr.NONE, 4, 0, 0]
    rows["flags"][6], rows["b1"][7] = 0, NAN
    V = lr.lift(np.asarray([[(0, 0), (1, 0), (0, 1)]] * 4, dtype=F))
    V[1, 2, 1] = NAN                        # a vertex word that is not finite
    V[2] = V[2] * F(1e-12)                  # a geometric normal whose squared length underflows
    Nv = np.zeros((4, 3, 3), dtype=F)
    Nv[..., 2] = 1
    got = shr.lightmap_normals(rows, V, None)
    assert (got[0, :3] != 0).any() and (got[3, :3] != 0).any() and (got[[1, 2, 4, 5, 6, 7]].view(np.uint32) == 0).all()
    Nv[3, 0, 0] = INF                       # a normal word that is not finite
    got = shr.lightmap_normals(rows, V, Nv)
    assert (got[[0, 2], :3] == (0, 0, 1)).all() and (got[[1, 3, 4, 5, 6, 7]].view(np.uint32) == 0).all()  # (triangle 2: the vertex normals have a length)
