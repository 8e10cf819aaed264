"""Irradiance moments and the variance-guided lightmap filter (sol_irradiance_moments, sol_lightmap_filter_var), the part that needs
no GPU: the four entry points are exported, declared, in HIP_SYMBOLS and in INTEGRATION.md; SolMoments (32 bytes) and SolLightmapFilterVarConfig (64
bytes) have the same size and offsets from gcc -std=c99 -pedantic and from ctypes; every refusal answers SOL_EINVAL in the stated order, in front of
the device check and with nothing written; the kernels are gfx950 code of the library and the radiance families keep their instance counts - and the
restatement the GPU tests compare against (tests/lightmap_filter_var_ref.py) has the properties a variance-guided filter must have."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lightmap_filter_var_ref as vr
import lightmap_ref as lr
from solstrale_amd import MOMENTS_DTYPE, _abi, device_count, moments_mean_variance, moments_to_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
MOMENTS_ENTRY_POINTS = ("sol_irradiance_moments_dev", "sol_irradiance_moments")
FILTER_ENTRY_POINTS = ("sol_lightmap_filter_var_dev", "sol_lightmap_filter_var")
CFG = _abi.SolLightmapFilterVarConfig
CFG_OFFSETS = {"size": 0, "width": 4, "height": 8, "iterations": 12, "normal_power_log2": 16, "sigma_position": 20, "sigma_plane": 24, "sigma_value": 28,
               "variance_floor": 32, "reserved": 36}
MOMENTS_OFFSETS = {"r": 0, "g": 4, "b": 8, "samples": 12, "r2": 16, "g2": 20, "b2": 24, "reserved": 28}
INF, NAN = float("inf"), float("nan")
F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


def test_the_entry_points_are_exported_declared_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in MOMENTS_ENTRY_POINTS + FILTER_ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\b" + name + r"\b", integration), f"INTEGRATION.md does not name {name}"
    for name in MOMENTS_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, const (void|SolRay)\* points", text), name
        assert len(getattr(lib, name).argtypes) == 6
    for name in FILTER_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, const SolLightmapFilterVarConfig\* config,", text), name
        assert len(getattr(lib, name).argtypes) == 7


def test_the_structs_agree_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(CFG) == 64 and C.sizeof(_abi.SolMoments) == 32
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == CFG_OFFSETS
    assert {n: getattr(_abi.SolMoments, n).offset for n, _ in _abi.SolMoments._fields_} == MOMENTS_OFFSETS
    assert MOMENTS_DTYPE.itemsize == 32 and [MOMENTS_DTYPE.fields[n][1] for n in ("sum", "samples", "sum2", "reserved")] == [0, 12, 16, 28]
    fields = ", ".join([f"(unsigned)offsetof(SolLightmapFilterVarConfig, {n})" for n in CFG_OFFSETS] + ["(unsigned)sizeof(SolMoments)"]
                       + [f"(unsigned)offsetof(SolMoments, {n})" for n in MOMENTS_OFFSETS])
    count = 2 + len(CFG_OFFSETS) + len(MOMENTS_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolLightmapFilterVarConfig), {fields});\n  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [64] + list(CFG_OFFSETS.values()) + [32] + list(MOMENTS_OFFSETS.values())


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def _icfg(**kw):
    c = _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=1)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_the_moments_refusals_are_sol_irradiance_s_in_its_order_before_the_device():
    """With or without a GPU: sol_irradiance's refusals, in its order (a null scene, a null configuration, size, samples, first_sample, n, mode, then
    - behind n == 0, which succeeds - the null pointers) and with its words. A zeroed block stands in for a scene: its has_medium byte is 0, and nothing
    else in front of the device check reads the handle (tests/test_gpu_irradiance_moments.py adds the refusal of a scene with a constant medium). Each
    bad argument is paired with every LATER one; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    points, out = (_abi.SolRay * 2)(), (_abi.SolMoments * 2)()
    stand_in = C.create_string_buffer(1 << 20)
    good = dict(scene=stand_in, n=2, c={}, points=points, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=28)), b"size"), (dict(c=dict(samples=0)), b"samples"),
             (dict(c=dict(first_sample=0xFFFFFFF0)), b"first_sample"), (dict(n=(1 << 31) + 1), b"2^31"), (dict(c=dict(mode=2)), b"mode"),
             (dict(points=None), b"null point"), (dict(out=None), b"null output")]
    for name in MOMENTS_ENTRY_POINTS:
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_icfg(**a["c"]))
            return fn(a["scene"], a["points"], None, a["n"], cfg, a["out"])

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, later_word in steps[k + 1:]:
                if (set(later) & set(broken)) - {"c"} or set(later.get("c", {})) & set(broken.get("c", {})) or ("cfg_null" in broken and "c" in later):
                    continue  # (two ways to break the same argument)
                args = {**good, **later, **broken, "c": {**later.get("c", {}), **broken.get("c", {})}}
                assert call(args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        # n == 0 is SOL_OK on any scene: nothing is read behind the scene pointer and nothing is written, whatever the pointers are
        assert call({**good, "n": 0}) == _abi.SOL_OK and call({**good, "n": 0, "points": None, "out": None}) == _abi.SOL_OK, name
        assert call({**good, "n": 0, "scene": None}) == _abi.SOL_EINVAL and b"null scene" in err()
        if device_count() == 0:
            assert call(good) == _abi.SOL_EDEVICE and call({**good, "c": dict(mode=_abi.SOL_IRRADIANCE_SPHERE, samples=40, first_sample=5)}) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(64)  # nothing was written


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, iterations=4, normal_power_log2=5, sigma_position=0.1, sigma_plane=0.1, sigma_value=4.0, variance_floor=1e-12)
    for k, v in kw.items():
        if k == "reserved":
            for i, r in enumerate(v):
                c.reserved[i] = r
        else:
            setattr(c, k, v)
    return c


def test_every_filter_refusal_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of the device check reads the handle. Each bad argument is
    paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    points, texels, moments, out, var = (C.c_float * 128)(), (C.c_uint32 * 64)(), (C.c_float * 128)(), (C.c_float * 64)(), (C.c_float * 64)()
    good = dict(scene=stand_in, c={}, points=points, texels=texels, moments=moments, out=out, var=var)
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=60)), b"size"),
             (dict(c=dict(reserved=(0, 0, 0, 0, 0, 0, 1))), b"reserved"), (dict(c=dict(reserved=(7,))), b"reserved"),
             (dict(c=dict(width=0)), b"atlas"), (dict(c=dict(height=16385)), b"atlas"),
             (dict(c=dict(iterations=0)), b"iterations"), (dict(c=dict(iterations=9)), b"iterations"),
             (dict(c=dict(normal_power_log2=8)), b"normal_power_log2"),
             (dict(c=dict(sigma_position=NAN)), b"sigma_position"), (dict(c=dict(sigma_position=0.9e-6)), b"sigma_position"),
             (dict(c=dict(sigma_plane=0.0)), b"sigma_plane"), (dict(c=dict(sigma_plane=NAN)), b"sigma_plane"),
             (dict(c=dict(sigma_value=-1.0)), b"sigma_value"), (dict(c=dict(sigma_value=NAN)), b"sigma_value"),
             (dict(c=dict(variance_floor=INF)), b"variance_floor"), (dict(c=dict(variance_floor=0.0)), b"variance_floor"),
             (dict(c=dict(variance_floor=NAN)), b"variance_floor"), (dict(c=dict(variance_floor=-1e-12)), b"variance_floor"),
             (dict(points=None), b"null point"), (dict(texels=None), b"null texel"), (dict(moments=None), b"null moments"), (dict(out=None), b"null output"),
             (dict(out=moments), b"out may not be moments"), (dict(var=moments), b"variance_out may not be moments"),
             (dict(var=out), b"variance_out may not be out")]
    for name in FILTER_ENTRY_POINTS:
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
            return fn(a["scene"], cfg, a["points"], a["texels"], a["moments"], a["out"], a["var"])

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, later_word in steps[k + 1:]:  # the earlier refusal is the one named
                if later_word == word or set(later.get("c", {})) & set(broken.get("c", {})) or (set(later) & set(broken)) - {"c"}:
                    continue  # (two ways to break the same argument)
                if broken.get("out", 1) is None and later.get("var") is out:
                    continue  # (variance_out == a null out is no second fault)
                args = {**good, **later, **broken, "c": {**later.get("c", {}), **broken.get("c", {})}}
                assert call(args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        # +inf is a legal sigma and a null variance_out a legal argument: with everything right the call gets as far as the device
        if device_count() == 0:
            assert call({**good, "c": dict(sigma_position=INF, sigma_plane=INF, sigma_value=INF)}) == _abi.SOL_EDEVICE
            assert call({**good, "var": None, "c": dict(sigma_position=1e-6, iterations=8, normal_power_log2=7, variance_floor=1e-30)}) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(256) and bytes(var) == bytes(256) and bytes(moments) == bytes(512)  # nothing was written


def test_the_kernels_are_gfx950_code_of_the_library_and_the_radiance_families_keep_their_counts():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for kernel in (b"sol_moments_project_kernel", b"sol_lightmap_filter_var_prepare_kernel", b"sol_lightmap_filter_var_pass_plain_kernel",
                   b"sol_lightmap_filter_var_pass_staged_kernel"):
        assert kernel in data, kernel
    # the moments query runs the ten per-sample instances as they stand: no new instance of any radiance family
    each = set(re.findall(rb"_Z24sol_radiance_each_kernelILb[01]ELb[01]ELb[01]ELb[01]EE", data))
    gather = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb1EE", data))
    plain = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb0EE", data))
    assert (len(each), len(gather), len(plain)) == (10, 10, 10), (sorted(each), sorted(gather), sorted(plain))
    assert len(set(re.findall(rb"_Z\d+sol_radiance_[a-z_]*kernel\w*", data))) == 30 + 1  # (+ sol_radiance_resolve_kernel)


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------------
def _chart(W, H, origin=(0.0, 0.0, 0.0), normal=(0.0, 1.0, 0.0), texel=0.01, axes=((1, 0, 0), (0, 0, 1))):
    """A flat W x H chart, fully owned: texel (i, j) at origin + i * texel * axes[0] + j * texel * axes[1], one normal."""
    j, i = np.divmod(np.arange(W * H), W)
    points = np.zeros((W * H, 8), dtype=F)
    points[:, 0:3] = (np.asarray(origin)[None, :] + texel * (i[:, None] * np.asarray(axes[0])[None, :] + j[:, None] * np.asarray(axes[1])[None, :])).astype(F)
    points[:, 3], points[:, 4:7], points[:, 7] = 1e-3, np.asarray(normal, dtype=F), np.inf
    texels = np.zeros(W * H, dtype=lr.TEXEL_DTYPE)
    texels["flags"] = 1
    return points, texels


def _side_by_side(a, b):
    (pa, ta, wa, h), (pb, tb, wb, _) = a, b
    p = np.concatenate([pa.reshape(h, wa, 8), pb.reshape(h, wb, 8)], axis=1).reshape(-1, 8)
    t = np.concatenate([ta.reshape(h, wa), tb.reshape(h, wb)], axis=1).reshape(-1)
    return p, t


def _moments(mean, variance, samples):
    """MOMENTS_DTYPE rows whose Prepare gives about (mean, variance) in real arithmetic: sum = N mean, sum2 = N (mean^2 + (N - 1) variance).
    mean, variance: [n, 3] or scalars; samples: [n] or a scalar."""
    mean = np.asarray(mean, dtype=np.float64)
    n = mean.shape[0]
    N = np.broadcast_to(np.asarray(samples, dtype=np.float64), (n,))[:, None]
    rows = np.zeros(n, dtype=MOMENTS_DTYPE)
    rows["sum"] = (N * mean).astype(F)
    rows["sum2"] = (N * (mean ** 2 + (N - 1) * np.asarray(variance, dtype=np.float64))).astype(F)
    rows["samples"] = N[:, 0].astype(np.uint32)
    return rows


def test_a_constant_field_with_zero_squared_deviation_returns_the_constant():
    """Every sample of a texel is the same power of two c (times a count that is a power of two): sum = N c, sum2 = N c^2 and x = c, all exact, so
    (sum2 / N) - (x * x) = 0 and v = 0 exactly. All means are equal: D = 0 and w_v = 1 whatever V is (den >= sigma_value^2 variance_floor > 0). Per
    pass a channel is sum / wsum with at most 25 products and 25 additions of positive terms and one division: within 52 u of a weighted mean of its
    input (tests/test_lightmap_filter_abi.py has the count), so n passes stay within 52 n u of c, and the final product with N is exact (a power of
    two): the bound asserted is 52 x 8 u = 2.5e-5 for every n. The variance stays 0 exactly: every term is w^2 x 0."""
    W, H = 19, 13
    points, texels = _chart(W, H)
    const = np.array([0.5, 2.0, 0.125])
    rows = _moments(np.tile(const, (W * H, 1)), 0.0, 16)
    x, v = moments_mean_variance(rows)
    assert (x == const.astype(F)).all() and (v == 0).all()
    for iterations in (1, 3, 8):
        out, var = vr.lightmap_filter_var(rows, points, texels, W, H, 0.02, iterations=iterations)
        rel = np.abs(out[:, :3].astype(np.float64) / (16 * const) - 1.0).max()
        assert rel <= 52 * 8 * U, (iterations, rel)
        assert (out.view(np.uint32)[:, 3] == 16).all() and (var == 0).all()


def test_with_every_factor_off_one_pass_scales_a_uniform_variance_by_the_sum_of_squared_weights():
    """Equal unit normals give c = 1 and every sigma +inf gives 1 / (1 + 0) = 1 (D and den are finite): w = k exactly. An interior texel has all 25
    taps: wsum = 1 exactly (the products k are dyadic, their partial sums too) and v' = sum (k^2 v) / (1 * 1). The sum of h^2 is 70/256, so v' =
    v (70/256)^2 in real arithmetic; in fp32 k^2 is exact (dyadic, 16 bits), each product k^2 v rounds once and each of the 25 additions of positive
    terms once: within 26 u, and Prepare's v is compared as the restatement computed it."""
    W, H = 11, 9
    points, texels = _chart(W, H)
    rng = np.random.default_rng(7)
    mean = rng.uniform(0.5, 2.0, (W * H, 3))
    rows = _moments(mean, 0.37, 8)
    _, v0 = moments_mean_variance(rows)
    out, var = vr.lightmap_filter_var(rows, points, texels, W, H, INF, sigma_plane=INF, sigma_value=INF, normal_power_log2=0, iterations=1)
    var = var.reshape(H, W, 4)
    v0 = v0.reshape(H, W, 3).astype(np.float64)
    h = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    k2 = np.outer(h, h) ** 2
    assert abs(k2.sum() - (70 / 256) ** 2) < 1e-18
    for j in range(2, H - 2):
        for i in range(2, W - 2):
            want = (k2[:, :, None] * v0[j - 2:j + 3, i - 2:i + 3]).sum(axis=(0, 1))
            assert np.abs(var[j, i, :3] / want - 1).max() <= 26 * U, (i, j)
    # and a variance that is uniform on the bits comes back as v x (70/256)^2 within the same 26 u
    rows = _moments(np.full((W * H, 3), 1.0), 0.25, 4)  # sum = 4, sum2 = 4 (1 + 3 / 4) = 7: v = (7/4 - 1) / 3 = 0.25 exactly
    _, v0 = moments_mean_variance(rows)
    assert (v0 == F(0.25)).all()
    _, var = vr.lightmap_filter_var(rows, points, texels, W, H, INF, sigma_plane=INF, sigma_value=INF, normal_power_log2=0, iterations=1)
    inner = var.reshape(H, W, 4)[2:-2, 2:-2, :3].astype(np.float64)
    assert np.abs(inner / (0.25 * (70 / 256) ** 2) - 1).max() <= 26 * U


def test_scaling_every_sample_by_a_power_of_two_scales_every_output_word_exactly():
    """c_s -> 2^k c_s: sums x 2^k, squared sums and variance_floor x 4^k. Every operation of the rule is then the same operation on scaled operands -
    x and the sums scale by 2^k, v, V, D and den by 4^k, D / den and every weight are unchanged - and scaling by a power of two commutes with fp32
    rounding as long as nothing leaves the normal range, which these magnitudes (1e-3 .. 1e3 before scaling, |k| <= 8) do not. So out scales by 2^k and
    variance_out by 4^k, bit for bit. (sol_lightmap_filter's tone map a / (1 + a) cannot do this.)"""
    W, H = 13, 9
    points, texels = _chart(W, H)
    rng = np.random.default_rng(12)
    c = (rng.uniform(0.0, 1.0, (6, W * H, 3)) ** 4 * 30.0).astype(F)  # heavy-tailed samples
    base = vr.moments_of_samples(c)
    out0, var0 = vr.lightmap_filter_var(base, points, texels, W, H, 0.02, iterations=4, variance_floor=2.0 ** -40)
    assert (out0[:, :3] != base["sum"]).any()
    for k in range(-8, 9):
        rows = base.copy()
        rows["sum"] = base["sum"] * F(2.0 ** k)
        rows["sum2"] = base["sum2"] * F(4.0 ** k)
        out, var = vr.lightmap_filter_var(rows, points, texels, W, H, 0.02, iterations=4, variance_floor=2.0 ** -40 * 4.0 ** k)
        assert ((out0[:, :3] * F(2.0 ** k)).view(np.uint32) == out[:, :3].view(np.uint32)).all(), k
        assert (out.view(np.uint32)[:, 3] == 6).all()
        assert ((var0 * F(4.0 ** k)).view(np.uint32) == var.view(np.uint32)).all(), k


def test_a_unit_step_holds_at_a_small_variance_and_mixes_at_a_large_one():
    """Two half-planes of one flat chart, means 1 and 2, every texel with the same variance v of the mean; the geometry factors are off (+inf; equal
    normals), sigma_value = 4, one pass. All variances are equal, so V = v + floor (the prefilter's weighted mean of equal numbers, within 12 u) and a tap
    across the step has D = 3 (three channels of difference 1): w_v = 1 / (1 + 3 / (16 V))^2.
      v = 1e-6: w_v <= (16 x 1.00001e-6 / 3)^2 < 2.9e-11. A texel's taps across carry at most sum k <= 1 and its own side at least the centre's 9/64,
        so the other side's share is below (64/9) x 2.9e-11 = 2.1e-10 of the step; with the 52 u of one pass's roundings the bound asserted is 1e-5.
      v = 1:    w_v = 1 / (1 + 3/16)^2 = 0.709. A texel in the column next to the step has the columns di = 1, 2 across: kernel weight 5/16, so the
        other side's share is 0.709 x 5/16 / (11/16 + 0.709 x 5/16) = 0.244 of the step; the bound asserted is 0.2."""
    W, H = 12, 8
    points, texels = _chart(W, H)
    mean = np.ones((H, W, 3))
    mean[:, W // 2:] = 2.0
    for variance, check in ((1e-6, "holds"), (1.0, "mixes")):
        rows = _moments(mean.reshape(-1, 3), variance, 4)
        out, _ = vr.lightmap_filter_var(rows, points, texels, W, H, INF, sigma_plane=INF, sigma_value=4.0, normal_power_log2=0, iterations=1)
        got = out[:, :3].astype(np.float64).reshape(H, W, 3) / 4.0
        if check == "holds":
            assert np.abs(got[:, :W // 2] - 1.0).max() <= 1e-5 and np.abs(got[:, W // 2:] - 2.0).max() <= 1e-5
        else:
            assert (got[:, W // 2 - 1] - 1.0 > 0.2).all() and (2.0 - got[:, W // 2] > 0.2).all()


def test_rows_that_are_not_live_come_back_as_stated_and_are_never_taps():
    W, H = 9, 9
    points, texels = _chart(W, H)
    rng = np.random.default_rng(2)
    rows = _moments(rng.uniform(0.1, 2.0, (W * H, 3)), rng.uniform(0.01, 0.5, (W * H, 3)), rng.integers(2, 40, W * H))
    rows["reserved"] = 77  # (not copied: out has four words)
    bad = {"unowned": 4 * W + 4, "position": 2 * W + 2, "normal": 2 * W + 6, "samples 0": 6 * W + 2, "samples 1": 6 * W + 6, "sum nan": 1 * W + 4,
           "sum2 inf": 7 * W + 4, "sum inf": 4 * W + 1, "sum2 nan": 4 * W + 7}
    texels["triangle"][bad["unowned"]] = lr.NONE
    points[bad["position"], 1], points[bad["normal"], 5] = np.inf, np.nan
    rows["samples"][bad["samples 0"]], rows["samples"][bad["samples 1"]] = 0, 1
    rows["sum"][bad["sum nan"], 1], rows["sum2"][bad["sum2 inf"], 2], rows["sum"][bad["sum inf"], 0], rows["sum2"][bad["sum2 nan"], 0] = np.nan, np.inf, -np.inf, np.nan
    out, var = vr.lightmap_filter_var(rows, points, texels, W, H, 0.05, iterations=3)
    dead = list(bad.values())
    keep = np.setdiff1d(np.arange(W * H), dead)
    assert (out.view(np.uint32)[dead] == vr.moments_rows(rows)[dead, :4]).all() and (var.view(np.uint32)[dead] == 0).all()
    assert np.isfinite(out[keep, :3]).all() and (out.view(np.uint32)[keep, 3] == rows["samples"][keep]).all()
    assert (var[keep, :3] > 0).all() and (var.view(np.uint32)[keep, 3] == 0).all()
    assert (out[keep, :3] != rows["sum"][keep]).any()
    # whatever the rows hold, no neighbour reads them
    other = rows.copy()
    other["sum"][dead] = rng.uniform(50.0, 90.0, (len(dead), 3)).astype(F)
    other["sum2"][dead] = rng.uniform(5000.0, 9000.0, (len(dead), 3)).astype(F)
    other["samples"][bad["samples 0"]], other["samples"][bad["samples 1"]] = 1, 0
    other["sum"][bad["sum nan"], 2], other["sum2"][bad["sum2 inf"], 0], other["sum"][bad["sum inf"], 1], other["sum2"][bad["sum2 nan"], 1] = np.inf, np.nan, np.nan, np.inf
    points2 = points.copy()
    points2[bad["position"], 0:3], points2[bad["normal"], 4:7] = (np.nan, 7.0, -np.inf), (np.inf, 0.0, 1.0)
    out2, var2 = vr.lightmap_filter_var(other, points2, texels, W, H, 0.05, iterations=3)
    assert (out.view(np.uint32)[keep] == out2.view(np.uint32)[keep]).all() and (var.view(np.uint32)[keep] == var2.view(np.uint32)[keep]).all()


def test_coplanar_charts_far_apart_in_the_world_do_not_mix():
    """Section 26's case: two coplanar charts, equal normals, neighbours in the atlas, 1e6 x sigma_position apart in the world; the plane factor is
    off by geometry (d = 0) and the value factor by sigma_value = +inf, so that only the distance factor stands between them: a tap across has w_d <=
    1.0001 (f / 1e6)^2 in pass i, f = 2^i, and the share of the other chart over four passes is at most (64/9) x 1.0001 x 85e-12 = 6.1e-10 of the step
    (tests/test_lightmap_filter_abi.py derives it). The roundings of four passes add 4 x 52 u = 1.3e-5 in the worst case, and the final product with N
    one more u; the bound asserted is 1.4e-5."""
    W, H, sigma = 8, 8, 1e-3
    a = _chart(W, H, texel=sigma / 2)
    b = _chart(W, H, origin=(1e6 * sigma, 0.0, 0.0), texel=sigma / 2)
    points, texels = _side_by_side(a + (W, H), b + (W, H))
    ca, cb = 0.7, 2.1
    mean = np.zeros((H, 2 * W, 3))
    mean[:, :W], mean[:, W:] = ca, cb
    rows = _moments(mean.reshape(-1, 3), 0.01, 8)
    x0, _ = moments_mean_variance(rows)
    x0 = x0.astype(np.float64).reshape(H, 2 * W, 3)
    out, _ = vr.lightmap_filter_var(rows, points, texels, 2 * W, H, sigma, sigma_value=INF, iterations=4)
    got = out[:, :3].astype(np.float64).reshape(H, 2 * W, 3) / 8.0
    assert np.abs(got[:, :W] / x0[:, :W] - 1).max() <= 1.4e-5 and np.abs(got[:, W:] / x0[:, W:] - 1).max() <= 1.4e-5
    mixed, _ = vr.lightmap_filter_var(rows, points, texels, 2 * W, H, INF, sigma_value=INF, iterations=4)
    mixed = mixed[:, :3].astype(np.float64).reshape(H, 2 * W, 3) / 8.0
    assert (mixed[:, W - 1] - ca > 0.1 * (cb - ca)).all() and (cb - mixed[:, W] > 0.1 * (cb - ca)).all()


def test_a_one_texel_atlas_returns_its_mean_and_its_variance():
    """The only tap is the centre: a pass answers x' = fl(fl(k x) / k) and v' = fl(fl(fl(k k) v) / fl(k k)) with k = 9/64 - two roundings each (k k =
    81/4096 is exact) -, and the prefilter V plays no part. So n passes answer within 2.01 n u of Prepare's (x, v), and out = x' N adds one rounding."""
    points, texels = _chart(1, 1)
    rng = np.random.default_rng(3)
    for iterations in (1, 8):
        for _ in range(50):
            rows = _moments(rng.uniform(0.1, 7.0, (1, 3)), rng.uniform(0.01, 2.0, (1, 3)), int(rng.integers(2, 100)))
            x, v = moments_mean_variance(rows)
            out, var = vr.lightmap_filter_var(rows, points, texels, 1, 1, 0.02, iterations=iterations)
            N = float(rows["samples"][0])
            assert np.abs(out[0, :3].astype(np.float64) / (x[0].astype(np.float64) * N) - 1).max() <= (2.01 * iterations + 1.01) * U
            assert np.abs(var[0, :3].astype(np.float64) / v[0].astype(np.float64) - 1).max() <= 2.01 * iterations * U
            assert out.view(np.uint32)[0, 3] == rows["samples"][0] and var[0, 3] == 0


def test_moments_mean_variance_is_prepare_word_for_word():
    rng = np.random.default_rng(9)
    n = 400
    rows = np.zeros(n, dtype=MOMENTS_DTYPE)
    rows["sum"] = (rng.uniform(0, 1, (n, 3)) ** 6 * 1e4).astype(F)
    rows["sum2"] = (rng.uniform(0, 1, (n, 3)) ** 8 * 1e9).astype(F)
    rows["samples"] = rng.integers(2, 5000, n)
    rows["sum"][:5], rows["sum2"][5:10] = F(3e30), F(3e38)  # x * x overflows; a huge square
    x, v = moments_mean_variance(rows)
    px, pv, _ = vr.prepare(rows)
    assert x.dtype == F and v.dtype == F
    assert (x.view(np.uint32) == px.view(np.uint32)).all() and (v.view(np.uint32) == pv.view(np.uint32)).all()
    assert (v[:5] == 0).all() and np.isfinite(v).all()
    # the raw [n, 8] float32 rows of the device route are the same rows
    x2, v2 = moments_mean_variance(rows.view(F).reshape(n, 8))
    assert (x2.view(np.uint32) == x.view(np.uint32)).all() and (v2.view(np.uint32) == v.view(np.uint32)).all()
    assert moments_to_numpy(rows.view(F).reshape(n, 8)).dtype == MOMENTS_DTYPE
    # samples 0 and 1: no division by zero leaks out
    few = np.zeros(2, dtype=MOMENTS_DTYPE)
    few["samples"], few["sum"], few["sum2"] = (0, 1), 2.0, 4.0
    x, v = moments_mean_variance(few)
    assert (x[0] == 0).all() and (x[1] == 2).all() and (v == 0).all()


def test_the_association_of_the_six_sums_is_section_19_s():
    """moments_of_samples against a plain loop for 17 samples: chunk 0 holds 16 samples, chunk 1 one, and the result is (0 + chunk0) + chunk1."""
    rng = np.random.default_rng(4)
    c = (rng.uniform(0, 1, (17, 5, 3)) ** 5 * 100).astype(F)
    rows = vr.moments_of_samples(c, valid=np.array([True, True, False, True, True]))
    for p in (0, 1, 3, 4):
        for ch in range(3):
            c0, q0 = F(0), F(0)
            for s in range(16):
                c0, q0 = c0 + c[s, p, ch], q0 + (c[s, p, ch] * c[s, p, ch])
            c1, q1 = F(0) + c[16, p, ch], F(0) + (c[16, p, ch] * c[16, p, ch])
            assert rows["sum"][p, ch] == (F(0) + c0) + c1 and rows["sum2"][p, ch] == (F(0) + q0) + q1
    assert rows["samples"].tolist() == [17, 17, 0, 17, 17] and (vr.moments_rows(rows)[2] == 0).all()
