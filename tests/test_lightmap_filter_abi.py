"""Lightmap filtering (sol_lightmap_filter), the part that needs no GPU: the two entry points are exported, declared, in HIP_SYMBOLS and
in INTEGRATION.md; SolLightmapFilterConfig (64 bytes) has the same size and offsets from gcc -std=c99 -pedantic and from ctypes; every refusal
answers SOL_EINVAL in the stated order, in front of the device check and with nothing written; the kernels are gfx950 code of the library - and the
restatement the GPU tests compare against (tests/lightmap_filter_ref.py) has the properties a chart-aware filter must have."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lightmap_filter_ref as fr
import lightmap_ref as lr
from solstrale_amd import _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_filter_dev", "sol_lightmap_filter")
CFG = _abi.SolLightmapFilterConfig
CFG_OFFSETS = {"size": 0, "width": 4, "height": 8, "iterations": 12, "normal_power_log2": 16, "channels": 20, "stride_bytes": 24, "sigma_position": 28,
               "sigma_plane": 32, "sigma_value": 36, "value_scale": 40, "reserved": 44}
INF, NAN = float("inf"), float("nan")
F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


def test_the_entry_points_are_exported_declared_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, const SolLightmapFilterConfig\* config,", text), name
        assert len(getattr(lib, name).argtypes) == 6
        assert re.search(r"\b" + name + r"\b", integration), f"INTEGRATION.md does not name {name}"


def test_the_struct_agrees_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(CFG) == 64
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == CFG_OFFSETS
    fields = ", ".join(f"(unsigned)offsetof(SolLightmapFilterConfig, {n})" for n in CFG_OFFSETS)
    count = 1 + len(CFG_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolLightmapFilterConfig), {fields});\n  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [64] + list(CFG_OFFSETS.values())


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, iterations=4, normal_power_log2=5, channels=3, stride_bytes=16, sigma_position=0.1, sigma_plane=0.1,
            sigma_value=0.25, value_scale=1.0)
    for k, v in kw.items():
        if k == "reserved":
            for i, r in enumerate(v):
                c.reserved[i] = r
        else:
            setattr(c, k, v)
    return c


def test_every_refusal_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of the device check reads the handle. Each bad argument is
    paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    points, texels, values, out = (C.c_float * 128)(), (C.c_uint32 * 64)(), (C.c_float * 64)(), (C.c_float * 64)()
    good = dict(scene=stand_in, c={}, points=points, texels=texels, values=values, out=out)
    # (what to break - "c": fields of the configuration -, the words sol_last_error must hold), in the header's order
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=60)), b"size"),
             (dict(c=dict(reserved=(0, 0, 0, 0, 1))), b"reserved"), (dict(c=dict(reserved=(7,))), b"reserved"),
             (dict(c=dict(width=0)), b"atlas"), (dict(c=dict(height=16385)), b"atlas"),
             (dict(c=dict(iterations=0)), b"iterations"), (dict(c=dict(iterations=9)), b"iterations"),
             (dict(c=dict(normal_power_log2=8)), b"normal_power_log2"),
             (dict(c=dict(sigma_position=NAN)), b"sigma_position"), (dict(c=dict(sigma_position=0.9e-6)), b"sigma_position"),
             (dict(c=dict(sigma_plane=0.0)), b"sigma_plane"), (dict(c=dict(sigma_plane=NAN)), b"sigma_plane"),
             (dict(c=dict(sigma_value=-1.0)), b"sigma_value"), (dict(c=dict(sigma_value=NAN)), b"sigma_value"),
             (dict(c=dict(value_scale=INF)), b"value_scale"), (dict(c=dict(value_scale=0.0)), b"value_scale"), (dict(c=dict(value_scale=NAN)), b"value_scale"),
             (dict(c=dict(channels=0)), b"channels (1 .. 32)"), (dict(c=dict(channels=33, stride_bytes=256)), b"channels (1 .. 32)"),
             (dict(c=dict(stride_bytes=18)), b"stride"), (dict(c=dict(stride_bytes=8)), b"stride"),
             (dict(points=None), b"null point"), (dict(texels=None), b"null texel"), (dict(values=None), b"null value"), (dict(out=None), b"null output"),
             (dict(out=values), b"out may not be values")]
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
            return fn(a["scene"], cfg, a["points"], a["texels"], a["values"], a["out"])

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, later_word in steps[k + 1:]:  # the earlier refusal is the one named
                if later_word == word or set(later.get("c", {})) & set(broken.get("c", {})) or (set(later) & set(broken)) - {"c"}:
                    continue  # (two ways to break the same argument)
                args = {**good, **later, **broken, "c": {**later.get("c", {}), **broken.get("c", {})}}
                assert call(args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        # +inf is a legal sigma: with everything right the call gets as far as the device
        if device_count() == 0:
            assert call({**good, "c": dict(sigma_position=INF, sigma_plane=INF, sigma_value=INF)}) == _abi.SOL_EDEVICE
            assert call({**good, "c": dict(sigma_position=1e-6, iterations=8, normal_power_log2=7, channels=32, stride_bytes=128)}) == _abi.SOL_EDEVICE
    assert bytes(out) == bytes(256) and bytes(values) == bytes(256)  # nothing was written


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for kernel in (b"sol_lightmap_filter_prepare_kernel", b"sol_lightmap_filter_pass_plain_kernel", b"sol_lightmap_filter_pass_staged_kernel"):
        assert kernel in data, kernel


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
    """Two charts of equal height next to each other in the atlas: columns of a, then columns of b."""
    (pa, ta, wa, h), (pb, tb, wb, _) = a, b
    p = np.concatenate([pa.reshape(h, wa, 8), pb.reshape(h, wb, 8)], axis=1).reshape(-1, 8)
    t = np.concatenate([ta.reshape(h, wa), tb.reshape(h, wb)], axis=1).reshape(-1)
    return p, t


@pytest.mark.parametrize("channels", [1, 3, 4, 5, 27, 32])
def test_a_constant_field_over_one_chart_is_reproduced(channels):
    """Per pass, a channel is sum / wsum with sum = fl(.. fl(fl(0 + fl(w0 x)) + fl(w1 x)) ..): at most 25 products and 25 additions of positive terms,
    each within a factor (1 + u), u = 2^-24, so sum = x * W * (1 + e1) with |e1| <= 26 u to first order, where W is the exact sum of the weights; wsum =
    W * (1 + e2) with |e2| <= 25 u; the division adds u: a pass answers within 52 u = 3.1e-6 of a weighted mean of its input. A weighted mean of
    values within d of x is within d of x, so n passes stay within 52 n u: 9.3e-6 for n = 3 and, in the worst case, 2.5e-5 for n = 8. The bound
    asserted is the issue's 1e-5 for every n all the same: the worst case needs every rounding of every pass to err the same way."""
    W, H = 19, 13
    points, texels = _chart(W, H)
    const = (F(0.7) + F(0.37) * np.arange(channels, dtype=F)).astype(F)
    values = np.tile(np.concatenate([const, [F(5.0)]]).astype(F), (W * H, 1))
    for iterations in range(1, 9):
        out = fr.lightmap_filter(values, points, texels, W, H, 0.02, iterations=iterations, channels=channels)
        rel = np.abs(out[:, :channels].astype(np.float64) / const.astype(np.float64) - 1.0).max()
        assert rel <= 1e-5, (iterations, rel)
        assert (out[:, channels] == F(5.0)).all()


def test_coplanar_charts_far_apart_in_the_world_do_not_mix():
    """Two coplanar charts, equal normals, neighbours in the atlas, 1e6 x sigma_position apart in the world; the plane and value factors are off
    (coplanar: d = 0; sigma_value = +inf), so that only the distance factor stands between them. A tap across has l2 >= (1e6 s)^2 (less the charts'
    own extent, 16 texels of s / 2: 8e-6 of it), so in pass i  w_d = 1 / (1 + l2 / (s f)^2) <= 1.0001 (f / 1e6)^2,  f = 2^i. The taps across carry at most
    the whole kernel, sum k <= 1, and the centre alone carries 9/64, so the share of the other chart in a pass is at most (64/9) 1.0001 (f / 1e6)^2;
    summed over f = 1, 2, 4, 8 that is 85 x 7.12e-12 = 6.1e-10 of the step |b - a|, here 2 a: 1.3e-9 relative. The roundings of four passes add
    4 x 52 u = 1.3e-5 in the worst case (see the constant-field test); the bound asserted is the issue's 1e-5."""
    W, H, sigma = 8, 8, 1e-3
    a = _chart(W, H, texel=sigma / 2)
    b = _chart(W, H, origin=(1e6 * sigma, 0.0, 0.0), texel=sigma / 2)
    points, texels = _side_by_side(a + (W, H), b + (W, H))
    ca, cb = F(0.7), F(2.1)
    values = np.zeros((2 * W * H, 4), dtype=F)
    values.reshape(H, 2 * W, 4)[:, :W, :3], values.reshape(H, 2 * W, 4)[:, W:, :3] = ca, cb
    out = fr.lightmap_filter(values, points, texels, 2 * W, H, sigma, sigma_value=INF, iterations=4).reshape(H, 2 * W, 4)
    assert np.abs(out[:, :W, :3].astype(np.float64) / float(ca) - 1).max() <= 1e-5
    assert np.abs(out[:, W:, :3].astype(np.float64) / float(cb) - 1).max() <= 1e-5
    # the distance factor off: the border columns take 5/16 of their weight from the other chart in the first pass alone
    mixed = fr.lightmap_filter(values, points, texels, 2 * W, H, INF, sigma_value=INF, iterations=4).reshape(H, 2 * W, 4)
    step = float(cb) - float(ca)
    assert (mixed[:, W - 1, :3] - ca > 0.1 * step).all() and (cb - mixed[:, W, :3] > 0.1 * step).all()


@pytest.mark.parametrize("power", [1, 5])
def test_a_right_angle_crease_exchanges_nothing(power):
    """n_p . n_q = ((0 * 1) + (1 * 0)) + (0 * 0) = 0 exactly, pos(0) = 0, squared it stays 0, and w = (..) * 0 * w_v is 0 or NaN: not > 0, skipped.
    So a side's answer does not depend on the other side's values: compared word for word."""
    W, H = 6, 9
    floor = _chart(W, H)
    wall = _chart(W, H, origin=(0.06, 0.0, 0.0), normal=(1.0, 0.0, 0.0), axes=((0, 1, 0), (0, 0, 1)))
    points, texels = _side_by_side(floor + (W, H), wall + (W, H))
    rng = np.random.default_rng(5)
    v1 = rng.uniform(0.1, 2.0, (H, 2 * W, 4)).astype(F)
    v2 = v1.copy()
    v2[:, W:, :3] = rng.uniform(5.0, 9.0, (H, W, 3)).astype(F)
    o1, o2 = (fr.lightmap_filter(v.reshape(-1, 4), points, texels, 2 * W, H, INF, sigma_value=INF, normal_power_log2=power, iterations=3).reshape(H, 2 * W, 4)
              for v in (v1, v2))
    assert (o1[:, :W].view(np.uint32) == o2[:, :W].view(np.uint32)).all()
    assert (o1[:, W:] != o2[:, W:]).any() and (o1[:, :W, :3] != v1[:, :W, :3]).any()


def test_with_every_factor_off_one_pass_is_the_plain_b3_mean_with_border_taps_dropped():
    """Equal unit normals give c = pos(1) = 1, every sigma +inf gives 1 / (1 + 0) = 1: w = k exactly. Against the same mean in float64 a channel is
    within 52 u (the constant-field test's count of roundings for one pass, all terms positive)."""
    W, H = 11, 7
    points, texels = _chart(W, H)
    rng = np.random.default_rng(11)
    values = rng.uniform(0.05, 4.0, (W * H, 3)).astype(F)
    out = fr.lightmap_filter(values, points, texels, W, H, INF, sigma_plane=INF, sigma_value=INF, normal_power_log2=0, iterations=1).reshape(H, W, 3)
    h = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    x = values.astype(np.float64).reshape(H, W, 3)
    for j in range(H):
        for i in range(W):
            num, den = np.zeros(3), 0.0
            for dj in range(-2, 3):
                for di in range(-2, 3):
                    if 0 <= j + dj < H and 0 <= i + di < W:
                        num += h[di + 2] * h[dj + 2] * x[j + dj, i + di]
                        den += h[di + 2] * h[dj + 2]
            assert np.abs(out[j, i] / (num / den) - 1).max() <= 52 * U, (i, j)


def test_rows_that_are_not_live_come_back_as_they_went_in_and_are_never_taps():
    W, H = 9, 9
    points, texels = _chart(W, H)
    rng = np.random.default_rng(2)
    values = rng.uniform(0.1, 2.0, (W * H, 4)).astype(F)
    values[:, 3] = np.arange(W * H, dtype=np.uint32).view(F)  # a trailing `samples` word
    bad = {"unowned": 4 * W + 4, "position": 2 * W + 2, "normal": 2 * W + 6, "value": 6 * W + 2, "unowned nan": 6 * W + 6}
    texels["triangle"][[bad["unowned"], bad["unowned nan"]]] = lr.NONE
    points[bad["position"], 1], points[bad["normal"], 5] = np.inf, np.nan
    values[bad["value"], 2] = -np.inf
    values[bad["unowned nan"], :3] = np.nan
    out = fr.lightmap_filter(values, points, texels, W, H, 0.05, iterations=3)
    rows = list(bad.values())
    assert (out.view(np.uint32)[rows] == values.view(np.uint32)[rows]).all()
    assert np.isfinite(out[np.setdiff1d(np.arange(W * H), rows), :3]).all()
    assert (out.view(np.uint32)[:, 3] == values.view(np.uint32)[:, 3]).all(), "the trailing word survives"
    # whatever the rows hold, no neighbour reads them
    other = values.copy()
    other[rows, :3] = rng.uniform(50.0, 90.0, (len(rows), 3)).astype(F)
    other[bad["value"], 2] = np.nan
    points2 = points.copy()
    points2[bad["position"], 0:3], points2[bad["normal"], 4:7] = (np.nan, 7.0, -np.inf), (np.inf, 0.0, 1.0)
    out2 = fr.lightmap_filter(other, points2, texels, W, H, 0.05, iterations=3)
    keep = np.setdiff1d(np.arange(W * H), rows)
    assert (out.view(np.uint32)[keep] == out2.view(np.uint32)[keep]).all()
    assert (out[keep, :3] != values[keep, :3]).any()


def test_a_one_texel_atlas_returns_its_input():
    """The only tap is the centre: a pass answers fl(fl(k x) / wsum) with wsum = fl(0 + k) = k = 9/64 - two roundings, the product and the division
    (fl(fl(9 x) / 9) is not x for every x: the rule is sum / wsum, and the restatement is not asked for more than the rule). So n passes answer
    within (1 + u)^(2n) - 1 <= 2.01 n u of the input, of either sign; a zero stays a zero, and the trailing word is the input's."""
    points, texels = _chart(1, 1)
    rng = np.random.default_rng(3)
    for iterations in (1, 8):
        for _ in range(50):
            values = np.concatenate([rng.uniform(-3.0, 7.0, 2).astype(F), [F(0.0)], np.array([123], dtype=np.uint32).view(F)]).astype(F)[None, :]
            out = fr.lightmap_filter(values, points, texels, 1, 1, 0.02, iterations=iterations)
            assert np.abs(out[0, :2].astype(np.float64) / values[0, :2].astype(np.float64) - 1).max() <= 2.01 * iterations * U
            assert (out.view(np.uint32)[0, 2:] == values.view(np.uint32)[0, 2:]).all()


def test_the_kernel_products_are_exact_and_sum_to_one():
    k = np.array([[a * b for a in fr.H5] for b in fr.H5], dtype=F)
    assert (k.astype(np.float64) == np.outer([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])).all()
    assert k.astype(np.float64).sum() == 1.0 and k[2, 2] == F(9 / 64)
