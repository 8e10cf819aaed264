"""Lightmap texel points and border dilation (sol_lightmap_points / sol_lightmap_dilate), the part that needs no GPU: the four entry
points are exported and declared, the header is still C99, SolLightmapConfig (32 bytes) and SolTexel (16 bytes) have the same size and offsets
from gcc and from ctypes, every refusal that needs no handle answers SOL_EINVAL in the stated order and in front of the device check with
nothing written - and the restatement the GPU tests compare against (tests/lightmap_ref.py) has the rule's own properties: a mesh that tiles
the atlas leaves no hole, every centre goes to the lowest index that contains it, and a triangle's vertex order changes no owner."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lightmap_ref as lr
from solstrale_amd import LIGHTMAP_TEXEL_DTYPE, _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_points_dev", "sol_lightmap_points", "sol_lightmap_dilate_dev", "sol_lightmap_dilate")
CFG = _abi.SolLightmapConfig
CFG_OFFSETS = {"size": 0, "width": 4, "height": 8, "flags": 12, "tmin": 16, "tmax": 20, "reserved": 24}
TEXEL_OFFSETS = {"triangle": 0, "b1": 4, "b2": 8, "flags": 12}
INF, NAN = float("inf"), float("nan")
GRID_SEED = 1  # (test_the_restatement_leaves_no_hole.. asserts that this seed gives a mesh without holes)


def test_the_four_entry_points_are_exported_and_declared():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene,", text), name
        assert getattr(lib, name).argtypes is not None
    assert len(lib.sol_lightmap_points.argtypes) == len(lib.sol_lightmap_points_dev.argtypes) == 8
    assert len(lib.sol_lightmap_dilate.argtypes) == len(lib.sol_lightmap_dilate_dev.argtypes) == 10
    assert re.search(r"#define SOL_ABI_VERSION 2\b", text)
    assert _abi.SOL_LIGHTMAP_CONSERVATIVE == 1 and re.search(r"#define SOL_LIGHTMAP_CONSERVATIVE 1u", text)


def test_the_structs_agree_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(CFG) == 32 and C.sizeof(_abi.SolTexel) == 16
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == CFG_OFFSETS
    assert {n: getattr(_abi.SolTexel, n).offset for n, _ in _abi.SolTexel._fields_} == TEXEL_OFFSETS
    dt = LIGHTMAP_TEXEL_DTYPE
    assert dt.itemsize == 16 and {n: dt.fields[n][1] for n in dt.names} == TEXEL_OFFSETS and dt == lr.TEXEL_DTYPE
    fields = ", ".join([f"(unsigned)offsetof(SolLightmapConfig, {n})" for n in CFG_OFFSETS] + [f"(unsigned)offsetof(SolTexel, {n})" for n in TEXEL_OFFSETS])
    count = 2 + len(CFG_OFFSETS) + len(TEXEL_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolLightmapConfig), (unsigned)sizeof(SolTexel), {fields});\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32, 16] + list(CFG_OFFSETS.values()) + list(TEXEL_OFFSETS.values())


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=4, height=4, flags=0, tmin=1e-3, tmax=INF)
    for k, v in kw.items():
        if k == "reserved":
            c.reserved[0], c.reserved[1] = v
        else:
            setattr(c, k, v)
    return c


def test_every_refusal_of_lightmap_points_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of the device check reads the handle. Each bad argument is
    paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    v, uv = (C.c_float * 18)(), (C.c_float * 12)()
    points, texels = (C.c_float * (16 * 8))(), (C.c_uint32 * (16 * 4))()
    good = dict(scene=stand_in, v=v, uv=uv, n=2, c={}, points=points, texels=texels)
    # (what to break - "c": fields of the configuration -, the word sol_last_error must hold), in the header's order
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=28)), b"size"),
             (dict(c=dict(reserved=(0, 1))), b"reserved"), (dict(c=dict(flags=2)), b"flags"), (dict(c=dict(width=0)), b"atlas"),
             (dict(c=dict(height=16385)), b"atlas"), (dict(c=dict(tmin=-1.0)), b"tmin"), (dict(c=dict(tmax=NAN)), b"tmin"), (dict(n=(1 << 31) - 1), b"2^31 - 2"),
             (dict(v=None), b"null vertex"), (dict(uv=None), b"null UV"), (dict(points=None), b"null point output"), (dict(texels=None), b"null texel output")]
    for name in ("sol_lightmap_points", "sol_lightmap_points_dev"):
        fn = getattr(lib, name)

        def call(a):
            cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
            return fn(a["scene"], a["v"], None, a["uv"], a["n"], cfg, a["points"], a["texels"])

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:  # the earlier refusal is the one named
                args = {**good, **later, **broken, "c": {**later.get("c", {}), **broken.get("c", {})}}
                assert call(args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
        if device_count() == 0:  # n_triangles == 0 needs no vertex and no UV pointer: with everything else right the call gets as far as the device
            assert call({**good, "n": 0, "v": None, "uv": None}) == _abi.SOL_EDEVICE
    assert bytes(points) == bytes(16 * 8 * 4) and bytes(texels) == bytes(16 * 4 * 4)  # nothing was written


def test_every_refusal_of_lightmap_dilate_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    err = lib.sol_last_error
    stand_in = C.create_string_buffer(1 << 20)
    texels, values, out, pass_of = (C.c_uint32 * 64)(), (C.c_float * 64)(), (C.c_float * 64)(), (C.c_uint8 * 16)()
    good = dict(scene=stand_in, texels=texels, w=4, h=4, values=values, channels=3, stride=16, passes=1, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(texels=None), b"null texel"), (dict(values=None), b"null value"), (dict(out=None), b"null output"),
             (dict(w=0), b"atlas"), (dict(h=16385), b"atlas"), (dict(channels=0), b"channels (1 .. 32)"), (dict(channels=33, stride=256), b"channels (1 .. 32)"),
             (dict(stride=18), b"stride"), (dict(stride=8), b"stride"), (dict(passes=255), b"passes"), (dict(out=values), b"out may not be values")]
    for name in ("sol_lightmap_dilate", "sol_lightmap_dilate_dev"):
        fn = getattr(lib, name)

        def call(a):
            return fn(a["scene"], a["texels"], a["w"], a["h"], a["values"], a["channels"], a["stride"], a["passes"], a["out"], pass_of)

        for k, (broken, word) in enumerate(steps):
            assert call({**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:
                if set(later) & set(broken):
                    continue
                assert call({**good, **later, **broken}) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())
    assert bytes(out) == bytes(256) and bytes(pass_of) == bytes(16)  # nothing was written


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_valid_arguments_reach_the_device_check():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    v, uv, points, texels = (C.c_float * 9)(), (C.c_float * 6)(), (C.c_float * 128)(), (C.c_uint32 * 64)()
    assert lib.sol_lightmap_points(stand_in, v, None, uv, 1, C.byref(_cfg()), points, texels) == _abi.SOL_EDEVICE
    assert lib.sol_lightmap_points(None, v, None, uv, 1, C.byref(_cfg()), points, texels) == _abi.SOL_EINVAL


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for kernel in (b"sol_lightmap_claim_small_kernel", b"sol_lightmap_claim_tiles_kernel", b"sol_lightmap_claim_large_kernel", b"sol_lightmap_emit_kernel",
                   b"sol_lightmap_dilate_begin_kernel", b"sol_lightmap_dilate_pass_kernel"):
        assert kernel in data, kernel


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------------
def _contains_f64(uv, px, py):
    """Is P inside the closed triangle, in float64 over the float32 texel-space corners (exact enough away from the edges)?"""
    a, b, c = uv.astype(np.float64)
    def e(q, r):
        return (r[0] - q[0]) * (py - q[1]) - (r[1] - q[1]) * (px - q[0])
    s = np.sign((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
    return np.minimum(np.minimum(s * e(b, c), s * e(c, a)), s * e(a, b))


def test_the_restatement_leaves_no_hole_and_gives_every_centre_to_the_lowest_index():
    W = H = 64
    V, T, N = lr.grid_mesh(16, GRID_SEED)
    assert len(V) == 512
    owner, _ = lr.lightmap_owner(V, T, W, H)
    assert (owner != lr.NONE).all(), "the jittered grid tiles [0, 1]^2: zero holes"
    assert (owner < len(V)).all()
    # the lowest-index rule, from the rule's own edge functions: no triangle below the owner has the centre inside, and the owner has
    j, i = np.divmod(np.arange(W * H), W)
    px, py = i.astype(np.float32) + np.float32(0.5), j.astype(np.float32) + np.float32(0.5)
    lowest = np.full(W * H, lr.NONE, dtype=np.uint32)
    for g in range(len(V) - 1, -1, -1):
        t = lr._setup(T[g], V[g], None, W, H)
        e0, e1, e2 = t.edges(px, py)
        lowest[(e0 >= 0) & (e1 >= 0) & (e2 >= 0)] = g
    assert (lowest == owner).all()
    # and geometrically (float64): the owner contains its centre up to rounding; a centre clearly inside a triangle is owned by it
    tex = T.astype(np.float32) * np.float32(W)
    margin = np.array([_contains_f64(tex[o], x, y) for o, x, y in zip(owner, px.astype(np.float64), py.astype(np.float64))])
    assert (margin > -1e-3).all()
    clear = 0
    for g in range(len(V)):
        inside = _contains_f64(tex[g], px.astype(np.float64), py.astype(np.float64)) > 1e-3
        assert (owner[inside] == g).all()
        clear += int(inside.sum())
    assert clear > 0.95 * W * H
    # a mesh that tiles the atlas leaves no conservative-only texel either, and normals change no owner
    points, texels = lr.lightmap_points(V, T, W, H, normals=N, conservative=True)
    assert (texels["flags"] == 1).all() and (texels["triangle"] == owner).all()
    assert np.allclose(np.sqrt((points[:, 4:7].astype(np.float64) ** 2).sum(axis=1)), 1.0, atol=1e-6)


def test_swapping_the_vertex_order_of_any_triangle_changes_no_owner():
    W = H = 64
    V, T, N = lr.grid_mesh(16, GRID_SEED)
    owner, _ = lr.lightmap_owner(V, T, W, H)
    rng = np.random.default_rng(3)
    orders = [(0, 2, 1), (1, 0, 2), (2, 1, 0), (1, 2, 0), (2, 0, 1)]
    V2, T2 = V.copy(), T.copy()
    for g in range(len(V)):
        o = list(orders[int(rng.integers(0, len(orders)))])
        V2[g], T2[g] = V[g][o], T[g][o]
    assert (T2 != T).any()
    swapped, _ = lr.lightmap_owner(V2, T2, W, H)
    assert (swapped == owner).all()
    for cons in (False, True):  # also off the grid: overlapping random triangles, conservative claims included
        c = rng.uniform(0, 1, (300, 1, 2))
        R = (c + rng.uniform(-0.08, 0.08, (300, 3, 2))).astype(np.float32)
        R2 = R[:, [2, 1, 0]]
        a, _ = lr.lightmap_owner(lr.lift(R), R, 48, 40, conservative=cons)
        b, _ = lr.lightmap_owner(lr.lift(R2), R2, 48, 40, conservative=cons)
        assert (a == b).all() and (a != lr.NONE).any()


def test_the_restatement_of_the_dilation_fills_ring_by_ring():
    W, H = 9, 7
    texels = np.zeros(W * H, dtype=lr.TEXEL_DTYPE)
    texels["triangle"] = lr.NONE
    texels["triangle"][3 * W + 4] = 0  # one owned texel in the middle
    values = np.zeros((W * H, 4), dtype=np.float32)
    values[3 * W + 4] = (2.0, 4.0, 8.0, 1.0)
    out, pass_of = lr.lightmap_dilate(values, texels, W, H, passes=2, channels=3)
    j, i = np.divmod(np.arange(W * H), W)
    ring = np.maximum(np.abs(i - 4), np.abs(j - 3)).reshape(H, W)
    assert (pass_of == np.where(ring <= 2, ring, 255)).all()
    assert (out.reshape(H, W, 4)[ring == 1] == (2.0, 4.0, 8.0, 0.0)).all()  # the mean of one covered neighbour; the rest of the row zero
    assert (out.reshape(H, W, 4)[ring == 2][:, :3] == (2.0, 4.0, 8.0)).all() and (out.reshape(H, W, 4)[ring > 2] == 0).all()
