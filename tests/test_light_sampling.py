"""Light tree and power-weighted light sampling (EXTENSION), the parts that need no device: the struct and the entry points,
the configuration and scene refusals of sol_light_sampling(_check), the weights of sol_light_weights against a numpy restatement, and the
host mirror's mode parsing. The device side is tests/test_gpu_light_sampling.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from solstrale_amd import CameraConfig, PathTracingShader, RenderConfig, SceneBuilder, _abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg(mode, **kw):
    c = dict(size=C.sizeof(_abi.SolLightSampling), mode=mode)
    c.update(kw)  # (kw may override the mode)
    return _abi.SolLightSampling(**c)


# ---- numpy restatement of the weights and the tables (csrc/sol_lights.hip) ----
def np_weights(desc):
    """w_i = area_i * Y_i in f64, list order; Y of the DiffuseLight's texture (solid: its colour, image: mean texel / 255); else 0."""
    w = np.zeros(desc.n_lights)
    for i in range(desc.n_lights):
        r = desc.lights[i]
        k, x = _abi.ref_kind(r), _abi.ref_index(r)
        if k == _abi.REF_QUAD:
            area, mat = desc.quads[x].area, desc.quads[x].material
        elif k == _abi.REF_TRIANGLE:
            area, mat = desc.triangles[x].area, desc.triangles[x].material
        elif k == _abi.REF_SPHERE:
            rad = desc.spheres[x].radius
            area, mat = 4.0 * math.pi * rad * rad, desc.spheres[x].material
        else:
            continue
        m = desc.materials[mat]
        if m.kind != _abi.MAT_DIFFUSE_LIGHT:
            continue
        t = desc.textures[m.albedo_tex]
        if t.kind == _abi.TEX_SOLID:
            rgb = [t.rgb[0], t.rgb[1], t.rgb[2]]
        else:
            n = t.width * t.height
            px = np.ctypeslib.as_array(C.cast(desc.texels, C.POINTER(C.c_uint8)), shape=(desc.n_texel_bytes,))
            px = px[t.texel_offset:t.texel_offset + 3 * n].reshape(n, 3).astype(np.float64) / 255.0
            rgb = [0.0, 0.0, 0.0]
            for row in px:  # (the library's order: a running sum per channel, then / n)
                for c in range(3):
                    rgb[c] += row[c]
            rgb = [v / n for v in rgb]
        v = area * (0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2])
        w[i] = v if (v > 0 and math.isfinite(v)) else 0.0
    return w


def np_tables(w):
    """(q, C, W): W the f64 sum in list order, C_i = (float)(prefix_i / W), C_{L-1} = 1, q_i = C_i - C_{i-1} in fp32."""
    W = 0.0
    for x in w:
        W += x
    cdf = np.zeros(len(w), np.float32)
    prefix = 0.0
    for i, x in enumerate(w):
        prefix += x
        cdf[i] = np.float32(prefix / W)
    cdf[-1] = np.float32(1.0)
    q = (cdf - np.concatenate([[np.float32(0)], cdf[:-1]])).astype(np.float32)
    return q, cdf, W


def lib_weights(sc):
    lib = _abi.load_hip()
    w = np.zeros(sc.desc.n_lights)
    assert lib.sol_light_weights(sc.desc_ptr, w.ctypes.data, w.size) == _abi.SOL_OK
    return w


def _three_lights(colors=((4., 4., 4.), (1., 0., 0.), (0., 0., 2.)), image=None):
    """A quad, a triangle and a sphere light over a Lambertian floor."""
    b = SceneBuilder()
    floor = b.Quad((-5., 0., -5.), (10., 0., 0.), (0., 0., 10.), b.Lambertian(b.SolidColor(.5, .5, .5)))
    m = [b.DiffuseLight(*c) for c in colors]
    objs = [floor, b.Quad((-1., 3., -1.), (2., 0., 0.), (0., 0., 1.5), m[0]),
            b.Triangle((2., 2., 0.), (3., 2., 0.), (2., 2., 1.), m[1]), b.Sphere((-2., 1., 1.), .5, m[2])]
    if image is not None:
        objs.append(b.Quad((0., 4., 0.), (1., 0., 0.), (0., 0., 1.), b.Lambertian(b.ImageMap(image))))
    cam = CameraConfig(40., 0., (0., 2., 8.), (0., 1., 0.), (0., 1., 0.))
    return b.finish(b.Bvh(objs), cam, (0., 0., 0.), RenderConfig(32, 24, 4, PathTracingShader(8)))


def test_entry_points_and_struct_layout(tmp_path):
    lib = _abi.load_hip()
    for n in ("sol_light_sampling", "sol_light_sampling_check", "sol_light_weights", "sol_light_tables", "sol_light_tree", "sol_light_eval"):
        assert hasattr(lib, n) and n in _abi.HIP_SYMBOLS
    assert hasattr(_abi.load_host(), "solh_set_light_sampling") and "solh_set_light_sampling" in _abi.HOST_SYMBOLS
    assert _abi.SolLightSampling not in _abi.ABI_STRUCTS and len(_abi.ABI_STRUCTS) == 11
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "probe.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "solstrale_hip.h"
#include "solstrale_host.h"
int main(void) {
  printf("%u %u %u %u %u %u %u\\n", (unsigned)sizeof(SolLightSampling), (unsigned)offsetof(SolLightSampling, size),
         (unsigned)offsetof(SolLightSampling, mode), (unsigned)offsetof(SolLightSampling, reserved), SOL_LIGHT_SAMPLING_UNIFORM,
         SOL_LIGHT_SAMPLING_TREE, SOL_LIGHT_SAMPLING_POWER);
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _abi.SolLightSampling
    assert got == [C.sizeof(S), S.size.offset, S.mode.offset, S.reserved.offset, 0, 1, 2] and C.sizeof(S) == 16


@pytest.mark.parametrize("bad", [dict(size=8), dict(mode=3), dict(mode=0xFFFFFFFF), dict(reserved=(C.c_uint32 * 2)(0, 1))],
                         ids=["size", "mode3", "mode_max", "reserved"])
def test_configuration_errors_need_no_device(bad):
    lib = _abi.load_hip()
    c = cfg(**{"mode": 1, **bad})
    assert lib.sol_light_sampling(None, C.byref(c)) == _abi.SOL_EINVAL
    assert b"sol_light_sampling" in lib.sol_last_error()  # refused for the configuration, not for the missing scene
    assert lib.sol_light_sampling_check(_three_lights().desc_ptr, C.byref(c)) == _abi.SOL_EINVAL
    assert b"sol_light_sampling_check" in lib.sol_last_error()


def test_scene_errors_need_no_device():
    lib = _abi.load_hip()
    assert lib.sol_light_sampling(None, C.byref(cfg(1))) == _abi.SOL_EINVAL and lib.sol_last_error() == b"null scene"
    assert lib.sol_light_sampling(None, None) == _abi.SOL_EINVAL
    assert lib.sol_light_tables(None, None, None, 0, None) == _abi.SOL_EINVAL
    assert lib.sol_light_tree(None, None, 0, None, None, None) == _abi.SOL_EINVAL
    assert lib.sol_light_eval(None, 0, None, 0, None) == _abi.SOL_EINVAL
    assert lib.sol_light_sampling_check(None, None) == _abi.SOL_EINVAL
    check = lambda sc, mode: lib.sol_light_sampling_check(sc.desc_ptr, C.byref(cfg(mode)) if mode is not None else None)
    sc = _three_lights()
    for m in (None, 0, 1, 2):
        assert check(sc, m) == _abi.SOL_OK, m
    # every light of power 0: black emission, ...
    black = _three_lights(colors=((0., 0., 0.), (0., 0., 0.), (-1., -1., -1.)))
    assert (lib_weights(black) == 0).all()
    assert check(black, 2) == _abi.SOL_EINVAL and b"power 0" in lib.sol_last_error()
    for m in (None, 0, 1):
        assert check(black, m) == _abi.SOL_OK  # modes 0 and 1 do not need power
    # ... a light whose material is not a DiffuseLight (the floor, listed as the only light) ...
    sc = _three_lights()
    d = sc.desc
    floor_ref = next(d.lights[i] for i in range(d.n_lights) if _abi.ref_kind(d.lights[i]) == _abi.REF_QUAD)
    floor_ref = (floor_ref & ~0x0FFFFFFF) | next(i for i in range(d.n_quads) if d.materials[d.quads[i].material].kind == _abi.MAT_LAMBERTIAN)
    one = (C.c_uint32 * 1)(floor_ref)
    saved = (d.lights, d.n_lights)
    d.lights, d.n_lights = C.cast(one, C.POINTER(C.c_uint32)), 1
    try:
        assert (lib_weights(sc) == 0).all()
        assert check(sc, 2) == _abi.SOL_EINVAL and check(sc, 1) == _abi.SOL_OK
    finally:
        d.lights, d.n_lights = saved
    # ... and lights of area 0
    sc = _three_lights()
    d = sc.desc
    for i in range(d.n_quads):
        d.quads[i].area = 0.0
    for i in range(d.n_triangles):
        d.triangles[i].area = 0.0
    for i in range(d.n_spheres):
        d.spheres[i].radius = 0.0
    assert (lib_weights(sc) == 0).all() and check(sc, 2) == _abi.SOL_EINVAL
    assert lib.sol_light_weights(sc.desc_ptr, None, 0) == _abi.SOL_EINVAL  # (no room)


def test_weights_match_the_numpy_restatement():
    for sc in (_three_lights(), scenes.mixed_power_lights(16), scenes.many_lights(9, "triangles"), scenes.many_lights(7, "spheres"),
               scenes.create_test_scene(RenderConfig(16, 16, 1, PathTracingShader(4)))):
        w = lib_weights(sc)
        assert w.tobytes() == np_weights(sc.desc).tobytes()
        assert (w > 0).all()
    # an image-textured DiffuseLight (the raw API: the host builder makes DiffuseLights of a solid colour): its mean texel
    img = np.random.default_rng(3).integers(0, 256, (5, 7, 3)).astype(np.uint8)
    sc = _three_lights(image=img)
    d = sc.desc
    q = next(i for i in range(d.n_quads) if d.textures[d.materials[d.quads[i].material].albedo_tex].kind == _abi.TEX_IMAGE)
    d.materials[d.quads[q].material].kind = _abi.MAT_DIFFUSE_LIGHT
    refs = (C.c_uint32 * (d.n_lights + 1))(*[d.lights[i] for i in range(d.n_lights)], (_abi.REF_QUAD << 28) | q)
    d.lights, d.n_lights = C.cast(refs, C.POINTER(C.c_uint32)), d.n_lights + 1
    w = lib_weights(sc)
    assert w.tobytes() == np_weights(d).tobytes()
    mean = img.reshape(-1, 3).astype(np.float64).mean(axis=0) / 255.0
    assert w[-1] == pytest.approx(d.quads[q].area * (0.2126 * mean[0] + 0.7152 * mean[1] + 0.0722 * mean[2]), rel=1e-12)


def test_table_restatement_properties():
    """The numpy tables the GPU test compares the device's against: C ends at 1, q sums to 1 within fp32 and is 0 for weight 0."""
    w = np.array([3.0, 0.0, 1e-30, 2.0, 0.0])
    q, c, W = np_tables(w)
    assert W == 5.0 + 1e-30 and c[-1] == 1.0 and q[1] == 0 and q[4] == 0 and q[2] == 0  # (1e-30 / 5 rounds C_2 onto C_1)
    assert (np.diff(c) >= 0).all() and abs(float(q.astype(np.float64).sum()) - 1.0) < 1e-6


def test_host_mirror_parses_modes():
    lib = _abi.load_host()
    b = lib.solh_builder_new()
    try:
        for m in (0, 1, 2):
            assert lib.solh_set_light_sampling(b, m) == 0
        for m in (3, 7, 0xFFFFFFFF):
            assert lib.solh_set_light_sampling(b, m) < 0, m
            assert b"solh_set_light_sampling" in lib.solh_last_error()
    finally:
        lib.solh_builder_free(b)
    for bad in ("uniform", "importance", 1, "Tree"):
        with pytest.raises(ValueError):
            RenderConfig(16, 16, 1, light_sampling=bad)
    assert RenderConfig(16, 16, 1).light_sampling is None
    for m in ("tree", "power"):
        assert RenderConfig(16, 16, 1, light_sampling=m).light_sampling == m
