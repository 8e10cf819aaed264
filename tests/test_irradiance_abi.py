"""Irradiance queries (sol_irradiance / sol_irradiance_dev / sol_irradiance_rays), the part that needs no GPU: the three entry
points are exported, the configuration has the layout the header states and the ctypes mirror agrees with it, the header is still C99, every
refusal that needs no device answers SOL_EINVAL in front of the device check and names its reason, the kernels are gfx950 code of the library -
and the occluder case of tests/test_gpu_irradiance.py is a fair one: for its seed and geometry the float oracle's directions stay clear of
the cone's edge and split as the solid angle says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import irradiance_util as iu
from solstrale_amd import _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_irradiance_dev", "sol_irradiance", "sol_irradiance_rays")
CFG = _abi.SolIrradianceConfig
OFFSETS = {"size": 0, "samples": 4, "first_sample": 8, "first_draw": 12, "seed": 16, "key_base": 24, "mode": 28}


def test_the_three_entry_points_are_exported():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\*", text), name


def test_the_configuration_has_the_layout_the_header_states():
    assert C.sizeof(CFG) == 32
    assert {n: getattr(CFG, n).offset for n, _ in CFG._fields_} == OFFSETS
    m = re.search(r"sizeof\(SolIrradianceConfig\) = (\d+): ([^*]*)\*/", open(HEADER).read())
    assert m and int(m.group(1)) == 32
    assert {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", m.group(2))} == OFFSETS
    assert (_abi.SOL_IRRADIANCE_COSINE, _abi.SOL_IRRADIANCE_SPHERE) == (0, 1)


def test_the_header_is_c99_and_the_compiler_agrees_with_the_mirror(tmp_path):
    fields = ", ".join(f"(unsigned)offsetof(SolIrradianceConfig, {n})" for n in OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\n#include "solstrale_host.h"\nint main(void) {\n'
                    '  unsigned v[] = {(unsigned)sizeof(SolIrradianceConfig), ' + fields + ', SOL_IRRADIANCE_COSINE, SOL_IRRADIANCE_SPHERE};\n'
                    '  unsigned i;\n  for (i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%u ", v[i]);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32] + list(OFFSETS.values()) + [0, 1]


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), samples=1)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _calls(lib, points, out, keys_out):
    """The three entry points as f(scene, n, config) over the same arrays."""
    return (("sol_irradiance", lambda s, n, c: lib.sol_irradiance(s, C.byref(points), None, n, c, C.byref(out))),
            ("sol_irradiance_dev", lambda s, n, c: lib.sol_irradiance_dev(s, C.byref(points), None, n, c, C.byref(out))),
            ("sol_irradiance_rays", lambda s, n, c: lib.sol_irradiance_rays(s, C.byref(points), None, n, c, C.byref(out), C.byref(keys_out))))


def test_every_refusal_that_needs_no_handle_is_einval_before_the_device():
    """With or without a GPU. The configuration and n are judged by a function that is not given the handle (radiance_config_check,
    sol_api.cpp), right behind the null test of the scene pointer: a zeroed block stands in for a scene - there is no way to make a real one
    without a device - and is never read. tests/test_gpu_irradiance.py repeats the refusals on a handle, with those that read it."""
    lib = _abi.load_hip()
    points, out, keys_out = (_abi.SolRay * 2)(), (_abi.SolRadiance * 4)(), (_abi.SolRayKey * 2)()
    stand_in = C.create_string_buffer(1 << 20)
    for name, f in _calls(lib, points, out, keys_out):
        for n in (2, 0):  # (a null scene also with n == 0)
            assert f(None, n, C.byref(_cfg())) == _abi.SOL_EINVAL, name
            assert b"null scene" in lib.sol_last_error() and name.encode() + b":" in lib.sol_last_error()
        assert f(stand_in, 2, None) == _abi.SOL_EINVAL and b"null configuration" in lib.sol_last_error()
        for bad, word in ((_cfg(size=28), b"size"), (_cfg(size=0), b"size"), (_cfg(samples=0), b"samples"),
                          (_cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample"), (_cfg(mode=2), b"mode"), (_cfg(mode=0xFFFFFFFF), b"mode")):
            assert f(stand_in, 2, C.byref(bad)) == _abi.SOL_EINVAL, (name, word)
            assert word in lib.sol_last_error(), (name, lib.sol_last_error())
        assert f(stand_in, (1 << 31) + 1, C.byref(_cfg())) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
        # the order is sol_radiance's: size, samples, first_sample, n, mode
        assert f(stand_in, (1 << 31) + 1, C.byref(_cfg(mode=7))) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
        assert f(stand_in, 2, C.byref(_cfg(samples=0, mode=7))) == _abi.SOL_EINVAL and b"samples" in lib.sol_last_error()
        assert f(stand_in, 2, C.byref(_cfg(size=8, samples=0))) == _abi.SOL_EINVAL and b"size" in lib.sol_last_error()
    # sol_irradiance_rays writes the rays of ONE sample
    rays_fn = _calls(lib, points, out, keys_out)[2][1]
    assert rays_fn(stand_in, 2, C.byref(_cfg(samples=2))) == _abi.SOL_EINVAL and b"samples" in lib.sol_last_error()
    assert bytes(out) == bytes(16 * 4) and bytes(keys_out) == bytes(8 * 2)  # nothing was written


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_a_null_scene_is_einval_not_edevice():
    lib = _abi.load_hip()
    points, out, keys_out = (_abi.SolRay * 1)(), (_abi.SolRadiance * 2)(), (_abi.SolRayKey * 1)()
    for name, f in _calls(lib, points, out, keys_out):
        assert f(None, 1, C.byref(_cfg())) == _abi.SOL_EINVAL, name  # otherwise valid arguments: not SOL_EDEVICE


def test_the_irradiance_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"sol_irradiance_rays_kernel" in data and b"amdgcn-amd-amdhsa--gfx950" in data
    # the gather instances are sol_radiance_kernel<SPILL, STRICT, ENV, LT, GATHER = true>: five template arguments, the last one set
    gather = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb1EE", data))
    plain = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb0EE", data))
    assert len(gather) == 10 and len(plain) == 10, (sorted(gather), sorted(plain))


# ---- the occluder case, predicted on the CPU -------------------------------------------------------------------------------------------
def test_the_occluder_case_is_clear_of_the_cone_s_edge_and_splits_as_the_solid_angle_says():
    """A condition on the seed and geometry tests/test_gpu_irradiance.py uses, checked here without a GPU: of the 64 x 1024 cosine
    directions the float oracle draws (function 8 of its table at first_draw = 0, through the normal's basis in numpy float64) at most 0.5 %
    lie within 1e-4 rad of the cone of half-angle asin(R / d), and the free ones number N (1 - p) within 5 sqrt(N p (1 - p)), p = (R / d)^2."""
    blocked, borderline = iu.occluder_prediction()
    n = blocked.size
    assert blocked.shape == (iu.OCC_POINTS, iu.OCC_SAMPLES) and n == 64 * 1024
    share = borderline.sum() / n
    p = iu.OCC_RATIO ** 2
    free = int((~blocked).sum())
    print(f"borderline {int(borderline.sum())} of {n} ({100 * share:.4f} %); free {free}, expected {n * (1 - p):.0f} +- {np.sqrt(n * p * (1 - p)):.0f}")
    assert share <= 0.005
    assert abs(free - n * (1 - p)) <= 5 * np.sqrt(n * p * (1 - p))
    # (the local directions are the generator's: unit length, in the upper hemisphere)
    local = iu.local_cosine_directions(iu.OCC_SEED, iu.OCC_KEY_BASE + np.arange(4), np.arange(8))
    assert np.allclose((local.astype(np.float64) ** 2).sum(axis=-1), 1.0, atol=1e-6) and (local[..., 2] >= 0).all()
