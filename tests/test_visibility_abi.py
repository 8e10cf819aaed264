"""Visibility gathers (sol_visibility / sol_visibility_dev), the part that needs no GPU: both entry points are exported and
declared, SolVisibility has 32 bytes and the stated offsets on both sides, every refusal that needs no handle answers SOL_EINVAL in the
stated order and in front of the device check, the kernels are gfx950 code of the library in eight instances - and the occluder case of
tests/test_gpu_visibility.py is a fair one: its directions stay clear of the cone's edge and its hit distances lie where the geometry says."""
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
ENTRY_POINTS = ("sol_visibility_dev", "sol_visibility")
CFG = _abi.SolIrradianceConfig
OFFSETS = {"bx": 0, "by": 4, "bz": 8, "open": 12, "t_sum": 16, "t2_sum": 20, "hits": 24, "samples": 28}
OCCLUDED, CLOSEST = _abi.SOL_QUERY_OCCLUDED, _abi.SOL_QUERY_CLOSEST


def test_both_entry_points_are_exported_and_declared():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, int mode,", text), name
        assert re.search(r"\b" + name + r"\b", open(os.path.join(ROOT, "INTEGRATION.md")).read()), name
    assert getattr(lib, "sol_visibility").argtypes is not None and len(lib.sol_visibility.argtypes) == 7 and len(lib.sol_visibility_dev.argtypes) == 7


def test_solvisibility_has_32_bytes_and_the_stated_offsets_on_both_sides(tmp_path):
    assert C.sizeof(_abi.SolVisibility) == 32
    assert {n: getattr(_abi.SolVisibility, n).offset for n, _ in _abi.SolVisibility._fields_} == OFFSETS
    from solstrale_amd import DeviceScene
    dt = DeviceScene.VISIBILITY_DTYPE
    assert dt.itemsize == 32 and {n: dt.fields[n][1] for n in dt.names} == {"bent": 0, "open": 12, "t_sum": 16, "t2_sum": 20, "hits": 24, "samples": 28}
    fields = ", ".join(f"(unsigned)offsetof(SolVisibility, {n})" for n in OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("%u" "{" %u" * len(OFFSETS)}", (unsigned)sizeof(SolVisibility), {fields});\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [32] + list(OFFSETS.values())


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), samples=1)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _calls(lib, points, out):
    return (("sol_visibility", lambda s, mode, n, c: lib.sol_visibility(s, mode, C.byref(points), None, n, c, C.byref(out))),
            ("sol_visibility_dev", lambda s, mode, n, c: lib.sol_visibility_dev(s, mode, C.byref(points), None, n, c, C.byref(out))))


def test_every_refusal_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene (tests/test_irradiance_abi.py): nothing in front of n == 0 reads the handle.
    The order: a null scene; an unknown mode; the configuration and n in sol_irradiance's order (size, samples, first_sample, n, direction mode);
    then n == 0 succeeds. (tests/test_gpu_visibility.py adds the refusals that read the handle: a constant medium, null pointers.)"""
    lib = _abi.load_hip()
    points, out = (_abi.SolRay * 2)(), (_abi.SolVisibility * 2)()
    stand_in = C.create_string_buffer(1 << 20)
    err = lib.sol_last_error
    for name, f in _calls(lib, points, out):
        tag = name.encode() + b":"
        for n in (2, 0):  # (a null scene also with n == 0, and in front of an unknown mode and a null configuration)
            assert f(None, OCCLUDED, n, C.byref(_cfg())) == _abi.SOL_EINVAL, name
            assert b"null scene" in err() and tag in err()
            assert f(None, 7, n, None) == _abi.SOL_EINVAL and b"null scene" in err()
        # an unknown mode is named, in sol_query's sentence, in front of everything about the configuration and also with n == 0
        for mode in (2, -1, 7):
            for n, c in ((2, C.byref(_cfg())), (0, C.byref(_cfg())), (2, None), (2, C.byref(_cfg(samples=0))), ((1 << 31) + 1, C.byref(_cfg()))):
                assert f(stand_in, mode, n, c) == _abi.SOL_EINVAL, (name, mode)
                assert f"unknown mode {mode} (SOL_QUERY_CLOSEST or SOL_QUERY_OCCLUDED)".encode() in err() and tag in err(), err()
        for mode in (OCCLUDED, CLOSEST):
            assert f(stand_in, mode, 2, None) == _abi.SOL_EINVAL and b"null configuration" in err()
            for bad, word in ((_cfg(size=28), b"size"), (_cfg(size=0), b"size"), (_cfg(samples=0), b"samples"),
                              (_cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample"), (_cfg(mode=2), b"unknown mode 2 (SOL_IRRADIANCE_COSINE"),
                              (_cfg(mode=0xFFFFFFFF), b"SOL_IRRADIANCE_SPHERE")):
                for n in (2, 0):  # (the configuration is judged in front of n == 0)
                    assert f(stand_in, mode, n, C.byref(bad)) == _abi.SOL_EINVAL, (name, word)
                    assert word in err() and tag in err(), (name, err())
            assert f(stand_in, mode, (1 << 31) + 1, C.byref(_cfg())) == _abi.SOL_EINVAL and b"2^31" in err() and b"points" in err()
            # sol_irradiance's order: size, samples, first_sample, n, direction mode
            assert f(stand_in, mode, (1 << 31) + 1, C.byref(_cfg(mode=7))) == _abi.SOL_EINVAL and b"2^31" in err()
            assert f(stand_in, mode, 2, C.byref(_cfg(samples=0, mode=7))) == _abi.SOL_EINVAL and b"samples" in err()
            assert f(stand_in, mode, 2, C.byref(_cfg(size=8, samples=0))) == _abi.SOL_EINVAL and b"size" in err()
            # n == 0 is SOL_OK: nothing is read behind the scene pointer (the medium is judged after it), nothing is written
            assert f(stand_in, mode, 0, C.byref(_cfg())) == _abi.SOL_OK, name
            assert f(stand_in, mode, 0, C.byref(_cfg(mode=_abi.SOL_IRRADIANCE_SPHERE, samples=40))) == _abi.SOL_OK, name
    assert bytes(out) == bytes(32 * 2)  # nothing was written


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_a_null_scene_is_einval_not_edevice():
    lib = _abi.load_hip()
    points, out = (_abi.SolRay * 1)(), (_abi.SolVisibility * 1)()
    for name, f in _calls(lib, points, out):
        assert f(None, OCCLUDED, 1, C.byref(_cfg())) == _abi.SOL_EINVAL, name  # otherwise valid arguments: not SOL_EDEVICE


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"sol_visibility_resolve_kernel" in data and b"amdgcn-amd-amdhsa--gfx950" in data
    # sol_visibility_kernel<ANY, SPILL, STRICT>: every combination
    vis = set(re.findall(rb"_Z21sol_visibility_kernelILb[01]ELb[01]ELb[01]EE", data))
    assert len(vis) == 8, sorted(vis)
    # the radiance family is what it was (tests/test_irradiance_abi.py, tests/test_irradiance_sh_abi.py)
    gather = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb1EE", data))
    plain = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb0EE", data))
    each = set(re.findall(rb"_Z24sol_radiance_each_kernelILb[01]ELb[01]ELb[01]ELb[01]EE", data))
    assert (len(gather), len(plain), len(each)) == (10, 10, 10)


# ---- the occluder case, predicted on the CPU -------------------------------------------------------------------------------------------
def test_the_occluder_case_is_clear_of_the_edge_and_its_hit_distances_lie_where_the_geometry_says():
    """The conditions tests/test_gpu_visibility.py relies on, for the seed and geometry of tests/irradiance_util.py: of the 64 x 1024 cosine
    directions at most 0.5 % are borderline, and the sphere's near intersection along every direction that is surely blocked - D cos(a) -
    sqrt(R^2 - D^2 sin^2(a)) at the angle a to the normal, in float64 - lies in [D - R, sqrt(D^2 - R^2)] = [0.8, 1.6]: from the pole of the
    sphere to its silhouette."""
    blocked, borderline = iu.occluder_prediction()
    assert blocked.shape == (iu.OCC_POINTS, iu.OCC_SAMPLES) == (64, 1024)
    assert borderline.sum() <= 0.005 * blocked.size
    D, R = iu.OCC_D, iu.OCC_R
    assert abs((D - R) - 0.8) < 1e-12 and abs(np.sqrt(D * D - R * R) - 1.6) < 1e-12
    keys = iu.OCC_KEY_BASE + np.arange(iu.OCC_POINTS)
    local = iu.local_cosine_directions(iu.OCC_SEED, keys, np.arange(iu.OCC_SAMPLES)).astype(np.float64)
    sure = blocked & ~borderline
    assert sure.sum() > 0.3 * blocked.size  # (sin^2 of the cone is 0.36)
    length = np.sqrt((local * local).sum(axis=-1))
    cosa = local[..., 2][sure] / length[sure]  # (the local frame's z is the normal)
    sin2 = 1.0 - cosa * cosa
    near = D * cosa - np.sqrt(R * R - D * D * sin2)
    print(f"occluder: {int(sure.sum())} sure-blocked directions, {int(borderline.sum())} borderline; near hit distance in [{near.min():.4f}, {near.max():.4f}]")
    assert near.min() >= D - R and near.max() <= np.sqrt(D * D - R * R)
