"""Radiance queries (sol_radiance / sol_radiance_dev / sol_camera_ray_keys), the part that needs no GPU: the three entry points
are exported, the three records have the layout the header states and the ctypes mirrors agree with it, the argument checks that need no
device answer SOL_EINVAL in front of the device check, and the kernels are gfx950 code of the library."""
import ctypes as C
import os
import re

import pytest

from solstrale_amd import _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_radiance_dev", "sol_radiance", "sol_camera_ray_keys")
CTYPES = {"float": (C.c_float, 4), "uint32_t": (C.c_uint32, 4), "uint64_t": (C.c_uint64, 8)}


def _header_struct(name):
    """Field names and C types of `typedef struct <name> { ... } <name>;` in the public header, in order."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in solstrale_hip.h"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_the_three_entry_points_are_exported():
    lib = _abi.load_hip()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\*", open(HEADER).read()), name


@pytest.mark.parametrize("name,mirror,size", [("SolRayKey", _abi.SolRayKey, 8), ("SolRadiance", _abi.SolRadiance, 16),
                                              ("SolRadianceConfig", _abi.SolRadianceConfig, 32)])
def test_the_records_have_the_header_s_layout(name, mirror, size):
    fields = _header_struct(name)
    assert [n for n, _ in mirror._fields_] == [n for n, _ in fields]
    at = 0
    for fname, ctype in fields:  # natural alignment, no padding: the header orders the fields so
        ct, width = CTYPES[ctype]
        assert at % width == 0, (fname, at)
        assert getattr(mirror, fname).offset == at and dict(mirror._fields_)[fname] is ct, fname
        at += width
    assert at == size == C.sizeof(mirror)


def test_the_header_states_the_configuration_s_offsets():
    text = open(HEADER).read()
    m = re.search(r"sizeof\(SolRadianceConfig\) = (\d+): ([^*]*)\*/", text)
    assert m and int(m.group(1)) == C.sizeof(_abi.SolRadianceConfig)
    stated = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", m.group(2))}
    assert stated == {n: getattr(_abi.SolRadianceConfig, n).offset for n, _ in _abi.SolRadianceConfig._fields_}


def _cfg(**kw):
    c = _abi.SolRadianceConfig(size=C.sizeof(_abi.SolRadianceConfig), samples=1)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_null_scene_and_null_configuration_are_einval_before_the_device():
    """With or without a GPU: what needs no device is refused before the device is looked for."""
    lib = _abi.load_hip()
    rays, out, cfg = (_abi.SolRay * 2)(), (_abi.SolRadiance * 2)(), _cfg()
    for f in (lib.sol_radiance, lib.sol_radiance_dev):
        assert f(None, C.byref(rays), None, 2, C.byref(cfg), C.byref(out)) == _abi.SOL_EINVAL
        assert b"null scene" in lib.sol_last_error()
        assert f(None, C.byref(rays), None, 0, C.byref(cfg), C.byref(out)) == _abi.SOL_EINVAL  # (a null scene also with n == 0)
    keys = (_abi.SolRayKey * 2)()
    assert lib.sol_camera_ray_keys(None, 0, 0, 1, 1, 0, 0, C.byref(keys)) == _abi.SOL_EINVAL
    assert b"null scene" in lib.sol_last_error()
    # The configuration and n are judged by a function that is not given the handle (radiance_config_check, sol_api.cpp), right behind the
    # null test of the scene pointer: a zeroed block stands in for a scene - there is no way to make a real one without a device - and is
    # never read. Every call below carries a configuration or an n that is refused there; tests/test_gpu_radiance.py repeats them on a handle.
    stand_in = C.create_string_buffer(1 << 20)
    for f in (lib.sol_radiance, lib.sol_radiance_dev):
        assert f(stand_in, C.byref(rays), None, 2, None, C.byref(out)) == _abi.SOL_EINVAL
        assert b"null configuration" in lib.sol_last_error()
        for bad, word in ((_cfg(size=28), b"size"), (_cfg(reserved=1), b"reserved"), (_cfg(samples=0), b"samples"),
                          (_cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample")):
            assert f(stand_in, C.byref(rays), None, 2, C.byref(bad), C.byref(out)) == _abi.SOL_EINVAL
            assert word in lib.sol_last_error(), lib.sol_last_error()
        assert f(stand_in, C.byref(rays), None, (1 << 31) + 1, C.byref(cfg), C.byref(out)) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
    assert bytes(out) == bytes(16 * 2)  # nothing was written


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_the_argument_checks_still_come_first():
    lib = _abi.load_hip()
    rays, out = (_abi.SolRay * 1)(), (_abi.SolRadiance * 1)()
    assert lib.sol_radiance(None, C.byref(rays), None, 1, C.byref(_cfg()), C.byref(out)) == _abi.SOL_EINVAL  # not SOL_EDEVICE


def test_the_radiance_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"sol_radiance_kernel" in data and b"sol_radiance_resolve_kernel" in data and b"sol_camera_ray_keys_kernel" in data
    assert b"amdgcn-amd-amdhsa--gfx950" in data
