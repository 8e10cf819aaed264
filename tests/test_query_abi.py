"""Ray queries, the part that needs no GPU: the three entry points are exported, SolRay and SolRayHit have the layout the header states,
the ctypes mirrors agree with it, the calls fail with SOL_EDEVICE where there is no device, and nothing else of the ABI moved."""
import ctypes as C
import os
import re

import pytest

from solstrale_amd import _abi, device_count, record_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_query_dev", "sol_query", "sol_camera_rays")


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


def test_the_query_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"sol_query_kernel" in data and b"sol_camera_rays_kernel" in data


@pytest.mark.parametrize("name,mirror", [("SolRay", _abi.SolRay), ("SolRayHit", _abi.SolRayHit)])
def test_ray_and_hit_are_32_bytes_and_the_mirrors_have_the_header_layout(name, mirror):
    fields = _header_struct(name)
    assert len(fields) == 8 and all(t in ("float", "uint32_t") for _, t in fields)  # eight 4-byte words: field k lies at byte 4 k
    assert C.sizeof(mirror) == 32
    assert [n for n, _ in mirror._fields_] == [n for n, _ in fields]
    for k, (fname, ctype) in enumerate(fields):
        assert getattr(mirror, fname).offset == 4 * k, fname
        assert dict(mirror._fields_)[fname] is (C.c_float if ctype == "float" else C.c_uint32), fname


def test_the_constants_match_the_header():
    text = open(HEADER).read()
    assert re.search(r"enum \{ SOL_QUERY_CLOSEST = 0, SOL_QUERY_OCCLUDED = 1 \};", text)
    assert re.search(r"enum \{ SOL_RAY_MISS = 0, SOL_RAY_HIT = 1, SOL_RAY_INVALID = 2 \};", text)
    assert (_abi.SOL_QUERY_CLOSEST, _abi.SOL_QUERY_OCCLUDED) == (0, 1)
    assert (_abi.SOL_RAY_MISS, _abi.SOL_RAY_HIT, _abi.SOL_RAY_INVALID) == (0, 1, 2)


def test_the_structured_hit_dtype_is_the_c_record():
    from solstrale_amd import DeviceScene
    dt = DeviceScene.RAY_HIT_DTYPE
    assert dt.itemsize == 32 and list(dt.names) == [n for n, _ in _abi.SolRayHit._fields_]
    assert [dt.fields[n][1] for n in dt.names] == [4 * k for k in range(8)]


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_the_calls_return_edevice():
    lib = _abi.load_hip()
    rays = (_abi.SolRay * 2)()
    hits = (_abi.SolRayHit * 2)()
    assert lib.sol_query(None, _abi.SOL_QUERY_CLOSEST, C.byref(rays), 2, C.byref(hits)) == _abi.SOL_EDEVICE
    assert b"no HIP device" in lib.sol_last_error()
    assert lib.sol_query_dev(None, _abi.SOL_QUERY_OCCLUDED, C.byref(rays), 2, C.byref(hits)) == _abi.SOL_EDEVICE
    assert lib.sol_camera_rays(None, 0, 0, 1, 1, 0, 0, C.byref(rays)) == _abi.SOL_EDEVICE


def test_abi_version_and_record_sizes_are_unchanged():
    text = open(HEADER).read()
    assert re.search(r"#define SOL_ABI_VERSION 2\b", text) and _abi.SOL_ABI_VERSION == 2
    assert record_sizes() == {"node": 64, "sphere": 32, "quad": 80, "triangle": 48, "triangle_shade": 64, "material": 48}
    lib = _abi.load_host()
    sizes = (C.c_uint32 * 11)()
    lib.solh_abi_sizes(sizes)
    assert [int(x) for x in sizes] == [C.sizeof(s) for s in _abi.ABI_STRUCTS]
