"""Moving the triangles of a live scene (sol_scene_set_triangles), the part that needs no GPU: sol_triangle_from_vertices is
Triangle::new_with_tex_coords bit for bit (against the host mirror, which matches the reference's known answers: tests/test_host.py), the
entry points are exported and refuse bad arguments with SOL_EINVAL before any device is touched, and the creation options struct grew
without breaking the callers of its first layout."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from solstrale_amd import CameraConfig, RenderConfig, SceneBuilder, _abi, scenes, triangle_from_vertices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
GEOMETRIC = ("v0", "v0v1", "v0v2", "normal", "tangent", "bi_tangent", "area", "uv0", "uv1", "uv2", "bbox")


def _field_bytes(t, name):
    v = getattr(t, name)
    return bytes(v) if not isinstance(v, float) else np.float64(v).tobytes()


def _special_triangles():
    """(name, vertices 3x3, uv 3x2): the corners of the constructor."""
    T = []
    uv = [(0.1, 0.2), (0.9, 0.15), (0.4, 0.8)]
    T.append(("large_coordinates", [(1e6 + 0.25, 1e6 - 3.5, -1e6 + 0.125), (1e6 + 2.75, 1e6 + 1.5, -1e6 - 1.0), (1e6 - 1.5, 1e6 + 0.5, -1e6 + 2.0)], uv))
    T.append(("small_coordinates", [(1.5e-6, -2e-6, 3e-6), (4e-6, 1e-6, -1e-6), (-2e-6, 3.5e-6, 2.5e-6)], uv))
    T.append(("thin_on_one_axis", [(7., 1., 2.), (7.00002, 3., 2.5), (7.00001, 1.5, 4.)], uv))            # x extent 2e-5 < PAD_DELTA
    T.append(("thin_on_two_axes", [(8., 1., 2.), (8.00003, 1.00004, 5.), (8.00001, 1.00002, 3.)], uv))
    T.append(("thin_on_three_axes", [(9., 1., 2.), (9.00003, 1.00004, 2.00002), (9.00001, 1.00002, 2.00005)], uv))
    T.append(("flat_axis_aligned", [(10., 0., 0.), (11., 0., 0.), (10., 0., 1.5)], uv))                     # y extent exactly 0
    T.append(("equal_uvs", [(12., 0., 0.), (13., 0.5, 0.), (12., 1., 1.)], [(0.5, 0.5)] * 3))                # r = 1 / 0: NaN tangents
    T.append(("zero_uvs", [(14., 0., 0.), (15., 0.5, 0.), (14., 1., 1.)], [(0., 0.)] * 3))
    T.append(("zero_area", [(16., 0., 0.), (17., 1., 2.), (18., 2., 4.)], uv))                               # collinear: n = 0, normal 0 / 0
    # the three rotations (sol_triangle_rotation: the record starts opposite the longest edge)
    T.append(("rotation_0", [(20., 0., 0.), (20., 5., 0.), (20., 0., 5.)], uv))    # longest: v1v2
    T.append(("rotation_1", [(22., 0., 0.), (22., 1., 0.), (22., 0., 7.)], uv))    # longest: v2v0 ... or v1v2; checked below
    T.append(("rotation_2", [(24., 0., 0.), (24., 9., 0.), (24., 4., 1.)], uv))    # longest: v0v1
    return T


@pytest.fixture(scope="module")
def flattened():
    """One scene of 1000 seeded triangles plus the special ones, built with SceneBuilder.triangles and flattened: (scene, inputs by v0 bytes)."""
    rng = np.random.default_rng(1707)
    n = 1000
    centre = rng.uniform(-40., 40., (n, 1, 3))
    verts = centre + rng.normal(size=(n, 3, 3)) * rng.uniform(0.01, 3., (n, 1, 1))
    uvs = rng.uniform(0., 1., (n, 3, 2)).astype(np.float32)
    special = _special_triangles()
    verts = np.concatenate([verts, np.array([s[1] for s in special], dtype=np.float64)])
    uvs = np.concatenate([uvs, np.array([s[2] for s in special], dtype=np.float32)])
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.5, .5, .5))
    first, count = b.triangles(verts, grey, uvs)
    light = b.Sphere((0., 200., 0.), 20., b.DiffuseLight(5., 5., 5.))
    sc = b.finish(b.Bvh(list(range(first, first + count)) + [light]), CameraConfig(40., 0., (0., 0., 150.), (0., 0., 0.), (0., 1., 0.)), (.2, .3, .5),
                  RenderConfig(16, 16, 1))
    by_v0 = {verts[i, 0].tobytes(): i for i in range(len(verts))}
    assert len(by_v0) == len(verts)
    return sc, verts, uvs, by_v0, {s[0]: n + k for k, s in enumerate(special)}


def test_triangle_from_vertices_is_the_host_mirror_bit_for_bit(flattened):
    sc, verts, uvs, by_v0, special = flattened
    d = sc.desc
    assert d.n_triangles == len(verts)
    seen, rotations, nan_tangents, padded_axes = set(), set(), 0, {0: 0, 1: 0, 2: 0, 3: 0}
    for j in range(d.n_triangles):
        want = d.triangles[j]
        i = by_v0[bytes(want.v0)]
        seen.add(i)
        got = _abi.SolTriangle(material=-77, dfs_index=0xABCDEF)
        triangle_from_vertices(verts[i], uvs[i], out=got)
        for f in GEOMETRIC:
            assert _field_bytes(got, f) == _field_bytes(want, f), (i, f, list(np.atleast_1d(getattr(got, f))), list(np.atleast_1d(getattr(want, f))))
        assert got.material == -77 and got.dfs_index == 0xABCDEF  # left alone
        rotations.add(_rotation(got))
        nan_tangents += int(np.isnan(np.array(got.tangent[:])).all())
        box = np.array(got.bbox.v[:]).reshape(3, 2)
        exact = np.stack([verts[i].min(axis=0), verts[i].max(axis=0)], axis=1)
        padded_axes[int((box != exact).any(axis=1).sum())] += 1
    assert len(seen) == len(verts)
    assert rotations == {0, 1, 2}
    assert nan_tangents >= 2 and padded_axes[1] >= 2 and padded_axes[2] >= 1 and padded_axes[3] >= 1, (nan_tangents, padded_axes)
    z = triangle_from_vertices(verts[special["zero_area"]], uvs[special["zero_area"]])
    assert z.area == 0.0 and np.isnan(np.array(z.normal[:])).all()


def _rotation(t):
    """sol_triangle_rotation (include/solstrale_hip.h) in numpy."""
    a, b = np.array(t.v0v1[:]), np.array(t.v0v2[:])
    c = b - a
    l01, l02, l12 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2], (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    k, best = 0, l12
    if l02 > best:
        best, k = l02, 1
    if l01 > best:
        k = 2
    return k


def test_the_entry_points_are_exported_and_the_header_states_the_contract():
    lib = _abi.load_hip()
    for name in ("sol_triangle_from_vertices", "sol_scene_set_triangles", "sol_scene_set_triangles_dev", "sol_scene_set_triangles_ms", "sol_scene_triangle_records"):
        assert hasattr(lib, name) and name in _abi.HIP_SYMBOLS
    text = open(HEADER).read()
    assert re.search(r"#define SOL_GEOM_NO_BACKGROUND_PROOF\s+1u", text) and _abi.SOL_GEOM_NO_BACKGROUND_PROOF == 1
    assert re.search(r"#define SOL_GEOM_REPROBE\s+2u", text) and _abi.SOL_GEOM_REPROBE == 2
    assert re.search(r"#define SOL_ERANGE \(-6\)", text) and _abi.SOL_ERANGE == -6
    assert re.search(r"typedef struct SolGeometryUpdate \{ uint32_t size, flags, reserved\[2\]; \} SolGeometryUpdate;", text)
    assert C.sizeof(_abi.SolGeometryUpdate) == 16


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    for name in (b"sol_triangle_records_kernel", b"sol_triangle_lights_kernel", b"sol_refit_level8_kernel"):
        assert name in data, name


def test_argument_errors_are_einval_before_the_device():
    """Null arguments, and a SolGeometryUpdate no version of the header had (its size, flag bits, reserved words) - with or without a GPU."""
    lib = _abi.load_hip()
    v = np.zeros((1, 3, 3))
    good = C.sizeof(_abi.SolGeometryUpdate)
    for fn in (lib.sol_scene_set_triangles, lib.sol_scene_set_triangles_dev):
        assert fn(None, v.ctypes.data, 1, None) == _abi.SOL_EINVAL
        assert b"null scene" in lib.sol_last_error()
        assert fn(None, None, 0, None) == _abi.SOL_EINVAL
        for upd, what in ((_abi.SolGeometryUpdate(size=4), b"size"), (_abi.SolGeometryUpdate(size=4097), b"size"),
                          (_abi.SolGeometryUpdate(size=good, flags=4), b"unknown bits"), (_abi.SolGeometryUpdate(size=good, flags=0x80000001), b"unknown bits"),
                          (_abi.SolGeometryUpdate(size=good, reserved=(C.c_uint32 * 2)(0, 1)), b"reserved"),
                          (_abi.SolGeometryUpdate(size=good, reserved=(C.c_uint32 * 2)(1, 0)), b"reserved")):
            assert fn(None, v.ctypes.data, 1, C.byref(upd)) == _abi.SOL_EINVAL
            assert what in lib.sol_last_error(), (what, lib.sol_last_error())
    t = _abi.SolTriangle()
    uv = np.zeros(6, dtype=np.float32)
    assert lib.sol_triangle_from_vertices(None, uv.ctypes.data, C.byref(t)) == _abi.SOL_EINVAL
    assert lib.sol_triangle_from_vertices(v.ctypes.data, None, C.byref(t)) == _abi.SOL_EINVAL
    assert lib.sol_triangle_from_vertices(v.ctypes.data, uv.ctypes.data, None) == _abi.SOL_EINVAL
    assert lib.sol_triangle_from_vertices(v.ctypes.data, uv.ctypes.data, C.byref(t)) == _abi.SOL_OK
    ms = (C.c_float * 4)()
    assert lib.sol_scene_set_triangles_ms(None, ms) == _abi.SOL_EINVAL
    n = C.c_uint32(7)
    assert lib.sol_scene_triangle_records(None, None, None, None, 0, C.byref(n)) == _abi.SOL_EINVAL and n.value == 7


def test_the_options_struct_grew_behind_its_reserved_words():
    """40 bytes now; the 32-byte layout of earlier callers still passes the option checks (the creation then fails for want of a device, or
    succeeds on one), and what lies behind a 32-byte struct is not read. The new words are checked: dynamic_triangles is 0 or 1, reserved2 is 0."""
    lib = _abi.load_hip()
    O = _abi.SolCreateOptions
    assert C.sizeof(O) == 40 and O.reserved.offset == 24 and O.dynamic_triangles.offset == 32 and O.reserved2.offset == 36
    sc = scenes.cornell_box(RenderConfig(16, 16, 1))

    def create(opt):
        h = C.c_void_p()
        rc = lib.sol_scene_create_ex(sc.desc_ptr, 0, C.byref(opt), C.byref(h))
        if h:
            lib.sol_scene_destroy(h)
        return rc

    passed = (_abi.SOL_EDEVICE, _abi.SOL_OK)
    assert create(O(size=40)) in passed and create(O(size=40, dynamic_triangles=1)) in passed
    assert create(O(size=32)) in passed
    assert create(O(size=32, dynamic_triangles=7, reserved2=9)) in passed          # behind the caller's struct: not read
    assert create(O(size=40, reserved=(C.c_int32 * 2)(5, -1))) in passed           # the old reserved words were never checked
    assert create(O(size=40, dynamic_triangles=2)) == _abi.SOL_EINVAL and b"dynamic_triangles" in lib.sol_last_error()
    assert create(O(size=40, dynamic_triangles=-1)) == _abi.SOL_EINVAL
    assert create(O(size=40, reserved2=1)) == _abi.SOL_EINVAL and b"reserved2" in lib.sol_last_error()
