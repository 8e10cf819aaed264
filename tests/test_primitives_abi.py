"""Moving the spheres and quads of a live scene (sol_scene_set_primitives), the part that needs no GPU: sol_sphere_from_center is
Sphere::new and sol_quad_from_corner is Quad::new bit for bit (against the host mirror's flattened SolSphere / SolQuad, which matches the
reference's known answers: tests/test_host.py), the entry points are exported and refuse bad arguments with SOL_EINVAL before any device is
touched, the ctypes structs have the header's sizes, and the creation options struct took the new word in the place of its last reserved one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from solstrale_amd import CameraConfig, RenderConfig, SceneBuilder, _abi, quad_from_corner, scenes, sphere_from_center

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
SPHERE_FIELDS = ("center", "radius", "bbox")
QUAD_FIELDS = ("q", "u", "v", "normal", "d", "w", "area", "bbox")
PAD = 0.0001


def _field_bytes(t, name):
    v = getattr(t, name)
    return bytes(v) if not isinstance(v, float) else np.float64(v).tobytes()


def _inputs():
    """1000 seeded spheres and 1000 seeded quads, then the corners of the two constructors. Every centre and every q is unique: they are the keys
    by which a flattened record (depth-first order) finds its input."""
    rng = np.random.default_rng(1808)
    n = 1000
    spheres = np.concatenate([rng.uniform(-40., 40., (n, 3)), rng.uniform(0.01, 3., (n, 1))], axis=1)
    special_s = {"negative_radius": (50., 1., 2., -1.5), "negative_small": (51., -1., 2., -1e-3), "zero_radius": (52., 1., -2., 0.),
                 "tiny": (1e-30, 2e-30, -3e-30, 1e-30), "huge": (1e12, -1e12, 0.5e12, 3e11), "huge_centre_small_radius": (1e12 + 2., 1., 1., 0.25),
                 "negative_zero_radius": (53., 1., 2., -0.0)}
    spheres = np.concatenate([spheres, np.array(list(special_s.values()), dtype=np.float64)])
    q = rng.uniform(-40., 40., (n, 3))
    u = rng.normal(size=(n, 3)) * rng.uniform(0.01, 5., (n, 1))
    v = rng.normal(size=(n, 3)) * rng.uniform(0.01, 5., (n, 1))
    quads = np.stack([q, u, v], axis=1)
    special_q = {
        "parallel_to_one_axis": ((60., 1., 2.), (2., 0., 0.), (0., 0., 3.)),         # flat in y: one padded axis
        "parallel_to_one_axis_b": ((61., 1., 2.), (0., 2., 1.), (0., -1., 3.)),      # flat in x
        "parallel_to_two_axes": ((62., 1., 2.), (0., 0., 2.), (0., 0., 3.)),         # u parallel to v along z: degenerate, two padded axes
        "degenerate_oblique": ((63., 1., 2.), (1., 2., 3.), (2., 4., 6.)),           # u parallel to v: n = 0, normal and w are 0 / 0
        "degenerate_zero_edge": ((64., 1., 2.), (0., 0., 0.), (1., 1., 1.)),
        "almost_flat": ((65., 1., 2.), (2., 0.00002, 0.), (0., 0.00003, 3.)),        # y extent 5e-5 < PAD_DELTA
        "tiny": ((1e-30, -2e-30, 3e-30), (1e-30, 0., 2e-30), (0., 3e-30, 1e-30)),
        "huge": ((1e12, 2e12, -1e12), (3e11, 1e10, 0.), (0., 2e11, 5e11)),
        "negative_edges": ((66., 1., 2.), (-2., -1., 0.5), (0.5, -3., -1.)),
    }
    quads = np.concatenate([quads, np.array(list(special_q.values()), dtype=np.float64)])
    return spheres, quads, {k: n + i for i, k in enumerate(special_s)}, {k: n + i for i, k in enumerate(special_q)}


@pytest.fixture(scope="module")
def flattened():
    spheres, quads, special_s, special_q = _inputs()
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.5, .5, .5))
    ids = [b.Sphere(tuple(r[:3]), float(r[3]), grey) for r in spheres] + [b.Quad(tuple(r[0]), tuple(r[1]), tuple(r[2]), grey) for r in quads]
    ids.append(b.Sphere((0., 200., 0.), 20., b.DiffuseLight(5., 5., 5.)))
    sc = b.finish(b.Bvh(ids), CameraConfig(40., 0., (0., 0., 150.), (0., 0., 0.), (0., 1., 0.)), (.2, .3, .5), RenderConfig(16, 16, 1))
    return sc, spheres, quads, special_s, special_q


def test_sphere_from_center_is_the_host_mirror_bit_for_bit(flattened):
    sc, spheres, quads, special, _ = flattened
    d = sc.desc
    by_centre = {spheres[i, :3].tobytes(): i for i in range(len(spheres))}
    assert len(by_centre) == len(spheres) and d.n_spheres == len(spheres) + 1
    seen = set()
    for j in range(d.n_spheres):
        want = d.spheres[j]
        i = by_centre.get(bytes(want.center))
        if i is None:
            continue  # the light
        seen.add(i)
        got = _abi.SolSphere(material=-77, dfs_index=0xABCDEF)
        sphere_from_center(spheres[i, :3], spheres[i, 3], out=got)
        for f in SPHERE_FIELDS:
            assert _field_bytes(got, f) == _field_bytes(want, f), (i, f)
        assert got.material == -77 and got.dfs_index == 0xABCDEF  # left alone
    assert len(seen) == len(spheres)
    neg = sphere_from_center(spheres[special["negative_radius"], :3], spheres[special["negative_radius"], 3])
    assert neg.radius == -1.5 and list(neg.bbox.v) == [48.5, 51.5, -0.5, 2.5, 0.5, 3.5]  # the box of |r|, the radius as given
    zero = sphere_from_center(spheres[special["zero_radius"], :3], 0.)
    assert list(zero.bbox.v) == [52., 52., 1., 1., -2., -2.]


def test_quad_from_corner_is_the_host_mirror_bit_for_bit(flattened):
    sc, spheres, quads, _, special = flattened
    d = sc.desc
    by_q = {quads[i, 0].tobytes(): i for i in range(len(quads))}
    assert len(by_q) == len(quads) and d.n_quads == len(quads)
    seen, padded_axes, nan_normals = set(), {0: 0, 1: 0, 2: 0, 3: 0}, 0
    for j in range(d.n_quads):
        want = d.quads[j]
        i = by_q[bytes(want.q)]
        seen.add(i)
        got = _abi.SolQuad(material=-77, dfs_index=0xABCDEF)
        quad_from_corner(quads[i, 0], quads[i, 1], quads[i, 2], out=got)
        for f in QUAD_FIELDS:
            assert _field_bytes(got, f) == _field_bytes(want, f), (i, f, list(np.atleast_1d(getattr(got, f))), list(np.atleast_1d(getattr(want, f))))
        assert got.material == -77 and got.dfs_index == 0xABCDEF
        corners = np.array([quads[i, 0], quads[i, 0] + quads[i, 1], quads[i, 0] + quads[i, 2], quads[i, 0] + quads[i, 1] + quads[i, 2]])
        box = np.array(got.bbox.v[:]).reshape(3, 2)
        exact = np.stack([corners.min(axis=0), corners.max(axis=0)], axis=1)
        padded_axes[int((box != exact).any(axis=1).sum())] += 1
        nan_normals += int(np.isnan(np.array(got.normal[:])).all())
    assert len(seen) == len(quads)
    assert padded_axes[1] >= 3 and padded_axes[2] >= 1 and nan_normals >= 3, (padded_axes, nan_normals)
    one = quad_from_corner(*quads[special["parallel_to_one_axis"]])
    assert list(one.bbox.v) == [60., 62., 1. - PAD / 2., 1. + PAD / 2., 2., 5.] and list(one.normal) == [0., -1., 0.] and one.area == 6.0 and one.d == -1.0
    two = quad_from_corner(*quads[special["parallel_to_two_axes"]])
    assert list(two.bbox.v) == [62. - PAD / 2., 62. + PAD / 2., 1. - PAD / 2., 1. + PAD / 2., 2., 7.]
    deg = quad_from_corner(*quads[special["degenerate_oblique"]])
    assert deg.area == 0.0 and np.isnan(np.array(deg.normal[:])).all() and np.isnan(np.array(deg.w[:])).all() and np.isnan(deg.d)
    # the NaN pattern: the host's default NaN (sign bit set on x86-64), as the flattened record holds it
    assert np.array(deg.normal[:]).view(np.uint64).tolist() == [0xFFF8000000000000] * 3


def test_the_entry_points_are_exported_and_the_structs_have_the_headers_sizes():
    lib = _abi.load_hip()
    for name in ("sol_sphere_from_center", "sol_quad_from_corner", "sol_scene_set_primitives", "sol_scene_primitive_records"):
        assert hasattr(lib, name) and name in _abi.HIP_SYMBOLS
    text = open(HEADER).read()
    assert re.search(r"#define SOL_PRIMS_DEVICE\s+1u", text) and _abi.SOL_PRIMS_DEVICE == 1
    m = re.search(r"typedef struct SolPrimitiveSet \{(.*?)\} SolPrimitiveSet;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = re.findall(r"[A-Za-z_]\w*", re.sub(r"\b(const|double|uint32_t)\b|\[\d+\]", "", body))
    assert names == [f[0] for f in _abi.SolPrimitiveSet._fields_], names  # the same fields in the same order
    # uint32 size, flags; three pointers; three counts; three reserved words
    assert C.sizeof(_abi.SolPrimitiveSet) == 8 + 3 * C.sizeof(C.c_void_p) + 12 + 12 == 56
    assert _abi.SolPrimitiveSet.triangles.offset == 8 and _abi.SolPrimitiveSet.n_triangles.offset == 32 and _abi.SolPrimitiveSet.reserved.offset == 44
    sizes = (C.c_uint32 * 11)()
    _abi.load_host().solh_abi_sizes(sizes)
    assert C.sizeof(_abi.SolSphere) == sizes[2] == 88 and C.sizeof(_abi.SolQuad) == sizes[3] == 192
    from solstrale_amd import DeviceScene
    assert DeviceScene.SPHERE_DTYPE.itemsize == 32 and DeviceScene.QUAD_DTYPE.itemsize == 80


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    for name in (b"sol_sphere_records_kernel", b"sol_quad_records_kernel", b"sol_primitive_lights_kernel", b"sol_refit_level8_kernel"):
        assert name in data, name


def test_argument_errors_are_einval_before_the_device():
    """Null arguments, all three pointers null, and structs no version of the header had (sizes, flag bits, reserved words) - on a null handle where
    the check comes before the handle is looked at, so with or without a GPU."""
    lib = _abi.load_hip()
    rows = np.zeros((1, 4))
    S, U = _abi.SolPrimitiveSet, _abi.SolGeometryUpdate
    good, good_u = C.sizeof(S), C.sizeof(U)

    def call(h, ps, upd=None):
        return lib.sol_scene_set_primitives(h, C.byref(ps) if ps is not None else None, C.byref(upd) if upd is not None else None)

    ok = S(size=good, spheres=rows.ctypes.data, n_spheres=1)
    assert call(None, ok) == _abi.SOL_EINVAL and b"null scene" in lib.sol_last_error()
    assert call(None, None) == _abi.SOL_EINVAL
    fake = C.c_void_p(0)  # (the checks below come before the handle: a null one shows that)
    for ps, what in ((S(size=4), b"SolPrimitiveSet.size"), (S(size=4097), b"SolPrimitiveSet.size"),
                     (S(size=good, flags=2, spheres=rows.ctypes.data, n_spheres=1), b"unknown bits"),
                     (S(size=good, flags=0x80000001, spheres=rows.ctypes.data, n_spheres=1), b"unknown bits"),
                     (S(size=good, spheres=rows.ctypes.data, n_spheres=1, reserved=(C.c_uint32 * 3)(0, 0, 1)), b"SolPrimitiveSet.reserved"),
                     (S(size=good, spheres=rows.ctypes.data, n_spheres=1, reserved=(C.c_uint32 * 3)(1, 0, 0)), b"SolPrimitiveSet.reserved")):
        assert call(fake, ps) == _abi.SOL_EINVAL
        assert what in lib.sol_last_error(), (what, lib.sol_last_error())
    for upd, what in ((U(size=4), b"SolGeometryUpdate.size"), (U(size=4097), b"SolGeometryUpdate.size"), (U(size=good_u, flags=4), b"unknown bits"),
                      (U(size=good_u, reserved=(C.c_uint32 * 2)(0, 1)), b"reserved")):
        assert call(fake, ok, upd) == _abi.SOL_EINVAL
        assert what in lib.sol_last_error(), (what, lib.sol_last_error())
    # the CPU constructors
    sp, qd = _abi.SolSphere(), _abi.SolQuad()
    v = np.array([1., 2., 3.])
    assert lib.sol_sphere_from_center(None, 1.0, C.byref(sp)) == _abi.SOL_EINVAL
    assert lib.sol_sphere_from_center(v.ctypes.data, 1.0, None) == _abi.SOL_EINVAL
    assert lib.sol_sphere_from_center(v.ctypes.data, 1.0, C.byref(sp)) == _abi.SOL_OK
    for args in ((None, v.ctypes.data, v.ctypes.data, C.byref(qd)), (v.ctypes.data, None, v.ctypes.data, C.byref(qd)),
                 (v.ctypes.data, v.ctypes.data, None, C.byref(qd)), (v.ctypes.data, v.ctypes.data, v.ctypes.data, None)):
        assert lib.sol_quad_from_corner(*args) == _abi.SOL_EINVAL
    assert lib.sol_quad_from_corner(v.ctypes.data, v.ctypes.data, v.ctypes.data, C.byref(qd)) == _abi.SOL_OK
    n = C.c_uint32(7)
    assert lib.sol_scene_primitive_records(None, _abi.REF_SPHERE, None, None, 0, C.byref(n)) == _abi.SOL_EINVAL and n.value == 7


def test_the_python_route_refuses_what_it_can_tell():
    from solstrale_amd import DeviceScene
    ds = DeviceScene.__new__(DeviceScene)  # (no handle: the argument checks come first)
    ds.h, ds.lib, ds.device = None, _abi.load_hip(), 0
    with pytest.raises(ValueError):
        ds.set_primitives()
    with pytest.raises(ValueError):
        ds.set_primitives(spheres=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        ds.set_primitives(quads=np.zeros((2, 9)))

    class FakeTensor:  # (mixing the routes is told before torch is needed)
        def data_ptr(self):
            return 16

    with pytest.raises(ValueError, match="one call"):
        ds.set_primitives(spheres=np.zeros((2, 4)), quads=FakeTensor())


def test_dynamic_primitives_took_the_last_reserved_word():
    """40 bytes as before, the new word at offset 36 where reserved2 was; both layouts pass the option checks (the creation then fails for want of a
    device, or succeeds on one). The word is 0 or 1, and 1 only together with dynamic_triangles, which it extends."""
    lib = _abi.load_hip()
    O = _abi.SolCreateOptions
    assert C.sizeof(O) == 40 and O.dynamic_triangles.offset == 32 and O.dynamic_primitives.offset == 36
    assert re.search(r"int32_t dynamic_triangles;.*?int32_t dynamic_primitives;[^}]*\} SolCreateOptions;", open(HEADER).read(), re.S)
    sc = scenes.cornell_box(RenderConfig(16, 16, 1))

    def create(opt):
        h = C.c_void_p()
        rc = lib.sol_scene_create_ex(sc.desc_ptr, 0, C.byref(opt), C.byref(h))
        if h:
            lib.sol_scene_destroy(h)
        return rc

    passed = (_abi.SOL_EDEVICE, _abi.SOL_OK)
    assert create(O(size=40, dynamic_triangles=1, dynamic_primitives=1)) in passed
    assert create(O(size=40, dynamic_triangles=1)) in passed and create(O(size=40)) in passed
    assert create(O(size=32, dynamic_triangles=7, dynamic_primitives=9)) in passed  # behind the caller's struct: not read
    assert create(O(size=36, dynamic_triangles=1, dynamic_primitives=9)) in passed
    assert create(O(size=40, dynamic_primitives=1)) == _abi.SOL_EINVAL and b"dynamic_triangles" in lib.sol_last_error()
    assert create(O(size=40, dynamic_triangles=1, dynamic_primitives=2)) == _abi.SOL_EINVAL and b"dynamic_primitives" in lib.sol_last_error()
    assert create(O(size=40, dynamic_triangles=1, dynamic_primitives=-1)) == _abi.SOL_EINVAL
