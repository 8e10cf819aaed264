"""The 7-wide node test's byte-permute selectors (sol_trace.h, SOL_SEL_TABLE; the render kernel and the query kernels both read them from
their LDS table) over every selector path: a closed shell of small triangles around the origin plus one quad, rays from inside and from
outside in all octants, along the axes with both signed zeros and with exactly one zero component.
Closest hits through sol_query are compared with the float oracle's own closest hit (status, t bit for bit, material) and, for triangle
hits, with a host evaluation of the fp32 contract's triangle test in numpy float32 over ALL triangles (the rotated records of
include/solstrale_hip.h, the operation order of sol_trace.h tri_test): t, the primitive (dfs_index), u and v bit for bit.
Frames of the same scene from the render kernel against the oracle's frame: the plain build, and the SPILL + STRICT build (a deep nested
chain under SOL_BVH=ref, one needle triangle)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import orc
import parity_util as pu
from far_rays import host_triangle_hits
from solstrale_amd import CameraConfig, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, world_tree_check

pytestmark = pytest.mark.gpu
HIT = _abi.SOL_RAY_HIT
OUTSIDE = np.array([3.7, -2.9, 3.3])  # (outside the shell, whose radius stays below 3.3)
F = np.float32


def shell_scene(width=32, height=32, spp=16, deep_and_needle=False):
    """A closed sphere-like shell of 12 x 13 x 2 - 2 x 13 = 286 triangles of radius ~3 (no two vertices on a common coordinate) and one quad
    light. deep_and_needle: also a needle triangle (80:1) inside the shell and, outside it, a chain of 120 spheres nested one Bvh per sphere."""
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.7, .6, .5))
    n_lat, n_lon = 12, 13

    def vert(i, j):
        th = np.pi * i / n_lat
        ph = 2 * np.pi * (j % n_lon) / n_lon + 0.1
        r = 3.0 + 0.2 * np.sin(3 * th + 2 * ph)
        return (r * np.sin(th) * np.cos(ph) + 0.013, r * np.cos(th) - 0.021, r * np.sin(th) * np.sin(ph) + 0.017)
    world = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, c, d, e = vert(i, j), vert(i + 1, j), vert(i + 1, j + 1), vert(i, j + 1)
            if i + 1 < n_lat:
                world.append(b.Triangle(a, c, d, grey))
            if i > 0:
                world.append(b.Triangle(a, d, e, grey))
    world.append(b.Quad((-1., 2., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(6., 6., 6.)))
    if deep_and_needle:
        world.append(b.Triangle((-2., -1.5, 0.), (2., -1.5, 0.), (2., -1.5, 0.05), grey))
        ids = [b.Sphere((float(x) * 0.25 - 15., -6. + 0.1 * (x % 3), 0.), 0.11, grey) for x in range(120)]
        inner = b.Bvh(ids[:2])
        for k in range(2, 120):
            inner = b.Bvh([inner, ids[k]]) if k % 2 else b.Bvh([ids[k], inner])
        world.append(inner)
    cam = CameraConfig(70., 0., (0.2, 0.1, 0.3), (0.5, 0.4, -1.), (0., 1., 0.))
    return b.finish(b.Bvh(world), cam, (.2, .3, .4), RenderConfig(width, height, spp, PathTracingShader(8)))


def directions():
    rng = np.random.default_rng(20)
    ds = [np.array(s, dtype=np.float64) * np.array([0.7, 1.3, 0.9]) for s in itertools.product((-1., 1.), repeat=3)]  # the 8 octants
    for axis in range(3):  # the 6 axis-parallel directions, zero components as +0.0 and as -0.0
        for sign, zero in itertools.product((-1., 1.), (0.0, -0.0)):
            d = np.full(3, zero)
            d[axis] = sign * 1.5
            ds.append(d)
    for axis in range(3):  # exactly one zero component: 3 axes x 4 sign pairs
        for s1, s2 in itertools.product((-1., 1.), repeat=2):
            d = np.array([s1 * 0.8, s2 * 1.1, 0.0])
            ds.append(np.roll(d, axis))
    for s in itertools.product((-1., 1.), repeat=3):  # 64 seeded random directions per octant
        ds += list(np.abs(rng.normal(size=(64, 3))) * rng.uniform(0.05, 30., (64, 1)) * np.array(s))
    return np.array(ds)


def as_rays(o, d):
    r = np.empty((len(o), 8), dtype=np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 0.001, d, np.inf
    return r


def oracle_hits(sc, rays):
    """orc_closest_hit in the float instantiation, ray by ray: (status, t as float, material)."""
    lib = orc.load()
    n = len(rays)
    status, t, mat = np.zeros(n, np.uint32), np.full(n, np.inf, np.float32), np.zeros(n, np.uint32)
    o, d, tt, mm = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(), C.c_uint32()
    for i, r in enumerate(rays):
        o[:], d[:] = [float(x) for x in r[0:3]], [float(x) for x in r[4:7]]
        if lib.orc_closest_hit(sc.desc_ptr, orc.ORC_F32, o, d, C.byref(tt), C.byref(mm)):
            status[i], t[i], mat[i] = HIT, np.float32(tt.value), mm.value
    return status, t, mat


def test_tree_has_inner_levels_and_partly_filled_nodes():
    """(no triangle is split and no primitive is referenced twice - asserted -, so the tree's children are its primitives and its nodes but
    the root: fewer than seven per node on average means some node is partly filled)"""
    chk = world_tree_check(shell_scene(), 1)
    assert chk["depth"] >= 3 and chk["n_wide"] >= 8, chk
    assert chk["n_extra_references"] == 0 and chk["n_split_triangles"] == 0, chk
    assert chk["n_primitives"] + chk["n_wide"] - 1 < 7 * chk["n_wide"], chk
    assert chk["box_violations"] == 0 and chk["leaf_mismatches"] == 0


def test_closest_hits_in_every_octant_equal_the_float_oracle():
    sc = shell_scene()
    d = directions()
    assert len(d) == 8 + 12 + 12 + 512
    rays = np.concatenate([as_rays(np.zeros((len(d), 3)), d), as_rays(np.tile(OUTSIDE, (len(d), 1)), d),
                           as_rays(np.tile(OUTSIDE, (len(d), 1)), -d)])
    with DeviceScene(sc) as dev:
        hits = dev.closest_hits(rays)
        occ = dev.occluded(rays)
    status, t, mat = oracle_hits(sc, rays)
    assert (occ == hits["status"]).all()  # (no invalid ray in the batch: the any-hit kernel answers what the closest-hit kernel does)
    assert (status[:len(d)] == HIT).all()  # (the shell is closed: every ray from the origin hits it)
    outside = status[len(d):] == HIT
    assert outside.any() and not outside.all()  # (from outside both answers occur)
    bad = np.nonzero((hits["status"] != status) | (hits["t"].view(np.uint32) != t.view(np.uint32)))[0]
    assert bad.size == 0, (bad[:8], rays[bad[:8]], hits[bad[:8]], t[bad[:8]])
    h = status == HIT
    assert (hits["material"][h] == mat[h]).all()
    # triangle hits: the same primitive and the same barycentrics as the fp32 contract evaluated over all triangles
    tri = h & (hits["kind"] == _abi.REF_TRIANGLE)
    assert tri.sum() > len(d) // 2 and (h & ~tri).any()  # (the quad is hit as well)
    ht, hdfs, hu, hv = host_triangle_hits(sc, rays)
    bits = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)
    bad = np.nonzero(tri & ((bits(hits["t"]) != bits(ht)) | (hits["dfs_index"] != hdfs) | (bits(hits["u"]) != bits(hu)) | (bits(hits["v"]) != bits(hv))))[0]
    assert bad.size == 0, (bad[:8], rays[bad[:8]], hits[bad[:8]], ht[bad[:8]], hdfs[bad[:8]], hu[bad[:8]], hv[bad[:8]])


def _frame_equals_oracle(sc, spp):
    with DeviceScene(sc) as dev:
        info = dev.info()
        dev.render(0, spp, pu.SEED)
        img = dev.read().astype(np.float64)
    ref, _ = orc.render(sc, 0, spp, pu.SEED, real=orc.ORC_F32)
    tol = 1e-5 * np.abs(ref) + 1e-7 * spp  # (the bound of the entry point's smoke run: the same fp32 samples summed in the same order)
    bad = int((np.abs(img - ref) > tol).any(axis=-1).sum())
    assert bad == 0 and np.isfinite(img).all() and img.mean() > 0, bad
    return info


def test_frame_of_the_shell_equals_the_float_oracle():
    _frame_equals_oracle(shell_scene(32, 32, 16), 16)


def test_frame_with_spill_and_needle_rule_equals_the_float_oracle(monkeypatch):
    monkeypatch.setenv("SOL_BVH", "ref")  # (the reference's own topology: the nested chain stays deep)
    info = _frame_equals_oracle(shell_scene(32, 32, 16, deep_and_needle=True), 16)
    assert info["stack_bound"] > info["lds_stack"], info  # the SPILL build of the kernel ran
    assert info["strict_triangles"], info                  # ... with STRICT
