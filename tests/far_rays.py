"""Helpers of the far-origin tests (tests/test_far_origins.py, tests/test_gpu_far_origins.py; DESIGN.md 4, rule 1's distance clause): one
scene, rays aimed at its primitives from origins `ratio * S` away, and three yardsticks for a batch of rays - the double oracle (the truth),
the float oracle (which walks the caller's binary tree with the padded fp32 boxes) and a TREE-FREE evaluation of the fp32 contract's
primitive tests over all primitives, which walks no tree and is therefore what "tree independence" means. No test in this file.

Also here: host_triangle_hits, the numpy restatement of the contract's triangle test that tests/test_gpu_node_visit.py compares with."""
import ctypes as C

import numpy as np

import orc
from solstrale_amd import CameraConfig, DeviceScene, SceneBuilder, _abi, world_tree_check

F = np.float32
INF = np.float32(np.inf)
HIT, MISS, INVALID = _abi.SOL_RAY_HIT, _abi.SOL_RAY_MISS, _abi.SOL_RAY_INVALID
TMIN = np.float32(0.001)
CAMERA_Z = 20.0
NEEDLE_ASPECT = 32.0  # SOL_NEEDLE_ASPECT (include/solstrale_hip.h)
CLASSES = ("sphere_axis", "sphere_random", "quad_normal", "quad_oblique", "triangle", "quad_axial")
LADDER = (1, 4, 16, 64, 256, 1024, 4096, 16384)


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
def has_needles(desc):
    """sol_scene_has_needles (include/solstrale_hip.h) restated: some triangle's longest edge squared is at least 64 times its area."""
    for i in range(desc.n_triangles):
        t = desc.triangles[i]
        a, b = np.array(t.v0v1[:]), np.array(t.v0v2[:])
        l2 = max((a * a).sum(), (b * b).sum(), ((b - a) ** 2).sum())
        if not l2 < 2.0 * NEEDLE_ASPECT * t.area:
            return True
    return False


def scene_S(desc, camera_origin=None):
    """box_pad_for's S (csrc/sol_tree.h): the largest |fp32 coordinate| of the root's box and of the camera origin."""
    assert _abi.ref_kind(desc.root) == _abi.REF_NODE
    v = list(desc.nodes[_abi.ref_index(desc.root)].bbox.v) + list(desc.camera.origin[:] if camera_origin is None else camera_origin)
    return float(np.abs(np.array(v, dtype=np.float64).astype(F)).max())


def far_scene(rc, camera=None):
    """40 spheres of radius 0.7 in [-8, 8]^3, 12 axis-aligned 2 x 2 quads (four per axis), one light quad, 60 small triangles (edge about
    0.5, random orientation, none a needle); no constant medium; the creation camera at (0, 0, 20) looking at the origin, so S = 20."""
    rng = np.random.default_rng(2024)
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(.6, .6, .6))
    red = b.Lambertian(b.SolidColor(.7, .2, .2))
    world = [b.Sphere(tuple(rng.uniform(-7.3, 7.3, 3)), 0.7, grey) for _ in range(40)]
    for axis in range(3):
        for _ in range(4):
            q = rng.uniform(-8., 6., 3)
            u, v = np.zeros(3), np.zeros(3)
            u[(axis + 1) % 3], v[(axis + 2) % 3] = 2., 2.
            world.append(b.Quad(tuple(q), tuple(u), tuple(v), red))
    world.append(b.Quad((-1., 9., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(8., 8., 8.)))
    for _ in range(60):
        p = rng.uniform(-7.5, 7.5, 3)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        c = np.cross(a, rng.normal(size=3))
        c /= np.linalg.norm(c)
        e1, e2 = 0.5 * a, rng.uniform(0.4, 0.6) * (0.5 * a + 0.866 * c)  # (about equilateral)
        world.append(b.Triangle(tuple(p), tuple(p + e1), tuple(p + e2), grey))
    cam = camera or CameraConfig(40., 0., (0., 0., CAMERA_Z), (0., 0., 0.), (0., 1., 0.))
    sc = b.finish(b.Bvh(world), cam, (.2, .3, .4), rc)
    d = sc.desc
    assert (d.n_spheres, d.n_quads, d.n_triangles, d.n_mediums) == (40, 13, 60, 0) and not has_needles(d)
    if camera is None:
        assert scene_S(d) == CAMERA_Z
        chk = world_tree_check(sc, 1)
        assert chk["depth"] >= 2 and chk["n_split_triangles"] == 0 and chk["n_extra_references"] == 0, chk
        assert chk["box_violations"] == 0 and chk["leaf_mismatches"] == 0, chk
    return sc


# ---- the rays ----------------------------------------------------------------------------------------------------------------------------
def as_rays(o, d, tmin=TMIN, tmax=INF):
    r = np.empty((len(o), 8), dtype=F)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perpendicular(rng, n):
    """A seeded unit vector perpendicular to each row of n."""
    return _unit(np.cross(n, _unit(n + rng.normal(size=n.shape) + 1e-3)))


def aimed_rays(scene, ratio, seed, per_class, S=None):
    """Rays aimed from outside at interior points of a primitive: the origin is target + unit direction x (ratio x S), cast to float32, and
    d = target - origin computed AFTER that cast, so |d| is the distance and the aimed hit sits at t = 1. tmin = 0.001, tmax = inf.
    Returns (rays [6 x per_class, 8] float32, class index per ray into CLASSES)."""
    d = scene.desc
    rng = np.random.default_rng([seed, int(ratio)])
    S = scene_S(d) if S is None else S
    n = per_class
    sph = np.array([[*d.spheres[i].center[:], d.spheres[i].radius] for i in range(d.n_spheres)])
    quad = np.array([[d.quads[i].q[:], d.quads[i].u[:], d.quads[i].v[:], d.quads[i].normal[:]] for i in range(d.n_quads)])
    tri = np.array([[d.triangles[i].v0[:], d.triangles[i].v0v1[:], d.triangles[i].v0v2[:], d.triangles[i].normal[:]] for i in range(d.n_triangles)])
    targets, away = [], []  # away: the unit vector from the target to the origin

    def on_sphere(w):
        """The point of a seeded sphere that faces `w`, moved up to 60 degrees aside; a draw that would land further aside (about one in ten)
        becomes the pole itself, where the hit point lies ON a face of the sphere's own box: the edge of rule 2."""
        s = sph[rng.integers(0, len(sph), n)]
        p = _unit(w + 0.8 * rng.uniform(-1., 1., (n, 3)))
        p = np.where(((p * w).sum(axis=1) < 0.5)[:, None], w, p)
        return s[:, :3] + s[:, 3:4] * p

    # sphere seen along each axis, both signs
    w = np.zeros((n, 3))
    w[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1., 1.], n)
    targets.append(on_sphere(w)); away.append(w)
    # sphere seen from a random direction
    w = _unit(rng.normal(size=(n, 3)))
    targets.append(on_sphere(w)); away.append(w)
    # quad seen nearly along its normal / obliquely (normal share 0.3)
    for share in (0.98, 0.3):
        q = quad[rng.integers(0, len(quad), n)]
        nrm = q[:, 3] * rng.choice([-1., 1.], (n, 1))
        targets.append(q[:, 0] + q[:, 1] * rng.uniform(0.2, 0.8, (n, 1)) + q[:, 2] * rng.uniform(0.2, 0.8, (n, 1)))
        away.append(share * nrm + np.sqrt(1. - share * share) * _perpendicular(rng, nrm))
    # triangle aimed at barycentrics in [0.2, 0.6], u + v <= 0.8
    t = tri[rng.integers(0, len(tri), n)]
    bu = rng.uniform(0.2, 0.6, (n, 1))
    bv = 0.2 + rng.uniform(0., 1., (n, 1)) * np.minimum(0.4, 0.6 - bu)
    nrm = t[:, 3] * rng.choice([-1., 1.], (n, 1))
    share = rng.uniform(0.3, 1.0, (n, 1))
    targets.append(t[:, 0] + t[:, 1] * bu + t[:, 2] * bv)
    away.append(share * nrm + np.sqrt(1. - share * share) * _perpendicular(rng, nrm))
    # axis-parallel rays aimed at quad interiors (made exactly parallel, with signed zeros, below)
    q = quad[rng.integers(0, len(quad), n)]
    axial_target = (q[:, 0] + q[:, 1] * rng.uniform(0.2, 0.8, (n, 1)) + q[:, 2] * rng.uniform(0.2, 0.8, (n, 1))).astype(F).astype(np.float64)
    axis = np.abs(q[:, 3]).argmax(axis=1)
    assert (np.abs(q[np.arange(n), 3, axis]) == 1.0).all()  # (every quad of the scene is axis-aligned)
    w = np.zeros((n, 3))
    w[np.arange(n), axis] = rng.choice([-1., 1.], n)
    targets.append(axial_target); away.append(w)

    targets, away = np.concatenate(targets), np.concatenate(away)
    origin = (targets + _unit(away) * (ratio * S)).astype(F)
    direction = (targets - origin.astype(np.float64)).astype(F)
    ax = slice(5 * n, 6 * n)
    zero = direction[ax] == 0
    assert (zero.sum(axis=1) == 2).all()  # (the float32 target and origin share two coordinates exactly)
    direction[ax] = np.where(zero, np.where(rng.random((n, 3)) < 0.5, F(0.0), F(-0.0)), direction[ax])
    z = direction[ax][zero]
    assert np.signbit(z).any() and not np.signbit(z).all()
    rays = as_rays(origin, direction)
    assert np.isfinite(rays[:, :7]).all() and (np.abs(rays[:, 4:7]).max(axis=1) > 0).all()
    return rays, np.repeat(np.arange(len(CLASSES)), n)


# ---- yardstick 1 and 2: the oracle's closest hit, ray by ray ----------------------------------------------------------------------------
def oracle_hits(sc, rays, real=orc.ORC_F32, own_interval=True):
    """orc_closest_hit ray by ray: (status, t, material). ORC_F32: t cast back to float32; ORC_F64: t as float64. The oracle's entry searches
    [0.001, inf) whatever the row says; own_interval: assert that the rows say the same."""
    lib = orc.load()
    n = len(rays)
    status, mat = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    t = np.full(n, np.inf, F if real == orc.ORC_F32 else np.float64)
    o, d, tt, mm = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(), C.c_uint32()
    for i, r in enumerate(rays):
        assert not own_interval or (r[3] == TMIN and r[7] == INF)
        o[:], d[:] = [float(x) for x in r[0:3]], [float(x) for x in r[4:7]]
        if lib.orc_closest_hit(sc.desc_ptr, real, o, d, C.byref(tt), C.byref(mm)):
            status[i], t[i], mat[i] = HIT, tt.value, mm.value
    return status, t, mat


def solid(status64, t64):
    """A ray is SOLID when the double oracle hits and |t - 1| < 0.05: the aimed primitive is the closest."""
    return (status64 == HIT) & (np.abs(t64 - 1.0) < 0.05)


def lost(is_solid, status, t, t64):
    """Solid rays for which an fp32 answer is a miss or a t more than 2 % off the truth."""
    with np.errstate(invalid="ignore"):
        return is_solid & ((status != HIT) | ~(np.abs(t.astype(np.float64) - t64) <= 0.02 * t64))


# ---- yardstick 3: the contract's primitive tests over ALL primitives, no tree -----------------------------------------------------------
def rotated_triangle_records(desc):
    """The device's triangle records (include/solstrale_hip.h, sol_triangle_rotation / sol_triangle_rotated): rotated in double to start at the
    vertex opposite the longest edge, then rounded to float. Returns (v0, e1, e2 [n, 3] float32, dfs_index, material)."""
    n = desc.n_triangles
    v0, e1, e2, dfs, mat = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 3)), np.empty(n, np.uint32), np.empty(n, np.uint32)
    for i in range(n):
        s = desc.triangles[i]
        p, a, b = np.array(s.v0[:]), np.array(s.v0v1[:]), np.array(s.v0v2[:])
        c = b - a
        l01, l02, l12 = (a * a).sum(), (b * b).sum(), (c * c).sum()
        k, best = 0, l12
        if l02 > best:
            best, k = l02, 1
        if l01 > best:
            k = 2
        v0[i], e1[i], e2[i] = [(p, a, b), (p + a, b - a, -a), (p + b, -b, a - b)][k]
        dfs[i], mat[i] = s.dfs_index, s.material
    return v0.astype(F), e1.astype(F), e2.astype(F), dfs, mat


def host_triangle_hits(sc, rays):
    """The closest triangle hit of every ray by the fp32 contract, evaluated here over all triangles: (t, dfs_index, u, v); t = inf: none.
    Records: rotated to start at the vertex opposite the longest edge (solstrale_hip.h, sol_triangle_rotation / sol_triangle_rotated), in
    double, then rounded to float. Test: Moller-Trumbore in the operation order of tri_test, sums left to right, one IEEE division; among
    equal t the LAST triangle in depth-first order wins."""
    v0, e1, e2, dfs, _ = rotated_triangle_records(sc.desc)
    ox, oy, oz = (rays[:, k].astype(F)[:, None] for k in (0, 1, 2))
    dx, dy, dz = (rays[:, k].astype(F)[:, None] for k in (4, 5, 6))
    col = lambda m: (m[None, :, 0], m[None, :, 1], m[None, :, 2])
    (ax, ay, az), (bx, by, bz), (vx, vy, vz) = col(e1), col(e2), col(v0)
    dot = lambda x0, y0, z0, x1, y1, z1: (x0 * x1 + y0 * y1) + z0 * z1
    with np.errstate(all="ignore"):
        px, py, pz = dy * bz - dz * by, dz * bx - dx * bz, dx * by - dy * bx  # cross3(d, e2)
        det = dot(ax, ay, az, px, py, pz)
        inv = F(1.0) / det
        tx, ty, tz = ox - vx, oy - vy, oz - vz
        qx, qy, qz = ty * az - tz * ay, tz * ax - tx * az, tx * ay - ty * ax  # cross3(t_vec, e1)
        u = dot(tx, ty, tz, px, py, pz) * inv
        v = dot(dx, dy, dz, qx, qy, qz) * inv
        t = dot(bx, by, bz, qx, qy, qz) * inv
        assert u.dtype == F and t.dtype == F
        ok = ~(np.abs(det) < F(1e-8)) & (u >= 0) & (u <= 1) & ~((v < 0) | (u + v > F(1.0))) & (t >= F(0.001))
    t = np.where(ok, t, F(np.inf))
    tbest = t.min(axis=1)
    tie = (t == tbest[:, None]) & ok
    win = np.where(tie, dfs[None, :].astype(np.int64), -1).argmax(axis=1)
    r = np.arange(len(rays))
    return tbest, dfs[win], u[r, win], v[r, win]


def sphere_slack_of(S):
    """DevScene::sphere_slack of a scene without needles: half the box pad, S * 2^-20 / 2, in float as sol_create.cpp computes it."""
    return F(F(S) * F(1.0 / 1048576.0)) * F(0.5)


def _rows(prims, rays):
    """Every (primitive, ray) pair as one row: [n_rays * n_prims, prim words + 8 ray words (o, d, tmin, tmax)], ray-major."""
    n, m = len(rays), len(prims)
    ray = np.concatenate([rays[:, 0:3], rays[:, 4:7], rays[:, 3:4], rays[:, 7:8]], axis=1)
    return np.concatenate([np.tile(prims, (n, 1)), np.repeat(ray, m, axis=0)], axis=1).astype(F)


def tree_free_hits(sc, rays, sphere_slack):
    """The fp32 contract without a tree: orc.eval_f32 fn 4 / 5 / 6 (Sphere::hit with the own-box rule, Quad::hit, Triangle::hit - bit for bit
    the device's tests, tests/test_gpu_functions.py) on every (primitive, ray) pair over the ray's own [tmin, tmax], inclusive at both ends as
    those tests are; spheres and quads through the device's plain casts (csrc/sol_primitive.h), triangles through the rotated records. The
    winner by (t, dfs) as `better` (csrc/sol_trace.h) chooses: the smallest t, among equal t the largest dfs_index. Returns a structured array
    of DeviceScene.RAY_HIT_DTYPE's fields: a miss is (inf, 0, 0, MISS, 0, 0, 0, 0)."""
    d = sc.desc
    rays = np.ascontiguousarray(rays, dtype=F)
    n = len(rays)
    ts, us, vs, kinds, dfss, mats = [], [], [], [], [], []

    def take(kind, out, m, dfs, mat, with_uv):
        out = out.reshape(n, m, -1)
        ts.append(np.where(out[:, :, 0] == 1.0, out[:, :, 1], INF))
        us.append(out[:, :, 2] if with_uv else np.zeros((n, m), F))
        vs.append(out[:, :, 3] if with_uv else np.zeros((n, m), F))
        kinds.append(np.full(m, kind, np.uint32)); dfss.append(np.asarray(dfs, np.uint32)); mats.append(np.asarray(mat, np.uint32))

    if d.n_spheres:
        s = [d.spheres[i] for i in range(d.n_spheres)]
        prims = np.array([[*x.center[:], abs(F(x.radius))] for x in s], dtype=np.float64).astype(F)
        rows = np.concatenate([_rows(prims, rays), np.full((n * len(s), 1), sphere_slack, F)], axis=1)
        take(_abi.REF_SPHERE, orc.eval_f32(4, rows, 2), len(s), [x.dfs_index for x in s], [x.material for x in s], False)
    if d.n_quads:
        q = [d.quads[i] for i in range(d.n_quads)]
        prims = np.array([[*x.normal[:], x.d, *x.q[:], *x.w[:], *x.u[:], *x.v[:]] for x in q], dtype=np.float64).astype(F)
        take(_abi.REF_QUAD, orc.eval_f32(5, _rows(prims, rays), 4), len(q), [x.dfs_index for x in q], [x.material for x in q], True)
    if d.n_triangles:
        v0, e1, e2, dfs, mat = rotated_triangle_records(d)
        take(_abi.REF_TRIANGLE, orc.eval_f32(6, _rows(np.concatenate([v0, e1, e2], axis=1), rays), 4), len(dfs), dfs, mat, True)
    t, u, v = np.concatenate(ts, axis=1), np.concatenate(us, axis=1), np.concatenate(vs, axis=1)
    kind, dfs, mat = np.concatenate(kinds), np.concatenate(dfss), np.concatenate(mats)
    tbest = t.min(axis=1)
    tie = (t == tbest[:, None]) & np.isfinite(t)
    win = np.where(tie, dfs[None, :].astype(np.int64), -1).argmax(axis=1)
    r = np.arange(n)
    out = np.zeros(n, dtype=DeviceScene.RAY_HIT_DTYPE)
    hit = np.isfinite(tbest)
    out["t"] = tbest
    out["status"] = np.where(hit, HIT, MISS)
    for name, val in (("u", u[r, win]), ("v", v[r, win]), ("kind", kind[win]), ("dfs_index", dfs[win]), ("material", mat[win])):
        out[name] = np.where(hit, val, 0)
    valid = np.isfinite(rays[:, :7]).all(axis=1) & (np.abs(rays[:, 4:7]).max(axis=1) > 0) & (rays[:, 3] >= 0) & (rays[:, 3] <= rays[:, 7])
    assert valid.all()  # (this yardstick answers valid rays only)
    return out


def primitive_exists(desc, kind, dfs, material):
    """True when the description holds a primitive of `kind` with this dfs_index and material."""
    arr, n = {_abi.REF_SPHERE: (desc.spheres, desc.n_spheres), _abi.REF_QUAD: (desc.quads, desc.n_quads),
              _abi.REF_TRIANGLE: (desc.triangles, desc.n_triangles)}.get(int(kind), (None, 0))
    return any(arr[i].dfs_index == int(dfs) and arr[i].material == int(material) for i in range(n))


# ---- the ladder: one seeded batch per rung, with its CPU yardsticks, made once per process ------------------------------------------------
# The envelope (profiles/far_origins.txt): E_MEASURED is the last rung of LADDER at which the float oracle finds every solid f64 hit of the
# batches below; E_DOC, one rung lower, is what include/solstrale_hip.h promises callers.
E_MEASURED = 16
E_DOC = E_MEASURED // 4
SEED = 1
PER_CLASS = 200
_cache = {}


def ladder_scene():
    if "scene" not in _cache:
        from solstrale_amd import PathTracingShader, RenderConfig
        _cache["scene"] = far_scene(RenderConfig(32, 32, 16, PathTracingShader(8)))
    return _cache["scene"]


def ladder_batch(ratio):
    """dict(rays, cls, status64, t64, solid, status32, t32, mat32, free): the rung's rays and what the three yardsticks say. Read-only."""
    if ratio not in _cache:
        sc = ladder_scene()
        rays, cls = aimed_rays(sc, ratio, SEED, PER_CLASS)
        s64, t64, _ = oracle_hits(sc, rays, orc.ORC_F64)
        s32, t32, m32 = oracle_hits(sc, rays, orc.ORC_F32)
        free = tree_free_hits(sc, rays, sphere_slack_of(scene_S(sc.desc)))
        b = dict(rays=rays, cls=cls, status64=s64, t64=t64, solid=solid(s64, t64), status32=s32, t32=t32, mat32=m32, free=free)
        for v in b.values():
            v.setflags(write=False)
        _cache[ratio] = b
    return _cache[ratio]


def per_class(mask, cls):
    return [int(mask[cls == k].sum()) for k in range(len(CLASSES))]
