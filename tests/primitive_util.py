"""Helpers of the sol_scene_set_primitives tests: the rows of a description's triangles, spheres and quads, a handful of moves, and
D' - the description a moved handle must be indistinguishable from: every moved SolTriangle / SolSphere / SolQuad made again by the CPU
constructor from its row (material, uv and dfs_index kept), every SolBvhNode::bbox the union of its children's, everything else the creation
description's. (tests/geometry_util.py is the triangles-only helper of DESIGN.md 17.)"""
import ctypes as C

import numpy as np

import geometry_util as gu
from solstrale_amd import _abi, quad_from_corner, sphere_from_center, triangle_from_vertices


def rows_of(desc):
    """dict(triangles [n, 3, 3], spheres [n, 4], quads [n, 3, 3]) in float64: the rows that move nothing."""
    s = np.zeros((desc.n_spheres, 4), dtype=np.float64)
    for i in range(desc.n_spheres):
        s[i, :3], s[i, 3] = desc.spheres[i].center[:], desc.spheres[i].radius
    q = np.zeros((desc.n_quads, 3, 3), dtype=np.float64)
    for i in range(desc.n_quads):
        q[i, 0], q[i, 1], q[i, 2] = desc.quads[i].q[:], desc.quads[i].u[:], desc.quads[i].v[:]
    return dict(triangles=gu.vertices_of(desc), spheres=s, quads=q)


def points_of(rows):
    """Every corner of every primitive (sphere: the corners of its box), [m, 3]."""
    t, s, q = rows["triangles"], rows["spheres"], rows["quads"]
    r = np.abs(s[:, 3:4])
    return np.concatenate([t.reshape(-1, 3), s[:, :3] - r, s[:, :3] + r, q[:, 0], q[:, 0] + q[:, 1], q[:, 0] + q[:, 2], q[:, 0] + q[:, 1] + q[:, 2]])


def extent_of(rows):
    """The extent of the bulk of the scene: between the 2nd and the 98th percentile of the corners per axis, so that one far light (the sphere
    chain's) does not set the size of a jitter."""
    p = points_of(rows)
    return float((np.percentile(p, 98, axis=0) - np.percentile(p, 2, axis=0)).max())


def targets_of(rows):
    """Points to aim rays at: the corners, the spheres' centres and the quads' centres, without what lies far from the bulk of the scene."""
    s, q = rows["spheres"], rows["quads"]
    p = np.concatenate([points_of(rows), s[:, :3], q[:, 0] + 0.5 * (q[:, 1] + q[:, 2])])
    return p[np.abs(p - np.median(p, axis=0)).max(axis=1) <= 3. * max(extent_of(rows), 1e-9)]


def centre_of(rows):
    p = points_of(rows)
    return 0.5 * (p.max(axis=0) + p.min(axis=0))


def scale(rows, factor, about=None):
    """Everything scaled about the centre of the scene's box: positions, radii, edges."""
    c = centre_of(rows) if about is None else np.asarray(about, dtype=np.float64)
    t, s, q = (np.array(rows[k], dtype=np.float64) for k in ("triangles", "spheres", "quads"))
    t = (t - c) * factor + c
    s[:, :3] = (s[:, :3] - c) * factor + c
    s[:, 3] *= factor
    q[:, 0] = (q[:, 0] - c) * factor + c
    q[:, 1:] *= factor
    return dict(triangles=t, spheres=s, quads=q)


def jitter(rows, seed=5, amount=0.05):
    """A seeded displacement of `amount` of the extent on every sphere and its radius scaled by U[0.5, 1.5]; the same displacement bound on every
    triangle vertex and quad corner, the quads' edges scaled by U[0.8, 1.2]."""
    rng = np.random.default_rng(seed)
    a = extent_of(rows) * amount
    t, s, q = (np.array(rows[k], dtype=np.float64) for k in ("triangles", "spheres", "quads"))
    s[:, :3] += rng.uniform(-a, a, (len(s), 3))
    s[:, 3] *= rng.uniform(0.5, 1.5, len(s))
    t += rng.uniform(-a, a, t.shape) * 0.2
    q[:, 0] += rng.uniform(-a, a, (len(q), 3))
    q[:, 1:] *= rng.uniform(0.8, 1.2, (len(q), 2, 1))
    return dict(triangles=t, spheres=s, quads=q)


def light_moved(desc, rows, shift=(0.04, -0.03, 0.05), factor=0.5):
    """The lights alone: every light that is a quad or a sphere translated by `shift` extents and shrunk to `factor` of its size about its own
    centre. Returns (rows, kinds that changed)."""
    ext = extent_of(rows)
    d = np.array(shift) * ext
    s, q = np.array(rows["spheres"]), np.array(rows["quads"])
    kinds = set()
    for k in range(desc.n_lights):
        kind, i = _abi.ref_kind(desc.lights[k]), _abi.ref_index(desc.lights[k])
        if kind == _abi.REF_QUAD:
            mid = q[i, 0] + 0.5 * (q[i, 1] + q[i, 2])
            q[i, 1:] *= factor
            q[i, 0] = mid - 0.5 * (q[i, 1] + q[i, 2]) + d
            kinds.add("quads")
        elif kind == _abi.REF_SPHERE:
            s[i, :3] += d
            s[i, 3] *= factor
            kinds.add("spheres")
    return dict(triangles=rows["triangles"], spheres=s, quads=q), kinds


class MovedScene:
    """D' of `scene` for the rows given (None: that kind as the scene has it): what DeviceScene, the oracle and background_blocks take a scene to
    be. Owns the new primitive and node arrays; everything else still points into `scene` (a Scene or another MovedScene), which it keeps alive."""

    def __init__(self, scene, triangles=None, spheres=None, quads=None):
        d0 = scene.desc
        self._scene = scene
        self.render_config = scene.render_config
        self.desc = _abi.SolSceneDesc.from_buffer_copy(d0)
        d = self.desc

        def copy(kind, src, n):
            arr = (kind * max(1, n))()
            if n:
                C.memmove(arr, src, C.sizeof(kind) * n)
            return arr

        self._tris, self._spheres, self._quads = copy(_abi.SolTriangle, d0.triangles, d0.n_triangles), copy(_abi.SolSphere, d0.spheres, d0.n_spheres), copy(_abi.SolQuad, d0.quads, d0.n_quads)
        self._nodes = copy(_abi.SolBvhNode, d0.nodes, d0.n_nodes)
        if triangles is not None:
            v = np.ascontiguousarray(triangles, dtype=np.float64)
            assert v.shape == (d0.n_triangles, 3, 3)
            for i in range(d0.n_triangles):
                t = self._tris[i]
                triangle_from_vertices(v[i], np.array([t.uv0[0], t.uv0[1], t.uv1[0], t.uv1[1], t.uv2[0], t.uv2[1]], dtype=np.float32), out=t)
        if spheres is not None:
            v = np.ascontiguousarray(spheres, dtype=np.float64)
            assert v.shape == (d0.n_spheres, 4)
            for i in range(d0.n_spheres):
                sphere_from_center(v[i, :3], v[i, 3], out=self._spheres[i])
        if quads is not None:
            v = np.ascontiguousarray(quads, dtype=np.float64)
            assert v.shape == (d0.n_quads, 3, 3)
            for i in range(d0.n_quads):
                quad_from_corner(v[i, 0], v[i, 1], v[i, 2], out=self._quads[i])
        d.triangles = C.cast(self._tris, C.POINTER(_abi.SolTriangle))
        d.spheres = C.cast(self._spheres, C.POINTER(_abi.SolSphere))
        d.quads = C.cast(self._quads, C.POINTER(_abi.SolQuad))
        d.nodes = C.cast(self._nodes, C.POINTER(_abi.SolBvhNode))
        self._union_boxes()
        self.desc_ptr = C.pointer(self.desc)

    @property
    def width(self):
        return int(self.desc.width)

    @property
    def height(self):
        return int(self.desc.height)

    def _box_of(self, ref):
        d, k, i = self.desc, _abi.ref_kind(ref), _abi.ref_index(ref)
        arr = {_abi.REF_NODE: self._nodes, _abi.REF_SPHERE: self._spheres, _abi.REF_QUAD: self._quads, _abi.REF_TRIANGLE: self._tris, _abi.REF_MEDIUM: d.mediums}[k]
        return list(arr[i].bbox.v)

    def _union_boxes(self):
        """Bottom-up: a node's box is the union of its children's (an explicit stack: the deep-chain scene is 120 levels)."""
        d = self.desc
        if _abi.ref_kind(d.root) != _abi.REF_NODE:
            return
        done = set()
        stack = [(_abi.ref_index(d.root), False)]
        while stack:
            i, ready = stack.pop()
            if i in done:
                continue
            n = self._nodes[i]
            kids = [r for r in (n.left, n.right) if _abi.ref_kind(r) != _abi.REF_NONE]
            if not ready:
                stack.append((i, True))
                stack += [(_abi.ref_index(r), False) for r in kids if _abi.ref_kind(r) == _abi.REF_NODE and _abi.ref_index(r) not in done]
                continue
            boxes = [self._box_of(r) for r in kids]
            for a in range(3):
                n.bbox.v[2 * a] = min(b[2 * a] for b in boxes)
                n.bbox.v[2 * a + 1] = max(b[2 * a + 1] for b in boxes)
            done.add(i)
