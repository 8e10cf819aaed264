"""Helpers of the sol_scene_set_triangles tests: the vertices of a description's triangles, a handful of moves, and D' - the
description a moved handle must be indistinguishable from: every SolTriangle made again by sol_triangle_from_vertices from its new vertices
(uv, material and dfs_index kept), every SolBvhNode::bbox the union of its children's, everything else the creation description's."""
import ctypes as C

import numpy as np

from solstrale_amd import _abi, triangle_from_vertices


def vertices_of(desc):
    """float64 [n, 3, 3]: (v0, v0 + v0v1, v0 + v0v2) of every triangle of the description."""
    out = np.zeros((desc.n_triangles, 3, 3), dtype=np.float64)
    for i in range(desc.n_triangles):
        t = desc.triangles[i]
        v0 = np.array(t.v0[:])
        out[i, 0], out[i, 1], out[i, 2] = v0, v0 + np.array(t.v0v1[:]), v0 + np.array(t.v0v2[:])
    return out


def extent_of(vertices):
    p = vertices.reshape(-1, 3)
    return float((p.max(axis=0) - p.min(axis=0)).max())


def move(vertices, kind, amount=None):
    """identity; sine: a displacement of 5 % of the extent; translate: 0.3 extents; scale: 1.5 x about the centre (or `amount`)."""
    v = np.array(vertices, dtype=np.float64)
    p = v.reshape(-1, 3)
    ext = extent_of(v)
    centre = 0.5 * (p.max(axis=0) + p.min(axis=0))
    if kind == "identity":
        return v
    if kind == "sine":
        a = ext * (0.05 if amount is None else amount)
        w = 2.0 * np.pi * 3.0 / max(ext, 1e-30)
        d = np.stack([np.sin(w * v[..., 1] + 0.3), np.sin(w * v[..., 2] + 1.1), np.sin(w * v[..., 0] + 2.0)], axis=-1)
        return v + a * d
    if kind == "translate":
        return v + ext * (0.3 if amount is None else amount) * np.array([0.6, 0.48, -0.64])
    if kind == "scale":
        return (v - centre) * (1.5 if amount is None else amount) + centre
    raise ValueError(kind)


class MovedScene:
    """D' of `scene` for `vertices` (float64 [n, 3, 3]): what DeviceScene, the oracle and background_blocks take a scene to be. Owns the new
    triangle and node arrays; everything else still points into `scene`, which it keeps alive."""

    def __init__(self, scene, vertices):
        d0 = scene.desc
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        assert v.shape == (d0.n_triangles, 3, 3)
        self._scene = scene
        self.render_config = scene.render_config
        self.desc = _abi.SolSceneDesc.from_buffer_copy(d0)
        d = self.desc
        self._tris = (_abi.SolTriangle * max(1, d0.n_triangles))()
        if d0.n_triangles:
            C.memmove(self._tris, d0.triangles, C.sizeof(_abi.SolTriangle) * d0.n_triangles)
        for i in range(d0.n_triangles):
            t = self._tris[i]
            uv = np.array([t.uv0[0], t.uv0[1], t.uv1[0], t.uv1[1], t.uv2[0], t.uv2[1]], dtype=np.float32)
            triangle_from_vertices(v[i], uv, out=t)
        self._nodes = (_abi.SolBvhNode * max(1, d0.n_nodes))()
        if d0.n_nodes:
            C.memmove(self._nodes, d0.nodes, C.sizeof(_abi.SolBvhNode) * d0.n_nodes)
        d.triangles = C.cast(self._tris, C.POINTER(_abi.SolTriangle))
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
        arr = {_abi.REF_NODE: self._nodes, _abi.REF_SPHERE: d.spheres, _abi.REF_QUAD: d.quads, _abi.REF_TRIANGLE: self._tris, _abi.REF_MEDIUM: d.mediums}[k]
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
