"""The `dfs_index` contract (include/solstrale_hip.h) restated for the tests: the number every record the world tree reaches
must carry, and descriptors the host never emits - the primitive tables in another order, a sub-tree referenced twice - built from the
host's own scenes.

The numbering: a pre-order walk from `root`, left child before right; every sphere, quad, triangle or medium it reaches takes the next
number, a medium before its boundary sub-tree is walked; a record reached more than once keeps the number of its LAST visit (the float
oracle, and the reference, let the later of two equal hits win, so that visit decides its ties). The walk here expands shared sub-trees
visit by visit: fine for the tests' scenes, not for a caller's adversarial one (the library's check is linear)."""
import ctypes as C

import numpy as np

from solstrale_amd import _abi

# reference kind -> (array field, count field, record type)
TABLES = {_abi.REF_SPHERE: ("spheres", "n_spheres", _abi.SolSphere), _abi.REF_QUAD: ("quads", "n_quads", _abi.SolQuad),
          _abi.REF_TRIANGLE: ("triangles", "n_triangles", _abi.SolTriangle), _abi.REF_MEDIUM: ("mediums", "n_mediums", _abi.SolMedium)}
KIND_NAMES = {_abi.REF_SPHERE: "sphere", _abi.REF_QUAD: "quad", _abi.REF_TRIANGLE: "triangle", _abi.REF_MEDIUM: "medium"}


def ref(kind, index):
    return (kind << 28) | index


def tree_numbering(desc):
    """{(kind, index): the number the record must carry} over every record the walk from desc.root reaches."""
    num = {}
    n = 0
    stack = [desc.root]
    while stack:
        r = stack.pop()
        k, i = _abi.ref_kind(r), _abi.ref_index(r)
        if k == _abi.REF_NONE:
            continue
        if k == _abi.REF_NODE:
            node = desc.nodes[i]
            stack.append(node.right)
            stack.append(node.left)
            continue
        num[(k, i)] = n
        n += 1
        if k == _abi.REF_MEDIUM:
            stack.append(desc.mediums[i].boundary)
    return num


def visit_order(desc):
    """Every visit of the walk in order, as (kind, index) (a shared sub-tree's records more than once)."""
    out = []
    stack = [desc.root]
    while stack:
        r = stack.pop()
        k, i = _abi.ref_kind(r), _abi.ref_index(r)
        if k == _abi.REF_NONE:
            continue
        if k == _abi.REF_NODE:
            stack.append(desc.nodes[i].right)
            stack.append(desc.nodes[i].left)
            continue
        out.append((k, i))
        if k == _abi.REF_MEDIUM:
            stack.append(desc.mediums[i].boundary)
    return out


def record(desc, kind, index):
    return getattr(desc, TABLES[kind][0])[index]


def get_dfs(desc, kind, index):
    return record(desc, kind, index).dfs_index


def set_dfs(desc, kind, index, value):
    record(desc, kind, index).dfs_index = value


def _raw(ptr, ctype, n):
    """The caller's table as an (n, sizeof record) byte matrix (a view, not a copy)."""
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * C.sizeof(ctype),)).reshape(n, C.sizeof(ctype))


def _remap(refs, new_of_old):
    refs = np.asarray(refs, dtype=np.uint32)
    kind, idx = refs >> 28, refs & 0x0FFFFFFF
    out = refs.copy()
    for k, perm in new_of_old.items():
        sel = kind == k
        out[sel] = (k << 28) | perm[idx[sel]]
    return out


class CopiedScene:
    """A copy of `scene`'s descriptor over tables of its own (nodes, primitives, mediums, lights); `perm` maps a reference kind to an
    order of that table (old index of each new record), and every node, light, medium-boundary and root reference is remapped to
    follow it. The dfs_index fields travel with their records: the same world, listed in another order. Materials, textures, texels and
    the environment map stay the parent's. Takes what DeviceScene and orc.render take (desc_ptr, width, height)."""

    def __init__(self, scene, perm=None):
        perm = perm or {}
        d = scene.desc
        self._parent = scene
        self._keep = []
        self.desc = _abi.SolSceneDesc()
        C.memmove(C.byref(self.desc), C.byref(d), C.sizeof(_abi.SolSceneDesc))
        new_of_old = {}
        for kind, (field, count, ctype) in TABLES.items():
            n = getattr(d, count)
            if n == 0:
                continue
            order = np.asarray(perm.get(kind, np.arange(n)), dtype=np.int64)
            assert sorted(order.tolist()) == list(range(n))
            inv = np.empty(n, dtype=np.uint32)
            inv[order] = np.arange(n, dtype=np.uint32)
            new_of_old[kind] = inv
            table = _raw(getattr(d, field), ctype, n)[order].copy()
            self._keep.append(table)
            setattr(self.desc, field, table.ctypes.data_as(C.POINTER(ctype)))
        if d.n_nodes:
            nodes = _raw(d.nodes, _abi.SolBvhNode, d.n_nodes).copy()
            at = _abi.SolBvhNode.left.offset
            assert _abi.SolBvhNode.right.offset == at + 4
            lr = np.ascontiguousarray(nodes[:, at:at + 8]).view(np.uint32)
            nodes[:, at:at + 8] = _remap(lr.ravel(), new_of_old).reshape(-1, 2).view(np.uint8)
            self._keep.append(nodes)
            self.desc.nodes = nodes.ctypes.data_as(C.POINTER(_abi.SolBvhNode))
        self.lights = (C.c_uint32 * max(1, d.n_lights))(*_remap([d.lights[i] for i in range(d.n_lights)], new_of_old).tolist())
        self.desc.lights = C.cast(self.lights, C.POINTER(C.c_uint32))
        for i in range(self.desc.n_mediums):
            self.desc.mediums[i].boundary = int(_remap([self.desc.mediums[i].boundary], new_of_old)[0])
        self.desc.root = int(_remap([d.root], new_of_old)[0])
        self.desc_ptr = C.pointer(self.desc)
        self.width, self.height = int(d.width), int(d.height)


def shuffled(scene, seed):
    """CopiedScene with the sphere, quad and triangle tables in a random order (seeded)."""
    rng = np.random.default_rng(seed)
    d = scene.desc
    perm = {}
    for k in (_abi.REF_SPHERE, _abi.REF_QUAD, _abi.REF_TRIANGLE):
        n = getattr(d, TABLES[k][1])
        if n > 1:
            p = rng.permutation(n)
            perm[k] = p if (p != np.arange(n)).any() else p[::-1]  # (never the identity)
    return CopiedScene(scene, perm)


def _union(*boxes):
    v = [0.] * 6
    for a in range(3):
        v[2 * a] = min(b.v[2 * a] for b in boxes)
        v[2 * a + 1] = max(b.v[2 * a + 1] for b in boxes)
    return _abi.SolAabb((C.c_double * 6)(*v))


def shared_subtree_scene(render_config, rule="last"):
    """Two coincident quads, red (A) and white (B), and a light sphere L under a tree the host never emits - a sub-tree S holding A is
    referenced from two nodes, with B walked between the two visits:

        N0 = (N1, N2)   N1 = (S, B)   N2 = (L, S)   S = (A, none)       visits: A, B, L, A

    rule "last": A carries 3 (its second visit), B 1, L 2 - the contract; the oracle's later-hit-wins makes A win every tie, and so
    must the device. rule "first": A carries 0, B 1, L 2 - the numbering of A's first visit, which the creation check refuses."""
    from solstrale_amd import CameraConfig, SceneBuilder
    b = SceneBuilder()
    red, white = b.Lambertian(b.SolidColor(1., 0., 0.)), b.Lambertian(b.SolidColor(.9, .9, .9))
    world = [b.Quad((-1., 0., -3.), (2., 0., 0.), (0., 2., 0.), red), b.Quad((-1., 0., -3.), (2., 0., 0.), (0., 2., 0.), white),
             b.Sphere((0., 50., 20.), 10., b.DiffuseLight(5, 5, 5))]
    cam = CameraConfig(50., 0., (0., 1., 1.), (0., 1., -3.), (0, 1, 0))
    sc = CopiedScene(b.finish(b.Bvh(world), cam, (.1, .1, .1), render_config))
    d = sc.desc
    assert d.n_quads == 2 and d.n_spheres == 1
    a = next(i for i in range(2) if d.materials[d.quads[i].material].albedo_tex >= 0 and d.textures[d.materials[d.quads[i].material].albedo_tex].rgb[1] == 0.)
    qa, qb, sl = ref(_abi.REF_QUAD, a), ref(_abi.REF_QUAD, 1 - a), ref(_abi.REF_SPHERE, 0)
    ba, bb, bl = d.quads[a].bbox, d.quads[1 - a].bbox, d.spheres[0].bbox
    node = lambda box, left, right: _abi.SolBvhNode(box, left, right)
    nodes = (_abi.SolBvhNode * 4)(node(_union(ba, bb, bl), ref(_abi.REF_NODE, 1), ref(_abi.REF_NODE, 2)),
                                  node(_union(ba, bb), ref(_abi.REF_NODE, 3), qb),
                                  node(_union(bl, ba), sl, ref(_abi.REF_NODE, 3)),
                                  node(_union(ba), qa, ref(_abi.REF_NONE, 0)))
    sc._keep.append(nodes)
    d.nodes = C.cast(nodes, C.POINTER(_abi.SolBvhNode))
    d.n_nodes = 4
    d.root = ref(_abi.REF_NODE, 0)
    d.quads[a].dfs_index = 3 if rule == "last" else 0
    d.quads[1 - a].dfs_index = 1
    d.spheres[0].dfs_index = 2
    sc.red_quad = a
    return sc
