"""Thin Python handle over the device C ABI (libsolstrale_hip.so). No compute happens in Python and there is no
fallback: every call goes to the HIP library and raises if it fails (e.g. SOL_EDEVICE without a GPU)."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from . import _abi


class DeviceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code
        self.msg = msg


def device_count():
    return int(_abi.load_hip().sol_device_count())


def comm_unique_id():
    """sol_comm_unique_id: 128 bytes rank 0 ships to the other ranks before sol_comm_init."""
    lib = _abi.load_hip()
    buf = (C.c_uint8 * _abi.UNIQUE_ID_BYTES)()
    rc = lib.sol_comm_unique_id(buf)
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    return bytes(buf)


def record_sizes():
    out = (C.c_uint32 * 6)()
    _abi.load_hip().sol_record_sizes(out)
    return dict(zip(("node", "sphere", "quad", "triangle", "triangle_shade", "material"), [int(x) for x in out]))


def eval_functions(fn, rows, out_cols, device=0):
    """sol_eval: device functions on rows of fp32 inputs (function-level parity tests)."""
    lib = _abi.load_hip()
    a = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.zeros((a.shape[0], out_cols), dtype=np.float32)
    rc = lib.sol_eval(device, fn, a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data, out_cols)
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    return out


def world_tree_check(scene, use_sah):
    """Host-only structural check of the 8-wide tree sol_scene_create would build for `scene` (no device needed)."""
    lib = _abi.load_hip()
    out = _abi.SolTreeCheck()
    rc = lib.sol_world_tree_check_ex(scene.desc_ptr, int(use_sah), C.byref(out), C.sizeof(out))  # (the size-prefixed form: every field)
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    return out.as_dict()


def background_blocks(scene, use_sah=0):
    """Host-only: which 8x8 pixel blocks of `scene` provably see nothing but the background (sol_background_blocks): a bool array
    [blocks_y, blocks_x]."""
    import numpy as np
    lib = _abi.load_hip()
    bx, by = (scene.width + 7) // 8, (scene.height + 7) // 8
    flags = (C.c_uint8 * (bx * by))()
    n = C.c_uint32()
    rc = lib.sol_background_blocks(scene.desc_ptr, int(use_sah), flags, bx * by, C.byref(n))
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    out = np.frombuffer(flags, dtype=np.uint8).reshape(by, bx).astype(bool)
    assert int(out.sum()) == n.value
    return out


def triangle_from_vertices(v, uv=None, out=None):
    """sol_triangle_from_vertices (CPU, no device): the SolTriangle of the vertices v (3 x 3 float64: v0, v1, v2) and the texture coordinates uv
    (3 x 2 float32, default zeros) - geometry, uvs and bbox; `out`: a SolTriangle to fill instead of a new one (its material and dfs_index stay)."""
    lib = _abi.load_hip()
    a = np.ascontiguousarray(v, dtype=np.float64).reshape(9)
    t = np.zeros(6, dtype=np.float32) if uv is None else np.ascontiguousarray(uv, dtype=np.float32).reshape(6)
    out = _abi.SolTriangle() if out is None else out
    rc = lib.sol_triangle_from_vertices(a.ctypes.data, t.ctypes.data, C.byref(out))
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    return out


def sphere_from_center(center, radius, out=None):
    """sol_sphere_from_center (CPU, no device): the SolSphere of a centre (3 float64) and a radius - center, radius and bbox; `out`: a SolSphere to
    fill instead of a new one (its material and dfs_index stay)."""
    lib = _abi.load_hip()
    c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    out = _abi.SolSphere() if out is None else out
    rc = lib.sol_sphere_from_center(c.ctypes.data, float(radius), C.byref(out))
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    return out


def quad_from_corner(q, u, v, out=None):
    """sol_quad_from_corner (CPU, no device): the SolQuad of a corner q and the edges u, v (3 float64 each) - q, u, v, normal, d, w, area and the
    padded bbox; `out`: a SolQuad to fill instead of a new one (its material and dfs_index stay)."""
    lib = _abi.load_hip()
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(3) for x in (q, u, v)]
    out = _abi.SolQuad() if out is None else out
    rc = lib.sol_quad_from_corner(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, C.byref(out))
    if rc != 0:
        raise DeviceError(rc, lib.sol_last_error().decode(errors="replace"))
    return out


# The constants of csrc/sol_sh.h: the fp32 roundings of sqrt(1/(4 pi)), sqrt(3/(4 pi)), sqrt(15/(4 pi)), sqrt(5/(16 pi)), sqrt(15/(16 pi)).
_SH9_K = tuple(np.float32(k) for k in (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396))


def sh9(directions):
    """The nine real SH terms up to l = 2 of sol_irradiance_sh on directions [..., 3], in numpy float32 and the bracketing of csrc/sol_sh.h, so
    bit for bit what the device multiplies a sample's colour by: order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), no
    Condon-Shortley sign, the direction as it comes (not normalised). Returns [..., 9] float32 - the caller's half of a reconstruction
    (sum_k L_k Y_k(n)) and of sh9_irradiance."""
    d = np.asarray(directions, dtype=np.float32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k0, k1, k2, k3, k4 = _SH9_K
    out = np.empty(d.shape[:-1] + (9,), dtype=np.float32)
    out[..., 0] = k0
    out[..., 1] = k1 * y
    out[..., 2] = k1 * z
    out[..., 3] = k1 * x
    out[..., 4] = (k2 * x) * y
    out[..., 5] = (k2 * y) * z
    out[..., 6] = k3 * ((np.float32(3.0) * (z * z)) - np.float32(1.0))
    out[..., 7] = (k2 * x) * z
    out[..., 8] = k4 * ((x * x) - (y * y))
    return out


def sh9_irradiance(L, normals):
    """Irradiance E(n) = sum_k A_l(k) L_k Y_k(n) for unit normals [m, 3] from radiance coefficients L [..., 9, 3] (SPHERE mode: L = 4 pi x sh /
    samples), with the cosine lobe's zonal factors A = (pi, 2 pi / 3, pi / 4) for l = 0, 1, 2. float64; returns [..., m, 3]."""
    a = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
    y = sh9(normals).astype(np.float64)
    return np.einsum("mk,...kc->...mc", y * a, np.asarray(L, dtype=np.float64))


# A SolTexel of sol_lightmap_points: the owning triangle (0xFFFFFFFF: none), the barycentrics b1, b2, the claim (1 centre, 2 conservative only).
LIGHTMAP_TEXEL_DTYPE = np.dtype([("triangle", np.uint32), ("b1", np.float32), ("b2", np.float32), ("flags", np.uint32)])


def lightmap_triangle_table(description, first, count):
    """The table sol_lightmap_coords takes: per dfs_index the lightmap triangle of the primitive, or SOL_TEXEL_NONE. Triangle first + k of the
    description (a Scene, or its SolSceneDesc - the one the handle was created from) is lightmap triangle k, row k of the uvs / vertices arrays;
    an entry also carries, in its two top bits, the rotation of the triangle's fp32 record (sol_triangle_rotation of include/solstrale_hip.h:
    the record starts opposite the longest edge), which is what a hit's (u, v) are measured in. uint32 [max dfs_index + 1]."""
    desc = getattr(description, "desc", description)
    first, count = int(first), int(count)
    if first < 0 or count < 0 or first + count > int(desc.n_triangles) or count > _abi.SOL_LIGHTMAP_TABLE_TRIANGLE_MASK:
        raise ValueError(f"triangles {first} .. {first + count} of a description with {int(desc.n_triangles)}")
    if count == 0:
        return np.zeros(0, dtype=np.uint32)
    rec = np.ctypeslib.as_array(C.cast(desc.triangles, C.POINTER(C.c_uint8)), shape=(int(desc.n_triangles), C.sizeof(_abi.SolTriangle)))[first:first + count]

    def field(name, dtype, n):
        at = getattr(_abi.SolTriangle, name).offset
        return np.ascontiguousarray(rec[:, at:at + n * np.dtype(dtype).itemsize]).view(dtype).reshape(count, n)
    a, b, dfs = field("v0v1", np.float64, 3), field("v0v2", np.float64, 3), field("dfs_index", np.uint32, 1)[:, 0]
    c = b - a
    l01, l02, l12 = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] for e in (a, b, c))
    k = np.where(l02 > l12, 1, 0)
    k = np.where(l01 > np.maximum(l12, l02), 2, k)
    table = np.full(int(dfs.max()) + 1, _abi.SOL_TEXEL_NONE, dtype=np.uint32)
    table[dfs] = np.arange(count, dtype=np.uint32) | (k.astype(np.uint32) << np.uint32(_abi.SOL_LIGHTMAP_TABLE_ROTATION_SHIFT))
    return table


def lightmap_mesh(description, first, count):
    """(vertices [count, 3, 3], uvs [count, 3, 2]) float32 of triangles first .. first + count of the description, in the description's order (the
    flattener's, not the builder's) and the triangles' own vertex order: the arrays lightmap_points and lightmap_sample take when the lightmap UVs
    are the description's texture coordinates - row k is the triangle lightmap_triangle_table(description, first, count) calls k."""
    desc = getattr(description, "desc", description)
    first, count = int(first), int(count)
    if first < 0 or count < 0 or first + count > int(desc.n_triangles):
        raise ValueError(f"triangles {first} .. {first + count} of a description with {int(desc.n_triangles)}")
    if count == 0:
        return np.zeros((0, 3, 3), dtype=np.float32), np.zeros((0, 3, 2), dtype=np.float32)
    rec = np.ctypeslib.as_array(C.cast(desc.triangles, C.POINTER(C.c_uint8)), shape=(int(desc.n_triangles), C.sizeof(_abi.SolTriangle)))[first:first + count]

    def field(name, dtype, n):
        at = getattr(_abi.SolTriangle, name).offset
        return np.ascontiguousarray(rec[:, at:at + n * np.dtype(dtype).itemsize]).view(dtype).reshape(count, n)
    v0, a, b = field("v0", np.float64, 3), field("v0v1", np.float64, 3), field("v0v2", np.float64, 3)
    V = np.stack([v0, v0 + a, v0 + b], axis=1).astype(np.float32)
    T = np.stack([field("uv0", np.float32, 2), field("uv1", np.float32, 2), field("uv2", np.float32, 2)], axis=1)
    return np.ascontiguousarray(V), np.ascontiguousarray(T)


CHART_NONE = 0xFFFFFFFF  # SOL_CHART_NONE: a triangle or texel without chart (DeviceScene.lightmap_charts)


def lightmap_mip_layout(width, height, levels=None):
    """The layout of a lightmap mip chain (sol_lightmap_mip_layout's rule) as a dict: `levels` - the count in force, level 0 counted
    (None or 0: all) -, `widths`, `heights` and `offsets` per level - W_l = (W_{l-1} + 1) // 2; offsets[l] is the first row of level l >= 1 in the
    chain, offsets[0] = 0: level 0 is the caller's atlas and not in the chain - and `rows`, the rows of the chain and the bytes of its cover
    plane."""
    width, height = int(width), int(height)
    if not (0 < width <= _abi.SOL_LIGHTMAP_MAX_SIZE and 0 < height <= _abi.SOL_LIGHTMAP_MAX_SIZE):
        raise ValueError(f"an atlas of {width} x {height} texels (1 .. {_abi.SOL_LIGHTMAP_MAX_SIZE} each way)")
    sizes = [(width, height)]
    while sizes[-1] != (1, 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    n = len(sizes) if not levels else int(levels)
    if not 1 <= n <= len(sizes):
        raise ValueError(f"{levels} levels (an atlas of {width} x {height} texels has {len(sizes)})")
    offsets, rows = [0], 0
    for w, h in sizes[1:n]:
        offsets.append(rows)
        rows += w * h
    return {"levels": n, "widths": [w for w, _ in sizes[:n]], "heights": [h for _, h in sizes[:n]], "offsets": offsets, "rows": rows}


def pixel_spread(vertical_fov_degrees, height):
    """The angle in radians between the rays of vertically neighbouring pixels at the centre of a pinhole image of `height` rows: what
    DeviceScene.lightmap_lod takes as `spread`."""
    return 2.0 * math.tan(math.radians(float(vertical_fov_degrees)) / 2.0) / float(height)


def lightmap_texels_to_numpy(rows):
    """The [n, 4] int32 device tensor DeviceScene.lightmap_points returned on the device route, as the structured host array."""
    return np.ascontiguousarray(rows.cpu().numpy()).view(LIGHTMAP_TEXEL_DTYPE).reshape(-1)


# A SolMoments of sol_irradiance_moments: the sums of the sample colours (sol_irradiance's answer), the count, the sums of their squares.
MOMENTS_DTYPE = np.dtype([("sum", np.float32, (3,)), ("samples", np.uint32), ("sum2", np.float32, (3,)), ("reserved", np.uint32)])


def moments_to_numpy(rows):
    """The [n, 8] float32 device tensor DeviceScene.irradiance_moments returned on the device route (or a host array of that shape), as the
    structured host array."""
    rows = rows.cpu().numpy() if hasattr(rows, "data_ptr") else rows
    return np.ascontiguousarray(rows).view(MOMENTS_DTYPE).reshape(-1)


def moments_mean_variance(rows):
    """The estimators of sol_irradiance_moments from its rows (a MOMENTS_DTYPE array, or what moments_to_numpy takes): (mean [n, 3], variance of
    the mean [n, 3]) in numpy float32 and exactly the operations of sol_lightmap_filter_var's "Prepare" - N = float32(samples), M = float32(samples
    - 1), x = sum / N, v = pos((sum2 / N) - (x * x)) / M - so bit for bit what the filter starts from. Rows with samples < 2 give a variance of
    zero, rows with samples = 0 a mean of zero too."""
    m = rows if isinstance(rows, np.ndarray) and rows.dtype == MOMENTS_DTYPE else moments_to_numpy(rows)
    f = np.float32
    n = m["samples"]
    with np.errstate(all="ignore"):
        N = n.astype(f)[:, None]
        M = (n - np.uint32(1)).astype(f)[:, None]
        x = m["sum"] / N
        d = (m["sum2"] / N) - (x * x)
        v = np.where(d > 0, d, f(0)).astype(f) / M
    x = np.where((n >= 1)[:, None], x, f(0)).astype(f)
    v = np.where((n >= 2)[:, None], v, f(0)).astype(f)
    return x, v


# What sol_visibility_oct gathers per texel and what sol_volume_build_depth makes of it.
OCT_TEXEL_DTYPE = np.dtype([("w", np.float32), ("w_open", np.float32), ("wt", np.float32), ("wt2", np.float32)])
DEPTH_TEXEL_DTYPE = np.dtype([("mean", np.float32), ("mean2", np.float32)])
# A SolProbe of sol_volume_build: the irradiance coefficients e[k][channel], the hit-distance moments, flags (1 valid, 2 has moments).
VOLUME_PROBE_DTYPE = np.dtype([("e", np.float32, (9, 3)), ("mean", np.float32), ("mean2", np.float32), ("flags", np.uint32), ("samples", np.uint32),
                               ("reserved", np.uint32)])


def volume_probes_to_numpy(rows):
    """The [n, 32] float32 device tensor DeviceScene.volume_build returned on the device route, as the structured host array."""
    return np.ascontiguousarray(rows.cpu().numpy()).view(VOLUME_PROBE_DTYPE).reshape(-1)


class VolumeGrid:
    """The probe grid of an irradiance volume (SolVolumeGrid): counts = (nx, ny, nz) probes, probe (i, j, k) at origin + (i, j, k) *
    spacing and in row (k * ny + j) * nx + i. backface / chebyshev: the two weights of volume_sample (probes behind the surface count less; a
    probe whose hit-distance moments say the point lies behind a wall counts less); normal_bias: a sample looks its cell up at position + unit
    normal * normal_bias."""

    def __init__(self, origin, spacing, counts, backface=True, chebyshev=True, normal_bias=0.0):
        self.origin = tuple(float(x) for x in origin)
        self.spacing = tuple(float(x) for x in (spacing if np.ndim(spacing) else (spacing,) * 3))
        self.counts = tuple(int(x) for x in counts)
        if len(self.origin) != 3 or len(self.spacing) != 3 or len(self.counts) != 3:
            raise ValueError("origin, spacing, counts: three numbers each (spacing may be one)")
        if any(c < 0 or c > 0xFFFFFFFF for c in self.counts):
            raise ValueError(f"counts: {self.counts} - each a 32-bit count (0 and more than 2^24 probes in all are the library's to refuse)")
        self.backface, self.chebyshev, self.normal_bias = bool(backface), bool(chebyshev), float(normal_bias)

    @property
    def n_probes(self):
        return self.counts[0] * self.counts[1] * self.counts[2]

    def record(self):
        """The SolVolumeGrid of this grid."""
        g = _abi.SolVolumeGrid(size=C.sizeof(_abi.SolVolumeGrid), nx=self.counts[0], ny=self.counts[1], nz=self.counts[2],
                               flags=(_abi.SOL_VOLUME_BACKFACE if self.backface else 0) | (_abi.SOL_VOLUME_CHEBYSHEV if self.chebyshev else 0),
                               normal_bias=self.normal_bias)
        g.origin[:] = self.origin
        g.spacing[:] = self.spacing
        return g


# A SolRayHit of sol_query and a SolVisibility of sol_visibility; DeviceScene carries both names too.
RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("status", np.uint32), ("kind", np.uint32),
                          ("dfs_index", np.uint32), ("material", np.uint32), ("reserved", np.uint32)])
VISIBILITY_DTYPE = np.dtype([("bent", np.float32, (3,)), ("open", np.uint32), ("t_sum", np.float32), ("t2_sum", np.float32),
                             ("hits", np.uint32), ("samples", np.uint32)])

# The element layouts of the array arguments and answers of the two-route entry points, written once: name -> (the structured host dtype or
# None, the host element dtype, the device dtype, what the host route takes besides the structured dtype). A structured array [..] is a device
# tensor [.., words] of its 32-bit words: LIGHTMAP_TEXEL_DTYPE [n] <-> int32 [n, 4], OCT_TEXEL_DTYPE [n, t] <-> float32 [n, t, 4]. On the host
# route "cast" takes any numbers and converts them (for a record: its raw rows [.., words]), "reshape" does the same for any shape that holds
# whole rows, "bits" takes uint32 or int32 and reinterprets them, and None takes the structured dtype alone; a tensor is brought over with
# .cpu() first and then goes as its raw rows.
_LAYOUTS = {
    "f32": (None, np.float32, "float32", "cast"),
    "f64": (None, np.float64, "float64", "cast"),
    "u8": (None, np.uint8, "uint8", "cast"),
    "u32": (None, np.uint32, "int32", "cast"),
    "words": (None, np.uint32, "int32", "bits"),
    "texel": (LIGHTMAP_TEXEL_DTYPE, np.int32, "int32", None),
    "hit": (RAY_HIT_DTYPE, np.int32, "int32", None),
    "moments": (MOMENTS_DTYPE, np.float32, "float32", "cast"),
    "visibility": (VISIBILITY_DTYPE, np.float32, "float32", "cast"),
    "probe": (VOLUME_PROBE_DTYPE, np.float32, "float32", "cast"),
    "oct": (OCT_TEXEL_DTYPE, np.float32, "float32", "reshape"),
    "depth": (DEPTH_TEXEL_DTYPE, np.float32, "float32", "reshape"),
}

# One array argument of a two-route entry point: its name, the caller's value, its layout (a key of _LAYOUTS) and its shape in elements of that
# layout - an int is an extent, None any extent, a string a symbol that the first argument to carry it binds for the others ("n", "k"). optional:
# None is taken and passes a null pointer; null_if_empty: so does an array without elements; aligned: a tensor's memory must be 16-byte aligned
# (the volume kernels move whole 16-byte words); flat: the host route takes any shape with as many elements (a plane as its rows); upload: on the
# device route a host value is staged as on the host route and copied to the scene's device ("any": so is a tensor that does not fit as it is).
_Arg = namedtuple("_Arg", "name value layout shape optional null_if_empty aligned flat upload", defaults=(False,) * 5)
# One answer: np.zeros of the layout's host dtype on the host route, torch.empty of its words on the device route (zero: torch.zeros).
_Out = namedtuple("_Out", "name layout shape zero null_if_empty", defaults=(False, False))


class DeviceScene:
    """sol_scene_create .. sol_scene_destroy"""

    def __init__(self, scene, device=0, world_tree=None, no_work_order_probe=False, split_percent=0, no_background_blocks=False, dynamic_triangles=False,
                 dynamic_primitives=False):
        """split_percent: SolCreateOptions.split_percent (0: the default budget of the device build's triangle pre-splitting, < 0: none);
        no_background_blocks: SolCreateOptions.no_background_blocks (do not look for blocks that provably see only the background);
        dynamic_triangles: SolCreateOptions.dynamic_triangles (keep what set_triangles needs); dynamic_primitives: SolCreateOptions.dynamic_primitives
        (keep what set_primitives needs to move spheres and quads as well; it extends dynamic_triangles and sets it)."""
        self.lib = _abi.load_hip()
        self.scene = scene
        self.h = C.c_void_p()
        dynamic_triangles = bool(dynamic_triangles or dynamic_primitives)
        if world_tree is None and not no_work_order_probe and not split_percent and not no_background_blocks and not dynamic_triangles:
            rc = self.lib.sol_scene_create(scene.desc_ptr, device, C.byref(self.h))
        else:
            opt = _abi.SolCreateOptions(size=C.sizeof(_abi.SolCreateOptions), world_tree=int(world_tree or 0),
                                        no_work_order_probe=1 if no_work_order_probe else 0, split_percent=int(split_percent),
                                        no_background_blocks=1 if no_background_blocks else 0, dynamic_triangles=1 if dynamic_triangles else 0,
                                        dynamic_primitives=1 if dynamic_primitives else 0)
            rc = self.lib.sol_scene_create_ex(scene.desc_ptr, device, C.byref(opt), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise DeviceError(rc, self.lib.sol_last_error().decode(errors="replace"))
        self.width, self.height = scene.width, scene.height
        self.device = int(device)

    def _chk(self, rc):
        if rc != 0:
            raise DeviceError(rc, self.lib.sol_last_error().decode(errors="replace"))

    def close(self):
        if self.h:
            self.lib.sol_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_partition(self, rank, world):
        self._chk(self.lib.sol_scene_set_partition(self.h, rank, world))

    def set_option(self, option, value):
        self._chk(self.lib.sol_scene_set_option(self.h, int(option), int(value)))

    def build_times(self):
        """Seconds sol_scene_create spent in host tree candidates / uploads / device tree build / probe renders."""
        out = (C.c_double * 4)()
        self._chk(self.lib.sol_scene_build_times(self.h, out))
        return dict(zip(("host_trees", "upload", "device_tree", "probes"), [float(x) for x in out]))

    def info(self):
        """sol_scene_info: the world tree in use (and why, when it is not the one asked for), the bound on the traversal stack."""
        r = _abi.SolSceneInfo()
        r.size = C.sizeof(r)
        self._chk(self.lib.sol_scene_info(self.h, C.byref(r)))
        return {"stack_bound": int(r.stack_bound), "lds_stack": int(r.lds_stack), "spill_stack": int(r.spill_stack),
                "tree_fallback": bool(r.tree_fallback), "tree_name": r.tree_name.decode(), "tree_note": r.tree_note.decode(),
                "split_references": int(r.split_references), "split_triangles": int(r.split_triangles), "split_area_ratio": float(r.split_area_ratio),
                "reinsertion_moves": int(r.reinsertion_moves), "reinsertion_area_ratio": float(r.reinsertion_area_ratio),
                "partition_table": int(r.partition_table), "partition_crc": int(r.partition_crc), "strict_triangles": bool(r.strict_triangles),
                "background_blocks": int(r.background_blocks), "background_pixels": int(r.background_pixels)}

    def path_stats(self):
        """sol_path_stats of the last counted render: primary hit fraction and the path-length histogram (shares of the samples)."""
        r = _abi.SolPathStats()
        r.size = C.sizeof(r)
        self._chk(self.lib.sol_path_stats(self.h, C.byref(r)))
        n = max(1, int(r.samples))
        bins = ("1", "2", "3-4", "5-8", "9-16", "17+")
        return {"samples": int(r.samples), "primary_hit_fraction": int(r.primary_hits) / n,
                "rays_per_path_histogram": {b: int(r.path_len[k]) / n for k, b in enumerate(bins)}}

    def max_samples_per_call(self):
        return int(self.lib.sol_max_samples_per_call(self.h))

    def comm_init(self, rank, world, unique_id):
        """sol_comm_init: RCCL communicator of the tile partition (collective over the ranks); also sets the partition."""
        buf = (C.c_uint8 * _abi.UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._chk(self.lib.sol_comm_init(self.h, rank, world, buf))

    def comm_destroy(self):
        self._chk(self.lib.sol_comm_destroy(self.h))

    def gather(self, image_ptr=0):
        """sol_gather: collective; rank 0 gets the row-major image in device memory `image_ptr` (0: the scene's own buffer)."""
        self._chk(self.lib.sol_gather(self.h, C.c_void_p(image_ptr)))

    def comm_self_check(self):
        self._chk(self.lib.sol_comm_self_check(self.h))

    def read_image(self):
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.lib.sol_read_image(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def set_stream(self, hip_stream):
        self._chk(self.lib.sol_scene_set_stream(self.h, C.c_void_p(hip_stream)))

    def accum_floats(self):
        return int(self.lib.sol_accum_floats(self.h))

    def accum_ptr(self):
        return int(self.lib.sol_accum_ptr(self.h) or 0)

    def bind_accum(self, device_ptr, n_floats):
        self._chk(self.lib.sol_scene_bind_accum(self.h, C.c_void_p(device_ptr), n_floats))

    def clear(self):
        self._chk(self.lib.sol_clear(self.h))

    def render(self, first_sample, n_samples, seed, counted=False):
        f = self.lib.sol_render_counted if counted else self.lib.sol_render
        self._chk(f(self.h, first_sample, n_samples, seed))

    def sync(self):
        self._chk(self.lib.sol_sync(self.h))

    def read(self):
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.lib.sol_read(self.h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def render_aux(self, first_sample, n_samples, seed):
        """Adds the samples' first-hit albedo and normal to the auxiliary accumulators (renderer/mod.rs:175-204)."""
        self._chk(self.lib.sol_render_aux(self.h, first_sample, n_samples, seed))

    def clear_aux(self):
        self._chk(self.lib.sol_clear_aux(self.h))

    def read_aux(self):
        """(albedo sums, normal sums), each (H, W, 3) float32, row 0 = top."""
        a = np.empty((self.height, self.width, 3), dtype=np.float32)
        n = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._chk(self.lib.sol_read_aux(self.h, a.ctypes.data_as(C.POINTER(C.c_float)), n.ctypes.data_as(C.POINTER(C.c_float))))
        return a, n

    def unpermute(self, gathered_ptr, world, image_ptr):
        self._chk(self.lib.sol_unpermute(self.h, C.c_void_p(gathered_ptr), world, C.c_void_p(image_ptr)))

    def tonemap_rgb8(self, image_ptr, num_samples):
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.lib.sol_tonemap_rgb8(self.h, C.c_void_p(image_ptr), num_samples,
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- adaptive sampling (EXTENSION) ----
    def adaptive_begin(self, round, min_samples, max_samples, threshold):
        """sol_adaptive_begin: clears the accumulator and opens a session of rounds of `round` samples."""
        cfg = _abi.SolAdaptive(size=C.sizeof(_abi.SolAdaptive), round=int(round), min_samples=int(min_samples),
                               max_samples=int(max_samples), threshold=float(threshold))
        self._chk(self.lib.sol_adaptive_begin(self.h, C.byref(cfg)))

    def adaptive_round(self, seed):
        """sol_adaptive_round: renders one round; returns the blocks the next round samples (0: done)."""
        n = C.c_uint32()
        self._chk(self.lib.sol_adaptive_round(self.h, seed, C.byref(n)))
        return int(n.value)

    def adaptive_run(self, seed):
        """Rounds until every block has stopped; returns the number of rounds."""
        rounds = 0
        while True:
            rounds += 1
            if self.adaptive_round(seed) == 0:
                return rounds

    def adaptive_counts(self):
        """Samples per pixel of every 8x8 block: uint32 array [blocks_y, blocks_x]."""
        bx, by = (self.width + 7) // 8, (self.height + 7) // 8
        out = np.zeros((by, bx), dtype=np.uint32)
        self._chk(self.lib.sol_adaptive_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def tonemap_rgb8_adaptive(self, image_ptr):
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.lib.sol_tonemap_rgb8_adaptive(self.h, C.c_void_p(image_ptr), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def adaptive_rescale(self, image_ptr):
        """sol_adaptive_rescale: image <- sum * max_samples / n_b in place (the input of bloom)."""
        self._chk(self.lib.sol_adaptive_rescale(self.h, C.c_void_p(image_ptr)))

    # ---- environment importance sampling (EXTENSION) ----
    def env_sampling(self, mode):
        """sol_env_sampling: mode None / 0 / "off" = off, "importance" / 1 = the environment map is one more light of the mixture."""
        m = {None: 0, 0: 0, "off": 0, 1: 1, "importance": 1}.get(mode, mode)
        if m not in (0, 1):
            raise ValueError(f"env_sampling: unknown mode {mode!r}")
        cfg = _abi.SolEnvSampling(size=C.sizeof(_abi.SolEnvSampling), mode=m)
        self._chk(self.lib.sol_env_sampling(self.h, C.byref(cfg)))

    def env_tables(self):
        """sol_env_tables: (marginal CDF [H'], conditional CDFs [H', W'], total), float32, H' = max(H - 1, 1), W' = max(W - 1, 1)."""
        d = self.scene.desc
        cw, ch = max(int(d.env_width) - 1, 1), max(int(d.env_height) - 1, 1)
        marg = np.zeros(ch, dtype=np.float32)
        cond = np.zeros((ch, cw), dtype=np.float32)
        total = C.c_float()
        self._chk(self.lib.sol_env_tables(self.h, marg.ctypes.data, marg.size, cond.ctypes.data, cond.size, C.byref(total)))
        return marg, cond, float(total.value)

    def env_eval(self, fn, rows):
        """sol_env_eval on the device: fn 0 ("sample"): rows (n, 2) of (r1, r2) -> (n, 6) direction xyz, pdf, cell i, cell j;
        fn 1 ("pdf"): rows (n, 3) of directions -> (n, 3) pdf, cell i, cell j."""
        fn = {"sample": 0, "pdf": 1}.get(fn, fn)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if fn not in (0, 1) or rows.ndim != 2 or rows.shape[1] != (2 if fn == 0 else 3):
            raise ValueError("env_eval: fn 0 takes (n, 2) rows, fn 1 (n, 3)")
        out = np.zeros((rows.shape[0], 6 if fn == 0 else 3), dtype=np.float32)
        self._chk(self.lib.sol_env_eval(self.h, fn, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out

    # ---- light tree and power-weighted light sampling (EXTENSION) ----
    def light_sampling(self, mode):
        """sol_light_sampling: mode None / 0 / "uniform", 1 / "tree" (the same frames through the light tree), 2 / "power"."""
        m = {None: 0, "uniform": 0, "tree": 1, "power": 2}.get(mode, mode)
        if m not in (0, 1, 2):
            raise ValueError(f"light_sampling: unknown mode {mode!r}")
        cfg = _abi.SolLightSampling(size=C.sizeof(_abi.SolLightSampling), mode=m)
        self._chk(self.lib.sol_light_sampling(self.h, C.byref(cfg)))

    def light_tables(self):
        """sol_light_tables: (q [L], C [L]) float32 as the device holds them, and W (the f64 sum of the weights). Needs mode 2 once."""
        n = int(self.scene.desc.n_lights)
        q = np.zeros(n, dtype=np.float32)
        cdf = np.zeros(n, dtype=np.float32)
        total = C.c_double()
        self._chk(self.lib.sol_light_tables(self.h, q.ctypes.data, cdf.ctypes.data, n, C.byref(total)))
        return q, cdf, float(total.value)

    def light_tree(self):
        """sol_light_tree: (nodes (N, 6) float32 = min xyz, max xyz; index of leaf 0; bytes). Needs mode 1 or 2 once."""
        nn, first, nb = C.c_uint32(), C.c_uint32(), C.c_size_t()
        self._chk(self.lib.sol_light_tree(self.h, None, 0, C.byref(nn), C.byref(first), C.byref(nb)))
        nodes = np.zeros((nn.value, 6), dtype=np.float32)
        self._chk(self.lib.sol_light_tree(self.h, nodes.ctypes.data, nodes.size, None, None, None))
        return nodes, int(first.value), int(nb.value)

    def light_eval(self, fn, rows):
        """sol_light_eval on the device: fn 0 ("density"): rows (n, 6) of origin xyz, direction xyz -> (n, 4) loop density, tree density,
        nodes visited, light tests; fn 1 ("select"): u (n,) -> (n,) selected light index (int64)."""
        fn = {"density": 0, "select": 1}.get(fn, fn)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if fn == 0 and (rows.ndim != 2 or rows.shape[1] != 6):
            raise ValueError("light_eval: fn 0 takes (n, 6) rows")
        if fn == 1:
            rows = rows.reshape(-1)
        elif fn != 0:
            raise ValueError(f"light_eval: unknown function {fn!r}")
        out = np.zeros((rows.shape[0], 4) if fn == 0 else rows.shape[0], dtype=np.float32)
        self._chk(self.lib.sol_light_eval(self.h, fn, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out if fn == 0 else out.astype(np.int64)

    def resolve_image(self):
        """Device pointer of the scene's own row-major image (W*H*3 floats) after un-permuting its accumulators."""
        p = C.c_void_p()
        self._chk(self.lib.sol_resolve_image(self.h, C.byref(p)))
        return p.value

    # ---- denoiser (EXTENSION) ----
    def resolve_aux(self):
        """sol_resolve_aux: (albedo device pointer, normal device pointer, aux samples) - the row-major planes (W*H*3 floats each) the
        scene owns, and the samples sol_render_aux added since they were last cleared."""
        a, n, m = C.c_void_p(), C.c_void_p(), C.c_uint32()
        self._chk(self.lib.sol_resolve_aux(self.h, C.byref(a), C.byref(n), C.byref(m)))
        return a.value, n.value, int(m.value)

    def denoise(self, image_ptr, num_samples, albedo_ptr, normal_ptr, aux_samples, iterations=None, sigma_color=None, normal_power=None):
        """sol_denoise: the guided a-trous filter on the device image (W*H*3 float sums of num_samples), in place, asynchronous."""
        cfg = _abi.denoise_config(iterations, sigma_color, normal_power)
        self._chk(self.lib.sol_denoise(self.h, C.c_void_p(image_ptr), num_samples, C.c_void_p(albedo_ptr), C.c_void_p(normal_ptr),
                                       aux_samples, C.byref(cfg)))

    def denoise_rgb8(self, image_ptr, num_samples, albedo_ptr, normal_ptr, aux_samples, iterations=None, sigma_color=None, normal_power=None):
        """sol_denoise_rgb8: the filter into scratch, then the Nop tone map -> RGB8 (H, W, 3); the image is left alone."""
        cfg = _abi.denoise_config(iterations, sigma_color, normal_power)
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.lib.sol_denoise_rgb8(self.h, C.c_void_p(image_ptr), num_samples, C.c_void_p(albedo_ptr), C.c_void_p(normal_ptr),
                                            aux_samples, C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ---- ray queries (EXTENSION) ----
    RAY_HIT_DTYPE = RAY_HIT_DTYPE

    # The two routes of an array entry point: sol_x takes host arrays and stages them, sol_x_dev takes device pointers, both in the same positions.
    @staticmethod
    def _on_device(x):
        """The route a value asks for: a tensor (whatever has data_ptr) goes the device route, everything else the host route."""
        return hasattr(x, "data_ptr")

    @staticmethod
    def _fit(shape, pattern, dims):
        """The symbols of `pattern` that `shape` binds beyond `dims`; None where it does not fit."""
        if len(shape) != len(pattern):
            return None
        new = {}
        for have, want in zip(shape, pattern):
            if isinstance(want, str):
                want = dims[want] if want in dims else new.setdefault(want, int(have))
            if want is not None and want != have:
                return None
        return new

    @staticmethod
    def _wanted(a, device):
        """What argument `a` has to be, for the refusal."""
        st, word, dev_dtype, raw = _LAYOUTS[a.layout]
        rows = a.shape + (() if st is None else (st.itemsize // 4,))

        def text(shape):
            return "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
        if device:
            return f"{a.name}: a contiguous {dev_dtype} tensor of shape {text(rows)} on the scene's device"
        if st is None:
            return f"{a.name}: {np.dtype(word).name} numbers of shape {text(rows)}" + (", or as many in another shape" if a.flat else "")
        return f"{a.name}: {a.layout} records of shape {text(a.shape)}" + ("" if raw is None else f", or their raw {np.dtype(word).name} rows {text(rows)}")

    def _host_rows(self, a, dims):
        """Argument `a` as the host route hands it over: a contiguous array of its layout, its shape checked (its symbols go to `dims`)."""
        st, word, _, raw = _LAYOUTS[a.layout]
        x = np.ascontiguousarray(a.value.cpu().numpy() if self._on_device(a.value) else a.value)
        pattern, fits = a.shape, True
        if st is not None and raw is None:  # (the structured dtype alone; a tensor holds its raw rows)
            x = x.view(st).reshape(-1) if self._on_device(a.value) else x
            fits = x.dtype == st
        elif raw == "bits" and x.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)):
            raise ValueError(f"{a.name}: 32-bit words (a uint32 or int32 array, or an int32 tensor), not {x.dtype}")
        else:  # (the words of the layout: a structured array reinterpreted, anything else converted)
            record = st is not None and x.dtype == st
            x = x.view(word) if record or raw == "bits" else np.ascontiguousarray(x.astype(word, copy=False))
            if st is not None:
                pattern += (st.itemsize // 4,)
                if raw == "reshape" and x.size % math.prod(pattern[1:]) == 0:
                    x = x.reshape((-1,) + pattern[1:])
                elif record:
                    x = x.reshape(-1, pattern[-1])
        if a.flat:
            x, pattern = x.reshape(-1), (math.prod(pattern),) if len(pattern) > 1 else pattern
        new = self._fit(x.shape, pattern, dims) if fits else None
        if new is None:
            raise ValueError(self._wanted(a, False))
        dims.update(new)
        return x

    def _stage(self, args, device):
        """Makes or checks the arrays of one call (`args`: _Arg, in the order they are checked) and waits for torch's stream when one of them is
        on the device. Returns (the pointers by name - None: a null pointer -, the extents the symbols stand for, what must live through the call)."""
        p, dims, keep = {}, {}, []
        if device:
            import torch
        for a in args:
            st, _, dev_dtype, raw = _LAYOUTS[a.layout]
            x, staged = a.value, None
            if x is None:
                if not a.optional:
                    raise ValueError(self._wanted(a, device) + ", not None")
                p[a.name] = None
                continue
            if device and self._on_device(x) and x.dtype == getattr(torch, dev_dtype) and x.is_contiguous() and x.is_cuda and x.device.index == self.device:
                shape, pattern = tuple(x.shape), a.shape + (() if st is None else (st.itemsize // 4,))
                if raw == "reshape" and shape:  # (a probe's map may come as one row)
                    shape, pattern = (shape[0], math.prod(shape[1:])), (pattern[0], math.prod(pattern[1:]))
                new = self._fit(shape, pattern, dims)
                if new is not None:
                    if a.aligned and x.data_ptr() % 16:  # (a view that starts inside an allocation: the kernels move whole 16-byte words)
                        raise ValueError(f"{a.name}: the tensor's memory must be 16-byte aligned")
                    dims.update(new)
                    staged = x
            if staged is None:
                if device and not (a.upload == "any" or a.upload and not self._on_device(x)):
                    raise ValueError(self._wanted(a, True))
                staged = self._host_rows(a, dims)
                if device:
                    staged = torch.from_numpy(staged.view(np.int32) if staged.dtype == np.uint32 else staged).to(f"cuda:{self.device}")
            keep.append(staged)
            empty = not (staged.numel() if device else staged.size)
            p[a.name] = None if a.null_if_empty and empty else staged.data_ptr() if device else staged.ctypes.data
        if device and keep:
            torch.cuda.current_stream(self.device).synchronize()  # (the tensors may still be in the making on torch's stream: the scene's is another)
        return p, dims, keep

    def _call(self, entry, args, outs, fn, device=None, dev_suffix="_dev", sync=True):
        """One call of a two-route entry point. The first argument decides the route (or `device` does); the arrays are made or checked (_stage),
        the answers `outs` (_Out) allocated, and fn(p, d) - p: the pointers of arguments and answers by name, d: the extents of the symbols - gives
        the arguments after the handle, the same for sol_x and sol_x_dev. The device route waits for torch's stream before the call and, unless
        the call blocks by itself (sync=False), for the scene's stream after it. Returns the answers by name."""
        device = self._on_device(args[0].value) if device is None else device
        p, d, keep = self._stage(args, device)
        if device:
            import torch
        made = {}
        for o in outs:
            st, word, dev_dtype, _ = _LAYOUTS[o.layout]
            shape = tuple(d[s] if isinstance(s, str) else int(s) for s in o.shape)
            if device:
                x = (torch.zeros if o.zero else torch.empty)(shape + (() if st is None else (st.itemsize // 4,)), dtype=getattr(torch, dev_dtype),
                                                             device=f"cuda:{self.device}")
            else:
                x = np.zeros(shape, dtype=st or word)
            made[o.name] = x
            p[o.name] = None if o.null_if_empty and not math.prod(shape) else x.data_ptr() if device else x.ctypes.data
        self._chk(getattr(self.lib, entry + (dev_suffix if device else ""))(self.h, *fn(p, d)))
        if device and sync:
            self.sync()
        return made

    @staticmethod
    def _split(rows, shape=(3,)):
        """The host route's [n, k + 1] rows of sums and a count as (sums [n, *shape] float32, counts [n] uint32); the device route's raw rows stay."""
        if not isinstance(rows, np.ndarray):
            return rows
        return np.ascontiguousarray(rows[:, :-1]).reshape((-1,) + shape), np.ascontiguousarray(rows[:, -1]).view(np.uint32)

    @staticmethod
    def _stride(values):
        """The bytes of a row of `values` for a config struct; 0 for what is not rows (the checks refuse it)."""
        return 4 * int(values.shape[1]) if getattr(values, "ndim", 0) == 2 else 0

    def _query(self, mode, rays):
        answer = "u32" if mode == _abi.SOL_QUERY_OCCLUDED else "hit"
        return self._call("sol_query", [_Arg("rays", rays, "f32", ("n", 8))], [_Out("out", answer, ("n",))],
                          lambda p, d: (mode, p["rays"], d["n"], p["out"]))["out"]

    def closest_hits(self, rays):
        """sol_query, SOL_QUERY_CLOSEST. A numpy [n, 8] float32 array of (origin xyz, tmin, direction xyz, tmax) goes the host route and
        returns a structured array (RAY_HIT_DTYPE); a contiguous [n, 8] float32 torch tensor on the scene's device goes through sol_query_dev
        without a host copy and returns an [n, 8] int32 device tensor of the same eight words (hits_to_numpy views it as the structured
        array); the call waits for torch's stream before and for the scene's stream after the launch."""
        return self._query(_abi.SOL_QUERY_CLOSEST, rays)

    def occluded(self, rays):
        """sol_query, SOL_QUERY_OCCLUDED: one status per ray (SOL_RAY_HIT exactly when closest_hits reports a hit); uint32 array, or an
        int32 device tensor for a device tensor of rays."""
        return self._query(_abi.SOL_QUERY_OCCLUDED, rays)

    @classmethod
    def hits_to_numpy(cls, hits):
        """The [n, 8] int32 device tensor closest_hits returned, as the structured host array."""
        return hits.cpu().numpy().view(cls.RAY_HIT_DTYPE).reshape(-1)

    def camera_rays(self, x0, y0, x1, y1, sample, seed):
        """sol_camera_rays: the camera rays of pixels [x0, x1) x [y0, y1) for (sample, seed) as an [h, w, 8] float32 device tensor."""
        import torch
        h, w = max(int(y1) - int(y0), 0), max(int(x1) - int(x0), 0)
        out = torch.empty((h, w, 8), dtype=torch.float32, device=f"cuda:{self.device}")
        self._chk(self.lib.sol_camera_rays(self.h, x0, y0, x1, y1, sample, seed, C.c_void_p(out.data_ptr())))
        self.sync()  # (the scene's stream is not torch's)
        return out

    # ---- radiance queries (EXTENSION) ----
    def radiance(self, rays, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0):
        """sol_radiance: the path-traced colour along the caller's rays, `samples` samples from `first_sample` on, in the handle's current shader
        and sampling modes. keys: per ray (pixel, first_draw) - the RNG key and the starting counter; None: key_base + i and first_draw. A numpy
        [n, 8] float32 array (and an optional [n, 2] uint32 one) goes the host route and returns (rgb_sum [n, 3] float32, samples [n] uint32);
        contiguous torch tensors on the scene's device ([n, 8] float32, [n, 2] int32) go through sol_radiance_dev without a host copy and return
        one [n, 4] float32 device tensor of the raw rows (r, g, b sums and the bits of the sample count); the call waits for torch's stream
        before and for the scene's stream after the launch."""
        cfg = _abi.SolRadianceConfig(size=C.sizeof(_abi.SolRadianceConfig), samples=int(samples), first_sample=int(first_sample), first_draw=int(first_draw),
                                     seed=int(seed), key_base=int(key_base) & 0xFFFFFFFF)
        return self._split(self._radiance("sol_radiance", "rays", rays, keys, cfg))

    def _radiance(self, entry, what, rays, keys, cfg, words=4, call=lambda *a: a):
        """The call radiance(), irradiance(), irradiance_sh(), visibility() and their kin share: `rays` are the [n, 8] rows (`what`: their name in
        messages), `keys` the optional [n, 2] rows of (pixel, first_draw), `words` the 32-bit words of an answer; `call` turns (rays, keys, n, config,
        out) into the entry point's own arguments. Returns the raw [n, words] float32 rows of either route."""
        return self._call(entry, [_Arg(what, rays, "f32", ("n", 8)), _Arg("keys", keys, "u32", ("n", 2), optional=True)], [_Out("out", "f32", ("n", words))],
                          lambda p, d: call(p[what], p["keys"], d["n"], C.byref(cfg), p["out"]))["out"]

    # ---- irradiance queries (EXTENSION) ----
    IRRADIANCE_MODES = {"cosine": _abi.SOL_IRRADIANCE_COSINE, "sphere": _abi.SOL_IRRADIANCE_SPHERE}

    def _irradiance_config(self, samples, first_sample, seed, key_base, first_draw, mode):
        if mode not in self.IRRADIANCE_MODES:
            raise ValueError(f"mode: 'cosine' or 'sphere', not {mode!r}")
        return _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=int(samples), first_sample=int(first_sample), first_draw=int(first_draw),
                                        seed=int(seed), key_base=int(key_base) & 0xFFFFFFFF, mode=self.IRRADIANCE_MODES[mode])

    def irradiance(self, points, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="cosine"):
        """sol_irradiance: the gather at the caller's points - rows of (position xyz, tmin, normal xyz, tmax). Every sample draws a fresh direction
        on the device ("cosine": cosine-weighted about the normal, irradiance = pi * sum / samples; "sphere": uniform, mean radiance = sum /
        samples) and is then radiance()'s path. keys, key_base, first_draw and the two routes with their return shapes are radiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        return self._split(self._radiance("sol_irradiance", "points", points, keys, cfg))

    def irradiance_rays(self, points, sample, seed=0, keys=None, key_base=0, first_draw=0, mode="cosine"):
        """sol_irradiance_rays: the rays sample `sample` of irradiance() starts with and the keys its paths go on from, as ([n, 8] float32, [n, 2]
        int32) device tensors: radiance(rays, samples=1, first_sample=sample, seed=seed, keys=keys) is that sample's contribution, bit for bit.
        points and keys: device tensors as for irradiance(), or host arrays, which are copied to the scene's device first."""
        cfg = self._irradiance_config(1, sample, seed, key_base, first_draw, mode)
        out = self._call("sol_irradiance_rays", [_Arg("points", points, "f32", ("n", 8), upload=True), _Arg("keys", keys, "u32", ("n", 2), optional=True, upload=True)],
                         [_Out("rays", "f32", ("n", 8)), _Out("keys_out", "u32", ("n", 2))],
                         lambda p, d: (p["points"], p["keys"], d["n"], C.byref(cfg), p["rays"], p["keys_out"]), device=True, dev_suffix="")
        return out["rays"], out["keys_out"]

    # ---- SH irradiance queries (EXTENSION) ----
    def irradiance_sh(self, points, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="sphere"):
        """sol_irradiance_sh: irradiance()'s gather projected onto the nine real SH terms up to l = 2 - per point the SUMS over the samples of
        colour x sh9(direction), in radiance()'s association. Host arrays return (sh [n, 9, 3] float32 sums, counts [n] uint32); device tensors
        go through sol_irradiance_sh_dev without a host copy and return one [n, 28] float32 device tensor of the raw rows (27 sums, k-major, and
        the bits of the sample count). "sphere": 4 pi x sh / samples are the radiance coefficients L_k, and sh9_irradiance(L, normals) the
        irradiance for any normal; "cosine": pi x sh / samples estimates the cosine-weighted projection about the point's normal. points, keys,
        key_base, first_draw and the waits of the two routes are irradiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        return self._split(self._radiance("sol_irradiance_sh", "points", points, keys, cfg, words=28), (9, 3))

    # ---- visibility gathers (EXTENSION) ----
    VISIBILITY_DTYPE = VISIBILITY_DTYPE

    def visibility(self, points, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="cosine", distances=False):
        """sol_visibility: how much of the hemisphere ("cosine") or of the sphere ("sphere") is open at the caller's points - rows of (position xyz,
        tmin, normal xyz, tmax), tmax being the occlusion radius. Every sample draws the direction irradiance() would draw and is answered as
        occluded() answers that ray (distances=True: as closest_hits() does, which also sums the hit distances and their squares). Per point:
        `open` samples that missed and `bent`, the sum of their directions; `hits`, `t_sum`, `t2_sum`; `samples`. open / samples is the ambient
        occlusion or the sky visibility, bent normalised the bent normal. Host arrays go the host route and return a structured array
        (VISIBILITY_DTYPE); device tensors go through sol_visibility_dev without a host copy and return the raw [n, 8] float32 rows
        (visibility_to_numpy views them as the structured array). points, keys, key_base, first_draw and the waits of the two routes are irradiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        qmode = _abi.SOL_QUERY_CLOSEST if distances else _abi.SOL_QUERY_OCCLUDED
        rows = self._radiance("sol_visibility", "points", points, keys, cfg, words=8, call=lambda *a: (qmode, *a))
        return rows.view(VISIBILITY_DTYPE).reshape(-1) if isinstance(rows, np.ndarray) else rows

    @classmethod
    def visibility_to_numpy(cls, rows):
        """The [n, 8] float32 device tensor visibility() returned, as the structured host array."""
        return np.ascontiguousarray(rows.cpu().numpy()).view(cls.VISIBILITY_DTYPE).reshape(-1)

    # ---- lightmap texel points and border dilation (EXTENSION) ----
    def lightmap_points(self, vertices, uvs, width, height, normals=None, tmin=1e-3, tmax=float("inf"), conservative=False):
        """sol_lightmap_points: the mesh's lightmap UVs rasterised into a `width` x `height` atlas. vertices [n, 3, 3], uvs [n, 3, 2] and the
        optional per-corner normals [n, 3, 3] are float32: numpy arrays go the host route, contiguous torch tensors on the scene's device go through
        sol_lightmap_points_dev without a copy. Returns (points, texels): the [height * width, 8] float32 rows (position, tmin, normal, tmax) that
        irradiance(), irradiance_sh() and visibility() take - eight zero words, an invalid point, where no triangle owns the texel - and the
        SolTexel rows (owner, b1, b2, flags): a LIGHTMAP_TEXEL_DTYPE array on the host route, an [n, 4] int32 device tensor on the device route
        (lightmap_texels_to_numpy views it). conservative: texels a triangle merely touches are claimed too, behind every centre claim."""
        cfg = _abi.SolLightmapConfig(size=C.sizeof(_abi.SolLightmapConfig), width=int(width), height=int(height),
                                     flags=_abi.SOL_LIGHTMAP_CONSERVATIVE if conservative else 0, tmin=float(tmin), tmax=float(tmax))
        wh = int(width) * int(height) if 0 < int(width) <= _abi.SOL_LIGHTMAP_MAX_SIZE and 0 < int(height) <= _abi.SOL_LIGHTMAP_MAX_SIZE else 1
        out = self._call("sol_lightmap_points", [_Arg("vertices", vertices, "f32", ("n", 3, 3)), _Arg("uvs", uvs, "f32", ("n", 3, 2)),
                                                 _Arg("normals", normals, "f32", ("n", 3, 3), optional=True)],
                         [_Out("points", "f32", (wh, 8)), _Out("texels", "texel", (wh,))],
                         lambda p, d: (p["vertices"], p["normals"], p["uvs"], d["n"], C.byref(cfg), p["points"], p["texels"]))
        return out["points"], out["texels"]

    def lightmap_dilate(self, values, texels, width, height, passes=1, channels=3, return_pass_of=False):
        """sol_lightmap_dilate: the border dilation that finishes a bake. values: `width * height` rows whose leading `channels` 32-bit words are
        floats (a [n, k] float32 array or tensor - the raw rows a gather returned: channels=3 for radiance / irradiance rows, 27 for irradiance_sh);
        texels: what lightmap_points returned. Owned rows are copied whole; in each of `passes` passes an uncovered texel with a covered neighbour
        gets their mean, the rest of its row zero. Host arrays go the host route, device tensors the device route, and the answer has the shape and
        place of `values`. return_pass_of: also the uint8 plane [height, width] of 0 owned, k filled in pass k, 255 never filled."""
        width, height = int(width), int(height)
        out = self._call("sol_lightmap_dilate", [_Arg("values", values, "f32", (width * height, "k")), _Arg("texels", texels, "texel", (width * height,))],
                         [_Out("out", "f32", (width * height, "k"))] + ([_Out("pass_of", "u8", (height, width))] if return_pass_of else []),
                         lambda p, d: (p["texels"], width, height, p["values"], int(channels), d["k"] * 4, int(passes), p["out"], p.get("pass_of")))
        return (out["out"], out["pass_of"]) if return_pass_of else out["out"]

    # ---- lightmap filtering (EXTENSION) ----
    def lightmap_filter(self, values, points, texels, width, height, sigma_position, sigma_plane=None, iterations=4, normal_power_log2=5, sigma_value=0.25,
                        value_scale=1.0, channels=3):
        """sol_lightmap_filter: the chart-aware a-trous filter between the gather and lightmap_dilate. values: `width * height` rows whose leading
        `channels` 32-bit words are floats (a [n, k] float32 array or tensor - the raw rows a gather returned: channels=3 for radiance / irradiance
        rows, 27 for irradiance_sh); points, texels: what lightmap_points returned. sigma_position is a WORLD LENGTH, about two texels' world size:
        the distance factor of pass i is 1 / (1 + |P_q - P_p|^2 / (sigma_position * 2^i)^2), and it is what keeps charts that are neighbours in the
        atlas from mixing. sigma_plane (None: sigma_position) is the same for the distance of the tap from the centre's tangent plane. The normal
        factor is pos(n_p . n_q)^(2^normal_power_log2). sigma_value compares the values after x * value_scale -> a / (1 + a); for irradiance SUMS
        value_scale is pi / samples, which brings them to irradiance. float("inf") switches a sigma's factor off. `iterations` passes (1..8) with
        steps 1, 2, 4, .. Rows of texels that are not live (no owner, or a word that is not finite) come back as they went in. Host arrays go the
        host route, device tensors the device route, and the answer has the shape and place of `values`."""
        width, height = int(width), int(height)
        cfg = _abi.SolLightmapFilterConfig(size=C.sizeof(_abi.SolLightmapFilterConfig), width=width, height=height, iterations=int(iterations),
                                           normal_power_log2=int(normal_power_log2), channels=int(channels), stride_bytes=self._stride(values),
                                           sigma_position=float(sigma_position), sigma_plane=float(sigma_position if sigma_plane is None else sigma_plane),
                                           sigma_value=float(sigma_value), value_scale=float(value_scale))
        wh = width * height
        args = [_Arg("values", values, "f32", (wh, "k")), _Arg("points", points, "f32", (wh, 8)), _Arg("texels", texels, "texel", (wh,))]
        return self._call("sol_lightmap_filter", args, [_Out("out", "f32", (wh, "k"))],
                          lambda p, d: (C.byref(cfg), p["points"], p["texels"], p["values"], p["out"]))["out"]

    # ---- irradiance moments and the variance-guided lightmap filter (EXTENSION) ----
    def irradiance_moments(self, points, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="cosine"):
        """sol_irradiance_moments: irradiance()'s gather with the sums of the squared sample colours beside it. Per point `sum` (irradiance()'s
        answer, bit for bit), `samples`, `sum2` - the sums over the samples of colour x colour per channel, in radiance()'s association - and
        `reserved` = 0. Host arrays go the host route and return a structured array (MOMENTS_DTYPE); device tensors go through
        sol_irradiance_moments_dev without a host copy and return the raw [n, 8] float32 rows (moments_to_numpy views them as the structured
        array). moments_mean_variance gives the mean and the variance of the mean. points, keys, key_base, first_draw, the modes and the waits
        of the two routes are irradiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        rows = self._radiance("sol_irradiance_moments", "points", points, keys, cfg, words=8)
        return rows.view(MOMENTS_DTYPE).reshape(-1) if isinstance(rows, np.ndarray) else rows

    def lightmap_filter_var(self, moments, points, texels, width, height, sigma_position, sigma_plane=None, iterations=4, normal_power_log2=5, sigma_value=4.0,
                            variance_floor=1e-12, return_variance=False):
        """sol_lightmap_filter_var: the variance-guided a-trous filter between irradiance_moments() and lightmap_dilate(). moments: `width * height`
        rows as irradiance_moments returned them (a MOMENTS_DTYPE array or [n, 8] float32 rows on the host route, the [n, 8] float32 device tensor
        on the device route); points, texels: what lightmap_points returned. sigma_position, sigma_plane (None: sigma_position), iterations and
        normal_power_log2 are lightmap_filter()'s. The value factor of a tap is 1 / (1 + D / (sigma_value^2 V))^2 with D the squared difference of
        the two means and V the centre's variance of the mean, prefiltered over 3 x 3 texels, plus variance_floor: sigma_value counts standard
        deviations, and the variance the filter carries shrinks from pass to pass. The defaults 4.0 (SVGF's value) and 1e-12 come from a CPU model
        of a bake and are not tuned on a device. float("inf") switches a sigma's factor off. Texels that are not live (no owner, fewer than two
        samples, a word that is not finite) come back as the first four words of their moments row. Returns the [width * height, 4] float32 rows
        of filtered SUMS (r, g, b and the bits of the sample count: what lightmap_filter returns for such a bake and lightmap_dilate takes), and
        with return_variance=True also the [width * height, 4] float32 rows (v_r, v_g, v_b, 0) of the variance of the filtered mean. Host arrays
        go the host route, device tensors the device route."""
        width, height = int(width), int(height)
        wh = width * height
        cfg = _abi.SolLightmapFilterVarConfig(size=C.sizeof(_abi.SolLightmapFilterVarConfig), width=width, height=height, iterations=int(iterations),
                                              normal_power_log2=int(normal_power_log2), sigma_position=float(sigma_position),
                                              sigma_plane=float(sigma_position if sigma_plane is None else sigma_plane), sigma_value=float(sigma_value),
                                              variance_floor=float(variance_floor))
        out = self._call("sol_lightmap_filter_var", [_Arg("moments", moments, "moments", (wh,)), _Arg("points", points, "f32", (wh, 8)),
                                                     _Arg("texels", texels, "texel", (wh,))],
                         [_Out("out", "f32", (wh, 4))] + ([_Out("variance", "f32", (wh, 4))] if return_variance else []),
                         lambda p, d: (C.byref(cfg), p["points"], p["texels"], p["moments"], p["out"], p.get("variance")))
        return (out["out"], out["variance"]) if return_variance else out["out"]

    # ---- adaptive irradiance gathers (EXTENSION) ----
    def irradiance_adaptive(self, points, max_samples, round=16, min_samples=32, threshold=0.05, floor=0.0, first_sample=0, seed=0, keys=None, key_base=0,
                            first_draw=0, mode="cosine", return_stats=False):
        """sol_irradiance_adaptive: irradiance_moments() in rounds of `round` samples (a positive multiple of 16) over the points still active. After
        every round a point stops when it holds max_samples, when one of its sums is not finite, or - from min_samples (a multiple of 16) on - when
        in every channel the variance of its mean (moments_mean_variance) is at most (threshold * max(mean, floor))^2: `threshold` is a relative
        standard error, `floor` keeps it from being relative to nothing in the dark, threshold = 0 never converges. A row that ends with N samples
        is, in all eight words, irradiance_moments(samples=N)'s row for the same point and key: the counts differ from row to row, nothing else does
        - lightmap_filter_var reads each row's own count, and radiance_rescale brings its output to one count for lightmap_dilate. Returns what
        irradiance_moments returns on either route (a MOMENTS_DTYPE array for host arrays, the raw [n, 8] float32 device tensor for device
        tensors); with return_stats=True also a dict of rounds, paths (the sum of the final counts), rows_valid, rows_converged and rows_capped.
        Both routes block: the library reads the active count back after every round. The defaults (round 16, min_samples 32, threshold 0.05,
        floor 0) are not tuned on a device. points, keys, key_base, first_draw and the modes are irradiance()'s."""
        cfg = self._irradiance_config(max_samples, first_sample, seed, key_base, first_draw, mode)
        ad = _abi.SolGatherAdaptive(size=C.sizeof(_abi.SolGatherAdaptive), round=int(round), min_samples=int(min_samples), threshold=float(threshold),
                                    floor=float(floor))
        stats = _abi.SolGatherAdaptiveStats(size=C.sizeof(_abi.SolGatherAdaptiveStats))
        rows = self._radiance("sol_irradiance_adaptive", "points", points, keys, cfg, words=8,
                              call=lambda p, k, n, c, out: (p, k, n, c, C.byref(ad), out, C.byref(stats)))
        if isinstance(rows, np.ndarray):
            rows = rows.view(MOMENTS_DTYPE).reshape(-1)
        if not return_stats:
            return rows
        return rows, {"rounds": int(stats.rounds), "paths": int(stats.paths), "rows_valid": int(stats.rows_valid), "rows_converged": int(stats.rows_converged),
                      "rows_capped": int(stats.rows_capped)}

    def radiance_rescale(self, rows, target_samples, in_place=False):
        """sol_radiance_rescale: [n, 4] float32 rows of sums (r, g, b and the bits of the sample count: what irradiance(), lightmap_filter() and
        lightmap_filter_var() return) brought to one count - a row with count c >= 1 becomes float32(float64(word) * target_samples / c) per
        channel with the count target_samples, a row with count 0 is copied. After an adaptive gather the filter's rows carry different counts, and
        lightmap_dilate averages sums: this goes between them. Host arrays go the host route and return an array, device tensors the device route
        and return a new tensor - or, in_place=True, `rows` itself, overwritten (a contiguous float32 array or tensor)."""
        if in_place and not self._on_device(rows) and np.ascontiguousarray(rows, dtype=np.float32) is not rows:
            raise ValueError("rows: in_place needs the contiguous float32 array itself")
        out = self._call("sol_radiance_rescale", [_Arg("rows", rows, "f32", ("n", 4))], [] if in_place else [_Out("out", "f32", ("n", 4))],
                         lambda p, d: (p["rows"], d["n"], int(target_samples), p.get("out", p["rows"])))
        return rows if in_place else out["out"]

    # ---- lightmap lookups (EXTENSION) ----
    def lightmap_coords(self, hits, triangle_of_dfs):
        """sol_lightmap_coords: closest_hits' rows turned into surface rows (triangle, b1, b2, flags) through `triangle_of_dfs`, the uint32 table
        lightmap_triangle_table makes (per dfs_index the lightmap triangle and its record's rotation, or SOL_TEXEL_NONE). A RAY_HIT_DTYPE array
        goes the host route and returns a LIGHTMAP_TEXEL_DTYPE array; the [n, 8] int32 device tensor closest_hits returned goes through
        sol_lightmap_coords_dev and returns an [n, 4] int32 device tensor (lightmap_texels_to_numpy views it). A miss, a sphere, a quad, and a
        triangle the table does not list answer (SOL_TEXEL_NONE, 0, 0, 0)."""
        table = _Arg("triangle_of_dfs", triangle_of_dfs, "u32", ("entries",), null_if_empty=True, flat=True, upload="any")  # (a host table is copied over)
        return self._call("sol_lightmap_coords", [_Arg("hits", hits, "hit", ("n",)), table], [_Out("out", "texel", ("n",))],
                          lambda p, d: (p["hits"], d["n"], p["triangle_of_dfs"], d["entries"], p["out"]))["out"]

    def lightmap_sample(self, values, coords, uvs, texels, width, height, channels=3, pass_of=None, nearest=False, chart_radius=None, vertices=None, points=None):
        """sol_lightmap_sample: the baked atlas `values` (`width * height` rows whose leading `channels` 32-bit words are floats: what
        lightmap_dilate returned) looked up at the surface rows `coords` (what lightmap_coords or lightmap_points returned). uvs [n, 3, 2] and
        texels are lightmap_points' arguments and answer; pass_of: lightmap_dilate's plane (a tap is covered when it is not 255), None: a tap is
        covered when a triangle owns it. The lookup is bilinear over the covered, finite taps, renormalised; nearest=True takes the one texel
        the point falls into. chart_radius (a world length) with vertices [n, 3, 3] and points (lightmap_points' rows) switches the chart guard
        on: an owned tap farther than that from the shaded point is left out. Returns [n, channels + 1] float32 rows - the channels, then the
        bits of the number of taps that contributed (0: nothing was found, the row is zero). Host arrays go the host route, device tensors the
        device route, decided by `values`."""
        width, height, channels = int(width), int(height), int(channels)
        cfg = _abi.SolLightmapSampleConfig(size=C.sizeof(_abi.SolLightmapSampleConfig), width=width, height=height, channels=channels,
                                           stride_bytes=self._stride(values), flags=_abi.SOL_LIGHTMAP_SAMPLE_NEAREST if nearest else 0,
                                           chart_radius=float("inf") if chart_radius is None else float(chart_radius))
        out_words = channels + 1 if 1 <= channels <= 32 else 1
        args = self._atlas_args(uvs, texels, pass_of, values, width, height) + self._guard_args(vertices, points, coords, width * height)
        return self._call("sol_lightmap_sample", args, [_Out("out", "f32", ("n", out_words))],
                          lambda p, d: (C.byref(cfg), p["uvs"], d["n_triangles"], p["texels"], p["pass_of"], p["values"], p["vertices"], p["points"], p["coords"],
                                        d["n"], p["out"]), device=self._on_device(values))["out"]

    def lightmap_view(self, values, uvs, texels, width, height, triangle_of_dfs, x0, y0, x1, y1, sample=0, seed=0, **sample_args):
        """The bake seen from the scene's camera: camera_rays -> closest_hits -> lightmap_coords -> lightmap_sample over the pixels [x0, x1) x
        [y0, y1), all on device memory (values, uvs, texels and what sample_args names are device tensors). Returns an [h, w, channels + 1]
        float32 device tensor; a pixel that misses, or hits something without lightmap, is zero with count 0."""
        _, _, coords, h, w = self._view_coords(triangle_of_dfs, x0, y0, x1, y1, sample, seed)
        return self.lightmap_sample(values, coords, uvs, texels, width, height, **sample_args).reshape(h, w, -1)

    def _view_coords(self, triangle_of_dfs, x0, y0, x1, y1, sample, seed):
        """The first steps of every view, camera_rays -> closest_hits -> lightmap_coords over the pixels [x0, x1) x [y0, y1): (rays [h * w, 8], hits,
        coords, h, w), device tensors."""
        rays = self.camera_rays(x0, y0, x1, y1, sample, seed)
        h, w = int(rays.shape[0]), int(rays.shape[1])
        rays = rays.reshape(-1, 8)
        hits = self.closest_hits(rays)
        return rays, hits, self.lightmap_coords(hits, triangle_of_dfs), h, w

    # ---- directional lightmaps (EXTENSION) ----
    @staticmethod
    def _atlas_args(uvs, texels, pass_of, values, width, height):
        """What every lookup takes of the atlas: the lightmap UVs (they bind n_triangles), lightmap_points' texels, lightmap_dilate's plane or None, and
        the atlas itself (it binds k, the words of a row)."""
        return [_Arg("uvs", uvs, "f32", ("n_triangles", 3, 2), null_if_empty=True), _Arg("texels", texels, "texel", (width * height,)),
                _Arg("pass_of", pass_of, "u8", (height, width), optional=True, flat=True), _Arg("values", values, "f32", (width * height, "k"))]

    @staticmethod
    def _guard_args(vertices, points, coords, wh):
        """The chart guard's two optional arrays and the surface rows (they bind n) of a lookup."""
        return [_Arg("vertices", vertices, "f32", ("n_triangles", 3, 3), optional=True), _Arg("points", points, "f32", (wh, 8), optional=True),
                _Arg("coords", coords, "texel", ("n",))]

    def lightmap_sh(self, values, coords, normals, uvs, texels, width, height, scale=1.0, pass_of=None, nearest=False, chart_radius=None, vertices=None,
                    points=None, clamp=False, coefficients=False):
        """sol_lightmap_sh: the baked atlas `values` of SolSh9 rows (`width * height` rows of 28 words or more, a multiple of 4: what
        irradiance_sh, lightmap_filter and lightmap_dilate(channels=27) returned) looked up at the surface rows `coords` exactly as
        lightmap_sample(channels=27) does, and evaluated as irradiance at `normals` [n, 4] (x, y, z, unused; taken as they come, not normalised):
        E = scale * sum_k A_k Y_k(n) L_k per channel, with clamp=True no less than 0. scale: 4 pi / samples for an irradiance_sh(mode="sphere")
        bake. Returns [n, 4] float32 rows (E_r, E_g, E_b, the bits of the number of live taps); a row without a live tap or with a normal that is
        not finite, zero or subnormal in length is zero. coefficients=True: no normals (None), no scale - the [n, 28] rows lightmap_sample
        (channels=27) answers, from the eight-lanes-to-a-row kernel. Host arrays go the host route, device tensors the device route, decided by
        `values`."""
        width, height = int(width), int(height)
        flags = ((_abi.SOL_LIGHTMAP_SH_NEAREST if nearest else 0) | (_abi.SOL_LIGHTMAP_SH_COEFFICIENTS if coefficients else 0)
                 | (_abi.SOL_LIGHTMAP_SH_CLAMP if clamp else 0))
        cfg = _abi.SolLightmapShConfig(size=C.sizeof(_abi.SolLightmapShConfig), width=width, height=height, stride_bytes=self._stride(values), flags=flags,
                                       chart_radius=float("inf") if chart_radius is None else float(chart_radius), scale=float(scale))
        args = (self._atlas_args(uvs, texels, pass_of, values, width, height) + self._guard_args(vertices, points, coords, width * height)
                + [_Arg("normals", normals, "f32", ("n", 4), optional=True)])
        return self._call("sol_lightmap_sh", args, [_Out("out", "f32", ("n", 28 if coefficients else 4))],
                          lambda p, d: (C.byref(cfg), p["uvs"], d["n_triangles"], p["texels"], p["pass_of"], p["values"], p["vertices"], p["points"], p["coords"],
                                        p["normals"], d["n"], p["out"]), device=self._on_device(values))["out"]

    def lightmap_normals(self, coords, vertices, normals=None):
        """sol_lightmap_normals: the unit normals of the surface rows `coords` by lightmap_points' rule - the triangle's geometric normal, or with
        per-vertex `normals` [n_triangles, 3, 3] their interpolation where it has a length - as [n, 4] float32 rows (nx, ny, nz, 0): what
        lightmap_sh takes. An invalid row, a triangle with a word that is not finite and a vector without length answer zeros. A
        LIGHTMAP_TEXEL_DTYPE array goes the host route, an [n, 4] int32 device tensor the device route."""
        return self._call("sol_lightmap_normals", [_Arg("coords", coords, "texel", ("n",)), _Arg("vertices", vertices, "f32", ("n_triangles", 3, 3), null_if_empty=True),
                                                   _Arg("normals", normals, "f32", ("n_triangles", 3, 3), optional=True, null_if_empty=True)],
                          [_Out("out", "f32", ("n", 4))],
                          lambda p, d: (p["coords"], d["n"], p["vertices"], p["normals"], d["n_triangles"], p["out"]))["out"]

    def lightmap_view_sh(self, values, uvs, texels, width, height, triangle_of_dfs, vertices, x0, y0, x1, y1, scale, sample=0, seed=0, vertex_normals=None,
                         perturb=None, **sh_args):
        """A directional bake seen from the scene's camera: camera_rays -> closest_hits -> lightmap_coords -> lightmap_normals -> lightmap_sh over
        the pixels [x0, x1) x [y0, y1), all on device memory. vertices [n_triangles, 3, 3] (and vertex_normals) give the surface's normals;
        `perturb`, an [h, w, 4] float32 device tensor of the caller's own normals, replaces them - the normal-mapped case. Returns an [h, w, 4]
        float32 device tensor (E_r, E_g, E_b, count), or [h, w, 28] with coefficients=True; a pixel that misses, or hits something without
        lightmap, is zero with count 0."""
        _, _, coords, h, w = self._view_coords(triangle_of_dfs, x0, y0, x1, y1, sample, seed)
        if sh_args.get("coefficients"):
            normals = None
        elif perturb is not None:
            if tuple(perturb.shape) != (h, w, 4):
                raise ValueError(f"perturb: an [{h}, {w}, 4] float32 device tensor")
            normals = perturb.reshape(-1, 4)
        else:
            normals = self.lightmap_normals(coords, vertices, vertex_normals)
        out = self.lightmap_sh(values, coords, normals, uvs, texels, width, height, scale=scale, **sh_args)
        return out.reshape(h, w, -1)

    # ---- lightmap mip chains (EXTENSION) ----
    def lightmap_mips(self, values, texels, width, height, channels=3, pass_of=None, levels=None):
        """sol_lightmap_mips: the mip chain of the baked atlas `values` (`width * height` rows whose leading `channels` 32-bit words are floats).
        A texel of a coarser level is the mean of the live ones among its four sources - covered (pass_of != 255 where lightmap_dilate's plane is
        given, else owned in `texels`) and finite -, so nothing uncovered bleeds in. Returns (mips, cover): the rows of levels 1 .. levels - 1
        packed as lightmap_mip_layout says, with the stride of `values`, and one byte per row, 0 covered, 255 not - a level's slice of both can be
        handed to lightmap_sample as (values, pass_of). levels: level 0 counted, None: all. Host arrays go the host route, device tensors the
        device route, decided by `values`."""
        width, height, channels = int(width), int(height), int(channels)
        lay = lightmap_mip_layout(width, height, levels)
        wh, rows = width * height, lay["rows"]
        out = self._call("sol_lightmap_mips", [_Arg("values", values, "f32", (wh, "k")), _Arg("texels", texels, "texel", (wh,)),
                                               _Arg("pass_of", pass_of, "u8", (height, width), optional=True, flat=True)],
                         [_Out("mips", "f32", (rows, "k"), null_if_empty=True), _Out("cover", "u8", (rows,), null_if_empty=True)],
                         lambda p, d: (p["texels"], p["pass_of"], width, height, p["values"], channels, d["k"] * 4, lay["levels"], p["mips"], p["cover"]))
        return out["mips"], out["cover"]

    def lightmap_sample_lod(self, values, mips, cover, lods, coords, uvs, texels, width, height, channels=3, pass_of=None, levels=None, chart_radius=None,
                            vertices=None, points=None):
        """sol_lightmap_sample_lod: lightmap_sample's bilinear lookup made trilinear over the chain lightmap_mips returned. lods: one float per row
        of `coords` - at most 0 (or NaN): level 0 alone, the answer of lightmap_sample word for word; at least levels - 1: the last level alone;
        between two levels both are looked up and mixed by the fraction, and a level without a live tap leaves the answer to the other. The chart
        guard (chart_radius, vertices, points) acts at level 0 only. Returns [n, channels + 1] float32 rows - the channels, then the bits of the
        number of taps that contributed over both levels (0 .. 8). Host arrays go the host route, device tensors the device route, decided by
        `values`."""
        width, height, channels = int(width), int(height), int(channels)
        lay = lightmap_mip_layout(width, height, levels)
        cfg = _abi.SolLightmapLodConfig(size=C.sizeof(_abi.SolLightmapLodConfig), width=width, height=height, channels=channels, stride_bytes=self._stride(values),
                                        flags=0, chart_radius=float("inf") if chart_radius is None else float(chart_radius), levels=lay["levels"])
        out_words = channels + 1 if 1 <= channels <= 32 else 1
        rows = lay["rows"]  # (a chain of level 0 alone has no rows: mips and cover are not looked at and go as null pointers)
        args = (self._atlas_args(uvs, texels, pass_of, values, width, height)
                + [_Arg("mips", mips if rows else None, "f32", (rows, "k"), optional=not rows), _Arg("cover", cover if rows else None, "u8", (rows,), optional=not rows)]
                + self._guard_args(vertices, points, coords, width * height) + [_Arg("lods", lods, "f32", ("n",))])
        return self._call("sol_lightmap_sample_lod", args, [_Out("out", "f32", ("n", out_words))],
                          lambda p, d: (C.byref(cfg), p["uvs"], d["n_triangles"], p["texels"], p["pass_of"], p["values"], p["mips"], p["cover"], p["vertices"],
                                        p["points"], p["coords"], p["lods"], d["n"], p["out"]), device=self._on_device(values))["out"]

    def lightmap_lod(self, rays, hits, coords, vertices, uvs, width, height, spread, bias=0.0):
        """sol_lightmap_lod: the level of detail of each hit - half the piecewise-linear log2 of the squared number of texels under a pixel along
        its footprint's major axis, plus `bias`, no less than 0. rays [n, 8], hits (closest_hits' rows) and coords (lightmap_coords' rows) belong
        together row by row; vertices [n_triangles, 3, 3] and uvs [n_triangles, 3, 2] are the lightmap mesh; spread: the angle in radians between
        the rays of neighbouring pixels (pixel_spread). A miss, an invalid row and a degenerate triangle answer 0. Returns [n] float32: what
        lightmap_sample_lod takes. Host arrays go the host route, device tensors the device route, decided by `rays`."""
        args = [_Arg("rays", rays, "f32", ("n", 8)), _Arg("hits", hits, "hit", ("n",)), _Arg("coords", coords, "texel", ("n",)),
                _Arg("vertices", vertices, "f32", ("n_triangles", 3, 3), null_if_empty=True), _Arg("uvs", uvs, "f32", ("n_triangles", 3, 2), null_if_empty=True)]
        return self._call("sol_lightmap_lod", args, [_Out("out", "f32", ("n",))],
                          lambda p, d: (p["rays"], p["hits"], p["coords"], d["n"], p["vertices"], p["uvs"], d["n_triangles"], int(width), int(height), float(spread),
                                        float(bias), p["out"]))["out"]

    def lightmap_view_lod(self, values, mips, cover, uvs, texels, width, height, triangle_of_dfs, vertices, x0, y0, x1, y1, spread, bias=0.0, sample=0, seed=0,
                          **sample_args):
        """The bake seen from the scene's camera without aliasing: camera_rays -> closest_hits -> lightmap_coords -> lightmap_lod ->
        lightmap_sample_lod over the pixels [x0, x1) x [y0, y1), all on device memory. spread: pixel_spread of the camera; sample_args: what
        lightmap_sample_lod takes by name (channels, pass_of, levels, chart_radius, points; `vertices` serves the guard too). Returns an
        [h, w, channels + 1] float32 device tensor; a pixel that misses, or hits something without lightmap, is zero with count 0."""
        rays, hits, coords, h, w = self._view_coords(triangle_of_dfs, x0, y0, x1, y1, sample, seed)
        lods = self.lightmap_lod(rays, hits, coords, vertices, uvs, width, height, spread, bias)
        if sample_args.get("points") is not None:
            sample_args = {**sample_args, "vertices": vertices}
        out = self.lightmap_sample_lod(values, mips, cover, lods, coords, uvs, texels, width, height, **sample_args)
        return out.reshape(h, w, -1)

    # ---- lightmap charts (EXTENSION) ----
    def lightmap_charts(self, uvs, vertices=None):
        """sol_lightmap_charts: the UV islands of a mesh. uvs [n, 3, 2] float32 and, optionally, vertices [n, 3, 3]: two triangles are connected
        when they have an edge in common - the unordered pair of its end points, (u, v) or with vertices (u, v, x, y, z), equal as numbers. Returns
        (chart_of_triangle [n] - dense ids in mesh order, CHART_NONE for a triangle with a word that is not finite -, n_charts). Host arrays go
        the host route and return a uint32 array; device tensors the device route and return an int32 tensor holding the same words."""
        out = self._call("sol_lightmap_charts", [_Arg("uvs", uvs, "f32", ("n", 3, 2), null_if_empty=True),
                                                 _Arg("vertices", vertices, "f32", ("n", 3, 3), optional=True, null_if_empty=True)],
                         [_Out("chart_of", "u32", ("n",), null_if_empty=True), _Out("n_charts", "u32", (1,), zero=True)],
                         lambda p, d: (p["uvs"], p["vertices"], d["n"], p["chart_of"], p["n_charts"]))
        return out["chart_of"], int(out["n_charts"][0])

    def lightmap_dilate_charts(self, values, texels, chart_of_triangle, width, height, passes=1, channels=3):
        """sol_lightmap_dilate_charts: lightmap_dilate that never averages across charts. chart_of_triangle: what lightmap_charts returned. A
        texel is owned when its triangle has a chart; a texel filled in a pass joins the chart most of its covered neighbours hold (the lowest
        id on a tie) and takes the mean of the neighbours of that chart only. Returns (out, pass_of [height, width] uint8, chart_plane
        [height, width] - the chart of every texel, CHART_NONE where nothing reached). Host arrays go the host route, device tensors the device
        route, decided by `values`."""
        width, height = int(width), int(height)
        wh = width * height
        out = self._call("sol_lightmap_dilate_charts", [_Arg("values", values, "f32", (wh, "k")), _Arg("texels", texels, "texel", (wh,)),
                                                        _Arg("chart_of_triangle", chart_of_triangle, "words", ("n_triangles",), optional=True, null_if_empty=True,
                                                             flat=True)],
                         [_Out("out", "f32", (wh, "k")), _Out("pass_of", "u8", (height, width)), _Out("chart_plane", "words", (height, width))],
                         lambda p, d: (p["texels"], width, height, p["values"], int(channels), d["k"] * 4, int(passes), p["chart_of_triangle"],
                                       d.get("n_triangles", 0), p["out"], p["pass_of"], p["chart_plane"]))
        return out["out"], out["pass_of"], out["chart_plane"]

    def lightmap_sample_charts(self, values, coords, uvs, texels, chart_of_triangle, chart_plane, width, height, channels=3, pass_of=None, nearest=False):
        """sol_lightmap_sample_charts: lightmap_sample guarded by chart id. chart_of_triangle: what lightmap_charts returned; chart_plane (and
        pass_of): what lightmap_dilate_charts returned. A tap contributes when it is inside, covered and finite and its plane word is the chart of
        the row's triangle - a dilated tap of a neighbouring chart included; a row whose triangle has no chart answers zeros. Returns
        [n, channels + 1] float32 rows as lightmap_sample does. Host arrays go the host route, device tensors the device route, decided by `values`."""
        width, height, channels = int(width), int(height), int(channels)
        cfg = _abi.SolLightmapSampleConfig(size=C.sizeof(_abi.SolLightmapSampleConfig), width=width, height=height, channels=channels,
                                           stride_bytes=self._stride(values), flags=_abi.SOL_LIGHTMAP_SAMPLE_NEAREST if nearest else 0, chart_radius=float("inf"))
        out_words = channels + 1 if 1 <= channels <= 32 else 1
        args = (self._atlas_args(uvs, texels, pass_of, values, width, height)
                + [_Arg("chart_of_triangle", chart_of_triangle, "words", ("n_triangles",), null_if_empty=True, flat=True),
                   _Arg("chart_plane", chart_plane, "words", (height, width), flat=True), _Arg("coords", coords, "texel", ("n",))])
        return self._call("sol_lightmap_sample_charts", args, [_Out("out", "f32", ("n", out_words))],
                          lambda p, d: (C.byref(cfg), p["uvs"], d["n_triangles"], p["texels"], p["pass_of"], p["values"], p["chart_of_triangle"], p["chart_plane"],
                                        p["coords"], d["n"], p["out"]), device=self._on_device(values))["out"]

    def lightmap_chart_levels(self, chart_plane, width, height, pass_of=None):
        """sol_lightmap_chart_levels: how many mip levels the atlas can have before two charts meet in one level - the `levels` to hand to
        lightmap_mips. chart_plane [height, width]: what lightmap_dilate_charts returned; pass_of: its plane, or None (every texel with a chart
        counts). Returns (levels, mixed_texels [15], mixed_windows [15]): per level l >= 1 the texels that hold two charts and the 2 x 2 windows -
        a bilinear footprint - that do. A host array goes the host route, a device tensor the device route."""
        width, height, levels = int(width), int(height), _abi.SOL_LIGHTMAP_MAX_LEVELS
        words = self._call("sol_lightmap_chart_levels", [_Arg("chart_plane", chart_plane, "words", (height, width), flat=True),
                                                         _Arg("pass_of", pass_of, "u8", (height, width), optional=True, flat=True)],
                           [_Out("answer", "u32", (1 + 2 * levels,), zero=True)],  # (the count, then the two rows of counts per level)
                           lambda p, d: (p["chart_plane"], p["pass_of"], width, height, p["answer"], p["answer"] + 4, p["answer"] + 4 + 4 * levels))["answer"]
        words = words if isinstance(words, np.ndarray) else words.cpu().numpy().view(np.uint32)
        return int(words[0]), words[1:1 + levels].copy(), words[1 + levels:].copy()

    def lightmap_view_charts(self, values, uvs, texels, chart_of_triangle, chart_plane, width, height, triangle_of_dfs, x0, y0, x1, y1, sample=0, seed=0,
                             **sample_args):
        """The bake seen from the scene's camera with the charts kept apart: camera_rays -> closest_hits -> lightmap_coords ->
        lightmap_sample_charts over the pixels [x0, x1) x [y0, y1), all on device memory. sample_args: what lightmap_sample_charts takes by name
        (channels, pass_of, nearest). Returns an [h, w, channels + 1] float32 device tensor."""
        _, _, coords, h, w = self._view_coords(triangle_of_dfs, x0, y0, x1, y1, sample, seed)
        out = self.lightmap_sample_charts(values, coords, uvs, texels, chart_of_triangle, chart_plane, width, height, **sample_args)
        return out.reshape(h, w, -1)

    # ---- irradiance volumes (EXTENSION) ----
    @staticmethod
    def _volume_rows(grid):
        """The rows to allocate for `grid`; 1 for a grid the library refuses."""
        return grid.n_probes if all(c > 0 for c in grid.counts) and grid.n_probes <= _abi.SOL_VOLUME_MAX_PROBES else 1

    def volume_points(self, grid, tmin=1e-3, tmax=float("inf"), host=False):
        """sol_volume_points: the rows (position, tmin, (0, 0, 1), tmax) of the probes of `grid` (a VolumeGrid), probe (i, j, k) in row (k * ny + j) *
        nx + i - what irradiance_sh(mode="sphere") and visibility(distances=True) take, with every position on the bits the one volume_sample
        measures from. Returns an [nx * ny * nz, 8] float32 tensor on the scene's device (sol_volume_points_dev), with host=True a numpy array
        (the host route)."""
        rec = grid.record()
        return self._call("sol_volume_points", [], [_Out("out", "f32", (self._volume_rows(grid), 8))],
                          lambda p, d: (C.byref(rec), float(tmin), float(tmax), p["out"]), device=not host)["out"]

    def volume_build(self, grid, sh, visibility=None, radius=None):
        """sol_volume_build: one SolProbe per probe of `grid` from what irradiance_sh(volume_points(grid), mode="sphere") answered - the sums must be
        SPHERE mode's - and, for the hit-distance moments, what visibility(.., distances=True) answered over points whose tmax is the finite
        `radius`. Without visibility, or with radius None, the probes carry no moments and the Chebyshev weight of volume_sample leaves them
        alone. A probe without samples or with a sum that is not finite is invalid (32 zero words) and is skipped by volume_sample. Host route:
        sh as irradiance_sh returned it - the pair (sums [n, 9, 3], counts [n]) - or raw [n, 28] float32 rows, visibility a VISIBILITY_DTYPE array
        or raw [n, 8] rows; returns a VOLUME_PROBE_DTYPE array. Device route: the [n, 28] and [n, 8] float32 tensors of the gathers, without a
        copy; returns the raw [n, 32] float32 device tensor (volume_probes_to_numpy views it)."""
        rec, rows = grid.record(), self._volume_rows(grid)
        if isinstance(sh, (tuple, list)):  # (irradiance_sh's pair: the raw rows again)
            sums, counts = sh
            sh = np.concatenate([np.ascontiguousarray(sums, dtype=np.float32).reshape(-1, 27),
                                 np.ascontiguousarray(counts).astype(np.uint32, copy=False).view(np.float32).reshape(-1, 1)], axis=1)
        return self._call("sol_volume_build", [_Arg("sh", sh, "f32", (rows, 28), aligned=True),
                                               _Arg("visibility", visibility, "visibility", (rows,), optional=True, aligned=True)],
                          [_Out("out", "probe", (rows,))],
                          lambda p, d: (C.byref(rec), p["sh"], p["visibility"], 0.0 if radius is None else float(radius), p["out"]))["out"]

    def volume_sample(self, grid, probes, points, depth=None, res=8):
        """sol_volume_sample: the irradiance at the caller's points - rows of (position xyz, tmin, normal xyz, tmax), irradiance()'s rows; tmin and
        tmax are not read - interpolated from the probes of `grid` that volume_build packed: trilinear weights over the cell of position + unit
        normal * normal_bias, times the backface and Chebyshev weights the grid's flags ask for, invalid probes left out. Host arrays (probes: a
        VOLUME_PROBE_DTYPE array or raw [n, 32] float32 rows) go the host route and return (rgb [n, 3] float32, samples [n] uint32), samples being
        the probes that contributed, 0 to 8; device tensors go through sol_volume_sample_dev without a copy and return the raw [n, 4] float32
        rows, which lightmap_dilate takes as they are. depth (sol_volume_sample_depth): the probes' res x res depth maps as
        volume_build_depth returned them (a DEPTH_TEXEL_DTYPE array, raw [n_probes, res * res, 2] float32 rows, or that device tensor) - the
        Chebyshev weight then reads mean and mean2 from a probe's map in the direction of the point instead of the probe's two isotropic words."""
        rec, rows = grid.record(), self._volume_rows(grid)
        args = [_Arg("points", points, "f32", ("n", 8), aligned=True), _Arg("probes", probes, "probe", (rows,), aligned=True)]
        if depth is None:
            out = self._call("sol_volume_sample", args, [_Out("out", "f32", ("n", 4))], lambda p, d: (C.byref(rec), p["probes"], p["points"], d["n"], p["out"]))
        else:
            oct_cfg = self._oct_config(res)
            args.append(_Arg("depth", depth, "depth", (rows, self._oct_texels(res)), aligned=True))
            out = self._call("sol_volume_sample_depth", args, [_Out("out", "f32", ("n", 4))],
                             lambda p, d: (C.byref(rec), p["probes"], p["depth"], C.byref(oct_cfg), p["points"], d["n"], p["out"]))
        return self._split(out["out"])

    # ---- directional distance moments: octahedral maps (EXTENSION) ----
    @staticmethod
    def _oct_config(res, sharpness_log2=0):
        return _abi.SolOctConfig(size=C.sizeof(_abi.SolOctConfig), res=int(res) & 0xFFFFFFFF, sharpness_log2=int(sharpness_log2) & 0xFFFFFFFF, reserved=0)

    @staticmethod
    def _oct_texels(res):
        """The texels per map to allocate for `res`; 1 for a res the library refuses."""
        return int(res) * int(res) if res in (4, 8, 16) else 1

    def visibility_oct(self, points, res=8, sharpness_log2=5, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="sphere"):
        """sol_visibility_oct: visibility(distances=True)'s samples at the caller's points, gathered per direction into a res x res octahedral map
        (res 4, 8 or 16): every texel sums the lobe weight c = max(dot(texel direction, sample direction), 0) ^ (2 ^ sharpness_log2) of all
        samples (w), of the misses (w_open), and c * t and c * t * t of the hits (wt, wt2) - what volume_build_depth turns into a probe's
        depth map. Returns [n, res * res, 4] float32: a numpy array on the host route (OCT_TEXEL_DTYPE views it), a device tensor on the device
        route. points, keys, key_base, first_draw and the waits of the two routes are irradiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        oct_cfg, texels = self._oct_config(res, sharpness_log2), self._oct_texels(res)
        rows = self._radiance("sol_visibility_oct", "points", points, keys, cfg, words=4 * texels,
                              call=lambda p, k, n, c, out: (p, k, n, c, C.byref(oct_cfg), out))
        return rows.reshape(-1, texels, 4)

    def volume_build_depth(self, grid, oct, radius, res=8, sharpness_log2=5):
        """sol_volume_build_depth: the probes' depth maps from what visibility_oct(volume_points(grid, tmax=radius), res, ..) answered: per texel
        the mean and the mean square of the hit distance clamped to `radius` - (radius, radius^2) where the texel saw nothing. Returns
        [n_probes, res * res, 2] float32, a numpy array for a host array (DEPTH_TEXEL_DTYPE views it) and a device tensor for a device tensor."""
        rec, rows = grid.record(), self._volume_rows(grid)
        oct_cfg, texels = self._oct_config(res, sharpness_log2), self._oct_texels(res)
        return self._call("sol_volume_build_depth", [_Arg("oct", oct, "oct", (rows, texels), aligned=True)], [_Out("out", "f32", (rows, texels, 2))],
                          lambda p, d: (C.byref(rec), p["oct"], C.byref(oct_cfg), float(radius), p["out"]))["out"]

    def camera_ray_keys(self, x0, y0, x1, y1, sample, seed):
        """sol_camera_ray_keys: (pixel, first_draw) of the camera rays of pixels [x0, x1) x [y0, y1) for (sample, seed) as an [h, w, 2] int32 device
        tensor: with them, radiance() over camera_rays() of the same arguments is the render's own sample."""
        import torch
        h, w = max(int(y1) - int(y0), 0), max(int(x1) - int(x0), 0)
        out = torch.empty((h, w, 2), dtype=torch.int32, device=f"cuda:{self.device}")
        self._chk(self.lib.sol_camera_ray_keys(self.h, x0, y0, x1, y1, sample, seed, C.c_void_p(out.data_ptr())))
        self.sync()  # (the scene's stream is not torch's)
        return out

    # ---- a new camera for a live scene (EXTENSION) ----
    def set_camera(self, camera, background_proof=True, reprobe=False):
        """sol_scene_set_camera: the same scene from another viewpoint, without building anything again. `camera`: a CameraConfig (cast by
        host.camera_record for this frame size) or a SolCamera. background_proof=False: do not look for background blocks for the new camera;
        reprobe=True: run creation's cost probe again. Clears the accumulator and the auxiliary planes, ends an adaptive session; blocks."""
        if not isinstance(camera, _abi.SolCamera):
            from .host import camera_record
            camera = camera_record(self.width, self.height, camera)
        upd = _abi.SolCameraUpdate(size=C.sizeof(_abi.SolCameraUpdate),
                                   flags=(0 if background_proof else _abi.SOL_CAMERA_NO_BACKGROUND_PROOF) | (_abi.SOL_CAMERA_REPROBE if reprobe else 0))
        self._chk(self.lib.sol_scene_set_camera(self.h, C.byref(camera), C.byref(upd)))

    def background_flags(self):
        """sol_scene_background_flags: the background blocks in force, a bool array [blocks_y, blocks_x] (as background_blocks() returns)."""
        bx, by = (self.width + 7) // 8, (self.height + 7) // 8
        flags = np.zeros((by, bx), dtype=np.uint8)
        n = C.c_uint32()
        self._chk(self.lib.sol_scene_background_flags(self.h, flags.ctypes.data, flags.size, C.byref(n)))
        assert int(flags.sum()) == n.value
        return flags.astype(bool)

    # ---- new vertices for the triangles of a live scene (EXTENSION) ----
    def set_triangles(self, vertices, background_proof=True, reprobe=False):
        """sol_scene_set_triangles: row i of `vertices` (float64 [n, 3, 3]: v0, v1, v2) moves triangle i of the creation description; the scene
        must have been created with dynamic_triangles=True. A numpy array goes the host route; a contiguous float64 torch tensor on the scene's
        device goes through sol_scene_set_triangles_dev without a copy. Clears the sums and the auxiliary planes, ends an adaptive session; blocks."""
        upd = _abi.SolGeometryUpdate(size=C.sizeof(_abi.SolGeometryUpdate),
                                     flags=(0 if background_proof else _abi.SOL_GEOM_NO_BACKGROUND_PROOF) | (_abi.SOL_GEOM_REPROBE if reprobe else 0))
        self._call("sol_scene_set_triangles", [_Arg("vertices", vertices, "f64", ("n", 3, 3))], [], lambda p, d: (p["vertices"], d["n"], C.byref(upd)),
                   sync=False)  # (the move blocks by itself)

    def set_triangles_ms(self):
        """sol_scene_set_triangles_ms: device-event ms of the last timed move: upload, records, refit, rest."""
        out = (C.c_float * 4)()
        self._chk(self.lib.sol_scene_set_triangles_ms(self.h, out))
        return dict(zip(("upload", "records", "refit", "rest"), [float(x) for x in out]))

    TRI_DTYPE = np.dtype([("v0", np.float32, 3), ("e1", np.float32, 3), ("e2", np.float32, 3), ("dfs", np.uint32), ("mat", np.int32), ("area", np.float32)])
    TRI_SHADE_DTYPE = np.dtype([("n", np.float32, 3), ("mat", np.int32), ("t", np.float32, 3), ("u0", np.float32), ("b", np.float32, 3), ("v0", np.float32),
                                ("u1", np.float32), ("v1", np.float32), ("u2", np.float32), ("v2", np.float32)])

    def triangle_records(self):
        """sol_scene_triangle_records: (intersect records, shading records, caller triangle of each record) as the device holds them."""
        n = C.c_uint32()
        self._chk(self.lib.sol_scene_triangle_records(self.h, None, None, None, 0, C.byref(n)))
        tris = np.zeros(n.value, dtype=self.TRI_DTYPE)
        shade = np.zeros(n.value, dtype=self.TRI_SHADE_DTYPE)
        of = np.zeros(n.value, dtype=np.uint32)
        self._chk(self.lib.sol_scene_triangle_records(self.h, tris.ctypes.data, shade.ctypes.data, of.ctypes.data, n.value, C.byref(n)))
        return tris, shade, of

    # ---- new places for the spheres and quads of a live scene, lights included (EXTENSION) ----
    def set_primitives(self, triangles=None, spheres=None, quads=None, background_proof=True, reprobe=False):
        """sol_scene_set_primitives: row i of `triangles` (float64 [n, 3, 3]: v0, v1, v2), `spheres` ([n, 4]: centre, radius) and `quads` ([n, 3, 3]:
        q, u, v) moves primitive i of that kind in the creation description; None: that kind stays. The scene must have been created with
        dynamic_primitives=True (triangles alone: dynamic_triangles=True is enough). numpy arrays go the host route; contiguous float64 torch
        tensors on the scene's device go the device route without a copy; the two are not mixed. One refit, one light rebuild and one background
        proof per call. Clears the sums and the auxiliary planes, ends an adaptive session; blocks."""
        upd = _abi.SolGeometryUpdate(size=C.sizeof(_abi.SolGeometryUpdate),
                                     flags=(0 if background_proof else _abi.SOL_GEOM_NO_BACKGROUND_PROOF) | (_abi.SOL_GEOM_REPROBE if reprobe else 0))
        given = {"triangles": (triangles, (3, 3)), "spheres": (spheres, (4,)), "quads": (quads, (3, 3))}
        given = {k: v for k, v in given.items() if v[0] is not None}
        if not given:
            raise ValueError("set_primitives: at least one of triangles, spheres, quads")
        on_device = [self._on_device(a) for a, _ in given.values()]
        if any(on_device) and not all(on_device):
            raise ValueError("set_primitives: host arrays and device tensors in one call (give all kinds the same way)")
        ps = _abi.SolPrimitiveSet(size=C.sizeof(_abi.SolPrimitiveSet), flags=_abi.SOL_PRIMS_DEVICE if on_device[0] else 0)
        keep = []
        for name, (a, shape) in given.items():
            p, d, staged = self._stage([_Arg(name, a, "f64", ("n",) + shape)], on_device[0])
            keep += staged
            # (an empty array's pointer may be null: the kind is given all the same)
            setattr(ps, name, C.c_void_p(p[name] or 16))
            setattr(ps, "n_" + name, d["n"])
        self._chk(self.lib.sol_scene_set_primitives(self.h, C.byref(ps), C.byref(upd)))

    SPHERE_DTYPE = np.dtype([("c", np.float32, 3), ("radius", np.float32), ("dfs", np.uint32), ("mat", np.int32), ("pad", np.uint32, 2)])
    QUAD_DTYPE = np.dtype([("n", np.float32, 3), ("d", np.float32), ("q", np.float32, 3), ("dfs", np.uint32), ("w", np.float32, 3), ("mat", np.int32),
                           ("u", np.float32, 3), ("area", np.float32), ("v", np.float32, 3), ("pad", np.float32)])

    def primitive_records(self, kind):
        """sol_scene_primitive_records: (records, caller index of each record) of the spheres (kind "sphere" or REF_SPHERE) or the quads ("quad",
        REF_QUAD) as the device holds them."""
        kind = {"sphere": _abi.REF_SPHERE, "quad": _abi.REF_QUAD}.get(kind, kind)
        n = C.c_uint32()
        self._chk(self.lib.sol_scene_primitive_records(self.h, int(kind), None, None, 0, C.byref(n)))
        rec = np.zeros(n.value, dtype=self.SPHERE_DTYPE if kind == _abi.REF_SPHERE else self.QUAD_DTYPE)
        of = np.zeros(n.value, dtype=np.uint32)
        self._chk(self.lib.sol_scene_primitive_records(self.h, int(kind), rec.ctypes.data, of.ctypes.data, n.value, C.byref(n)))
        return rec, of

    BLOOM_DEFAULT_THRESHOLD = 3.0 ** 0.5  # Vec3::new(1., 1., 1.).length() (bloom.rs:39)
    BLOOM_DEFAULT_MAX = 1.7976931348623157e308  # f64::MAX (bloom.rs:40)

    def bloom(self, image_ptr, num_samples, kernel_size_fraction, threshold=None, max_intensity=None):
        """BloomPostProcessor::intermediate_post_process on the device image, in place."""
        self._chk(self.lib.sol_bloom(self.h, C.c_void_p(image_ptr), num_samples, kernel_size_fraction,
                                     self.BLOOM_DEFAULT_THRESHOLD if threshold is None else threshold,
                                     self.BLOOM_DEFAULT_MAX if max_intensity is None else max_intensity))

    def bloom_rgb8(self, image_ptr, num_samples, kernel_size_fraction, threshold=None, max_intensity=None):
        """BloomPostProcessor::post_process of the device image -> RGB8 (H, W, 3)."""
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        self._chk(self.lib.sol_bloom_rgb8(self.h, C.c_void_p(image_ptr), num_samples, kernel_size_fraction,
                                          self.BLOOM_DEFAULT_THRESHOLD if threshold is None else threshold,
                                          self.BLOOM_DEFAULT_MAX if max_intensity is None else max_intensity,
                                          out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def debug_path(self, x, y, sample, seed, max_rows=80):
        """Rays of one path: rows of (o xyz, d xyz, t, ref bits, dfs bits, depth, 0, 0); returns (rows, colour)."""
        buf = np.zeros((max_rows, 12), dtype=np.float32)
        self._chk(self.lib.sol_debug_path(self.h, x, y, sample, seed, buf.ctypes.data, max_rows))
        n = int(np.argmax(buf[:, 3] == -1.0)) if (buf[:, 3] == -1.0).any() else max_rows - 1
        return buf[:n], buf[n, :3].copy()

    def kernel_timing(self, enable=True):
        self._chk(self.lib.sol_kernel_timing(self.h, 1 if enable else 0))

    def last_kernel_ms(self):
        ms, grid = C.c_float(), C.c_uint32()
        self._chk(self.lib.sol_last_kernel_ms(self.h, C.byref(ms), C.byref(grid)))
        return float(ms.value), int(grid.value)

    def phase_stats(self):
        st = _abi.SolStats()
        self._chk(self.lib.sol_stats(self.h, C.byref(st)))
        return st.phases()

    def stats(self):
        st = _abi.SolStats()
        self._chk(self.lib.sol_stats(self.h, C.byref(st)))
        return st.as_dict()


# ---- lightmap unwrap (EXTENSION): no scene, so no DeviceScene ----
class _DeviceCalls(DeviceScene):
    """The two-route call path (DeviceScene._stage and _call) for entry points that take a device index where the others take a
    handle: the index stands in the handle's place, and there is nothing to create or destroy."""

    def __init__(self, device):
        self.lib = _abi.load_hip()
        self.device = int(device)
        self.h = int(device)

    def close(self):
        pass


UnwrapResult = namedtuple("UnwrapResult", "n_charts live_triangles used_width used_height overflow content_texels")
UnwrapFit = namedtuple("UnwrapFit", "uvs chart_of_triangle result texels_per_unit overflow_at")
UNWRAP_OVERFLOW_WIDTH, UNWRAP_OVERFLOW_HEIGHT = _abi.SOL_UNWRAP_OVERFLOW_WIDTH, _abi.SOL_UNWRAP_OVERFLOW_HEIGHT


def lightmap_unwrap(vertices, width, height, texels_per_unit, gutter=2, crease_cos=-1.0, device=0):
    """sol_lightmap_unwrap: lightmap UVs for a mesh. vertices [n, 3, 3] float32. Charts are the connected pieces of the mesh whose triangles face
    the same way along the same dominant axis (and, across an edge, whose unit normals have a dot product >= crease_cos); each is projected
    along that axis at texels_per_unit and the charts are packed by the greedy shelf rule into a width x height atlas with `gutter` texels
    between them. Returns (uvs [n, 3, 2] float32, chart_of_triangle [n], result): what lightmap_points, lightmap_dilate_charts and
    lightmap_sample_charts take. When result.overflow is not 0 - bit 0: a chart is wider than the atlas, bit 1: used_height > height - the UVs
    are zero and the labels CHART_NONE; the sizes are still reported (lightmap_unwrap_fit looks for a density that fits). Self-overlapping
    charts (a spiral ramp) are not detected: raise crease_cos to cut them. Host arrays go the host route; device tensors of `device` the device
    route, on torch's current stream, and return tensors (the labels as int32 words). Both routes block."""
    calls = _DeviceCalls(device)
    on_device = calls._on_device(vertices)
    cfg = _abi.SolUnwrapConfig(size=C.sizeof(_abi.SolUnwrapConfig), width=int(width), height=int(height), gutter=int(gutter),
                               texels_per_unit=float(texels_per_unit), crease_cos=float(crease_cos))
    stream = ()
    if on_device:
        import torch
        stream = (C.c_void_p(torch.cuda.current_stream(calls.device).cuda_stream),)
    out = calls._call("sol_lightmap_unwrap", [_Arg("vertices", vertices, "f32", ("n", 3, 3), null_if_empty=True)],
                      [_Out("uvs", "f32", ("n", 3, 2), null_if_empty=True), _Out("chart_of", "u32", ("n",), null_if_empty=True),
                       _Out("result", "u32", (8,), zero=True)],
                      lambda p, d: stream + (C.byref(cfg), p["vertices"], d["n"], p["uvs"], p["chart_of"], p["result"]), device=on_device, sync=False)
    words = (out["result"].cpu().numpy() if on_device else out["result"]).view(np.uint32)
    result = UnwrapResult(*(int(w) for w in words[:5]), int(words[6]) | (int(words[7]) << 32))
    return out["uvs"], out["chart_of"], result


def lightmap_unwrap_fit(vertices, width, height, gutter=2, crease_cos=-1.0, device=0, steps=16):
    """The densest lightmap_unwrap that fits: texels_per_unit is doubled from one texel over the mesh's largest extent until the unwrap
    overflows, then bisected `steps` times between the last density that fit and the first that did not. Returns UnwrapFit(uvs,
    chart_of_triangle, result, texels_per_unit, overflow_at): the densest probe that fit and the least density probed that overflowed - one
    bisection step denser. No device code of its own: every probe is one lightmap_unwrap. The defaults (gutter,
    steps, the starting density) are not tuned. Raises ValueError when even the starting density overflows (more charts than the atlas has
    room for at any density)."""
    v = vertices.detach().cpu().numpy() if DeviceScene._on_device(vertices) else np.asarray(vertices, dtype=np.float32)
    v = v.reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    extent = float((v.max(axis=0) - v.min(axis=0)).max()) if len(v) else 0.0
    lo = 1.0 / extent if extent > 0 else 1.0

    def probe(t):
        return lightmap_unwrap(vertices, width, height, t, gutter=gutter, crease_cos=crease_cos, device=device)
    best = probe(lo)
    if best[2].overflow:
        raise ValueError(f"lightmap_unwrap_fit: {best[2].n_charts} charts overflow a {width} x {height} atlas at every density")
    hi = lo * 2.0
    for _ in range(64):  # (2^64 times the starting density: no atlas holds that)
        out = probe(hi)
        if out[2].overflow:
            break
        best, lo, hi = out, hi, hi * 2.0
    for _ in range(int(steps)):
        mid = 0.5 * (lo + hi)
        out = probe(mid)
        if out[2].overflow:
            hi = mid
        else:
            best, lo = out, mid
    return UnwrapFit(*best, lo, hi)
