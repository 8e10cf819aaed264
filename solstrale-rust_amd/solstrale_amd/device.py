"""Thin Python handle over the device C ABI (libsolstrale_hip.so). No compute happens in Python and there is no
fallback: every call goes to the HIP library and raises if it fails (e.g. SOL_EDEVICE without a GPU)."""
import ctypes as C
import math

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
    RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("status", np.uint32), ("kind", np.uint32),
                              ("dfs_index", np.uint32), ("material", np.uint32), ("reserved", np.uint32)])

    def _query(self, mode, rays):
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):  # the host route: sol_query stages the arrays itself
            a = np.ascontiguousarray(rays, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 8:
                raise ValueError("rays: an [n, 8] float32 array of (origin xyz, tmin, direction xyz, tmax)")
            out = np.zeros(a.shape[0], dtype=np.uint32 if mode == _abi.SOL_QUERY_OCCLUDED else self.RAY_HIT_DTYPE)
            self._chk(self.lib.sol_query(self.h, mode, a.ctypes.data, a.shape[0], out.ctypes.data))
            return out
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous() or not rays.is_cuda:
            raise ValueError("rays: a contiguous [n, 8] float32 tensor on the scene's device")
        n = int(rays.shape[0])
        out = torch.empty((n,) if mode == _abi.SOL_QUERY_OCCLUDED else (n, 8), dtype=torch.int32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()  # (the rays may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_query_dev(self.h, mode, C.c_void_p(rays.data_ptr()), n, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

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
        return self._radiance(self.lib.sol_radiance, self.lib.sol_radiance_dev, "rays", "origin xyz, tmin, direction xyz, tmax", rays, keys, cfg)

    def _radiance(self, host_fn, dev_fn, what, row, rays, keys, cfg, words=4, raw=False):
        """The two routes radiance(), irradiance(), irradiance_sh() and visibility() share: `rays` are the [n, 8] rows (`what`: their name in messages,
        `row`: their words), `words` the 32-bit words of an answer (4: a SolRadiance, returned split into sums and counts; 28: a SolSh9 and 8: a
        SolVisibility, returned raw)."""
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):  # the host route: the library stages the arrays itself
            a = np.ascontiguousarray(rays, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 8:
                raise ValueError(f"{what}: an [n, 8] float32 array of ({row})")
            k = None
            if keys is not None:
                k = np.ascontiguousarray(keys.cpu().numpy() if hasattr(keys, "data_ptr") else keys).astype(np.uint32, copy=False)
                if k.shape != (a.shape[0], 2):
                    raise ValueError(f"keys: an [n, 2] uint32 array of (pixel, first_draw), one row per row of {what}")
                k = np.ascontiguousarray(k)
            out = np.zeros((a.shape[0], words), dtype=np.float32)
            self._chk(host_fn(self.h, a.ctypes.data, None if k is None else k.ctypes.data, a.shape[0], C.byref(cfg), out.ctypes.data))
            if words != 4 or raw:
                return out
            return np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3]).view(np.uint32)
        import torch
        n = self._device_rows(what, rays, keys)
        out = torch.empty((n, words), dtype=torch.float32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()  # (the rays may still be in the making on torch's stream: the scene's is another)
        self._chk(dev_fn(self.h, C.c_void_p(rays.data_ptr()), C.c_void_p(keys.data_ptr()) if keys is not None else None, n, C.byref(cfg),
                         C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def _device_rows(self, what, rays, keys):
        """Checks the device tensors of a radiance or irradiance call; returns n."""
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous() or not rays.is_cuda:
            raise ValueError(f"{what}: a contiguous [n, 8] float32 tensor on the scene's device")
        if rays.device.index != self.device:
            raise ValueError(f"{what}: the tensor is on cuda:{rays.device.index}, the scene on cuda:{self.device}")
        n = int(rays.shape[0])
        if keys is not None and (not hasattr(keys, "data_ptr") or keys.dtype != torch.int32 or tuple(keys.shape) != (n, 2) or not keys.is_contiguous()
                                 or keys.device != rays.device):
            raise ValueError(f"keys: a contiguous [n, 2] int32 tensor of (pixel, first_draw) on the device of {what}")
        return n

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
        return self._radiance(self.lib.sol_irradiance, self.lib.sol_irradiance_dev, "points", "position xyz, tmin, normal xyz, tmax", points, keys, cfg)

    def irradiance_rays(self, points, sample, seed=0, keys=None, key_base=0, first_draw=0, mode="cosine"):
        """sol_irradiance_rays: the rays sample `sample` of irradiance() starts with and the keys its paths go on from, as ([n, 8] float32, [n, 2]
        int32) device tensors: radiance(rays, samples=1, first_sample=sample, seed=seed, keys=keys) is that sample's contribution, bit for bit.
        points and keys: device tensors as for irradiance(), or host arrays, which are copied to the scene's device first."""
        import torch
        cfg = self._irradiance_config(1, sample, seed, key_base, first_draw, mode)
        dev = f"cuda:{self.device}"
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):
            a = np.ascontiguousarray(points, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 8:
                raise ValueError("points: an [n, 8] float32 array of (position xyz, tmin, normal xyz, tmax)")
            points = torch.from_numpy(a).to(dev)
        if keys is not None and not hasattr(keys, "data_ptr"):
            k = np.ascontiguousarray(np.ascontiguousarray(keys).astype(np.uint32, copy=False))
            keys = torch.from_numpy(k.view(np.int32)).to(dev)
        n = self._device_rows("points", points, keys)
        rays = torch.empty((n, 8), dtype=torch.float32, device=points.device)
        keys_out = torch.empty((n, 2), dtype=torch.int32, device=points.device)
        torch.cuda.current_stream(points.device).synchronize()  # (the points may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_irradiance_rays(self.h, C.c_void_p(points.data_ptr()), C.c_void_p(keys.data_ptr()) if keys is not None else None, n, C.byref(cfg),
                                               C.c_void_p(rays.data_ptr()), C.c_void_p(keys_out.data_ptr())))
        self.sync()
        return rays, keys_out

    # ---- SH irradiance queries (EXTENSION) ----
    def irradiance_sh(self, points, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="sphere"):
        """sol_irradiance_sh: irradiance()'s gather projected onto the nine real SH terms up to l = 2 - per point the SUMS over the samples of
        colour x sh9(direction), in radiance()'s association. Host arrays return (sh [n, 9, 3] float32 sums, counts [n] uint32); device tensors
        go through sol_irradiance_sh_dev without a host copy and return one [n, 28] float32 device tensor of the raw rows (27 sums, k-major, and
        the bits of the sample count). "sphere": 4 pi x sh / samples are the radiance coefficients L_k, and sh9_irradiance(L, normals) the
        irradiance for any normal; "cosine": pi x sh / samples estimates the cosine-weighted projection about the point's normal. points, keys,
        key_base, first_draw and the waits of the two routes are irradiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        rows = self._radiance(self.lib.sol_irradiance_sh, self.lib.sol_irradiance_sh_dev, "points", "position xyz, tmin, normal xyz, tmax", points, keys, cfg, words=28)
        if isinstance(rows, np.ndarray):
            return np.ascontiguousarray(rows[:, :27]).reshape(-1, 9, 3), np.ascontiguousarray(rows[:, 27]).view(np.uint32)
        return rows

    # ---- visibility gathers (EXTENSION) ----
    VISIBILITY_DTYPE = np.dtype([("bent", np.float32, (3,)), ("open", np.uint32), ("t_sum", np.float32), ("t2_sum", np.float32),
                                 ("hits", np.uint32), ("samples", np.uint32)])

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
        rows = self._radiance(lambda h, *a: self.lib.sol_visibility(h, qmode, *a), lambda h, *a: self.lib.sol_visibility_dev(h, qmode, *a), "points",
                              "position xyz, tmin, normal xyz, tmax", points, keys, cfg, words=8)
        if isinstance(rows, np.ndarray):
            return rows.view(self.VISIBILITY_DTYPE).reshape(-1)
        return rows

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
        arrays = (("vertices", vertices, (3, 3)), ("uvs", uvs, (3, 2)), ("normals", normals, (3, 3)))
        if isinstance(vertices, np.ndarray) or not hasattr(vertices, "data_ptr"):  # the host route
            a = []
            for name, x, tail in arrays:
                if x is None and name == "normals":
                    a.append(None)
                    continue
                x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "data_ptr") else x, dtype=np.float32)
                if x.ndim != 3 or x.shape[1:] != tail or (a and x.shape[0] != a[0].shape[0]):
                    raise ValueError(f"{name}: a float32 [n, {tail[0]}, {tail[1]}] array, one row per triangle")
                a.append(x)
            points = np.zeros((wh, 8), dtype=np.float32)
            texels = np.zeros(wh, dtype=LIGHTMAP_TEXEL_DTYPE)
            self._chk(self.lib.sol_lightmap_points(self.h, a[0].ctypes.data, None if a[2] is None else a[2].ctypes.data, a[1].ctypes.data, a[0].shape[0],
                                                   C.byref(cfg), points.ctypes.data, texels.ctypes.data))
            return points, texels
        import torch
        n = int(vertices.shape[0])
        for name, x, tail in arrays:
            if x is None:
                continue
            if (not hasattr(x, "data_ptr") or x.dtype != torch.float32 or x.dim() != 3 or tuple(x.shape) != (n,) + tail or not x.is_contiguous() or not x.is_cuda
                    or x.device.index != self.device):
                raise ValueError(f"{name}: a contiguous float32 [n, {tail[0]}, {tail[1]}] tensor on the scene's device, one row per triangle")
        points = torch.empty((wh, 8), dtype=torch.float32, device=vertices.device)
        texels = torch.empty((wh, 4), dtype=torch.int32, device=vertices.device)
        torch.cuda.current_stream(vertices.device).synchronize()  # (the arrays may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_points_dev(self.h, C.c_void_p(vertices.data_ptr()), C.c_void_p(normals.data_ptr()) if normals is not None else None,
                                                   C.c_void_p(uvs.data_ptr()), n, C.byref(cfg), C.c_void_p(points.data_ptr()), C.c_void_p(texels.data_ptr())))
        self.sync()
        return points, texels

    def lightmap_dilate(self, values, texels, width, height, passes=1, channels=3, return_pass_of=False):
        """sol_lightmap_dilate: the border dilation that finishes a bake. values: `width * height` rows whose leading `channels` 32-bit words are
        floats (a [n, k] float32 array or tensor - the raw rows a gather returned: channels=3 for radiance / irradiance rows, 27 for irradiance_sh);
        texels: what lightmap_points returned. Owned rows are copied whole; in each of `passes` passes an uncovered texel with a covered neighbour
        gets their mean, the rest of its row zero. Host arrays go the host route, device tensors the device route, and the answer has the shape and
        place of `values`. return_pass_of: also the uint8 plane [height, width] of 0 owned, k filled in pass k, 255 never filled."""
        width, height = int(width), int(height)
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            v = np.ascontiguousarray(values, dtype=np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            if v.ndim != 2 or v.shape[0] != width * height or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (width * height,):
                raise ValueError("values: [width * height, k] float32 rows; texels: width * height LIGHTMAP_TEXEL_DTYPE rows")
            out = np.zeros_like(v)
            pass_of = np.zeros((height, width), dtype=np.uint8) if return_pass_of else None
            self._chk(self.lib.sol_lightmap_dilate(self.h, t.ctypes.data, width, height, v.ctypes.data, int(channels), v.shape[1] * 4, int(passes), out.ctypes.data,
                                                   None if pass_of is None else pass_of.ctypes.data))
            return (out, pass_of) if return_pass_of else out
        import torch
        if (values.dtype != torch.float32 or values.dim() != 2 or values.shape[0] != width * height or not values.is_contiguous() or not values.is_cuda
                or values.device.index != self.device):
            raise ValueError("values: a contiguous [width * height, k] float32 tensor on the scene's device")
        if (not hasattr(texels, "data_ptr") or texels.dtype != torch.int32 or tuple(texels.shape) != (width * height, 4) or not texels.is_contiguous()
                or texels.device != values.device):
            raise ValueError("texels: the contiguous [width * height, 4] int32 tensor lightmap_points returned, on the device of values")
        out = torch.empty_like(values)
        pass_of = torch.empty((height, width), dtype=torch.uint8, device=values.device) if return_pass_of else None
        torch.cuda.current_stream(values.device).synchronize()  # (the values may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_dilate_dev(self.h, C.c_void_p(texels.data_ptr()), width, height, C.c_void_p(values.data_ptr()), int(channels),
                                                   int(values.shape[1]) * 4, int(passes), C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(pass_of.data_ptr()) if pass_of is not None else None))
        self.sync()
        return (out, pass_of) if return_pass_of else out

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
        host = isinstance(values, np.ndarray) or not hasattr(values, "data_ptr")
        k = int(values.shape[1]) if getattr(values, "ndim", 0) == 2 else 0
        cfg = _abi.SolLightmapFilterConfig(size=C.sizeof(_abi.SolLightmapFilterConfig), width=width, height=height, iterations=int(iterations),
                                           normal_power_log2=int(normal_power_log2), channels=int(channels), stride_bytes=4 * k,
                                           sigma_position=float(sigma_position), sigma_plane=float(sigma_position if sigma_plane is None else sigma_plane),
                                           sigma_value=float(sigma_value), value_scale=float(value_scale))
        if host:
            v = np.ascontiguousarray(values, dtype=np.float32)
            p = np.ascontiguousarray(points.cpu().numpy() if hasattr(points, "data_ptr") else points, dtype=np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            if (v.ndim != 2 or v.shape[0] != width * height or p.shape != (width * height, 8) or t.dtype != LIGHTMAP_TEXEL_DTYPE
                    or t.shape != (width * height,)):
                raise ValueError("values: [width * height, k] float32 rows; points: [width * height, 8] float32 rows; texels: width * height "
                                 "LIGHTMAP_TEXEL_DTYPE rows")
            out = np.zeros_like(v)
            self._chk(self.lib.sol_lightmap_filter(self.h, C.byref(cfg), p.ctypes.data, t.ctypes.data, v.ctypes.data, out.ctypes.data))
            return out
        import torch
        if (values.dtype != torch.float32 or values.dim() != 2 or values.shape[0] != width * height or not values.is_contiguous() or not values.is_cuda
                or values.device.index != self.device):
            raise ValueError("values: a contiguous [width * height, k] float32 tensor on the scene's device")
        if (not hasattr(points, "data_ptr") or points.dtype != torch.float32 or tuple(points.shape) != (width * height, 8) or not points.is_contiguous()
                or points.device != values.device):
            raise ValueError("points: the contiguous [width * height, 8] float32 tensor lightmap_points returned, on the device of values")
        if (not hasattr(texels, "data_ptr") or texels.dtype != torch.int32 or tuple(texels.shape) != (width * height, 4) or not texels.is_contiguous()
                or texels.device != values.device):
            raise ValueError("texels: the contiguous [width * height, 4] int32 tensor lightmap_points returned, on the device of values")
        out = torch.empty_like(values)
        torch.cuda.current_stream(values.device).synchronize()  # (the values may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_filter_dev(self.h, C.byref(cfg), C.c_void_p(points.data_ptr()), C.c_void_p(texels.data_ptr()),
                                                   C.c_void_p(values.data_ptr()), C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    # ---- irradiance moments and the variance-guided lightmap filter (EXTENSION) ----
    def irradiance_moments(self, points, samples=1, first_sample=0, seed=0, keys=None, key_base=0, first_draw=0, mode="cosine"):
        """sol_irradiance_moments: irradiance()'s gather with the sums of the squared sample colours beside it. Per point `sum` (irradiance()'s
        answer, bit for bit), `samples`, `sum2` - the sums over the samples of colour x colour per channel, in radiance()'s association - and
        `reserved` = 0. Host arrays go the host route and return a structured array (MOMENTS_DTYPE); device tensors go through
        sol_irradiance_moments_dev without a host copy and return the raw [n, 8] float32 rows (moments_to_numpy views them as the structured
        array). moments_mean_variance gives the mean and the variance of the mean. points, keys, key_base, first_draw, the modes and the waits
        of the two routes are irradiance()'s."""
        cfg = self._irradiance_config(samples, first_sample, seed, key_base, first_draw, mode)
        rows = self._radiance(self.lib.sol_irradiance_moments, self.lib.sol_irradiance_moments_dev, "points", "position xyz, tmin, normal xyz, tmax", points, keys,
                              cfg, words=8)
        if isinstance(rows, np.ndarray):
            return rows.view(MOMENTS_DTYPE).reshape(-1)
        return rows

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
        if isinstance(moments, np.ndarray) or not hasattr(moments, "data_ptr"):  # the host route
            m = np.ascontiguousarray(moments)
            m = m.view(np.float32).reshape(-1, 8) if m.dtype == MOMENTS_DTYPE else np.ascontiguousarray(m, dtype=np.float32)
            p = np.ascontiguousarray(points.cpu().numpy() if hasattr(points, "data_ptr") else points, dtype=np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            if m.shape != (wh, 8) or p.shape != (wh, 8) or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,):
                raise ValueError("moments: width * height MOMENTS_DTYPE rows (or [width * height, 8] float32); points: [width * height, 8] float32 rows; "
                                 "texels: width * height LIGHTMAP_TEXEL_DTYPE rows")
            out = np.zeros((wh, 4), dtype=np.float32)
            var = np.zeros((wh, 4), dtype=np.float32) if return_variance else None
            self._chk(self.lib.sol_lightmap_filter_var(self.h, C.byref(cfg), p.ctypes.data, t.ctypes.data, m.ctypes.data, out.ctypes.data,
                                                       None if var is None else var.ctypes.data))
            return (out, var) if return_variance else out
        import torch
        if (moments.dtype != torch.float32 or tuple(moments.shape) != (wh, 8) or not moments.is_contiguous() or not moments.is_cuda
                or moments.device.index != self.device):
            raise ValueError("moments: the contiguous [width * height, 8] float32 tensor irradiance_moments returned, on the scene's device")
        if (not hasattr(points, "data_ptr") or points.dtype != torch.float32 or tuple(points.shape) != (wh, 8) or not points.is_contiguous()
                or points.device != moments.device):
            raise ValueError("points: the contiguous [width * height, 8] float32 tensor lightmap_points returned, on the device of moments")
        if (not hasattr(texels, "data_ptr") or texels.dtype != torch.int32 or tuple(texels.shape) != (wh, 4) or not texels.is_contiguous()
                or texels.device != moments.device):
            raise ValueError("texels: the contiguous [width * height, 4] int32 tensor lightmap_points returned, on the device of moments")
        out = torch.empty((wh, 4), dtype=torch.float32, device=moments.device)
        var = torch.empty((wh, 4), dtype=torch.float32, device=moments.device) if return_variance else None
        torch.cuda.current_stream(moments.device).synchronize()  # (the moments may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_filter_var_dev(self.h, C.byref(cfg), C.c_void_p(points.data_ptr()), C.c_void_p(texels.data_ptr()),
                                                       C.c_void_p(moments.data_ptr()), C.c_void_p(out.data_ptr()),
                                                       C.c_void_p(var.data_ptr()) if var is not None else None))
        self.sync()
        return (out, var) if return_variance else out

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

        def host_fn(h, p, k, n, c, out):
            return self.lib.sol_irradiance_adaptive(h, p, k, n, c, C.byref(ad), out, C.byref(stats))

        def dev_fn(h, p, k, n, c, out):
            return self.lib.sol_irradiance_adaptive_dev(h, p, k, n, c, C.byref(ad), out, C.byref(stats))

        rows = self._radiance(host_fn, dev_fn, "points", "position xyz, tmin, normal xyz, tmax", points, keys, cfg, words=8)
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
        target = int(target_samples)
        if isinstance(rows, np.ndarray) or not hasattr(rows, "data_ptr"):
            a = np.ascontiguousarray(rows, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 4:
                raise ValueError("rows: an [n, 4] float32 array of (r, g, b sums, the bits of the sample count)")
            if in_place and a is not rows:
                raise ValueError("rows: in_place needs the contiguous float32 array itself")
            out = a if in_place else np.zeros_like(a)
            self._chk(self.lib.sol_radiance_rescale(self.h, a.ctypes.data, a.shape[0], target, out.ctypes.data))
            return out
        import torch
        if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 4 or not rows.is_contiguous() or not rows.is_cuda or rows.device.index != self.device:
            raise ValueError("rows: a contiguous [n, 4] float32 tensor on the scene's device")
        out = rows if in_place else torch.empty_like(rows)
        torch.cuda.current_stream(rows.device).synchronize()  # (the rows may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_radiance_rescale_dev(self.h, C.c_void_p(rows.data_ptr()), int(rows.shape[0]), target, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    # ---- lightmap lookups (EXTENSION) ----
    def lightmap_coords(self, hits, triangle_of_dfs):
        """sol_lightmap_coords: closest_hits' rows turned into surface rows (triangle, b1, b2, flags) through `triangle_of_dfs`, the uint32 table
        lightmap_triangle_table makes (per dfs_index the lightmap triangle and its record's rotation, or SOL_TEXEL_NONE). A RAY_HIT_DTYPE array
        goes the host route and returns a LIGHTMAP_TEXEL_DTYPE array; the [n, 8] int32 device tensor closest_hits returned goes through
        sol_lightmap_coords_dev and returns an [n, 4] int32 device tensor (lightmap_texels_to_numpy views it). A miss, a sphere, a quad, and a
        triangle the table does not list answer (SOL_TEXEL_NONE, 0, 0, 0)."""
        table = np.ascontiguousarray(triangle_of_dfs.cpu().numpy() if hasattr(triangle_of_dfs, "data_ptr") else triangle_of_dfs).astype(np.uint32, copy=False).reshape(-1)
        if isinstance(hits, np.ndarray) or not hasattr(hits, "data_ptr"):  # the host route
            h = np.ascontiguousarray(hits)
            if h.dtype != self.RAY_HIT_DTYPE or h.ndim != 1:
                raise ValueError("hits: a RAY_HIT_DTYPE array, what closest_hits returned")
            out = np.zeros(h.shape[0], dtype=LIGHTMAP_TEXEL_DTYPE)
            self._chk(self.lib.sol_lightmap_coords(self.h, h.ctypes.data, h.shape[0], table.ctypes.data if len(table) else None, len(table), out.ctypes.data))
            return out
        import torch
        if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 8 or not hits.is_contiguous() or not hits.is_cuda or hits.device.index != self.device:
            raise ValueError("hits: the contiguous [n, 8] int32 tensor closest_hits returned, on the scene's device")
        d_table = (triangle_of_dfs if hasattr(triangle_of_dfs, "data_ptr") and triangle_of_dfs.is_cuda and triangle_of_dfs.dtype == torch.int32
                   and triangle_of_dfs.is_contiguous() else torch.from_numpy(table.view(np.int32)).to(hits.device))
        out = torch.empty((int(hits.shape[0]), 4), dtype=torch.int32, device=hits.device)
        torch.cuda.current_stream(hits.device).synchronize()  # (the hits and the table may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_coords_dev(self.h, C.c_void_p(hits.data_ptr()), int(hits.shape[0]), C.c_void_p(d_table.data_ptr()) if len(table) else None,
                                                   len(table), C.c_void_p(out.data_ptr())))
        self.sync()
        return out

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
        k = int(values.shape[1]) if getattr(values, "ndim", 0) == 2 else 0
        cfg = _abi.SolLightmapSampleConfig(size=C.sizeof(_abi.SolLightmapSampleConfig), width=width, height=height, channels=channels, stride_bytes=4 * k,
                                           flags=_abi.SOL_LIGHTMAP_SAMPLE_NEAREST if nearest else 0,
                                           chart_radius=float("inf") if chart_radius is None else float(chart_radius))
        out_words = channels + 1 if 1 <= channels <= 32 else 1
        wh = width * height
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            host = self._host_array
            v, u, vx, p = host(values, np.float32), host(uvs, np.float32), host(vertices, np.float32), host(points, np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            c = np.ascontiguousarray(lightmap_texels_to_numpy(coords) if hasattr(coords, "data_ptr") else coords)
            po = host(pass_of, np.uint8)
            if (v.ndim != 2 or v.shape[0] != wh or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,) or c.dtype != LIGHTMAP_TEXEL_DTYPE or c.ndim != 1
                    or u.ndim != 3 or u.shape[1:] != (3, 2) or (po is not None and po.size != wh) or (vx is not None and vx.shape != (u.shape[0], 3, 3))
                    or (p is not None and p.shape != (wh, 8))):
                raise ValueError("values: [width * height, k] float32 rows; texels, coords: LIGHTMAP_TEXEL_DTYPE rows; uvs: [n, 3, 2]; pass_of: width * height "
                                 "bytes; vertices: [n, 3, 3]; points: [width * height, 8]")
            out = np.zeros((c.shape[0], out_words), dtype=np.float32)
            self._chk(self.lib.sol_lightmap_sample(self.h, C.byref(cfg), u.ctypes.data if len(u) else None, u.shape[0], t.ctypes.data,
                                                   None if po is None else po.ctypes.data, v.ctypes.data, None if vx is None else vx.ctypes.data,
                                                   None if p is None else p.ctypes.data, c.ctypes.data, c.shape[0], out.ctypes.data))
            return out
        import torch
        dev = self._device_pointer
        n_tri = int(uvs.shape[0]) if hasattr(uvs, "shape") and len(uvs.shape) == 3 else 0
        args = (dev("uvs", uvs, torch.float32, (None, 3, 2)), n_tri, dev("texels", texels, torch.int32, (wh, 4)), dev("pass_of", pass_of, torch.uint8, (height, width)),
                dev("values", values, torch.float32, (wh, None)), dev("vertices", vertices, torch.float32, (n_tri, 3, 3)),
                dev("points", points, torch.float32, (wh, 8)), dev("coords", coords, torch.int32, (None, 4)), int(coords.shape[0]))
        out = torch.empty((int(coords.shape[0]), out_words), dtype=torch.float32, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()  # (the arrays may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_sample_dev(self.h, C.byref(cfg), *args, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def lightmap_view(self, values, uvs, texels, width, height, triangle_of_dfs, x0, y0, x1, y1, sample=0, seed=0, **sample_args):
        """The bake seen from the scene's camera: camera_rays -> closest_hits -> lightmap_coords -> lightmap_sample over the pixels [x0, x1) x
        [y0, y1), all on device memory (values, uvs, texels and what sample_args names are device tensors). Returns an [h, w, channels + 1]
        float32 device tensor; a pixel that misses, or hits something without lightmap, is zero with count 0."""
        rays = self.camera_rays(x0, y0, x1, y1, sample, seed)
        h, w = int(rays.shape[0]), int(rays.shape[1])
        coords = self.lightmap_coords(self.closest_hits(rays.reshape(-1, 8)), triangle_of_dfs)
        out = self.lightmap_sample(values, coords, uvs, texels, width, height, **sample_args)
        return out.reshape(h, w, -1)

    # ---- directional lightmaps (EXTENSION) ----
    def _device_pointer(self, name, x, dtype, shape):
        """The address of a device tensor argument (None: none), after its dtype, layout, device and shape (None: any extent) are checked."""
        if x is None:
            return None
        if (not hasattr(x, "data_ptr") or x.dtype != dtype or not x.is_contiguous() or not x.is_cuda or x.device.index != self.device
                or len(shape) != x.dim() or any(s is not None and s != d for s, d in zip(shape, x.shape))):
            raise ValueError(f"{name}: a contiguous {dtype} tensor of shape {list(shape)} on the scene's device")
        return C.c_void_p(x.data_ptr())

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
        k = int(values.shape[1]) if getattr(values, "ndim", 0) == 2 else 0
        flags = ((_abi.SOL_LIGHTMAP_SH_NEAREST if nearest else 0) | (_abi.SOL_LIGHTMAP_SH_COEFFICIENTS if coefficients else 0)
                 | (_abi.SOL_LIGHTMAP_SH_CLAMP if clamp else 0))
        cfg = _abi.SolLightmapShConfig(size=C.sizeof(_abi.SolLightmapShConfig), width=width, height=height, stride_bytes=4 * k, flags=flags,
                                       chart_radius=float("inf") if chart_radius is None else float(chart_radius), scale=float(scale))
        out_words = 28 if coefficients else 4
        wh = width * height
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            host = self._host_array
            v, u, vx, p, nr = host(values, np.float32), host(uvs, np.float32), host(vertices, np.float32), host(points, np.float32), host(normals, np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            c = np.ascontiguousarray(lightmap_texels_to_numpy(coords) if hasattr(coords, "data_ptr") else coords)
            po = host(pass_of, np.uint8)
            if (v.ndim != 2 or v.shape[0] != wh or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,) or c.dtype != LIGHTMAP_TEXEL_DTYPE or c.ndim != 1
                    or u.ndim != 3 or u.shape[1:] != (3, 2) or (po is not None and po.size != wh) or (vx is not None and vx.shape != (u.shape[0], 3, 3))
                    or (p is not None and p.shape != (wh, 8)) or (nr is not None and nr.shape != (c.shape[0], 4))):
                raise ValueError("values: [width * height, k] float32 rows; texels, coords: LIGHTMAP_TEXEL_DTYPE rows; normals: [n, 4]; uvs: [n, 3, 2]; "
                                 "pass_of: width * height bytes; vertices: [n, 3, 3]; points: [width * height, 8]")
            out = np.zeros((c.shape[0], out_words), dtype=np.float32)
            self._chk(self.lib.sol_lightmap_sh(self.h, C.byref(cfg), u.ctypes.data if len(u) else None, u.shape[0], t.ctypes.data,
                                               None if po is None else po.ctypes.data, v.ctypes.data, None if vx is None else vx.ctypes.data,
                                               None if p is None else p.ctypes.data, c.ctypes.data, None if nr is None else nr.ctypes.data, c.shape[0],
                                               out.ctypes.data))
            return out
        import torch
        dev = self._device_pointer
        n_tri = int(uvs.shape[0]) if hasattr(uvs, "shape") and len(uvs.shape) == 3 else 0
        n = int(coords.shape[0])
        args = (dev("uvs", uvs, torch.float32, (None, 3, 2)), n_tri, dev("texels", texels, torch.int32, (wh, 4)), dev("pass_of", pass_of, torch.uint8, (height, width)),
                dev("values", values, torch.float32, (wh, None)), dev("vertices", vertices, torch.float32, (n_tri, 3, 3)),
                dev("points", points, torch.float32, (wh, 8)), dev("coords", coords, torch.int32, (None, 4)), dev("normals", normals, torch.float32, (n, 4)), n)
        out = torch.empty((n, out_words), dtype=torch.float32, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()  # (the arrays may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_sh_dev(self.h, C.byref(cfg), *args, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def lightmap_normals(self, coords, vertices, normals=None):
        """sol_lightmap_normals: the unit normals of the surface rows `coords` by lightmap_points' rule - the triangle's geometric normal, or with
        per-vertex `normals` [n_triangles, 3, 3] their interpolation where it has a length - as [n, 4] float32 rows (nx, ny, nz, 0): what
        lightmap_sh takes. An invalid row, a triangle with a word that is not finite and a vector without length answer zeros. A
        LIGHTMAP_TEXEL_DTYPE array goes the host route, an [n, 4] int32 device tensor the device route."""
        if isinstance(coords, np.ndarray) or not hasattr(coords, "data_ptr"):  # the host route
            c = np.ascontiguousarray(coords)
            v = np.ascontiguousarray(vertices.cpu().numpy() if hasattr(vertices, "data_ptr") else vertices, dtype=np.float32)
            nr = None if normals is None else np.ascontiguousarray(normals.cpu().numpy() if hasattr(normals, "data_ptr") else normals, dtype=np.float32)
            if c.dtype != LIGHTMAP_TEXEL_DTYPE or c.ndim != 1 or v.ndim != 3 or v.shape[1:] != (3, 3) or (nr is not None and nr.shape != v.shape):
                raise ValueError("coords: LIGHTMAP_TEXEL_DTYPE rows; vertices, normals: [n_triangles, 3, 3]")
            out = np.zeros((c.shape[0], 4), dtype=np.float32)
            self._chk(self.lib.sol_lightmap_normals(self.h, c.ctypes.data, c.shape[0], v.ctypes.data if len(v) else None,
                                                    None if nr is None or not len(v) else nr.ctypes.data, v.shape[0], out.ctypes.data))
            return out
        import torch
        n_tri = int(vertices.shape[0]) if hasattr(vertices, "shape") and len(vertices.shape) == 3 else 0
        dev = self._device_pointer
        d_coords, d_vertices = dev("coords", coords, torch.int32, (None, 4)), dev("vertices", vertices, torch.float32, (None, 3, 3))
        d_normals = dev("normals", normals, torch.float32, (n_tri, 3, 3))
        out = torch.empty((int(coords.shape[0]), 4), dtype=torch.float32, device=coords.device)
        torch.cuda.current_stream(coords.device).synchronize()  # (the rows may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_normals_dev(self.h, d_coords, int(coords.shape[0]), d_vertices if n_tri else None, d_normals if n_tri else None, n_tri,
                                                    C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def lightmap_view_sh(self, values, uvs, texels, width, height, triangle_of_dfs, vertices, x0, y0, x1, y1, scale, sample=0, seed=0, vertex_normals=None,
                         perturb=None, **sh_args):
        """A directional bake seen from the scene's camera: camera_rays -> closest_hits -> lightmap_coords -> lightmap_normals -> lightmap_sh over
        the pixels [x0, x1) x [y0, y1), all on device memory. vertices [n_triangles, 3, 3] (and vertex_normals) give the surface's normals;
        `perturb`, an [h, w, 4] float32 device tensor of the caller's own normals, replaces them - the normal-mapped case. Returns an [h, w, 4]
        float32 device tensor (E_r, E_g, E_b, count), or [h, w, 28] with coefficients=True; a pixel that misses, or hits something without
        lightmap, is zero with count 0."""
        rays = self.camera_rays(x0, y0, x1, y1, sample, seed)
        h, w = int(rays.shape[0]), int(rays.shape[1])
        coords = self.lightmap_coords(self.closest_hits(rays.reshape(-1, 8)), triangle_of_dfs)
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
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            v = np.ascontiguousarray(values, dtype=np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            po = None if pass_of is None else np.ascontiguousarray(pass_of.cpu().numpy() if hasattr(pass_of, "data_ptr") else pass_of, dtype=np.uint8)
            if v.ndim != 2 or v.shape[0] != wh or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,) or (po is not None and po.size != wh):
                raise ValueError("values: [width * height, k] float32 rows; texels: width * height LIGHTMAP_TEXEL_DTYPE rows; pass_of: width * height bytes")
            mips, cover = np.zeros((rows, v.shape[1]), dtype=np.float32), np.zeros(rows, dtype=np.uint8)
            self._chk(self.lib.sol_lightmap_mips(self.h, t.ctypes.data, None if po is None else po.ctypes.data, width, height, v.ctypes.data, channels,
                                                 v.shape[1] * 4, lay["levels"], mips.ctypes.data if rows else None, cover.ctypes.data if rows else None))
            return mips, cover
        import torch
        dev = self._device_pointer
        d_values, d_texels = dev("values", values, torch.float32, (wh, None)), dev("texels", texels, torch.int32, (wh, 4))
        d_pass = dev("pass_of", pass_of, torch.uint8, (height, width))
        mips = torch.empty((rows, int(values.shape[1])), dtype=torch.float32, device=values.device)
        cover = torch.empty((rows,), dtype=torch.uint8, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()  # (the values may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_mips_dev(self.h, d_texels, d_pass, width, height, d_values, channels, int(values.shape[1]) * 4, lay["levels"],
                                                 C.c_void_p(mips.data_ptr()) if rows else None, C.c_void_p(cover.data_ptr()) if rows else None))
        self.sync()
        return mips, cover

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
        k = int(values.shape[1]) if getattr(values, "ndim", 0) == 2 else 0
        cfg = _abi.SolLightmapLodConfig(size=C.sizeof(_abi.SolLightmapLodConfig), width=width, height=height, channels=channels, stride_bytes=4 * k, flags=0,
                                        chart_radius=float("inf") if chart_radius is None else float(chart_radius), levels=lay["levels"])
        out_words = channels + 1 if 1 <= channels <= 32 else 1
        wh, rows = width * height, lay["rows"]
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            host = self._host_array
            v, u, vx, p = host(values, np.float32), host(uvs, np.float32), host(vertices, np.float32), host(points, np.float32)
            m, cv, ld, po = host(mips, np.float32), host(cover, np.uint8), host(lods, np.float32), host(pass_of, np.uint8)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            c = np.ascontiguousarray(lightmap_texels_to_numpy(coords) if hasattr(coords, "data_ptr") else coords)
            if (v.ndim != 2 or v.shape[0] != wh or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,) or c.dtype != LIGHTMAP_TEXEL_DTYPE or c.ndim != 1
                    or u.ndim != 3 or u.shape[1:] != (3, 2) or (po is not None and po.size != wh) or (vx is not None and vx.shape != (u.shape[0], 3, 3))
                    or (p is not None and p.shape != (wh, 8)) or ld.shape != (c.shape[0],)
                    or (rows and (m is None or cv is None or m.shape != (rows, v.shape[1]) or cv.shape != (rows,)))):
                raise ValueError("values: [width * height, k] float32 rows; mips: [rows, k] and cover: [rows] as lightmap_mip_layout says; lods: [n]; texels, "
                                 "coords: LIGHTMAP_TEXEL_DTYPE rows; uvs: [n, 3, 2]; pass_of: width * height bytes; vertices: [n, 3, 3]; points: "
                                 "[width * height, 8]")
            out = np.zeros((c.shape[0], out_words), dtype=np.float32)
            self._chk(self.lib.sol_lightmap_sample_lod(self.h, C.byref(cfg), u.ctypes.data if len(u) else None, u.shape[0], t.ctypes.data,
                                                       None if po is None else po.ctypes.data, v.ctypes.data, m.ctypes.data if rows else None,
                                                       cv.ctypes.data if rows else None, None if vx is None else vx.ctypes.data,
                                                       None if p is None else p.ctypes.data, c.ctypes.data, ld.ctypes.data, c.shape[0], out.ctypes.data))
            return out
        import torch
        dev = self._device_pointer
        n_tri = int(uvs.shape[0]) if hasattr(uvs, "shape") and len(uvs.shape) == 3 else 0
        n = int(coords.shape[0])
        args = (dev("uvs", uvs, torch.float32, (None, 3, 2)), n_tri, dev("texels", texels, torch.int32, (wh, 4)), dev("pass_of", pass_of, torch.uint8, (height, width)),
                dev("values", values, torch.float32, (wh, None)), dev("mips", mips, torch.float32, (rows, k)) if rows else None,
                dev("cover", cover, torch.uint8, (rows,)) if rows else None, dev("vertices", vertices, torch.float32, (n_tri, 3, 3)),
                dev("points", points, torch.float32, (wh, 8)), dev("coords", coords, torch.int32, (None, 4)), dev("lods", lods, torch.float32, (n,)), n)
        out = torch.empty((n, out_words), dtype=torch.float32, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()  # (the arrays may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_sample_lod_dev(self.h, C.byref(cfg), *args, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def lightmap_lod(self, rays, hits, coords, vertices, uvs, width, height, spread, bias=0.0):
        """sol_lightmap_lod: the level of detail of each hit - half the piecewise-linear log2 of the squared number of texels under a pixel along
        its footprint's major axis, plus `bias`, no less than 0. rays [n, 8], hits (closest_hits' rows) and coords (lightmap_coords' rows) belong
        together row by row; vertices [n_triangles, 3, 3] and uvs [n_triangles, 3, 2] are the lightmap mesh; spread: the angle in radians between
        the rays of neighbouring pixels (pixel_spread). A miss, an invalid row and a degenerate triangle answer 0. Returns [n] float32: what
        lightmap_sample_lod takes. Host arrays go the host route, device tensors the device route, decided by `rays`."""
        width, height = int(width), int(height)
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):  # the host route
            r = np.ascontiguousarray(rays, dtype=np.float32)
            h = np.ascontiguousarray(self.hits_to_numpy(hits) if hasattr(hits, "data_ptr") else hits)
            c = np.ascontiguousarray(lightmap_texels_to_numpy(coords) if hasattr(coords, "data_ptr") else coords)
            v = np.ascontiguousarray(vertices.cpu().numpy() if hasattr(vertices, "data_ptr") else vertices, dtype=np.float32)
            u = np.ascontiguousarray(uvs.cpu().numpy() if hasattr(uvs, "data_ptr") else uvs, dtype=np.float32)
            if (r.ndim != 2 or r.shape[1] != 8 or h.dtype != self.RAY_HIT_DTYPE or h.shape != (r.shape[0],) or c.dtype != LIGHTMAP_TEXEL_DTYPE
                    or c.shape != (r.shape[0],) or v.ndim != 3 or v.shape[1:] != (3, 3) or u.shape != (v.shape[0], 3, 2)):
                raise ValueError("rays: [n, 8] float32; hits: n RAY_HIT_DTYPE rows; coords: n LIGHTMAP_TEXEL_DTYPE rows; vertices: [t, 3, 3]; uvs: [t, 3, 2]")
            out = np.zeros(r.shape[0], dtype=np.float32)
            self._chk(self.lib.sol_lightmap_lod(self.h, r.ctypes.data, h.ctypes.data, c.ctypes.data, r.shape[0], v.ctypes.data if len(v) else None,
                                                u.ctypes.data if len(v) else None, v.shape[0], width, height, float(spread), float(bias), out.ctypes.data))
            return out
        import torch
        dev = self._device_pointer
        n = int(rays.shape[0])
        n_tri = int(vertices.shape[0]) if hasattr(vertices, "shape") and len(vertices.shape) == 3 else 0
        d_rays, d_hits, d_coords = dev("rays", rays, torch.float32, (n, 8)), dev("hits", hits, torch.int32, (n, 8)), dev("coords", coords, torch.int32, (n, 4))
        d_vertices, d_uvs = dev("vertices", vertices, torch.float32, (n_tri, 3, 3)), dev("uvs", uvs, torch.float32, (n_tri, 3, 2))
        out = torch.empty((n,), dtype=torch.float32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()  # (the rows may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_lod_dev(self.h, d_rays, d_hits, d_coords, n, d_vertices if n_tri else None, d_uvs if n_tri else None, n_tri, width, height,
                                                float(spread), float(bias), C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def lightmap_view_lod(self, values, mips, cover, uvs, texels, width, height, triangle_of_dfs, vertices, x0, y0, x1, y1, spread, bias=0.0, sample=0, seed=0,
                          **sample_args):
        """The bake seen from the scene's camera without aliasing: camera_rays -> closest_hits -> lightmap_coords -> lightmap_lod ->
        lightmap_sample_lod over the pixels [x0, x1) x [y0, y1), all on device memory. spread: pixel_spread of the camera; sample_args: what
        lightmap_sample_lod takes by name (channels, pass_of, levels, chart_radius, points; `vertices` serves the guard too). Returns an
        [h, w, channels + 1] float32 device tensor; a pixel that misses, or hits something without lightmap, is zero with count 0."""
        rays = self.camera_rays(x0, y0, x1, y1, sample, seed)
        h, w = int(rays.shape[0]), int(rays.shape[1])
        rays = rays.reshape(-1, 8)
        hits = self.closest_hits(rays)
        coords = self.lightmap_coords(hits, triangle_of_dfs)
        lods = self.lightmap_lod(rays, hits, coords, vertices, uvs, width, height, spread, bias)
        if sample_args.get("points") is not None:
            sample_args = {**sample_args, "vertices": vertices}
        out = self.lightmap_sample_lod(values, mips, cover, lods, coords, uvs, texels, width, height, **sample_args)
        return out.reshape(h, w, -1)

    # ---- lightmap charts (EXTENSION) ----
    @staticmethod
    def _host_array(x, dtype=None):
        return None if x is None else np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "data_ptr") else x, dtype=dtype)

    @classmethod
    def _host_words(cls, name, x):
        """A host array (or device tensor) of chart labels as contiguous uint32 words: uint32 as it is, int32 reinterpreted; anything else is refused."""
        a = cls._host_array(x)
        if a.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)):
            raise ValueError(f"{name}: 32-bit words (a uint32 or int32 array, or an int32 tensor), not {a.dtype}")
        return a.view(np.uint32).reshape(-1)

    def lightmap_charts(self, uvs, vertices=None):
        """sol_lightmap_charts: the UV islands of a mesh. uvs [n, 3, 2] float32 and, optionally, vertices [n, 3, 3]: two triangles are connected
        when they have an edge in common - the unordered pair of its end points, (u, v) or with vertices (u, v, x, y, z), equal as numbers. Returns
        (chart_of_triangle [n] - dense ids in mesh order, CHART_NONE for a triangle with a word that is not finite -, n_charts). Host arrays go
        the host route and return a uint32 array; device tensors the device route and return an int32 tensor holding the same words."""
        if isinstance(uvs, np.ndarray) or not hasattr(uvs, "data_ptr"):  # the host route
            u, vx = self._host_array(uvs, np.float32), self._host_array(vertices, np.float32)
            if u.ndim != 3 or u.shape[1:] != (3, 2) or (vx is not None and vx.shape != (u.shape[0], 3, 3)):
                raise ValueError("uvs: [n, 3, 2] float32; vertices: [n, 3, 3] float32 or None")
            n = u.shape[0]
            chart_of, n_charts = np.zeros(n, dtype=np.uint32), C.c_uint32(0)
            self._chk(self.lib.sol_lightmap_charts(self.h, u.ctypes.data if n else None, vx.ctypes.data if (vx is not None and n) else None, n,
                                                   chart_of.ctypes.data if n else None, C.addressof(n_charts)))
            return chart_of, int(n_charts.value)
        import torch
        d_uvs = self._device_pointer("uvs", uvs, torch.float32, (None, 3, 2))
        n = int(uvs.shape[0])
        d_vertices = self._device_pointer("vertices", vertices, torch.float32, (n, 3, 3))
        chart_of = torch.empty((n,), dtype=torch.int32, device=uvs.device)
        n_charts = torch.zeros((1,), dtype=torch.int32, device=uvs.device)
        torch.cuda.current_stream(uvs.device).synchronize()  # (the arrays may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_lightmap_charts_dev(self.h, d_uvs if n else None, d_vertices if n else None, n, C.c_void_p(chart_of.data_ptr()) if n else None,
                                                   C.c_void_p(n_charts.data_ptr())))
        self.sync()
        return chart_of, int(n_charts.item())

    def lightmap_dilate_charts(self, values, texels, chart_of_triangle, width, height, passes=1, channels=3):
        """sol_lightmap_dilate_charts: lightmap_dilate that never averages across charts. chart_of_triangle: what lightmap_charts returned. A
        texel is owned when its triangle has a chart; a texel filled in a pass joins the chart most of its covered neighbours hold (the lowest
        id on a tie) and takes the mean of the neighbours of that chart only. Returns (out, pass_of [height, width] uint8, chart_plane
        [height, width] - the chart of every texel, CHART_NONE where nothing reached). Host arrays go the host route, device tensors the device
        route, decided by `values`."""
        width, height = int(width), int(height)
        wh = width * height
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            v = np.ascontiguousarray(values, dtype=np.float32)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            ch = self._host_words("chart_of_triangle", chart_of_triangle) if chart_of_triangle is not None else np.zeros(0, dtype=np.uint32)
            if v.ndim != 2 or v.shape[0] != wh or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,):
                raise ValueError("values: [width * height, k] float32 rows; texels: width * height LIGHTMAP_TEXEL_DTYPE rows")
            out, pass_of, plane = np.zeros_like(v), np.zeros((height, width), dtype=np.uint8), np.zeros((height, width), dtype=np.uint32)
            self._chk(self.lib.sol_lightmap_dilate_charts(self.h, t.ctypes.data, width, height, v.ctypes.data, int(channels), v.shape[1] * 4, int(passes),
                                                          ch.ctypes.data if len(ch) else None, len(ch), out.ctypes.data, pass_of.ctypes.data, plane.ctypes.data))
            return out, pass_of, plane
        import torch
        d_values = self._device_pointer("values", values, torch.float32, (wh, None))
        d_texels = self._device_pointer("texels", texels, torch.int32, (wh, 4))
        d_chart = self._device_pointer("chart_of_triangle", chart_of_triangle, torch.int32, (None,))
        n_tri = int(chart_of_triangle.shape[0])
        out = torch.empty_like(values)
        pass_of = torch.empty((height, width), dtype=torch.uint8, device=values.device)
        plane = torch.empty((height, width), dtype=torch.int32, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()
        self._chk(self.lib.sol_lightmap_dilate_charts_dev(self.h, d_texels, width, height, d_values, int(channels), int(values.shape[1]) * 4, int(passes),
                                                          d_chart if n_tri else None, n_tri, C.c_void_p(out.data_ptr()), C.c_void_p(pass_of.data_ptr()),
                                                          C.c_void_p(plane.data_ptr())))
        self.sync()
        return out, pass_of, plane

    def lightmap_sample_charts(self, values, coords, uvs, texels, chart_of_triangle, chart_plane, width, height, channels=3, pass_of=None, nearest=False):
        """sol_lightmap_sample_charts: lightmap_sample guarded by chart id. chart_of_triangle: what lightmap_charts returned; chart_plane (and
        pass_of): what lightmap_dilate_charts returned. A tap contributes when it is inside, covered and finite and its plane word is the chart of
        the row's triangle - a dilated tap of a neighbouring chart included; a row whose triangle has no chart answers zeros. Returns
        [n, channels + 1] float32 rows as lightmap_sample does. Host arrays go the host route, device tensors the device route, decided by `values`."""
        width, height, channels = int(width), int(height), int(channels)
        k = int(values.shape[1]) if getattr(values, "ndim", 0) == 2 else 0
        cfg = _abi.SolLightmapSampleConfig(size=C.sizeof(_abi.SolLightmapSampleConfig), width=width, height=height, channels=channels, stride_bytes=4 * k,
                                           flags=_abi.SOL_LIGHTMAP_SAMPLE_NEAREST if nearest else 0, chart_radius=float("inf"))
        out_words = channels + 1 if 1 <= channels <= 32 else 1
        wh = width * height
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):  # the host route
            v, u, po = self._host_array(values, np.float32), self._host_array(uvs, np.float32), self._host_array(pass_of, np.uint8)
            t = np.ascontiguousarray(lightmap_texels_to_numpy(texels) if hasattr(texels, "data_ptr") else texels)
            c = np.ascontiguousarray(lightmap_texels_to_numpy(coords) if hasattr(coords, "data_ptr") else coords)
            ch, pl = self._host_words("chart_of_triangle", chart_of_triangle), self._host_words("chart_plane", chart_plane)
            if (v.ndim != 2 or v.shape[0] != wh or t.dtype != LIGHTMAP_TEXEL_DTYPE or t.shape != (wh,) or c.dtype != LIGHTMAP_TEXEL_DTYPE or c.ndim != 1
                    or u.ndim != 3 or u.shape[1:] != (3, 2) or (po is not None and po.size != wh) or ch.shape != (u.shape[0],) or pl.shape != (wh,)):
                raise ValueError("values: [width * height, k] float32 rows; texels, coords: LIGHTMAP_TEXEL_DTYPE rows; uvs: [n, 3, 2]; pass_of: width * height "
                                 "bytes; chart_of_triangle: n words; chart_plane: width * height words")
            out = np.zeros((c.shape[0], out_words), dtype=np.float32)
            self._chk(self.lib.sol_lightmap_sample_charts(self.h, C.byref(cfg), u.ctypes.data if len(u) else None, u.shape[0], t.ctypes.data,
                                                          None if po is None else po.ctypes.data, v.ctypes.data, ch.ctypes.data if len(ch) else None,
                                                          pl.ctypes.data, c.ctypes.data, c.shape[0], out.ctypes.data))
            return out
        import torch
        n_tri = int(uvs.shape[0]) if hasattr(uvs, "shape") and len(uvs.shape) == 3 else 0
        dev = self._device_pointer
        args = (dev("uvs", uvs, torch.float32, (None, 3, 2)), n_tri, dev("texels", texels, torch.int32, (wh, 4)), dev("pass_of", pass_of, torch.uint8, (height, width)),
                dev("values", values, torch.float32, (wh, None)), dev("chart_of_triangle", chart_of_triangle, torch.int32, (n_tri,)),
                dev("chart_plane", chart_plane, torch.int32, (height, width)), dev("coords", coords, torch.int32, (None, 4)), int(coords.shape[0]))
        out = torch.empty((int(coords.shape[0]), out_words), dtype=torch.float32, device=values.device)
        torch.cuda.current_stream(values.device).synchronize()
        self._chk(self.lib.sol_lightmap_sample_charts_dev(self.h, C.byref(cfg), *args, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def lightmap_chart_levels(self, chart_plane, width, height, pass_of=None):
        """sol_lightmap_chart_levels: how many mip levels the atlas can have before two charts meet in one level - the `levels` to hand to
        lightmap_mips. chart_plane [height, width]: what lightmap_dilate_charts returned; pass_of: its plane, or None (every texel with a chart
        counts). Returns (levels, mixed_texels [15], mixed_windows [15]): per level l >= 1 the texels that hold two charts and the 2 x 2 windows -
        a bilinear footprint - that do. A host array goes the host route, a device tensor the device route."""
        width, height = int(width), int(height)
        if isinstance(chart_plane, np.ndarray) or not hasattr(chart_plane, "data_ptr"):  # the host route
            pl, po = self._host_words("chart_plane", chart_plane), self._host_array(pass_of, np.uint8)
            if pl.shape != (width * height,) or (po is not None and po.size != width * height):
                raise ValueError("chart_plane: width * height 32-bit words; pass_of: width * height bytes")
            levels = C.c_uint32(0)
            mixed_texels, mixed_windows = np.zeros(_abi.SOL_LIGHTMAP_MAX_LEVELS, dtype=np.uint32), np.zeros(_abi.SOL_LIGHTMAP_MAX_LEVELS, dtype=np.uint32)
            self._chk(self.lib.sol_lightmap_chart_levels(self.h, pl.ctypes.data, None if po is None else po.ctypes.data, width, height, C.addressof(levels),
                                                         mixed_texels.ctypes.data, mixed_windows.ctypes.data))
            return int(levels.value), mixed_texels, mixed_windows
        import torch
        d_plane = self._device_pointer("chart_plane", chart_plane, torch.int32, (height, width))
        d_pass = self._device_pointer("pass_of", pass_of, torch.uint8, (height, width))
        answer = torch.zeros((1 + 2 * _abi.SOL_LIGHTMAP_MAX_LEVELS,), dtype=torch.int32, device=chart_plane.device)
        torch.cuda.current_stream(chart_plane.device).synchronize()
        base = answer.data_ptr()
        self._chk(self.lib.sol_lightmap_chart_levels_dev(self.h, d_plane, d_pass, width, height, C.c_void_p(base), C.c_void_p(base + 4),
                                                         C.c_void_p(base + 4 + 4 * _abi.SOL_LIGHTMAP_MAX_LEVELS)))
        self.sync()
        words = answer.cpu().numpy().view(np.uint32)
        return int(words[0]), words[1:1 + _abi.SOL_LIGHTMAP_MAX_LEVELS].copy(), words[1 + _abi.SOL_LIGHTMAP_MAX_LEVELS:].copy()

    def lightmap_view_charts(self, values, uvs, texels, chart_of_triangle, chart_plane, width, height, triangle_of_dfs, x0, y0, x1, y1, sample=0, seed=0,
                             **sample_args):
        """The bake seen from the scene's camera with the charts kept apart: camera_rays -> closest_hits -> lightmap_coords ->
        lightmap_sample_charts over the pixels [x0, x1) x [y0, y1), all on device memory. sample_args: what lightmap_sample_charts takes by name
        (channels, pass_of, nearest). Returns an [h, w, channels + 1] float32 device tensor."""
        rays = self.camera_rays(x0, y0, x1, y1, sample, seed)
        h, w = int(rays.shape[0]), int(rays.shape[1])
        coords = self.lightmap_coords(self.closest_hits(rays.reshape(-1, 8)), triangle_of_dfs)
        out = self.lightmap_sample_charts(values, coords, uvs, texels, chart_of_triangle, chart_plane, width, height, **sample_args)
        return out.reshape(h, w, -1)

    # ---- irradiance volumes (EXTENSION) ----
    @staticmethod
    def _volume_rows(grid):
        """The rows to allocate for `grid`; 1 for a grid the library refuses."""
        return grid.n_probes if all(c > 0 for c in grid.counts) and grid.n_probes <= _abi.SOL_VOLUME_MAX_PROBES else 1

    def _volume_tensor(self, name, x, rows, words):
        import torch
        if (not hasattr(x, "data_ptr") or x.dtype != torch.float32 or x.dim() != 2 or (rows is not None and x.shape[0] != rows) or x.shape[1] != words
                or not x.is_contiguous() or not x.is_cuda or x.device.index != self.device):
            raise ValueError(f"{name}: a contiguous [{'n' if rows is None else rows}, {words}] float32 tensor on the scene's device")
        if x.data_ptr() % 16:  # (a view that starts inside an allocation: the kernels move whole 16-byte words)
            raise ValueError(f"{name}: the tensor's memory must be 16-byte aligned")
        return C.c_void_p(x.data_ptr())

    def volume_points(self, grid, tmin=1e-3, tmax=float("inf"), host=False):
        """sol_volume_points: the rows (position, tmin, (0, 0, 1), tmax) of the probes of `grid` (a VolumeGrid), probe (i, j, k) in row (k * ny + j) *
        nx + i - what irradiance_sh(mode="sphere") and visibility(distances=True) take, with every position on the bits the one volume_sample
        measures from. Returns an [nx * ny * nz, 8] float32 tensor on the scene's device (sol_volume_points_dev), with host=True a numpy array
        (the host route)."""
        rec, rows = grid.record(), self._volume_rows(grid)
        if host:
            out = np.zeros((rows, 8), dtype=np.float32)
            self._chk(self.lib.sol_volume_points(self.h, C.byref(rec), float(tmin), float(tmax), out.ctypes.data))
            return out
        import torch
        out = torch.empty((rows, 8), dtype=torch.float32, device=f"cuda:{self.device}")
        self._chk(self.lib.sol_volume_points_dev(self.h, C.byref(rec), float(tmin), float(tmax), C.c_void_p(out.data_ptr())))
        self.sync()  # (the scene's stream is not torch's)
        return out

    def volume_build(self, grid, sh, visibility=None, radius=None):
        """sol_volume_build: one SolProbe per probe of `grid` from what irradiance_sh(volume_points(grid), mode="sphere") answered - the sums must be
        SPHERE mode's - and, for the hit-distance moments, what visibility(.., distances=True) answered over points whose tmax is the finite
        `radius`. Without visibility, or with radius None, the probes carry no moments and the Chebyshev weight of volume_sample leaves them
        alone. A probe without samples or with a sum that is not finite is invalid (32 zero words) and is skipped by volume_sample. Host route:
        sh as irradiance_sh returned it - the pair (sums [n, 9, 3], counts [n]) - or raw [n, 28] float32 rows, visibility a VISIBILITY_DTYPE array
        or raw [n, 8] rows; returns a VOLUME_PROBE_DTYPE array. Device route: the [n, 28] and [n, 8] float32 tensors of the gathers, without a
        copy; returns the raw [n, 32] float32 device tensor (volume_probes_to_numpy views it)."""
        rec, rows = grid.record(), self._volume_rows(grid)
        radius = 0.0 if radius is None else float(radius)
        if isinstance(sh, (tuple, list, np.ndarray)):  # the host route
            if isinstance(sh, (tuple, list)):
                sums, counts = sh
                a = np.concatenate([np.ascontiguousarray(sums, dtype=np.float32).reshape(-1, 27),
                                    np.ascontiguousarray(counts).astype(np.uint32, copy=False).view(np.float32).reshape(-1, 1)], axis=1)
            else:
                a = np.ascontiguousarray(sh, dtype=np.float32)
            a = np.ascontiguousarray(a)
            if a.shape != (rows, 28):
                raise ValueError("sh: the (sums [n, 9, 3], counts [n]) irradiance_sh returned, or raw [n, 28] float32 rows, one per probe of the grid")
            v = None
            if visibility is not None:
                v = self.visibility_to_numpy(visibility) if hasattr(visibility, "data_ptr") else np.ascontiguousarray(visibility)
                v = v.view(np.float32).reshape(-1, 8) if v.dtype == self.VISIBILITY_DTYPE else np.ascontiguousarray(v, dtype=np.float32)
                if v.shape != (rows, 8):
                    raise ValueError("visibility: a VISIBILITY_DTYPE array or raw [n, 8] float32 rows, one per probe of the grid")
                v = np.ascontiguousarray(v)
            out = np.zeros(rows, dtype=VOLUME_PROBE_DTYPE)
            self._chk(self.lib.sol_volume_build(self.h, C.byref(rec), a.ctypes.data, None if v is None else v.ctypes.data, radius, out.ctypes.data))
            return out
        import torch
        p_sh = self._volume_tensor("sh", sh, rows, 28)
        p_vis = None if visibility is None else self._volume_tensor("visibility", visibility, rows, 8)
        out = torch.empty((rows, 32), dtype=torch.float32, device=sh.device)
        torch.cuda.current_stream(sh.device).synchronize()  # (the sums may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_volume_build_dev(self.h, C.byref(rec), p_sh, p_vis, radius, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def volume_sample(self, grid, probes, points, depth=None, res=8):
        """sol_volume_sample: the irradiance at the caller's points - rows of (position xyz, tmin, normal xyz, tmax), irradiance()'s rows; tmin and
        tmax are not read - interpolated from the probes of `grid` that volume_build packed: trilinear weights over the cell of position + unit
        normal * normal_bias, times the backface and Chebyshev weights the grid's flags ask for, invalid probes left out. Host arrays (probes: a
        VOLUME_PROBE_DTYPE array or raw [n, 32] float32 rows) go the host route and return (rgb [n, 3] float32, samples [n] uint32), samples being
        the probes that contributed, 0 to 8; device tensors go through sol_volume_sample_dev without a copy and return the raw [n, 4] float32
        rows, which lightmap_dilate takes as they are. depth (sol_volume_sample_depth): the probes' res x res depth maps as
        volume_build_depth returned them (a DEPTH_TEXEL_DTYPE array, raw [n_probes, res * res, 2] float32 rows, or that device tensor) - the
        Chebyshev weight then reads mean and mean2 from a probe's map in the direction of the point instead of the probe's two isotropic words."""
        if depth is not None:
            return self._volume_sample_depth(grid, probes, points, depth, res)
        rec, rows = grid.record(), self._volume_rows(grid)
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):  # the host route
            a = np.ascontiguousarray(points, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 8:
                raise ValueError("points: an [n, 8] float32 array of (position xyz, tmin, normal xyz, tmax)")
            p = volume_probes_to_numpy(probes) if hasattr(probes, "data_ptr") else np.ascontiguousarray(probes)
            p = p.view(np.float32).reshape(-1, 32) if p.dtype == VOLUME_PROBE_DTYPE else np.ascontiguousarray(p, dtype=np.float32)
            if p.shape != (rows, 32):
                raise ValueError("probes: a VOLUME_PROBE_DTYPE array or raw [n, 32] float32 rows, one per probe of the grid")
            p = np.ascontiguousarray(p)
            out = np.zeros((a.shape[0], 4), dtype=np.float32)
            self._chk(self.lib.sol_volume_sample(self.h, C.byref(rec), p.ctypes.data, a.ctypes.data, a.shape[0], out.ctypes.data))
            return np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3]).view(np.uint32)
        import torch
        p_points = self._volume_tensor("points", points, None, 8)
        p_probes = self._volume_tensor("probes", probes, rows, 32)
        n = int(points.shape[0])
        out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
        torch.cuda.current_stream(points.device).synchronize()  # (the points may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_volume_sample_dev(self.h, C.byref(rec), p_probes, p_points, n, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

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
        rows = self._radiance(lambda h, p, k, n, c, o: self.lib.sol_visibility_oct(h, p, k, n, c, C.byref(oct_cfg), o),
                              lambda h, p, k, n, c, o: self.lib.sol_visibility_oct_dev(h, p, k, n, c, C.byref(oct_cfg), o), "points",
                              "position xyz, tmin, normal xyz, tmax", points, keys, cfg, words=4 * texels, raw=True)
        return rows.reshape(-1, texels, 4)

    def volume_build_depth(self, grid, oct, radius, res=8, sharpness_log2=5):
        """sol_volume_build_depth: the probes' depth maps from what visibility_oct(volume_points(grid, tmax=radius), res, ..) answered: per texel
        the mean and the mean square of the hit distance clamped to `radius` - (radius, radius^2) where the texel saw nothing. Returns
        [n_probes, res * res, 2] float32, a numpy array for a host array (DEPTH_TEXEL_DTYPE views it) and a device tensor for a device tensor."""
        rec, rows = grid.record(), self._volume_rows(grid)
        oct_cfg, texels = self._oct_config(res, sharpness_log2), self._oct_texels(res)
        if isinstance(oct, np.ndarray) or not hasattr(oct, "data_ptr"):  # the host route
            a = np.ascontiguousarray(oct)
            a = np.ascontiguousarray(a.view(np.float32) if a.dtype == OCT_TEXEL_DTYPE else a.astype(np.float32, copy=False)).reshape(-1, texels, 4)
            if a.shape[0] != rows:
                raise ValueError("oct: [n_probes, res * res, 4] float32 rows as visibility_oct returned them, one map per probe of the grid")
            out = np.zeros((rows, texels, 2), dtype=np.float32)
            self._chk(self.lib.sol_volume_build_depth(self.h, C.byref(rec), a.ctypes.data, C.byref(oct_cfg), float(radius), out.ctypes.data))
            return out
        import torch
        p_oct = self._volume_tensor("oct", oct.reshape(oct.shape[0], -1), rows, texels * 4)
        out = torch.empty((rows, texels, 2), dtype=torch.float32, device=oct.device)
        torch.cuda.current_stream(oct.device).synchronize()  # (the sums may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_volume_build_depth_dev(self.h, C.byref(rec), p_oct, C.byref(oct_cfg), float(radius), C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    def _volume_sample_depth(self, grid, probes, points, depth, res):
        rec, rows = grid.record(), self._volume_rows(grid)
        oct_cfg, texels = self._oct_config(res), self._oct_texels(res)
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):  # the host route
            a = np.ascontiguousarray(points, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 8:
                raise ValueError("points: an [n, 8] float32 array of (position xyz, tmin, normal xyz, tmax)")
            p = volume_probes_to_numpy(probes) if hasattr(probes, "data_ptr") else np.ascontiguousarray(probes)
            p = p.view(np.float32).reshape(-1, 32) if p.dtype == VOLUME_PROBE_DTYPE else np.ascontiguousarray(p, dtype=np.float32)
            if p.shape != (rows, 32):
                raise ValueError("probes: a VOLUME_PROBE_DTYPE array or raw [n, 32] float32 rows, one per probe of the grid")
            d = np.ascontiguousarray(depth.cpu().numpy() if hasattr(depth, "data_ptr") else depth)
            d = np.ascontiguousarray(d.view(np.float32) if d.dtype == DEPTH_TEXEL_DTYPE else d.astype(np.float32, copy=False)).reshape(-1, texels, 2)
            if d.shape[0] != rows:
                raise ValueError("depth: [n_probes, res * res, 2] float32 rows as volume_build_depth returned them, one map per probe of the grid")
            out = np.zeros((a.shape[0], 4), dtype=np.float32)
            self._chk(self.lib.sol_volume_sample_depth(self.h, C.byref(rec), np.ascontiguousarray(p).ctypes.data, d.ctypes.data, C.byref(oct_cfg), a.ctypes.data,
                                                       a.shape[0], out.ctypes.data))
            return np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3]).view(np.uint32)
        import torch
        p_points = self._volume_tensor("points", points, None, 8)
        p_probes = self._volume_tensor("probes", probes, rows, 32)
        p_depth = self._volume_tensor("depth", depth.reshape(depth.shape[0], -1) if hasattr(depth, "data_ptr") else depth, rows, texels * 2)
        n = int(points.shape[0])
        out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
        torch.cuda.current_stream(points.device).synchronize()  # (the points may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_volume_sample_depth_dev(self.h, C.byref(rec), p_probes, p_depth, C.byref(oct_cfg), p_points, n, C.c_void_p(out.data_ptr())))
        self.sync()
        return out

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
        if isinstance(vertices, np.ndarray) or not hasattr(vertices, "data_ptr"):
            a = np.ascontiguousarray(vertices, dtype=np.float64)
            if a.ndim != 3 or a.shape[1:] != (3, 3):
                raise ValueError("vertices: a float64 [n, 3, 3] array of (v0, v1, v2)")
            self._chk(self.lib.sol_scene_set_triangles(self.h, a.ctypes.data, a.shape[0], C.byref(upd)))
            return
        import torch
        if vertices.dtype != torch.float64 or vertices.dim() != 3 or tuple(vertices.shape[1:]) != (3, 3) or not vertices.is_contiguous() or not vertices.is_cuda:
            raise ValueError("vertices: a contiguous float64 [n, 3, 3] tensor on the scene's device")
        if vertices.device.index != self.device:
            raise ValueError(f"vertices: the tensor is on cuda:{vertices.device.index}, the scene on cuda:{self.device}")
        torch.cuda.current_stream(vertices.device).synchronize()  # (the vertices may still be in the making on torch's stream: the scene's is another)
        self._chk(self.lib.sol_scene_set_triangles_dev(self.h, C.c_void_p(vertices.data_ptr()), int(vertices.shape[0]), C.byref(upd)))

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
        on_device = [not isinstance(a, np.ndarray) and hasattr(a, "data_ptr") for a, _ in given.values()]
        if any(on_device) and not all(on_device):
            raise ValueError("set_primitives: host arrays and device tensors in one call (give all kinds the same way)")
        ps = _abi.SolPrimitiveSet(size=C.sizeof(_abi.SolPrimitiveSet), flags=_abi.SOL_PRIMS_DEVICE if on_device[0] else 0)
        keep = []
        for name, (a, shape) in given.items():
            what = f"{name}: a contiguous float64 [n, {', '.join(map(str, shape))}] " + ("tensor on the scene's device" if on_device[0] else "array")
            if on_device[0]:
                import torch
                if a.dtype != torch.float64 or a.dim() != 1 + len(shape) or tuple(a.shape[1:]) != shape or not a.is_contiguous() or not a.is_cuda:
                    raise ValueError(what)
                if a.device.index != self.device:
                    raise ValueError(f"{name}: the tensor is on cuda:{a.device.index}, the scene on cuda:{self.device}")
                torch.cuda.current_stream(a.device).synchronize()  # (the rows may still be in the making on torch's stream: the scene's is another)
                ptr = a.data_ptr()
            else:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.ndim != 1 + len(shape) or a.shape[1:] != shape:
                    raise ValueError(what)
                ptr = a.ctypes.data
            keep.append(a)
            # (an empty array's pointer may be null: the kind is given all the same)
            setattr(ps, name, C.c_void_p(ptr or 16))
            setattr(ps, "n_" + name, int(a.shape[0]))
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
