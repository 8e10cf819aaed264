"""ctypes mirror of include/solstrale_hip.h and include/solstrale_host.h.

This is harness plumbing for tests/ and bench.py: the product is the C-ABI shared library
(`libsolstrale_hip.so`, hand-written HIP for gfx950) and the C++ host above it. Layouts are asserted against
the C side at import time through `solh_abi_sizes` (tests/test_abi.py).
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(PKG_DIR))
BUILD_DIR = os.environ.get("SOLSTRALE_BUILD_DIR") or os.path.join(os.path.dirname(PKG_DIR), "_build")  # env: kernel A/B variants
HIP_LIB = os.path.join(BUILD_DIR, "libsolstrale_hip.so")
HOST_LIB = os.path.join(BUILD_DIR, "libsolstrale_host.so")

SOL_ABI_VERSION = 2
SOL_OK, SOL_EINVAL, SOL_ENOLIGHT, SOL_EDEVICE, SOL_EDEPTH, SOL_ENOMEM, SOL_ERANGE = 0, -1, -2, -3, -4, -5, -6
REF_NONE, REF_NODE, REF_SPHERE, REF_QUAD, REF_TRIANGLE, REF_MEDIUM = range(6)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC, MAT_BLEND = range(6)
TEX_SOLID, TEX_IMAGE = 0, 1
SHADER_PATH_TRACING, SHADER_ALBEDO, SHADER_NORMAL, SHADER_SIMPLE = range(4)


def ref_kind(r):
    return (r >> 28) & 0xF


def ref_index(r):
    return r & 0x0FFFFFFF


class SolAabb(C.Structure):
    _fields_ = [("v", C.c_double * 6)]


class SolBvhNode(C.Structure):
    _fields_ = [("bbox", SolAabb), ("left", C.c_uint32), ("right", C.c_uint32)]


class SolSphere(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("radius", C.c_double), ("bbox", SolAabb),
                ("material", C.c_int32), ("dfs_index", C.c_uint32)]


class SolQuad(C.Structure):
    _fields_ = [("q", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3), ("normal", C.c_double * 3),
                ("d", C.c_double), ("w", C.c_double * 3), ("area", C.c_double), ("bbox", SolAabb),
                ("material", C.c_int32), ("dfs_index", C.c_uint32)]


class SolTriangle(C.Structure):
    _fields_ = [("v0", C.c_double * 3), ("v0v1", C.c_double * 3), ("v0v2", C.c_double * 3),
                ("normal", C.c_double * 3), ("tangent", C.c_double * 3), ("bi_tangent", C.c_double * 3),
                ("area", C.c_double), ("uv0", C.c_float * 2), ("uv1", C.c_float * 2), ("uv2", C.c_float * 2),
                ("bbox", SolAabb), ("material", C.c_int32), ("dfs_index", C.c_uint32)]


class SolMedium(C.Structure):
    _fields_ = [("boundary", C.c_uint32), ("material", C.c_int32), ("negative_inverse_density", C.c_double),
                ("bbox", SolAabb), ("dfs_index", C.c_uint32), ("_pad", C.c_uint32)]


class SolMaterial(C.Structure):
    _fields_ = [("kind", C.c_int32), ("albedo_tex", C.c_int32), ("normal_tex", C.c_int32), ("m1", C.c_int32),
                ("m2", C.c_int32), ("_pad", C.c_int32), ("param", C.c_double)]


class SolTexture(C.Structure):
    _fields_ = [("kind", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32), ("_pad", C.c_uint32),
                ("texel_offset", C.c_uint64), ("rgb", C.c_double * 3)]


class SolCamera(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("lower_left_corner", C.c_double * 3), ("horizontal", C.c_double * 3),
                ("vertical", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3),
                ("lens_radius", C.c_double)]


class SolSceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("shader_kind", C.c_uint32), ("max_depth", C.c_uint32), ("root", C.c_uint32),
                ("background", C.c_double * 3), ("camera", SolCamera),
                ("nodes", C.POINTER(SolBvhNode)), ("n_nodes", C.c_uint32),
                ("spheres", C.POINTER(SolSphere)), ("n_spheres", C.c_uint32),
                ("quads", C.POINTER(SolQuad)), ("n_quads", C.c_uint32),
                ("triangles", C.POINTER(SolTriangle)), ("n_triangles", C.c_uint32),
                ("mediums", C.POINTER(SolMedium)), ("n_mediums", C.c_uint32),
                ("materials", C.POINTER(SolMaterial)), ("n_materials", C.c_uint32),
                ("textures", C.POINTER(SolTexture)), ("n_textures", C.c_uint32),
                ("texels", C.POINTER(C.c_uint8)), ("n_texel_bytes", C.c_uint64),
                ("lights", C.POINTER(C.c_uint32)), ("n_lights", C.c_uint32),
                ("env_texels", C.POINTER(C.c_float)), ("env_width", C.c_uint32), ("env_height", C.c_uint32),
                ("env_scale", C.c_double)]


class SolStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "node_visits", "sphere_tests", "quad_tests",
                                          "triangle_tests", "shades", "texel_fetches", "max_stack")] + \
               [("phase", C.c_uint64 * 6)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "phase"}

    def phases(self):
        p = [int(x) for x in self.phase]
        return {k: (p[2 * i] / p[2 * i + 1] if p[2 * i + 1] else 0.0) for i, k in enumerate(("traverse", "shade", "generate"))}


ABI_STRUCTS = [SolAabb, SolBvhNode, SolSphere, SolQuad, SolTriangle, SolMedium, SolMaterial, SolTexture, SolCamera,
               SolSceneDesc, SolStats]

PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_uint8), C.c_uint32,
                          C.c_uint32)
ABORT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
IMAGE_DECODER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                               C.POINTER(C.POINTER(C.c_uint8)))

_D3 = C.POINTER(C.c_double)
_libs = {}


def _sig(lib, name, res, args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = args
    return f


TREE_AUTO, TREE_REF, TREE_SAH8, TREE_SAH16, TREE_SAH64, TREE_DEVICE, TREE_HOST_PROBE = range(7)
OPT_SWITCH_BELOW, OPT_MAX_BLOCKS_PER_CU, OPT_KERNEL, OPT_WORK_ORDER, OPT_FINE_TAIL, OPT_BALANCED_PARTITION, OPT_BACKGROUND_BLOCKS = 1, 2, 3, 4, 5, 6, 7
UNIQUE_ID_BYTES = 128


class _DynamicPrimitivesWord(C.Union):
    """The last word of SolCreateOptions under both of its names: `reserved2` in the header before DESIGN.md 18, `dynamic_primitives` since."""
    _fields_ = [("dynamic_primitives", C.c_int32), ("reserved2", C.c_int32)]


class SolCreateOptions(C.Structure):
    _anonymous_ = ("_last",)
    _fields_ = [("size", C.c_uint32), ("world_tree", C.c_int32), ("no_work_order_probe", C.c_int32), ("split_percent", C.c_int32),
                ("reinsertion_rounds", C.c_int32), ("no_background_blocks", C.c_int32), ("reserved", C.c_int32 * 2),
                ("dynamic_triangles", C.c_int32), ("_last", _DynamicPrimitivesWord)]


class SolSceneInfo(C.Structure):
    _fields_ = [("size", C.c_uint32), ("stack_bound", C.c_uint32), ("lds_stack", C.c_uint32), ("spill_stack", C.c_uint32),
                ("tree_fallback", C.c_uint32), ("tree_name", C.c_char * 32), ("tree_note", C.c_char * 192),
                ("split_references", C.c_uint32), ("split_triangles", C.c_uint32), ("split_area_ratio", C.c_float),
                ("reinsertion_moves", C.c_uint32), ("reinsertion_area_ratio", C.c_float),
                ("partition_table", C.c_uint32), ("partition_crc", C.c_uint32), ("strict_triangles", C.c_uint32),
                ("background_blocks", C.c_uint32), ("background_pixels", C.c_uint32)]


class SolPathStats(C.Structure):
    _fields_ = [("size", C.c_uint32), ("pad", C.c_uint32), ("samples", C.c_uint64), ("primary_hits", C.c_uint64), ("path_len", C.c_uint64 * 6)]


class SolAdaptive(C.Structure):
    """EXTENSION: adaptive sampling (sol_adaptive_begin)."""
    _fields_ = [("size", C.c_uint32), ("round", C.c_uint32), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32),
                ("threshold", C.c_float)]


SOL_ENV_SAMPLING_OFF, SOL_ENV_SAMPLING_IMPORTANCE = 0, 1


class SolEnvSampling(C.Structure):
    """EXTENSION: environment importance sampling (sol_env_sampling). Not in ABI_STRUCTS (solh_abi_sizes has 11 sizes)."""
    _fields_ = [("size", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SOL_LIGHT_SAMPLING_UNIFORM, SOL_LIGHT_SAMPLING_TREE, SOL_LIGHT_SAMPLING_POWER = 0, 1, 2


class SolLightSampling(C.Structure):
    """EXTENSION: light tree / power-weighted light sampling (sol_light_sampling). Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("mode", C.c_uint32), ("reserved", C.c_uint32 * 2)]


DENOISE_DEFAULT_ITERATIONS, DENOISE_DEFAULT_SIGMA_COLOR, DENOISE_DEFAULT_NORMAL_POWER = 5, 0.25, 64.0


class SolDenoise(C.Structure):
    """EXTENSION: the albedo / normal guided a-trous denoiser (sol_denoise). Not in ABI_STRUCTS (solh_abi_sizes has 11 sizes)."""
    _fields_ = [("size", C.c_uint32), ("iterations", C.c_uint32), ("sigma_color", C.c_float), ("normal_power", C.c_float),
                ("reserved", C.c_uint32 * 2)]


def denoise_config(iterations=None, sigma_color=None, normal_power=None):
    """A SolDenoise with the defaults where an argument is None."""
    return SolDenoise(size=C.sizeof(SolDenoise), iterations=DENOISE_DEFAULT_ITERATIONS if iterations is None else int(iterations),
                      sigma_color=DENOISE_DEFAULT_SIGMA_COLOR if sigma_color is None else float(sigma_color),
                      normal_power=DENOISE_DEFAULT_NORMAL_POWER if normal_power is None else float(normal_power))


SOL_QUERY_CLOSEST, SOL_QUERY_OCCLUDED = 0, 1
SOL_RAY_MISS, SOL_RAY_HIT, SOL_RAY_INVALID = 0, 1, 2


class SolRay(C.Structure):
    """EXTENSION: a query ray (sol_query): origin + t * direction, t in [tmin, tmax]. Not in ABI_STRUCTS."""
    _fields_ = [("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float), ("tmin", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float), ("tmax", C.c_float)]


class SolRayHit(C.Structure):
    """EXTENSION: the answer of SOL_QUERY_CLOSEST to one ray. Not in ABI_STRUCTS."""
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("status", C.c_uint32), ("kind", C.c_uint32),
                ("dfs_index", C.c_uint32), ("material", C.c_uint32), ("reserved", C.c_uint32)]


class SolRayKey(C.Structure):
    """EXTENSION: the RNG key and the starting counter of a radiance-query ray (sol_radiance). Not in ABI_STRUCTS."""
    _fields_ = [("pixel", C.c_uint32), ("first_draw", C.c_uint32)]


class SolRadiance(C.Structure):
    """EXTENSION: the answer of sol_radiance to one ray: colour SUMS over `samples` samples. Not in ABI_STRUCTS."""
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("samples", C.c_uint32)]


class SolRadianceConfig(C.Structure):
    """EXTENSION: the sample range, seed and default keys of a radiance query. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("samples", C.c_uint32), ("first_sample", C.c_uint32), ("first_draw", C.c_uint32),
                ("seed", C.c_uint64), ("key_base", C.c_uint32), ("reserved", C.c_uint32)]


SOL_IRRADIANCE_COSINE, SOL_IRRADIANCE_SPHERE = 0, 1


class SolIrradianceConfig(C.Structure):
    """EXTENSION: the sample range, seed, default keys and direction mode of an irradiance query (sol_irradiance). Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("samples", C.c_uint32), ("first_sample", C.c_uint32), ("first_draw", C.c_uint32),
                ("seed", C.c_uint64), ("key_base", C.c_uint32), ("mode", C.c_uint32)]


class SolSh9(C.Structure):
    """EXTENSION: the answer of sol_irradiance_sh to one point: c[k][channel], the SUMS over `samples` samples of colour x Y_k(direction)
    for the nine real SH terms up to l = 2. 112 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("c", (C.c_float * 3) * 9), ("samples", C.c_uint32)]


class SolVisibility(C.Structure):
    """EXTENSION: the answer of sol_visibility to one point: the SUM of the open directions (the bent normal, not normalised), the
    count of open samples, the sums of the hit distances and of their squares, the count of hits and the sample count. 32 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("bx", C.c_float), ("by", C.c_float), ("bz", C.c_float), ("open", C.c_uint32),
                ("t_sum", C.c_float), ("t2_sum", C.c_float), ("hits", C.c_uint32), ("samples", C.c_uint32)]


class SolLightmapConfig(C.Structure):
    """EXTENSION: the atlas of sol_lightmap_points: size = sizeof, W x H texels, flags (SOL_LIGHTMAP_CONSERVATIVE), the tmin and tmax
    written into every point row. 32 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flags", C.c_uint32), ("tmin", C.c_float), ("tmax", C.c_float),
                ("reserved", C.c_uint32 * 2)]


class SolTexel(C.Structure):
    """EXTENSION: what sol_lightmap_points knows of one texel: the owning triangle (SOL_TEXEL_NONE: none), the barycentrics b1, b2 of the point and
    how it was claimed (1: centre inside, 2: conservative only). 16 bytes."""
    _fields_ = [("triangle", C.c_uint32), ("b1", C.c_float), ("b2", C.c_float), ("flags", C.c_uint32)]


SOL_LIGHTMAP_CONSERVATIVE, SOL_LIGHTMAP_MAX_SIZE, SOL_TEXEL_NONE = 1, 16384, 0xFFFFFFFF


class SolLightmapSampleConfig(C.Structure):
    """EXTENSION: the configuration of sol_lightmap_sample: size = sizeof, W x H texels, the rows' channels and stride, flags
    (SOL_LIGHTMAP_SAMPLE_NEAREST), the radius of the chart guard (> 0; +inf: off), reserved = 0. 32 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("stride_bytes", C.c_uint32),
                ("flags", C.c_uint32), ("chart_radius", C.c_float), ("reserved", C.c_uint32)]


SOL_LIGHTMAP_SAMPLE_NEAREST, SOL_LIGHTMAP_TABLE_ROTATION_SHIFT, SOL_LIGHTMAP_TABLE_TRIANGLE_MASK = 1, 30, 0x3FFFFFFF


class SolUnwrapConfig(C.Structure):
    """EXTENSION: the configuration of sol_lightmap_unwrap: size = sizeof, the atlas W x H in texels, the gutter (0 .. 64), the
    density, the crease cosine (-1 .. 1), flags = 0, reserved = 0. 32 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("gutter", C.c_uint32), ("texels_per_unit", C.c_float),
                ("crease_cos", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SolUnwrapResult(C.Structure):
    """EXTENSION: what sol_lightmap_unwrap reports: charts, live triangles, the atlas the packing used, the overflow bits
    (SOL_UNWRAP_OVERFLOW_WIDTH, _HEIGHT) and the sum of the content rectangles. 32 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("n_charts", C.c_uint32), ("live_triangles", C.c_uint32), ("used_width", C.c_uint32), ("used_height", C.c_uint32),
                ("overflow", C.c_uint32), ("reserved", C.c_uint32), ("content_texels", C.c_uint64)]


SOL_UNWRAP_MAX_GUTTER, SOL_UNWRAP_OVERFLOW_WIDTH, SOL_UNWRAP_OVERFLOW_HEIGHT = 64, 1, 2


class SolLightmapShConfig(C.Structure):
    """EXTENSION: the configuration of sol_lightmap_sh: size = sizeof, W x H texels, the stride of the SolSh9 rows (>= 112, a
    multiple of 16), flags (SOL_LIGHTMAP_SH_*), the radius of the chart guard (> 0; +inf: off), the caller's factor on E, reserved = 0. 32 bytes.
    Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("stride_bytes", C.c_uint32), ("flags", C.c_uint32),
                ("chart_radius", C.c_float), ("scale", C.c_float), ("reserved", C.c_uint32)]


SOL_LIGHTMAP_SH_NEAREST, SOL_LIGHTMAP_SH_COEFFICIENTS, SOL_LIGHTMAP_SH_CLAMP = 1, 2, 4


class SolLightmapLodConfig(C.Structure):
    """EXTENSION: the configuration of sol_lightmap_sample_lod: size = sizeof, W x H texels, the rows' channels and stride, flags = 0,
    the radius of the chart guard (> 0; +inf: off), the levels of the chain with level 0 counted (0: all), reserved = 0. 40 bytes. Not in
    ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("stride_bytes", C.c_uint32),
                ("flags", C.c_uint32), ("chart_radius", C.c_float), ("levels", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SOL_LIGHTMAP_MAX_LEVELS = 15


class SolLightmapFilterConfig(C.Structure):
    """EXTENSION: the configuration of sol_lightmap_filter: size = sizeof, W x H texels, 1..8 passes, the normal factor's exponent as a
    power of two (0..7), the rows' channels and stride, the widths of the distance, plane and value factors (>= 1e-6 or +inf), the scale a value is
    multiplied with before it is tone-mapped, reserved = 0. 64 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32),
                ("channels", C.c_uint32), ("stride_bytes", C.c_uint32), ("sigma_position", C.c_float), ("sigma_plane", C.c_float),
                ("sigma_value", C.c_float), ("value_scale", C.c_float), ("reserved", C.c_uint32 * 5)]


class SolMoments(C.Structure):
    """EXTENSION: the answer of sol_irradiance_moments to one point: the SUMS over `samples` samples of the colour (sol_irradiance's
    answer, bit for bit) and of its squares per channel; reserved = 0. 32 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("samples", C.c_uint32),
                ("r2", C.c_float), ("g2", C.c_float), ("b2", C.c_float), ("reserved", C.c_uint32)]


class SolLightmapFilterVarConfig(C.Structure):
    """EXTENSION: the configuration of sol_lightmap_filter_var: size = sizeof, W x H texels, 1..8 passes, the normal factor's exponent
    as a power of two (0..7), the widths of the distance and plane factors, the width of the value factor in standard deviations of the mean (all
    >= 1e-6 or +inf), the floor added to the prefiltered variance (finite, > 0), reserved = 0. 64 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32),
                ("sigma_position", C.c_float), ("sigma_plane", C.c_float), ("sigma_value", C.c_float), ("variance_floor", C.c_float),
                ("reserved", C.c_uint32 * 7)]


class SolGatherAdaptive(C.Structure):
    """EXTENSION: the rounds and the stop rule of sol_irradiance_adaptive: size = sizeof, samples per round (a positive multiple of
    16), the count below which no row is judged converged (a multiple of 16), reserved = 0, the relative standard error of the mean that counts as
    converged (0 = never) and the floor under the mean it is relative to. 24 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("round", C.c_uint32), ("min_samples", C.c_uint32), ("reserved", C.c_uint32), ("threshold", C.c_float),
                ("floor", C.c_float)]


class SolGatherAdaptiveStats(C.Structure):
    """EXTENSION: what sol_irradiance_adaptive reports: size = sizeof on entry; the rounds launched, the sum of the rows' final
    counts, the valid rows, the rows the rule judged converged and the rows that reached the maximum. 40 bytes. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("rounds", C.c_uint32), ("paths", C.c_uint64), ("rows_valid", C.c_uint64), ("rows_converged", C.c_uint64),
                ("rows_capped", C.c_uint64)]


class SolVolumeGrid(C.Structure):
    """EXTENSION: the probe grid of an irradiance volume (sol_volume_points / _build / _sample): size = sizeof, nx x ny x nz probes, the
    position of probe (0, 0, 0), the spacing per axis, flags (SOL_VOLUME_BACKFACE | SOL_VOLUME_CHEBYSHEV) and the normal bias of a sample. 48 bytes.
    Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32), ("origin", C.c_float * 3), ("spacing", C.c_float * 3),
                ("flags", C.c_uint32), ("normal_bias", C.c_float)]


class SolProbe(C.Structure):
    """EXTENSION: one probe of an irradiance volume as sol_volume_build packs it: e[k][channel], the irradiance coefficients with the cosine lobe
    folded in; the mean and the mean square of the hit distance; flags (SOL_PROBE_VALID | SOL_PROBE_MOMENTS); the gather's samples. 128 bytes."""
    _fields_ = [("e", (C.c_float * 3) * 9), ("mean", C.c_float), ("mean2", C.c_float), ("flags", C.c_uint32), ("samples", C.c_uint32),
                ("reserved", C.c_uint32)]


SOL_VOLUME_BACKFACE, SOL_VOLUME_CHEBYSHEV, SOL_VOLUME_MAX_PROBES, SOL_PROBE_VALID, SOL_PROBE_MOMENTS = 1, 2, 1 << 24, 1, 2


class SolOctConfig(C.Structure):
    """EXTENSION: the octahedral maps of the directional distance moments (sol_visibility_oct, sol_volume_build_depth, sol_volume_sample_depth;
    DESIGN.md 25): size = sizeof, res x res texels per map (4, 8 or 16), the lobe's exponent as a power of two (0..6), reserved = 0. 16 bytes.
    Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("res", C.c_uint32), ("sharpness_log2", C.c_uint32), ("reserved", C.c_uint32)]


class SolOctTexel(C.Structure):
    """EXTENSION: one texel of what sol_visibility_oct gathers: the sums of the lobe weights of all samples, of the open ones, and of weight x
    distance and weight x distance^2 of the hits. 16 bytes."""
    _fields_ = [("w", C.c_float), ("w_open", C.c_float), ("wt", C.c_float), ("wt2", C.c_float)]


class SolDepthTexel(C.Structure):
    """EXTENSION: one texel of a probe's depth map as sol_volume_build_depth writes it: the mean and the mean square of the hit distance in the
    texel's direction, clamped to the radius. 8 bytes."""
    _fields_ = [("mean", C.c_float), ("mean2", C.c_float)]

SOL_CAMERA_NO_BACKGROUND_PROOF, SOL_CAMERA_REPROBE = 1, 2


class SolCameraUpdate(C.Structure):
    """EXTENSION: how sol_scene_set_camera moves the camera of a live scene. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SOL_GEOM_NO_BACKGROUND_PROOF, SOL_GEOM_REPROBE = 1, 2


class SolGeometryUpdate(C.Structure):
    """EXTENSION: how sol_scene_set_triangles moves the triangles of a live scene. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


SOL_PRIMS_DEVICE = 1


class SolPrimitiveSet(C.Structure):
    """EXTENSION: the rows sol_scene_set_primitives moves the triangles, spheres and quads of a live scene to. Not in ABI_STRUCTS."""
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("triangles", C.c_void_p), ("spheres", C.c_void_p), ("quads", C.c_void_p),
                ("n_triangles", C.c_uint32), ("n_spheres", C.c_uint32), ("n_quads", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class SolTreeCheck(C.Structure):
    _fields_ = [("n_wide", C.c_uint32), ("n_leaf_refs", C.c_uint32), ("n_primitives", C.c_uint32), ("depth", C.c_uint32),
                ("max_children", C.c_uint32), ("box_violations", C.c_uint32), ("leaf_mismatches", C.c_uint32),
                ("bad_empty_slots", C.c_uint32), ("inner_area", C.c_double), ("leaf_area", C.c_double),
                ("n_extra_references", C.c_uint32), ("n_split_triangles", C.c_uint32), ("split_uncovered", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def load_hip():
    """Loads libsolstrale_hip.so (the product). Fails loudly if it has not been built."""
    if "hip" in _libs:
        return _libs["hip"]
    if not os.path.exists(HIP_LIB):
        raise RuntimeError(f"{HIP_LIB} is missing: run `python __graft_entry__.py build` (hipcc --offload-arch=gfx950)")
    lib = C.CDLL(HIP_LIB, mode=C.RTLD_GLOBAL)
    P = C.c_void_p
    _sig(lib, "sol_device_count", C.c_int, [])
    _sig(lib, "sol_scene_create", C.c_int, [C.POINTER(SolSceneDesc), C.c_int, C.POINTER(P)])
    _sig(lib, "sol_scene_destroy", None, [P])
    _sig(lib, "sol_scene_set_partition", C.c_int, [P, C.c_int, C.c_int])
    _sig(lib, "sol_accum_floats", C.c_size_t, [P])
    _sig(lib, "sol_accum_ptr", C.c_void_p, [P])
    _sig(lib, "sol_scene_bind_accum", C.c_int, [P, C.c_void_p, C.c_size_t])
    _sig(lib, "sol_scene_set_stream", C.c_int, [P, C.c_void_p])
    _sig(lib, "sol_clear", C.c_int, [P])
    _sig(lib, "sol_render", C.c_int, [P, C.c_uint32, C.c_uint32, C.c_uint64])
    _sig(lib, "sol_render_counted", C.c_int, [P, C.c_uint32, C.c_uint32, C.c_uint64])
    _sig(lib, "sol_sync", C.c_int, [P])
    _sig(lib, "sol_read", C.c_int, [P, C.POINTER(C.c_float)])
    _sig(lib, "sol_render_aux", C.c_int, [P, C.c_uint32, C.c_uint32, C.c_uint64])
    _sig(lib, "sol_clear_aux", C.c_int, [P])
    _sig(lib, "sol_read_aux", C.c_int, [P, C.POINTER(C.c_float), C.POINTER(C.c_float)])
    _sig(lib, "sol_unpermute", C.c_int, [P, C.c_void_p, C.c_int, C.c_void_p])
    _sig(lib, "sol_tonemap_rgb8", C.c_int, [P, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint8)])
    _sig(lib, "sol_resolve_image", C.c_int, [P, C.POINTER(C.c_void_p)])
    _sig(lib, "sol_bloom", C.c_int, [P, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double])
    _sig(lib, "sol_bloom_rgb8", C.c_int, [P, C.c_void_p, C.c_uint32, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_uint8)])
    _sig(lib, "sol_gaussian_blur_weights", C.c_int, [C.c_uint32, C.c_double, C.POINTER(C.c_double)])
    _sig(lib, "sol_stats", C.c_int, [P, C.POINTER(SolStats)])
    _sig(lib, "sol_world_tree_check", C.c_int, [C.c_void_p, C.c_int, C.POINTER(SolTreeCheck)])
    _sig(lib, "sol_world_tree_check_ex", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t])
    _sig(lib, "sol_record_sizes", C.c_int, [C.POINTER(C.c_uint32)])
    _sig(lib, "sol_last_error", C.c_char_p, [])
    _sig(lib, "sol_debug_path", C.c_int, [P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32])
    _sig(lib, "sol_kernel_timing", C.c_int, [P, C.c_int])
    _sig(lib, "sol_last_kernel_ms", C.c_int, [P, C.POINTER(C.c_float), C.POINTER(C.c_uint32)])
    _sig(lib, "sol_eval", C.c_int, [C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32])
    _sig(lib, "sol_scene_create_ex", C.c_int, [C.POINTER(SolSceneDesc), C.c_int, C.POINTER(SolCreateOptions), C.POINTER(P)])
    _sig(lib, "sol_scene_build_times", C.c_int, [P, C.POINTER(C.c_double)])
    _sig(lib, "sol_scene_set_option", C.c_int, [P, C.c_int, C.c_int64])
    _sig(lib, "sol_background_blocks", C.c_int, [P, C.c_int, P, C.c_size_t, C.POINTER(C.c_uint32)])
    _sig(lib, "sol_scene_info", C.c_int, [P, C.POINTER(SolSceneInfo)])
    _sig(lib, "sol_path_stats", C.c_int, [P, C.POINTER(SolPathStats)])
    _sig(lib, "sol_comm_unique_id", C.c_int, [C.POINTER(C.c_uint8)])
    _sig(lib, "sol_comm_init", C.c_int, [P, C.c_int, C.c_int, C.POINTER(C.c_uint8)])
    _sig(lib, "sol_comm_destroy", C.c_int, [P])
    _sig(lib, "sol_gather", C.c_int, [P, C.c_void_p])
    _sig(lib, "sol_comm_self_check", C.c_int, [P])
    _sig(lib, "sol_gather_local", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)])
    _sig(lib, "sol_read_image", C.c_int, [P, C.POINTER(C.c_float)])
    _sig(lib, "sol_max_samples_per_call", C.c_uint32, [P])
    _sig(lib, "sol_adaptive_begin", C.c_int, [P, C.POINTER(SolAdaptive)])
    _sig(lib, "sol_adaptive_round", C.c_int, [P, C.c_uint64, C.POINTER(C.c_uint32)])
    _sig(lib, "sol_adaptive_counts", C.c_int, [P, C.POINTER(C.c_uint32), C.c_size_t])
    _sig(lib, "sol_tonemap_rgb8_adaptive", C.c_int, [P, C.c_void_p, C.POINTER(C.c_uint8)])
    _sig(lib, "sol_adaptive_rescale", C.c_int, [P, C.c_void_p])
    _sig(lib, "sol_env_sampling", C.c_int, [P, C.POINTER(SolEnvSampling)])
    _sig(lib, "sol_env_sampling_check", C.c_int, [C.c_void_p, C.POINTER(SolEnvSampling)])
    _sig(lib, "sol_env_tables", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_float)])
    _sig(lib, "sol_env_eval", C.c_int, [P, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])
    _sig(lib, "sol_light_sampling", C.c_int, [P, C.POINTER(SolLightSampling)])
    _sig(lib, "sol_light_sampling_check", C.c_int, [C.c_void_p, C.POINTER(SolLightSampling)])
    _sig(lib, "sol_light_weights", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t])
    _sig(lib, "sol_light_tables", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)])
    _sig(lib, "sol_light_tree", C.c_int, [P, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)])
    _sig(lib, "sol_light_eval", C.c_int, [P, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])
    _sig(lib, "sol_denoise_check", C.c_int, [C.POINTER(SolDenoise)])
    _sig(lib, "sol_resolve_aux", C.c_int, [P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)])
    _sig(lib, "sol_denoise", C.c_int, [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(SolDenoise)])
    _sig(lib, "sol_denoise_rgb8", C.c_int, [P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(SolDenoise),
                                            C.POINTER(C.c_uint8)])
    _sig(lib, "sol_query_dev", C.c_int, [P, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_query", C.c_int, [P, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_camera_rays", C.c_int, [P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p])
    _sig(lib, "sol_radiance_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolRadianceConfig), C.c_void_p])
    _sig(lib, "sol_radiance", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolRadianceConfig), C.c_void_p])
    _sig(lib, "sol_camera_ray_keys", C.c_int, [P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p])
    _sig(lib, "sol_irradiance_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_irradiance", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_irradiance_rays", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p, C.c_void_p])
    _sig(lib, "sol_irradiance_sh_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_irradiance_sh", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_visibility_dev", C.c_int, [P, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_visibility", C.c_int, [P, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_lightmap_points_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolLightmapConfig), C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_points", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolLightmapConfig), C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_dilate_dev", C.c_int, [P, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_dilate", C.c_int, [P, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_filter_dev", C.c_int, [P, C.POINTER(SolLightmapFilterConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_filter", C.c_int, [P, C.POINTER(SolLightmapFilterConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_irradiance_moments_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_irradiance_moments", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.c_void_p])
    _sig(lib, "sol_lightmap_filter_var_dev", C.c_int, [P, C.POINTER(SolLightmapFilterVarConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_filter_var", C.c_int, [P, C.POINTER(SolLightmapFilterVarConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_irradiance_adaptive_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.POINTER(SolGatherAdaptive),
                                                       C.c_void_p, C.POINTER(SolGatherAdaptiveStats)])
    _sig(lib, "sol_irradiance_adaptive", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.POINTER(SolGatherAdaptive),
                                                   C.c_void_p, C.POINTER(SolGatherAdaptiveStats)])
    _sig(lib, "sol_radiance_rescale_dev", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p])
    _sig(lib, "sol_radiance_rescale", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p])
    _sig(lib, "sol_lightmap_coords_dev", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_lightmap_coords", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_lightmap_sample_dev", C.c_int, [P, C.POINTER(SolLightmapSampleConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_lightmap_sample", C.c_int, [P, C.POINTER(SolLightmapSampleConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    for name in ("sol_lightmap_sh_dev", "sol_lightmap_sh"):
        _sig(lib, name, C.c_int, [P, C.POINTER(SolLightmapShConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_lightmap_normals_dev", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_lightmap_normals", C.c_int, [P, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_lightmap_mip_layout", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
    for name in ("sol_lightmap_mips_dev", "sol_lightmap_mips"):
        _sig(lib, name, C.c_int, [P, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
    for name in ("sol_lightmap_sample_lod_dev", "sol_lightmap_sample_lod"):
        _sig(lib, name, C.c_int, [P, C.POINTER(SolLightmapLodConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    for name in ("sol_lightmap_lod_dev", "sol_lightmap_lod"):
        _sig(lib, name, C.c_int, [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_float,
                                  C.c_float, C.c_void_p])
    for name in ("sol_lightmap_charts_dev", "sol_lightmap_charts"):
        _sig(lib, name, C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p])
    for name in ("sol_lightmap_dilate_charts_dev", "sol_lightmap_dilate_charts"):
        _sig(lib, name, C.c_int, [P, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_void_p])
    for name in ("sol_lightmap_sample_charts_dev", "sol_lightmap_sample_charts"):
        _sig(lib, name, C.c_int, [P, C.POINTER(SolLightmapSampleConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p])
    for name in ("sol_lightmap_chart_levels_dev", "sol_lightmap_chart_levels"):
        _sig(lib, name, C.c_int, [P, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_unwrap", C.c_int, [C.c_int, C.POINTER(SolUnwrapConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "sol_lightmap_unwrap_stage_ms", C.c_int, [C.POINTER(C.c_float)])
    _sig(lib, "sol_lightmap_unwrap_dev", C.c_int, [C.c_int, C.c_void_p, C.POINTER(SolUnwrapConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                   C.c_void_p])
    _sig(lib, "sol_volume_points_dev", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_float, C.c_float, C.c_void_p])
    _sig(lib, "sol_volume_points", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_float, C.c_float, C.c_void_p])
    _sig(lib, "sol_volume_build_dev", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p])
    _sig(lib, "sol_volume_build", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.c_void_p, C.c_float, C.c_void_p])
    _sig(lib, "sol_volume_sample_dev", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_volume_sample", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_visibility_oct_dev", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.POINTER(SolOctConfig), C.c_void_p])
    _sig(lib, "sol_visibility_oct", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SolIrradianceConfig), C.POINTER(SolOctConfig), C.c_void_p])
    _sig(lib, "sol_volume_build_depth_dev", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.POINTER(SolOctConfig), C.c_float, C.c_void_p])
    _sig(lib, "sol_volume_build_depth", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.POINTER(SolOctConfig), C.c_float, C.c_void_p])
    _sig(lib, "sol_volume_sample_depth_dev", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.c_void_p, C.POINTER(SolOctConfig), C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_volume_sample_depth", C.c_int, [P, C.POINTER(SolVolumeGrid), C.c_void_p, C.c_void_p, C.POINTER(SolOctConfig), C.c_void_p, C.c_size_t, C.c_void_p])
    _sig(lib, "sol_scene_set_camera", C.c_int, [P, C.POINTER(SolCamera), C.POINTER(SolCameraUpdate)])
    _sig(lib, "sol_scene_background_flags", C.c_int, [P, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)])
    _sig(lib, "sol_triangle_from_vertices", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SolTriangle)])
    _sig(lib, "sol_scene_set_triangles", C.c_int, [P, C.c_void_p, C.c_uint32, C.POINTER(SolGeometryUpdate)])
    _sig(lib, "sol_scene_set_triangles_dev", C.c_int, [P, C.c_void_p, C.c_uint32, C.POINTER(SolGeometryUpdate)])
    _sig(lib, "sol_scene_set_triangles_ms", C.c_int, [P, C.POINTER(C.c_float)])
    _sig(lib, "sol_scene_triangle_records", C.c_int, [P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)])
    _sig(lib, "sol_sphere_from_center", C.c_int, [C.c_void_p, C.c_double, C.POINTER(SolSphere)])
    _sig(lib, "sol_quad_from_corner", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SolQuad)])
    _sig(lib, "sol_scene_set_primitives", C.c_int, [P, C.POINTER(SolPrimitiveSet), C.POINTER(SolGeometryUpdate)])
    _sig(lib, "sol_scene_primitive_records", C.c_int, [P, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)])
    _libs["hip"] = lib
    return lib


HIP_SYMBOLS = ["sol_device_count", "sol_scene_create", "sol_scene_destroy", "sol_scene_set_partition",
               "sol_accum_floats", "sol_accum_ptr", "sol_scene_bind_accum", "sol_scene_set_stream", "sol_clear",
               "sol_render", "sol_render_counted", "sol_sync", "sol_read", "sol_unpermute", "sol_tonemap_rgb8",
               "sol_stats", "sol_record_sizes", "sol_last_error", "sol_eval", "sol_kernel_timing", "sol_last_kernel_ms",
               "sol_debug_path", "sol_resolve_image", "sol_bloom", "sol_bloom_rgb8", "sol_gaussian_blur_weights", "sol_world_tree_check", "sol_world_tree_check_ex", "sol_render_aux", "sol_clear_aux", "sol_read_aux",
               "sol_scene_create_ex", "sol_scene_build_times", "sol_scene_set_option", "sol_scene_info", "sol_path_stats", "sol_comm_unique_id", "sol_comm_init",
               "sol_comm_destroy", "sol_gather", "sol_gather_local", "sol_comm_self_check", "sol_read_image", "sol_max_samples_per_call", "sol_background_blocks",
               "sol_adaptive_begin", "sol_adaptive_round", "sol_adaptive_counts", "sol_tonemap_rgb8_adaptive", "sol_adaptive_rescale",
               "sol_env_sampling", "sol_env_sampling_check", "sol_env_tables", "sol_env_eval",
               "sol_light_sampling", "sol_light_sampling_check", "sol_light_weights", "sol_light_tables", "sol_light_tree", "sol_light_eval",
               "sol_denoise_check", "sol_resolve_aux", "sol_denoise", "sol_denoise_rgb8",
               "sol_query_dev", "sol_query", "sol_camera_rays", "sol_scene_set_camera", "sol_scene_background_flags",
               "sol_triangle_from_vertices", "sol_scene_set_triangles", "sol_scene_set_triangles_dev", "sol_scene_set_triangles_ms", "sol_scene_triangle_records",
               "sol_sphere_from_center", "sol_quad_from_corner", "sol_scene_set_primitives", "sol_scene_primitive_records",
               "sol_radiance_dev", "sol_radiance", "sol_camera_ray_keys", "sol_irradiance_dev", "sol_irradiance", "sol_irradiance_rays",
               "sol_irradiance_sh_dev", "sol_irradiance_sh", "sol_visibility_dev", "sol_visibility",
               "sol_lightmap_points_dev", "sol_lightmap_points", "sol_lightmap_dilate_dev", "sol_lightmap_dilate",
               "sol_lightmap_filter_dev", "sol_lightmap_filter",
               "sol_irradiance_moments_dev", "sol_irradiance_moments", "sol_lightmap_filter_var_dev", "sol_lightmap_filter_var",
               "sol_irradiance_adaptive_dev", "sol_irradiance_adaptive", "sol_radiance_rescale_dev", "sol_radiance_rescale",
               "sol_lightmap_coords_dev", "sol_lightmap_coords", "sol_lightmap_sample_dev", "sol_lightmap_sample",
               "sol_lightmap_sh_dev", "sol_lightmap_sh", "sol_lightmap_normals_dev", "sol_lightmap_normals",
               "sol_lightmap_mip_layout", "sol_lightmap_mips_dev", "sol_lightmap_mips", "sol_lightmap_sample_lod_dev", "sol_lightmap_sample_lod",
               "sol_lightmap_lod_dev", "sol_lightmap_lod",
               "sol_lightmap_charts_dev", "sol_lightmap_charts", "sol_lightmap_dilate_charts_dev", "sol_lightmap_dilate_charts",
               "sol_lightmap_sample_charts_dev", "sol_lightmap_sample_charts", "sol_lightmap_chart_levels_dev", "sol_lightmap_chart_levels",
               "sol_lightmap_unwrap_dev", "sol_lightmap_unwrap", "sol_lightmap_unwrap_stage_ms",
               "sol_volume_points_dev", "sol_volume_points", "sol_volume_build_dev", "sol_volume_build", "sol_volume_sample_dev", "sol_volume_sample",
               "sol_visibility_oct_dev", "sol_visibility_oct", "sol_volume_build_depth_dev", "sol_volume_build_depth", "sol_volume_sample_depth_dev",
               "sol_volume_sample_depth"]


def load_host():
    if "host" in _libs:
        return _libs["host"]
    load_hip()  # libsolstrale_host.so links against the device library (ray_trace)
    if not os.path.exists(HOST_LIB):
        raise RuntimeError(f"{HOST_LIB} is missing: run `python __graft_entry__.py build`")
    lib = C.CDLL(HOST_LIB)
    B = C.c_void_p
    I = C.c_int
    D = C.c_double
    _sig(lib, "solh_builder_new", B, [])
    _sig(lib, "solh_builder_free", None, [B])
    _sig(lib, "solh_last_error", C.c_char_p, [])
    _sig(lib, "solh_transform", I, [B, I, C.POINTER(C.c_int), _D3])
    _sig(lib, "solh_solid_color", I, [B, D, D, D])
    _sig(lib, "solh_image_map", I, [B, C.c_uint32, C.c_uint32, C.c_void_p])
    _sig(lib, "solh_normal_texture", I, [B, C.c_uint32, C.c_uint32, C.c_void_p])
    _sig(lib, "solh_lambertian", I, [B, I, I])
    _sig(lib, "solh_metal", I, [B, I, I, D])
    _sig(lib, "solh_dielectric", I, [B, I, I, D])
    _sig(lib, "solh_diffuse_light", I, [B, D, D, D, D])
    _sig(lib, "solh_blend", I, [B, I, I, D])
    _sig(lib, "solh_sphere", I, [B, _D3, D, I])
    _sig(lib, "solh_quad", I, [B, _D3, _D3, _D3, I, I])
    _sig(lib, "solh_box", I, [B, _D3, _D3, I, I])
    _sig(lib, "solh_triangle", I, [B, _D3, _D3, _D3, C.POINTER(C.c_float), I, I])
    _sig(lib, "solh_triangles", I, [B, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, I])
    _sig(lib, "solh_spheres", I, [B, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
    _sig(lib, "solh_constant_medium", I, [B, I, D, _D3])
    _sig(lib, "solh_bvh", I, [B, I, C.POINTER(C.c_int)])
    _sig(lib, "solh_bvh_range", I, [B, I, I])
    _sig(lib, "solh_finish", C.POINTER(SolSceneDesc),
         [B, I, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _D3, D, D, _D3, _D3, _D3])
    _sig(lib, "solh_camera", I, [C.c_uint32, C.c_uint32, D, D, _D3, _D3, _D3, C.POINTER(SolCamera)])
    _sig(lib, "solh_environment", I, [B, C.c_uint32, C.c_uint32, C.c_void_p, D])
    _sig(lib, "solh_tree_depth", C.c_uint32, [B])
    _sig(lib, "solh_ray_trace", I, [B, C.c_uint32, C.c_uint64, I, D, I, PROGRESS_FN, ABORT_FN, C.c_void_p])
    _sig(lib, "solh_ray_trace_devices", I, [B, C.c_uint32, C.c_uint64, I, D, I, C.POINTER(C.c_int), PROGRESS_FN, ABORT_FN, C.c_void_p])
    _sig(lib, "solh_load_obj", I, [B, C.c_char_p, C.c_char_p, I, I, IMAGE_DECODER_FN, C.c_void_p])
    _sig(lib, "solh_set_post_processors", I, [B, I, C.POINTER(C.c_int), C.POINTER(C.c_double)])
    _sig(lib, "solh_set_adaptive", I, [B, C.c_uint32, C.c_uint32, D])
    _sig(lib, "solh_set_env_sampling", I, [B, C.c_uint32])
    _sig(lib, "solh_set_light_sampling", I, [B, C.c_uint32])
    _sig(lib, "solh_abi_sizes", None, [C.POINTER(C.c_uint32)])
    _sig(lib, "solh_to_rgb_color", None, [_D3, C.c_uint32, C.POINTER(C.c_uint8)])
    _libs["host"] = lib
    return lib


HOST_SYMBOLS = ["solh_builder_new", "solh_builder_free", "solh_last_error", "solh_transform", "solh_solid_color",
                "solh_image_map", "solh_normal_texture", "solh_lambertian", "solh_metal", "solh_dielectric",
                "solh_diffuse_light", "solh_blend", "solh_sphere", "solh_quad", "solh_box", "solh_triangle",
                "solh_triangles", "solh_spheres", "solh_constant_medium", "solh_bvh", "solh_bvh_range", "solh_finish",
                "solh_tree_depth", "solh_environment", "solh_ray_trace", "solh_ray_trace_devices", "solh_abi_sizes", "solh_to_rgb_color", "solh_set_post_processors", "solh_load_obj",
                "solh_set_adaptive", "solh_set_env_sampling", "solh_set_light_sampling", "solh_camera"]


def d3(v):
    return (C.c_double * 3)(float(v[0]), float(v[1]), float(v[2]))
