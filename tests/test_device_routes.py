"""The Python binding's two routes, pinned without a device: a DeviceScene without a handle over a recording stand-in for the library. Every
array-taking wrapper is called on the host route (numpy arrays) and on the device route (tensors that say they are on the scene's device, with
torch's allocations kept on the CPU), and the recorded call is compared word for word: entry point, scalars, config bytes, which pointers are
null, whose memory the pointers name, the order of the stream waits, and the type, shape and dtype of the answer. The refusals - every argument of
every wrapper with a wrong extent, dtype, layout or device - must name the offender and reach no entry point; the inputs the wrappers leave to the
library to refuse must reach it."""
import ctypes as C
import types
from collections import namedtuple

import numpy as np
import pytest

from solstrale_amd import _abi
from solstrale_amd.device import (DEPTH_TEXEL_DTYPE, LIGHTMAP_TEXEL_DTYPE, MOMENTS_DTYPE, OCT_TEXEL_DTYPE, VOLUME_PROBE_DTYPE, DeviceScene, VolumeGrid)

torch = pytest.importorskip("torch")

F, U8, U32, I32 = np.float32, np.uint8, np.uint32, np.int32
TEXEL, HIT, VIS, PROBE = LIGHTMAP_TEXEL_DTYPE, DeviceScene.RAY_HIT_DTYPE, DeviceScene.VISIBILITY_DTYPE, VOLUME_PROBE_DTYPE
HANDLE = 0x5C3E0  # (what stands for the scene's handle: the first argument of every call)
W = H = 4  # the atlas
WH, T, N, RES = W * H, 2, 3, 4  # its texels; triangles; rows; the side of an octahedral map
GRID = VolumeGrid((0.0, 0.0, 0.0), 1.0, (2, 2, 2))
PROBES, OCT = 8, RES * RES
LEVELS = _abi.SOL_LIGHTMAP_MAX_LEVELS
INF = float("inf")


class Recorder:
    """Stands for the library: every attribute is a function that records (name, arguments) and answers SOL_OK. `peek`: {position: bytes} to
    read at the pointers of the next entry point while the call is in progress (the wrapper's own copies are still alive then)."""

    def __init__(self):
        self.calls, self.peek, self.seen = [], {}, {}

    def __getattr__(self, name):
        def call(*args):
            if name not in ("sol_sync", "sol_scene_destroy"):
                self.seen = {at: C.string_at(address(args[at]), n) for at, n in self.peek.items() if address(args[at])}
            self.calls.append((name, args))
            return 0
        return call

    def names(self):
        return [name for name, _ in self.calls]


def scene():
    ds = DeviceScene.__new__(DeviceScene)  # (no handle, no library, no device: tests/test_primitives_abi.py does the same)
    ds.h, ds.lib, ds.device, ds.width, ds.height = HANDLE, Recorder(), 0, 8, 8
    return ds


def address(x):
    return x.value if isinstance(x, C.c_void_p) else x


class OnDevice:
    """A CPU tensor that says it is on cuda:`index`: the wrappers' checks cannot tell, and nothing here dereferences the pointer on a device."""

    def __init__(self, t, index=0):
        self.t, self.is_cuda, self.device = t, True, types.SimpleNamespace(type="cuda", index=index)

    def __getattr__(self, name):
        return getattr(self.t, name)

    def reshape(self, *shape):
        return OnDevice(self.t.reshape(*shape), self.device.index)

    def cpu(self):
        return self.t


@pytest.fixture
def cpu_torch(monkeypatch):
    """torch's allocations stay on the CPU whatever device is asked for, and a wait for torch's stream is recorded instead: the device route runs
    to its end without a device. Returns the list the waits go to (set to a Recorder's `calls`)."""
    events = []
    empty, zeros, empty_like = torch.empty, torch.zeros, torch.empty_like
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: empty(*a, **k))
    monkeypatch.setattr(torch, "zeros", lambda *a, device=None, **k: zeros(*a, **k))
    monkeypatch.setattr(torch, "empty_like", lambda x, **k: empty_like(getattr(x, "t", x)))
    stream = types.SimpleNamespace(synchronize=lambda: events[0].append(("torch_wait", ())))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: stream)
    return events


# ---- the arrays -------------------------------------------------------------------------------------------------------------------------------
def seq(*shape, dtype=F):
    return (np.arange(int(np.prod(shape))) % 251 + 1).astype(dtype).reshape(shape)


def records(n, dtype):
    return (np.arange(n * dtype.itemsize // 4, dtype=U32) + 1).view(dtype)


def device_rows(a):
    """What the device route takes for the host array `a`: the words of a structured array as rows, unsigned words as int32."""
    if a.dtype.names:
        return np.ascontiguousarray(a).view(I32 if a.dtype in (TEXEL, HIT) else F).reshape(a.shape + (-1,))
    return a.view(I32) if a.dtype == U32 else a


def tensor(a, index=0):
    return OnDevice(torch.from_numpy(np.ascontiguousarray(device_rows(a))), index)


RAYS, KEYS = seq(N, 8), seq(N, 2, dtype=U32)
VERTICES, UVS, NORMALS = seq(T, 3, 3), seq(T, 3, 2), seq(T, 3, 3)
VALUES, VALUES28, POINTS16 = seq(WH, 4), seq(WH, 28), seq(WH, 8)
TEXELS, COORDS, HITS, MOMENTS = records(WH, TEXEL), records(N, TEXEL), records(N, HIT), records(WH, MOMENTS_DTYPE)
PASS_OF, PLANE, CHART_OF, TABLE = seq(H, W, dtype=U8), seq(H, W, dtype=U32), seq(T, dtype=U32), seq(5, dtype=U32)
NORMALS4, LODS, ROWS4 = seq(N, 4), seq(N), seq(N, 4)
MIPS, COVER = seq(5, 4), seq(5, dtype=U8)  # (a 4 x 4 atlas: levels of 2 x 2 and 1 x 1 texels)
SH, VISIBILITY, PROBE_ROWS = seq(PROBES, 28), records(PROBES, VIS), records(PROBES, PROBE)
OCT_ROWS, DEPTH_ROWS = seq(PROBES, OCT, 4), seq(PROBES, OCT, 2)
VERTICES64 = seq(T, 3, 3, dtype=np.float64)


def config(kind, **fields):
    return bytes(kind(size=C.sizeof(kind), **fields))


def gather_config(samples=2, first_sample=1, seed=7, key_base=5, first_draw=3, mode=_abi.SOL_IRRADIANCE_COSINE):
    return config(_abi.SolIrradianceConfig, samples=samples, first_sample=first_sample, first_draw=first_draw, seed=seed, key_base=key_base, mode=mode)


GATHER = dict(samples=2, first_sample=1, seed=7, key_base=5, first_draw=3)
SAMPLE_CFG = config(_abi.SolLightmapSampleConfig, width=W, height=H, channels=3, stride_bytes=16, flags=0, chart_radius=INF)
OCT_CFG = config(_abi.SolOctConfig, res=RES, sharpness_log2=5, reserved=0)
UPDATE = config(_abi.SolGeometryUpdate, flags=0)

# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
# args: {name: (host array, the extents of it that the wrapper pins)} in the order the wrapper checks them; the first decides the route.
# call(ds, a): the wrapper's call, `a` holding what is given of args by name (absent: None).
# want(a): the arguments after the handle - In(name): the pointer to that argument's words (None when it is absent), OUT: another pointer that is
# not null, bytes: a config struct by reference, anything else: a scalar.
# host / device: what comes back on either route as (shape, dtype) per array; other values are compared as they are.
Case = namedtuple("Case", "id args call entry want host device optional")
In = namedtuple("In", "name")
OUT = object()
CASES = []


def case(id, args, call, entry, want, host, device=None, optional=()):
    CASES.append(Case(id, args, call, entry, want, host, device, optional))


def gather(id, method, entry, cfg, host, device, extra_scalars=(), extra_configs=(), first="points", **kw):
    case(id, {first: (RAYS, (1,)), "keys": (KEYS, (0, 1))}, lambda ds, a: getattr(ds, method)(a[first], keys=a.get("keys"), **GATHER, **kw), entry,
         lambda a: [*extra_scalars, In(first), In("keys"), N, cfg, *extra_configs, OUT], host, device, optional=("keys",))


case("closest_hits", {"rays": (RAYS, (1,))}, lambda ds, a: ds.closest_hits(a["rays"]), "sol_query",
     lambda a: [_abi.SOL_QUERY_CLOSEST, In("rays"), N, OUT], ((N,), HIT), ((N, 8), torch.int32))
case("occluded", {"rays": (RAYS, (1,))}, lambda ds, a: ds.occluded(a["rays"]), "sol_query",
     lambda a: [_abi.SOL_QUERY_OCCLUDED, In("rays"), N, OUT], ((N,), U32), ((N,), torch.int32))
gather("radiance", "radiance", "sol_radiance", config(_abi.SolRadianceConfig, samples=2, first_sample=1, first_draw=3, seed=7, key_base=5),
       (((N, 3), F), ((N,), U32)), ((N, 4), torch.float32), first="rays")
gather("irradiance", "irradiance", "sol_irradiance", gather_config(), (((N, 3), F), ((N,), U32)), ((N, 4), torch.float32))
gather("irradiance_sh", "irradiance_sh", "sol_irradiance_sh", gather_config(mode=_abi.SOL_IRRADIANCE_SPHERE), (((N, 9, 3), F), ((N,), U32)),
       ((N, 28), torch.float32))
gather("visibility", "visibility", "sol_visibility", gather_config(), ((N,), VIS), ((N, 8), torch.float32), extra_scalars=(_abi.SOL_QUERY_OCCLUDED,))
gather("visibility_distances", "visibility", "sol_visibility", gather_config(), ((N,), VIS), ((N, 8), torch.float32),
       extra_scalars=(_abi.SOL_QUERY_CLOSEST,), distances=True)
gather("irradiance_moments", "irradiance_moments", "sol_irradiance_moments", gather_config(), ((N,), MOMENTS_DTYPE), ((N, 8), torch.float32))
gather("visibility_oct", "visibility_oct", "sol_visibility_oct", gather_config(mode=_abi.SOL_IRRADIANCE_SPHERE), ((N, OCT, 4), F),
       ((N, OCT, 4), torch.float32), extra_configs=(OCT_CFG,), res=RES)
case("irradiance_adaptive", {"points": (RAYS, (1,)), "keys": (KEYS, (0, 1))},
     lambda ds, a: ds.irradiance_adaptive(a["points"], 64, round=16, min_samples=32, threshold=0.25, floor=0.5, first_sample=1, seed=7, keys=a.get("keys"),
                                          key_base=5, first_draw=3), "sol_irradiance_adaptive",
     lambda a: [In("points"), In("keys"), N, gather_config(samples=64), config(_abi.SolGatherAdaptive, round=16, min_samples=32, threshold=0.25, floor=0.5), OUT,
                config(_abi.SolGatherAdaptiveStats)], ((N,), MOMENTS_DTYPE), ((N, 8), torch.float32), optional=("keys",))
case("lightmap_points", {"vertices": (VERTICES, (1, 2)), "uvs": (UVS, (0, 1, 2)), "normals": (NORMALS, (0, 1, 2))},
     lambda ds, a: ds.lightmap_points(a["vertices"], a["uvs"], W, H, normals=a.get("normals"), tmin=0.5, tmax=2.0, conservative=True), "sol_lightmap_points",
     lambda a: [In("vertices"), In("normals"), In("uvs"), T,
                config(_abi.SolLightmapConfig, width=W, height=H, flags=_abi.SOL_LIGHTMAP_CONSERVATIVE, tmin=0.5, tmax=2.0), OUT, OUT],
     (((WH, 8), F), ((WH,), TEXEL)), (((WH, 8), torch.float32), ((WH, 4), torch.int32)), optional=("normals",))
case("lightmap_dilate", {"values": (VALUES, (0,)), "texels": (TEXELS, (0,))}, lambda ds, a: ds.lightmap_dilate(a["values"], a["texels"], W, H, passes=2, channels=3),
     "sol_lightmap_dilate", lambda a: [In("texels"), W, H, In("values"), 3, 16, 2, OUT, None], ((WH, 4), F), ((WH, 4), torch.float32))
case("lightmap_dilate_pass_of", {"values": (VALUES, (0,)), "texels": (TEXELS, (0,))},
     lambda ds, a: ds.lightmap_dilate(a["values"], a["texels"], W, H, return_pass_of=True), "sol_lightmap_dilate",
     lambda a: [In("texels"), W, H, In("values"), 3, 16, 1, OUT, OUT], (((WH, 4), F), ((H, W), U8)), (((WH, 4), torch.float32), ((H, W), torch.uint8)))
case("lightmap_filter", {"values": (VALUES, (0,)), "points": (POINTS16, (0, 1)), "texels": (TEXELS, (0,))},
     lambda ds, a: ds.lightmap_filter(a["values"], a["points"], a["texels"], W, H, 0.5, sigma_plane=0.25, iterations=3, normal_power_log2=4, sigma_value=0.75,
                                      value_scale=2.0), "sol_lightmap_filter",
     lambda a: [config(_abi.SolLightmapFilterConfig, width=W, height=H, iterations=3, normal_power_log2=4, channels=3, stride_bytes=16, sigma_position=0.5,
                       sigma_plane=0.25, sigma_value=0.75, value_scale=2.0), In("points"), In("texels"), In("values"), OUT], ((WH, 4), F), ((WH, 4), torch.float32))
FILTER_VAR_CFG = config(_abi.SolLightmapFilterVarConfig, width=W, height=H, iterations=4, normal_power_log2=5, sigma_position=0.5, sigma_plane=0.5, sigma_value=4.0,
                        variance_floor=1e-12)
for id, flag, out, host, device in (("lightmap_filter_var", False, None, ((WH, 4), F), ((WH, 4), torch.float32)),
                                    ("lightmap_filter_var_variance", True, OUT, (((WH, 4), F),) * 2, (((WH, 4), torch.float32),) * 2)):
    case(id, {"moments": (MOMENTS, (0,)), "points": (POINTS16, (0, 1)), "texels": (TEXELS, (0,))},
         lambda ds, a, flag=flag: ds.lightmap_filter_var(a["moments"], a["points"], a["texels"], W, H, 0.5, return_variance=flag), "sol_lightmap_filter_var",
         lambda a, out=out: [FILTER_VAR_CFG, In("points"), In("texels"), In("moments"), OUT, out], host, device)
case("radiance_rescale", {"rows": (ROWS4, (1,))}, lambda ds, a: ds.radiance_rescale(a["rows"], 8), "sol_radiance_rescale", lambda a: [In("rows"), N, 8, OUT],
     ((N, 4), F), ((N, 4), torch.float32))
case("lightmap_coords", {"hits": (HITS, ()), "triangle_of_dfs": (TABLE, None)}, lambda ds, a: ds.lightmap_coords(a["hits"], a["triangle_of_dfs"]),
     "sol_lightmap_coords", lambda a: [In("hits"), N, In("triangle_of_dfs"), 5, OUT], ((N,), TEXEL), ((N, 4), torch.int32))
SAMPLE_ARGS = {"values": (VALUES, (0,)), "coords": (COORDS, ()), "uvs": (UVS, (1, 2)), "texels": (TEXELS, (0,)), "pass_of": (PASS_OF, (0, 1)),
               "vertices": (VERTICES, (0, 1, 2)), "points": (POINTS16, (0, 1))}
# (the device route checks uvs first: what pins the triangles of `vertices` comes before it in both)
SAMPLE_ARGS = {k: SAMPLE_ARGS[k] for k in ("values", "uvs", "texels", "pass_of", "vertices", "points", "coords")}
case("lightmap_sample", SAMPLE_ARGS,
     lambda ds, a: ds.lightmap_sample(a["values"], a["coords"], a["uvs"], a["texels"], W, H, pass_of=a.get("pass_of"), vertices=a.get("vertices"),
                                      points=a.get("points")), "sol_lightmap_sample",
     lambda a: [SAMPLE_CFG, In("uvs"), T, In("texels"), In("pass_of"), In("values"), In("vertices"), In("points"), In("coords"), N, OUT], ((N, 4), F),
     ((N, 4), torch.float32), optional=("pass_of", "vertices", "points"))
SH_ARGS = {**SAMPLE_ARGS, "values": (VALUES28, (0,)), "normals": (NORMALS4, (0, 1))}
case("lightmap_sh", SH_ARGS,
     lambda ds, a: ds.lightmap_sh(a["values"], a["coords"], a["normals"], a["uvs"], a["texels"], W, H, scale=0.5, pass_of=a.get("pass_of"), nearest=True,
                                  chart_radius=1.5, vertices=a.get("vertices"), points=a.get("points"), clamp=True), "sol_lightmap_sh",
     lambda a: [config(_abi.SolLightmapShConfig, width=W, height=H, stride_bytes=112, flags=_abi.SOL_LIGHTMAP_SH_NEAREST | _abi.SOL_LIGHTMAP_SH_CLAMP, chart_radius=1.5,
                       scale=0.5), In("uvs"), T, In("texels"), In("pass_of"), In("values"), In("vertices"), In("points"), In("coords"), In("normals"), N, OUT],
     ((N, 4), F), ((N, 4), torch.float32), optional=("pass_of", "vertices", "points"))
case("lightmap_sh_coefficients", {k: v for k, v in SH_ARGS.items() if k in ("values", "uvs", "texels", "coords")},
     lambda ds, a: ds.lightmap_sh(a["values"], a["coords"], None, a["uvs"], a["texels"], W, H, coefficients=True), "sol_lightmap_sh",
     lambda a: [config(_abi.SolLightmapShConfig, width=W, height=H, stride_bytes=112, flags=_abi.SOL_LIGHTMAP_SH_COEFFICIENTS, chart_radius=INF, scale=1.0),
                In("uvs"), T, In("texels"), None, In("values"), None, None, In("coords"), None, N, OUT], ((N, 28), F), ((N, 28), torch.float32))
case("lightmap_normals", {"coords": (COORDS, ()), "vertices": (VERTICES, (1, 2)), "normals": (NORMALS, (0, 1, 2))},
     lambda ds, a: ds.lightmap_normals(a["coords"], a["vertices"], a.get("normals")), "sol_lightmap_normals",
     lambda a: [In("coords"), N, In("vertices"), In("normals"), T, OUT], ((N, 4), F), ((N, 4), torch.float32), optional=("normals",))
case("lightmap_mips", {"values": (VALUES, (0,)), "texels": (TEXELS, (0,)), "pass_of": (PASS_OF, (0, 1))},
     lambda ds, a: ds.lightmap_mips(a["values"], a["texels"], W, H, pass_of=a.get("pass_of")), "sol_lightmap_mips",
     lambda a: [In("texels"), In("pass_of"), W, H, In("values"), 3, 16, 3, OUT, OUT], (((5, 4), F), ((5,), U8)), (((5, 4), torch.float32), ((5,), torch.uint8)),
     optional=("pass_of",))
case("lightmap_mips_one_level", {"values": (VALUES, (0,)), "texels": (TEXELS, (0,))}, lambda ds, a: ds.lightmap_mips(a["values"], a["texels"], W, H, levels=1),
     "sol_lightmap_mips", lambda a: [In("texels"), None, W, H, In("values"), 3, 16, 1, None, None], (((0, 4), F), ((0,), U8)),
     (((0, 4), torch.float32), ((0,), torch.uint8)))
LOD_ARGS = {"values": (VALUES, (0,)), "uvs": (UVS, (1, 2)), "texels": (TEXELS, (0,)), "pass_of": (PASS_OF, (0, 1)), "mips": (MIPS, (0, 1)), "cover": (COVER, (0,)),
            "vertices": (VERTICES, (0, 1, 2)), "points": (POINTS16, (0, 1)), "coords": (COORDS, ()), "lods": (LODS, (0,))}


def lod_config(levels):
    return config(_abi.SolLightmapLodConfig, width=W, height=H, channels=3, stride_bytes=16, flags=0, chart_radius=INF, levels=levels)


case("lightmap_sample_lod", LOD_ARGS,
     lambda ds, a: ds.lightmap_sample_lod(a["values"], a["mips"], a["cover"], a["lods"], a["coords"], a["uvs"], a["texels"], W, H, pass_of=a.get("pass_of"),
                                          vertices=a.get("vertices"), points=a.get("points")), "sol_lightmap_sample_lod",
     lambda a: [lod_config(3), In("uvs"), T, In("texels"), In("pass_of"), In("values"), In("mips"), In("cover"), In("vertices"), In("points"), In("coords"),
                In("lods"), N, OUT], ((N, 4), F), ((N, 4), torch.float32), optional=("pass_of", "vertices", "points"))
case("lightmap_sample_lod_one_level", {k: v for k, v in LOD_ARGS.items() if k in ("values", "uvs", "texels", "coords", "lods")},
     lambda ds, a: ds.lightmap_sample_lod(a["values"], None, None, a["lods"], a["coords"], a["uvs"], a["texels"], W, H, levels=1), "sol_lightmap_sample_lod",
     lambda a: [lod_config(1), In("uvs"), T, In("texels"), None, In("values"), None, None, None, None, In("coords"), In("lods"), N, OUT], ((N, 4), F),
     ((N, 4), torch.float32))
case("lightmap_lod", {"rays": (RAYS, (1,)), "hits": (HITS, (0,)), "coords": (COORDS, (0,)), "vertices": (VERTICES, (1, 2)), "uvs": (UVS, (0, 1, 2))},
     lambda ds, a: ds.lightmap_lod(a["rays"], a["hits"], a["coords"], a["vertices"], a["uvs"], W, H, 0.125, bias=0.5), "sol_lightmap_lod",
     lambda a: [In("rays"), In("hits"), In("coords"), N, In("vertices"), In("uvs"), T, W, H, 0.125, 0.5, OUT], ((N,), F), ((N,), torch.float32))
case("lightmap_charts", {"uvs": (UVS, (1, 2)), "vertices": (VERTICES, (0, 1, 2))}, lambda ds, a: ds.lightmap_charts(a["uvs"], a.get("vertices")), "sol_lightmap_charts",
     lambda a: [In("uvs"), In("vertices"), T, OUT, OUT], (((T,), U32), 0), (((T,), torch.int32), 0), optional=("vertices",))
case("lightmap_dilate_charts", {"values": (VALUES, (0,)), "texels": (TEXELS, (0,)), "chart_of_triangle": (CHART_OF, None)},
     lambda ds, a: ds.lightmap_dilate_charts(a["values"], a["texels"], a["chart_of_triangle"], W, H, passes=2), "sol_lightmap_dilate_charts",
     lambda a: [In("texels"), W, H, In("values"), 3, 16, 2, In("chart_of_triangle"), T, OUT, OUT, OUT], (((WH, 4), F), ((H, W), U8), ((H, W), U32)),
     (((WH, 4), torch.float32), ((H, W), torch.uint8), ((H, W), torch.int32)))
case("lightmap_sample_charts", {"values": (VALUES, (0,)), "uvs": (UVS, (1, 2)), "texels": (TEXELS, (0,)), "pass_of": (PASS_OF, (0, 1)),
                                "chart_of_triangle": (CHART_OF, (0,)), "chart_plane": (PLANE, (0, 1)), "coords": (COORDS, ())},
     lambda ds, a: ds.lightmap_sample_charts(a["values"], a["coords"], a["uvs"], a["texels"], a["chart_of_triangle"], a["chart_plane"], W, H, pass_of=a.get("pass_of")),
     "sol_lightmap_sample_charts",
     lambda a: [SAMPLE_CFG, In("uvs"), T, In("texels"), In("pass_of"), In("values"), In("chart_of_triangle"), In("chart_plane"), In("coords"), N, OUT], ((N, 4), F),
     ((N, 4), torch.float32), optional=("pass_of",))
case("lightmap_chart_levels", {"chart_plane": (PLANE, (0, 1)), "pass_of": (PASS_OF, (0, 1))},
     lambda ds, a: ds.lightmap_chart_levels(a["chart_plane"], W, H, a.get("pass_of")), "sol_lightmap_chart_levels",
     lambda a: [In("chart_plane"), In("pass_of"), W, H, OUT, OUT, OUT], (0, ((LEVELS,), U32), ((LEVELS,), U32)), (0, ((LEVELS,), U32), ((LEVELS,), U32)),
     optional=("pass_of",))
GRID_RECORD = bytes(GRID.record())
case("volume_build", {"sh": (SH, (0, 1)), "visibility": (VISIBILITY, (0,))}, lambda ds, a: ds.volume_build(GRID, a["sh"], a.get("visibility"), radius=2.5),
     "sol_volume_build", lambda a: [GRID_RECORD, In("sh"), In("visibility"), 2.5, OUT], ((PROBES,), PROBE), ((PROBES, 32), torch.float32), optional=("visibility",))
case("volume_sample", {"points": (RAYS, (1,)), "probes": (PROBE_ROWS, (0,))}, lambda ds, a: ds.volume_sample(GRID, a["probes"], a["points"]), "sol_volume_sample",
     lambda a: [GRID_RECORD, In("probes"), In("points"), N, OUT], (((N, 3), F), ((N,), U32)), ((N, 4), torch.float32))
case("volume_build_depth", {"oct": (OCT_ROWS, (0,))}, lambda ds, a: ds.volume_build_depth(GRID, a["oct"], 2.5, res=RES), "sol_volume_build_depth",
     lambda a: [GRID_RECORD, In("oct"), OCT_CFG, 2.5, OUT], ((PROBES, OCT, 2), F), ((PROBES, OCT, 2), torch.float32))
case("volume_sample_depth", {"points": (RAYS, (1,)), "probes": (PROBE_ROWS, (0,)), "depth": (DEPTH_ROWS, (0,))},
     lambda ds, a: ds.volume_sample(GRID, a["probes"], a["points"], depth=a["depth"], res=RES), "sol_volume_sample_depth",
     lambda a: [GRID_RECORD, In("probes"), In("depth"), config(_abi.SolOctConfig, res=RES, sharpness_log2=0, reserved=0), In("points"), N, OUT],
     (((N, 3), F), ((N,), U32)), ((N, 4), torch.float32))
case("set_triangles", {"vertices": (VERTICES64, (1, 2))}, lambda ds, a: ds.set_triangles(a["vertices"]), "sol_scene_set_triangles",
     lambda a: [In("vertices"), T, UPDATE], None, None)

BY_ID = {c.id: c for c in CASES}
IDS = list(BY_ID)


def given_sets(c):
    """Every optional argument once present and once absent: all of them, none of them, and each alone."""
    names = list(c.args)
    sets = [names, [n for n in names if n not in c.optional]] + [[n for n in names if n not in c.optional or n == o] for o in c.optional]
    return [s for k, s in enumerate(sets) if s not in sets[:k]]


def same_argument(got, want):
    if want is None:
        return got is None
    if want is OUT or isinstance(want, In):
        return isinstance(got, (int, C.c_void_p)) and bool(address(got))
    if isinstance(want, bytes):
        return bytes(got._obj) == want
    return not isinstance(got, C.c_void_p) and type(got) in (int, float) and got == want


def check_call(ds, c, given, host):
    """Calls the wrapper with the arguments `given` of the case on one route and compares what the library was handed."""
    arrays = {name: c.args[name][0] for name in given}
    a = arrays if host else {name: tensor(x) for name, x in arrays.items()}
    want = [w if not isinstance(w, In) or w.name in given else None for w in c.want(a)]
    inputs = {at + 1: arrays[w.name] for at, w in enumerate(want) if isinstance(w, In)}
    ds.lib.calls.clear()
    ds.lib.peek = {at: x.nbytes for at, x in inputs.items()}
    got = c.call(ds, a)
    entry = [(name, args) for name, args in ds.lib.calls if name not in ("sol_sync", "torch_wait")]
    assert [name for name, _ in entry] == [c.entry + ("" if host else "_dev")]
    args = entry[0][1]
    assert args[0] == HANDLE and len(args) == 1 + len(want), args
    for at, w in enumerate(want):
        assert same_argument(args[at + 1], w), (c.id, "argument", at + 1, args[at + 1], w)
    for at, x in inputs.items():  # (the words at the pointer are the caller's, and on the device route so is the address)
        assert ds.lib.seen[at] == x.tobytes(), (c.id, "the words of argument", at)
        assert host or address(args[at]) == a[want[at - 1].name].data_ptr()
    return got


def check_answer(got, want, kind):
    if want is None or isinstance(want, int):
        assert got == want and type(got) is type(want)
    elif not (len(want) == 2 and all(isinstance(n, int) for n in want[0]) and not isinstance(want[1], (tuple, int))):  # (several answers)
        assert isinstance(got, tuple) and len(got) == len(want)
        for g, w in zip(got, want):
            check_answer(g, w, kind)
    else:
        kind = np.ndarray if isinstance(want[1], (np.dtype, type)) else kind
        assert isinstance(got, kind) and tuple(got.shape) == want[0] and got.dtype == want[1], (type(got), got.shape, got.dtype, want)


# ---- (a) the host route -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", IDS)
def test_host_route_hands_the_library_the_callers_arrays(id):
    c, ds = BY_ID[id], scene()
    for given in given_sets(c):
        check_answer(check_call(ds, c, given, host=True), c.host, np.ndarray)
        assert ds.lib.names() == [c.entry]  # (no wait: nothing is on a stream)


def test_host_route_takes_rows_tensors_and_pairs_for_the_structured_arrays():
    """The host side of the layout table: the raw rows of a record, a tensor brought over, irradiance_sh's (sums, counts)."""
    ds = scene()
    on_cpu = {name: torch.from_numpy(device_rows(x)) for name, x in (("texels", TEXELS), ("coords", COORDS), ("points", POINTS16), ("uvs", UVS))}
    ds.lib.peek = {4: TEXELS.nbytes, 9: COORDS.nbytes}
    out = ds.lightmap_sample(VALUES, on_cpu["coords"], on_cpu["uvs"], on_cpu["texels"], W, H, points=on_cpu["points"], vertices=VERTICES)
    assert ds.lib.names() == ["sol_lightmap_sample"] and ds.lib.seen == {4: TEXELS.tobytes(), 9: COORDS.tobytes()} and out.shape == (N, 4)
    for moments in (MOMENTS, device_rows(MOMENTS)):
        ds.lib.calls.clear()
        ds.lib.peek = {4: MOMENTS.nbytes}
        ds.lightmap_filter_var(moments, POINTS16, TEXELS, W, H, 0.5)
        assert ds.lib.names() == ["sol_lightmap_filter_var"] and ds.lib.seen == {4: MOMENTS.tobytes()}
    sums, counts = seq(PROBES, 9, 3), seq(PROBES, dtype=U32)
    rows = np.concatenate([sums.reshape(PROBES, 27), counts.view(F).reshape(PROBES, 1)], axis=1)
    for sh, vis, probes in (((sums, counts), device_rows(VISIBILITY), device_rows(PROBE_ROWS)), ([sums, counts], VISIBILITY, PROBE_ROWS)):
        ds.lib.calls.clear()
        ds.lib.peek = {2: rows.nbytes, 3: VISIBILITY.nbytes}
        assert ds.volume_build(GRID, sh, vis, radius=1.0).dtype == PROBE
        assert ds.lib.seen == {2: rows.tobytes(), 3: VISIBILITY.tobytes()}
        ds.lib.peek = {2: PROBE_ROWS.nbytes}
        ds.volume_sample(GRID, probes, RAYS)
        assert ds.lib.seen == {2: PROBE_ROWS.tobytes()}
    for oct, depth in ((OCT_ROWS, DEPTH_ROWS), (OCT_ROWS.view(OCT_TEXEL_DTYPE), DEPTH_ROWS.view(DEPTH_TEXEL_DTYPE)), (OCT_ROWS.reshape(-1), DEPTH_ROWS.reshape(-1, 2))):
        ds.lib.peek = {2: OCT_ROWS.nbytes}
        assert ds.volume_build_depth(GRID, oct, 1.0, res=RES).shape == (PROBES, OCT, 2) and ds.lib.seen == {2: OCT_ROWS.tobytes()}
        ds.lib.peek = {3: DEPTH_ROWS.nbytes}
        ds.volume_sample(GRID, PROBE_ROWS, RAYS, depth=depth, res=RES)
        assert ds.lib.seen == {3: DEPTH_ROWS.tobytes()}
    ds.lib.peek = {2: KEYS.nbytes}
    ds.radiance(RAYS.tolist(), keys=KEYS.astype(np.int64))  # (lists and other integers are converted)
    assert ds.lib.seen == {2: KEYS.tobytes()}
    ds.lib.peek = {3: TABLE.nbytes}
    ds.lightmap_coords(HITS, TABLE.astype(np.int64))
    assert ds.lib.seen == {3: TABLE.tobytes()}
    ds.lib.peek = {8: CHART_OF.nbytes}
    ds.lightmap_dilate_charts(VALUES, TEXELS, CHART_OF.view(I32), W, H)  # (int32 holds the same words)
    assert ds.lib.seen == {8: CHART_OF.tobytes()}
    ds.lib.peek = {2: PASS_OF.nbytes}
    ds.lightmap_mips(VALUES, TEXELS, W, H, pass_of=PASS_OF.reshape(-1))  # (a plane is taken by its size on this route)
    assert ds.lib.seen == {2: PASS_OF.tobytes()}


def test_empty_arrays_go_as_null_pointers():
    """Zero triangles, an empty table, no labels: the pointer is null and the count 0, on the host route."""
    ds, none3, none2 = scene(), np.zeros((0, 3, 3), dtype=F), np.zeros((0, 3, 2), dtype=F)

    def last():
        name, args = ds.lib.calls[-1]
        return name, [None if a is None else "p" if isinstance(a, int) and a > 4096 else a for a in args[1:] if not hasattr(a, "_obj")]
    ds.lightmap_sample(VALUES, COORDS, none2, TEXELS, W, H)
    assert last() == ("sol_lightmap_sample", [None, 0, "p", None, "p", None, None, "p", N, "p"])
    ds.lightmap_sample(VALUES, COORDS, none2, TEXELS, W, H, vertices=none3)
    assert last()[1][5] == "p"  # (only uvs goes null: the library reads no vertex of no triangle)
    ds.lightmap_sample_charts(VALUES, COORDS, none2, TEXELS, np.zeros(0, dtype=U32), PLANE, W, H)
    assert last() == ("sol_lightmap_sample_charts", [None, 0, "p", None, "p", None, "p", "p", N, "p"])
    ds.lightmap_normals(COORDS, none3, none3)
    assert last() == ("sol_lightmap_normals", ["p", N, None, None, 0, "p"])
    ds.lightmap_lod(RAYS, HITS, COORDS, none3, none2, W, H, 0.125)
    assert last() == ("sol_lightmap_lod", ["p", "p", "p", N, None, None, 0, W, H, 0.125, 0.0, "p"])
    chart_of, n = ds.lightmap_charts(none2, none3)
    assert last() == ("sol_lightmap_charts", [None, None, 0, None, "p"]) and chart_of.shape == (0,) and chart_of.dtype == U32 and n == 0
    ds.lightmap_coords(HITS, np.zeros(0, dtype=U32))
    assert last() == ("sol_lightmap_coords", ["p", N, None, 0, "p"])
    for labels in (None, np.zeros(0, dtype=U32)):
        ds.lightmap_dilate_charts(VALUES, TEXELS, labels, W, H)
        assert last() == ("sol_lightmap_dilate_charts", ["p", W, H, "p", 3, 16, 1, None, 0, "p", "p", "p"])
    ds.lightmap_sample(np.zeros((0, 4), dtype=F), COORDS[:0], UVS, TEXELS[:0], 0, 0)  # (no atlas and no rows: the rest is the library's to refuse)
    assert last()[0] == "sol_lightmap_sample" and last()[1][8] == 0


def test_radiance_rescale_in_place_hands_the_rows_back(cpu_torch):
    ds = scene()
    cpu_torch.append(ds.lib.calls)
    rows = ROWS4.copy()
    assert ds.radiance_rescale(rows, 8, in_place=True) is rows
    (name, args), = ds.lib.calls
    assert name == "sol_radiance_rescale" and args[1] == args[4] == rows.ctypes.data
    for bad in (ROWS4.astype(np.float64), ROWS4[:, ::-1], ROWS4.tolist()):
        with pytest.raises(ValueError, match="rows"):
            ds.radiance_rescale(bad, 8, in_place=True)
    d_rows = tensor(ROWS4)
    ds.lib.calls.clear()
    assert ds.radiance_rescale(d_rows, 8, in_place=True) is d_rows
    assert ds.lib.names() == ["torch_wait", "sol_radiance_rescale_dev", "sol_sync"]
    args = ds.lib.calls[1][1]
    assert address(args[1]) == address(args[4]) == d_rows.data_ptr()


def test_volume_points_takes_no_array_and_waits_for_no_tensor(cpu_torch):
    ds = scene()
    cpu_torch.append(ds.lib.calls)
    out = ds.volume_points(GRID, tmin=0.5, tmax=2.0, host=True)
    (name, args), = ds.lib.calls
    assert name == "sol_volume_points" and bytes(args[1]._obj) == GRID_RECORD and args[2:4] == (0.5, 2.0) and args[4] == out.ctypes.data
    assert isinstance(out, np.ndarray) and out.shape == (PROBES, 8) and out.dtype == F
    ds.lib.calls.clear()
    out = ds.volume_points(GRID, tmin=0.5, tmax=2.0)
    assert ds.lib.names() == ["sol_volume_points_dev", "sol_sync"]  # (no input is a tensor: torch's stream is not waited for)
    args = ds.lib.calls[0][1]
    assert bytes(args[1]._obj) == GRID_RECORD and args[2:4] == (0.5, 2.0) and address(args[4]) == out.data_ptr()
    assert tuple(out.shape) == (PROBES, 8) and out.dtype == torch.float32


def primitive_set(ds):
    (name, args), = ds.lib.calls
    assert name == "sol_scene_set_primitives" and args[0] == HANDLE and bytes(args[2]._obj) == UPDATE
    return args[1]._obj


def test_set_primitives_hands_over_every_kind_it_is_given(cpu_torch):
    ds = scene()
    cpu_torch.append(ds.lib.calls)
    spheres, quads = seq(2, 4, dtype=np.float64), seq(1, 3, 3, dtype=np.float64)
    ds.set_primitives(triangles=VERTICES64, spheres=spheres, quads=quads)
    ps = primitive_set(ds)
    assert (ps.flags, ps.n_triangles, ps.n_spheres, ps.n_quads) == (0, T, 2, 1)
    assert (ps.triangles, ps.spheres, ps.quads) == (VERTICES64.ctypes.data, spheres.ctypes.data, quads.ctypes.data)
    ds.lib.calls.clear()
    ds.set_primitives(spheres=np.zeros((0, 4)), background_proof=False, reprobe=True)
    (name, args), = ds.lib.calls
    assert bytes(args[2]._obj) == config(_abi.SolGeometryUpdate, flags=_abi.SOL_GEOM_NO_BACKGROUND_PROOF | _abi.SOL_GEOM_REPROBE)
    ps = args[1]._obj
    assert ps.spheres and ps.n_spheres == 0 and not ps.triangles and not ps.quads  # (an empty kind is given all the same: its pointer is not null)
    ds.lib.calls.clear()
    d_spheres, d_quads = tensor(spheres), tensor(quads)
    ds.set_primitives(spheres=d_spheres, quads=d_quads)
    assert ds.lib.names()[-1] == "sol_scene_set_primitives" and set(ds.lib.names()[:-1]) == {"torch_wait"}  # (the call blocks: no wait after it)
    ps = ds.lib.calls[-1][1][1]._obj
    assert (ps.flags, ps.spheres, ps.quads, ps.n_spheres, ps.n_quads) == (_abi.SOL_PRIMS_DEVICE, d_spheres.data_ptr(), d_quads.data_ptr(), 2, 1)
    ds.lib.calls.clear()
    with pytest.raises(ValueError, match="one call"):
        ds.set_primitives(spheres=d_spheres, quads=quads)
    with pytest.raises(ValueError, match="set_primitives"):
        ds.set_primitives()
    for kind, bad in (("triangles", np.zeros((2, 9))), ("spheres", np.zeros((2, 3))), ("quads", np.zeros((3, 3)))):
        with pytest.raises(ValueError, match=f"^{kind}:"):
            ds.set_primitives(**{kind: bad})
        for d_bad in (torch.from_numpy(spheres if kind == "spheres" else quads), tensor(bad), tensor(spheres.astype(F) if kind == "spheres" else quads.astype(F)),
                      tensor(spheres if kind == "spheres" else quads, index=1)):
            with pytest.raises(ValueError, match=f"^{kind}:"):
                ds.set_primitives(**{kind: d_bad})
    assert ds.lib.calls == []


# ---- the device route -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id", [id for id in IDS])
def test_device_route_hands_the_library_the_callers_tensors_between_two_waits(id, cpu_torch):
    c, ds = BY_ID[id], scene()
    cpu_torch.append(ds.lib.calls)
    for given in given_sets(c):
        got = check_call(ds, c, given, host=False)
        check_answer(got, c.device, torch.Tensor)
        blocks = c.id == "set_triangles"  # (the move blocks by itself: the scene's stream is not waited for)
        assert ds.lib.names() == ["torch_wait", c.entry + "_dev"] + ([] if blocks else ["sol_sync"])


def test_device_route_takes_no_labels_as_the_host_route_does(cpu_torch):
    """lightmap_dilate_charts(chart_of_triangle=None): a null table of 0 labels on either route. (New with the shared call path: the device route
    used to end in an AttributeError.)"""
    ds = scene()
    cpu_torch.append(ds.lib.calls)
    out, pass_of, plane = ds.lightmap_dilate_charts(tensor(VALUES), tensor(TEXELS), None, W, H)
    args = ds.lib.calls[1][1]
    assert ds.lib.names() == ["torch_wait", "sol_lightmap_dilate_charts_dev", "sol_sync"] and args[8] is None and args[9] == 0
    assert tuple(plane.shape) == (H, W) and plane.dtype == torch.int32


def wrong(a, kind, dim=None):
    """`a` with one thing wrong for the device route."""
    if kind == "host":  # (a tensor that is not on a device)
        return torch.from_numpy(np.ascontiguousarray(device_rows(a)))
    if kind == "index":
        return tensor(a, index=1)
    rows = np.ascontiguousarray(device_rows(a))
    if kind == "dtype":
        return tensor(rows.astype({np.dtype(F): I32, np.dtype(np.float64): F}.get(rows.dtype, F)))
    if kind == "layout":  # (every second element of a tensor twice as long: the same shape, not contiguous)
        wide = torch.from_numpy(np.repeat(rows, 2, axis=-1))
        return OnDevice(wide[..., ::2])
    shape = list(rows.shape)
    shape[dim] += 1
    return tensor(np.zeros(shape, dtype=rows.dtype))


def refusals(route):
    for c in CASES:
        for name, (a, pinned) in c.args.items():
            if route == "host":  # (one wrong shape: an extent the wrapper pins, or one extent more where it pins none)
                if pinned is not None:
                    yield pytest.param(c.id, name, "extent" if pinned else "rank", pinned[0] if pinned else None, id=f"{c.id}-{name}")
                continue
            if name == "triangle_of_dfs":  # (lightmap_coords copies a table it cannot use as it is over: nothing to refuse)
                continue
            words = (a.ndim,) if a.dtype.names else ()  # (the words of a record are one more extent of its rows)
            for kind in ("host", "index", "dtype", "layout"):
                yield pytest.param(c.id, name, kind, None, id=f"{c.id}-{name}-{kind}")
            for dim in (pinned or ()) + words:
                yield pytest.param(c.id, name, "extent", dim, id=f"{c.id}-{name}-extent{dim}")


@pytest.mark.parametrize("id, name, kind, dim", list(refusals("device")))
def test_device_route_refuses_by_name(id, name, kind, dim, cpu_torch):
    """(The rays of closest_hits and occluded on another device than the scene's are new with the shared call path: that check was missing.)"""
    c, ds = BY_ID[id], scene()
    cpu_torch.append(ds.lib.calls)
    a = {n: tensor(x) for n, (x, _) in c.args.items()}
    a[name] = wrong(c.args[name][0], kind, dim)
    with pytest.raises(ValueError, match=f"^{name}:"):
        c.call(ds, a)
    assert ds.lib.calls == []


def test_device_route_refuses_a_tensor_inside_an_allocation_for_the_volumes(cpu_torch):
    ds = scene()
    for name, rows, call in (("sh", SH, lambda x: ds.volume_build(GRID, x)), ("probes", PROBE_ROWS, lambda x: ds.volume_sample(GRID, x, tensor(RAYS))),
                             ("points", RAYS, lambda x: ds.volume_sample(GRID, tensor(PROBE_ROWS), x)),
                             ("oct", OCT_ROWS, lambda x: ds.volume_build_depth(GRID, x, 1.0, res=RES)),
                             ("depth", DEPTH_ROWS, lambda x: ds.volume_sample(GRID, tensor(PROBE_ROWS), tensor(RAYS), depth=x, res=RES))):
        rows = device_rows(rows)
        inside = torch.zeros(rows.size + 1)[1:].reshape(rows.shape)
        assert inside.data_ptr() % 16 == 4 and inside.is_contiguous()
        with pytest.raises(ValueError, match=f"^{name}:.*16-byte aligned"):
            call(OnDevice(inside))
    assert ds.lib.calls == []


def test_irradiance_rays_checks_before_it_copies():
    ds = scene()
    for points, keys, name in ((RAYS[:, :7], None, "points"), (torch.from_numpy(RAYS), None, "points"), (tensor(RAYS), torch.from_numpy(KEYS.view(I32)), "keys"),
                               (tensor(RAYS), tensor(KEYS[:2]), "keys"), (tensor(RAYS, index=1), None, "points"), (tensor(RAYS.astype(np.float64)), None, "points")):
        with pytest.raises(ValueError, match=f"^{name}:"):
            ds.irradiance_rays(points, 0, keys=keys)
    assert ds.lib.calls == []


def test_irradiance_rays_on_the_device(cpu_torch):
    ds = scene()
    cpu_torch.append(ds.lib.calls)
    points, keys = tensor(RAYS), tensor(KEYS)
    rays, keys_out = ds.irradiance_rays(points, 4, seed=7, keys=keys, key_base=5, first_draw=3, mode="sphere")
    assert ds.lib.names() == ["torch_wait", "sol_irradiance_rays", "sol_sync"]
    args = ds.lib.calls[1][1]
    assert [address(x) for x in args[:4]] == [HANDLE, points.data_ptr(), keys.data_ptr(), N]
    assert bytes(args[4]._obj) == gather_config(samples=1, first_sample=4, mode=_abi.SOL_IRRADIANCE_SPHERE)
    assert [address(x) for x in args[5:]] == [rays.data_ptr(), keys_out.data_ptr()]
    assert (tuple(rays.shape), rays.dtype, tuple(keys_out.shape), keys_out.dtype) == ((N, 8), torch.float32, (N, 2), torch.int32)


# ---- (c) the host route's refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id, name, kind, dim", list(refusals("host")))
def test_host_route_refuses_by_name(id, name, kind, dim):
    """The message starts with the argument that is wrong. (New with the shared call path: the host routes used to list every argument in one
    sentence, so this holds before it only where the offender happens to come first.)"""
    c, ds = BY_ID[id], scene()
    a = {n: x for n, (x, _) in c.args.items()}
    shape = list(a[name].shape)
    if kind == "rank":
        shape.append(1)
    else:
        shape[dim] += 1
    a[name] = np.zeros(shape, dtype=a[name].dtype)
    with pytest.raises(ValueError, match=f"^{name}:"):
        c.call(ds, a)
    assert ds.lib.calls == []


def test_label_arrays_of_another_width_are_refused_by_name():
    ds, wide = scene(), np.zeros(T, dtype=np.int64)
    with pytest.raises(ValueError, match="^chart_of_triangle:"):
        ds.lightmap_dilate_charts(VALUES, TEXELS, wide, W, H)
    with pytest.raises(ValueError, match="^chart_of_triangle:"):
        ds.lightmap_sample_charts(VALUES, COORDS, UVS, TEXELS, wide, PLANE, W, H)
    with pytest.raises(ValueError, match="^chart_plane:"):
        ds.lightmap_sample_charts(VALUES, COORDS, UVS, TEXELS, CHART_OF, PLANE.astype(F), W, H)
    with pytest.raises(ValueError, match="^chart_plane:"):
        ds.lightmap_chart_levels(PLANE.astype(np.int64), W, H)
    with pytest.raises(ValueError, match="mode"):
        ds.irradiance(RAYS, mode="hemisphere")
    assert ds.lib.calls == []


# ---- (d) what is left to the library to refuse -------------------------------------------------------------------------------------------------
def test_what_the_library_refuses_reaches_it():
    """A bad width, channel count, grid or res: the wrapper allocates one row (or one word) and lets the library answer SOL_EINVAL."""
    ds = scene()

    def reaches(call):
        before = len(ds.lib.calls)
        out = call()
        assert len(ds.lib.calls) == before + 1
        return out
    for width, height in ((0, H), (W, _abi.SOL_LIGHTMAP_MAX_SIZE + 1)):
        points, texels = reaches(lambda: ds.lightmap_points(VERTICES, UVS, width, height))
        assert points.shape == (1, 8) and texels.shape == (1,)
    for channels in (0, 33):
        assert reaches(lambda: ds.lightmap_sample(VALUES, COORDS, UVS, TEXELS, W, H, channels=channels)).shape == (N, 1)
        assert reaches(lambda: ds.lightmap_sample_lod(VALUES, MIPS, COVER, LODS, COORDS, UVS, TEXELS, W, H, channels=channels)).shape == (N, 1)
        assert reaches(lambda: ds.lightmap_sample_charts(VALUES, COORDS, UVS, TEXELS, CHART_OF, PLANE, W, H, channels=channels)).shape == (N, 1)
        reaches(lambda: ds.lightmap_dilate(VALUES, TEXELS, W, H, channels=channels))
        reaches(lambda: ds.lightmap_mips(VALUES, TEXELS, W, H, channels=channels))
    assert reaches(lambda: ds.lightmap_filter(VALUES, POINTS16, TEXELS, W, H, 0.5, iterations=99, channels=5)).shape == (WH, 4)
    assert reaches(lambda: ds.lightmap_sh(VALUES, COORDS, NORMALS4, UVS, TEXELS, W, H)).shape == (N, 4)  # (rows too short for a SolSh9)
    for counts in ((0, 2, 2), (1 << 12, 1 << 12, 2)):
        none = VolumeGrid((0.0, 0.0, 0.0), 1.0, counts)
        assert reaches(lambda: ds.volume_points(none, host=True)).shape == (1, 8)
        assert reaches(lambda: ds.volume_build(none, SH[:1], VISIBILITY[:1])).shape == (1,)
        assert reaches(lambda: ds.volume_sample(none, PROBE_ROWS[:1], RAYS))[0].shape == (N, 3)
        assert reaches(lambda: ds.volume_build_depth(none, OCT_ROWS[:1], 1.0, res=RES)).shape == (1, OCT, 2)
    assert reaches(lambda: ds.visibility_oct(RAYS, res=5)).shape == (N, 1, 4)
    assert reaches(lambda: ds.volume_build_depth(GRID, OCT_ROWS[:, :1], 1.0, res=5)).shape == (PROBES, 1, 2)
    assert reaches(lambda: ds.volume_sample(GRID, PROBE_ROWS, RAYS, depth=DEPTH_ROWS[:, :1], res=7))[0].shape == (N, 3)
    reaches(lambda: ds.set_triangles(np.zeros((0, 3, 3))))
    assert "sol_sync" not in ds.lib.names()
