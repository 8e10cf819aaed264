"""Scratch reuse and call order across the entry points that came after the render path (the companion of tests/test_gpu_buffer_growth.py, whose
rule it keeps: a buffer that grew must hold nothing of its past, and one that did not must still be large enough). Every family has a test file of
its own in which a fresh handle makes its calls in one fixed order; here one long-lived handle makes the calls of several families, at several
sizes, one after another, so that every call finds its scratch (DevBuf, csrc/sol_scene.h: reserve keeps nothing and zeroes nothing) as another
family or another size left it. What such an order can show and a fresh handle cannot: a kernel that relies on scratch being zero or holding
its own family's values, a size in the wrong unit, a reserve that frees what a queued launch still uses.

Yardsticks. A family that traces nothing is compared word for word with its numpy restatement (tests/lightmap*_ref.py, volume_ref.py,
depth_ref.py); a traced family with a FRESH handle that makes only that one call (its agreement with the oracle is pinned in its own file). No call
is compared with the same call on the same handle.

The second part issues whole bakes through the raw `_dev` entry points with no synchronisation between the calls and compares every intermediate
with the synchronising wrappers on a fresh handle.

`Step` and the catalogue of calls below are also what tests/test_gpu_call_sequences_ext.py draws from. Atlases are at most 130 x 67, meshes at most
4096 triangles, batches at most 257 rows, gathers at most 48 samples."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import depth_ref as dr
import irradiance_adaptive_ref as ar
import lightmap_charts_ref as cr
import lightmap_filter_ref as fr
import lightmap_filter_var_ref as fvr
import lightmap_mips_ref as mr
import lightmap_ref as lr
import lightmap_sample_ref as sr
import lightmap_sh_ref as shr
import parity_util as pu
import primitive_util as prim
import volume_ref as vr
from solstrale_amd import (CameraConfig, DeviceScene, PathTracingShader, RenderConfig, VolumeGrid, _abi, camera_record, lightmap_mip_layout,
                           lightmap_triangle_table, pixel_spread, scenes)
from test_gpu_irradiance import surface_points, with_invalid_rows
from test_gpu_lightmap_charts import charted, label_cases, label_ref
from test_gpu_lightmap_charts import spoiled as charts_spoiled
from test_gpu_lightmap_filter import atlas as filter_atlas
from test_gpu_lightmap_filter import rows_of
from test_gpu_lightmap_filter_var import moments_of
from test_gpu_lightmap_mips import chain, lods_for
from test_gpu_lightmap_sample import atlas, floor_under_a_light, lookup_mesh
from test_gpu_lightmap_sh import row_normals
from test_gpu_set_triangles import _mesh_scene
from test_gpu_volume import random_sums
from test_gpu_volume_depth import random_depth, random_oct_sums

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F, U = np.float32, np.uint32
RC = RenderConfig(32, 32, 1)
RADIANCE_ROWS = "128"  # the smallest SOL_RADIANCE_ROWS the families' own tests use (tests/test_gpu_radiance.py, test_gpu_visibility.py)


# ---- comparing ------------------------------------------------------------------------------------------------------------------------------------
def words(x):
    """An array, a structured array, a number or a device tensor as a flat array of its 32-bit words (a byte plane: of its bytes)."""
    x = x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
    if x.dtype.kind in "iu" and x.dtype.itemsize == 8:  # (a count the wrapper returned as a Python int)
        x = x.astype(U)
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view(np.uint8 if x.dtype.itemsize == 1 else U)


def host(outputs):
    """What a call returned, as a tuple of host arrays that own their memory."""
    outputs = outputs if isinstance(outputs, (tuple, list)) else (outputs,)
    return tuple(x.cpu().numpy().copy() if hasattr(x, "data_ptr") else np.array(x) for x in outputs)


def assert_same(got, want, what, nan_for_nan=False):
    """Every output of a call, word for word. nan_for_nan: two words that are both NaN as floats count as equal (the a-trous filters' own files
    compare so: which NaN an overflowing sum becomes is not part of their rule)."""
    got, want = host(got), host(want)
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        gw, ww = words(g), words(w)
        assert gw.shape == ww.shape, (what, "output", k, g.shape, w.shape)
        differ = gw != ww
        if nan_for_nan and gw.dtype == U:
            differ &= ~(np.isnan(gw.view(F)) & np.isnan(ww.view(F)))
        if differ.any():
            bad = np.nonzero(differ)[0]
            raise AssertionError((what, "output", k, f"{len(bad)} of {len(gw)} words differ", bad[:8].tolist(), gw[bad[:4]].tolist(), ww[bad[:4]].tolist()))


def dev(x):
    """A host array as a device tensor of the same words (structured rows as [n, k] int32, uint32 as int32); None stays None."""
    import torch
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    if x.dtype.names:
        x = x.view(np.int32).reshape(len(x), x.dtype.itemsize // 4) if len(x) else np.zeros((0, x.dtype.itemsize // 4), dtype=np.int32)
    elif x.dtype == U:
        x = x.view(np.int32)
    return torch.from_numpy(x.copy()).cuda()


def R(h, *xs):
    """The arrays of a call on its route: as they are (host) or as device tensors."""
    return xs if h else tuple(dev(x) for x in xs)


def E(name, h):
    return name if h else name + "_dev"


class Step:
    """One call of the catalogue. entry: the ABI entry point it goes through; text: what a trace shows of it (and the key its yardstick is kept
    under); run(ds): makes the call on `ds` and returns its outputs; want(): the restatement's outputs, None for a traced call - its yardstick is
    a fresh handle."""

    def __init__(self, entry, text, run, want=None, nan_for_nan=False):
        self.entry, self.text, self.run, self.want, self.nan_for_nan = entry, f"{entry}: {text}", run, want, nan_for_nan
        self.traced = want is None


_wants = {}


def expected(step, state_key, fresh):
    """The yardstick's outputs of `step`, computed once per distinct call (and, traced, per scene state): fresh() opens a new handle of that state."""
    key = (step.text, state_key if step.traced else None)
    if key not in _wants:
        if step.traced:
            with fresh() as f:
                _wants[key] = host(step.run(f))
        else:
            _wants[key] = host(step.want())
    return _wants[key]


def cornell():
    return DeviceScene(scenes.cornell_box(RC))


def run_order(ds, steps, state_key="cornell", fresh=cornell):
    for k, step in enumerate(steps):
        got = host(step.run(ds))
        assert_same(got, expected(step, state_key, fresh), (k, step.text), step.nan_for_nan)


# ---- the catalogue: families that trace nothing ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices, uvs, normals or None) of the meshes the orders rasterise and label: 0, 1, 65, 128, 133 and 4096 triangles."""
    if name == "lookup":  # tests/test_gpu_lightmap_sample.py's: ownership is made from the UVs with the hole
        V, _, T = lookup_mesh()
        return V, T, None
    if name == "strip":
        T = np.ascontiguousarray(label_cases()["strip"][0])
        return lr.lift(T), T, None
    V, T, N = lr.grid_mesh(8, 3)
    n = {"grid": 128, "n65": 65, "one": 1, "empty": 0}[name]
    return np.ascontiguousarray(V[:n]), np.ascontiguousarray(T[:n]), np.ascontiguousarray(N[:n])


@functools.lru_cache(maxsize=None)
def values_of(n, channels, nwords, seed):
    return rows_of(n, channels, nwords, seed)


def lm_points(name, W, H, conservative, h):
    V, T, N = mesh(name)

    def want():
        if name == "lookup" and conservative:
            return atlas(W, H).points, atlas(W, H).texels  # (the same call of the restatement, made once for every file)
        return lr.lightmap_points(V, T, W, H, normals=N, conservative=conservative)
    return Step(E("sol_lightmap_points", h), f"{name} {W}x{H} conservative={conservative}",
                lambda ds: ds.lightmap_points(*R(h, V, T), W, H, normals=R(h, N)[0], conservative=conservative), want)


def lm_dilate(W, H, channels, passes, h, pass_of=True):
    """pass_of=False: the caller asks for no pass_of plane (a null pass_of_out: the rows alone)"""
    A, values = atlas(W, H), values_of(W * H, channels, channels + 1, 7 * W + H)
    return Step(E("sol_lightmap_dilate", h), f"{W}x{H} channels={channels} passes={passes}" + ("" if pass_of else " no pass_of"),
                lambda ds: ds.lightmap_dilate(*R(h, values, A.texels), W, H, passes=passes, channels=channels, return_pass_of=pass_of),
                lambda: lr.lightmap_dilate(values, A.texels, W, H, passes=passes, channels=channels)[:2 if pass_of else 1])


def lm_filter(W, H, channels, iterations, h):
    P, T, sigma = filter_atlas(W, H)
    values = values_of(W * H, channels, channels + 1, 3 * W + H)
    kw = dict(sigma_position=sigma, iterations=iterations, channels=channels)
    return Step(E("sol_lightmap_filter", h), f"{W}x{H} channels={channels} iterations={iterations}",
                lambda ds: ds.lightmap_filter(*R(h, values, P, T), W, H, **kw), lambda: fr.lightmap_filter(values, P, T, W, H, **kw), nan_for_nan=True)


def lm_filter_var(W, H, iterations, h, variance=True):
    """variance=False: the caller asks for no variance plane (a null variance_out: the filtered rows alone)"""
    P, T, sigma = filter_atlas(W, H)
    M = moments_of(W * H, W)
    kw = dict(sigma_position=sigma, iterations=iterations)
    return Step(E("sol_lightmap_filter_var", h), f"{W}x{H} iterations={iterations}" + ("" if variance else " no variance"),
                lambda ds: ds.lightmap_filter_var(*R(h, M.view(F).reshape(-1, 8), P, T), W, H, return_variance=variance, **kw),
                lambda: fvr.lightmap_filter_var(M, P, T, W, H, **kw)[:2 if variance else 1], nan_for_nan=True)


class _Floor:
    """The floor under a light of tests/test_gpu_lightmap_sample.py and, from a fresh handle of it, the camera's rays and their hits: the inputs
    of the calls that turn hits into surface rows and levels of detail (inputs, not answers: those come from the restatements)."""

    def __init__(self):
        self.sc, self.V, self.T = floor_under_a_light()
        self.table = lightmap_triangle_table(self.sc, 0, len(self.V))
        with DeviceScene(self.sc) as f:
            self.rays = f.camera_rays(0, 0, 32, 32, 0, SEED).reshape(-1, 8).cpu().numpy()
            self.hits = f.closest_hits(self.rays)
        pick = np.random.default_rng(4).permutation(len(self.rays))  # (hits, misses and the light mixed in every prefix)
        self.rays, self.hits = np.ascontiguousarray(self.rays[pick]), np.ascontiguousarray(self.hits[pick])
        self.coords = sr.lightmap_coords(self.hits, self.table)
        self.spread = pixel_spread(40.0, 32)


@functools.lru_cache(maxsize=None)
def floor():
    return _Floor()


def lm_coords(n, h, n_dfs=None):
    """n_dfs: the table cut to its first so many entries (0: an empty table, a null pointer - every hit is unlisted)"""
    fl = floor()
    hits, table = fl.hits[:n], fl.table[:n_dfs]
    return Step(E("sol_lightmap_coords", h), f"n={n}" + ("" if n_dfs is None else f" n_dfs={n_dfs}"), lambda ds: ds.lightmap_coords(R(h, hits)[0], table),
                lambda: sr.lightmap_coords(hits, table))


def lm_lod(n, W, H, h, n_triangles=None):
    """n_triangles: the mesh cut to its first so many triangles (0: no mesh, null pointers - every row answers 0)"""
    fl = floor()
    rays, hits, coords, V, T = fl.rays[:n], fl.hits[:n], fl.coords[:n], np.ascontiguousarray(fl.V[:n_triangles]), np.ascontiguousarray(fl.T[:n_triangles])
    return Step(E("sol_lightmap_lod", h), f"n={n} {W}x{H}" + ("" if n_triangles is None else f" n_triangles={n_triangles}"),
                lambda ds: ds.lightmap_lod(*R(h, rays, hits, coords, V, T), W, H, fl.spread, 0.25),
                lambda: mr.lightmap_lod(rays, hits, coords, V, T, W, H, fl.spread, 0.25))


def lm_sample(W, H, channels, passes, n, nearest, h):
    A = atlas(W, H)
    values, pass_of, rows = A.values[(channels, passes)], None if passes is None else A.pass_of[passes], A.rows[:n]
    kw = dict(channels=channels, nearest=nearest)
    return Step(E("sol_lightmap_sample", h), f"{W}x{H} channels={channels} passes={passes} n={n} nearest={nearest}",
                lambda ds: ds.lightmap_sample(*R(h, values, rows, A.uvs, A.texels), W, H, pass_of=R(h, pass_of)[0], **kw),
                lambda: sr.lightmap_sample(values, rows, A.uvs, A.texels, W, H, pass_of=pass_of, **kw))


def lm_sh(W, H, passes, n, h):
    A = atlas(W, H)
    values, pass_of, rows = A.values[(27, passes)], None if passes is None else A.pass_of[passes], A.rows[:n]
    normals = row_normals(257, W + H)[:n]
    return Step(E("sol_lightmap_sh", h), f"{W}x{H} passes={passes} n={n}",
                lambda ds: ds.lightmap_sh(*R(h, values, rows, normals, A.uvs, A.texels), W, H, scale=0.37, pass_of=R(h, pass_of)[0]),
                lambda: shr.lightmap_sh(values, rows, normals, A.uvs, A.texels, W, H, scale=0.37, pass_of=pass_of))


def lm_normals(n, h):
    A = atlas(64, 64)
    rows = A.rows[:n]
    finite = np.where(np.isfinite(A.vertices), A.vertices, F(1.0)).astype(F)
    N = (finite[:, ::-1] + F(0.25)).astype(F)  # per-corner normals of some length
    return Step(E("sol_lightmap_normals", h), f"n={n}", lambda ds: ds.lightmap_normals(*R(h, rows, A.vertices, N)), lambda: shr.lightmap_normals(rows, A.vertices, N))


def lm_mips(W, H, channels, passes, levels, h):
    A = atlas(W, H)
    values, pass_of, mips, cover = chain(A, channels, passes)
    nrows = lightmap_mip_layout(W, H, levels)["rows"]  # (a shorter chain is the full one's beginning)
    return Step(E("sol_lightmap_mips", h), f"{W}x{H} channels={channels} passes={passes} levels={levels}",
                lambda ds: ds.lightmap_mips(*R(h, values, A.texels), W, H, channels=channels, pass_of=R(h, pass_of)[0], levels=levels),
                lambda: (mips[:nrows], cover[:nrows]))


def lm_sample_lod(W, H, channels, passes, n, h, radius=None):
    """radius: the chart guard on - a finite chart_radius with the guard arrays (the mesh's vertices, the atlas's points)"""
    A = atlas(W, H)
    values, pass_of, mips, cover = chain(A, channels, passes)
    levels = lightmap_mip_layout(W, H)["levels"]
    lods, rows = lods_for(257, levels)[:n], A.rows[:n]
    guard = {} if radius is None else dict(chart_radius=radius, vertices=A.vertices, points=A.points)
    return Step(E("sol_lightmap_sample_lod", h), f"{W}x{H} channels={channels} passes={passes} n={n}" + ("" if radius is None else f" radius={radius}"),
                lambda ds: ds.lightmap_sample_lod(*R(h, values, mips, cover, lods, rows, A.uvs, A.texels), W, H, channels=channels, pass_of=R(h, pass_of)[0],
                                                  **{k: v if k == "chart_radius" else R(h, v)[0] for k, v in guard.items()}),
                lambda: mr.lightmap_sample_lod(values, mips, cover, lods, rows, A.uvs, A.texels, W, H, channels=channels, pass_of=pass_of, **guard))


def lm_charts(name, h):
    uvs, vertices = label_cases()[name]
    uvs, vertices = np.ascontiguousarray(uvs), None if vertices is None else np.ascontiguousarray(vertices)
    return Step(E("sol_lightmap_charts", h), name, lambda ds: ds.lightmap_charts(*R(h, uvs, vertices)), lambda: label_ref(name))


def lm_dilate_charts(W, H, channels, passes, h):
    Q = charted(W, H)
    return Step(E("sol_lightmap_dilate_charts", h), f"{W}x{H} channels={channels} passes={passes}",
                lambda ds: ds.lightmap_dilate_charts(*R(h, Q.raw[channels], Q.texels, Q.chart_of), W, H, passes=passes, channels=channels),
                lambda: Q.ref[(channels, passes)])


def lm_sample_charts(W, H, channels, passes, n, h):
    Q = charted(W, H)
    values, pass_of, plane = charts_spoiled(Q, channels, passes)
    rows = Q.A.rows[:n]
    return Step(E("sol_lightmap_sample_charts", h), f"{W}x{H} channels={channels} passes={passes} n={n}",
                lambda ds: ds.lightmap_sample_charts(*R(h, values, rows, Q.A.uvs, Q.texels, Q.chart_of, plane), W, H, channels=channels, pass_of=R(h, pass_of)[0]),
                lambda: cr.lightmap_sample_charts(values, rows, Q.A.uvs, Q.texels, Q.chart_of, plane, W, H, channels=channels, pass_of=pass_of))


def lm_chart_levels(W, H, passes, h):
    _, pass_of, plane = charted(W, H).ref[(3, passes)]

    def run(ds):
        levels, texels, windows = ds.lightmap_chart_levels(*R(h, plane), W, H, pass_of=R(h, pass_of)[0])
        return np.asarray([levels], dtype=U), texels, windows

    def want():
        levels, texels, windows = cr.lightmap_chart_levels(plane, W, H, pass_of)
        return np.asarray([levels], dtype=U), texels, windows
    return Step(E("sol_lightmap_chart_levels", h), f"{W}x{H} passes={passes}", run, want)


def rescale(n, target, h):
    rows = np.ascontiguousarray(values_of(257, 3, 4, 77)[:n]).copy()
    rows.view(U)[:, 3] = np.arange(n, dtype=U) % 5 * 16  # counts 0, 16, .. 64
    return Step(E("sol_radiance_rescale", h), f"n={n} target={target}", lambda ds: ds.radiance_rescale(R(h, rows)[0], target), lambda: ar.rescale(rows, target))


# volumes and depth maps
def grid_of(counts):
    return VolumeGrid((-1.0, 0.5, 2.0), (0.5, 0.75, 1.25), counts, backface=True, chebyshev=True, normal_bias=0.1)


@functools.lru_cache(maxsize=None)
def volume_case(counts, n=257):
    """(probes [n_probes, 32] by the restatement, point rows [n, 8] in and around the grid) of one grid"""
    g = grid_of(counts)
    sh, vis = random_sums(g.n_probes, 11 + g.n_probes)
    rng = np.random.default_rng(g.n_probes)
    at = vr.probe_positions(g)
    lo, size = at[0].astype(np.float64), (at[-1] - at[0]).astype(np.float64)
    pos = lo + rng.uniform(-0.3, 1.3, (n, 3)) * np.where(size > 0, size, 1.0)
    return sh, vis, vr.volume_build(sh, vis, radius=2.0), vr.point_rows(pos.astype(F), vr.unit_normals(rng, n))


def vol_points(counts, h):
    g = grid_of(counts)
    return Step(E("sol_volume_points", h), f"{counts}", lambda ds: ds.volume_points(g, tmin=0.25, tmax=7.5, host=h), lambda: vr.volume_points(g, tmin=0.25, tmax=7.5))


def vol_build(counts, h, visibility=True):
    """visibility=False: no SolVisibility rows (a null pointer: the probes' distance words by the rule without them)"""
    g = grid_of(counts)
    sh, vis, probes, _ = volume_case(counts)
    if not visibility:
        return Step(E("sol_volume_build", h), f"{counts} no visibility", lambda ds: ds.volume_build(g, R(h, sh)[0], None, radius=2.0),
                    lambda: vr.volume_build(sh, None, radius=2.0))
    return Step(E("sol_volume_build", h), f"{counts}", lambda ds: ds.volume_build(g, *R(h, sh, vis), radius=2.0), lambda: probes)


def _rgba(out):
    """volume_sample's host pair as the raw rows of its device route"""
    return np.concatenate([out[0], out[1].view(F)[:, None]], axis=1) if isinstance(out, tuple) else out


def vol_sample(counts, n, h):
    g = grid_of(counts)
    _, _, probes, points = volume_case(counts)
    return Step(E("sol_volume_sample", h), f"{counts} n={n}", lambda ds: _rgba(ds.volume_sample(g, *R(h, probes, points[:n]))),
                lambda: vr.volume_sample(g, probes, points[:n]))


def vol_build_depth(counts, res, h):
    g = grid_of(counts)
    sums = random_oct_sums(g.n_probes, res, 20 + res)
    return Step(E("sol_volume_build_depth", h), f"{counts} res={res}", lambda ds: ds.volume_build_depth(g, R(h, sums)[0], 2.0, res=res), lambda: dr.build_depth(sums, 2.0))


def vol_sample_depth(counts, res, n, h):
    g = grid_of(counts)
    _, _, probes, points = volume_case(counts)
    depth = random_depth(g.n_probes, res, 30 + res)
    return Step(E("sol_volume_sample_depth", h), f"{counts} res={res} n={n}",
                lambda ds: _rgba(ds.volume_sample(g, *R(h, probes, points[:n]), depth=R(h, depth)[0], res=res)),
                lambda: dr.volume_sample_depth(g, probes, depth, res, points[:n]))


# ---- the catalogue: traced families (the yardstick is a fresh handle) -------------------------------------------------------------------------------
class Inputs:
    """The rays and points a scene's traced calls take: the camera's rays with an invalid one among them, and points on the scene's surfaces with
    a row of every invalid class (tests/test_gpu_irradiance.py) - 257 of each. Made once per scene, by a fresh handle."""

    def __init__(self, sc):
        with DeviceScene(sc) as f:
            rays = f.camera_rays(0, 0, sc.width, sc.height, 0, SEED).reshape(-1, 8).cpu().numpy()
            points = with_invalid_rows(surface_points(sc, f, 246))[0]
        self.rays = np.ascontiguousarray(rays[np.random.default_rng(3).permutation(len(rays))[:257]])
        self.rays[5, 4:7] = 0.0
        self.points = np.ascontiguousarray(points[:257])
        assert self.rays.shape == self.points.shape == (257, 8)


_inputs = {}


def inputs(name="cornell"):
    if name not in _inputs:
        _inputs[name] = Inputs(scenes.cornell_box(RC) if name == "cornell" else deep_scene() if name == "deep" else dynamic_base())
    return _inputs[name]


@functools.lru_cache(maxsize=None)
def deep_scene():
    """tests/test_gpu_queries.py's sphere chain of 120 levels: created under SOL_BVH=ref its tree needs 42 stack words, 10 past the LDS stack"""
    from test_gpu_queries import _deep_chain
    return _deep_chain()


def keys_of(n):
    return np.stack([np.arange(n) * 3 + 1, np.arange(n) % 7], axis=1).astype(U)


def query(mode, n, h, scene="cornell"):
    rays = inputs(scene).rays[:n]
    return Step(E("sol_query", h), f"{mode} n={n}", lambda ds: (ds.closest_hits if mode == "closest" else ds.occluded)(R(h, rays)[0]))


def _gather(entry, method, text, n, h, scene, use_keys, **kw):
    a = inputs(scene)
    rows = (a.rays if method == "radiance" else a.points)[:n]
    keys = keys_of(n) if use_keys else None
    return Step(E(entry, h), f"{text} n={n} keys={use_keys} {sorted(kw.items())}", lambda ds: getattr(ds, method)(R(h, rows)[0], keys=R(h, keys)[0], seed=SEED, **kw))


def radiance(n, samples, h, scene="cornell", use_keys=False, key_base=7):
    return _gather("sol_radiance", "radiance", "", n, h, scene, use_keys, samples=samples, key_base=key_base)


def irradiance(n, samples, h, scene="cornell", use_keys=False, key_base=7, mode="cosine"):
    return _gather("sol_irradiance", "irradiance", "", n, h, scene, use_keys, samples=samples, key_base=key_base, mode=mode)


def irradiance_sh(n, samples, h, scene="cornell", use_keys=False, key_base=7):
    return _gather("sol_irradiance_sh", "irradiance_sh", "", n, h, scene, use_keys, samples=samples, key_base=key_base)


def irradiance_moments(n, samples, h, scene="cornell", use_keys=False, key_base=7):
    return _gather("sol_irradiance_moments", "irradiance_moments", "", n, h, scene, use_keys, samples=samples, key_base=key_base)


def irradiance_adaptive(n, max_samples, rnd, threshold, h, scene="cornell", use_keys=False, key_base=7):
    return _gather("sol_irradiance_adaptive", "irradiance_adaptive", "", n, h, scene, use_keys, max_samples=max_samples, round=rnd, min_samples=16, threshold=threshold,
                   key_base=key_base)


def visibility(n, samples, distances, h, scene="cornell", use_keys=False, key_base=7):
    return _gather("sol_visibility", "visibility", "", n, h, scene, use_keys, samples=samples, distances=distances, key_base=key_base)


def visibility_oct(n, samples, res, h, scene="cornell", use_keys=False, key_base=7):
    return _gather("sol_visibility_oct", "visibility_oct", "", n, h, scene, use_keys, samples=samples, res=res, key_base=key_base)


def irradiance_rays(n, sample, scene="cornell"):
    points = inputs(scene).points[:n]
    return Step("sol_irradiance_rays", f"n={n} sample={sample}", lambda ds: ds.irradiance_rays(dev(points), sample, seed=SEED, key_base=7))


# ---- a handle that can be moved ---------------------------------------------------------------------------------------------------------------------
CAMERAS = (CameraConfig(40., 0., (0., 4., 10.), (0., 1., 0.), (0., 1., 0.)), CameraConfig(45., 0., (7., 3., 6.), (0., 1., 0.), (0., 1., 0.)))


@functools.lru_cache(maxsize=None)
def dynamic_base():
    """tests/test_gpu_set_triangles.py's mesh scene - 128 triangles over a floor quad, a sphere and a quad light in one list - at 32 x 32"""
    return _mesh_scene(rc=RenderConfig(32, 32, 1, PathTracingShader(8)), camera=CAMERAS[0], cells=8)


@functools.lru_cache(maxsize=None)
def dynamic_rows(k):
    """Row sets the moves choose from: 0 the creation description's, then seeded jitters and a scaling of it (tests/primitive_util.py)."""
    rows = prim.rows_of(dynamic_base().desc)
    return rows if k == 0 else prim.scale(rows, 1.1) if k == 3 else prim.jitter(rows, 4 + k)


class Moved:
    """The description a moved handle stands for: which camera, which triangle rows, which sphere and quad rows, which light sampling mode."""

    def __init__(self):
        self.camera = self.triangles = self.primitives = self.light = 0

    def key(self):
        return ("mesh", self.camera, self.triangles, self.primitives, self.light)

    def scene(self):
        m = prim.MovedScene(dynamic_base(), triangles=dynamic_rows(self.triangles)["triangles"], spheres=dynamic_rows(self.primitives)["spheres"],
                            quads=dynamic_rows(self.primitives)["quads"])
        m.desc.camera = camera_record(m.width, m.height, CAMERAS[self.camera])
        return m

    def fresh(self):
        """a new handle of the moved description, not created for moves"""
        ds = DeviceScene(self.scene())
        if self.light:
            ds.light_sampling(self.light)
        return ds


# ---- 1. the orders ----------------------------------------------------------------------------------------------------------------------------------
def test_lm_owner_serves_points_charts_dilations_and_levels_in_turn():
    """lm_owner, in 32-bit words. lightmap_points takes 16 + W x H + 2 n (owner words at 16 .. 16 + W x H, claimed with atomicMin: stale owners of
    another mesh lie exactly where the second, smaller call's owners go, and a lower stale index would win); the dilations (2 W x H + 3) / 4 for
    their two byte planes; lightmap_charts its hash, sort and union-find scratch (LcScratch::words, tens of words per triangle); chart_levels the
    rows of the coarser levels + 1."""
    owner = [lm_points("lookup", 130, 67, True, True),         # 16 + 8710 + 266 = 8992 words, owners of 133 triangles
             lm_charts("strip", False),                          # LcScratch::words of 4096 triangles: grows (large after medium)
             lm_dilate_charts(64, 64, 3, 4, False),              # 2048 words (small after large): byte planes over the sort scratch
             lm_points("grid", 16, 16, True, False),             # 16 + 256 + 256 = 528 words: the one that matters
             lm_points("grid", 16, 16, False, False),
             lm_chart_levels(130, 67, 4, False),                 # 2993 + 1 words
             lm_dilate(5, 3, 3, 1, False)]                       # 8 words
    with cornell() as ds:
        run_order(ds, owner)
        run_order(ds, owner[::-1])                               # small then large, every family after every other
        run_order(ds, [lm_points("lookup", 130, 67, True, False), lm_dilate(130, 67, 27, 4, True), lm_points("lookup", 130, 67, False, True),  # A, B, A
                       lm_points("empty", 1, 1, False, False), lm_points("one", 5, 3, True, True), lm_points("n65", 64, 64, True, False),
                       lm_charts("n0", False), lm_charts("n1", True), lm_charts("n65", False), lm_dilate_charts(1, 1, 3, 0, False), lm_dilate(64, 64, 3, 0, False)])


def test_lm_stage_serves_the_host_route_of_every_user_in_turn():
    """lm_stage, in bytes: every host route stages its inputs and outputs there, each array rounded up to 256 bytes. Largest and smallest shapes
    alternate - 130 x 67 x 28 words is 975520 bytes per value array, a 1 x 1 atlas a few times 256 -, so that every call after the first finds
    either a buffer that has to grow or one that holds a larger call's arrays at other offsets. In the middle the two host routes of the adaptive
    gather's family: sol_irradiance_adaptive stages through rad_in / rad_out, its companion sol_radiance_rescale through lm_stage
    (csrc/sol_gather_adaptive.cpp)."""
    stage = [lm_points("lookup", 130, 67, True, True),            # 133 x (36 + 24) + 8710 x (32 + 16) bytes
             lm_dilate(1, 1, 3, 0, True),                          # 4 arrays of 256 bytes
             lm_filter(130, 67, 27, 1, True),                      # 8710 x (32 + 16 + 2 x 112) bytes
             lm_filter_var(5, 3, 1, True),                         # 15 x (32 + 16 + 32 + 16 + 16) bytes
             lm_coords(257, True), lm_sample(1, 1, 3, None, 1, False, True),
             lm_sh(130, 67, 4, 257, True),                         # 8710 x 112 bytes of values and the rest
             lm_normals(1, True),
             irradiance_adaptive(257, 48, 16, 0.0, True),          # rad_in / rad_keys / rad_out
             rescale(257, 32, True), rescale(1, 7, True),          # 257 x 16 bytes, then 16
             lm_mips(130, 67, 27, 1, None, True),                  # 8710 x 112 in, 2993 x 113 out
             lm_sample_lod(5, 3, 3, 4, 63, True), lm_lod(257, 130, 67, True), lm_charts("n1", True),
             lm_dilate_charts(130, 67, 27, 4, True),               # 8710 x (16 + 2 x 112 + 1 + 4) bytes
             lm_sample_charts(1, 1, 3, 0, 1, True), lm_chart_levels(130, 67, 4, True), lm_chart_levels(1, 1, 0, True),
             lm_charts("strip", True), lm_points("empty", 1, 1, False, True)]
    # what a host route stages or leaves out by a null pointer or a zero count, each beside its counterpart, at the smallest shapes that still run the
    # kernels: no pass_of plane and no variance plane asked for, an empty table and no mesh (a required array of 0 bytes), the chart guard's arrays
    stage += [lm_dilate(5, 3, 3, 1, True, pass_of=False), lm_dilate(5, 3, 3, 1, True),
              lm_filter_var(5, 3, 1, True, variance=False),
              lm_coords(65, True, n_dfs=0), lm_coords(1, True, n_dfs=2), lm_lod(65, 5, 3, True, n_triangles=0), lm_lod(1, 5, 3, True, n_triangles=2),
              lm_sample_lod(5, 3, 3, 4, 65, True, radius=5.0), lm_sample_lod(5, 3, 3, 4, 1, True)]
    with cornell() as ds:
        run_order(ds, stage)
        run_order(ds, stage[::-1])


def test_filter_planes_serve_both_filters_at_three_and_twenty_seven_channels():
    """lf_guide (2 W x H float4) and lf_planes (float4; sol_lightmap_filter: 2 x ceil(channels / 4) x W x H, sol_lightmap_filter_var: 4 x W x H)."""
    with cornell() as ds:
        run_order(ds, [lm_filter(130, 67, 3, 3, False),            # planes 2 x 8710 = 17420, guide 17420
                       lm_filter_var(16, 16, 1, False),            # planes 4 x 256 = 1024 (small after large, another family's values below)
                       lm_filter(64, 64, 27, 1, False),            # planes 14 x 4096 = 57344 (grows), guide 8192 (does not)
                       lm_filter_var(130, 67, 3, True),            # planes 4 x 8710 = 34840 (large after larger), guide 17420
                       lm_filter(16, 16, 3, 3, True), lm_filter(130, 67, 27, 3, False),  # small then large: 512, then 14 x 8710 = 121940
                       lm_filter_var(1, 1, 1, False), lm_filter(5, 3, 27, 1, True), lm_filter_var(64, 64, 3, False)])


# (method of DeviceScene, rows, what it is asked for): the order over the gathers' shared scratch, as data - the child process below makes the same calls
RAD_CALLS = [("radiance", 257, dict(samples=48)),                                   # 5 groups x 3 chunks: 960 rows
             ("irradiance", 63, dict(samples=1, mode="cosine")),                    # one chunk: direct, rad_partial is not touched
             ("irradiance_sh", 65, dict(samples=17)),                               # per sample: 128 x 17 = 2176 rows (grows)
             ("visibility", 257, dict(samples=48, distances=True)),                 # chunk sums of 2 rows: 1920 rows (reused, smaller)
             ("visibility_oct", 65, dict(samples=17, res=8)),                       # per sample, four a row: 128 x 17 / 4 = 544 rows
             ("irradiance_moments", 64, dict(samples=16)),                          # per sample: 64 x 16 = 1024 rows
             ("irradiance_adaptive", 257, dict(max_samples=48, round=16, min_samples=16, threshold=0.0)),  # moments rounds over 320 x 16 = 5120 rows (grows), ga_* of 257
             ("radiance", 257, dict(samples=48))]                                   # as at first, over what all of them left
RAD_KEY_BASE = 7


def rad_order(h):
    """rad_work and rad_partial (and, on the host route, rad_in / rad_keys / rad_out; rad_spill stays at its 16 words on this shallow tree: the deep
    tree's order is test_spill_tails_serve_every_gather_family_and_the_queries_on_a_deep_tree). rad_partial in rows of 16 bytes, for n points in
    ceil(n / 64) groups over c chunks of 16 samples: chunk sums of 1 row (radiance, irradiance, visibility) 64 x groups x c, of 2 rows
    (visibility with distances) twice that, per sample values (SH and moments: one a row; the octahedral maps: four a row) 64 x groups x
    samples / per_row."""
    return [_gather("sol_" + method, method, "", n, h, "cornell", False, key_base=RAD_KEY_BASE, **kw) for method, n, kw in RAD_CALLS]


def test_gather_scratch_serves_seven_families_in_turn():
    with cornell() as ds:
        run_order(ds, rad_order(False))
        run_order(ds, rad_order(True))     # the staged host routes: rad_in 257, 63, 65 .. rows
        run_order(ds, [irradiance(1, 17, False), visibility(1, 16, False, True), irradiance_sh(257, 48, False), irradiance_moments(1, 1, True),  # small, large
                       visibility_oct(257, 48, 4, False), irradiance_adaptive(65, 48, 16, 0.0, False), irradiance_adaptive(257, 17, 16, 0.05, True),
                       irradiance_adaptive(1, 16, 16, 0.0, False),
                       radiance(257, 48, True, use_keys=True), radiance(65, 17, True, use_keys=True), irradiance(1, 17, True, use_keys=True),  # rad_keys: 257, 65, 1 rows
                       irradiance(0, 16, False)])


RAD_CHILD = r"""
import json
import sys
import numpy as np
from solstrale_amd import DeviceScene, RenderConfig, scenes
a = np.load(sys.argv[1])
out = {}
with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
    for k, (method, n, kw) in enumerate(json.loads(str(a["calls"]))):
        rows = np.ascontiguousarray(a["rays" if method == "radiance" else "points"][:n])
        got = getattr(ds, method)(rows, seed=int(a["seed"]), key_base=int(a["key_base"]), **kw)
        for j, x in enumerate(got if isinstance(got, tuple) else (got,)):
            out[f"{k}_{j}"] = np.ascontiguousarray(x).reshape(-1).view(np.uint32)
np.savez(sys.argv[2], **out)
"""


def test_gather_scratch_under_a_bounded_partial_buffer(tmp_path):
    """The same order with SOL_RADIANCE_ROWS = 128: every call of more than one chunk runs in slices of 64 points and windows of few chunks while
    the buffer changes shape from family to family. The bound is read at creation, hence a fresh child process (under a time limit of its own);
    the yardsticks are this process's fresh handles with the default bound - a point's answer does not depend on the bound (each family's file).
    The child takes the staged host route, whose launches are the device route's (csrc/sol_gather.h: the bound acts in the launch plan both
    share), and so starts no second torch runtime: that alone would cost more than all the other orders of this file together."""
    import json
    np.savez(tmp_path / "in.npz", rays=inputs().rays, points=inputs().points, seed=SEED, key_base=RAD_KEY_BASE, calls=json.dumps(RAD_CALLS))
    env = {**os.environ, "SOL_RADIANCE_ROWS": RADIANCE_ROWS, "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", RAD_CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.load(tmp_path / "out.npz")
    for k, step in enumerate(rad_order(True)):
        want = expected(step, "cornell", cornell)
        assert_same([got[f"{k}_{j}"] for j in range(len(want))], [words(w) for w in want], (RADIANCE_ROWS, k, step.text))


def test_volume_staging_serves_probes_and_depth_maps_in_turn():
    """vol_stage, in bytes (arrays rounded up to 256): volume_points n x 32; volume_build n x (112 + 32 + 128); volume_sample n x 128 + m x (32 + 16);
    build_depth n x res^2 x (16 + 8); sample_depth adds n x res^2 x 8 to volume_sample's. n = 125, 24 and 1 probes, m = 257 points."""
    big, mid, one = (5, 5, 5), (2, 3, 4), (1, 1, 1)
    with cornell() as ds:
        run_order(ds, [vol_points(big, True), vol_build(big, True), vol_sample(big, 257, True),                # 4000, 34048, 28416 bytes
                       vol_build_depth(mid, 4, True), vol_sample_depth(mid, 4, 65, True),                      # 9216 + .. bytes: reused
                       vol_sample(one, 1, True),                                                               # 3 x 256 bytes
                       vol_build_depth(big, 8, True), vol_sample_depth(big, 8, 257, True),                     # 192000 bytes: grows; 64000 more
                       vol_points(one, True), vol_build(one, True), vol_sample_depth(one, 4, 63, True), vol_build(mid, True), vol_sample(big, 64, True),
                       vol_points(mid, False), vol_build(big, False), vol_sample(mid, 257, False), vol_build_depth(big, 4, False),  # (the device routes stage nothing)
                       vol_sample_depth(big, 8, 1, False), vol_points(big, True),
                       vol_build(one, True, visibility=False), vol_build(big, True, visibility=False)])               # no visibility rows: none staged, a null pointer


def test_query_staging_serves_both_modes_and_routes_in_turn():
    """query_in (rays) and query_out (rows of 32 bytes; an occlusion query writes one word a ray into the same buffer). query_spill stays at its
    16 words on this shallow tree: the deep tree's order is test_spill_tails_serve_every_gather_family_and_the_queries_on_a_deep_tree."""
    for h in (True, False):
        with cornell() as ds:
            run_order(ds, [query("closest", 257, h),               # 257 rays, 257 x 32 bytes out
                           query("occluded", 1, h),                # 1 ray: a word at the start of what held a hit row
                           query("closest", 65, h),                # in between: rows 1 .. 64 lie over the first call's
                           query("occluded", 257, h), query("closest", 1, h), query("closest", 0, h), query("occluded", 64, not h), query("closest", 257, not h)])


def test_spill_tails_serve_every_gather_family_and_the_queries_on_a_deep_tree(monkeypatch):
    """rad_spill and query_spill, in 32-bit words: sol_launch_plan (csrc/sol_launch.cpp) sizes the tail of EVERY launch as workgroups x 256 threads x
    (stack_bound - 32) words, workgroups = min(CUs x the kernel's blocks per CU, ceil(items / 256)) - 16 words while the tree fits the LDS stack, as
    on every other handle of this file. Under SOL_BVH=ref the sphere chain needs 42 words, so 2560 words a workgroup, and the spill builds of the
    kernels run. The families differ in their items (chunk sums: 64 x groups x chunks; per sample: 64 x groups x samples; a query: its rays), so
    each finds the tail of another family's launch: one sized for another launch is what this order is for."""
    monkeypatch.setenv("SOL_BVH", "ref")

    def fresh():
        return DeviceScene(deep_scene())
    gathers = lambda h: [radiance(257, 48, h, "deep"),                       # 960 items: 4 workgroups, 10240 words
                         irradiance(63, 1, h, "deep"),                       # 64 items: 1 workgroup, 2560 words (shrinks: the buffer stays)
                         irradiance_sh(65, 17, h, "deep"),                   # 2176 items: 9 workgroups, 23040 words (grows)
                         visibility(257, 48, True, h, "deep"),               # 960 items: 10240 words, the closest-hit build
                         visibility(63, 16, False, h, "deep"),               # 64 items: 2560 words, the any-hit build
                         visibility_oct(65, 17, 8, h, "deep"),               # 2176 items: 23040 words
                         irradiance_moments(64, 16, h, "deep"),              # 1024 items: 4 workgroups, 10240 words
                         irradiance_adaptive(257, 48, 16, 0.0, h, "deep"),   # rounds of 5120 items: 20 workgroups, 51200 words (grows)
                         radiance(257, 48, h, "deep")]                       # 10240 words again, in what the adaptive rounds left
    queries = lambda h: [query("closest", 257, h, "deep"),                   # query_spill: 2 workgroups, 5120 words
                         query("occluded", 1, h, "deep"),                    # 1 workgroup, 2560 words
                         query("closest", 65, h, "deep"),                    # 2560 words
                         query("occluded", 257, h, "deep"), query("closest", 257, h, "deep")]  # 5120 words
    with fresh() as ds:
        info = ds.info()
        assert info["stack_bound"] - info["lds_stack"] == 10, info  # (the sizes above)
        run_order(ds, gathers(False) + queries(False), "deep", fresh)
        run_order(ds, queries(True) + gathers(True)[::-1], "deep", fresh)   # small then large, and the host routes
    hits = expected(query("closest", 257, False, "deep"), "deep", fresh)[0]
    assert (hits.reshape(-1, 8)[:, 3] == _abi.SOL_RAY_HIT).any()        # (the rays do search the chain)


def test_a_gather_and_a_lightmap_call_before_and_after_every_move():
    """A handle created for moves: after sol_scene_set_camera, sol_scene_set_triangles (both routes) and sol_scene_set_primitives the gathers answer
    what a fresh handle of the moved description answers, out of scratch the calls before the move filled - and the lightmap calls, which read no
    scene, answer the restatement all along."""
    import torch
    state = Moved()
    around = lambda: [irradiance(65, 17, False, "mesh"), radiance(257, 48, True, "mesh"), query("closest", 257, False, "mesh"), lm_points("grid", 16, 16, True, False),
                      visibility(63, 16, True, True, "mesh"), lm_dilate(5, 3, 3, 1, True)]
    with DeviceScene(dynamic_base(), dynamic_primitives=True) as ds:
        run_order(ds, around(), state.key(), state.fresh)
        ds.set_camera(CAMERAS[1])
        state.camera = 1
        run_order(ds, around(), state.key(), state.fresh)
        ds.set_triangles(dynamic_rows(1)["triangles"])
        state.triangles = 1
        run_order(ds, around(), state.key(), state.fresh)
        ds.set_primitives(**dynamic_rows(2))
        state.triangles = state.primitives = 2
        run_order(ds, around(), state.key(), state.fresh)
        ds.set_triangles(torch.from_numpy(np.ascontiguousarray(dynamic_rows(3)["triangles"])).cuda())
        state.triangles = 3
        run_order(ds, around(), state.key(), state.fresh)
        ds.set_camera(CAMERAS[0])
        ds.set_primitives(**dynamic_rows(0))
        state.camera = state.triangles = state.primitives = 0
        run_order(ds, around(), state.key(), state.fresh)


# ---- 2. whole bakes on device memory, nothing synchronised in between -------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr())


class Bake:
    """The two bakes of a W x W atlas of the floor under a light, five samples a texel. wrapped(f): through DeviceScene's wrappers, which
    synchronise after every call; queued(ds): the same calls through the raw `_dev` entry points into arrays allocated beforehand, nothing
    synchronised until the end. Both return the list of every intermediate and the final rows."""
    SAMPLES = 5

    def __init__(self, W, sh):
        import torch
        fl = floor()
        self.W, self.sh, self.n = W, sh, W * W
        self.dV, self.dT = torch.from_numpy(fl.V).cuda(), torch.from_numpy(fl.T).cuda()
        self.sigma = 2.0 * 4.0 / (0.75 * W)  # two texels' world size: the floor is 4 units wide over three quarters of the atlas
        self.levels = lightmap_mip_layout(W, W)["levels"]
        self.mip_rows = lightmap_mip_layout(W, W)["rows"]
        self.lods = torch.from_numpy(lods_for(self.n, self.levels, seed=W)).cuda()
        self.normals = torch.from_numpy(row_normals(self.n, W)).cuda()

    def wrapped(self, f):
        W, s = self.W, self.SAMPLES
        points, texels = f.lightmap_points(self.dV, self.dT, W, W)
        if self.sh:
            rows = f.irradiance_sh(points, samples=s, seed=SEED)
            filtered = f.lightmap_filter(rows, points, texels, W, W, self.sigma, iterations=3, value_scale=4.0 * math.pi / s, channels=27)
            baked, pass_of = f.lightmap_dilate(filtered, texels, W, W, passes=2, channels=27, return_pass_of=True)
            shaded = f.lightmap_sh(baked, texels, self.normals, self.dT, texels, W, W, scale=4.0 * math.pi / s, pass_of=pass_of)
            return [points, texels, rows, filtered, baked, pass_of, shaded]
        rows = f.irradiance(points, samples=s, seed=SEED)
        filtered = f.lightmap_filter(rows, points, texels, W, W, self.sigma, iterations=3, value_scale=math.pi / s)
        chart_of, n_charts = f.lightmap_charts(self.dT, self.dV)
        baked, pass_of, plane = f.lightmap_dilate_charts(filtered, texels, chart_of, W, W, passes=2)
        mips, cover = f.lightmap_mips(baked, texels, W, W, pass_of=pass_of)
        looked = f.lightmap_sample_lod(baked, mips, cover, self.lods, texels, self.dT, texels, W, W, pass_of=pass_of)
        return [points, texels, rows, filtered, chart_of, np.asarray([n_charts], dtype=U), baked, pass_of, plane, mips, cover, looked]

    def queued(self, ds):
        import torch
        W, n, s, L, h = self.W, self.n, self.SAMPLES, ds.lib, ds.h
        nt = len(self.dV)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")
        points, texels = new((n, 8)), new((n, 4), torch.int32)
        k = 28 if self.sh else 4
        rows, filtered, baked, pass_of = new((n, k)), new((n, k)), new((n, k)), new((W, W), torch.uint8)
        chart_of, n_charts, plane = new((nt,), torch.int32), new((1,), torch.int32), new((W, W), torch.int32)
        mips, cover, final = new((self.mip_rows, 4)), new((self.mip_rows,), torch.uint8), new((n, 4))
        lm = _abi.SolLightmapConfig(size=C.sizeof(_abi.SolLightmapConfig), width=W, height=W, flags=0, tmin=1e-3, tmax=float("inf"))
        ir = _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=s, first_sample=0, first_draw=0, seed=SEED, key_base=0,
                                      mode=_abi.SOL_IRRADIANCE_SPHERE if self.sh else _abi.SOL_IRRADIANCE_COSINE)
        fc = _abi.SolLightmapFilterConfig(size=C.sizeof(_abi.SolLightmapFilterConfig), width=W, height=W, iterations=3, normal_power_log2=5, channels=k - 1,
                                          stride_bytes=4 * k, sigma_position=self.sigma, sigma_plane=self.sigma, sigma_value=0.25,
                                          value_scale=(4.0 if self.sh else 1.0) * math.pi / s)
        torch.cuda.synchronize()  # once: everything above is there, nothing below waits for anything but the handle's stream
        ds._chk(L.sol_lightmap_points_dev(h, _p(self.dV), None, _p(self.dT), nt, C.byref(lm), _p(points), _p(texels)))
        if self.sh:
            ds._chk(L.sol_irradiance_sh_dev(h, _p(points), None, n, C.byref(ir), _p(rows)))
            ds._chk(L.sol_lightmap_filter_dev(h, C.byref(fc), _p(points), _p(texels), _p(rows), _p(filtered)))
            ds._chk(L.sol_lightmap_dilate_dev(h, _p(texels), W, W, _p(filtered), 27, 4 * k, 2, _p(baked), _p(pass_of)))
            sc = _abi.SolLightmapShConfig(size=C.sizeof(_abi.SolLightmapShConfig), width=W, height=W, stride_bytes=4 * k, flags=0, chart_radius=float("inf"),
                                          scale=4.0 * math.pi / s)
            ds._chk(L.sol_lightmap_sh_dev(h, C.byref(sc), _p(self.dT), nt, _p(texels), _p(pass_of), _p(baked), None, None, _p(texels), _p(self.normals), n, _p(final)))
            ds.sync()
            return [points, texels, rows, filtered, baked, pass_of, final]
        ds._chk(L.sol_irradiance_dev(h, _p(points), None, n, C.byref(ir), _p(rows)))
        ds._chk(L.sol_lightmap_filter_dev(h, C.byref(fc), _p(points), _p(texels), _p(rows), _p(filtered)))
        ds._chk(L.sol_lightmap_charts_dev(h, _p(self.dT), _p(self.dV), nt, _p(chart_of), _p(n_charts)))
        ds._chk(L.sol_lightmap_dilate_charts_dev(h, _p(texels), W, W, _p(filtered), 3, 4 * k, 2, _p(chart_of), nt, _p(baked), _p(pass_of), _p(plane)))
        ds._chk(L.sol_lightmap_mips_dev(h, _p(texels), _p(pass_of), W, W, _p(baked), 3, 4 * k, self.levels, _p(mips) if self.mip_rows else None,
                                        _p(cover) if self.mip_rows else None))
        lc = _abi.SolLightmapLodConfig(size=C.sizeof(_abi.SolLightmapLodConfig), width=W, height=W, channels=3, stride_bytes=4 * k, flags=0,
                                       chart_radius=float("inf"), levels=self.levels)
        ds._chk(L.sol_lightmap_sample_lod_dev(h, C.byref(lc), _p(self.dT), nt, _p(texels), _p(pass_of), _p(baked), _p(mips) if self.mip_rows else None,
                                              _p(cover) if self.mip_rows else None, None, None, _p(texels), _p(self.lods), n, _p(final)))
        ds.sync()
        return [points, texels, rows, filtered, chart_of, n_charts, baked, pass_of, plane, mips, cover, final]


_bakes = {}


def bake_yardstick(W, sh):
    if (W, sh) not in _bakes:
        with DeviceScene(floor().sc) as f:
            _bakes[(W, sh)] = host(Bake(W, sh).wrapped(f))
    return _bakes[(W, sh)]


@pytest.mark.parametrize("sh", [False, True], ids=["irradiance_charts_mips_lod", "sh_filter27_dilate_shade"])
def test_a_bake_queued_without_synchronisation_equals_the_synchronised_bake(sh):
    """32 x 32, then 16 x 16 (every scratch buffer is larger than needed and holds the first bake's values), then 64 x 64 (lm_owner, lf_guide,
    lf_planes and rad_partial must grow in the middle of a chain: reserve frees and allocates while the earlier calls of the chain are still
    queued), then 32 x 32 once more on the caller's stream."""
    import torch
    with DeviceScene(floor().sc) as ds:
        for W in (32, 16, 64):
            assert_same(Bake(W, sh).queued(ds), bake_yardstick(W, sh), (W, "the handle's own stream"))
        stream = torch.cuda.Stream()
        ds.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                assert_same(Bake(32, sh).queued(ds), bake_yardstick(32, sh), (32, "the caller's stream"))
        finally:
            ds.set_stream(0)
        assert_same(Bake(16, sh).queued(ds), bake_yardstick(16, sh), (16, "the handle's own stream again"))
    lit = bake_yardstick(32, sh)[-1]
    assert np.isfinite(lit[:, :3]).all() and (lit[:, :3] > 0).any()  # (the bake shows the light: the chains compare more than zeros)
