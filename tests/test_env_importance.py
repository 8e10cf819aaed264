"""Environment importance sampling (EXTENSION): sol_env_sampling, sol_env_sampling_check, sol_env_tables, sol_env_eval,
solh_set_env_sampling and RenderConfig(env_sampling=...). The tables are restated in numpy in the documented summation order; the
sampler and its density are judged through the device's own functions; the estimator against the oracle-pinned BSDF-only frames."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import f64_gate
import orc
import parity_util as pu
from solstrale_amd import (AlbedoShader, CameraConfig, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, scenes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = pu.SEED
IMPORTANCE = _abi.SolEnvSampling(size=C.sizeof(_abi.SolEnvSampling), mode=_abi.SOL_ENV_SAMPLING_IMPORTANCE)
# BSDF-only frame variance / IS frame variance on the Lambertian scene under soft_sun_sky(), 128x96, 16 spp: 2.995 measured on the MI355X
# (profiles/env_importance.txt); the bound is half of it, at least 2. (On the sun sky there is no reduction: see the profile.)
VARIANCE_RATIO_BOUND = 2.0


# ---- numpy restatement of the cells, weights and tables (csrc/sol_envmap.hip) ----
def cell_dims(w, h):
    return max(w - 1, 1), max(h - 1, 1)


def np_weights(env):
    h, w, _ = env.shape
    cw, ch = cell_dims(w, h)
    t = np.asarray(env, dtype=np.float32)[:ch, :cw]
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.float32(0.2126) * t[..., 0] + np.float32(0.7152) * t[..., 1]
        y = y + np.float32(0.0722) * t[..., 2]
        s = np.sin(np.pi * (1.0 - (np.arange(ch) + 0.5) / ch)).astype(np.float32)
        wt = y * s[:, None]
    return np.where(np.isfinite(wt) & (wt > 0), wt, np.float32(0)).astype(np.float32)


def np_tables(env):
    wt = np_weights(env)
    ch, cw = wt.shape
    c = np.add.accumulate(wt, axis=1, dtype=np.float32)
    rows = c[:, -1]
    uniform = np.arange(1, cw + 1, dtype=np.float32) / np.float32(cw)
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.where(rows[:, None] > 0, c / rows[:, None], uniform[None, :]).astype(np.float32)
    m = np.add.accumulate(rows, dtype=np.float32)
    return (m / m[-1]).astype(np.float32), cond, np.float32(m[-1])


def np_cell(d, w, h):
    """The cell of directions d (n, 3) by env_color's mapping (sol_path.h / oracle.cpp env_color), in f64, clamped into the cells."""
    cw, ch = cell_dims(w, h)
    n = d / np.linalg.norm(d, axis=-1, keepdims=True)
    theta = np.arccos(np.clip(-n[..., 1], -1.0, 1.0))
    phi = -np.arctan2(n[..., 2], n[..., 0]) + np.pi
    u, v = phi / (2 * np.pi), theta / np.pi
    i = np.clip(np.floor(u * cw), 0, cw - 1).astype(np.int64)
    j = np.clip(np.floor((1.0 - v) * ch), 0, ch - 1).astype(np.int64)
    return i, j


def _scene_with_env(env, scale=1.0, rc=None, light=True):
    b = SceneBuilder()
    lamb = b.Lambertian(b.SolidColor(.5, .45, .4))
    objs = [b.Sphere((0., 1., 0.), 1., lamb), b.Quad((-6., 0., -6.), (12., 0., 0.), (0., 0., 12.), b.Lambertian(b.SolidColor(.4, .4, .4)))]
    if light:
        objs.append(b.Quad((-1., 4., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(1., 1., 1.)))
    if env is not None:
        b.environment(env, scale)
    cam = CameraConfig(40., 0., (0., 2., 7.), (0., 1., 0.), (0., 1., 0.))
    return b.finish(b.Bvh(objs), cam, (.2, .3, .4), rc or RenderConfig(64, 48, 16, PathTracingShader(8)))


def _ragged_map():
    rng = np.random.default_rng(7)
    env = rng.uniform(0.0, 2.0, (5, 37, 3)).astype(np.float32)
    env[2] = 0.0           # a row of weight 0: never drawn, uniform conditional CDF
    env[0, 3] = -1.0       # weights that are not above 0 count as 0
    env[1, 36] = 1e6       # the last column has no cell: it must not count
    return env


# ---- CPU ----
def test_entry_points_and_struct_layout(tmp_path):
    lib = _abi.load_hip()
    for n in ("sol_env_sampling", "sol_env_sampling_check", "sol_env_tables", "sol_env_eval"):
        assert hasattr(lib, n) and n in _abi.HIP_SYMBOLS
    assert hasattr(_abi.load_host(), "solh_set_env_sampling")
    assert _abi.SolEnvSampling not in _abi.ABI_STRUCTS and len(_abi.ABI_STRUCTS) == 11
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "probe.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "solstrale_hip.h"
#include "solstrale_host.h"
int main(void) {
  printf("%u %u %u %u %u %u\\n", (unsigned)sizeof(SolEnvSampling), (unsigned)offsetof(SolEnvSampling, size), (unsigned)offsetof(SolEnvSampling, mode),
         (unsigned)offsetof(SolEnvSampling, reserved), SOL_ENV_SAMPLING_OFF, SOL_ENV_SAMPLING_IMPORTANCE);
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _abi.SolEnvSampling
    assert got == [C.sizeof(S), S.size.offset, S.mode.offset, S.reserved.offset, 0, 1] and C.sizeof(S) == 16


@pytest.mark.parametrize("bad", [dict(size=8), dict(mode=2), dict(mode=0xFFFFFFFF), dict(reserved=(C.c_uint32 * 2)(0, 1))],
                         ids=["size", "mode2", "mode_max", "reserved"])
def test_configuration_errors_need_no_device(bad):
    lib = _abi.load_hip()
    cfg = dict(size=C.sizeof(_abi.SolEnvSampling), mode=1)
    cfg.update(bad)
    c = _abi.SolEnvSampling(**cfg)
    assert lib.sol_env_sampling(None, C.byref(c)) == _abi.SOL_EINVAL
    assert b"sol_env_sampling" in lib.sol_last_error()  # refused for the configuration, not for the missing scene
    sc = _scene_with_env(scenes.procedural_sky(32, 16))
    assert lib.sol_env_sampling_check(sc.desc_ptr, C.byref(c)) == _abi.SOL_EINVAL


def test_scene_errors_need_no_device():
    lib = _abi.load_hip()
    assert lib.sol_env_sampling(None, C.byref(IMPORTANCE)) == _abi.SOL_EINVAL and lib.sol_last_error() == b"null scene"
    assert lib.sol_env_sampling(None, None) == _abi.SOL_EINVAL
    assert lib.sol_env_tables(None, None, 0, None, 0, None) == _abi.SOL_EINVAL
    assert lib.sol_env_eval(None, 0, None, 0, None) == _abi.SOL_EINVAL
    check = lambda sc, cfg=IMPORTANCE: lib.sol_env_sampling_check(sc.desc_ptr, C.byref(cfg) if cfg is not None else None)
    assert check(_scene_with_env(scenes.procedural_sky(32, 16))) == _abi.SOL_OK
    assert check(_scene_with_env(_ragged_map())) == _abi.SOL_OK
    no_env = _scene_with_env(None)
    assert check(no_env) == _abi.SOL_EINVAL and b"no environment" in lib.sol_last_error()
    assert check(no_env, None) == _abi.SOL_OK  # off is always allowed
    assert check(no_env, _abi.SolEnvSampling(size=C.sizeof(_abi.SolEnvSampling), mode=0)) == _abi.SOL_OK
    zero = np.zeros((16, 32, 3), np.float32)
    zero[:, -1] = 5.0   # the last column has no cell
    zero[-1, :] = 5.0   # nor has the last row
    zero[3, 4] = (-1.0, -2.0, -3.0)  # negative luminance: weight 0
    assert check(_scene_with_env(zero)) == _abi.SOL_EINVAL and b"weight 0" in lib.sol_last_error()
    for scale in (0.0, -1.0):
        sc = _scene_with_env(scenes.procedural_sky(32, 16))
        sc.desc.env_scale = scale
        assert check(sc) == _abi.SOL_EINVAL and b"env_scale" in lib.sol_last_error()
    sc = _scene_with_env(scenes.procedural_sky(32, 16))
    sc.desc.abi_version = 1  # a version-1 description has no environment fields
    assert check(sc) == _abi.SOL_EINVAL


def test_host_mirror_rejects_unknown_modes():
    lib = _abi.load_host()
    b = lib.solh_builder_new()
    try:
        assert lib.solh_set_env_sampling(b, 0) == 0
        assert lib.solh_set_env_sampling(b, 1) == 0
        for m in (2, 7, 0xFFFFFFFF):
            assert lib.solh_set_env_sampling(b, m) < 0, m
            assert b"solh_set_env_sampling" in lib.solh_last_error()
    finally:
        lib.solh_builder_free(b)
    with pytest.raises(ValueError):
        RenderConfig(16, 16, 1, env_sampling="uniform")
    assert RenderConfig(16, 16, 1).env_sampling is None and RenderConfig(16, 16, 1, env_sampling="importance").env_sampling == "importance"


def _sky_scene(look_at, env, w=48, h=32, fov=70.0):
    """Nothing in view: the AlbedoShader frame is the environment seen through the camera (tests/test_environment.py's sky scene)."""
    b = SceneBuilder()
    light = b.Sphere((0., -1e5, 0.), 1., b.DiffuseLight(1, 1, 1))
    b.environment(env, 2.0)
    cam = CameraConfig(fov, 0., (0., 0., 0.), look_at, (0., 1., 0.) if abs(look_at[1]) < 0.9 else (1., 0., 0.))
    return b.finish(b.Bvh([light, light]), cam, (9., 9., 9.), RenderConfig(w, h, 1, AlbedoShader()))


def _pixel_rays(sc, px, py):
    """Camera rays through (px + a, py + b) of every pixel (generate_path without the jitter's draws)."""
    cam = sc.desc.camera
    o, llc, hor, ver = (np.array(getattr(cam, k)[:]) for k in ("origin", "lower_left_corner", "horizontal", "vertical"))
    W, H = sc.width, sc.height
    u = px / (W - 1)
    v = ((H - 1) - py) / (H - 1)  # (py counted from the top; the jitter adds to y_ref = H - 1 - py)
    return llc + hor * u[..., None] + ver * v[..., None] - o


@pytest.mark.parametrize("W,H", [(16, 8), (1, 8), (16, 1), (2, 2), (1, 1), (2, 5), (7, 2)])
def test_cells_are_the_texels_the_oracle_reads(W, H):
    """Cell (i, j) = texel (i, j): numpy's cell of a direction is the texel the f64 oracle shows for it. A pixel's ray is jittered by up to one
    pixel: pixels whose footprint spans more than one cell are not judged."""
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    env = np.stack([ii, jj, np.ones_like(ii)], -1).astype(np.float32)
    judged = 0
    for look in ((1., 0., 0.), (0., 0., 1.), (-1., 0.2, 0.3), (0., 1., 0.), (0., -1., 0.), (1., 1., -1.)):
        sc = _sky_scene(look, env)
        img, _ = orc.render(sc, 0, 1, SEED, real=orc.ORC_F64)
        ti, tj = np.rint(img[..., 0] / 2.0).astype(int), np.rint(img[..., 1] / 2.0).astype(int)
        py, px = np.mgrid[0:sc.height, 0:sc.width].astype(np.float64)
        cells = [np_cell(_pixel_rays(sc, px + a, py - b), W, H) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1), (.5, .5))]
        same = np.all([(c[0] == cells[0][0]) & (c[1] == cells[0][1]) for c in cells], axis=0)
        assert (ti[same] == cells[0][0][same]).all() and (tj[same] == cells[0][1][same]).all(), (look, W, H)
        judged += int(same.sum())
    assert judged > 0.5 * 6 * 48 * 32


# ---- GPU ----
def _frame(ds, n, seed=SEED):
    ds.clear()
    ds.render(0, n, seed)
    return ds.read()


@pytest.mark.gpu
def test_default_frames_are_unchanged():
    sc = scenes.create_test_scene_with_environment(RenderConfig(64, 48, 16, PathTracingShader(50)))
    with DeviceScene(sc) as ds:
        base = _frame(ds, 16)
        ds.env_sampling(0)
        assert np.array_equal(_frame(ds, 16), base)
        ds.env_sampling("importance")
        on = _frame(ds, 16)
        assert not np.array_equal(on, base) and np.isfinite(on).all()
        ds.env_sampling(None)
        assert np.array_equal(_frame(ds, 16), base)
    ref, _ = orc.render(sc, 0, 16, SEED, real=orc.ORC_F32)
    res = pu.compare(base, ref, 16)
    assert res["bad_pixels"] == 0, res  # (and the default is still the oracle's frame)


@pytest.mark.gpu
def test_refusals_on_the_device():
    with DeviceScene(_scene_with_env(None)) as ds:
        with pytest.raises(Exception, match="no environment"):
            ds.env_sampling("importance")
        with pytest.raises(Exception):
            ds.env_tables()
        ds.env_sampling(0)
    sc = _scene_with_env(scenes.procedural_sky(32, 16))
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        lib = ds.lib
        rows = (C.c_float * 48)()
        assert lib.sol_render_counted(ds.h, 0, 16, SEED) == _abi.SOL_EINVAL
        assert lib.sol_debug_path(ds.h, 1, 1, 0, SEED, rows, 4) == _abi.SOL_EINVAL and b"sol_debug_path" in lib.sol_last_error()
        ds.env_sampling(0)
        ds.render(0, 16, SEED, counted=True)  # usable again


@pytest.mark.gpu
@pytest.mark.parametrize("env", [scenes.procedural_sky(256, 128), _ragged_map()], ids=["sky_256x128", "ragged_37x5"])
def test_tables_match_the_numpy_restatement(env):
    sc = _scene_with_env(env)
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        marg, cond, total = ds.env_tables()
    m, c, t = np_tables(env)
    assert marg.tobytes() == m.tobytes()
    assert cond.tobytes() == c.tobytes()
    assert np.float32(total) == t
    assert marg[-1] == 1.0 and (np.diff(marg) >= 0).all()


@pytest.mark.gpu
def test_tables_and_frames_are_deterministic_across_handles():
    sc = scenes.create_test_scene_with_environment(RenderConfig(96, 64, 16, PathTracingShader(50)))
    out = []
    with DeviceScene(sc) as a, DeviceScene(sc) as b:
        for ds in (a, b):
            ds.env_sampling("importance")
            marg, cond, total = ds.env_tables()
            out.append((marg.tobytes() + cond.tobytes(), total, zlib.crc32(_frame(ds, 32).tobytes())))
    assert out[0] == out[1]


@pytest.mark.gpu
def test_sampler_and_pdf():
    env = scenes.procedural_sky(256, 128)
    H, W, _ = env.shape
    cw, ch = cell_dims(W, H)
    n = 1 << 20
    rng = np.random.default_rng(1234)
    r = (rng.integers(0, 1 << 24, (n, 2)) * 2.0 ** -24).astype(np.float32)  # the renderer's draws: multiples of 2^-24 in [0, 1)
    with DeviceScene(_scene_with_env(env)) as ds:
        ds.env_sampling("importance")
        s = ds.env_eval("sample", r)
        d = s[:, :3]
        p = ds.env_eval("pdf", d)
        # quadrature: 4 x 4 points per cell, integrand p * 2 pi^2 sin(theta) du dv (constant on a cell)
        k = 4
        uu = (np.arange(cw * k) + 0.5) / (cw * k)
        ww = (np.arange(ch * k) + 0.5) / (ch * k)  # 1 - v
        U, Wv = np.meshgrid(uu, ww)
        theta, phi = np.pi * (1.0 - Wv), 2.0 * np.pi * U
        q = np.stack([-np.sin(theta) * np.cos(phi), -np.cos(theta), np.sin(theta) * np.sin(phi)], -1).reshape(-1, 3)
        pq = ds.env_eval("pdf", q)[:, 0].astype(np.float64)
    si, sj = s[:, 4].astype(np.int64), s[:, 5].astype(np.int64)
    assert np.linalg.norm(d, axis=1).max() < 1 + 1e-5 and np.isfinite(s).all()
    # the cell of every direction under env_color's mapping is the sampled one, but for a handful at cell borders, which are neighbours
    ni, nj = np_cell(d.astype(np.float64), W, H)
    off = (ni != si) | (nj != sj)
    assert off.sum() <= 1e-4 * n, off.sum()
    di = np.abs(ni - si)
    assert ((np.minimum(di, cw - di) <= 1) & (np.abs(nj - sj) <= 1))[off].all()
    # pdf(sample(r)) is the sampler's own pdf
    same = (p[:, 1].astype(np.int64) == si) & (p[:, 2].astype(np.int64) == sj)
    assert same.mean() > 0.999
    np.testing.assert_allclose(p[same, 0], s[same, 3], rtol=1e-5)
    assert (s[:, 3] > 0).all()
    # chi-square of the cell histogram against w / sum(w) (cells expecting fewer than 5 pooled)
    wt = np_weights(env).astype(np.float64)
    expect = (wt / wt.sum()).ravel() * n
    got = np.bincount(sj * cw + si, minlength=cw * ch).astype(np.float64)
    assert got[expect == 0].sum() == 0
    big = expect >= 5
    e = np.append(expect[big], expect[~big].sum())
    o = np.append(got[big], got[~big].sum())
    keep = e > 0
    chi2 = float((((o - e) ** 2)[keep] / e[keep]).sum())
    from scipy.stats import chi2 as chi2_dist
    pval = float(chi2_dist.sf(chi2, keep.sum() - 1))
    assert pval > 1e-3, (chi2, keep.sum(), pval)
    # the density integrates to 1 over the sphere
    integral = float((pq * 2.0 * np.pi ** 2 * np.sin(theta.ravel())).sum() / (cw * k * ch * k))
    assert abs(integral - 1.0) < 1e-3, integral


def _smooth_sky(w=64, h=32, top=1.2, bottom=0.2):
    """A smooth non-uniform sky, radiance <= 1.2, no sun."""
    v = (np.arange(h) + 0.5) / h
    u = (np.arange(w) + 0.5) / w
    base = bottom + (top - bottom) * (1.0 - v)[:, None] * (0.75 + 0.25 * np.cos(2 * np.pi * u))[None, :]
    return np.stack([base, base * 0.9, base * 0.8], -1).astype(np.float32)


def soft_sun_sky(w=128, h=64, sun_dir=(0.45, 0.7, -0.55), radius_deg=8.0, sun=3.0):
    """The smooth sky (radiance 0.1 .. 0.4) with a soft sun: a disc of radiance 3 and radius 8 degrees - a peaked map on which the min(3) filter
    of a Lambertian scene with albedo <= 0.5 still never binds (factor <= 1 per level, radiance <= 3)."""
    env = _smooth_sky(w, h, top=0.4, bottom=0.1)
    theta = np.pi * ((np.arange(h) + 0.5) / h)[:, None] * np.ones((1, w))  # row 0 = up: theta = pi (1 - (1 - v)), y = -cos(theta)
    phi = 2.0 * np.pi * ((np.arange(w) + 0.5) / w)[None, :] * np.ones((h, 1))
    d = np.stack([-np.sin(np.pi - theta) * np.cos(phi), np.cos(theta), np.sin(np.pi - theta) * np.sin(phi)], -1)
    sd = np.asarray(sun_dir, np.float64) / np.linalg.norm(sun_dir)
    env[(d @ sd) > np.cos(np.radians(radius_deg))] = sun
    return env


def _lambertian_scene(rc, env=None):
    """Lambertian only (albedo <= 0.5: every level's factor is <= 1, so the min(3) filter never binds while radiance <= 3) under the smooth sky
    (or `env`) and one dim quad light."""
    b = SceneBuilder()
    objs = [b.Sphere((0., 1., 0.), 1., b.Lambertian(b.SolidColor(.5, .4, .3))),
            b.Sphere((-2.2, .7, .8), .7, b.Lambertian(b.SolidColor(.2, .45, .35))),
            b.Quad((-6., 0., -6.), (12., 0., 0.), (0., 0., 12.), b.Lambertian(b.SolidColor(.45, .45, .45))),
            b.Quad((1.5, 3., -1.), (1.5, 0., 0.), (0., 0., 1.5), b.DiffuseLight(1.2, 1.1, 1.0))]
    b.environment(_smooth_sky() if env is None else env, 1.0)
    cam = CameraConfig(40., 0., (0., 2.5, 7.), (0., .8, 0.), (0., 1., 0.))
    return b.finish(b.Bvh(objs), cam, (0., 0., 0.), rc)


# the shape of f64_gate.BOUNDS: (rel_of_noise, apart, |z|, |rays rel|). The IS frame follows other paths than the f64 BSDF-only frame: its
# noise adds to the f64 sets' (rel bound in noise units 4, |z| 4), every pixel is "apart", and rays are not judged (the window's rays are the
# float oracle's BSDF-only count: counted renders refuse importance sampling)
UNBIASED_BOUNDS = (4.0, 1.01, 4.0, 3e-3)


@pytest.mark.gpu
def test_unbiased_where_the_filter_cannot_bind():
    spp, rect = 256, (24, 24, 88, 72)
    sc = _lambertian_scene(RenderConfig(112, 84, spp, PathTracingShader(6)))
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        is_frame = _frame(ds, spp)
        ds.env_sampling(0)
        bsdf_frame = _frame(ds, spp)

    def fp32_window_rays(win, n):
        _, st = orc.render(win, 0, n, SEED, real=orc.ORC_F32)
        return st["live_rays"], st["samples"]

    m = f64_gate.measure(sc, rect, spp, lambda s, n, r: is_frame, fp32_window_rays)
    assert m["mean_f64"] > 0 and not f64_gate.exceeded(m, UNBIASED_BOUNDS), (f64_gate.exceeded(m, UNBIASED_BOUNDS), m)
    # and against the device's own BSDF-only frame, over the whole image: the two estimators' pixel differences are zero-mean noise
    d = (is_frame.astype(np.float64) - bsdf_frame.astype(np.float64)).sum(axis=-1) / spp
    z = d.sum() / np.sqrt((d ** 2).sum())
    assert abs(z) < 4.0, z
    assert abs(is_frame.mean() / bsdf_frame.mean() - 1.0) < 0.01


@pytest.mark.gpu
def test_furnace():
    """A large quad of albedo a seen head-on under a constant sky L (the light hides behind it): every camera ray sees a * L."""
    a, L, spp = 0.5, 0.8, 64
    b = SceneBuilder()
    wall = b.Quad((-500., -500., 0.), (1000., 0., 0.), (0., 1000., 0.), b.Lambertian(b.SolidColor(a, a, a)))
    light = b.Sphere((0., 0., -50.), 1., b.DiffuseLight(1., 1., 1.))
    b.environment(np.full((8, 16, 3), L, np.float32), 1.0)
    cam = CameraConfig(30., 0., (0., 0., 10.), (0., 0., 0.), (0., 1., 0.))
    sc = b.finish(b.Bvh([wall, light]), cam, (0., 0., 0.), RenderConfig(64, 64, spp, PathTracingShader(4)))
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        img = _frame(ds, spp).astype(np.float64) / spp
    px = img.mean(axis=-1).ravel()
    err = px.std() / np.sqrt(px.size)
    assert abs(px.mean() - a * L) < 4.0 * err + 1e-6, (px.mean(), a * L, err)


def _two_seed_variance(ds, spp):
    f1 = _frame(ds, spp, SEED).astype(np.float64) / spp
    f2 = _frame(ds, spp, SEED + 1).astype(np.float64) / spp
    return float(((f1 - f2) ** 2).mean() / 2.0)


@pytest.mark.gpu
def test_importance_sampling_reduces_noise_where_the_filter_cannot_bind():
    spp = 16
    sc = _lambertian_scene(RenderConfig(128, 96, spp, PathTracingShader(6)), soft_sun_sky())
    with DeviceScene(sc) as ds:
        off = _two_seed_variance(ds, spp)
        ds.env_sampling("importance")
        on = _two_seed_variance(ds, spp)
    print(f"soft sun: two-seed variance BSDF-only {off:.5g}, importance {on:.5g}, ratio {off / on:.3f}")
    assert off / on >= VARIANCE_RATIO_BOUND, (off, on)


@pytest.mark.gpu
def test_sun_sky_frame_is_brighter_where_the_filter_binds():
    """Under procedural_sky's sun (radiance 60) the BSDF-only estimator clips nearly every sun hit to 3; the IS frame draws the sun often with
    small factors and clips less of its energy: brighter, by many standard errors of the difference. (Its variance is about the BSDF-only
    frame's - profiles/env_importance.txt: under the clip the two estimate different amounts of sunlight.)"""
    spp = 64
    sc = _lambertian_scene(RenderConfig(128, 96, spp, PathTracingShader(6)), scenes.procedural_sky(256, 128))
    with DeviceScene(sc) as ds:
        off = [_frame(ds, spp, s).astype(np.float64) / spp for s in (SEED, SEED + 1)]
        ds.env_sampling("importance")
        on = [_frame(ds, spp, s).astype(np.float64) / spp for s in (SEED, SEED + 1)]
    gain = (on[0] - off[0]).sum(axis=-1)
    spread = np.sqrt(((on[0] - on[1]).sum(axis=-1) ** 2 + (off[0] - off[1]).sum(axis=-1) ** 2).sum() / 2.0)  # std of gain.sum(), two-seed pairs
    print(f"sun sky: mean BSDF-only {off[0].mean():.5f}, importance {on[0].mean():.5f}, z {gain.sum() / spread:.1f}, variance ratio "
          f"{((off[0] - off[1]) ** 2).mean() / ((on[0] - on[1]) ** 2).mean():.3f}")
    assert gain.sum() > 6.0 * spread


@pytest.mark.gpu
def test_adaptive_threshold_zero_is_the_fixed_frame():
    sc = scenes.create_test_scene_with_environment(RenderConfig(72, 40, 48, PathTracingShader(50)))
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        fixed = _frame(ds, 48)
        ds.adaptive_begin(16, 16, 48, 0.0)
        ds.adaptive_run(SEED)
        assert ds.read().tobytes() == fixed.tobytes()
        ds.env_sampling(0)
        assert not np.array_equal(_frame(ds, 48), fixed)


@pytest.mark.gpu
def test_ray_trace_with_env_sampling():
    rc = RenderConfig(64, 48, 32, PathTracingShader(50), env_sampling="importance")
    sc = scenes.create_test_scene_with_environment(rc)
    _, last = sc.ray_trace()
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        ds.render(0, 32, rc.seed)
        want = ds.tonemap_rgb8(ds.resolve_image(), 32)
        ds.env_sampling(0)
        _frame(ds, 32, rc.seed)
        plain = ds.tonemap_rgb8(ds.resolve_image(), 32)
    assert last is not None and (last == want).all() and not (last == plain).all()
    no_env = _scene_with_env(None, rc=RenderConfig(32, 32, 16, PathTracingShader(8), env_sampling="importance"))
    with pytest.raises(Exception, match="no environment"):
        no_env.ray_trace()
