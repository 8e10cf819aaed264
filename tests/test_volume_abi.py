"""Irradiance volumes (sol_volume_points / sol_volume_build / sol_volume_sample), the part that needs no GPU: the six entry points
are exported and declared, the header is still C99, SolVolumeGrid (48 bytes) and SolProbe (128 bytes) have the same size and offsets from gcc and
from ctypes, every refusal answers SOL_EINVAL in the stated order and in front of the device check with nothing written, the kernels are in the
library - and the restatement the GPU tests compare against (tests/volume_ref.py) has the rule's own properties: constant radiance gives pi x L
everywhere, a linear field is reproduced, the variance test and the backface weight do what they say, skipped probes are counted out.

The bound of the two exact properties, 1e-5 relative: 4 pi^2 k0^2 = pi and trilinear weights reproduce a linear field, so both are exact in real
arithmetic; the chain from the sums to the answer is about fifteen fp32 roundings of 2^-24 = 6e-8 each, 9e-7 in sum, and the bound is about ten
times that."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import volume_ref as vr
from solstrale_amd import VOLUME_PROBE_DTYPE, VolumeGrid, _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_volume_points_dev", "sol_volume_points", "sol_volume_build_dev", "sol_volume_build", "sol_volume_sample_dev", "sol_volume_sample")
GRID = _abi.SolVolumeGrid
GRID_OFFSETS = {"size": 0, "nx": 4, "ny": 8, "nz": 12, "origin": 16, "spacing": 28, "flags": 40, "normal_bias": 44}
PROBE_OFFSETS = {"e": 0, "mean": 108, "mean2": 112, "flags": 116, "samples": 120, "reserved": 124}
F, U = np.float32, np.uint32
INF, NAN = float("inf"), float("nan")
RTOL = 1e-5


def test_the_six_entry_points_are_exported_and_declared():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, const SolVolumeGrid\* grid,", text), name
        assert getattr(lib, name).argtypes is not None
    assert len(lib.sol_volume_points.argtypes) == len(lib.sol_volume_points_dev.argtypes) == 5
    assert len(lib.sol_volume_build.argtypes) == len(lib.sol_volume_build_dev.argtypes) == 6
    assert len(lib.sol_volume_sample.argtypes) == len(lib.sol_volume_sample_dev.argtypes) == 6
    assert re.search(r"#define SOL_ABI_VERSION 2\b", text)
    for name, value in (("SOL_VOLUME_BACKFACE", 1), ("SOL_VOLUME_CHEBYSHEV", 2), ("SOL_VOLUME_MAX_PROBES", 1 << 24), ("SOL_PROBE_VALID", 1), ("SOL_PROBE_MOMENTS", 2)):
        assert getattr(_abi, name) == value and re.search(rf"#define {name} {value}u", text), name


def test_the_structs_agree_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    assert C.sizeof(GRID) == 48 and C.sizeof(_abi.SolProbe) == 128
    assert {n: getattr(GRID, n).offset for n, _ in GRID._fields_} == GRID_OFFSETS
    assert {n: getattr(_abi.SolProbe, n).offset for n, _ in _abi.SolProbe._fields_} == PROBE_OFFSETS
    dt = VOLUME_PROBE_DTYPE
    assert dt.itemsize == 128 and {n: dt.fields[n][1] for n in dt.names} == PROBE_OFFSETS and dt == vr.PROBE_DTYPE
    fields = ", ".join([f"(unsigned)offsetof(SolVolumeGrid, {n})" for n in GRID_OFFSETS] + [f"(unsigned)offsetof(SolProbe, {n})" for n in PROBE_OFFSETS])
    count = 2 + len(GRID_OFFSETS) + len(PROBE_OFFSETS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", (unsigned)sizeof(SolVolumeGrid), (unsigned)sizeof(SolProbe), {fields});\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [48, 128] + list(GRID_OFFSETS.values()) + list(PROBE_OFFSETS.values())
    rec = VolumeGrid((1, 2, 3), (0.5, 0.25, 2.0), (4, 5, 6), backface=False, normal_bias=0.125).record()
    assert (rec.size, rec.nx, rec.ny, rec.nz, rec.flags, rec.normal_bias) == (48, 4, 5, 6, 2, 0.125)
    assert tuple(rec.origin) == (1, 2, 3) and tuple(rec.spacing) == (0.5, 0.25, 2.0)
    for counts in ((-1, 2, 2), (2, 1 << 32, 2)):  # (named where they are made, not wrapped into another count)
        with pytest.raises(ValueError, match="counts"):
            VolumeGrid((0, 0, 0), 1.0, counts)


def _grid(**kw):
    g = GRID(size=C.sizeof(GRID), nx=2, ny=2, nz=1, flags=3, normal_bias=0.0)
    g.origin[:] = (0.0, 0.0, 0.0)
    g.spacing[:] = (1.0, 1.0, NAN)  # (one probe along z: its spacing is never read)
    for k, v in kw.items():
        if k in ("origin", "spacing"):
            axis, value = v
            getattr(g, k)[axis] = value
        else:
            setattr(g, k, v)
    return g


# what all three calls refuse, in the header's order: (fields of the grid to break, the word sol_last_error must hold)
GRID_STEPS = [(dict(scene=None), b"null scene"), (dict(grid_null=True), b"null grid"), (dict(g=dict(size=44)), b"size"), (dict(g=dict(flags=4)), b"flags"),
              (dict(g=dict(ny=0)), b"at least 1"), (dict(g=dict(nx=4097, ny=4097)), b"2^24"), (dict(g=dict(origin=(1, INF))), b"origin"),
              (dict(g=dict(spacing=(0, 0.0))), b"spacing"), (dict(g=dict(normal_bias=NAN)), b"normal_bias")]


def _refusals(names, steps, good, call):
    """Each bad argument alone, then paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    for name in names:
        fn = getattr(lib, name)
        for k, (broken, word) in enumerate(steps):
            assert call(fn, {**good, **broken}) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:
                args = {**good, **later, **broken, "g": {**later.get("g", {}), **broken.get("g", {})}}
                assert call(fn, args) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())


def _grid_arg(a):
    return None if a.get("grid_null") else C.byref(_grid(**a["g"]))


def test_every_refusal_of_volume_points_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of the device check reads the handle."""
    stand_in = C.create_string_buffer(1 << 20)
    points = (C.c_float * (4 * 8))()
    good = dict(scene=stand_in, g={}, tmin=1e-3, tmax=INF, points=points)
    steps = GRID_STEPS + [(dict(tmin=-1.0), b"tmin"), (dict(tmax=NAN), b"tmin"), (dict(tmin=2.0, tmax=1.0), b"tmin"), (dict(points=None), b"null point output")]
    _refusals(("sol_volume_points", "sol_volume_points_dev"), steps, good, lambda fn, a: fn(a["scene"], _grid_arg(a), a["tmin"], a["tmax"], a["points"]))
    assert bytes(points) == bytes(4 * 8 * 4)  # nothing was written


def test_every_refusal_of_volume_build_comes_in_the_stated_order_before_the_device():
    stand_in = C.create_string_buffer(1 << 20)
    sh, vis, probes = (C.c_float * (4 * 28))(), (C.c_float * (4 * 8))(), (C.c_float * (4 * 32))()
    good = dict(scene=stand_in, g={}, sh=sh, vis=vis, probes=probes)
    steps = GRID_STEPS + [(dict(sh=None), b"null SolSh9"), (dict(probes=None), b"null probe output")]
    _refusals(("sol_volume_build", "sol_volume_build_dev"), steps, good, lambda fn, a: fn(a["scene"], _grid_arg(a), a["sh"], a["vis"], 1.0, a["probes"]))
    assert bytes(probes) == bytes(4 * 32 * 4)


def test_every_refusal_of_volume_sample_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    probes, points, out = (C.c_float * (4 * 32))(), (C.c_float * (3 * 8))(), (C.c_float * (3 * 4))()
    good = dict(scene=stand_in, g={}, probes=probes, points=points, n=3, out=out)
    steps = GRID_STEPS + [(dict(n=(1 << 31) + 1), b"2^31"), (dict(probes=None), b"null probe"), (dict(points=None), b"null point"), (dict(out=None), b"null output")]

    def call(fn, a):
        return fn(a["scene"], _grid_arg(a), a["probes"], a["points"], a["n"], a["out"])

    _refusals(("sol_volume_sample", "sol_volume_sample_dev"), steps, good, call)
    for name in ("sol_volume_sample", "sol_volume_sample_dev"):
        fn = getattr(lib, name)
        # n == 0 succeeds - with null pointers, with or without a device - but only behind the grid's refusals
        assert call(fn, {**good, "n": 0, "probes": None, "points": None, "out": None}) == _abi.SOL_OK, name
        assert call(fn, {**good, "n": 0, "g": dict(nx=0)}) == _abi.SOL_EINVAL, name
    assert bytes(out) == bytes(3 * 4 * 4)


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_valid_arguments_reach_the_device_check():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    sh, probes, points, out = (C.c_float * (4 * 28))(), (C.c_float * (4 * 32))(), (C.c_float * (4 * 8))(), (C.c_float * (4 * 4))()
    g = C.byref(_grid())
    assert lib.sol_volume_points(stand_in, g, 1e-3, INF, points) == _abi.SOL_EDEVICE
    assert lib.sol_volume_points_dev(stand_in, g, 0.0, 0.0, points) == _abi.SOL_EDEVICE
    assert lib.sol_volume_build(stand_in, g, sh, None, NAN, probes) == _abi.SOL_EDEVICE  # (no visibility, any radius: judged per probe)
    assert lib.sol_volume_build_dev(stand_in, g, sh, None, 1.0, probes) == _abi.SOL_EDEVICE
    assert lib.sol_volume_sample(stand_in, g, probes, points, 4, out) == _abi.SOL_EDEVICE
    assert lib.sol_volume_sample_dev(stand_in, g, probes, points, 1 << 31, out) == _abi.SOL_EDEVICE
    assert lib.sol_volume_sample(None, g, probes, points, 4, out) == _abi.SOL_EINVAL


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    for kernel in (b"sol_volume_points_kernel", b"sol_volume_build_kernel", b"sol_volume_sample_kernel"):
        assert kernel in data, kernel


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------------
def _points_in_and_around(grid, rng, n):
    """positions inside the grid and up to two cells outside every face, with unit normals"""
    lo = np.asarray(grid.origin)
    size = np.asarray(grid.spacing) * (np.asarray(grid.counts) - 1)
    pos = lo + rng.uniform(-0.5, 1.5, (n, 3)) * size
    pos[: n // 2] = lo + rng.uniform(0, 1, (n // 2, 3)) * size
    return vr.point_rows(pos, vr.unit_normals(rng, n))


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)], ids=["plain", "backface", "chebyshev", "both"])
def test_constant_radiance_answers_pi_times_the_radiance_everywhere(flags):
    rng = np.random.default_rng(1)
    grid = VolumeGrid((-1.0, 0.5, 2.0), (0.5, 0.75, 1.25), (5, 4, 3), backface=flags[0], chebyshev=flags[1], normal_bias=0.1)
    L = np.array([0.25, 1.0, 3.5])
    sh = vr.constant_sh(grid.n_probes, L, samples=64)
    assert (sh[:, 3:27] == 0).all()
    vis = np.zeros((grid.n_probes, 8), dtype=F)  # every sample a hit at distance 10: the variance test lets everything through
    vis[:, 4], vis[:, 5] = 64 * 10.0, 64 * 100.0
    vis.view(U)[:, 6:8] = 64
    probes = vr.volume_build(sh, vis, radius=20.0)
    assert (probes.view(U)[:, 29] == 3).all() and np.allclose(probes[:, 27], 10.0) and np.allclose(probes[:, 28], 100.0)
    out = vr.volume_sample(grid, probes, _points_in_and_around(grid, rng, 600))
    assert (out.view(U)[:, 3] >= 1).all() and (out.view(U)[:, 3] <= 8).all()
    assert np.abs(out[:, :3] / (np.pi * L) - 1.0).max() < RTOL


def test_a_linear_field_is_reproduced_inside_the_grid_with_both_flags_off():
    rng = np.random.default_rng(2)
    grid = VolumeGrid((-1.0, 0.5, 2.0), (0.5, 0.75, 1.25), (5, 4, 3), backface=False, chebyshev=False)
    slope = np.array([[0.3, -0.2, 0.1], [0.0, 0.5, 0.0], [-0.1, -0.1, 0.4]])  # per channel

    def field(pos):
        return 2.0 + pos.astype(np.float64) @ slope.T  # in [0.9, 4] over the grid: the relative bound means something

    at = vr.probe_positions(grid)
    probes = vr.probes_of_values(field(at))
    size = np.asarray(grid.spacing) * (np.asarray(grid.counts) - 1)
    pos = (np.asarray(grid.origin) + rng.uniform(0, 1, (500, 3)) * size).astype(F)
    out = vr.volume_sample(grid, probes, vr.point_rows(pos, vr.unit_normals(rng, 500)))
    want = field(pos)
    assert want.min() > 0.5
    assert np.abs(out[:, :3] / want - 1.0).max() < RTOL
    assert (out.view(U)[:, 3] == 8).all()  # random points lie on no grid plane
    # outside the grid the answer is the field at the nearest point of the grid's box (the clamp), not the field's own value
    far = vr.volume_sample(grid, probes, vr.point_rows(np.asarray(grid.origin) - 3.0, [(0, 0, 1)]))
    assert np.abs(far[0, :3] / field(at[:1])[0] - 1.0).max() < RTOL and far.view(U)[0, 3] == 1


def _two_probes(values=((1.0, 1.0, 1.0), (5.0, 5.0, 5.0))):
    """two probes along x at x = 0 and x = 4; the point halfway"""
    return vr.probes_of_values(values), vr.point_rows([(2.0, 0.0, 0.0)], [(0, 0, 1)])


def test_the_variance_test_shuts_out_a_probe_that_sees_a_wall_in_front_of_the_point():
    probes, point = _two_probes()
    w = probes.view(U)
    probes[0, 27], probes[0, 28] = 1.0, 1.0  # mean = 1, mean2 = 1: every ray of probe 0 ended at distance 1; the point is 2 away
    w[0, 29] |= vr.MOMENTS
    on = vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=False, chebyshev=True), probes, point)
    off = vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=False, chebyshev=False), probes, point)
    assert on.view(U)[0, 3] == 1 and (on[0, :3] == 5.0).all()   # probe 0 contributes nothing
    assert off.view(U)[0, 3] == 2 and (off[0, :3] == 3.0).all()  # (0.5 * 1 + 0.5 * 5) / 1
    # a probe without the moments bit is left alone, whatever its words say
    w[0, 29] &= ~U(vr.MOMENTS)
    assert (vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=False, chebyshev=True), probes, point) == off).all()
    # variance lets some of it through: mean = 1, mean2 = 2: v = 1, t = 1, h = 1/2, factor 1/8
    probes[0, 28] = 2.0
    w[0, 29] |= vr.MOMENTS
    some = vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=False, chebyshev=True), probes, point)
    assert some.view(U)[0, 3] == 2 and np.allclose(some[0, :3], (0.0625 * 1 + 0.5 * 5) / 0.5625, rtol=RTOL)


def test_the_backface_flag_lowers_the_share_of_a_probe_behind_the_surface():
    probes, point = _two_probes()
    point[0, 4:7] = (1, 0, 0)  # the surface faces +x: probe 0 (x = 0) is behind it, probe 1 (x = 4) in front
    plain = vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=False, chebyshev=False), probes, point)
    back = vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=True, chebyshev=False), probes, point)
    assert (plain[0, :3] == 3.0).all() and back.view(U)[0, 3] == 2
    # behind: c = -1, b = 0, factor 0.2; in front: c = 1, b = 1, factor 1.2 - shares 1/7 and 6/7
    assert np.allclose(back[0, :3], (0.1 * 1 + 0.6 * 5) / 0.7, rtol=RTOL) and (back[0, :3] > plain[0, :3]).all()
    # a point on a probe: l2 == 0, the factor is left out for that probe
    on = vr.point_rows([(0.0, 0.0, 0.0)], [(1, 0, 0)])
    out = vr.volume_sample(VolumeGrid((0, 0, 0), 4.0, (2, 1, 1), backface=True, chebyshev=False), probes, on)
    assert out.view(U)[0, 3] == 1 and (out[0, :3] == 1.0).all()


def test_invalid_probes_and_zero_weight_corners_are_counted_out():
    rng = np.random.default_rng(3)
    grid = VolumeGrid((0, 0, 0), 1.0, (3, 3, 3), backface=False, chebyshev=False)
    probes = vr.probes_of_values(np.full((27, 3), 2.0))
    inside = vr.point_rows([(0.5, 0.5, 0.5)], [(0, 0, 1)])
    assert vr.volume_sample(grid, probes, inside).view(U)[0, 3] == 8
    # points on a plane, on a line and on a probe touch 4, 2 and 1 corners with weight
    for pos, want in (((0.5, 0.5, 1.0), 4), ((0.5, 1.0, 1.0), 2), ((1.0, 1.0, 1.0), 1), ((2.0, 2.0, 2.0), 1), ((0.5, 0.5, 2.0), 4), ((-1.0, 0.5, 0.5), 4)):
        out = vr.volume_sample(grid, probes, vr.point_rows([pos], [(0, 0, 1)]))
        assert out.view(U)[0, 3] == want and (out[0, :3] == 2.0).all(), pos
    # a one-probe axis: the second layer is never looked at
    flat = VolumeGrid((0, 0, 0), (1.0, 1.0, NAN), (3, 3, 1), backface=False, chebyshev=False)
    out = vr.volume_sample(flat, probes[:9], vr.point_rows([(0.5, 0.5, 7.0)], [(0, 0, 1)]))
    assert out.view(U)[0, 3] == 4 and (out[0, :3] == 2.0).all()
    # invalid probes leave: the others are renormalised
    for dead in (1, 3, 7):
        p = probes.copy()
        cell = [(k * 3 + j) * 3 + i for k in (0, 1) for j in (0, 1) for i in (0, 1)]
        p[rng.permutation(cell)[:dead]] = 0
        out = vr.volume_sample(grid, p, inside)
        assert out.view(U)[0, 3] == 8 - dead and np.allclose(out[0, :3], 2.0, rtol=RTOL)
    # all eight invalid: four zero words
    p = probes.copy()
    p[cell] = 0
    assert (vr.volume_sample(grid, p, inside).view(U) == 0).all()
    # and an invalid row: four zero words too
    for bad in ((NAN, 0, 0, 0, 0, 1), (0, INF, 0, 0, 0, 1), (0, 0, 0, 0, 0, 0), (0, 0, 0, 1e-30, 0, 0), (0, 0, 0, 1e30, 0, 0), (0, 0, 0, 0, NAN, 1)):
        row = vr.point_rows([bad[:3]], [bad[3:]])
        assert (vr.volume_sample(grid, probes, row).view(U) == 0).all(), bad


def test_the_build_of_the_restatement_marks_what_it_cannot_use():
    sh = vr.constant_sh(6, (1.0, 2.0, 3.0), samples=16)
    sh.view(U)[1, 27] = 0          # no samples
    sh[2, 5], sh[3, 26] = NAN, INF  # a sum that is not finite
    vis = np.zeros((6, 8), dtype=F)
    vis[:, 4], vis[:, 5] = 8.0, 16.0
    vis.view(U)[:, 3], vis.view(U)[:, 6], vis.view(U)[:, 7] = 12, 4, 16
    vis.view(U)[4, 7] = 0          # a visibility row without samples
    vis[5, 4] = INF
    probes = vr.volume_build(sh, vis, radius=2.0)
    w = probes.view(U)
    assert (w[1:4] == 0).all() and (w[[0, 4, 5], 29] == (3, 1, 1)).all() and (w[[0, 4, 5], 30] == 16).all() and (w[:, 31] == 0).all()
    assert probes[0, 27] == F((8.0 + 12 * 2.0) / 16) and probes[0, 28] == F((16.0 + 12 * 4.0) / 16) and (probes[4:, 27:29] == 0).all()
    assert np.allclose(probes[0, 0:3] * 0.28209479177387814, np.pi * np.array([1.0, 2.0, 3.0]), rtol=RTOL) and (probes[0, 3:27] == 0).all()
    for kw in (dict(visibility=None), dict(visibility=vis, radius=0.0), dict(visibility=vis, radius=INF), dict(visibility=vis, radius=NAN)):
        assert (vr.volume_build(sh, **kw).view(U)[[0, 4, 5], 29] == 1).all(), kw
