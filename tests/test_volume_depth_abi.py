"""Directional distance moments (sol_visibility_oct / sol_volume_build_depth / sol_volume_sample_depth), the part that needs no GPU:
the six entry points are exported and declared, the header is still C99, SolOctConfig (16 bytes), SolOctTexel (16) and SolDepthTexel (8) have
the same size and offsets from gcc and from ctypes, every refusal that needs no handle answers SOL_EINVAL in the stated order and in front of
the device check with nothing written, the kernels are in the library beside the unchanged visibility and radiance families - and the
restatement the GPU tests compare against (tests/depth_ref.py) has the rule's own properties: unit texel directions that encode onto their own
centres, a map that interpolates continuously across every edge and corner, a wall that is seen on one side only, and a sampler that is
sol_volume_sample's wherever the map cannot matter.

Bounds. Directions: a texel direction is a division by a correctly rounded square root of three products, unit within a few 2^-24; 1e-6 as the
issue states. Encode of a texel's own direction: u is recovered through about eight roundings of 6e-8 on numbers below 1 and multiplied by res <=
16, so within 1e-5 texels. Continuity: two directions 2e-6 apart across an edge land 2e-6 x res texels apart after folding, and the map's values
differ by at most 2 per texel (the test function's range), so 1e-4 is ten times what the rule allows; the same function without the fold differs
by more than 0.1 there. The wall case's 1e-3 and exact 1 are the issue's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_ref as dr
import volume_ref as vr
from solstrale_amd import DEPTH_TEXEL_DTYPE, OCT_TEXEL_DTYPE, VolumeGrid, _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_visibility_oct_dev", "sol_visibility_oct", "sol_volume_build_depth_dev", "sol_volume_build_depth", "sol_volume_sample_depth_dev",
                "sol_volume_sample_depth")
CFG_OFFSETS = {"size": 0, "res": 4, "sharpness_log2": 8, "reserved": 12}
OCT_OFFSETS = {"w": 0, "w_open": 4, "wt": 8, "wt2": 12}
DEPTH_OFFSETS = {"mean": 0, "mean2": 4}
GRID, ICFG, OCFG = _abi.SolVolumeGrid, _abi.SolIrradianceConfig, _abi.SolOctConfig
F, U = np.float32, np.uint32
INF, NAN = float("inf"), float("nan")


def test_the_six_entry_points_are_exported_and_declared():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\* scene, ", text), name
        assert getattr(lib, name).argtypes is not None
    assert len(lib.sol_visibility_oct.argtypes) == len(lib.sol_visibility_oct_dev.argtypes) == 7
    assert len(lib.sol_volume_build_depth.argtypes) == len(lib.sol_volume_build_depth_dev.argtypes) == 6
    assert len(lib.sol_volume_sample_depth.argtypes) == len(lib.sol_volume_sample_depth_dev.argtypes) == 8


def test_the_structs_agree_between_gcc_and_ctypes_and_the_header_is_c99(tmp_path):
    records = (("SolOctConfig", _abi.SolOctConfig, 16, CFG_OFFSETS), ("SolOctTexel", _abi.SolOctTexel, 16, OCT_OFFSETS),
               ("SolDepthTexel", _abi.SolDepthTexel, 8, DEPTH_OFFSETS))
    for name, rec, size, offsets in records:
        assert C.sizeof(rec) == size, name
        assert {n: getattr(rec, n).offset for n, _ in rec._fields_} == offsets, name
    for dt, size, offsets in ((OCT_TEXEL_DTYPE, 16, OCT_OFFSETS), (DEPTH_TEXEL_DTYPE, 8, DEPTH_OFFSETS)):
        assert dt.itemsize == size and {n: dt.fields[n][1] for n in dt.names} == offsets
    sizes = ", ".join(f"(unsigned)sizeof({name})" for name, _, _, _ in records)
    fields = ", ".join(f"(unsigned)offsetof({name}, {n})" for name, _, _, offsets in records for n in offsets)
    count = 3 + sum(len(o) for _, _, _, o in records)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   f'  printf("{"%u " * count}", {sizes}, {fields});\n  return 0;\n}}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [16, 16, 8] + [v for _, _, _, o in records for v in o.values()]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
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


def _icfg(**kw):
    c = ICFG(size=C.sizeof(ICFG), samples=1, mode=_abi.SOL_IRRADIANCE_SPHERE)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _ocfg(**kw):
    c = OCFG(size=C.sizeof(OCFG), res=4, sharpness_log2=5, reserved=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


GRID_STEPS = [(dict(scene=None), b"null scene"), (dict(grid_null=True), b"null grid"), (dict(g=dict(size=44)), b"SolVolumeGrid.size"),
              (dict(g=dict(flags=4)), b"flags"), (dict(g=dict(ny=0)), b"at least 1"), (dict(g=dict(nx=4097, ny=4097)), b"2^24"),
              (dict(g=dict(origin=(1, INF))), b"origin"), (dict(g=dict(spacing=(0, 0.0))), b"spacing"), (dict(g=dict(normal_bias=NAN)), b"normal_bias")]
OCT_STEPS = [(dict(oct_null=True), b"null SolOctConfig"), (dict(o=dict(size=12)), b"SolOctConfig.size"), (dict(o=dict(res=5)), b"SolOctConfig.res"),
             (dict(o=dict(sharpness_log2=7)), b"sharpness_log2"), (dict(o=dict(reserved=1)), b"reserved")]


def _merge(good, *parts):
    a = dict(good)
    for part in parts:
        for k, v in part.items():
            a[k] = {**a.get(k, {}), **v} if k in ("g", "o", "c") else v
    return a


def _refusals(names, steps, good, call):
    """Each bad argument alone, then paired with every LATER bad argument of the list; the earlier one must be named."""
    lib = _abi.load_hip()
    err = lib.sol_last_error
    for name in names:
        fn = getattr(lib, name)
        for k, (broken, word) in enumerate(steps):
            assert call(fn, _merge(good, broken)) == _abi.SOL_EINVAL, (name, word)
            assert word in err() and name.encode() + b":" in err(), (name, word, err())
            for later, _ in steps[k + 1:]:
                assert call(fn, _merge(good, later, broken)) == _abi.SOL_EINVAL and word in err(), (name, word, later, err())


def _grid_arg(a):
    return None if a.get("grid_null") else C.byref(_grid(**a["g"]))


def _oct_arg(a):
    return None if a.get("oct_null") else C.byref(_ocfg(**a["o"]))


def test_every_refusal_of_visibility_oct_that_needs_no_handle_comes_in_the_stated_order_before_the_device():
    """With or without a GPU. A zeroed block stands in for a scene: nothing in front of n == 0 reads the handle, and behind it a zeroed handle has no
    medium. sol_visibility's order, the SolOctConfig directly after the SolIrradianceConfig and n."""
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    points, out = (_abi.SolRay * 2)(), (_abi.SolOctTexel * (2 * 256))()
    good = dict(scene=stand_in, c={}, n=2, o={}, points=points, out=out)
    steps = [(dict(scene=None), b"null scene"), (dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=28)), b"SolIrradianceConfig.size"),
             (dict(c=dict(samples=0)), b"samples"), (dict(c=dict(first_sample=0xFFFFFFF0)), b"first_sample"), (dict(n=(1 << 31) + 1), b"2^31"),
             (dict(c=dict(mode=2)), b"unknown mode 2 (SOL_IRRADIANCE_COSINE")] + OCT_STEPS + [(dict(points=None), b"null point"), (dict(out=None), b"null output")]

    def call(fn, a):
        return fn(a["scene"], a["points"], None, a["n"], None if a.get("cfg_null") else C.byref(_icfg(**a["c"])), _oct_arg(a), a["out"])

    _refusals(("sol_visibility_oct", "sol_visibility_oct_dev"), steps, good, call)
    for name in ("sol_visibility_oct", "sol_visibility_oct_dev"):
        fn = getattr(lib, name)
        # n == 0 succeeds - with null pointers, with or without a device - but only behind both configurations
        assert call(fn, _merge(good, dict(n=0, points=None, out=None))) == _abi.SOL_OK, name
        assert call(fn, _merge(good, dict(n=0, o=dict(res=32)))) == _abi.SOL_EINVAL and b"SolOctConfig.res" in lib.sol_last_error(), name
        assert call(fn, _merge(good, dict(n=0, c=dict(samples=0)))) == _abi.SOL_EINVAL, name
        for res in (4, 8, 16):
            for sharp in (0, 6):
                assert call(fn, _merge(good, dict(n=0, o=dict(res=res, sharpness_log2=sharp)))) == _abi.SOL_OK, (name, res, sharp)
    assert bytes(out) == bytes(2 * 256 * 16)  # nothing was written


def test_every_refusal_of_volume_build_depth_comes_in_the_stated_order_before_the_device():
    stand_in = C.create_string_buffer(1 << 20)
    oct_rows, depth = (C.c_float * (4 * 16 * 4))(), (C.c_float * (4 * 16 * 2))()
    good = dict(scene=stand_in, g={}, o={}, radius=2.0, oct=oct_rows, depth=depth)
    steps = GRID_STEPS + OCT_STEPS + [(dict(radius=0.0), b"radius"), (dict(radius=INF), b"radius"), (dict(radius=NAN), b"radius"), (dict(radius=-1.0), b"radius"),
                                      (dict(oct=None), b"null SolOctTexel"), (dict(depth=None), b"null output")]
    _refusals(("sol_volume_build_depth", "sol_volume_build_depth_dev"), steps, good,
              lambda fn, a: fn(a["scene"], _grid_arg(a), a["oct"], _oct_arg(a), a["radius"], a["depth"]))
    assert bytes(depth) == bytes(4 * 16 * 2 * 4)


def test_every_refusal_of_volume_sample_depth_comes_in_the_stated_order_before_the_device():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    probes, depth, points, out = (C.c_float * (4 * 32))(), (C.c_float * (4 * 16 * 2))(), (C.c_float * (3 * 8))(), (C.c_float * (3 * 4))()
    good = dict(scene=stand_in, g={}, o={}, probes=probes, depth=depth, points=points, n=3, out=out)
    steps = GRID_STEPS + OCT_STEPS + [(dict(n=(1 << 31) + 1), b"2^31"), (dict(probes=None), b"null probe"), (dict(depth=None), b"null depth"),
                                      (dict(points=None), b"null point"), (dict(out=None), b"null output")]

    def call(fn, a):
        return fn(a["scene"], _grid_arg(a), a["probes"], a["depth"], _oct_arg(a), a["points"], a["n"], a["out"])

    _refusals(("sol_volume_sample_depth", "sol_volume_sample_depth_dev"), steps, good, call)
    for name in ("sol_volume_sample_depth", "sol_volume_sample_depth_dev"):
        fn = getattr(lib, name)
        assert call(fn, _merge(good, dict(n=0, probes=None, depth=None, points=None, out=None))) == _abi.SOL_OK, name
        assert call(fn, _merge(good, dict(n=0, g=dict(nx=0)))) == _abi.SOL_EINVAL, name
        assert call(fn, _merge(good, dict(n=0, o=dict(res=0)))) == _abi.SOL_EINVAL, name
    assert bytes(out) == bytes(3 * 4 * 4)


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_valid_arguments_reach_the_device_check():
    lib = _abi.load_hip()
    stand_in = C.create_string_buffer(1 << 20)
    points, oct_rows, depth = (_abi.SolRay * 4)(), (C.c_float * (4 * 16 * 4))(), (C.c_float * (4 * 16 * 2))()
    probes, out = (C.c_float * (4 * 32))(), (C.c_float * (4 * 4))()
    g, o, c = C.byref(_grid()), C.byref(_ocfg()), C.byref(_icfg())
    assert lib.sol_visibility_oct(stand_in, points, None, 4, c, o, oct_rows) == _abi.SOL_EDEVICE
    assert lib.sol_visibility_oct_dev(stand_in, points, None, 4, c, o, oct_rows) == _abi.SOL_EDEVICE
    assert lib.sol_volume_build_depth(stand_in, g, oct_rows, o, 1.0, depth) == _abi.SOL_EDEVICE
    assert lib.sol_volume_build_depth_dev(stand_in, g, oct_rows, o, 1.0, depth) == _abi.SOL_EDEVICE
    assert lib.sol_volume_sample_depth(stand_in, g, probes, depth, o, points, 4, out) == _abi.SOL_EDEVICE
    assert lib.sol_volume_sample_depth_dev(stand_in, g, probes, depth, o, points, 1 << 31, out) == _abi.SOL_EDEVICE
    assert lib.sol_visibility_oct(None, points, None, 4, c, o, oct_rows) == _abi.SOL_EINVAL


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    each = set(re.findall(rb"_Z21sol_depth_each_kernelILb[01]ELb[01]EE", data))
    assert len(each) == 4, sorted(each)  # <SPILL, STRICT>: every combination
    project = set(re.findall(rb"_Z24sol_depth_project_kernelILi(?:4|8|16)EE", data))
    assert len(project) == 3, sorted(project)
    for kernel in (b"sol_depth_project_plain_kernel", b"sol_depth_build_kernel", b"sol_volume_sample_depth_kernel"):
        assert kernel in data, kernel
    # the visibility and radiance families are what they were (tests/test_visibility_abi.py)
    assert len(set(re.findall(rb"_Z21sol_visibility_kernelILb[01]ELb[01]ELb[01]EE", data))) == 8
    gather = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb1EE", data))
    plain = set(re.findall(rb"_Z19sol_radiance_kernelILb[01]ELb[01]ELb[01]ELb[01]ELb0EE", data))
    radiance_each = set(re.findall(rb"_Z24sol_radiance_each_kernelILb[01]ELb[01]ELb[01]ELb[01]EE", data))
    assert (len(gather), len(plain), len(radiance_each)) == (10, 10, 10)


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [4, 8, 16])
def test_texel_directions_are_unit_and_encode_onto_their_own_centres(res):
    T = dr.texel_directions(res)
    assert T.dtype == F and T.shape == (res * res, 3)
    length = np.sqrt((T.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length - 1).max() <= 1e-6
    rows, wts = dr.lookup([T[:, 0], T[:, 1], T[:, 2]], res)
    # a centre is texel coordinate (i, j) exactly: all of the weight on one texel, the texel itself - up to 1e-5 texels either way
    x = np.arange(res * res)
    got_i = sum(w.astype(np.float64) * (r % res) for r, w in zip(rows, wts))
    got_j = sum(w.astype(np.float64) * (r // res) for r, w in zip(rows, wts))
    heavy = np.argmax(np.stack(wts), axis=0)
    assert (np.stack(rows)[heavy, x] == x).all()
    assert np.stack(wts).max(axis=0).min() >= 1 - 2e-5
    interior = ((x % res) > 0) & ((x % res) < res - 1) & ((x // res) > 0) & ((x // res) < res - 1)  # (at the rim a neighbour is a folded texel elsewhere)
    assert np.abs(got_i - x % res)[interior].max() <= 1e-5 and np.abs(got_j - x // res)[interior].max() <= 1e-5


def _smooth(T):
    T = T.astype(np.float64)
    return (0.3 + 0.5 * T[:, 0] - 0.2 * T[:, 1] * T[:, 2] + 0.4 * T[:, 2] + 0.3 * T[:, 0] * T[:, 1]).astype(F)


def _across_the_rim(delta):
    """Pairs of unit directions `2 delta` apart on either side of what the map's four edges and four corners are on the sphere: the half planes
    y = 0 and x = 0 of the lower hemisphere, and the pole (0, 0, -1)."""
    a, b = [], []
    for s in np.linspace(0.05, 0.95, 19):  # along each edge
        z = -np.sqrt(1 - s * s)
        for sign in (1.0, -1.0):
            a += [(sign * s, delta, z), (delta, sign * s, z)]
            b += [(sign * s, -delta, z), (-delta, sign * s, z)]
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):  # around the pole: the four corners
        a += [(sx * delta, sy * delta, -1.0), (sx * delta, sy * delta, -1.0)]
        b += [(-sx * delta, sy * delta, -1.0), (-sx * delta, -sy * delta, -1.0)]
    a, b = np.asarray(a), np.asarray(b)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F), (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(F)


@pytest.mark.parametrize("res", [4, 8, 16])
def test_the_fold_rule_interpolates_continuously_across_every_edge_and_corner(res, monkeypatch):
    values = _smooth(dr.texel_directions(res))
    depth_map = np.stack([values, values * values], axis=1)
    a, b = _across_the_rim(1e-6)
    # the pairs do sit on either side of a map edge: their heaviest texels are different rows, far apart in the map
    ra, _ = dr.lookup([a[:, 0], a[:, 1], a[:, 2]], res)
    rb, _ = dr.lookup([b[:, 0], b[:, 1], b[:, 2]], res)
    assert (ra[0] != rb[0]).any()
    ma, _ = dr.interpolate(depth_map, a, res)
    mb, _ = dr.interpolate(depth_map, b, res)
    assert np.abs(ma - mb).max() <= 1e-4, np.abs(ma - mb).max()
    # the same comparison has teeth: with neighbours clamped at the rim instead of folded, the map jumps there
    monkeypatch.setattr(dr, "fold", lambda i, j, r: np.clip(j, 0, r - 1) * r + np.clip(i, 0, r - 1))
    ca, _ = dr.interpolate(depth_map, a, res)
    cb, _ = dr.interpolate(depth_map, b, res)
    assert np.abs(ca - cb).max() > 0.1


def test_the_fold_rule_is_the_octahedron_s_edge_rule_in_integers():
    res = 8
    i = np.array([-1, -1, 3, 8, 8, -1, 8, 2])
    j = np.array([2, -1, -1, 5, 8, 8, -1, 8])
    # beyond one edge the other index is mirrored; beyond a corner both
    want = [(0, 5), (7, 7), (4, 0), (7, 2), (0, 0), (7, 0), (0, 7), (5, 7)]
    assert dr.fold(i, j, res).tolist() == [cj * res + ci for ci, cj in want]
    inside = np.arange(res)
    assert (dr.fold(inside[:, None], inside[None, :], res) == inside[None, :] * res + inside[:, None]).all()


def _wall_probe(res, sharpness, n, seed):
    """A probe at the origin, a wall at x = +1, everything else open to a radius of 10: n uniform directions, their hits, the probe's map and its
    isotropic moments from the same samples."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    with np.errstate(all="ignore"):
        t = (F(1) / d[:, 0]).astype(F)
    hit = (d[:, 0] > 0) & (t < 10)
    sums = dr.accumulate(res, sharpness, d[:, None, :], t[:, None], hit[:, None], np.ones((n, 1), dtype=bool))  # (n samples of one point)
    depth_map = dr.build_depth(sums, 10.0)[0]
    t_sum, t2_sum, opened = F(0), F(0), 0
    for k in range(n):
        if hit[k]:
            t_sum, t2_sum = F(t_sum + t[k]), F(t2_sum + F(t[k] * t[k]))
        else:
            opened += 1
    mean = F(F(t_sum + F(F(opened) * F(10))) / F(n))
    mean2 = F(F(t2_sum + F(F(F(opened) * F(10)) * F(10))) / F(n))
    return depth_map, mean, mean2


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("sharpness", [3, 5])
@pytest.mark.parametrize("res", [4, 8, 16])
def test_the_wall_case_the_map_sees_the_wall_on_its_side_only(res, sharpness, n, seed):
    depth_map, mean, mean2 = _wall_probe(res, sharpness, n, seed)
    q = np.array([[3, 0.3, -0.2], [-3, 0.3, -0.2]], dtype=F)  # behind the wall, and its mirror image in the open
    dist = np.sqrt((q * q).sum(axis=1)).astype(F)
    m, m2 = dr.interpolate(depth_map, q, res)
    factor = dr.chebyshev_factor(m, m2, dist)
    print(f"res {res} sharpness_log2 {sharpness} n {n} seed {seed}: factor behind the wall {factor[0]:.3e}, in the open {factor[1]!r}")
    assert factor[0] <= 1e-3 and factor[1] == 1.0
    iso = dr.chebyshev_factor(np.full(2, mean), np.full(2, mean2), dist)
    assert (iso == 1.0).all()  # the isotropic moments of the same samples cannot tell the two apart


def _grid_case(rng, counts=(3, 4, 2), res=8, flags=(True, True)):
    grid = VolumeGrid((-1.0, 0.5, 2.0), (0.75, 0.5, 1.25), counts, backface=flags[0], chebyshev=flags[1], normal_bias=0.1)
    n = grid.n_probes
    probes = np.zeros((n, 32), dtype=F)
    probes[:, :27] = rng.normal(size=(n, 27)).astype(F) * F(0.3)
    probes[:, 0:3] += F(2.0)
    probes[:, 27], probes[:, 28] = F(0.4), F(0.2)
    probes.view(U)[:, 29] = np.where(rng.random(n) < 0.85, vr.VALID | vr.MOMENTS, 0)
    probes.view(U)[:, 30] = 64
    lo = np.asarray(grid.origin)
    size = np.asarray(grid.spacing) * (np.asarray(grid.counts) - 1)
    pos = lo + rng.uniform(-0.3, 1.3, (500, 3)) * size
    points = vr.point_rows(pos.astype(F), vr.unit_normals(rng, 500))
    return grid, probes, points


def test_with_chebyshev_off_the_restated_sampler_is_volume_sample_word_for_word():
    rng = np.random.default_rng(11)
    for backface in (False, True):
        grid, probes, points = _grid_case(rng, flags=(backface, False))
        depth = rng.uniform(0.01, 1.0, (grid.n_probes, 64, 2)).astype(F)  # whatever the maps hold
        got = dr.volume_sample_depth(grid, probes, depth, 8, points)
        want = vr.volume_sample(grid, probes, points)
        assert (got.view(U) == want.view(U)).all()
        assert (got.view(U)[:, 3] > 0).sum() > 400


def test_a_probe_whose_texels_are_all_radius_attenuates_nothing_inside_the_radius():
    rng = np.random.default_rng(12)
    grid, probes, points = _grid_case(rng)
    radius = F(8.0)  # beyond the cell's diagonal: every corner's probe is within the radius of the point
    empty = dr.build_depth(np.zeros((grid.n_probes, 64, 4), dtype=F), radius)
    assert (empty[..., 0] == radius).all() and (empty[..., 1] == radius * radius).all()
    got = dr.volume_sample_depth(grid, probes, empty, 8, points)
    unattenuated = VolumeGrid(grid.origin, grid.spacing, grid.counts, backface=True, chebyshev=False, normal_bias=grid.normal_bias)
    want = vr.volume_sample(unattenuated, probes, points)
    assert (got.view(U) == want.view(U)).all()
    # ... while a map that says "a wall at 0.05" does attenuate: the flag is not simply ignored
    near = np.zeros((grid.n_probes, 64, 2), dtype=F)
    near[..., 0], near[..., 1] = F(0.05), F(0.0026)
    assert (dr.volume_sample_depth(grid, probes, near, 8, points).view(U) != want.view(U)).any()


def test_build_depth_restated_handles_texels_without_information():
    sums = np.array([[[2.0, 0.5, 3.0, 5.0], [0.0, 0.0, 0.0, 0.0], [NAN, 0.0, 1.0, 1.0], [1.0, 0.0, INF, 1.0], [-1.0, 0.0, 1.0, 1.0]]], dtype=F)
    out = dr.build_depth(sums, 4.0)[0]
    assert out[0, 0] == F((F(3.0) + F(0.5) * F(4.0)) / F(2.0)) and out[0, 1] == F((F(5.0) + F(F(0.5) * F(4.0)) * F(4.0)) / F(2.0))
    assert (out[1:] == np.array([4.0, 16.0], dtype=F)).all()
