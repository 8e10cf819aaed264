"""Lightmap unwrap (sol_lightmap_unwrap / sol_lightmap_unwrap_dev), the part that needs no GPU: the two entry points are exported,
declared without a scene and documented, the header is C99, the kernels are gfx950 code of the library, every refusal answers SOL_EINVAL in
the stated order and in front of the device check with nothing written - and the restatement the GPU tests compare against
(tests/lightmap_unwrap_ref.py) has the rule's own properties, all exact: the chart counts of known meshes, dense labels in mesh order, the
partition under a permutation, UVs inside the atlas, the labels back from tests/lightmap_charts_ref.py, the gutter under both rasterisers of
tests/lightmap_ref.py, the packing beside the sequential greedy loop, and a tap for every surface row of a conservative bake."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import lightmap_charts_ref as cr
import lightmap_ref as lr
import lightmap_sample_ref as sr
import lightmap_unwrap_ref as ur
import solstrale_amd
from solstrale_amd import CHART_NONE, _abi, device_count
from test_lightmap_mips_abi import _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_lightmap_unwrap_dev", "sol_lightmap_unwrap")
KERNELS = (b"sol_lightmap_unwrap_normals_kernel", b"sol_lightmap_unwrap_match_kernel", b"sol_lightmap_unwrap_extents_kernel",
           b"sol_lightmap_unwrap_rects_kernel", b"sol_lightmap_unwrap_next_kernel", b"sol_lightmap_unwrap_walk_kernel",
           b"sol_lightmap_unwrap_place_kernel", b"sol_lightmap_unwrap_write_kernel")
CFG = _abi.SolUnwrapConfig
F = np.float32
INF, NAN = float("inf"), float("nan")
NONE = ur.NONE


def test_the_entry_points_are_exported_declared_without_a_scene_and_documented():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(int device,", text), name
        assert re.search(r"\b" + name + r"\b", guide), name
    assert len(lib.sol_lightmap_unwrap.argtypes) == 7 and len(lib.sol_lightmap_unwrap_dev.argtypes) == 8
    assert C.sizeof(_abi.SolUnwrapConfig) == 32 and C.sizeof(_abi.SolUnwrapResult) == 32 == ur.RESULT_DTYPE.itemsize
    assert [f[0] for f in _abi.SolUnwrapResult._fields_] == list(ur.RESULT_DTYPE.names)
    assert re.search(r"#define SOL_UNWRAP_MAX_GUTTER 64u", text) and ur.MAX_GUTTER == _abi.SOL_UNWRAP_MAX_GUTTER == 64
    assert (ur.OVERFLOW_WIDTH, ur.OVERFLOW_HEIGHT) == (_abi.SOL_UNWRAP_OVERFLOW_WIDTH, _abi.SOL_UNWRAP_OVERFLOW_HEIGHT) == (1, 2)
    assert "SOL_LIGHTMAP_UNWRAP=collide" in text and "BOTH BLOCK" in text and "spiral ramp" in text and CHART_NONE == NONE
    for fn in ("lightmap_unwrap", "lightmap_unwrap_fit"):
        assert callable(getattr(solstrale_amd, fn))
    ms = (C.c_float * 8)(*([7.0] * 8))
    assert lib.sol_lightmap_unwrap_stage_ms(None) == _abi.SOL_EINVAL and lib.sol_lightmap_unwrap_stage_ms(ms) == _abi.SOL_OK
    assert list(ms) == [0.0] * 8  # no call of this thread was timed


def test_the_header_is_c99(tmp_path):
    src = tmp_path / "unwrap.c"
    src.write_text('#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                   '  int (*f[2])(void) = {(int (*)(void))sol_lightmap_unwrap_dev, (int (*)(void))sol_lightmap_unwrap};\n'
                   '  SolUnwrapConfig c = {sizeof(SolUnwrapConfig), 4, 4, 1, 1.0f, -1.0f, 0, 0};\n  SolUnwrapResult r;\n  float v[9] = {0};\n'
                   '  int rc = sol_lightmap_unwrap(0, &c, v, (size_t)0, NULL, NULL, &r);\n'
                   '  printf("%u %u %d %d %u", (unsigned)sizeof c, (unsigned)sizeof r, f[0] != 0, rc, (unsigned)(r.n_charts + r.content_texels));\n  return 0;\n}\n')
    exe = tmp_path / "unwrap"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L" + os.path.dirname(_abi.HIP_LIB), "-lsolstrale_hip", "-Wl,-rpath," + os.path.dirname(_abi.HIP_LIB)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert got == ["32", "32", "1", "0", "0"]


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data
    names = set(re.findall(rb"_Z\d+(sol_[a-z0-9_]+_kernel)[A-Za-z0-9_]*\.kd", data))
    for k in KERNELS:
        assert k in names, k


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), width=64, height=64, gutter=2, texels_per_unit=4.0, crease_cos=-1.0, flags=0, reserved=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_every_refusal_comes_in_the_stated_order_before_the_device_and_writes_nothing():
    lib = _abi.load_hip()
    vertices, uvs, chart_of, result = (C.c_float * 18)(), (C.c_float * 12)(), (C.c_uint32 * 2)(), (C.c_uint32 * 8)(*([7] * 8))
    good = dict(c={}, vertices=vertices, n=2, uvs=uvs, chart_of=chart_of, result=result)
    steps = [(dict(cfg_null=True), b"null configuration"), (dict(c=dict(size=36)), b"size"), (dict(c=dict(reserved=1)), b"reserved"),
             (dict(c=dict(flags=1)), b"unknown bits"), (dict(c=dict(width=0)), b"atlas"), (dict(c=dict(height=16385)), b"atlas"),
             (dict(c=dict(gutter=65)), b"gutter"), (dict(c=dict(texels_per_unit=0.0)), b"texels_per_unit"),
             (dict(c=dict(texels_per_unit=INF)), b"texels_per_unit"), (dict(c=dict(texels_per_unit=NAN)), b"texels_per_unit"),
             (dict(c=dict(crease_cos=1.5)), b"crease_cos"), (dict(c=dict(crease_cos=NAN)), b"crease_cos"), (dict(n=(1 << 30) + 1), b"at most 2^30"),
             (dict(vertices=None), b"null vertex"), (dict(uvs=None), b"null UV output"), (dict(chart_of=None), b"null label output"),
             (dict(result=None), b"null result")]

    def call(name, a):
        cfg = None if a.get("cfg_null") else C.byref(_cfg(**a["c"]))
        stream = (None,) if name.endswith("_dev") else ()
        return getattr(lib, name)(0, *stream, cfg, a["vertices"], a["n"], a["uvs"], a["chart_of"], a["result"])

    _walk(steps, good, call, ENTRY_POINTS)
    assert bytes(uvs) == bytes(48) and bytes(chart_of) == bytes(8) and list(result) == [7] * 8  # nothing was written
    # no triangle: the host form needs no device and writes a zero result
    assert call("sol_lightmap_unwrap", {**good, "n": 0, "vertices": None, "uvs": None, "chart_of": None}) == _abi.SOL_OK and list(result) == [0] * 8
    if device_count() == 0:
        for name in ENTRY_POINTS:
            assert call(name, good) == _abi.SOL_EDEVICE
        assert call("sol_lightmap_unwrap_dev", {**good, "n": 0}) == _abi.SOL_EDEVICE  # (its result is device memory)


# ---- the charts of the restatement ----------------------------------------------------------------------------------------------------------
def _unwrap(v, W=256, H=256, tpu=8.0, **kw):
    return ur.lightmap_unwrap(v, W, H, tpu, **kw)


def _partition(labels):
    """the partition a label array stands for, as a set of frozensets of triangle indices (NONE: left out)"""
    return {frozenset(np.nonzero(labels == c)[0].tolist()) for c in np.unique(labels) if c != NONE}


def test_known_meshes_have_their_chart_counts():
    uvs, ch, res = _unwrap(ur.cube())
    assert res["n_charts"] == 6 and res["live_triangles"] == 12 and res["overflow"] == 0
    assert ch.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert _unwrap(ur.grid(8))[2]["n_charts"] == 1
    two_floors = np.concatenate([ur.grid(4), ur.grid(4) + F([0, 3, 0])])
    uvs, ch, res = _unwrap(two_floors)
    assert res["n_charts"] == 2 and (ch[:32] == 0).all() and (ch[32:] == 1).all()
    uvs, ch, res = _unwrap(ur.fin())
    assert ch.tolist() == [0, 0, 1] and res["n_charts"] == 2
    for order in ([2, 0, 1], [0, 2, 1], [1, 2, 0]):  # wherever the standing triangle sorts, the two flat ones are joined
        assert len(_partition(_unwrap(ur.fin()[order])[1])) == 2
    bumped = ur.grid(8, bump=0.5)
    assert _unwrap(bumped)[2]["n_charts"] == 1  # a height field keeps its class: one chart with the class rule alone
    assert _unwrap(bumped, crease_cos=0.95)[2]["n_charts"] > 1


def test_dead_triangles_join_nothing_and_leave_the_other_labels_alone():
    clean = ur.grid(6)
    v, at = ur.with_dead(clean)
    uvs, ch, res = _unwrap(v)
    assert (ch[at] == NONE).all() and res["live_triangles"] == len(v) - 3
    assert not uvs[at].any() and uvs[at].tobytes() == bytes(3 * 24)  # six +0 words
    live = np.setdiff1d(np.arange(len(v)), at)
    assert (ch[live] != NONE).all()
    # dead triangles are holes: what they connected falls apart, nothing else changes
    keep = np.ones(len(v), dtype=bool)
    keep[at] = False
    assert _partition(ch) == {frozenset(np.nonzero(keep)[0][sorted(p)].tolist()) for p in _partition(_unwrap(clean[keep])[1])}


def test_labels_are_dense_and_in_mesh_order_and_a_permutation_permutes_the_partition():
    v = np.concatenate([ur.cube(), ur.grid(5) + F([3, 0, 0]), ur.fin() + F([0, 0, 4]), ur.disjoint(20) + F([10, 0, 10])])
    uvs, ch, res, d = ur.lightmap_unwrap(v, 512, 512, 6.0, detail=True)
    m = int(res["n_charts"])
    assert res["overflow"] == 0 and sorted(np.unique(ch).tolist()) == list(range(m))
    first = [int(np.nonzero(ch == c)[0][0]) for c in range(m)]
    assert first == sorted(first)  # a chart's id is the rank of its lowest triangle
    perm = np.random.default_rng(5).permutation(len(v))
    uvs2, ch2, res2, d2 = ur.lightmap_unwrap(v[perm], 512, 512, 6.0, detail=True)
    assert _partition(ch2) == {frozenset(int(np.nonzero(perm == t)[0][0]) for t in p) for p in _partition(ch)}
    assert sorted(zip(d["cw"].tolist(), d["ch"].tolist())) == sorted(zip(d2["cw"].tolist(), d2["ch"].tolist()))  # the multiset of rectangles
    assert res2["content_texels"] == res["content_texels"] and res2["used_height"] == res["used_height"]


def test_uvs_lie_in_the_atlas_and_the_charts_come_back_from_the_chart_labelling():
    for v, W, H, tpu, kw in ((ur.cube(), 64, 64, 8.0, {}), (ur.grid(8, bump=0.5), 128, 96, 9.5, dict(crease_cos=0.95)), (ur.disjoint(300), 64, 700, 7.0, dict(gutter=0)),
                             (ur.with_dead(ur.grid(6))[0][:-1], 100, 60, 11.0, dict(gutter=1))):
        uvs, ch, res = ur.lightmap_unwrap(v, W, H, tpu, **kw)
        assert res["overflow"] == 0 and (uvs >= 0).all() and (uvs <= 1).all()
        # sol_lightmap_charts over (uvs, vertices) finds the same islands. (Its liveness is finiteness alone: a zero-area triangle, dead here, is
        # an island of its own there, so the comparison is over the triangles that are live here.)
        back, _ = cr.lightmap_charts(uvs, v)
        live = ch != NONE
        assert _partition(np.where(live, back, NONE)) == _partition(ch)
        ranks = {int(b): k for k, b in enumerate(sorted(set(back[live].tolist())))}
        assert [ranks[int(b)] for b in back[live]] == ch[live].tolist()
    uvs, ch, res = _unwrap(ur.cube())
    assert cr.lightmap_charts(uvs, ur.cube())[0].tolist() == ch.tolist()


def _owner_charts(v, uvs, ch, W, H, conservative):
    owner, _ = lr.lightmap_owner(v, uvs, W, H, conservative=conservative)
    tri = owner & np.uint32(0x7FFFFFFF)
    return np.where(owner == NONE, NONE, ch[np.minimum(tri, len(ch) - 1)]).reshape(H, W).astype(np.int64), owner


def test_the_gutter_separates_the_claims_of_different_charts_under_both_rasterisers():
    """At least `gutter` unclaimed texels between texels claimed by different charts: no texel within Chebyshev distance `gutter` of a claimed
    texel is claimed by another chart. Whole-texel corners (the cube at density 8: every corner on a texel line) are the case the guard
    texels of the content rectangle exist for."""
    cases = ((ur.cube(), 64, 64, 8.0, 0), (ur.cube(), 64, 64, 8.0, 1), (ur.cube(), 96, 64, 8.0, 3), (ur.grid(6, bump=0.6), 128, 128, 10.0, 2),
             (ur.disjoint(60), 64, 128, 8.0, 1), (ur.disjoint(60), 61, 128, 6.5, 0))
    for v, W, H, tpu, g in cases:
        kw = dict(crease_cos=0.9) if len(v) == 72 else {}
        uvs, ch, res = ur.lightmap_unwrap(v, W, H, tpu, gutter=g, **kw)
        assert res["overflow"] == 0
        for conservative in (False, True):
            plane, owner = _owner_charts(v, uvs, ch, W, H, conservative)
            assert (owner != NONE).any()
            pad = np.full((H + 2 * (g + 1), W + 2 * (g + 1)), NONE, dtype=np.int64)
            pad[g + 1:g + 1 + H, g + 1:g + 1 + W] = plane
            for dj in range(-(g + 1), g + 2):
                for di in range(-(g + 1), g + 2):
                    other = pad[g + 1 + dj:g + 1 + dj + H, g + 1 + di:g + 1 + di + W]
                    clash = (plane != NONE) & (other != NONE) & (other != plane)
                    assert not clash.any(), (len(v), W, H, g, conservative, di, dj)


def test_an_edge_in_the_atlas_is_the_projected_edge_at_the_density():
    """(uv1 - uv0) * width against (projected corner 1 - projected corner 0): both sides go through a translation, a division by the atlas extent
    and a product with it, each rounded once at a magnitude below the atlas extent - three roundings of at most 2^-24 x extent each."""
    for v, W, H, tpu in ((ur.cube(), 64, 64, 7.3), (ur.grid(6, bump=0.4), 128, 96, 11.7)):
        uvs, ch, res, d = ur.lightmap_unwrap(v, W, H, tpu, detail=True)
        assert res["overflow"] == 0
        xy = d["xy"].astype(np.float64)
        for k, n in ((0, W), (1, H)):
            got = (uvs[:, 1, k].astype(np.float64) - uvs[:, 0, k]) * n
            want = xy[:, 1, k] - xy[:, 0, k]
            assert np.abs(got - want).max() <= 3 * n * 2.0 ** -24
        # and inside a chart equal positions have equal words
        flat_p, flat_uv, flat_c = v.reshape(-1, 3), uvs.reshape(-1, 2), np.repeat(ch, 3)
        seen = {}
        for p, uv, c in zip(flat_p, flat_uv, flat_c):
            key = (int(c), p.tobytes())
            assert seen.setdefault(key, uv.tobytes()) == uv.tobytes()


# ---- the packing ----------------------------------------------------------------------------------------------------------------------------
def _greedy(w, h, W, H):
    """the shelf rule as one reads it: a plain loop over the sorted rectangles"""
    order = sorted(range(len(w)), key=lambda i: (-h[i], -w[i], i))
    x = y = shelf_h = used_w = 0
    pos, opened = {}, False
    for i in order:
        if not opened or x + w[i] > W:
            if opened:
                y += shelf_h
                if y > ur.MAX_SIZE:
                    break
            x, shelf_h, opened = 0, h[i], True
        pos[i] = (x, y)
        x += w[i]
        used_w = max(used_w, x)
    used_h = y + shelf_h if opened and y <= ur.MAX_SIZE else y
    return pos, used_w, used_h, (1 if any(wi > W for wi in w) else 0) | (2 if used_h > H else 0)


def _same_packing(w, h, W, H):
    x, y, reached, used_w, used_h, overflow = ur.pack(w, h, W, H)
    pos, want_w, want_h, want_overflow = _greedy(list(w), list(h), W, H)
    assert (used_w, used_h, overflow) == (want_w, want_h, want_overflow), (used_w, used_h, overflow, want_w, want_h, want_overflow)
    assert sorted(np.nonzero(reached)[0].tolist()) == sorted(pos)
    for i, (px, py) in pos.items():
        assert (int(x[i]), int(y[i])) == (px, py), i
    return x, y, used_w, used_h, overflow


def test_the_packing_is_the_sequential_greedy_loop():
    rng = np.random.default_rng(11)
    for _ in range(60):
        m = int(rng.integers(1, 200))
        W = int(rng.integers(8, 300))
        hi = int(rng.choice([4, 12, 60]))
        w, h = rng.integers(3, hi + 1, m), rng.integers(3, hi + 1, m)
        _same_packing(w, h, W, int(rng.integers(1, 4000)))
    _same_packing(rng.integers(3, 9, 5000), rng.integers(3000, 6000, 5000), 16, 16384)  # the walk stops beyond 16384


def test_packing_edge_cases():
    x, y, *_ = _same_packing([5, 5, 5, 5], [4, 4, 4, 4], 10, 100)  # equal rectangles go by id
    assert (x.tolist(), y.tolist()) == ([0, 5, 0, 5], [0, 0, 4, 4])
    x, y, uw, uh, ov = _same_packing([10, 3], [4, 4], 10, 100)  # a rectangle that fills the width fits, and leaves no room
    assert (x.tolist(), y.tolist(), uw, uh, ov) == ([0, 0], [0, 4], 10, 8, 0)
    x, y, uw, uh, ov = _same_packing([7, 3], [4, 4], 10, 100)
    assert (x.tolist(), y.tolist(), uw) == ([0, 7], [0, 0], 10)  # exactly the width: fits
    x, y, uw, uh, ov = _same_packing([7, 4], [4, 4], 10, 100)
    assert (x.tolist(), y.tolist()) == ([0, 0], [0, 4])  # one texel more: the next shelf
    *_, uw, uh, ov = _same_packing([11, 3], [4, 4], 10, 100)
    assert ov == 1 and uw == 11  # wider than the atlas
    *_, uw, uh, ov = _same_packing([6, 6], [4, 4], 10, 7)
    assert ov == 2 and uh == 8  # one shelf too many for the height
    *_, uw, uh, ov = _same_packing([6, 6], [4, 4], 10, 8)
    assert ov == 0


def test_both_overflow_bits_leave_zero_uvs_and_no_labels_but_keep_the_sizes():
    v = ur.cube()
    uvs, ch, res = ur.lightmap_unwrap(v, 8, 64, 8.0)  # a face spans the texel lines 0 .. 8: 9 texels + 2 guards + 2 gutter
    assert res["overflow"] & 1 and not uvs.any() and (ch == NONE).all()
    assert res["n_charts"] == 6 and res["live_triangles"] == 12 and res["used_width"] == 13 and res["content_texels"] == 6 * 121
    uvs, ch, res = ur.lightmap_unwrap(v, 26, 38, 8.0)  # two faces a shelf, three shelves of 13
    assert res["overflow"] == 2 and res["used_height"] == 39 and res["used_width"] == 26 and not uvs.any() and (ch == NONE).all()
    assert ur.lightmap_unwrap(v, 26, 39, 8.0)[2]["overflow"] == 0
    huge = ur.lightmap_unwrap(v, 64, 64, 1e30)[2]  # extents no atlas holds are reported as 32767
    assert huge["overflow"] & 1 and huge["used_width"] == 32767 + 2


# ---- end to end on the restatements ---------------------------------------------------------------------------------------------------------
def test_every_surface_row_of_a_conservative_bake_finds_a_tap():
    v = np.concatenate([ur.cube(), ur.grid(5, bump=0.3) + F([2, 0, 0]), ur.disjoint(12) * F(0.5) + F([0, 2, 0])])
    W, H = 96, 80
    uvs, ch, res = ur.lightmap_unwrap(v, W, H, 5.3, gutter=2)
    assert res["overflow"] == 0
    points, texels = lr.lightmap_points(v, uvs, W, H, conservative=True)
    values = np.ones((W * H, 4), dtype=F)
    out, pass_of, plane = cr.lightmap_dilate_charts(values, texels, ch, W, H, passes=0)
    rng = np.random.default_rng(13)
    rows = np.zeros(3000, dtype=sr.TEXEL_DTYPE)
    b = rng.dirichlet((1.0, 1.0, 1.0), len(rows)).astype(F)
    b[:300] = np.eye(3, dtype=F)[rng.integers(0, 3, 300)]  # corners too
    rows["triangle"], rows["b1"], rows["b2"], rows["flags"] = rng.integers(0, len(v), len(rows)), b[:, 1], b[:, 2], 1
    for nearest in (False, True):
        got = cr.lightmap_sample_charts(out, rows, uvs, texels, ch, plane, W, H, pass_of=pass_of, nearest=nearest)
        taps = got[:, 3].view(np.uint32)
        assert (taps >= 1).all(), (nearest, int((taps == 0).sum()))
