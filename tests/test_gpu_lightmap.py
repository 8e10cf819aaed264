"""Lightmap texel points and border dilation on the device (sol_lightmap_points / sol_lightmap_dilate). The yardstick is
tests/lightmap_ref.py, the rule restated in numpy float32: points, texels, dilated rows and pass_of are compared word for word, with and without
conservative claims, with and without normals, on the host route and the device route. Around it: guard rows, skipped triangles, both balance
extremes of the claim pass, determinism under a permutation, a stream of the caller's, the whole bake end to end, and neutrality. Atlases are at
most 256 x 256, meshes at most 4097 triangles."""
import ctypes as C
import zlib

import numpy as np
import pytest

import lightmap_ref as lr
import parity_util as pu
from solstrale_amd import CameraConfig, DeviceScene, RenderConfig, SceneBuilder, _abi, lightmap_texels_to_numpy, scenes
from test_gpu_irradiance import _path_stats

pytestmark = pytest.mark.gpu
SEED = pu.SEED
F = np.float32
INF, NAN = F(np.inf), F(np.nan)
RC = RenderConfig(32, 32, 1)
GRID_SEED = 1


@pytest.fixture(scope="module")
def ds():
    with DeviceScene(scenes.cornell_box(RC)) as d:  # (the geometry of a lightmap call is the caller's: any handle serves)
        yield d


def assert_words_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape[0] == want.shape[0], (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(got.shape[0], -1), want.view(np.uint32).reshape(want.shape[0], -1)
    if g.shape != w.shape or (g != w).any():
        bad = np.nonzero((g != w).any(axis=1))[0]
        raise AssertionError((what, len(bad), len(g), bad[:5], got[bad[:3]], want[bad[:3]]))


def check_all_ways(ds, V, T, W, H, N=None, what="", **kw):
    """Both routes x conservative or not x normals or not against the restatement; returns the restatement's answers keyed by (conservative, normals)."""
    import torch
    V, T = np.ascontiguousarray(V, dtype=F), np.ascontiguousarray(T, dtype=F)
    dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    dN = None if N is None else torch.from_numpy(np.ascontiguousarray(N, dtype=F)).cuda()
    want = {}
    for cons in (False, True):
        for normals in ((None,) if N is None else (None, N)):
            ref_p, ref_t = lr.lightmap_points(V, T, W, H, normals=normals, conservative=cons, **kw)
            tag = (what, "conservative" if cons else "centre", "normals" if normals is not None else "geometric")
            p, t = ds.lightmap_points(V, T, W, H, normals=normals, conservative=cons, **kw)
            assert p.shape == (W * H, 8) and t.shape == (W * H,)
            assert_words_equal(p, ref_p, tag + ("host", "points"))
            assert_words_equal(t, ref_t, tag + ("host", "texels"))
            p, t = ds.lightmap_points(dV, dT, W, H, normals=None if normals is None else dN, conservative=cons, **kw)
            assert_words_equal(p.cpu().numpy(), ref_p, tag + ("device", "points"))
            assert_words_equal(lightmap_texels_to_numpy(t), ref_t, tag + ("device", "texels"))
            want[(cons, normals is not None)] = (ref_p, ref_t)
    return want


def tri(*uv):
    return np.asarray([uv], dtype=F).reshape(-1, 3, 2)


# ---- 1. the rule, case by case ----------------------------------------------------------------------------------------------------------------
def test_one_triangle_over_half_of_an_odd_sized_atlas(ds):
    T = tri((0, 0), (1, 0), (0, 1))
    N = np.asarray([[(0.1, 1, 0), (0, 1, 0.2), (-0.3, 2, 0)]], dtype=F)
    want = check_all_ways(ds, lr.lift(T), T, 63, 65, N, "half", tmin=0.25, tmax=7.5)
    p, t = want[(False, False)]
    owned = t["triangle"] == 0
    assert 0.45 * 63 * 65 < owned.sum() < 0.55 * 63 * 65 and (t["triangle"][~owned] == lr.NONE).all()
    assert (p[owned, 3] == F(0.25)).all() and (p[owned, 7] == F(7.5)).all() and (p[~owned] == 0).all()
    assert (t["flags"][owned] == 1).all() and (t["flags"][~owned] == 0).all()
    assert (want[(True, False)][1]["flags"] == 2).sum() > 30  # the conservative rim along the diagonal


def test_two_triangles_sharing_the_diagonal_lose_no_centre_and_own_none_twice(ds):
    W = H = 64
    T = np.concatenate([tri((0, 0), (1, 0), (1, 1)), tri((0, 0), (1, 1), (0, 1))])
    t = check_all_ways(ds, lr.lift(T), T, W, H, None, "diagonal")[(False, False)][1]
    owner = t["triangle"].reshape(H, W)
    assert (owner != lr.NONE).all()                        # none lost
    assert (np.diag(owner) == 0).all()                     # every centre on the diagonal belongs to both: the lower index owns it
    assert (owner[np.triu_indices(W, 1)] == 0).all() and (owner[np.tril_indices(W, -1)] == 1).all()  # (row j, column i: i > j is triangle 0's side)
    # the same pair with the second triangle mirrored in UV order (negative area2)
    T2 = np.concatenate([tri((0, 0), (1, 0), (1, 1)), tri((0, 0), (0, 1), (1, 1))])
    t2 = check_all_ways(ds, lr.lift(T2), T2, W, H, None, "diagonal mirrored")[(False, False)][1]
    assert (t2["triangle"] == t["triangle"]).all()


def test_of_two_overlapping_charts_the_lowest_index_wins(ds):
    T = np.concatenate([tri((0.1, 0.1), (0.9, 0.15), (0.4, 0.8)), tri((0.3, 0.05), (0.95, 0.6), (0.2, 0.9))])
    V = lr.lift(T)
    V[1, :, 1] = 1.0  # the second chart lies higher: its rows differ from the first's
    t = check_all_ways(ds, V, T, 48, 40, None, "overlap")[(True, False)][1]
    a, _ = lr.lightmap_owner(V[:1], T[:1], 48, 40)
    b, _ = lr.lightmap_owner(V[1:], T[1:], 48, 40)
    both = (a != lr.NONE) & (b != lr.NONE)
    assert both.sum() > 200 and (t["triangle"][both] == 0).all() and (t["triangle"][(a == lr.NONE) & (b != lr.NONE)] == 1).all()


def test_the_smallest_atlas_and_an_empty_call(ds):
    T = tri((0, 0), (1, 0), (0, 1))
    t = check_all_ways(ds, lr.lift(T), T, 1, 1, None, "1x1")[(False, False)][1]
    assert t["triangle"][0] == 0  # the centre (0.5, 0.5) lies on the hypotenuse
    want = check_all_ways(ds, np.zeros((0, 3, 3), F), np.zeros((0, 3, 2), F), 5, 3, None, "no triangles")
    assert (want[(False, False)][1]["triangle"] == lr.NONE).all() and (want[(False, False)][0] == 0).all()


def test_triangles_partly_and_wholly_outside_are_clipped_and_nothing_is_written_out_of_bounds(ds):
    import torch
    W, H, G = 37, 29, 64
    T = np.concatenate([tri((-0.4, 0.3), (0.6, -0.5), (1.7, 1.4)), tri((1.2, 1.1), (2.0, 1.3), (1.5, 2.5)), tri((-3, -3), (-2, -3), (-3, 7)),
                        tri((0.2, -1e30), (0.4, 1e30), (0.3, 0.5)), tri((0.5, 0.5), (3e38, 0.6), (0.5, 0.9))])
    V = lr.lift(np.clip(T, -8, 8))
    want = check_all_ways(ds, V, T, W, H, None, "clipped")
    assert 0 < (want[(False, False)][1]["triangle"] == 0).sum() < W * H
    assert not (want[(True, False)][1]["triangle"] == 1).any() and not (want[(True, False)][1]["triangle"] == 2).any()
    # guard rows around both outputs of the device route
    dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
    for cons in (0, 1):
        points = torch.full(((W * H + 2 * G), 8), 7.0, dtype=torch.float32, device="cuda")
        texels = torch.full(((W * H + 2 * G), 4), 7, dtype=torch.int32, device="cuda")
        cfg = _abi.SolLightmapConfig(size=32, width=W, height=H, flags=cons, tmin=1e-3, tmax=float("inf"))
        torch.cuda.synchronize()
        ds._chk(ds.lib.sol_lightmap_points_dev(ds.h, C.c_void_p(dV.data_ptr()), None, C.c_void_p(dT.data_ptr()), len(T), C.byref(cfg),
                                                C.c_void_p(points[G:].data_ptr()), C.c_void_p(texels[G:].data_ptr())))
        ds.sync()
        assert (points[:G] == 7).all() and (points[G + W * H:] == 7).all() and (texels[:G] == 7).all() and (texels[G + W * H:] == 7).all()
        assert_words_equal(points[G:G + W * H].cpu().numpy(), want[(bool(cons), False)][0], "guarded points")


def test_degenerate_and_non_finite_triangles_are_skipped(ds):
    """The bad triangles come first: were one of them not skipped, its lower index would win the texels of the good one behind them."""
    good_uv = tri((0.05, 0.05), (0.95, 0.1), (0.5, 0.95))[0]
    uv_cases, pos_cases, nrm_cases = [], [], []
    base_pos, base_nrm = lr.lift(good_uv[None])[0], np.asarray([(0, 1, 0)] * 3, dtype=F)

    def add(uv=None, pos=None, nrm=None):
        uv_cases.append(good_uv.copy() if uv is None else uv)
        pos_cases.append(base_pos.copy() if pos is None else pos)
        nrm_cases.append(base_nrm.copy() if nrm is None else nrm)

    add(uv=np.asarray([(0.2, 0.2), (0.5, 0.5), (0.8, 0.8)], dtype=F))  # zero-area UVs: collinear
    add(uv=np.asarray([(0.3, 0.3)] * 3, dtype=F))                     # zero-area UVs: one point
    add(pos=np.asarray([(0, 0, 0), (1, 1, 1), (2, 2, 2)], dtype=F))   # zero-area positions
    add(pos=np.asarray([(1e-30, 0, 0), (0, 1e-30, 0), (0, 0, 0)], dtype=F))  # a geometric normal whose squared length underflows
    for bad in (NAN, INF, -INF):
        for which in range(3):
            a = [good_uv.copy(), base_pos.copy(), base_nrm.copy()]
            a[which][1, 1] = bad
            add(*a)
    add()  # the good one, last
    T, V, N = np.asarray(uv_cases, dtype=F), np.asarray(pos_cases, dtype=F), np.asarray(nrm_cases, dtype=F)
    n = len(T)
    want = check_all_ways(ds, V, T, 40, 33, N, "skipped")
    for cons in (False, True):
        t = want[(cons, True)][1]
        assert set(np.unique(t["triangle"])) == {n - 1, lr.NONE}
    # without normals the triangles whose only fault is a normal are good: the first of them owns the texels
    first_bad_normal = 4 + 2
    assert set(np.unique(want[(False, False)][1]["triangle"])) == {first_bad_normal, lr.NONE}


def small_triangles(n=4097, seed=5):
    """n random triangles, most smaller than a texel of a 256 x 256 atlas, some a few texels large; some reach over the border."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.02, 1.02, (n, 1, 2))
    T = (c + rng.uniform(-1, 1, (n, 3, 2)) * rng.choice([0.001, 0.002, 0.02], (n, 1, 1))).astype(F)
    V = lr.lift(T)
    V[..., 1] = rng.uniform(-1, 1, V.shape[:2]).astype(F)
    return V, T, rng.normal(size=V.shape).astype(F)


def test_many_triangles_smaller_than_a_texel(ds):
    W = H = 256
    V, T, N = small_triangles()
    assert len(V) == 4097
    want = check_all_ways(ds, V, T, W, H, None, "small triangles")
    centre, cons = want[(False, False)][1], want[(True, False)][1]
    owners_centre, owners_cons = set(np.unique(centre["triangle"])) - {lr.NONE}, set(np.unique(cons["triangle"])) - {lr.NONE}
    touching = int(((T[..., 0].max(1) >= 0) & (T[..., 0].min(1) <= 1) & (T[..., 1].max(1) >= 0) & (T[..., 1].min(1) <= 1)).sum())
    # Two thirds of the triangles span at most one texel and hold its centre with a probability below their area, a small fraction: centre mode
    # leaves most triangles without a texel. A conservative claim is lost only to a triangle that covers the same texel, and all of them together
    # cover well under half of the atlas: most triangles that touch the atlas own a texel then.
    assert len(owners_centre) < 0.5 * len(V) and (cons["flags"] != 0).mean() < 0.5
    assert len(owners_cons) > 0.6 * touching and owners_centre <= owners_cons
    assert (cons["flags"] == 2).sum() > (cons["flags"] == 1).sum() > 0
    had = centre["flags"] == 1                          # centre claims still beat conservative ones
    assert (cons["flags"][had] == 1).all() and (cons["triangle"][had] == centre["triangle"][had]).all()
    assert (cons["flags"][~had] != 1).all()


def test_one_triangle_over_a_whole_atlas(ds):
    T = tri((-0.5, -0.5), (2.5, -0.5), (-0.5, 2.5))
    want = check_all_ways(ds, lr.lift(T), T, 256, 256, None, "whole atlas")
    assert (want[(False, False)][1]["triangle"] == 0).all()
    # and a mesh in which every path of the claim pass has work: large, medium and small boxes overlapping
    V, T2, N = small_triangles(600, seed=9)
    rng = np.random.default_rng(4)
    mid = (rng.uniform(0, 1, (40, 1, 2)) + rng.uniform(-0.2, 0.2, (40, 3, 2))).astype(F)
    Tm = np.concatenate([T2[:300], mid, T, T2[300:]])
    Vm = lr.lift(Tm)
    Vm[..., 1] = rng.uniform(-1, 1, Vm.shape[:2]).astype(F)
    check_all_ways(ds, Vm, Tm, 256, 200, None, "mixed sizes")


def test_the_owners_follow_a_permutation_of_the_triangles(ds):
    W, H = 61, 64
    V, T, N = lr.grid_mesh(16, GRID_SEED)
    base = check_all_ways(ds, V, T, W, H, N, "grid")[(False, True)]
    assert (base[1]["triangle"] != lr.NONE).all()
    perm = np.random.default_rng(8).permutation(len(V))  # new index k holds old triangle perm[k]
    moved = check_all_ways(ds, V[perm], T[perm], W, H, N[perm], "grid permuted")[(False, True)]
    back = perm[moved[1]["triangle"]]
    # the same triangle owns the texel wherever only one contains its centre; a centre on a shared edge may change hands between the two
    same = back == base[1]["triangle"]
    assert same.mean() > 0.99
    assert_words_equal(moved[0][same], base[0][same], "rows under the permutation")
    for x in np.nonzero(~same)[0]:
        e = lr._setup(T[back[x]], V[back[x]], None, W, H).edges(F(x % W) + F(0.5), F(x // W) + F(0.5))
        assert min(e) == 0, "only a centre ON an edge can change hands"


def test_a_stream_of_the_callers(ds):
    import torch
    V, T, N = lr.grid_mesh(8, 3)
    W, H = 50, 41
    ref_p, ref_t = lr.lightmap_points(V, T, W, H, normals=N, conservative=True)
    stream = torch.cuda.Stream()
    ds.set_stream(stream.cuda_stream)
    try:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        p, t = ds.lightmap_points(dV, dT, W, H, normals=dN, conservative=True)
        assert_words_equal(p.cpu().numpy(), ref_p, "points on the caller's stream")
        assert_words_equal(lightmap_texels_to_numpy(t), ref_t, "texels on the caller's stream")
        values = torch.from_numpy(np.random.default_rng(1).normal(size=(W * H, 4)).astype(F)).cuda()
        out, pass_of = ds.lightmap_dilate(values, t, W, H, passes=3, return_pass_of=True)
        want, want_pass = lr.lightmap_dilate(values.cpu().numpy(), ref_t, W, H, passes=3, channels=3)
        assert_words_equal(out.cpu().numpy(), want, "dilation on the caller's stream")
        assert (pass_of.cpu().numpy() == want_pass).all()
        hp, ht = ds.lightmap_points(V, T, W, H, normals=N, conservative=True)
        assert_words_equal(hp, ref_p, "host route on the caller's stream")
    finally:
        ds.set_stream(0)


# ---- 2. dilation ----------------------------------------------------------------------------------------------------------------------------
def coverage_atlases():
    """(name, W, H, owned [H, W] bool): an island, a ring with a hole, islands that meet, a full and an empty atlas"""
    out = []
    W, H = 45, 38
    j, i = np.mgrid[0:H, 0:W]
    out.append(("island", W, H, (np.abs(i - 20) < 4) & (np.abs(j - 17) < 3)))
    r2 = (i - 22) ** 2 + (j - 19) ** 2
    out.append(("ring", W, H, (r2 < 15 ** 2) & (r2 > 9 ** 2)))
    out.append(("islands and border", W, H, ((i + 2 * j) % 23 == 0) | ((i == 0) & (j > 30)) | ((i == W - 1) & (j == H - 1))))
    out.append(("full", 16, 9, np.ones((9, 16), dtype=bool)))
    out.append(("empty", 16, 9, np.zeros((9, 16), dtype=bool)))
    out.append(("far corner", 300, 1, np.arange(300)[None, :] == 0))  # only 254 passes' worth of a 300-texel row gets filled
    return out


@pytest.mark.parametrize("channels, words", [(1, 1), (3, 4), (27, 28), (2, 5)], ids=["plane", "radiance_rows", "sh9_rows", "two_of_five"])
def test_dilation_equals_the_restatement_bit_for_bit(ds, channels, words):
    import torch
    rng = np.random.default_rng(channels)
    for name, W, H, owned in coverage_atlases():
        texels = np.zeros(W * H, dtype=lr.TEXEL_DTYPE)
        texels["triangle"] = np.where(owned.reshape(-1), 5, lr.NONE)
        values = (rng.normal(size=(W * H, words)) * rng.choice([1e-3, 1.0, 1e4], (W * H, 1))).astype(F)
        values[:, channels:] = np.arange(W * H * (words - channels), dtype=np.uint32).reshape(W * H, -1).view(F)  # (counts and padding are words, not floats)
        d_values = torch.from_numpy(values).cuda()
        d_texels = torch.from_numpy(texels.view(np.int32).reshape(-1, 4)).cuda()
        for passes in (0, 1, 4, 254):
            want, want_pass = lr.lightmap_dilate(values, texels, W, H, passes=passes, channels=channels)
            got, pass_of = ds.lightmap_dilate(values, texels, W, H, passes=passes, channels=channels, return_pass_of=True)
            assert_words_equal(got, want, (name, passes, "host"))
            assert (pass_of == want_pass).all(), (name, passes, "host pass_of")
            got, pass_of = ds.lightmap_dilate(d_values, d_texels, W, H, passes=passes, channels=channels, return_pass_of=True)
            assert_words_equal(got.cpu().numpy(), want, (name, passes, "device"))
            assert (pass_of.cpu().numpy() == want_pass).all(), (name, passes, "device pass_of")
            assert_words_equal(ds.lightmap_dilate(d_values, d_texels, W, H, passes=passes, channels=channels).cpu().numpy(), want, (name, passes, "no pass_of"))
            # pass_of on its own terms
            assert ((want_pass == 0) == owned).all() and ((want_pass[~owned] <= passes) | (want_pass[~owned] == 255)).all()
            if passes == 0:
                assert (want_pass[~owned] == 255).all()
            if name == "far corner":
                assert (want_pass[0, 1:] == np.where(np.arange(1, 300) <= passes, np.arange(1, 300), 255)).all()
            if name == "empty":
                assert (want_pass == 255).all() and (want.view(np.uint32) == 0).all()


# ---- 3. the whole bake ------------------------------------------------------------------------------------------------------------------------
def floor_under_a_light():
    """A triangle floor (the jittered grid mesh, its lightmap chart in the middle three quarters of the atlas) under a quad light."""
    V, T, N = lr.grid_mesh(8, 2)
    V, T, N = (np.ascontiguousarray(a[:, [0, 2, 1]]) for a in (V, T, N))  # (wound so that the geometric normals point up, at the light)
    T = np.ascontiguousarray(T * F(0.75) + F(0.125), dtype=F)
    b = SceneBuilder()
    grey = b.Lambertian(b.SolidColor(0.7, 0.7, 0.7))
    first, n = b.triangles(V.astype(np.float64), grey, uvs=T)
    light = b.Quad((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), b.DiffuseLight(8, 8, 8))
    cam = CameraConfig(40.0, 0.0, (0.0, 6.0, 6.0), (0.0, 0.0, 0.0), (0, 1, 0))
    return b.finish(b.Bvh(list(range(first, first + n)) + [light]), cam, (0.0, 0.0, 0.0), RC), V, T, N


def test_points_then_irradiance_then_dilation_is_the_bake_of_the_restatement():
    import torch
    W = H = 32
    sc, V, T, N = floor_under_a_light()
    ref_p, ref_t = lr.lightmap_points(V, T, W, H, normals=N)
    owned = ref_t["triangle"] != lr.NONE
    assert 0.5 * W * H < owned.sum() < 0.65 * W * H  # the chart is (0.75 x 32)^2 = 576 of 1024 texels
    with DeviceScene(sc) as ds:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        points, texels = ds.lightmap_points(dV, dT, W, H, normals=dN)
        rows = ds.irradiance(points, samples=17, seed=SEED)
        baked, pass_of = ds.lightmap_dilate(rows, texels, W, H, passes=2, return_pass_of=True)
        # the same over the restatement's rows
        rgb, samples = ds.irradiance(ref_p, samples=17, seed=SEED)
    ref_rows = np.concatenate([rgb, samples.view(F)[:, None]], axis=1)
    assert_words_equal(rows.cpu().numpy(), ref_rows, "irradiance over the device's points")
    want, want_pass = lr.lightmap_dilate(ref_rows, ref_t, W, H, passes=2, channels=3)
    assert_words_equal(baked.cpu().numpy(), want, "the bake")
    assert (pass_of.cpu().numpy() == want_pass).all()
    assert (samples[owned] == 17).all() and (samples[~owned] == 0).all() and (rgb[~owned] == 0).all()  # an unowned row is an invalid point
    lum = baked.cpu().numpy()[:, :3].sum(axis=1).reshape(H, W)
    under = lum[12:20, 12:20].mean()       # below the light's centre
    corners = np.mean([lum[4:8, 4:8].mean(), lum[4:8, 24:28].mean(), lum[24:28, 4:8].mean(), lum[24:28, 24:28].mean()])
    assert under > 2.0 * corners > 0.0
    ring = want_pass == 1
    assert ring.sum() > 90 and (lum[ring] > 0).mean() > 0.5  # the border took its neighbours' light


# ---- 4. neutrality ----------------------------------------------------------------------------------------------------------------------------
def test_lightmap_calls_between_renders_change_no_frame_plane_or_statistic():
    import torch
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))
    V, T, N = lr.grid_mesh(8, 2)
    T2 = (T * F(0.6) + F(0.2)).astype(F)

    def sequence(ds, between):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        between()
        ds.render(8, 8, SEED)
        between()
        ds.render_aux(0, 4, SEED)
        between()
        radiance = ds.radiance(ds.camera_rays(0, 0, 8, 8, 0, SEED).reshape(-1, 8), samples=3, seed=SEED).cpu().numpy()
        between()
        vis = ds.visibility_to_numpy(ds.visibility(ds.camera_rays(0, 0, 8, 8, 1, SEED).reshape(-1, 8), samples=20, seed=SEED))
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(radiance.tobytes()), zlib.crc32(vis.tobytes()))

    with DeviceScene(sc) as ds:
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T2).cuda()

        def lightmap():
            p, t = ds.lightmap_points(dV, dT, 40, 24, conservative=True)
            ds.lightmap_dilate(ds.irradiance(p, samples=2, seed=SEED), t, 40, 24, passes=3)
            hp, ht = ds.lightmap_points(V, T2, 16, 16, normals=N)
            ds.lightmap_dilate(hp, ht, 16, 16, passes=1, channels=8)

        want = sequence(ds, lambda: None)
        assert sequence(ds, lightmap) == want and want[3]["rays"] > 0


def test_a_scene_with_a_constant_medium_is_not_refused():
    V, T, N = lr.grid_mesh(4, 2)
    sc = scenes.create_test_scene(RC)
    assert sc.desc.n_mediums > 0
    with DeviceScene(sc) as ds:
        p, t = ds.lightmap_points(V, T, 20, 20, normals=N)
        ref_p, ref_t = lr.lightmap_points(V, T, 20, 20, normals=N)
        assert_words_equal(p, ref_p, "points on a scene with a medium")
        assert_words_equal(t, ref_t, "texels on a scene with a medium")
        out = ds.lightmap_dilate(p, t, 20, 20, passes=1, channels=8)
        assert_words_equal(out, lr.lightmap_dilate(p, ref_t, 20, 20, passes=1, channels=8)[0], "dilation on a scene with a medium")
