"""Adaptive irradiance gathers on the device (sol_irradiance_adaptive, sol_radiance_rescale). The anchor is the fixed call: a row that
ends with N samples equals irradiance_moments(samples = N)'s row for the same point and key in all eight words, and which N a row ends with is the
stop rule of csrc/sol_gather_adaptive.h, restated in numpy (tests/irradiance_adaptive_ref.py) and applied to the fixed calls' answers at N = round,
2 round, .. - so the count map, every word and the statistics are compared exactly. Around it: both modes and routes, invalid rows, keys, batch
shapes, the split over points in a child process, every estimator kernel, refusals, neutrality, the rescale and the chain of a bake. Frames are
32 x 32."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import irradiance_adaptive_ref as ar
import lightmap_filter_var_ref as vr
import lightmap_ref as lr
from solstrale_amd import MOMENTS_DTYPE, DeviceError, DeviceScene, RenderConfig, _abi, moments_mean_variance, scenes
from test_gpu_irradiance import INVALID_CLASSES, MODES, RC, SEED, _cornell, _path_stats, _random_mixed, _variation, surface_points, with_invalid_rows
from test_gpu_lightmap_filter import assert_words_equal, floor_under_a_light

pytestmark = pytest.mark.gpu
F = np.float32
FIRST = 5


def _words(rows):
    rows = rows.cpu().numpy() if hasattr(rows, "data_ptr") else rows
    return np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 8)


def _fixed(ds, points, N, mode="cosine", keys=None, key_base=7, first_draw=0, first=FIRST):
    return _words(ds.irradiance_moments(points, samples=N, first_sample=first, seed=SEED, keys=keys, key_base=key_base, first_draw=first_draw, mode=mode))


def _adaptive(ds, points, mx, rnd=16, min_samples=32, threshold=0.0, floor=0.0, mode="cosine", keys=None, key_base=7, first_draw=0, first=FIRST, device=False):
    if device:
        import torch
        points = torch.from_numpy(np.ascontiguousarray(points)).cuda()
        keys = None if keys is None else torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).cuda()
    rows, stats = ds.irradiance_adaptive(points, mx, round=rnd, min_samples=min_samples, threshold=threshold, floor=floor, first_sample=first, seed=SEED, keys=keys,
                                         key_base=key_base, first_draw=first_draw, mode=mode, return_stats=True)
    if device:
        assert rows.is_cuda and tuple(rows.shape) == (len(points), 8)
    else:
        assert rows.dtype == MOMENTS_DTYPE and rows.shape == (len(points),)
    return _words(rows), stats


def median_threshold(fixed_at_min, is_valid, floor):
    """The threshold at which about half the rows stop at the first judgement: the median over the valid rows of max_j v[j] / max(x[j], floor)^2 of the
    fixed call at N = min_samples, through a square root, in float64."""
    x, v = moments_mean_variance(np.ascontiguousarray(fixed_at_min).view(F).reshape(-1, 8))
    x, v = x[is_valid].astype(np.float64), v[is_valid].astype(np.float64)
    ratio = (v / np.maximum(x, float(floor)) ** 2).max(axis=1)
    return float(np.sqrt(np.median(ratio)))


def assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, mx, rnd, min_samples, threshold, floor, device=False, fixed=None, **kw):
    """The call's count map, words and statistics against the restated rule applied to the fixed calls' answers. Returns (counts, verdicts)."""
    fixed = fixed if fixed is not None else {N: _fixed(ds, points, N, **kw) for N in ar.round_counts(mx, rnd)}
    got, stats = _adaptive(ds, points, mx, rnd, min_samples, threshold, floor, device=device, **kw)
    counts, verdicts, rounds = ar.count_map(lambda N: fixed[N], is_valid, mx, rnd, min_samples, threshold, floor)
    assert (got[:, 3] == counts).all(), ("the count map", int((got[:, 3] != counts).sum()), len(counts), np.unique(got[:, 3]), np.unique(counts))
    for N in fixed:
        at = counts == N
        off = int((got[at] != fixed[N][at]).any(axis=1).sum())
        assert off == 0, ("rows that stopped at", N, off, int(at.sum()))
    assert (got[~is_valid] == 0).all() and (got[:, 7] == 0).all()
    assert stats == ar.stats_of(counts, verdicts, rounds), (stats, ar.stats_of(counts, verdicts, rounds))
    return counts, verdicts


# ---- 1. threshold 0: the fixed call, word for word -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_cornell, _random_mixed], ids=["cornell", "random_mixed"])
def test_a_threshold_of_zero_is_the_fixed_call_word_for_word(make):
    sc = make()
    assert sc.desc.n_mediums == 0
    with DeviceScene(sc) as ds:
        points, is_valid = with_invalid_rows(surface_points(sc, ds, 300))
        for mode in MODES:
            for mx in (16, 17, 48, 80):
                want = _fixed(ds, points, mx, mode=mode)
                assert (want[is_valid, 3] == mx).all() and (want[~is_valid] == 0).all() and len({r.tobytes() for r in want}) > 100
                for device in (False, True):
                    got, stats = _adaptive(ds, points, mx, threshold=0.0, mode=mode, device=device)
                    off = int((got != want).any(axis=1).sum())
                    assert off == 0, (mode, mx, device, off)
                    n_valid = int(is_valid.sum())
                    assert stats == {"rounds": -(-mx // 16), "paths": n_valid * mx, "rows_valid": n_valid, "rows_converged": 0, "rows_capped": n_valid}, (mode, mx, stats)
        # a round of 32 and a minimum of 0 change nothing either
        got, stats = _adaptive(ds, points, 80, rnd=32, min_samples=0, threshold=0.0)
        assert (got == _fixed(ds, points, 80)).all() and stats["rounds"] == 3


# ---- 2. a positive threshold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [_cornell, _random_mixed], ids=["cornell", "random_mixed"])
def test_a_positive_threshold_stops_rows_by_the_restated_rule_and_every_row_is_the_fixed_call_of_its_own_count(make):
    """The threshold is the median, over the valid rows of the fixed call at N = min_samples, of the relative variance the rule compares (so about
    half the rows stop at the first judgement). At least a tenth of the valid rows must stop before the maximum and at least a tenth must not stop
    at the first judgement: the map has something to compare."""
    sc = make()
    mx, rnd, min_samples, floor = 96, 16, 32, 0.01
    with DeviceScene(sc) as ds:
        points, is_valid = with_invalid_rows(surface_points(sc, ds, 300))
        for mode in MODES:
            fixed = {N: _fixed(ds, points, N, mode=mode) for N in ar.round_counts(mx, rnd)}
            threshold = median_threshold(fixed[min_samples], is_valid, floor)
            assert threshold > 0 and np.isfinite(threshold)
            for device in (False, True):
                counts, verdicts = assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, mx, rnd, min_samples, threshold, floor, device=device,
                                                                                    fixed=fixed, mode=mode)
            n_valid = int(is_valid.sum())
            early, later = int(((counts < mx) & is_valid).sum()), int(((counts > min_samples) & is_valid).sum())
            print(f"{mode}: threshold {threshold:.4g}: counts {dict(zip(*[a.tolist() for a in np.unique(counts[is_valid], return_counts=True)]))}")
            assert early >= n_valid / 10 and later >= n_valid / 10, (mode, threshold, early, later, n_valid)
            assert (verdicts[is_valid & (counts < mx)] == ar.CONVERGED).all()


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------------------
THRESHOLD, FLOOR = 0.3, 0.01  # (fixed numbers for the shape tests: what they compare is one call against another)


def _shape_inputs(ds, sc):
    rng = np.random.default_rng(9)
    points, is_valid = with_invalid_rows(surface_points(sc, ds, 257 - len(INVALID_CLASSES)))
    keys = np.stack([rng.integers(0, 2 ** 32, 257), 3 * rng.integers(0, 2, 257)], axis=1).astype(np.uint32)  # first_draw 0 and 3
    return points, is_valid, keys


@pytest.fixture(scope="module")
def shapes():
    """The 257 rows, their keys and the whole call's answers with and without keys: computed once, shared and left unchanged."""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        points, is_valid, keys = _shape_inputs(ds, sc)
        want = {use_keys: _adaptive(ds, points, 64, threshold=THRESHOLD, floor=FLOOR, keys=keys if use_keys else None, key_base=40)[0] for use_keys in (True, False)}
    return points, is_valid, keys, want


def test_batch_shape_order_and_keys_do_not_change_a_point_s_answer(shapes):
    """n = 1, 63, 64, 65, 257 and a permutation: the answers follow the points. Keys carry first_draw 0 and 3; without keys key_base and first_draw
    shift the streams, and explicit keys (key_base + i, 3) give first_draw = 3's bits - the compact rows of a later round draw from the stream the
    point would have had in place."""
    points, is_valid, keys, want = shapes
    perm = np.random.default_rng(10).permutation(257)
    with DeviceScene(_cornell()) as ds:
        for use_keys in (True, False):
            whole = want[use_keys]
            assert len(np.unique(whole[is_valid, 3])) >= 2 and (whole[~is_valid] == 0).all(), np.unique(whole[:, 3])
            assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, 64, 16, 32, THRESHOLD, FLOOR, keys=keys if use_keys else None, key_base=40)
            for n in (1, 63, 64, 65):
                part, _ = _adaptive(ds, points[:n], 64, threshold=THRESHOLD, floor=FLOOR, keys=keys[:n] if use_keys else None, key_base=40)
                assert (part == whole[:n]).all(), (use_keys, n)
            if use_keys:
                got, _ = _adaptive(ds, points[perm], 64, threshold=THRESHOLD, floor=FLOOR, keys=keys[perm], key_base=40, device=True)
                assert (got == whole[perm]).all(), "a permutation"
                continue
            tail, _ = _adaptive(ds, points[100:], 64, threshold=THRESHOLD, floor=FLOOR, key_base=140)
            assert (tail == whole[100:]).all()
            shifted, _ = _adaptive(ds, points, 64, threshold=THRESHOLD, floor=FLOOR, key_base=40, first_draw=3)
            assert (shifted != whole).any()
            k3 = np.stack([40 + np.arange(257), np.full(257, 3)], axis=1).astype(np.uint32)
            for device in (False, True):
                explicit, _ = _adaptive(ds, points, 64, threshold=THRESHOLD, floor=FLOOR, keys=k3, key_base=0, device=device)
                assert (explicit == shifted).all(), device
            assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, 64, 16, 32, THRESHOLD, FLOOR, key_base=40, first_draw=3)


CHILD = """
import sys
import numpy as np
from solstrale_amd import DeviceScene, RenderConfig, scenes
a = np.load(sys.argv[1])
out = {}
with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
    for k, use_keys in enumerate((True, False)):
        rows, stats = ds.irradiance_adaptive(a["points"], 64, round=16, min_samples=32, threshold=float(a["threshold"]), floor=float(a["floor"]), first_sample=5,
                                             seed=int(a["seed"]), keys=a["keys"] if use_keys else None, key_base=40, return_stats=True)
        out[f"rows{k}"] = rows.view(np.uint32).reshape(-1, 8)
        out[f"stats{k}"] = np.array([stats[n] for n in ("rounds", "paths", "rows_valid", "rows_converged", "rows_capped")], dtype=np.uint64)
np.savez(sys.argv[2], **out)
"""


def test_the_split_over_points_does_not_change_a_point_s_answer(shapes, tmp_path):
    """SOL_GATHER_ROWS is read at creation: a bound of 64 rows runs in a fresh child process. 257 points then go in five parts, each with its own
    rounds and compaction; the rows are the default bound's, bit for bit, and so are the statistics - rounds is the most any part ran."""
    points, is_valid, keys, want = shapes
    np.savez(tmp_path / "in.npz", points=points, keys=keys, seed=SEED, threshold=THRESHOLD, floor=FLOOR)
    env = {**os.environ, "SOL_GATHER_ROWS": "64", "PYTHONPATH": os.pathsep.join(p for p in sys.path if p)}
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "out.npz")
    with DeviceScene(_cornell()) as ds:
        for k, use_keys in enumerate((True, False)):
            assert (got[f"rows{k}"] == want[use_keys]).all(), use_keys
            _, stats = _adaptive(ds, points, 64, threshold=THRESHOLD, floor=FLOOR, keys=keys if use_keys else None, key_base=40)
            assert got[f"stats{k}"].tolist() == [stats[n] for n in ("rounds", "paths", "rows_valid", "rows_converged", "rows_capped")], use_keys


# ---- 4. every estimator kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["env_importance", "light_tree", "needles_strict", "deep_chain_spill"])
def test_the_rounds_are_the_fixed_call_in_every_estimator_kernel(name, monkeypatch):
    make, env, env_mode, light_mode, expect = _variation(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = make()
    assert sc.desc.n_mediums == 0
    with DeviceScene(sc) as ds:
        info = ds.info()
        if "strict_triangles" in expect:
            assert info["strict_triangles"]
        if "spill" in expect:
            assert info["stack_bound"] > info["lds_stack"], info
        points = surface_points(sc, ds, 24, hover=0.5)
        if env_mode:
            ds.env_sampling(env_mode)
        if light_mode:
            ds.light_sampling(light_mode)
        is_valid = np.ones(24, bool)
        fixed = {N: _fixed(ds, points, N) for N in ar.round_counts(64, 16)}
        assert np.isfinite(fixed[64].view(F)[:, :3]).all() and np.abs(fixed[64].view(F)[:, :3]).sum() > 0
        assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, 64, 16, 32, 0.0, 0.0, fixed=fixed)
        threshold = median_threshold(fixed[32], is_valid, 0.01)
        assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, 64, 16, 32, threshold, 0.01, fixed=fixed)
        assert_adaptive_is_the_rule_over_the_fixed_calls(ds, points, is_valid, 64, 16, 32, threshold, 0.01, fixed=fixed, device=True)


# ---- 5. refusals and neutrality --------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_handle():
    point = np.array([[0., 0., 0., 0.001, 0., 1., 0., np.inf]], dtype=np.float32)
    CFG, AD, STATS = _abi.SolIrradianceConfig, _abi.SolGatherAdaptive, _abi.SolGatherAdaptiveStats
    cfg = lambda **kw: CFG(**{**dict(size=C.sizeof(CFG), samples=32), **kw})
    ad = lambda **kw: AD(**{**dict(size=C.sizeof(AD), round=16, min_samples=16, threshold=0.1, floor=0.0), **kw})
    with DeviceScene(scenes.create_test_scene(RC)) as ds:  # (a constant medium)
        for f in (lambda: ds.irradiance_adaptive(point, 32), lambda: ds.irradiance_adaptive(point, 32, mode="sphere", threshold=0.0)):
            with pytest.raises(DeviceError) as e:
                f()
            assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        for fn in (ds.lib.sol_irradiance_adaptive, ds.lib.sol_irradiance_adaptive_dev):
            assert fn(ds.h, None, None, 0, C.byref(cfg()), C.byref(ad()), None, None) == _abi.SOL_OK  # n == 0 succeeds on any scene
            assert fn(ds.h, None, None, 1, C.byref(cfg()), C.byref(ad()), None, None) == _abi.SOL_EINVAL and b"medium" in ds.lib.sol_last_error()  # before the pointers
            assert fn(ds.h, None, None, 1, C.byref(cfg()), C.byref(ad(round=8)), None, None) == _abi.SOL_EINVAL and b"round" in ds.lib.sol_last_error()  # after the rule
        # nothing is traced by the rescale: a scene with a medium is served
        rows = np.array([[2.0, 4.0, 8.0, 0.0]], dtype=F)
        rows.view(np.uint32)[0, 3] = 2
        assert ds.radiance_rescale(rows, 8).view(np.uint32).tolist() == [[F(8.0).view(np.uint32), F(16.0).view(np.uint32), F(32.0).view(np.uint32), 8]]
    with DeviceScene(_cornell()) as ds:
        lib, out = ds.lib, np.full(8, 7, np.uint32)
        for name, fn in (("sol_irradiance_adaptive", lib.sol_irradiance_adaptive), ("sol_irradiance_adaptive_dev", lib.sol_irradiance_adaptive_dev)):
            def call(c=cfg(), a=ad(), pts=point.ctypes.data, n=1, o=out.ctypes.data, st=None):
                return fn(ds.h, pts, None, n, C.byref(c) if c is not None else None, C.byref(a) if a is not None else None, o, st)
            for kw, word in ((dict(c=cfg(samples=0)), b"samples"), (dict(c=None), b"null configuration"), (dict(c=cfg(mode=2)), b"mode"),
                             (dict(a=None), b"null adaptive configuration"), (dict(a=ad(size=28)), b"SolGatherAdaptive.size"), (dict(a=ad(reserved=3)), b"reserved"),
                             (dict(a=ad(round=0)), b"round"), (dict(a=ad(round=40)), b"round"), (dict(a=ad(min_samples=17)), b"min_samples"),
                             (dict(a=ad(threshold=-1.0)), b"threshold"), (dict(a=ad(floor=float("nan"))), b"floor"),
                             (dict(st=C.byref(STATS(size=8))), b"SolGatherAdaptiveStats"), (dict(pts=None), b"null point"), (dict(o=None), b"null output")):
                assert call(**kw) == _abi.SOL_EINVAL and word in lib.sol_last_error() and name.encode() + b":" in lib.sol_last_error(), (name, word, lib.sol_last_error())
            assert call(pts=None, n=0, o=None) == _abi.SOL_OK
        assert (out == 7).all()
        for kw in (dict(round=24), dict(min_samples=8), dict(threshold=float("inf")), dict(floor=-0.5)):
            with pytest.raises(DeviceError) as e:
                ds.irradiance_adaptive(point, 32, **kw)
            assert e.value.code == _abi.SOL_EINVAL
        with pytest.raises(ValueError):
            ds.irradiance_adaptive(point, 32, mode="ambient")
        with pytest.raises(DeviceError):
            ds.radiance_rescale(np.zeros((1, 4), F), 0)


def test_adaptive_gathers_between_renders_change_no_frame_plane_statistic_or_other_query():
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))

    def sequence(ds, points, query):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        query()
        ds.render(8, 8, SEED)
        query()
        ds.render_aux(0, 4, SEED)
        query()
        irr = ds.irradiance(points, samples=20, first_sample=1, seed=SEED, key_base=3)[0]
        query()
        mom = ds.irradiance_moments(points, samples=20, first_sample=1, seed=SEED, key_base=3)
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return (zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds)),
                zlib.crc32(irr.tobytes()), zlib.crc32(mom.tobytes()))

    with DeviceScene(sc) as ds:
        points = surface_points(sc, ds, 64)

        def query():
            ds.irradiance_adaptive(points, 48, threshold=0.3, floor=0.01, seed=SEED)
            ds.irradiance_adaptive(points, 40, round=32, min_samples=0, threshold=0.0, first_sample=3, seed=SEED, key_base=5, mode="sphere")
            ds.radiance_rescale(np.ones((5, 4), F), 3)

        want = sequence(ds, points, lambda: None)
        assert sequence(ds, points, query) == want and want[3]["rays"] > 0


# ---- 6. the rescale ----------------------------------------------------------------------------------------------------------------------------
def test_the_rescale_is_the_restatement_word_for_word_on_both_routes_in_place_and_out_of_place():
    import torch
    rng = np.random.default_rng(21)
    n = 1000  # (four workgroups, the last one short)
    rows = np.zeros((n, 4), F)
    rows[:, :3] = ((rng.uniform(0, 1, (n, 3)) ** 6 * 1e4) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    cnt = rows.view(np.uint32)[:, 3]
    cnt[:] = rng.integers(1, 200, n)
    cnt[::7] = 0
    cnt[1::7] = 1
    cnt[2::7] = 16777217 + 2 * rng.integers(0, 1000, len(cnt[2::7]))  # above 2^24: float32 cannot hold them
    cnt[3::7] = 64
    rows[5, :3], rows[6, :3], rows[12, :3] = (np.inf, -0.0, np.nan), (F(3e38), F(1e-42), F(-1e-45)), (F(3e38), F(-3e38), 0.0)
    with DeviceScene(_cornell()) as ds:
        for target in (1, 64, 96, (1 << 24) + 3, 0xFFFFFFFF):
            want = ar.rescale(rows, target)
            assert_words_equal(ds.radiance_rescale(rows, target), want, ("host", target))
            dev = torch.from_numpy(rows).cuda()
            out = ds.radiance_rescale(dev, target)
            assert out.data_ptr() != dev.data_ptr()
            assert_words_equal(out.cpu().numpy(), want, ("device", target))
            assert_words_equal(dev.cpu().numpy(), rows, "the input is not written")
            assert ds.radiance_rescale(dev, target, in_place=True) is dev
            assert_words_equal(dev.cpu().numpy(), want, ("device, in place", target))
            mine = rows.copy()
            assert ds.radiance_rescale(mine, target, in_place=True) is mine
            assert_words_equal(mine, want, ("host, in place", target))
        same = rows[3::7].copy()
        assert (ds.radiance_rescale(same, 64).view(np.uint32) == same.view(np.uint32))[~np.isnan(same).any(axis=1)].all()  # equal counts: bit for bit
        assert ds.radiance_rescale(np.zeros((0, 4), F), 5).shape == (0, 4)


# ---- 7. the chain ------------------------------------------------------------------------------------------------------------------------------
def test_a_bake_through_the_adaptive_gather_the_filter_the_rescale_and_the_dilation():
    """lightmap_points -> irradiance_adaptive -> lightmap_filter_var -> radiance_rescale -> lightmap_dilate on device memory over a 16 x 16 atlas,
    against the numpy restatements of the filter, the rescale and the dilation fed the adaptive rows, word for word; the adaptive rows themselves
    against the rule over the fixed calls."""
    import torch
    W = H = 16
    mx, floor = 64, 0.01
    sc, V, T, N = floor_under_a_light()
    sigma = 2.0 * 4.0 / (0.75 * W)
    with DeviceScene(sc) as ds:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        points, texels = ds.lightmap_points(dV, dT, W, H, normals=dN)
        p, t = points.cpu().numpy(), texels.cpu().numpy().view(lr.TEXEL_DTYPE).reshape(-1)
        owned = t["triangle"] != lr.NONE
        assert 0.3 * W * H < owned.sum() < 0.8 * W * H
        fixed = {n: _fixed(ds, p, n, key_base=0, first=0) for n in ar.round_counts(mx, 16)}
        threshold = median_threshold(fixed[32], owned, floor)
        counts, _ = assert_adaptive_is_the_rule_over_the_fixed_calls(ds, p, owned, mx, 16, 32, threshold, floor, fixed=fixed, device=True, key_base=0, first=0)
        assert len(np.unique(counts[owned])) >= 2, np.unique(counts)
        rows = ds.irradiance_adaptive(points, mx, threshold=threshold, floor=floor, seed=SEED)
        filtered = ds.lightmap_filter_var(rows, points, texels, W, H, sigma_position=sigma)
        rescaled = ds.radiance_rescale(filtered, mx)
        dilated = ds.lightmap_dilate(rescaled, texels, W, H, passes=2)
        rows_np = rows.cpu().numpy()
        assert (_words(rows_np)[:, 3] == counts).all()
        want_filtered, _ = vr.lightmap_filter_var(rows_np, p, t, W, H, sigma_position=sigma)
        assert_words_equal(filtered.cpu().numpy(), want_filtered, "the filter")
        assert (want_filtered.view(np.uint32)[:, 3] == counts).all(), "the filter carries each row's own count"
        want_rescaled = ar.rescale(want_filtered, mx)
        assert_words_equal(rescaled.cpu().numpy(), want_rescaled, "the rescale")
        assert (want_rescaled.view(np.uint32)[owned, 3] == mx).all() and (want_rescaled.view(np.uint32)[~owned, 3] == 0).all()
        want_dilated, _ = lr.lightmap_dilate(want_rescaled, t, W, H, passes=2)
        assert_words_equal(dilated.cpu().numpy(), want_dilated, "the dilation")
