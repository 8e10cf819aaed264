"""Queries, gathers and bakes past their first size boundaries (profiles/size_boundaries.txt). Every other GPU test gives a kernel
less work than one launch of one small grid; these give it the smallest input that crosses a boundary of the code: several items per resident lane
of a persistent kernel (the refill of csrc/sol_wave.h), more workgroup counts than the scan's 1024 threads (csrc/sol_gather_adaptive.hip), more
than one tile of the render's compaction (csrc/sol_adaptive.hip), more rows than a host route stages at a time, more elements than a capped grid
has threads. Every check is exact: the expected words are those of a small call of the same entry point - whose correctness the other tests pin
against the oracle or a restatement - or an existing numpy restatement. tests/size_boundaries.py holds the construction: a base set of a few hundred
distinct rows, indexed by a seeded random array."""
import numpy as np
import pytest

import image_metric as im
import irradiance_adaptive_ref as ar
import post as opost  # (test infrastructure: the bloom restatement)
import size_boundaries as sb
import test_gpu_adaptive as ta
import test_gpu_queries as tq
from size_boundaries import SETTINGS, WINDOW, to_dev, keys_to_dev, words
from solstrale_amd import DeviceScene, RenderConfig, _abi, scenes
from test_gpu_irradiance import SEED, _cornell, _deep_chain, _random_mixed, surface_points, with_invalid_rows
from test_gpu_irradiance_adaptive import _fixed, median_threshold

pytestmark = pytest.mark.gpu
F = np.float32
FIRST = 5
HIT, MISS, INVALID = _abi.SOL_RAY_HIT, _abi.SOL_RAY_MISS, _abi.SOL_RAY_INVALID
MODES = ("cosine", "sphere")
# name -> (the gathers' scene, the queries' scene, environment, the settings it runs under). The deep chain under SOL_BVH=ref searches past the LDS
# stack: once per kernel family, eight items per lane of one workgroup per CU - the spill tail of a lane that took a second item.
SCENES = {"cornell": (_cornell, tq._cornell, {}, SETTINGS), "random_mixed": (_random_mixed, tq._random_mixed, {}, SETTINGS),
          "deep_chain_spill": (_deep_chain, tq._deep_chain, {"SOL_BVH": "ref"}, ((1, 8),))}


def _open(name, monkeypatch, queries=False):
    gather, query, env, settings = SCENES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = (query if queries else gather)()
    assert sc.desc.n_mediums == 0
    ds = DeviceScene(sc)
    if env:
        info = ds.info()
        assert info["stack_bound"] > info["lds_stack"], info
    return sc, ds, settings


def _keys_for(n, seed=31):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 2 ** 32, n), 3 * rng.integers(0, 2, n)], axis=1).astype(np.uint32)  # (first_draw 0 and 3)


def _base_points(name, sc, ds):
    """A few hundred surface points with one invalid row of every class; on the chain, whose frame shows few surfaces, 24 points twelve times over -
    the rows' keys differ. Returns (rows, is_valid, keys)."""
    p = np.tile(surface_points(sc, ds, 24, hover=0.5), (12, 1)) if name == "deep_chain_spill" else surface_points(sc, ds, 300)
    points, is_valid = with_invalid_rows(p)
    return points, is_valid, _keys_for(len(points))


def _base_rays(sc, ds):
    """tests/test_gpu_queries.py's mix, 800 rays - every miss is one and the same answer, so the distinct ones are the hits - and the invalid rows."""
    rays, is_valid = with_invalid_rows(tq.ray_mix(sc, ds, 7, per_class=200))
    return rays, is_valid, _keys_for(len(rays))


def _boundaries(bpc):
    return (1 << 18, 1 << 20, sb.resident_lanes(bpc))


def _refill_case(ds, call, base, keys, n_of, items_of, settings, what, min_distinct=100):
    """The shared construction for one family: the small call decides whether the base set will do; then, under every setting, the big call with
    the base rows' keys against it and - keys given - the big call without keys against windows of small calls."""
    base_dev, keys_dev = to_dev(base), None if keys is None else keys_to_dev(keys)
    sb.apply(ds, 0, 0)
    small = words(call(base_dev, keys_dev, 0))
    assert sb.distinct_rows(small) >= min_distinct, (what, sb.distinct_rows(small))
    for k, (bpc, switch_below) in enumerate(settings):
        sb.apply(ds, bpc, switch_below)
        n = n_of(bpc)
        sb.assert_refills(items_of(n), bpc)
        idx = sb.assert_copies_equal_the_small_call(call, base_dev, keys_dev, small, n, 100 + k, (what, bpc, switch_below))
        if keys is not None:
            rows = base_dev[to_dev(idx)]
            sb.assert_windows_equal_small_calls(call, rows, 40, _boundaries(bpc), 200 + k, (what, bpc, switch_below, "no keys"))
    sb.apply(ds, 0, 0)
    return small


# ---- 1. queries: more rays than lanes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_ray_queries_answer_every_ray_of_a_batch_of_several_per_lane(name, monkeypatch):
    """closest_hits and occluded over device tensors: the grid is min(n_cu x blocks_per_cu, ceil(n / 256)), and whole waves stride over the batch
    from the second ray of a lane on."""
    sc, ds, settings = _open(name, monkeypatch, queries=True)
    with ds:
        rays, is_valid, _ = _base_rays(sc, ds)
        status = ds.closest_hits(rays)["status"]
        assert (status[~is_valid] == INVALID).all() and (status == HIT).sum() >= 10 and (status == MISS).sum() >= 10, np.unique(status, return_counts=True)
        _refill_case(ds, lambda r, k, kb: ds.closest_hits(r), rays, None, lambda bpc: sb.rows_for(bpc, 1), sb.plan_items, settings, "closest_hits")
        _refill_case(ds, lambda r, k, kb: ds.occluded(r), rays, None, lambda bpc: sb.rows_for(bpc, 1), sb.plan_items, settings, "occluded", min_distinct=3)


# ---- 2. radiance: one chunk (direct) and three (the partial buffer and the resolve) -----------------------------------------------------------------
@pytest.mark.parametrize("samples", [16, 48], ids=["one_chunk_direct", "three_chunks_resolved"])
@pytest.mark.parametrize("name", list(SCENES))
def test_radiance_refills_its_lanes(name, samples, monkeypatch):
    sc, ds, settings = _open(name, monkeypatch, queries=True)
    chunks = -(-samples // 16)
    with ds:
        rays, is_valid, keys = _base_rays(sc, ds)
        call = lambda r, k, kb: ds.radiance(r, samples=samples, first_sample=FIRST, seed=SEED, keys=k, key_base=kb)
        small = _refill_case(ds, call, rays, keys, lambda bpc: sb.rows_for(bpc, chunks), lambda n: sb.plan_items(n, samples), settings, ("radiance", samples))
        small = small.cpu().numpy()
        assert (small[is_valid, 3] == samples).all() and (small[~is_valid] == 0).all()
        status = ds.closest_hits(rays)["status"]  # (paths of one ray beside paths that bounce: the lanes of a wave finish at different times)
        assert (status == HIT).sum() >= 10 and (status == MISS).sum() >= 10, np.unique(status, return_counts=True)


# ---- 3. chunk sums: irradiance and visibility, 48 samples --------------------------------------------------------------------------------------------
def _gather_call(ds, family, mode):
    kw = lambda k, kb: dict(samples=48, first_sample=FIRST, seed=SEED, keys=k, key_base=kb, mode=mode)
    if family == "irradiance":
        return lambda p, k, kb: ds.irradiance(p, **kw(k, kb))
    return lambda p, k, kb: ds.visibility(p, distances=family == "visibility_distances", **kw(k, kb))


def _with_radius(ds, points, is_valid):
    """Half of the valid points get a finite tmax, the median distance at which their first sixteen sphere samples hit: misses beside hits."""
    probe = ds.visibility_to_numpy(ds.visibility(to_dev(points), samples=16, seed=SEED, mode="sphere", distances=True))
    hit = probe["hits"] > 0
    assert hit.any()
    radius = F(np.median(probe["t_sum"][hit] / probe["hits"][hit]))
    assert np.isfinite(radius) and radius > 0
    out = points.copy()
    half = is_valid & (np.arange(len(points)) % 2 == 0)
    out[half, 7] = radius
    return out


@pytest.mark.parametrize("family", ["irradiance", "visibility_occluded", "visibility_distances"])
@pytest.mark.parametrize("name", list(SCENES))
def test_chunk_sum_gathers_refill_their_lanes(name, family, monkeypatch):
    """Items are (chunk, point) pairs: chunks x groups x 64 of them."""
    sc, ds, settings = _open(name, monkeypatch)
    with ds:
        points, is_valid, keys = _base_points(name, sc, ds)
        if family != "irradiance":
            points = _with_radius(ds, points, is_valid)
        for mode in MODES:
            small = _refill_case(ds, _gather_call(ds, family, mode), points, keys, lambda bpc: sb.rows_for(bpc, 3), lambda n: sb.plan_items(n, 48), settings,
                                 (family, mode)).cpu().numpy()
            assert (small[~is_valid] == 0).all()
            if family != "irradiance":
                v = small.view(np.uint32)
                assert (v[is_valid, 7] == 48).all() and (v[is_valid, 3] > 0).sum() >= 30 and (v[is_valid, 6] > 0).sum() >= 30, (family, mode)  # open, hits


# ---- 4. per sample: SH, moments and the octahedral maps ----------------------------------------------------------------------------------------------
PER_SAMPLE = {"sh": ({}, lambda ds, kw: lambda p, k, kb: ds.irradiance_sh(p, keys=k, key_base=kb, **kw)),
              "moments": ({}, lambda ds, kw: lambda p, k, kb: ds.irradiance_moments(p, keys=k, key_base=kb, **kw)),
              "oct4": ({}, lambda ds, kw: lambda p, k, kb: ds.visibility_oct(p, res=4, keys=k, key_base=kb, **kw)),
              "oct8": ({}, lambda ds, kw: lambda p, k, kb: ds.visibility_oct(p, res=8, keys=k, key_base=kb, **kw)),
              "oct4_plain": ({"SOL_DEPTH_PROJECT": "plain"}, lambda ds, kw: lambda p, k, kb: ds.visibility_oct(p, res=4, keys=k, key_base=kb, **kw)),
              "oct8_plain": ({"SOL_DEPTH_PROJECT": "plain"}, lambda ds, kw: lambda p, k, kb: ds.visibility_oct(p, res=8, keys=k, key_base=kb, **kw))}
PER_SAMPLE_CASES = [(n, f) for n in SCENES for f in PER_SAMPLE if not (f.endswith("_plain") and n != "cornell")]


@pytest.mark.parametrize("name, family", PER_SAMPLE_CASES)
def test_per_sample_gathers_refill_their_lanes(name, family, monkeypatch):
    """Items are (sample, point) pairs, samples x groups x 64 of them, and a projection kernel follows the trace: 2^18 + 65 points x 16 samples under
    every setting. Both projection kernels of the octahedral maps (SOL_DEPTH_PROJECT=plain: the measured alternative)."""
    env, make = PER_SAMPLE[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, ds, settings = _open(name, monkeypatch)
    n = (1 << 18) + 65
    assert n >= 262145
    with ds:
        points, is_valid, keys = _base_points(name, sc, ds)
        if family.startswith("oct"):
            points = _with_radius(ds, points, is_valid)
        call = make(ds, dict(samples=16, first_sample=FIRST, seed=SEED))
        small = _refill_case(ds, call, points, keys, lambda bpc: n, lambda m: sb.plan_items(m, 16, per_sample=True), settings, family).cpu().numpy()
        assert (small[~is_valid] == 0).all() and (small[is_valid] != 0).any(axis=1).all()


# ---- 5. the adaptive gather: more workgroup counts than the scan has threads -------------------------------------------------------------------------
ADAPTIVE = dict(mx=64, rnd=16, min_samples=32, floor=0.01)
SCAN_ROWS = (1024 * 256, 1024 * 256 + 1, 2048 * 256 + 1)  # n_wg = 1024 (a count per thread), 1025 (per = 2, half the threads idle), 2049 (per = 3)


def _adaptive_call(ds, host, threshold, stats_out=None):
    def call(p, k, kb):
        if host:
            p, k = p.cpu().numpy() if hasattr(p, "data_ptr") else p, None if k is None else k.cpu().numpy().view(np.uint32)
        rows, stats = ds.irradiance_adaptive(p, ADAPTIVE["mx"], round=ADAPTIVE["rnd"], min_samples=ADAPTIVE["min_samples"], threshold=threshold,
                                             floor=ADAPTIVE["floor"], first_sample=FIRST, seed=SEED, keys=k, key_base=kb, return_stats=True)
        if stats_out is not None:
            stats_out.append(stats)
        return rows.view(np.uint32).reshape(-1, 8) if host else rows
    return call


@pytest.mark.parametrize("name, host", [("cornell", True), ("cornell", False), ("random_mixed", False), ("deep_chain_spill", False)],
                         ids=["cornell-host", "cornell-device", "random_mixed-device", "deep_chain_spill-device"])
def test_the_adaptive_gather_scans_more_workgroups_than_threads(name, host, monkeypatch):
    """Active rows n with ceil(n / 256) = 1024, 1025 and 2049 workgroup counts for the one workgroup of 1024 threads that scans them. With keys the
    count map and every word are the small call's - itself the rule over the fixed calls - and the statistics those of the copies; without keys
    windows are small calls, and the statistics add up. The threshold is the median of the base set: between a tenth and nine tenths of its
    valid rows stop before the maximum, so later rounds compact."""
    sc, ds, settings = _open(name, monkeypatch)
    mx, rnd, min_samples, floor = (ADAPTIVE[k] for k in ("mx", "rnd", "min_samples", "floor"))
    with ds:
        points, is_valid, keys = _base_points(name, sc, ds)
        fixed = {N: _fixed(ds, points, N, keys=keys, key_base=0) for N in ar.round_counts(mx, rnd)}
        threshold = median_threshold(fixed[min_samples], is_valid, floor)
        assert threshold > 0 and np.isfinite(threshold)
        counts, verdicts, rounds = ar.count_map(lambda N: fixed[N], is_valid, mx, rnd, min_samples, threshold, floor)
        early = int(((counts < mx) & is_valid).sum())
        assert 0.1 * is_valid.sum() <= early <= 0.9 * is_valid.sum(), (early, int(is_valid.sum()))
        stats = []
        call = _adaptive_call(ds, host, threshold, stats)
        base_dev, keys_dev = to_dev(points), keys_to_dev(keys)
        small = words(call(base_dev, keys_dev, 0))
        got = small.cpu().numpy().view(np.uint32)
        assert (got[:, 3] == counts).all() and all((got[counts == N] == fixed[N][counts == N]).all() for N in fixed) and (got[~is_valid] == 0).all()
        assert stats[-1] == ar.stats_of(counts, verdicts, rounds) and sb.distinct_rows(small) >= 100
        picks = settings if len(settings) == 1 else ((1, 8), (0, 0), (0, 64))
        for k, n in enumerate(SCAN_ROWS):
            bpc, switch_below = picks[k % len(picks)]
            sb.apply(ds, bpc, switch_below)
            n_wg = -(-n // 256)
            assert n_wg == (1024, 1025, 2049)[k] and -(-n_wg // 1024) == (1, 2, 3)[k]
            sb.assert_refills(sb.plan_items(n, rnd, per_sample=True), bpc)
            idx = sb.assert_copies_equal_the_small_call(call, base_dev, keys_dev, small, n, 300 + k, (name, host, n, "keys"))
            assert stats[-1] == ar.stats_of(counts[idx], verdicts[idx], rounds), (n, stats[-1])
            big = sb.assert_windows_equal_small_calls(call, base_dev[to_dev(idx)], 40, (1 << 18, 1 << 19), 400 + k, (name, host, n, "no keys"))
            whole = stats[-1 - len(sb.window_spans(n, (1 << 18, 1 << 19), 400 + k))]
            final = big[:, 3].cpu().numpy().view(np.uint32)
            assert whole["paths"] == int(final.astype(np.uint64).sum()) and whole["rows_valid"] == int((final > 0).sum()) == int(is_valid[idx].sum())
            assert whole["rows_converged"] + whole["rows_capped"] == whole["rows_valid"] and len(np.unique(final)) >= 3, (n, whole)


# ---- 6. the adaptive render: more than one tile of the compaction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("work_order", [0, 1], ids=["identity_order", "work_order"])
@pytest.mark.parametrize("size", [(264, 264), (300, 260)], ids=["264x264", "ragged_300x260"])
def test_an_adaptive_render_of_more_than_1024_blocks_compacts_every_tile(size, work_order):
    """The compaction walks the work order in tiles of 1024 blocks and carries the count of the tiles in front: 1089 and 1254 local blocks. Every
    pixel is the fixed render of its block's count and the count map is the restated stop rule, on a scene with background blocks, under both work
    orders. (A partition of two ranks is refused by sol_adaptive_begin - adaptive sampling is single-rank, tests/test_gpu_adaptive.py pins the
    refusal -, so there is no such case.)"""
    w, h = size
    rnd, mn, mx = 16, 32, 96
    sc = scenes.statue_like(RenderConfig(w, h, mx), n_triangles=20000)
    assert ((w + 7) // 8) * ((h + 7) // 8) > 1024
    with DeviceScene(sc) as ds:
        ds.set_option(_abi.OPT_WORK_ORDER, work_order)
        assert ds.info()["background_blocks"] > 0
        sums = ta._round_sums(ds, rnd, mx)
        for thr in (0.03, 0.1):
            img, counts = ta._adaptive(ds, rnd, mn, mx, thr)
            ta._assert_matches_fixed(ds, img, counts)
            want, near = ta._restate(sums, rnd, mn, mx, thr, w, h)
            differ = counts != want
            assert not (differ & ~near).any(), (thr, np.argwhere(differ & ~near)[:8])
            assert (counts > mn).any() and (counts == mn).any(), thr  # (some blocks go on past the first judgement, others have stopped: the lists shrink)


# ---- 7. host routes: more rows than the staging holds --------------------------------------------------------------------------------------------------
GATHER_CAP = 1 << 20  # SOL_GATHER_STAGE_POINTS, RESCALE_STAGE_ROWS
QUERY_CAP = 1 << 22   # QUERY_STAGE_RAYS
DEPTH_CAP = (1 << 24) // (16 * 16)  # DEPTH_STAGE_TEXELS / res^2 at res = 16


def _host_route_case(host_call, dev_call, base, keys, cap, what, key_base=7):
    """n = cap + 65 rows through the host route, which stages `cap` at a time: without keys the device route's words over the same rows and windows
    of small host calls on each side of the cap; with keys the small host call's rows and the device route's again."""
    n = cap + 65
    idx = sb.random_index(len(base), n, 17)
    rows = np.ascontiguousarray(base[idx])
    rows_dev = to_dev(rows)
    whole = sb.assert_windows_equal_small_calls(host_call, rows, key_base, (cap,), 18, (what, "host, no keys"), host=True)
    off, where = sb.rows_off(whole, words(dev_call(rows_dev, None, key_base)))
    assert off == 0, (what, "host and device route, no keys", off, where)
    # (a row's answer depends on its key: a window computed from another key_base would differ in many rows - with one sample most dark rows are alike)
    assert sb.distinct_rows(whole[:WINDOW]) >= 30 and sb.distinct_rows(whole[cap:]) >= 10, (sb.distinct_rows(whole[:WINDOW]), sb.distinct_rows(whole[cap:]))
    del whole
    if keys is None:
        return
    small = words(host_call(base, keys, 0))
    assert sb.distinct_rows(small) >= 100
    big = words(host_call(rows, np.ascontiguousarray(keys[idx]), 0))
    off, where = sb.rows_off(big, small[to_dev(idx)])
    assert off == 0, (what, "host route with keys against the small call", off, where)
    off, where = sb.rows_off(big, words(dev_call(rows_dev, keys_to_dev(keys[idx]), 0)))
    assert off == 0, (what, "host and device route with keys", off, where)


def _joined(answer):
    """The host route's (sums, counts) as the device route's four words."""
    rgb, cnt = answer
    return np.concatenate([rgb.view(np.uint32), cnt.reshape(-1, 1)], axis=1)


def _dev_or_host(fn, join=None):
    """call(rows, keys, key_base) for either route of a public method: device tensors pass through, host arrays come back as uint32 words."""
    def call(p, k, kb):
        out = fn(p, k, kb)
        if hasattr(out, "data_ptr"):
            return out
        out = join(out) if join else out
        return np.ascontiguousarray(out).view(np.uint32).reshape(len(p), -1)
    return call


@pytest.mark.parametrize("family", ["irradiance", "irradiance_moments", "radiance"])
def test_a_gather_s_host_route_stages_more_than_its_cap(family):
    sc = tq._cornell() if family == "radiance" else _cornell()
    with DeviceScene(sc) as ds:
        base, _, keys = _base_rays(sc, ds) if family == "radiance" else _base_points("cornell", sc, ds)
        kw = dict(samples=1, first_sample=FIRST, seed=SEED)
        if family == "irradiance":
            call = _dev_or_host(lambda p, k, kb: ds.irradiance(p, keys=k, key_base=kb, **kw), _joined)
        elif family == "radiance":
            call = _dev_or_host(lambda p, k, kb: ds.radiance(p, keys=k, key_base=kb, **kw), _joined)
        else:
            call = _dev_or_host(lambda p, k, kb: ds.irradiance_moments(p, keys=k, key_base=kb, **kw))
        _host_route_case(call, call, base, keys, GATHER_CAP, family)


def test_the_adaptive_gather_s_host_route_stages_more_than_its_cap():
    """Threshold 0, one round of 16: the fixed call over the same rows, word for word, through the staging of sol_irradiance_adaptive."""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        base, is_valid, keys = _base_points("cornell", sc, ds)
        stats = []

        def adaptive(p, k, kb):
            rows, st = ds.irradiance_adaptive(p, 16, round=16, min_samples=0, threshold=0.0, first_sample=FIRST, seed=SEED, keys=k, key_base=kb, return_stats=True)
            stats.append(st)
            return rows

        fixed = _dev_or_host(lambda p, k, kb: ds.irradiance_moments(p, samples=16, first_sample=FIRST, seed=SEED, keys=k, key_base=kb))
        _host_route_case(_dev_or_host(adaptive), fixed, base, keys, GATHER_CAP, "irradiance_adaptive")
        n_valid = int(is_valid[sb.random_index(len(base), GATHER_CAP + 65, 17)].sum())
        assert stats[-1] == {"rounds": 1, "paths": 16 * n_valid, "rows_valid": n_valid, "rows_converged": 0, "rows_capped": n_valid}, stats[-1]


def test_the_rescale_s_host_route_stages_more_than_its_cap():
    rng = np.random.default_rng(21)
    n = GATHER_CAP + 65
    rows = np.zeros((n, 4), F)
    rows[:, :3] = ((rng.uniform(0, 1, (n, 3)) ** 6 * 1e4) * rng.choice([-1.0, 1.0], (n, 3))).astype(F)
    cnt = rows.view(np.uint32)[:, 3]
    cnt[:] = rng.integers(1, 200, n)
    cnt[::7], cnt[1::7], cnt[3::7] = 0, 1, 64
    rows[n - 3, :3], rows[GATHER_CAP, :3] = (np.inf, -0.0, np.nan), (F(3e38), F(1e-42), F(-1e-45))
    with DeviceScene(_cornell()) as ds:
        for target in (96, (1 << 24) + 3):
            want = words(ar.rescale(rows, target))
            for what, got in (("host", ds.radiance_rescale(rows, target)), ("device", ds.radiance_rescale(to_dev(rows), target))):
                off, where = sb.rows_off(words(got), want)
                assert off == 0, (what, target, off, where)
        mine = rows.copy()
        assert ds.radiance_rescale(mine, 96, in_place=True) is mine and sb.rows_off(words(mine), words(ar.rescale(rows, 96)))[0] == 0


@pytest.mark.parametrize("mode", ["closest", "occluded"])
def test_the_ray_queries_host_route_stages_more_than_its_cap(mode):
    sc = tq._cornell()
    with DeviceScene(sc) as ds:
        base, _, _ = _base_rays(sc, ds)
        fn = ds.closest_hits if mode == "closest" else ds.occluded
        call = _dev_or_host(lambda r, k, kb: fn(r))
        n = QUERY_CAP + 65
        idx = sb.random_index(len(base), n, 17)
        small = words(call(base, None, 0))
        assert sb.distinct_rows(small) >= (100 if mode == "closest" else 3)
        rays = np.ascontiguousarray(base[idx])
        host = words(call(rays, None, 0))
        off, where = sb.rows_off(host, small[to_dev(idx)])
        assert off == 0, (mode, "host route against the small call", off, where)
        off, where = sb.rows_off(host, words(call(to_dev(rays), None, 0)))
        assert off == 0, (mode, "host and device route", off, where)


def test_the_octahedral_gather_s_host_route_stages_more_than_its_cap():
    """res = 16: 256 texels a point, 65 536 points a stage. One sample."""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        base, is_valid, keys = _base_points("cornell", sc, ds)
        base = _with_radius(ds, base, is_valid)
        call = _dev_or_host(lambda p, k, kb: ds.visibility_oct(p, res=16, samples=1, first_sample=FIRST, seed=SEED, keys=k, key_base=kb))
        _host_route_case(call, call, base, keys, DEPTH_CAP, "visibility_oct")


# ---- 8. capped grids with grid-stride loops ----------------------------------------------------------------------------------------------------------------
TONEMAP_THREADS = 4096 * 256
BLOOM_THREADS = 8192 * 256


def _synthetic_sums(w, h, spp, seed):
    """Sums of `spp` samples: mostly in range, some far above; zeros of both signs, negatives, NaN, both infinities and the values that land on the
    8-bit steps - spp x (k / 256)^2 and their float32 neighbours - all over the frame, also behind the grid's first pass."""
    rng = np.random.default_rng(seed)
    a = (rng.random((h, w, 3)) ** 3 * 1.5 * spp).astype(F)
    flat = a.reshape(-1)
    steps = (spp * (np.arange(257) / 256.0) ** 2).astype(F)
    special = np.concatenate([[0.0, -0.0, -1.0, -1e-30, np.nan, np.inf, -np.inf, 1e30], steps, np.nextafter(steps, F(np.inf)), np.nextafter(steps, F(-np.inf))]).astype(F)
    at = rng.permutation(flat.size)[:200 * len(special)]
    flat[at] = np.tile(special, 200)
    assert (at >= TONEMAP_THREADS).sum() > 5 * len(special)
    return a


def test_the_tone_maps_reach_every_float_of_a_frame_larger_than_their_grid():
    import torch
    w, h = 640, 600
    assert w * h * 3 > TONEMAP_THREADS
    with DeviceScene(scenes.cornell_box(RenderConfig(w, h, 64))) as ds:
        sums = _synthetic_sums(w, h, 7, 5)
        img = torch.from_numpy(sums).cuda().contiguous()
        got = ds.tonemap_rgb8(img.data_ptr(), 7)
        assert (got == im.sums_to_rgb8(sums, 7)).all(), int((got != im.sums_to_rgb8(sums, 7)).sum())
        for thr in (0.2, 0.1, 0.05, 0.02):
            _, counts = ta._adaptive(ds, 16, 32, 64, thr)
            if len(np.unique(counts)) >= 2:
                break
        assert len(np.unique(counts)) >= 2, np.unique(counts)
        per_pixel = ta._per_pixel(counts, w, h).astype(np.float64)[..., None]
        sums = (_synthetic_sums(w, h, 1, 6) * per_pixel).astype(F)
        img = torch.from_numpy(sums).cuda().contiguous()
        got = ds.tonemap_rgb8_adaptive(img.data_ptr())
        want = im.sums_to_rgb8(sums, per_pixel)
        assert (got == want).all(), int((got != want).sum())
        assert len(np.unique(want)) == 256


@pytest.mark.parametrize("balanced", [0, 1], ids=["b_mod_n", "balanced_table"])
def test_unpermute_reaches_every_pixel_of_a_frame_larger_than_its_grid(balanced):
    """tests/test_gpu_parity.py's partition check at 1100 x 960, two ranks: every rank's tiles, gathered and un-permuted, are the single-rank frame."""
    import torch
    sc = scenes.cornell_box(RenderConfig(1100, 960, 2))
    assert sc.width * sc.height > TONEMAP_THREADS
    world = 2
    with DeviceScene(sc) as ds:
        ds.render(0, 2, SEED)
        whole = ds.read()
        assert len(np.unique(whole[..., 1])) > 10000
        ds.set_option(_abi.OPT_BALANCED_PARTITION, balanced)
        ds.set_partition(0, world)
        n = ds.accum_floats()
        gathered = torch.zeros(world * n, dtype=torch.float32, device="cuda")
        for r in range(world):
            ds.set_partition(r, world)
            ds.bind_accum(gathered.data_ptr() + r * n * 4, n)
            ds.render(0, 2, SEED)
            ds.sync()
        ds.set_partition(0, world)
        image = torch.empty(sc.height * sc.width * 3, dtype=torch.float32, device="cuda")
        ds.unpermute(gathered.data_ptr(), world, image.data_ptr())
        ds.sync()
        torch.cuda.synchronize()
        out = image.cpu().numpy().reshape(sc.height, sc.width, 3)
    assert (out.view(np.uint32) == whole.view(np.uint32)).all(), int((out != whole).any(axis=-1).sum())


def test_bloom_reaches_every_pixel_of_a_frame_larger_than_its_grid():
    """kernel_size_fraction = 0: a blur of one tap, so the bright pass and the finish - the two kernels of the capped grid - are all there is."""
    import torch
    w, h, spp, thr, maxi = 1920, 1100, 3, 1.5, 6.0
    assert w * h > BLOOM_THREADS
    rng = np.random.default_rng(8)
    p = (rng.random((h, w, 3)) ** 6 * 40.0 * spp).astype(F)  # mostly dark, some pixels above the threshold, some above the maximum
    p[rng.random((h, w)) < 0.01] = 0.0
    want64 = opost.bloom_intermediate(p.astype(np.float64), spp, 0.0, thr, maxi)
    length = np.sqrt((p.astype(np.float64) ** 2).sum(axis=-1)).reshape(-1)[BLOOM_THREADS:]
    assert (length < thr * spp).any() and ((length >= thr * spp) & (length <= maxi * spp)).any() and (length > maxi * spp).any()
    with DeviceScene(scenes.cornell_box(RenderConfig(w, h, 1))) as ds:
        img = torch.from_numpy(p).cuda().contiguous()
        rgb = ds.bloom_rgb8(img.data_ptr(), spp, 0.0, thr, maxi)
        assert (img.cpu().numpy() == p).all()
        ds.bloom(img.data_ptr(), spp, 0.0, thr, maxi)
        ds.sync()
        torch.cuda.synchronize()
        inter = img.cpu().numpy()
    assert (rgb == opost.to_rgb8(want64, spp)).all()
    assert (inter == want64.astype(F)).all()


# ---- 9. what the audit of the remaining kernels found (profiles/size_boundaries.txt) ---------------------------------------------------------------------
def test_the_lightmap_claim_lists_are_longer_than_the_persistent_grids():
    """sol_lightmap_points hands boxes of more than 16 texels to a persistent grid of n_cu x 8 workgroups, a wave per list entry, and the tiles of a
    box of more than 64 tiles to every wave of that grid: more entries than waves, so a wave takes a second entry, and one triangle of more tiles
    than waves, so a wave takes a second tile of it. Against the numpy restatement on both routes; the whole-atlas triangle is the last one, so it
    owns only what the others leave."""
    import lightmap_ref as lr
    from solstrale_amd import lightmap_texels_to_numpy
    from test_gpu_lightmap import assert_words_equal, tri
    W = H = 1024
    n_waves = sb.n_cu() * 8 * 4
    cells = int(np.ceil(np.sqrt(n_waves))) + 3
    rng = np.random.default_rng(12)
    y, x = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    origin = np.stack([x, y], axis=-1).reshape(-1, 1, 2)
    corners = np.array([[0.05, 0.05], [0.9, 0.1], [0.15, 0.9]]) + rng.uniform(-0.04, 0.04, (cells * cells, 3, 2))
    medium = ((origin + corners) / cells).astype(F)
    T = np.concatenate([medium, tri((-0.5, -0.5), (2.5, -0.5), (-0.5, 2.5))])
    box = (medium.max(axis=1) - medium.min(axis=1)) * W
    assert len(medium) > n_waves and (np.floor(box).min(axis=1) ** 2 > 16).all() and (np.ceil(box / 8 + 1).prod(axis=1) <= 64).all()  # list 0, and they stay there
    assert (W // 8) * (H // 8) > n_waves  # the tiles of the last triangle, on list 1
    V = lr.lift(T)
    V[..., 1] = rng.uniform(-1, 1, V.shape[:2]).astype(F)
    ref_p, ref_t = lr.lightmap_points(V, T, W, H)
    owners = np.unique(ref_t["triangle"])
    assert len(owners) == len(T) and (ref_t["triangle"] == len(T) - 1).mean() > 0.3
    with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:
        p, t = ds.lightmap_points(to_dev(V), to_dev(T), W, H)
        assert_words_equal(p.cpu().numpy(), ref_p, "device, points")
        assert_words_equal(lightmap_texels_to_numpy(t), ref_t, "device, texels")
        p, t = ds.lightmap_points(V, T, W, H)
        assert_words_equal(p, ref_p, "host, points")
        assert_words_equal(t, ref_t, "host, texels")


def test_the_denoiser_reaches_every_pixel_of_a_frame_larger_than_its_grid():
    """sol_denoise's prepare and finish kernels run a grid capped at 4096 x 256 threads over the pixels. One a-trous pass reads two pixels to each
    side, taps outside the image dropped, so a crop of the frame, denoised on a handle of the crop's size, answers the frame's own words at every
    pixel whose taps lie inside both or outside both: at crops in the first corner, in the last - behind the grid's first pass - and in between."""
    import torch
    from test_gpu_denoise import _inputs
    w, h, cw, ch = 1100, 960, 96, 40
    assert w * h > TONEMAP_THREADS and (h - ch) * w < TONEMAP_THREADS
    S, n, A, N, m = _inputs(w, h, 77)

    def run(ds, planes):
        img, alb, nrm = (torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes)
        torch.cuda.synchronize()
        ds.denoise(img.data_ptr(), n, alb.data_ptr(), nrm.data_ptr(), m, iterations=1)
        ds.sync()
        return img.cpu().numpy()

    with DeviceScene(scenes.cornell_box(RenderConfig(w, h, 1))) as ds:
        big = run(ds, (S, A, N))
    assert np.isfinite(big).all() and (big != S).mean() > 0.25  # (the pass is not the identity: a pixel's answer depends on its neighbours)
    with DeviceScene(scenes.cornell_box(RenderConfig(cw, ch, 1))) as ds:
        for x0, y0 in ((0, 0), (w - cw, h - ch), (TONEMAP_THREADS % w - cw // 2, h - ch), (200, 400)):
            small = run(ds, [p[y0:y0 + ch, x0:x0 + cw] for p in (S, A, N)])
            xa, xb, ya, yb = 0 if x0 == 0 else 2, cw if x0 + cw == w else cw - 2, 0 if y0 == 0 else 2, ch if y0 + ch == h else ch - 2
            got, want = np.ascontiguousarray(small[ya:yb, xa:xb]), np.ascontiguousarray(big[y0 + ya:y0 + yb, x0 + xa:x0 + xb])
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), ((x0, y0), int((got != want).any(axis=-1).sum()))
