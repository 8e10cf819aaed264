"""Visibility gathers on the device (sol_visibility / sol_visibility_dev). The anchor is the identity with the ray queries:
sol_irradiance_rays writes the ray of a sample, sol_query answers it, and the counters and sums are sol_radiance's association of those
answers, restated in numpy float32 and compared word for word. Around it: the float oracle directly, an occluder whose blocked directions and
hit distances the CPU predicts, batch shapes, invalid rows, the splits of a bounded partial buffer, the two routes, refusals and neutrality.
Frames are at most 64 x 64."""
import ctypes as C
import zlib

import numpy as np
import pytest

import irradiance_util as iu
import parity_util as pu
from solstrale_amd import CameraConfig, DeviceError, DeviceScene, RenderConfig, SceneBuilder, _abi, scenes
from test_gpu_irradiance import INVALID_CLASSES, _cornell, _deep_chain, _needles, _occluder_scene, _path_stats, _random_mixed, with_invalid_rows

pytestmark = pytest.mark.gpu
SEED = pu.SEED
INF = np.float32(np.inf)
MODES = ("cosine", "sphere")
RC = RenderConfig(32, 32, 1)
HIT, MISS, INVALID = _abi.SOL_RAY_HIT, _abi.SOL_RAY_MISS, _abi.SOL_RAY_INVALID
VIS = DeviceScene.VISIBILITY_DTYPE


# ---- points and the restatement ----------------------------------------------------------------------------------------------------------
def hit_points(sc, ds, count, seed=1):
    """`count` points where the camera rays of as many samples as it takes hit the scene, the normal being the ray's direction turned round (not
    unit length); tmin = 0.001, tmax = inf. Rows of (position, tmin, normal, tmax)."""
    pos, nrm = [], []
    for s in range(16):
        rays = ds.camera_rays(0, 0, sc.width, sc.height, s, SEED).cpu().numpy().reshape(-1, 8)
        hits = ds.closest_hits(rays)
        ok = np.nonzero(hits["status"] == HIT)[0]
        pos.append(rays[ok, 0:3] + hits["t"][ok, None] * rays[ok, 4:7])
        nrm.append(-rays[ok, 4:7])
        if sum(len(x) for x in pos) >= count:
            break
    pos, nrm = np.concatenate(pos), np.concatenate(nrm)
    assert len(pos) >= count, (len(pos), count)
    ok = np.random.default_rng(seed).permutation(len(pos))[:count]
    p = np.empty((count, 8), dtype=np.float32)
    p[:, 0:3], p[:, 3], p[:, 4:7], p[:, 7] = pos[ok], 0.001, nrm[ok], INF
    return p


def per_sample_answers(ds, points, first, k, **kw):
    """For each sample s in [first, first + k): the rays sol_irradiance_rays writes, and what closest_hits and occluded answer for them.
    Returns (status [k, n] uint32, t [k, n] float32, d [k, n, 3] float32)."""
    status, t, d = [], [], []
    for s in range(first, first + k):
        rays, _ = ds.irradiance_rays(points, s, seed=SEED, **kw)
        hits = ds.hits_to_numpy(ds.closest_hits(rays))
        occ = ds.occluded(rays).cpu().numpy().view(np.uint32)
        assert (occ == hits["status"]).all()  # (HIT exactly where the closest query hits; INVALID where it is)
        status.append(hits["status"].copy())
        t.append(hits["t"].copy())
        d.append(rays.cpu().numpy()[:, 4:7].copy())
    return np.stack(status), np.stack(t), np.stack(d)


def restate(status, t, d, k, distances, is_valid=None):
    """The contract in numpy float32 over the first k samples: chunks of 16 counted from the first sample, a chunk sum 0 + x + x .. in sample
    order, the chunks in order on top of 0; fl(t * t) a product of its own; a hit adds nothing to b and a miss nothing to the t sums; an INVALID
    made ray is counted nowhere; an invalid point answers eight zero words."""
    n = status.shape[1]
    out = np.zeros(n, dtype=VIS)
    b, ts, t2s = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for c0 in range(0, k, 16):
        cb, ct, ct2 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        for j in range(c0, min(c0 + 16, k)):
            hit, miss = status[j] == HIT, status[j] == MISS
            cb = np.where(miss[:, None], cb + d[j], cb)
            if distances:
                tt = np.where(hit, t[j], np.float32(0)).astype(np.float32)
                sq = tt * tt
                assert sq.dtype == np.float32
                ct, ct2 = np.where(hit, ct + tt, ct), np.where(hit, ct2 + sq, ct2)
        b, ts, t2s = b + cb, ts + ct, t2s + ct2
    assert b.dtype == ts.dtype == t2s.dtype == np.float32
    out["bent"], out["t_sum"], out["t2_sum"] = b, ts, t2s
    out["open"], out["hits"], out["samples"] = (status[:k] == MISS).sum(axis=0), (status[:k] == HIT).sum(axis=0), k
    if is_valid is not None:
        out[~is_valid] = np.zeros(1, dtype=VIS)
    return out


def assert_rows_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1))[0]
        raise AssertionError((what, len(bad), len(got), got[bad[:3]], want[bad[:3]]))


# ---- 1. the identity with the ray queries, bit for bit --------------------------------------------------------------------------------------
KS = (1, 15, 16, 17, 48)
FIRST = 5
# (direction mode, keys given?, first_draw): both modes, keys and key_base, first_draw 0 and 3 - each value with each of the others' at least once
COMBOS = (("cosine", False, 0), ("cosine", True, 3), ("sphere", False, 3), ("sphere", True, 0))


@pytest.mark.parametrize("make, env, expect", [(_cornell, {}, {}), (_random_mixed, {}, {}), (_needles, {}, {"strict_triangles": True}),
                                               (_deep_chain, {"SOL_BVH": "ref"}, {"spill": True})],
                         ids=["cornell", "random_mixed", "needles_strict", "deep_chain_spill"])
def test_visibility_is_the_association_over_the_ray_queries_of_its_own_rays(make, env, expect, monkeypatch):
    """Half of the points get a finite tmax: the upper quartile of the distances at which the first sample's rays of those points hit (1 where
    none does), so that about a quarter of the rays that would hit fall outside it. The share of hits among all samples of the case is
    asserted to lie in (5 %, 95 %): neither the hit nor the miss branch goes untested."""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = make()
    d = sc.desc
    assert d.n_mediums == 0 and d.n_spheres + d.n_quads + d.n_triangles <= 2000 and sc.width <= 64 and sc.height <= 64
    rng = np.random.default_rng(11)
    with DeviceScene(sc) as ds:
        info = ds.info()
        if "strict_triangles" in expect:
            assert info["strict_triangles"]
        if "spill" in expect:
            assert info["stack_bound"] > info["lds_stack"], info
        n = 200
        points = hit_points(sc, ds, n)
        probe = np.concatenate([per_sample_answers(ds, points[::2], FIRST, 1, key_base=7, mode=m)[1][0] for m in MODES])
        radius = np.float32(np.quantile(probe[np.isfinite(probe)], 0.75)) if np.isfinite(probe).any() else np.float32(1.0)
        points[::2, 7] = radius
        keys = np.stack([rng.integers(0, 2 ** 32, n), np.zeros(n)], axis=1).astype(np.uint32)
        dev_points = torch.from_numpy(points).cuda()
        n_hits = n_all = 0
        for mode, with_keys, first_draw in COMBOS:
            keys[:, 1] = first_draw
            dev_keys = torch.from_numpy(keys.view(np.int32)).cuda() if with_keys else None
            kw = dict(keys=dev_keys, key_base=7, first_draw=0 if with_keys else first_draw, mode=mode)  # (with keys the configuration's first_draw is not read)
            status, t, dirs = per_sample_answers(ds, dev_points, FIRST, max(KS), **kw)
            assert (status != INVALID).all()
            n_hits, n_all = n_hits + int((status == HIT).sum()), n_all + status.size
            for k in KS:
                for distances in (True, False):
                    got = ds.visibility_to_numpy(ds.visibility(dev_points, samples=k, first_sample=FIRST, seed=SEED, distances=distances, **kw))
                    want = restate(status, t, dirs, k, distances)
                    assert_rows_equal(got, want, (mode, with_keys, first_draw, k, distances))
                    assert (got["hits"] + got["open"] == k).all() and (got["samples"] == k).all()
                    if not distances:
                        assert (got["t_sum"].view(np.uint32) == 0).all() and (got["t2_sum"].view(np.uint32) == 0).all()  # +0
        share = n_hits / n_all
        print(f"hits: {n_hits} of {n_all} samples ({100 * share:.1f} %), finite radius {radius:.4f}")
        assert 0.05 < share < 0.95, share


# ---- 2. the float oracle directly ------------------------------------------------------------------------------------------------------------
def test_counters_and_distance_sums_equal_the_float_oracle_s():
    """64 points x 16 samples on the random mixed scene, tmin = 0.001 and tmax = inf (the oracle's interval): status and t of every ray
    sol_irradiance_rays writes from orc_closest_hit in the float instantiation, as tests/test_gpu_queries.py's oracle_hits takes them."""
    from test_gpu_queries import oracle_hits
    sc = _random_mixed()
    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, 64)
        for mode in MODES:
            status, t, dirs = [], [], []
            for s in range(16):
                rays = ds.irradiance_rays(points, s, seed=SEED, key_base=3, mode=mode)[0].cpu().numpy()
                st, tt, _ = oracle_hits(sc, rays)
                status.append(st), t.append(tt), dirs.append(rays[:, 4:7].copy())
            status, t, dirs = np.stack(status), np.stack(t), np.stack(dirs)
            assert 0 < (status == HIT).sum() < status.size
            got = ds.visibility(points, samples=16, seed=SEED, key_base=3, mode=mode, distances=True)
            assert_rows_equal(got, restate(status, t, dirs, 16, True), mode)


# ---- 3. the occluder, predicted on the CPU ---------------------------------------------------------------------------------------------------
def test_the_occluder_blocks_the_directions_and_at_the_distances_the_cpu_predicts():
    """tests/test_gpu_irradiance.py's scene: a black sphere of radius 1.2 at distance 2 along the normal, background (1, 1, 1); 64 points x 1024
    cosine samples. (tests/test_visibility_abi.py checks the conditions on the CPU: at most 0.5 % borderline, near hits in [0.8, 1.6].)"""
    sc = _occluder_scene()
    n, samples = iu.OCC_POINTS, iu.OCC_SAMPLES
    points = np.zeros((n, 8), dtype=np.float32)
    points[:, 4:7], points[:, 7] = iu.OCC_NORMAL, INF
    blocked, borderline = iu.occluder_prediction()
    sure_free, n_border = (~blocked & ~borderline).sum(axis=1), borderline.sum(axis=1)
    w = iu.onb(iu.OCC_NORMAL)[2]
    kw = dict(samples=samples, seed=iu.OCC_SEED, key_base=iu.OCC_KEY_BASE, mode="cosine")
    with DeviceScene(sc) as ds:
        vis = ds.visibility(points, **kw)
        assert (vis["samples"] == samples).all() and (vis["hits"] + vis["open"] == samples).all()
        free = vis["open"].astype(np.int64)
        off = int(((free < sure_free) | (free > sure_free + n_border)).sum())
        print(f"open {int(free.sum())} of {n * samples}; predicted {int(sure_free.sum())} + up to {int(n_border.sum())} borderline; points off: {off}")
        assert off == 0, (free, sure_free, n_border)
        assert (free[n_border == 0] == sure_free[n_border == 0]).all()
        # another kernel and another schedule counting the same directions
        rgb, cnt = ds.irradiance(points, **kw)
        assert (cnt == samples).all() and (rgb[:, 0] == free.astype(np.float32)).all(), (rgb[:, 0], free)
        # the bent normal
        bent = vis["bent"].astype(np.float64)
        length = np.sqrt((bent * bent).sum(axis=1))
        assert ((bent * w).sum(axis=1) > 0).all() and (length <= free * (1 + 1e-6)).all()
        # an occlusion radius short of the sphere (D - R = 0.8): everything is open
        near = points.copy()
        near[:, 7] = 0.5
        for distances in (False, True):
            v = ds.visibility(near, distances=distances, **kw)
            assert (v["open"] == samples).all() and (v["hits"] == 0).all() and (v["t_sum"] == 0).all() and (v["t2_sum"] == 0).all()
        # the hit distances
        vd = ds.visibility(points, distances=True, **kw)
        assert (vd["open"] == vis["open"]).all() and (vd["hits"] == vis["hits"]).all() and vd["bent"].tobytes() == vis["bent"].tobytes() and (vd["hits"] > 0).all()
        mean_t = vd["t_sum"].astype(np.float64) / vd["hits"]
        mean_t2 = vd["t2_sum"].astype(np.float64) / vd["hits"]
        print(f"mean hit distance per point in [{mean_t.min():.4f}, {mean_t.max():.4f}]")
        assert (mean_t >= 0.79).all() and (mean_t <= 1.61).all()
        assert (mean_t2 >= 0.79 ** 2).all() and (mean_t2 <= 1.61 ** 2).all() and (mean_t2 >= mean_t ** 2 * (1 - 1e-4)).all()


# ---- 4. batch shape and order ---------------------------------------------------------------------------------------------------------------
def test_batch_shape_order_and_keys_do_not_change_a_point_s_answer():
    sc = scenes.cornell_box(RenderConfig(64, 64, 1))
    rng = np.random.default_rng(9)
    big = 4097
    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, big)
        points[::3, 7] = 200.0  # (the box is 555 wide)
        perm = rng.permutation(big)
        for mode, samples, distances in (("cosine", 3, True), ("sphere", 17, True), ("cosine", 33, False)):
            kw = dict(samples=samples, first_sample=2, seed=SEED, mode=mode, distances=distances)
            whole = ds.visibility(points, key_base=40, first_draw=2, **kw)
            assert (whole["samples"] == samples).all() and 0 < whole["hits"].sum() < samples * big and len({r.tobytes() for r in whole}) > big // 2
            # keys that say what key_base and first_draw said: the same answers
            keys = np.stack([40 + np.arange(big), np.full(big, 2)], axis=1).astype(np.uint32)
            assert_rows_equal(ds.visibility(points, keys=keys, key_base=9, first_draw=5, **kw), whole, (mode, "keys"))
            for n in (1, 63, 64, 65, 257, 4097):
                assert_rows_equal(ds.visibility(points[:n], keys=keys[:n], **kw), whole[:n], (mode, samples, n))
                assert_rows_equal(ds.visibility(points[:n], key_base=40, first_draw=2, **kw), whole[:n], (mode, samples, n, "key_base"))
            assert_rows_equal(ds.visibility(points[perm], keys=keys[perm], **kw), whole[perm], (mode, "permutation"))
        with pytest.raises(ValueError):
            ds.visibility(points[:, :7])
        with pytest.raises(ValueError):
            ds.visibility(points, mode="ambient")


# ---- 5. invalid input -----------------------------------------------------------------------------------------------------------------------
def test_invalid_rows_answer_zero_words_and_leave_their_neighbours_alone():
    sc = _cornell()
    rng = np.random.default_rng(5)
    with DeviceScene(sc) as ds:
        clean = hit_points(sc, ds, 150)
        rows, is_valid = with_invalid_rows(clean)
        assert len(rows) == 150 + len(INVALID_CLASSES) and (~is_valid).sum() == len(INVALID_CLASSES)
        keys = np.stack([rng.integers(0, 2 ** 32, len(rows)), rng.integers(0, 8, len(rows))], axis=1).astype(np.uint32)
        for mode in MODES:
            for samples in (16, 48):  # the kernel's own store; the resolve kernel
                for distances in (False, True):
                    kw = dict(samples=samples, first_sample=1, seed=SEED, mode=mode, distances=distances)
                    got = ds.visibility(rows, keys=keys, **kw)
                    assert got[~is_valid].tobytes() == bytes(32 * len(INVALID_CLASSES)), (mode, samples)
                    assert (got["samples"][is_valid] == samples).all() and (got["hits"][is_valid] + got["open"][is_valid] == samples).all()
                    assert_rows_equal(got[is_valid], ds.visibility(rows[is_valid], keys=keys[is_valid], **kw), (mode, samples, distances))


def test_a_normal_whose_squared_length_underflows_is_counted_nowhere_and_the_call_returns():
    """(1e-30, 0, 0): the row is valid, its squared length is not a normal fp32 number - the condition sol_irradiance states is broken. The
    cosine rays made about it are what sol_irradiance_rays writes, INVALID where sol_query says so: counted in neither counter."""
    sc = _cornell()
    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, 70)
        points[33, 4:7] = [1e-30, 0.0, 0.0]
        for mode in MODES:
            status, t, dirs = per_sample_answers(ds, points, 2, 48, key_base=1, mode=mode)
            if mode == "cosine":
                assert (status[:, 33] == INVALID).all() and (np.delete(status, 33, axis=1) != INVALID).all()
            else:
                assert (status != INVALID).all()  # (the normal only counts towards validity)
            for samples in (16, 48):
                got = ds.visibility(points, samples=samples, first_sample=2, seed=SEED, key_base=1, mode=mode, distances=True)
                assert_rows_equal(got, restate(status, t, dirs, samples, True), (mode, samples))
                if mode == "cosine":
                    assert got["hits"][33] == 0 and got["open"][33] == 0 and got["samples"][33] == samples


# ---- 6. the splits --------------------------------------------------------------------------------------------------------------------------
def test_a_bounded_partial_buffer_gives_the_default_bound_s_bits(monkeypatch):
    """SOL_RADIANCE_ROWS = 128 is 64 visibility rows: 300 points x 80 samples (five chunks) run as five slices of 64 points, each in five
    windows of one chunk carried on by the resolve kernel. SOL_RADIANCE_ROWS = 256 is 128 rows: 40 samples (three chunks, the last one short)
    run in slices of 64 points, each in a window of two chunks and one of the short chunk alone."""
    sc = _cornell()
    calls = [dict(mode="cosine", distances=True), dict(mode="sphere", distances=False)]
    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, 300)
        points[::2, 7] = 150.0
        want = [ds.visibility(points, samples=80, first_sample=3, seed=SEED, key_base=40, **kw) for kw in calls]
        want40 = [ds.visibility(points, samples=40, first_sample=3, seed=SEED, key_base=40, **kw) for kw in calls]
        assert 0 < want[0]["hits"].sum() < 80 * 300 and (want[0]["t_sum"] > 0).any()
        assert 0 < want40[0]["hits"].sum() < 40 * 300 and (want40[0]["t_sum"] > 0).any()
    monkeypatch.setenv("SOL_RADIANCE_ROWS", "128")
    with DeviceScene(sc) as ds:
        for kw, w in zip(calls, want):
            assert_rows_equal(ds.visibility(points, samples=80, first_sample=3, seed=SEED, key_base=40, **kw), w, kw)
    monkeypatch.setenv("SOL_RADIANCE_ROWS", "256")
    with DeviceScene(sc) as ds:
        for kw, w in zip(calls, want40):
            assert_rows_equal(ds.visibility(points, samples=40, first_sample=3, seed=SEED, key_base=40, **kw), w, (40, kw))


# ---- 7. routes ------------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_host_arrays_and_another_stream_give_the_same_bytes():
    import torch
    sc = _cornell()
    rng = np.random.default_rng(3)
    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, 257)
        points[::2, 7] = 150.0
        keys = np.stack([rng.integers(0, 2 ** 32, 257), 2 * rng.integers(0, 8, 257)], axis=1).astype(np.uint32)
        dev_points, dev_keys = torch.from_numpy(points).cuda(), torch.from_numpy(keys.view(np.int32)).cuda()
        stream = torch.cuda.Stream()
        for samples in (7, 40):
            for with_keys in (True, False):
                kw = dict(samples=samples, first_sample=3, seed=SEED, key_base=12, distances=True)
                host = ds.visibility(points, keys=keys if with_keys else None, **kw)
                assert host.dtype == VIS and host.shape == (257,)
                dev = ds.visibility(dev_points, keys=dev_keys if with_keys else None, **kw)
                assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (257, 8)
                assert_rows_equal(ds.visibility_to_numpy(dev), host, (samples, with_keys))
                torch.cuda.synchronize()
                ds.set_stream(stream.cuda_stream)
                try:
                    other = ds.visibility(dev_points, keys=dev_keys if with_keys else None, **kw)
                    on_host = ds.visibility(points, keys=keys if with_keys else None, **kw)
                finally:
                    ds.set_stream(0)
                assert_rows_equal(ds.visibility_to_numpy(other), host, (samples, with_keys, "stream"))
                assert_rows_equal(on_host, host, (samples, with_keys, "stream, host route"))


# ---- 8. refusals on a handle -----------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_handle():
    point = np.array([[0., 0., 0., 0.001, 0., 1., 0., np.inf]], dtype=np.float32)
    CFG = _abi.SolIrradianceConfig
    cfg = lambda **kw: CFG(**{**dict(size=C.sizeof(CFG), samples=1), **kw})
    with DeviceScene(scenes.create_test_scene(RC)) as ds:  # (a constant medium)
        for f in (lambda: ds.visibility(point), lambda: ds.visibility(point, mode="sphere", distances=True)):
            with pytest.raises(DeviceError) as e:
                f()
            assert e.value.code == _abi.SOL_EINVAL and "medium" in e.value.msg
        for mode in (_abi.SOL_QUERY_OCCLUDED, _abi.SOL_QUERY_CLOSEST):
            assert ds.lib.sol_visibility(ds.h, mode, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK  # n == 0 succeeds on any scene
            assert ds.lib.sol_visibility_dev(ds.h, mode, None, None, 0, C.byref(cfg()), None) == _abi.SOL_OK
        # the configuration is judged in front of the medium
        out = np.full(8, 7, np.uint32)
        assert ds.lib.sol_visibility(ds.h, 0, point.ctypes.data, None, 1, C.byref(cfg(samples=0)), out.ctypes.data) == _abi.SOL_EINVAL
        assert b"samples" in ds.lib.sol_last_error()
    with DeviceScene(_cornell()) as ds:
        lib, out = ds.lib, np.full(8, 7, np.uint32)
        for fn in (lib.sol_visibility, lib.sol_visibility_dev):
            call = lambda c, mode=_abi.SOL_QUERY_OCCLUDED, pts=point.ctypes.data, n=1, o=out.ctypes.data: fn(ds.h, mode, pts, None, n, C.byref(c), o)
            assert call(cfg(), pts=None) == _abi.SOL_EINVAL and b"null point" in lib.sol_last_error()
            assert call(cfg(), o=None) == _abi.SOL_EINVAL and b"null output" in lib.sol_last_error()
            assert call(cfg(), mode=3) == _abi.SOL_EINVAL and b"unknown mode 3" in lib.sol_last_error()
            assert call(cfg(mode=2)) == _abi.SOL_EINVAL and b"SOL_IRRADIANCE_COSINE" in lib.sol_last_error()
            assert call(cfg(), pts=None, n=0, o=None) == _abi.SOL_OK
        assert (out == 7).all()
        assert lib.sol_visibility(ds.h, _abi.SOL_QUERY_CLOSEST, point.ctypes.data, None, 1, C.byref(cfg(first_sample=0xFFFFFFEF, samples=1)), out.ctypes.data) == _abi.SOL_OK
        assert out[7] == 1 and out[3] + out[6] == 1  # the last sample there is


# ---- 9. neutrality --------------------------------------------------------------------------------------------------------------------------
def test_visibility_gathers_between_renders_change_no_frame_plane_or_statistic():
    sc = scenes.cornell_box(RenderConfig(32, 32, 16))

    def sequence(ds, query):
        ds.clear()
        ds.clear_aux()
        ds.render(0, 8, SEED, counted=True)
        query()
        ds.render(8, 8, SEED)
        query()
        ds.render_aux(0, 4, SEED)
        query()
        frame, (albedo, normal) = ds.read(), ds.read_aux()
        return zlib.crc32(frame.tobytes()), zlib.crc32(albedo.tobytes()), zlib.crc32(normal.tobytes()), ds.stats(), bytes(_path_stats(ds))

    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, 64)

        def query():
            ds.visibility(points, samples=1, seed=SEED)
            ds.visibility(points, samples=40, first_sample=3, seed=SEED, key_base=5, mode="sphere", distances=True)

        want = sequence(ds, lambda: None)
        assert sequence(ds, query) == want and want[3]["rays"] > 0
        # inside an adaptive session with threshold 0 (every block runs to max_samples)
        ds.clear()
        ds.render(0, 32, SEED)
        frame = ds.read()
        ds.adaptive_begin(16, 16, 32, 0.0)
        assert ds.adaptive_round(SEED) > 0
        query()
        assert ds.adaptive_round(SEED) == 0
        assert ds.read().tobytes() == frame.tobytes() and (ds.adaptive_counts() == 32).all()


def test_the_four_gathers_share_scratch_and_keep_their_own_bits():
    sc = _cornell()
    with DeviceScene(sc) as ds:
        points = hit_points(sc, ds, 130)
    kw = dict(samples=40, first_sample=1, seed=SEED, key_base=3)
    rad = lambda ds: ds.radiance(points, **kw)[0].tobytes()  # (the rows as rays: from the surface back along the camera ray)
    irr = lambda ds: ds.irradiance(points, **kw)[0].tobytes()
    sh = lambda ds: ds.irradiance_sh(points, **kw)[0].tobytes()
    vis = lambda ds: ds.visibility(points, distances=True, **kw).tobytes()
    small = lambda ds: ds.visibility(points[:5], samples=17, seed=SEED, mode="sphere").tobytes()
    alone = []
    for f in (rad, irr, sh, vis):
        with DeviceScene(sc) as ds:
            alone.append(f(ds))
    assert len(set(alone)) == 4
    with DeviceScene(sc) as ds:
        assert vis(ds) == alone[3] and rad(ds) == alone[0] and small(ds) and sh(ds) == alone[2] and vis(ds) == alone[3] and irr(ds) == alone[1] and vis(ds) == alone[3]
    with DeviceScene(sc) as ds:
        assert sh(ds) == alone[2] and vis(ds) == alone[3] and irr(ds) == alone[1] and rad(ds) == alone[0]
