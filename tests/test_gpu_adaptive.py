"""Adaptive sampling (EXTENSION): sol_adaptive_begin / _round / _counts, sol_tonemap_rgb8_adaptive, sol_adaptive_rescale and
ray_trace with RenderConfig(adaptive=...). The contract: every pixel of a block that received n_b samples equals, bit for bit, a fixed
render of n_b samples; the count map follows the stop rule restated in numpy below."""
import numpy as np
import pytest

import orc
import parity_util as pu
from solstrale_amd import (AdaptiveSampling, BloomPostProcessor, DeviceError, DeviceScene, HostError, RenderConfig, _abi,
                           background_blocks, scenes)

pytestmark = pytest.mark.gpu
SEED = pu.SEED


def _fixed(ds, n, first=0):
    ds.clear()
    ds.render(first, n, SEED)
    return ds.read()


def _adaptive(ds, rnd, mn, mx, thr):
    ds.adaptive_begin(rnd, mn, mx, thr)
    ds.adaptive_run(SEED)
    return ds.read(), ds.adaptive_counts()


def _per_pixel(counts, w, h):
    return np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)[:h, :w]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_matches_fixed(ds, img, counts):
    pc = _per_pixel(counts, ds.width, ds.height)
    for n in np.unique(counts):
        want = _fixed(ds, int(n))
        m = pc == n
        assert (_bits(img[m]) == _bits(want[m])).all(), f"pixels with {n} samples differ from a fixed render of {n}"


def _restate(round_sums, rnd, mn, mx, thr, w, h):
    """numpy restatement of the stop rule: fp32, the kernel's order of operations. Returns (counts, near) where `near`
    marks blocks with a pixel within 1e-3 relative of the threshold at a round that was evaluated."""
    f = np.float32
    bx, by = (w + 7) // 8, (h + 7) // 8
    counts = np.zeros((by, bx), np.uint32)
    active = np.ones((by, bx), bool)
    near = np.zeros((by, bx), bool)
    mean = np.zeros((h, w), f)
    m2 = np.zeros((h, w), f)
    done = 0
    pad = np.zeros((by * 8, bx * 8), bool)
    for k, (rs, n) in enumerate(round_sums, start=1):
        if not active.any():
            break
        act_px = _per_pixel(active, w, h)
        m = (rs / f(n)).astype(f)
        y = (f(0.2126) * m[..., 0] + f(0.7152) * m[..., 1]) + f(0.0722) * m[..., 2]
        kf = f(k)
        d = (y - mean).astype(f)
        mean_n = (mean + d / kf).astype(f)
        m2_n = (m2 + d * (y - mean_n)).astype(f)
        mean = np.where(act_px, mean_n, mean)
        m2 = np.where(act_px, m2_n, m2)
        done += n
        conv = np.zeros((h, w), bool)
        if thr > 0 and k >= 2 and done >= mn:
            with np.errstate(invalid="ignore", divide="ignore"):
                se = np.sqrt((m2 / (kf * (kf - f(1)))).astype(f))
                lim = (f(thr) * np.maximum(mean, f(1.0 / 256.0))).astype(f)
            conv = se <= lim
            close = np.abs(se.astype(np.float64) - lim) <= 1e-3 * lim
            pad[:] = False
            pad[:h, :w] = close
            near |= active & pad.reshape(by, 8, bx, 8).any(axis=(1, 3))
        full = np.ones((by * 8, bx * 8), bool)  # padding pixels count as converged
        full[:h, :w] = conv
        stop = full.reshape(by, 8, bx, 8).all(axis=(1, 3)) | (done >= mx)
        counts[active] = done
        active &= ~stop
    return counts, near


def _round_sums(ds, rnd, mx):
    out, first = [], 0
    while first < mx:
        n = min(rnd, mx - first)
        out.append((_fixed(ds, n, first), n))
        first += n
    return out


@pytest.mark.parametrize("make", [lambda: scenes.cornell_box(RenderConfig(96, 80, 80)),
                                  lambda: scenes.create_test_scene(RenderConfig(100, 60, 80)),
                                  lambda: scenes.sponza_like(RenderConfig(120, 72, 80), n_triangles=20000)],
                         ids=["c1", "test_scene_media_lights", "c3_small"])
def test_threshold_zero_reproduces_the_fixed_frame(make):
    sc = make()
    with DeviceScene(sc) as ds:
        img, counts = _adaptive(ds, 32, 64, 80, 0.0)
        assert (counts == 80).all()
        rgb = ds.tonemap_rgb8_adaptive(ds.resolve_image())
        want = _fixed(ds, 80)
        assert (_bits(img) == _bits(want)).all()
        assert (rgb == ds.tonemap_rgb8(ds.resolve_image(), 80)).all()


def _mixed_session(ds):
    for thr in (0.2, 0.1, 0.05, 0.03, 0.02, 0.01):
        img, counts = _adaptive(ds, 16, 32, 128, thr)
        if len(np.unique(counts)) >= 3:
            return thr, img, counts
    raise AssertionError("no threshold gave three distinct counts")


def test_mixed_counts_equal_fixed_renders_and_the_oracle():
    sc = scenes.create_test_scene(RenderConfig(64, 48, 128))
    with DeviceScene(sc) as ds:
        thr, img, counts = _mixed_session(ds)
        assert len(np.unique(counts)) >= 3, counts
        _assert_matches_fixed(ds, img, counts)
    pc = _per_pixel(counts, sc.width, sc.height)
    rect = (16, 8, 48, 40)
    x0, y0, x1, y1 = rect
    ref = np.zeros(img.shape, np.float64)
    for n in np.unique(pc[y0:y1, x0:x1]):
        r, _ = orc.render(sc, 0, int(n), SEED, real=orc.ORC_F32, rect=rect)
        ref[pc == n] = r[pc == n]
    res = pu.compare(img, ref, int(pc[y0:y1, x0:x1].min()), rect)
    assert res["bad_pixels"] == 0, (thr, res)


def test_stop_rule_matches_the_numpy_restatement():
    sc = scenes.statue_like(RenderConfig(163, 91, 96), n_triangles=20000)  # ragged size, background blocks
    rnd, mn, mx = 16, 32, 96
    with DeviceScene(sc) as ds:
        sums = _round_sums(ds, rnd, mx)
        prev = None
        for thr in (0.01, 0.03, 0.1, 0.3):
            _, counts = _adaptive(ds, rnd, mn, mx, thr)
            want, near = _restate(sums, rnd, mn, mx, thr, sc.width, sc.height)
            differ = counts != want
            assert not (differ & ~near).any(), (thr, np.argwhere(differ & ~near)[:8])
            assert counts.min() >= mn and counts.max() <= mx
            assert ((counts % rnd == 0) | (counts == mx)).all()
            if prev is not None:
                assert (counts <= prev).all(), thr  # a larger threshold never gives more samples
            prev = counts
            bg = background_blocks(sc)
            assert bg.any()
            assert (counts[bg] == mn).all(), thr


def test_count_map_is_deterministic_across_options_and_trees():
    sc = scenes.sponza_like(RenderConfig(120, 72, 64), n_triangles=20000)
    args = (16, 32, 64, 0.05)
    with DeviceScene(sc) as ds:
        img0, c0 = _adaptive(ds, *args)
        img1, c1 = _adaptive(ds, *args)
        assert (c0 == c1).all() and (_bits(img0) == _bits(img1)).all()
        assert len(np.unique(c0)) >= 2
        for opt, values in ((_abi.OPT_SWITCH_BELOW, (0, 8, 64)), (_abi.OPT_MAX_BLOCKS_PER_CU, (1, 0)), (_abi.OPT_WORK_ORDER, (0, 1)),
                            (_abi.OPT_FINE_TAIL, (0, 4, 64, -1)), (_abi.OPT_KERNEL, (1, 0)), (_abi.OPT_BACKGROUND_BLOCKS, (0, 1))):
            for v in values:
                ds.set_option(opt, v)
                img, c = _adaptive(ds, *args)
                assert (c == c0).all() and (_bits(img) == _bits(img0)).all(), (opt, v)
    for tree in (_abi.TREE_REF, _abi.TREE_SAH8, _abi.TREE_SAH16, _abi.TREE_SAH64, _abi.TREE_DEVICE, _abi.TREE_HOST_PROBE):
        with DeviceScene(sc, world_tree=tree) as ds:
            img, c = _adaptive(ds, *args)
            assert (c == c0).all() and (_bits(img) == _bits(img0)).all(), tree


@pytest.mark.parametrize("size", [(37, 21), (2, 2), (8, 9)], ids=["ragged", "smallest_image", "one_row_of_padding"])  # (2x2: sol_scene_create refuses 1x1)
def test_edge_sizes(size):
    sc = scenes.cornell_box(RenderConfig(size[0], size[1], 64))
    with DeviceScene(sc) as ds:
        img, counts = _adaptive(ds, 16, 32, 64, 0.05)
        assert counts.shape == ((size[1] + 7) // 8, (size[0] + 7) // 8)
        assert counts.min() >= 32
        _assert_matches_fixed(ds, img, counts)
        want, near = _restate(_round_sums(ds, 16, 64), 16, 32, 64, 0.05, size[0], size[1])
        assert not ((counts != want) & ~near).any()


def test_min_equal_to_max():
    sc = scenes.cornell_box(RenderConfig(40, 24, 48))
    with DeviceScene(sc) as ds:
        img, counts = _adaptive(ds, 16, 48, 48, 10.0)
        assert (counts == 48).all()
        assert (_bits(img) == _bits(_fixed(ds, 48))).all()


def _host_scene(post=None, spp=64, adaptive=AdaptiveSampling(16, 32, 0.05)):
    return scenes.create_test_scene(RenderConfig(64, 48, spp, post_processors=post, adaptive=adaptive))


def test_ray_trace_with_adaptive_sampling():
    sc = _host_scene()
    events, last = sc.ray_trace(strategy="every_sample")
    with DeviceScene(sc) as ds:
        _, counts = _adaptive(ds, 16, 32, 64, 0.05)
        want = ds.tonemap_rgb8_adaptive(ds.resolve_image())
    assert last is not None and (last == want).all()
    prog = [e[0] for e in events]
    assert len(prog) >= 2 and prog[-1] == 1.0
    assert all(b > a for a, b in zip(prog, prog[1:])), prog
    assert all(e[3] for e in events)  # every round an image
    # abort between rounds: no error, fewer events
    seen = []
    events2, _ = sc.ray_trace(strategy="every_sample", abort=lambda: len(seen) >= 1, on_progress=lambda *a: seen.append(a))
    assert 1 <= len(events2) < len(events)
    # one device only
    with pytest.raises(HostError):
        sc.ray_trace(devices=[0, 0])


def test_ray_trace_adaptive_bloom_rescales():
    sc = _host_scene(post=[BloomPostProcessor(0.05)])
    _, last = sc.ray_trace()
    with DeviceScene(sc) as ds:
        _adaptive(ds, 16, 32, 64, 0.05)
        img = ds.resolve_image()
        ds.adaptive_rescale(img)
        want = ds.bloom_rgb8(img, 64, 0.05)
    assert (last == want).all()


def test_ray_trace_adaptive_threshold_zero_is_the_fixed_image():
    fixed = scenes.create_test_scene(RenderConfig(64, 48, 64))
    adapt = _host_scene(adaptive=AdaptiveSampling(16, 32, 0.0))
    assert (adapt.ray_trace()[1] == fixed.ray_trace()[1]).all()


def test_abi_errors_leave_the_scene_usable():
    sc = scenes.cornell_box(RenderConfig(48, 40, 32))
    lib = _abi.load_hip()
    with DeviceScene(sc) as ds:
        want = _fixed(ds, 32)
        n = np.zeros(1, np.uint32)
        rc = lib.sol_adaptive_round(ds.h, SEED, n.ctypes.data_as(_abi.C.POINTER(_abi.C.c_uint32)))  # outside a session
        assert rc == _abi.SOL_EINVAL
        for args in ((8, 32, 32, 0.1), (16, 24, 32, 0.1), (16, 48, 32, 0.1), (16, 32, 32, -0.1), (16, 32, 32, float("nan")), (0, 32, 32, 0.1),
                     (16, 0, 0, 0.1)):
            with pytest.raises(DeviceError) as e:
                ds.adaptive_begin(*args)
            assert e.value.code == _abi.SOL_EINVAL, args
        cfg = _abi.SolAdaptive(size=8, round=16, min_samples=32, max_samples=32, threshold=0.1)
        assert lib.sol_adaptive_begin(ds.h, _abi.C.byref(cfg)) == _abi.SOL_EINVAL
        ds.set_partition(0, 2)
        with pytest.raises(DeviceError) as e:
            ds.adaptive_begin(16, 32, 32, 0.1)
        assert e.value.code == _abi.SOL_EINVAL
        ds.set_partition(0, 1)
        # sol_clear / sol_render / sol_scene_set_partition end a session
        for end in (ds.clear, lambda: ds.render(0, 16, SEED), lambda: ds.set_partition(0, 1)):
            ds.adaptive_begin(16, 32, 32, 0.1)
            ds.adaptive_round(SEED)
            end()
            with pytest.raises(DeviceError) as e:
                ds.adaptive_round(SEED)
            assert e.value.code == _abi.SOL_EINVAL
        assert lib.sol_adaptive_counts(ds.h, n.ctypes.data_as(_abi.C.POINTER(_abi.C.c_uint32)), 0) == _abi.SOL_EINVAL  # (too few entries)
        assert (_bits(_fixed(ds, 32)) == _bits(want)).all()
