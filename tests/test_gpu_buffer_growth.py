"""The growth orders of a handle's device buffers that random call sequences reach only by luck: every scratch buffer and table of a handle is
a DevBuf (csrc/sol_scene.h) that is freed and allocated again when a call needs more than it holds. Each case drives one long-lived handle through
such an order and compares it bit for bit with a fresh handle that made only the last call: a buffer that grew must hold nothing of its past, and
one that did not must still be large enough.
The scratch of the queries, gathers, lightmap and volume calls, shared between families, is under the same rule in tests/test_gpu_scratch_reuse.py."""
import numpy as np
import pytest

import parity_util as pu
from solstrale_amd import CameraConfig, DeviceScene, PathTracingShader, RenderConfig, SceneBuilder, _abi, scenes

pytestmark = pytest.mark.gpu
SEED = pu.SEED


def _small_cornell():
    return scenes.cornell_box(RenderConfig(40, 24, 16))  # 5 x 3 blocks, the right column and the bottom row ragged


def _frame(ds, spp, seed=SEED):
    ds.clear()
    ds.render(0, spp, seed)
    return ds.read()


def _same(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _own_pixels(frame):
    """(h, w) bool: the pixels of the 8x8 blocks in which the frame of one rank holds anything but zeros."""
    h, w = frame.shape[:2]
    by, bx = (h + 7) // 8, (w + 7) // 8
    padded = np.zeros((by * 8, bx * 8), dtype=bool)
    padded[:h, :w] = (frame != 0).any(axis=2)
    blocks = padded.reshape(by, 8, bx, 8).any(axis=(1, 3))
    return np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:h, :w]


def _same_t(a, b):
    """Two device tensors of 32-bit words, bit for bit."""
    import torch
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def test_render_scratch_grows_after_use_and_is_reused_after_a_clear():
    """16 spp is one chunk, 48 spp three: `partial` grows after it was used, then serves the smaller call again."""
    sc = _small_cornell()
    with DeviceScene(sc) as fresh:
        want16 = _frame(fresh, 16)
    with DeviceScene(sc) as fresh:
        want48 = _frame(fresh, 48)
    with DeviceScene(sc) as ds:
        first = _frame(ds, 16)
        got48 = _frame(ds, 48)
        got16 = _frame(ds, 16)  # (sol_clear, then 16 spp again)
    assert _same(first, want16) and _same(got48, want48) and _same(got16, want16)
    assert not _same(want16, want48)


@pytest.mark.parametrize("w,h,table", [(40, 24, 0), (76, 60, 1)], ids=["15_blocks", "80_blocks_table"])
def test_partition_tables_follow_a_sequence_of_partitions(w, h, table):
    """SOL_OPT_BALANCED_PARTITION, then (0, 1), (2, 3), (0, 2), (0, 1): the tables of the partition and the work order shrink and grow. Creation
    probes the block costs from 64 blocks on: the 15 blocks of the first case fall back to b % world (no table), the 80 of the second - ragged
    too - are dealt out by the table."""
    sc = scenes.cornell_box(RenderConfig(w, h, 16))
    with DeviceScene(sc) as fresh:
        want = _frame(fresh, 16)
    halves = {}
    with DeviceScene(sc) as ds:
        ds.set_option(_abi.OPT_BALANCED_PARTITION, 1)
        for rank, world in ((0, 1), (2, 3), (0, 2), (0, 1)):
            ds.set_partition(rank, world)
            if world == 2:
                assert ds.info()["partition_table"] == table
            got = _frame(ds, 16)
            if world == 2:
                halves[rank] = got
    assert _same(got, want)
    with DeviceScene(sc) as other:
        other.set_option(_abi.OPT_BALANCED_PARTITION, 1)
        other.set_partition(1, 2)
        halves[1] = _frame(other, 16)
    # a rank's frame holds its own blocks and zeros elsewhere: every block lies in exactly one of the two, and there it is the whole frame's
    mine = [_own_pixels(halves[r]) for r in (0, 1)]
    assert not (mine[0] & mine[1]).any() and mine[0].any() and mine[1].any()
    assert (halves[0] + halves[1] == want).all()
    for r in (0, 1):
        assert _same(halves[r][mine[r]], want[mine[r]]) and not halves[r][~mine[r]].any()


def test_spill_tail_of_a_grown_grid(monkeypatch):
    """A tree deeper than the LDS stack: the spill tail is sized by the grid. SOL_OPT_MAX_BLOCKS_PER_CU = 1, then 0, then longer launches and
    batches: each launch's tail must be that of its own grid, for the render, the queries and the radiance queries (three areas)."""
    import torch
    from test_gpu_queries import _deep_chain
    monkeypatch.setenv("SOL_BVH", "ref")
    sc = _deep_chain()

    def answers(ds, rays):
        return ds.closest_hits(rays), ds.occluded(rays), ds.radiance(rays, samples=16, seed=SEED)

    with DeviceScene(sc) as fresh:
        info = fresh.info()
        assert info["stack_bound"] > info["lds_stack"], info
        want = _frame(fresh, 16)
        rays = fresh.camera_rays(0, 0, 64, 64, 0, SEED).reshape(-1, 8).contiguous()
        want_all = answers(fresh, rays)
    with DeviceScene(sc) as fresh:
        want_64 = answers(fresh, rays[:64].contiguous())
    with DeviceScene(sc) as ds:
        assert ds.info()["stack_bound"] > ds.info()["lds_stack"]
        ds.kernel_timing(True)
        ds.set_option(_abi.OPT_MAX_BLOCKS_PER_CU, 1)
        capped = _frame(ds, 16)
        grid_16 = ds.last_kernel_ms()[1]
        ds.set_option(_abi.OPT_MAX_BLOCKS_PER_CU, 0)
        free = _frame(ds, 16)
        assert _same(capped, want) and _same(free, want)
        # The workgroups of a 16-spp launch over 64 blocks (16, fewer without the background blocks) fit under either cap: its grid does not
        # grow. A launch of enough chunks to fill more than one workgroup per CU does grow when the cap goes: its frame under the cap - a grid
        # and a spill tail of one workgroup per CU - against its frame without.
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        spp_many = 16 * (n_cu // max(grid_16 - 1, 1) + 2)
        ds.set_option(_abi.OPT_MAX_BLOCKS_PER_CU, 1)
        capped = _frame(ds, spp_many)
        grid_capped = ds.last_kernel_ms()[1]
        ds.set_option(_abi.OPT_MAX_BLOCKS_PER_CU, 0)
        free = _frame(ds, spp_many)
        grid_free = ds.last_kernel_ms()[1]
        assert grid_free > grid_capped >= grid_16, (grid_16, grid_capped, grid_free, n_cu, spp_many)
        assert _same(capped, free) and not _same(free, want)
        got_64 = answers(ds, rays[:64].contiguous())   # one workgroup ..
        got_all = answers(ds, rays)                      # .. then sixteen
        for g64, gall, w64, wall in zip(got_64, got_all, want_64, want_all):
            assert _same_t(g64, w64) and _same_t(gall, wall) and _same_t(g64, gall[:64])
        assert int((got_all[1] == _abi.SOL_RAY_HIT).sum()) > 0 and float(got_all[2][:, :3].sum()) > 0
        assert _same(_frame(ds, 16), want)  # (and the render's own area is none of theirs)


def test_host_route_staging_grows_and_is_reused():
    """sol_query with 64, 4096 and 64 rays; sol_radiance with 64 rays x 16 samples, then 256 rays x 48 samples - three chunks, so the partial
    buffer appears after the first use. Every answer is the one a fresh handle gives to that call alone."""
    sc = scenes.cornell_box(RenderConfig(64, 64, 1))
    with DeviceScene(sc) as fresh:
        rays = fresh.camera_rays(0, 0, 64, 64, 0, SEED).reshape(-1, 8).cpu().numpy()
    rays[5, 4:7] = 0.0  # (an invalid ray among them)
    calls = [("closest", 64, 0), ("occluded", 64, 0), ("closest", 4096, 0), ("occluded", 4096, 0), ("closest", 64, 0), ("occluded", 64, 0),
             ("radiance", 64, 16), ("radiance", 256, 48)]

    def call(ds, what, n, samples):
        if what == "radiance":
            rgb, count = ds.radiance(rays[:n], samples=samples, seed=SEED)
            return np.concatenate([rgb.view(np.uint32), count.reshape(-1, 1)], axis=1)
        out = ds.closest_hits(rays[:n]) if what == "closest" else ds.occluded(rays[:n])
        return np.ascontiguousarray(out).view(np.uint32)

    want = []
    for c in calls:
        with DeviceScene(sc) as fresh:
            want.append(call(fresh, *c))
    with DeviceScene(sc) as ds:
        got = [call(ds, *c) for c in calls]
    for c, g, w in zip(calls, got, want):
        assert g.shape == w.shape and (g == w).all(), c
    assert (want[2].reshape(4096, 8)[:, 3] == _abi.SOL_RAY_HIT).sum() > 1000 and want[2].reshape(4096, 8)[5, 3] == _abi.SOL_RAY_INVALID
    assert (want[7][:, 3] == 48).sum() == 255 and want[7][5, 3] == 0


def test_adaptive_session_after_a_plain_life():
    """Render, sol_adaptive_begin, two rounds, sol_clear, sol_adaptive_begin again, to completion: the counts and the image of a fresh handle
    that ran only the last session."""
    sc = _small_cornell()
    session = (16, 32, 128, 0.05)
    with DeviceScene(sc) as fresh:
        fresh.adaptive_begin(*session)
        want_rounds = fresh.adaptive_run(SEED)
        want_counts, want = fresh.adaptive_counts(), fresh.read()
    with DeviceScene(sc) as ds:
        ds.render(0, 48, SEED + 1)
        ds.adaptive_begin(16, 16, 64, 0.5)
        ds.adaptive_round(SEED + 2)
        ds.adaptive_round(SEED + 2)
        ds.clear()
        ds.adaptive_begin(*session)
        rounds = ds.adaptive_run(SEED)
        counts, got = ds.adaptive_counts(), ds.read()
    assert rounds == want_rounds and (counts == want_counts).all() and _same(got, want)
    assert counts.shape == (3, 5) and counts.min() >= 32 and counts.max() <= 128


def test_destroy_after_every_lazily_created_buffer():
    """A handle that has used every buffer it creates on demand - auxiliary planes, bloom, denoise, environment tables, light tree and tables,
    queries, radiance queries, an adaptive session - is destroyed; the next handle renders the frame the first one began with."""
    b = SceneBuilder()  # (an environment map, two lights, no constant medium: every extension accepts the scene)
    b.environment(scenes.procedural_sky(64, 32), 0.8)
    grey = b.Lambertian(b.SolidColor(.5, .45, .4))
    world = [b.Sphere((0., 1., 0.), 1., grey), b.Quad((-6., 0., -6.), (12., 0., 0.), (0., 0., 12.), grey),
             b.Quad((-1., 4., -1.), (2., 0., 0.), (0., 0., 2.), b.DiffuseLight(4., 4., 4.)), b.Sphere((3., 3., 0.), .5, b.DiffuseLight(2., 2., 2.))]
    cam = CameraConfig(40., 0., (0., 2., 7.), (0., 1., 0.), (0., 1., 0.))
    sc = b.finish(b.Bvh(world), cam, (.2, .3, .4), RenderConfig(40, 24, 16, PathTracingShader(8)))
    assert sc.desc.env_width > 0 and sc.desc.n_mediums == 0 and sc.desc.n_lights == 2
    ds = DeviceScene(sc)
    want = _frame(ds, 16)
    rays = ds.camera_rays(0, 0, 40, 24, 0, SEED).reshape(-1, 8).cpu().numpy()
    ds.render_aux(0, 16, SEED)
    albedo, normal, aux_samples = ds.resolve_aux()
    image = ds.resolve_image()
    ds.denoise(image, 16, albedo, normal, aux_samples)
    ds.denoise_rgb8(image, 16, albedo, normal, aux_samples)
    ds.bloom_rgb8(image, 16, 0.1)
    ds.env_sampling("importance")
    ds.light_sampling("power")
    ds.render(16, 48, SEED)
    ds.closest_hits(rays)
    ds.occluded(rays[:64])
    ds.radiance(rays, samples=48, seed=SEED)
    ds.radiance(rays[:64], samples=16, seed=SEED, keys=np.stack([np.arange(64), np.full(64, 2)], axis=1).astype(np.uint32))
    ds.adaptive_begin(16, 32, 64, 0.1)
    ds.adaptive_run(SEED)
    ds.tonemap_rgb8_adaptive(ds.resolve_image())
    ds.set_option(_abi.OPT_BALANCED_PARTITION, 1)
    ds.set_partition(1, 2)
    ds.render(0, 16, SEED)
    ds.close()
    with DeviceScene(sc) as again:
        assert _same(_frame(again, 16), want)
