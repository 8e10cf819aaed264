"""The render launch (csrc/sol_launch.cpp, sol_render_impl) takes one description of its job - sample range, accumulator, the VIEW of the scene it
renders, the device copy that view goes to - and never edits the handle to describe a launch: the auxiliary planes, the cost probe and the rounds of
adaptive sampling render views of their own. Each case drives one handle through launches of several kinds and compares it, bit for bit, with a fresh
handle that makes only the compared call. Frames are 40 x 24 (5 x 3 blocks, the right column and the bottom row ragged) unless a case says why not."""
import numpy as np
import pytest

import parity_util as pu
from solstrale_amd import DeviceScene, PathTracingShader, RenderConfig, _abi, scenes

pytestmark = pytest.mark.gpu
SEED = pu.SEED


def _frame(ds, spp, seed=SEED):
    ds.clear()
    ds.render(0, spp, seed)
    return ds.read()


def _same(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def test_a_launch_describes_itself_and_leaves_the_handle_alone():
    """Plain renders around auxiliary renders - whose normal pass swaps out the background and the environment pointer - and around an auxiliary
    render that is refused for its work-item count before anything is launched: frames, planes, the sample count of the planes and sol_scene_info
    are those of handles that never saw the other calls.
    The planes are compared bit for bit with a fresh handle that makes the same two auxiliary calls, (0, 20) and (20, 4). A fresh render_aux(0, 24)
    adds the same 24 samples in another order - samples 16 .. 23 are one chunk there, summed by its lane and added to the plane once, and two
    additions to the plane here - so its fp32 sums are not these bits (measured on an MI355X, the library before the launch took a job description and
    after alike: 20 + 4 against 24 differs in 551 of the 2880 albedo floats and 265 of the normal ones, by at most 1.9e-6 on sums of up to 240 and
    24; 16 + 8, split at the chunk, differs in none). Against that handle the bound
    is the one of two summation orders of n = 24 terms in fp32, 2 (n - 1) 2^-24 sum |x_i|: the albedo samples are not negative (sum |x_i| = the
    sum), a normal's components are at most 1 (sum |x_i| <= 24)."""
    sc = scenes.create_test_scene_with_environment(RenderConfig(40, 24, 16))
    assert sc.desc.env_width > 0
    with DeviceScene(sc) as fresh:
        want = _frame(fresh, 20)  # one whole chunk and a ragged one
    with DeviceScene(sc) as fresh:
        fresh.render_aux(0, 20, SEED)
        fresh.render_aux(20, 4, SEED)
        want_albedo, want_normal = fresh.read_aux()
    with DeviceScene(sc) as fresh:
        fresh.render_aux(0, 24, SEED)
        once_albedo, once_normal = fresh.read_aux()
    with DeviceScene(sc) as ds:
        info = ds.info()
        first = _frame(ds, 20)
        ds.render_aux(0, 20, SEED)
        assert ds.lib.sol_render_aux(ds.h, 0, 0xFFFFFFF0, SEED) == _abi.SOL_EINVAL
        assert b"work items" in ds.lib.sol_last_error()
        ds.render_aux(20, 4, SEED)
        again = _frame(ds, 20)
        albedo, normal = ds.read_aux()
        assert ds.resolve_aux()[2] == 24  # (the refused call added nothing)
        assert ds.info() == info
    assert _same(first, want) and _same(again, want)
    assert _same(albedo, want_albedo) and _same(normal, want_normal)
    order = 2 * 23 * 2.0 ** -24
    assert (once_albedo >= 0).all() and (np.abs(albedo.astype(np.float64) - once_albedo) <= order * once_albedo).all()
    assert (np.abs(normal.astype(np.float64) - once_normal) <= order * 24).all()
    assert np.abs(want_albedo).sum() > 0 and np.abs(want_normal).sum() > 0 and not _same(want_albedo, want_normal)


def test_the_view_s_shader_picks_the_estimator_not_the_handle_s():
    """Environment importance sampling and power-weighted light sampling are estimators of the path-tracing shader: the auxiliary planes, views
    under the albedo and the normal shader, are those of a handle with both modes off, and the handle's own frames keep running them."""
    from test_gpu_radiance import assert_render_identity
    sc = pu.env_two_lights(RenderConfig(40, 24, 16, PathTracingShader(8)))
    assert sc.desc.env_width > 0 and sc.desc.n_lights >= 2
    with DeviceScene(sc) as plain:
        plain.render_aux(0, 16, SEED)
        want_albedo, want_normal = plain.read_aux()
        want_plain = _frame(plain, 16)
    with DeviceScene(sc) as fresh:
        fresh.env_sampling("importance")
        fresh.light_sampling("power")
        want = _frame(fresh, 16)
    assert not _same(want, want_plain)  # (the modes are other estimators: other frames)
    with DeviceScene(sc) as ds:
        ds.env_sampling("importance")
        ds.light_sampling("power")
        ds.render_aux(0, 16, SEED)
        albedo, normal = ds.read_aux()
        assert _same(albedo, want_albedo) and _same(normal, want_normal)
        assert _same(_frame(ds, 16), want)
        assert_render_identity(ds, sc, 0)


def test_probe_views_leave_no_table_behind():
    """76 x 60: 80 blocks, above the 64 from which creation runs the cost probe. The probe renders a view whose cost tables are its own; after a
    reprobe (the same camera set again) a counted render counts what a fresh handle's counts, and a plain frame is the fresh handle's."""
    sc = scenes.cornell_box(RenderConfig(76, 60, 16))
    with DeviceScene(sc) as fresh:
        fresh.render(0, 16, SEED, counted=True)
        want_stats = fresh.stats()
    with DeviceScene(sc) as fresh:
        want = _frame(fresh, 16)
    with DeviceScene(sc) as ds:
        ds.set_camera(_abi.SolCamera.from_buffer_copy(sc.desc.camera), reprobe=True)
        ds.render(0, 16, SEED, counted=True)
        stats = ds.stats()
        got = _frame(ds, 16)
    assert stats == want_stats and stats["samples"] >= 76 * 60 * 16
    assert _same(got, want)


def test_an_adaptive_round_is_the_job_it_says_it_is():
    """Threshold 0: every block runs to max_samples, the adaptive frame is the plain 48-spp frame (tests/test_gpu_adaptive.py) - here after an
    auxiliary render on the same handle, so that the rounds' views start from a scene record that an earlier launch must not have disturbed."""
    sc = scenes.cornell_box(RenderConfig(40, 24, 16))
    with DeviceScene(sc) as fresh:
        want = _frame(fresh, 48)
    with DeviceScene(sc) as ds:
        ds.render_aux(0, 16, SEED)
        ds.adaptive_begin(16, 16, 48, 0.0)
        ds.adaptive_run(SEED)
        adaptive = ds.read()
        counts = ds.adaptive_counts()
        plain = _frame(ds, 48)
    assert (counts == 48).all()
    assert _same(adaptive, want) and _same(plain, want)
