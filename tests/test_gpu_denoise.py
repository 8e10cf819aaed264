"""The denoiser on the device: the kernels against the numpy restatement (tests/denoise_ref.py), the bytes of
sol_denoise_rgb8, determinism, the auxiliary sample count of sol_resolve_aux, the quality it buys on two scenes, and ray_trace with a
DenoisePostProcessor against the explicit DeviceScene sequence.

Quality ratios measured on MI355X (denoised MSE / raw MSE in the display domain, RGB8 of to_rgb_color, against a 4096-spp render of
another seed; profiles/denoise_quality.txt): cornell_box 0.166, create_test_scene 0.515 (0.150 of the unguided a-trous)."""
import os
import sys

import numpy as np
import pytest

import denoise_ref as dr
import parity_util as pu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import post as opost  # noqa: E402  (test infrastructure: the to_rgb_color restatement)


def _inputs(w, h, seed, n=4, m=2):
    """Random HDR colour (means up to 40), albedo in [0, 1.2], unit normals with about 10 % misses; as sums over n / m samples."""
    rng = np.random.default_rng(seed)
    col = rng.random((h, w, 3)) ** 4 * 40.
    alb = rng.random((h, w, 3)) * 1.2
    nrm = rng.normal(size=(h, w, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nrm[rng.random((h, w)) < 0.1] = 0.
    return (col * n).astype(np.float32), n, (alb * m).astype(np.float32), (nrm * m).astype(np.float32), m


def _scene(w, h, spp=1, post_processors=None):
    from solstrale_amd import RenderConfig, scenes
    return scenes.cornell_box(RenderConfig(w, h, spp, post_processors=post_processors))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(2, 2), (7, 5), (129, 67), (640, 360)])
def test_device_matches_the_restatement(w, h):
    """Every element: |dev - ref| <= 1e-4 (1 + |ref|) on the means; sol_denoise_rgb8 = sol_denoise + sol_tonemap_rgb8 byte for byte, and
    two calls give the same bytes. The filter runs on the scene's image size, and sol_scene_create takes 2x2 at the least: the 1x1 known
    answer is the restatement's (tests/test_denoise.py)."""
    import torch
    from solstrale_amd import DeviceScene
    S, n, A, N, m = _inputs(w, h, w * 1000 + h)
    with DeviceScene(_scene(w, h)) as ds:
        src = torch.from_numpy(S).cuda().contiguous()
        alb = torch.from_numpy(A).cuda().contiguous()
        nrm = torch.from_numpy(N).cuda().contiguous()
        torch.cuda.synchronize()
        for it in (1, 5, 8):
            img = src.clone()
            torch.cuda.synchronize()
            rgb = ds.denoise_rgb8(src.data_ptr(), n, alb.data_ptr(), nrm.data_ptr(), m, iterations=it)
            assert (ds.denoise_rgb8(src.data_ptr(), n, alb.data_ptr(), nrm.data_ptr(), m, iterations=it) == rgb).all()
            ds.denoise(img.data_ptr(), n, alb.data_ptr(), nrm.data_ptr(), m, iterations=it)
            ds.sync()
            assert (ds.tonemap_rgb8(img.data_ptr(), n) == rgb).all()
            got = img.cpu().numpy().astype(np.float64) / n
            assert (src.cpu().numpy() == S).all()  # sol_denoise_rgb8 leaves its input alone
            want = dr.denoise(S, n, A, N, m, iterations=it) / n
            excess = np.abs(got - want) - 1e-4 * (1. + np.abs(want))
            assert np.isfinite(got).all() and (excess <= 0).all(), (it, float(excess.max()), int((excess > 0).sum()))


@pytest.mark.gpu
def test_resolve_aux_counts_the_aux_samples():
    from solstrale_amd import DeviceError, DeviceScene, _abi
    with DeviceScene(_scene(40, 24)) as ds:
        with pytest.raises(DeviceError) as e:
            ds.resolve_aux()
        assert e.value.code == _abi.SOL_EINVAL and "sol_render_aux" in e.value.msg
        ds.render_aux(0, 16, pu.SEED)
        ap, np_, m = ds.resolve_aux()
        assert m == 16 and ap and np_ and ap != np_ and ap != ds.resolve_image()
        ds.render_aux(16, 16, pu.SEED)
        assert ds.resolve_aux()[2] == 32
        albedo, normal = ds.read_aux()
        a_ptr, n_ptr, _ = ds.resolve_aux()
        ds.sync()
        for ptr, want in ((a_ptr, albedo), (n_ptr, normal)):  # the resolved planes are the sums sol_read_aux copies out
            assert (_device_plane(ptr, 24, 40) == want).all()
        ds.clear_aux()
        assert ds.resolve_aux()[2] == 0
        ds.set_partition(0, 2)
        with pytest.raises(DeviceError) as e:
            ds.resolve_aux()
        assert e.value.code == _abi.SOL_EINVAL and "rank-local" in e.value.msg


def _device_plane(ptr, h, w):
    """(h, w, 3) float32 of device memory at ptr, copied to the host by torch."""
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": (h, w, 3), "typestr": "<f4", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_View(), device="cuda").cpu().numpy()


def _render_pair(sc, spp, seed, ref_spp, ref_seed):
    """(raw sums, RGB8 of the denoised frame, RGB8 of the reference) for `sc`: spp samples of colour and aux planes with `seed`."""
    from solstrale_amd import DeviceScene
    with DeviceScene(sc) as ds:
        ds.render(0, spp, seed)
        ds.render_aux(0, spp, seed)
        raw = ds.read().astype(np.float64)
        img = ds.resolve_image()
        a, n, m = ds.resolve_aux()
        den = ds.denoise_rgb8(img, spp, a, n, m)
        ds.clear()
        ds.render(0, ref_spp, ref_seed)
        ref = ds.read().astype(np.float64)
    return raw, den, opost.to_rgb8(ref, ref_spp)


def _mse(a, b):
    return float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())


@pytest.mark.gpu
def test_quality_cornell_box():
    """scenes.cornell_box, 128x128, 16 spp against 4096 spp of another seed, display domain: denoised MSE <= 0.5 x raw MSE.
    Measured on MI355X (profiles/denoise_quality.txt): raw MSE 285.8, denoised 47.4, ratio 0.166."""
    from solstrale_amd import RenderConfig, scenes
    spp = 16
    raw, den, ref8 = _render_pair(scenes.cornell_box(RenderConfig(128, 128, spp)), spp, pu.SEED, 4096, pu.SEED + 77)
    raw_mse, den_mse = _mse(opost.to_rgb8(raw, spp), ref8), _mse(den, ref8)
    print(f"denoise quality cornell_box 128x128 16spp: raw MSE {raw_mse:.2f}, denoised MSE {den_mse:.2f}, ratio {den_mse / raw_mse:.3f}")
    assert den_mse <= 0.5 * raw_mse


@pytest.mark.gpu
def test_quality_image_textured_scene():
    """scenes.create_test_scene (image-textured ground, glass, medium), 128x128, 16 spp against 4096 spp of another seed: the guided filter
    beats the raw frame and the same a-trous with every w = 1 and no demodulation (numpy) on display-domain MSE.
    Measured on MI355X (profiles/denoise_quality.txt): raw MSE 1115.6, plain a-trous 3840.5, denoised 574.2 - ratio 0.515 to raw,
    0.150 to plain."""
    from solstrale_amd import RenderConfig, scenes
    spp = 16
    raw, den, ref8 = _render_pair(scenes.create_test_scene(RenderConfig(128, 128, spp)), spp, pu.SEED, 4096, pu.SEED + 77)
    raw_mse, den_mse = _mse(opost.to_rgb8(raw, spp), ref8), _mse(den, ref8)
    plain_mse = _mse(opost.to_rgb8(dr.plain_atrous(raw, spp, dr.DEFAULTS["iterations"]), spp), ref8)
    print(f"denoise quality create_test_scene 128x128 16spp: raw MSE {raw_mse:.2f}, plain a-trous MSE {plain_mse:.2f}, "
          f"denoised MSE {den_mse:.2f}, ratio to raw {den_mse / raw_mse:.3f}, to plain {den_mse / plain_mse:.3f}")
    assert den_mse < raw_mse and den_mse < plain_mse


@pytest.mark.gpu
def test_ray_trace_with_the_denoiser_is_the_explicit_sequence():
    from solstrale_amd import BloomPostProcessor, DenoisePostProcessor, DeviceScene
    spp = 16
    sc = _scene(96, 64, spp, [DenoisePostProcessor()])
    events, img = sc.ray_trace()
    assert img is not None and len(events) == spp
    with DeviceScene(sc) as ds:
        ds.render(0, spp, sc.render_config.seed)
        ds.render_aux(0, spp, sc.render_config.seed)
        p = ds.resolve_image()
        a, n, m = ds.resolve_aux()
        assert m == spp
        want = ds.denoise_rgb8(p, spp, a, n, m)
        plain = ds.tonemap_rgb8(ds.resolve_image(), spp)
        ds.bloom(p, spp, 0.1)
        bloomed = ds.denoise_rgb8(p, spp, a, n, m)
    assert (img == want).all()
    assert (img != plain).any()
    _, img2 = _scene(96, 64, spp, [BloomPostProcessor(0.1), DenoisePostProcessor()]).ray_trace()
    assert (img2 == bloomed).all()
    _, img3 = _scene(96, 64, spp, [DenoisePostProcessor(2, 0.5, 8)]).ray_trace()
    assert img3.shape == (64, 96, 3) and (img3 != img).any()
