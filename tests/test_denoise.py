"""The denoiser without a device: its C ABI (configuration checks, the ctypes layout, no CPU fallback), the post-processor
chain of the host (DenoisePostProcessor last only, its parameters checked where the chain is installed) and known answers of the numpy
restatement in tests/denoise_ref.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import parity_util  # noqa: F401  (puts the package on sys.path)
from solstrale_amd import _abi, device_count

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = math.nan
ENTRY_POINTS = ["sol_denoise_check", "sol_resolve_aux", "sol_denoise", "sol_denoise_rgb8"]


def _cfg(**kw):
    c = _abi.denoise_config()
    for k, v in kw.items():
        if k == "reserved":
            c.reserved[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported():
    lib = _abi.load_hip()
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert n in _abi.HIP_SYMBOLS


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_header_is_c99_and_layout_matches(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text("""#include <stddef.h>
#include <stdio.h>
#include "solstrale_hip.h"
int main(void) {
  printf("%u %u %u %u %u %u %u %g %g\\n", (unsigned)sizeof(SolDenoise), (unsigned)offsetof(SolDenoise, size), (unsigned)offsetof(SolDenoise, iterations),
         (unsigned)offsetof(SolDenoise, sigma_color), (unsigned)offsetof(SolDenoise, normal_power), (unsigned)offsetof(SolDenoise, reserved),
         SOL_DENOISE_DEFAULT_ITERATIONS, (double)SOL_DENOISE_DEFAULT_SIGMA_COLOR, (double)SOL_DENOISE_DEFAULT_NORMAL_POWER);
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    S = _abi.SolDenoise
    assert [int(x) for x in got[:6]] == [C.sizeof(S), S.size.offset, S.iterations.offset, S.sigma_color.offset, S.normal_power.offset,
                                         S.reserved.offset]
    assert (int(got[6]), float(got[7]), float(got[8])) == (_abi.DENOISE_DEFAULT_ITERATIONS, _abi.DENOISE_DEFAULT_SIGMA_COLOR,
                                                           _abi.DENOISE_DEFAULT_NORMAL_POWER)


def test_check_accepts_null_and_the_defaults():
    lib = _abi.load_hip()
    assert lib.sol_denoise_check(None) == 0
    assert lib.sol_denoise_check(C.byref(_abi.denoise_config())) == 0
    for kw in (dict(iterations=1), dict(iterations=8), dict(normal_power=0.), dict(sigma_color=1e-6)):
        assert lib.sol_denoise_check(C.byref(_cfg(**kw))) == 0, kw


BAD = [(dict(size=8), b"size"), (dict(size=C.sizeof(_abi.SolDenoise) + 4), b"size"), (dict(iterations=0), b"iterations"),
       (dict(iterations=9), b"iterations"), (dict(sigma_color=0.), b"sigma_color"), (dict(sigma_color=-1.), b"sigma_color"),
       (dict(sigma_color=math.nan), b"sigma_color"), (dict(sigma_color=math.inf), b"sigma_color"), (dict(normal_power=-0.5), b"normal_power"),
       (dict(normal_power=math.nan), b"normal_power"), (dict(normal_power=math.inf), b"normal_power"), (dict(reserved=(0, 1)), b"reserved"),
       (dict(reserved=(1, 7)), b"reserved")]
BAD_IDS = ["size8", "size_big", "iter0", "iter9", "sigma0", "sigma_neg", "sigma_nan", "sigma_inf", "power_neg", "power_nan", "power_inf",
           "reserved0", "reserved1"]


@pytest.mark.parametrize("bad,word", BAD, ids=BAD_IDS)
def test_check_refuses_each_bad_field_with_a_message(bad, word):
    lib = _abi.load_hip()
    assert lib.sol_denoise_check(C.byref(_cfg(**bad))) == _abi.SOL_EINVAL
    msg = lib.sol_last_error()
    assert msg.startswith(b"sol_denoise: ") and word in msg, msg


@pytest.mark.parametrize("bad,word", BAD[:3], ids=BAD_IDS[:3])
def test_the_same_checks_run_before_the_device(bad, word):
    """sol_denoise / sol_denoise_rgb8 refuse a bad configuration before anything else - without a scene, and without a device."""
    lib = _abi.load_hip()
    rgb = (C.c_uint8 * 3)()
    assert lib.sol_denoise(None, None, 1, None, None, 1, C.byref(_cfg(**bad))) == _abi.SOL_EINVAL
    assert word in lib.sol_last_error()
    assert lib.sol_denoise_rgb8(None, None, 1, None, None, 1, C.byref(_cfg(**bad)), rgb) == _abi.SOL_EINVAL
    assert word in lib.sol_last_error()


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_no_cpu_fallback_without_a_gpu():
    lib = _abi.load_hip()
    a, n, m = C.c_void_p(), C.c_void_p(), C.c_uint32()
    rgb = (C.c_uint8 * 3)()
    assert lib.sol_resolve_aux(None, C.byref(a), C.byref(n), C.byref(m)) == _abi.SOL_EDEVICE
    assert lib.sol_denoise(None, None, 1, None, None, 1, None) == _abi.SOL_EDEVICE
    assert lib.sol_denoise(None, None, 1, None, None, 1, C.byref(_abi.denoise_config())) == _abi.SOL_EDEVICE
    assert lib.sol_denoise_rgb8(None, None, 1, None, None, 1, None, rgb) == _abi.SOL_EDEVICE


# ---- host chain -------------------------------------------------------------------------------------------------------------
def _set(kinds, params):
    lib = _abi.load_host()
    b = lib.solh_builder_new()
    try:
        k = (C.c_int * max(1, len(kinds)))(*kinds)
        p = (C.c_double * max(1, len(params)))(*params)
        rc = lib.solh_set_post_processors(b, len(kinds), k, p)
        return rc, lib.solh_last_error().decode()
    finally:
        lib.solh_builder_free(b)


def test_host_chain_takes_the_denoiser_last_only():
    nan = math.nan
    assert _set([2], [nan, nan, nan])[0] == 0
    assert _set([2], [3., 0.5, 16.])[0] == 0
    assert _set([1, 2], [0.1, nan, nan, nan, nan, nan])[0] == 0
    assert _set([0, 1, 2], [0., 0., 0., 0.1, 1., nan, 8., 0.1, 0.])[0] == 0
    for kinds, params in (([2, 0], [nan] * 3 + [0.] * 3), ([2, 1], [nan] * 3 + [0.1, nan, nan]), ([2, 2], [nan] * 6)):
        rc, msg = _set(kinds, params)
        assert rc < 0 and msg == "DenoisePostProcessor can not be used as an intermediate post processor", (kinds, msg)


@pytest.mark.parametrize("params,word", [((0., NAN, NAN), "iterations"), ((9., NAN, NAN), "iterations"), ((2.5, NAN, NAN), "iterations"),
                                         ((NAN, 0., NAN), "sigma_color"), ((NAN, -1., NAN), "sigma_color"), ((NAN, math.inf, NAN), "sigma_color"),
                                         ((NAN, NAN, -1.), "normal_power"), ((NAN, NAN, math.inf), "normal_power")],
                         ids=["iter0", "iter9", "iter_frac", "sigma0", "sigma_neg", "sigma_inf", "power_neg", "power_inf"])
def test_host_chain_refuses_bad_parameters(params, word):
    rc, msg = _set([2], list(params))
    assert rc < 0 and msg.startswith("DenoisePostProcessor: ") and word in msg, msg


def test_python_post_processor_round_trips_through_render_config():
    from solstrale_amd import DenoisePostProcessor, NopPostProcessor, RenderConfig
    import solstrale_amd
    assert solstrale_amd.DenoisePostProcessor is DenoisePostProcessor
    kind, prm = DenoisePostProcessor()
    assert kind == 2 and len(prm) == 3 and all(math.isnan(x) for x in prm)
    rc = RenderConfig(32, 16, 4, post_processors=[NopPostProcessor(), DenoisePostProcessor(3, 0.5, 16)])
    assert rc.post_processors[-1] == (2, (3.0, 0.5, 16.0))
    assert _set([k for k, _ in rc.post_processors], [x for _, p in rc.post_processors for x in p])[0] == 0
    kind, prm = DenoisePostProcessor(sigma_color=0.1)
    assert math.isnan(prm[0]) and prm[1] == 0.1 and math.isnan(prm[2])


# ---- the restatement's known answers ------------------------------------------------------------------------------------------
def _planes(colour, albedo, normal, n=4, m=2):  # (powers of two: the float32 means are exact)
    colour, albedo, normal = (np.asarray(x, dtype=np.float64) for x in (colour, albedo, normal))
    return (colour * n).astype(np.float32), n, (albedo * m).astype(np.float32), (normal * m).astype(np.float32), m


def test_restatement_one_pixel_returns_its_input():
    S, n, A, N, m = _planes([[[0.7, 3.5, 12.]]], [[[0.5, 0.005, 1.1]]], [[[0., 0., 1.]]])
    for it in (1, 5, 8):
        out = dr.denoise(S, n, A, N, m, iterations=it)
        assert np.allclose(out, S.astype(np.float64), rtol=1e-12, atol=0.)


def test_restatement_constant_image_stays_constant():
    h, w = 23, 31
    colour = np.broadcast_to([2.0, 0.25, 7.5], (h, w, 3))
    albedo = np.broadcast_to([0.8, 0.3, 0.6], (h, w, 3))
    normal = np.broadcast_to(np.array([1., 2., 2.]) / 3., (h, w, 3))
    S, n, A, N, m = _planes(colour, albedo, normal)
    want = S.astype(np.float64)
    for it in (1, 3, 8):
        out = dr.denoise(S, n, A, N, m, iterations=it)
        assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max(), it


def test_restatement_opposite_half_planes_never_mix():
    h, w = 20, 24
    rng = np.random.default_rng(3)
    colour = rng.random((h, w, 3)) * 5.
    normal = np.zeros((h, w, 3))
    normal[:, : w // 2, 2] = 1.
    normal[:, w // 2:, 2] = -1.
    S, n, A, N, m = _planes(colour, np.full((h, w, 3), 0.5), normal)
    out = dr.denoise(S, n, A, N, m, iterations=5)
    for half in (np.s_[:, : w // 2], np.s_[:, w // 2:]):
        alone = dr.denoise(S[half], n, A[half], N[half], m, iterations=5)
        assert np.abs(out[half] - alone).max() <= 1e-12 * np.abs(alone).max()
    # and each half really is filtered
    assert np.abs(out - S.astype(np.float64)).max() > 0.1


def test_restatement_miss_among_hits_keeps_its_own_value():
    h, w = 9, 9
    rng = np.random.default_rng(4)
    colour = rng.random((h, w, 3)) * 4.
    normal = np.broadcast_to([0., 1., 0.], (h, w, 3)).copy()
    normal[4, 4] = 0.  # a miss in the middle
    S, n, A, N, m = _planes(colour, np.full((h, w, 3), 0.7), normal)
    out = dr.denoise(S, n, A, N, m, iterations=4)
    assert abs(out[4, 4] - S[4, 4].astype(np.float64)).max() <= 1e-12 * float(S[4, 4].max())
    assert np.abs(out - S.astype(np.float64)).max() > 0.1  # the hits around it are filtered


def test_restatement_albedo_at_or_below_one_percent_is_not_divided():
    S, n, A, N, m = _planes([[[1.0, 1.0, 1.0], [3.0, 3.0, 3.0]]], [[[0.005, 0.5, 0.011], [0.01, 0.25, 0.]]], [[[0., 0., 1.], [0., 0., 1.]]], m=1)
    e, f, g, hit = dr.prepare(S, n, A, N, m)
    assert np.allclose(f, [[[1.0, 0.5, 0.011], [1.0, 0.25, 1.0]]], rtol=1e-7)
    assert np.allclose(e, [[[1.0, 2.0, 1.0 / 0.011], [3.0, 12.0, 3.0]]], rtol=1e-6)
    assert hit.all() and np.allclose(g, [[[0., 0., 1.], [0., 0., 1.]]])


def test_restatement_non_finite_colour_counts_as_zero_and_weights_fall_with_distance():
    S, n, A, N, m = _planes([[[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]], np.full((1, 2, 3), 0.5), [[[0., 0., 1.], [0., 0., 1.]]], n=1, m=1)
    S[0, 1, 0] = np.inf
    S[0, 0, 2] = np.nan
    e, _, _, _ = dr.prepare(S, n, A, N, m)
    assert e[0, 1, 0] == 0. and e[0, 0, 2] == 0. and np.isfinite(e).all()
    # a neighbour in another colour is weighted down; with a wide sigma_color it counts almost fully
    S2, n, A, N, m = _planes([[[0.2, 0.2, 0.2], [20., 20., 20.]]], np.ones((1, 2, 3)), [[[0., 0., 1.], [0., 0., 1.]]], n=1, m=1)
    narrow = dr.denoise(S2, n, A, N, m, iterations=1, sigma_color=0.05)
    wide = dr.denoise(S2, n, A, N, m, iterations=1, sigma_color=100.)
    assert abs(narrow[0, 0, 0] - 0.2) < 1e-6 and wide[0, 0, 0] > 5.


def test_ray_trace_refuses_several_devices_and_adaptive_sampling():
    """Checked before any device is touched: the denoiser renders its guide planes on one device and is not combined with adaptive
    sampling."""
    from solstrale_amd import AdaptiveSampling, DenoisePostProcessor, HostError, RenderConfig, scenes
    sc = scenes.cornell_box(RenderConfig(32, 16, 16, post_processors=[DenoisePostProcessor()]))
    with pytest.raises(HostError, match="^ray_trace: the denoiser renders on one device$"):
        sc.ray_trace(devices=[0, 0])
    sc = scenes.cornell_box(RenderConfig(32, 16, 16, post_processors=[DenoisePostProcessor()], adaptive=AdaptiveSampling(16, 16, 0.05)))
    with pytest.raises(HostError, match="^ray_trace: adaptive sampling and the denoiser cannot be combined$"):
        sc.ray_trace()
