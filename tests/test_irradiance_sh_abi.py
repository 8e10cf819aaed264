"""SH irradiance queries (sol_irradiance_sh / sol_irradiance_sh_dev), the part that needs no GPU: both entry points are
exported, SolSh9 has 112 bytes on both sides, every refusal that needs no device answers SOL_EINVAL in front of the device check and names
its reason in sol_irradiance's words, n == 0 succeeds, the kernels are gfx950 code of the library - and the caller's half, sh9 and
sh9_irradiance, is an orthonormal basis and the cosine lobe's convolution."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from solstrale_amd import _abi, device_count, sh9, sh9_irradiance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "solstrale_hip.h")
ENTRY_POINTS = ("sol_irradiance_sh_dev", "sol_irradiance_sh")
CFG = _abi.SolIrradianceConfig


def test_both_entry_points_are_exported():
    lib = _abi.load_hip()
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libsolstrale_hip.so does not export {name}"
        assert name in _abi.HIP_SYMBOLS
        assert re.search(r"\bint " + name + r"\(SolScene\*", text), name
        assert re.search(r"\b" + name + r"\b", open(os.path.join(ROOT, "INTEGRATION.md")).read()), name


def test_solsh9_has_112_bytes_on_both_sides(tmp_path):
    assert C.sizeof(_abi.SolSh9) == 112 and _abi.SolSh9.c.offset == 0 and _abi.SolSh9.samples.offset == 108
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solstrale_hip.h"\nint main(void) {\n'
                    '  printf("%u %u %u %u", (unsigned)sizeof(SolSh9), (unsigned)offsetof(SolSh9, c), (unsigned)offsetof(SolSh9, samples), (unsigned)sizeof(((SolSh9*)0)->c[0]));\n'
                    '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [112, 0, 108, 12]


def _cfg(**kw):
    c = CFG(size=C.sizeof(CFG), samples=1)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _calls(lib, points, out):
    return (("sol_irradiance_sh", lambda s, n, c: lib.sol_irradiance_sh(s, C.byref(points), None, n, c, C.byref(out))),
            ("sol_irradiance_sh_dev", lambda s, n, c: lib.sol_irradiance_sh_dev(s, C.byref(points), None, n, c, C.byref(out))))


def test_every_refusal_comes_with_its_word_before_the_device():
    """With or without a GPU: sol_irradiance's refusals, in its order and with its words (tests/test_irradiance_abi.py). The configuration and
    n are judged by a function that is not given the handle, right behind the null test of the scene pointer: a zeroed block stands in for a
    scene and is never read. (tests/test_gpu_irradiance_sh.py adds the refusal that reads the handle: a constant medium.)"""
    lib = _abi.load_hip()
    points, out = (_abi.SolRay * 2)(), (_abi.SolSh9 * 2)()
    stand_in = C.create_string_buffer(1 << 20)
    for name, f in _calls(lib, points, out):
        for n in (2, 0):  # (a null scene also with n == 0)
            assert f(None, n, C.byref(_cfg())) == _abi.SOL_EINVAL, name
            assert b"null scene" in lib.sol_last_error() and name.encode() + b":" in lib.sol_last_error()
        assert f(stand_in, 2, None) == _abi.SOL_EINVAL and b"null configuration" in lib.sol_last_error()
        for bad, word in ((_cfg(size=28), b"size"), (_cfg(size=0), b"size"), (_cfg(samples=0), b"samples"),
                          (_cfg(first_sample=0xFFFFFFF0, samples=1), b"first_sample"), (_cfg(mode=2), b"mode"), (_cfg(mode=0xFFFFFFFF), b"mode")):
            assert f(stand_in, 2, C.byref(bad)) == _abi.SOL_EINVAL, (name, word)
            assert word in lib.sol_last_error() and name.encode() + b":" in lib.sol_last_error(), (name, lib.sol_last_error())
        assert f(stand_in, (1 << 31) + 1, C.byref(_cfg())) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
        # the order is sol_radiance's: size, samples, first_sample, n, mode
        assert f(stand_in, (1 << 31) + 1, C.byref(_cfg(mode=7))) == _abi.SOL_EINVAL and b"2^31" in lib.sol_last_error()
        assert f(stand_in, 2, C.byref(_cfg(samples=0, mode=7))) == _abi.SOL_EINVAL and b"samples" in lib.sol_last_error()
        assert f(stand_in, 2, C.byref(_cfg(size=8, samples=0))) == _abi.SOL_EINVAL and b"size" in lib.sol_last_error()
        # n == 0 is SOL_OK: nothing is read behind the scene pointer (has_medium is judged after it), nothing is written
        assert f(stand_in, 0, C.byref(_cfg())) == _abi.SOL_OK, name
        assert f(stand_in, 0, C.byref(_cfg(mode=_abi.SOL_IRRADIANCE_SPHERE, samples=40))) == _abi.SOL_OK, name
    assert bytes(out) == bytes(112 * 2)  # nothing was written


@pytest.mark.skipif(device_count() > 0, reason="only meaningful without a GPU")
def test_without_a_gpu_a_null_scene_is_einval_not_edevice():
    lib = _abi.load_hip()
    points, out = (_abi.SolRay * 1)(), (_abi.SolSh9 * 1)()
    for name, f in _calls(lib, points, out):
        assert f(None, 1, C.byref(_cfg())) == _abi.SOL_EINVAL, name  # otherwise valid arguments: not SOL_EDEVICE


def test_the_kernels_are_gfx950_code_of_the_library():
    data = open(_abi.HIP_LIB, "rb").read()
    assert b"sol_sh_project_kernel" in data and b"amdgcn-amd-amdhsa--gfx950" in data
    # the per-sample instances: sol_radiance_each_kernel<SPILL, STRICT, ENV, LT>, the ten combinations the radiance table has
    each = set(re.findall(rb"_Z24sol_radiance_each_kernelILb[01]ELb[01]ELb[01]ELb[01]EE", data))
    assert len(each) == 10, sorted(each)


# ---- the caller's half --------------------------------------------------------------------------------------------------------------------
def _quadrature(n_theta=8, n_phi=16):
    """Gauss-Legendre in cos(theta) x uniform in phi, float64 weights adding up to 4 pi: exact for polynomials of degree <= 2 n_theta - 1 in z and
    below n_phi in the azimuth - the products of two l <= 2 terms have degree 4."""
    z, wz = np.polynomial.legendre.leggauss(n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    d = np.stack([r * np.cos(pp), r * np.sin(pp), zz], axis=-1).reshape(-1, 3)
    w = (wz[:, None] * np.full(n_phi, 2.0 * np.pi / n_phi)[None, :]).reshape(-1)
    return d, w


def test_sh9_is_float32_and_orthonormal():
    """The Gram matrix of sh9 over the quadrature equals the identity within 1e-5: a value is at most four fp32 roundings (2^-24 relative each)
    on magnitudes <= 1.1 - and the directions are rounded to fp32 first, one more of the same size -, so a product of two errs by below 7e-7,
    summed against weights that total 4 pi: below 9e-6."""
    d, w = _quadrature()
    assert abs(w.sum() - 4.0 * np.pi) < 1e-12
    y = sh9(d)
    assert y.dtype == np.float32 and y.shape == (len(d), 9)
    assert sh9(d.astype(np.float32).reshape(8, 16, 3)).shape == (8, 16, 9)
    assert sh9(np.array([0.0, 0.0, 1.0])).dtype == np.float32
    assert np.abs(y).max() <= 1.1
    gram = np.einsum("i,ik,il->kl", w, y.astype(np.float64), y.astype(np.float64))
    err = np.abs(gram - np.eye(9)).max()
    print(f"sh9 Gram matrix over {len(d)} quadrature points: max |G - I| = {err:.3e}")
    assert err <= 1e-5
    # the stated order and signs, on the axes: Y1 ~ y, Y2 ~ z, Y3 ~ x, no Condon-Shortley sign
    ax = sh9(np.eye(3))
    assert ax[1, 1] > 0 and ax[2, 2] > 0 and ax[0, 3] > 0 and ax[2, 6] > 0 and ax[0, 8] > 0 and ax[1, 8] < 0
    assert sh9(np.array([1.0, 1.0, 0.0]))[4] > 0 and sh9(np.array([0.0, 1.0, 1.0]))[5] > 0 and sh9(np.array([1.0, 0.0, 1.0]))[7] > 0


def test_the_statistical_case_s_seed_stays_inside_five_sigma():
    """A condition on the seed tests/test_gpu_irradiance_sh.py uses, checked here without a GPU before that seed was chosen: over the float
    oracle's 64 x 1024 uniform directions (function 8's sphere draws, which are the device's at first_draw = 2), 4 pi / N x the sum of Y_k is
    sqrt(4 pi) for k = 0 and within 5 sqrt(4 pi / N) of 0 for every k >= 1 and every point (the variance of Y_k under the uniform sphere is
    1 / (4 pi))."""
    import irradiance_sh_util as su
    m = su.stat_basis_means()
    assert m.shape == (su.STAT_POINTS, 9)
    bound = 5.0 * np.sqrt(4.0 * np.pi / su.STAT_SAMPLES)
    worst = np.abs(m[:, 1:]).max()
    print(f"statistical case: max |4 pi sum Y_k / N| over k >= 1 = {worst:.4f}, bound {bound:.4f} ({worst / bound * 5:.2f} sigma)")
    assert np.abs(m[:, 0] - np.sqrt(4.0 * np.pi)).max() <= 1e-6 * np.sqrt(4.0 * np.pi)
    assert worst <= 0.9 * bound  # (a margin for the device's fp32 sums)


def test_sh9_irradiance_is_the_cosine_lobe_s_convolution():
    """L(w) = 1 + 0.5 w_z has the coefficients L_0 = sqrt(4 pi), L_2 = 0.5 sqrt(4 pi / 3) and gives E(n) = pi + (pi / 3) n_z."""
    L = np.zeros((9, 3))
    L[0], L[2] = np.sqrt(4.0 * np.pi), 0.5 * np.sqrt(4.0 * np.pi / 3.0)
    rng = np.random.default_rng(4)
    normals = np.concatenate([np.eye(3), -np.eye(3), rng.normal(size=(6, 3))])
    normals /= np.sqrt((normals ** 2).sum(axis=1, keepdims=True))
    e = sh9_irradiance(L, normals)
    assert e.shape == (12, 3)
    want = np.pi + (np.pi / 3.0) * normals[:, 2].astype(np.float32).astype(np.float64)  # (sh9 rounds the normal to fp32 first)
    err = np.abs(e - want[:, None]).max() / np.pi
    print(f"sh9_irradiance against pi + (pi / 3) n_z over {len(normals)} normals: max error / pi = {err:.3e}")
    assert (np.abs(e - want[:, None]) <= 1e-6 * np.abs(want[:, None])).all()
    # a batch of probes in front: [..., 9, 3] -> [..., m, 3]
    assert sh9_irradiance(np.stack([L, 2 * L]), normals).shape == (2, 12, 3)
