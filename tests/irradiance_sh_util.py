"""What the SH irradiance tests share (tests/test_irradiance_sh_abi.py on the CPU, tests/test_gpu_irradiance_sh.py on the device): the sums'
association restated in numpy float32, and the seed of the statistical case with the CPU's prediction for it."""
import numpy as np

import irradiance_util as iu
from solstrale_amd import sh9

# The statistical case: 64 points, 1024 SPHERE samples from sample 0 at first_draw = 2 - the float oracle's function-8 sphere draws.
STAT_SEED = 0x5EED5A99
STAT_KEY_BASE = 3000
STAT_POINTS, STAT_SAMPLES = 64, 1024


def association(terms):
    """terms: [k, ...] float32, one term per sample counted from first_sample. Chunk sums of up to 16 samples, each 0 + t + t + .. in sample
    order, then the chunks in order on top of 0: sol_radiance's association, restated in numpy float32."""
    terms = np.asarray(terms)
    assert terms.dtype == np.float32
    total = np.zeros(terms.shape[1:], dtype=np.float32)
    for c0 in range(0, len(terms), 16):
        chunk = np.zeros(terms.shape[1:], dtype=np.float32)
        for j in range(c0, min(c0 + 16, len(terms))):
            chunk = chunk + terms[j]
        total = total + chunk
    assert total.dtype == np.float32
    return total


def projected(colours, directions):
    """fl(c_s[channel] x Y_k(d_s)): colours [k, n, 3] and directions [k, n, 3] float32 -> [k, n, 9, 3] float32."""
    c, y = np.asarray(colours), sh9(directions)
    assert c.dtype == np.float32 and y.dtype == np.float32
    t = c[..., None, :] * y[..., :, None]
    assert t.dtype == np.float32
    return t


def stat_basis_means():
    """4 pi / N x the sum over the case's samples of Y_k(d) per point, [points, 9] float64, from the float oracle's draws: what the device's
    4 pi c[k] / N is under a background of 1, up to fp32 rounding."""
    p, _ = iu.sphere_draws_after_the_cosine(STAT_SEED, STAT_KEY_BASE + np.arange(STAT_POINTS), np.arange(STAT_SAMPLES))
    p = p.astype(np.float64)
    d = p / np.sqrt((p * p).sum(axis=-1, keepdims=True))
    return 4.0 * np.pi * sh9(d).astype(np.float64).sum(axis=1) / STAT_SAMPLES
