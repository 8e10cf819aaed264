"""numpy restatement of the denoiser's filter contract (include/solstrale_hip.h "denoiser"), for the tests.

Images are (H, W, 3) arrays, row 0 = top. The means are formed in float32 as the device forms them (c = S / n, a = A / m, v = N / m, and
the 0.01 albedo test), everything after that in float64 unless dtype=np.float32 asks for the device's single-precision operation order
(tone t(x) = x / (1 + x), squared distance summed r, g, b, times 1 / sigma_i^2; the exp and pow of numpy may differ from the device's in
the last bit). The taps are summed dy inner, dx outer, as on the device."""
import numpy as np

B3 = (1. / 16., 1. / 4., 3. / 8., 1. / 4., 1. / 16.)
DEFAULTS = dict(iterations=5, sigma_color=0.25, normal_power=64.0)


def prepare(S, n, A, N, m, dtype=np.float64):
    """Steps 1-3: (e, f, g, hit). e = demodulated colour, f = per-channel albedo factor, g = unit guide normal (0 on a miss)."""
    c32 = np.asarray(S, dtype=np.float32) / np.float32(n)
    c32 = np.where(np.isfinite(c32), c32, np.float32(0.))
    a32 = np.asarray(A, dtype=np.float32) / np.float32(m)
    f32 = np.where(a32 > np.float32(0.01), a32, np.float32(1.))
    v32 = np.asarray(N, dtype=np.float32) / np.float32(m)
    if dtype == np.float32:
        e = c32 / f32
        ln = np.sqrt(v32[..., 0] * v32[..., 0] + v32[..., 1] * v32[..., 1] + v32[..., 2] * v32[..., 2])
        hit = ln > np.float32(1e-3)
        g = np.where(hit[..., None], v32 / np.where(hit, ln, np.float32(1.))[..., None], np.float32(0.))
        return e, f32, g.astype(np.float32), hit
    c, f, v = c32.astype(np.float64), f32.astype(np.float64), v32.astype(np.float64)
    e = c / f
    ln = np.sqrt((v * v).sum(-1))
    hit = ln > 1e-3
    g = np.where(hit[..., None], v / np.where(hit, ln, 1.)[..., None], 0.)
    return e, f, g, hit


def _tone(x):
    x = np.maximum(x, x.dtype.type(0))
    return x / (x.dtype.type(1) + x)


def _rect(H, W, ox, oy):
    """(pixels p, taps q = p + (ox, oy)) as slice pairs of the rectangle where q lies inside the image; None when empty."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def atrous_pass(e, g, hit, step, sigma2, normal_power, guided=True):
    """Step 4, one pass at tap spacing `step`. guided=False: every w_pq = 1 (the plain B3 a-trous blur). Taps outside the image are
    skipped; the centre tap counts with w = 1."""
    dt = e.dtype.type
    H, W = e.shape[:2]
    t = _tone(e)
    inv = dt(1.0 / sigma2)
    num = np.zeros_like(e)
    den = np.zeros((H, W), dtype=e.dtype)
    for i in range(5):
        for j in range(5):
            w0 = dt(B3[i]) * dt(B3[j])
            r = _rect(H, W, (i - 2) * step, (j - 2) * step)
            if r is None:
                continue
            P, Q = r
            eq = e[Q]
            if i == 2 and j == 2 or not guided:
                w = np.full(eq.shape[:2], w0, dtype=e.dtype)
            else:
                d = t[P] - t[Q]
                wc = np.exp(-(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) * inv)
                gp, gq, hp, hq = g[P], g[Q], hit[P], hit[Q]
                dot = gp[..., 0] * gq[..., 0] + gp[..., 1] * gq[..., 1] + gp[..., 2] * gq[..., 2]
                wn = np.where(hp & hq, np.maximum(dot, dt(0)) ** dt(normal_power), np.where(~hp & ~hq, dt(1), dt(0)))
                w = w0 * (wc * wn)
            num[P] = num[P] + w[..., None] * eq
            den[P] = den[P] + w
    return num / den[..., None]


def denoise(S, n, A, N, m, iterations=5, sigma_color=0.25, normal_power=64.0, dtype=np.float64):
    """The whole filter: colour sums over n samples, albedo / normal sums over m -> denoised SUMS (times n), float64."""
    e, f, g, hit = prepare(S, n, A, N, m, dtype)
    sigma = float(np.float32(sigma_color))  # (the device holds sigma_color and normal_power in fp32)
    power = float(np.float32(normal_power))
    for i in range(int(iterations)):
        sigma2 = sigma * sigma * 4.0 ** -i
        if dtype == np.float32:
            sigma2 = float(np.float32(1.0 / sigma2)) ** -1  # (the device multiplies by 1 / sigma_i^2 rounded to fp32)
        e = atrous_pass(e, g, hit, 1 << i, sigma2, power)
    return (e.astype(np.float64) * f.astype(np.float64)) * float(n)


def plain_atrous(S, n, iterations=5):
    """The unguided baseline: the same B3 a-trous passes on the colour means with every w = 1 and no demodulation -> sums."""
    c = np.asarray(S, dtype=np.float64) / float(n)
    c = np.where(np.isfinite(c), c, 0.)
    hit = np.ones(c.shape[:2], dtype=bool)
    for i in range(int(iterations)):
        c = atrous_pass(c, c, hit, 1 << i, 1.0, 0.0, guided=False)
    return c * float(n)
