"""The rule of sol_lightmap_filter_var (include/solstrale_hip.h) restated in numpy float32: a loop over passes, the nine taps of the
variance prefilter and the 25 B3 taps, vectorised over the atlas. It is the yardstick of tests/test_lightmap_filter_var_abi.py and
tests/test_gpu_lightmap_filter_var.py and shares no code with the device: every operation below is one float32 operation, in the order the header
states, so the device's words can be compared bit for bit. The taps' order and skips and the factors k, w_d, w_pl and c are section 26's and come
from tests/lightmap_filter_ref.py (tap_weights with no value channel: D = 0, w_v = 1 / (1 + 0 / 1) = 1, and the weight it returns is
((k * w_d) * w_pl) * c times one); also restated here is sol_irradiance_moments' association of the per-sample colours (moments_of_samples)."""
import numpy as np

import lightmap_filter_ref as fr

F = np.float32
NONE = fr.NONE
H3 = (F(1 / 4), F(1 / 2), F(1 / 4))
ONE, ZERO = fr.ONE, fr.ZERO
MOMENTS_DTYPE = np.dtype([("sum", np.float32, (3,)), ("samples", np.uint32), ("sum2", np.float32, (3,)), ("reserved", np.uint32)])
CHUNK = 16


def moments_rows(moments):
    """[n, 8] uint32 words of MOMENTS_DTYPE rows or of [n, 8] float32 rows."""
    m = np.ascontiguousarray(moments)
    return m.view(np.uint32).reshape(-1, 8)


def live_texels(moments, points, texels):
    """[n] bool: owned, the six position and normal words finite, samples >= 2, the six sums finite."""
    w = moments_rows(moments)
    f = w.view(F)
    p = np.asarray(points, dtype=F)
    return ((np.asarray(texels)["triangle"] != NONE) & np.isfinite(p[:, 0:3]).all(axis=1) & np.isfinite(p[:, 4:7]).all(axis=1) & (w[:, 3] >= 2)
            & np.isfinite(f[:, 0:3]).all(axis=1) & np.isfinite(f[:, 4:7]).all(axis=1))


def prepare(moments):
    """Prepare, for every row (the caller masks the rows that are not live): (x [n, 3], v [n, 3], N [n])."""
    w = moments_rows(moments)
    f = w.view(F)
    with np.errstate(all="ignore"):
        N = w[:, 3].astype(F)
        M = (w[:, 3] - np.uint32(1)).astype(F)
        x = f[:, 0:3] / N[:, None]
        v = fr._pos((f[:, 4:7] / N[:, None]) - (x * x)) / M[:, None]
    assert x.dtype == F and v.dtype == F
    return x, v, N


def _shift(Hh, Ww, oy, ox):
    if abs(oy) >= Hh or abs(ox) >= Ww:
        return None
    dst = (slice(max(0, -oy), Hh - max(0, oy)), slice(max(0, -ox), Ww - max(0, ox)))
    src = (slice(max(0, oy), Hh - max(0, -oy)), slice(max(0, ox), Ww - max(0, -ox)))
    return dst, src


def lightmap_filter_var(moments, points, texels, width, height, sigma_position, sigma_plane=None, iterations=4, normal_power_log2=5, sigma_value=4.0,
                        variance_floor=1e-12):
    """(out [W * H, 4] float32 rows, variance_out [W * H, 4] float32 rows) as sol_lightmap_filter_var writes them."""
    W, Hh = int(width), int(height)
    words = moments_rows(moments)
    points = np.asarray(points, dtype=F)
    live1 = live_texels(moments, points, texels)
    live = live1.reshape(Hh, W)
    P, Nn = points[:, 0:3].reshape(Hh, W, 3), points[:, 4:7].reshape(Hh, W, 3)
    x1, v1, N1 = prepare(moments)
    x = np.where(live1[:, None], x1, ZERO).astype(F).reshape(Hh, W, 3)
    v = np.where(live1[:, None], v1, ZERO).astype(F).reshape(Hh, W, 3)
    sigma_plane = sigma_position if sigma_plane is None else sigma_plane
    floor = F(variance_floor)
    no_values = np.zeros((Hh, W, 0), dtype=F)
    with np.errstate(all="ignore"):
        svs = F(sigma_value) * F(sigma_value)
        for i in range(int(iterations)):
            step = 1 << i
            f = F(step)
            s, sp = F(sigma_position) * f, F(sigma_plane) * f
            ss, sps = s * s, sp * sp
            # the variance prefilter: nine texels one apart, whatever the step
            vb = np.zeros((Hh, W, 3), dtype=F)
            gs = np.zeros((Hh, W), dtype=F)
            for dj in range(-1, 2):
                for di in range(-1, 2):
                    sh = _shift(Hh, W, dj, di)
                    if sh is None:
                        continue
                    dst, src = sh
                    g = H3[di + 1] * H3[dj + 1]
                    ok = live[dst] & live[src]
                    vb[dst] = np.where(ok[..., None], vb[dst] + (g * v[src]), vb[dst])
                    gs[dst] = np.where(ok, gs[dst] + g, gs[dst])
            V = (((vb[..., 0] / gs) + (vb[..., 1] / gs)) + (vb[..., 2] / gs)) + floor
            den = svs * V
            assert den.dtype == F
            total = np.zeros((Hh, W, 3), dtype=F)
            vs = np.zeros((Hh, W, 3), dtype=F)
            wsum = np.zeros((Hh, W), dtype=F)
            for dj in range(-2, 3):
                for di in range(-2, 3):
                    tap = fr.tap_weights(P, Nn, no_values, live, dj, di, step, ss, sps, ONE, int(normal_power_log2), 0)
                    if tap is None:
                        continue
                    dst, src, ok, w = tap
                    if not (di == 0 and dj == 0):
                        D = np.zeros(ok.shape, dtype=F)
                        for j in range(3):
                            dv = x[dst][..., j] - x[src][..., j]
                            D = D + (dv * dv)
                        w_v = ONE / (ONE + (D / den[dst]))
                        w_v = w_v * w_v
                        w = w * w_v
                        ok = ok & (w > 0)
                    assert w.dtype == F
                    ww = w * w
                    total[dst] = np.where(ok[..., None], total[dst] + (w[..., None] * x[src]), total[dst])
                    vs[dst] = np.where(ok[..., None], vs[dst] + (ww[..., None] * v[src]), vs[dst])
                    wsum[dst] = np.where(ok, wsum[dst] + w, wsum[dst])
            nx = total / wsum[..., None]
            nv = vs / (wsum * wsum)[..., None]
            assert nx.dtype == F and nv.dtype == F
            x = np.where(live[..., None], nx, x)
            v = np.where(live[..., None], nv, v)
        scaled = x.reshape(W * Hh, 3) * N1[:, None]
    out = words[:, 0:4].copy()
    out.view(F)[live1, 0:3] = scaled[live1]
    var = np.zeros((W * Hh, 4), dtype=F)
    var[live1, 0:3] = v.reshape(W * Hh, 3)[live1]
    return out.view(F), var


def moments_of_samples(colours, valid=None):
    """sol_irradiance_moments' six sums from the per-sample colours c_s, [k, n, 3] float32 in sample order: chunks of 16 counted from the first
    sample, a chunk sum 0 + t + t .., the result ((0 + chunk0) + chunk1) + ..; the squares are rounded once before they are added. Returns
    MOMENTS_DTYPE rows; rows that are not `valid` are eight zero words."""
    c = np.asarray(colours, dtype=F)
    k, n = c.shape[0], c.shape[1]
    total = np.zeros((n, 6), dtype=F)
    for j0 in range(0, k, CHUNK):
        chunk = np.zeros((n, 6), dtype=F)
        for j in range(j0, min(j0 + CHUNK, k)):
            chunk[:, 0:3] = chunk[:, 0:3] + c[j]
            chunk[:, 3:6] = chunk[:, 3:6] + (c[j] * c[j])
        total = total + chunk
    rows = np.zeros(n, dtype=MOMENTS_DTYPE)
    rows["sum"], rows["sum2"], rows["samples"] = total[:, 0:3], total[:, 3:6], k
    if valid is not None:
        rows[~np.asarray(valid)] = np.zeros(1, dtype=MOMENTS_DTYPE)
    return rows
