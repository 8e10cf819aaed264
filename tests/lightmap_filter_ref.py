"""The rule of sol_lightmap_filter (include/solstrale_hip.h) restated in numpy float32: a loop over passes and the 25 taps, vectorised
over the atlas. It is the yardstick of tests/test_lightmap_filter_abi.py and tests/test_gpu_lightmap_filter.py and shares no code with the device:
every operation below is one float32 operation, in the order the header states, so the device's words can be compared bit for bit."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
ONE, ZERO = F(1), F(0)


def _pos(x):
    return np.where(x > 0, x, ZERO).astype(F)


def _dot(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def live_texels(values, points, texels, channels):
    """[n] bool: owned, the six position and normal words finite, the `channels` value words finite."""
    v = np.asarray(values, dtype=F)
    p = np.asarray(points, dtype=F)
    return ((np.asarray(texels)["triangle"] != NONE) & np.isfinite(p[:, 0:3]).all(axis=1) & np.isfinite(p[:, 4:7]).all(axis=1)
            & np.isfinite(v[:, :channels]).all(axis=1))


def tap_weights(P, N, T, live, dj, di, step, ss, sps, svs, npl2, m):
    """For the tap (di, dj) * step of every centre that has it inside the atlas: (dst, src, ok, w) - the slices of the centres and of their taps,
    whether the tap counts and its weight. P, N: [H, W, 3]; T: [H, W, m] the toned values of the pass's input."""
    Hh, Ww = live.shape
    oy, ox = dj * step, di * step
    if abs(oy) >= Hh or abs(ox) >= Ww:
        return None
    dst = (slice(max(0, -oy), Hh - max(0, oy)), slice(max(0, -ox), Ww - max(0, ox)))
    src = (slice(max(0, oy), Hh - max(0, -oy)), slice(max(0, ox), Ww - max(0, -ox)))
    k = H5[di + 2] * H5[dj + 2]
    ok = live[dst] & live[src]
    if di == 0 and dj == 0:
        return dst, src, ok, np.full(ok.shape, k, dtype=F)
    E = P[src] - P[dst]
    l2 = _dot(E, E)
    w_d = ONE / (ONE + (l2 / ss))
    d = _dot(N[dst], E)
    w_pl = ONE / (ONE + ((d * d) / sps))
    c = _pos(_dot(N[dst], N[src]))
    for _ in range(npl2):
        c = c * c
    D = np.zeros(ok.shape, dtype=F)
    for j in range(m):
        dv = T[dst][..., j] - T[src][..., j]
        D = D + (dv * dv)
    w_v = ONE / (ONE + (D / svs))
    w_v = w_v * w_v
    w = (((k * w_d) * w_pl) * c) * w_v
    assert w.dtype == F
    return dst, src, ok & (w > 0), w


def lightmap_filter(values, points, texels, width, height, sigma_position, sigma_plane=None, iterations=4, normal_power_log2=5, sigma_value=0.25,
                    value_scale=1.0, channels=3):
    """`out` as sol_lightmap_filter writes it; values: [H * W, k] float32 rows whose leading `channels` words are filtered."""
    W, Hh = int(width), int(height)
    values = np.ascontiguousarray(values, dtype=F)
    words = values.view(np.uint32).reshape(W * Hh, -1)
    points = np.asarray(points, dtype=F)
    live1 = live_texels(values, points, texels, channels)
    live = live1.reshape(Hh, W)
    P, N = points[:, 0:3].reshape(Hh, W, 3), points[:, 4:7].reshape(Hh, W, 3)
    x = values[:, :channels].reshape(Hh, W, channels).copy()
    m = min(channels, 3)
    sigma_plane = sigma_position if sigma_plane is None else sigma_plane
    scale = F(value_scale)
    with np.errstate(all="ignore"):
        for i in range(int(iterations)):
            step = 1 << i
            f = F(step)
            s, sp, sv = F(sigma_position) * f, F(sigma_plane) * f, F(sigma_value) / f
            ss, sps, svs = s * s, sp * sp, sv * sv
            a = _pos(x[..., :m] * scale)
            T = a / (ONE + a)
            total = np.zeros((Hh, W, channels), dtype=F)
            wsum = np.zeros((Hh, W), dtype=F)
            for dj in range(-2, 3):
                for di in range(-2, 3):
                    tap = tap_weights(P, N, T, live, dj, di, step, ss, sps, svs, int(normal_power_log2), m)
                    if tap is None:
                        continue
                    dst, src, ok, w = tap
                    total[dst] = np.where(ok[..., None], total[dst] + (w[..., None] * x[src]), total[dst])
                    wsum[dst] = np.where(ok, wsum[dst] + w, wsum[dst])
            new = total / wsum[..., None]
            assert new.dtype == F
            x = np.where(live[..., None], new, x)
    out = words.copy()
    out.view(F)[live1, :channels] = x.reshape(W * Hh, channels)[live1]
    return out.view(F).reshape(values.shape)
