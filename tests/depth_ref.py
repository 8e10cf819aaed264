"""The rule of sol_visibility_oct, sol_volume_build_depth and sol_volume_sample_depth (include/solstrale_hip.h) restated in numpy
float32. It is the yardstick of tests/test_volume_depth_abi.py and tests/test_gpu_volume_depth.py and shares no code with the device: every
operation below is one float32 operation, in the order the header states, so the device's words can be compared bit for bit. The parts of the
sampler that sol_volume_sample states are taken from tests/volume_ref.py's helpers; the corner loop is written out again with the one changed step.
Maps go in and out raw: [n, R * R, 4] SolOctTexel sums, [n, R * R, 2] SolDepthTexel moments."""
import numpy as np

from solstrale_amd import sh9
from volume_ref import VALID, _axis_position, _dot, _normal, _pos

F = np.float32
U = np.uint32
CHUNK = 16


def _sgn(x):
    return np.where(x >= 0, F(1), F(-1)).astype(F)


def texel_directions(res):
    """[res * res, 3] float32: the unit direction of texel (i, j) in row j * res + i"""
    x = np.arange(res * res)
    i, j = (x % res).astype(F), (x // res).astype(F)
    fr = F(res)
    u = (((i + F(0.5)) / fr) * F(2)) - F(1)
    v = (((j + F(0.5)) / fr) * F(2)) - F(1)
    z = (F(1) - np.abs(u)) - np.abs(v)
    fold = z < 0
    tx = np.where(fold, (F(1) - np.abs(v)) * _sgn(u), u)
    ty = np.where(fold, (F(1) - np.abs(u)) * _sgn(v), v)
    t = [tx, ty, z]
    ln = np.sqrt(_dot(t, t))
    return np.stack([tx / ln, ty / ln, z / ln], axis=1).astype(F)


def lobe(T, d, sharpness_log2):
    """c[n, texels] of directions d[n, 3] in the texels T[texels, 3]"""
    c = _pos((T[None, :, 0] * d[:, None, 0] + T[None, :, 1] * d[:, None, 1]) + T[None, :, 2] * d[:, None, 2])
    for _ in range(sharpness_log2):
        c = c * c
    return c.astype(F)


def accumulate(res, sharpness_log2, directions, t, hit, made, valid=None):
    """[n, res * res, 4] sums (w, w_open, wt, wt2) of samples 0 .. S - 1 counted from the call's first sample: directions [S, n, 3] as drawn, t
    [S, n] the hit distances, hit [S, n] and made [S, n] booleans (a made ray that is not a hit is a miss). Rows where `valid` is False are zero."""
    directions = np.asarray(directions, dtype=F)
    t = np.asarray(t, dtype=F)
    S, n = t.shape
    T = texel_directions(res)
    total = np.zeros((n, res * res, 4), dtype=F)
    chunk = np.zeros_like(total)
    with np.errstate(all="ignore"):
        for s in range(S):
            c = lobe(T, directions[s], sharpness_log2)
            m, h = made[s][:, None], (made[s] & hit[s])[:, None]
            o = (made[s] & ~hit[s])[:, None]
            ts = np.where(hit[s], t[s], F(0)).astype(F)[:, None]
            ct = c * ts
            chunk[:, :, 0] = np.where(m, chunk[:, :, 0] + c, chunk[:, :, 0])
            chunk[:, :, 1] = np.where(o, chunk[:, :, 1] + c, chunk[:, :, 1])
            chunk[:, :, 2] = np.where(h, chunk[:, :, 2] + ct, chunk[:, :, 2])
            chunk[:, :, 3] = np.where(h, chunk[:, :, 3] + (ct * ts), chunk[:, :, 3])
            if s % CHUNK == CHUNK - 1 or s == S - 1:
                total = total + chunk
                chunk = np.zeros_like(total)
    if valid is not None:
        total[~np.asarray(valid)] = 0
    return total


def build_depth(oct, radius):
    """[n, texels, 2] (mean, mean2) from [n, texels, 4] sums"""
    o = np.ascontiguousarray(oct, dtype=F)
    radius = F(radius)
    with np.errstate(all="ignore"):
        w, w_open, wt, wt2 = o[..., 0], o[..., 1], o[..., 2], o[..., 3]
        ok = (w > 0) & np.isfinite(o).all(axis=-1)
        s = w_open * radius
        mean = (wt + s) / w
        mean2 = (wt2 + (s * radius)) / w
        out = np.stack([np.where(ok, mean, radius), np.where(ok, mean2, radius * radius)], axis=-1)
    return out.astype(F)


def _axis(p, res):
    hi = F(res) - F(0.5)
    u = (p * F(0.5)) + F(0.5)
    tx = (u * F(res)) - F(0.5)
    tx = np.where(tx > F(-0.5), tx, F(-0.5)).astype(F)
    tx = np.where(tx < hi, tx, hi).astype(F)
    fl = np.floor(tx)
    return fl.astype(np.int64), (tx - fl).astype(F)


def fold(i, j, res):
    """the row of neighbour (i, j), i and j in [-1, res]: beyond one edge the other index is mirrored, beyond a corner both"""
    top = res - 1
    oi, oj = (i < 0) | (i > top), (j < 0) | (j > top)
    ci, cj = np.clip(i, 0, top), np.clip(j, 0, top)
    cj = np.where(oi, top - cj, cj)
    ci = np.where(oj, top - ci, ci)
    return cj * res + ci


def lookup(D, res):
    """rows [4][n] and weights [4][n] (texels 00, 10, 01, 11) of the directions D = [Dx, Dy, Dz], each [n] float32 and not all zero"""
    with np.errstate(all="ignore"):
        s = (np.abs(D[0]) + np.abs(D[1])) + np.abs(D[2])
        px, py = D[0] / s, D[1] / s
        low = D[2] < 0
        fx = (F(1) - np.abs(py)) * _sgn(px)
        fy = (F(1) - np.abs(px)) * _sgn(py)
        px, py = np.where(low, fx, px).astype(F), np.where(low, fy, py).astype(F)
        i0, a = _axis(px, res)
        j0, b = _axis(py, res)
    rows = [fold(i0, j0, res), fold(i0 + 1, j0, res), fold(i0, j0 + 1, res), fold(i0 + 1, j0 + 1, res)]
    wts = [(F(1) - a) * (F(1) - b), a * (F(1) - b), (F(1) - a) * b, a * b]
    return rows, wts


def bilinear(m, wts):
    return ((m[0] * wts[0]) + (m[1] * wts[1])) + ((m[2] * wts[2]) + (m[3] * wts[3]))


def interpolate(depth_map, D, res):
    """(mean, mean2) [n] of one map [texels, 2] in the directions D [n, 3]"""
    D = np.asarray(D, dtype=F)
    rows, wts = lookup([D[:, 0], D[:, 1], D[:, 2]], res)
    return bilinear([depth_map[r, 0] for r in rows], wts), bilinear([depth_map[r, 1] for r in rows], wts)


def chebyshev_factor(mean, mean2, dist):
    """sol_volume_sample's Chebyshev lines: the factor a corner's weight is multiplied by"""
    mean, mean2, dist = (np.asarray(x, dtype=F) for x in (mean, mean2, dist))
    with np.errstate(all="ignore"):
        v = _pos(mean2 - (mean * mean))
        t = dist - mean
        den = v + (t * t)
        h = v / den
        return np.where((dist > mean) & (den > 0), (h * h) * h, F(1)).astype(F)


def volume_sample_depth(grid, probes, depth, res, points):
    """[n, 4] float32 SolRadiance rows: volume_ref.volume_sample with the Chebyshev step reading the probes' maps"""
    probes = np.ascontiguousarray(probes).view(F).reshape(-1, 32)
    depth = np.ascontiguousarray(depth, dtype=F).reshape(len(probes), res * res, 2)
    pts = np.array(points, dtype=F, copy=True).reshape(-1, 8)
    m = len(pts)
    counts = grid.counts
    assert len(probes) == counts[0] * counts[1] * counts[2]
    bias = F(grid.normal_bias)
    with np.errstate(all="ignore"):
        finite = np.isfinite(pts[:, 0:3]).all(axis=1) & np.isfinite(pts[:, 4:7]).all(axis=1)
        N = [pts[:, 4], pts[:, 5], pts[:, 6]]
        valid = finite & _normal(_dot(N, N))
        pts[~valid] = (0, 0, 0, 0, 0, 0, 1, 0)
        p = [pts[:, 0], pts[:, 1], pts[:, 2]]
        N = [pts[:, 4], pts[:, 5], pts[:, 6]]
        r = np.sqrt(_dot(N, N))
        n = [N[a] / r for a in range(3)]
        q = [p[a] + (n[a] * bias) for a in range(3)]
        Y = sh9(np.stack(n, axis=1))
        i0, f = [], []
        for a in range(3):
            if counts[a] == 1:
                g = np.zeros(m, dtype=F)
            else:
                hi = F(counts[a] - 1)
                g = (q[a] - F(grid.origin[a])) / F(grid.spacing[a])
                g = np.where(g > 0, g, F(0))
                g = np.where(g < hi, g, hi)
            lo = np.minimum(np.floor(g).astype(np.int64), max(counts[a] - 2, 0))
            i0.append(lo)
            f.append(g - lo.astype(F))
        total = [np.zeros(m, dtype=F) for _ in range(3)]
        wsum = np.zeros(m, dtype=F)
        samples = np.zeros(m, dtype=U)
        for c in range(8):
            d = (c & 1, (c >> 1) & 1, c >> 2)
            wa = [f[a] if d[a] else (F(1) - f[a]) for a in range(3)]
            w = (wa[0] * wa[1]) * wa[2]
            active = valid & (w != 0)
            idx = [np.minimum(i0[a] + d[a], counts[a] - 1) for a in range(3)]
            probe = (idx[2] * counts[1] + idx[1]) * counts[0] + idx[0]
            e = probes[probe]
            flags = np.ascontiguousarray(e[:, 29]).view(U)
            active &= (flags & VALID) != 0
            at = [_axis_position(grid, a, idx[a]) for a in range(3)]
            if grid.backface:
                D = [at[a] - p[a] for a in range(3)]
                l2 = _dot(D, D)
                cos = _dot(D, n) / np.sqrt(l2)
                b = (cos + F(1)) * F(0.5)
                w = np.where(l2 > 0, w * ((b * b) + F(0.2)), w)
            if grid.chebyshev:
                D = [q[a] - at[a] for a in range(3)]
                dist = np.sqrt(_dot(D, D))
                rows, wts = lookup(D, res)
                mean = bilinear([depth[probe, rw, 0] for rw in rows], wts)
                mean2 = bilinear([depth[probe, rw, 1] for rw in rows], wts)
                w = np.where(dist > 0, w * chebyshev_factor(mean, mean2, dist), w)
            active &= w > 0
            samples += active.astype(U)
            for ch in range(3):
                E = np.zeros(m, dtype=F)
                for k in range(9):
                    E = E + (e[:, k * 3 + ch] * Y[:, k])
                total[ch] = np.where(active, total[ch] + (w * _pos(E)), total[ch])
            wsum = np.where(active, wsum + w, wsum)
        out = np.zeros((m, 4), dtype=F)
        some = samples != 0
        for ch in range(3):
            out[:, ch] = np.where(some, total[ch] / wsum, F(0))
        out.view(U)[:, 3] = samples
    return out
