"""The rule of sol_volume_points, sol_volume_build and sol_volume_sample (include/solstrale_hip.h) restated in numpy float32,
vectorised over probes and points with a plain loop over the eight corners of a cell. It is the yardstick of tests/test_volume_abi.py and
tests/test_gpu_volume.py and shares no code with the device: every operation below is one float32 operation, in the order the header states, so
the device's words can be compared bit for bit. (The nine SH terms are solstrale_amd.sh9, the restatement of csrc/sol_sh.h that the SH irradiance
tests pin to the device.) A grid is anything with origin, spacing, counts, backface, chebyshev and normal_bias - a solstrale_amd.VolumeGrid.
Rows go in and out raw: [n, 28] SolSh9, [n, 8] SolVisibility, [n, 32] SolProbe, [n, 8] points, [n, 4] SolRadiance, float32 with the counts as bits."""
import numpy as np

from solstrale_amd import sh9

F = np.float32
U = np.uint32
K4PI = F(4.0 * np.pi)
ZONAL = np.repeat([F(np.pi), F(2.0 * np.pi / 3.0), F(np.pi / 4.0)], [3, 9, 15]).astype(F)  # A[l(k)] per word k * 3 + c of the 27
PROBE_DTYPE = np.dtype([("e", np.float32, (9, 3)), ("mean", np.float32), ("mean2", np.float32), ("flags", np.uint32), ("samples", np.uint32),
                        ("reserved", np.uint32)])
VALID, MOMENTS = 1, 2


def _normal(x):
    """finite, not zero, not subnormal - elementwise on float32"""
    e = np.ascontiguousarray(x, dtype=F).view(U) & U(0x7F800000)
    return (e != 0) & (e != U(0x7F800000))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _pos(x):
    return np.where(x > 0, x, F(0))


def _axis_position(grid, a, i):
    """o + ((float)i * s); o itself on an axis with one probe"""
    if grid.counts[a] == 1:
        return np.full(np.shape(i), F(grid.origin[a]), dtype=F)
    return F(grid.origin[a]) + (np.asarray(i).astype(F) * F(grid.spacing[a]))


def probe_positions(grid):
    """[nx * ny * nz, 3] float32, probe (i, j, k) in row (k * ny + j) * nx + i"""
    nx, ny, nz = grid.counts
    x = np.arange(nx * ny * nz)
    with np.errstate(all="ignore"):
        return np.stack([_axis_position(grid, 0, x % nx), _axis_position(grid, 1, (x // nx) % ny), _axis_position(grid, 2, x // (nx * ny))], axis=1)


def volume_points(grid, tmin=1e-3, tmax=float("inf")):
    at = probe_positions(grid)
    rows = np.zeros((len(at), 8), dtype=F)
    rows[:, 0:3], rows[:, 3], rows[:, 6], rows[:, 7] = at, F(tmin), F(1), F(tmax)
    return rows


def volume_build(sh, visibility=None, radius=0.0):
    """[n, 32] float32 probe rows from [n, 28] SolSh9 rows and (or None) [n, 8] SolVisibility rows"""
    sh = np.ascontiguousarray(sh, dtype=F)
    n = len(sh)
    radius = F(radius)
    out = np.zeros((n, 32), dtype=F)
    words = out.view(U)
    samples = np.ascontiguousarray(sh[:, 27]).view(U)
    with np.errstate(all="ignore"):
        valid = (samples != 0) & np.isfinite(sh[:, :27]).all(axis=1)
        fs = samples.astype(F)
        out[:, :27] = ((sh[:, :27] * K4PI) / fs[:, None]) * ZONAL[None, :]
        words[:, 29] = VALID
        words[:, 30] = samples
        if visibility is not None:
            vis = np.ascontiguousarray(visibility).view(F).reshape(n, 8)
            vw = vis.view(U)
            moments = (vw[:, 7] != 0) & np.isfinite(vis[:, 4]) & np.isfinite(vis[:, 5]) & bool(np.isfinite(radius) and radius > 0)
            vopen, vs = vw[:, 3].astype(F), vw[:, 7].astype(F)
            out[:, 27] = np.where(moments, (vis[:, 4] + (vopen * radius)) / vs, F(0))
            out[:, 28] = np.where(moments, (vis[:, 5] + ((vopen * radius) * radius)) / vs, F(0))
            words[:, 29] |= np.where(moments, U(MOMENTS), U(0))
    words[~valid] = 0
    return out


def volume_sample(grid, probes, points):
    """[n, 4] float32 SolRadiance rows (r, g, b, the bits of the count of probes that contributed)"""
    probes = np.ascontiguousarray(probes).view(F).reshape(-1, 32)
    pts = np.array(points, dtype=F, copy=True).reshape(-1, 8)
    m = len(pts)
    counts = grid.counts
    assert len(probes) == counts[0] * counts[1] * counts[2]
    bias = F(grid.normal_bias)
    with np.errstate(all="ignore"):
        finite = np.isfinite(pts[:, 0:3]).all(axis=1) & np.isfinite(pts[:, 4:7]).all(axis=1)
        N = [pts[:, 4], pts[:, 5], pts[:, 6]]
        valid = finite & _normal(_dot(N, N))
        pts[~valid] = (0, 0, 0, 0, 0, 0, 1, 0)  # (computed like the others, answered with zeros)
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
            idx = [np.minimum(i0[a] + d[a], counts[a] - 1) for a in range(3)]  # (a zero-weight corner may lie outside; it is not looked at)
            e = probes[(idx[2] * counts[1] + idx[1]) * counts[0] + idx[0]]
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
                mean, mean2 = e[:, 27], e[:, 28]
                D = [at[a] - q[a] for a in range(3)]
                dist = np.sqrt(_dot(D, D))
                v = _pos(mean2 - (mean * mean))
                t = dist - mean
                den = v + (t * t)
                h = v / den
                w = np.where(((flags & MOMENTS) != 0) & (dist > mean) & (den > 0), w * ((h * h) * h), w)
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


# ---- what the tests share ----
def constant_sh(n, radiance, samples=64):
    """[n, 28] SolSh9 rows of probes that saw the constant radiance `radiance` (3 numbers) in every direction: c[0] = samples * L * k0, the rest 0"""
    rows = np.zeros((n, 28), dtype=F)
    rows[:, 0:3] = (F(samples) * np.asarray(radiance, dtype=F)) * sh9(np.zeros((1, 3), dtype=F))[0, 0]
    rows.view(U)[:, 27] = samples
    return rows


def probes_of_values(values):
    """[n, 32] valid probes without moments whose irradiance is values[n, 3] for every normal: e[0] = value / k0"""
    values = np.asarray(values, dtype=np.float64)
    rows = np.zeros((len(values), 32), dtype=F)
    rows[:, 0:3] = (values / float(sh9(np.zeros((1, 3), dtype=F))[0, 0])).astype(F)
    rows.view(U)[:, 29] = VALID
    rows.view(U)[:, 30] = 1
    return rows


def unit_normals(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def point_rows(positions, normals):
    rows = np.zeros((len(positions), 8), dtype=F)
    rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7] = positions, normals, F(1e-3), F(np.inf)
    return rows
