"""The rule of sol_lightmap_sh and sol_lightmap_normals (include/solstrale_hip.h) restated in numpy float32, vectorised over the rows.
It is the yardstick of tests/test_lightmap_sh_abi.py and tests/test_gpu_lightmap_sh.py and shares no code with the device: every operation below is
one float32 operation, in the order the header states, so the device's words can be compared bit for bit. The lookup is the lookup of
tests/lightmap_sample_ref.py with 27 channels - the header says so - and is taken from there."""
import numpy as np

import lightmap_sample_ref as sr

F = np.float32
NONE = sr.NONE
TEXEL_DTYPE = sr.TEXEL_DTYPE
CHANNELS = 27
A = (F(np.pi),) + (F(2.0 * np.pi / 3.0),) * 3 + (F(np.pi / 4.0),) * 5  # the cosine lobe's zonal factors, rounded to float32
K = tuple(F(x) for x in (np.sqrt(1 / (4 * np.pi)), np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi)), np.sqrt(5 / (16 * np.pi)), np.sqrt(15 / (16 * np.pi))))
ONE, ZERO, THREE = F(1), F(0), F(3)


def normal_number(x):
    """finite, not zero, not subnormal - elementwise on float32"""
    e = np.asarray(x, dtype=F).view(np.uint32) & np.uint32(0x7F800000)
    return (e != 0) & (e != np.uint32(0x7F800000))


def basis(x, y, z):
    """the nine terms Y_k of the header's SH section, in its bracketing"""
    k0, k1, k2, k3, k4 = K
    return [np.full(x.shape, k0, dtype=F), k1 * y, k1 * z, k1 * x, (k2 * x) * y, (k2 * y) * z, k3 * ((THREE * (z * z)) - ONE), (k2 * x) * z,
            k4 * ((x * x) - (y * y))]


def lightmap_sh(values, coords, normals, uvs, texels, width, height, scale=1.0, pass_of=None, nearest=False, chart_radius=np.inf, vertices=None, points=None,
                clamp=False, coefficients=False):
    """[n, 4] rows (E_r, E_g, E_b, the bits of the count) as sol_lightmap_sh writes them, or with coefficients=True its [n, 28] rows."""
    rows = sr.lightmap_sample(values, coords, uvs, texels, width, height, channels=CHANNELS, pass_of=pass_of, nearest=nearest, chart_radius=chart_radius,
                              vertices=vertices, points=points)
    if coefficients:
        return rows
    L, count = rows[:, :CHANNELS], rows[:, CHANNELS].view(np.uint32)
    nrm = np.ascontiguousarray(normals, dtype=F).reshape(len(rows), 4)
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    out = np.zeros((len(rows), 4), dtype=F)
    with np.errstate(all="ignore"):
        ok = (count != 0) & sr.finite(x) & sr.finite(y) & sr.finite(z) & normal_number(((x * x) + (y * y)) + (z * z))
        Y = basis(x, y, z)
        B = [A[k] * Y[k] for k in range(9)]
        for ch in range(3):
            E = np.zeros(len(rows), dtype=F)
            for k in range(9):
                E = E + (B[k] * L[:, 3 * k + ch])
            E = E * F(scale)
            if clamp:
                E = np.where(E > 0, E, ZERO)
            assert E.dtype == F
            out[:, ch] = np.where(ok, E, ZERO)
    out[:, 3] = np.where(ok, count, 0).astype(np.uint32).view(F)
    return out


def lightmap_normals(coords, vertices, normals=None):
    """[n, 4] rows (nx, ny, nz, 0) as sol_lightmap_normals writes them."""
    coords = np.asarray(coords)
    V = np.asarray(vertices, dtype=F).reshape(-1, 3, 3)
    N = None if normals is None else np.asarray(normals, dtype=F).reshape(-1, 3, 3)
    n, nt = len(coords), len(V)
    out = np.zeros((n, 4), dtype=F)
    with np.errstate(all="ignore"):
        tri, b1, b2 = coords["triangle"], coords["b1"].astype(F), coords["b2"].astype(F)
        valid = (coords["flags"] != 0) & (tri != NONE) & (tri < nt) & sr.finite(b1) & sr.finite(b2)
        g = np.where(valid, tri, 0).astype(np.int64)
        v = V[g] if nt else np.zeros((n, 3, 3), dtype=F)
        valid &= sr.finite(v).reshape(n, 9).all(axis=1)
        b0 = (ONE - b1) - b2
        a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        vec = [a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]]
        if N is not None:
            m = N[g] if nt else np.zeros((n, 3, 3), dtype=F)
            valid &= sr.finite(m).reshape(n, 9).all(axis=1)
            mix = [((m[:, 0, k] * b0) + (m[:, 1, k] * b1)) + (m[:, 2, k] * b2) for k in range(3)]
            use = normal_number((mix[0] * mix[0] + mix[1] * mix[1]) + mix[2] * mix[2])
            vec = [np.where(use, mix[k], vec[k]) for k in range(3)]
        len2 = (vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]
        valid &= normal_number(len2)
        length = np.sqrt(len2)
        assert length.dtype == F
        for k in range(3):
            out[:, k] = np.where(valid, vec[k] / length, ZERO)
    return out
