"""The rule of sol_lightmap_mip_layout, sol_lightmap_mips, sol_lightmap_sample_lod and sol_lightmap_lod (include/solstrale_hip.h)
restated in numpy float32, vectorised over texels and rows. It is the yardstick of tests/test_lightmap_mips_abi.py and
tests/test_gpu_lightmap_mips.py and shares no code with the device: every operation below is one float32 operation, in the order the header
states, so the device's words can be compared bit for bit. Level 0's lookup is tests/lightmap_sample_ref.py's, called, not restated."""
import numpy as np

import lightmap_sample_ref as sr

F = np.float32
NONE = 0xFFFFFFFF
UNCOVERED = 255
MAX_LEVELS = 15
ONE, HALF, ZERO = F(1), F(0.5), F(0)
RAY_HIT = 1
finite = sr.finite


def mip_layout(width, height, levels=None):
    """(levels, widths, heights, row offsets, total rows): level 0 is the atlas (offset 0: it is not in the chain), level l >= 1 starts at row
    sum_{k=1}^{l-1} W_k H_k. levels None or 0: all."""
    w, h, sizes = int(width), int(height), []
    while True:
        sizes.append((w, h))
        if w == 1 and h == 1:
            break
        w, h = (w + 1) // 2, (h + 1) // 2
    n = len(sizes) if not levels else int(levels)
    assert 1 <= n <= len(sizes)
    offsets, total = [0], 0
    for l in range(1, n):
        offsets.append(total)
        total += sizes[l][0] * sizes[l][1]
    return n, [s[0] for s in sizes[:n]], [s[1] for s in sizes[:n]], offsets, total


def lightmap_mips(values, texels, width, height, channels=3, pass_of=None, levels=None):
    """(mips [rows, k] float32 words, cover [rows] uint8) as sol_lightmap_mips writes them; values: [W * H, k] rows of 32-bit words."""
    W, H, ch = int(width), int(height), int(channels)
    rows = np.ascontiguousarray(values).view(np.uint32).reshape(W * H, -1)
    k = rows.shape[1]
    n, ws, hs, offsets, total = mip_layout(W, H, levels)
    mips, cover = np.zeros((total, k), dtype=np.uint32), np.zeros(total, dtype=np.uint8)
    covered = (np.asarray(pass_of).reshape(-1) != UNCOVERED) if pass_of is not None else (np.asarray(texels)["triangle"] != NONE)
    live = (covered & finite(rows[:, :ch].view(F)).all(axis=1)).reshape(H, W)
    src = rows.reshape(H, W, k)
    with np.errstate(all="ignore"):
        for l in range(1, n):
            Ws, Hs, Wd, Hd = ws[l - 1], hs[l - 1], ws[l], hs[l]
            total_x = np.zeros((Hd, Wd, ch), dtype=F)
            count = np.zeros((Hd, Wd), dtype=np.uint32)
            rest = np.zeros((Hd, Wd, k), dtype=np.uint32)  # the whole row of the first live tap
            found = np.zeros((Hd, Wd), dtype=bool)
            for t in range(4):
                di, dj = t & 1, t >> 1
                jj, ii = np.meshgrid(2 * np.arange(Hd) + dj, 2 * np.arange(Wd) + di, indexing="ij")
                inside = (ii < Ws) & (jj < Hs)
                ci, cj = np.where(inside, ii, 0), np.where(inside, jj, 0)
                tap_live = inside & live[cj, ci]
                x = src[cj, ci]
                total_x = np.where(tap_live[..., None], total_x + x[..., :ch].view(F), total_x)
                count += tap_live
                first = tap_live & ~found
                rest[first] = x[first]
                found |= tap_live
            mean = total_x / count.astype(F)[..., None]
            assert mean.dtype == F
            ok = found & finite(mean).all(axis=2)
            out = rest
            out[..., :ch] = mean.view(np.uint32)
            out[~ok] = 0
            mips[offsets[l]:offsets[l] + Wd * Hd] = out.reshape(Wd * Hd, k)
            cover[offsets[l]:offsets[l] + Wd * Hd] = np.where(ok, 0, UNCOVERED).reshape(-1)
            src, live = out, ok
    return mips.view(F), cover


def _level_lookup(l, rows_l, cover_l, Wl, Hl, u, v, valid, W, H, ch):
    """sol_lightmap_sample's bilinear rule over level l >= 1: (answer [n, ch], wsum > 0, count)"""
    n = len(u)
    val = rows_l.view(F)[:, :ch]
    s = F(2.0 ** -l)
    x, y = ((u * F(W)) * s) - HALF, ((v * F(H)) * s) - HALF
    inside = valid & (x >= -1) & (x < F(Wl)) & (y >= -1) & (y < F(Hl))
    xf, yf = np.floor(np.where(inside, x, ZERO)), np.floor(np.where(inside, y, ZERO))
    i0, j0 = xf.astype(np.int64), yf.astype(np.int64)
    fx, fy = np.where(inside, x, ZERO) - xf, np.where(inside, y, ZERO) - yf
    wsum, total, count = np.zeros(n, dtype=F), np.zeros((n, ch), dtype=F), np.zeros(n, dtype=np.uint32)
    for k in range(4):
        i, j = i0 + (k & 1), j0 + (k >> 1)
        live = inside & (i >= 0) & (j >= 0) & (i < Wl) & (j < Hl)
        at = np.where(live, j * Wl + i, 0)
        live &= cover_l[at] != UNCOVERED
        live &= finite(val[at]).all(axis=1)
        wx, wy = (fx if k & 1 else ONE - fx), (fy if k >> 1 else ONE - fy)
        w = wx * wy
        wsum = np.where(live, wsum + w, wsum)
        total = np.where(live[:, None], total + (w[:, None] * val[at]), total)
        count += live
    ok = wsum > 0
    answer = total / wsum[:, None]
    assert answer.dtype == F
    return np.where(ok[:, None], answer, ZERO), ok, np.where(ok, count, 0).astype(np.uint32)


def clamp_lod(lods, levels):
    lam = np.asarray(lods, dtype=F)
    lam = np.where(lam > 0, lam, ZERO)
    return np.where(lam >= F(levels - 1), F(levels - 1), lam).astype(F)


def lightmap_sample_lod(values, mips, cover, lods, coords, uvs, texels, width, height, channels=3, pass_of=None, levels=None, chart_radius=np.inf,
                        vertices=None, points=None):
    """[n, channels + 1] rows of 32-bit words (as float32; the last word is the count) as sol_lightmap_sample_lod writes them."""
    W, H, ch = int(width), int(height), int(channels)
    nl, ws, hs, offsets, total_rows = mip_layout(W, H, levels)
    coords = np.asarray(coords)
    n = len(coords)
    uv_rows = np.asarray(uvs, dtype=F).reshape(-1, 6)
    nt = len(uv_rows)
    guard = vertices is not None and points is not None and bool(np.isfinite(F(chart_radius)))
    with np.errstate(all="ignore"):
        # level 0: the existing restatement, with the chart guard
        r0 = sr.lightmap_sample(values, coords, uvs, texels, W, H, channels=ch, pass_of=pass_of, chart_radius=chart_radius, vertices=vertices, points=points)
        a0, c0 = r0[:, :ch], r0[:, ch].view(np.uint32)
        answers, oks, counts = [a0], [c0 > 0], [c0]
        # the row, as sol_lightmap_sample judges it
        tri, b1, b2 = coords["triangle"], coords["b1"].astype(F), coords["b2"].astype(F)
        valid = (coords["flags"] != 0) & (tri != NONE) & (tri < nt) & finite(b1) & finite(b2)
        g = np.where(valid, tri, 0).astype(np.int64)
        uv = (uv_rows if nt else np.zeros((1, 6), dtype=F))[g]
        valid &= finite(uv).all(axis=1)
        if guard:
            vx = np.asarray(vertices, dtype=F).reshape(-1, 9)
            valid &= finite((vx if nt else np.zeros((1, 9), dtype=F))[g]).all(axis=1)
        b0 = (ONE - b1) - b2
        u = ((uv[:, 0] * b0) + (uv[:, 2] * b1)) + (uv[:, 4] * b2)
        v = ((uv[:, 1] * b0) + (uv[:, 3] * b1)) + (uv[:, 5] * b2)
        if nl > 1:
            chain = np.ascontiguousarray(mips).view(np.uint32).reshape(total_rows, -1)
            cov = np.asarray(cover, dtype=np.uint8).reshape(-1)
        for l in range(1, nl):
            lo, hi = offsets[l], offsets[l] + ws[l] * hs[l]
            a, ok, c = _level_lookup(l, chain[lo:hi], cov[lo:hi], ws[l], hs[l], u, v, valid, W, H, ch)
            answers.append(a), oks.append(ok), counts.append(c)
        A, OK, CNT = np.stack(answers), np.stack(oks), np.stack(counts)
        lam = clamp_lod(lods, nl)
        lf = np.floor(lam)
        f = lam - lf
        l0 = lf.astype(np.int64)
        l1 = np.minimum(l0 + 1, nl - 1)
        two = f != 0
        rows = np.arange(n)
        a, ok_a, n_a = A[l0, rows], OK[l0, rows], CNT[l0, rows]
        b, ok_b, n_b = A[l1, rows], OK[l1, rows] & two, np.where(two, CNT[l1, rows], 0)
        gq = ONE - f
        blend = (a * gq[:, None]) + (b * f[:, None])
        assert blend.dtype == F
        out = np.zeros((n, ch + 1), dtype=np.uint32)
        both, only_a, only_b = ok_a & ok_b, ok_a & ~ok_b, ok_b & ~ok_a
        out[both, :ch] = blend[both].view(np.uint32)
        out[only_a, :ch] = a[only_a].view(np.uint32)
        out[only_b, :ch] = b[only_b].view(np.uint32)
        out[:, ch] = np.where(ok_a, n_a, 0) + np.where(ok_b, n_b, 0)
    return out.view(F)


def plog2(q):
    """the piecewise-linear logarithm from the bits of q"""
    bits = np.asarray(q, dtype=F).view(np.uint32)
    e = ((bits >> np.uint32(23)).astype(np.int64) - 127).astype(F)
    m = (bits & np.uint32(0x7FFFFF)).astype(F) * F(2.0 ** -23)
    return e + m


def _len2(a):
    return ((a[0] * a[0]) + (a[1] * a[1])) + (a[2] * a[2])


def lightmap_lod(rays, hits, coords, vertices, uvs, width, height, spread, bias=0.0):
    """[n] float32 as sol_lightmap_lod writes them. rays: [n, 8] float32; hits: sr.HIT_DTYPE; coords: sr.TEXEL_DTYPE."""
    rays, hits, coords = np.asarray(rays, dtype=F).reshape(-1, 8), np.asarray(hits), np.asarray(coords)
    vx, uv = np.asarray(vertices, dtype=F).reshape(-1, 9), np.asarray(uvs, dtype=F).reshape(-1, 6)
    nt = len(vx)
    spread, bias, fw, fh = F(spread), F(bias), F(int(width)), F(int(height))
    with np.errstate(all="ignore"):
        t = hits["t"].astype(F)
        tri = coords["triangle"]
        ok = (hits["status"] == RAY_HIT) & (coords["flags"] != 0) & (tri != NONE) & (tri < nt) & finite(t) & (t > 0)
        ok &= finite(rays[:, 0:3]).all(axis=1) & finite(rays[:, 4:7]).all(axis=1)
        g = np.where(ok, tri, 0).astype(np.int64)
        P = (vx if nt else np.zeros((1, 9), dtype=F))[g]
        T = (uv if nt else np.zeros((1, 6), dtype=F))[g]
        ok &= finite(P).all(axis=1) & finite(T).all(axis=1)
        ax, ay, bx, by, cx, cy = T[:, 0] * fw, T[:, 1] * fh, T[:, 2] * fw, T[:, 3] * fh, T[:, 4] * fw, T[:, 5] * fh
        area2 = ((bx - ax) * (cy - ay)) - ((by - ay) * (cx - ax))
        ok &= (area2 != 0) & finite(area2)
        a = np.where(area2 < 0, -area2, area2)
        e1, e2 = [P[:, 3 + k] - P[:, k] for k in range(3)], [P[:, 6 + k] - P[:, k] for k in range(3)]
        N = ((e1[1] * e2[2]) - (e1[2] * e2[1]), (e1[2] * e2[0]) - (e1[0] * e2[2]), (e1[0] * e2[1]) - (e1[1] * e2[0]))
        D = (rays[:, 4], rays[:, 5], rays[:, 6])
        nn, dd = _len2(N), _len2(D)
        en = nn.view(np.uint32) & np.uint32(0x7F800000)
        ok &= (en != 0) & (en != np.uint32(0x7F800000))
        dn = ((D[0] * N[0]) + (D[1] * N[1])) + (D[2] * N[2])
        c2 = (dn * dn) / (dd * nn)
        c2 = np.where(c2 >= F(1 / 64), c2, F(1 / 64))
        r = spread * t
        q = ((r * r) * (a / np.sqrt(nn))) / c2
        lam = np.where(q > 1, bias + (HALF * plog2(q)), bias)
        assert lam.dtype == F and q.dtype == F
        out = np.where(ok & (lam > 0), lam, ZERO).astype(F)
    return out
