"""The rule of sol_lightmap_coords and sol_lightmap_sample (include/solstrale_hip.h) restated in numpy float32, vectorised over the
rows. It is the yardstick of tests/test_lightmap_sample_abi.py and tests/test_gpu_lightmap_sample.py and shares no code with the device: every
operation below is one float32 operation, in the order the header states, so the device's words can be compared bit for bit."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
TEXEL_DTYPE = np.dtype([("triangle", np.uint32), ("b1", np.float32), ("b2", np.float32), ("flags", np.uint32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("status", np.uint32), ("kind", np.uint32), ("dfs_index", np.uint32),
                      ("material", np.uint32), ("reserved", np.uint32)])
RAY_HIT, REF_QUAD, REF_TRIANGLE = 1, 3, 4
ROTATION_SHIFT, TRIANGLE_MASK = 30, 0x3FFFFFFF
ONE, HALF, ZERO = F(1), F(0.5), F(0)


def finite(x):
    """the exponent field is not all ones - elementwise on float32"""
    return (np.asarray(x, dtype=F).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def lightmap_coords(hits, triangle_of_dfs):
    """The surface rows of `hits` (HIT_DTYPE) through the table (uint32: triangle | rotation << 30, or NONE)."""
    hits = np.asarray(hits)
    table = np.asarray(triangle_of_dfs, dtype=np.uint32).reshape(-1)
    n = len(hits)
    out = np.zeros(n, dtype=TEXEL_DTYPE)
    out["triangle"] = NONE
    listed = (hits["status"] == RAY_HIT) & (hits["kind"] == REF_TRIANGLE) & (hits["dfs_index"] < len(table))
    entry = np.full(n, NONE, dtype=np.uint32)
    entry[listed] = table[hits["dfs_index"][listed]]
    k = entry >> np.uint32(ROTATION_SHIFT)
    ok = listed & (k != 3)
    with np.errstate(all="ignore"):
        u, v = hits["u"].astype(F), hits["v"].astype(F)
        w = (ONE - u) - v
    b1 = np.where(k == 0, u, np.where(k == 1, w, v))
    b2 = np.where(k == 0, v, np.where(k == 1, u, w))
    out["triangle"][ok] = entry[ok] & np.uint32(TRIANGLE_MASK)
    out["b1"][ok], out["b2"][ok], out["flags"][ok] = b1[ok], b2[ok], 1
    return out


def _lerp3(a0, a1, a2, b0, b1, b2):
    return ((a0 * b0) + (a1 * b1)) + (a2 * b2)


def lightmap_sample(values, coords, uvs, texels, width, height, channels=3, pass_of=None, nearest=False, chart_radius=np.inf, vertices=None, points=None,
                    return_taps=False):
    """[n, channels + 1] rows of 32-bit words (as float32; the last word is the count) as sol_lightmap_sample writes them. values: [W * H, k] rows of
    32-bit words whose leading `channels` are floats. return_taps: also the [n, 4] bool plane of the live taps (before the wsum > 0 test)."""
    W, H, ch = int(width), int(height), int(channels)
    val = np.ascontiguousarray(values).view(F).reshape(W * H, -1)[:, :ch]
    coords, texels = np.asarray(coords), np.asarray(texels)
    uvs = np.asarray(uvs, dtype=F).reshape(-1, 6)
    n, nt = len(coords), len(uvs)
    guard = vertices is not None and points is not None and bool(np.isfinite(F(chart_radius)))
    out = np.zeros((n, ch + 1), dtype=np.uint32)
    taps_live = np.zeros((n, 4), dtype=bool)
    with np.errstate(all="ignore"):
        tri, b1, b2 = coords["triangle"], coords["b1"].astype(F), coords["b2"].astype(F)
        valid = (coords["flags"] != 0) & (tri != NONE) & (tri < nt) & finite(b1) & finite(b2)
        g = np.where(valid, tri, 0).astype(np.int64)
        if nt == 0:
            uvs = np.zeros((1, 6), dtype=F)
        uv = uvs[g]
        valid &= finite(uv).all(axis=1)
        b0 = (ONE - b1) - b2
        if guard:
            vx = np.asarray(vertices, dtype=F).reshape(-1, 9)
            if nt == 0:
                vx = np.zeros((1, 9), dtype=F)
            vx = vx[g]
            valid &= finite(vx).all(axis=1)
            P = [_lerp3(vx[:, a], vx[:, 3 + a], vx[:, 6 + a], b0, b1, b2) for a in range(3)]
        u = _lerp3(uv[:, 0], uv[:, 2], uv[:, 4], b0, b1, b2)
        v = _lerp3(uv[:, 1], uv[:, 3], uv[:, 5], b0, b1, b2)
        fw, fh = F(W), F(H)
        if nearest:
            x, y = u * fw, v * fh
            inside = valid & (x >= 0) & (x < fw) & (y >= 0) & (y < fh)
            n_taps = 1
        else:
            x, y = (u * fw) - HALF, (v * fh) - HALF
            inside = valid & (x >= -1) & (x < fw) & (y >= -1) & (y < fh)
            n_taps = 4
        xf, yf = np.floor(np.where(inside, x, ZERO)), np.floor(np.where(inside, y, ZERO))
        i0, j0 = xf.astype(np.int64), yf.astype(np.int64)
        fx, fy = np.where(inside, x, ZERO) - xf, np.where(inside, y, ZERO) - yf
        weights, index = [], []
        r2 = F(chart_radius) * F(chart_radius) if guard else None
        for k in range(n_taps):
            i, j = i0 + (k & 1), j0 + (k >> 1)
            live = inside & (i >= 0) & (j >= 0) & (i < W) & (j < H)
            at = np.where(live, j * W + i, 0)
            live &= (np.asarray(pass_of).reshape(-1)[at] != 255) if pass_of is not None else (texels["triangle"][at] != NONE)
            live &= finite(val[at]).all(axis=1)
            if guard:
                q = np.asarray(points, dtype=F).reshape(W * H, 8)[at, :3]
                tested = (texels["flags"][at] != 0) & finite(q).all(axis=1)
                e = [q[:, a] - P[a] for a in range(3)]
                d2 = ((e[0] * e[0]) + (e[1] * e[1])) + (e[2] * e[2])
                live &= ~tested | (d2 <= r2)
            wx, wy = (fx if k & 1 else ONE - fx), (fy if k >> 1 else ONE - fy)
            weights.append(wx * wy)
            index.append(at)
            taps_live[:, k] = live
        if nearest:
            got = taps_live[:, 0]
            out[got, :ch] = val[index[0][got]].view(np.uint32)
            out[:, ch] = got
        else:
            wsum = np.zeros(n, dtype=F)
            total = np.zeros((n, ch), dtype=F)
            for k in range(4):
                live = taps_live[:, k]
                wsum = np.where(live, wsum + weights[k], wsum)
                total = np.where(live[:, None], total + (weights[k][:, None] * val[index[k]]), total)
            ok = wsum > 0
            answer = total / wsum[:, None]
            assert answer.dtype == F and wsum.dtype == F
            out[ok, :ch] = answer[ok].view(np.uint32)
            out[:, ch] = np.where(ok, taps_live.sum(axis=1), 0)
    rows = out.view(F)
    return (rows, taps_live) if return_taps else rows
