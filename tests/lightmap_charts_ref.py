"""The rule of sol_lightmap_charts, sol_lightmap_dilate_charts, sol_lightmap_sample_charts and sol_lightmap_chart_levels (include/solstrale_hip.h,
DESIGN.md 32) restated in numpy. It is the yardstick of tests/test_lightmap_charts_abi.py and tests/test_gpu_lightmap_charts.py and shares no code
with the device: every float operation below is one float32 operation, in the order the header states, so the device's words can be compared bit
for bit. The neighbour order of the dilation is tests/lightmap_ref.py's, the lookup is tests/lightmap_sample_ref.py's and the layout of the levels
tests/lightmap_mips_ref.py's - imported, not restated."""
import numpy as np

import lightmap_mips_ref as mr
import lightmap_ref as lr
import lightmap_sample_ref as sr

F = np.float32
NONE = 0xFFFFFFFF
MIXED = 0xFFFFFFFE
MAX_LEVELS = mr.MAX_LEVELS
MAX_TRIANGLES = 1 << 30
finite = sr.finite


# ---- the labelling --------------------------------------------------------------------------------------------------------------------------
def edge_keys(uvs, vertices=None):
    """([n, 3, 2 * k] uint32 keys, [n] bool live): edge e joins corners e and (e + 1) % 3; an end point is (u, v) or (u, v, x, y, z), every word
    x + 0.0f; the lower end point - the first differing word, as an unsigned integer, is smaller - comes first."""
    uvs = np.asarray(uvs, dtype=F).reshape(-1, 3, 2)
    n = len(uvs)
    words = uvs
    live = finite(uvs).reshape(n, 6).all(axis=1)
    if vertices is not None:
        vx = np.asarray(vertices, dtype=F).reshape(-1, 3, 3)
        assert len(vx) == n
        words = np.concatenate([uvs, vx], axis=2)
        live &= finite(vx).reshape(n, 9).all(axis=1)
    with np.errstate(all="ignore"):
        canon = np.ascontiguousarray((words + F(0)).astype(F)).view(np.uint32)  # -0 -> +0
    k = canon.shape[2]
    keys = np.zeros((n, 3, 2 * k), dtype=np.uint32)
    for e in range(3):
        a, b = canon[:, e], canon[:, (e + 1) % 3]
        differ = a != b
        first = np.argmax(differ, axis=1)  # (0 where they are equal: no swap then)
        rows = np.arange(n)
        swap = differ.any(axis=1) & (b[rows, first] < a[rows, first])
        keys[:, e, :k] = np.where(swap[:, None], b, a)
        keys[:, e, k:] = np.where(swap[:, None], a, b)
    return keys, live


def lightmap_charts(uvs, vertices=None):
    """(chart_of_triangle [n] uint32, n_charts) as sol_lightmap_charts writes them."""
    keys, live = edge_keys(uvs, vertices)
    n = len(live)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    idx = np.nonzero(live)[0]
    if len(idx):
        flat = keys[idx].reshape(len(idx) * 3, -1)
        tri = np.repeat(idx, 3)
        _, group = np.unique(flat, axis=0, return_inverse=True)
        group = np.asarray(group).reshape(-1)
        order = np.argsort(group, kind="stable")
        g, t = group[order], tri[order]
        for p in np.nonzero(g[1:] == g[:-1])[0]:  # neighbours within a run of equal keys: the run becomes one set
            a, b = find(int(t[p])), find(int(t[p + 1]))
            if a != b:
                parent[max(a, b)] = min(a, b)  # the root of a set is its lowest index
    chart = np.full(n, NONE, dtype=np.uint32)
    roots = np.asarray([find(int(x)) for x in idx], dtype=np.int64)
    lowest = np.unique(roots)  # sorted: the rank of a root among the roots
    chart[idx] = np.searchsorted(lowest, roots).astype(np.uint32)
    return chart, len(lowest)


# ---- the dilation ---------------------------------------------------------------------------------------------------------------------------
def _shift(plane, di, dj, fill):
    """plane seen from each texel at its neighbour (i + di, j + dj); `fill` outside the atlas"""
    H, W = plane.shape[:2]
    out = np.full_like(plane, fill)
    dst = (slice(max(0, -dj), H - max(0, dj)), slice(max(0, -di), W - max(0, di)))
    src = (slice(max(0, dj), H - max(0, -dj)), slice(max(0, di), W - max(0, -di)))
    out[dst] = plane[src]
    return out


def lightmap_dilate_charts(values, texels, chart_of_triangle, width, height, passes=1, channels=3):
    """(out, pass_of [H, W] uint8, chart plane [H, W] uint32) as sol_lightmap_dilate_charts writes them."""
    W, H = int(width), int(height)
    words = np.ascontiguousarray(values).view(np.uint32).reshape(W * H, -1)
    chart_of = np.asarray(chart_of_triangle, dtype=np.uint32).reshape(-1)
    tri = np.asarray(texels)["triangle"].astype(np.int64)
    in_range = tri < len(chart_of)
    chart = np.full(W * H, NONE, dtype=np.uint32)
    chart[in_range] = chart_of[tri[in_range]]
    owned = chart != NONE
    out = np.zeros_like(words)
    out[owned] = words[owned]
    outf = out.view(F).reshape(H, W, -1)
    plane = chart.reshape(H, W).copy()
    pass_of = np.where(owned, 0, 255).astype(np.uint8).reshape(H, W)
    with np.errstate(all="ignore"):
        for p in range(1, int(passes) + 1):
            cov = pass_of != 255
            nb_cov = [_shift(cov, di, dj, False) for di, dj in lr.NEIGHBOURS]
            nb_chart = [np.where(c, _shift(plane, di, dj, NONE), NONE) for c, (di, dj) in zip(nb_cov, lr.NEIGHBOURS)]
            fill = ~cov & np.any(nb_cov, axis=0)
            if not fill.any():
                break
            # the vote: the chart most covered neighbours hold, the lowest id on a tie
            best, best_n = np.full((H, W), NONE, dtype=np.uint32), np.zeros((H, W), dtype=np.int32)
            for k in range(8):
                n_k = np.zeros((H, W), dtype=np.int32)
                for q in range(8):
                    n_k += nb_cov[q] & nb_cov[k] & (nb_chart[q] == nb_chart[k])
                better = nb_cov[k] & ((n_k > best_n) | ((n_k == best_n) & (nb_chart[k] < best)))
                best, best_n = np.where(better, nb_chart[k], best), np.where(better, n_k, best_n)
            s = np.zeros((H, W, channels), dtype=F)
            for k, (di, dj) in enumerate(lr.NEIGHBOURS):
                take = nb_cov[k] & (nb_chart[k] == best)
                nb_val = _shift(outf[..., :channels], di, dj, F(0))
                s = np.where(take[..., None], s + nb_val, s)
            assert s.dtype == F
            outf[fill, :channels] = s[fill] / best_n[fill, None].astype(F)
            plane[fill] = best[fill]
            pass_of[fill] = p
    return out.view(np.asarray(values).dtype).reshape(np.asarray(values).shape), pass_of, plane


# ---- the lookup -----------------------------------------------------------------------------------------------------------------------------
def lightmap_sample_charts(values, coords, uvs, texels, chart_of_triangle, chart_plane, width, height, channels=3, pass_of=None, nearest=False):
    """[n, channels + 1] rows as sol_lightmap_sample_charts writes them: per chart the lookup of tests/lightmap_sample_ref.py over a coverage plane
    in which only that chart's texels are covered; a row whose triangle has no chart answers zeros."""
    W, H, ch = int(width), int(height), int(channels)
    coords, texels = np.asarray(coords), np.asarray(texels)
    chart_of = np.asarray(chart_of_triangle, dtype=np.uint32).reshape(-1)
    plane = np.asarray(chart_plane, dtype=np.uint32).reshape(-1)
    covered = (np.asarray(pass_of).reshape(-1) != 255) if pass_of is not None else (texels["triangle"] != NONE)
    tri = coords["triangle"].astype(np.int64)
    row_chart = np.full(len(coords), NONE, dtype=np.uint32)
    ok = tri < len(chart_of)
    row_chart[ok] = chart_of[tri[ok]]
    out = np.zeros((len(coords), ch + 1), dtype=F)
    for c in np.unique(row_chart):
        if c == NONE:
            continue
        rows = np.nonzero(row_chart == c)[0]
        cover_c = np.where(covered & (plane == c), 0, 255).astype(np.uint8)
        out[rows] = sr.lightmap_sample(values, coords[rows], uvs, texels, W, H, channels=ch, pass_of=cover_c, nearest=nearest)
    return out


# ---- the levels -----------------------------------------------------------------------------------------------------------------------------
def _merge(acc, s):
    """one more source plane `s` (NONE: not live) into the reduction `acc`"""
    out = np.where(s == NONE, acc, np.where(acc == NONE, s, np.where((acc == s) & (s != MIXED), acc, MIXED)))
    return out.astype(np.uint32)


def chart_level_planes(chart_plane, width, height, pass_of=None):
    """the list of level planes [H_l, W_l] uint32 (chart, NONE or MIXED), level 0 first"""
    W, H = int(width), int(height)
    plane = np.asarray(chart_plane, dtype=np.uint32).reshape(H, W).copy()
    if pass_of is not None:
        plane[np.asarray(pass_of).reshape(H, W) == 255] = NONE
    n, ws, hs, _, _ = mr.mip_layout(W, H)
    planes = [plane]
    for l in range(1, n):
        Ws, Hs, Wd, Hd = ws[l - 1], hs[l - 1], ws[l], hs[l]
        src = np.full((2 * Hd, 2 * Wd), NONE, dtype=np.uint32)  # (a source outside level l - 1 is not there)
        src[:Hs, :Ws] = planes[-1]
        acc = np.full((Hd, Wd), NONE, dtype=np.uint32)
        for t in range(4):
            acc = _merge(acc, src[(t >> 1)::2, (t & 1)::2])
        planes.append(acc)
    return planes


def lightmap_chart_levels(chart_plane, width, height, pass_of=None):
    """(levels, mixed_texels [MAX_LEVELS] uint32, mixed_windows [MAX_LEVELS] uint32) as sol_lightmap_chart_levels writes them."""
    planes = chart_level_planes(chart_plane, width, height, pass_of)
    mixed_texels, mixed_windows = np.zeros(MAX_LEVELS, dtype=np.uint32), np.zeros(MAX_LEVELS, dtype=np.uint32)
    for l in range(1, len(planes)):
        P = planes[l]
        Hl, Wl = P.shape
        mixed_texels[l] = (P == MIXED).sum()
        pad = np.full((Hl + 1, Wl + 1), NONE, dtype=np.uint32)
        pad[:Hl, :Wl] = P
        Hw, Ww = max(Hl - 1, 1), max(Wl - 1, 1)
        acc = np.full((Hw, Ww), NONE, dtype=np.uint32)
        for t in range(4):
            acc = _merge(acc, pad[(t >> 1):(t >> 1) + Hw, (t & 1):(t & 1) + Ww])
        mixed_windows[l] = (acc == MIXED).sum()
    levels = 1
    while levels < len(planes) and mixed_texels[levels] == 0 and mixed_windows[levels] == 0:
        levels += 1
    return levels, mixed_texels, mixed_windows
