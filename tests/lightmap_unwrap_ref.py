"""The rule of sol_lightmap_unwrap (include/solstrale_hip.h) restated in numpy. It is the yardstick of
tests/test_lightmap_unwrap_abi.py and tests/test_gpu_lightmap_unwrap.py and shares no code with the device: every float operation below is one
float32 operation, in the order the header states, so the device's words can be compared bit for bit. The canonical edge words are
tests/lightmap_charts_ref.py's - imported, not restated. The packing is written the way the device computes it (prefix sums, the first rectangle
that no longer fits, the orbit of 0); tests/test_lightmap_unwrap_abi.py sets it beside the sequential loop. Also the meshes the two tests share."""
import numpy as np

import lightmap_charts_ref as cr
import lightmap_ref as lr

F = np.float32
NONE = 0xFFFFFFFF
MAX_SIZE = 16384
MAX_CONTENT = 32767
MAX_GUTTER = 64
OVERFLOW_WIDTH, OVERFLOW_HEIGHT = 1, 2
RESULT_DTYPE = np.dtype([("n_charts", np.uint32), ("live_triangles", np.uint32), ("used_width", np.uint32), ("used_height", np.uint32),
                         ("overflow", np.uint32), ("reserved", np.uint32), ("content_texels", np.uint64)])


# ---- triangles and charts -------------------------------------------------------------------------------------------------------------------
def triangle_classes(vertices):
    """([n] bool live, [n] class 2 a + s, [n, 3] float32 unit normals) of [n, 3, 3] positions."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3, 3)
    n = len(v)
    with np.errstate(all="ignore"):
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        nx, ny, nz = lr._cross((e1[:, 0], e1[:, 1], e1[:, 2]), (e2[:, 0], e2[:, 1], e2[:, 2]))
        nrm = np.stack([nx, ny, nz], axis=1).astype(F)
        d = lr._len2((nx, ny, nz))
        assert d.dtype == F
        live = cr.finite(v).reshape(n, 9).all(axis=1) & lr._normal(d)
        mag = np.where(live[:, None], np.abs(nrm), F(0))
        a = np.argmax(mag, axis=1)  # (the first of equal maxima: the lowest index)
        s = nrm[np.arange(n), a] < 0
        unit = (nrm / np.sqrt(d)[:, None]).astype(F)
    return live, (2 * a + s).astype(np.uint32), unit


def lightmap_unwrap_charts(vertices, crease_cos=-1.0):
    """(chart_of_triangle [n] uint32 - before any overflow -, n_charts, live, class): two live triangles are joined when they share an edge
    (equal canonical position words), have the same class and dot(unit_a, unit_b) >= crease_cos; every pair on an edge is judged."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3, 3)
    n = len(v)
    live, cls, unit = triangle_classes(v)
    keys, _ = cr.edge_keys(np.zeros((n, 3, 2), dtype=F), v)
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    cc = F(crease_cos)
    idx = np.nonzero(live)[0]
    if len(idx):
        flat = keys[idx].reshape(len(idx) * 3, -1)
        tri = np.repeat(idx, 3)
        _, group = np.unique(flat, axis=0, return_inverse=True)
        group = np.asarray(group).reshape(-1)
        order = np.argsort(group, kind="stable")
        g, t = group[order], tri[order]
        starts = np.nonzero(np.r_[True, g[1:] != g[:-1]])[0]
        ends = np.r_[starts[1:], len(g)]
        for s, e in zip(starts, ends):
            for p in range(s, e):
                for q in range(s, p):
                    a, b = int(t[p]), int(t[q])
                    if cls[a] != cls[b]:
                        continue
                    dot = (unit[a, 0] * unit[b, 0] + unit[a, 1] * unit[b, 1]) + unit[a, 2] * unit[b, 2]
                    assert dot.dtype == F
                    if not dot >= cc:
                        continue
                    ra, rb = find(a), find(b)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
    chart = np.full(n, NONE, dtype=np.uint32)
    roots = np.asarray([find(int(x)) for x in idx], dtype=np.int64)
    lowest = np.unique(roots)
    chart[idx] = np.searchsorted(lowest, roots).astype(np.uint32)
    return chart, len(lowest), live, cls


# ---- projection, extents, packing -----------------------------------------------------------------------------------------------------------
def project(vertices, cls, texels_per_unit):
    """[n, 3, 2] float32: corner c of triangle t at (p[(a + 1) % 3], p[(a + 2) % 3]) * texels_per_unit + 0"""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3, 3)
    a = (np.asarray(cls) >> 1).astype(np.int64)
    rows = np.arange(len(v))[:, None]
    with np.errstate(all="ignore"):
        x = (v[rows, np.arange(3)[None, :], ((a + 1) % 3)[:, None]] * F(texels_per_unit)) + F(0)
        y = (v[rows, np.arange(3)[None, :], ((a + 2) % 3)[:, None]] * F(texels_per_unit)) + F(0)
    out = np.stack([x, y], axis=-1)
    assert out.dtype == F
    return out


def content_extent(lo, hi):
    """(content texels [m] int64, floor(lo) [m] float32): e = (floor(hi) + 1) - floor(lo), e + 2 with the guards, 32767 outside 1 .. 32765"""
    with np.errstate(all="ignore"):
        f = np.floor(lo).astype(F)
        e = (np.floor(hi).astype(F) + F(1)) - f
        ok = (e >= F(1)) & (e <= F(32765))
        return np.where(ok, np.where(ok, e, F(1)).astype(np.int64) + 2, MAX_CONTENT), f


def sort_order(w, h):
    """the order the rectangles are walked in: height descending, width descending, id ascending - one 64-bit key"""
    w, h = np.asarray(w, dtype=np.uint64), np.asarray(h, dtype=np.uint64)
    key = ((np.uint64(0xFFFF) - h) << np.uint64(46)) | ((np.uint64(0xFFFF) - w) << np.uint64(30)) | np.arange(len(w), dtype=np.uint64)
    return np.argsort(key, kind="stable")


def pack(w, h, width, height):
    """The greedy shelf rule over rectangles (w, h) by id, as the device computes it. Returns (x [m], y [m] by id - of the rectangles the walk
    reached -, reached [m] bool, used_width, used_height, overflow)."""
    w, h = np.asarray(w, dtype=np.int64), np.asarray(h, dtype=np.int64)
    m = len(w)
    order = sort_order(w, h)
    sw, sh = w[order], h[order]
    prefix = np.cumsum(sw)  # prefix[i]: the widths 0 .. i added
    base = np.r_[0, prefix[:-1]] if m else prefix
    nxt = np.minimum(np.maximum(np.searchsorted(prefix, base + int(width), side="right"), np.arange(m) + 1), m)
    x, y, reached = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=bool)
    i, top, used_w = 0, 0, 0
    while i < m:
        j = int(nxt[i])
        used_w = max(used_w, int(prefix[j - 1] - base[i]))
        x[order[i:j]] = base[i:j] - base[i]
        y[order[i:j]] = top
        reached[order[i:j]] = True
        top += int(sh[i])
        i = j
        if top > MAX_SIZE:
            break
    overflow = (OVERFLOW_WIDTH if m and int(w.max()) > int(width) else 0) | (OVERFLOW_HEIGHT if top > int(height) else 0)
    return x, y, reached, used_w, top, overflow


# ---- the call -------------------------------------------------------------------------------------------------------------------------------
def lightmap_unwrap(vertices, width, height, texels_per_unit, gutter=2, crease_cos=-1.0, detail=False):
    """(uvs [n, 3, 2] float32, chart_of_triangle [n] uint32, result - one RESULT_DTYPE record) as sol_lightmap_unwrap writes them. detail: also
    a dict of what lies between (the labels before overflow, the rectangles by chart id)."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3, 3)
    n, W, H, g = len(v), int(width), int(height), int(gutter)
    result = np.zeros((), dtype=RESULT_DTYPE)
    uvs = np.zeros((n, 3, 2), dtype=F)
    if n == 0:
        return (uvs, np.zeros(0, dtype=np.uint32), result) + (({},) if detail else ())
    chart, m, live, cls = lightmap_unwrap_charts(v, crease_cos)
    xy = project(v, cls, texels_per_unit)
    idx = np.nonzero(live)[0]
    lo, hi = np.full((m, 2), np.inf, dtype=F), np.full((m, 2), -np.inf, dtype=F)
    for c in range(3):
        np.minimum.at(lo, chart[idx], xy[idx, c])
        np.maximum.at(hi, chart[idx], xy[idx, c])
    cw, fx = content_extent(lo[:, 0], hi[:, 0])
    ch, fy = content_extent(lo[:, 1], hi[:, 1])
    x, y, reached, used_w, used_h, overflow = pack(cw + g, ch + g, W, H)
    result["n_charts"], result["live_triangles"] = m, len(idx)
    result["used_width"], result["used_height"], result["overflow"] = used_w, used_h, overflow
    result["content_texels"] = int((cw * ch).sum())
    labels = chart.copy()
    if overflow:
        labels[:] = NONE
    else:
        c = chart[idx]
        with np.errstate(all="ignore"):
            u = ((xy[idx, :, 0] - fx[c][:, None]) + (x[c] + 1).astype(F)[:, None]) / F(W)
            w = ((xy[idx, :, 1] - fy[c][:, None]) + (y[c] + 1).astype(F)[:, None]) / F(H)
        assert u.dtype == F and w.dtype == F
        uvs[idx, :, 0], uvs[idx, :, 1] = u, w
    if detail:
        return uvs, labels, result, {"chart": chart, "cw": cw, "ch": ch, "x": x, "y": y, "cls": cls, "live": live, "xy": xy, "fx": fx, "fy": fy}
    return uvs, labels, result


def result_words(result):
    """a result record (the restatement's or the device's) as its eight 32-bit words"""
    return np.ascontiguousarray(np.asarray(result, dtype=RESULT_DTYPE).reshape(1)).view(np.uint32).copy()


# ---- meshes the tests share --------------------------------------------------------------------------------------------------------------
def cube(size=1.0):
    """12 triangles, two per face, faces sharing their edges' positions"""
    s = F(size)
    c = np.asarray([[x, y, z] for x in (0, s) for y in (0, s) for z in (0, s)], dtype=F)  # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, d, e in quads:
        tris += [[c[a], c[b], c[d]], [c[a], c[d], c[e]]]
    return np.asarray(tris, dtype=F)


def grid(cells, seed=1, jitter=0.3, bump=0.0, size=4.0):
    """cells x cells quads in the plane y = 0 (two triangles each), the inner points jittered; bump: the height of a sine field over it"""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, cells + 1)
    u, w = np.meshgrid(g, g)
    inner = (slice(1, -1), slice(1, -1))
    u[inner] += rng.uniform(-jitter, jitter, u[inner].shape) / cells
    w[inner] += rng.uniform(-jitter, jitter, w[inner].shape) / cells
    hgt = bump * np.sin(7.0 * u) * np.cos(5.0 * w)
    p = np.stack([u * size, hgt, w * size], axis=-1).astype(F)
    tris = []
    for j in range(cells):
        for i in range(cells):
            for a, b, c in (((j, i), (j, i + 1), (j + 1, i + 1)), ((j, i), (j + 1, i + 1), (j + 1, i))):
                tris.append([p[a], p[b], p[c]])
    return np.asarray(tris, dtype=F)


def fin():
    """three triangles on one edge: two in the plane y = 0 on either side of it, one standing on it"""
    a, b = [0, 0, 0], [0, 0, 1]
    return np.asarray([[a, b, [1, 0, 0.5]], [b, a, [-1, 0, 0.5]], [a, b, [0.1, 1, 0.5]]], dtype=F)


def disjoint(n, seed=2, sizes=(0.2, 0.45, 0.7)):
    """n small triangles in the plane y = 0 that share nothing, of a few sizes (equal rectangles, many shelves)"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    s = np.asarray(sizes)[rng.integers(0, len(sizes), n)]
    x0, z0 = (k % 256) * 2.0 + 0.125, (k // 256) * 2.0 + 0.125
    zero = np.zeros(n)
    v = np.stack([np.stack([x0, zero, z0], -1), np.stack([x0, zero, z0 + s], -1), np.stack([x0 + s, zero, z0], -1)], axis=1)
    return v.astype(F)


def with_dead(vertices, seed=3):
    """a copy with a NaN triangle, an infinite one and a zero-area one put in"""
    v = np.array(vertices, dtype=F)
    rng = np.random.default_rng(seed)
    at = rng.choice(len(v), 3, replace=False)
    v[at[0], 1, 2] = np.nan
    v[at[1], 0, 0] = np.inf
    v[at[2], 2] = v[at[2], 1]
    return v, at
