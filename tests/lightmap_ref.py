"""The rule of sol_lightmap_points and sol_lightmap_dilate (include/solstrale_hip.h) restated in numpy float32: a plain Python loop
over triangles, vectorised over each triangle's candidate texels. It is the yardstick of tests/test_lightmap_abi.py and
tests/test_gpu_lightmap.py and shares no code with the device: every operation below is one float32 operation, in the order the header states,
so the device's words can be compared bit for bit. Also the meshes those tests share."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
TEXEL_DTYPE = np.dtype([("triangle", np.uint32), ("b1", np.float32), ("b2", np.float32), ("flags", np.uint32)])
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))  # (di, dj) in the order the values are added


def _normal(x):
    """finite, not zero, not subnormal - elementwise on float32"""
    e = np.asarray(x, dtype=F).view(np.uint32) & np.uint32(0x7F800000)
    return (e != 0) & (e != np.uint32(0x7F800000))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _len2(a):
    return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]


def _edge(q, r, px, py):
    """edge(Q, R, P) with (Q, R) in lexicographic order, negated when the triangle's own order is the other one"""
    if q[0] < r[0] or (q[0] == r[0] and q[1] <= r[1]):
        return (r[0] - q[0]) * (py - q[1]) - (r[1] - q[1]) * (px - q[0])
    return -((q[0] - r[0]) * (py - r[1]) - (q[1] - r[1]) * (px - r[0]))


class _Tri:
    """A triangle that is not skipped: its corners in texel space, area2 made positive, `flip`, and its geometric normal."""

    def __init__(self, A, B, C, area2, flip, pos, nrm, geo):
        self.A, self.B, self.C, self.area2, self.flip, self.pos, self.nrm, self.geo = A, B, C, area2, flip, pos, nrm, geo

    def edges(self, px, py):
        e0, e1, e2 = _edge(self.B, self.C, px, py), _edge(self.C, self.A, px, py), _edge(self.A, self.B, px, py)
        return (-e0, -e1, -e2) if self.flip else (e0, e1, e2)


def _setup(uv, pos, nrm, W, H):
    if not (np.isfinite(uv).all() and np.isfinite(pos).all() and (nrm is None or np.isfinite(nrm).all())):
        return None
    fw, fh = F(W), F(H)
    A, B, C = ((uv[k, 0] * fw, uv[k, 1] * fh) for k in range(3))
    area2 = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
    if area2 == 0 or not np.isfinite(area2):
        return None
    geo = _cross(tuple(pos[1] - pos[0]), tuple(pos[2] - pos[0]))
    if not _normal(_len2(geo)):
        return None
    flip = bool(area2 < 0)
    return _Tri(A, B, C, -area2 if flip else area2, flip, pos, nrm, geo)


def _candidates(t, W, H):
    """(i, j) index grids of the texels whose closed square overlaps the triangle's closed bounding box, or None"""
    xs, ys = (t.A[0], t.B[0], t.C[0]), (t.A[1], t.B[1], t.C[1])
    I, J = np.arange(W).astype(F), np.arange(H).astype(F)
    ii = np.nonzero((I <= max(xs)) & (I + F(1) >= min(xs)))[0]
    jj = np.nonzero((J <= max(ys)) & (J + F(1) >= min(ys)))[0]
    if len(ii) == 0 or len(jj) == 0:
        return None
    return np.meshgrid(ii, jj)


def lightmap_owner(vertices, uvs, width, height, normals=None, conservative=False):
    """The owner words: per texel the minimum over all claims of index | (conservative_only << 31); 0xFFFFFFFF: empty. Also the triangles kept."""
    vertices, uvs = np.asarray(vertices, dtype=F), np.asarray(uvs, dtype=F)
    normals = None if normals is None else np.asarray(normals, dtype=F)
    W, H = int(width), int(height)
    owner = np.full(W * H, NONE, dtype=np.uint32)
    tris = {}
    with np.errstate(all="ignore"):
        for g in range(len(vertices)):
            t = _setup(uvs[g], vertices[g], None if normals is None else normals[g], W, H)
            if t is None:
                continue
            tris[g] = t
            cand = _candidates(t, W, H)
            if cand is None:
                continue
            gi, gj = cand
            e0, e1, e2 = t.edges(gi.astype(F) + F(0.5), gj.astype(F) + F(0.5))
            centre = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
            key = np.where(centre, np.uint32(g), np.uint32(NONE))
            if conservative:
                some = [np.zeros(gi.shape, dtype=bool) for _ in range(3)]
                for c in range(4):
                    ce = t.edges((gi + (c & 1)).astype(F), (gj + (c >> 1)).astype(F))
                    for k in range(3):
                        some[k] |= ce[k] >= 0
                key = np.where(~centre & some[0] & some[1] & some[2], np.uint32(g | 0x80000000), key)
            sel = key != NONE
            at = (gj * W + gi)[sel]
            owner[at] = np.minimum(owner[at], key[sel])
    return owner, tris


def lightmap_points(vertices, uvs, width, height, normals=None, tmin=1e-3, tmax=np.inf, conservative=False):
    """(points [H * W, 8] float32, texels [H * W] TEXEL_DTYPE) as sol_lightmap_points writes them."""
    W, H = int(width), int(height)
    owner, tris = lightmap_owner(vertices, uvs, W, H, normals, conservative)
    points = np.zeros((W * H, 8), dtype=F)
    texels = np.zeros(W * H, dtype=TEXEL_DTYPE)
    texels["triangle"] = NONE
    one = F(1)
    with np.errstate(all="ignore"):
        order = np.argsort(owner, kind="stable")  # the texels grouped by their owner word
        keys, first = np.unique(owner[order], return_index=True)
        for key, lo, hi in zip(keys, first, list(first[1:]) + [len(order)]):
            if key == NONE:
                continue
            g, claim = int(key & np.uint32(0x7FFFFFFF)), 2 if key & np.uint32(0x80000000) else 1
            t = tris[g]
            at = order[lo:hi]
            j, i = at // W, at % W
            _, e1, e2 = t.edges(i.astype(F) + F(0.5), j.astype(F) + F(0.5))
            b1, b2 = e1 / t.area2, e2 / t.area2
            b0 = (one - b1) - b2
            if claim == 2:
                c0, c1, c2 = (np.where(b > 0, b, F(0)) for b in (b0, b1, b2))
                s = (c0 + c1) + c2
                b1, b2 = c1 / s, c2 / s
                b0 = (one - b1) - b2
            v = t.pos
            for k in range(3):
                points[at, k] = ((v[0, k] * b0) + (v[1, k] * b1)) + (v[2, k] * b2)
            n = [np.full(len(at), t.geo[k], dtype=F) for k in range(3)]
            if t.nrm is not None:
                m = [((t.nrm[0, k] * b0) + (t.nrm[1, k] * b1)) + (t.nrm[2, k] * b2) for k in range(3)]
                ok = _normal(_len2(m))
                n = [np.where(ok, m[k], n[k]) for k in range(3)]
            length = np.sqrt(_len2(n))
            for k in range(3):
                points[at, 4 + k] = n[k] / length
            points[at, 3], points[at, 7] = F(tmin), F(tmax)
            texels["triangle"][at], texels["b1"][at], texels["b2"][at], texels["flags"][at] = g, b1, b2, claim
    assert points.dtype == F
    return points, texels


def lightmap_dilate(values, texels, width, height, passes=1, channels=3):
    """(out, pass_of [H, W] uint8) as sol_lightmap_dilate writes them; values: [H * W, k] rows of 32-bit words whose leading `channels` are floats."""
    W, H = int(width), int(height)
    words = np.ascontiguousarray(values).view(np.uint32).reshape(W * H, -1)
    owned = (np.asarray(texels)["triangle"] != NONE)
    out = np.zeros_like(words)
    out[owned] = words[owned]
    outf = out.view(F).reshape(H, W, -1)
    pass_of = np.where(owned, 0, 255).astype(np.uint8).reshape(H, W)
    with np.errstate(all="ignore"):
        for p in range(1, int(passes) + 1):
            cov = pass_of != 255
            s = np.zeros((H, W, channels), dtype=F)
            count = np.zeros((H, W), dtype=np.int32)
            for di, dj in NEIGHBOURS:  # the neighbour of (i, j) is (i + di, j + dj); none outside the atlas
                nb_cov = np.zeros((H, W), dtype=bool)
                nb_val = np.zeros((H, W, channels), dtype=F)
                dst = (slice(max(0, -dj), H - max(0, dj)), slice(max(0, -di), W - max(0, di)))
                src = (slice(max(0, dj), H - max(0, -dj)), slice(max(0, di), W - max(0, -di)))
                nb_cov[dst] = cov[src]
                nb_val[dst] = outf[src][..., :channels]
                s = np.where(nb_cov[..., None], s + nb_val, s)
                count += nb_cov
            fill = ~cov & (count > 0)
            if not fill.any():
                break  # (no later pass fills anything either)
            outf[fill, :channels] = s[fill] / count[fill, None].astype(F)
            pass_of[fill] = p
    assert s.dtype == F if passes else True
    return out.view(np.asarray(values).dtype).reshape(np.asarray(values).shape), pass_of


# ---- meshes the tests share --------------------------------------------------------------------------------------------------------------
def grid_mesh(cells, seed, jitter=0.35):
    """A `cells` x `cells` grid of quads tiling [0, 1]^2 in UV, two triangles each, the inner grid points jittered by up to `jitter` of a cell
    (the border stays put, so the mesh covers the square exactly). Positions: the UV plane lifted to a gentle height field; per-corner normals
    of that field. Returns (vertices [n, 3, 3], uvs [n, 3, 2], normals [n, 3, 3]) float32, n = 2 * cells^2."""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, cells + 1)
    u, v = np.meshgrid(g, g)
    inner = (slice(1, -1), slice(1, -1))
    u[inner] += rng.uniform(-jitter, jitter, u[inner].shape) / cells
    v[inner] += rng.uniform(-jitter, jitter, v[inner].shape) / cells
    u, v = u.astype(F), v.astype(F)
    h = (0.1 * np.sin(3.0 * u) * np.cos(2.0 * v)).astype(F)
    p = np.stack([u * 4 - 2, h, v * 4 - 2], axis=-1).astype(F)
    nr = np.stack([-0.3 * np.cos(3.0 * u) * np.cos(2.0 * v) / 4, np.ones_like(u), 0.2 * np.sin(3.0 * u) * np.sin(2.0 * v) / 4], axis=-1).astype(F)
    t = np.stack([u, v], axis=-1)
    V, T, N = [], [], []
    for y in range(cells):
        for x in range(cells):
            for a, b, c in (((y, x), (y, x + 1), (y + 1, x + 1)), ((y, x), (y + 1, x + 1), (y + 1, x))):
                V.append([p[a], p[b], p[c]]); T.append([t[a], t[b], t[c]]); N.append([nr[a], nr[b], nr[c]])
    return np.asarray(V, dtype=F), np.asarray(T, dtype=F), np.asarray(N, dtype=F)


def lift(uvs):
    """Positions for triangles given only by UVs: the UV plane at y = 0, x = 4u - 2, z = 4v - 2."""
    uvs = np.asarray(uvs, dtype=F)
    z = np.zeros(uvs.shape[:-1], dtype=F)
    return np.stack([uvs[..., 0] * F(4) - F(2), z, uvs[..., 1] * F(4) - F(2)], axis=-1).astype(F)
