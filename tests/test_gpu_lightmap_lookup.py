"""The third device-against-device identity of the lightmap lookups (csrc/sol_lightmap_lookup.h): sol_lightmap_sh in coefficient
mode on an atlas of SolSh9 rows answers the 28 words per row that sol_lightmap_sample answers with channels = 27 and a stride of 112 bytes on the
same atlas and rows - eight lanes per row on the shared steps of that header against a lane per row on the sample kernel's own text. (The
other two: the mip lookup at level 0 and the one-chart lookup, tests/test_gpu_lightmap_mips.py and tests/test_gpu_lightmap_charts.py.) Bilinear and
nearest, with the dilation's plane and without, with the chart guard at a finite radius and off. The shape is the smallest at which the two could
part: an atlas of 37 x 29 texels, a third of it unowned, and 32 * 5 + 5 rows - five workgroups of the sh kernel and five rows, past an octet, a
wave and a workgroup of it and past a wave of the sample kernel - with every class of invalid row between good ones, UVs that leave the atlas,
value words that are not finite, and garbage in word 27, which neither call may judge. No reference is needed: the words are compared with each
other; the counts are looked at so that the comparison is about rows of every kind."""
import numpy as np
import pytest

import lightmap_ref as lr
import lightmap_sample_ref as sr
from solstrale_amd import DeviceScene, RenderConfig, scenes
from test_gpu_lightmap_sample import assert_words_equal, texels_tensor
from test_lightmap_sample_abi import invalid_rows

pytestmark = pytest.mark.gpu
F = np.float32
INF, NAN = F(np.inf), F(np.nan)
W, H, N_ROWS = 37, 29, 32 * 5 + 5
RADIUS = 0.12  # texel centres lie 4 / 37 = 0.108 and 4 / 29 = 0.138 apart in the lifted plane: some of a row's four taps are within, some are not


def lookup_case(seed=37):
    """uvs, vertices, texels, points, pass_of, values, rows: made by hand, not rasterised - ownership is a random two thirds of the atlas, an owned
    texel's point is its centre lifted as the vertices are, so that the guard's distances are those between texel centres."""
    rng = np.random.default_rng(seed)
    _, T, _ = lr.grid_mesh(5, 3)
    outside = np.asarray([[(-0.3, 0.2), (0.3, -0.2), (0.2, 0.4)], [(0.8, 0.8), (1.3, 0.9), (0.9, 1.4)], [(1e30, 0.5), (0.5, 1e30), (-1e30, -1e30)]], dtype=F)
    bad = np.asarray([[(0.2, 0.2), (NAN, 0.3), (0.3, 0.8)], [(0.6, 0.2), (0.8, 0.3), (0.7, 0.5)]], dtype=F)  # a UV word, and (below) a vertex word
    uvs = np.concatenate([T, outside, bad])
    nt = len(uvs)
    vertices = lr.lift(np.nan_to_num(np.clip(uvs, -8, 8)))
    vertices[nt - 1, 2, 0] = INF
    owned = rng.random(W * H) < 2 / 3
    texels = np.zeros(W * H, dtype=sr.TEXEL_DTYPE)
    texels["triangle"] = np.where(owned, rng.integers(0, len(T), W * H), sr.NONE)
    texels["b1"], texels["b2"], texels["flags"] = F(0.25), F(0.25), np.where(owned, rng.integers(1, 3, W * H), 0)
    j, i = np.divmod(np.arange(W * H), W)
    points = np.zeros((W * H, 8), dtype=F)
    points[:, 0:3] = lr.lift(np.stack([(i + 0.5) / W, (j + 0.5) / H], axis=-1))
    points[:, 3], points[:, 4:7], points[:, 7] = 1e-3, (0, 1, 0), INF
    points[~owned] = 0
    points[owned & (rng.random(W * H) < 0.05), 1] = NAN  # a position word that is not finite: the guard lets the tap through
    pass_of = np.where(owned, 0, np.where(rng.random(W * H) < 0.5, rng.integers(1, 4, W * H), 255)).astype(np.uint8).reshape(H, W)
    values = (rng.normal(size=(W * H, 28)) * rng.choice([1e-3, 1.0, 1e4], (W * H, 1))).astype(F)
    for word in (0, 13, 26):  # three different lanes of an octet
        spoil = rng.random(W * H) < 0.03
        values[spoil, word] = rng.choice([INF, -INF, NAN], int(spoil.sum()))
    values[:, 27] = np.where(rng.random(W * H) < 0.5, rng.choice([INF, NAN], W * H), rng.integers(0, 1 << 32, W * H, dtype=np.uint32).view(F))
    b = rng.dirichlet((1.0, 1.0, 1.0), N_ROWS).astype(F)
    rows = np.zeros(N_ROWS, dtype=sr.TEXEL_DTYPE)
    rows["triangle"], rows["b1"], rows["b2"], rows["flags"] = rng.integers(0, nt - 2, N_ROWS), b[:, 1], b[:, 2], rng.integers(1, 3, N_ROWS)
    rows["triangle"][::9] = rng.integers(len(T), len(T) + 3, len(rows[::9]))  # UVs that leave the atlas, in part or altogether
    names, invalid = invalid_rows(nt, nt - 2, nt - 1)
    where = 3 + 16 * np.arange(len(invalid))  # each between good rows, two to a workgroup of the sh kernel
    assert where[-1] < N_ROWS - 1
    rows[where] = invalid
    return dict(uvs=uvs, vertices=vertices, texels=texels, points=points, pass_of=pass_of, values=values, rows=rows, invalid=where, names=names)


@pytest.fixture(scope="module")
def case():
    import torch
    with DeviceScene(scenes.cornell_box(RenderConfig(32, 32, 1))) as ds:  # (the geometry of a lookup is the caller's: any handle serves)
        c = lookup_case()
        dev = {k: torch.from_numpy(c[k]).cuda() for k in ("uvs", "vertices", "points", "pass_of", "values")}
        dev["texels"], dev["rows"] = texels_tensor(c["texels"]), texels_tensor(c["rows"])
        yield ds, c, dev


@pytest.mark.parametrize("guard", [False, True], ids=["no guard", "guard 0.12"])
@pytest.mark.parametrize("plane", [False, True], ids=["ownership", "pass_of"])
@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
def test_sh_coefficients_are_the_devices_own_lightmap_sample_of_27_channels(case, nearest, plane, guard):
    ds, c, dev = case
    kw = dict(pass_of=dev["pass_of"] if plane else None, nearest=nearest)
    if guard:
        kw.update(chart_radius=RADIUS, vertices=dev["vertices"], points=dev["points"])
    coeff = ds.lightmap_sh(dev["values"], dev["rows"], None, dev["uvs"], dev["texels"], W, H, coefficients=True, **kw).cpu().numpy()
    own = ds.lightmap_sample(dev["values"], dev["rows"], dev["uvs"], dev["texels"], W, H, channels=27, **kw).cpu().numpy()
    assert coeff.shape == own.shape == (N_ROWS, 28)
    assert_words_equal(coeff, own, ("sh coefficients against lightmap_sample(channels=27)", nearest, plane, guard))
    count = own[:, 27].view(np.uint32)
    invalid = c["invalid"] if guard else c["invalid"][:-1]  # (the last class is a vertex word: judged under the guard only)
    assert (own[invalid].view(np.uint32) == 0).all(), [c["names"][k] for k in np.nonzero((own[c["invalid"]].view(np.uint32) != 0).any(axis=1))[0]]
    assert np.isfinite(own[:, :27]).all()  # no word that is not finite, and nothing of word 27, reached an answer
    if nearest:
        assert set(np.unique(count)) == {0, 1}
    else:  # partial coverage: the comparison is not about full and empty rows alone
        assert (count == 4).any() and ((count >= 1) & (count <= 3)).any() and (count == 0).sum() > len(c["invalid"]) and count.max() == 4
