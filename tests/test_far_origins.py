"""The fp32 contract's own envelope in the distance of a ray's origin (rule 1's distance clause), on the CPU: the float
oracle against the double oracle on rays aimed at the primitives of one scene from origins 1 to 16384 times S away (tests/far_rays.py).
Rule 1 pads every box by S * 2^-20 and rule 2 accepts a sphere's hit point within S * 2^-21 of the sphere's own box; a ray from |o| carries
a rounding error of about |o| * 2^-23 in its hit point and its slab parameters, so beyond a few S both margins run out: hits on flat
primitives are lost to flat boxes, hits at a sphere's pole to rule 2. Measured with the committed generator (profiles/far_origins.txt):
every solid f64 hit is found up to E_MEASURED = 16 x S; at 64 x S the spheres seen along an axis lose their pole hits, from 256 x S on quads
seen along their normal or along an axis lose hits to their flat boxes. The tests on the device are tests/test_gpu_far_origins.py."""
import numpy as np
import pytest

import far_rays as fr
from far_rays import CLASSES, E_DOC, E_MEASURED, HIT, LADDER


def _lost_by_the_float_oracle(ratio):
    b = fr.ladder_batch(ratio)
    return fr.lost(b["solid"], b["status32"], b["t32"], b["t64"])


def test_the_scene_and_the_constants_are_what_the_ladder_assumes():
    sc = fr.ladder_scene()
    assert fr.scene_S(sc.desc) == 20.0 and fr.sphere_slack_of(20.0) == np.float32(20.0 * 2.0 ** -21)
    assert E_MEASURED in LADDER and E_DOC == E_MEASURED // 4 and E_DOC in LADDER and LADDER[-1] > E_MEASURED
    assert all(b == 4 * a for a, b in zip(LADDER, LADDER[1:]))


@pytest.mark.parametrize("ratio", LADDER)
def test_the_generator_aims_at_what_it_says(ratio):
    """Every class has its rays, origins lie ratio x S from their targets, |d| is that distance (so the aimed hit is at t = 1), and at least
    60 % of a rung's rays are solid: the double oracle's closest hit is the aimed one (origins of the first rungs sit inside the cloud)."""
    b = fr.ladder_batch(ratio)
    rays, cls = b["rays"], b["cls"]
    assert len(rays) == len(CLASSES) * fr.PER_CLASS and (np.bincount(cls) == fr.PER_CLASS).all()
    length = np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1)
    assert np.allclose(length, ratio * 20.0, rtol=1e-6)
    share = b["solid"].mean()
    print(f"far: ratio {ratio}: solid per class {fr.per_class(b['solid'], cls)} of {fr.PER_CLASS}, share {share:.3f}")
    assert share >= 0.6, share
    axial = rays[cls == CLASSES.index("quad_axial"), 4:7]
    assert ((axial == 0).sum(axis=1) == 2).all()
    if ratio >= 16:  # (outside the cloud every aimed hit is the closest)
        assert share >= 0.99, share


@pytest.mark.parametrize("ratio", [r for r in LADDER if r <= E_MEASURED])
def test_inside_the_envelope_the_float_oracle_finds_every_solid_hit(ratio):
    b = fr.ladder_batch(ratio)
    lost = _lost_by_the_float_oracle(ratio)
    print(f"far: ratio {ratio}: lost by the float oracle per class {fr.per_class(lost, b['cls'])}")
    assert not lost.any(), (ratio, fr.per_class(lost, b["cls"]), b["rays"][lost][:4])


@pytest.mark.parametrize("ratio", [r for r in LADDER if r <= E_MEASURED])
def test_inside_the_envelope_the_tree_free_evaluation_is_the_float_oracle(ratio):
    """Yardstick 3 against yardstick 2: the contract's primitive tests over all primitives give the oracle's status, t bit for bit and material."""
    b = fr.ladder_batch(ratio)
    free = b["free"]
    bad = (free["status"] != b["status32"]) | (free["t"].view(np.uint32) != b["t32"].view(np.uint32)) | ((b["status32"] == HIT) & (free["material"] != b["mat32"]))
    assert not bad.any(), (ratio, fr.per_class(bad, b["cls"]), b["rays"][bad][:4], free[bad][:4], b["t32"][bad][:4])
    assert (free["status"] == HIT).mean() > 0.9


def test_the_ladder_reaches_the_edge():
    """Above E_MEASURED the float oracle does lose solid hits - the very next rung already -, so the clean rungs are clean because the
    margins hold there and not because the rays are harmless. Recorded per rung and class, with what the tree-free evaluation loses (the
    primitive tests alone, no box: the difference is what flat boxes cost)."""
    total = {}
    for ratio in LADDER:
        b = fr.ladder_batch(ratio)
        lost = _lost_by_the_float_oracle(ratio)
        free_lost = fr.lost(b["solid"], b["free"]["status"], b["free"]["t"], b["t64"])
        apart = (b["free"]["status"] != b["status32"]) | (b["free"]["t"].view(np.uint32) != b["t32"].view(np.uint32))
        print(f"far: ratio {ratio}: solid {fr.per_class(b['solid'], b['cls'])} lost by the float oracle {fr.per_class(lost, b['cls'])} "
              f"by the tree-free evaluation {fr.per_class(free_lost, b['cls'])} oracle != tree-free {fr.per_class(apart, b['cls'])}")
        total[ratio] = int(lost.sum())
    above = [r for r in LADDER if r > E_MEASURED]
    assert total[above[0]] > 0, total
    assert all(total[r] > 0 for r in above), total
    flat = [CLASSES.index(c) for c in ("quad_normal", "quad_oblique", "quad_axial")]
    b = fr.ladder_batch(1024)
    lost = _lost_by_the_float_oracle(1024)
    assert sum(fr.per_class(lost, b["cls"])[k] for k in flat) > 0  # (hits on flat primitives, aimed at 0.2 - 0.8 of the quad: lost to flat boxes)
