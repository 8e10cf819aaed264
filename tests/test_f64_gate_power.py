"""The power of the fp32-vs-f64 gate (tests/test_gpu_vs_f64.py), measured on the CPU: what does it see of each fp32-only rule of DESIGN.md 4?

Device and float oracle share those rules, so the bit-parity suite cannot see a defect both sides share; only the gate, which puts the fp32
frame next to the oracle's DOUBLE instantiation, can. Here the float oracle with one rule switched off (orc.render's disabled_rules) stands
in the gate's fp32 slot - a device that lacks the rule, since device = float oracle within 1e-5 - and the gate's own bounds
(f64_gate.BOUNDS, DEEP_BOUNDS) judge it. Full table, every rule: profiles/f64_gate_power.txt (tests/tools/f64_gate_power.py).

What the gate sees (a rule is asserted here when its mutant breaks a standing bound by at least 1.5 times):
  rule 8 (flat self-hit)          C1 tall box at 1024 spp: rel -1.35e-5, z -4.91, apart 0.0048, rays +1.0e-5 - z, apart and rays each fail.
                                  At 64 spp the same defect reads z -1.2 and passes: only the 1024-spp cases see it.
  rule 5 (sphere point on sphere) C2 with two bounces: rays +4.9e-5 against a bound of 1e-5 (the contract: 0). On C2 itself (max_depth 50)
                                  the defect is -1.7e-3 in the mean, 0.36 of the noise that paths rounding apart make there: passes.
  rule 6 (cancellation-free roots) C2 with two bounces (rays +1.4e-4, apart 0.016) and C2 itself at 64 spp (rel 1.8 x the noise).
  rule 4 (rotated triangle records) the stress mesh's rods: rel +2.05e-3 (3.4 x the bound), z +7.3, apart 0.24.
What it cannot see at an affordable cost - the rules stay (DESIGN.md 4 says why each exists):
  rule 7 (quad point on plane)    with rule 8 on, C1's tall box at 1024 spp reads z -1.40, apart 0.0005, rays -9e-8 (contract: -1.16, 0.0005,
                                  +7e-8): rule 8 catches the re-hits rule 7 prevents. Without both, the crop is round 5's z -4.4 at 64 spp.
  rules 1, 2, 3 (box pad, sphere roots in their box, needle triangles): they keep a hit inside every box that bounds its primitive (tree
                                  independence). Their defects - a hit lost to a flat node box, a frame that depends on the tree - do not
                                  fire on the crops measured: rules 1 and 2 change no pixel of C1, the two-bounce C2 or the stress mesh's
                                  rods, rule 3 moves the rods from z +3.47 to +3.66. Where they do fire (a flat node 3000 units out; rule 2
                                  with rule 6 off, rule 3 with rule 4 off, each under two trees): tests/test_fp32_contract.py::
                                  test_each_rule_bit_brings_its_defect_back. Gate (i), the bit-parity suite across trees and kernels, holds them.
"""
import pytest

import f64_gate as fg
import orc

C1, TWO_BOUNCES, HET = "c1_cornell", "c2_spheres_two_bounces", "c3_heterogeneous"


@pytest.fixture(scope="module")
def gate():
    """measure() for (case, crop, spp, rules switched off); the f64 side of a crop is rendered once and shared by every mutant."""
    f64 = {}
    scenes = {}

    def run(name, crop, spp, rules=()):
        case = fg.case(name)
        rect = dict(case[4])[crop]
        if (name, spp) not in scenes:
            scenes[name, spp] = fg.make_scene(case, spp)
        sc = scenes[name, spp]
        if (name, crop, spp) not in f64:
            f64[name, crop, spp] = fg.f64_side(sc, rect, spp)
        mask = 0
        for k in rules:
            mask |= orc.rule_bit(k)
        frame, window = fg.mutant(mask)
        return fg.measure(sc, rect, spp, frame, window, f64=f64[name, crop, spp])

    return run


@pytest.mark.parametrize("name,crop,spp,bounds", [
    (C1, "tall_box_and_wall", fg.SPP, fg.BOUNDS[C1]),
    (C1, "tall_box_and_wall", fg.DEEP_SPP, fg.DEEP_BOUNDS[C1]),
    (TWO_BOUNCES, "dense", fg.SPP, fg.BOUNDS[TWO_BOUNCES]),
    (HET, "rods_and_rails", fg.SPP, fg.BOUNDS[HET]),
])
def test_the_contract_passes(gate, name, crop, spp, bounds):
    """(a) Mask 0 - the contract the device is held to bit for bit - passes the gate's bounds on every crop used below."""
    m = gate(name, crop, spp)
    assert m["mean_f64"] > 0
    assert not fg.exceeded(m, bounds), m


def test_the_gate_sees_rule_8_only_at_1024_spp(gate):
    """(b) The defect that shipped last: without rule 8, C1's tall box fails the 1024-spp bounds three separate ways, and reproduces the
    pre-rule-8 device row of profiles/r05_gpu_vs_f64.txt (a disabled rule in the float oracle stands in faithfully for a device without it).
    At the gate's 64 spp the same defect passes."""
    m = gate(C1, "tall_box_and_wall", fg.DEEP_SPP, rules=(8,))
    over = fg.exceeded(m, fg.DEEP_BOUNDS[C1])
    assert {"z", "apart", "rays_rel"} <= set(over), (over, m)
    assert min(over[k] for k in ("z", "apart", "rays_rel")) >= 1.5, over
    assert m["rel"] == pytest.approx(-1.35e-5, abs=0.01e-5), m
    assert m["z"] == pytest.approx(-4.91, abs=0.01), m
    assert m["apart"] == pytest.approx(0.0048, abs=0.00005), m
    assert not fg.exceeded(gate(C1, "tall_box_and_wall", fg.SPP, rules=(8,)), fg.BOUNDS[C1])


def test_the_gate_sees_rule_5(gate):
    """(c) Without rule 5 a ray scattered from a point just inside a sphere (fp32 t from 800 units) re-hits the sphere from within: with two
    bounces per path fp32 and f64 otherwise trace the same rays, and the surplus breaks the rays bound."""
    m = gate(TWO_BOUNCES, "dense", fg.SPP, rules=(5,))
    over = fg.exceeded(m, fg.BOUNDS[TWO_BOUNCES])
    assert over.get("rays_rel", 0) >= 1.5, (over, m)
    assert m["rays_rel"] > 0, m  # (surplus: one-signed)


def test_the_gate_sees_rule_6(gate):
    """(d) Without the cancellation-free sphere test the rims of the distant spheres are misjudged: the two-bounce crop fails."""
    m = gate(TWO_BOUNCES, "dense", fg.SPP, rules=(6,))
    over = fg.exceeded(m, fg.BOUNDS[TWO_BOUNCES])
    assert over and max(over.values()) >= 1.5, (over, m)


def test_the_gate_sees_rule_4(gate):
    """(d) Triangle records in the reference's vertex order (Moeller-Trumbore's error grows with the two edges at v0): on the stress mesh's
    thin rods the crop reads +2.05e-3 (3.4 x the bound), z +7.3, a quarter of its pixels apart."""
    m = gate(HET, "rods_and_rails", fg.SPP, rules=(4,))
    over = fg.exceeded(m, fg.BOUNDS[HET])
    assert {"rel", "z", "apart"} <= set(over) and max(over.values()) >= 1.5, (over, m)


def test_what_the_gate_cannot_see(gate):
    """Named in the module docstring and DESIGN.md 4: rule 7 under rule 8 passes at 1024 spp; rule 1 does not fire on C1's crop (no node
    box there is flat at large coordinates). If this starts failing, the gate has learnt to see more: move the rule up into the asserted list."""
    m7 = gate(C1, "tall_box_and_wall", fg.DEEP_SPP, rules=(7,))
    assert not fg.exceeded(m7, fg.DEEP_BOUNDS[C1]), m7
    m0, m1 = gate(C1, "tall_box_and_wall", fg.SPP), gate(C1, "tall_box_and_wall", fg.SPP, rules=(1,))
    assert m1 == m0
