"""Prints what the fp32-vs-f64 gate (tests/f64_gate.py) sees of each fp32-only rule of DESIGN.md 4: the float oracle with one rule switched off
(orc.render's disabled_rules) stands in the gate's fp32 slot - a device that lacks the rule, since device = float oracle - on the cheapest
gate case and crop where the rule could fire. Not a pytest (tests/test_f64_gate_power.py asserts a subset); the record is
profiles/f64_gate_power.txt. Runs on the CPU only.
Usage: python f64_gate_power.py"""
import _paths  # noqa: F401
import sys
import time

import numpy as np

import f64_gate as fg
import orc

# (case, crop, spp, rules switched off one at a time; 0 = the contract)
ROWS = [
    ("c1_cornell", "tall_box_and_wall", 64, (0, 1, 7, 8)),
    ("c1_cornell", "tall_box_and_wall", 1024, (0, 1, 7, 8)),
    ("c1_cornell", "light_and_ceiling", 1024, (0, 7, 8)),
    ("c2_spheres_two_bounces", "dense", 64, (0, 1, 2, 5, 6)),
    ("c2_cornell_spheres", "dense", 64, (0, 5, 6)),
    ("c3_heterogeneous", "rods_and_rails", 64, (0, 1, 3, 4, 8)),
    ("c5_statue", "glass_head_rim", 64, (0, 4)),
    ("profiling_workload", "centre", 1024, (0,)),
    ("profiling_workload", "left_objects", 1024, (0,)),
]


def main():
    print("fp32 side: the oracle's float instantiation with the named rule switched off; f64 side: the double instantiation; seed "
          f"{fg.pu.SEED:#x}, 128x128 crops of the full frame. 'same' = the fp32 crop is bit-identical to the contract's (mask 0).", flush=True)
    print(f"{'off':>4s} {'spp':>5s} " + fg.header() + "  same", flush=True)
    for name, crop, spp, rules in ROWS:
        t0 = time.time()
        case = fg.case(name)
        rect = dict(case[4])[crop]
        x0, y0, x1, y1 = rect
        sc = fg.make_scene(case, spp)
        f64 = fg.f64_side(sc, rect, spp)
        base = None
        for k in rules:
            mask = orc.rule_bit(k) if k else 0
            frame, window = fg.mutant(mask)
            img = frame(sc, spp, rect)[y0:y1, x0:x1]
            base = img if k == 0 else base
            m = fg.measure(sc, rect, spp, lambda *_: img_full(img, sc, rect), window, f64=f64)
            same = "" if base is None or k == 0 else ("yes" if np.array_equal(img, base) else "no")
            print(f"{'-' if k == 0 else k:>4} {spp:5d} " + fg.row(name, crop, m) + f"  {same}", flush=True)
        print(f"  ({name} {crop} {spp} spp: {time.time() - t0:.1f} s)", file=sys.stderr, flush=True)


def img_full(img, sc, rect):
    """The crop put back into a frame of the scene's size (measure() reads only the crop)."""
    x0, y0, x1, y1 = rect
    out = np.zeros((sc.height, sc.width, 3))
    out[y0:y1, x0:x1] = img
    return out


if __name__ == "__main__":
    main()
