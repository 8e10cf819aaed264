"""The standing gate that is NOT common-mode: the HIP fp32 frame next to the oracle's DOUBLE instantiation - the reference's own arithmetic
(src/hittable/sphere.rs:64-108, triangle.rs:119-173, quad.rs:150-194, geo/mod.rs:159-188; pinned by the reference's 22 golden images) -
on two 128x128 crops of every BASELINE workload at its full scene and resolution: C1, C2, C3, the heterogeneous stress mesh (both cameras),
C4 at 4K, C5, C5 + HDRI, the reference's profiling workload, and far-camera variants of C3 and C5 (the regime that hid the fp32 sphere
defect of rounds 1-3: BASELINE config 2 rendered 8.3 % darker than f64 while every fp32-vs-fp32 parity test was green).

Statistics, cases and bounds: tests/f64_gate.py. Per crop, at 64 spp and the seed of every parity test:
  (i)   rays per sample of the device within the case's bound of f64's (0.3 %; crop rendered as a window frame by both sides);
  (ii)  |relative difference of the crop means| below the case's `rel_of_noise` x the measured noise of the crop mean (two independent f64
        sample sets of the same size), and the pixel differences' own t statistic |z| below the case's bound (3; 4.5 where a known offset
        sits: the stress mesh's coplanar pair, the glass head's cracks through a long lens) - a rule that loses or invents energy gives the
        differences one sign (the sphere defect: z ~ -37 on C2), paths that merely round apart give |z| ~ 1;
  (iii) the fraction of pixels whose paths rounded apart below the case's ceiling.
C1 and the profiling workload stand at 1024 spp as well (f64_gate.DEEP_BOUNDS), where rule 8's defect - a few samples in a million - fails (i), (ii)
and (iii) each; C2 with two bounces per path is where rule 5's defect shows (surplus rays). What each bound catches: tests/test_f64_gate_power.py
and profiles/f64_gate_power.txt (the float oracle with one fp32 rule switched off in the fp32 slot).
Measured figures (MI355X): profiles/r05_gpu_vs_f64.txt (tests/tools/gpu_vs_f64.py prints the table), profiles/f64_gate_power.txt.
"""
import pytest

import f64_gate as fg
import parity_util as pu
from solstrale_amd import DeviceScene

pytestmark = pytest.mark.gpu

def device_frame(scene, spp, rect):
    with DeviceScene(scene) as ds:
        ds.render(0, spp, pu.SEED)
        return ds.read()


def device_window(win, spp):
    with DeviceScene(win) as ds:
        ds.render(0, spp, pu.SEED, counted=True)
        st = ds.stats()
    assert st["samples"] == win.width * win.height * spp
    return st["rays"], st["samples"]


def run_case(case, spp, bounds):
    name = case[0]
    sc = fg.make_scene(case, spp)
    frames = {}

    def frame(scene, spp, rect):  # one device render of the full frame serves both crops
        if "f" not in frames:
            frames["f"] = device_frame(scene, spp, rect)
        return frames["f"]

    for crop, rect in case[4]:
        m = fg.measure(sc, rect, spp, frame, device_window)
        print(fg.row(name, crop, m))
        fg.check(name, crop, m, bounds)


@pytest.mark.parametrize("case", fg.CASES, ids=[c[0] for c in fg.CASES])
def test_device_follows_the_reference_arithmetic(case):
    run_case(case, fg.SPP, fg.BOUNDS[case[0]])


@pytest.mark.parametrize("name", fg.DEEP_CASES)
def test_device_follows_the_reference_arithmetic_at_1024_spp(name):
    run_case(fg.case(name), fg.DEEP_SPP, fg.DEEP_BOUNDS[name])


def test_the_gate_sees_a_shared_defect():
    """The gate's own sensitivity: a fp32 side that loses 0.5 % of its energy - a sixteenth of what the sphere defect lost - fails (ii),
    although it would pass any fp32-vs-fp32 comparison with an oracle that shares the loss."""
    import numpy as np
    case = fg.case("profiling_workload")
    sc = fg.make_scene(case)
    rect = case[4][0][1]

    def dimmed(scene, spp, r):
        img = device_frame(scene, spp, r).astype(np.float64)
        return img * 0.995

    m = fg.measure(sc, rect, fg.SPP, dimmed, device_window)
    rel_of_noise, _, z_max, _ = fg.BOUNDS["profiling_workload"]
    assert abs(m["z"]) > z_max or abs(m["rel"]) > rel_of_noise * m["noise"], m
