"""The standing fp32-vs-f64 gate: the cases and the statistics (tests/test_gpu_vs_f64.py asserts them, tests/tools/gpu_vs_f64.py prints the
table kept under profiles/). TEST INFRASTRUCTURE.

Every other parity test holds the device to the oracle's FLOAT instantiation, which this repository designs together with the device
(the fp32-only rules of include/solstrale_hip.h and DESIGN.md 4): a defect the two share is invisible there - round 4 found BASELINE
config 2 rendering 8.3 % darker than the reference's arithmetic for three rounds that way. Here the fp32 side is put next to the
oracle's DOUBLE instantiation - the reference's own arithmetic (src/hittable/sphere.rs:64-108, triangle.rs:119-173, quad.rs:150-194,
geo/mod.rs:159-188), pinned by the reference's 22 golden images - on crops of every BASELINE workload at its full scene and resolution.

At one seed the two renders follow the same paths except where a rounding decides a branch; a path that rounds apart contributes a
difference of either sign, a RULE that loses or invents energy (or rays) a signed one. Per crop:
  rel        (mean fp32 - mean f64) / mean f64 of the crop
  noise      relative standard error of the crop mean at this sample count, from the pixelwise differences of two independent f64 sample
             sets of the same size (samples [0, spp) and [spp, 2 spp))
  two_sets   the relative difference of those two sets' means (one draw of that noise; the figure profiles/r04_float_vs_double.txt quotes)
  apart      fraction of pixels whose fp32 and f64 values differ by more than 1e-4 + 1e-3 |f64| in some channel (paths that rounded apart)
  z          sum of the pixel differences / sqrt(sum of their squares): the differences' own t statistic; independent zero-mean
             differences give |z| ~ 1, a one-signed offset over n pixels sqrt(n)
  rays       rays per sample of the fp32 side and of f64 on the crop as a WINDOW frame (parity_util.WindowScene), and their ratio - 1. Rays = the
             searches the DEVICE runs (SolStats::rays): it ends a path at a ScatterPdf level whose factor is zero, where the reference traces on
             and multiplies by zero; the oracle counts those apart (OrcStats::live_rays = the device's definition)
"""
import functools

import numpy as np

import orc
import parity_util as pu
from solstrale_amd import PathTracingShader, RenderConfig, scenes

SPP = 64
# the cases that also stand at DEEP_SPP (tests/test_gpu_vs_f64.py): 16 x the samples, where a defect of a few samples in a million - rule 8's,
# 124 of 16.7 M on C1's tall box - reaches |z| ~ 5 (profiles/f64_gate_power.txt)
DEEP_SPP = 1024
DEEP_CASES = ("c1_cornell", "profiling_workload")
# (name, factory(render_config), width, height, [(crop name, rect), ...])
CASES = [
    ("c1_cornell", lambda rc: scenes.cornell_box(rc), 400, 400,
     [("tall_box_and_wall", (60, 120, 188, 248)), ("light_and_ceiling", (136, 0, 264, 128))]),
    ("c2_cornell_spheres", lambda rc: scenes.cornell_spheres(rc), 1920, 1080,
     [("dense", (900, 500, 1028, 628)), ("box_edges", (1180, 560, 1308, 688))]),
    ("c3_atrium", lambda rc: scenes.sponza_like(rc), 1920, 1080,
     [("across_hall", (900, 500, 1028, 628)), ("corner", (0, 952, 128, 1080))]),
    ("c3_heterogeneous", lambda rc: scenes.sponza_like(rc, mesh="heterogeneous"), 1920, 1080,
     [("across_hall", (900, 500, 1028, 628)), ("rods_and_rails", (600, 380, 728, 508))]),
    ("c3_heterogeneous_interior", lambda rc: scenes.sponza_like(rc, mesh="heterogeneous", camera="interior"), 1920, 1080,
     [("under_gallery", (1000, 300, 1128, 428)), ("colonnade", (896, 476, 1024, 604))]),
    ("c4_atrium_4k", lambda rc: scenes.sponza_like(rc), 3840, 2160,
     [("across_hall", (1800, 1000, 1928, 1128)), ("corner", (0, 2032, 128, 2160))]),
    ("c5_statue", lambda rc: scenes.statue_like(rc), 1920, 1080,
     [("body_drapery", (896, 476, 1024, 604)), ("glass_head_rim", (900, 60, 1028, 188))]),
    ("c5_statue_hdri", lambda rc: scenes.statue_like(rc, environment=True), 1920, 1080,
     [("body_drapery", (896, 476, 1024, 604)), ("glass_orb", (1150, 860, 1278, 988))]),
    ("profiling_workload", lambda rc: scenes.create_test_scene(rc), 800, 400,
     [("centre", (336, 136, 464, 264)), ("left_objects", (120, 150, 248, 278))]),
    # the regime that hid the sphere defect: a long lens far from the objects (an origin's digits lost against the objects' size)
    ("c3_atrium_far", lambda rc: scenes.sponza_like(rc, camera="far"), 1920, 1080,
     [("roof_opening", (900, 500, 1028, 628)), ("gallery_edge", (900, 250, 1028, 378))]),
    ("c5_statue_far", lambda rc: scenes.statue_like(rc, camera="far"), 1920, 1080,
     [("body_drapery", (896, 476, 1024, 604)), ("glass_head_rim", (900, 60, 1028, 188))]),
    # C2 with paths of two bounces: the sphere field seen from 800 units (rule 5's regime) without the deep paths that round apart - at
    # max_depth 50 a quarter of the crop's pixels do, and their noise hides rule 5's defect; here fp32 and f64 trace the same rays, and the
    # re-hits from inside a sphere that rule 5 prevents show as surplus rays (profiles/f64_gate_power.txt)
    ("c2_spheres_two_bounces", lambda rc: scenes.cornell_spheres(RenderConfig(rc.width, rc.height, rc.samples_per_pixel, PathTracingShader(2))),
     1920, 1080, [("dense", (900, 500, 1028, 628))]),
]


# case -> (rel_of_noise, ceiling of `apart`, bound of |z|, bound of |rays rel|). Measured |rel| / noise is at most 0.33 (c5_statue_far, glass rim)
# and 0.14 elsewhere; `apart` at 64 spp: C2 0.27 (12 rays per sample through 10 000 spheres seen from 800 units), atrium 0.02 - 0.07, statue
# 0.002 - 0.044; |z| < 2 in both crops everywhere but the three cases kept at 4.5 (rods_and_rails +3.5, under_gallery -2.2, far glass rim -2.6).
BOUNDS = {
    "c1_cornell": (0.6, 0.02, 3.0, 3e-3),
    "c2_cornell_spheres": (0.6, 0.40, 3.0, 3e-3),
    "c3_atrium": (0.6, 0.08, 3.0, 3e-3),
    "c3_heterogeneous": (0.6, 0.08, 4.5, 3e-3),
    "c3_heterogeneous_interior": (0.6, 0.12, 4.5, 3e-3),
    "c4_atrium_4k": (0.6, 0.08, 3.0, 3e-3),
    "c5_statue": (0.6, 0.02, 3.0, 3e-3),
    "c5_statue_hdri": (0.6, 0.02, 3.0, 3e-3),
    "profiling_workload": (0.6, 0.01, 3.0, 3e-3),
    "c3_atrium_far": (0.6, 0.10, 3.0, 3e-3),
    "c5_statue_far": (0.6, 0.08, 4.5, 3e-3),
    # two bounces: fp32 and f64 trace the same rays (rays rel 0, apart 2e-4); without rule 5 the re-hits from inside a sphere give +4.9e-5
    "c2_spheres_two_bounces": (0.6, 0.002, 3.0, 1e-5),
}
# at f64_gate.DEEP_SPP (1024): without rule 8, C1's tall-box crop reads z -4.9, apart 0.0048, rays +1.0e-5 - each outside these
DEEP_BOUNDS = {
    "c1_cornell": (0.6, 0.002, 3.0, 5e-6),
    "profiling_workload": (0.6, 0.006, 3.0, 5e-6),
}


def exceeded(m, bounds):
    """{statistic: |measured| / bound} of every bound that measure()'s result `m` breaks (empty: the crop passes)."""
    rel_of_noise, apart_max, z_max, rays_rel_max = bounds
    ratios = {"rays_rel": abs(m["rays_rel"]) / rays_rel_max, "rel": abs(m["rel"]) / (rel_of_noise * m["noise"]),
              "z": abs(m["z"]) / z_max, "apart": m["apart"] / apart_max}
    return {k: v for k, v in ratios.items() if v > 1.0 or (k == "z" and v == 1.0)}  # (|z| < z_max: equality fails too)


def check(name, crop, m, bounds):
    assert m["mean_f64"] > 0
    assert not exceeded(m, bounds), (name, crop, exceeded(m, bounds), m)


def float_oracle_frame(scene, spp, rect, disabled_rules=0):
    """The fp32 side on the CPU (tools only): the oracle's float instantiation on the crop (disabled_rules: a mutant of the contract,
    orc.render)."""
    img, _ = orc.render(scene, 0, spp, pu.SEED, real=orc.ORC_F32, rect=rect, disabled_rules=disabled_rules)
    return img


def float_oracle_window(win, spp, disabled_rules=0):
    _, st = orc.render(win, 0, spp, pu.SEED, real=orc.ORC_F32, disabled_rules=disabled_rules)
    return st["live_rays"], st["samples"]


def mutant(disabled_rules):
    """(frame, window) of the float oracle with fp32 rules switched off (orc.render's disabled_rules): measure()'s fp32 side for a contract
    that lacks them - what a device without those rules would give, since device = float oracle (tests/test_f64_gate_power.py)."""
    return (functools.partial(float_oracle_frame, disabled_rules=disabled_rules),
            functools.partial(float_oracle_window, disabled_rules=disabled_rules))


def f64_side(scene, rect, spp):
    """What measure() needs of the double instantiation: two independent sample sets of the crop (per-sample means) and the live rays per
    sample of the crop as a window frame. It does not depend on the fp32 side: callers that put several fp32 sides next to one crop share it."""
    x0, y0, x1, y1 = rect
    crop = (slice(y0, y1), slice(x0, x1))
    a, _ = orc.render(scene, 0, spp, pu.SEED, real=orc.ORC_F64, rect=rect)
    b, _ = orc.render(scene, spp, spp, pu.SEED, real=orc.ORC_F64, rect=rect)
    _, st = orc.render(pu.WindowScene(scene, rect), 0, spp, pu.SEED, real=orc.ORC_F64)
    return a[crop] / spp, b[crop] / spp, st["live_rays"] / st["samples"]


def measure(scene, rect, spp, fp32_frame, fp32_window_rays, f64=None):
    """fp32_frame(scene, spp, rect) -> (H, W, 3) sums of the whole frame (only the crop is read);
    fp32_window_rays(window_scene, spp) -> (rays, samples) of a counted render of the window frame;
    f64: f64_side(scene, rect, spp) if the caller has it already."""
    x0, y0, x1, y1 = rect
    crop = (slice(y0, y1), slice(x0, x1))
    g = np.asarray(fp32_frame(scene, spp, rect), dtype=np.float64)[crop] / spp
    a, b, r64 = f64 if f64 is not None else f64_side(scene, rect, spp)
    assert np.isfinite(g).all() and np.isfinite(a).all() and np.isfinite(b).all()
    mean = a.mean()
    n = a.size
    noise = np.sqrt(((a - b) ** 2).sum() / 2.0) / n / mean
    d = (g - a).sum(axis=-1)
    apart = (np.abs(g - a) > 1e-4 + 1e-3 * np.abs(a)).any(axis=-1)
    ss = np.sqrt((d ** 2).sum())
    rays32, samples32 = fp32_window_rays(pu.WindowScene(scene, rect), spp)
    r32 = rays32 / samples32
    return {"mean_f64": float(mean), "rel": float((g.mean() - mean) / mean), "noise": float(noise), "two_sets": float((b.mean() - mean) / mean),
            "apart": float(apart.mean()), "z": float(d.sum() / ss) if ss > 0 else 0.0,
            "rays_fp32": float(r32), "rays_f64": float(r64), "rays_rel": float(r32 / r64 - 1.0)}


def header():
    return (f"{'workload':28s} {'crop':16s} {'mean f64':>9s} {'rel':>10s} {'noise':>9s} {'two f64 sets':>12s} {'apart':>7s} {'z':>6s} "
            f"{'rays fp32':>9s} {'rays f64':>9s} {'rays rel':>9s}")


def row(name, crop, m):
    return (f"{name:28s} {crop:16s} {m['mean_f64']:9.5f} {m['rel']:+10.2e} {m['noise']:9.2e} {m['two_sets']:+12.2e} {m['apart']:7.4f} {m['z']:+6.2f} "
            f"{m['rays_fp32']:9.4f} {m['rays_f64']:9.4f} {m['rays_rel']:+9.2e}")


def case(name):
    return next(c for c in CASES if c[0] == name)


def make_scene(case, spp=SPP):
    name, factory, w, h, crops = case
    return factory(RenderConfig(w, h, spp))
