"""Environment importance sampling against the BSDF-only estimator: time per frame, two-seed variance, equal-time efficiency.

    python tests/tools/env_is_bench.py [--cases c5_hdri,test_scene] [--spp 16] [--repeat 3]

Per case and mode (off = BSDF-only, on = sol_env_sampling importance), at the same spp:
  ms         wall time of one frame (sol_clear .. sol_render .. sol_sync), best of --repeat
  var        per-pixel variance of the per-sample mean, mean((F1 - F2)^2) / 2 over two frames of different seeds (F: sums / spp), over the
             whole frame and over the named crops
  eff        1 / (var * ms): equal-time efficiency; the on/off ratio of var and eff is printed per row
Cases: c5_hdri = the statue stand-in under the procedural 2048x1024 sky at 1920x1080 (bench.py --workload c5 --hdri), crops of
tests/f64_gate.py's c5_statue_hdri; test_scene = create_test_scene_with_environment (256x128 sky) at 800x400; lamb_soft_sun / lamb_sun_sky =
tests/test_env_importance.py's Lambertian scene (albedo <= 0.5) at 512x384 under its soft sun (the min(3) filter never binds) and under
procedural_sky(256, 128) (it binds on the sun). One text table on stdout.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _paths  # noqa: E402,F401

import test_env_importance as tei  # noqa: E402
from solstrale_amd import DeviceScene, PathTracingShader, RenderConfig, scenes  # noqa: E402

SEED, SEED2 = 0x5017A1E, 0xB0B5EED
CASES = {
    "c5_hdri": (lambda spp: scenes.statue_like(RenderConfig(1920, 1080, spp), environment=True),
                {"body_drapery": (896, 476, 1024, 604), "glass_orb": (1150, 860, 1278, 988)}),
    "test_scene": (lambda spp: scenes.create_test_scene_with_environment(RenderConfig(800, 400, spp, PathTracingShader(50))),
                   {"centre": (336, 136, 464, 264)}),
    # Lambertian only, albedo <= 0.5 (tests/test_env_importance.py): under the soft sun the min(3) filter never binds; under the sun sky it does
    "lamb_soft_sun": (lambda spp: tei._lambertian_scene(RenderConfig(512, 384, spp, PathTracingShader(6)), tei.soft_sun_sky()),
                      {"centre": (192, 128, 320, 256)}),
    "lamb_sun_sky": (lambda spp: tei._lambertian_scene(RenderConfig(512, 384, spp, PathTracingShader(6)), scenes.procedural_sky(256, 128)),
                     {"centre": (192, 128, 320, 256)}),
}


def frame(ds, spp, seed):
    ds.clear()
    ds.sync()
    t = time.perf_counter()
    ds.render(0, spp, seed)
    ds.sync()
    return (time.perf_counter() - t) * 1e3, ds.read().astype(np.float64) / spp


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default="c5_hdri,test_scene,lamb_soft_sun,lamb_sun_sky")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    print(f"# tests/tools/env_is_bench.py --spp {a.spp} --repeat {a.repeat} (ms: best of {a.repeat}; var: mean((F1-F2)^2)/2 of per-sample means)")
    print(f"{'case':13s} {'mode':4s} {'ms':>9s} {'var(frame)':>11s} {'eff':>10s} {'var on/off':>10s} {'eff on/off':>10s}  crops var (on/off)")
    for case in a.cases.split(","):
        make, crops = CASES[case]
        sc = make(a.spp)
        res = {}
        with DeviceScene(sc) as ds:
            for mode in ("off", "on"):
                ds.env_sampling("importance" if mode == "on" else 0)
                frame(ds, a.spp, SEED)  # (warm-up: tables, code objects)
                ms = min(frame(ds, a.spp, SEED)[0] for _ in range(a.repeat))
                _, f1 = frame(ds, a.spp, SEED)
                _, f2 = frame(ds, a.spp, SEED2)
                d2 = (f1 - f2) ** 2 / 2.0
                cv = {k: float(d2[y0:y1, x0:x1].mean()) for k, (x0, y0, x1, y1) in crops.items()}
                res[mode] = (ms, float(d2.mean()), cv, float(f1.mean()))
        for mode in ("off", "on"):
            ms, var, cv, mean = res[mode]
            eff = 1.0 / (var * ms)
            r_var = var / res["off"][1]
            r_eff = eff * (res["off"][1] * res["off"][0])
            crop_txt = "  ".join(f"{k} {v:.4g}" + (f" ({v / res['off'][2][k]:.3f})" if mode == "on" else "") for k, v in cv.items())
            print(f"{case:13s} {mode:4s} {ms:9.2f} {var:11.5g} {eff:10.4g} {r_var:10.3f} {r_eff:10.3f}  {crop_txt}  mean {mean:.4f}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
