"""Adaptive sampling against the fixed loop: wall time, samples spent and error, per scene and threshold.

    python tests/tools/adaptive_bench.py [--cases c3,c5] [--spp 512] [--round 64] [--min 128] [--thresholds 0,0.01,0.02,0.05,0.1]

For each case at 1920x1080 (max = --spp): the fixed loop (sol_render in 64-sample launches up to max, as ray_trace's OnlyFinal batches) and
adaptive sessions at each threshold, best of --repeat timed runs each. Columns:
  time_ms      wall time of the session (begin .. last round, synchronised)
  vs_fixed     time / fixed loop's time
  spent        samples spent / (pixels * max)
  rmse/noise   RMSE of the per-pixel means against the fixed max-spp frame of the same seed, over that frame's own noise
               (RMSE of two fixed frames of different seeds / sqrt 2): how much of the fixed frame's error the skipped samples add
  indep        RMSE against the fixed frame of ANOTHER seed over the RMSE of the two fixed frames (1.0 = as good as the fixed frame)
One text table on stdout; --json adds one JSON line per row.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _paths  # noqa: E402,F401

from solstrale_amd import DeviceScene, RenderConfig, scenes  # noqa: E402

SEED, SEED2 = 0x5017A1E, 0xB0B5EED


def make(case, spp):
    rc = RenderConfig(1920, 1080, spp)
    return {"c3": lambda: scenes.sponza_like(rc), "c5": lambda: scenes.statue_like(rc), "c1": lambda: scenes.cornell_box(rc)}[case]()


def fixed(ds, spp, seed, batch=64):
    ds.clear()
    ds.sync()
    t = time.perf_counter()
    done = 0
    while done < spp:
        n = min(batch, spp - done)
        ds.render(done, n, seed)
        done += n
    ds.sync()
    return (time.perf_counter() - t) * 1e3, ds.read().astype(np.float64) / spp


def adaptive(ds, spp, rnd, mn, thr, seed):
    ds.sync()
    t = time.perf_counter()
    ds.adaptive_begin(rnd, mn, spp, thr)
    rounds = ds.adaptive_run(seed)
    ds.sync()
    ms = (time.perf_counter() - t) * 1e3
    counts = ds.adaptive_counts()
    per_px = np.repeat(np.repeat(counts, 8, 0), 8, 1)[:ds.height, :ds.width].astype(np.float64)
    return ms, ds.read().astype(np.float64) / per_px[..., None], per_px, rounds


def rmse(a, b):
    return float(np.sqrt(((a - b) ** 2).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c5")
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--round", type=int, default=64)
    ap.add_argument("--min", type=int, default=128)
    ap.add_argument("--thresholds", default="0,0.01,0.02,0.05,0.1")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--no-fixed", action="store_true", help="adaptive sessions only (e.g. under rocprofv3)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    thresholds = [float(x) for x in a.thresholds.split(",")]
    print(f"{'case':5} {'threshold':>9} {'round':>5} {'min':>4} {'rounds':>6} {'time_ms':>9} {'vs_fixed':>8} {'spent':>6} {'rmse/noise':>10} {'indep':>6}")
    for case in a.cases.split(","):
        sc = make(case, a.spp)
        with DeviceScene(sc) as ds:
            ref = ref2 = None
            t_fixed = float("nan")
            if not a.no_fixed:
                t_fixed = min(fixed(ds, a.spp, SEED)[0] for _ in range(a.repeat))
                _, ref = fixed(ds, a.spp, SEED)
                _, ref2 = fixed(ds, a.spp, SEED2)
                noise = rmse(ref, ref2) / np.sqrt(2.0)
                print(f"{case:5} {'fixed':>9} {'':>5} {'':>4} {'':>6} {t_fixed:9.1f} {1.0:8.3f} {1.0:6.3f} {'':>10} {'':>6}")
            for thr in thresholds:
                best = None
                for _ in range(a.repeat):
                    r = adaptive(ds, a.spp, a.round, a.min, thr, SEED)
                    best = r if best is None or r[0] < best[0] else best
                ms, mean, per_px, rounds = best
                spent = float(per_px.mean() / a.spp)
                row = {"case": case, "threshold": thr, "round": a.round, "min": a.min, "max": a.spp, "rounds": rounds, "time_ms": ms,
                       "fixed_ms": t_fixed, "spent": spent}
                line = f"{case:5} {thr:9.3f} {a.round:5d} {a.min:4d} {rounds:6d} {ms:9.1f} {ms / t_fixed:8.3f} {spent:6.3f}"
                if ref is not None:
                    row["rmse_over_noise"] = rmse(mean, ref) / noise
                    row["indep"] = rmse(mean, ref2) / rmse(ref, ref2)
                    line += f" {row['rmse_over_noise']:10.3f} {row['indep']:6.3f}"
                print(line, flush=True)
                if a.json:
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
