"""Light sampling modes against light count: Msamples/s of modes 0 (uniform, the loop), 1 (tree) and 2 (power) on the same
frames, and the tree's build time.

    python tests/tools/light_bench.py [--lights 1,4,64,1024,4096] [--kind quads] [--size 256] [--spp 32] [--repeat 3]

Scene: scenes.many_lights(L, kind) (the Cornell box with its lamp replaced by L lamps of the same total power) at size x size. Per L and mode:
one warm-up frame, then --repeat frames timed with device events around the render kernel (sol_kernel_timing; best of --repeat);
Msamples/s = pixels x spp / kernel time. build ms: wall time of the first sol_light_sampling call of mode 1 on a fresh handle (the tree's
launches and their synchronisation), best of --repeat handles. x0: Msamples/s over mode 0's at the same L. One text table on stdout.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _paths  # noqa: E402,F401

from solstrale_amd import DeviceScene, PathTracingShader, RenderConfig, scenes  # noqa: E402

SEED = 0x5017A1E


def msamples(ds, n_pix, spp, repeat):
    ds.clear()
    ds.render(0, spp, SEED)  # (warm-up: code objects, the DevScene copy)
    ds.sync()
    best = float("inf")
    for _ in range(repeat):
        ds.clear()
        ds.render(0, spp, SEED)
        ms, _ = ds.last_kernel_ms()
        best = min(best, ms)
    return n_pix * spp / (best * 1e3), best


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lights", default="1,4,64,1024,4096")
    ap.add_argument("--kind", default="quads")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    print(f"# tests/tools/light_bench.py --kind {a.kind} --size {a.size} --spp {a.spp} --repeat {a.repeat} "
          f"(kernel time by device events, best of {a.repeat})")
    print(f"{'L':>5s} {'mode':6s} {'ms':>9s} {'Msamples/s':>11s} {'x0':>7s} {'tree KiB':>9s} {'build ms':>9s}")
    for L in [int(x) for x in a.lights.split(",")]:
        rc = RenderConfig(a.size, a.size, a.spp, PathTracingShader(50))
        sc = scenes.many_lights(L, a.kind, rc)
        build = float("inf")
        for _ in range(a.repeat):
            with DeviceScene(sc) as ds:
                ds.sync()
                t = time.perf_counter()
                ds.light_sampling("tree")
                build = min(build, (time.perf_counter() - t) * 1e3)
        rows = {}
        with DeviceScene(sc) as ds:
            ds.kernel_timing(True)
            for mode in ("uniform", "tree", "power"):
                ds.light_sampling(mode)
                rows[mode] = msamples(ds, a.size * a.size, a.spp, a.repeat)
            _, _, nbytes = ds.light_tree()
        for mode in ("uniform", "tree", "power"):
            ms_s, ms = rows[mode]
            extra = f" {nbytes / 1024:9.1f} {build:9.3f}" if mode == "tree" else ""
            print(f"{L:5d} {mode:6s} {ms:9.3f} {ms_s:11.1f} {ms_s / rows['uniform'][0]:7.2f}{extra}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
