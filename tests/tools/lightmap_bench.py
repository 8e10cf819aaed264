"""Times of the lightmap rasteriser and the border dilation (sol_lightmap_points_dev / sol_lightmap_dilate_dev); its output is
profiles/lightmap.txt. Everything is resident in device memory, outputs allocated beforehand; a time is the host clock around a window of back-to-back
calls (at least 0.1 s of them) that ends in a wait for the scene's stream, per call, the least of `--reps` windows after a warm-up: launches and
the two clears of a call are inside it.

  isa      registers, scratch and LDS of the kernels in csrc/sol_lightmap.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  ab       the claim pass's candidates at both extremes on a 4096 x 4096 atlas - one triangle over the whole atlas, and a million triangles smaller
           than a texel - each as the product's hybrid (lane <= 16 texels < wave <= 64 tiles < device), a lane per triangle (SOL_LIGHTMAP_CLAIM=lane)
           and a wave per triangle (SOL_LIGHTMAP_CLAIM=wave); beside them the call over no triangles (the clear and the emit pass alone)
  bake     at 1024^2 and 4096^2, over a jittered grid mesh that fills the atlas (cells of 4 x 4 texels, two triangles each): lightmap_points,
           a 4-pass lightmap_dilate of SolRadiance rows, and for proportion a 64-sample irradiance over the same rows (a floor under a quad light)
  restate  the numpy restatement (tests/lightmap_ref.py) on the same input: the Python loop over triangles this call replaces (no GPU needed)

  python tests/tools/lightmap_bench.py [--parts isa,ab,bake,restate] [--sizes 1024,4096] [--restate-sizes 1024] [--reps 3] [--out profiles/lightmap.txt]
A part that is not run is written down as "not measured".
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

import _paths  # noqa: F401
import lightmap_ref as lr

ROOT = _paths.ROOT
F = np.float32


def grid_mesh(cells, seed=1, jitter=0.35):
    """lightmap_ref.grid_mesh without its Python loop: a cells x cells jittered grid tiling [0, 1]^2, on the plane y = 0, normals up."""
    rng = np.random.default_rng(seed)
    g = np.linspace(0.0, 1.0, cells + 1)
    u, v = np.meshgrid(g, g)
    u[1:-1, 1:-1] += rng.uniform(-jitter, jitter, (cells - 1, cells - 1)) / cells
    v[1:-1, 1:-1] += rng.uniform(-jitter, jitter, (cells - 1, cells - 1)) / cells
    t = np.stack([u, v], axis=-1).astype(F)
    a, b, c, d = t[:-1, :-1], t[:-1, 1:], t[1:, 1:], t[1:, :-1]
    T = np.stack([np.stack([a, c, b], axis=2), np.stack([a, d, c], axis=2)], axis=2).reshape(-1, 3, 2)  # (wound so that the normals point up)
    return lr.lift(T), np.ascontiguousarray(T), np.broadcast_to(np.asarray((0, 1, 0), dtype=F), T.shape[:2] + (3,)).copy()


def timed(fn, sync, reps):
    """ms per call: after a warm-up, `reps` windows of back-to-back calls ended by one wait for the stream, each window at least 0.1 s long (or
    one call, if a call is longer); the least window counts."""
    fn(); sync()
    t0 = time.perf_counter()
    fn(); sync()
    inner = max(1, min(500, int(0.1 / max(time.perf_counter() - t0, 1e-6))))
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        best = min(best, (time.perf_counter() - t0) / inner)
    return best * 1e3


def floor_scene():
    from solstrale_amd import CameraConfig, RenderConfig, SceneBuilder
    b = SceneBuilder()
    floor = b.Quad((-2.0, 0.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), b.Lambertian(b.SolidColor(0.7, 0.7, 0.7)))
    light = b.Quad((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), b.DiffuseLight(8, 8, 8))
    return b.finish(b.Bvh([floor, light]), CameraConfig(40.0, 0.0, (0.0, 6.0, 6.0), (0.0, 0.0, 0.0), (0, 1, 0)), (0.0, 0.0, 0.0), RenderConfig(32, 32, 1))


def points_call(ds, dV, dN, dT, n, W, H, points, texels, conservative=False):
    from solstrale_amd import _abi
    cfg = _abi.SolLightmapConfig(size=32, width=W, height=H, flags=1 if conservative else 0, tmin=1e-3, tmax=float("inf"))
    ds._chk(ds.lib.sol_lightmap_points_dev(ds.h, C.c_void_p(dV.data_ptr()) if n else None, C.c_void_p(dN.data_ptr()) if dN is not None else None,
                                            C.c_void_p(dT.data_ptr()) if n else None, n, C.byref(cfg), C.c_void_p(points.data_ptr()), C.c_void_p(texels.data_ptr())))


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "lightmap.s"), "csrc/sol_lightmap.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        lds = sorted(set(l.split(":")[1].strip() for l in open(os.path.join(tmp, "lightmap.s")) if ".group_segment_fixed_size:" in l))
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap.hip): LDS bytes of every kernel: " + ", ".join(lds))
    out.extend("  " + l.strip() for l in r.stdout.splitlines())


def part_ab(out, reps):
    import torch
    from solstrale_amd import DeviceScene
    W = H = 4096
    rng = np.random.default_rng(7)
    n_small = 1 << 20
    c = rng.uniform(0, 1, (n_small, 1, 2))
    small = (c + rng.uniform(-1, 1, (n_small, 3, 2)) * (0.4 / W)).astype(F)  # boxes of at most 0.8 texels
    whole = np.asarray([[(-0.5, -0.5), (2.5, -0.5), (-0.5, 2.5)]], dtype=F)
    cases = (("one triangle over the whole atlas", whole), (f"{n_small} triangles smaller than a texel", small), ("no triangles (clear + emit)", whole[:0]))
    points = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
    texels = torch.empty((W * H, 4), dtype=torch.int32, device="cuda")
    out.append(f"ab: claim-pass candidates, {W} x {H} atlas, ms per sol_lightmap_points_dev call (clear + claim + emit), centre / conservative")
    for variant in ("hybrid", "lane", "wave"):
        os.environ.pop("SOL_LIGHTMAP_CLAIM", None)
        if variant != "hybrid":
            os.environ["SOL_LIGHTMAP_CLAIM"] = variant
        with DeviceScene(floor_scene()) as ds:
            for name, T in cases:
                dT, dV = torch.from_numpy(T).cuda(), torch.from_numpy(lr.lift(T)).cuda()
                ms = [timed(lambda: points_call(ds, dV, None, dT, len(T), W, H, points, texels, cons), ds.sync, reps) for cons in (False, True)]
                owned = int((texels[:, 0] != -1).sum().item())
                out.append(f"  {variant:6s}  {name:45s} {ms[0]:10.3f} / {ms[1]:10.3f} ms   texels owned {owned}")
    os.environ.pop("SOL_LIGHTMAP_CLAIM", None)


def part_bake(out, sizes, reps):
    import torch
    from solstrale_amd import DeviceScene
    out.append("bake: jittered grid mesh filling the atlas (cells of 4 x 4 texels), ms per call, device route")
    with DeviceScene(floor_scene()) as ds:
        for W in sizes:
            V, T, N = grid_mesh(W // 4)
            dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
            points = torch.empty((W * W, 8), dtype=torch.float32, device="cuda")
            texels = torch.empty((W * W, 4), dtype=torch.int32, device="cuda")
            ms_points = timed(lambda: points_call(ds, dV, dN, dT, len(T), W, W, points, texels), ds.sync, reps)
            ms_cons = timed(lambda: points_call(ds, dV, dN, dT, len(T), W, W, points, texels, True), ds.sync, reps)
            owned = int((texels[:, 0] != -1).sum().item())
            rows = ds.irradiance(points, samples=64, seed=1)
            ms_irr = timed(lambda: ds.irradiance(points, samples=64, seed=1), lambda: None, reps)
            # a chart with borders to fill: the texels outside the middle three quarters count as unowned
            j, i = torch.meshgrid(torch.arange(W, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
            border = ((i < W // 8) | (i >= W - W // 8) | (j < W // 8) | (j >= W - W // 8)).reshape(-1)
            chart = texels.clone()
            chart[border, 0] = -1
            baked = torch.empty_like(rows)

            def dilate():
                ds._chk(ds.lib.sol_lightmap_dilate_dev(ds.h, C.c_void_p(chart.data_ptr()), W, W, C.c_void_p(rows.data_ptr()), 3, 16, 4, C.c_void_p(baked.data_ptr()), None))

            ms_dilate = timed(dilate, ds.sync, reps)
            out.append(f"  {W:5d}^2  {len(T):8d} triangles  lightmap_points {ms_points:9.3f} ms (conservative {ms_cons:9.3f})  owned {owned}/{W * W}  "
                       f"lightmap_dilate x4 {ms_dilate:9.3f} ms  irradiance 64 samples {ms_irr:10.1f} ms ({W * W * 64 / ms_irr / 1e6:.2f} G paths/s)")
            del points, texels, rows, chart, baked, dV, dT, dN


def part_restate(out, sizes):
    out.append("restate: tests/lightmap_ref.py (numpy float32, a Python loop over triangles) on the bake's input, seconds on the host")
    for W in sizes:
        V, T, N = grid_mesh(W // 4)
        t0 = time.perf_counter()
        _, texels = lr.lightmap_points(V, T, W, W, normals=N)
        s_points = time.perf_counter() - t0
        t0 = time.perf_counter()
        lr.lightmap_dilate(np.zeros((W * W, 4), dtype=F), texels, W, W, passes=4, channels=3)
        out.append(f"  {W:5d}^2  {len(T):8d} triangles  lightmap_points {s_points:9.2f} s  lightmap_dilate x4 {time.perf_counter() - t0:7.2f} s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,ab,bake,restate")
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--restate-sizes", default="1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["lightmap texel points and border dilation (DESIGN.md 23): tests/tools/lightmap_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    if "ab" in parts or "bake" in parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_bench: no HIP device visible; parts ab and bake have nothing to measure without one")
    if "ab" in parts:
        part_ab(out, a.reps)
    if "bake" in parts:
        part_bake(out, [int(x) for x in a.sizes.split(",")], a.reps)
    if "restate" in parts:
        part_restate(out, [int(x) for x in a.restate_sizes.split(",")])
    out.extend(f"{p}: not measured" for p in ("isa", "ab", "bake", "restate") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
