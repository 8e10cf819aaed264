"""Times of the directional distance moments (sol_visibility_oct_dev / sol_volume_build_depth_dev / sol_volume_sample_depth_dev); it
writes profiles/volume_depth.txt. (The committed file is one run's output with headings and commentary added by hand.) The workload is BASELINE
config 3, the atrium at 1920x1080, as in tests/tools/volume_bench.py: probe grids over the world box, and the two million points where the frame's
camera rays hit. Everything is resident in device memory. A gather's time is one call through the Python method and the wait behind it; a
sampler's time is the host clock around a window of back-to-back calls (at least 0.1 s) that ends in a wait for the scene's stream. Repetitions
alternate between the candidates of a comparison; the least and the median of `--reps` are written down.

  isa      registers, scratch and LDS of the kernels in csrc/sol_depth.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  gather   visibility_oct at `--samples` samples, res 8, on a 32^3 and a 64^3 grid, beside visibility(distances=True) on the same points (the cost of
           going directional) and beside the round trip it replaces: per sample irradiance_rays + closest_hits + a torch accumulation of the same sums
  project  the same call at res 4, 8 and 16 on the 32^3 grid with the projection kernel of the product and with SOL_DEPTH_PROJECT=plain (a thread per
           texel that draws every direction itself); the gather kernel in front is the same, so the difference of the two is the projection kernels'
  sample   volume_sample over the surface points with depth maps and without, and over the same points moved onto a probe plane

  python tests/tools/volume_depth_bench.py [--parts isa,gather,project,sample] [--small] [--samples 256] [--reps 3] [--out profiles/volume_depth.txt]
A part that is not run is written down as "not measured".
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

import _paths  # noqa: F401
from volume_bench import floor_scene, timed

ROOT = _paths.ROOT


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "depth.s"), "csrc/sol_depth.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "depth.s")).read().splitlines()
    lds = [l.split(":")[1].strip() for l in text if ".group_segment_fixed_size:" in l]
    sgpr = [l.split(":")[1].strip() for l in text if l.strip().startswith(".sgpr_count:")]
    out.append("isa (tests/tools/isa.sh csrc/sol_depth.hip): LDS bytes in the order below: " + ", ".join(lds) + "; SGPRs: " + ", ".join(sgpr))
    out.extend("  " + l.strip() for l in r.stdout.splitlines())


def alternating(candidates, reps):
    """{name: (least ms, median ms)} of callables that wait for their own work; one warm-up each, then `reps` rounds in which they take turns"""
    for fn in candidates.values():
        fn()
    times = {k: [] for k in candidates}
    for _ in range(reps):
        for k, fn in candidates.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (min(v), float(np.median(v))) for k, v in times.items()}


def round_trip(ds, at, samples, seed, res, sharpness):
    """What visibility_oct replaces: per sample the rays, their closest hits, and the lobe-weighted sums in torch (one association: sample order)."""
    import torch
    import depth_ref as dr
    from solstrale_amd import _abi
    T =torch.from_numpy(dr.texel_directions(res)).cuda()
    sums = torch.zeros((at.shape[0], res * res, 4), dtype=torch.float32, device="cuda")
    for s in range(samples):
        rays, _ = ds.irradiance_rays(at, s, seed=seed, mode="sphere")
        hits = ds.closest_hits(rays)
        c = torch.clamp(rays[:, 4:7] @ T.T, min=0.0)
        for _ in range(sharpness):
            c = c * c
        hit = (hits[:, 3] == _abi.SOL_RAY_HIT)[:, None]
        t = hits[:, 0].contiguous().view(torch.float32)[:, None]
        sums[:, :, 0] += c
        sums[:, :, 1] += torch.where(hit, torch.zeros_like(c), c)
        sums[:, :, 2] += torch.where(hit, c * t, torch.zeros_like(c))
        sums[:, :, 3] += torch.where(hit, c * t * t, torch.zeros_like(c))
    torch.cuda.synchronize()
    return sums


def part_gpu(out, parts, small, samples, reps):
    import ctypes as C
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, VolumeGrid, _abi, scenes
    w, h = (480, 270) if small else (1920, 1080)
    sizes = (4, 8) if small else (32, 64)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed = 0x5017A1E
    d = sc.desc
    v = d.nodes[_abi.ref_index(d.root)].bbox.v
    lo, hi = np.array([v[0], v[2], v[4]]), np.array([v[1], v[3], v[5]])

    def grid_of(g, backface=True, chebyshev=True):
        cell = (hi - lo) / g
        return VolumeGrid(lo + 0.5 * cell, cell, (g, g, g), backface=backface, chebyshev=chebyshev, normal_bias=float(0.1 * cell.min())), float(2.0 * np.linalg.norm(cell))

    out.append(f"workload: sponza_like, {d.n_triangles} triangles, {w}x{h}; grids over the world box; {samples} samples per gather; least / median of {reps} alternating repetitions")
    if "gather" in parts:
        with DeviceScene(sc) as ds:
            for g in sizes:
                grid, radius = grid_of(g)
                at = ds.volume_points(grid, tmax=radius)
                kw = dict(samples=samples, seed=seed, mode="sphere")
                res = alternating({"oct": lambda: ds.visibility_oct(at, res=8, sharpness_log2=5, **kw), "iso": lambda: ds.visibility(at, distances=True, **kw),
                                   "trip": lambda: round_trip(ds, at, samples, seed, 8, 5)}, reps)
                rays = g ** 3 * samples
                out.append(f"gather {g}^3 = {g ** 3} probes x {samples} samples, res 8, sharpness_log2 5, radius {radius:.3f} (ms, least / median):")
                out.append(f"  visibility_oct {res['oct'][0]:9.3f} / {res['oct'][1]:9.3f}  ({rays / res['oct'][0] / 1e6:.2f} G rays/s)   visibility(distances) {res['iso'][0]:9.3f} / {res['iso'][1]:9.3f}"
                           f"   round trip {res['trip'][0]:9.3f} / {res['trip'][1]:9.3f}   oct / iso {res['oct'][0] / res['iso'][0]:.2f}   trip / oct {res['trip'][0] / res['oct'][0]:.1f}")
    if "project" in parts:
        g = sizes[0]
        grid, radius = grid_of(g)
        handles = {}
        try:
            for variant in ("wave", "plain"):
                os.environ.pop("SOL_DEPTH_PROJECT", None)
                if variant == "plain":
                    os.environ["SOL_DEPTH_PROJECT"] = "plain"
                handles[variant] = DeviceScene(sc).__enter__()  # (the override is read when the handle is made)
            os.environ.pop("SOL_DEPTH_PROJECT", None)
            at = handles["wave"].volume_points(grid, tmax=radius)
            kw = dict(samples=samples, seed=seed, mode="sphere", sharpness_log2=5)
            out.append(f"project {g}^3 probes x {samples} samples: visibility_oct with the product's projection kernel and with SOL_DEPTH_PROJECT=plain (ms, least / median)")
            for r in (4, 8, 16):
                res = alternating({k: (lambda k=k: handles[k].visibility_oct(at, res=r, **kw)) for k in handles}, reps)
                same = torch.equal(handles["wave"].visibility_oct(at, res=r, **kw).view(torch.int32), handles["plain"].visibility_oct(at, res=r, **kw).view(torch.int32))
                out.append(f"  res {r:2d}   wave {res['wave'][0]:9.3f} / {res['wave'][1]:9.3f}   plain {res['plain'][0]:9.3f} / {res['plain'][1]:9.3f}   plain - wave {res['plain'][0] - res['wave'][0]:9.3f}"
                           f"   the same words: {same}")
            iso = alternating({"iso": lambda: handles["wave"].visibility(at, distances=True, samples=samples, seed=seed, mode="sphere")}, reps)
            out.append(f"  visibility(distances) on the same points, the search alone: {iso['iso'][0]:9.3f} / {iso['iso'][1]:9.3f}")
        finally:
            for hnd in handles.values():
                hnd.__exit__(None, None, None)
    if "sample" in parts:
        g = sizes[0]
        grid, radius = grid_of(g)
        with DeviceScene(sc) as ds:
            cam = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8).contiguous()
            hits = ds.closest_hits(cam)
            ds.clear_aux()
            ds.render_aux(0, 1, seed)
            normal = torch.from_numpy(ds.read_aux()[1].reshape(-1, 3)).cuda()
            ds.clear_aux()
            ok = (hits[:, 3] == _abi.SOL_RAY_HIT) & (normal.abs().sum(dim=1) > 0.5)
            t = hits[:, 0].contiguous().view(torch.float32)
            points = torch.empty((int(ok.sum().item()), 8), dtype=torch.float32, device="cuda")
            points[:, 0:3] = (cam[:, 0:3] + t[:, None] * cam[:, 4:7])[ok]
            points[:, 3], points[:, 7] = 0.001, float("inf")
            points[:, 4:7] = normal[ok]
            del cam, hits, normal, t, ok
            n = int(points.shape[0])
            at = ds.volume_points(grid, tmax=radius)
            few = min(samples, 64)
            sh = ds.irradiance_sh(ds.volume_points(grid), samples=few, seed=seed, mode="sphere")
            vis = ds.visibility(at, samples=few, seed=seed, mode="sphere", distances=True)
            probes = ds.volume_build(grid, sh, vis, radius)
            depth = {r: ds.volume_build_depth(grid, ds.visibility_oct(at, res=r, sharpness_log2=5, samples=few, seed=seed), radius, res=r) for r in (4, 8, 16)}
        with DeviceScene(floor_scene()) as cheap:  # (the handle supplies the stream only)
            res_buf = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            oy, sy = np.float32(grid.origin[1]), np.float32(grid.spacing[1])
            snapped = points.clone()
            snapped[:, 1] = oy + torch.clamp(torch.round((points[:, 1] - oy) / sy), 0, g - 1) * sy
            out.append(f"sample: {n} points from {g}^3 probes built at {few} samples, us per call (least of {reps} windows of back-to-back calls); depth: sol_volume_sample_depth_dev")
            for name, pts, bias in (("surface points", points, grid.normal_bias), ("points on a probe plane", snapped, 0.0)):
                for bf, ch in ((True, True), (False, True), (True, False)):
                    rec = VolumeGrid(grid.origin, grid.spacing, grid.counts, backface=bf, chebyshev=ch, normal_bias=bias).record()
                    iso = timed(lambda: cheap._chk(cheap.lib.sol_volume_sample_dev(cheap.h, C.byref(rec), C.c_void_p(probes.data_ptr()), C.c_void_p(pts.data_ptr()), n,
                                                                                  C.c_void_p(res_buf.data_ptr()))), cheap.sync, reps)
                    line = f"  {name:24s} backface {int(bf)} chebyshev {int(ch)}   isotropic {iso * 1e3:8.1f} us"
                    for r in (4, 8, 16):
                        cfg = cheap._oct_config(r)
                        ms = timed(lambda: cheap._chk(cheap.lib.sol_volume_sample_depth_dev(cheap.h, C.byref(rec), C.c_void_p(probes.data_ptr()), C.c_void_p(depth[r].data_ptr()),
                                                                                           C.byref(cfg), C.c_void_p(pts.data_ptr()), n, C.c_void_p(res_buf.data_ptr()))), cheap.sync, reps)
                        line += f"   depth res {r:2d} {ms * 1e3:8.1f} us ({ms / iso:.2f} x)"
                    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,gather,project,sample")
    ap.add_argument("--small", action="store_true", help="a 20 000-triangle atrium at 480x270 and 4^3 / 8^3 grids (a rehearsal, not a measurement)")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_depth.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["directional distance moments (DESIGN.md 25): tests/tools/volume_depth_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    gpu_parts = [p for p in ("gather", "project", "sample") if p in parts]
    if gpu_parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("volume_depth_bench: no HIP device visible; parts gather, project and sample have nothing to measure without one")
        part_gpu(out, gpu_parts, a.small, a.samples, a.reps)
    out.extend(f"{p}: not measured" for p in ("isa", "gather", "project", "sample") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
