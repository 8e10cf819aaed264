"""Times of the irradiance volume (sol_volume_points_dev / sol_volume_build_dev / sol_volume_sample_dev); it writes
profiles/volume.txt. (The committed file is one run's output with headings, commentary and a fifth part added by hand; its first paragraph says
which lines are which.) The workload is BASELINE config 3, the atrium at 1920x1080: the points are where the frame's camera rays (sample 0) hit,
with the normals of the auxiliary normal plane (what tests/tools/irradiance_bench.py makes), about two million; the volume is a 32^3 grid over the
world box. Everything is resident in device memory, outputs allocated beforehand. A short call's time is the host clock around a window of
back-to-back calls (at least 0.1 s of them) that ends in a wait for the scene's stream, per call, the least of `--reps` windows after a warm-up;
a gather's time is one call and the wait behind it, the least of `--reps`.

  isa      registers, scratch and LDS of the kernels in csrc/sol_volume.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  chain    on the atrium's handle: volume_points, irradiance_sh and visibility at `--samples` samples over the 32^3 probes, volume_build,
           volume_sample over the surface points - beside the `--samples`-sample irradiance call over the same surface points that the chain replaces
  sample   sol_volume_sample_dev over the same points and probes in both kernel shapes - the product (a zero-weight corner is not fetched) and
           SOL_VOLUME_SAMPLE=loadall (all eight corners fetched whatever their weight) -, under all four flag combinations and over the same
           points moved onto a probe plane, where the skip has work; beside
           it the time to stream 48 bytes per point at the 8 TB/s HBM peak bench.py --full uses for its roofline. Both shapes' words are compared.
  restate  the numpy restatement (tests/volume_ref.py) over the same points on the host's CPU, compared word for word with the device

  python tests/tools/volume_bench.py [--parts isa,chain,sample,restate] [--small] [--samples 64] [--reps 3] [--out profiles/volume.txt]
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
import volume_ref as vr

ROOT = _paths.ROOT
HBM_PEAK_GBPS = 8000.0  # bench.py's roofline peak


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


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "volume.s"), "csrc/sol_volume.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "volume.s")).read().splitlines()
    lds = sorted(set(l.split(":")[1].strip() for l in text if ".group_segment_fixed_size:" in l))
    sgpr = [l.split(":")[1].strip() for l in text if l.strip().startswith(".sgpr_count:")]
    out.append("isa (tests/tools/isa.sh csrc/sol_volume.hip): LDS bytes of every kernel: " + ", ".join(lds) + "; SGPRs in the order below: " + ", ".join(sgpr))
    out.extend("  " + l.strip() for l in r.stdout.splitlines())


def sample_call(ds, rec, probes, points, out):
    import ctypes as C
    ds._chk(ds.lib.sol_volume_sample_dev(ds.h, C.byref(rec), C.c_void_p(probes.data_ptr()), C.c_void_p(points.data_ptr()), int(points.shape[0]), C.c_void_p(out.data_ptr())))


def part_gpu(out, parts, small, samples, reps):
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, VolumeGrid, _abi, scenes
    w, h = (480, 270) if small else (1920, 1080)
    g = 8 if small else 32
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed = 0x5017A1E
    with DeviceScene(sc) as ds:
        # the surface points: hit positions of the frame's camera rays, normals from the auxiliary normal plane (tests/tools/irradiance_bench.py)
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
        d = sc.desc
        v = d.nodes[_abi.ref_index(d.root)].bbox.v
        lo, hi = np.array([v[0], v[2], v[4]]), np.array([v[1], v[3], v[5]])
        cell = (hi - lo) / g
        radius = float(2.0 * np.linalg.norm(cell))

        def grid_of(backface=True, chebyshev=True):
            return VolumeGrid(lo + 0.5 * cell, cell, (g, g, g), backface=backface, chebyshev=chebyshev, normal_bias=float(0.1 * cell.min()))

        grid = grid_of()
        rec = grid.record()
        out.append(f"workload: sponza_like, {d.n_triangles} triangles, {w}x{h}: {n} surface points; a {g}^3 grid over the world box, spacing "
                   f"{cell[0]:.3f} x {cell[1]:.3f} x {cell[2]:.3f}, normal_bias {grid.normal_bias:.4f}, moment radius {radius:.3f}; {samples} samples per gather")

        def once(fn):
            best = float("inf")
            for _ in range(reps + 1):  # (the first is the warm-up)
                t0 = time.perf_counter()
                r = fn()
                best = min(best, time.perf_counter() - t0) if _ else best
            return best * 1e3, r

        # the chain (every Python method waits for the scene's stream before it returns)
        ms_points, at = once(lambda: ds.volume_points(grid))
        ms_sh, sh = once(lambda: ds.irradiance_sh(at, samples=samples, seed=seed, mode="sphere"))
        at_r = ds.volume_points(grid, tmax=radius)
        ms_vis, vis = once(lambda: ds.visibility(at_r, samples=samples, seed=seed, mode="sphere", distances=True))
        ms_build, probes = once(lambda: ds.volume_build(grid, sh, vis, radius))
        ms_sample, lit = once(lambda: ds.volume_sample(grid, probes, points))
        flags = probes[:, 29].contiguous().view(torch.int32)
        count = lit[:, 3].contiguous().view(torch.int32)
        if "chain" in parts:
            ms_irr, direct = once(lambda: ds.irradiance(points, samples=samples, seed=seed))
            points_buf = torch.empty((g ** 3, 8), dtype=torch.float32, device="cuda")
            probes_buf = torch.empty((g ** 3, 32), dtype=torch.float32, device="cuda")
            import ctypes as C
            ms_points_dev = timed(lambda: ds._chk(ds.lib.sol_volume_points_dev(ds.h, C.byref(rec), 1e-3, float("inf"), C.c_void_p(points_buf.data_ptr()))), ds.sync, reps)
            ms_build_dev = timed(lambda: ds._chk(ds.lib.sol_volume_build_dev(ds.h, C.byref(rec), C.c_void_p(sh.data_ptr()), C.c_void_p(vis.data_ptr()), radius,
                                                                              C.c_void_p(probes_buf.data_ptr()))), ds.sync, reps)
            total = ms_points + ms_sh + ms_vis + ms_build + ms_sample
            out.append(f"chain: ms per call through the Python methods (each waits for the stream), {g}^3 = {g ** 3} probes, {n} points")
            out.append(f"  volume_points {ms_points:9.3f}   irradiance_sh x{samples} {ms_sh:9.3f}   visibility x{samples} {ms_vis:9.3f}   volume_build {ms_build:9.3f}   "
                       f"volume_sample {ms_sample:9.3f}   sum {total:9.3f} ms")
            out.append(f"  irradiance x{samples} over the same {n} points (what the chain replaces): {ms_irr:9.1f} ms - the chain takes 1/{ms_irr / total:.1f} of it, "
                       f"a resample of the baked volume 1/{ms_irr / ms_sample:.0f}")
            out.append(f"  back-to-back device calls at {g}^3: sol_volume_points_dev {ms_points_dev * 1e3:8.1f} us, sol_volume_build_dev {ms_build_dev * 1e3:8.1f} us")
            out.append(f"  probes valid {int((flags & 1).ne(0).sum())}/{g ** 3}, with moments {int((flags & 2).ne(0).sum())}; points answered {int(count.ne(0).sum())}/{n}, "
                       f"mean probes per point {float(count.float().mean()):.2f}; mean irradiance volume {[round(float(x), 4) for x in lit[:, :3].double().mean(0)]} "
                       f"direct pi * sum / samples {[round(float(x) * np.pi / samples, 4) for x in direct[:, :3].double().mean(0)]}")
        if "sample" in parts:
            stream_us = n * 48 / (HBM_PEAK_GBPS * 1e9) * 1e6
            out.append(f"sample: sol_volume_sample_dev, {n} points from {g}^3 probes, us per call and G points/s; 48 bytes per point at {HBM_PEAK_GBPS / 1000:.0f} TB/s: {stream_us:.1f} us")
            answers = {}
            for variant in ("product", "loadall"):
                os.environ.pop("SOL_VOLUME_SAMPLE", None)
                if variant == "loadall":
                    os.environ["SOL_VOLUME_SAMPLE"] = "loadall"
                with DeviceScene(floor_scene()) as cheap:  # (the handle supplies the stream only; the override is read when it is made)
                    res = torch.empty((n, 4), dtype=torch.float32, device="cuda")
                    for bf, ch in ((True, True), (False, False), (True, False), (False, True)):
                        r = grid_of(bf, ch).record()
                        ms = timed(lambda: sample_call(cheap, r, probes, points, res), cheap.sync, reps)
                        answers[(variant, bf, ch)] = res.clone()
                        out.append(f"  {variant:8s} backface {int(bf)} chebyshev {int(ch)}  {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G points/s  {ms * 1e3 / stream_us:6.2f} x the stream time")
                    # where the skip has work: the same points moved onto the nearest probe plane along y (a lightmap of an axis-aligned floor), no bias
                    flat = VolumeGrid(grid.origin, grid.spacing, grid.counts, backface=False, chebyshev=False, normal_bias=0.0)
                    oy, sy = np.float32(flat.origin[1]), np.float32(flat.spacing[1])
                    snapped = points.clone()
                    snapped[:, 1] = oy + torch.clamp(torch.round((points[:, 1] - oy) / sy), 0, g - 1) * sy
                    r = flat.record()
                    ms = timed(lambda: sample_call(cheap, r, probes, snapped, res), cheap.sync, reps)
                    answers[(variant, "plane")] = res.clone()
                    corners = float(res[:, 3].contiguous().view(torch.int32).float().mean())
                    out.append(f"  {variant:8s} points on a probe plane, no flags  {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G points/s  corners with weight per point {corners:.2f}")
            os.environ.pop("SOL_VOLUME_SAMPLE", None)
            same = torch.equal(answers[("product", "plane")].view(torch.int32), answers[("loadall", "plane")].view(torch.int32)) and all(torch.equal(answers[("product",) + k].view(torch.int32), answers[("loadall",) + k].view(torch.int32)) for k in ((True, True), (False, False), (True, False), (False, True)))
            out.append(f"  the two shapes answer the same words: {same}")
        if "restate" in parts:
            h_probes, h_points = probes.cpu().numpy(), points.cpu().numpy()
            t0 = time.perf_counter()
            want = vr.volume_sample(grid, h_probes, h_points)
            s = time.perf_counter() - t0
            equal = bool((want.view(np.uint32) == lit.cpu().numpy().view(np.uint32)).all())
            out.append(f"restate: tests/volume_ref.py (numpy float32) over the same {n} points on the host: {s:8.2f} s ({n / s / 1e6:.2f} M points/s); equal to the device word for word: {equal}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,chain,sample,restate")
    ap.add_argument("--small", action="store_true", help="a 20 000-triangle atrium at 480x270 and an 8^3 grid (a rehearsal, not a measurement)")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["irradiance volumes (DESIGN.md 24): tests/tools/volume_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    gpu_parts = [p for p in ("chain", "sample", "restate") if p in parts]
    if gpu_parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("volume_bench: no HIP device visible; parts chain, sample and restate have nothing to measure without one")
        part_gpu(out, gpu_parts, a.small, a.samples, a.reps)
    out.extend(f"{p}: not measured" for p in ("isa", "chain", "sample", "restate") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
