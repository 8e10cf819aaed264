"""Times of the lightmap mip chain (sol_lightmap_mips_dev / sol_lightmap_sample_lod_dev / sol_lightmap_lod_dev); it writes
profiles/lightmap_mips.txt. (The committed file is one run's output with commentary added by hand.) The atlas is profiles/lightmap_sample.txt's: the
jittered grid mesh (cells of 4 x 4 texels, two triangles each) filling 4096 x 4096 texels, rasterised on the device. Everything is resident in
device memory, outputs allocated beforehand. A call's time is the host clock around a window of back-to-back calls (at least 0.1 s of them) that
ends in a wait for the scene's stream, per call, the least of `--reps` windows after a warm-up.

  isa      registers, scratch and LDS of the kernels in csrc/sol_lightmap_mips.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  chain    the full chain at 3 channels (SolRadiance rows) and 27 (SolSh9 rows), with the tail kernel (the product) and without (SOL_LIGHTMAP_MIPS=levels,
           read at every call) in the same run, the answers compared byte for byte; beside them the time of streaming level 0 once at the
           roofline's HBM rate and a 4-pass sol_lightmap_dilate_dev of the same rows
  lookup   two million surface rows in texel order and in random order, lods all 0, all 0.5 and all 2.5, against sol_lightmap_sample_dev over the
           same rows; 3 channels and 27
  lod      sol_lightmap_lod_dev over two million synthetic hits of the grid mesh
  view     lightmap_view_lod at 1920 x 1080 over the atrium (a chart per triangle) beside lightmap_view, through the Python methods

  python tests/tools/lightmap_mips_bench.py [--parts isa,chain,lookup,lod,view] [--small] [--reps 3] [--out profiles/lightmap_mips.txt]
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
import lightmap_sample_ref as sr
from lightmap_bench import floor_scene, grid_mesh, points_call, timed

ROOT = _paths.ROOT
F = np.float32
HBM_PEAK_GBPS = 8000.0  # bench.py's roofline peak, as tests/tools/volume_bench.py
PARTS = ("isa", "chain", "lookup", "lod", "view")


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "lmm.s"), "csrc/sol_lightmap_mips.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "lmm.s")).read().splitlines()
    lds = [l.split(":")[1].strip() for l in text if l.strip().startswith(".group_segment_fixed_size:")]
    sgpr = [l.split(":")[1].strip() for l in text if l.strip().startswith(".sgpr_count:")]
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_mips.hip): in the order below, static LDS bytes (the tail kernel's LDS is dynamic: at most 62720): "
               + ", ".join(lds) + "; SGPRs: " + ", ".join(sgpr))
    out.extend("  " + l.strip() for l in r.stdout.splitlines())


def p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def part_gpu(out, parts, small, reps):
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, lightmap_mip_layout, lightmap_triangle_table, pixel_spread, scenes
    W = H = 512 if small else 4096
    n = 100000 if small else 2000000
    rng = np.random.default_rng(7)
    V, T, N = grid_mesh(W // 4)
    lay = lightmap_mip_layout(W, H)
    with DeviceScene(floor_scene()) as ds:  # (the handle supplies the stream and the scratch only)
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        points = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
        texels = torch.empty((W * H, 4), dtype=torch.int32, device="cuda")
        points_call(ds, dV, None, dT, len(V), W, H, points, texels)
        ds.sync()
        del points
        pass_of = torch.zeros((H, W), dtype=torch.uint8, device="cuda")  # (the mesh fills the atlas: every texel owned)
        out.append(f"workload: the jittered grid mesh, {len(V)} triangles, over a {W} x {H} atlas; {lay['levels']} levels, {lay['rows']} chain rows")
        chains = {}
        for channels, words in ((3, 4), (27, 28)):
            values = torch.from_numpy(rng.normal(size=(W * H, words)).astype(F)).cuda()
            mips = torch.empty((lay["rows"], words), dtype=torch.float32, device="cuda")
            cover = torch.empty((lay["rows"],), dtype=torch.uint8, device="cuda")
            chains[channels] = (values, mips, cover, words)
            if "chain" not in parts:
                ds._chk(ds.lib.sol_lightmap_mips_dev(ds.h, p(texels), p(pass_of), W, H, p(values), channels, 4 * words, 0, p(mips), p(cover)))
                ds.sync()
                continue
            mips2, cover2 = torch.empty_like(mips), torch.empty_like(cover)

            def call(m, c):
                ds._chk(ds.lib.sol_lightmap_mips_dev(ds.h, p(texels), p(pass_of), W, H, p(values), channels, 4 * words, 0, p(m), p(c)))

            os.environ["SOL_LIGHTMAP_MIPS"] = "levels"
            ms_levels = timed(lambda: call(mips2, cover2), ds.sync, reps)
            os.environ.pop("SOL_LIGHTMAP_MIPS")
            ms_tail = timed(lambda: call(mips, cover), ds.sync, reps)
            equal = bool(torch.equal(mips.view(torch.int32), mips2.view(torch.int32)) and torch.equal(cover, cover2))
            dil = torch.empty_like(values)
            ms_dilate = timed(lambda: ds._chk(ds.lib.sol_lightmap_dilate_dev(ds.h, p(texels), W, H, p(values), channels, 4 * words, 4, p(dil), None)), ds.sync, reps)
            del dil, mips2, cover2
            stream_us = W * H * (4 * words + 1) / (HBM_PEAK_GBPS * 1e9) * 1e6
            out.append(f"  chain {channels:2d} channels ({4 * words:3d} B rows)  default path {ms_tail * 1e3:9.1f} us   level launches only {ms_levels * 1e3:9.1f} us   "
                       f"(tail kernel {'used' if words <= 12 else 'not used: the rows do not fit LDS'}; equal byte for byte: {equal})   level 0 streamed once at "
                       f"{HBM_PEAK_GBPS / 1000:.0f} TB/s {stream_us:7.1f} us ({ms_tail * 1e3 / stream_us:.2f} x)   4-pass lightmap_dilate {ms_dilate * 1e3:9.1f} us")
        if "chain" in parts:  # smaller atlases, where the tail is a larger share of the chain: 3 channels, every texel owned
            for S in (64, 256, 1024):
                rows = lightmap_mip_layout(S, S)["rows"]
                v = torch.from_numpy(rng.normal(size=(S * S, 4)).astype(F)).cuda()
                t = torch.zeros((S * S, 4), dtype=torch.int32, device="cuda")
                m, c = torch.empty((rows, 4), dtype=torch.float32, device="cuda"), torch.empty((rows,), dtype=torch.uint8, device="cuda")
                ms = {}
                for shape in ("levels", "default"):
                    if shape == "levels":
                        os.environ["SOL_LIGHTMAP_MIPS"] = "levels"
                    ms[shape] = timed(lambda: ds._chk(ds.lib.sol_lightmap_mips_dev(ds.h, p(t), None, S, S, p(v), 3, 16, 0, p(m), p(c))), ds.sync, reps)
                    os.environ.pop("SOL_LIGHTMAP_MIPS", None)
                out.append(f"  chain  3 channels, {S:4d} x {S:4d}: default path {ms['default'] * 1e3:8.1f} us   level launches only {ms['levels'] * 1e3:8.1f} us")
        b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
        rand = np.zeros(n, dtype=sr.TEXEL_DTYPE)
        rand["triangle"], rand["b1"], rand["b2"], rand["flags"] = rng.integers(0, len(V), n), b[:, 1], b[:, 2], 1
        sets = {"texel order": texels[:n].contiguous(), "random": torch.from_numpy(rand.view(np.int32).reshape(-1, 4)).cuda()}
        if "lookup" in parts:
            for channels in (3, 27):
                values, mips, cover, words = chains[channels]
                res, res2 = (torch.empty((n, channels + 1), dtype=torch.float32, device="cuda") for _ in range(2))
                cfg = _abi.SolLightmapLodConfig(size=40, width=W, height=H, channels=channels, stride_bytes=4 * words, flags=0, chart_radius=float("inf"), levels=0)
                cfg0 = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=channels, stride_bytes=4 * words, flags=0, chart_radius=float("inf"))
                for which, coords in sets.items():
                    ms0 = timed(lambda: ds._chk(ds.lib.sol_lightmap_sample_dev(ds.h, C.byref(cfg0), p(dT), len(T), p(texels), p(pass_of), p(values), None, None,
                                                                               p(coords), n, p(res2))), ds.sync, reps)
                    line = f"  lookup {channels:2d} channels {which:11s} lightmap_sample {ms0 * 1e3:9.1f} us"
                    for lod in (0.0, 0.5, 2.5):
                        lods = torch.full((n,), lod, dtype=torch.float32, device="cuda")
                        ms = timed(lambda: ds._chk(ds.lib.sol_lightmap_sample_lod_dev(ds.h, C.byref(cfg), p(dT), len(T), p(texels), p(pass_of), p(values), p(mips),
                                                                                      p(cover), None, None, p(coords), p(lods), n, p(res))), ds.sync, reps)
                        line += f"   lod {lod}: {ms * 1e3:9.1f} us ({ms / ms0:.2f} x)"
                        if lod == 0.0:
                            line += f" equal word for word: {bool(torch.equal(res.view(torch.int32), res2.view(torch.int32)))}"
                    out.append(line)
                del res, res2
        if "lod" in parts:
            hits = np.zeros(n, dtype=sr.HIT_DTYPE)
            hits["status"], hits["kind"], hits["t"] = 1, 4, rng.uniform(1.0, 50.0, n)
            rays = rng.normal(size=(n, 8)).astype(F)
            d_rays, d_hits = torch.from_numpy(rays).cuda(), torch.from_numpy(hits.view(np.int32).reshape(-1, 8)).cuda()
            res = torch.empty((n,), dtype=torch.float32, device="cuda")
            for which, coords in sets.items():
                ms = timed(lambda: ds._chk(ds.lib.sol_lightmap_lod_dev(ds.h, p(d_rays), p(d_hits), p(coords), n, p(dV), p(dT), len(V), W, H, 0.001, 0.0, p(res))),
                           ds.sync, reps)
                stream_us = n * (32 + 32 + 16 + 60 + 4) / (HBM_PEAK_GBPS * 1e9) * 1e6
                out.append(f"  lod {which:11s} sol_lightmap_lod_dev over {n} hits {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s  144 B/row unshared = {stream_us:.1f} us at "
                           f"{HBM_PEAK_GBPS / 1000:.0f} TB/s ({ms * 1e3 / stream_us:.2f} x); answers above 0: {int((res > 0).sum())}")
    if "view" in parts:
        from solstrale_amd import lightmap_mesh
        w, h = (480, 270) if small else (1920, 1080)
        sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(w, h, 16))
        nt = int(sc.desc.n_triangles)
        table = lightmap_triangle_table(sc, 0, nt)
        side = int(np.ceil(np.sqrt(nt)))  # every triangle a chart of its own: cell k of a square grid of cells
        k = np.arange(nt)
        cx, cy = (k % side).astype(np.float64) / side, (k // side).astype(np.float64) / side
        corner = np.asarray([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)]) / side
        uvs = np.stack([np.stack([cx + corner[c, 0], cy + corner[c, 1]], axis=-1) for c in range(3)], axis=1).astype(F)
        with DeviceScene(sc) as ds:
            d_uvs, d_table = torch.from_numpy(uvs).cuda(), torch.from_numpy(table.view(np.int32)).cuda()
            V2, _ = lightmap_mesh(sc, 0, nt)
            dV2 = torch.from_numpy(V2).cuda()
            p2, t2 = ds.lightmap_points(dV2, d_uvs, W, H)
            del p2
            baked, pass_of = ds.lightmap_dilate(torch.from_numpy(rng.normal(size=(W * H, 4)).astype(F)).cuda(), t2, W, H, passes=2, return_pass_of=True)
            mips, cover = ds.lightmap_mips(baked, t2, W, H, pass_of=pass_of)
            seed, spread = 0x5017A1E, pixel_spread(40.0, h)

            def once(fn):
                best, r = float("inf"), None
                for i in range(reps + 1):  # (the first is the warm-up; every Python method waits for the scene's stream before it returns)
                    t0 = time.perf_counter()
                    r = fn()
                    best = min(best, time.perf_counter() - t0) if i else best
                return best * 1e3, r
            ms_plain, _ = once(lambda: ds.lightmap_view(baked, d_uvs, t2, W, H, d_table, 0, 0, w, h, sample=0, seed=seed, pass_of=pass_of))
            ms_lod, view = once(lambda: ds.lightmap_view_lod(baked, mips, cover, d_uvs, t2, W, H, d_table, dV2, 0, 0, w, h, spread, sample=0, seed=seed, pass_of=pass_of))
            rays = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8)
            hits = ds.closest_hits(rays)
            coords = ds.lightmap_coords(hits, d_table)
            ms_l, lods = once(lambda: ds.lightmap_lod(rays, hits, coords, dV2, d_uvs, W, H, spread))
            ms_s, _ = once(lambda: ds.lightmap_sample_lod(baked, mips, cover, lods, coords, d_uvs, t2, W, H, pass_of=pass_of))
            hit = lods[lods > 0]
            out.append(f"view: the atrium, {nt} triangles, {w}x{h}, a {W} x {H} atlas with a chart per triangle, ms per call through the Python methods (each waits "
                       f"for the stream): lightmap_view {ms_plain:8.3f}   lightmap_view_lod {ms_lod:8.3f}   of it lightmap_lod {ms_l:8.3f}, lightmap_sample_lod "
                       f"{ms_s:8.3f}; pixels with lod > 0: {int(hit.numel())}/{w * h}, mean {float(hit.mean()) if hit.numel() else 0.0:.2f}, largest {float(lods.max()):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--small", action="store_true", help="a 512 x 512 atlas, 100 000 rows, a 20 000-triangle atrium at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_mips.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["lightmap mip chains (DESIGN.md 31): tests/tools/lightmap_mips_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    gpu_parts = [x for x in PARTS[1:] if x in parts]
    if gpu_parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_mips_bench: no HIP device visible; only part isa has something to measure without one")
        part_gpu(out, gpu_parts, a.small, a.reps)
    out.extend(f"{x}: not measured" for x in PARTS if x not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
