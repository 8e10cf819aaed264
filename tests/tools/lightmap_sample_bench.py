"""Times of the lightmap lookups (sol_lightmap_coords_dev / sol_lightmap_sample_dev); it writes profiles/lightmap_sample.txt. (The
committed file is one run's output with headings and commentary added by hand; its first paragraph says which lines are which.) The atlas is
profiles/lightmap.txt's: the jittered grid mesh (cells of 4 x 4 texels, two triangles each) filling 4096 x 4096 texels, rasterised on the device;
the values are random rows, SolRadiance (3 channels, 16 bytes) and SolSh9 (27 channels, 112 bytes). Two sets of two million surface rows:
`random` - a random triangle and random weights each, incoherent - and `texel order` - the atlas's own SolTexel rows from the first texel on,
coherent. Everything is resident in device memory, outputs allocated beforehand. A call's time is the host clock around a window of back-to-back
calls (at least 0.1 s of them) that ends in a wait for the scene's stream, per call, the least of `--reps` windows after a warm-up.

  isa      registers, scratch and LDS of the kernels in csrc/sol_lightmap_sample.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  sample   sol_lightmap_sample_dev: both row sets x 3 and 27 channels x bilinear and nearest, with the dilation's plane; the chart guard on (3
           channels); beside each the bytes a row moves when nothing is shared and the time those take at the 8 TB/s HBM peak volume_bench.py uses
  coords   sol_lightmap_coords_dev over two million hits
  view     the lightmap_view chain at 1920 x 1080 over the atrium (BASELINE config 3; every triangle a chart of its own in the atlas) call by
           call, beside closest_hits alone
  restate  the numpy restatement (tests/lightmap_sample_ref.py) over the first `--restate-rows` random rows on the host's CPU, compared word for
           word with the device

  python tests/tools/lightmap_sample_bench.py [--parts isa,sample,coords,view,restate] [--small] [--reps 3] [--out profiles/lightmap_sample.txt]
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


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "ls.s"), "csrc/sol_lightmap_sample.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "ls.s")).read().splitlines()
    lds = sorted(set(l.split(":")[1].strip() for l in text if ".group_segment_fixed_size:" in l))
    sgpr = [l.split(":")[1].strip() for l in text if l.strip().startswith(".sgpr_count:")]
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_sample.hip): LDS bytes of every kernel: " + ", ".join(lds) + "; SGPRs in the order below: " + ", ".join(sgpr))
    out.extend("  " + l.strip() for l in r.stdout.splitlines())


def sample_call(ds, cfg, uvs, texels, pass_of, values, vertices, points, coords, res):
    def p(x):
        return None if x is None else C.c_void_p(x.data_ptr())
    ds._chk(ds.lib.sol_lightmap_sample_dev(ds.h, C.byref(cfg), p(uvs), int(uvs.shape[0]), p(texels), p(pass_of), p(values), p(vertices), p(points), p(coords),
                                            int(coords.shape[0]), p(res)))


def row_bytes(channels, pass_of, guard):
    """what one row moves when it shares nothing: its own 16 bytes, six UV words, per tap the coverage byte or the SolTexel, the value words, and
    the answer; with the guard nine vertex words and per tap the SolTexel and the first dwordx4 of the point row"""
    tap = (1 if pass_of else 16) + 4 * channels + ((16 if pass_of else 0) + 16 if guard else 0)
    return 16 + 24 + (36 if guard else 0) + 4 * tap + 4 * (channels + 1)


def part_gpu(out, parts, small, reps, restate_rows):
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, lightmap_triangle_table, scenes
    W = H = 512 if small else 4096
    n = 100000 if small else 2000000
    rng = np.random.default_rng(7)
    V, T, N = grid_mesh(W // 4)
    with DeviceScene(floor_scene()) as ds:  # (the handle supplies the stream and the scratch only)
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        points = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
        texels = torch.empty((W * H, 4), dtype=torch.int32, device="cuda")
        points_call(ds, dV, None, dT, len(V), W, H, points, texels)
        ds.sync()
        pass_of = torch.zeros((H, W), dtype=torch.uint8, device="cuda")  # (the mesh fills the atlas: every texel owned)
        owned = int((texels[:, 0] != -1).sum())
        out.append(f"workload: the jittered grid mesh, {len(V)} triangles, over a {W} x {H} atlas, {owned} texels owned; {n} surface rows per set")
        b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
        rand = np.zeros(n, dtype=sr.TEXEL_DTYPE)
        rand["triangle"], rand["b1"], rand["b2"], rand["flags"] = rng.integers(0, len(V), n), b[:, 1], b[:, 2], 1
        sets = {"random": torch.from_numpy(rand.view(np.int32).reshape(-1, 4)).cuda(), "texel order": texels[:n].contiguous()}
        if "sample" in parts or "restate" in parts:
            for channels, words in ((3, 4), (27, 28)):
                values = torch.from_numpy(rng.normal(size=(W * H, words)).astype(F)).cuda()
                res = torch.empty((n, channels + 1), dtype=torch.float32, device="cuda")
                for flags, name in ((0, "bilinear"), (1, "nearest")):
                    cfg = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=channels, stride_bytes=4 * words, flags=flags, chart_radius=float("inf"))
                    for which, coords in sets.items():
                        if "sample" not in parts:
                            continue
                        ms = timed(lambda: sample_call(ds, cfg, dT, texels, pass_of, values, None, None, coords, res), ds.sync, reps)
                        by = row_bytes(channels, True, False) if not flags else 16 + 24 + 1 + 4 * channels + 4 * (channels + 1)
                        stream_us = n * by / (HBM_PEAK_GBPS * 1e9) * 1e6
                        taps = float(res[:, channels].contiguous().view(torch.int32).float().mean())
                        out.append(f"  sample {channels:2d} channels {name:8s} {which:11s} {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s  {by:4d} B/row unshared = "
                                   f"{stream_us:7.1f} us at {HBM_PEAK_GBPS / 1000:.0f} TB/s ({ms * 1e3 / stream_us:5.2f} x)  taps per row {taps:.2f}")
                if channels == 3 and "sample" in parts:
                    cfg = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=3, stride_bytes=16, flags=0, chart_radius=0.05)
                    for which, coords in sets.items():
                        ms = timed(lambda: sample_call(ds, cfg, dT, texels, pass_of, values, dV, points, coords, res), ds.sync, reps)
                        taps = float(res[:, 3].contiguous().view(torch.int32).float().mean())
                        out.append(f"  sample  3 channels bilinear {which:11s} chart guard 0.05 {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s  "
                                   f"{row_bytes(3, True, True)} B/row unshared  taps per row {taps:.2f}")
                    cfg = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=3, stride_bytes=16, flags=0, chart_radius=float("inf"))
                    for which, coords in sets.items():
                        ms = timed(lambda: sample_call(ds, cfg, dT, texels, None, values, None, None, coords, res), ds.sync, reps)
                        out.append(f"  sample  3 channels bilinear {which:11s} no pass_of (coverage from the SolTexel rows) {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s  "
                                   f"{row_bytes(3, False, False)} B/row unshared")
                if channels == 3 and "restate" in parts:
                    k = min(restate_rows, n)
                    cfg = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=3, stride_bytes=16, flags=0, chart_radius=float("inf"))
                    sample_call(ds, cfg, dT, texels, pass_of, values, None, None, sets["random"], res)
                    ds.sync()
                    h_values, h_texels = values.cpu().numpy(), texels.cpu().numpy().view(sr.TEXEL_DTYPE).reshape(-1)
                    t0 = time.perf_counter()
                    want = sr.lightmap_sample(h_values, rand[:k], T, h_texels, W, H, pass_of=np.zeros((H, W), np.uint8))
                    s = time.perf_counter() - t0
                    equal = bool((want.view(np.uint32) == res[:k].cpu().numpy().view(np.uint32)).all())
                    out.append(f"restate: tests/lightmap_sample_ref.py (numpy float32) over the first {k} random rows on the host: {s:8.3f} s ({k / s / 1e6:.2f} M rows/s); "
                               f"equal to the device word for word: {equal}")
                del values, res
        if "coords" in parts:
            hits = np.zeros(n, dtype=sr.HIT_DTYPE)
            hits["status"], hits["kind"] = rng.integers(0, 2, n), rng.choice([3, 4], n)
            hits["u"], hits["v"], hits["dfs_index"] = b[:, 1], b[:, 2], rng.integers(0, len(V), n)
            table = (np.arange(len(V), dtype=np.uint32) | (rng.integers(0, 3, len(V)).astype(np.uint32) << np.uint32(30)))
            d_hits, d_table = torch.from_numpy(hits.view(np.int32).reshape(-1, 8)).cuda(), torch.from_numpy(table.view(np.int32)).cuda()
            res = torch.empty((n, 4), dtype=torch.int32, device="cuda")
            ms = timed(lambda: ds._chk(ds.lib.sol_lightmap_coords_dev(ds.h, C.c_void_p(d_hits.data_ptr()), n, C.c_void_p(d_table.data_ptr()), len(table),
                                                                      C.c_void_p(res.data_ptr()))), ds.sync, reps)
            stream_us = n * 52 / (HBM_PEAK_GBPS * 1e9) * 1e6
            out.append(f"coords: sol_lightmap_coords_dev over {n} hits (half of them hits, half of those triangles) {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s  "
                       f"52 B/row = {stream_us:.1f} us at {HBM_PEAK_GBPS / 1000:.0f} TB/s ({ms * 1e3 / stream_us:.2f} x)")
    if "view" in parts:
        from solstrale_amd import lightmap_mesh
        w, h = (480, 270) if small else (1920, 1080)
        sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(w, h, 16))
        nt = int(sc.desc.n_triangles)
        table = lightmap_triangle_table(sc, 0, nt)
        # every triangle a chart of its own: cell k of a square grid of cells, the triangle's corners at three of the cell's
        side = int(np.ceil(np.sqrt(nt)))
        k = np.arange(nt)
        cx, cy = (k % side).astype(np.float64) / side, (k // side).astype(np.float64) / side
        corner = np.asarray([(0.1, 0.1), (0.9, 0.1), (0.1, 0.9)]) / side
        uvs = np.stack([np.stack([cx + corner[c, 0], cy + corner[c, 1]], axis=-1) for c in range(3)], axis=1).astype(F)
        with DeviceScene(sc) as ds:
            d_uvs, d_table = torch.from_numpy(uvs).cuda(), torch.from_numpy(table.view(np.int32)).cuda()
            V2, _ = lightmap_mesh(sc, 0, nt)
            p2, t2 = ds.lightmap_points(torch.from_numpy(V2).cuda(), d_uvs, W, H)
            baked, pass_of = ds.lightmap_dilate(torch.from_numpy(rng.normal(size=(W * H, 4)).astype(F)).cuda(), t2, W, H, passes=2, return_pass_of=True)
            seed = 0x5017A1E
            rays = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8).contiguous()

            def once(fn):
                best, r = float("inf"), None
                for i in range(reps + 1):  # (the first is the warm-up; every Python method waits for the scene's stream before it returns)
                    t0 = time.perf_counter()
                    r = fn()
                    best = min(best, time.perf_counter() - t0) if i else best
                return best * 1e3, r
            ms_rays, _ = once(lambda: ds.camera_rays(0, 0, w, h, 0, seed))
            ms_hits, hits = once(lambda: ds.closest_hits(rays))
            ms_coords, coords = once(lambda: ds.lightmap_coords(hits, d_table))
            ms_sample, lit = once(lambda: ds.lightmap_sample(baked, coords, d_uvs, t2, W, H, pass_of=pass_of))
            ms_view, view = once(lambda: ds.lightmap_view(baked, d_uvs, t2, W, H, d_table, 0, 0, w, h, sample=0, seed=seed, pass_of=pass_of))
            count = lit[:, 3].contiguous().view(torch.int32)
            out.append(f"view: the atrium, {nt} triangles, {w}x{h}, a {W} x {H} atlas with a chart per triangle, ms per call through the Python methods (each waits for the stream)")
            out.append(f"  camera_rays {ms_rays:8.3f}   closest_hits {ms_hits:8.3f}   lightmap_coords {ms_coords:8.3f}   lightmap_sample {ms_sample:8.3f}   "
                       f"lightmap_view (all four) {ms_view:8.3f} ms; pixels with a tap {int(count.ne(0).sum())}/{w * h}; the view equals the four calls: "
                       f"{bool(torch.equal(view.reshape(-1, 4).view(torch.int32), lit.view(torch.int32)))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,sample,coords,view,restate")
    ap.add_argument("--small", action="store_true", help="a 512 x 512 atlas, 100 000 rows, a 20 000-triangle atrium at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate-rows", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_sample.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["lightmap lookups (DESIGN.md 29): tests/tools/lightmap_sample_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    gpu_parts = [p for p in ("sample", "coords", "view", "restate") if p in parts]
    if gpu_parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_sample_bench: no HIP device visible; parts sample, coords, view and restate have nothing to measure without one")
        part_gpu(out, gpu_parts, a.small, a.reps, a.restate_rows)
    out.extend(f"{p}: not measured" for p in ("isa", "sample", "coords", "view", "restate") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
