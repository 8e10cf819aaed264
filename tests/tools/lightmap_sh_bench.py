"""Times of the directional lightmap (sol_lightmap_sh_dev / sol_lightmap_normals_dev); it writes profiles/lightmap_sh.txt. (The
committed file is one run's output with headings and commentary added by hand; its first paragraph says which lines are which.) The atlas is
profiles/lightmap_sample.txt's: the jittered grid mesh (cells of 4 x 4 texels, two triangles each) filling 4096 x 4096 texels, rasterised on the
device; the values are random SolSh9 rows (112 bytes). Two sets of two million surface rows: `random` - a random triangle and random weights each,
incoherent - and `texel order` - the atlas's own SolTexel rows from the first texel on, coherent. Everything is resident in device memory, outputs
allocated beforehand. A call's time is the host clock around a window of back-to-back calls (at least 0.1 s of them) that ends in a wait for the
scene's stream, per call, the least of `--reps` windows after a warm-up.

  isa           registers, scratch and LDS of the kernels in csrc/sol_lightmap_sh.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  coefficients  sol_lightmap_sh_dev with SOL_LIGHTMAP_SH_COEFFICIENTS (eight lanes to a row) against sol_lightmap_sample_dev with 27 channels (a
                lane to a row) in the same run, both row sets, bilinear and nearest; the answers are compared word for word
  sh            the evaluation (with and without the clamp) against coefficient mode, both row sets
  normals       sol_lightmap_normals_dev over both row sets, with and without vertex normals
  view          the chain of tests/test_gpu_lightmap_sh.py on the floor under a light: the mean over the lit pixels with normals tilted 45 degrees
                toward the light's side and away from it, and their ratio
  restate       the numpy restatement (tests/lightmap_sh_ref.py) over the first `--restate-rows` random rows on the host's CPU, compared word for
                word with the device

  python tests/tools/lightmap_sh_bench.py [--parts isa,sh,coefficients,normals,view,restate] [--small] [--reps 3] [--out profiles/lightmap_sh.txt]
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
import lightmap_sh_ref as shr
from lightmap_bench import floor_scene, grid_mesh, points_call, timed

ROOT = _paths.ROOT
F = np.float32
HBM_PEAK_GBPS = 8000.0  # bench.py's roofline peak, as tests/tools/volume_bench.py
PARTS = ("isa", "sh", "coefficients", "normals", "view", "restate")
ROW_BYTES = 4 * 112 + 16 + 16 + 16  # four taps of a SolSh9, the surface row, the normal, the answer
PARENT = "the parent's record (profiles/lightmap_sample.txt): 27 channels bilinear, a lane to a row, 4.03 ms in texel order, 8.44 ms random"


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "lsh.s"), "csrc/sol_lightmap_sh.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "lsh.s")).read().splitlines()
    lds = [l.split(":")[1].strip() for l in text if l.strip().startswith(".group_segment_fixed_size:")]
    sgpr = [l.split(":")[1].strip() for l in text if l.strip().startswith(".sgpr_count:")]
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_sh.hip): in the order below, LDS bytes: " + ", ".join(lds) + "; SGPRs: " + ", ".join(sgpr))
    out.extend("  " + l.strip() for l in r.stdout.splitlines())


def p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def part_gpu(out, parts, small, reps, restate_rows):
    import torch
    from solstrale_amd import DeviceScene, _abi
    W = H = 512 if small else 4096
    n = 100000 if small else 2000000
    rng = np.random.default_rng(7)
    V, T, N = grid_mesh(W // 4)
    stream_us = n * ROW_BYTES / (HBM_PEAK_GBPS * 1e9) * 1e6
    with DeviceScene(floor_scene()) as ds:  # (the handle supplies the stream and the scratch only)
        dV, dT, dN = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(N).cuda()
        points = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
        texels = torch.empty((W * H, 4), dtype=torch.int32, device="cuda")
        points_call(ds, dV, None, dT, len(V), W, H, points, texels)
        ds.sync()
        del points
        pass_of = torch.zeros((H, W), dtype=torch.uint8, device="cuda")  # (the mesh fills the atlas: every texel owned)
        out.append(f"workload: the jittered grid mesh, {len(V)} triangles, over a {W} x {H} atlas of SolSh9 rows; {n} surface rows per set; "
                   f"{ROW_BYTES} B/row unshared (4 x 112 + 16 + 16 + 16) = {stream_us:.1f} us at {HBM_PEAK_GBPS / 1000:.0f} TB/s")
        out.append(PARENT)
        b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(F)
        rand = np.zeros(n, dtype=sr.TEXEL_DTYPE)
        rand["triangle"], rand["b1"], rand["b2"], rand["flags"] = rng.integers(0, len(V), n), b[:, 1], b[:, 2], 1
        sets = {"texel order": texels[:n].contiguous(), "random": torch.from_numpy(rand.view(np.int32).reshape(-1, 4)).cuda()}
        h_normals = rng.normal(size=(n, 4)).astype(F)
        normals = torch.from_numpy(h_normals).cuda()
        values = torch.from_numpy(rng.normal(size=(W * H, 28)).astype(F)).cuda()
        res28, res28b, res4 = (torch.empty((n, k), dtype=torch.float32, device="cuda") for k in (28, 28, 4))

        def sh_call(flags, coords, nrm, res, scale=0.25):
            cfg = _abi.SolLightmapShConfig(size=32, width=W, height=H, stride_bytes=112, flags=flags, chart_radius=float("inf"), scale=scale)
            ds._chk(ds.lib.sol_lightmap_sh_dev(ds.h, C.byref(cfg), p(dT), len(T), p(texels), p(pass_of), p(values), None, None, p(coords), p(nrm), n, p(res)))

        def sample_call(flags, coords, res):
            cfg = _abi.SolLightmapSampleConfig(size=32, width=W, height=H, channels=27, stride_bytes=112, flags=flags, chart_radius=float("inf"))
            ds._chk(ds.lib.sol_lightmap_sample_dev(ds.h, C.byref(cfg), p(dT), len(T), p(texels), p(pass_of), p(values), None, None, p(coords), n, p(res)))

        coeff_ms = {}
        if "coefficients" in parts or "sh" in parts:
            for flags, name in ((0, "bilinear"), (1, "nearest")):
                for which, coords in sets.items():
                    ms8 = timed(lambda: sh_call(flags | _abi.SOL_LIGHTMAP_SH_COEFFICIENTS, coords, None, res28), ds.sync, reps)
                    coeff_ms[(name, which)] = ms8
                    if "coefficients" not in parts:
                        continue
                    ms1 = timed(lambda: sample_call(flags, coords, res28b), ds.sync, reps)
                    equal = bool(torch.equal(res28.view(torch.int32), res28b.view(torch.int32)))
                    out.append(f"  coefficients {name:8s} {which:11s} eight lanes to a row {ms8 * 1e3:9.1f} us ({ms8 * 1e3 / stream_us:5.2f} x the stream time)   "
                               f"lightmap_sample(channels=27), a lane to a row {ms1 * 1e3:9.1f} us   ratio {ms1 / ms8:5.2f}   equal word for word: {equal}")
        if "sh" in parts:
            for flags, name in ((0, "bilinear"), (_abi.SOL_LIGHTMAP_SH_CLAMP, "bilinear, clamp"), (1, "nearest")):
                for which, coords in sets.items():
                    ms = timed(lambda: sh_call(flags, coords, normals, res4), ds.sync, reps)
                    base = coeff_ms[("nearest" if flags == 1 else "bilinear", which)]
                    out.append(f"  sh {name:15s} {which:11s} {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s ({ms * 1e3 / stream_us:5.2f} x the stream time)   "
                               f"coefficient mode {base * 1e3:9.1f} us   evaluation / coefficients {ms / base:5.2f}")
        if "normals" in parts:
            for which, coords in sets.items():
                for name, vn in (("geometric", None), ("vertex normals", dN)):
                    ms = timed(lambda: ds._chk(ds.lib.sol_lightmap_normals_dev(ds.h, p(coords), n, p(dV), p(vn), len(V), p(res4))), ds.sync, reps)
                    by = 16 + 36 + (36 if vn is not None else 0) + 16
                    out.append(f"  normals {name:14s} {which:11s} {ms * 1e3:9.1f} us  {n / ms / 1e6:7.2f} G rows/s  {by} B/row unshared = "
                               f"{n * by / (HBM_PEAK_GBPS * 1e9) * 1e6:.1f} us at {HBM_PEAK_GBPS / 1000:.0f} TB/s")
        if "restate" in parts:
            k = min(restate_rows, n)
            sh_call(_abi.SOL_LIGHTMAP_SH_CLAMP, sets["random"], normals, res4)
            ds.sync()
            h_values, h_texels = values.cpu().numpy(), texels.cpu().numpy().view(sr.TEXEL_DTYPE).reshape(-1)
            t0 = time.perf_counter()
            want = shr.lightmap_sh(h_values, rand[:k], h_normals[:k], T, h_texels, W, H, scale=0.25, pass_of=np.zeros((H, W), np.uint8), clamp=True)
            s = time.perf_counter() - t0
            equal = bool((want.view(np.uint32) == res4[:k].cpu().numpy().view(np.uint32)).all())
            out.append(f"restate: tests/lightmap_sh_ref.py (numpy float32) over the first {k} random rows on the host: {s:8.3f} s ({k / s / 1e6:.2f} M rows/s); "
                       f"equal to the device word for word: {equal}")
    if "view" in parts:
        from test_gpu_lightmap_sample import floor_under_a_light
        from test_gpu_lightmap_sh import bake_and_view
        sc, V2, T2 = floor_under_a_light()
        with DeviceScene(sc) as ds:
            b = bake_and_view(ds, sc, V2, T2)
        lum = b["lum"]
        out.append(f"view: the floor under a light (tests/test_gpu_lightmap_sh.py), a 32 x 32 atlas baked with 64 samples, 32 x 32 pixels, {int(b['lit'].sum())} lit pixels: "
                   f"mean E with normals tilted 45 degrees toward the light's side {lum['toward']:.4f}, away {lum['away']:.4f}, ratio {lum['toward'] / lum['away']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--small", action="store_true", help="a 512 x 512 atlas, 100 000 rows (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--restate-rows", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_sh.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["directional lightmaps (DESIGN.md 30): tests/tools/lightmap_sh_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    gpu_parts = [x for x in PARTS[1:] if x in parts]
    if gpu_parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_sh_bench: no HIP device visible; only part isa has something to measure without one")
        part_gpu(out, gpu_parts, a.small, a.reps, a.restate_rows)
    out.extend(f"{x}: not measured" for x in PARTS if x not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
