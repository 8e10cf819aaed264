"""Times of the lightmap charts (sol_lightmap_charts_dev / sol_lightmap_dilate_charts_dev / sol_lightmap_sample_charts_dev /
sol_lightmap_chart_levels_dev); it writes profiles/lightmap_charts.txt. (The committed file is one run's output with commentary
added by hand.) The mesh is profiles/lightmap.txt's: the jittered grid mesh (cells of 4 x 4 texels, two triangles each) filling 4096 x 4096
texels - two million triangles. Everything is resident in device memory, outputs allocated beforehand. A call's time is the host clock around a
window of back-to-back calls (at least 0.1 s of them) that ends in a wait for the scene's stream, per call, the least of `--reps` windows after a
warm-up.

  isa      registers, scratch and LDS of the kernels in csrc/sol_lightmap_charts.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  charts   the labelling of the grid mesh without and with vertices, and of the same triangles made disjoint (each shrunk towards its centroid: two
           million charts); beside it, in the same run, sol_lightmap_points_dev of that mesh. The stages of a labelling - hash, sort, match and
           union, flatten, scan, ids - are a kernel trace of part `trace`:
             rocprofv3 --kernel-trace --stats -- python tests/tools/lightmap_charts_bench.py --parts trace --out /dev/null
  dilate   sol_lightmap_dilate_charts_dev against sol_lightmap_dilate_dev over the same rows, 4 passes, 3 channels and 27; the atlas is the
           grid mesh's chart shrunk to the middle three quarters, so that the passes have a border to fill
  sample   sol_lightmap_sample_charts_dev against sol_lightmap_sample_dev over the same two million rows, in texel order and in random order
  levels   sol_lightmap_chart_levels_dev of that atlas
  restate  tests/lightmap_charts_ref.py's labelling of 200 000 triangles of the grid mesh on the CPU
  trace    (only when named; it measures nothing itself) ten labellings without vertices, then ten with them, for the kernel trace above; the
           profile's by-hand section is that trace folded per kernel

  python tests/tools/lightmap_charts_bench.py [--parts isa,charts,dilate,sample,levels,restate] [--small] [--reps 3] [--out profiles/lightmap_charts.txt]
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
import lightmap_charts_ref as cr
from lightmap_bench import floor_scene, grid_mesh, points_call, timed

ROOT = _paths.ROOT
F = np.float32
PARTS = ("isa", "charts", "dilate", "sample", "levels", "restate")


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "lc.s"), "csrc/sol_lightmap_charts.hip"], capture_output=True,
                           text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "lc.s")).read().splitlines()
    keys = (".group_segment_fixed_size", ".name", ".private_segment_fixed_size", ".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
    fields = [l.strip() for l in text if l.strip().split(":")[0] in keys]
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_charts.hip; rocPRIM's own kernels are left out): VGPRs, SGPRs, scratch bytes, static LDS bytes, spills")
    for k in range(0, len(fields) - 6, 7):
        f = {a.strip(): b.strip() for a, b in (x.split(":", 1) for x in fields[k:k + 7])}
        if "sol_lightmap" in f[".name"]:
            out.append(f"  {f['.name']}: {f['.vgpr_count']} VGPRs, {f['.sgpr_count']} SGPRs, scratch {f['.private_segment_fixed_size']}, LDS "
                       f"{f['.group_segment_fixed_size']}, spills {f['.vgpr_spill_count']} + {f['.sgpr_spill_count']}")


def p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def part_gpu(out, parts, small, reps):
    import torch
    from solstrale_amd import DeviceScene, _abi
    W = H = 512 if small else 4096
    n_rows = 100000 if small else 2000000
    rng = np.random.default_rng(7)
    V, T, N = grid_mesh(W // 4)
    n = len(T)
    with DeviceScene(floor_scene()) as ds:  # (the handle supplies the stream and the scratch only)
        lib, h = ds.lib, ds.h
        dV, dT = torch.from_numpy(V).cuda(), torch.from_numpy(T).cuda()
        chart_of = torch.empty((n,), dtype=torch.int32, device="cuda")
        n_charts = torch.zeros((1,), dtype=torch.int32, device="cuda")
        out.append(f"workload: the jittered grid mesh, {n} triangles, over a {W} x {H} atlas")

        def label(uvs, vertices):
            ds._chk(lib.sol_lightmap_charts_dev(h, p(uvs), p(vertices), n, p(chart_of), p(n_charts)))

        if "trace" in parts:
            for vertices in (None, dV):  # (the trace's first ten dispatches of each kernel are without vertices, the last ten with)
                for _ in range(10):
                    label(dT, vertices)
                ds.sync()
            out.append(f"trace: 10 labellings of {n} triangles without vertices, then 10 with them ({int(n_charts.item())} chart)")
        if "charts" in parts:
            centre = T.mean(axis=1, keepdims=True)
            d_apart = torch.from_numpy(((T - centre) * F(0.5) + centre).astype(F)).cuda()
            for name, uvs, vertices in (("uvs only", dT, None), ("uvs and vertices", dT, dV), ("disjoint, uvs only", d_apart, None)):
                ms = timed(lambda: label(uvs, vertices), ds.sync, reps)
                out.append(f"charts: {name}: {ms:.3f} ms, {int(n_charts.item())} charts ({n / ms * 1e-3:.1f} M triangles/s)")
            points = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
            texels = torch.empty((W * H, 4), dtype=torch.int32, device="cuda")
            ms = timed(lambda: points_call(ds, dV, None, dT, n, W, H, points, texels), ds.sync, reps)
            out.append(f"charts: beside it, sol_lightmap_points_dev of the same mesh: {ms:.3f} ms")
            del points, texels, d_apart
        if not {"dilate", "sample", "levels"} & set(parts):
            return
        # the atlas of the other parts: the mesh's chart in the middle three quarters
        T2 = np.ascontiguousarray(T * F(0.75) + F(0.125), dtype=F)
        dT2 = torch.from_numpy(T2).cuda()
        points = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
        texels = torch.empty((W * H, 4), dtype=torch.int32, device="cuda")
        points_call(ds, dV, None, dT2, n, W, H, points, texels)
        ds.sync()
        del points
        label(dT2, None)
        ds.sync()
        pass_of = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        plane = torch.empty((H, W), dtype=torch.int32, device="cuda")
        baked = {}
        for channels, words in ((3, 4), (27, 28)):
            values = torch.from_numpy(rng.normal(size=(W * H, words)).astype(F)).cuda()
            dilated = torch.empty_like(values)
            if "dilate" in parts:
                old = timed(lambda: ds._chk(lib.sol_lightmap_dilate_dev(h, p(texels), W, H, p(values), channels, words * 4, 4, p(dilated), p(pass_of))), ds.sync, reps)
                keep = dilated.clone()
                new = timed(lambda: ds._chk(lib.sol_lightmap_dilate_charts_dev(h, p(texels), W, H, p(values), channels, words * 4, 4, p(chart_of), n, p(dilated),
                                                                               p(pass_of), p(plane))), ds.sync, reps)
                same = torch.equal(keep.view(torch.int32), dilated.view(torch.int32))
                out.append(f"dilate: {channels} channels, 4 passes: dilate_charts {new:.3f} ms, lightmap_dilate {old:.3f} ms ({new / old:.2f} x); one chart, the same "
                           f"bytes: {same}")
                del keep
            else:
                ds._chk(lib.sol_lightmap_dilate_charts_dev(h, p(texels), W, H, p(values), channels, words * 4, 4, p(chart_of), n, p(dilated), p(pass_of), p(plane)))
                ds.sync()
            baked[channels] = (dilated, words)
            del values
        if "sample" in parts:
            own = torch.nonzero(texels[:, 3] != 0)[:, 0]
            ordered = texels[own[:n_rows]].contiguous()
            shuffled = ordered[torch.randperm(len(ordered), device="cuda")].contiguous()
            for channels, (values, words) in baked.items():
                cfg = _abi.SolLightmapSampleConfig(size=C.sizeof(_abi.SolLightmapSampleConfig), width=W, height=H, channels=channels, stride_bytes=4 * words, flags=0,
                                                   chart_radius=float("inf"))
                a = torch.empty((len(ordered), channels + 1), dtype=torch.float32, device="cuda")
                b = torch.empty_like(a)
                for name, rows in (("texel order", ordered), ("random order", shuffled)):
                    old = timed(lambda: ds._chk(lib.sol_lightmap_sample_dev(h, C.byref(cfg), p(dT2), n, p(texels), p(pass_of), p(values), None, None, p(rows),
                                                                            len(rows), p(a))), ds.sync, reps)
                    new = timed(lambda: ds._chk(lib.sol_lightmap_sample_charts_dev(h, C.byref(cfg), p(dT2), n, p(texels), p(pass_of), p(values), p(chart_of), p(plane),
                                                                                   p(rows), len(rows), p(b))), ds.sync, reps)
                    out.append(f"sample: {channels} channels, {len(rows)} rows in {name}: sample_charts {new:.3f} ms, lightmap_sample {old:.3f} ms "
                               f"({new / old:.2f} x); one chart, the same words: {torch.equal(a.view(torch.int32), b.view(torch.int32))}")
        if "levels" in parts:
            answer = torch.zeros((31,), dtype=torch.int32, device="cuda")
            base = answer.data_ptr()
            ms = timed(lambda: ds._chk(lib.sol_lightmap_chart_levels_dev(h, p(plane), p(pass_of), W, H, C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 64))),
                       ds.sync, reps)
            out.append(f"levels: {ms:.3f} ms; levels = {int(answer[0].item())} (one chart: all of them)")


def part_restate(out):
    V, T, N = grid_mesh(316)  # 199 712 triangles
    t0 = time.perf_counter()
    chart, n = cr.lightmap_charts(T)
    out.append(f"restate: tests/lightmap_charts_ref.py labels {len(T)} triangles in {(time.perf_counter() - t0) * 1e3:.0f} ms on the CPU ({n} chart)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--small", action="store_true", help="a 512 x 512 atlas, 100 000 rows (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_charts.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["lightmap charts (DESIGN.md 32): tests/tools/lightmap_charts_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    gpu_parts = [x for x in ("trace",) + PARTS[1:-1] if x in parts]
    if gpu_parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_charts_bench: no HIP device visible; only parts isa and restate have something to measure without one")
        part_gpu(out, gpu_parts, a.small, a.reps)
    if "restate" in parts:
        part_restate(out)
    out.extend(f"{x}: not measured" for x in PARTS if x not in parts)
    text = "\n".join(out) + "\n"
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
