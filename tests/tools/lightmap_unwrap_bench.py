"""Times and quality of the lightmap unwrap (sol_lightmap_unwrap_dev); it writes profiles/lightmap_unwrap.txt. (The committed
file is one run's output with commentary added by hand.) Everything is resident in device memory, outputs allocated beforehand. A call allocates
and frees its own scratch, so two times are reported per mesh: the launches alone - device events around the stages, recorded by the library
under SOL_LIGHTMAP_UNWRAP=stages and read with sol_lightmap_unwrap_stage_ms, the window with the least total of `--reps` calls after a warm-up -
and the host clock around the whole call (allocation, launches, wait, free), the least of the same calls.

  isa      registers, scratch and LDS of the kernels in csrc/sol_lightmap_unwrap.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  meshes   the two-million-triangle jittered grid of tests/tools/lightmap_bench.py (one chart: the worst case of the unions and of the extent
           atomics), the atrium mesh of `scenes`, and two million disjoint triangles (a chart each: the worst case of the packing). Beside each,
           in the same run, the yardstick: sol_lightmap_charts_dev over (the unwrap's uvs, vertices) of the same mesh, timed as
           tests/tools/lightmap_charts_bench.py times it
  quality  lightmap_unwrap_fit of the atrium into 4096 x 4096: charts and fill = content_texels / (width x used_height), beside the grid of
           tests/tools/lightmap_sample_bench.py that gives every triangle a cell of its own
  restate  tests/lightmap_unwrap_ref.py on the largest prefix of the jittered grid it finishes in about a minute (no GPU needed)

  python tests/tools/lightmap_unwrap_bench.py [--parts isa,meshes,quality,restate] [--small] [--reps 3] [--out profiles/lightmap_unwrap.txt]
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
import lightmap_unwrap_ref as ur
from lightmap_bench import floor_scene, grid_mesh, timed

ROOT = _paths.ROOT
F = np.float32
PARTS = ("isa", "meshes", "quality", "restate")
STAGES = ("normals+hash", "sort", "unions+ids", "extents", "rects+sort", "pack", "write")


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), os.path.join(tmp, "lu.s"), "csrc/sol_lightmap_unwrap.hip"], capture_output=True,
                           text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        text = open(os.path.join(tmp, "lu.s")).read().splitlines()
    keys = (".group_segment_fixed_size", ".name", ".private_segment_fixed_size", ".sgpr_count", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
    fields = [l.strip() for l in text if l.strip().split(":")[0] in keys]
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_unwrap.hip; rocPRIM's own kernels are left out): VGPRs, SGPRs, scratch bytes, static LDS bytes, spills")
    for k in range(0, len(fields) - 6, 7):
        f = {a.strip(): b.strip() for a, b in (x.split(":", 1) for x in fields[k:k + 7])}
        if "sol_lightmap" in f[".name"]:
            out.append(f"  {f['.name']}: {f['.vgpr_count']} VGPRs, {f['.sgpr_count']} SGPRs, scratch {f['.private_segment_fixed_size']}, LDS "
                       f"{f['.group_segment_fixed_size']}, spills {f['.vgpr_spill_count']} + {f['.sgpr_spill_count']}")


def p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def atrium(small):
    from solstrale_amd import RenderConfig, lightmap_mesh, scenes
    sc = scenes.sponza_like(RenderConfig(64, 48, 1), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(64, 48, 1), texture_size=16)
    return lightmap_mesh(sc, 0, int(sc.desc.n_triangles))[0]


def part_meshes(out, small, reps):
    import torch
    from solstrale_amd import DeviceScene, _abi
    lib = _abi.load_hip()
    cells = 128 if small else 1024
    grid = grid_mesh(cells)[0]
    centre = grid.mean(axis=1, keepdims=True)
    apart = ((grid - centre) * F(0.5) + centre).astype(F)
    meshes = (("jittered grid (one chart)", grid, 4096, 4096, 1000.0 if not small else 100.0), ("atrium", atrium(small), 4096, 4096, 8.0),
              ("disjoint triangles (a chart each)", apart, 16384, 16384, 1000.0 if not small else 100.0))
    os.environ["SOL_LIGHTMAP_UNWRAP"] = "stages"
    with DeviceScene(floor_scene()) as ds:  # (the yardstick's handle: it supplies the stream and the scratch of sol_lightmap_charts_dev)
        for name, V, W, H, tpu in meshes:
            n = len(V)
            dV = torch.from_numpy(np.ascontiguousarray(V)).cuda()
            uvs = torch.empty((n, 3, 2), dtype=torch.float32, device="cuda")
            ch = torch.empty((n,), dtype=torch.int32, device="cuda")
            res = torch.zeros((8,), dtype=torch.int32, device="cuda")
            cfg = _abi.SolUnwrapConfig(size=C.sizeof(_abi.SolUnwrapConfig), width=W, height=H, gutter=2, texels_per_unit=tpu, crease_cos=-1.0)
            torch.cuda.synchronize()
            best, wall = None, float("inf")
            for k in range(reps + 1):  # (the first is the warm-up)
                t0 = time.perf_counter()
                rc = lib.sol_lightmap_unwrap_dev(0, None, C.byref(cfg), p(dV), n, p(uvs), p(ch), p(res))
                dt = (time.perf_counter() - t0) * 1e3
                if rc != 0:
                    raise SystemExit(lib.sol_last_error().decode())
                ms = (C.c_float * 8)()
                lib.sol_lightmap_unwrap_stage_ms(ms)
                if k and (best is None or ms[7] < best[7]):
                    best = list(ms)
                if k:
                    wall = min(wall, dt)
            r = res.cpu().numpy().view(np.uint32)
            content = int(r[6]) | (int(r[7]) << 32)
            out.append(f"meshes: {name}: {n} triangles into {W} x {H} at {tpu:g} texels per unit: {int(r[0])} charts, used {int(r[2])} x {int(r[3])}, overflow {int(r[4])}, "
                       f"content {content} texels")
            out.append(f"  launches {best[7]:.3f} ms ({n / best[7] * 1e-3:.1f} M triangles/s); the call's wall time {wall:.3f} ms")
            out.append("  stages: " + ", ".join(f"{s} {best[k]:.3f}" for k, s in enumerate(STAGES)) + " ms")
            n_charts = torch.zeros((1,), dtype=torch.int32, device="cuda")
            back = torch.empty((n,), dtype=torch.int32, device="cuda")
            yard = timed(lambda: ds._chk(ds.lib.sol_lightmap_charts_dev(ds.h, p(uvs), p(dV), n, p(back), p(n_charts))), ds.sync, reps)
            same = bool(torch.equal(back, ch)) if int(r[4]) == 0 else None
            out.append(f"  yardstick: sol_lightmap_charts_dev(uvs, vertices) of the same mesh {yard:.3f} ms, {int(n_charts.item())} charts; unwrap launches / yardstick "
                       f"{best[7] / yard:.2f} x; the same labels: {same}")
            del dV, uvs, ch, back
    os.environ.pop("SOL_LIGHTMAP_UNWRAP", None)


def part_quality(out, small):
    import torch
    from solstrale_amd import lightmap_unwrap_fit
    V = atrium(small)
    t0 = time.perf_counter()
    fit = lightmap_unwrap_fit(torch.from_numpy(V).cuda(), 4096, 4096)
    dt = time.perf_counter() - t0
    r = fit.result
    out.append(f"quality: lightmap_unwrap_fit of the atrium ({len(V)} triangles) into 4096 x 4096, gutter 2, crease_cos -1, 16 steps: {dt:.2f} s; "
               f"{fit.texels_per_unit:.4f} texels per unit, {r.n_charts} charts, used {r.used_width} x {r.used_height}, fill "
               f"{r.content_texels / (4096 * r.used_height):.3f} (content_texels / (width x used_height))")
    side = int(np.ceil(np.sqrt(len(V))))
    out.append(f"  beside it, a cell per triangle: {len(V)} charts in cells of {4096 / side:.2f} texels, the triangle over 0.8 x 0.8 of its cell and half of that: fill 0.32")


def part_restate(out):
    for cells in (64, 256, 1024):
        V = grid_mesh(cells)[0]
        t0 = time.perf_counter()
        uvs, ch, res = ur.lightmap_unwrap(V, 4096, 4096, 100.0)
        dt = time.perf_counter() - t0
        out.append(f"restate: tests/lightmap_unwrap_ref.py unwraps {len(V)} triangles in {dt * 1e3:.0f} ms on the CPU ({int(res['n_charts'])} chart)")
        if dt > 20:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--small", action="store_true", help="32 768 triangles and a 20 000-triangle atrium (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_unwrap.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["lightmap unwrap (DESIGN.md 35): tests/tools/lightmap_unwrap_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    if {"meshes", "quality"} & set(parts):
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_unwrap_bench: no HIP device visible; only parts isa and restate have something to measure without one")
        if "meshes" in parts:
            part_meshes(out, a.small, a.reps)
        if "quality" in parts:
            part_quality(out, a.small)
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
