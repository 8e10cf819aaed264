"""Times of the lightmap filter (sol_lightmap_filter_dev); its output is profiles/lightmap_filter.txt. Everything is resident in device
memory, outputs allocated beforehand; a time is the host clock around a window of back-to-back calls (at least 0.1 s of them) that ends in a wait
for the scene's stream, per call, after a warm-up. The pass shapes are three handles of one process (SOL_LIGHTMAP_FILTER is read at creation) and
alternate window by window; the least of `--reps` windows counts.

  isa      registers, scratch, LDS and waves per SIMD of the kernels in csrc/sol_lightmap_filter.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  shapes   the jittered grid mesh of lightmap_bench.py filling 1024^2 and 4096^2, iterations = 4, at 3 channels (SolRadiance rows) and 27 (SolSh9
           rows): plain (a lane per (texel, channel group)), staged (steps 1 and 2 from a tile in LDS), fold (plain, every group in one lane);
           the same words from all three, checked at the timed sizes; beside them the 64-sample irradiance over the same rows and the 4-pass
           dilation; and the bytes a pass asks for and must move, computed from the shapes
  chain    the 64 x 64 bake of tests/test_gpu_lightmap_filter.py: MSE of the 4-sample atlas against the 1024-sample truth, unfiltered and
           filtered, at the default sigma_value and beside it
  restate  the numpy restatement (tests/lightmap_filter_ref.py) at 256^2 (no GPU needed)

  python tests/tools/lightmap_filter_bench.py [--parts isa,shapes,chain,restate] [--sizes 1024,4096] [--reps 3] [--out profiles/lightmap_filter.txt]
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
import lightmap_filter_ref as fr
import lightmap_ref as lr
from lightmap_bench import floor_scene, grid_mesh, points_call

ROOT = _paths.ROOT
F = np.float32
SHAPES = ("plain", "staged", "fold")
ITERATIONS = 4


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "filter.s")
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), path, "csrc/sol_lightmap_filter.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        meta, block = {}, {}
        for line in open(path):  # the kernels' metadata: one block of `.key: value` lines per kernel, opened by a line that starts with "- ."
            s = line.strip()
            if s.startswith("- ."):
                block = {}
                s = s[2:]
            if s.startswith(".name:") and "sol_lightmap_filter" in s:
                meta[s.split()[-1]] = block
            for key in (".vgpr_count:", ".sgpr_count:", ".group_segment_fixed_size:", ".private_segment_fixed_size:", ".vgpr_spill_count:", ".sgpr_spill_count:"):
                if s.startswith(key):
                    block[key.strip(".:")] = int(s.split()[-1])
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_filter.hip): VGPRs, SGPRs, LDS bytes, scratch bytes, spilled VGPRs / SGPRs, waves per SIMD")
    for name, m in meta.items():
        vgpr = (m["vgpr_count"] + 7) // 8 * 8
        waves = min(8, 512 // max(vgpr, 1))
        if m["group_segment_fixed_size"]:  # 160 KiB of LDS per CU, workgroups of 4 waves over 4 SIMDs
            waves = min(waves, (160 * 1024) // m["group_segment_fixed_size"])
        short = name[name.index("sol_lightmap_filter"):name.index("_kernel") + 7]
        out.append(f"  {short:42s} {m['vgpr_count']:4d} {m['sgpr_count']:4d} {m['group_segment_fixed_size']:6d} {m['private_segment_fixed_size']:3d} "
                   f"{m['vgpr_spill_count']} / {m['sgpr_spill_count']}   {waves} waves per SIMD")


def timed_alternating(calls, sync, reps):
    """ms per call of each of `calls` (name -> function): warmed up, then `reps` rounds in which the candidates take turns, one window each."""
    inner = {}
    for name, fn in calls.items():
        fn(); sync()
        t0 = time.perf_counter()
        fn(); sync()
        inner[name] = max(1, min(500, int(0.1 / max(time.perf_counter() - t0, 1e-6))))
    best = {name: float("inf") for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            for _ in range(inner[name]):
                fn()
            sync()
            best[name] = min(best[name], (time.perf_counter() - t0) / inner[name] * 1e3)
    return best


def pass_bytes(channels):
    """(asked, moved) bytes per texel and pass, from the shapes: a lane reads, per tap, the two guide dwordx4 and group 0 of the input, and its own
    group where that is another one (the centre tap reads no second guide word and no group 0 again); what must move is each plane once: the guides
    and the input read, the output written."""
    groups = (channels + 3) // 4
    per_tap = lambda g: 32 + 16 + (16 if g else 0)  # noqa: E731
    asked = sum(25 * per_tap(g) + 16 for g in range(groups))
    moved = 32 + 16 * groups + 16 * groups
    return asked, moved


def part_shapes(out, sizes, reps):
    import torch
    from solstrale_amd import DeviceScene, _abi
    handles = {}
    for shape in SHAPES:
        os.environ["SOL_LIGHTMAP_FILTER"] = shape
        handles[shape] = DeviceScene(floor_scene())
    os.environ.pop("SOL_LIGHTMAP_FILTER", None)
    out.append(f"shapes: jittered grid mesh filling the atlas (cells of 4 x 4 texels), iterations = {ITERATIONS}, ms per sol_lightmap_filter_dev call "
               f"(prepare + {ITERATIONS} passes), device route, least of {reps} alternating windows")
    try:
        first = handles["plain"]
        for W in sizes:
            V, T, N = grid_mesh(W // 4)
            dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
            points = torch.empty((W * W, 8), dtype=torch.float32, device="cuda")
            texels = torch.empty((W * W, 4), dtype=torch.int32, device="cuda")
            points_call(first, dV, dN, dT, len(T), W, W, points, texels)
            first.sync()
            del dV, dT, dN
            sigma = 2.0 * 4.0 / W
            for channels, words in ((3, 4), (27, 28)):
                gen = torch.Generator(device="cuda").manual_seed(channels)
                values = torch.rand((W * W, words), dtype=torch.float32, device="cuda", generator=gen) * 3.0
                outs = {s: torch.empty_like(values) for s in SHAPES}
                cfg = _abi.SolLightmapFilterConfig(size=64, width=W, height=W, iterations=ITERATIONS, normal_power_log2=5, channels=channels, stride_bytes=4 * words,
                                                   sigma_position=sigma, sigma_plane=sigma, sigma_value=0.25, value_scale=1.0)

                def call(shape):
                    d = handles[shape]
                    d._chk(d.lib.sol_lightmap_filter_dev(d.h, C.byref(cfg), C.c_void_p(points.data_ptr()), C.c_void_p(texels.data_ptr()), C.c_void_p(values.data_ptr()),
                                                         C.c_void_p(outs[shape].data_ptr())))

                def sync_all():
                    for d in handles.values():
                        d.sync()

                torch.cuda.synchronize()
                ms = timed_alternating({s: (lambda s=s: call(s)) for s in SHAPES}, sync_all, reps)
                same = all(torch.equal(outs["plain"].view(torch.int32), outs[s].view(torch.int32)) for s in SHAPES[1:])
                changed = float((outs["plain"][:, :channels] != values[:, :channels]).float().mean().item())
                asked, moved = pass_bytes(channels)
                per_pass = ms["plain"] / ITERATIONS  # (the prepare pass included: an upper bound of a pass)
                out.append(f"  {W:5d}^2  {channels:2d} channels (stride {4 * words:3d})  " + "  ".join(f"{s} {ms[s]:9.3f} ms" for s in SHAPES) +
                           f"   same words: {'yes' if same else 'NO'}   words changed {changed:.3f}")
                out.append(f"          plain: {asked} bytes asked for and {moved} bytes that must move per texel and pass; at {per_pass:.3f} ms a pass that is "
                           f"{asked * W * W / per_pass / 1e9:.2f} TB/s asked of L1 / L2 and {moved * W * W / per_pass / 1e9:.2f} TB/s of unique traffic")
                if channels == 3:
                    chart = texels.clone()
                    j, i = torch.meshgrid(torch.arange(W, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
                    chart[((i < W // 8) | (i >= W - W // 8) | (j < W // 8) | (j >= W - W // 8)).reshape(-1), 0] = -1
                    baked = torch.empty_like(values)

                    def dilate():
                        first._chk(first.lib.sol_lightmap_dilate_dev(first.h, C.c_void_p(chart.data_ptr()), W, W, C.c_void_p(values.data_ptr()), 3, 16, 4,
                                                                      C.c_void_p(baked.data_ptr()), None))

                    other = timed_alternating({"dilate": dilate}, first.sync, reps)
                    first.irradiance(points, samples=64, seed=1)
                    t_irr = timed_alternating({"irradiance": lambda: first.irradiance(points, samples=64, seed=1)}, lambda: None, reps)
                    out.append(f"          beside it: irradiance 64 samples over the same rows {t_irr['irradiance']:9.1f} ms, lightmap_dilate x4 {other['dilate']:9.3f} ms")
                    del chart, baked
                del values, outs
            del points, texels
    finally:
        for d in handles.values():
            d.close()
    out.append("  L2 requests or arithmetic: counters not measured. Read from the figures above: see DESIGN.md 26.")


def part_chain(out):
    import torch
    from solstrale_amd import CameraConfig, DeviceScene, RenderConfig, SceneBuilder
    W = H = 64
    V, T, N = lr.grid_mesh(8, 2)
    V, T, N = (np.ascontiguousarray(a[:, [0, 2, 1]]) for a in (V, T, N))
    T = np.ascontiguousarray(T * F(0.75) + F(0.125), dtype=F)
    b = SceneBuilder()
    first, n = b.triangles(V.astype(np.float64), b.Lambertian(b.SolidColor(0.7, 0.7, 0.7)), uvs=T)
    light = b.Quad((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), b.DiffuseLight(8, 8, 8))
    sc = b.finish(b.Bvh(list(range(first, first + n)) + [light]), CameraConfig(40.0, 0.0, (0.0, 6.0, 6.0), (0.0, 0.0, 0.0), (0, 1, 0)), (0.0, 0.0, 0.0),
                  RenderConfig(32, 32, 1))
    sigma = 2.0 * 4.0 / (0.75 * W)
    out.append(f"chain: floor under a quad light, {W} x {H} atlas, sigma_position {sigma:.4f} (two texels), iterations 4, normal_power_log2 5: MSE of the "
               "irradiance (sums x pi / samples) over the owned texels against the 1024-sample gather of another seed")
    with DeviceScene(sc) as ds:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        points, texels = ds.lightmap_points(dV, dT, W, H, normals=dN)
        owned = (texels[:, 0] != -1).cpu().numpy()
        truth = ds.irradiance(points, samples=1024, seed=977 + 0x5017A1E)
        e_truth = truth.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / 1024)
        for low in (4, 16, 64):
            noisy = ds.irradiance(points, samples=low, seed=0x5017A1E)
            e_noisy = noisy.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / low)
            mse_noisy = ((e_noisy - e_truth) ** 2).mean()
            for sigma_value in (0.25, 1.0, float("inf")):
                f = ds.lightmap_filter(noisy, points, texels, W, H, sigma_position=sigma, sigma_value=sigma_value, value_scale=np.pi / low)
                mse = ((f.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / low) - e_truth) ** 2).mean()
                out.append(f"  {low:3d} samples  sigma_value {sigma_value:5.2f}  unfiltered {mse_noisy:10.5g}  filtered {mse:10.5g}  ratio {mse_noisy / mse:7.3f}")
        for sigma_value in (0.25, 1.0, float("inf")):
            f = ds.lightmap_filter(truth, points, texels, W, H, sigma_position=sigma, sigma_value=sigma_value, value_scale=np.pi / 1024)
            mse = ((f.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / 1024) - e_truth) ** 2).mean()
            out.append(f"  fed the 1024-sample atlas, sigma_value {sigma_value:5.2f}: the filter adds an MSE of {mse:10.5g} (mean irradiance {e_truth.mean():.4g})")


def part_restate(out):
    W = 256
    V, T, N = grid_mesh(W // 4)
    points, texels = lr.lightmap_points(V, T, W, W, normals=N)
    values = np.random.default_rng(1).uniform(0, 3, (W * W, 4)).astype(F)
    t0 = time.perf_counter()
    fr.lightmap_filter(values, points, texels, W, W, sigma_position=2.0 * 4.0 / W, iterations=ITERATIONS)
    out.append(f"restate: tests/lightmap_filter_ref.py (numpy float32) at {W}^2, 3 channels, iterations = {ITERATIONS}: {time.perf_counter() - t0:.2f} s on the host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,shapes,chain,restate")
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_filter.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["lightmap filtering (DESIGN.md 26): tests/tools/lightmap_filter_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    if "shapes" in parts or "chain" in parts:
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_filter_bench: no HIP device visible; parts shapes and chain have nothing to measure without one")
    if "shapes" in parts:
        part_shapes(out, [int(x) for x in a.sizes.split(",")], a.reps)
    if "chain" in parts:
        part_chain(out)
    if "restate" in parts:
        part_restate(out)
    out.extend(f"{p}: not measured" for p in ("isa", "shapes", "chain", "restate") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
