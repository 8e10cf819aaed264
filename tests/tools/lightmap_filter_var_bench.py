"""Times and errors of the irradiance moments and the variance-guided lightmap filter (sol_irradiance_moments_dev, sol_lightmap_filter_var_dev;
DESIGN.md 27); its output is profiles/lightmap_filter_var.txt. Everything is resident in device memory, outputs allocated beforehand. The timing
method of the filter part is tests/tools/lightmap_filter_bench.py's (the host clock around a window of back-to-back calls that ends in a wait for the
scene's stream, candidates alternating window by window, the least of `--reps` windows); the gather part's is tests/tools/irradiance_sh_bench.py's
(device events on the scene's stream, repetitions alternating after one warm-up of each).

  isa      registers, scratch, LDS and waves per SIMD of the kernels in csrc/sol_lightmap_filter_var.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  shapes   the jittered grid mesh of lightmap_bench.py filling 1024^2 and 4096^2, iterations = 4: sol_lightmap_filter_var plain and staged (two
           handles of one process: SOL_LIGHTMAP_FILTER is read at creation), with and without variance_out, beside sol_lightmap_filter at 3 channels
           (its product shape) in the same run; the same words from both shapes, checked at the timed sizes
  gather   irradiance_moments against irradiance and irradiance_sh over the visible surface points of BASELINE config 3 (the atrium at 1920x1080)
           at 64 samples, COSINE for the first two as a bake runs them and SPHERE for the SH leg as its own record has it; Mpaths/s
  chain    the 64 x 64 bake of tests/test_gpu_lightmap_filter_var.py at 4, 16, 64 and 1024 samples: MSE against the 1024-sample truth of another
           seed, unfiltered, sol_lightmap_filter at its defaults and with sigma_value = inf, and sol_lightmap_filter_var at sigma_value 1, 2, 4, 8
  restate  the numpy restatement (tests/lightmap_filter_var_ref.py) at 256^2 (no GPU needed)

  python tests/tools/lightmap_filter_var_bench.py [--parts isa,shapes,gather,chain,restate] [--sizes 1024,4096] [--reps 3] [--small] [--out FILE]
A part that is not run is written down as "not measured". Lines the tool does not write - what a reader makes of the figures - are added to the
profile by hand under the heading "by hand".
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
import lightmap_filter_var_ref as vr
import lightmap_ref as lr
from lightmap_bench import floor_scene, grid_mesh, points_call
from lightmap_filter_bench import timed_alternating

ROOT = _paths.ROOT
F = np.float32
ITERATIONS = 4
SEED = 0x5017A1E


def part_isa(out):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "filter_var.s")
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), path, "csrc/sol_lightmap_filter_var.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        meta, block = {}, {}
        for line in open(path):  # the kernels' metadata: one block of `.key: value` lines per kernel, opened by a line that starts with "- ."
            s = line.strip()
            if s.startswith("- ."):
                block = {}
                s = s[2:]
            if s.startswith(".name:") and "_kernel" in s:
                meta[s.split()[-1]] = block
            for key in (".vgpr_count:", ".sgpr_count:", ".group_segment_fixed_size:", ".private_segment_fixed_size:", ".vgpr_spill_count:", ".sgpr_spill_count:"):
                if s.startswith(key):
                    block[key.strip(".:")] = int(s.split()[-1])
    out.append("isa (tests/tools/isa.sh csrc/sol_lightmap_filter_var.hip): VGPRs, SGPRs, LDS bytes, scratch bytes, spilled VGPRs / SGPRs, waves per SIMD")
    for name, m in meta.items():
        vgpr = (m["vgpr_count"] + 7) // 8 * 8
        waves = min(8, 512 // max(vgpr, 1))
        if m["group_segment_fixed_size"]:  # 160 KiB of LDS per CU, workgroups of 4 waves over 4 SIMDs
            waves = min(waves, (160 * 1024) // m["group_segment_fixed_size"])
        short = name[name.index("sol_"):name.index("_kernel") + 7]
        out.append(f"  {short:46s} {m['vgpr_count']:4d} {m['sgpr_count']:4d} {m['group_segment_fixed_size']:6d} {m['private_segment_fixed_size']:3d} "
                   f"{m['vgpr_spill_count']} / {m['sgpr_spill_count']}   {waves} waves per SIMD")


def part_shapes(out, sizes, reps):
    import torch
    from solstrale_amd import DeviceScene, _abi
    handles = {}
    for shape in ("plain", "staged"):
        os.environ["SOL_LIGHTMAP_FILTER"] = shape
        handles[shape] = DeviceScene(floor_scene())
    os.environ.pop("SOL_LIGHTMAP_FILTER", None)
    handles["old"] = DeviceScene(floor_scene())  # sol_lightmap_filter in its product shape
    out.append(f"shapes: jittered grid mesh filling the atlas (cells of 4 x 4 texels), iterations = {ITERATIONS}, ms per call (prepare + {ITERATIONS} passes), device "
               f"route, least of {reps} alternating windows; `old` is sol_lightmap_filter_dev at 3 channels (stride 16) over the first four words of the same rows")
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
            gen = torch.Generator(device="cuda").manual_seed(3)
            samples = 16
            mean = torch.rand((W * W, 3), dtype=torch.float32, device="cuda", generator=gen) * 3.0
            rel = torch.rand((W * W, 3), dtype=torch.float32, device="cuda", generator=gen)
            moments = torch.zeros((W * W, 8), dtype=torch.float32, device="cuda")
            moments[:, 0:3] = mean * samples
            moments[:, 4:7] = samples * (mean * mean + (samples - 1) * (mean * mean) * rel)
            moments.view(torch.int32)[:, 3] = samples
            values = moments[:, 0:4].contiguous()
            outs = {s: torch.empty((W * W, 4), dtype=torch.float32, device="cuda") for s in ("plain", "staged", "plain+var", "staged+var", "old")}
            vars_ = {s: torch.empty((W * W, 4), dtype=torch.float32, device="cuda") for s in ("plain", "staged")}
            cfg = _abi.SolLightmapFilterVarConfig(size=64, width=W, height=W, iterations=ITERATIONS, normal_power_log2=5, sigma_position=sigma, sigma_plane=sigma,
                                                  sigma_value=4.0, variance_floor=1e-12)
            old_cfg = _abi.SolLightmapFilterConfig(size=64, width=W, height=W, iterations=ITERATIONS, normal_power_log2=5, channels=3, stride_bytes=16,
                                                   sigma_position=sigma, sigma_plane=sigma, sigma_value=0.25, value_scale=1.0 / samples)
            ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

            def call(shape, with_var):
                d = handles[shape]
                d._chk(d.lib.sol_lightmap_filter_var_dev(d.h, C.byref(cfg), ptr(points), ptr(texels), ptr(moments), ptr(outs[shape + ("+var" if with_var else "")]),
                                                         ptr(vars_[shape]) if with_var else None))

            def old():
                d = handles["old"]
                d._chk(d.lib.sol_lightmap_filter_dev(d.h, C.byref(old_cfg), ptr(points), ptr(texels), ptr(values), ptr(outs["old"])))

            def sync_all():
                for d in handles.values():
                    d.sync()

            torch.cuda.synchronize()
            calls = {"plain": lambda: call("plain", False), "staged": lambda: call("staged", False), "plain+var": lambda: call("plain", True),
                     "staged+var": lambda: call("staged", True), "old": old}
            ms = timed_alternating(calls, sync_all, reps)
            same = (torch.equal(outs["plain"].view(torch.int32), outs["staged"].view(torch.int32)) and torch.equal(outs["plain"].view(torch.int32), outs["plain+var"].view(torch.int32))
                    and torch.equal(outs["staged"].view(torch.int32), outs["staged+var"].view(torch.int32)) and torch.equal(vars_["plain"].view(torch.int32), vars_["staged"].view(torch.int32)))
            changed = float((outs["plain"][:, :3] != values[:, :3]).float().mean().item())
            out.append(f"  {W:5d}^2  " + "  ".join(f"{s} {ms[s]:8.3f} ms" for s in calls) + f"   same words: {'yes' if same else 'NO'}   words changed {changed:.3f}")
            out.append(f"          staged / old {ms['staged'] / ms['old']:.3f}   plain / old {ms['plain'] / ms['old']:.3f}   plain / staged {ms['plain'] / ms['staged']:.3f}")
            del moments, values, outs, vars_, mean, rel, points, texels
    finally:
        for d in handles.values():
            d.close()


def part_gather(out, reps, small):
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, scenes
    w, h = (480, 270) if small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(w, h, 16))
    spp = 64
    with DeviceScene(sc) as ds:
        stream = torch.cuda.Stream()
        cam = ds.camera_rays(0, 0, w, h, 0, SEED).reshape(-1, 8).contiguous()
        hits = ds.closest_hits(cam)
        ds.clear_aux()
        ds.render_aux(0, 1, SEED)
        normal = torch.from_numpy(ds.read_aux()[1].reshape(-1, 3)).cuda()
        ds.clear_aux()
        ok = (hits[:, 3] == _abi.SOL_RAY_HIT) & (normal.abs().sum(dim=1) > 0.5)
        t = hits[:, 0].contiguous().view(torch.float32)
        n = int(ok.sum().item())
        points = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        points[:, 0:3] = (cam[:, 0:3] + t[:, None] * cam[:, 4:7])[ok]
        points[:, 3], points[:, 7] = 0.001, float("inf")
        points[:, 4:7] = normal[ok]
        del cam, hits, normal, t, ok
        out_m = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        out_i = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        out_s = torch.empty((n, 28), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.set_stream(stream.cuda_stream)
        ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        icfg = lambda mode: _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=spp, first_sample=0, seed=SEED, mode=mode)  # noqa: E731
        cos, sph = _abi.SOL_IRRADIANCE_COSINE, _abi.SOL_IRRADIANCE_SPHERE
        legs = {"irradiance_moments": lambda: ds._chk(ds.lib.sol_irradiance_moments_dev(ds.h, ptr(points), None, n, C.byref(icfg(cos)), ptr(out_m))),
                "irradiance": lambda: ds._chk(ds.lib.sol_irradiance_dev(ds.h, ptr(points), None, n, C.byref(icfg(cos)), ptr(out_i))),
                "irradiance_sh (sphere)": lambda: ds._chk(ds.lib.sol_irradiance_sh_dev(ds.h, ptr(points), None, n, C.byref(icfg(sph)), ptr(out_s))),
                "irradiance (sphere)": lambda: ds._chk(ds.lib.sol_irradiance_dev(ds.h, ptr(points), None, n, C.byref(icfg(sph)), ptr(out_i)))}

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        for call in legs.values():
            call()
        ds.sync()
        stream.synchronize()
        rates = {k: [] for k in legs}
        for _ in range(reps):
            for k, call in legs.items():
                rates[k].append(n * spp / timed(call) / 1e6)
        legs["irradiance"]()
        ds.sync()
        same = torch.equal(out_m[:, 0:4].contiguous().view(torch.int32), out_i.view(torch.int32))
        ds.set_stream(0)
    out.append(f"gather: sponza_like {sc.desc.n_triangles} triangles {w}x{h}, {n} visible surface points, {spp} samples, {reps} repetitions alternating after one "
               "warm-up of each, device events on the scene's stream, Mpaths/s: median (least - most)")
    for k, r in rates.items():
        out.append(f"  {k:26s} {np.median(r):8.1f}  ({min(r):8.1f} - {max(r):8.1f})")
    med = {k: float(np.median(r)) for k, r in rates.items()}
    out.append(f"  irradiance_moments / irradiance {med['irradiance_moments'] / med['irradiance']:.3f}   irradiance_sh / irradiance (sphere) "
               f"{med['irradiance_sh (sphere)'] / med['irradiance (sphere)']:.3f}   the moments' first four words are irradiance's: {'yes' if same else 'NO'}")


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
    svs = (1.0, 2.0, 4.0, 8.0)
    out.append(f"chain: floor under a quad light, {W} x {H} atlas, sigma_position {sigma:.4f} (two texels), iterations 4, normal_power_log2 5, variance_floor 1e-12: "
               "MSE of the irradiance (sums x pi / samples) over the owned texels against the 1024-sample gather of another seed")
    out.append("  samples  unfiltered   old default (0.25)   old sigma_value inf   " + "   ".join(f"var sigma_value {s:g}" for s in svs))
    with DeviceScene(sc) as ds:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        points, texels = ds.lightmap_points(dV, dT, W, H, normals=dN)
        owned = (texels[:, 0] != -1).cpu().numpy()
        truth = ds.irradiance(points, samples=1024, seed=977 + SEED)
        e_truth = truth.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / 1024)
        mse_of = lambda rows, k: ((rows.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / k) - e_truth) ** 2).mean()  # noqa: E731
        for low in (4, 16, 64, 1024):
            seed = SEED if low != 1024 else 977 + SEED  # (the 1024-sample row feeds the filters the truth itself: what they add to a clean atlas)
            moments = ds.irradiance_moments(points, samples=low, seed=seed)
            noisy = moments[:, 0:4].contiguous()
            row = [mse_of(noisy, low)]
            for sigma_value in (0.25, float("inf")):
                row.append(mse_of(ds.lightmap_filter(noisy, points, texels, W, H, sigma_position=sigma, sigma_value=sigma_value, value_scale=np.pi / low), low))
            for sigma_value in svs:
                row.append(mse_of(ds.lightmap_filter_var(moments, points, texels, W, H, sigma_position=sigma, sigma_value=sigma_value), low))
            out.append(f"  {low:7d}  " + "  ".join(f"{x:12.5g}" for x in row))
            if low != 1024:  # (the 1024 row is the error a filter adds to the truth itself: no ratio)
                out.append("    ratio              " + "  ".join(f"{row[0] / x:12.3f}" for x in row[1:]) + "   (unfiltered / filtered)")
        out.append(f"  mean irradiance of the truth {e_truth.mean():.4g}")


def part_restate(out):
    W = 256
    V, T, N = grid_mesh(W // 4)
    points, texels = lr.lightmap_points(V, T, W, W, normals=N)
    rng = np.random.default_rng(1)
    rows = np.zeros(W * W, dtype=vr.MOMENTS_DTYPE)
    mean = rng.uniform(0, 3, (W * W, 3))
    rows["samples"], rows["sum"], rows["sum2"] = 16, (16 * mean).astype(F), (16 * (mean ** 2 + 15 * 0.3 * mean ** 2)).astype(F)
    t0 = time.perf_counter()
    vr.lightmap_filter_var(rows, points, texels, W, W, sigma_position=2.0 * 4.0 / W, iterations=ITERATIONS)
    out.append(f"restate: tests/lightmap_filter_var_ref.py (numpy float32) at {W}^2, iterations = {ITERATIONS}: {time.perf_counter() - t0:.2f} s on the host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,shapes,gather,chain,restate")
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="gather: a 20 000-triangle atrium at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_filter_var.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["irradiance moments and variance-guided lightmap filtering (DESIGN.md 27): tests/tools/lightmap_filter_var_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    if {"shapes", "gather", "chain"} & set(parts):
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("lightmap_filter_var_bench: no HIP device visible; parts shapes, gather and chain have nothing to measure without one")
    if "shapes" in parts:
        part_shapes(out, [int(x) for x in a.sizes.split(",")], a.reps)
    if "gather" in parts:
        part_gather(out, a.reps, a.small)
    if "chain" in parts:
        part_chain(out)
    if "restate" in parts:
        part_restate(out)
    out.extend(f"{p}: not measured" for p in ("isa", "shapes", "gather", "chain", "restate") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
