"""Throughput of the SH irradiance queries (sol_irradiance_sh_dev) on BASELINE config 3, the atrium at 1920x1080, rows resident
in device memory, timed with device events on the scene's stream. One JSON line; profiles/irradiance_sh.txt holds its output.

Three legs over the same rows - the points where the frame's camera rays (sample 0) hit, with the normals of the auxiliary normal plane - in
SPHERE mode, `--samples` samples each, `--reps` repetitions, alternating, after one warm-up of each; paths per second:
  sh          sol_irradiance_sh_dev: one call;
  irradiance  sol_irradiance_dev over the same rows: the scalar gather, what the 27 sums cost on top of it;
  round_trip  what the call replaces: per sample sol_irradiance_rays + sol_radiance_dev (samples = 1) + a projection in torch on the device
              (nine basis values per direction, 27 multiply-adds per sample into an [n, 9, 3] accumulator).

  python tests/tools/irradiance_sh_bench.py [--reps 3] [--small] [--samples 64]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "solstrale-rust_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--small", action="store_true", help="a 20 000-triangle atrium at 480x270 (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, device_count, scenes
    if device_count() < 1:
        raise SystemExit("irradiance_sh_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if a.small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed, spp, mode = 0x5017A1E, a.samples, _abi.SOL_IRRADIANCE_SPHERE
    with DeviceScene(sc) as ds:
        stream = torch.cuda.Stream()
        # the points: hit positions of the frame's camera rays, normals from the auxiliary normal plane
        cam = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8).contiguous()
        hits = ds.closest_hits(cam)
        ds.clear_aux()
        ds.render_aux(0, 1, seed)
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
        out_sh = torch.empty((n, 28), dtype=torch.float32, device="cuda")
        out_irr = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        rays, keys = torch.empty((n, 8), dtype=torch.float32, device="cuda"), torch.empty((n, 2), dtype=torch.int32, device="cuda")
        colour = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        acc = torch.zeros((n, 9, 3), dtype=torch.float32, device="cuda")
        k0, k1, k2, k3, k4 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
        torch.cuda.synchronize()
        ds.set_stream(stream.cuda_stream)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        icfg = lambda samples, first: _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=samples, first_sample=first, seed=seed, mode=mode)

        def sh():
            ds._chk(ds.lib.sol_irradiance_sh_dev(ds.h, ptr(points), None, n, C.byref(icfg(spp, 0)), ptr(out_sh)))

        def irradiance():
            ds._chk(ds.lib.sol_irradiance_dev(ds.h, ptr(points), None, n, C.byref(icfg(spp, 0)), ptr(out_irr)))

        def round_trip():
            with torch.cuda.stream(stream):  # (the library's launches and torch's kernels in one stream: ordered without a wait)
                acc.zero_()
                for s in range(spp):
                    ds._chk(ds.lib.sol_irradiance_rays(ds.h, ptr(points), None, n, C.byref(icfg(1, s)), ptr(rays), ptr(keys)))
                    rcfg = _abi.SolRadianceConfig(size=C.sizeof(_abi.SolRadianceConfig), samples=1, first_sample=s, seed=seed)
                    ds._chk(ds.lib.sol_radiance_dev(ds.h, ptr(rays), ptr(keys), n, C.byref(rcfg), ptr(colour)))
                    x, y, z = rays[:, 4], rays[:, 5], rays[:, 6]
                    basis = torch.stack([torch.full_like(x, k0), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * (3.0 * z * z - 1.0), k2 * x * z,
                                         k4 * (x * x - y * y)], dim=1)
                    acc.addcmul_(colour[:, None, 0:3], basis[:, :, None])

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        legs = {"sh": sh, "irradiance": irradiance, "round_trip": round_trip}
        for call in legs.values():  # warm-up: code objects, the scene record, the scratch buffers, torch's kernels
            call()
        ds.sync()
        stream.synchronize()
        rates = {k: [] for k in legs}
        for _ in range(a.reps):  # alternating
            for k, call in legs.items():
                rates[k].append(n * spp / timed(call) / 1e6)
        res = {"what": "SH irradiance queries against the scalar gather and against the per-sample round trip over the same rows, SPHERE, Mpaths/s",
               "scene": f"sponza_like {sc.desc.n_triangles} triangles {w}x{h}", "samples": spp, "rows": n}
        for k, r in rates.items():
            res[k] = {"median": round(float(np.median(r)), 1), "min": round(min(r), 1), "max": round(max(r), 1), "reps": [round(x, 1) for x in r]}
        res["sh_over_irradiance"] = round(res["sh"]["median"] / res["irradiance"]["median"], 4)
        res["sh_over_round_trip"] = round(res["sh"]["median"] / res["round_trip"]["median"], 4)
        # the three legs answer the same question: the l = 0 sums against k0 x the scalar sums, and every sum against the round trip's (other orders
        # of addition: agreement to rounding, not on the bits)
        sums = out_sh[:, :27].reshape(n, 9, 3).double()
        scale = float(sums.abs().mean().item())
        res["mean_abs_sum"] = round(scale, 5)
        res["max_abs_l0_minus_k0_scalar_over_mean"] = float(((sums[:, 0] - k0 * out_irr[:, :3].double()).abs().max() / scale).item())
        res["max_abs_sh_minus_round_trip_over_mean"] = float(((sums - acc.double()).abs().max() / scale).item())
        res["samples_answered"] = int(out_sh[:, 27].contiguous().view(torch.int32).sum().item())
        ds.set_stream(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
