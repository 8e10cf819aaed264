"""Throughput of the irradiance queries (sol_irradiance_dev) on BASELINE config 3, the atrium at 1920x1080, rows resident in
device memory, timed with device events on the scene's stream. One JSON line; profiles/irradiance_queries.txt holds its output.

  (a) lightmap-like: the points are where the frame's camera rays (sample 0) hit, with the normals of the auxiliary normal plane; COSINE,
      samples = 64 - beside sol_radiance_dev with samples = 64 over the same number of rows (the same positions, each looking along its
      normal): what the direction drawn per sample costs, or gains, against one ray traced 64 times. Paths per second; `--reps` repetitions
      each, alternating.
  (b) probe grid: 32^3 points on a regular grid inside the world box, SPHERE, samples = 64 - beside sol_radiance_dev over the same positions
      with one random direction each.

  python tests/tools/irradiance_bench.py [--reps 3] [--small] [--samples 64]
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
    ap.add_argument("--small", action="store_true", help="a 20 000-triangle atrium at 480x270 and an 8^3 grid (a rehearsal, not a measurement)")
    a = ap.parse_args()
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, device_count, scenes
    if device_count() < 1:
        raise SystemExit("irradiance_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if a.small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed, spp = 0x5017A1E, a.samples
    with DeviceScene(sc) as ds:
        stream = torch.cuda.Stream()
        # (a) the points: hit positions of the frame's camera rays, normals from the auxiliary normal plane
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
        # (b) the probe grid
        d = sc.desc
        v = d.nodes[_abi.ref_index(d.root)].bbox.v
        lo, hi = np.array([v[0], v[2], v[4]]), np.array([v[1], v[3], v[5]])
        g = 8 if a.small else 32
        axes = [lo[k] + (np.arange(g) + 0.5) / g * (hi[k] - lo[k]) for k in range(3)]
        grid = np.zeros((g ** 3, 8), dtype=np.float32)
        grid[:, 0:3] = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        grid[:, 3], grid[:, 5], grid[:, 7] = 0.001, 1.0, np.inf
        probes = torch.from_numpy(grid).cuda()
        dirs = np.random.default_rng(1).normal(size=(g ** 3, 3))
        grid[:, 4:7] = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        probe_rays = torch.from_numpy(grid).cuda()
        torch.cuda.synchronize()
        ds.set_stream(stream.cuda_stream)

        def irradiance(rows, out, mode):
            cfg = _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=spp, seed=seed, mode=mode)
            ds._chk(ds.lib.sol_irradiance_dev(ds.h, C.c_void_p(rows.data_ptr()), None, int(rows.shape[0]), C.byref(cfg), C.c_void_p(out.data_ptr())))

        def radiance(rows, out):
            cfg = _abi.SolRadianceConfig(size=C.sizeof(_abi.SolRadianceConfig), samples=spp, seed=seed)
            ds._chk(ds.lib.sol_radiance_dev(ds.h, C.c_void_p(rows.data_ptr()), None, int(rows.shape[0]), C.byref(cfg), C.c_void_p(out.data_ptr())))

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        res = {"what": "irradiance queries against radiance queries over the same number of rows, Mpaths/s",
               "scene": f"sponza_like {sc.desc.n_triangles} triangles {w}x{h}", "samples": spp}
        for name, rows, rays, mode in (("surface_cosine", points, points, _abi.SOL_IRRADIANCE_COSINE), ("probe_grid_sphere", probes, probe_rays, _abi.SOL_IRRADIANCE_SPHERE)):
            n = int(rows.shape[0])
            out_i, out_r = torch.empty((n, 4), dtype=torch.float32, device="cuda"), torch.empty((n, 4), dtype=torch.float32, device="cuda")
            legs = {"irradiance": lambda: irradiance(rows, out_i, mode), "radiance": lambda: radiance(rays, out_r)}
            for call in legs.values():  # warm-up: code objects, the scene record, the scratch buffers
                call()
            ds.sync()
            rates = {k: [] for k in legs}
            for _ in range(a.reps):  # alternating
                for k, call in legs.items():
                    rates[k].append(n * spp / timed(call) / 1e6)
            leg = {"rows": n}
            for k, r in rates.items():
                leg[k] = {"median": round(float(np.median(r)), 1), "min": round(min(r), 1), "max": round(max(r), 1), "reps": [round(x, 1) for x in r]}
            leg["irradiance_over_radiance"] = round(leg["irradiance"]["median"] / leg["radiance"]["median"], 4)
            leg["mean_irradiance_sum_per_sample"] = [round(float(x), 5) for x in (out_i[:, :3].double().mean(0) / spp).tolist()]
            leg["samples_answered"] = int(out_i[:, 3].contiguous().view(torch.int32).sum().item())
            res[name] = leg
        ds.set_stream(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
