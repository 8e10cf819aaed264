"""Throughput of the radiance queries (sol_radiance_dev) on BASELINE config 3, the atrium at 1920x1080, rays resident in device
memory, timed with device events on the scene's stream. One JSON line; profiles/radiance_queries.txt holds its output.

  (a) against the render: the camera rays and keys of one sample of the frame, samples = 16, beside sol_render of the same 16 samples of the
      same frame in the same session - `--reps` repetitions each, alternating. The yardstick is the render's rate; the allowed shortfall is
      the spread of the render leg's own repetitions.
  (b) probe grids: 65 536 random origins inside the world box with random directions, samples = 64; and 1 024 origins with samples = 4096
      (256 chunks per ray: the partial buffer and the resolve kernel). Msamples/s and Mrays/s; a record, not a bound.

  python tests/tools/radiance_bench.py [--reps 5] [--small] [--no-probes]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 20 000-triangle atrium at 480x270 and smaller grids (a rehearsal, not a measurement)")
    ap.add_argument("--no-probes", action="store_true", help="leg (a) only")
    a = ap.parse_args()
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, device_count, scenes
    if device_count() < 1:
        raise SystemExit("radiance_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if a.small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed, spp = 0x5017A1E, 16
    with DeviceScene(sc) as ds:
        stream = torch.cuda.Stream()
        rays = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8).contiguous()
        keys = ds.camera_ray_keys(0, 0, w, h, 0, seed).reshape(-1, 2).contiguous()
        n = int(rays.shape[0])
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.set_stream(stream.cuda_stream)

        def query(r, k, o, samples, key_base=0):
            cfg = _abi.SolRadianceConfig(size=C.sizeof(_abi.SolRadianceConfig), samples=samples, seed=seed, key_base=key_base, first_draw=2)
            ds._chk(ds.lib.sol_radiance_dev(ds.h, C.c_void_p(r.data_ptr()), C.c_void_p(k.data_ptr()) if k is not None else None, int(r.shape[0]), C.byref(cfg),
                                            C.c_void_p(o.data_ptr())))

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        legs = {"radiance": lambda: query(rays, keys, out, spp), "render": lambda: ds.render(0, spp, seed)}
        for call in legs.values():  # warm-up: code objects, the scene record, the scratch buffers
            for _ in range(2):
                call()
        ds.sync()
        rates = {k: [] for k in legs}
        for _ in range(a.reps):  # alternating
            for name, call in legs.items():
                rates[name].append(n * spp / timed(call) / 1e6)
        res = {"what": "radiance queries against the render, Msamples/s", "scene": f"sponza_like {sc.desc.n_triangles} triangles {w}x{h}", "rays": n, "samples": spp}
        for k, v in rates.items():
            res[k] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "reps": [round(x, 1) for x in v]}
        res["radiance_over_render"] = round(res["radiance"]["median"] / res["render"]["median"], 4)
        res["render_spread"] = round((res["render"]["max"] - res["render"]["min"]) / res["render"]["median"], 4)
        res["checksum"] = float(out[:, :3].double().sum().item())
        if not a.no_probes:
            d = sc.desc
            v = d.nodes[_abi.ref_index(d.root)].bbox.v
            lo, hi = np.array([v[0], v[2], v[4]]), np.array([v[1], v[3], v[5]])
            rng = np.random.default_rng(1)
            grids = ((4096, 16), (256, 256)) if a.small else ((65536, 64), (1024, 4096))
            res["probes"] = {}
            for m, samples in grids:
                p = np.empty((m, 8), dtype=np.float32)
                p[:, 0:3], p[:, 3], p[:, 7] = rng.uniform(lo, hi, (m, 3)), 0.001, np.inf
                dirs = rng.normal(size=(m, 3))
                p[:, 4:7] = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
                pr, po = torch.from_numpy(p).cuda(), torch.empty((m, 4), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                query(pr, None, po, min(samples, 16))
                ds.sync()
                ts = [timed(lambda: query(pr, None, po, samples)) for _ in range(a.reps)]
                t = float(np.median(ts))
                res["probes"][f"{m}x{samples}"] = {"median_s": round(t, 5), "Msamples_per_s": round(m * samples / t / 1e6, 1), "Mrays_per_s": round(m / t / 1e6, 3),
                                                   "reps_s": [round(x, 5) for x in ts], "mean_rgb": [round(float(x), 5) for x in (po[:, :3].double().mean(0) / samples).tolist()]}
        ds.set_stream(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
