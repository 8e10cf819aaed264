"""Throughput of the ray queries (sol_query_dev) on BASELINE config 3, the atrium at 1920x1080: its camera rays of one sample
as they come (coherent) and after a seeded permutation (incoherent), in both modes, rays resident in device memory, timed with device events
on the scene's stream; beside them the render kernel's own traced-ray rate from a counted render of the same scene. One JSON line;
profiles/ray_queries.txt holds its output (and profiles/ray_queries_ab.txt the run that compared two schedules of the kernel).

  python tests/tools/query_bench.py [--reps 5] [--calls 20] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "solstrale-rust_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="launches per timed window")
    ap.add_argument("--small", action="store_true", help="a 20 000-triangle atrium at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--no-render", action="store_true", help="skip the counted render (the context figure)")
    a = ap.parse_args()
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, device_count, scenes
    if device_count() < 1:
        raise SystemExit("query_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if a.small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed = 0x5017A1E
    with DeviceScene(sc) as ds:
        stream = torch.cuda.Stream()
        rays = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8).contiguous()
        n = int(rays.shape[0])
        perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
        workloads = {"coherent": rays, "incoherent": rays[perm].contiguous()}
        hits = torch.empty((n, 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ds.set_stream(stream.cuda_stream)
        results, checks = {}, {}
        for wname, r in workloads.items():
            for mode, mname in ((_abi.SOL_QUERY_CLOSEST, "closest"), (_abi.SOL_QUERY_OCCLUDED, "occluded")):
                call = lambda: ds._chk(ds.lib.sol_query_dev(ds.h, mode, C.c_void_p(r.data_ptr()), n, C.c_void_p(hits.data_ptr())))
                for _ in range(3):  # warm-up: code object, the scene record, the spill area
                    call()
                ds.sync()
                rates = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.calls):
                        call()
                    e1.record(stream)
                    e1.synchronize()
                    rates.append(n * a.calls / (e0.elapsed_time(e1) * 1e-3) / 1e6)
                results[f"{wname}/{mname}"] = rates
                st = hits[:, 3] if mode == _abi.SOL_QUERY_CLOSEST else hits.reshape(-1)[:n]
                checks[f"{wname}/{mname}"] = int((st == _abi.SOL_RAY_HIT).sum().item())
        ds.set_stream(0)
        out = {"what": "ray queries, Mrays/s", "scene": f"sponza_like {sc.desc.n_triangles} triangles {w}x{h}", "rays": n,
               "calls_per_window": a.calls, "hits": checks}
        for k, v in results.items():
            out[k] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1), "reps": [round(x, 1) for x in v]}
        assert checks["coherent/closest"] == checks["coherent/occluded"] == checks["incoherent/closest"] == checks["incoherent/occluded"], checks
        if not a.no_render:  # context: the rays the render kernel traces per second, counted build, same scene
            ds.render(0, 16, seed, counted=True)
            ds.sync()
            ds.clear()
            t0 = time.perf_counter()
            ds.render(0, 16, seed, counted=True)
            ds.sync()
            dt = time.perf_counter() - t0
            st = ds.stats()
            ds.clear()
            ds.kernel_timing(True)
            ds.render(0, 16, seed)
            ms, _ = ds.last_kernel_ms()
            out["render_context"] = {"counted_rays": st["rays"], "counted_render_s": round(dt, 4), "counted_Mrays_per_s": round(st["rays"] / dt / 1e6, 1),
                                     "product_kernel_ms_16spp": round(ms, 3), "product_Mrays_per_s": round(st["rays"] / (ms * 1e-3) / 1e6, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
