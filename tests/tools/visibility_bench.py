"""Throughput of the visibility gathers (sol_visibility_dev) on BASELINE config 3, the atrium at 1920x1080, rows resident in
device memory, timed with device events on the scene's stream. One JSON line; profiles/visibility.txt holds its output.

Two point sets, as tests/tools/irradiance_bench.py takes them: `surface_cosine` - where the frame's camera rays (sample 0) hit, with the
normals of the auxiliary normal plane, COSINE - and `probe_grid_sphere` - 32^3 points on a regular grid inside the world box, SPHERE. Each in
both query modes (occluded, closest), `--samples` samples per point, Mrays/s, `--reps` repetitions alternating:

  (a) gather      sol_visibility_dev: one call.
  (b) round_trip  what it replaces: per sample sol_irradiance_rays + sol_query_dev on device tensors and a torch reduction of the answers
                  (counts, bent normal, distance sums), all on the scene's stream.
  (c) query       sol_query_dev alone over the n x samples rays made beforehand: the upper bracket (no draw, no reduction, one launch).

  python tests/tools/visibility_bench.py [--reps 3] [--small] [--samples 64] [--switch N] [--grid G]
  --switch N: the developer override SOL_SWITCH for the handle (the search loop's leave vote; 0: leave only when no lane searches).
  --grid G:   G^3 probes instead of 32^3 (a call over 32^3 probes at 64 samples is 131 072 work items, half of what the machine holds at once).
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
    ap.add_argument("--switch", type=int, default=None)
    ap.add_argument("--grid", type=int, default=0, help="points per axis of the probe grid (default 32; 8 with --small)")
    a = ap.parse_args()
    if a.switch is not None:
        os.environ["SOL_SWITCH"] = str(a.switch)
    import torch
    from solstrale_amd import DeviceScene, RenderConfig, _abi, device_count, scenes
    if device_count() < 1:
        raise SystemExit("visibility_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if a.small else scenes.sponza_like(RenderConfig(w, h, 16))
    seed, spp = 0x5017A1E, a.samples
    HIT, MISS = _abi.SOL_RAY_HIT, _abi.SOL_RAY_MISS
    with DeviceScene(sc) as ds:
        stream = torch.cuda.Stream()
        # the surface points: hit positions of the frame's camera rays, normals from the auxiliary normal plane
        cam = ds.camera_rays(0, 0, w, h, 0, seed).reshape(-1, 8).contiguous()
        hits = ds.closest_hits(cam)
        ds.clear_aux()
        ds.render_aux(0, 1, seed)
        normal = torch.from_numpy(ds.read_aux()[1].reshape(-1, 3)).cuda()
        ds.clear_aux()
        ok = (hits[:, 3] == HIT) & (normal.abs().sum(dim=1) > 0.5)
        t = hits[:, 0].contiguous().view(torch.float32)
        points = torch.empty((int(ok.sum().item()), 8), dtype=torch.float32, device="cuda")
        points[:, 0:3] = (cam[:, 0:3] + t[:, None] * cam[:, 4:7])[ok]
        points[:, 3], points[:, 7] = 0.001, float("inf")
        points[:, 4:7] = normal[ok]
        del cam, hits, normal, t, ok
        # the probe grid
        d = sc.desc
        v = d.nodes[_abi.ref_index(d.root)].bbox.v
        lo, hi = np.array([v[0], v[2], v[4]]), np.array([v[1], v[3], v[5]])
        g = a.grid or (8 if a.small else 32)
        axes = [lo[k] + (np.arange(g) + 0.5) / g * (hi[k] - lo[k]) for k in range(3)]
        grid = np.zeros((g ** 3, 8), dtype=np.float32)
        grid[:, 0:3] = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        grid[:, 3], grid[:, 5], grid[:, 7] = 0.001, 1.0, np.inf
        probes = torch.from_numpy(grid).cuda()
        torch.cuda.synchronize()
        ds.set_stream(stream.cuda_stream)

        def config(mode, samples, first_sample=0):
            return _abi.SolIrradianceConfig(size=C.sizeof(_abi.SolIrradianceConfig), samples=samples, first_sample=first_sample, seed=seed, mode=mode)

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        res = {"what": "visibility gathers against the round trip they replace and against plain ray queries, Mrays/s",
               "scene": f"sponza_like {sc.desc.n_triangles} triangles {w}x{h}", "samples": spp, "switch_below": ds.info().get("switch_below", a.switch)}
        with torch.cuda.stream(stream):
            for name, rows, dmode in (("surface_cosine", points, _abi.SOL_IRRADIANCE_COSINE), ("probe_grid_sphere", probes, _abi.SOL_IRRADIANCE_SPHERE)):
                n = int(rows.shape[0])
                rays_1 = torch.empty((n, 8), dtype=torch.float32, device="cuda")
                keys_1 = torch.empty((n, 2), dtype=torch.int32, device="cuda")
                # (c)'s rays: every sample's, made beforehand
                rays_all = torch.empty((spp, n, 8), dtype=torch.float32, device="cuda")
                for s in range(spp):
                    cfg = config(dmode, 1, s)
                    ds._chk(ds.lib.sol_irradiance_rays(ds.h, C.c_void_p(rows.data_ptr()), None, n, C.byref(cfg), C.c_void_p(rays_all[s].data_ptr()),
                                                       C.c_void_p(keys_1.data_ptr())))
                ds.sync()
                for qmode, qname in ((_abi.SOL_QUERY_OCCLUDED, "occluded"), (_abi.SOL_QUERY_CLOSEST, "closest")):
                    closest = qmode == _abi.SOL_QUERY_CLOSEST
                    out_a = torch.empty((n, 8), dtype=torch.float32, device="cuda")
                    ans_1 = torch.empty((n, 8) if closest else (n,), dtype=torch.int32, device="cuda")
                    ans_all = torch.empty((spp * n, 8) if closest else (spp * n,), dtype=torch.int32, device="cuda")
                    acc = {}

                    def gather():
                        cfg = config(dmode, spp)
                        ds._chk(ds.lib.sol_visibility_dev(ds.h, qmode, C.c_void_p(rows.data_ptr()), None, n, C.byref(cfg), C.c_void_p(out_a.data_ptr())))

                    def round_trip():
                        bent = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
                        n_open, n_hits = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
                        t_sum, t2_sum = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
                        for s in range(spp):
                            cfg = config(dmode, 1, s)
                            ds._chk(ds.lib.sol_irradiance_rays(ds.h, C.c_void_p(rows.data_ptr()), None, n, C.byref(cfg), C.c_void_p(rays_1.data_ptr()),
                                                               C.c_void_p(keys_1.data_ptr())))
                            ds._chk(ds.lib.sol_query_dev(ds.h, qmode, C.c_void_p(rays_1.data_ptr()), n, C.c_void_p(ans_1.data_ptr())))
                            status = ans_1[:, 3] if closest else ans_1
                            miss, hit = status == MISS, status == HIT
                            n_open += miss
                            n_hits += hit
                            bent += rays_1[:, 4:7] * miss[:, None]
                            if closest:
                                tt = torch.where(hit, ans_1[:, 0].view(torch.float32), torch.zeros((), device="cuda"))
                                t_sum += tt
                                t2_sum += tt * tt
                        acc["open"], acc["hits"], acc["t_sum"] = n_open, n_hits, t_sum

                    def query():
                        ds._chk(ds.lib.sol_query_dev(ds.h, qmode, C.c_void_p(rays_all.data_ptr()), spp * n, C.c_void_p(ans_all.data_ptr())))

                    legs = {"gather": gather, "round_trip": round_trip, "query": query}
                    for call in legs.values():  # warm-up: code objects, the scene record, the scratch buffers, torch's allocator
                        call()
                    ds.sync()
                    rates = {k: [] for k in legs}
                    for _ in range(a.reps):  # alternating
                        for k, call in legs.items():
                            rates[k].append(n * spp / timed(call) / 1e6)
                    leg = {"rows": n}
                    for k, r in rates.items():
                        leg[k] = {"median": round(float(np.median(r)), 1), "min": round(min(r), 1), "max": round(max(r), 1), "reps": [round(x, 1) for x in r]}
                    leg["gather_over_round_trip"] = round(leg["gather"]["median"] / leg["round_trip"]["median"], 4)
                    leg["gather_over_query"] = round(leg["gather"]["median"] / leg["query"]["median"], 4)
                    # the three legs count the same rays the same way
                    st_all = ans_all[:, 3] if closest else ans_all
                    leg["open"] = [int(out_a[:, 3].contiguous().view(torch.int32).sum().item()), int(acc["open"].sum().item()), int((st_all == MISS).sum().item())]
                    leg["hits"] = [int(out_a[:, 6].contiguous().view(torch.int32).sum().item()), int(acc["hits"].sum().item()), int((st_all == HIT).sum().item())]
                    assert leg["open"][0] == leg["open"][1] == leg["open"][2] and leg["hits"][0] == leg["hits"][1] == leg["hits"][2], leg
                    leg["open_share"] = round(leg["open"][0] / (n * spp), 4)
                    if closest:
                        leg["mean_hit_distance"] = [round(float(out_a[:, 4].double().sum().item()) / max(leg["hits"][0], 1), 4),
                                                    round(float(acc["t_sum"].double().sum().item()) / max(leg["hits"][0], 1), 4)]
                    res[f"{name}/{qname}"] = leg
                    del out_a, ans_1, ans_all
                del rays_all
        ds.set_stream(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
