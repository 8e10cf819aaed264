"""What moving the triangles of a live scene costs (sol_scene_set_triangles) on BASELINE configs 3 and 5 at 1920x1080, beside the
only route there was before it - sol_scene_destroy + sol_scene_create -, and what the refitted tree costs a frame:

  move     wall time of sol_scene_set_triangles (host vertices) and sol_scene_set_triangles_dev (a device tensor), alternating between two
           displaced states of the mesh, and the same call's device-event split (sol_scene_set_triangles_ms: upload / records and lights
           kernels / refit launches / rest = light tables, background proof, uploads)
  create   sol_scene_create + sol_scene_destroy of the moved description D', in the same session
  quality  a 64-spp frame on the refitted tree - as a plain move leaves the handle, and after a move with SOL_GEOM_REPROBE (the work order of
           creation's cost probe again) - against the same frame on a handle freshly created from D', at sine displacements of 0, 1, 5 and
           20 % of the extent, with the default pre-splitting and without (moved split parts carry the whole triangle's box)

D' is made here with numpy (the triangle constructor and the bottom-up box union, vectorised): a timing aid - tests/geometry_util.py makes
the bit-exact one the tests compare with. Medians of --reps repetitions with their range; one JSON line per scene.
  python tests/tools/set_triangles_bench.py [c3 c5] [--reps 7] [--small] [--no-quality] [--quality-only]"""
import argparse
import ctypes as C
import json
import sys
import time

import _paths  # noqa: F401
import numpy as np

TRI = np.dtype([("v0", "f8", 3), ("v0v1", "f8", 3), ("v0v2", "f8", 3), ("normal", "f8", 3), ("tangent", "f8", 3), ("bi_tangent", "f8", 3),
                ("area", "f8"), ("uv", "f4", 6), ("bbox", "f8", 6), ("material", "i4"), ("dfs_index", "u4")])
NODE = np.dtype([("bbox", "f8", 6), ("left", "u4"), ("right", "u4")])


def _stat(v, digits=3):
    return {"median": round(float(np.median(v)), digits), "min": round(min(v), digits), "max": round(max(v), digits), "n": len(v)}


def _ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def _array(ptr, n, dtype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * dtype.itemsize,)).view(dtype)


class Moved:
    """D' of `scene` for `verts` [n, 3, 3], made with numpy."""

    def __init__(self, scene, verts):
        from solstrale_amd import _abi
        d0 = scene.desc
        assert TRI.itemsize == C.sizeof(_abi.SolTriangle) and NODE.itemsize == C.sizeof(_abi.SolBvhNode)
        self._scene, self.render_config = scene, scene.render_config
        self.desc = _abi.SolSceneDesc.from_buffer_copy(d0)
        t = _array(d0.triangles, d0.n_triangles, TRI).copy()
        e1, e2 = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
        n = np.cross(e1, e2)
        ln = np.sqrt((n * n).sum(axis=1))
        with np.errstate(all="ignore"):
            t["v0"], t["v0v1"], t["v0v2"], t["normal"], t["area"] = verts[:, 0], e1, e2, n / ln[:, None], ln / 2.
        lo, hi = verts.min(axis=1), verts.max(axis=1)
        thin = (hi - lo) < 1e-4
        lo, hi = np.where(thin, lo - 5e-5, lo), np.where(thin, hi + 5e-5, hi)
        t["bbox"][:, 0::2], t["bbox"][:, 1::2] = lo, hi  # (the tangents stay the old ones: a timing aid)
        nodes = _array(d0.nodes, d0.n_nodes, NODE).copy()
        prim = {2: _array(d0.spheres, d0.n_spheres, np.dtype([("head", "f8", 4), ("bbox", "f8", 6), ("tail", "u4", 2)]))["bbox"] if d0.n_spheres else None,
                3: np.array([list(d0.quads[i].bbox.v) for i in range(d0.n_quads)]).reshape(-1, 6), 4: t["bbox"]}

        def boxes_of(refs):
            kind, idx = refs >> 28, refs & 0x0FFFFFFF
            out = np.tile(np.array([np.inf, -np.inf] * 3), (len(refs), 1))
            for k, src in ((1, nodes["bbox"]), (2, prim[2]), (3, prim[3]), (4, prim[4])):
                m = kind == k
                if m.any():
                    out[m] = src[idx[m]]
            return out

        for _ in range(4096):  # bottom-up by relaxation: one vectorised pass per level
            l, r = boxes_of(nodes["left"]), boxes_of(nodes["right"])
            new = np.empty_like(l)
            new[:, 0::2], new[:, 1::2] = np.minimum(l[:, 0::2], r[:, 0::2]), np.maximum(l[:, 1::2], r[:, 1::2])
            if (new == nodes["bbox"]).all():
                break
            nodes["bbox"] = new
        self._t, self._n = t, nodes
        self.desc.triangles = C.cast(t.ctypes.data, C.POINTER(_abi.SolTriangle))
        self.desc.nodes = C.cast(nodes.ctypes.data, C.POINTER(_abi.SolBvhNode))
        self.desc_ptr = C.pointer(self.desc)
        self.width, self.height = int(d0.width), int(d0.height)


def vertices_of(scene):
    t = _array(scene.desc.triangles, scene.desc.n_triangles, TRI)
    return np.stack([t["v0"], t["v0"] + t["v0v1"], t["v0"] + t["v0v2"]], axis=1)


def sine(v, fraction, phase=0.0):
    p = v.reshape(-1, 3)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    w = 2.0 * np.pi * 3.0 / ext
    d = np.stack([np.sin(w * v[..., 1] + 0.3 + phase), np.sin(w * v[..., 2] + 1.1 + phase), np.sin(w * v[..., 0] + 2.0 + phase)], axis=-1)
    return np.ascontiguousarray(v + ext * fraction * d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=["c3", "c5"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="20 000 triangles at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    ap.add_argument("--no-device", action="store_true", help="build the descriptions only (a rehearsal without a GPU)")
    a = ap.parse_args()
    from solstrale_amd import DeviceScene, RenderConfig, device_count, scenes
    if not a.no_device and device_count() < 1:
        raise SystemExit("set_triangles_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    small = dict(n_triangles=20000) if a.small else {}
    make = {"c3": lambda: scenes.sponza_like(RenderConfig(w, h, 16), texture_size=16 if a.small else 1024, **small),
            "c5": lambda: scenes.statue_like(RenderConfig(w, h, 16), **small)}
    seed = 0x5017A1E
    for name in a.scenes:
        sc = make[name]()
        v0 = vertices_of(sc)
        states = [sine(v0, 0.01, 0.0), sine(v0, 0.01, 1.0)]
        out = {"what": "triangle move of a live scene, ms", "scene": f"{name} {sc.desc.n_triangles} triangles {w}x{h}", "reps": a.reps}
        moved = Moved(sc, states[0])
        if a.no_device:
            print(json.dumps(dict(out, nodes=int(sc.desc.n_nodes), rehearsal=True)), flush=True)
            continue
        import torch

        def create():
            with DeviceScene(moved) as d:
                d.sync()

        print(f"[set_triangles_bench] {name}: descriptions made", file=sys.stderr, flush=True)
        create()  # (code objects, the allocator)
        if not a.quality_only:
            out["create_ms"] = _stat([_ms(create) for _ in range(a.reps)], 1)
        for key in () if a.quality_only else ("",):
            with DeviceScene(sc, dynamic_triangles=True) as ds:
                dev = [torch.from_numpy(s).to(f"cuda:{ds.device}") for s in states]
                for k in range(2):  # warm-up: code objects, the flags buffer
                    ds.set_triangles(states[k])
                    ds.set_triangles(dev[k])
                out["move_host_ms" + key] = _stat([_ms(lambda: ds.set_triangles(states[k % 2])) for k in range(a.reps)])
                out["move_device_ms" + key] = _stat([_ms(lambda: ds.set_triangles(dev[k % 2])) for k in range(a.reps)])
                out["move_device_no_proof_ms" + key] = _stat([_ms(lambda: ds.set_triangles(dev[k % 2], background_proof=False)) for k in range(a.reps)])
                ds.kernel_timing(True)
                for route, src in (("host", states), ("device", dev)):
                    parts = []
                    for k in range(a.reps):
                        ds.set_triangles(src[k % 2])
                        parts.append(ds.set_triangles_ms())
                    out[f"split_{route}_ms" + key] = {p: _stat([x[p] for x in parts]) for p in parts[0]}
                ds.kernel_timing(False)
                info = ds.info()
                out["wide_nodes_levels" + key] = [info["stack_bound"]]
        if not a.quality_only:
            out["speedup_host_route"] = round(out["create_ms"]["median"] / out["move_host_ms"]["median"], 1)
        if not a.no_quality:
            q = {}
            for split in (0, -1):
                with DeviceScene(sc, dynamic_triangles=True, split_percent=split) as ds:
                    for frac in (0.0, 0.01, 0.05, 0.20):
                        v = sine(v0, frac)
                        ds.set_triangles(v)

                        def frame(d=ds):
                            d.clear()
                            d.render(0, 64, seed)
                            d.sync()

                        frame()
                        refit = [_ms(frame) for _ in range(a.reps)]
                        ds.set_triangles(v, reprobe=True)  # (the cost probe again: the work order a fresh handle has)
                        frame()
                        reprobed = [_ms(frame) for _ in range(a.reps)]
                        with DeviceScene(Moved(sc, v), split_percent=split) as fresh:
                            frame(fresh)
                            new = [_ms(lambda: frame(fresh)) for _ in range(a.reps)]
                        print(f"[set_triangles_bench] {name} split {split} amplitude {frac} done", file=sys.stderr, flush=True)
                        q[f"split_{'default' if split == 0 else 'off'}_amplitude_{frac}"] = {
                            "refit_tree_frame_ms": _stat(refit), "refit_tree_reprobed_frame_ms": _stat(reprobed), "fresh_tree_frame_ms": _stat(new),
                            "ratio": round(float(np.median(refit) / np.median(new)), 3), "ratio_reprobed": round(float(np.median(reprobed) / np.median(new)), 3)}
            out["quality_64spp"] = q
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
