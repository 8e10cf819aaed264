"""What moving the spheres and quads of a live scene costs (sol_scene_set_primitives) at 1920x1080, beside the only route there
was before it - sol_scene_destroy + sol_scene_create of the moved description:

  c2 spheres   every sphere of BASELINE config 2 (Cornell + 10 000 spheres) displaced by 1 % of the box: a particle step
  c3 light     the quad lights of config 3 alone, shrunk to half their size (all quads travel: one of them moves among the static rest)
  c5 light     the same on config 5
  c5 all       config 5's triangles under a sine of 1 % of the extent, its spheres and its quads (the lights shrunk) in ONE call

each from host arrays and from device tensors, alternating between two states: wall time of the call and its device-event split
(sol_scene_set_triangles_ms: upload / records and lights kernels / refit launches / rest = light tables, background proof, uploads), and
sol_scene_create + sol_scene_destroy of a description of the moved scene in the same session. That description is a timing aid: the moved
primitives are the CPU constructors' (tests/primitive_util.py), moved triangles and their node boxes numpy's (set_triangles_bench.Moved); where
only a light shrinks inside its old box the node boxes are left as they are (they still bound it). Medians of --reps repetitions with their
range; one JSON line per case.
  python tests/tools/set_primitives_bench.py [c2 c3 c5] [--reps 7] [--small]"""
import argparse
import json
import os
import sys

import _paths  # noqa: F401
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from set_triangles_bench import Moved, _ms, _stat, sine, vertices_of  # noqa: E402


def _rows(desc):
    s = np.array([[*desc.spheres[i].center, desc.spheres[i].radius] for i in range(desc.n_spheres)], dtype=np.float64).reshape(-1, 4)
    q = np.array([[desc.quads[i].q[:], desc.quads[i].u[:], desc.quads[i].v[:]] for i in range(desc.n_quads)], dtype=np.float64).reshape(-1, 3, 3)
    return s, q


def _lights_shrunk(desc, spheres, quads, factor):
    from solstrale_amd import _abi
    s, q = spheres.copy(), quads.copy()
    for k in range(desc.n_lights):
        kind, i = _abi.ref_kind(desc.lights[k]), _abi.ref_index(desc.lights[k])
        if kind == _abi.REF_QUAD:
            mid = q[i, 0] + 0.5 * (q[i, 1] + q[i, 2])
            q[i, 1:] *= factor
            q[i, 0] = mid - 0.5 * (q[i, 1] + q[i, 2])
        elif kind == _abi.REF_SPHERE:
            s[i, 3] *= factor
    return s, q


class WithPrimitives:
    """`scene` (a Scene or a Moved) with its sphere and quad records made again from rows by the CPU constructors; node boxes as they are."""

    def __init__(self, scene, spheres, quads):
        import ctypes as C
        from solstrale_amd import _abi, quad_from_corner, sphere_from_center
        d0 = scene.desc
        self._scene, self.render_config = scene, scene.render_config
        self.desc = _abi.SolSceneDesc.from_buffer_copy(d0)
        self._s, self._q = (_abi.SolSphere * max(1, d0.n_spheres))(), (_abi.SolQuad * max(1, d0.n_quads))()
        if d0.n_spheres:
            C.memmove(self._s, d0.spheres, C.sizeof(_abi.SolSphere) * d0.n_spheres)
        if d0.n_quads:
            C.memmove(self._q, d0.quads, C.sizeof(_abi.SolQuad) * d0.n_quads)
        for i in range(d0.n_spheres):
            sphere_from_center(spheres[i, :3], spheres[i, 3], out=self._s[i])
        for i in range(d0.n_quads):
            quad_from_corner(quads[i, 0], quads[i, 1], quads[i, 2], out=self._q[i])
        self.desc.spheres, self.desc.quads = C.cast(self._s, C.POINTER(_abi.SolSphere)), C.cast(self._q, C.POINTER(_abi.SolQuad))
        self.desc_ptr = C.pointer(self.desc)
        self.width, self.height = int(d0.width), int(d0.height)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=["c2", "c3", "c5"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="small scenes at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--no-device", action="store_true", help="build the descriptions only (a rehearsal without a GPU)")
    a = ap.parse_args()
    from solstrale_amd import DeviceScene, RenderConfig, device_count, scenes
    if not a.no_device and device_count() < 1:
        raise SystemExit("set_primitives_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    small = dict(n_triangles=20000) if a.small else {}
    make = {"c2": lambda: scenes.cornell_spheres(RenderConfig(w, h, 16), n_spheres=500 if a.small else 10000),
            "c3": lambda: scenes.sponza_like(RenderConfig(w, h, 16), texture_size=16 if a.small else 1024, **small),
            "c5": lambda: scenes.statue_like(RenderConfig(w, h, 16), **small)}
    for name in a.scenes:
        sc = make[name]()
        d = sc.desc
        s0, q0 = _rows(d)
        rng = np.random.default_rng(2)
        cases = {}
        if name == "c2":
            states = []
            for k in range(2):
                s = s0.copy()
                s[:, :3] += rng.uniform(-5.55, 5.55, (len(s), 3))
                states.append(dict(spheres=s))
            # (spheres that left their old leaf boxes: the moved description needs the node boxes made again - the tests' exact helper)
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
            import primitive_util
            cases["spheres"] = (states, primitive_util.MovedScene(sc, spheres=states[0]["spheres"]))
        else:
            lights = [dict(quads=_lights_shrunk(d, s0, q0, f)[1]) for f in (0.5, 0.6)]
            cases["light"] = (lights, WithPrimitives(sc, s0, lights[0]["quads"]))
            if name == "c5":
                v0 = vertices_of(sc)
                alls = []
                for k, f in enumerate((0.5, 0.6)):
                    s, q = _lights_shrunk(d, s0, q0, f)
                    alls.append(dict(triangles=sine(v0, 0.01, float(k)), spheres=s, quads=q))
                cases["all"] = (alls, WithPrimitives(Moved(sc, alls[0]["triangles"]), alls[0]["spheres"], alls[0]["quads"]))
        for case, (states, moved) in cases.items():
            out = {"what": f"{case} move of a live scene, ms", "scene": f"{name} {d.n_triangles} triangles {d.n_spheres} spheres {d.n_quads} quads {w}x{h}", "reps": a.reps}
            if a.no_device:
                print(json.dumps(dict(out, rehearsal=True)), flush=True)
                continue
            import torch

            def create():
                with DeviceScene(moved) as fresh:
                    fresh.sync()

            create()  # (code objects, the allocator)
            out["create_ms"] = _stat([_ms(create) for _ in range(a.reps)], 1)
            with DeviceScene(sc, dynamic_primitives=True) as ds:
                dev = [{k: torch.from_numpy(np.ascontiguousarray(v)).to(f"cuda:{ds.device}") for k, v in st.items()} for st in states]
                for k in range(2):  # warm-up: code objects, the flags buffer
                    ds.set_primitives(**states[k])
                    ds.set_primitives(**dev[k])
                out["move_host_ms"] = _stat([_ms(lambda: ds.set_primitives(**states[k % 2])) for k in range(a.reps)])
                out["move_device_ms"] = _stat([_ms(lambda: ds.set_primitives(**dev[k % 2])) for k in range(a.reps)])
                ds.kernel_timing(True)
                for route, src in (("host", states), ("device", dev)):
                    parts = []
                    for k in range(a.reps):
                        ds.set_primitives(**src[k % 2])
                        parts.append(ds.set_triangles_ms())
                    out[f"split_{route}_ms"] = {p: _stat([x[p] for x in parts]) for p in parts[0]}
                ds.kernel_timing(False)
            out["speedup_host_route"] = round(out["create_ms"]["median"] / out["move_host_ms"]["median"], 1)
            print(json.dumps(out), flush=True)
            print(f"[set_primitives_bench] {name} {case} done", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
