"""What a camera move of a live scene costs (sol_scene_set_camera) on BASELINE configs 3 and 5 at 1920x1080, beside the only
route there was before it - sol_scene_create of the same description with the new camera - and beside the host proof it replaces:

  move        wall time of sol_scene_set_camera, to camera B and back to camera A: with the background proof (the default), with
              SOL_CAMERA_NO_BACKGROUND_PROOF, with SOL_CAMERA_REPROBE
  proof       sol_background_proof_kernel alone, from device events (sol_kernel_timing), per direction
  create      sol_scene_create + sol_scene_destroy of the description with camera B
  host_proof  find_background_blocks on the host for either camera: sol_background_blocks at 1080p minus the same call on a 16x9 frame
              (the tree build both calls make does not depend on the frame; the 16x9 frame has two blocks)
  frame       a 16-spp and a 512-spp frame of camera A on the handle as created and after a move to it with the proof, without it, and
              with proof and SOL_CAMERA_REPROBE: clear + render + sync, wall time, and the render kernel alone from device events

Medians of --reps repetitions with their spread; one JSON line per scene. profiles/set_camera.txt holds a run.
  python tests/tools/set_camera_bench.py [c3 c5] [--reps 5] [--small] [--create-only]
--create-only measures `create` alone and uses nothing an older commit lacks: copied into a checkout of the parent commit it times the parent's
own library in the same session."""
import argparse
import ctypes as C
import json
import time

import _paths  # noqa: F401
import numpy as np


def _stat(v, digits=3):
    return {"median": round(float(np.median(v)), digits), "min": round(min(v), digits), "max": round(max(v), digits), "n": len(v)}


def _ms(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=["c3", "c5"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="20 000 triangles at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--create-only", action="store_true")
    a = ap.parse_args()
    from solstrale_amd import CameraConfig, DeviceScene, RenderConfig, _abi, background_blocks, device_count, scenes
    if device_count() < 1:
        raise SystemExit("set_camera_bench: no HIP device visible; there is nothing to measure without one")
    w, h = (480, 270) if a.small else (1920, 1080)
    small = dict(n_triangles=20000) if a.small else {}
    # camera B: the scene's other preset (C3: the interior view, C5: the close-up); A: the default
    make = {"c3": lambda cam: scenes.sponza_like(RenderConfig(w, h, 16), camera=cam, texture_size=16 if a.small else 1024, **small),
            "c5": lambda cam: scenes.statue_like(RenderConfig(w, h, 16), camera=cam, **small)}
    other = {"c3": "interior", "c5": "closeup"}
    seed = 0x5017A1E
    for name in a.scenes:
        sc_a, sc_b = make[name]("default"), make[name](other[name])
        cam_a, cam_b = _abi.SolCamera(), _abi.SolCamera()
        C.memmove(C.byref(cam_a), C.byref(sc_a.desc.camera), C.sizeof(cam_a))
        C.memmove(C.byref(cam_b), C.byref(sc_b.desc.camera), C.sizeof(cam_b))
        out = {"what": "camera move of a live scene, ms", "scene": f"{name} {sc_a.desc.n_triangles} triangles {w}x{h}", "reps": a.reps}

        def create():
            with DeviceScene(sc_b) as d:
                d.sync()

        create()  # (code objects, the allocator)
        out["create_ms"] = _stat([_ms(create) for _ in range(a.reps)], 1)
        if a.create_only:
            print(json.dumps(out), flush=True)
            continue
        with DeviceScene(sc_a) as ds:
            cams = [cam_b, cam_a]

            def timed_frames(spp, key):
                def frame():
                    ds.clear()
                    ds.render(0, spp, seed)
                    ds.sync()

                frame()
                out[f"frame_{spp}spp_{key}_ms"] = _stat([_ms(frame) for _ in range(a.reps)])
                ds.kernel_timing(True)
                kern = []
                for _ in range(a.reps):
                    frame()
                    kern.append(ds.last_kernel_ms()[0])
                ds.kernel_timing(False)
                out[f"frame_{spp}spp_{key}_kernel_ms"] = _stat(kern)

            for spp in (16, 512):  # the handle as created: camera A's background blocks AND the creation probe's block costs
                timed_frames(spp, "as_created")
            for k in range(2):  # warm-up: the code object, the flags buffer
                ds.set_camera(cams[k % 2])
            for key, kw in (("move_proof_ms", {}), ("move_no_proof_ms", dict(background_proof=False)), ("move_reprobe_ms", dict(reprobe=True))):
                t = [_ms(lambda: ds.set_camera(cams[k % 2], **kw)) for k in range(2 * a.reps)]
                out[key] = {"to_b": _stat(t[0::2]), "to_a": _stat(t[1::2])}
            ds.kernel_timing(True)
            kern = []
            for k in range(2 * a.reps):
                ds.set_camera(cams[k % 2])
                kern.append(ds.last_kernel_ms()[0])
            ds.kernel_timing(False)
            out["proof_kernel_ms"] = {"to_b": _stat(kern[0::2]), "to_a": _stat(kern[1::2])}
            ds.set_camera(cam_b)
            out["background_blocks_b"] = ds.info()["background_blocks"]
            ds.set_camera(cam_a)
            out["background_blocks_a"] = ds.info()["background_blocks"]
            out["blocks"] = ((w + 7) // 8) * ((h + 7) // 8)
            for spp in (16, 512):  # frames of camera A, the view with open background, after a move to it
                for key, kw in (("proof", {}), ("no_proof", dict(background_proof=False)), ("proof_reprobe", dict(reprobe=True))):
                    ds.set_camera(cam_a, **kw)
                    timed_frames(spp, key)
        # the host proof: the diagnostic at the full frame minus the same tree build with a two-block frame
        for cam, sc in (("a", sc_a), ("b", sc_b)):
            full = [_ms(lambda: background_blocks(sc, 0)) for _ in range(a.reps)]
            sc.desc.width, sc.desc.height = 16, 9
            tiny = [_ms(lambda: background_blocks(sc, 0)) for _ in range(a.reps)]
            sc.desc.width, sc.desc.height = w, h
            out[f"host_diagnostic_{cam}_full_ms"], out[f"host_diagnostic_{cam}_two_blocks_ms"] = _stat(full, 1), _stat(tiny, 1)
            out[f"host_proof_{cam}_ms"] = round(float(np.median(full) - np.median(tiny)), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
