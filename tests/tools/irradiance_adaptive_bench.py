"""Times, counts and errors of the adaptive irradiance gathers (sol_irradiance_adaptive_dev); its output is
profiles/irradiance_adaptive.txt. Everything is resident in device memory, outputs allocated beforehand. The adaptive call blocks (one read-back per
round), so every leg is timed with the host clock around the call and a wait for the scene's stream; repetitions alternate after one warm-up of each
leg, the median and the range are written.

  isa      registers, LDS and scratch of the kernels in csrc/sol_gather_adaptive.hip (tests/tools/isa.sh; needs hipcc, no GPU)
  gather   the visible surface points of BASELINE config 3 (the atrium at 1920x1080), COSINE, max = 64, round = 16: threshold = 0 against
           irradiance_moments(samples = 64) of the same tree over the same points (the same words, checked) - the overhead of the rounds -, a single
           round of 64 (judge only), and positive thresholds at max = 64 and 256 with their mean count, beside fixed calls of about that count
  rounds   (for a kernel trace: `rocprofv3 --kernel-trace --stats -- python tests/tools/irradiance_adaptive_bench.py --parts rounds`) three
           threshold = 0 calls over the same points and nothing else that is timed: the compaction kernels' share of a round is read off the trace
  bake     the 64 x 64 floor bake of tests/test_gpu_lightmap_filter_var.py, max = 256: two positive thresholds at min_samples 32 and 128 - mean
           count, time, MSE against a 1024-sample truth of another seed - beside fixed calls of about the same mean count

  python tests/tools/irradiance_adaptive_bench.py [--parts isa,gather,bake] [--reps 5] [--small] [--out FILE]
A part that is not run is written down as "not measured". Lines the tool does not write are added to the profile by hand under "by hand".
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

import _paths  # noqa: F401
import lightmap_ref as lr

ROOT = _paths.ROOT
F = np.float32
SEED = 0x5017A1E


def part_isa(out):
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gather_adaptive.s")
        r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tools", "isa.sh"), path, "csrc/sol_gather_adaptive.hip"], capture_output=True, text=True)
        if r.returncode != 0:
            out.append("isa: not measured (no hipcc)")
            return
        meta, block = {}, {}
        for line in open(path):
            s = line.strip()
            if s.startswith("- ."):
                block = {}
                s = s[2:]
            if s.startswith(".name:") and "_kernel" in s:
                meta[s.split()[-1]] = block
            for key in (".vgpr_count:", ".sgpr_count:", ".group_segment_fixed_size:", ".private_segment_fixed_size:", ".vgpr_spill_count:", ".sgpr_spill_count:"):
                if s.startswith(key):
                    block[key.strip(".:")] = int(s.split()[-1])
    out.append("isa (tests/tools/isa.sh csrc/sol_gather_adaptive.hip): VGPRs, SGPRs, LDS bytes, scratch bytes, spilled VGPRs / SGPRs")
    for name, m in meta.items():
        short = name[name.index("sol_"):name.index("_kernel") + 7]
        out.append(f"  {short:30s} {m['vgpr_count']:4d} {m['sgpr_count']:4d} {m['group_segment_fixed_size']:6d} {m['private_segment_fixed_size']:3d} "
                   f"{m['vgpr_spill_count']} / {m['sgpr_spill_count']}")


def _c3_points(ds, w, h):
    import torch
    from solstrale_amd import _abi
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
    return points


class Legs:
    """Calls over one set of points on one handle, outputs allocated beforehand."""

    def __init__(self, ds, points):
        import torch
        from solstrale_amd import _abi
        self.ds, self.points, self.n, self.abi = ds, points, int(points.shape[0]), _abi
        self.out_fixed = torch.empty((self.n, 8), dtype=torch.float32, device="cuda")
        self.out_adaptive = torch.empty((self.n, 8), dtype=torch.float32, device="cuda")
        self.stats = _abi.SolGatherAdaptiveStats(size=C.sizeof(_abi.SolGatherAdaptiveStats))

    def _cfg(self, samples, seed):
        return self.abi.SolIrradianceConfig(size=C.sizeof(self.abi.SolIrradianceConfig), samples=samples, first_sample=0, seed=seed, mode=self.abi.SOL_IRRADIANCE_COSINE)

    def fixed(self, samples, seed=SEED):
        ds = self.ds
        ds._chk(ds.lib.sol_irradiance_moments_dev(ds.h, C.c_void_p(self.points.data_ptr()), None, self.n, C.byref(self._cfg(samples, seed)),
                                                  C.c_void_p(self.out_fixed.data_ptr())))
        ds.sync()

    def adaptive(self, mx, rnd, min_samples, threshold, floor, seed=SEED):
        ds = self.ds
        ad = self.abi.SolGatherAdaptive(size=C.sizeof(self.abi.SolGatherAdaptive), round=rnd, min_samples=min_samples, threshold=threshold, floor=floor)
        ds._chk(ds.lib.sol_irradiance_adaptive_dev(ds.h, C.c_void_p(self.points.data_ptr()), None, self.n, C.byref(self._cfg(mx, seed)), C.byref(ad),
                                                   C.c_void_p(self.out_adaptive.data_ptr()), C.byref(self.stats)))
        ds.sync()


def timed_alternating(legs, reps):
    """ms per leg: [reps] host-clock times of each call (which ends in a wait for the stream), alternating after one warm-up of each."""
    for call in legs.values():
        call()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, call in legs.items():
            t0 = time.perf_counter()
            call()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def _line(k, r, extra=""):
    return f"  {k:44s} {np.median(r):9.3f} ms  ({min(r):9.3f} - {max(r):9.3f}){extra}"


def _atrium(small):
    from solstrale_amd import RenderConfig, scenes
    w, h = (480, 270) if small else (1920, 1080)
    sc = scenes.sponza_like(RenderConfig(w, h, 16), n_triangles=20000, texture_size=16) if small else scenes.sponza_like(RenderConfig(w, h, 16))
    return sc, w, h


def part_gather(out, reps, small):
    import torch
    from solstrale_amd import DeviceScene
    sc, w, h = _atrium(small)
    mx = 64
    with DeviceScene(sc) as ds:
        L = Legs(ds, _c3_points(ds, w, h))
        torch.cuda.synchronize()
        n = L.n
        out.append(f"gather: sponza_like {sc.desc.n_triangles} triangles {w}x{h}, {n} visible surface points, COSINE, max = {mx}, device route, host clock around the "
                   f"blocking call, {reps} repetitions alternating after one warm-up of each: median (least - most)")
        legs = {f"irradiance_moments(samples = {mx})": lambda: L.fixed(mx),
                "adaptive threshold 0, round 16 (4 rounds)": lambda: L.adaptive(mx, 16, 32, 0.0, 0.0),
                "adaptive threshold 0, round 32 (2 rounds)": lambda: L.adaptive(mx, 32, 32, 0.0, 0.0),
                "adaptive threshold 0, round 64 (1 round)": lambda: L.adaptive(mx, 64, 64, 0.0, 0.0)}
        ms = timed_alternating(legs, reps)
        L.fixed(mx)
        L.adaptive(mx, 16, 32, 0.0, 0.0)
        same = torch.equal(L.out_fixed.view(torch.int32), L.out_adaptive.view(torch.int32))
        base = float(np.median(ms[f"irradiance_moments(samples = {mx})"]))
        for k, r in ms.items():
            out.append(_line(k, r, f"   x {np.median(r) / base:.3f}"))
        out.append(f"  threshold 0 answers the fixed call's words: {'yes' if same else 'NO'}; rounds {L.stats.rounds}, paths {L.stats.paths} = {n} x {mx}: "
                   f"{'yes' if L.stats.paths == n * mx else 'NO'}")
        for big, threshold in ((64, 0.2), (256, 0.1), (256, 0.2)):
            L.adaptive(big, 16, 32, threshold, 0.01)
            st = L.stats
            mean = st.paths / max(st.rows_valid, 1)
            near = max(16, int(round(mean / 16.0)) * 16)
            legs = {f"adaptive max {big}, threshold {threshold}, floor 0.01": lambda m=big, t=threshold: L.adaptive(m, 16, 32, t, 0.01),
                    f"irradiance_moments(samples = {near})": lambda k=near: L.fixed(k)}
            if near != big:
                legs[f"irradiance_moments(samples = {big})"] = lambda k=big: L.fixed(k)
            ms = timed_alternating(legs, min(reps, 3))
            out.append(f"  max {big}, threshold {threshold}, min_samples 32: mean count {mean:.2f} ({st.rows_converged} of {st.rows_valid} rows converged, {st.rows_capped} "
                       f"capped, {st.rounds} rounds)")
            for k, r in ms.items():
                out.append("  " + _line(k, r))


def part_rounds(out, small):
    from solstrale_amd import DeviceScene
    sc, w, h = _atrium(small)
    with DeviceScene(sc) as ds:
        L = Legs(ds, _c3_points(ds, w, h))
        for _ in range(3):
            L.adaptive(64, 16, 32, 0.0, 0.0)
        out.append(f"rounds: three threshold = 0 calls of four rounds over {L.n} points (for a kernel trace; nothing is timed here)")


def part_bake(out, reps):
    import torch
    from solstrale_amd import CameraConfig, DeviceScene, RenderConfig, SceneBuilder
    W = H = 64
    mx, high = 256, 1024
    V, T, N = lr.grid_mesh(8, 2)
    V, T, N = (np.ascontiguousarray(a[:, [0, 2, 1]]) for a in (V, T, N))
    T = np.ascontiguousarray(T * F(0.75) + F(0.125), dtype=F)
    b = SceneBuilder()
    first, n = b.triangles(V.astype(np.float64), b.Lambertian(b.SolidColor(0.7, 0.7, 0.7)), uvs=T)
    light = b.Quad((-1.0, 2.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), b.DiffuseLight(8, 8, 8))
    sc = b.finish(b.Bvh(list(range(first, first + n)) + [light]), CameraConfig(40.0, 0.0, (0.0, 6.0, 6.0), (0.0, 0.0, 0.0), (0, 1, 0)), (0.0, 0.0, 0.0),
                  RenderConfig(32, 32, 1))
    out.append(f"bake: floor under a quad light, {W} x {H} atlas, COSINE, round 16, floor 0.01, max = {mx}: MSE of the irradiance (sum x pi / count) "
               f"over the owned texels against the {high}-sample gather of another seed; ms: median of {reps} by the host clock")
    with DeviceScene(sc) as ds:
        dV, dT, dN = (torch.from_numpy(a).cuda() for a in (V, T, N))
        points, texels = ds.lightmap_points(dV, dT, W, H, normals=dN)
        owned = (texels[:, 0] != -1).cpu().numpy()
        L = Legs(ds, points)
        L.fixed(high, seed=977 + SEED)
        e_truth = L.out_fixed.cpu().numpy()[owned, :3].astype(np.float64) * (np.pi / high)

        def mse_of(rows):
            r = rows.cpu().numpy()[owned]
            count = r.view(np.uint32)[:, 3].astype(np.float64)
            return float(((r[:, :3].astype(np.float64) * (np.pi / count[:, None]) - e_truth) ** 2).mean())

        for min_samples in (32, 128):
            for threshold in (0.05, 0.1):
                L.adaptive(mx, 16, min_samples, threshold, 0.01)
                st = L.stats
                mean = st.paths / max(st.rows_valid, 1)
                mse_adaptive = mse_of(L.out_adaptive)
                counts = L.out_adaptive.cpu().numpy().view(np.uint32)[owned, 3]
                dark = int((L.out_adaptive.cpu().numpy()[owned, :3].sum(axis=1) == 0).sum())
                near = max(16, int(round(mean / 16.0)) * 16)
                L.fixed(near)
                mse_fixed = mse_of(L.out_fixed)
                ms = timed_alternating({"adaptive": lambda t=threshold, m=min_samples: L.adaptive(mx, 16, m, t, 0.01), "fixed": lambda k=near: L.fixed(k)}, reps)
                out.append(f"  min_samples {min_samples}, threshold {threshold}: mean count {mean:.2f} ({st.rows_converged} of {st.rows_valid} converged, {st.rows_capped} "
                           f"capped, {st.rounds} rounds; {int((counts == min_samples).sum())} rows stopped at {min_samples}, {dark} rows with a sum of 0), MSE "
                           f"{mse_adaptive:.5g}, {np.median(ms['adaptive']):.3f} ms;  fixed samples = {near}: MSE {mse_fixed:.5g}, {np.median(ms['fixed']):.3f} ms;  "
                           f"MSE fixed / adaptive {mse_fixed / mse_adaptive:.3f}")
        out.append(f"  mean irradiance of the truth {e_truth.mean():.4g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="isa,gather,bake")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="gather, rounds: a 20 000-triangle atrium at 480x270 (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irradiance_adaptive.txt"))
    a = ap.parse_args()
    parts = a.parts.split(",")
    out = ["adaptive irradiance gathers (DESIGN.md 28): tests/tools/irradiance_adaptive_bench.py " + " ".join(sys.argv[1:])]
    if "isa" in parts:
        part_isa(out)
    if {"gather", "rounds", "bake"} & set(parts):
        from solstrale_amd import device_count
        if device_count() < 1:
            raise SystemExit("irradiance_adaptive_bench: no HIP device visible; parts gather, rounds and bake have nothing to measure without one")
    if "gather" in parts:
        part_gather(out, a.reps, a.small)
    if "rounds" in parts:
        part_rounds(out, a.small)
    if "bake" in parts:
        part_bake(out, a.reps)
    out.extend(f"{p}: not measured" for p in ("isa", "gather", "bake") if p not in parts)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
