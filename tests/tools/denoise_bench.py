"""Times the device denoiser (sol_denoise) on a 1920x1080 frame at K = 1, 5 and 8 passes (not a pytest): device events on the
scene's stream (bound to a torch stream) around REPS calls after WARMUP, median of ROUNDS rounds. Usage: python denoise_bench.py [--out FILE]"""
import _paths  # noqa: F401  (sys.path)
import argparse
import statistics

import numpy as np
import torch

from solstrale_amd import DeviceScene, RenderConfig, scenes

W, H, N, M = 1920, 1080, 16, 16
WARMUP, REPS, ROUNDS = 3, 10, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    lines = []
    g = torch.Generator(device="cuda").manual_seed(1)
    img = (torch.rand(H, W, 3, device="cuda", generator=g) ** 4 * 40. * N).contiguous()
    alb = (torch.rand(H, W, 3, device="cuda", generator=g) * 1.2 * M).contiguous()
    nrm = torch.randn(H, W, 3, device="cuda", generator=g)
    nrm = (nrm / nrm.norm(dim=-1, keepdim=True) * M).contiguous()
    nrm[torch.rand(H, W, device="cuda", generator=g) < 0.1] = 0.
    stream = torch.cuda.Stream()  # (a stream of its own: handle 0, torch's default stream, would mean "the scene's own stream")
    torch.cuda.synchronize()
    with DeviceScene(scenes.cornell_box(RenderConfig(W, H, 1)), no_work_order_probe=True) as ds, torch.cuda.stream(stream):
        ds.set_stream(stream.cuda_stream)
        for k in (1, 5, 8):
            work = img.clone()
            for _ in range(WARMUP):
                ds.denoise(work.data_ptr(), N, alb.data_ptr(), nrm.data_ptr(), M, iterations=k)
            ms = []
            for _ in range(ROUNDS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(REPS):
                    ds.denoise(work.data_ptr(), N, alb.data_ptr(), nrm.data_ptr(), M, iterations=k)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b) / REPS)
            med = statistics.median(ms)
            # unique bytes: prepare reads 3 x 12 B and writes 2 x 16 B per pixel, a pass reads 2 x 16 B and writes 16 B, finish reads 16 + 12 B
            # and writes 12 B; the 24 further taps of a pass are re-reads served by the caches
            unique = W * H * (36 + 32 + k * 48 + 40)
            lines.append(f"denoise {W}x{H} K={k}: {med:.3f} ms (median of {ROUNDS} x {REPS} calls; min {min(ms):.3f}, max {max(ms):.3f}), "
                         f"{unique / med / 1e6:.0f} GB/s of unique bytes")
            print(lines[-1], flush=True)
        ds.set_stream(0)
    torch.cuda.synchronize()
    assert np.isfinite(work.cpu().numpy()).all()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
