"""Time the temporal x2 latent upscaler and its per-frame GroupNorm kernel on the MI355X (device events around 20 back-to-back calls, warm-up first, new and
old forms alternated inside one timed loop).  Prints one JSON line per measurement.

    python tools/temporal_upscaler_time.py [--reps 50] [--warmup 20] [--only pass,norm]

pass: TemporalUpscaler.forward_nhwc at the full width (128 -> 512, 4 + 4 blocks, random weights) on the stage-1 latent 9x16x24 and on
      9x32x48, both semantics.
norm: ltx2_groupnorm_frames_silu (with residual and SiLU) on [17][384][512] and [17][1536][512], interleaved and contiguous, against
      the only way the parent commit computes per-frame statistics: ltx2_groupnorm_silu once per frame (contiguous groups; it has no
      interleaved form), and against a device-to-device copy of the same tensor (hipMemcpy through torch) as the HBM copy rate.
      bytes = x read + res read + y written = 6 bytes per element; copy bytes = 4 per element."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.model.upscaler import TemporalUpscaler  # noqa: E402


def timed(fns, reps, warmup, inner=1):
    """median / min ms per call of each fn.  One event pair brackets `inner` back-to-back calls, so the interval is the device's time
    for the queue of launches and not the host's gap after the first event; the forms alternate inside one loop (same clocks, same
    neighbours)."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / inner)
    return [(statistics.median(m), min(m)) for m in ms]


def time_norm(reps, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for frames, P, C in ((17, 384, 512), (17, 1536, 512)):
        x = torch.randn(frames, P, C, generator=g).to(dev, torch.bfloat16)
        res = torch.randn(frames, P, C, generator=g).to(dev, torch.bfloat16)
        gamma, beta = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
        y = torch.empty_like(x)
        fns = [lambda: K.groupnorm_frames_silu(x, gamma, beta, 32, res=res, interleaved=True),
               lambda: K.groupnorm_frames_silu(x, gamma, beta, 32, res=res, interleaved=False),
               lambda: [K.groupnorm_silu(x[f], gamma, beta, 32, res=res[f]) for f in range(frames)],
               lambda: y.copy_(x)]
        names = ["frames_interleaved", "frames_contiguous", "per_frame_groupnorm_silu_x%d" % frames, "copy"]
        r = timed(fns, reps, warmup, inner=20)
        n = x.numel()
        copy_rate = 4 * n / (r[3][0] * 1e-3) / 1e12
        for name, (med, mn), byts in zip(names, r, (6 * n, 6 * n, 8 * n, 4 * n)):
            rate = byts / (med * 1e-3) / 1e12
            print(json.dumps({"what": "norm", "shape": [frames, P, C], "form": name, "median_us": round(med * 1e3, 2), "min_us": round(mn * 1e3, 2),
                              "bytes": byts, "TB_per_s": round(rate, 3), "fraction_of_copy_rate": round(rate / copy_rate, 3)}))
        same = torch.equal(K.groupnorm_frames_silu(x, gamma, beta, 32, res=res, interleaved=False),
                           torch.stack([K.groupnorm_silu(x[f], gamma, beta, 32, res=res[f]) for f in range(frames)]))
        diff = (K.groupnorm_frames_silu(x, gamma, beta, 32, res=res, interleaved=False).float()
                - torch.stack([K.groupnorm_silu(x[f], gamma, beta, 32, res=res[f]) for f in range(frames)]).float()).abs().max()
        print(json.dumps({"what": "norm_vs_per_frame_loop", "shape": [frames, P, C], "bit_identical": bool(same), "max_abs_diff": float(diff)}))


def time_pass(reps, warmup):
    dev = torch.device("cuda:0")
    for cs in (False, True):
        up = TemporalUpscaler(device=dev, checkpoint_semantics=cs)
        up.init_random_weights(seed=0)
        for f, h, w in ((9, 16, 24), (9, 32, 48)):
            x = torch.randn(f, h, w, 128, generator=torch.Generator().manual_seed(1)).to(dev, torch.bfloat16)
            (med, mn), = timed([lambda: up.forward_nhwc(x)], reps, warmup)
            print(json.dumps({"what": "pass", "latent": [f, h, w], "checkpoint_semantics": cs, "median_ms": round(med, 3), "min_ms": round(mn, 3),
                              "out_frames": 2 * f - 1}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="pass,norm")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("temporal_upscaler_time.py needs an MI355X: there is no CPU timing")
    if "norm" in a.only:
        time_norm(a.reps, a.warmup)
    if "pass" in a.only:
        time_pass(max(10, a.reps // 2), max(3, a.warmup // 5))


if __name__ == "__main__":
    main()
