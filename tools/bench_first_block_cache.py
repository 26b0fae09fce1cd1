"""The first-block cache at the bench geometry (video-only DiT, N = 3456 tokens, S = 1024, 48 layers, bf16, random weights): the dev-model
standard CFG loop (cfg 3, guidance_rescale 0.7) over 40 steps, ms per step, one box, one session, alternated --
  captured   the cache off: standard_cfg_denoise_loop as before, one captured graph (the parent commit's path: nothing of the cache runs)
  eager      the cache off, one C call per step (use_hip_graph=False): what the eager loop alone costs
  t = 0      the cache on and never skipping: eager loop + copy + metric + read-back per evaluation, the pure overhead
  t = +inf   every evaluation but the first and the last step's reuses the tail: the floor
and the three kernels alone on one [N][D] fp32 stream, us per launch from device events over 50 launches.  Random weights say nothing about
hit rates or picture quality at a useful threshold: not verified with real weights.

    python tools/bench_first_block_cache.py [--steps 40] [--reps 3] [--layers 48] [out.md]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import _first_block_cache_loop, first_block_cache_last_stats, standard_cfg_denoise_loop  # noqa: E402
from ltx_2_mlx_amd.types import VideoLatentShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    vs = VideoLatentTools(VideoLatentPatchifier(1), VideoLatentShape(1, 128, 9, 16, 24), fps=25.0).create_initial_state(device=dev)
    n = vs.latent.shape[1]
    vs = vs.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    ctx, nctx = (0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev) for _ in range(2))
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    x0m = X0Model(m)
    plain = lambda graph: standard_cfg_denoise_loop(x0m, vs, sig, ctx, nctx, 3.0, 0.7, use_hip_graph=graph)      # noqa: E731
    # t = 0 is "off" for the public loop, so the driver is called directly with it
    cached = lambda t: _first_block_cache_loop(m, vs, sig, ctx, nctx, 3.0, 0.7, t, None, False)      # noqa: E731
    ways = {"captured, cache off": lambda: plain(True), "eager, cache off": lambda: plain(False), "cache on, t = 0": lambda: cached(0.0),
            "cache on, t = +inf": lambda: cached(float("inf"))}
    times, counts = {k: [] for k in ways}, {}
    for rep in range(a.reps + 1):                    # one warm-up round, alternated afterwards
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 1:
                times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
            if "cache on" in name:
                counts[name] = [(d["evaluations"], d["skips"]) for d in first_block_cache_last_stats()]
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"video-only DiT, N = {n} tokens, S = 1024, {a.layers} layers, bf16, cfg 3, guidance_rescale 0.7, {a.steps} steps; wall clock around the whole "
             f"loop (prepare included), medians of {a.reps} (min - max)", "", "| loop | ms per step | (evaluations, skips) per slot |", "|---|---|---|"]
    lines += [f"| {k} | {med[k]:.2f} ({min(times[k]):.2f} - {max(times[k]):.2f}) | {counts.get(k, '-')} |" for k in ways]
    k = list(ways)
    lines += ["", f"eager / captured: {med[k[1]] / med[k[0]]:.4f}", f"t = 0 / captured (the overhead): {med[k[2]] / med[k[0]]:.4f}",
              f"t = +inf / captured (the floor): {med[k[3]] / med[k[0]]:.4f}", ""]
    d = m.inner_dim
    h0, h1, hp, r = (torch.randn(n, d, generator=g, device=dev) for _ in range(4))

    def timed(fn, iters=50):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    L, st = K.nv.lib(), K.nv.stream
    part = torch.empty(int(L.ltx2_fbc_metric_blocks(n * d)), 2, device=dev, dtype=torch.float64)
    rec = torch.zeros(3, device=dev, dtype=torch.float64)
    save = h0.clone()
    mb = n * d * 4 / 1e6
    rows = (("copy of h0 (hipMemcpyAsync in the engine; torch copy_ here)", 2, lambda: save.copy_(h0)),
            ("fbc_head_metric (both launches; writes r and h1)", 5,
             lambda: K.nv.check(L.ltx2_fbc_head_metric(K.nv.ptr(save), K.nv.ptr(h1), K.nv.ptr(hp), K.nv.ptr(r), K.nv.ptr(save), K.nv.ptr(part), K.nv.ptr(rec), 0.0,
                                                       n * d, st()))),
            ("fbc_store_tail", 3, lambda: K.fbc_store_tail(h1, h0, tail=r)), ("fbc_apply_tail", 3, lambda: K.fbc_apply_tail(h1, r)))
    lines += [f"| kernel ([{n}][{d}] fp32) | us per launch | operands read + written | MB | GB/s |", "|---|---|---|---|---|"]
    for name, ops, fn in rows:
        us = timed(fn)
        lines.append(f"| {name} | {us:.1f} | {ops} | {ops * mb:.1f} | {ops * mb / us * 1e3:.0f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
