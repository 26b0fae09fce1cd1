"""One guided step of the standard one-stage loop at the bench geometry (video-only DiT, N = 3456 tokens, S = 1024, 48 layers, bf16, random
weights; cfg 3, guidance_rescale 0.7): ms per call, alternated, medians over device events --
  guided Euler step          LTXModel.guided_step_ (ltx2_dit_guided_step): the yardstick, it runs at the parent commit too
  rescaled guided step       LTXModel.rescaled_guided_step_ (two forwards, the two statistics launches, the step kernel), and at rescale 0
  4-step loop                one rescaled_guided_step_ call per step against one replay of the captured graph
and the new kernels alone on the video latent beside guided_euler_step, with the bytes each moves: 200 launches as ONE captured graph, so
that the figure is the device's time per launch and not the host's time per Python call (the host-launched figure is printed beside it).
The operands of 200 identical launches stay in the 256 MB last-level cache: the bandwidth is that cache's, not HBM's.

    python tools/standard_cfg_time.py [--reps 20] [--layers 48] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import modality_from_state  # noqa: E402
from ltx_2_mlx_amd.types import VideoLatentShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
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
    neg = m.clone_sharing_weights()
    m.prepare(ctx, vs.positions)
    neg.prepare(nctx, vs.positions)
    lat = vs.latent[0].clone()
    s0, s1 = 0.9, 0.7
    vm = lambda s: modality_from_state(vs, ctx, s, uniform=True)      # noqa: E731
    ways = {"guided Euler step (guided_step_)": lambda: m.guided_step_(neg, lat.clone(), vm(s0), s0, s1, 3.0),
            "rescaled guided step (rescaled_guided_step_, rescale 0.7)": lambda: m.rescaled_guided_step_(neg, lat.clone(), vm(s0), s0, s1, 3.0, 0.7),
            "rescaled guided step, rescale 0 (no statistics)": lambda: m.rescaled_guided_step_(neg, lat.clone(), vm(s0), s0, s1, 3.0, 0.0)}
    sig = [float(s) for s in LTX2Scheduler().execute(steps=4)]
    loop_lat = lat.clone()

    def per_call_loop():
        for i in range(4):
            m.rescaled_guided_step_(neg, loop_lat, vm(sig[i]), sig[i], sig[i + 1], 3.0, 0.7)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m.capture_rescaled_guided_graph(neg, loop_lat, sig, 3.0, 0.7)
    side.synchronize()
    ways["4-step loop, one C call per step"] = per_call_loop
    ways["4-step loop, one graph replay"] = m.replay_rescaled_guided_graph
    times = {k: [] for k in ways}
    for rep in range(a.reps + 2):                    # two warm-up rounds, alternated afterwards
        for name, fn in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"video-only DiT, N = {n} tokens, S = 1024, {a.layers} layers, bf16, cfg 3, guidance_rescale 0.7, medians of {a.reps} (min - max)", "", "| call | ms |",
             "|---|---|"]
    lines += [f"| {k} | {med[k]:.2f} ({min(times[k]):.2f} - {max(times[k]):.2f}) |" for k in ways]
    k = list(ways)
    lines += ["", f"rescaled guided step / guided Euler step: {med[k[1]] / med[k[0]]:.4f}", f"without statistics / guided Euler step: {med[k[2]] / med[k[0]]:.4f}",
              f"graph replay / per-call loop: {med[k[4]] / med[k[3]]:.4f}", ""]
    x, vc, vu, out = (torch.randn(n, 128, generator=g, device=dev) for _ in range(4))
    ts = torch.full((1,), 0.9, device=dev)
    blocks = K.channel_guidance_stats_blocks(n, 128)
    partials = torch.empty(blocks, 4, 128, device=dev, dtype=torch.float64)
    stats = torch.empty(4, 128, device=dev)

    def span(run, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    def timed(fn, iters=200):
        """-> (us per call inside one captured graph of `iters` calls, us per call from the host), each the best of three"""
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(iters):
                fn()
        graph.replay()
        host = lambda: [fn() for _ in range(iters)]      # noqa: E731
        return min(span(graph.replay, iters) for _ in range(3)), min(span(host, iters) for _ in range(3))

    mb = n * 128 * 4 / 1e6          # one [N][C] fp32 operand
    lines += ["| kernel (video latent, uniform timesteps) | us in a graph of 200 | us launched from the host | operands read + written | MB | GB/s (graph) |",
              "|---|---|---|---|---|---|"]
    for name, ops, fn in (("guided_euler_step", 4, lambda: K.guided_euler_step(x, vc, vu, ts, 3.0, 0.9, 0.7, out=out)),
                          (f"channel_guidance_stats (two launches, {blocks - 1} blocks of rows)", 3,
                           lambda: K.channel_guidance_stats(x, vc, vu, ts, 3.0, partials=partials, stats=stats)),
                          ("rescaled_guided_euler_step", 4, lambda: K.rescaled_guided_euler_step(x, vc, vu, ts, 3.0, 0.7, 0.9, 0.7, stats=stats, out=out)),
                          ("rescaled_guided_euler_step, no stats", 4, lambda: K.rescaled_guided_euler_step(x, vc, vu, ts, 3.0, 0.7, 0.9, 0.7, out=out))):
        us, host_us = timed(fn)
        lines.append(f"| {name} | {us:.1f} | {host_us:.1f} | {ops} | {ops * mb:.2f} | {ops * mb / us * 1e3:.0f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
