"""Keyframe interpolation's guided step at the bench geometry plus two appended keyframes (N = 3456 + 2 * 384 tokens, full width, 48 layers,
bf16, random weights): ms per classifier-free-guided step three ways, alternated --
  eager glue   the existing joint_denoise_loop(video_guider=CFGGuider): two X0Model calls, torch guide + blend, ltx2_euler_step
  one call     LTXModel.guided_step_ per step (ltx2_dit_guided_step)
  graph        one captured graph of all the steps (ltx2_dit_graph_capture_guided)
and the guided Euler kernel alone against a device copy of the same bytes.

    python tools/keyframe_time.py [--steps 8] [--reps 3] [--layers 48] [out.md]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoConditionByKeyframeIndex, VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import guided_denoise_loop, joint_denoise_loop  # noqa: E402
from ltx_2_mlx_amd.types import VideoLatentShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    tools = VideoLatentTools(VideoLatentPatchifier(1), VideoLatentShape(1, 128, 9, 16, 24), fps=24.0)
    st = tools.create_initial_state(device=dev)
    for idx, strength in ((0, 1.0), (64, 0.9)):
        st = VideoConditionByKeyframeIndex(torch.randn(1, 128, 1, 16, 24, generator=g, device=dev), idx, strength).apply_to(st, tools)
    n = st.latent.shape[1]
    st = st.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    ctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    nctx = 0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev)
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    x0m, stepper, guider = X0Model(m), EulerDiffusionStep(), CFGGuider(3.0)
    ways = {
        "eager glue (existing)": lambda: joint_denoise_loop(x0m, False, st, None, sig, ctx, None, stepper, use_hip_graph=False,
                                                            negative_video_context=nctx, video_guider=guider),
        "one guided_step_ call per step": lambda: guided_denoise_loop(x0m, st, sig, ctx, nctx, guider, stepper, use_hip_graph=False),
        "graph replay (capture included)": lambda: guided_denoise_loop(x0m, st, sig, ctx, nctx, guider, stepper, use_hip_graph=True),
    }
    best = {k: float("inf") for k in ways}
    for rep in range(a.reps + 1):                   # the first round warms up (allocation, the per-prompt setup); alternated afterwards
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                best[name] = min(best[name], (time.perf_counter() - t0) / a.steps * 1e3)
    # replay alone: capture once, time the launches
    neg = m.clone_sharing_weights()
    lat = st.latent[0].clone()
    mask, clean = st.denoise_mask[0].reshape(-1).contiguous(), st.clean_latent[0].contiguous()
    m.prepare(ctx, st.positions, per_token=True)
    neg.prepare(nctx, st.positions, per_token=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.capture_guided_graph(neg, lat, sig, 3.0, denoise_mask=mask, clean_latent=clean)
        m.replay_guided_graph()
        side.synchronize()
        replay = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m.replay_guided_graph()
            side.synchronize()
            replay = min(replay, (time.perf_counter() - t0) / a.steps * 1e3)
    # the kernel alone beside a device copy of the bytes it moves (x, two velocities, clean in; x out: 5 x N x 128 fp32)
    x, vc, vu = (torch.randn(n, 128, generator=g, device=dev) for _ in range(3))
    ts = (mask * 0.5).contiguous()
    src, dst = torch.empty(5 * n * 128 // 2, device=dev), torch.empty(5 * n * 128 // 2, device=dev)     # a copy reads and writes: half the elements

    def timed(fn, iters=200):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    t_k = min(timed(lambda: K.guided_euler_step(x, vc, vu, ts, 3.0, 0.5, 0.25, mask=mask, clean=clean, out=x)) for _ in range(3))
    t_c = min(timed(lambda: dst.copy_(src)) for _ in range(3))
    mb = 5 * n * 128 * 4 / 1e6
    lines = [f"N = {n} tokens ({n - 768} video + 2 x 384 keyframe), {a.layers} layers, full width, bf16, cfg 3, {a.steps} steps, best of {a.reps}", "",
             "| guided step | ms / step |", "|---|---|"]
    lines += [f"| {k} | {v:.2f} |" for k, v in best.items()]
    lines += [f"| graph replay alone | {replay:.2f} |", "",
              f"guided Euler kernel alone: {t_k:.1f} us for {mb:.1f} MB ({mb / t_k * 1e-3:.2f} TB/s); device copy of the same bytes: {t_c:.1f} us "
              f"({mb / t_c * 1e-3:.2f} TB/s)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
