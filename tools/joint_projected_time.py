"""OneStagePipeline's joint audio+video guided loop at the bench AudioVideo geometry (LTX-2.3-style AudioVideo DiT, N = 3456 video + 68 audio
tokens, S = 1024, 48 layers, bf16, random weights; cfg 3 on the video, 7 on the audio, rescale 0.7: a CFGStarRescalingGuider per modality, no
conditioning): ms per STEP of an 8-step loop, alternated, medians over device events --
  captured    joint_projected_denoise_loop without a callback: ltx2_dit_graph_capture_projected_joint_av, then ltx2_dit_graph_launch (the capture
              is part of every timed loop, as it is of every pipeline call)
  C calls     joint_projected_denoise_loop with use_hip_graph=False: LTXModel.projected_step_joint_av_ per step (two forwards, the sums kernel,
              the step kernel over both latents)
  eager       joint_denoise_loop with the same guiders: two X0Model calls and the torch guiders per step (the route OneStagePipeline took
              before; it runs on the parent commit's library too)
and the two pair kernels alone.

    python tools/joint_projected_time.py [--reps 10] [--layers 48] [--steps 8] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import AudioPatchifier, CFGStarRescalingGuider, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines import common  # noqa: E402
from ltx_2_mlx_amd.types import AudioLatentShape, VideoLatentShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(model_type=LTXModelType.AudioVideo, num_layers=a.layers, caption_channels=None, cross_attention_adaln=True, apply_gated_attention=True,
                 av_ca_timestep_scale_multiplier=1000, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    vs = VideoLatentTools(VideoLatentPatchifier(1), VideoLatentShape(1, 128, 9, 16, 24), fps=25.0).create_initial_state(device=dev)
    as_ = AudioLatentTools(AudioPatchifier(1), AudioLatentShape(1, 8, 68, 16)).create_initial_state(device=dev)
    vs, as_ = (st.replace(latent=torch.randn(st.latent.shape, generator=g, device=dev)) for st in (vs, as_))
    n, na = vs.latent.shape[1], as_.latent.shape[1]
    vctx, actx, nvctx, nactx = [0.1 * torch.randn(1, 1024, d, generator=g, device=dev) for d in (m.inner_dim, m.audio_inner_dim, m.inner_dim, m.audio_inner_dim)]
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    x0m, stepper = X0Model(m), EulerDiffusionStep()
    guiders = lambda: (CFGStarRescalingGuider(3.0), CFGStarRescalingGuider(7.0))      # noqa: E731
    ways = {}
    if hasattr(common, "joint_projected_denoise_loop"):          # absent on the parent commit: the eager loop alone is timed there
        for name, graph in (("captured (capture + one graph launch)", True), ("C calls (projected_step_joint_av_ per step)", False)):
            ways[name] = lambda graph=graph: common.joint_projected_denoise_loop(x0m, vs, as_, sig, vctx, actx, nvctx, nactx, *guiders(), stepper, None, graph)
    eager = "eager (joint_denoise_loop, CFG* on both)"
    ways[eager] = lambda: common.joint_denoise_loop(x0m, True, vs, as_, sig, vctx, actx, stepper, None, False, negative_video_context=nvctx,
                                                    negative_audio_context=nactx, video_guider=guiders()[0], audio_guider=guiders()[1])
    times = {k: [] for k in ways}
    for rep in range(a.reps + 2):                    # two warm-up rounds (allocation, the per-prompt setup of both contexts), alternated afterwards
        for name, fn in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                times[name].append(e0.elapsed_time(e1) / a.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"LTX-2.3-style AudioVideo DiT, N = {n} + Na = {na} tokens, S = 1024, {a.layers} layers, bf16, CFG* 3 / 7, {a.steps}-step loops, ms per step, "
             f"medians of {a.reps} (min - max)", "", "| loop | ms per step | relative to the eager loop |", "|---|---|---|"]
    lines += [f"| {k} | {med[k]:.2f} ({min(times[k]):.2f} - {max(times[k]):.2f}) | {med[k] / med[eager]:.3f} |" for k in ways]
    if hasattr(K, "projected_euler_step_pair"):
        x, vc, vu = (torch.randn(n, 128, generator=g, device=dev) for _ in range(3))
        ax, avc, avu = (torch.randn(na, 128, generator=g, device=dev) for _ in range(3))
        ts = torch.tensor([0.9], device=dev)
        segs = [dict(x=x_, vel_cond=c_, vel_uncond=u_, timesteps=ts, mode=0, scale=s, out=x_.clone(),
                     partials=torch.empty(K.guidance_sums_blocks(*x_.shape), 5, device=dev, dtype=torch.float64)) for x_, c_, u_, s in ((x, vc, vu, 3.0), (ax, avc, avu, 7.0))]
        sums = [{k: v for k, v in s.items() if k in ("x", "vel_cond", "vel_uncond", "timesteps", "partials")} for s in segs]

        def timed(fn, iters=200):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters * 1e3

        lines += ["", f"guidance_sums_pair (video + audio): {min(timed(lambda: K.guidance_sums_pair(*sums)) for _ in range(3)):.1f} us; "
                  f"projected_euler_step_pair (CFG* on both): {min(timed(lambda: K.projected_euler_step_pair(*segs, 0.9, 0.7)) for _ in range(3)):.1f} us "
                  "(host-side call included)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
