"""OneStagePipeline's joint audio+video STG loop at the bench AudioVideo geometry (LTX-2.3-style AudioVideo DiT, N = 3456 video + 68 audio tokens,
S = 1024, 48 layers, bf16, random weights; plain CFG 3 on the video and 7 on the audio, STG on block 29 at every step, no conditioning): ms per
STEP of an 8-step loop, alternated, medians over device events --
  eager, video STG     joint_denoise_loop with an STGGuider: three X0Model calls and the torch guiders per step (the route OneStagePipeline took
                       before joint_stg_denoise_loop existed; it runs on the parent commit too)
  device, STG 1 / 0    joint_stg_denoise_loop: LTXModel.stg_step_joint_av_ per step, the audio not STG-guided (what the eager row computes)
  device, STG 1 / 1    the same with the audio STG term
  eager, STG 1 / 1     joint_stg_denoise_loop(fused=False), the comparison form
and the pair kernel alone.

    python tools/joint_stg_time.py [--reps 5] [--layers 48] [--steps 8] [--block 29] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import (AudioPatchifier, CFGGuider, EulerDiffusionStep, LTX2Scheduler, STGGuider, VideoLatentPatchifier,  # noqa: E402
                                      create_batched_stg_config)
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines import common  # noqa: E402
from ltx_2_mlx_amd.types import AudioLatentShape, VideoLatentShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--block", type=int, default=29)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    blocks = [min(a.block, a.layers - 1)]
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
    eager = "eager, video STG (joint_denoise_loop: the route before)"
    ways = {eager: lambda: common.joint_denoise_loop(x0m, True, vs, as_, sig, vctx, actx, stepper, None, False, negative_video_context=nvctx,
                                                     negative_audio_context=nactx, video_guider=CFGGuider(3.0), audio_guider=CFGGuider(7.0),
                                                     stg_guider=STGGuider(1.0), stg_perturbations=create_batched_stg_config(1, blocks=blocks), stg_cutoff=1.0)}
    if hasattr(common, "joint_stg_denoise_loop"):                # absent on the parent commit: the eager loop alone is timed there
        joint = lambda audio_stg, fused: common.joint_stg_denoise_loop(x0m, vs, as_, sig, vctx, actx, nvctx, nactx, CFGGuider(3.0), CFGGuider(7.0),      # noqa: E731
                                                                       STGGuider(1.0), STGGuider(audio_stg) if audio_stg else None, blocks, 1.0, None, False, fused)
        ways["device, STG 1 / 0 (stg_step_joint_av_ per step)"] = lambda: joint(0.0, True)
        ways["device, STG 1 / 1 (stg_step_joint_av_ per step)"] = lambda: joint(1.0, True)
        ways["eager, STG 1 / 1 (joint_stg_denoise_loop(fused=False))"] = lambda: joint(1.0, False)
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
    lines = [f"LTX-2.3-style AudioVideo DiT, N = {n} + Na = {na} tokens, S = 1024, {a.layers} layers, bf16, plain CFG 3 / 7, STG on block {blocks[0]} at every step, "
             f"{a.steps}-step loops, ms per step, medians of {a.reps} (min - max)", "", "| loop | ms per step | relative to the eager video-STG loop |", "|---|---|---|"]
    lines += [f"| {k} | {med[k]:.2f} ({min(times[k]):.2f} - {max(times[k]):.2f}) | {med[k] / med[eager]:.3f} |" for k in ways]
    if hasattr(K, "stg_euler_step_pair"):
        x, vc, vu, vp = (torch.randn(n, 128, generator=g, device=dev) for _ in range(4))
        ax, avc, avu, avp = (torch.randn(na, 128, generator=g, device=dev) for _ in range(4))
        ts = torch.tensor([0.9], device=dev)
        segs = [dict(x=x_, vel_cond=c_, vel_uncond=u_, vel_perturbed=p_, timesteps=ts, cfg_scale=s, stg_scale=1.0, out=x_.clone())
                for x_, c_, u_, p_, s in ((x, vc, vu, vp, 3.0), (ax, avc, avu, avp, 7.0))]

        def timed(fn, iters=200):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters * 1e3

        lines += ["", f"stg_euler_step_pair (video + audio, CFG and STG on both): {min(timed(lambda: K.stg_euler_step_pair(*segs, 0.9, 0.7)) for _ in range(3)):.1f} us "
                  "(host-side call included)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
