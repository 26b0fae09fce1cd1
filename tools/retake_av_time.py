"""The joint guided step of a retake with sound at the bench AudioVideo geometry (LTX-2.3-style AudioVideo DiT, N = 3456 video + 68 audio tokens,
S = 1024, 48 layers, bf16, random weights; cfg 3 on the video, 7 on the audio; the denoise mask on latent frames 3 .. 5 of 9 and on the audio
tokens of the same seconds): ms per STEP of an 8-step loop, alternated, medians over device events --
  captured    ltx2_dit_graph_capture_guided_joint_av once, then ltx2_dit_graph_launch per loop
  C calls     LTXModel.guided_step_joint_av_ per step (two forwards + one kernel over both latents)
  eager       joint_denoise_loop with CFGGuider on both modalities: two X0Model calls and the separate torch ops per step (the path a joint
              guided loop took before; it runs on the parent commit's library too)
and the pair kernel alone.

    python tools/retake_av_time.py [--reps 10] [--layers 48] [--steps 8] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import AudioPatchifier, CFGGuider, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import joint_denoise_loop  # noqa: E402
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
    n, na = vs.latent.shape[1], as_.latent.shape[1]
    vmask, amask = torch.zeros(1, n, 1, device=dev), torch.zeros(1, na, 1, device=dev)
    vmask[:, 3 * 384: 6 * 384] = 1.0
    amask[:, 17: 41] = 1.0
    states = []
    for st, mask in ((vs, vmask), (as_, amask)):
        clean, noise = (torch.randn(st.latent.shape, generator=g, device=dev) for _ in range(2))
        states.append(st.replace(latent=noise * mask + clean * (1 - mask), denoise_mask=mask, clean_latent=clean))
    vs, as_ = states
    vctx, actx, nvctx, nactx = [0.1 * torch.randn(1, 1024, d, generator=g, device=dev) for d in (m.inner_dim, m.audio_inner_dim, m.inner_dim, m.audio_inner_dim)]
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    x0m, stepper = X0Model(m), EulerDiffusionStep()
    have_joint = hasattr(m, "guided_step_joint_av_") and hasattr(m._L, "ltx2_dit_guided_step_joint_av")      # an A/B library from before the entry
    ways = {}
    if have_joint:
        from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state
        neg = m.clone_sharing_weights()
        m.prepare(vctx, vs.positions, per_token=True, audio_context=actx, audio_positions=as_.positions)
        neg.prepare(nvctx, vs.positions, per_token=True, audio_context=nactx, audio_positions=as_.positions)
        lat, alat = vs.latent[0].clone(), as_.latent[0].clone()
        cond = dict(denoise_mask=vmask[0, :, 0].contiguous(), clean_latent=vs.clean_latent[0].contiguous(),
                    audio_denoise_mask=amask[0, :, 0].contiguous(), audio_clean_latent=as_.clean_latent[0].contiguous())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.capture_guided_joint_graph(neg, lat, alat, sig, 3.0, 7.0, **cond)
        torch.cuda.current_stream().wait_stream(side)

        def captured():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                m.replay_guided_joint_graph()
            torch.cuda.current_stream().wait_stream(side)

        def c_calls():
            l2, a2 = vs.latent[0].clone(), as_.latent[0].clone()
            for i in range(a.steps):
                m.guided_step_joint_av_(neg, l2, a2, modality_from_state(vs.replace(latent=l2[None]), vctx, sig[i]),
                                        audio_modality_from_state(as_.replace(latent=a2[None]), actx, sig[i]), sig[i], sig[i + 1], 3.0, 7.0, **cond)

        ways["captured (one graph launch)"] = captured
        ways["C calls (guided_step_joint_av_ per step)"] = c_calls
    ways["eager (joint_denoise_loop, CFGGuider on both)"] = lambda: joint_denoise_loop(
        x0m, True, vs, as_, sig, vctx, actx, stepper, None, False, negative_video_context=nvctx, negative_audio_context=nactx, video_guider=CFGGuider(3.0),
        audio_guider=CFGGuider(7.0))
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
    base = med["eager (joint_denoise_loop, CFGGuider on both)"]
    lines = [f"LTX-2.3-style AudioVideo DiT, N = {n} + Na = {na} tokens ({int(vmask.sum())} + {int(amask.sum())} regenerated), S = 1024, {a.layers} layers, bf16, "
             f"{a.steps}-step loops, ms per step, medians of {a.reps} (min - max)", "", "| loop | ms per step | relative to the eager loop |", "|---|---|---|"]
    lines += [f"| {k} | {med[k]:.2f} ({min(times[k]):.2f} - {max(times[k]):.2f}) | {med[k] / base:.3f} |" for k in ways]
    if have_joint:
        x, vc, vu, cl = (torch.randn(n, 128, generator=g, device=dev) for _ in range(4))
        ax, avc, avu, acl = (torch.randn(na, 128, generator=g, device=dev) for _ in range(4))
        vm1, am1 = vmask[0, :, 0].contiguous(), amask[0, :, 0].contiguous()
        seg = lambda x_, c_, u_, mk, cl_, cfg: dict(x=x_, vel_cond=c_, vel_uncond=u_, timesteps=mk * 0.9, cfg_scale=cfg, mask=mk, clean=cl_, out=x_)      # noqa: E731

        def timed(fn, iters=200):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters * 1e3

        sv, sa = seg(x, vc, vu, vm1, cl, 3.0), seg(ax, avc, avu, am1, acl, 7.0)
        lines += ["", f"guided_euler_step_pair (video + audio, masked, in place): {min(timed(lambda: K.guided_euler_step_pair(sv, sa, 0.9, 0.7)) for _ in range(3)):.1f} us "
                  "(host-side call included)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
