"""One stage-1 step of the two-stage pipeline at the bench AudioVideo geometry (LTX-2.3-style AudioVideo DiT, N = 3456 video + 68 audio tokens,
S = 1024, 48 layers, bf16, random weights; cfg 3 / 7, modality 3): ms per call, alternated, medians over device events --
  ltx2_dit_denoise_step_av   the existing joint step (one forward + x0 + Euler): the yardstick, it runs at the parent commit too
  plain forward              ltx2_dit_forward_av
  isolated forward           ltx2_dit_forward_isolated_av (no cross-modal attention)
  fused step                 LTXModel.mm_guided_step_av_ (three forwards + one kernel over both latents)
  eager step                 multimodal_denoise_loop(fused=False): three X0Model calls and the separate torch ops
and the four new kernels alone on the video latent.

    python tools/two_stage_time.py [--reps 20] [--layers 48] [out.md]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import AudioPatchifier, MultiModalGuider, MultiModalGuiderParams, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning import VideoLatentTools  # noqa: E402
from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state, multimodal_denoise_loop  # noqa: E402
from ltx_2_mlx_amd.types import AudioLatentShape, VideoLatentShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=48)
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
    vs = vs.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    as_ = as_.replace(latent=torch.randn(1, na, 128, generator=g, device=dev))
    ctxs = [0.1 * torch.randn(1, 1024, d, generator=g, device=dev) for d in (m.inner_dim, m.audio_inner_dim, m.inner_dim, m.audio_inner_dim)]
    vctx, actx, nvctx, nactx = ctxs
    sig = [0.9, 0.7]
    vg = MultiModalGuider(MultiModalGuiderParams(cfg_scale=3.0, modality_scale=3.0))
    ag = MultiModalGuider(MultiModalGuiderParams(cfg_scale=7.0, modality_scale=3.0))
    vm, am = modality_from_state(vs, vctx, sig[0], uniform=True), audio_modality_from_state(as_, actx, sig[0], uniform=True)
    neg = m.clone_sharing_weights()
    m.prepare(vctx, vs.positions, audio_context=actx, audio_positions=as_.positions)
    neg.prepare(nvctx, vs.positions, audio_context=nactx, audio_positions=as_.positions)
    lat, alat = vs.latent[0].clone(), as_.latent[0].clone()
    iso = (torch.empty_like(lat), torch.empty_like(alat))
    x0m = X0Model(m)
    ways = {"ltx2_dit_denoise_step_av (existing joint step)": lambda: m.denoise_step_(lat.clone(), vm, sig[0], sig[1], audio_latent=alat.clone(), audio=am),
            "plain forward": lambda: m(vm, am),
            "isolated forward": lambda: m.forward_isolated(vm, am),
            "fused step (mm_guided_step_av_)": lambda: m.mm_guided_step_av_(neg, lat.clone(), alat.clone(), vm, am, sig[0], sig[1], vg.params, ag.params, isolated=iso),
            "eager step (three X0Model calls + torch ops)": lambda: multimodal_denoise_loop(x0m, vs, as_, sig, vctx, actx, nvctx, nactx, vg, ag, fused=False)}
    times = {k: [] for k in ways}
    for rep in range(a.reps + 2):                    # two warm-up rounds (allocation, the per-prompt setup of both contexts), alternated afterwards
        for name, fn in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= 2:
                times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"LTX-2.3-style AudioVideo DiT, N = {n} + Na = {na} tokens, S = 1024, {a.layers} layers, bf16, medians of {a.reps} (min - max)", "",
             "| call | ms | relative to the plain forward |", "|---|---|---|"]
    lines += [f"| {k} | {med[k]:.2f} ({min(times[k]):.2f} - {max(times[k]):.2f}) | {med[k] / med['plain forward']:.3f} |" for k in ways]
    lines += ["", f"isolated / plain forward: {med['isolated forward'] / med['plain forward']:.3f}",
              f"fused step / eager step: {med['fused step (mm_guided_step_av_)'] / med['eager step (three X0Model calls + torch ops)']:.3f}", ""]
    x, vc, vu, vi = (torch.randn(n, 128, generator=g, device=dev) for _ in range(4))
    ax, avc, avu, avi = (torch.randn(na, 128, generator=g, device=dev) for _ in range(4))
    ts = torch.full((1,), 0.9, device=dev)
    out, aout = torch.empty_like(x), torch.empty_like(ax)
    part = K.mm_guidance_sums(x, vc, ts, 3.0, 0.0, 3.0, vel_uncond=vu, vel_isolated=vi)

    def timed(fn, iters=200):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    seg = lambda x_, c_, u_, i_, o_, cfg: dict(x=x_, vel_cond=c_, vel_uncond=u_, vel_isolated=i_, timesteps=ts, cfg_scale=cfg, stg_scale=0.0, modality_scale=3.0, out=o_)  # noqa: E731
    for name, fn in (("mm_guided_euler_step (video)", lambda: K.mm_guided_euler_step(x, vc, ts, 3.0, 0.0, 3.0, 0.9, 0.7, vel_uncond=vu, vel_isolated=vi, out=out)),
                     ("mm_guided_euler_step_pair (video + audio)", lambda: K.mm_guided_euler_step_pair(seg(x, vc, vu, vi, out, 3.0), seg(ax, avc, avu, avi, aout, 7.0), 0.9, 0.7)),
                     ("mm_guidance_sums (video)", lambda: K.mm_guidance_sums(x, vc, ts, 3.0, 0.0, 3.0, vel_uncond=vu, vel_isolated=vi, partials=part)),
                     ("mm_rescaled_euler_step (video)", lambda: K.mm_rescaled_euler_step(x, vc, ts, part, 3.0, 0.0, 3.0, 0.7, 0.9, 0.7, vel_uncond=vu, vel_isolated=vi, out=out))):
        lines.append(f"{name}: {min(timed(fn) for _ in range(3)):.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
