"""The audio-to-video pipeline's stage-1 loop at its default geometry (512x768x97 -> stage 1 at 256x384: N = 13 * 8 * 12 = 1248 video tokens, 97
frozen audio tokens; AudioVideo model, full width, 48 layers, bf16, random weights): ms per classifier-free-guided step three ways, alternated --
  eager glue   the existing joint_denoise_loop(video_guider=CFGGuider(3), audio_guider=CFGGuider(1)) over the frozen audio state: two X0Model
               calls, torch guide + blend, ltx2_euler_step per modality
  one call     LTXModel.guided_step_av_ per step (ltx2_dit_guided_step_av)
  graph        one captured graph of all the steps (ltx2_dit_graph_capture_guided_av), capture included
and the replay alone.

    python tools/a2vid_time.py [--steps 8] [--reps 3] [--layers 48] [out.md]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd.components import CFGGuider, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier  # noqa: E402
from ltx_2_mlx_amd.components.patchifiers import AudioPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import frozen_audio_guided_loop, joint_denoise_loop, video_tools_for  # noqa: E402
from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(model_type=LTXModelType.AudioVideo, num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    g = torch.Generator(device=dev).manual_seed(3)
    frames, h, w, fps = 97, 256, 384, 25.0
    st = video_tools_for(VideoLatentPatchifier(1), frames, h, w, fps).create_initial_state(device=dev)
    n = st.latent.shape[1]
    st = st.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    ashape = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=frames, height=h, width=w, fps=fps))
    ast = AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=ashape).create_initial_state(
        initial_latent=torch.randn(1, 8, ashape.frames, 16, generator=g, device=dev))
    ast = ast.replace(denoise_mask=torch.zeros_like(ast.denoise_mask))
    na = ast.latent.shape[1]
    vctx, actx, nvctx, nactx = (0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev) for _ in range(4))
    sig = [float(s) for s in LTX2Scheduler().execute(steps=a.steps)]
    x0m, stepper = X0Model(m), EulerDiffusionStep()
    new = lambda graph: frozen_audio_guided_loop(x0m, st, ast, sig, vctx, actx, nvctx, nactx, 3.0, stepper, None, graph)          # noqa: E731
    ways = {
        "eager glue (existing)": lambda: joint_denoise_loop(x0m, True, st, ast, sig, vctx, actx, stepper, use_hip_graph=False, negative_video_context=nvctx,
                                                            negative_audio_context=nactx, video_guider=CFGGuider(3.0), audio_guider=CFGGuider(1.0)),
        "one guided_step_av_ call per step": lambda: new(False),
        "graph replay (capture included)": lambda: new(True),
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
    lat, alat = st.latent[0].clone(), ast.latent[0].float().contiguous()
    amask = ast.denoise_mask[0].reshape(-1).float().contiguous()
    m.prepare(vctx, st.positions, per_token=True, audio_context=actx, audio_positions=ast.positions)
    neg.prepare(nvctx, st.positions, per_token=True, audio_context=nactx, audio_positions=ast.positions)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.capture_guided_av_graph(neg, lat, alat, sig, 3.0, audio_denoise_mask=amask)
        m.replay_guided_av_graph()
        side.synchronize()
        replay = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            m.replay_guided_av_graph()
            side.synchronize()
            replay = min(replay, (time.perf_counter() - t0) / a.steps * 1e3)
    lines = [f"N = {n} video tokens + {na} frozen audio tokens, {a.layers} layers, full width, bf16, cfg 3, {a.steps} steps, best of {a.reps}", "",
             "| guided step, audio frozen | ms / step |", "|---|---|"]
    lines += [f"| {k} | {v:.2f} |" for k, v in best.items()]
    lines += [f"| graph replay alone | {replay:.2f} |"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
