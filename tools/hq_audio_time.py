"""The HQ pipeline's joint audio+video stage-1 loop at its default geometry (1088x1920x97 -> stage 1 at 544x960: N = 13 * 17 * 30 = 6630 video
tokens, 97 audio tokens; AudioVideo model, full width, 48 layers, bf16, random weights): ms per guided res_2s step two ways, alternated --
  eager pieces  the step composed from existing public entries: four forward_av calls (two contexts x two evaluations) and four
                single-modality kernel calls (res2s_midpoint and res2s_combine, once per modality)
  one call      LTXModel.res2s_step_av_ per step (ltx2_dit_res2s_step_av: the pair kernels, one launch per pass)
The eager pieces against one call is what the single launch per pass (and the one C call) saves.

    python tools/hq_audio_time.py [--steps 4] [--reps 3] [--layers 48] [out.md]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.components import LTX2Scheduler, VideoLatentPatchifier, get_res2s_coefficients  # noqa: E402
from ltx_2_mlx_amd.components.patchifiers import AudioPatchifier  # noqa: E402
from ltx_2_mlx_amd.conditioning.tools import AudioLatentTools  # noqa: E402
from ltx_2_mlx_amd.model.transformer import LTXModel, LTXModelType, X0Model  # noqa: E402
from ltx_2_mlx_amd.pipelines.common import audio_modality_from_state, modality_from_state, res2s_av_denoise_loop, video_tools_for  # noqa: E402
from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape  # noqa: E402

CFG, ACFG = 3.0, 7.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=48)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = LTXModel(model_type=LTXModelType.AudioVideo, num_layers=a.layers, device=dev)
    m.init_random_weights(seed=0)
    neg = m.clone_sharing_weights()
    g = torch.Generator(device=dev).manual_seed(3)
    frames, h, w, fps = 97, 544, 960, 25.0
    st = video_tools_for(VideoLatentPatchifier(1), frames, h, w, fps).create_initial_state(device=dev)
    n = st.latent.shape[1]
    st = st.replace(latent=torch.randn(1, n, 128, generator=g, device=dev))
    ashape = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=frames, height=h, width=w, fps=fps))
    ast = AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=ashape).create_initial_state(
        initial_latent=torch.randn(1, 8, ashape.frames, 16, generator=g, device=dev))
    na = ast.latent.shape[1]
    vctx, actx, nvctx, nactx = (0.1 * torch.randn(1, 1024, 3840, generator=g, device=dev) for _ in range(4))
    sig = torch.tensor([float(s) for s in LTX2Scheduler().execute(steps=a.steps)][:-1] + [0.0011], dtype=torch.float32).tolist()
    x0m = X0Model(m)

    def pieces():
        lat, alat = st.latent[0].clone(), ast.latent[0].float().clone()
        for i in range(a.steps):
            s, sn = sig[i], sig[i + 1]
            hh = -math.log(sn / s)
            a21, b1, b2 = get_res2s_coefficients(hh, {})
            nb = 100 if (hh < 0.5 and s > 0.03) else 0
            sub = float(np.float32(math.sqrt(s * sn)))
            ts = torch.tensor([s], device=dev)

            def vel(x, xa, sg):
                mods = lambda vc, ac: (modality_from_state(st.replace(latent=x[None]), vc, sg, uniform=True),          # noqa: E731
                                       audio_modality_from_state(ast.replace(latent=xa[None]), ac, sg, uniform=True))
                pv, pa = m(*mods(vctx, actx))
                uv, ua = neg(*mods(nvctx, nactx))
                return pv[0], pa[0], uv[0], ua[0]

            pv, pa, uv, ua = (t.clone() for t in vel(lat, alat, s))
            xm, an, e = K.res2s_midpoint(lat, pv, uv, ts, CFG, hh * a21, nb)
            xma, ana, ea = K.res2s_midpoint(alat, pa, ua, ts, ACFG, hh * a21, nb)
            pv, pa, uv, ua = vel(xm, xma, sub)
            tsub = torch.tensor([sub], device=dev)
            K.res2s_combine(xm, pv, uv, tsub, CFG, an, e, hh, b1, b2, out=lat)
            K.res2s_combine(xma, pa, ua, tsub, ACFG, ana, ea, hh, b1, b2, out=alat)
        return lat, alat

    ways = {"eager pieces (4 forward_av + 4 single-modality kernel calls)": pieces,
            "one res2s_step_av_ call per step": lambda: res2s_av_denoise_loop(x0m, st, ast, sig, vctx, actx, nvctx, nactx, CFG, ACFG)}
    best = {k: float("inf") for k in ways}
    for rep in range(a.reps + 1):                   # the first round warms up (allocation, the per-prompt setup); alternated afterwards
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                best[name] = min(best[name], (time.perf_counter() - t0) / a.steps * 1e3)
    names = list(best)
    lines = [f"N = {n} video tokens + {na} audio tokens, {a.layers} layers, full width, bf16, cfg {CFG:g} / audio cfg {ACFG:g}, {a.steps} steps, best of {a.reps}",
             "", "| joint res_2s step | ms / step |", "|---|---|"]
    lines += [f"| {k} | {v:.2f} |" for k, v in best.items()]
    lines += ["",
              f"One call against the eager pieces: {best[names[0]] - best[names[1]]:+.2f} ms / step "
              f"({(best[names[0]] - best[names[1]]) / best[names[0]] * 100:+.2f} %), as measured; a step is four AudioVideo evaluations, so the two launches "
              "saved are a small part of it."]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
