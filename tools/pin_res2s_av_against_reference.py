"""Generate tests/golden/res2s_av_loop.npz by executing the REFERENCE'S OWN TI2VidHQPipeline._res2s_denoise_loop
(LTX_2_MLX/pipelines/ti2vid_hq.py:153-319) with a video AND an audio state, through the mlx->torch shim (tools/mlx_shim.py), on the CPU in float32:

    python tools/pin_res2s_av_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

A 12 x 8 video state whose denoise mask holds 0, 0.1 and 1 and a 5 x 6 audio state with an all-ones mask; a stub two-modality transformer
(tests/hq_audio_ref.stub_x0_av, its parameters stored in the file: each modality's output depends on both latents, its own context and
sigma); cfg_scale 3 on the video and audio_cfg_scale 7 on the audio; two sigma tables (a 4-step scheduler table ending in 0, and one ending
at 0.0005 > 0, so the final-step branch runs), each with guidance on and, without a negative context, off.
Data only; no reference source travels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_res2s_av_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

N, CV, NA, CA, S = 12, 8, 5, 6, 4
CFG, AUDIO_CFG = 3.0, 7.0
SEED = 57
FINAL_TABLE = [0.5, 0.1, 0.0005]                            # ends above 0: no injection, the last step takes the final-step branch


def loops():
    import hq_audio_ref as R
    from LTX_2_MLX.components.schedulers import LTX2Scheduler
    from LTX_2_MLX.pipelines.ti2vid_hq import TI2VidHQPipeline
    from LTX_2_MLX.types import LatentState
    g = torch.Generator().manual_seed(SEED)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    p = dict(w_v=0.5 * r(CV, CV), w_a=0.5 * r(CA, CA), x_av=0.5 * r(CA, CV), x_va=0.5 * r(CV, CA), bias_v=r(CV), bias_a=r(CA))
    vctx, nvctx, actx, nactx = r(1, S, CV), r(1, S, CV), r(1, S, CA), r(1, S, CA)
    vlat, vclean, alat = r(1, N, CV), r(1, N, CV), r(1, NA, CA)
    vmask = torch.ones(1, N, 1)
    vmask[:, 0:4] = 0.0
    vmask[:, 4:6] = 0.1
    amask = torch.ones(1, NA, 1)
    x0_pos, x0_neg = R.stub_x0_av(p, vctx, actx), R.stub_x0_av(p, nvctx, nactx)
    u = shim._unwrap

    def transformer(video_mod, audio_mod):        # stands where the reference's X0Model stands: two Modalities -> two denoised arrays
        neg = torch.equal(u(video_mod.context), nvctx)
        assert torch.equal(u(audio_mod.context), nactx if neg else actx)
        s, sa = float(u(video_mod.sigma)[0]), float(u(audio_mod.sigma)[0])
        assert s == sa
        v, a = (x0_neg if neg else x0_pos)(u(video_mod.latent), u(video_mod.timesteps), u(audio_mod.latent), u(audio_mod.timesteps), s)
        return shim._wrap(v), shim._wrap(a)

    pipe = TI2VidHQPipeline.__new__(TI2VidHQPipeline)
    pipe.transformer, pipe.is_av_model = transformer, True
    tables = dict(scheduler=[float(s) for s in LTX2Scheduler().execute(steps=4)], final=FINAL_TABLE)
    out = {k: v.numpy() for k, v in p.items()}
    out.update(video_context=vctx.numpy(), negative_video_context=nvctx.numpy(), audio_context=actx.numpy(), negative_audio_context=nactx.numpy(),
               video_latent=vlat.numpy(), video_clean=vclean.numpy(), video_mask=vmask.numpy(), audio_latent=alat.numpy(), audio_mask=amask.numpy(),
               cfg_scale=np.float64(CFG), audio_cfg_scale=np.float64(AUDIO_CFG))
    w = shim._wrap
    for name, sig in tables.items():
        for guided in (True, False):
            vs = LatentState(latent=w(vlat.clone()), denoise_mask=w(vmask), positions=w(torch.zeros(1, 3, N, 2)), clean_latent=w(vclean))
            as_ = LatentState(latent=w(alat.clone()), denoise_mask=w(amask), positions=w(torch.zeros(1, 1, NA, 2)), clean_latent=w(alat.clone()))
            calls = []
            rv, ra = pipe._res2s_denoise_loop(vs, as_, sig, w(vctx), w(actx), w(nvctx) if guided else None, w(nactx) if guided else None, CFG, AUDIO_CFG,
                                              callback=lambda i, n: calls.append((i, n)))
            tag = f"{name}_{'guided' if guided else 'plain'}"
            out[f"sigmas_{name}"] = np.array(sig, dtype=np.float64)
            out[f"video_{tag}"] = u(rv.latent).float().numpy()
            out[f"audio_{tag}"] = u(ra.latent).float().numpy()
            out[f"callbacks_{tag}"] = np.array(calls, dtype=np.int64).reshape(-1, 2)
    return out


def main():
    arrays = loops()
    path = os.path.join(ROOT, "tests", "golden", "res2s_av_loop.npz")
    np.savez(path, **arrays)
    for k in sorted(arrays):
        if k.startswith(("video_s", "video_f", "audio_s", "audio_f")):
            print(k, arrays[k].shape, arrays[k].dtype, "finite", bool(np.isfinite(arrays[k]).all()))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
