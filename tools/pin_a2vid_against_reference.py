"""Generate tests/golden/a2vid_loop.npz by executing the REFERENCE'S OWN A2VidPipelineTwoStage._video_only_denoise_loop
(LTX_2_MLX/pipelines/a2vid_two_stage.py:225-271, with its modality_from_state, post_process_latent and EulerDiffusionStep) through the
mlx->torch shim (tools/mlx_shim.py), over a toy callable transformer (tests/a2vid_ref.toy_x0_video):

    python tools/pin_a2vid_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

State: 6 video tokens x 8 channels (the first two conditioned: mask 0 and 0.25), 4 frozen audio tokens, 3 steps.  Three runs: cfg 3 with
negative_audio_context None (the loop falls back to audio_context), cfg 1 with both negative contexts (no second evaluation), cfg 3 without a
negative video context (none either).  A fourth, cfg 3 WITH a negative audio context, cannot be recorded: the reference writes
`negative_audio_context or audio_context`, and the truth value of an array with more than one element raises, in MLX as in the shim; the
tool checks that it does.  Stored: the seeded inputs, each run's video latent, the audio latent the loop returned and the callback's
reports.  Data only; no reference source travels.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_a2vid_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

N, NA, C, S = 6, 4, 8, 5
SIGMAS = (1.0, 0.75, 0.4, 0.0)
SEED = 23
RUNS = {"cfg3_no_negative_audio": (3.0, True, False), "cfg1": (1.0, True, True), "cfg3_no_negative": (3.0, False, False)}


def main():
    import a2vid_ref as R
    from LTX_2_MLX.components import EulerDiffusionStep
    from LTX_2_MLX.pipelines.a2vid_two_stage import A2VidPipelineTwoStage
    from LTX_2_MLX.types import LatentState
    g = torch.Generator().manual_seed(SEED)
    lat, clean, audio = torch.randn(1, N, C, generator=g), torch.randn(1, N, C, generator=g), torch.randn(1, NA, C, generator=g)
    mask = torch.ones(1, N, 1)
    mask[0, 0, 0], mask[0, 1, 0] = 0.0, 0.25
    vctx, actx, nvctx, nactx = (torch.randn(1, S, C, generator=g) for _ in range(4))
    A = shim.Arr
    t = lambda a: a.t.detach().float()          # noqa: E731

    def transformer(video, audio_mod):
        x0 = R.toy_x0_video(t(video.latent), t(video.timesteps), t(video.context), t(audio_mod.latent), t(audio_mod.timesteps), t(audio_mod.context),
                            float(t(video.sigma)[0]))
        assert float(t(audio_mod.sigma)[0]) == float(t(video.sigma)[0])
        return A(x0), A(t(audio_mod.latent) - t(audio_mod.timesteps) * 7.0)      # the audio x0 is never used by the loop

    pipe = A2VidPipelineTwoStage.__new__(A2VidPipelineTwoStage)                  # the loop reads the transformer and the stepper only
    pipe.transformer, pipe.stepper = transformer, EulerDiffusionStep()

    def states():
        return (LatentState(latent=A(lat.clone()), denoise_mask=A(mask.clone()), positions=A(torch.zeros(1, 3, N, 2)), clean_latent=A(clean.clone())),
                LatentState(latent=A(audio.clone()), denoise_mask=A(torch.zeros(1, NA, 1)), positions=A(torch.zeros(1, 1, NA, 2)), clean_latent=A(audio.clone())))

    try:
        pipe._video_only_denoise_loop(*states(), mx.array(list(SIGMAS)), A(vctx), A(actx), A(nvctx), A(nactx), cfg_scale=3.0)
        sys.exit("the reference's loop took a negative audio context: record that run as well")
    except RuntimeError as e:
        print(f"cfg 3 with a negative audio context raises in the reference: {e}")
    out = dict(latent=lat.numpy(), clean_latent=clean.numpy(), denoise_mask=mask.numpy(), audio=audio.numpy(), sigmas=np.array(SIGMAS, np.float64),
               video_context=vctx.numpy(), audio_context=actx.numpy(), negative_video_context=nvctx.numpy(), negative_audio_context=nactx.numpy())
    for name, (scale, neg_v, neg_a) in RUNS.items():
        vstate, astate = states()
        seen = []
        v, a = pipe._video_only_denoise_loop(vstate, astate, mx.array(list(SIGMAS)), A(vctx), A(actx), A(nvctx) if neg_v else None,
                                             A(nactx) if neg_a else None, cfg_scale=scale, callback=lambda i, n: seen.append((i, n)))
        out[name + "_video"], out[name + "_audio"], out[name + "_callback"] = t(v.latent).numpy(), t(a.latent).numpy(), np.array(seen, np.int64)
    path = os.path.join(ROOT, "tests", "golden", "a2vid_loop.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, runs {list(RUNS)}")


if __name__ == "__main__":
    main()
