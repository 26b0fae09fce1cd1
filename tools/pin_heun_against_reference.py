"""Generate tests/golden/heun_ge.npz by executing the REFERENCE'S OWN HeunDiffusionStep.step (LTX_2_MLX/components/diffusion_steps.py) and
OneStagePipeline._denoise_loop_heun / _denoise_loop_cfg (LTX_2_MLX/pipelines/one_stage.py) through the mlx->torch shim (tools/mlx_shim.py), on
the CPU in float32:

    python tools/pin_heun_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

(a) step: a 6 x 8 sample and two x0 predictions of the closed-form denoiser tests/heun_ref.closed_form_x0 (its w and bias stored in the file):
    the step without denoised_at_predicted, with it, and with sigma_next = 0.
(b) loops: a 12 x 8 state whose denoise mask holds 0, 0.1 and 1, that denoiser as the transformer (the negative context scales its bias),
    CFGGuider at 3, a 4-step LTX2Scheduler table, ge_gamma = 2: _denoise_loop_heun without GE, _denoise_loop_heun with it, _denoise_loop_cfg
    with it.
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
    sys.exit("usage: python tools/pin_heun_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

N, C = 12, 8
CFG, GAMMA, SEED = 3.0, 2.0, 47
NEG_BIAS = -0.5          # the negative context's denoiser: the same w, bias * NEG_BIAS


def main():
    import heun_ref as R
    from LTX_2_MLX.components.diffusion_steps import EulerDiffusionStep, HeunDiffusionStep
    from LTX_2_MLX.components.guiders import CFGGuider
    from LTX_2_MLX.components.schedulers import LTX2Scheduler
    from LTX_2_MLX.pipelines.one_stage import OneStagePipeline
    from LTX_2_MLX.types import LatentState
    g = torch.Generator().manual_seed(SEED)
    w, bias = 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    x0_pos, x0_neg = R.closed_form_x0(w, bias), R.closed_form_x0(w, bias * NEG_BIAS)
    out = dict(w=w.numpy(), bias=bias.numpy(), neg_bias=np.float64(NEG_BIAS), cfg_scale=np.float64(CFG), ge_gamma=np.float64(GAMMA))

    # (a) the step
    sample = torch.randn(6, C, generator=g)
    sig3 = [0.8, 0.5, 0.0]
    one = lambda s: torch.full((6, 1), s)        # noqa: E731
    d1 = x0_pos(sample, one(sig3[0]), sig3[0])
    step = HeunDiffusionStep()
    pred = shim._unwrap(step.step(shim._wrap(sample), shim._wrap(d1), shim._wrap(torch.tensor(sig3)), 0))
    d2 = x0_pos(pred, one(sig3[1]), sig3[1])
    full = shim._unwrap(step.step(shim._wrap(sample), shim._wrap(d1), shim._wrap(torch.tensor(sig3)), 0, denoised_at_predicted=shim._wrap(d2)))
    d_last = x0_pos(sample, one(sig3[1]), sig3[1])
    last = shim._unwrap(step.step(shim._wrap(sample), shim._wrap(d_last), shim._wrap(torch.tensor(sig3)), 1))
    out.update(step_sigmas=np.array(sig3, np.float64), step_sample=sample.numpy(), step_denoised=d1.numpy(), step_predicted=pred.float().numpy(),
               step_denoised_at_predicted=d2.numpy(), step_result=full.float().numpy(), step_denoised_last=d_last.numpy(),
               step_result_to_zero=last.float().numpy())

    # (b) the loops
    latent, clean = torch.randn(1, N, C, generator=g), torch.randn(1, N, C, generator=g)
    mask = torch.ones(1, N, 1)
    mask[:, 0:4] = 0.0
    mask[:, 4:6] = 0.1
    ctx, nctx = torch.zeros(1, 1, C), torch.ones(1, 1, C)        # only tell the two denoisers apart

    def transformer(video_mod, **_):        # stands where the reference's X0Model stands: Modality -> denoised
        fn = x0_neg if bool(shim._unwrap(video_mod.context).any()) else x0_pos
        sigma = float(shim._unwrap(video_mod.sigma).reshape(-1)[0]) if getattr(video_mod, "sigma", None) is not None else \
            float(shim._unwrap(video_mod.timesteps).max())
        return shim._wrap(fn(shim._unwrap(video_mod.latent), shim._unwrap(video_mod.timesteps), sigma))

    pipe = OneStagePipeline.__new__(OneStagePipeline)
    pipe.transformer = transformer
    sig = LTX2Scheduler().execute(steps=4)
    state = lambda: LatentState(latent=shim._wrap(latent.clone()), denoise_mask=shim._wrap(mask), positions=shim._wrap(torch.zeros(1, 3, N, 2)),      # noqa: E731
                                clean_latent=shim._wrap(clean))
    common = dict(sigmas=sig, positive_context=shim._wrap(ctx), negative_context=shim._wrap(nctx), guider=CFGGuider(scale=CFG))
    runs = dict(heun=pipe._denoise_loop_heun(video_state=state(), stepper=HeunDiffusionStep(), **common),
                heun_ge=pipe._denoise_loop_heun(video_state=state(), stepper=HeunDiffusionStep(), ge_gamma=GAMMA, **common),
                euler_ge=pipe._denoise_loop_cfg(video_state=state(), stepper=EulerDiffusionStep(), ge_gamma=GAMMA, **common))
    out.update(latent=latent.numpy(), clean=clean.numpy(), mask=mask.numpy(), sigmas=np.array([float(s) for s in sig], np.float64))
    for name, res in runs.items():
        out["result_" + name] = shim._unwrap(res.latent).float().numpy()
    np.savez(os.path.join(ROOT, "tests", "golden", "heun_ge.npz"), **out)
    for k in sorted(out):
        if k.startswith(("result_", "step_result", "step_predicted")):
            print(k, out[k].shape, out[k].dtype, "finite", bool(np.isfinite(out[k]).all()), float(np.abs(out[k]).mean()))


if __name__ == "__main__":
    main()
