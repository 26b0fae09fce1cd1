"""Generate tests/golden/res2s_coefficients.json and tests/golden/res2s_loop_tiny.npz by executing the REFERENCE'S OWN
get_res2s_coefficients (LTX_2_MLX/components/res2s.py) and TI2VidHQPipeline._res2s_denoise_loop (LTX_2_MLX/pipelines/ti2vid_hq.py)
through the mlx->torch shim (tools/mlx_shim.py), on the CPU in float32:

    python tools/pin_res2s_against_reference.py REFERENCE_DIR      (the directory that holds LTX_2_MLX/)

(a) coefficients: (a21, b1, b2) for h in 0, 1e-12, 0.05, 0.49, 0.5, 2.0 and the log(s_i / s_{i+1}) of a 15-step LTX2Scheduler table.
(b) loop: a 24 x 8 state whose denoise mask holds 0, 0.1 and 1, a stub transformer (tests/res2s_ref.stub_x0: a fixed linear map plus a
    tanh, stored in the file, the same function of (latent, context, sigma) for the positive and the negative context), cfg 3, over three
    sigma tables: a 4-step scheduler table ending in 0; one whose steps straddle both bong conditions (h < 0.5; sigma > 0.03); one ending
    at 0.0005 > 0, so the final-step branch runs.
Data only; no reference source travels.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_res2s_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
sys.path.insert(0, sys.argv[1])

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()

N, C, S = 24, 8, 4
CFG = 3.0
SEED = 31
BONG_TABLE = [0.9, 0.7, 0.2, 0.05, 0.035, 0.025, 0.02, 0.005]   # (h < 0.5, sigma > 0.03) per step: both, sigma only x2, both x2, h only, neither
FINAL_TABLE = [0.5, 0.1, 0.0005]                            # ends above 0: no injection, the last step takes the final-step branch


def coefficients():
    from LTX_2_MLX.components.res2s import get_res2s_coefficients
    from LTX_2_MLX.components.schedulers import LTX2Scheduler
    sig = [float(s) for s in LTX2Scheduler().execute(steps=15)]
    hs = [0.0, 1e-12, 0.05, 0.49, 0.5, 2.0] + [math.log(sig[i] / sig[i + 1]) for i in range(len(sig) - 2)]
    cache = {}
    rows = [dict(h=h, c2=0.5, coefficients=list(get_res2s_coefficients(h, cache, 0.5))) for h in hs]
    rows.append(dict(h=0.3, c2=0.25, coefficients=list(get_res2s_coefficients(0.3, {}, 0.25))))
    return dict(scheduler_sigmas_15=sig, rows=rows)


def loops():
    import res2s_ref as R
    from LTX_2_MLX.components.schedulers import LTX2Scheduler
    from LTX_2_MLX.pipelines.ti2vid_hq import TI2VidHQPipeline
    from LTX_2_MLX.types import LatentState
    g = torch.Generator().manual_seed(SEED)
    w = 0.5 * torch.randn(C, C, generator=g)
    bias = torch.randn(C, generator=g)
    ctx, nctx = torch.randn(1, S, C, generator=g), torch.randn(1, S, C, generator=g)
    latent, clean = torch.randn(1, N, C, generator=g), torch.randn(1, N, C, generator=g)
    mask = torch.ones(1, N, 1)
    mask[:, 0:8] = 0.0
    mask[:, 8:12] = 0.1
    x0_pos, x0_neg = R.stub_x0(w, bias, ctx), R.stub_x0(w, bias, nctx)

    def transformer(video_mod):        # stands where the reference's X0Model stands: Modality -> denoised
        c = shim._unwrap(video_mod.context)
        return shim._wrap((x0_neg if torch.equal(c, nctx) else x0_pos)(shim._unwrap(video_mod.latent), shim._unwrap(video_mod.timesteps), float(shim._unwrap(video_mod.sigma)[0])))

    pipe = TI2VidHQPipeline.__new__(TI2VidHQPipeline)
    pipe.transformer, pipe.is_av_model = transformer, False
    tables = dict(scheduler=[float(s) for s in LTX2Scheduler().execute(steps=4)], bong=BONG_TABLE, final=FINAL_TABLE)
    out = dict(w=w.numpy(), bias=bias.numpy(), context=ctx.numpy(), negative_context=nctx.numpy(), latent=latent.numpy(), clean=clean.numpy(),
               mask=mask.numpy(), cfg_scale=np.float64(CFG))
    for name, sig in tables.items():
        state = LatentState(latent=shim._wrap(latent.clone()), denoise_mask=shim._wrap(mask), positions=shim._wrap(torch.zeros(1, 3, N, 2)),
                            clean_latent=shim._wrap(clean))
        calls = []
        res, _ = pipe._res2s_denoise_loop(state, None, sig, shim._wrap(ctx), None,
                                          shim._wrap(nctx), None, CFG, 7.0, callback=lambda i, n: calls.append((i, n)))
        out[f"sigmas_{name}"] = np.array(sig, dtype=np.float64)
        out[f"result_{name}"] = shim._unwrap(res.latent).float().numpy()
        out[f"callbacks_{name}"] = np.array(calls, dtype=np.int64).reshape(-1, 2)
    return out


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "res2s_coefficients.json"), "w") as f:
        json.dump(coefficients(), f, indent=1)
    arrays = loops()
    np.savez(os.path.join(gold, "res2s_loop_tiny.npz"), **arrays)
    for k in sorted(arrays):
        if k.startswith("result_"):
            print(k, arrays[k].shape, arrays[k].dtype, "callbacks", arrays["callbacks_" + k[7:]].tolist(), "finite", bool(np.isfinite(arrays[k]).all()))


if __name__ == "__main__":
    main()
