"""fp32 restatement (torch, CPU) of the joint audio+video res_2s loop of the HQ pipeline (reference pipelines/ti2vid_hq.py:153-319) and the
two-modality stub denoiser of tests/golden/res2s_av_loop.npz.  Checker side only: nothing here is imported by the package."""
import math

import torch

from oracle import loop

import res2s_ref as R
from ltx_2_mlx_amd.components.res2s import get_res2s_coefficients


def _mean_tokens(x):
    """Mean over the token axis as sequential adds in a fixed order: (1, N, C) -> (1, 1, C)."""
    acc = x[:, 0:1]
    for k in range(1, x.shape[1]):
        acc = acc + x[:, k:k + 1]
    return acc * (1.0 / x.shape[1])


def _mix(x, w):
    acc = x[..., 0:1] * w[0]
    for k in range(1, w.shape[0]):
        acc = acc + x[..., k:k + 1] * w[k]
    return acc


def stub_x0_av(p, video_context, audio_context):
    """The stub AudioVideo denoiser of res2s_av_loop.npz: each modality's velocity is a tanh of a fixed linear map of its own latent, a map
    of the OTHER latent's token mean, its own context's mean and sigma times a bias.  Element-wise ops in a fixed order.
    p: dict with w_v (Cv, Cv), w_a (Ca, Ca), x_av (Ca, Cv: audio mean -> video), x_va (Cv, Ca), bias_v (Cv,), bias_a (Ca,).
    -> x0(video tokens (1, N, Cv), video timesteps (1, N, 1), audio tokens (1, Na, Ca), audio timesteps (1, Na, 1), sigma) -> (x0_v, x0_a)."""
    cv, ca = _mean_tokens(video_context), _mean_tokens(audio_context)

    def x0(xv, tsv, xa, tsa, sigma):
        s = torch.tensor([sigma], dtype=torch.float32)
        acc_v = cv + s * p["bias_v"] + _mix(_mean_tokens(xa), p["x_av"]) + _mix(xv, p["w_v"])
        acc_a = ca + s * p["bias_a"] + _mix(_mean_tokens(xv), p["x_va"]) + _mix(xa, p["w_a"])
        return xv - tsv * torch.tanh(acc_v), xa - tsa * torch.tanh(acc_a)
    return x0


def res2s_av_loop(video, audio, x0_pos, x0_neg, sigmas, cfg_scale, audio_cfg_scale, trace=None, callbacks=None):
    """The reference's joint loop in fp32.  video / audio: (tokens (1, N, C), mask (1, N, 1), clean (1, N, C)); x0_pos / x0_neg as
    stub_x0_av returns them (x0_neg None: no negative context).  trace receives (sigma, sigma_next, final) per executed step, callbacks
    (step, total) where the reference calls back.  -> (video tokens, audio tokens)."""
    n, sig = R.loop_sigmas(sigmas)
    guide = (cfg_scale > 1.0 or audio_cfg_scale > 1.0) and x0_neg is not None
    cache = {}
    (xv, vmask, vclean), (xa, amask, aclean) = video, audio
    xv, xa = xv.float(), xa.float()

    def denoised(xv, xa, s):
        tv, ta = loop.timesteps_from_mask(vmask, s), loop.timesteps_from_mask(amask, s)
        pv, pa = x0_pos(xv, tv, xa, ta, s)
        nv, na = x0_neg(xv, tv, xa, ta, s) if guide else (None, None)
        return R.guide_blend(pv, nv, vmask, vclean, cfg_scale), R.guide_blend(pa, na, amask, aclean, audio_cfg_scale)

    for i in range(n):
        s, sn = sig[i], sig[i + 1]
        h = -math.log(sn / s) if (s > 0 and sn > 0) else 0.0
        dv, da = denoised(xv, xa, s)
        final = h == 0.0 or sn <= 0.001
        if trace is not None:
            trace.append((s, sn, final))
        if final:
            xv, xa = dv, da
            break
        a21, b1, b2 = get_res2s_coefficients(h, cache, 0.5)
        n_bong = 100 if (h < 0.5 and s > 0.03) else 0
        mv, anv, ev = R.midpoint_from_d(xv, dv, h * a21, n_bong)
        ma, ana, ea = R.midpoint_from_d(xa, da, h * a21, n_bong)
        dv2, da2 = denoised(mv, ma, math.sqrt(s * sn))
        xv, xa = R.combine_from_d(dv2, anv, ev, h, b1, b2), R.combine_from_d(da2, ana, ea, h, b1, b2)
        if callbacks is not None:
            callbacks.append((i + 1, n))
    return xv, xa


def av_x0(w, cfg, video_positions, audio_positions, video_context, audio_context):
    """The x0 callable of res2s_av_loop over oracle.dit_av (fp32): both modalities carry Modality.sigma = the step's sigma."""
    from oracle import dit_av

    def f(xv, tsv, xa, tsa, sigma):
        sg = torch.tensor([sigma], dtype=torch.float32)
        video = dict(latent=xv, context=video_context, timesteps=tsv, sigma=sg, positions=video_positions)
        aud = dict(latent=xa, context=audio_context, timesteps=tsa, sigma=sg, positions=audio_positions)
        return dit_av.av_x0_model(video, aud, w, cfg)
    return f
