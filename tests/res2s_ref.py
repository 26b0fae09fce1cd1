"""fp32 restatement (torch, CPU) of what the res_2s feature computes: the two kernels element by element, the reference's loop with its sigma
handling, the stub denoiser of tests/golden/res2s_loop_tiny.npz and stage 1 of the HQ pipeline.  Checker side only: nothing here is
imported by the package."""
import math

import numpy as np
import torch

from oracle import loop

from ltx_2_mlx_amd.components.res2s import get_res2s_coefficients

f32 = lambda v: torch.tensor(np.float32(v))        # a host scalar as it meets an fp32 array


def guide_blend(p, n, mask, clean, cfg_scale):
    """The HQ pipeline's guidance on two x0 predictions (uncond + scale * (cond - uncond); n None: none) and post_process_latent."""
    g = p if n is None else n + f32(cfg_scale) * (p - n)
    if mask is None:
        return g
    m = mask.reshape(g.shape[0], -1, 1).float() if g.dim() == 3 else mask.reshape(-1, 1).float()
    return g * m + clean * (1 - m)


def midpoint_from_d(x, d, c, n_bong):
    """anchor = x, eps1 = d - anchor, x_mid = anchor + c*eps1, then the bong iteration -> (x_mid, anchor, eps1)."""
    c = f32(c)
    an = x
    e = d - an
    xm = an + c * e
    for _ in range(n_bong):
        an = xm - c * e
        e = d - an
    return xm, an, e


def combine_from_d(d2, anchor, eps1, h, b1, b2):
    return anchor + f32(h) * (f32(b1) * eps1 + f32(b2) * (d2 - anchor))


def _x0(x, v, ts):
    return x - ts.reshape(-1, 1).float() * v


def midpoint(x, vc, vu, ts, mask, clean, cfg_scale, c, n_bong, final=False):
    """ltx2_res2s_midpoint's sequence as separate fp32 torch ops.  x, vc, vu, clean: (rows, C); ts: (1,) or (rows,); mask: (rows,) or None.
    -> (x_mid, anchor, eps1); final: (d, None, None)."""
    d = guide_blend(_x0(x, vc, ts), None if vu is None else _x0(x, vu, ts), mask, clean, cfg_scale)
    return (d, None, None) if final else midpoint_from_d(x, d, c, n_bong)


def combine(x_mid, vc, vu, ts, mask, clean, cfg_scale, anchor, eps1, h, b1, b2):
    """ltx2_res2s_combine's sequence as separate fp32 torch ops."""
    d2 = guide_blend(_x0(x_mid, vc, ts), None if vu is None else _x0(x_mid, vu, ts), mask, clean, cfg_scale)
    return combine_from_d(d2, anchor, eps1, h, b1, b2)


def loop_sigmas(sigmas):
    """The reference's sigma handling (pipelines/ti2vid_hq.py:167-172): -> (number of steps, the list the steps read)."""
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    if sig[-1] == 0.0:
        sig = sig[:-1] + [0.0011, 0.0]
    return n, sig


def res2s_loop(tokens, mask, clean, x0_pos, x0_neg, sigmas, cfg_scale, audio_cfg_scale=7.0, trace=None):
    """The reference's res_2s loop (pipelines/ti2vid_hq.py:153-273, video branch) in fp32.  x0_pos / x0_neg(tokens, timesteps (B, N, 1),
    sigma) -> x0; x0_neg None: no negative context.  trace: a list that receives (sigma, sigma_next, final) per executed step."""
    n, sig = loop_sigmas(sigmas)
    guide = (cfg_scale > 1.0 or audio_cfg_scale > 1.0) and x0_neg is not None
    cache = {}
    x = tokens.float()

    def denoised(x, s):
        ts = loop.timesteps_from_mask(mask, s)
        return guide_blend(x0_pos(x, ts, s), x0_neg(x, ts, s) if guide else None, mask, clean, cfg_scale)

    for i in range(n):
        s, sn = sig[i], sig[i + 1]
        h = -math.log(sn / s) if (s > 0 and sn > 0) else 0.0
        d = denoised(x, s)
        final = h == 0.0 or sn <= 0.001
        if trace is not None:
            trace.append((s, sn, final))
        if final:
            x = d
            break
        a21, b1, b2 = get_res2s_coefficients(h, cache, 0.5)
        xm, an, e = midpoint_from_d(x, d, h * a21, 100 if (h < 0.5 and s > 0.03) else 0)
        x = combine_from_d(denoised(xm, math.sqrt(s * sn)), an, e, h, b1, b2)
    return x


def stub_x0(w, bias, context):
    """The stub denoiser of res2s_loop_tiny.npz: a fixed linear map of the latent plus terms in the context and sigma, through a tanh,
    as a velocity.  Written as separate element-wise ops in a fixed order so that it is the same function wherever it runs.
    w (C, C), bias (C,), context (1, S, C) -> x0(tokens (1, N, C), timesteps (1, N, 1), sigma)."""
    ctx = context[:, 0:1]
    for s in range(1, context.shape[1]):
        ctx = ctx + context[:, s:s + 1]
    ctx = ctx * (1.0 / context.shape[1])

    def x0(x, ts, sigma):
        acc = ctx + torch.tensor([sigma], dtype=torch.float32) * bias
        for k in range(w.shape[0]):
            acc = acc + x[..., k:k + 1] * w[k]
        return x - ts * torch.tanh(acc)
    return x0


def stage1(image_latents, frame_idx, strengths, grid, fps, noise, x0_pos, x0_neg, sigmas, cfg_scale):
    """TI2VidHQPipeline stage 1 with a supplied noise tensor: zero initial state of `grid` = (F, H, W) latent frames, each image latent
    (1, 128, 1, H, W) spliced over the tokens of its latent frame with mask 1 - strength, noised at scale 1, the res_2s loop,
    unpatchified -> (1, 128, F, H, W).  x0_*(tokens, timesteps, sigma, positions)."""
    f, h, w = grid
    n = f * h * w
    lat = torch.zeros(1, n, 128)
    clean, mask, pos = lat.clone(), torch.ones(1, n, 1), loop.video_positions(1, f, h, w, fps)
    for il, idx, st in zip(image_latents, frame_idx, strengths):
        tok = loop.patchify(il.float())
        a = idx * h * w
        lat[:, a:a + tok.shape[1]] = tok
        clean[:, a:a + tok.shape[1]] = tok
        mask[:, a:a + tok.shape[1]] = 1.0 - st
    x = loop.gaussian_noiser(lat, mask, noise, 1.0)
    x = res2s_loop(x, mask, clean, lambda t, ts, s: x0_pos(t, ts, s, pos), None if x0_neg is None else (lambda t, ts, s: x0_neg(t, ts, s, pos)),
                   sigmas, cfg_scale)
    return loop.unpatchify(x, f, h, w)
