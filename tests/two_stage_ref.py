"""fp32 restatement (torch / numpy, CPU) of the two-stage pipeline's guidance (reference components/guiders.py:244-273, pipelines/two_stage.py:314-401):
MultiModalGuider.calculate and the step kernels' element-wise sequence as separate fp32 torch ops, the rescale factor in float64, the stage-1 loop
over any x0 callables, the modality-isolated pass as oracle.dit_av on weights whose cross-modal out-projections are zero, and the two-stage
composition.  Checker side only: nothing here is imported by the package."""
import math

import numpy as np
import torch

from oracle import loop

f32 = np.float32


def x0(x, v, ts):
    """x - t*v as the kernels form it; None stays None.  x, v: (rows, C); ts: (1,) or (rows,)."""
    return None if v is None else x - ts.reshape(-1, 1).float() * v


def calculate(a, u, p, m, cfg_scale, stg_scale, modality_scale):
    """MultiModalGuider.calculate without rescale on x0 predictions, every operation a separate fp32 op, the scale differences formed in fp32
    (the engine's scalar type).  u / p / m None: that pass did not run."""
    pred = a
    if u is not None:
        pred = pred + torch.tensor(f32(cfg_scale) - f32(1.0)) * (a - u)
    if p is not None:
        pred = pred + torch.tensor(f32(stg_scale)) * (a - p)
    if m is not None:
        pred = pred + torch.tensor(f32(modality_scale) - f32(1.0)) * (a - m)
    return pred


def sums_f64(a, pred):
    """(S_a, S_aa, S_p, S_pp) in float64 from the fp32 tensors."""
    a, pred = a.double(), pred.double()
    return float(a.sum()), float((a * a).sum()), float(pred.sum()), float((pred * pred).sum())


def rescale_factor_f64(s, n, rescale_scale):
    """f = rescale*sqrt((var_a + 1e-8)/(var_p + 1e-8)) + (1 - rescale) in float64 from the four sums, var = (S2 - S1^2/n)/n (mx.var);
    rescale is the fp32 value the engine holds."""
    r = float(f32(rescale_scale))
    var_a, var_p = (s[1] - s[0] * s[0] / n) / n, (s[3] - s[2] * s[2] / n) / n
    return r * math.sqrt((var_a + 1e-8) / (var_p + 1e-8)) + (1.0 - r)


def ulps(got: float, want: float) -> float:
    """|got - fp32(want)| in units of the fp32 spacing at want."""
    w = f32(want)
    return abs(float(f32(got)) - float(w)) / float(np.spacing(np.abs(w)))


def mm_step(x, pred, mask, clean, sigma, sigma_next, f=None):
    """The step kernels' tail as separate fp32 ops: [pred*f], the mask / clean blend, Euler with 1/sigma and sigma_next - sigma formed in fp32."""
    if sigma == 0:
        raise ValueError("Sigma can't be 0.0")
    if f is not None:
        pred = pred * torch.tensor(f32(f))
    if mask is not None:
        mk = mask.reshape(-1, 1).float()
        pred = pred * mk + clean * (1 - mk)
    return x + ((x - pred) * torch.tensor(f32(1.0) / f32(sigma))) * torch.tensor(f32(sigma_next) - f32(sigma))


def zero_cross_modal(w):
    """The weights with every block's audio_to_video_attn.to_out and video_to_audio_attn.to_out (weight and bias) zeroed: on them the plain
    AudioVideo forward IS the modality-isolated pass (each cross-modal attention adds gate * 0 to its residual stream)."""
    out = dict(w)
    for k, v in w.items():
        if ".audio_to_video_attn.to_out." in k or ".video_to_audio_attn.to_out." in k:
            out[k] = torch.zeros_like(v)
    assert sum(o is not w[k] for k, o in out.items()) > 0
    return out


def guide(params, cond, unc, ptb, mod):
    """calculate with one modality's MultiModalGuiderParams-like object, the rescale factor in float64 rounded once to fp32."""
    pred = calculate(cond, unc, ptb, mod, params.cfg_scale, params.stg_scale, params.modality_scale)
    if params.rescale_scale != 0:
        pred = pred * torch.tensor(f32(rescale_factor_f64(sums_f64(cond, pred), cond.numel(), params.rescale_scale)))
    return pred


def stage1_loop(video, audio, x0_pos, x0_neg, x0_iso, sigmas, video_params, audio_params):
    """The reference's _denoise_loop_cfg_av in fp32.  video / audio: (tokens (1, N, C), mask (1, N, 1), clean (1, N, C)); x0_pos / x0_neg /
    x0_iso: callables (video tokens, video timesteps, audio tokens, audio timesteps, sigma) -> (x0_v, x0_a), None: the pass does not run
    (its term is left out of both modalities).  -> (video tokens, audio tokens)."""
    (xv, vmask, vclean), (xa, amask, aclean) = video, audio
    xv, xa = xv.float(), xa.float()
    sig = [float(s) for s in sigmas]
    for i in range(len(sig) - 1):
        s = sig[i]
        tv, ta = loop.timesteps_from_mask(vmask, s), loop.timesteps_from_mask(amask, s)
        cond = x0_pos(xv, tv, xa, ta, s)
        unc = x0_neg(xv, tv, xa, ta, s) if x0_neg is not None else (None, None)
        mod = x0_iso(xv, tv, xa, ta, s) if x0_iso is not None else (None, None)
        dv = loop.post_process_latent(guide(video_params, cond[0], unc[0], None, mod[0]), vmask, vclean)
        da = loop.post_process_latent(guide(audio_params, cond[1], unc[1], None, mod[1]), amask, aclean)
        xv, xa = loop.euler_step(xv, dv, s, sig[i + 1]), loop.euler_step(xa, da, s, sig[i + 1])
    return xv, xa


def plain_loop(video, audio, x0_pos, sigmas):
    """Stage 2: the joint loop without guidance (reference _denoise_loop_simple_av) in fp32, all tokens free."""
    xv, xa = video.float(), audio.float()
    ones_v, ones_a = torch.ones(1, xv.shape[1], 1), torch.ones(1, xa.shape[1], 1)
    sig = [float(s) for s in sigmas]
    for i in range(len(sig) - 1):
        dv, da = x0_pos(xv, ones_v * sig[i], xa, ones_a * sig[i], sig[i])
        xv, xa = loop.euler_step(xv, dv, sig[i], sig[i + 1]), loop.euler_step(xa, da, sig[i], sig[i + 1])
    return xv, xa


def av_x0(w, cfg, video_positions, audio_positions, video_context, audio_context):
    """An x0 callable of stage1_loop over oracle.dit_av (fp32): both modalities carry Modality.sigma = the step's sigma."""
    from oracle import dit_av

    def f(xv, tsv, xa, tsa, sigma):
        sg = torch.tensor([sigma], dtype=torch.float32)
        video = dict(latent=xv, context=video_context, timesteps=tsv, sigma=sg, positions=video_positions)
        aud = dict(latent=xa, context=audio_context, timesteps=tsa, sigma=sg, positions=audio_positions)
        return dit_av.av_x0_model(video, aud, w, cfg)
    return f


def two_stage(noises, x0s_stage1, x0_stage2, sigmas1, sigmas2, video_params, audio_params, upscale, grid):
    """The two-stage composition over x0 callables: stage 1 from pure noise (noise_scale 1), `upscale` on the unpatchified video latent
    (the package's un-normalise -> upscaler -> normalise, a component with tests of its own), both latents re-noised at sigmas2[0] and the plain
    joint loop.  noises: (video 1, audio 1, video 2, audio 2) patchified; x0s_stage1: (pos, neg, iso) at stage 1's positions, x0_stage2 at stage
    2's; grid: (f, h, w) of stage 1.  -> (final video tokens, final audio tokens, stage-1 video tokens, stage-1 audio tokens)."""
    n1, a1, n2, a2 = noises
    ones = lambda t: torch.ones(1, t.shape[1], 1)      # noqa: E731
    v1, au1 = stage1_loop((n1, ones(n1), n1), (a1, ones(a1), a1), *x0s_stage1, sigmas1, video_params, audio_params)
    up = loop.patchify(upscale(loop.unpatchify(v1, *grid)))
    s0 = float(sigmas2[0])
    v2, au2 = plain_loop(n2 * s0 + up * (1 - s0), a2 * s0 + au1 * (1 - s0), x0_stage2, sigmas2)
    return v2, au2, v1, au1
