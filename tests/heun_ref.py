"""fp32 restatement (torch) of what the Heun / GE feature computes: the kernels element by element as separate, individually rounded ops, and
the reference's Heun and Euler + GE loops (pipelines/one_stage.py:224-330, 334-464, 466-568, 570-729) over a denoiser passed in as a function.
Checker side only: nothing here is imported by the package."""
import numpy as np
import torch

from oracle import loop

f = np.float32
f32 = lambda v: torch.tensor(np.float32(v))        # noqa: E731  a host scalar as it meets an fp32 array


def _guided(x, vc, vu, ts, cfg_scale):
    t = ts.reshape(-1, 1).float()
    a = x - t * vc
    return a if vu is None else a + f32(f(cfg_scale) - f(1.0)) * (a - (x - t * vu))


def _blend(g, mask, clean):
    if mask is None:
        return g
    m = mask.reshape(-1, 1).float()
    return g * m + clean * (1 - m)


def heun_predict(x, vc, vu, ts, mask, clean, cfg_scale, sigma, sigma_next, ge_gamma=0.0, prev=None, first=True):
    """ltx2_heun_predict's sequence; the scalars formed in numpy float32 as the host code forms them.  x, vc, vu, clean, prev: (rows, C);
    ts: (1,) or (rows,); mask: (rows,) or None.  -> (d, xp, the new prev or None)."""
    inv, dt = f32(f(1.0) / f(sigma)), f32(f(sigma_next) - f(sigma))
    g = _guided(x, vc, vu, ts, cfg_scale)
    cur = None
    if ge_gamma > 0:
        cur = (x - g) * inv
        if not first:
            g = x - (f32(ge_gamma) * (cur - prev) + prev) * f32(sigma)
    d = _blend(g, mask, clean)
    return d, x + ((x - d) * inv) * dt, cur


def heun_correct(x, d, xp, vc, vu, ts, mask, clean, cfg_scale, sigma, sigma_next):
    """ltx2_heun_correct's sequence."""
    inv, inv_next, dt = f32(f(1.0) / f(sigma)), f32(f(1.0) / f(sigma_next)), f32(f(sigma_next) - f(sigma))
    d2 = _blend(_guided(xp, vc, vu, ts, cfg_scale), mask, clean)
    return x + (f32(0.5) * ((x - d) * inv + (xp - d2) * inv_next)) * dt


def sample_loop(heun, mods, x0_pos, x0_neg, sigmas, ge_gamma=0.0, trace=None):
    """The reference's loops in fp32, its statements one by one.  mods: one dict per modality (the video first) with tokens (B, N, C), mask
    (B, N, 1), clean and cfg_scale; x0_pos / x0_neg(list of tokens, list of timesteps (B, N, 1), sigma) -> list of x0 (x0_neg None: no
    guidance).  heun False: the Euler loop.  GE acts on the first modality alone.  trace: a list that receives per step the video's
    (uncorrected velocity, blended x0).  -> the list of final latents."""
    xs = [m["tokens"] if m["tokens"].dtype == torch.float64 else m["tokens"].float() for m in mods]          # fp64 only where the caller asks for it
    prev = None

    def denoised(xs, s):
        ts = [loop.timesteps_from_mask(m["mask"], s) for m in mods]
        p = x0_pos(xs, ts, s)
        if x0_neg is None:
            return list(p)
        n = x0_neg(xs, ts, s)
        return [a + (m["cfg_scale"] - 1) * (a - b) for m, a, b in zip(mods, p, n)]

    blend = lambda ds: [loop.post_process_latent(d, m["mask"], m["clean"]) for d, m in zip(ds, mods)]       # noqa: E731
    for i in range(len(sigmas) - 1):
        s, sn = float(sigmas[i]), float(sigmas[i + 1])
        dt = sn - s
        d = denoised(xs, s)
        cur = None
        if ge_gamma > 0 and s > 0:
            cur = (xs[0] - d[0]) / s
            if prev is not None:
                d[0] = xs[0] - (ge_gamma * (cur - prev) + prev) * s
            prev = cur
        d = blend(d)
        if trace is not None:
            trace.append((cur, d[0]))
        v1 = [(x - x0) / s for x, x0 in zip(xs, d)]
        xp = [x + v * dt for x, v in zip(xs, v1)]
        if not heun:
            xs = xp
        elif sn == 0:
            xs = d
        else:
            d2 = blend(denoised(xp, sn))
            xs = [x + (0.5 * (v + (p - x2) / sn)) * dt for x, v, p, x2 in zip(xs, v1, xp, d2)]
    return xs


def video_loop(heun, tokens, mask, clean, x0_pos, x0_neg, sigmas, cfg_scale, ge_gamma=0.0, trace=None):
    """sample_loop for the video alone: x0_pos / x0_neg(tokens, timesteps, sigma) -> x0."""
    one = lambda fn: None if fn is None else (lambda xs, ts, s: [fn(xs[0], ts[0], s)])       # noqa: E731
    return sample_loop(heun, [dict(tokens=tokens, mask=mask, clean=clean, cfg_scale=cfg_scale)], one(x0_pos), one(x0_neg), sigmas, ge_gamma, trace)[0]


def closed_form_x0(w, bias):
    """The closed-form denoiser of tests/golden/heun_ge.npz: x0 = x - timesteps * tanh(x * w + sigma * bias), element-wise; w, bias: (C,)."""
    def x0(x, ts, sigma):
        return x - ts * torch.tanh(x * w + torch.tensor([sigma], dtype=torch.float32) * bias)
    return x0
