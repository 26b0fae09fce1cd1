"""Restatement (torch / numpy, CPU) of the projected guidance step: the element-wise sequences of ltx2_guidance_sums and
ltx2_projected_euler_step as separate fp32 torch ops, the five sums and the scalars in float64, and the guided loop with the torch guiders.
Checker side only: nothing here is imported by the package."""
import math

import numpy as np
import torch

from oracle import loop

f32 = np.float32


def x0_pair(x, vc, vu, ts):
    """a = x - t*vc, b = x - t*vu as the kernels form them.  x, vc, vu: (rows, C); ts: (1,) or (rows,)."""
    t = ts.reshape(-1, 1).float()
    return x - t * vc, x - t * vu


def guidance(a, b, running=None, momentum=0.0, first=True):
    """g of ltx2_guidance_sums: a - b, or with a running buffer momentum*running + (a - b) unless `first`.  The result is the new running."""
    g = a - b
    if running is not None and not first:
        g = torch.tensor(f32(momentum)) * running + g
    return g


def sums_f64(a, b, g):
    """S_aa, S_ab, S_bb, S_gg, S_ga in float64 from the fp32 tensors, and sum |term| of each (for the conditioning check)."""
    a, b, g = a.double(), b.double(), g.double()
    terms = (a * a, a * b, b * b, g * g, g * a)
    return [float(t.sum()) for t in terms], [float(t.abs().sum()) for t in terms]


def scalars_f64(s, mode, norm_threshold):
    """The scalars of ltx2_projected_euler_step in float64: (coef,) for mode 0, (sf, proj) for modes 1 and 2."""
    s_aa, s_ab, s_bb, s_gg, s_ga = s
    if mode == 0:
        return (s_ab / (s_bb + 1e-8),)
    thr = float(f32(norm_threshold))
    sf = min(1.0, thr / math.sqrt(s_gg)) if thr > 0 else 1.0
    return sf, sf * s_ga / (s_aa + 1e-8)


def ulps(got: float, want: float) -> float:
    """|got - fp32(want)| in units of the fp32 spacing at want."""
    w = f32(want)
    return abs(float(f32(got)) - float(w)) / float(np.spacing(np.abs(w)))


def projected_step(x, a, b, g, mask, clean, mode, scale, eta, k0, k1, sigma, sigma_next):
    """ltx2_projected_euler_step's element-wise sequence as separate fp32 torch ops, given the fp32 scalars the kernel used (k0 = coef or
    sf, k1 = proj).  g: a - b, or the running guidance (mode 2 with momentum)."""
    if sigma == 0:
        raise ValueError("Sigma can't be 0.0")
    mult = torch.tensor(f32(scale) if mode == 2 else f32(scale) - f32(1.0))
    inv = torch.tensor(f32(1.0) / f32(sigma))
    dt = torch.tensor(f32(sigma_next) - f32(sigma))
    k0, k1, eta = torch.tensor(f32(k0)), torch.tensor(f32(k1)), torch.tensor(f32(eta))
    if mode == 0:
        d = a + mult * (a - k0 * b)
    else:
        gs = g * k0
        par = k1 * a
        apg = par * eta + (gs - par)
        d = a + apg * mult
    if mask is not None:
        m = mask.reshape(-1, 1).float()
        d = d * m + clean * (1 - m)
    return x + ((x - d) * inv) * dt


def guided_loop(tokens, mask, clean, x0_pos, x0_neg, sigmas, guider):
    """The reference's guided loop (guider.guide on the two x0 predictions over ALL tokens, post_process_latent, Euler) in fp32 with a
    torch guider.  x0_pos / x0_neg(tokens, timesteps (B, N, 1), sigma) -> x0."""
    if hasattr(guider, "reset"):
        guider.reset()
    x = tokens.float()
    for i in range(len(sigmas) - 1):
        s = float(sigmas[i])
        ts = loop.timesteps_from_mask(mask, s)
        x0 = loop.post_process_latent(guider.guide(x0_pos(x, ts, s), x0_neg(x, ts, s)), mask, clean)
        x = loop.euler_step(x, x0, s, float(sigmas[i + 1]))
    return x
