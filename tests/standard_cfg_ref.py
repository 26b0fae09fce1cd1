"""fp32 / float64 restatement (torch and numpy, CPU) of the guided standard one-stage loop: classifier-free guidance from the unconditional side,
the per-channel rescale, the x0 Euler step, and the loop over them.  Written from the definition (include/ltx2hip.h), for token-layout latents
(rows = F*H*W tokens, C channels: statistics over the rows).  Checker side only: nothing here is imported by the package."""
import numpy as np
import torch

EPS = 1e-8


def channel_stats64(g, a):
    """float64 two-pass statistics of (rows, C) arrays -> (4, C) float64: mean_g, std_g, mean_a, std_a with std = sqrt(mean((v - mean)^2) + 1e-8)."""
    out = []
    for v in (np.asarray(g, np.float64), np.asarray(a, np.float64)):
        mean = v.mean(axis=0)
        out += [mean, np.sqrt(((v - mean) ** 2).mean(axis=0) + EPS)]
    return np.stack(out)


def guidance(x, vc, vu, ts, cfg_scale):
    """(a, g) as separate fp32 torch ops: a = x - t*vc, b = x - t*vu, g = b + cfg*(a - b).  ts: (1,) or (rows,)."""
    t = ts.reshape(-1, 1).float()
    a = x - t * vc
    b = x - t * vu
    return a, b + torch.tensor(np.float32(cfg_scale)) * (a - b)


def rescale_noise_cfg(g, a, stats, guidance_rescale):
    """gr = ((g - mean_g)/std_g)*std_a + mean_a, then r*gr + (1 - r)*g, each operation rounded in the dtype of g; stats (4, C) in that dtype.
    The two scalars are rounded from Python doubles, as torch rounds a Python scalar: r and 1 - r separately."""
    r, q = torch.tensor(guidance_rescale, dtype=g.dtype), torch.tensor(1 - guidance_rescale, dtype=g.dtype)
    gr = (g - stats[0]) / stats[1] * stats[3] + stats[2]
    return r * gr + q * g


def euler_x0(x, d, sigma, sigma_next):
    """x + ((x - d)*(1/sigma))*(sigma_next - sigma): the Euler step on an x0 prediction, the scalars formed in float32 as the host code forms them."""
    if sigma == 0:
        raise ValueError("Sigma can't be 0.0")
    f = np.float32
    return x + ((x - d) * torch.tensor(f(1.0) / f(sigma))) * torch.tensor(f(sigma_next) - f(sigma))


def rescaled_guided_euler_step(x, vc, vu, ts, stats, cfg_scale, guidance_rescale, sigma, sigma_next):
    """ltx2_rescaled_guided_euler_step's sequence as separate fp32 torch ops; stats None: no rescale."""
    a, g = guidance(x, vc, vu, ts, cfg_scale)
    if stats is not None:
        g = rescale_noise_cfg(g, a, stats, guidance_rescale)
    return euler_x0(x, g, sigma, sigma_next)


def standard_cfg_loop(tokens, x0_pos, x0_neg, sigmas, cfg_scale, guidance_rescale):
    """The guided standard loop on (1, N, C) tokens in fp32, statistics in float64: x0_pos / x0_neg(tokens, timesteps (1,), sigma) -> x0.  Per step
    g = uncond + cfg*(cond - uncond), with guidance_rescale > 0 the per-channel rescale towards cond, then the Euler step."""
    x = tokens.float()
    for i in range(len(sigmas) - 1):
        s = float(sigmas[i])
        ts = torch.tensor([s])
        cond, uncond = x0_pos(x, ts, s), x0_neg(x, ts, s)
        g = uncond + cfg_scale * (cond - uncond)
        if guidance_rescale > 0:
            stats = torch.from_numpy(channel_stats64(g[0].numpy(), cond[0].numpy())).float()
            g = rescale_noise_cfg(g[0], cond[0], stats, guidance_rescale)[None]
        x = euler_x0(x, g, s, float(sigmas[i + 1]))
    return x
