"""fp32 restatement (torch, CPU) of what the keyframe interpolation feature computes: the guided Euler step element by element, the
appended-token conditioning, the guided loop and stage 1 of the pipeline.  Checker side only: nothing here is imported by the package."""
import numpy as np
import torch

from oracle import loop


def guided_euler_step(x, vc, vu, ts, mask, clean, cfg_scale, sigma, sigma_next):
    """ltx2_guided_euler_step's sequence as separate fp32 torch ops (each individually rounded); the scalars are formed in numpy float32
    as the host code forms them.  x, vc, vu, clean: (rows, C); ts: (1,) or (rows,); mask: (rows,) or None."""
    if sigma == 0:
        raise ValueError("Sigma can't be 0.0")
    f = np.float32
    s1 = torch.tensor(f(cfg_scale) - f(1.0))
    inv = torch.tensor(f(1.0) / f(sigma))
    dt = torch.tensor(f(sigma_next) - f(sigma))
    t = ts.reshape(-1, 1).float()
    a = x - t * vc
    b = x - t * vu
    d = a + s1 * (a - b)
    if mask is not None:
        m = mask.reshape(-1, 1).float()
        d = d * m + clean * (1 - m)
    return x + ((x - d) * inv) * dt


def append_keyframe(latent, clean, mask, positions, kf_latent, frame_idx, strength, fps):
    """VideoConditionByKeyframeIndex.apply_to restated on plain tensors: (B, C, 1, H, W) keyframe tokens appended with their own positions."""
    _, _, f, h, w = kf_latent.shape
    tokens = loop.patchify(kf_latent.float())
    pos = loop.video_positions(kf_latent.shape[0], f, h, w, 1.0, causal_fix=(frame_idx == 0))     # fps 1: temporal bounds still in frames
    pos[:, 0] = (pos[:, 0] + frame_idx) / fps
    m = torch.full((tokens.shape[0], tokens.shape[1], 1), 1.0 - strength)
    return (torch.cat([latent, tokens], 1), torch.cat([clean, tokens], 1), torch.cat([mask, m], 1), torch.cat([positions, pos], 2))


def guided_loop(tokens, mask, clean, x0_pos, x0_neg, sigmas, cfg_scale):
    """The reference's keyframe stage-1 loop (CFGGuider on the x0 predictions, post_process_latent, Euler) in fp32.
    x0_pos / x0_neg(tokens, timesteps (B, N, 1), sigma) -> x0."""
    x = tokens.float()
    for i in range(len(sigmas) - 1):
        s = float(sigmas[i])
        ts = loop.timesteps_from_mask(mask, s)
        p, n = x0_pos(x, ts, s), x0_neg(x, ts, s)
        x0 = loop.post_process_latent(p + (cfg_scale - 1) * (p - n), mask, clean)
        x = loop.euler_step(x, x0, s, float(sigmas[i + 1]))
    return x


def stage1(kf_latents, frame_idx, strengths, grid, fps, noise, x0_pos, x0_neg, sigmas, cfg_scale):
    """KeyframeInterpolationPipeline stage 1 with a supplied noise tensor: zero initial state of `grid` = (F, H, W) latent frames, keyframes
    appended, noised at scale 1, guided loop, appended tokens cut off, unpatchified -> (1, 128, F, H, W)."""
    f, h, w = grid
    n = f * h * w
    lat = torch.zeros(1, n, 128)
    state = (lat, lat.clone(), torch.ones(1, n, 1), loop.video_positions(1, f, h, w, fps))
    for kl, idx, st in zip(kf_latents, frame_idx, strengths):
        state = append_keyframe(*state, kl, idx, st, fps)
    lat, clean, mask, pos = state
    x = loop.gaussian_noiser(lat, mask, noise, 1.0)
    x = guided_loop(x, mask, clean, lambda t, ts, s: x0_pos(t, ts, s, pos), lambda t, ts, s: x0_neg(t, ts, s, pos), sigmas, cfg_scale)
    return loop.unpatchify(x[:, :n], f, h, w)
