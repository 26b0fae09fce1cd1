"""fp32 restatement (torch, CPU) of stage 1 of the IC-LoRA pipeline: the control clip through the oracle VAE encoder, its tokens appended
at frame 0 (tests/keyframe_ref.append_keyframe), the guidance-free distilled loop.  Checker side only."""
import numpy as np
import torch

from oracle import loop

import keyframe_ref as KR


def control_tensor(frames):
    """uint8 (F, H, W, 3) -> (1, 3, F, H, W) in [-1, 1], as the reference's load_control_signal_tensor forms it."""
    return torch.from_numpy(np.asarray(frames).astype(np.float32) / 127.5 - 1.0).permute(3, 0, 1, 2)[None]


def stage1(control_latents, strengths, grid, fps, noise, x0, sigmas):
    """ICLoraPipeline stage 1 with a supplied noise tensor and no image: zero initial state of `grid` = (F, H, W) latent frames, every control
    latent (1, 128, F, H, W) appended at frame 0 with mask 1 - strength, noised at scale 1, the loop of oracle.loop.denoise_loop_pipeline,
    appended tokens cut off, unpatchified -> (1, 128, F, H, W).  x0(tokens, timesteps, sigma, positions)."""
    f, h, w = grid
    n = f * h * w
    lat = torch.zeros(1, n, 128)
    state = (lat, lat.clone(), torch.ones(1, n, 1), loop.video_positions(1, f, h, w, fps))
    for cl, st in zip(control_latents, strengths):
        state = KR.append_keyframe(*state, cl, 0, st, fps)
    lat, clean, mask, pos = state
    x = loop.gaussian_noiser(lat, mask, noise, 1.0)
    x = loop.denoise_loop_pipeline(x, mask, clean, lambda t, ts, s: x0(t, ts, s, pos), sigmas)
    return loop.unpatchify(x[:, :n], f, h, w)
