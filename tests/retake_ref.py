"""Restatement (numpy / fp32 torch, CPU) of what the retake feature computes, written from the reference's description
(LTX_2_MLX/pipelines/retake.py) and the C header, not from the package: the time window in latent and pixel frames, the state preparation,
the integer composite and the fp32 sampling loop.  Checker side only: nothing here is imported by the package."""
import numpy as np
import torch

from oracle import loop

import keyframe_ref as KR


def frame_window(start_time, end_time, fps, latent_frames):
    """TemporalRegionMask's arithmetic (reference :168-173): seconds -> pixel frames (truncated) -> latent frames [f0, f1)."""
    sp, ep = int(start_time * fps), int(end_time * fps)
    return max(0, (sp - 1) // 8), min(latent_frames, (ep - 1) // 8 + 1)


def pixel_frames_of(k):
    """The pixel frames latent frame k decodes to: frame 0 alone for k = 0, else 8(k-1)+1 .. 8k."""
    return [0] if k == 0 else list(range(8 * (k - 1) + 1, 8 * k + 1))


def pixel_window(window, pixel_frames):
    """[p0, p1): the first and one past the last pixel frame the latent frames [f0, f1) cover, cut at the clip's length."""
    f0, f1 = window
    if f0 >= f1:
        return 0, 0
    covered = [p for k in range(f0, f1) for p in pixel_frames_of(k) if p < pixel_frames]
    return (covered[0], covered[-1] + 1) if covered else (pixel_frames, pixel_frames)


def prepare(encoded, window, noise, noise_scale=1.0):
    """encoded (1, C, F, H, W), noise (1, N, C) -> (clean (1, N, C), mask (1, N, 1), latent (1, N, C)) in fp32: patchify, 1 on the tokens of
    the latent frames [f0, f1), GaussianNoiser with the supplied noise."""
    _, _, f, h, w = encoded.shape
    clean = loop.patchify(encoded.float())
    mask = torch.zeros(1, f * h * w, 1)
    mask[:, window[0] * h * w: window[1] * h * w] = 1.0
    return clean, mask, loop.gaussian_noiser(clean, mask, noise.float(), noise_scale)


def composite_weights(frames, p0, p1, ramp):
    """a[t] of the header's formula: ramp + 1 inside [p0, p1), max(ramp + 1 - d, 0) at distance d outside."""
    a = np.zeros(frames, np.int64)
    for t in range(frames):
        if p0 <= t < p1:
            a[t] = ramp + 1
        else:
            d = p0 - t if t < p0 else t - p1 + 1
            a[t] = max(ramp + 1 - d, 0)
    return a


def composite(decoded, source, p0, p1, ramp):
    """uint8 (T, H, W, 3) x 2 -> uint8: (decoded*a + source*(R - a) + R//2) // R per byte, R = ramp + 1, in Python-width integers."""
    r = ramp + 1
    a = composite_weights(decoded.shape[0], p0, p1, ramp).reshape(-1, 1, 1, 1)
    out = (decoded.astype(np.int64) * a + source.astype(np.int64) * (r - a) + r // 2) // r
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def retake_latent(encoded, window, noise, x0_fn, sigmas, cfg=None, fps=24.0):
    """RetakePipeline up to the latent, in fp32: encoded (1, 128, F, H, W) from the oracle encoder, mask on `window`, noise at scale 1, then
    the distilled loop (cfg None; oracle.loop.denoise_loop_pipeline) or the guided one (cfg = (scale, x0_neg_fn); keyframe_ref.guided_loop).
    x0_fn(tokens, timesteps, sigma, positions) -> x0."""
    _, _, f, h, w = encoded.shape
    clean, mask, x = prepare(encoded, window, noise)
    pos = loop.video_positions(1, f, h, w, fps)
    if cfg is None:
        x = loop.denoise_loop_pipeline(x, mask, clean, lambda t, ts, s: x0_fn(t, ts, s, pos), sigmas)
    else:
        scale, x0_neg = cfg
        x = KR.guided_loop(x, mask, clean, lambda t, ts, s: x0_fn(t, ts, s, pos), lambda t, ts, s: x0_neg(t, ts, s, pos), sigmas, scale)
    return loop.unpatchify(x, f, h, w)
