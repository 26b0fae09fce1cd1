"""fp32 torch restatement of what a retake with sound computes, written from the reference's description (LTX_2_MLX/pipelines/retake.py:234-291,
components/patchifiers.py:243-411) and the C header, not from the package: the sound track's state, the waveform composite, the audio window
and the reference's _denoise_loop run with an audio state over oracle.dit_av.  Checker side only: nothing here is imported by the package."""
import math

import torch

from oracle import loop


def prepare_audio(encoded, window, noise, noise_scale=1.0):
    """encoded (1, C, T, M), noise (1, T, C*M) -> (clean (1, T, C*M), mask (1, T, 1), latent (1, T, C*M)), fp32, on encoded's device: the
    AudioPatchifier's patchify, 1 on the latent frames [a0, a1), GaussianNoiser's statements one by one."""
    _, c, t, m = encoded.shape
    clean = encoded.float().permute(0, 2, 1, 3).reshape(1, t, c * m).contiguous()
    mask = torch.zeros(1, t, 1, device=encoded.device)
    mask[:, window[0]: window[1]] = 1.0
    sm = mask * torch.tensor(noise_scale, dtype=torch.float32)
    return clean, mask, noise.float() * sm + clean * (1 - sm)


def composite_audio(decoded, source, s0, s1, ramp):
    """fp32 (channels, S) x 2 -> fp32: decoded on [s0, s1); at distance d outside (s0 - s before, s - s1 + 1 after), with R = ramp + 1 and
    a = max(R - d, 0): (decoded * a + source * (R - a)) / R as separate fp32 statements; a == 0 is the source itself."""
    s = torch.arange(decoded.shape[1], device=decoded.device)
    d = torch.where(s < s0, s0 - s, s - s1 + 1)
    r = ramp + 1
    a = torch.clamp(r - d, min=0)
    af, bf, rf = a.to(torch.float32), (r - a).to(torch.float32), torch.tensor(float(r), dtype=torch.float32, device=decoded.device)
    faded = (decoded * af + source * bf) / rf
    inside = (s >= s0) & (s < s1)
    return torch.where(inside, decoded, torch.where(a == 0, source, faded))


def token_seconds(k, sample_rate=16000, hop_length=160, downsample=4):
    """Start of audio latent frame k in seconds (its end is the start of k + 1): causal, max(4k - 3, 0) mel frames of hop_length samples."""
    return max(downsample * k + 1 - downsample, 0) * hop_length / sample_rate


def audio_window(t0, t1, tokens):
    """[a0, a1): the audio latent frames whose [start, end) seconds intersect [t0, t1), found by bisection on the closed forms in double:
    a0 is the first frame whose end exceeds t0, a1 the first whose start reaches t1.  (0, 0) when that is empty."""
    a0 = next((k for k in range(tokens) if token_seconds(k + 1) > t0), tokens)
    a1 = next((k for k in range(tokens) if token_seconds(k) >= t1), tokens)
    return (a0, a1) if a0 < a1 else (0, 0)


def video_seconds(pixel_window, fps):
    return pixel_window[0] / fps, pixel_window[1] / fps


def sample_window(window, rate):
    """The audio window in samples of a waveform at `rate`."""
    return int(round(token_seconds(window[0]) * rate)), int(round(token_seconds(window[1]) * rate))


def av_x0(w, cfg, video_positions, audio_positions):
    """(video tokens, video timesteps, video context, audio tokens, audio timesteps, audio context, sigma) -> (video x0, audio x0) over
    oracle.dit_av in fp32; both modalities carry Modality.sigma = the step's sigma."""
    from oracle import dit_av

    def f(x, ts, vctx, audio, a_ts, actx, sigma):
        sg = torch.tensor([sigma], dtype=torch.float32)
        video = dict(latent=x, context=vctx, timesteps=ts, sigma=sg, positions=video_positions)
        aud = dict(latent=audio, context=actx, timesteps=a_ts, sigma=sg, positions=audio_positions)
        return dit_av.av_x0_model(video, aud, w, cfg)
    return f


def denoise_loop(video, audio, sigmas, x0, vctx, actx, nvctx=None, nactx=None, cfg_scale=1.0, audio_cfg_scale=None):
    """The reference's RetakePipeline._denoise_loop (:234-291) with an audio state.  video / audio: (tokens, mask (1, n, 1), clean).  One
    cfg_scale on both modalities as the reference has it (audio_cfg_scale: this code base's addition), in the reference's own order
    uncond + scale * (cond - uncond), under its condition cfg_scale > 1 and a negative video context; post_process_latent and Euler on both."""
    (vx, vmask, vclean), (ax, amask, aclean) = video, audio
    vx, ax = vx.float(), ax.float()
    a_scale = cfg_scale if audio_cfg_scale is None else audio_cfg_scale
    for i in range(len(sigmas) - 1):
        s, s_next = float(sigmas[i]), float(sigmas[i + 1])
        vts, ats = loop.timesteps_from_mask(vmask, s), loop.timesteps_from_mask(amask, s)
        dv, da = x0(vx, vts, vctx, ax, ats, actx, s)
        if (cfg_scale > 1.0 or a_scale > 1.0) and nvctx is not None and nactx is not None:
            uv, ua = x0(vx, vts, nvctx, ax, ats, nactx, s)
            dv = uv + cfg_scale * (dv - uv)
            da = ua + a_scale * (da - ua)
        vx = loop.euler_step(vx, loop.post_process_latent(dv, vmask, vclean), s, s_next)
        ax = loop.euler_step(ax, loop.post_process_latent(da, amask, aclean), s, s_next)
    return vx, ax


def retake_av_latents(encoded_video, frame_window, video_noise, encoded_audio, audio_win, audio_noise, w, cfg, sigmas, vctx, actx, nvctx=None,
                      nactx=None, cfg_scale=1.0, audio_cfg_scale=None, fps=24.0):
    """The pipeline up to both latents in fp32: encoded_video (1, 128, F, H, W) with the mask on frame_window, encoded_audio (1, C, T, M) with
    the mask on audio_win, noise at scale 1 on the masked tokens, the loop above.  -> (video (1, 128, F, H, W), audio (1, C, T, M))."""
    from oracle import dit_av
    _, _, f, h, wd = encoded_video.shape
    _, c, t, m = encoded_audio.shape
    vclean = loop.patchify(encoded_video.float())
    vmask = torch.zeros(1, f * h * wd, 1)
    vmask[:, frame_window[0] * h * wd: frame_window[1] * h * wd] = 1.0
    vx = loop.gaussian_noiser(vclean, vmask, video_noise.float(), 1.0)
    aclean, amask, ax = prepare_audio(encoded_audio, audio_win, audio_noise, 1.0)
    x0 = av_x0(w, cfg, loop.video_positions(1, f, h, wd, fps), dit_av.audio_positions(1, t))
    vx, ax = denoise_loop((vx, vmask, vclean), (ax, amask, aclean), sigmas, x0, vctx, actx, nvctx, nactx, cfg_scale, audio_cfg_scale)
    return loop.unpatchify(vx, f, h, wd), ax.reshape(1, t, c, m).permute(0, 2, 1, 3).contiguous()


assert math.isclose(token_seconds(1), 0.01) and token_seconds(0) == 0.0
