"""fp32 restatement (torch, CPU) of what the audio-to-video feature computes: the reference's _video_only_denoise_loop
(pipelines/a2vid_two_stage.py:225-271) over any x0 callable, and the two-stage composition over oracle.dit_av.  Checker side only: nothing
here is imported by the package.  The loop is pinned against the reference's own class by tests/golden/a2vid_loop.npz
(tools/pin_a2vid_against_reference.py)."""
import torch

from oracle import loop


def video_only_denoise_loop(x, mask, clean, audio, sigmas, x0_video, video_context, audio_context, negative_video_context=None,
                            negative_audio_context=None, cfg_scale=1.0, callback=None):
    """x (B, N, C) video tokens with their denoise mask (B, N, 1) and clean latent; audio (B, Na, C) frozen: fed to every evaluation with
    timesteps 0 (its mask is all zero), never written.  x0_video(x, video_timesteps (B, N, 1), video_context, audio, audio_timesteps
    (B, Na, 1), audio_context, sigma) -> the video x0.  CFG in the reference's own order (uncond + scale * (cond - uncond)) on the video
    alone, when cfg_scale > 1 and a negative video context is given; its audio context is `negative_audio_context or audio_context`.
    -> (the video tokens, the audio tokens given)."""
    x = x.float()
    n = len(sigmas) - 1
    a_ts = torch.zeros(audio.shape[0], audio.shape[1], 1)
    for i in range(n):
        s = float(sigmas[i])
        ts = loop.timesteps_from_mask(mask, s)
        d = x0_video(x, ts, video_context, audio, a_ts, audio_context, s)
        if cfg_scale > 1.0 and negative_video_context is not None:
            nactx = negative_audio_context if negative_audio_context is not None else audio_context
            u = x0_video(x, ts, negative_video_context, audio, a_ts, nactx, s)
            d = u + cfg_scale * (d - u)
        x = loop.euler_step(x, loop.post_process_latent(d, mask, clean), s, float(sigmas[i + 1]))
        if callback:
            callback(i + 1, n)
    return x, audio


def toy_x0_video(x, ts, vctx, audio, a_ts, actx, sigma):
    """A transformer small enough to run under the reference's own loop (tools/pin_a2vid_against_reference.py): the video x0 depends on every
    input the loop feeds it -- the video latent and timesteps, both contexts, the audio latent, its timesteps and sigma."""
    vel = 0.5 * x + 0.25 * vctx.mean() + 0.125 * audio.mean(dim=1, keepdim=True) * (1.0 + actx.mean()) + a_ts.sum() - 0.0625 * float(sigma)
    return x - ts * vel


def av_x0_video(w, cfg, video_positions, audio_positions):
    """The x0 callable of video_only_denoise_loop over oracle.dit_av (fp32): both modalities evaluated, the video x0 returned.  Both
    modalities carry Modality.sigma = the step's sigma, as modality_from_state / audio_modality_from_state set it."""
    from oracle import dit_av

    def f(x, ts, vctx, audio, a_ts, actx, sigma):
        sg = torch.tensor([sigma], dtype=torch.float32)
        video = dict(latent=x, context=vctx, timesteps=ts, sigma=sg, positions=video_positions)
        aud = dict(latent=audio, context=actx, timesteps=a_ts, sigma=sg, positions=audio_positions)
        return dit_av.av_x0_model(video, aud, w, cfg)[0]
    return f


def two_stage(noise1, noise2, audio, grid, fps, w, cfg, upscale, sigmas1, sigmas2, vctx, actx, nvctx, nactx, cfg_scale, stage1_loop=None):
    """A2VidPipelineTwoStage without image conditioning and with supplied noises: stage 1 on `grid` = (F, H, W) latent frames from pure noise
    at cfg_scale over the frozen audio tokens, `upscale` ((1, 128, F, H, W) -> (1, 128, F, 2H, 2W), statistics included), stage 2 noised at
    sigmas2[0] and refined without guidance over the SAME audio tokens.  stage1_loop / the default: video_only_denoise_loop.
    -> (stage-1 latent (1, 128, F, H, W), final latent (1, 128, F, 2H, 2W))."""
    from oracle import dit_av
    f, h, wd = grid
    apos = dit_av.audio_positions(1, audio.shape[1])
    run = stage1_loop or video_only_denoise_loop

    def stage(x, hh, ww, sigmas, negative, scale):
        n = f * hh * ww
        mask, clean = torch.ones(1, n, 1), torch.zeros(1, n, 128)
        x0 = av_x0_video(w, cfg, loop.video_positions(1, f, hh, ww, fps), apos)
        out, _ = run(x, mask, clean, audio, sigmas, x0, vctx, actx, negative[0], negative[1], scale)
        return loop.unpatchify(out, f, hh, ww)

    lat1 = stage(loop.gaussian_noiser(torch.zeros(1, f * h * wd, 128), torch.ones(1, f * h * wd, 1), noise1, 1.0), h, wd, sigmas1, (nvctx, nactx), cfg_scale)
    up = loop.patchify(upscale(lat1).float())
    x2 = loop.gaussian_noiser(up, torch.ones(1, up.shape[1], 1), noise2, float(sigmas2[0]))
    return lat1, stage(x2, 2 * h, 2 * wd, sigmas2, (None, None), 1.0)
