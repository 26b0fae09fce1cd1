"""Retake with sound without a GPU: the audio window's arithmetic against the restatement and by hand, the configuration and the refusals that
stand before anything touches the device, the restatements of tests/retake_av_ref.py against hand-worked values, and the C ABI's new entries."""
import os
import re

import pytest
import torch

import retake_av_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_audio_window_arithmetic():
    """Token k spans max(4k - 3, 0) .. 4k + 1 hundredths of a second: [0, .01), [.01, .05), [.05, .09), ..."""
    from ltx_2_mlx_amd.components.patchifiers import AudioPatchifier
    from ltx_2_mlx_amd.pipelines import audio_token_window
    from ltx_2_mlx_amd.types import AudioLatentShape
    t = 18
    assert audio_token_window(0.0, 0.01, t) == (0, 1)                      # the causal first token alone
    assert audio_token_window(0.0, 0.005, t) == (0, 1)
    assert audio_token_window(0.01, 0.05, t) == (1, 2)                     # exactly one token: neither neighbour is touched
    assert audio_token_window(0.02, 0.05, t) == (1, 2)                     # ends exactly on a token boundary: token 2 starts there and is outside
    assert audio_token_window(0.02, 0.05 + 1e-9, t) == (1, 3)
    assert audio_token_window(0.05, 0.09, t) == (2, 3)                     # starts exactly on a boundary: token 1 ends there and is outside
    assert audio_token_window(1 / 24, 9 / 24, t) == (1, 11)                # pixel frames [1, 9) at 24 fps
    assert audio_token_window(0.4, 17.5 / 24, t) == (10, 18)               # to the clip's end
    assert audio_token_window(0.4, 100.0, t) == (10, 18)
    assert audio_token_window(0.66, 0.70, t) == (17, 18)                   # the last token: .65 .. .69 is token 17's start .. end
    assert audio_token_window(0.69, 0.70, t) == (0, 0)                     # past the last token's end (17 frames at 24 fps last .708 s)
    assert audio_token_window(5.0, 6.0, t) == (0, 0) and audio_token_window(0.0, 0.0, t) == (0, 0)       # no token touched
    # the restatement's bisection and the patchifier's own bounds (fp32 there, double here) agree with it
    bounds = AudioPatchifier(patch_size=1).get_patch_grid_bounds(AudioLatentShape(1, 8, t, 16))[0, 0].double()
    for t0, t1 in ((0.0, 0.01), (0.013, 0.37), (1 / 24, 9 / 24), (0.4, 0.7), (0.33, 0.3301), (0.7, 5.0), (0.0, 9.0)):
        got = audio_token_window(t0, t1, t)
        assert got == AR.audio_window(t0, t1, t), (t0, t1)
        hit = [k for k in range(t) if float(bounds[k, 0]) < t1 - 1e-6 and float(bounds[k, 1]) > t0 + 1e-6]
        assert got == ((hit[0], hit[-1] + 1) if hit else (0, 0)), (t0, t1)
    assert AR.sample_window((1, 11), 24000) == (240, 9840) and AR.sample_window((0, 1), 16000) == (0, 160)


def test_config_and_exports():
    import ltx_2_mlx_amd.pipelines as P
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.transformer import LTXModel
    c = P.RetakeConfig(start_time=1.0, end_time=2.0)
    assert (c.audio_cfg_scale, c.composite_source_audio, c.audio_composite_ramp_ms) == (None, False, 20.0)
    assert (c.regenerate_video, c.regenerate_audio, c.composite_source, c.composite_ramp, c.use_hip_graph) == (True, True, False, 4, True)
    names = [f.name for f in c.__dataclass_fields__.values()]
    assert names[-3:] == ["audio_cfg_scale", "composite_source_audio", "audio_composite_ramp_ms"] and names.index("composite_ramp") == len(names) - 4
    with pytest.raises(ValueError, match="audio_composite_ramp_ms"):
        P.RetakeConfig(start_time=1.0, end_time=2.0, audio_composite_ramp_ms=-1.0)
    for name in ("joint_guided_denoise_loop", "audio_token_window"):
        assert hasattr(P, name) and name in P.__all__, name
    for name in ("retake_prepare_audio", "retake_composite_audio", "guided_euler_step_pair"):
        assert callable(getattr(K, name)), name
    for name in ("guided_step_joint_av_", "capture_guided_joint_graph", "replay_guided_joint_graph"):
        assert callable(getattr(LTXModel, name)), name


class _VideoOnly:
    """Enough of an LTXModel for RetakePipeline's constructor: a VideoOnly model."""
    model_type = None


def test_refusals_before_the_device():
    """What RetakePipeline refuses with a sound track before it loads or encodes anything: a VideoOnly model, a missing audio context, a
    guider override, both flags False."""
    from ltx_2_mlx_amd.components import CFGGuider
    from ltx_2_mlx_amd.model.transformer import LTXModelType, X0Model
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline
    ctx, track = torch.zeros(1, 4, 8), torch.zeros(1, 8, 18, 16)
    conf = RetakeConfig(start_time=0.4, end_time=0.7, fps=24.0)
    pipe = RetakePipeline(X0Model(_VideoOnly()), object(), None)
    with pytest.raises(ValueError, match=r"requires an audio-video \(AV\) model"):
        pipe(None, ctx, None, conf, audio_encoding=ctx, audio_latent=track)
    av = _VideoOnly()
    av.model_type = LTXModelType.AudioVideo
    pipe = RetakePipeline(X0Model(av), object(), None)
    assert pipe.is_av_model and pipe.audio_window is None and pipe.audio_sample_window is None and pipe.audio_latent is None
    with pytest.raises(ValueError, match="audio_encoding"):
        pipe(None, ctx, None, conf, audio_latent=track)
    with pytest.raises(ValueError, match="audio_encoding"):
        pipe(None, ctx, None, conf, audio_path="track.wav")
    with pytest.raises(NotImplementedError, match="guider override"):
        pipe(None, ctx, None, conf, audio_encoding=ctx, audio_latent=track, guider=CFGGuider(2.0))
    both = RetakeConfig(start_time=0.4, end_time=0.7, fps=24.0, regenerate_video=False, regenerate_audio=False)
    with pytest.raises(ValueError, match="both False"):
        pipe(None, ctx, None, both, audio_encoding=ctx, audio_latent=track)


def test_decoded_waveform_window():
    """_decode_audio on stand-in decoders: the waveform (2, S) of the vocoder, the audio window in its samples (token k starts at
    max(4k - 3, 0) * 10 ms; at 24 kHz a mel frame is 240 samples), cut at S; composite_source_audio without the source file is refused."""
    from ltx_2_mlx_amd.model.transformer import LTXModelType, X0Model
    from ltx_2_mlx_amd.pipelines import RetakeConfig, RetakePipeline

    class Vocoder:
        output_sample_rate = 24000

        def __call__(self, mel):
            return torch.arange(2 * 16560, dtype=torch.float32).reshape(1, 2, 16560)       # (4 * 18 - 3) mel frames of 240 samples

    av = _VideoOnly()
    av.model_type = LTXModelType.AudioVideo
    pipe = RetakePipeline(X0Model(av), object(), None, audio_decoder=lambda latent: latent, vocoder=Vocoder())
    conf = RetakeConfig(start_time=0.4, end_time=0.7, fps=24.0)
    for window, samples in (((1, 11), (240, 9840)), ((0, 1), (0, 240)), ((10, 18), (8880, 16560)), ((0, 0), (0, 0))):
        pipe.audio_window = window
        wave = pipe._decode_audio(torch.zeros(1, 8, 18, 16), None, conf)
        assert wave.shape == (2, 16560) and wave.is_contiguous() and pipe.audio_sample_window == samples == (AR.sample_window(window, 24000) if window[1] else (0, 0))
    keep = RetakeConfig(start_time=0.4, end_time=0.7, fps=24.0, composite_source_audio=True)
    with pytest.raises(ValueError, match="audio_path"):
        pipe._decode_audio(torch.zeros(1, 8, 18, 16), None, keep)


def test_restatements_by_hand():
    """prepare_audio and composite_audio of tests/retake_av_ref.py on values worked by hand."""
    enc = torch.arange(2 * 3 * 2, dtype=torch.float32).reshape(1, 2, 3, 2)          # enc[c][t][m] = 6c + 2t + m
    noise = torch.full((1, 3, 4), 100.0)
    clean, mask, lat = AR.prepare_audio(enc, (1, 2), noise, 0.5)
    assert clean[0].tolist() == [[0, 1, 6, 7], [2, 3, 8, 9], [4, 5, 10, 11]] and mask[0, :, 0].tolist() == [0, 1, 0]
    assert lat[0].tolist() == [[0, 1, 6, 7], [51, 51.5, 54, 54.5], [4, 5, 10, 11]]
    dec, src = torch.full((1, 9), 8.0), torch.zeros(1, 9)
    src[0, 0] = -0.0
    out = AR.composite_audio(dec, src, 4, 6, 3)                                    # R = 4: weights 1 2 3 | 4 4 | 3 2 1 0
    assert out[0].tolist() == [0.0, 2.0, 4.0, 6.0, 8.0, 8.0, 6.0, 4.0, 2.0]
    hard = AR.composite_audio(dec, src, 4, 6, 0)
    assert hard[0].tolist() == [0, 0, 0, 0, 8, 8, 0, 0, 0] and torch.equal(hard[0, :4].view(torch.int32), src[0, :4].view(torch.int32))
    third = AR.composite_audio(torch.full((1, 3), 1.0), torch.zeros(1, 3), 0, 1, 2)            # 2/3 and 1/3 as one IEEE divide each
    assert third[0].tolist() == [1.0, float(torch.tensor(2.0) / torch.tensor(3.0)), float(torch.tensor(1.0) / torch.tensor(3.0))]


def test_denoise_loop_restatement_on_a_toy_model():
    """The reference's loop with an audio state on a linear toy x0: masked tokens move, the others keep their clean bits; one scale on both
    modalities unless audio_cfg_scale is given; no negative context, no guidance."""
    g = torch.Generator().manual_seed(5)
    vclean, aclean, vn, an = (torch.randn(1, n, 4, generator=g) for n in (6, 5, 6, 5))
    vmask, amask = torch.zeros(1, 6, 1), torch.zeros(1, 5, 1)
    vmask[:, 2:4], amask[:, 1:3] = 1.0, 1.0
    video = (vn * vmask + vclean * (1 - vmask), vmask, vclean)
    audio = (an * amask + aclean * (1 - amask), amask, aclean)

    def x0(x, ts, vctx, a, ats, actx, sigma):
        return x - ts * (0.5 * x + vctx + 0.1 * a.mean()), a - ats * (0.25 * a + actx + 0.1 * x.mean())

    sig = [1.0, 0.6, 0.2, 0.0]
    v1, a1 = AR.denoise_loop(video, audio, sig, x0, 0.3, 0.2, -0.1, -0.2, 3.0)
    keep_v, keep_a = vmask[0, :, 0] == 0, amask[0, :, 0] == 0
    assert torch.equal(v1[0][keep_v], vclean[0][keep_v]) and torch.equal(a1[0][keep_a], aclean[0][keep_a])
    assert not torch.equal(v1[0][~keep_v], video[0][0][~keep_v]) and not torch.equal(a1[0][~keep_a], audio[0][0][~keep_a])
    v2, a2 = AR.denoise_loop(video, audio, sig, x0, 0.3, 0.2, -0.1, -0.2, 3.0, 7.0)
    assert not torch.equal(a2, a1)
    v3, a3 = AR.denoise_loop(video, audio, sig, x0, 0.3, 0.2, None, -0.2, 3.0)
    v4, a4 = AR.denoise_loop(video, audio, sig, x0, 0.3, 0.2, -0.1, -0.2, 1.0)
    assert torch.equal(v3, v4) and torch.equal(a3, a4) and not torch.equal(v3, v1)


def test_abi_symbols():
    """The five new entries are declared in the header with the binding's argument counts; the ABI version is still 3."""
    from ltx_2_mlx_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    assert re.search(r"#define\s+LTX2_ABI_VERSION\s+3\b", header) and nv.ABI_VERSION == 3
    assert re.search(r"#define\s+LTX2_RETAKE_AUDIO_MAX_RAMP\s+16777215\b", header) and nv.RETAKE_AUDIO_MAX_RAMP == 16777215
    for name, n_args in (("ltx2_retake_prepare_audio", 12), ("ltx2_retake_composite_audio", 9), ("ltx2_guided_euler_step_pair", 25),
                         ("ltx2_dit_guided_step_joint_av", 18), ("ltx2_dit_graph_capture_guided_joint_av", 17)):
        assert name in nv.SIGNATURES and name in nv.exported_symbols() and nv.SIGNATURES[name][0] is nv.i32, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(decl.split(",")) == len(nv.SIGNATURES[name][1]) == n_args, name
    docs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("ltx2_guided_euler_step_pair", "ltx2_dit_guided_step_joint_av", "ltx2_dit_graph_capture_guided_joint_av"):
        assert name in docs, name


# ------------------------------------------------------------------ generate_video: the route
def test_generate_video_route_resolution(monkeypatch, tmp_path):
    """retake_av is chosen only with BOTH retake_video and retake_audio, ahead of the silent retake route; the plain retake request resolves
    exactly as before; retake_audio alone is a ValueError; the route's own refusals stand before any model loads."""
    import inspect
    import sys
    import wave

    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate as gen

    class Routed(Exception):
        pass

    def stop(*a, **k):
        raise Routed()

    for name in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_with_gemma"):
        monkeypatch.setattr(gen, name, stop)
    clip, track = str(tmp_path / "c.npy"), str(tmp_path / "t.wav")
    np.save(clip, np.zeros((20, 64, 96, 3), np.uint8))
    with wave.open(track, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes(np.zeros(800, "<i2").tobytes())
    sig = inspect.signature(gen.generate_video)
    base = {k: p.default for k, p in sig.parameters.items() if k != "prompt"}
    base.update(prompt="p", use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), retake_video=clip, retake_start_time=0.4, retake_end_time=0.7)
    resolve = lambda **kw: gen._resolve_request({**base, **kw})          # noqa: E731
    r = resolve(retake_audio=track, model_variant="dev", cfg_scale=3.0, retake_audio_cfg=7.0, retake_composite=True)
    assert r.route == "retake_av" and r.generate_audio is True and r.av and not r.need_cfg and r.retake_window == (1, 2)
    assert (r.num_frames, r.height, r.width, r.retake_fps, r.retake_audio, r.retake_audio_cfg) == (17, 64, 96, 24.0, track, 7.0)
    # the plain request: the route, and every attribute of the request, as without the new keywords
    plain = resolve()
    assert plain.route == "retake" and plain.generate_audio is False and not plain.av and plain.retake_audio is None and plain.retake_audio_cfg is None
    assert (plain.num_frames, plain.height, plain.width, plain.retake_fps, plain.retake_window) == (17, 64, 96, 24.0, (1, 2))
    assert resolve(retake_audio_cfg=7.0).route == "retake"                                   # the scale alone selects nothing
    assert gen._ROUTE_EXCLUDES["retake"][0] == ("generate_audio", "audio_path", "keyframes", "control_video", "image_path", "two_stage_distilled",
                                                 "upscale_spatial", "upscale_temporal", "fp8_resident", "pipeline_type")
    assert gen._ROUTE_OWNS["retake"] == ("apg_scale",) and gen._ROUTE_OWNS["retake_av"] == ()
    assert list(gen._ROUTES).index("retake_av") < list(gen._ROUTES).index("retake") and "retake_av" in gen._REQUIRES
    # retake_audio alone
    with pytest.raises(ValueError, match="retake_audio .* is the sound track of retake_video"):
        resolve(retake_video=None, retake_audio=track)
    with pytest.raises(ValueError, match="retake_audio"):
        gen.generate_video("p", use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), retake_audio=track)
    # the route's refusals, by name, before anything loads
    for extra in (dict(audio_path="a.wav"), dict(keyframes=["k.png:0"]), dict(control_video="c.npy"), dict(two_stage_distilled=True),
                  dict(upscale_spatial=True), dict(upscale_temporal=True), dict(fp8_resident=True), dict(pipeline_type="distilled")):
        with pytest.raises(NotImplementedError, match=f"{list(extra)[0]} with retake_video and retake_audio"):
            resolve(retake_audio=track, **extra)
    with pytest.raises(NotImplementedError, match="apg_scale"):
        resolve(retake_audio=track, model_variant="dev", apg_scale=3.0)
    with pytest.raises(FileNotFoundError, match="retake audio track not found"):
        resolve(retake_audio=str(tmp_path / "missing.wav"))
    with pytest.raises(ValueError, match="touches no frame"):
        resolve(retake_audio=track, retake_start_time=5.0, retake_end_time=6.0)
    for other in (dict(a2vid_two_stage=True, audio_path=track), dict(ti2vid_hq_audio=True), dict(two_stage_cfg=True)):
        with pytest.raises(NotImplementedError, match="retake_video with"):
            resolve(retake_audio=track, spatial_upscaler_weights="random", **other)
    # everything in order: the first loader is reached
    with pytest.raises(Routed):
        gen.generate_video("p", use_gemma=False, device="cpu", output_path=str(tmp_path / "o.mp4"), retake_video=clip, retake_audio=track,
                           retake_start_time=0.4, retake_end_time=0.7)
    # the command line
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["p", "--retake", clip, "--retake-audio", track, "--retake-audio-cfg", "7", "--retake-start", "2",
                                                            "--retake-end", "3", "--retake-keep-source"]))
    assert (k["retake_video"], k["retake_audio"], k["retake_audio_cfg"], k["retake_start_time"], k["retake_end_time"], k["retake_composite"]) == \
        (clip, track, 7.0, 2.0, 3.0, True)
    k = gen.kwargs_from_args(gen.build_parser().parse_args(["p"]))
    assert k["retake_audio"] is None and k["retake_audio_cfg"] is None
    for name in ("retake_audio", "retake_audio_cfg"):
        assert sig.parameters[name].kind == inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is None
    # a muxed retake enters ffmpeg at its source's rate; every other mux as before
    cmd = gen.ffmpeg_av_command(96, 64, "a.wav", 24000, "o.mp4", fps=30.0, input_fps=30.0)
    assert cmd[cmd.index("-framerate") + 1] == "30" and "-vf" not in cmd
    cmd = gen.ffmpeg_av_command(96, 64, "a.wav", 24000, "o.mp4", fps=24)
    assert cmd[cmd.index("-framerate") + 1] == "24" and "-vf" not in cmd
