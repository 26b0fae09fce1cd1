"""Audio VAE encoder, host side: the fp32 restatement (tests/audio_encoder_ref.py) against the vector recorded from the reference's own
AudioEncoder (tests/golden/audio_encoder_tiny.npz, tools/pin_audio_encoder_against_reference.py), the frame bookkeeping against
AudioLatentShape, the checkpoint key spellings, the C ABI entries, the refusals of generate_video / OneStagePipeline before any model
loads, and load_audio_file.  No GPU."""
import inspect
import os
import re
import sys
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import audio_encoder_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "audio_encoder_tiny.npz")


def _tiny_encoder(device="cpu"):
    from ltx_2_mlx_amd.model.audio_vae import AudioEncoder
    c = R.TINY_ENCODER
    return AudioEncoder(ch=c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"], z_channels=c["z_channels"], mel_bins=R.TINY_MEL_BINS,
                        device=device)


def test_package_keeps_the_reference_names():
    import ltx_2_mlx_amd.model.audio_vae as A
    for name in ("AudioEncoder", "load_audio_encoder_weights", "encode_audio", "AudioProcessor", "load_audio_file"):
        assert hasattr(A, name) and name in A.__all__, name
    params = lambda f: list(inspect.signature(f).parameters)          # noqa: E731
    assert params(A.AudioEncoder.__init__)[1:12] == ["ch", "in_ch", "ch_mult", "num_res_blocks", "z_channels", "mel_bins", "double_z", "sample_rate",
                                                     "mel_hop_length", "is_causal", "compute_dtype"]
    assert params(A.load_audio_encoder_weights) == ["encoder", "weights_path"] and params(A.encode_audio) == ["spectrogram", "encoder"]
    assert params(A.load_audio_file) == ["audio_path", "target_sr", "start_time", "max_duration"]
    with pytest.raises(NotImplementedError, match="is_causal"):
        A.AudioEncoder(is_causal=False, device="cpu")
    enc = A.AudioEncoder(compute_dtype=torch.bfloat16, device="cpu")
    assert enc.compute_dtype == torch.float32
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # a CPU model holds weights; it does not run
        enc(torch.zeros(1, 2, 5, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.AudioProcessor(device="cpu").waveform_to_mel(np.zeros((1, 4000), np.float32), 16000)
    assert "not built" not in A.__doc__


def test_restatement_matches_the_reference_golden():
    """The fp32 restatement against the reference's own AudioEncoder (run through the mlx shim, weights through the reference's loader).
    Gate at 5x the measured rel-L2."""
    g = np.load(GOLD)
    assert int(g["seed"]) == R.TINY_SEED
    mel = R.tiny_input()
    assert np.array_equal(mel.numpy(), g["mel"])
    y = R.encoder_forward(mel, R.tiny_weights(), **R.TINY_ENCODER)
    assert y.shape == g["latent"].shape == (1, 2, 4, 4)
    a, b = y.double().numpy(), g["latent"].astype(np.float64)
    err = float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print(f"restatement vs reference golden: rel-L2 {err:.3e}")
    assert err < 3.3e-6, err                                                # measured 6.6e-7
    # the statistics matter to the vector: a c*F+f / f*z+c swap of their index is far outside the gate
    sd = R.tiny_weights()
    swapped = dict(sd)
    swapped[R.MEAN] = sd[R.MEAN].reshape(2, 4).t().reshape(-1)
    assert float((R.encoder_forward(mel, swapped, **R.TINY_ENCODER) - y).abs().max()) > 1e-2


@pytest.mark.parametrize("fps", [24.0, 25.0])
@pytest.mark.parametrize("frames", [9, 25, 97, 121])
def test_output_frames_and_waveform_fit_give_the_audio_latent_shape(frames, fps):
    """A waveform cut or padded to num_frames / fps seconds -> centred mel frames -> output_frames: at most one surplus latent frame over
    AudioLatentShape.from_video_pixel_shape(...).frames, which fit_audio_latent crops; a short latent is an error."""
    import generate
    from ltx_2_mlx_amd.model.audio_vae import AudioEncoder, AudioProcessor
    from ltx_2_mlx_amd.types import AudioLatentShape, VideoPixelShape
    proc, enc = AudioProcessor(device="cpu"), AudioEncoder(device="cpu")
    want = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=frames, height=64, width=64, fps=fps)).frames
    samples = proc.samples_for_video(frames, fps)
    assert samples == round(frames / fps * 16000)
    for n in (samples // 3, samples, samples + 777):          # shorter (padded with silence), exact, longer (cut)
        w = proc.fit_waveform(np.ones((2, n), np.float32), samples)
        assert w.shape == (2, samples) and float(w[:, :min(n, samples)].min()) == 1.0 and float(np.abs(w[:, min(n, samples):]).sum()) == 0.0
    t_mel = proc.mel_frames(samples)
    assert t_mel == 1 + samples // 160
    got = enc.output_frames(t_mel)
    assert got == -(-t_mel // 4) and 0 <= got - want <= 1
    fitted = generate.fit_audio_latent(torch.zeros(1, 8, got, 16), want)
    assert fitted.shape == (1, 8, want, 16) == AudioLatentShape(1, 8, want, 16).to_tuple()
    with pytest.raises(ValueError, match="latent frames"):
        generate.fit_audio_latent(torch.zeros(1, 8, want - 1, 16), want)
    # the decoder's inverse bookkeeping: T latent frames decode to 4T - 3 mel frames, which encode back to T
    assert all(enc.output_frames(4 * t - 3) == t for t in range(1, 40))
    assert [enc.output_frames(t) for t in (1, 2, 13, 21, 22)] == [1, 1, 4, 6, 6]


def test_load_state_dict_accepts_both_key_spellings(tmp_path):
    """The reference loader's spelling, the decoder checkpoints' doubled `.conv.`, the shared statistics as a fallback; a wrong shape
    raises; through a safetensors file (bf16) as load_audio_encoder_weights reads it."""
    from safetensors.torch import save_file
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.audio_vae import load_audio_encoder_weights
    sd = R.tiny_weights()
    enc = _tiny_encoder()
    assert sorted(enc.expected_weight_shapes()) == sorted(sd)
    assert all(tuple(sd[k].shape) == s for k, s in enc.expected_weight_shapes().items())
    assert enc.load_state_dict(sd) == len(sd)
    assert all(torch.equal(v, sd[k]) for k, v in enc.state_dict().items()) and sorted(enc.state_dict()) == sorted(sd)
    assert torch.equal(enc._packed[R.ENC + "down.0.downsample.conv.weight"], K.pack_conv_weight(sd[R.ENC + "down.0.downsample.conv.weight"]))

    def doubled(k):
        stem, leaf = k.rsplit(".", 1)
        return f"{stem}.conv.{leaf}"

    dd = {(k if "per_channel_statistics" in k else doubled(k)): v for k, v in sd.items()}
    assert R.ENC + "conv_in.conv.weight" in dd and R.ENC + "down.1.downsample.conv.conv.bias" in dd and R.ENC + "mid.block_2.conv2.conv.weight" in dd
    enc2 = _tiny_encoder()
    assert enc2.load_state_dict(dd) == len(sd)
    assert all(torch.equal(v, sd[k]) for k, v in enc2.state_dict().items())
    # the shared statistics are taken only when the encoder's own are absent
    shared = {k: v for k, v in dd.items() if "per_channel_statistics" not in k}
    shared["audio_vae.per_channel_statistics.mean-of-means"] = sd[R.MEAN] + 1
    shared["audio_vae.per_channel_statistics.std-of-means"] = sd[R.STD] + 2
    enc3 = _tiny_encoder()
    assert enc3.load_state_dict(shared) == len(sd)
    assert torch.equal(enc3.per_channel_statistics.mean_of_means, sd[R.MEAN] + 1) and torch.equal(enc3.per_channel_statistics.std_of_means, sd[R.STD] + 2)
    enc3.load_state_dict(dict(shared, **{R.MEAN: sd[R.MEAN], R.STD: sd[R.STD]}))
    assert torch.equal(enc3.per_channel_statistics.mean_of_means, sd[R.MEAN])
    for bad in (R.ENC + "conv_in.weight", R.ENC + "conv_in.conv.weight", R.MEAN):
        with pytest.raises(ValueError, match="shape"):
            _tiny_encoder().load_state_dict({bad: torch.zeros(3, 3)})
    # the file loader, bf16 tensors, doubled spelling + shared statistics; a file without encoder keys leaves the encoder as it was
    save_file({k: v.to(torch.bfloat16).contiguous() for k, v in shared.items()}, str(tmp_path / "enc.safetensors"))
    enc4 = _tiny_encoder()
    load_audio_encoder_weights(enc4, str(tmp_path / "enc.safetensors"))
    up = lambda t: t.to(torch.bfloat16).float()                               # noqa: E731
    got = enc4.state_dict()
    assert sorted(got) == sorted(sd) and all(got[k].dtype == torch.float32 for k in got)
    assert all(torch.equal(got[k], up(sd[k])) for k in sd if "per_channel_statistics" not in k)
    assert torch.equal(got[R.MEAN], up(sd[R.MEAN] + 1))
    save_file({"x": torch.zeros(1)}, str(tmp_path / "none.safetensors"))
    load_audio_encoder_weights(enc4, str(tmp_path / "none.safetensors"))
    assert torch.equal(enc4.state_dict()[R.MEAN], up(sd[R.MEAN] + 1))
    with pytest.raises(RuntimeError, match="not loaded"):
        _tiny_encoder()._conv(torch.zeros(1), "conv_in", 3)


def test_entries_are_declared_bound_and_resolve():
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    header = open(os.path.join(ROOT, "include", "ltx2hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = nv.lib()
    for name, n_args in (("ltx2_audio_conv2d_strided", 23), ("ltx2_audio_latent_normalize", 9)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, f"{name} not declared in include/ltx2hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = nv.SIGNATURES[name]
        assert res is nv.i32 and len(args) == len(params) == n_args
        for p, a in zip(params, args):
            want = nv.vp if "*" in p else nv.i64 if p.startswith("int64_t") else nv.f32 if p.startswith("float") else nv.i32
            assert a is want, (name, p)
        assert hasattr(lib, name) and hasattr(nv.lib(torch.float16), name)
        assert name in integration
    params = [p.strip() for p in re.search(r"int\s+ltx2_audio_conv2d_strided\s*\(([^)]*)\)", header).group(1).split(",")]
    assert params[15:17] == ["int stride_h", "int stride_w"]
    assert "#define LTX2_AUDIO_ACT_SILU 4" in header and nv.AUDIO_ACT_SILU == 4
    assert callable(K.audio_conv2d_strided) and callable(K.audio_latent_normalize)
    # ltx2_audio_conv keeps its signature
    m = re.search(r"int\s+ltx2_audio_conv\s*\(([^)]*)\)", header)
    assert len(m.group(1).split(",")) == 28 == len(nv.SIGNATURES["ltx2_audio_conv"][1])


def test_audio_flag_is_refused_before_any_model_loads(tmp_path, monkeypatch):
    """--audio on the video-only branch (the flag does not imply --generate-audio) and with --two-stage-distilled raise before a
    transformer, a VAE or a text encoder is built; OneStagePipeline(initial_audio_latent=) raises on a video-only transformer."""
    import generate

    def boom(*a, **k):
        raise AssertionError("a model was loaded")

    for name in ("load_transformer", "load_av_transformer", "create_vae_decoder", "create_dummy_text_encoding", "encode_audio_for_video"):
        monkeypatch.setattr(generate, name, boom)
    wav = tmp_path / "a.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.zeros(16, "<i2").tobytes())
    kw = dict(use_gemma=False, output_path=str(tmp_path / "o.mp4"), num_frames=9, height=64, width=64)
    with pytest.raises(ValueError, match="generate_audio=True"):
        generate.generate_video("a prompt", audio_path=str(wav), **kw)
    with pytest.raises(NotImplementedError, match="two_stage_distilled"):
        generate.generate_video("a prompt", audio_path=str(wav), generate_audio=True, two_stage_distilled=True, **kw)
    with pytest.raises(FileNotFoundError):
        generate.generate_video("a prompt", audio_path=str(tmp_path / "missing.wav"), generate_audio=True, **kw)
    a = generate.build_parser().parse_args(["p", "--audio", "x.wav", "--audio-start", "1.5", "--audio-duration", "2"])
    k = generate.kwargs_from_args(a)
    assert (k["audio_path"], k["audio_start_time"], k["audio_max_duration"]) == ("x.wav", 1.5, 2.0) and k["generate_audio"] is False
    k = generate.kwargs_from_args(generate.build_parser().parse_args(["p"]))
    assert (k["audio_path"], k["audio_start_time"], k["audio_max_duration"]) == (None, 0.0, None)
    sig = inspect.signature(generate.generate_video).parameters
    assert all(sig[n].kind == inspect.Parameter.KEYWORD_ONLY for n in ("audio_path", "audio_start_time", "audio_max_duration"))

    from ltx_2_mlx_amd.model.transformer import LTXModelType
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline

    class VideoOnly:
        model_type = LTXModelType.VideoOnly
        device = torch.device("cpu")

    pipe = OneStagePipeline.__new__(OneStagePipeline)
    pipe.transformer = type("X0", (), {"velocity_model": VideoOnly()})()
    pipe.is_av_model = False
    cfg = OneStageCFGConfig(height=64, width=64, num_frames=9, num_inference_steps=2, cfg_scale=1.0, audio_cfg_scale=1.0)
    with pytest.raises(ValueError, match="initial_audio_latent needs an AudioVideo transformer"):
        pipe(torch.zeros(1, 4, 8), None, cfg, initial_audio_latent=torch.zeros(1, 8, 9, 16))
    assert inspect.signature(OneStagePipeline.__call__).parameters["initial_audio_latent"].kind == inspect.Parameter.KEYWORD_ONLY


def test_load_audio_file_trim_mono_and_resample(tmp_path):
    """A 10-sample stereo 16-bit wav written here: (channels, samples) at int16 / 32768, the start / duration trim at the file's rate,
    the nearest-index resample (np.linspace(0, n - 1, int(n * target / sr)).astype(int), a2vid_two_stage.py:148-153), all to equality;
    a mono file stays one channel, which the processor duplicates."""
    from ltx_2_mlx_amd.model.audio_vae import load_audio_file
    pcm = np.array([[100 * i, -3000 - 7 * i] for i in range(10)], dtype="<i2")

    def write(path, data, rate):
        with wave.open(str(path), "wb") as f:
            f.setnchannels(data.shape[1])
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(np.ascontiguousarray(data).tobytes())

    write(tmp_path / "s.wav", pcm, 16000)
    ref = (pcm.astype(np.float32) / 32768.0).T
    data, sr = load_audio_file(str(tmp_path / "s.wav"))
    assert sr == 16000 and data.dtype == np.float32 and data.shape == (2, 10) and np.array_equal(data, ref)
    # trim: start 3 samples in, at most 4 samples
    data, _ = load_audio_file(str(tmp_path / "s.wav"), 16000, start_time=3 / 16000, max_duration=4 / 16000)
    assert np.array_equal(data, ref[:, 3:7])
    # resample 8 kHz -> 16 kHz and 16 kHz -> 8 kHz by nearest index, after the trim
    write(tmp_path / "r.wav", pcm, 8000)
    data, sr = load_audio_file(str(tmp_path / "r.wav"), 16000)
    assert sr == 16000 and np.array_equal(data, ref[:, np.linspace(0, 9, 20).astype(int)])
    data, sr = load_audio_file(str(tmp_path / "r.wav"), 16000, start_time=2 / 8000, max_duration=6 / 8000)
    assert np.array_equal(data, ref[:, 2:8][:, np.linspace(0, 5, 12).astype(int)])
    data, sr = load_audio_file(str(tmp_path / "s.wav"), 8000)
    assert sr == 8000 and np.array_equal(data, ref[:, np.linspace(0, 9, 5).astype(int)])
    # mono
    write(tmp_path / "m.wav", pcm[:, :1], 16000)
    data, sr = load_audio_file(str(tmp_path / "m.wav"))
    assert data.shape == (1, 10) and np.array_equal(data, ref[:1])


def test_mel_filterbank_and_basis_follow_the_definition():
    """The processor's vectorised float64 bases against the entry-by-entry ones of the restatement."""
    from ltx_2_mlx_amd.model.audio_vae.processor import slaney_mel_filterbank, windowed_dft_basis
    fb = slaney_mel_filterbank(16000, 1024, 64, 0.0, 8000.0)
    ref = R.mel_filterbank(16000, 1024, 64, 0.0, 8000.0)
    assert fb.shape == ref.shape == (64, 513) and np.abs(fb - ref).max() < 1e-15 and (fb.sum(1) > 0).all()
    b = windowed_dft_basis(64, 64)
    x = np.random.RandomState(0).randn(64)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(64) / 64)
    spec = np.fft.rfft(x * win)
    assert np.abs(b[:33] @ x - spec.real).max() < 1e-12 and np.abs(b[33:] @ x - spec.imag).max() < 1e-12
