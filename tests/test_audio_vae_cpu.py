"""Audio VAE decoder / vocoder pieces that need no GPU: the reference-name surface of model/audio_vae, the weight packings the HIP
kernels read (emulated in torch), the checkpoint-metadata vocoder choice, the int16 WAV writer and the mux command, and the shapes of the
fp32 restatement (tests/audio_vae_ref.py), pinned to the reference's own output (tests/golden/audio_vae_tiny.npz, written by
tools/pin_audio_vae_against_reference.py), and the loaders' key and layout mapping on synthetic safetensors files."""
import inspect
import json
import os
import struct
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import audio_vae_ref as R  # noqa: E402


def test_package_keeps_the_reference_names():
    import ltx_2_mlx_amd.model.audio_vae as A
    for name in ("AudioDecoder", "Vocoder", "VocoderWithBWE", "load_audio_decoder_weights", "load_vocoder_weights",
                 "load_vocoder_with_bwe_weights", "PerChannelStatistics", "MelSTFT"):
        assert hasattr(A, name) and name in A.__all__, name
    params = lambda f: list(inspect.signature(f).parameters)          # noqa: E731
    assert params(A.AudioDecoder.__init__)[1:11] == ["ch", "out_ch", "ch_mult", "num_res_blocks", "z_channels", "mel_bins", "sample_rate",
                                                     "mel_hop_length", "is_causal", "compute_dtype"]
    assert params(A.Vocoder.__init__)[1:15] == ["resblock_kernel_sizes", "upsample_rates", "upsample_kernel_sizes", "resblock_dilation_sizes",
                                                "upsample_initial_channel", "stereo", "output_sample_rate", "compute_dtype", "resblock",
                                                "activation", "apply_final_activation", "use_tanh_at_final", "use_bias_at_final", "device"]
    assert params(A.VocoderWithBWE.__init__)[1:] == ["vocoder", "bwe_generator", "mel_stft", "input_sampling_rate", "output_sampling_rate",
                                                     "hop_length"]
    assert params(A.MelSTFT.__init__)[1:5] == ["filter_length", "hop_length", "win_length", "n_mel_channels"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # a CPU model holds weights; it does not run
        A.AudioDecoder(device="cpu")(torch.zeros(1, 8, 4, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.Vocoder(device="cpu")(torch.zeros(1, 2, 4, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.MelSTFT(64, 16, 64, 8, device="cpu").mel_spectrogram(torch.zeros(2, 256))


def test_conv_weight_packing_matches_torch():
    """pack_conv_weight's [(i * kw + j) * c_in + c][n] layout, read the way ltx2_audio_conv reads it, is the torch convolution."""
    from ltx_2_mlx_amd import kernels as K
    w = torch.randn(6, 5, 3, 3)
    p = K.pack_conv_weight(w)
    assert p.shape == (45, 8) and torch.equal(p[:, 6:], torch.zeros(45, 2))
    x = torch.randn(5, 7, 9)
    xp = F.pad(x, (1, 1, 2, 0))
    cols = torch.stack([xp[:, i:i + 7, j:j + 9] for i in range(3) for j in range(3)])            # [9, c, 7, 9]
    emu = torch.einsum("tchw,tcn->nhw", cols, p[:, :6].reshape(9, 5, 6))
    assert torch.allclose(emu, F.conv2d(xp[None], w)[0], atol=1e-5)


@pytest.mark.parametrize("k,rate", [(16, 6), (15, 5), (8, 2), (4, 2), (11, 3)])
def test_conv_transpose_polyphase_packing_matches_torch(k, rate):
    """The polyphase decomposition ltx2_audio_conv_transpose1d runs (phase ph, first output o0, input index q0 + n - (ntaps - 1) + t),
    emulated in torch on the packed weight, is ConvTranspose1d."""
    from ltx_2_mlx_amd import kernels as K
    cin, cout, t_in = 4, 3, 9
    w = torch.randn(cin, cout, k)
    x = torch.randn(t_in, cin)
    pad = (k - rate) // 2
    ref = F.conv_transpose1d(x.t()[None], w, stride=rate, padding=pad)[0].t()
    t_out = ref.shape[0]
    wp = K.pack_conv_transpose_weight(w, rate)
    ntaps = (k + rate - 1) // rate
    out = torch.zeros(t_out, cout)
    for ph in range(rate):
        o0 = (ph - pad) % rate
        q0 = (o0 + pad) // rate
        for n in range((t_out - o0 + rate - 1) // rate):
            acc = torch.zeros(cout)
            for t in range(ntaps):
                i = q0 + n - (ntaps - 1) + t
                if 0 <= i < t_in:
                    acc += x[i] @ wp[ph, t, :, :cout]
            out[o0 + rate * n] = acc
    assert torch.allclose(out, ref, atol=1e-5)


def test_create_vocoder_for_checkpoint_follows_the_metadata(tmp_path, monkeypatch):
    """No `bwe` in config.vocoder -> the plain Vocoder (LTX-2.0); with it -> VocoderWithBWE from the metadata's values (LTX-2.3)."""
    from safetensors.torch import save_file
    import generate
    import ltx_2_mlx_amd.model.audio_vae as A

    class Rec:
        def __init__(self, *args, **kw):
            self.args, self.kw = args, kw

    for name in ("Vocoder", "VocoderWithBWE", "MelSTFT"):
        monkeypatch.setattr(A, name, type(name, (Rec,), {}))
    plain = tmp_path / "a.safetensors"
    save_file({"x": torch.zeros(1)}, str(plain), metadata={"config": json.dumps({"vocoder": {"upsample_initial_channel": 1024}})})
    v, is_bwe = generate.create_vocoder_for_checkpoint(str(plain), device="cpu")
    assert not is_bwe and type(v).__name__ == "Vocoder" and v.kw.get("resblock", "1") == "1"
    bwe_cfg = {"vocoder": {"vocoder": {"upsample_initial_channel": 1536, "resblock": "AMP1"},
                           "bwe": {"upsample_rates": [6, 5, 2, 2, 2, 2], "upsample_kernel_sizes": [12, 11, 4, 4, 4, 4], "n_fft": 512, "hop_length": 80,
                                   "num_mels": 64, "input_sampling_rate": 16000, "output_sampling_rate": 48000}}}
    ck = tmp_path / "b.safetensors"
    save_file({"x": torch.zeros(1)}, str(ck), metadata={"config": json.dumps(bwe_cfg)})
    v, is_bwe = generate.create_vocoder_for_checkpoint(str(ck), device="cpu")
    assert is_bwe and type(v).__name__ == "VocoderWithBWE"
    inner, bwe, mel = v.kw["vocoder"], v.kw["bwe_generator"], v.kw["mel_stft"]
    assert inner.kw["upsample_initial_channel"] == 1536 and inner.kw["resblock"] == "AMP1" and inner.kw["output_sample_rate"] == 16000
    assert bwe.kw["upsample_rates"] == [6, 5, 2, 2, 2, 2] and bwe.kw["apply_final_activation"] is False and bwe.kw["output_sample_rate"] == 48000
    assert mel.kw == dict(filter_length=512, hop_length=80, win_length=512, n_mel_channels=64, device="cpu")
    assert v.kw["input_sampling_rate"] == 16000 and v.kw["output_sampling_rate"] == 48000 and v.kw["hop_length"] == 80
    assert not generate.checkpoint_has_audio_decoders(str(ck))


def test_wav_writer_header_rate_count_interleave(tmp_path):
    import generate
    wav = torch.stack([torch.linspace(-1.2, 1.2, 1000), -torch.linspace(0, 0.5, 1000)])[None]          # (1, 2, 1000)
    path = generate.write_wav(str(tmp_path / "a.wav"), wav, 48000)
    with wave.open(path, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (2, 2, 48000, 1000)
        pcm = np.frombuffer(f.readframes(1000), dtype="<i2").reshape(1000, 2)
    ref = (wav[0].numpy() * 32767).clip(-32768, 32767).astype(np.int16)
    assert np.array_equal(pcm[:, 0], ref[0]) and np.array_equal(pcm[:, 1], ref[1])           # left, right interleaved per frame
    assert pcm[0, 0] == -32768 and pcm[-1, 0] == 32767                                           # clipped
    raw = open(path, "rb").read(44)
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and struct.unpack("<HHI", raw[20:28]) == (1, 2, 48000)


def test_mux_command_keeps_the_reference_settings():
    import generate
    cmd = generate.ffmpeg_av_command(384, 256, "a.wav", 24000, "out.mp4", fps=24, speed=3.0)
    assert cmd[cmd.index("-i", cmd.index("-i") + 1) + 1] == "a.wav"
    assert cmd[cmd.index("-af") + 1] == "atempo=2.0,atempo=1.5"
    out_opts = cmd[cmd.index("-c:v"):]                               # the output options (the input side has its own -pix_fmt rgb24)
    for a, b in (("-c:v", "libx264"), ("-c:a", "aac"), ("-b:a", "320k"), ("-ar", "24000"), ("-pix_fmt", "yuv420p"), ("-crf", "18")):
        assert out_opts[out_opts.index(a) + 1] == b
    assert "-shortest" in cmd and cmd[-1] == "out.mp4"


def test_restatement_shapes():
    """The restatement's own bookkeeping: 4T - 3 frames x 4F mel bins; T * prod(rates) samples; the BWE output at the output rate."""
    g = torch.Generator().manual_seed(0)
    ch, mult = 16, (1, 2)
    sd = {"audio_vae.per_channel_statistics.mean-of-means": torch.zeros(ch), "audio_vae.per_channel_statistics.std-of-means": torch.ones(ch)}

    def conv(name, co, ci, k):
        sd[R.DEC + name + ".weight"] = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
        sd[R.DEC + name + ".bias"] = torch.zeros(co)

    conv("conv_in.conv", 32, 8, 3)
    for b in ("mid.block_1", "mid.block_2"):
        conv(b + ".conv1.conv", 32, 32, 3)
        conv(b + ".conv2.conv", 32, 32, 3)
    conv("up.1.block.0.conv1.conv", 32, 32, 3)
    conv("up.1.block.0.conv2.conv", 32, 32, 3)
    conv("up.1.upsample.conv.conv", 32, 32, 3)
    conv("up.0.block.0.conv1.conv", 16, 32, 3)
    conv("up.0.block.0.conv2.conv", 16, 16, 3)
    conv("up.0.block.0.nin_shortcut.conv", 16, 32, 1)
    conv("conv_out.conv", 2, 16, 3)
    y = R.decoder_forward(torch.randn(1, 8, 5, 2, generator=g), sd, ch=ch, ch_mult=mult, num_res_blocks=1)
    assert y.shape == (1, 2, 2 * 5 - 1, 4)           # one upsample level here: 2T - 1 rows, 2F columns, trimmed to 4F
    filt, width, ks = R.hann_filter(2)
    assert ks == 29 and width == 7 and abs(float(filt.sum()) - 1.0) < 1e-2


GOLD = os.path.join(ROOT, "tests", "golden", "audio_vae_tiny.npz")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_restatement_matches_the_reference_golden():
    """The fp32 restatement against the reference's own AudioDecoder, LTX-2.0 Vocoder, AMP1 Vocoder and VocoderWithBWE (run through the
    mlx shim, weights through the reference's loaders).  Gates at <= 5x the measured rel-L2."""
    g = np.load(GOLD)
    assert int(g["seed"]) == R.TINY_SEED
    dec, voc, amp, bwe = R.tiny_weights()
    z, mel = R.tiny_inputs()
    assert np.array_equal(z.numpy(), g["z"]) and np.array_equal(mel.numpy(), g["mel"])
    d = R.TINY_DECODER
    y = R.decoder_forward(z, dec, ch=d["ch"], out_ch=d["out_ch"], ch_mult=d["ch_mult"], num_res_blocks=d["num_res_blocks"])
    assert y.shape == g["decoder"].shape == (1, 2, 4 * 6 - 3, 8)
    assert _rel(y, g["decoder"]) < 4.5e-6                                   # measured 9.1e-7
    strip = lambda sd: {k[len("vocoder."):]: v for k, v in sd.items()}      # noqa: E731
    assert _rel(R.vocoder_forward(mel, strip(voc), R.TINY_VOCODER), g["vocoder"]) < 2.5e-6          # measured 4.9e-7
    assert _rel(R.vocoder_forward(mel, strip(amp), R.TINY_AMP), g["vocoder_amp"]) < 6e-6            # measured 1.3e-6
    s = R.TINY_STFT
    y = R.vocoder_bwe_forward(mel, bwe, R.TINY_AMP, R.TINY_BWE, dict(n_fft=s["n_fft"]), s["in_rate"], s["out_rate"], s["hop"])
    assert y.shape == g["vocoder_bwe"].shape == (1, 2, 2 * 88)
    assert _rel(y, g["vocoder_bwe"]) < 2.2e-5                                # measured 4.5e-6


def _tiny_models(device):
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder, MelSTFT, Vocoder, VocoderWithBWE
    d = R.TINY_DECODER
    dec = AudioDecoder(ch=d["ch"], out_ch=d["out_ch"], ch_mult=d["ch_mult"], num_res_blocks=d["num_res_blocks"], z_channels=d["z_channels"],
                       mel_bins=2, device=device)
    cfg = lambda c: {k: c[k] for k in ("resblock_kernel_sizes", "upsample_rates", "upsample_kernel_sizes", "resblock_dilation_sizes",  # noqa: E731
                                       "upsample_initial_channel")}
    voc = Vocoder(**cfg(R.TINY_VOCODER), device=device)
    amp = Vocoder(**cfg(R.TINY_AMP), resblock="AMP1", activation="snakebeta", device=device)
    s = R.TINY_STFT
    vb = VocoderWithBWE(Vocoder(**cfg(R.TINY_AMP), resblock="AMP1", activation="snakebeta", device=device),
                        Vocoder(**cfg(R.TINY_BWE), resblock="AMP1", activation="snakebeta", apply_final_activation=False, device=device),
                        MelSTFT(s["n_fft"], s["hop"], s["n_fft"], s["n_mels"], device=device), s["in_rate"], s["out_rate"], s["hop"])
    return dec, voc, amp, vb


def test_loaders_map_checkpoint_keys_and_layouts(tmp_path):
    """load_audio_decoder_weights / load_vocoder_weights / load_vocoder_with_bwe_weights on synthetic safetensors files in the checkpoints'
    names and PyTorch layouts, stored bf16: every tensor lands (upcast to fp32) where the model reads it, transposed-conv weights keep
    (in, out, k) and feed the polyphase packing, the mel_stft buffers reach the MelSTFT."""
    from safetensors.torch import save_file
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.audio_vae import load_audio_decoder_weights, load_vocoder_weights, load_vocoder_with_bwe_weights
    dec_w, voc_w, amp_w, bwe_w = R.tiny_weights()
    bf = lambda sd: {k: v.to(torch.bfloat16).contiguous() for k, v in sd.items()}      # noqa: E731
    for name, sd in (("dec", dec_w), ("voc", voc_w), ("amp", amp_w), ("bwe", bwe_w)):
        save_file(bf(sd), str(tmp_path / f"{name}.safetensors"))
    dec, voc, amp, vb = _tiny_models("cpu")
    load_audio_decoder_weights(dec, str(tmp_path / "dec.safetensors"))
    load_vocoder_weights(voc, str(tmp_path / "voc.safetensors"))
    load_vocoder_weights(amp, str(tmp_path / "amp.safetensors"))
    load_vocoder_with_bwe_weights(vb, str(tmp_path / "bwe.safetensors"))
    up = lambda t: t.to(torch.bfloat16).float()                               # noqa: E731

    def same(model_sd, src, prefix):
        want = {k[len(prefix):]: v for k, v in src.items() if k.startswith(prefix)} if prefix else src
        assert sorted(model_sd) == sorted(want)
        for k, v in want.items():
            assert model_sd[k].dtype == torch.float32 and torch.equal(model_sd[k].reshape(v.shape), up(v)), k

    same(dec.state_dict(), dec_w, "")
    same(voc.state_dict(), voc_w, "vocoder.")
    same(amp.state_dict(), amp_w, "vocoder.")
    same(vb.vocoder.state_dict(), {k: v for k, v in bwe_w.items() if k.startswith("vocoder.vocoder.")}, "vocoder.vocoder.")
    same(vb.bwe_generator.state_dict(), {k: v for k, v in bwe_w.items() if k.startswith("vocoder.bwe_generator.")}, "vocoder.bwe_generator.")
    assert torch.equal(vb.mel_stft.stft_fn.forward_basis, up(bwe_w["vocoder.mel_stft.stft_fn.forward_basis"]))
    assert torch.equal(vb.mel_stft.mel_basis, up(bwe_w["vocoder.mel_stft.mel_basis"]))
    assert torch.equal(voc._packed["ups.0.weight"], K.pack_conv_transpose_weight(up(voc_w["vocoder.ups.0.weight"]), 4))
    assert torch.equal(dec._packed["audio_vae.decoder.conv_in.conv.weight"], K.pack_conv_weight(up(dec_w["audio_vae.decoder.conv_in.conv.weight"])))
    # a checkpoint without the audio VAE keeps the decoder as it was, as the reference's loader does
    save_file({"x": torch.zeros(1)}, str(tmp_path / "none.safetensors"))
    load_audio_decoder_weights(dec, str(tmp_path / "none.safetensors"))
    same(dec.state_dict(), dec_w, "")
