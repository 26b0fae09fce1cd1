"""Audio VAE decoder + vocoders on the MI355X: the fp32 kernels of csrc/audio.hip against fp32 torch on edge shapes, the models against
the fp32 restatement (tests/audio_vae_ref.py) at production width on ~1 s of audio, the pipeline and generate_video paths end to end.
Parity gates sit at <= 5x the value measured on the GPU."""
import os
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import measure, rel_l2  # noqa: E402

import audio_vae_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(*shape, generator=g)


@pytest.mark.parametrize("t,cin,cout,k,dil,stride,pad,pro,epi", [
    (300, 64, 96, 3, 1, 1, 1, 1, "res"),          # dilation 1, leaky prologue, residual epilogue
    (301, 64, 64, 3, 3, 1, 3, 1, "acc"),          # dilation 3, scaled accumulate
    (257, 32, 32, 7, 5, 1, 15, 0, "tanh"),        # dilation 5, k 7, tanh
    (200, 18, 40, 11, 1, 1, 5, 0, "clip"),        # k 11, K = 198 not a multiple of 16, c_in not a multiple of 4 (scalar staging)
    (4000, 1, 66, 64, 1, 16, 48, 0, "none"),      # stride-hop STFT: one input channel
    (50, 512, 512, 7, 1, 1, 3, 0, "none"),        # a grid under one round
    (129, 128, 2, 7, 1, 1, 3, 1, "tanh"),         # conv_post: 2 output channels
])
def test_audio_conv1d_matches_torch(t, cin, cout, k, dil, stride, pad, pro, epi):
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    x = _rand(t, cin, seed=t)
    w = _rand(cout, cin, k, seed=k, scale=1 / (cin * k) ** 0.5)
    b = _rand(cout, seed=3, scale=0.1)
    t_out = (t + 2 * pad - dil * (k - 1) - 1) // stride + 1
    xin = F.leaky_relu(x, 0.1) if pro else x
    ref = F.conv1d(F.pad(xin.t()[None], (pad, pad)), w, b, stride=stride, dilation=dil)[0].t()
    kw = dict(stride=stride, dilation=dil, padding=pad, prologue=nv.AUDIO_PRO_LEAKY_RELU if pro else 0, slope=0.1)
    res = _rand(t_out, cout, seed=9)
    prior = _rand(t_out, cout, seed=10)
    out = None
    if epi == "res":
        kw["res"] = res.to(DEV)
        ref = ref + res
    elif epi == "acc":
        out = prior.clone().to(DEV)
        kw.update(res=res.to(DEV), out=out, alpha=1 / 3, beta=1.0)
        ref = prior + (ref + res) / 3
    elif epi == "tanh":
        kw["act"] = nv.AUDIO_ACT_TANH
        ref = torch.tanh(ref)
    elif epi == "clip":
        kw["act"] = nv.AUDIO_ACT_CLIP
        ref = torch.clamp(ref, -1, 1)
    y = K.audio_conv1d(x.to(DEV), K.pack_conv_weight(w.to(DEV)), b.to(DEV), cout, k, **kw)
    torch.cuda.synchronize()
    assert y.shape == (t_out, cout)
    err = rel_l2(y.cpu(), ref)
    assert err < 5e-6, err           # measured 0 - 1.1e-6 (the largest: K = 3584, a grid under one round)


def test_audio_conv_magnitude_prologue_log_epilogue():
    """The mel product as MelSTFT runs it: a 1x1 conv over |X| (the magnitude prologue reads the real | imaginary halves of one row,
    c_in = 1025 not a multiple of 4) with log(max(., 1e-5)) as the epilogue, into a column slice of a wider output."""
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    nf, n_mels, frames = 1025, 128, 77
    spec = _rand(frames, 2 * nf, seed=31)
    basis = torch.rand(n_mels, nf, generator=torch.Generator().manual_seed(32)) * (torch.rand(n_mels, 1, generator=torch.Generator().manual_seed(33)) > 0.1)
    ref = torch.log(torch.clamp(torch.sqrt(spec[:, :nf] ** 2 + spec[:, nf:] ** 2) @ basis.t(), min=1e-5))
    out = torch.zeros(frames, 2 * n_mels, device=DEV)
    K.audio_conv1d(spec.to(DEV), K.pack_conv_weight(basis[:, :, None].to(DEV)), None, n_mels, 1, c_in=nf, prologue=nv.AUDIO_PRO_MAGNITUDE,
                   act=nv.AUDIO_ACT_LOG, out=out[:, n_mels:])
    torch.cuda.synchronize()
    assert torch.equal(out[:, :n_mels].cpu(), torch.zeros(frames, n_mels))          # the other channel's columns untouched
    err = rel_l2(out[:, n_mels:].cpu(), ref)
    assert err < 6e-7, err           # measured 1.2e-7


@pytest.mark.parametrize("k,rate,cin,cout,t", [(16, 6, 64, 32, 37), (15, 5, 48, 24, 40), (8, 2, 32, 16, 101), (4, 2, 32, 16, 64), (4, 2, 16, 2, 5)])
def test_audio_conv_transpose1d_matches_torch(k, rate, cin, cout, t):
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    x = _rand(t, cin, seed=k)
    w = _rand(cin, cout, k, seed=rate, scale=1 / cin ** 0.5)
    b = _rand(cout, seed=1, scale=0.1)
    pad = (k - rate) // 2
    ref = F.conv_transpose1d(F.leaky_relu(x, 0.1).t()[None], w, b, stride=rate, padding=pad)[0].t()
    y = K.audio_conv_transpose1d(x.to(DEV), K.pack_conv_transpose_weight(w.to(DEV), rate), b.to(DEV), cout, k, rate, pad,
                                 prologue=nv.AUDIO_PRO_LEAKY_RELU, slope=0.1)
    torch.cuda.synchronize()
    assert y.shape == ref.shape
    err = rel_l2(y.cpu(), ref)
    assert err < 1.2e-6, err         # measured 1.2e-7 - 2.4e-7


@pytest.mark.parametrize("h,w,cin,cout,k,up", [(20, 16, 8, 64, 3, False), (13, 16, 64, 64, 3, True), (37, 64, 64, 32, 1, False),
                                               (9, 8, 128, 2, 3, False)])
def test_audio_conv2d_matches_torch(h, w, cin, cout, k, up):
    from ltx_2_mlx_amd import kernels as K
    x = _rand(cin, h, w, seed=h)
    wt = _rand(cout, cin, k, k, seed=w, scale=1 / (cin * k * k) ** 0.5)
    b = _rand(cout, seed=2, scale=0.1)
    xin = x.repeat_interleave(2, 1).repeat_interleave(2, 2) if up else x
    p = k - 1
    ref = F.conv2d(F.pad(xin[None], (p // 2, p - p // 2, p, 0)), wt, b)[0]
    ref = ref[:, 1:] if up else ref
    y = K.audio_conv2d(x.permute(1, 2, 0).contiguous().to(DEV), K.pack_conv_weight(wt.to(DEV)), b.to(DEV), cout, k, k, p, p // 2, upsample=up)
    torch.cuda.synchronize()
    err = rel_l2(y.permute(2, 0, 1).cpu(), ref)
    assert err < 3.5e-6, err         # measured 1.0e-7 - 7.1e-7


def test_audio_row_kernels_match_torch():
    """PixelNorm + SiLU, the fused anti-aliased SnakeBeta (C not a multiple of 64, T not a multiple of 64) and the Hann x2 resampler."""
    from ltx_2_mlx_amd import kernels as K
    from ltx_2_mlx_amd.model.audio_vae.vocoder import hann_resample_filter, kaiser_sinc_filter1d
    x = _rand(3, 7, 256, seed=1)
    err = rel_l2(K.audio_pixnorm_silu(x.to(DEV)).cpu(), R._pixnorm_silu(x.permute(2, 0, 1)[None])[0].permute(1, 2, 0))
    assert err < 5e-7, err           # measured <= 9.4e-8
    t, c = 150, 40
    x = _rand(t, c, seed=2)
    f = kaiser_sinc_filter1d(0.25, 0.3, 12)
    sd = {"a.act.alpha": _rand(c, seed=3, scale=0.3), "a.act.beta": _rand(c, seed=4, scale=0.3), "a.upsample.filter": f,
          "a.downsample.lowpass.filter": f}
    ref = R._snake_aa(x.t()[None], sd, "a")[0].t()
    y = K.audio_snake_aa(x.to(DEV), sd["a.act.alpha"].to(DEV), sd["a.act.beta"].to(DEV), f.reshape(-1).to(DEV), f.reshape(-1).to(DEV))
    err = rel_l2(y.cpu(), ref)
    assert err < 5e-7, err           # measured <= 9.4e-8
    filt, width, pad_left = hann_resample_filter(2)
    ref = R._upsample1d(x.t()[None], filt.reshape(-1), 2, width, pad_left, filt.numel() - 2)[0].t()
    y = K.audio_upsample(x.to(DEV), filt.reshape(-1).to(DEV), 2, width, pad_left, 2 * t)
    torch.cuda.synchronize()
    err = rel_l2(y.cpu(), ref)
    assert err < 5e-7, err           # measured <= 9.4e-8


def test_audio_entry_points_reject_bad_arguments():
    from ltx_2_mlx_amd import _native as nv
    x = torch.zeros(64, 16, device=DEV)
    w = torch.zeros(48, 16, device=DEV)
    with pytest.raises(ValueError, match="ldw"):          # ldw not a multiple of 4
        nv.check(nv.lib().ltx2_audio_conv(nv.ptr(x), 16, 1, 64, 16, nv.ptr(w), 15, None, nv.ptr(x), 16, 1, 62, 15, 1, 3, 1, 1, 0, 0, 0, 0, 0.0,
                                          None, 0, 1.0, 0.0, 0, nv.stream()))
    with pytest.raises(ValueError, match="in place"):
        nv.check(nv.lib().ltx2_audio_snake_aa(nv.ptr(x), 16, 64, 16, nv.ptr(x), nv.ptr(x), nv.ptr(x), 12, nv.ptr(x), 12, nv.ptr(x), 16, nv.stream()))
    with pytest.raises(ValueError, match="multiple of 4"):
        nv.check(nv.lib().ltx2_audio_pixnorm_silu(nv.ptr(x), 16, nv.ptr(x), 16, 64, 6, 1e-6, nv.stream()))


# ------------------------------------------------------------------------------------------------------------------------ models
def test_audio_decoder_matches_restatement():
    """Production AudioDecoder (ch 128, mult (1, 2, 4), 3 blocks per level) on 26 latent frames (~1 s: 101 mel frames)."""
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder
    dec = AudioDecoder(device=DEV)
    dec.init_random_weights(5)
    z = _rand(1, 8, 26, 16, seed=6)
    y = dec(z.to(DEV).to(torch.bfloat16))
    torch.cuda.synchronize()
    sd = {k: v.cpu() for k, v in dec.state_dict().items()}
    ref = R.decoder_forward(z.to(torch.bfloat16).float(), sd)
    assert y.shape == (1, 2, 101, 64) and y.dtype == torch.float32
    err = measure("decoder rel_l2", rel_l2(y.cpu(), ref))
    assert err < 1.5e-5, err         # measured 3.2e-6


def test_vocoder_ltx20_production_width_matches_restatement():
    """HiFi-GAN Vocoder at upsample_initial_channel 1024 (the LTX-2.0 defaults) on 101 mel frames (~1 s at 24 kHz)."""
    from ltx_2_mlx_amd.model.audio_vae import Vocoder
    voc = Vocoder(device=DEV)
    voc.init_random_weights(7)
    mel = _rand(1, 2, 101, 64, seed=8)
    y = voc(mel.to(DEV))
    torch.cuda.synchronize()
    cfg = dict(resblock_kernel_sizes=[3, 7, 11], upsample_rates=[6, 5, 2, 2, 2], upsample_kernel_sizes=[16, 15, 8, 4, 4],
               resblock_dilation_sizes=[[1, 3, 5]] * 3)
    ref = R.vocoder_forward(mel, {k: v.cpu() for k, v in voc.state_dict().items()}, cfg)
    assert y.shape == (1, 2, 101 * 240)
    err = measure("vocoder 2.0 rel_l2", rel_l2(y.cpu(), ref))
    assert err < 1.5e-6, err         # measured 3.0e-7


def _bwe(dev, seed=11):
    from ltx_2_mlx_amd.model.audio_vae import MelSTFT, Vocoder, VocoderWithBWE
    inner = Vocoder(resblock="AMP1", activation="snakebeta", device=dev)
    bwe = Vocoder(upsample_rates=[5, 4, 4, 2], upsample_kernel_sizes=[15, 8, 8, 4], upsample_initial_channel=256, resblock="AMP1",
                  activation="snakebeta", apply_final_activation=False, output_sample_rate=48000, device=dev)
    inner.init_random_weights(seed)
    bwe.init_random_weights(seed + 1)
    mel_stft = MelSTFT(512, 80, 512, 64, device=dev)
    mel_stft.set_buffers(R.dft_basis(512), R.dft_basis(512), R.mel_filterbank(64, 257))
    return VocoderWithBWE(inner, bwe, mel_stft, 24000, 48000, 80)


BWE_CFG = dict(resblock="AMP1", resblock_kernel_sizes=[3, 7, 11], upsample_rates=[5, 4, 4, 2], upsample_kernel_sizes=[15, 8, 8, 4],
               resblock_dilation_sizes=[[1, 3, 5]] * 3)
VOC_CFG = dict(resblock="AMP1", resblock_kernel_sizes=[3, 7, 11], upsample_rates=[6, 5, 2, 2, 2], upsample_kernel_sizes=[16, 15, 8, 4, 4],
               resblock_dilation_sizes=[[1, 3, 5]] * 3)


def _bwe_state(v):
    sd = {"vocoder.vocoder." + k: t.cpu() for k, t in v.vocoder.state_dict().items()}
    sd.update({"vocoder.bwe_generator." + k: t.cpu() for k, t in v.bwe_generator.state_dict().items()})
    sd["vocoder.mel_stft.stft_fn.forward_basis"] = v.mel_stft.stft_fn.forward_basis.cpu()
    sd["vocoder.mel_stft.mel_basis"] = v.mel_stft.mel_basis.cpu()
    return sd


def test_vocoder_amp_and_bwe_match_restatement():
    """BigVGAN-v2 AMP1 Vocoder (1024 channels) and VocoderWithBWE (real windowed-DFT basis, mel basis, Hann x2 skip) on 101 mel frames."""
    v = _bwe(DEV)
    mel = _rand(1, 2, 101, 64, seed=12)
    base = v.vocoder(mel.to(DEV))
    y = v(mel.to(DEV))
    torch.cuda.synchronize()
    sd = _bwe_state(v)
    ref_base = R.vocoder_forward(mel, {k[len("vocoder.vocoder."):]: t for k, t in sd.items() if k.startswith("vocoder.vocoder.")}, VOC_CFG)
    err = measure("vocoder AMP1 rel_l2", rel_l2(base.cpu(), ref_base))
    assert err < 3.5e-5, err         # measured 7.4e-6
    ref = R.vocoder_bwe_forward(mel, sd, VOC_CFG, BWE_CFG, dict(n_fft=512), 24000, 48000, 80)
    assert y.shape == ref.shape == (1, 2, 2 * 101 * 240)
    assert float(y.abs().max()) <= 1.0
    err = measure("vocoder BWE rel_l2", rel_l2(y.cpu(), ref))
    assert err < 4.5e-5, err         # measured 9.6e-6


def test_reference_golden_through_the_hip_path(tmp_path):
    """tests/golden/audio_vae_tiny.npz (the reference's own decoder and vocoders, tools/pin_audio_vae_against_reference.py) through the HIP
    models, their weights read by this package's loaders from a safetensors file in the checkpoints' names and layouts."""
    from safetensors.torch import save_file
    from ltx_2_mlx_amd.model.audio_vae import load_audio_decoder_weights, load_vocoder_weights, load_vocoder_with_bwe_weights
    from test_audio_vae_cpu import _tiny_models
    g = np.load(os.path.join(ROOT, "tests", "golden", "audio_vae_tiny.npz"))
    dec_w, voc_w, amp_w, bwe_w = R.tiny_weights()
    for name, sd in (("dec", dec_w), ("voc", voc_w), ("amp", amp_w), ("bwe", bwe_w)):
        save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / f"{name}.safetensors"))
    dec, voc, amp, vb = _tiny_models(DEV)
    load_audio_decoder_weights(dec, str(tmp_path / "dec.safetensors"))
    load_vocoder_weights(voc, str(tmp_path / "voc.safetensors"))
    load_vocoder_weights(amp, str(tmp_path / "amp.safetensors"))
    load_vocoder_with_bwe_weights(vb, str(tmp_path / "bwe.safetensors"))
    z, mel = torch.from_numpy(g["z"]).to(DEV), torch.from_numpy(g["mel"]).to(DEV)
    got = {"decoder": dec(z), "vocoder": voc(mel), "vocoder_amp": amp(mel), "vocoder_bwe": vb(mel)}
    torch.cuda.synchronize()
    for k, y in got.items():
        assert tuple(y.shape) == g[k].shape, k
        err = measure(f"golden {k}", rel_l2(y.cpu(), torch.from_numpy(g[k])))
        assert err < GOLDEN_GATES[k], (k, err)


GOLDEN_GATES = {"decoder": 4.4e-6, "vocoder": 2.8e-6, "vocoder_amp": 6.4e-6, "vocoder_bwe": 1.9e-5}     # measured 8.8e-7, 5.7e-7, 1.3e-6, 3.9e-6


# ------------------------------------------------------------------------------------------------------------------------ pipelines
def _write_audio_checkpoint(path, dec, voc):
    from safetensors.torch import save_file
    sd = {k: v.cpu().contiguous() for k, v in dec.state_dict().items()}
    sd.update({"vocoder." + k: v.cpu().contiguous().to(torch.bfloat16) for k, v in voc.state_dict().items()})
    save_file(sd, str(path))
    return sd


def test_one_stage_pipeline_returns_waveform(tmp_path):
    """OneStagePipeline(audio_decoder=, vocoder=) on an AudioVideo transformer returns the waveform in place of the latent."""
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder, Vocoder
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    model = generate.load_av_transformer(None, num_layers=2, compute_dtype=torch.bfloat16, use_fp8=False, low_memory=False, caption_channels=3840,
                                         cross_attention_adaln=False, apply_gated_attention=False, num_heads=2, seed=0, device=DEV)
    dec = AudioDecoder(device=DEV)
    dec.init_random_weights(1)
    voc = Vocoder(upsample_initial_channel=128, device=DEV)
    voc.init_random_weights(2)
    enc, _ = generate.create_dummy_text_encoding("a prompt", device=DEV)
    cfg = OneStageCFGConfig(height=256, width=256, num_frames=9, seed=1, fps=25.0, num_inference_steps=2, cfg_scale=1.0, audio_cfg_scale=1.0,
                            audio_enabled=True)
    plain = OneStagePipeline(model)
    _, latent = plain(enc, None, cfg, positive_audio_encoding=enc)
    _, wav = OneStagePipeline(model, audio_decoder=dec, vocoder=voc)(enc, None, cfg, positive_audio_encoding=enc)
    torch.cuda.synchronize()
    assert latent.dim() == 4 and latent.shape[1] == 8
    t = latent.shape[2]
    assert wav.shape == (1, 2, (4 * t - 3) * 240) and torch.isfinite(wav).all()
    ref = voc(dec(latent))
    measure("pipeline waveform vs decoders on the latent", rel_l2(wav, ref))
    assert torch.equal(wav, ref)     # the same kernels on the same latent: bit-identical (measured 0)


def test_generate_video_decodes_audio(tmp_path):
    """generate_video(generate_audio=True, decode_audio=True) on random weights writes the latent .npz and a stereo 16-bit .wav at the
    vocoder's rate; generate_video(weights_path=...) on a synthetic LTX-2.3 checkpoint that also carries audio_vae.* / vocoder.* tensors
    decodes them under decode_audio=None, and its .wav matches the restatement run on the same tensors and the saved latent."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    kw = dict(height=256, width=384, num_frames=17, num_steps=2, seed=3, num_layers=2, num_heads=2, vae_base_channels=64, use_gemma=False,
              generate_audio=True)
    generate.generate_video("a test prompt", output_path=str(tmp_path / "a.mp4"), decode_audio=True, **kw)
    lat = np.load(tmp_path / "a_audio_latent.npz")["latent"]
    with wave.open(str(tmp_path / "a.wav"), "rb") as f:
        assert f.getnchannels() == 2 and f.getsampwidth() == 2 and f.getframerate() == 24000
        assert f.getnframes() == (4 * lat.shape[2] - 3) * 240
    # decode_audio=None without a checkpoint: the latent only
    generate.generate_video("a test prompt", output_path=str(tmp_path / "b.mp4"), **kw)
    assert (tmp_path / "b_audio_latent.npz").exists() and not (tmp_path / "b.wav").exists()

    # a checkpoint that carries audio_vae.* / vocoder.* tensors is decoded under decode_audio=None through generate_video(weights_path=...)
    import json
    from safetensors.torch import save_file
    from oracle import dit_av, vae
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder, Vocoder
    blocks = [["res_x", {"num_layers": 1}], ["compress_all", {"multiplier": 2, "residual": True}], ["res_x", {"num_layers": 1}]]
    vw = vae.make_vae_weights(vae.VAEConfig(decoder_blocks=blocks, base_channels=32, timestep_conditioning=False), 5)
    cfg = dit_av.AVConfig(num_attention_heads=4, attention_head_dim=128, audio_heads=4, audio_head_dim=64, num_layers=2, caption_channels=None,
                          cross_attention_adaln=True, apply_gated_attention=True)
    tensors = {"model.diffusion_model." + k: v.contiguous() for k, v in dit_av.make_av_weights(cfg, seed=6).items()}
    tensors.update({k: v.contiguous() for k, v in vw.items()})
    dec = AudioDecoder(device="cpu")
    dec.init_random_weights(21)
    voc = Vocoder(device="cpu")
    voc.init_random_weights(22)
    sd = {k: v.contiguous() for k, v in dec.state_dict().items()}
    sd.update({"vocoder." + k: v.contiguous().to(torch.bfloat16) for k, v in voc.state_dict().items()})
    tensors.update(sd)
    ck = str(tmp_path / "av_audio.safetensors")
    save_file(tensors, ck, metadata={"model_version": "2.3.0", "config": json.dumps({"vae": {"decoder_blocks": blocks, "decoder_base_channels": 32,
                                                                                          "timestep_conditioning": False}})})
    assert generate.checkpoint_has_audio_decoders(ck)
    generate.generate_video("a test prompt", height=64, width=96, num_frames=9, num_steps=2, seed=3, weights_path=ck, use_gemma=False, num_layers=2,
                            num_heads=4, output_path=str(tmp_path / "c.mp4"), save_mp4=False, generate_audio=True)
    lat = np.load(tmp_path / "c_audio_latent.npz")["latent"]
    with wave.open(str(tmp_path / "c.wav"), "rb") as f:
        assert (f.getnchannels(), f.getframerate(), f.getnframes()) == (2, 24000, (4 * lat.shape[2] - 3) * 240)
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").reshape(-1, 2).T
    z = torch.from_numpy(lat)
    ref = R.vocoder_forward(R.decoder_forward(z, sd), {k[len("vocoder."):]: t for k, t in sd.items() if k.startswith("vocoder.")},
                            dict(resblock_kernel_sizes=[3, 7, 11], upsample_rates=[6, 5, 2, 2, 2], upsample_kernel_sizes=[16, 15, 8, 4, 4],
                                 resblock_dilation_sizes=[[1, 3, 5]] * 3))
    ref_pcm = (ref[0].numpy() * 32767).clip(-32768, 32767).astype(np.int16)             # the reference's int16 scaling
    measure("checkpoint decode (.wav) vs restatement, max |int16 diff|", np.abs(pcm.astype(np.int32) - ref_pcm).max())
    assert pcm.shape == ref_pcm.shape and np.abs(pcm.astype(np.int32) - ref_pcm).max() <= 1         # at most a rounding step apart
