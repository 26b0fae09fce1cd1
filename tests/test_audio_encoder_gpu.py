"""Audio VAE encoder on the MI355X: the strided convolution against exact integer arithmetic, the SiLU epilogue and the latent
normalisation against float64 / fp32 torch, AudioEncoder against the reference's own vector (tests/golden/audio_encoder_tiny.npz) and, at
production width, against the fp32 restatement (tests/audio_encoder_ref.py), the log-mel front end against its float64 definition, and
the frozen audio latent through OneStagePipeline's eager and captured loops.  Parity gates sit at <= 5x the value measured on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import measure, rel_l2  # noqa: E402

import audio_encoder_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ints(lo, hi, *shape, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _pearson(a, b):
    a, b = a.double().flatten() - a.double().mean(), b.double().flatten() - b.double().mean()
    return float((a @ b) / (a.norm() * b.norm()))


def _strided(x, w, b, stride, res=None, act=0):
    """x (C, H, W), w (O, C, 3, 3) on the host -> the kernel's (O, H_out, W_out) on the host"""
    from ltx_2_mlx_amd import kernels as K
    y = K.audio_conv2d_strided(x.permute(1, 2, 0).contiguous().to(DEV), K.pack_conv_weight(w.to(DEV)), None if b is None else b.to(DEV), w.shape[0], 3, 3,
                               2, 1, stride=stride, res=None if res is None else res.permute(1, 2, 0).contiguous().to(DEV), act=act)
    torch.cuda.synchronize()
    return y.permute(2, 0, 1).cpu()


def _ref64(x, w, b, stride, res=None):
    y = F.conv2d(F.pad(x.double()[None], (1, 1, 2, 0)), w.double(), None if b is None else b.double(), stride=stride)[0]      # encoder.py:23-33
    return y if res is None else y + res.double()


SHAPES = [(1, 1), (2, 3), (5, 4), (7, 64), (34, 6), (33, 9)]          # odd / even on both axes, one pixel, M across the 64- and 128-row tiles
C_IN = [2, 6, 8, 128]                                                    # scalar and vector operand loads, K = 54 not a multiple of 16
C_OUT = [3, 16, 40, 130]                                                 # every N tile width, a ragged last tile


@pytest.mark.parametrize("stride", [(2, 2), (2, 1), (1, 2)])
@pytest.mark.parametrize("hw", SHAPES)
def test_strided_conv_is_exact_on_integers(hw, stride):
    """Integer inputs in [-4, 4], weights in [-3, 3] (bias and residual too): every partial sum is an integer below 2^24
    (K <= 9 * 128 taps x 12), so the fp32 MFMA result must EQUAL float64 F.conv2d of the padded image at that stride."""
    h, w = hw
    ho, wo = (h - 1) // stride[0] + 1, (w - 1) // stride[1] + 1
    n = 0
    for ci in C_IN:
        for co in C_OUT:
            x = _ints(-4, 4, ci, h, w, seed=ci + 7 * co)
            wt = _ints(-3, 3, co, ci, 3, 3, seed=co + 11 * ci)
            bias, res = _ints(-4, 4, co, seed=3), _ints(-4, 4, co, ho, wo, seed=4)
            for b, r in ((bias, res), (None, None), (bias, None), (None, res)):
                y = _strided(x, wt, b, stride, r)
                ref = _ref64(x, wt, b, stride, r)
                assert y.shape == (co, ho, wo)
                assert torch.equal(y.double(), ref), (ci, co, b is not None, r is not None, float((y.double() - ref).abs().max()))
                n += 1
    assert n == 64


@pytest.mark.parametrize("hw", SHAPES)
def test_stride_one_equals_audio_conv2d_bit_for_bit(hw):
    from ltx_2_mlx_amd import kernels as K
    h, w = hw
    for ci, co in ((2, 3), (6, 40), (8, 16), (128, 130)):
        x = _rand(h, w, ci, seed=h + ci).to(DEV)
        wt = K.pack_conv_weight(_rand(co, ci, 3, 3, seed=co, scale=(9 * ci) ** -0.5).to(DEV))
        b, res = _rand(co, seed=1, scale=0.1).to(DEV), _rand(h, w, co, seed=2).to(DEV)
        for bb, rr in ((b, res), (None, None)):
            assert torch.equal(K.audio_conv2d_strided(x, wt, bb, co, 3, 3, 2, 1, stride=(1, 1), res=rr), K.audio_conv2d(x, wt, bb, co, 3, 3, 2, 1, res=rr))


@pytest.mark.parametrize("ci,co", [(2, 16), (6, 40), (8, 130), (128, 128)])
def test_strided_conv_random_floats(ci, co):
    """One random-float case per operand path (scalar loads: c_in 2 and 6; vector loads: 8 and 128) at stride (2, 2), under the bound
    of the stride-1 audio conv test (tests/test_audio_vae_gpu.py: rel-L2 < 3.5e-6)."""
    x = _rand(ci, 33, 21, seed=ci)
    wt = _rand(co, ci, 3, 3, seed=co, scale=(9 * ci) ** -0.5)
    b, res = _rand(co, seed=5, scale=0.1), _rand(co, 17, 11, seed=6)
    err = rel_l2(_strided(x, wt, b, (2, 2), res), _ref64(x, wt, b, (2, 2), res))
    assert err < 3.5e-6, err         # measured 6.3e-8 - 4.1e-7


def test_strided_entry_rejects_bad_arguments():
    from ltx_2_mlx_amd import _native as nv
    from ltx_2_mlx_amd import kernels as K
    x, w = torch.zeros(4, 4, 8, device=DEV), torch.zeros(72, 8, device=DEV)
    y2 = torch.zeros(2, 2, 8, device=DEV)
    with pytest.raises(ValueError, match="stride_h"):
        nv.check(nv.lib().ltx2_audio_conv2d_strided(nv.ptr(x), 8, 4, 4, 8, nv.ptr(w), 8, None, nv.ptr(y2), 8, 2, 2, 8, 3, 3, 0, 2, 2, 1, None, 0, 0, nv.stream()))
    with pytest.raises(ValueError, match="act"):
        K.audio_conv2d_strided(x, w, None, 8, 3, 3, 2, 1, stride=(2, 2), act=nv.AUDIO_ACT_TANH)
    y = torch.zeros(4, 2, 8, device=DEV)
    with pytest.raises(ValueError, match="reach past"):          # 4 output rows at stride 2 would start beyond the 4 input rows
        nv.check(nv.lib().ltx2_audio_conv2d_strided(nv.ptr(x), 8, 4, 4, 8, nv.ptr(w), 8, None, nv.ptr(y), 8, 4, 2, 8, 3, 3, 2, 2, 2, 1, None, 0, 0, nv.stream()))
    with pytest.raises(ValueError, match=r"act 4 \(0\.\.3\)"):     # ltx2_audio_conv keeps its own argument checks
        nv.check(nv.lib().ltx2_audio_conv(nv.ptr(x), 8, 4, 4, 8, nv.ptr(w), 8, None, nv.ptr(y), 8, 4, 4, 8, 3, 3, 1, 1, 2, 1, 0, 0, 0.0, None, 0, 1.0, 0.0, 4,
                                          nv.stream()))
    with pytest.raises(ValueError, match="audio_latent_normalize"):
        nv.check(nv.lib().ltx2_audio_latent_normalize(nv.ptr(x), 1, nv.ptr(x), nv.ptr(x), nv.ptr(y), 4, 4, 8, nv.stream()))


def test_silu_epilogue_against_float64():
    """silu(bias + res + conv) in the conv's epilogue on one 3 x 5 image, c = 12.  Inputs are dyadic (multiples of 1/4, weights in
    {-1, 0, 1}), so the pre-activation v is exact in fp32 and the whole error is the epilogue's v * (1 / (1 + expf(-v))): one expf
    (<= 1 ulp = 2u relative, u = 2^-24), one add, one divide and one multiply (<= u each): |y - silu(v)| <= 5u |silu(v)|; gated at 6u,
    plus the smallest normal fp32 where silu(v) underflows for very negative v."""
    from ltx_2_mlx_amd import _native as nv
    c = 12
    x = _ints(-8, 8, c, 3, 5, seed=1) / 4
    wt = _ints(-1, 1, c, c, 3, 3, seed=2)
    b, res = _ints(-4, 4, c, seed=3) / 4, _ints(-8, 8, c, 3, 5, seed=4) / 4
    v = _ref64(x, wt, b, (1, 1), res)
    assert torch.equal(_strided(x, wt, b, (1, 1), res).double(), v)                  # the pre-activation is exact
    y = _strided(x, wt, b, (1, 1), res, act=nv.AUDIO_ACT_SILU).double()
    ref = v * torch.sigmoid(v)
    u = 2.0 ** -24
    worst = float(((y - ref).abs() / ref.abs().clamp_min(1.2e-38)).max())
    measure("silu epilogue, max relative error / u", worst / u)          # measured 1.55 u
    assert float(v.abs().max()) > 4 and float(v.abs().min()) < 1                      # both tails and the middle of the sigmoid are hit
    assert bool(((y - ref).abs() <= 6 * u * ref.abs() + 1.2e-38).all()), worst / u


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("z", [2, 8])
@pytest.mark.parametrize("f", [4, 16])
@pytest.mark.parametrize("t", [1, 5])
def test_latent_normalize_equals_torch(t, f, z, wide):
    """(h[t, f, c] - mean[c * F + f]) / std[c * F + f] equals fp32 CPU torch bit for bit: ld = z and 2z (double_z), a std that is no power
    of two, statistics that differ at every index (a c * F + f / f * z + c swap changes the result)."""
    from ltx_2_mlx_amd import kernels as K
    ld = 2 * z if wide else z
    h = _rand(t, f, ld, seed=t + f + z, scale=3.0)
    i = torch.arange(z * f, dtype=torch.float32)
    mean, std = 0.37 * i - 1.3, 0.7 + 0.013 * i
    y = K.audio_latent_normalize(h.to(DEV), mean.to(DEV), std.to(DEV), z)
    torch.cuda.synchronize()
    ref = (h[:, :, :z].permute(2, 0, 1) - mean.view(z, 1, f)) / std.view(z, 1, f)
    assert y.shape == (z, t, f) and torch.equal(y.cpu(), ref)
    # the restatement's patchify -> normalize -> unpatchify is the same thing
    assert torch.equal(R.normalize_latents(h.permute(2, 0, 1)[None], mean, std, z)[0], ref)
    swapped = (h[:, :, :z].permute(2, 0, 1) - mean.view(f, z).t().reshape(z, 1, f)) / std.view(z, 1, f)
    assert not torch.equal(swapped, ref)


# ------------------------------------------------------------------------------------------------------------------------ model
GATE_TINY, GATE_FULL, GATE_LOGMEL = 2.1e-6, 1.0e-5, 1.3e-5          # <= 5x the values measured on the MI355X (beside each assertion)


def test_tiny_encoder_matches_the_reference_golden(tmp_path):
    """tests/golden/audio_encoder_tiny.npz (the reference's own AudioEncoder, tools/pin_audio_encoder_against_reference.py) through the
    HIP encoder, its weights read by load_audio_encoder_weights from a safetensors file in the reference loader's key spelling."""
    from safetensors.torch import save_file
    from ltx_2_mlx_amd.model.audio_vae import encode_audio, load_audio_encoder_weights
    from test_audio_encoder_cpu import _tiny_encoder
    g = np.load(os.path.join(ROOT, "tests", "golden", "audio_encoder_tiny.npz"))
    save_file({k: v.contiguous() for k, v in R.tiny_weights().items()}, str(tmp_path / "enc.safetensors"))
    enc = _tiny_encoder(DEV)
    load_audio_encoder_weights(enc, str(tmp_path / "enc.safetensors"))
    y = encode_audio(torch.from_numpy(g["mel"]).to(DEV), enc)
    torch.cuda.synchronize()
    assert tuple(y.shape) == g["latent"].shape == (1, 2, 4, 4) and y.dtype == torch.float32
    err = measure("golden encoder", rel_l2(y.cpu(), torch.from_numpy(g["latent"])))
    assert err < GATE_TINY, err          # measured 4.2e-7


@pytest.fixture(scope="module")
def full_encoder():
    from ltx_2_mlx_amd.model.audio_vae import AudioEncoder
    enc = AudioEncoder(device=DEV)
    enc.init_random_weights(5)
    return enc, {k: v.cpu() for k, v in enc.state_dict().items()}


@pytest.mark.parametrize("t_mel", [21, 22])
def test_full_width_encoder_matches_restatement(full_encoder, t_mel):
    """Production AudioEncoder (ch 128, mult (1, 2, 4), 3 blocks per level) on 21 and 22 mel frames x 64 bins: both parities through both
    downsamples (21 -> 11 -> 6, 22 -> 11 -> 6); two encodes of the same input are bit-identical."""
    enc, sd = full_encoder
    mel = _rand(1, 2, t_mel, 64, seed=t_mel, scale=2.0)
    y = enc(mel.to(DEV))
    y2 = enc(mel.to(DEV))
    torch.cuda.synchronize()
    ref = R.encoder_forward(mel, sd)
    assert y.shape == ref.shape == (1, 8, enc.output_frames(t_mel), 16) and y.dtype == torch.float32
    assert torch.equal(y, y2)
    err = measure(f"encoder T_mel {t_mel} rel_l2", rel_l2(y.cpu(), ref))
    p = measure(f"encoder T_mel {t_mel} pearson", _pearson(y.cpu(), ref))
    assert err < GATE_FULL and p > 0.999, (err, p)          # measured 2.02e-6 (21) / 2.03e-6 (22), Pearson 1.000000


def test_decoder_of_encoder_keeps_the_mel_shape(full_encoder):
    from ltx_2_mlx_amd.model.audio_vae import AudioDecoder
    enc, _ = full_encoder
    dec = AudioDecoder(device=DEV)
    dec.init_random_weights(6)
    for t in (1, 6):
        mel = _rand(1, 2, 4 * t - 3, 64, seed=t).to(DEV)
        z = enc(mel)
        assert z.shape == (1, 8, t, 16) and dec(z).shape == mel.shape


@pytest.mark.parametrize("channels", [1, 2])
def test_log_mel_matches_the_float64_definition(channels):
    """AudioProcessor.waveform_to_mel against the float64 numpy definition on 0.3 s of seeded noise (amplitude 0.1) plus a 440 Hz sine:
    the mel energies sit far above the 1e-5 clamp, so every element is compared.  Absolute error in the log domain."""
    from ltx_2_mlx_amd.model.audio_vae import AudioProcessor
    rs = np.random.RandomState(7)
    n = 4800
    t = np.arange(n) / 16000.0
    w = np.stack([0.1 * rs.randn(n) + 0.5 * np.sin(2 * np.pi * 440.0 * t + 0.3 * c) for c in range(channels)]).astype(np.float32)
    ref = R.log_mel_f64(w)
    assert ref.shape == (1, 2, 31, 64) and float(ref.min()) > np.log(1e-5) + 3
    y = AudioProcessor(device=DEV).waveform_to_mel(w, 16000)
    torch.cuda.synchronize()
    assert y.shape == (1, 2, 31, 64) and y.dtype == torch.float32
    if channels == 1:
        assert torch.equal(y[0, 0], y[0, 1])
    err = measure(f"log-mel {channels}ch max |log diff|", float((y.cpu().double() - torch.from_numpy(ref)).abs().max()))
    assert err < GATE_LOGMEL, err          # measured 2.7e-6 (mono and stereo)


# ------------------------------------------------------------------------------------------------------------------------ loop
def test_frozen_audio_latent_through_both_loops(dev):
    """OneStagePipeline(initial_audio_latent=) on the smallest AudioVideo test transformer, 4 steps: the returned audio latent IS the input,
    eager and captured; the two loops' video latents are bit-identical; another audio latent gives another video; None changes nothing."""
    from test_parity import make_av
    from ltx_2_mlx_amd.pipelines import OneStageCFGConfig, OneStagePipeline
    from ltx_2_mlx_amd.types import AudioLatentShape
    _, _, _, m = make_av(dev, False, seed=23)
    H, W, Fr, S = 64, 96, 9, 24
    g = torch.Generator().manual_seed(31)
    noise = torch.randn(1, 2 * 2 * 3, 128, generator=g).to(dev)
    anoise = torch.randn(1, 9, 128, generator=g).to(dev)
    vctx, actx = (0.1 * torch.randn(1, S, 64, generator=g)).to(dev), (0.1 * torch.randn(1, S, 64, generator=g)).to(dev)
    ta = AudioLatentShape.from_duration(1, Fr / 25.0).frames
    a1, a2 = torch.randn(1, 8, ta, 16, generator=g).to(dev), torch.randn(1, 8, ta, 16, generator=g).to(dev)
    kw = dict(height=H, width=W, num_frames=Fr, seed=1, fps=25.0, num_inference_steps=4, cfg_scale=1.0, audio_cfg_scale=1.0, rescale_scale=0.0)
    pipe = OneStagePipeline(m, None, None)

    def run(graph, **extra):
        out = pipe(vctx, None, OneStageCFGConfig(use_hip_graph=graph, **kw), positive_audio_encoding=actx, initial_noise=noise, **extra)
        torch.cuda.synchronize()
        return out

    lat_e, aud_e = run(False, initial_audio_latent=a1)
    lat_g, aud_g = run(True, initial_audio_latent=a1)
    assert aud_e.shape == a1.shape and torch.equal(aud_e, a1) and torch.equal(aud_g, a1)
    measure("frozen audio: graph vs eager video latent rel_l2", rel_l2(lat_g.cpu(), lat_e.cpu()))
    assert torch.equal(lat_g, lat_e)
    assert torch.isfinite(lat_e).all()
    for graph in (False, True):
        lat_o, aud_o = run(graph, initial_audio_latent=a2)
        measure("frozen audio: another audio latent, video latent rel_l2", rel_l2(lat_o.cpu(), lat_e.cpu()))
        assert torch.equal(aud_o, a2) and not torch.equal(lat_o, lat_e)                  # the video listens to the audio
    with pytest.raises(ValueError, match="does not match"):
        run(False, initial_audio_latent=a1[:, :, :-1])
    # initial_audio_latent=None: the call as it was, same seeds -> same result (audio noised and denoised, returned only when enabled)
    base_lat, base_aud = run(False, initial_audio_noise=anoise)
    none_lat, none_aud = run(False, initial_audio_noise=anoise, initial_audio_latent=None)
    assert base_aud is None and none_aud is None and torch.equal(base_lat, none_lat)
    assert not torch.equal(base_lat, lat_e)


def test_generate_video_to_an_audio_file(tmp_path):
    """generate_video(generate_audio=True, audio_path=...) on random weights: a 0.4 s mono 8 kHz wav is resampled, padded with silence to the
    video's 17 / 25 s, encoded and kept frozen: `<stem>_audio_latent.npz` holds exactly what encode_audio_for_video gives for that file."""
    import wave
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import generate
    pcm = (8000 * np.sin(2 * np.pi * 330.0 * np.arange(3200) / 8000.0)).astype("<i2")
    with wave.open(str(tmp_path / "in.wav"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes(pcm.tobytes())
    frames = generate.generate_video("a test prompt", height=256, width=384, num_frames=17, num_steps=2, seed=3, num_layers=2, num_heads=2,
                                     vae_base_channels=64, use_gemma=False, generate_audio=True, audio_path=str(tmp_path / "in.wav"),
                                     output_path=str(tmp_path / "a.mp4"), save_mp4=False)
    assert frames.shape == (17, 256, 384, 3)
    lat = np.load(tmp_path / "a_audio_latent.npz")["latent"]
    want, wav, sr = generate.encode_audio_for_video(str(tmp_path / "in.wav"), 17, 25.0, None, seed=3 + 5)
    assert lat.shape == (1, 8, 17, 16) and np.isfinite(lat).all() and np.array_equal(lat, want.cpu().numpy())
    assert sr == 16000 and wav.shape == (1, 10880) and float(np.abs(wav[:, 6400:]).max()) == 0.0 and float(np.abs(wav[:, :6400]).max()) > 0.2
