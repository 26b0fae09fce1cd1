"""fp32 CPU restatement of the reference's audio VAE encoder (LTX_2_MLX/model/audio_vae/encoder.py, with decoder.py's CausalConv2d,
PixelNorm and SimpleResBlock2d) in plain torch, on checkpoint-named state dicts in PyTorch layouts and the reference loader's key
spelling (`audio_vae.encoder.conv_in.weight`, encoder.py:206-303); and a float64 numpy log-mel written from its definition (centred
reflect-padded frames, periodic Hann window, |rfft|, Slaney mel filterbank, log with the 1e-5 clamp).  The HIP path is checked against
both."""
import math

import numpy as np
import torch
import torch.nn.functional as F

ENC = "audio_vae.encoder."
MEAN = ENC + "per_channel_statistics.mean-of-means"
STD = ENC + "per_channel_statistics.std-of-means"


def causal_conv2d(x, w, b=None, stride=1):
    """CausalConv2d, CausalityAxis.HEIGHT (decoder.py:84-147): k - 1 rows on top, (k - 1) / 2 columns each side, then the stride."""
    p = w.shape[-1] - 1
    return F.conv2d(F.pad(x, (p // 2, p - p // 2, p, 0)), w, b, stride=stride)


def _conv(x, sd, name, stride=1):
    return causal_conv2d(x, sd[ENC + name + ".weight"].float(), sd[ENC + name + ".bias"].float(), stride)


def pixnorm_silu(x, eps=1e-6):
    return F.silu(x / torch.sqrt(torch.mean(x * x, dim=1, keepdim=True) + eps))          # PixelNorm (decoder.py:27-53) + silu


def _resblock2d(x, sd, pre, cin, cout):
    """SimpleResBlock2d (decoder.py:150-208)"""
    h = _conv(pixnorm_silu(x), sd, f"{pre}.conv1")
    h = _conv(pixnorm_silu(h), sd, f"{pre}.conv2")
    if cin != cout:
        x = _conv(x, sd, f"{pre}.nin_shortcut")
    return x + h


def normalize_latents(h, mean, std, z):
    """encoder.py:172-203: the mean half, patchify (B, C, T, F) -> (B, T, C * F), (x - mean) / std, unpatchify."""
    m = h[:, :z]
    b, c, t, f = m.shape
    p = m.permute(0, 2, 1, 3).reshape(b, t, c * f)
    return ((p - mean.float()) / std.float()).reshape(b, t, c, f).permute(0, 2, 1, 3)


def encoder_forward(mel, sd, ch=128, ch_mult=(1, 2, 4), num_res_blocks=3, z_channels=8):
    """mel (B, 2, T, n_mels) -> (B, z, T_a, n_mels / 4), AudioEncoder.__call__ (encoder.py:127-170)."""
    h = _conv(mel.float(), sd, "conv_in")
    block_in = ch
    for lvl in range(len(ch_mult)):
        block_out = ch * ch_mult[lvl]
        for i in range(num_res_blocks):
            h = _resblock2d(h, sd, f"down.{lvl}.block.{i}", block_in, block_out)
            block_in = block_out
        if lvl != len(ch_mult) - 1:
            h = _conv(h, sd, f"down.{lvl}.downsample.conv", stride=2)          # Downsample2d (encoder.py:23-33)
    base = ch * ch_mult[-1]
    h = _resblock2d(h, sd, "mid.block_1", base, base)
    h = _resblock2d(h, sd, "mid.block_2", base, base)
    h = _conv(F.silu(h), sd, "conv_out")                                        # encoder.py:159-161: silu, no norm
    return normalize_latents(h, sd[MEAN], sd[STD], z_channels)


def make_encoder_weights(ch, ch_mult, num_res_blocks, z_channels, in_ch=2, seed=0, double_z=True):
    """Checkpoint-named, PyTorch-layout AudioEncoder weights in the reference loader's spelling, with non-trivial statistics."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, co, ci, k):
        sd[ENC + name + ".weight"] = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
        sd[ENC + name + ".bias"] = 0.1 * torch.randn(co, generator=g)

    conv("conv_in", ch, in_ch, 3)
    block_in = ch
    for lvl in range(len(ch_mult)):
        block_out = ch * ch_mult[lvl]
        for i in range(num_res_blocks):
            conv(f"down.{lvl}.block.{i}.conv1", block_out, block_in, 3)
            conv(f"down.{lvl}.block.{i}.conv2", block_out, block_out, 3)
            if block_in != block_out:
                conv(f"down.{lvl}.block.{i}.nin_shortcut", block_out, block_in, 1)
            block_in = block_out
        if lvl != len(ch_mult) - 1:
            conv(f"down.{lvl}.downsample.conv", block_out, block_out, 3)
    base = ch * ch_mult[-1]
    for b in ("mid.block_1", "mid.block_2"):
        conv(b + ".conv1", base, base, 3)
        conv(b + ".conv2", base, base, 3)
    conv("conv_out", 2 * z_channels if double_z else z_channels, base, 3)
    sd[MEAN] = 0.3 * torch.randn(ch, generator=g)
    sd[STD] = 0.7 + 0.6 * torch.rand(ch, generator=g)
    return sd


# the tiny configuration of tests/golden/audio_encoder_tiny.npz (tools/pin_audio_encoder_against_reference.py): statistics of
# ch = z_channels * mel_bins = 8 entries, an odd T_mel (13 -> 7 -> 4), 16 mel bins (-> 8 -> 4)
TINY_ENCODER = dict(ch=8, ch_mult=(1, 2, 4), num_res_blocks=1, z_channels=2)
TINY_MEL_BINS = 4
TINY_SEED = 8642


def tiny_weights():
    return make_encoder_weights(seed=TINY_SEED, **TINY_ENCODER)


def tiny_input():
    g = torch.Generator().manual_seed(TINY_SEED + 1)
    return torch.randn(1, 2, 13, 16, generator=g)


# ---------------------------------------------------------------------------------------------------------------- log-mel, float64
def _hz_to_mel(f):
    """Slaney scale: 200 / 3 Hz per mel below 1 kHz, then ln(6.4) / 27 per mel."""
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _mel_to_hz(m):
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max):
    """(n_mels, n_fft / 2 + 1) float64, written entry by entry: triangle m rises from edge m to edge m + 1 and falls to edge m + 2 (edges
    equally spaced in mel), scaled by 2 / (edge m + 2 - edge m) (Slaney's area normalisation)."""
    lo, hi = _hz_to_mel(f_min), _hz_to_mel(f_max)
    edges = [_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    fb = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        a, b, c = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sample_rate / n_fft
            fb[m, k] = max(0.0, min((f - a) / (b - a), (c - f) / (c - b))) * 2.0 / (c - a)
    return fb


def log_mel_f64(waveform, sample_rate=16000, n_fft=1024, win_length=1024, hop_length=160, n_mels=64, f_min=0.0, f_max=8000.0):
    """waveform [C, samples] -> (1, 2, 1 + samples // hop, n_mels) float64; mono is duplicated."""
    w = np.asarray(waveform, dtype=np.float64)
    n = np.arange(win_length)
    win = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    win[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
    fb = mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max)
    out = []
    for c in range(w.shape[0]):
        y = np.pad(w[c], n_fft // 2, mode="reflect")
        frames = 1 + w.shape[1] // hop_length
        spec = np.stack([np.abs(np.fft.rfft(y[t * hop_length:t * hop_length + n_fft] * win)) for t in range(frames)])
        out.append(np.log(np.maximum(spec @ fb.T, 1e-5)))
    if len(out) == 1:
        out = out * 2
    return np.stack(out)[None]
