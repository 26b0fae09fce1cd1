"""fp32 CPU restatement of the reference's audio VAE decoder and vocoders (LTX_2_MLX/model/audio_vae/decoder.py, vocoder.py) in plain
torch, on checkpoint-named state dicts in PyTorch layouts.  It follows the reference's composition step by step (pads, slices, the
stack-and-mean, the leaky-relu slopes); the HIP path is checked against it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

DEC = "audio_vae.decoder."


# ---------------------------------------------------------------------------------------------------------------- decoder
def _causal_conv2d(x, sd, name, k):
    p = k - 1
    x = F.pad(x, (p // 2, p - p // 2, p, 0))                 # width symmetric, height (time) causal: decoder.py:84-147
    return F.conv2d(x, sd[DEC + name + ".weight"].float(), sd[DEC + name + ".bias"].float())


def _pixnorm_silu(x, eps=1e-6):
    return F.silu(x / torch.sqrt(torch.mean(x * x, dim=1, keepdim=True) + eps))


def _resblock2d(x, sd, pre, cin, cout):
    h = _causal_conv2d(_pixnorm_silu(x), sd, f"{pre}.conv1.conv", 3)
    h = _causal_conv2d(_pixnorm_silu(h), sd, f"{pre}.conv2.conv", 3)
    if cin != cout:
        x = _causal_conv2d(x, sd, f"{pre}.nin_shortcut.conv", 1)
    return x + h


def decoder_forward(sample, sd, ch=128, out_ch=2, ch_mult=(1, 2, 4), num_res_blocks=3):
    """sample (B, z, T, F) -> (B, out_ch, 4T - 3, 4F), AudioDecoder.__call__ (decoder.py:362-424)."""
    x = sample.float()
    b, c, t, f = x.shape
    mean = sd["audio_vae.per_channel_statistics.mean-of-means"].float()
    std = sd["audio_vae.per_channel_statistics.std-of-means"].float()
    x = (x.permute(0, 2, 1, 3).reshape(b, t, c * f) * std + mean).reshape(b, t, c, f).permute(0, 2, 1, 3)
    base = ch * ch_mult[-1]
    h = _causal_conv2d(x, sd, "conv_in.conv", 3)
    h = _resblock2d(h, sd, "mid.block_1", base, base)
    h = _resblock2d(h, sd, "mid.block_2", base, base)
    block_in = base
    for lvl in reversed(range(len(ch_mult))):
        block_out = ch * ch_mult[lvl]
        for i in range(num_res_blocks):
            h = _resblock2d(h, sd, f"up.{lvl}.block.{i}", block_in, block_out)
            block_in = block_out
        if lvl != 0:
            h = h.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
            h = _causal_conv2d(h, sd, f"up.{lvl}.upsample.conv.conv", 3)[:, :, 1:, :]
    h = _causal_conv2d(_pixnorm_silu(h), sd, "conv_out.conv", 3)
    return h[:, :out_ch, :max(4 * t - 3, 1), :4 * f]


# ---------------------------------------------------------------------------------------------------------------- vocoder
def _upsample1d(x, filt, ratio, pad, pad_left, pad_right):
    c = x.shape[1]
    k = filt.numel()
    x = F.pad(x, (pad, pad), mode="replicate")
    y = ratio * F.conv_transpose1d(x, filt.reshape(1, 1, k).expand(c, 1, k).float(), stride=ratio, groups=c)
    return y[:, :, pad_left:y.shape[2] - pad_right]


def _snake_aa(x, sd, pre):
    """Activation1d(SnakeBeta): UpSample1d(2, 12) -> SnakeBeta -> DownSample1d(2, 12) (vocoder.py:162-412)."""
    fu = sd[pre + ".upsample.filter"].reshape(-1).float()
    fd = sd[pre + ".downsample.lowpass.filter"].reshape(-1).float()
    ku, kd = fu.numel(), fd.numel()
    p = ku // 2 - 1
    y = _upsample1d(x, fu, 2, p, p * 2 + (ku - 2) // 2, p * 2 + (ku - 2 + 1) // 2)
    a = torch.exp(sd[pre + ".act.alpha"].float())[None, :, None]
    bt = torch.exp(sd[pre + ".act.beta"].float())[None, :, None]
    y = y + (1.0 / (bt + 1e-9)) * torch.sin(y * a) ** 2
    even = kd % 2 == 0
    y = F.pad(y, (kd // 2 - int(even), kd // 2), mode="replicate")
    c = y.shape[1]
    return F.conv1d(y, fd.reshape(1, 1, kd).expand(c, 1, kd), stride=2, groups=c)


def _conv1d(x, sd, name, k, dilation=1):
    return F.conv1d(x, sd[name + ".weight"].float(), sd[name + ".bias"].float(), padding=(k - 1) * dilation // 2, dilation=dilation)


def vocoder_forward(mel, sd, cfg):
    """Vocoder.__call__ (vocoder.py:748-809).  sd: vocoder-relative names; cfg: dict of the Vocoder constructor's values."""
    rk, ur, uk, rd = cfg["resblock_kernel_sizes"], cfg["upsample_rates"], cfg["upsample_kernel_sizes"], cfg["resblock_dilation_sizes"]
    amp = cfg.get("resblock", "1") == "AMP1"
    x = mel.float().transpose(2, 3)
    b, s, m, t = x.shape
    x = _conv1d(x.reshape(b, s * m, t), sd, "conv_pre", 7)
    nk = len(rk)
    for i, (rate, k) in enumerate(zip(ur, uk)):
        if not amp:
            x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, sd[f"ups.{i}.weight"].float(), sd[f"ups.{i}.bias"].float(), stride=rate, padding=(k - rate) // 2)
        outs = []
        for j, (k2, dil) in enumerate(zip(rk, rd)):
            pre = f"resblocks.{i * nk + j}"
            h = x
            for d_i, d in enumerate(dil):
                if amp:
                    xt = _snake_aa(h, sd, f"{pre}.acts1.{d_i}")
                    xt = _conv1d(xt, sd, f"{pre}.convs1.{d_i}", k2, d)
                    xt = _snake_aa(xt, sd, f"{pre}.acts2.{d_i}")
                    xt = _conv1d(xt, sd, f"{pre}.convs2.{d_i}", k2)
                else:
                    xt = _conv1d(F.leaky_relu(h, 0.1), sd, f"{pre}.convs1.{d_i}", k2, d)
                    xt = _conv1d(F.leaky_relu(xt, 0.1), sd, f"{pre}.convs2.{d_i}", k2)
                h = xt + h
            outs.append(h)
        x = torch.stack(outs, 0).mean(0)
    x = _snake_aa(x, sd, "act_post") if amp else F.leaky_relu(x, 0.01)
    x = _conv1d(x, sd, "conv_post", 7)
    if cfg.get("apply_final_activation", True):
        x = torch.tanh(x) if cfg.get("use_tanh_at_final", True) else torch.clamp(x, -1, 1)
    return x


def hann_filter(ratio, rolloff=0.99, lowpass_filter_width=6):
    width = math.ceil(lowpass_filter_width / rolloff)
    ks = 2 * width * ratio + 1
    ta = np.arange(ks) / ratio - width
    tr = ta * rolloff
    window = np.cos(np.clip(tr, -lowpass_filter_width, lowpass_filter_width) * math.pi / lowpass_filter_width / 2) ** 2
    sinc = np.where(tr == 0, 1.0, np.sin(np.pi * tr) / np.where(tr == 0, 1.0, np.pi * tr))
    return torch.from_numpy((sinc * window * rolloff / ratio).astype(np.float32)), width, ks


def log_mel(y, forward_basis, mel_basis, n_fft, hop, win):
    """MelSTFT.mel_spectrogram's log-mel (vocoder.py:477-551): y (B, T) -> (B, n_mels, frames)."""
    y = F.pad(y[:, None, :].float(), (max(0, win - hop), 0))
    spec = F.conv1d(y, forward_basis.float(), stride=hop)
    nf = spec.shape[1] // 2
    mag = torch.sqrt(spec[:, :nf] ** 2 + spec[:, nf:] ** 2)
    return torch.log(torch.clamp(torch.einsum("mf,bft->bmt", mel_basis.float(), mag), min=1e-5))


def vocoder_bwe_forward(mel, sd, voc_cfg, bwe_cfg, stft_cfg, in_rate, out_rate, hop):
    """VocoderWithBWE.__call__ (vocoder.py:596-652).  sd: checkpoint names (vocoder.vocoder.…, vocoder.bwe_generator.…, vocoder.mel_stft.…)."""
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}          # noqa: E731
    x = vocoder_forward(mel, sub("vocoder.vocoder."), voc_cfg)
    length = x.shape[2]
    out_len = length * out_rate // in_rate
    if length % hop:
        x = F.pad(x, (0, hop - length % hop))
    b, c, t = x.shape
    lm = log_mel(x.reshape(b * c, t), sd["vocoder.mel_stft.stft_fn.forward_basis"], sd["vocoder.mel_stft.mel_basis"], stft_cfg["n_fft"], hop,
                 stft_cfg["n_fft"])
    lm = lm.reshape(b, c, lm.shape[1], lm.shape[2]).transpose(2, 3)
    residual = vocoder_forward(lm, sub("vocoder.bwe_generator."), dict(bwe_cfg, apply_final_activation=False))
    ratio = out_rate // in_rate
    filt, width, ks = hann_filter(ratio)
    skip = _upsample1d(x, filt, ratio, width, 2 * width * ratio, ks - ratio)
    return torch.clamp(residual + skip, -1, 1)[:, :, :out_len]


# ---------------------------------------------------------------------------------------------------------------- helpers
def dft_basis(n_fft):
    """A real Hann-windowed DFT basis in the checkpoint's forward_basis layout (2 * (n_fft / 2 + 1), 1, n_fft): real rows, then imaginary."""
    nf = n_fft // 2 + 1
    n = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
    ang = 2 * np.pi * np.arange(nf)[:, None] * n[None, :] / n_fft
    return torch.from_numpy(np.concatenate([np.cos(ang) * win, -np.sin(ang) * win])[:, None, :].astype(np.float32))


def mel_filterbank(n_mels, nf, seed=0):
    """A non-negative triangular-ish (n_mels, nf) basis: the test's stand-in for the checkpoint's mel_basis."""
    g = torch.Generator().manual_seed(seed)
    centers = torch.linspace(0, nf - 1, n_mels + 2)
    f = torch.arange(nf, dtype=torch.float32)
    tri = torch.clamp(1 - (f[None, :] - centers[1:-1, None]).abs() / (centers[1] - centers[0]), min=0)
    return tri * (1 + 0.1 * torch.rand(n_mels, 1, generator=g))


# ---------------------------------------------------------------------------------------------------------------- seeded weights
def _kaiser12():
    """UpSample1d(2, 12) / DownSample1d(2, 12)'s kaiser-sinc filter (cutoff 0.25, half width 0.3), vocoder.py:180-216."""
    half = 6
    amplitude = 2.285 * (half - 1) * math.pi * (4 * 0.3) + 7.95
    beta = 0.1102 * (amplitude - 8.7) if amplitude > 50 else (0.5842 * (amplitude - 21) ** 0.4 + 0.07886 * (amplitude - 21.0) if amplitude >= 21 else 0.0)
    t = np.arange(-half, half) + 0.5
    x = 2 * 0.25 * t
    f = 2 * 0.25 * np.kaiser(12, beta) * np.where(x == 0, 1.0, np.sin(np.pi * x) / np.where(x == 0, 1.0, np.pi * x))
    return torch.from_numpy((f / f.sum()).reshape(1, 1, 12).astype(np.float32))


def make_decoder_weights(ch, ch_mult, num_res_blocks, z_channels, out_ch, seed):
    """Checkpoint-named, PyTorch-layout AudioDecoder weights (`audio_vae.decoder.…`, `audio_vae.per_channel_statistics.…`)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, co, ci, k):
        sd[DEC + name + ".weight"] = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
        sd[DEC + name + ".bias"] = 0.1 * torch.randn(co, generator=g)

    base = ch * ch_mult[-1]
    conv("conv_in.conv", base, z_channels, 3)
    for b in ("mid.block_1", "mid.block_2"):
        conv(b + ".conv1.conv", base, base, 3)
        conv(b + ".conv2.conv", base, base, 3)
    block_in = base
    for lvl in reversed(range(len(ch_mult))):
        block_out = ch * ch_mult[lvl]
        for i in range(num_res_blocks):
            conv(f"up.{lvl}.block.{i}.conv1.conv", block_out, block_in, 3)
            conv(f"up.{lvl}.block.{i}.conv2.conv", block_out, block_out, 3)
            if block_in != block_out:
                conv(f"up.{lvl}.block.{i}.nin_shortcut.conv", block_out, block_in, 1)
            block_in = block_out
        if lvl != 0:
            conv(f"up.{lvl}.upsample.conv.conv", block_out, block_out, 3)
    conv("conv_out.conv", out_ch, ch, 3)
    sd["audio_vae.per_channel_statistics.mean-of-means"] = 0.1 * torch.randn(ch, generator=g)
    sd["audio_vae.per_channel_statistics.std-of-means"] = 1.0 + 0.1 * torch.rand(ch, generator=g)
    return sd


def make_vocoder_weights(cfg, seed, prefix="vocoder.", stereo=True):
    """Checkpoint-named, PyTorch-layout Vocoder weights (conv (out, in, k), transposed conv (in, out, k)); AMP1 adds SnakeBeta
    alpha / beta and the kaiser filter buffers."""
    g = torch.Generator().manual_seed(seed)
    rk, ur, uk, rd = cfg["resblock_kernel_sizes"], cfg["upsample_rates"], cfg["upsample_kernel_sizes"], cfg["resblock_dilation_sizes"]
    c0 = cfg["upsample_initial_channel"]
    amp = cfg.get("resblock", "1") == "AMP1"
    sd = {}

    def conv(name, co, ci, k):
        sd[prefix + name + ".weight"] = torch.randn(co, ci, k, generator=g) / (ci * k) ** 0.5
        sd[prefix + name + ".bias"] = 0.1 * torch.randn(co, generator=g)

    def act(name, c):
        sd[prefix + name + ".act.alpha"] = 0.3 * torch.randn(c, generator=g)
        sd[prefix + name + ".act.beta"] = 0.3 * torch.randn(c, generator=g)
        sd[prefix + name + ".upsample.filter"] = _kaiser12()
        sd[prefix + name + ".downsample.lowpass.filter"] = _kaiser12()

    conv("conv_pre", c0, 128 if stereo else 64, 7)
    for i, k in enumerate(uk):
        ci, co = c0 // 2 ** i, c0 // 2 ** (i + 1)
        sd[prefix + f"ups.{i}.weight"] = torch.randn(ci, co, k, generator=g) / (ci * k / ur[i]) ** 0.5
        sd[prefix + f"ups.{i}.bias"] = 0.1 * torch.randn(co, generator=g)
        for j, (k2, dil) in enumerate(zip(rk, rd)):
            for d in range(len(dil)):
                conv(f"resblocks.{i * len(rk) + j}.convs1.{d}", co, co, k2)
                conv(f"resblocks.{i * len(rk) + j}.convs2.{d}", co, co, k2)
                if amp:
                    act(f"resblocks.{i * len(rk) + j}.acts1.{d}", co)
                    act(f"resblocks.{i * len(rk) + j}.acts2.{d}", co)
    final = c0 // 2 ** len(ur)
    if amp:
        act("act_post", final)
    conv("conv_post", 2 if stereo else 1, final, 7)
    return sd


# the tiny configurations of tests/golden/audio_vae_tiny.npz (tools/pin_audio_vae_against_reference.py)
TINY_DECODER = dict(ch=16, ch_mult=(1, 2, 4), num_res_blocks=1, z_channels=8, out_ch=2)
TINY_VOCODER = dict(resblock_kernel_sizes=[3, 7], upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], resblock_dilation_sizes=[[1, 3], [1, 3]],
                    upsample_initial_channel=32)
TINY_AMP = dict(TINY_VOCODER, resblock="AMP1")
TINY_BWE = dict(resblock="AMP1", resblock_kernel_sizes=[3], upsample_rates=[4, 4, 2], upsample_kernel_sizes=[8, 8, 4], resblock_dilation_sizes=[[1, 3]],
                upsample_initial_channel=32)
TINY_STFT = dict(n_fft=64, hop=16, n_mels=64, in_rate=8000, out_rate=16000)
TINY_SEED = 4321


def tiny_weights():
    """(decoder, LTX-2.0 vocoder, AMP1 vocoder, VocoderWithBWE) checkpoint-named state dicts of the golden."""
    dec = make_decoder_weights(seed=TINY_SEED, **TINY_DECODER)
    voc = make_vocoder_weights(TINY_VOCODER, TINY_SEED + 1)
    amp = make_vocoder_weights(TINY_AMP, TINY_SEED + 2)
    bwe = make_vocoder_weights(TINY_AMP, TINY_SEED + 3, prefix="vocoder.vocoder.")
    bwe.update(make_vocoder_weights(TINY_BWE, TINY_SEED + 4, prefix="vocoder.bwe_generator."))
    nf = TINY_STFT["n_fft"] // 2 + 1
    bwe["vocoder.mel_stft.stft_fn.forward_basis"] = dft_basis(TINY_STFT["n_fft"])
    bwe["vocoder.mel_stft.stft_fn.inverse_basis"] = dft_basis(TINY_STFT["n_fft"])
    bwe["vocoder.mel_stft.mel_basis"] = mel_filterbank(TINY_STFT["n_mels"], nf, seed=TINY_SEED + 5)
    return dec, voc, amp, bwe


def tiny_inputs():
    g = torch.Generator().manual_seed(TINY_SEED + 6)
    return torch.randn(1, 8, 6, 2, generator=g), torch.randn(1, 2, 11, 64, generator=g)
