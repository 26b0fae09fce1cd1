"""HiFi-GAN / BigVGAN-v2 vocoders (reference LTX_2_MLX/model/audio_vae/vocoder.py) on the MI355X: stereo log-mel (B, 2, T, mel)
-> waveform (B, 2, samples), fp32 end to end as the reference runs them (vocoder.py:599-612, :758-760).

Channels-last [T, C] throughout.  Every Conv1d is ltx2_audio_conv on the exact-f32 MFMA with the block's LeakyReLU as its operand
prologue and `x + conv2(...)` as its epilogue; the three resblocks' mean is a scaled accumulate into one buffer (no stack + mean);
ConvTranspose1d runs as `rate` polyphase convolutions; Activation1d(SnakeBeta) is one fused kernel; the BWE skip path is the
polyphase Hann-sinc resampler, and `clip(residual + skip, -1, 1)` is the BWE generator's conv_post epilogue.  The MelSTFT of
VocoderWithBWE is the same conv (stride = hop, one input channel) and a 1x1 conv over |X| with log(max(., 1e-5)) as its epilogue.
Weights keep the checkpoint's names and PyTorch layouts (conv (out, in, k), transposed conv (in, out, k))."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from ... import _native as nv
from ... import kernels as K

LRELU_SLOPE = 0.1


def kaiser_sinc_filter1d(cutoff: float, half_width: float, kernel_size: int) -> torch.Tensor:
    """The reference's kaiser-windowed sinc filter (vocoder.py:180-216), shape (1, 1, kernel_size) fp32."""
    even = kernel_size % 2 == 0
    half_size = kernel_size // 2
    delta_f = 4 * half_width
    amplitude = 2.285 * (half_size - 1) * math.pi * delta_f + 7.95
    if amplitude > 50.0:
        beta = 0.1102 * (amplitude - 8.7)
    elif amplitude >= 21.0:
        beta = 0.5842 * (amplitude - 21) ** 0.4 + 0.07886 * (amplitude - 21.0)
    else:
        beta = 0.0
    window = np.kaiser(kernel_size, beta)
    time = (np.arange(-half_size, half_size) + 0.5) if even else (np.arange(kernel_size) - half_size)
    if cutoff == 0:
        filter_ = np.zeros_like(time)
    else:
        x = 2 * cutoff * time
        safe_denom = np.where(x == 0, 1.0, np.pi * x)
        sinc = np.where(x == 0, 1.0, np.sin(np.pi * x) / safe_denom)
        filter_ = 2 * cutoff * window * sinc
        filter_ /= filter_.sum()
    return torch.from_numpy(filter_.reshape(1, 1, kernel_size).astype(np.float32))


def hann_resample_filter(ratio: int, rolloff: float = 0.99, lowpass_filter_width: int = 6) -> Tuple[torch.Tensor, int, int]:
    """UpSample1d(ratio, window_type="hann") (vocoder.py:317-341): (filter (1, 1, 2 width ratio + 1), pad = width, pad_left)."""
    width = math.ceil(lowpass_filter_width / rolloff)
    kernel_size = 2 * width * ratio + 1
    time_axis = np.arange(kernel_size) / ratio - width
    time_axis_rolloff = time_axis * rolloff
    time_clamped = np.clip(time_axis_rolloff, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(time_clamped * math.pi / lowpass_filter_width / 2) ** 2
    safe_denom = np.where(time_axis_rolloff == 0, 1.0, np.pi * time_axis_rolloff)
    sinc_vals = np.where(time_axis_rolloff == 0, 1.0, np.sin(np.pi * time_axis_rolloff) / safe_denom)
    filt = (sinc_vals * window * rolloff / ratio).reshape(1, 1, -1).astype(np.float32)
    return torch.from_numpy(filt), width, 2 * width * ratio


class Vocoder:
    """Mirrors the reference's Vocoder: resblock="1" is HiFi-GAN (LeakyReLU 0.1 in the blocks, 0.01 before conv_post), resblock="AMP1"
    BigVGAN v2 (anti-aliased SnakeBeta).  Input (B, 2, T, mel_bins) stereo log-mel, output (B, 2, T * prod(upsample_rates))."""

    def __init__(self, resblock_kernel_sizes: Optional[List[int]] = None, upsample_rates: Optional[List[int]] = None,
                 upsample_kernel_sizes: Optional[List[int]] = None, resblock_dilation_sizes: Optional[List[List[int]]] = None,
                 upsample_initial_channel: int = 1024, stereo: bool = True, output_sample_rate: int = 24000,
                 compute_dtype: torch.dtype = torch.float32, resblock: str = "1", activation: str = "snake", apply_final_activation: bool = True,
                 use_tanh_at_final: bool = True, use_bias_at_final: bool = True, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device(device)          # a CPU vocoder only holds weights (loaders, tests); synthesis needs the GPU
        self.resblock_kernel_sizes = list(resblock_kernel_sizes or [3, 7, 11])
        self.upsample_rates = list(upsample_rates or [6, 5, 2, 2, 2])
        self.upsample_kernel_sizes = list(upsample_kernel_sizes or [16, 15, 8, 4, 4])
        self.resblock_dilation_sizes = [list(d) for d in (resblock_dilation_sizes or [[1, 3, 5], [1, 3, 5], [1, 3, 5]])]
        self.upsample_initial_channel = upsample_initial_channel
        self.output_sample_rate = output_sample_rate
        self.num_kernels = len(self.resblock_kernel_sizes)
        self.num_upsamples = len(self.upsample_rates)
        self.compute_dtype = torch.float32
        self.is_amp = resblock == "AMP1"
        self.activation = activation
        self.apply_final_activation = apply_final_activation
        self.use_tanh_at_final = use_tanh_at_final
        self.in_channels = 128 if stereo else 64
        self.out_channels = 2 if stereo else 1
        self.final_channels = upsample_initial_channel // (2 ** self.num_upsamples)
        self.upsample_factor = math.prod(self.upsample_rates)
        self._w: Dict[str, torch.Tensor] = {}
        self._packed: Dict[str, torch.Tensor] = {}
        if self.is_amp:                      # filter buffers default to the reference's kaiser filters; a checkpoint overrides them
            up = kaiser_sinc_filter1d(0.25, 0.3, 12)
            sd = {}
            for key in self.expected_weight_shapes():
                if key.endswith(".filter"):
                    sd[key] = up
            self.load_state_dict(sd)

    def _activations(self):
        """checkpoint prefixes of the Activation1d modules and their channels"""
        out = []
        for i in range(self.num_upsamples):
            ch = self.upsample_initial_channel // (2 ** (i + 1))
            for j in range(self.num_kernels):
                for d in range(len(self.resblock_dilation_sizes[j])):
                    out += [(f"resblocks.{i * self.num_kernels + j}.acts1.{d}", ch), (f"resblocks.{i * self.num_kernels + j}.acts2.{d}", ch)]
        out.append(("act_post", self.final_channels))
        return out

    def expected_weight_shapes(self) -> Dict[str, Tuple[int, ...]]:
        s: Dict[str, Tuple[int, ...]] = {}
        c0 = self.upsample_initial_channel
        s["conv_pre.weight"], s["conv_pre.bias"] = (c0, self.in_channels, 7), (c0,)
        for i, (rate, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            s[f"ups.{i}.weight"], s[f"ups.{i}.bias"] = (c0 // 2 ** i, c0 // 2 ** (i + 1), k), (c0 // 2 ** (i + 1),)
            ch = c0 // 2 ** (i + 1)
            for j, (k2, dil) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
                for d in range(len(dil)):
                    for conv in ("convs1", "convs2"):
                        pre = f"resblocks.{i * self.num_kernels + j}.{conv}.{d}"
                        s[pre + ".weight"], s[pre + ".bias"] = (ch, ch, k2), (ch,)
        if self.is_amp:
            for pre, ch in self._activations():
                s[pre + ".act.alpha"] = (ch,)
                s[pre + ".act.beta"] = (ch,)
                s[pre + ".upsample.filter"] = (1, 1, 12)
                s[pre + ".downsample.lowpass.filter"] = (1, 1, 12)
        s["conv_post.weight"], s["conv_post.bias"] = (self.out_channels, self.final_channels, 7), (self.out_channels,)
        return s

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> int:
        """Names relative to the vocoder (`conv_pre.weight`, `ups.0.weight`, …) -> fp32 device tensors; absent keys keep their values."""
        n = 0
        for key, shape in self.expected_weight_shapes().items():
            if key not in sd:
                continue
            t = sd[key].to(self.device, torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError(f"vocoder {key}: shape {tuple(t.shape)}, expected {shape}")
            n += 1
            self._w[key] = t.reshape(-1).contiguous() if key.endswith(".filter") else t.contiguous()
            if key.startswith("ups.") and key.endswith(".weight"):
                i = int(key.split(".")[1])
                self._packed[key] = K.pack_conv_transpose_weight(t, self.upsample_rates[i])
            elif key.endswith(".weight"):
                self._packed[key] = K.pack_conv_weight(t)
        return n

    def init_random_weights(self, seed: int = 0) -> None:
        """Conv weights ~ N(0, 1) / sqrt(fan_in), biases ~ 0.1 N(0, 1), SnakeBeta alpha / beta ~ 0.1 N(0, 1) (log scale); the filter
        buffers keep the reference's kaiser filters."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for key, shape in self.expected_weight_shapes().items():
            if key.endswith(".filter"):
                continue
            if key.endswith(".weight"):
                fan_in = (shape[0] if key.startswith("ups.") else shape[1]) * shape[2]
                sd[key] = torch.randn(shape, generator=g) / fan_in ** 0.5
            else:
                sd[key] = 0.1 * torch.randn(shape, generator=g)
        self.load_state_dict(sd)

    def output_length(self, frames: int) -> int:
        """waveform samples for `frames` mel frames (each ConvTranspose1d gives (T - 1) rate + k - 2 ((k - rate) // 2))"""
        for rate, k in zip(self.upsample_rates, self.upsample_kernel_sizes):
            frames = (frames - 1) * rate + k - 2 * ((k - rate) // 2)
        return frames

    def state_dict(self) -> Dict[str, torch.Tensor]:
        shapes = self.expected_weight_shapes()
        return {k: v.reshape(shapes[k]) for k, v in self._w.items()}

    # ------------------------------------------------------------------ forward
    def _need(self, key):
        if key not in self._w:
            raise RuntimeError(f"Vocoder: {key} not loaded (load_vocoder_weights / init_random_weights)")
        return self._w[key]

    def _conv(self, x, name, k, dilation=1, prologue=nv.AUDIO_PRO_NONE, slope=0.0, **epi):
        w = self._need(name + ".weight")
        return K.audio_conv1d(x, self._packed[name + ".weight"], self._w[name + ".bias"], w.shape[0], k, dilation=dilation,
                              padding=(k - 1) * dilation // 2, prologue=prologue, slope=slope, **epi)

    def _snake(self, x, pre):
        return K.audio_snake_aa(x, self._need(pre + ".act.alpha"), self._need(pre + ".act.beta"), self._need(pre + ".upsample.filter"),
                                self._need(pre + ".downsample.lowpass.filter"))

    def _resblock_into(self, x, idx, k, dilations, mean, first):
        """mean (+)= block(x) / num_kernels, where block = ResBlock1 / AMPBlock1 (vocoder.py:146-154, :447-457)."""
        cur, buf = x, None
        for d_i, d in enumerate(dilations):
            pre = f"resblocks.{idx}"
            last = d_i == len(dilations) - 1
            if self.is_amp:
                t = self._conv(self._snake(cur, f"{pre}.acts1.{d_i}"), f"{pre}.convs1.{d_i}", k, dilation=d)
                t = self._snake(t, f"{pre}.acts2.{d_i}")
                pro = dict()
            else:
                t = self._conv(cur, f"{pre}.convs1.{d_i}", k, dilation=d, prologue=nv.AUDIO_PRO_LEAKY_RELU, slope=LRELU_SLOPE)
                pro = dict(prologue=nv.AUDIO_PRO_LEAKY_RELU, slope=LRELU_SLOPE)
            if last:
                self._conv(t, f"{pre}.convs2.{d_i}", k, res=cur, out=mean, alpha=1.0 / self.num_kernels, beta=0.0 if first else 1.0, **pro)
            else:
                if buf is None:
                    buf = torch.empty_like(x)
                self._conv(t, f"{pre}.convs2.{d_i}", k, res=cur, out=buf, **pro)
                cur = buf

    def _forward_cl(self, x: torch.Tensor, final_res: Optional[torch.Tensor] = None, final_act: Optional[int] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [T, in_channels] channels-last fp32 -> waveform [T * upsample_factor, out_channels].  final_res / final_act replace the
        configured final activation with act(conv_post + final_res) (VocoderWithBWE's clip(residual + skip))."""
        h = self._conv(x, "conv_pre", 7)
        for i, (rate, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            w = self._need(f"ups.{i}.weight")
            pro = dict(prologue=nv.AUDIO_PRO_NONE) if self.is_amp else dict(prologue=nv.AUDIO_PRO_LEAKY_RELU, slope=LRELU_SLOPE)
            h = K.audio_conv_transpose1d(h, self._packed[f"ups.{i}.weight"], self._w[f"ups.{i}.bias"], w.shape[1], k, rate, (k - rate) // 2, **pro)
            mean = torch.empty_like(h)
            for j, (k2, dil) in enumerate(zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes)):
                self._resblock_into(h, i * self.num_kernels + j, k2, dil, mean, j == 0)
            h = mean
        if final_act is None:
            final_act = nv.AUDIO_ACT_NONE
            if self.apply_final_activation:
                final_act = nv.AUDIO_ACT_TANH if self.use_tanh_at_final else nv.AUDIO_ACT_CLIP
        if self.is_amp:
            return self._conv(self._snake(h, "act_post"), "conv_post", 7, res=final_res, act=final_act, out=out)
        # PyTorch's default leaky_relu slope (0.01) before conv_post, not LRELU_SLOPE (vocoder.py:796-798)
        return self._conv(h, "conv_post", 7, prologue=nv.AUDIO_PRO_LEAKY_RELU, slope=0.01, res=final_res, act=final_act, out=out)

    @staticmethod
    def _mel_to_cl(mel: torch.Tensor) -> torch.Tensor:
        """(2, T, mel) -> [T, 2 * mel], channel s * mel + m (the reference's transpose + reshape, vocoder.py:762-767)"""
        s, t, m = mel.shape
        return mel.permute(1, 0, 2).reshape(t, s * m).contiguous()

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, 2, T, mel_bins) log-mel -> waveform (B, 2, T * prod(upsample_rates)), fp32."""
        if not x.is_cuda or self.device.type != "cuda":
            raise RuntimeError("Vocoder runs on the MI355X only (no CPU fallback): a CUDA vocoder and a CUDA tensor")
        x = x.float()
        return torch.stack([self._forward_cl(self._mel_to_cl(x[b])).t() for b in range(x.shape[0])])


class _STFTFn:
    def __init__(self, filter_length: int, hop_length: int, win_length: int, device):
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        n_freqs = filter_length // 2 + 1
        self.forward_basis = torch.zeros(n_freqs * 2, 1, filter_length, device=device)
        self.inverse_basis = torch.zeros(n_freqs * 2, 1, filter_length, device=device)


class MelSTFT:
    """Log-mel spectrogram with checkpoint buffers (vocoder.py:460-551): STFT as a strided conv with forward_basis, causal left pad
    win_length - hop_length, then log(max(mel_basis @ |X|, 1e-5))."""

    def __init__(self, filter_length: int, hop_length: int, win_length: int, n_mel_channels: int, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device(device)
        self.stft_fn = _STFTFn(filter_length, hop_length, win_length, self.device)
        self.n_freqs = filter_length // 2 + 1
        self.n_mel_channels = n_mel_channels
        self.mel_basis = torch.zeros(n_mel_channels, self.n_freqs, device=self.device)
        self._packed: Dict[str, torch.Tensor] = {}

    def set_buffers(self, forward_basis=None, inverse_basis=None, mel_basis=None) -> None:
        if forward_basis is not None:
            self.stft_fn.forward_basis = forward_basis.to(self.device, torch.float32).contiguous()
        if inverse_basis is not None:
            self.stft_fn.inverse_basis = inverse_basis.to(self.device, torch.float32).contiguous()
        if mel_basis is not None:
            self.mel_basis = mel_basis.to(self.device, torch.float32).contiguous()
        self._packed = {"stft": K.pack_conv_weight(self.stft_fn.forward_basis), "mel": K.pack_conv_weight(self.mel_basis[:, :, None])}

    def log_mel_into(self, y: torch.Tensor, out: torch.Tensor) -> None:
        """y: one waveform channel [L, 1] (any row stride) -> out [frames, n_mel_channels] (any row stride)."""
        if not self._packed:
            self.set_buffers()
        f = self.stft_fn
        left = max(0, f.win_length - f.hop_length)
        frames = (y.shape[0] + left - f.filter_length) // f.hop_length + 1
        spec = K.audio_conv1d(y, self._packed["stft"], None, 2 * self.n_freqs, f.filter_length, stride=f.hop_length, padding=left, t_out=frames)
        K.audio_conv1d(spec, self._packed["mel"], None, self.n_mel_channels, 1, c_in=self.n_freqs, prologue=nv.AUDIO_PRO_MAGNITUDE,
                       act=nv.AUDIO_ACT_LOG, out=out)

    def mel_spectrogram(self, y: torch.Tensor):
        """y (B, T) -> (log_mel (B, n_mel_channels, frames), magnitude, phase, energy), the reference's 4-tuple (vocoder.py:532-551).
        Only the log-mel is formed on this path (the magnitude is folded into the mel product's operand staging); magnitude, phase and
        energy are returned as None, so unpacking the tuple works and using them fails loudly."""
        if not y.is_cuda or self.device.type != "cuda":
            raise RuntimeError("MelSTFT runs on the MI355X only (no CPU fallback): a CUDA MelSTFT and a CUDA tensor")
        f = self.stft_fn
        left = max(0, f.win_length - f.hop_length)
        frames = (y.shape[1] + left - f.filter_length) // f.hop_length + 1
        out = torch.empty(y.shape[0], frames, self.n_mel_channels, device=self.device)
        for b in range(y.shape[0]):
            self.log_mel_into(y[b].float().contiguous()[:, None], out[b])
        return out.transpose(1, 2), None, None, None


class VocoderWithBWE:
    """Vocoder + bandwidth extension (vocoder.py:554-652): base waveform -> log-mel -> BWE generator residual, plus the Hann-sinc
    resampled base waveform; clip(residual + skip, -1, 1) trimmed to T * output / input rate."""

    def __init__(self, vocoder: Vocoder, bwe_generator: Vocoder, mel_stft: MelSTFT, input_sampling_rate: int, output_sampling_rate: int,
                 hop_length: int):
        self.vocoder, self.bwe_generator, self.mel_stft = vocoder, bwe_generator, mel_stft
        self.input_sampling_rate, self.output_sampling_rate = input_sampling_rate, output_sampling_rate
        self.hop_length = hop_length
        self.output_sample_rate = output_sampling_rate
        self.ratio = output_sampling_rate // input_sampling_rate
        filt, self._rs_pad, self._rs_pad_left = hann_resample_filter(self.ratio)
        self.resampler_filter = filt.reshape(-1).to(vocoder.device)

    def __call__(self, mel_spec: torch.Tensor) -> torch.Tensor:
        """mel_spec (B, 2, T, mel_bins) -> waveform (B, 2, T_out) in [-1, 1], fp32."""
        if not mel_spec.is_cuda or self.vocoder.device.type != "cuda" or self.bwe_generator.device.type != "cuda":
            raise RuntimeError("VocoderWithBWE runs on the MI355X only (no CPU fallback): CUDA vocoders and a CUDA tensor")
        mel_spec = mel_spec.float()
        outs = []
        for b in range(mel_spec.shape[0]):
            x = self.vocoder._forward_cl(Vocoder._mel_to_cl(mel_spec[b]))                # [L, C]
            length = x.shape[0]
            output_length = length * self.output_sampling_rate // self.input_sampling_rate
            padded = -(-length // self.hop_length) * self.hop_length
            if padded != length:
                x = torch.cat([x, x.new_zeros(padded - length, x.shape[1])])
            n_ch, n_mels = x.shape[1], self.mel_stft.n_mel_channels
            left = max(0, self.mel_stft.stft_fn.win_length - self.hop_length)
            frames = (padded + left - self.mel_stft.stft_fn.filter_length) // self.hop_length + 1
            mel = torch.empty(frames, n_ch * n_mels, device=x.device)
            for c in range(n_ch):
                self.mel_stft.log_mel_into(x[:, c:c + 1], mel[:, c * n_mels:(c + 1) * n_mels])
            skip = K.audio_upsample(x, self.resampler_filter, self.ratio, self._rs_pad, self._rs_pad_left, self.ratio * padded)
            bwe_len = self.bwe_generator.output_length(frames)
            if bwe_len != skip.shape[0]:
                raise ValueError(f"VocoderWithBWE: the BWE residual has {bwe_len} samples, the resampled skip {skip.shape[0]} "
                                 "(hop_length * output / input rate must equal the BWE generator's upsampling)")
            y = self.bwe_generator._forward_cl(mel, final_res=skip, final_act=nv.AUDIO_ACT_CLIP)
            outs.append(y[:output_length].t())
        return torch.stack(outs)


def _load_prefixed(st, prefix: str, shapes) -> Dict[str, torch.Tensor]:
    keys = set(st.keys())
    names = [prefix + k for k in shapes if prefix + k in keys]
    return {k[len(prefix):]: v for k, v in st.load(names).items()}


def load_vocoder_weights(vocoder: Vocoder, weights_path: str) -> None:
    """`vocoder.…` tensors of a safetensors checkpoint -> vocoder (bf16 upcast; transposed-conv weights (in, out, k))."""
    from ...loader.weight_converter import SafetensorsStream
    print(f"Loading Vocoder weights from {weights_path}...")
    with SafetensorsStream(weights_path, "cpu") as st:
        if not any(k.startswith("vocoder.") for k in st.keys()):
            print("  Warning: No vocoder weights found in checkpoint")
            return
        n = vocoder.load_state_dict(_load_prefixed(st, "vocoder.", vocoder.expected_weight_shapes()))
    print(f"  Loaded {n} vocoder weight tensors")


def load_vocoder_with_bwe_weights(vocoder_with_bwe: VocoderWithBWE, weights_path: str) -> None:
    """`vocoder.vocoder.…`, `vocoder.bwe_generator.…` and `vocoder.mel_stft.…` tensors -> VocoderWithBWE."""
    from ...loader.weight_converter import SafetensorsStream
    print(f"Loading VocoderWithBWE weights from {weights_path}...")
    with SafetensorsStream(weights_path, "cpu") as st:
        n = vocoder_with_bwe.vocoder.load_state_dict(_load_prefixed(st, "vocoder.vocoder.", vocoder_with_bwe.vocoder.expected_weight_shapes()))
        n += vocoder_with_bwe.bwe_generator.load_state_dict(
            _load_prefixed(st, "vocoder.bwe_generator.", vocoder_with_bwe.bwe_generator.expected_weight_shapes()))
        bufs = _load_prefixed(st, "vocoder.mel_stft.", {"stft_fn.forward_basis": 0, "stft_fn.inverse_basis": 0, "mel_basis": 0})
        vocoder_with_bwe.mel_stft.set_buffers(bufs.get("stft_fn.forward_basis"), bufs.get("stft_fn.inverse_basis"), bufs.get("mel_basis"))
        n += len(bufs)
    print(f"  Loaded {n} vocoder+BWE weight tensors")
