"""Audio VAE decoder (reference LTX_2_MLX/model/audio_vae/decoder.py) on the MI355X: latent (B, 8, T, 16) -> stereo log-mel
(B, 2, 4T - 3, 64), fp32 end to end (the reference forces fp32 here, decoder.py:302-304).

Every convolution is ltx2_audio_conv (csrc/audio.hip) on the exact-f32 MFMA, channels-last [H = time, W = mel, C]:
CausalConv2d pads 2 rows on top (causal along time) and 1 column each side; Upsample2d's nearest x2 and its dropped first row are
folded into the conv's input indexing; PixelNorm + SiLU is one row kernel; a ResBlock's `x + conv2(...)` (or `nin_shortcut(x) + ...`)
is the conv2 epilogue.  Weights keep the checkpoint's key names and PyTorch layouts (`audio_vae.decoder.…` with the doubled `.conv`)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from ... import kernels as K
from ...components.patchifiers import AudioPatchifier
from ...types import AudioLatentShape

LATENT_DOWNSAMPLE_FACTOR = 4
PREFIX = "audio_vae.decoder."
STATS_MEAN = "audio_vae.per_channel_statistics.mean-of-means"
STATS_STD = "audio_vae.per_channel_statistics.std-of-means"


class PerChannelStatistics:
    """Per-channel latent statistics (checkpoint buffers `mean-of-means` / `std-of-means`), applied in patchified (B, T, C*F) space."""

    def __init__(self, latent_channels: int, device: Union[str, torch.device] = "cuda"):
        self.latent_channels = latent_channels
        self.mean_of_means = torch.zeros(latent_channels, device=device)
        self.std_of_means = torch.ones(latent_channels, device=device)

    def normalize(self, x: torch.Tensor) -> torch.Tensor:
        return (x - self.mean_of_means[None, None, :]) / self.std_of_means[None, None, :]

    def denormalize(self, x: torch.Tensor) -> torch.Tensor:
        return x * self.std_of_means[None, None, :] + self.mean_of_means[None, None, :]


class AudioDecoder:
    """Mirrors the reference's AudioDecoder (constructor arguments, checkpoint keys, output trimming).  is_causal=True is the only
    causality built (CausalityAxis.HEIGHT, the reference's default)."""

    def __init__(self, ch: int = 128, out_ch: int = 2, ch_mult: Tuple[int, ...] = (1, 2, 4), num_res_blocks: int = 3, z_channels: int = 8,
                 mel_bins: int = 16, sample_rate: int = 16000, mel_hop_length: int = 160, is_causal: bool = True,
                 compute_dtype: torch.dtype = torch.float32, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device(device)          # a CPU decoder only holds weights (loaders, tests); decoding needs the GPU
        if not is_causal:
            raise NotImplementedError("AudioDecoder(is_causal=False): only the causal (HEIGHT) decoder of the checkpoints is built")
        self.ch, self.out_ch, self.ch_mult, self.num_res_blocks = ch, out_ch, tuple(ch_mult), num_res_blocks
        self.num_resolutions = len(ch_mult)
        self.z_channels, self.mel_bins, self.is_causal = z_channels, mel_bins, is_causal
        self.compute_dtype = torch.float32           # fp32 regardless of the argument, as the reference decodes
        self.per_channel_statistics = PerChannelStatistics(ch, self.device)
        self.patchifier = AudioPatchifier(patch_size=1, audio_latent_downsample_factor=LATENT_DOWNSAMPLE_FACTOR, sample_rate=sample_rate,
                                          hop_length=mel_hop_length, is_causal=is_causal)
        # (pt level, [(block prefix, c_in, c_out)], upsample?) from the deepest level up, as the reference builds up_blocks
        self.levels = []
        block_in = ch * ch_mult[-1]
        for lvl in reversed(range(self.num_resolutions)):
            block_out = ch * ch_mult[lvl]
            blocks = []
            for i in range(num_res_blocks):
                blocks.append((f"up.{lvl}.block.{i}", block_in, block_out))
                block_in = block_out
            self.levels.append((lvl, blocks, lvl != 0))
        self._w: Dict[str, torch.Tensor] = {}
        self._packed: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ weights
    def _convs(self):
        """(checkpoint conv prefix without `.weight`, c_out, c_in, k)"""
        base = self.ch * self.ch_mult[-1]
        out = [("conv_in.conv", base, self.z_channels, 3)]
        for name in ("mid.block_1", "mid.block_2"):
            out += [(f"{name}.conv1.conv", base, base, 3), (f"{name}.conv2.conv", base, base, 3)]
        for lvl, blocks, up in self.levels:
            for pre, ci, co in blocks:
                out += [(f"{pre}.conv1.conv", co, ci, 3), (f"{pre}.conv2.conv", co, co, 3)]
                if ci != co:
                    out.append((f"{pre}.nin_shortcut.conv", co, ci, 1))
            if up:
                co = blocks[-1][2]
                out.append((f"up.{lvl}.upsample.conv.conv", co, co, 3))
        out.append(("conv_out.conv", self.out_ch, self.ch, 3))
        return out

    def expected_weight_shapes(self) -> Dict[str, Tuple[int, ...]]:
        s = {STATS_MEAN: (self.ch,), STATS_STD: (self.ch,)}
        for name, co, ci, k in self._convs():
            s[PREFIX + name + ".weight"] = (co, ci, k, k)
            s[PREFIX + name + ".bias"] = (co,)
        return s

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> int:
        """Checkpoint-named tensors (any float dtype, any device) -> fp32 device weights; keys absent from `sd` keep their values
        (the reference's loader skips them too).  Returns the number of tensors taken."""
        shapes = self.expected_weight_shapes()
        n = 0
        for key, shape in shapes.items():
            if key not in sd:
                continue
            t = sd[key].to(self.device, torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError(f"{key}: shape {tuple(t.shape)}, expected {shape}")
            n += 1
            if key == STATS_MEAN:
                self.per_channel_statistics.mean_of_means = t.contiguous()
            elif key == STATS_STD:
                self.per_channel_statistics.std_of_means = t.contiguous()
            else:
                self._w[key] = t.contiguous()
                if key.endswith(".weight"):
                    self._packed[key] = K.pack_conv_weight(t)
        return n

    def init_random_weights(self, seed: int = 0) -> None:
        """Weights ~ N(0, 1) / sqrt(fan_in), biases ~ 0.1 N(0, 1), statistics near (0, 1): for tests and checkpoint-less runs."""
        g = torch.Generator().manual_seed(seed)
        sd = {}
        for key, shape in self.expected_weight_shapes().items():
            if key == STATS_MEAN:
                sd[key] = 0.1 * torch.randn(shape, generator=g)
            elif key == STATS_STD:
                sd[key] = 1.0 + 0.1 * torch.rand(shape, generator=g)
            elif key.endswith(".weight"):
                fan_in = shape[1] * shape[2] * shape[3]
                sd[key] = torch.randn(shape, generator=g) / fan_in ** 0.5
            else:
                sd[key] = 0.1 * torch.randn(shape, generator=g)
        self.load_state_dict(sd)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = dict(self._w)
        sd[STATS_MEAN] = self.per_channel_statistics.mean_of_means
        sd[STATS_STD] = self.per_channel_statistics.std_of_means
        return sd

    # ------------------------------------------------------------------ forward
    def _conv(self, x, name, k, upsample=False, res=None):
        w = self._packed.get(PREFIX + name + ".weight")
        if w is None:
            raise RuntimeError(f"AudioDecoder: weight {PREFIX + name}.weight not loaded (load_audio_decoder_weights / init_random_weights)")
        pad = k - 1
        return K.audio_conv2d(x, w, self._w[PREFIX + name + ".bias"], self._w[PREFIX + name + ".weight"].shape[0], k, k, pad, pad // 2,
                              upsample=upsample, res=res)

    def _resblock(self, x, pre, c_in, c_out):
        h = self._conv(K.audio_pixnorm_silu(x), f"{pre}.conv1.conv", 3)
        skip = self._conv(x, f"{pre}.nin_shortcut.conv", 1) if c_in != c_out else x
        return self._conv(K.audio_pixnorm_silu(h), f"{pre}.conv2.conv", 3, res=skip)

    def _denormalize_latents(self, sample: torch.Tensor) -> torch.Tensor:
        shape = AudioLatentShape(batch=sample.shape[0], channels=sample.shape[1], frames=sample.shape[2], mel_bins=sample.shape[3])
        return self.patchifier.unpatchify(self.per_channel_statistics.denormalize(self.patchifier.patchify(sample)), shape)

    def __call__(self, sample: torch.Tensor) -> torch.Tensor:
        """sample (B, z_channels, T, mel_bins) -> log-mel (B, out_ch, 4T - 3, 4 mel_bins), fp32."""
        if not sample.is_cuda or self.device.type != "cuda":
            raise RuntimeError("AudioDecoder runs on the MI355X only (no CPU fallback): a CUDA decoder and a CUDA tensor")
        sample = self._denormalize_latents(sample.float())
        b, _, t, f = sample.shape
        target_frames = max(t * LATENT_DOWNSAMPLE_FACTOR - (LATENT_DOWNSAMPLE_FACTOR - 1), 1)
        target_mel = f * LATENT_DOWNSAMPLE_FACTOR
        base = self.ch * self.ch_mult[-1]
        outs = []
        for i in range(b):
            h = self._conv(sample[i].permute(1, 2, 0).contiguous(), "conv_in.conv", 3)          # [T, F, C]
            h = self._resblock(h, "mid.block_1", base, base)
            h = self._resblock(h, "mid.block_2", base, base)
            for lvl, blocks, up in self.levels:
                for pre, ci, co in blocks:
                    h = self._resblock(h, pre, ci, co)
                if up:
                    h = self._conv(h, f"up.{lvl}.upsample.conv.conv", 3, upsample=True)
            h = self._conv(K.audio_pixnorm_silu(h), "conv_out.conv", 3)
            outs.append(h[:target_frames, :target_mel].permute(2, 0, 1))
        return torch.stack(outs)[:, :self.out_ch]


def load_audio_decoder_weights(decoder: AudioDecoder, weights_path: str) -> None:
    """`audio_vae.decoder.…` and `audio_vae.per_channel_statistics.…` tensors of a safetensors checkpoint -> decoder (bf16 upcast)."""
    from ...loader.weight_converter import SafetensorsStream
    print(f"Loading Audio VAE decoder weights from {weights_path}...")
    with SafetensorsStream(weights_path, "cpu") as st:
        keys = st.keys()
        if not any(k.startswith("audio_vae.") for k in keys):
            print("  Warning: No audio VAE weights found in checkpoint")
            return
        wanted = [k for k in decoder.expected_weight_shapes() if k in set(keys)]
        n = decoder.load_state_dict(st.load(wanted))
    print(f"  Loaded {n} audio decoder weight tensors")
