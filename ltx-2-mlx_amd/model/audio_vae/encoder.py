"""Audio VAE encoder (reference LTX_2_MLX/model/audio_vae/encoder.py) on the MI355X: stereo log-mel (B, 2, T_mel, 64) -> latent
(B, 8, T_a, 16), fp32 end to end like the decoder.

The decoder's kernels in the other direction (csrc/audio.hip), channels-last [H = time, W = mel, C]: conv_in reads the two mel channels
through the kernel's scalar-load path; a SimpleResBlock2d is audio_pixnorm_silu + conv with the residual in conv2's epilogue, exactly as
AudioDecoder._resblock; Downsample2d (CausalConv2d(k = 3, stride = 2): 2 rows on top, 1 column each side, every second output along time
and mel) is ltx2_audio_conv2d_strided, which computes only the outputs it keeps; the tail's silu(h) (no PixelNorm, unlike the decoder's)
is the epilogue of mid.block_2.conv2, applied after the residual add; conv_out's channels-last result goes through
ltx2_audio_latent_normalize (patchify -> normalize -> unpatchify on the mean half, encoder.py:172-203) in one pass.

Checkpoint keys: the reference's loader spells them `audio_vae.encoder.conv_in.weight`, `...down.{l}.block.{i}.conv1.weight`,
`...down.{l}.downsample.conv.weight`, `...per_channel_statistics.mean-of-means` (encoder.py:206-303); the decoder checkpoints double the
`.conv.` (`conv_in.conv.weight`).  That loader was never exercised by a pipeline of the reference, so which spelling released weights carry
is NOT verified: load_state_dict takes either, and falls back to the shared `audio_vae.per_channel_statistics.*` for the statistics."""
from __future__ import annotations

from typing import Dict, Tuple, Union

import torch

from ... import _native as nv
from ... import kernels as K
from ...components.patchifiers import AudioPatchifier
from .decoder import LATENT_DOWNSAMPLE_FACTOR, PerChannelStatistics

PREFIX = "audio_vae.encoder."
STATS_MEAN = PREFIX + "per_channel_statistics.mean-of-means"
STATS_STD = PREFIX + "per_channel_statistics.std-of-means"
SHARED_STATS = {STATS_MEAN: "audio_vae.per_channel_statistics.mean-of-means", STATS_STD: "audio_vae.per_channel_statistics.std-of-means"}


def _doubled(key: str) -> str:
    """The decoder checkpoints' spelling of a conv tensor: `<conv>.weight` -> `<conv>.conv.weight`."""
    stem, leaf = key.rsplit(".", 1)
    return f"{stem}.conv.{leaf}"


class AudioEncoder:
    """Mirrors the reference's AudioEncoder (constructor arguments, call signature, checkpoint keys).  is_causal=True is the only causality
    built (CausalityAxis.HEIGHT, the reference's default)."""

    def __init__(self, ch: int = 128, in_ch: int = 2, ch_mult: Tuple[int, ...] = (1, 2, 4), num_res_blocks: int = 3, z_channels: int = 8,
                 mel_bins: int = 16, double_z: bool = True, sample_rate: int = 16000, mel_hop_length: int = 160, is_causal: bool = True,
                 compute_dtype: torch.dtype = torch.float32, device: Union[str, torch.device] = "cuda"):
        self.device = torch.device(device)          # a CPU encoder only holds weights (loaders, tests); encoding needs the GPU
        if not is_causal:
            raise NotImplementedError("AudioEncoder(is_causal=False): only the causal (HEIGHT) encoder of the checkpoints is built")
        self.ch, self.in_ch, self.ch_mult, self.num_res_blocks = ch, in_ch, tuple(ch_mult), num_res_blocks
        self.num_resolutions = len(ch_mult)
        self.z_channels, self.mel_bins, self.double_z, self.is_causal = z_channels, mel_bins, double_z, is_causal
        self.compute_dtype = torch.float32           # fp32 regardless of the argument, like the decoder
        # patchified statistics: ch entries = z_channels * mel_bins (encoder.py:78-80)
        self.per_channel_statistics = PerChannelStatistics(ch, self.device)
        self.patchifier = AudioPatchifier(patch_size=1, audio_latent_downsample_factor=LATENT_DOWNSAMPLE_FACTOR, sample_rate=sample_rate,
                                          hop_length=mel_hop_length, is_causal=is_causal)
        # (level, [(block prefix, c_in, c_out)], downsample?) in forward order, as the reference builds down_blocks
        self.levels = []
        block_in = ch
        for lvl in range(self.num_resolutions):
            block_out = ch * ch_mult[lvl]
            blocks = []
            for i in range(num_res_blocks):
                blocks.append((f"down.{lvl}.block.{i}", block_in, block_out))
                block_in = block_out
            self.levels.append((lvl, blocks, lvl != self.num_resolutions - 1))
        self.out_channels = 2 * z_channels if double_z else z_channels
        self._w: Dict[str, torch.Tensor] = {}
        self._packed: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ weights
    def _convs(self):
        """(checkpoint conv prefix without `.weight`, c_out, c_in, k), in the reference loader's spelling"""
        out = [("conv_in", self.ch, self.in_ch, 3)]
        for lvl, blocks, down in self.levels:
            for pre, ci, co in blocks:
                out += [(f"{pre}.conv1", co, ci, 3), (f"{pre}.conv2", co, co, 3)]
                if ci != co:
                    out.append((f"{pre}.nin_shortcut", co, ci, 1))
            if down:
                co = blocks[-1][2]
                out.append((f"down.{lvl}.downsample.conv", co, co, 3))
        base = self.ch * self.ch_mult[-1]
        for name in ("mid.block_1", "mid.block_2"):
            out += [(f"{name}.conv1", base, base, 3), (f"{name}.conv2", base, base, 3)]
        out.append(("conv_out", self.out_channels, base, 3))
        return out

    def expected_weight_shapes(self) -> Dict[str, Tuple[int, ...]]:
        s = {STATS_MEAN: (self.ch,), STATS_STD: (self.ch,)}
        for name, co, ci, k in self._convs():
            s[PREFIX + name + ".weight"] = (co, ci, k, k)
            s[PREFIX + name + ".bias"] = (co,)
        return s

    def checkpoint_keys(self, key: str) -> Tuple[str, ...]:
        """The spellings load_state_dict accepts for one expected key, in order of preference."""
        if key in SHARED_STATS:
            return (key, SHARED_STATS[key])
        return (key, _doubled(key))

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> int:
        """Checkpoint-named tensors (any float dtype, any device) -> fp32 device weights, in the reference loader's spelling or the decoder
        checkpoints' doubled `.conv.` one; the statistics also from the shared `audio_vae.per_channel_statistics.*`.  Keys absent from
        `sd` keep their values.  Returns the number of tensors taken."""
        n = 0
        for key, shape in self.expected_weight_shapes().items():
            src = next((k for k in self.checkpoint_keys(key) if k in sd), None)
            if src is None:
                continue
            t = sd[src].to(self.device, torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError(f"{src}: shape {tuple(t.shape)}, expected {shape}")
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
    def output_frames(self, t_mel: int) -> int:
        """Latent frames of t_mel mel frames (host only): each Downsample2d keeps (T - 1) // 2 + 1 rows."""
        t = int(t_mel)
        for _ in range(self.num_resolutions - 1):
            t = (t - 1) // 2 + 1
        return t

    def _conv(self, x, name, k, res=None, stride=1, act=nv.AUDIO_ACT_NONE):
        w = self._packed.get(PREFIX + name + ".weight")
        if w is None:
            raise RuntimeError(f"AudioEncoder: weight {PREFIX + name}.weight not loaded (load_audio_encoder_weights / init_random_weights)")
        pad = k - 1
        bias, c_out = self._w[PREFIX + name + ".bias"], self._w[PREFIX + name + ".weight"].shape[0]
        if stride == 1 and act == nv.AUDIO_ACT_NONE:
            return K.audio_conv2d(x, w, bias, c_out, k, k, pad, pad // 2, res=res)
        return K.audio_conv2d_strided(x, w, bias, c_out, k, k, pad, pad // 2, stride=(stride, stride), res=res, act=act)

    def _resblock(self, x, pre, c_in, c_out, act=nv.AUDIO_ACT_NONE):
        h = self._conv(K.audio_pixnorm_silu(x), f"{pre}.conv1", 3)
        skip = self._conv(x, f"{pre}.nin_shortcut", 1) if c_in != c_out else x
        return self._conv(K.audio_pixnorm_silu(h), f"{pre}.conv2", 3, res=skip, act=act)

    def __call__(self, spectrogram: torch.Tensor) -> torch.Tensor:
        """spectrogram (B, in_ch, T_mel, n_mels) -> latent (B, z_channels, output_frames(T_mel), n_mels / 4), fp32, normalised."""
        if not spectrogram.is_cuda or self.device.type != "cuda":
            raise RuntimeError("AudioEncoder runs on the MI355X only (no CPU fallback): a CUDA encoder and a CUDA tensor")
        spectrogram = spectrogram.float()
        b, c, _, _ = spectrogram.shape
        if c != self.in_ch:
            raise ValueError(f"AudioEncoder: {c} input channels, expected {self.in_ch}")
        base = self.ch * self.ch_mult[-1]
        stats = self.per_channel_statistics
        outs = []
        for i in range(b):
            h = self._conv(spectrogram[i].permute(1, 2, 0).contiguous(), "conv_in", 3)          # [T, mel, C]
            for lvl, blocks, down in self.levels:
                for pre, ci, co in blocks:
                    h = self._resblock(h, pre, ci, co)
                if down:
                    h = self._conv(h, f"down.{lvl}.downsample.conv", 3, stride=2)
            h = self._resblock(h, "mid.block_1", base, base)
            h = self._resblock(h, "mid.block_2", base, base, act=nv.AUDIO_ACT_SILU)               # the tail's silu(h), in conv2's epilogue
            h = self._conv(h, "conv_out", 3)                                                        # [T_a, F, 2z]
            if stats.mean_of_means.numel() != self.z_channels * h.shape[1]:
                raise ValueError(f"AudioEncoder: {h.shape[1]} latent mel bins x {self.z_channels} channels do not match the "
                                 f"{stats.mean_of_means.numel()} per-channel statistics")
            outs.append(K.audio_latent_normalize(h, stats.mean_of_means, stats.std_of_means, self.z_channels))
        return torch.stack(outs)


def load_audio_encoder_weights(encoder: AudioEncoder, weights_path: str) -> None:
    """`audio_vae.encoder.…` tensors of a safetensors checkpoint -> encoder (bf16 upcast), in either key spelling (see the module
    docstring); without any, the encoder is left as it was, as the reference's loader does."""
    from ...loader.weight_converter import SafetensorsStream
    print(f"  Loading audio encoder weights from {weights_path}...")
    with SafetensorsStream(weights_path, "cpu") as st:
        keys = set(st.keys())
        if not any(k.startswith(PREFIX) for k in keys):
            print("  Warning: No audio encoder keys found in weights file")
            return
        wanted = [k for key in encoder.expected_weight_shapes() for k in encoder.checkpoint_keys(key) if k in keys]
        n = encoder.load_state_dict(st.load(wanted))
    print(f"  Loaded {n} audio encoder weight tensors")


def encode_audio(spectrogram: torch.Tensor, encoder: AudioEncoder) -> torch.Tensor:
    """Mel spectrogram (B, 2, time, mel_bins) -> latent (B, z_channels, frames, mel_bins / 4) (reference encoder.py:306-320)."""
    return encoder(spectrogram)
