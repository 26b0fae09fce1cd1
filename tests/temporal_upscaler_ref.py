"""fp32 torch restatement of the reference's temporal x2 latent upscaler (LTX_2_MLX/model/upscaler/temporal.py), the checker of
tests/test_temporal_upscaler_{cpu,gpu}.py.  Two semantics, as ltx_2_mlx_amd.model.upscaler.TemporalUpscaler:

  checkpoint_semantics=False  what the reference computes: GroupNorm per frame over MLX's default (interleaved) groups, shuffle
                              reading channel p * C + c
  checkpoint_semantics=True   what the upstream PyTorch model computes: torch.nn.GroupNorm on the 5-D tensor, shuffle
                              "b (c p1) f h w -> b c (f p1) h w" (channel 2c + p)

tests/golden/temporal_upscaler_tiny.npz pins the first against the reference's own code (tools/pin_temporal_upscaler_against_reference.py).
"""
from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn.functional as F


@dataclass
class TemporalUpscalerConfig:
    """Constructor keywords of the reference (temporal.py:234-240)."""
    latent_channels: int = 128
    hidden_channels: int = 512
    num_res_blocks: int = 4
    num_groups: int = 32
    eps: float = 1e-5           # mlx.nn.GroupNorm default


TINY = TemporalUpscalerConfig(latent_channels=64, hidden_channels=64, num_res_blocks=1, num_groups=32)
TINY_SEED, TINY_INPUT_SEED, TINY_INPUT_SHAPE = 5, 6, (1, 64, 3, 5, 6)


def weight_shapes(cfg: TemporalUpscalerConfig) -> Dict[str, tuple]:
    """Checkpoint keys and shapes (load_temporal_upscaler_weights, temporal.py:345-416)."""
    c, m = cfg.latent_channels, cfg.hidden_channels
    s = {"initial_conv.weight": (m, c, 3, 3, 3), "initial_conv.bias": (m,), "initial_norm.weight": (m,), "initial_norm.bias": (m,),
         "upsampler.0.weight": (2 * m, m, 3, 3, 3), "upsampler.0.bias": (2 * m,), "final_conv.weight": (c, m, 3, 3, 3), "final_conv.bias": (c,)}
    for stage in ("res_blocks", "post_upsample_res_blocks"):
        for i in range(cfg.num_res_blocks):
            for cv in ("conv1", "conv2"):
                s[f"{stage}.{i}.{cv}.weight"] = (m, m, 3, 3, 3)
                s[f"{stage}.{i}.{cv}.bias"] = (m,)
            for nm in ("norm1", "norm2"):
                s[f"{stage}.{i}.{nm}.weight"] = (m,)
                s[f"{stage}.{i}.{nm}.bias"] = (m,)
    return s


def make_weights(cfg: TemporalUpscalerConfig, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded weights: convs at 1/sqrt(fan_in), norm weights around 1, biases small but non-zero."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in weight_shapes(cfg).items():
        if "norm" in k:
            sd[k] = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            sd[k] = 0.02 * torch.randn(shp, generator=g)
        else:
            sd[k] = torch.randn(shp, generator=g) / (shp[1] * 27) ** 0.5
    return sd


def tiny_input() -> torch.Tensor:
    return torch.randn(TINY_INPUT_SHAPE, generator=torch.Generator().manual_seed(TINY_INPUT_SEED))


def conv3d(x, w, b):
    """3x3x3, zero padding 1 in T/H/W (temporal.py:20-91, padding=1)."""
    return F.conv3d(x, w, b, padding=1)


def group_norm_frames(x, weight, bias, groups, eps, interleaved=True):
    """temporal.py:130-135 / 279-284: (B, C, T, H, W) -> (B*T, H, W, C) -> mlx.nn.GroupNorm: statistics per frame.  MLX's default
    GroupNorm reshapes the channel axis to (..., groups): group of channel c = c % groups (interleaved); interleaved=False is the
    pytorch_compatible grouping c // (C // groups), per frame."""
    b, c, t, h, w = x.shape
    v = x.permute(0, 2, 3, 4, 1).reshape(b * t, h * w, c)
    g = v.reshape(b * t, -1, groups) if interleaved else v.reshape(b * t, h * w, groups, c // groups)
    dims = (1,) if interleaved else (1, 3)
    mean = g.mean(dim=dims, keepdim=True)
    var = g.var(dim=dims, keepdim=True, unbiased=False)
    y = ((g - mean) * torch.rsqrt(var + eps)).reshape(b * t, h * w, c) * weight + bias
    return y.reshape(b, t, h, w, c).permute(0, 4, 1, 2, 3)


def group_norm(x, weight, bias, cfg, checkpoint_semantics):
    if checkpoint_semantics:        # upstream: torch.nn.GroupNorm(groups, C) on (B, C, T, H, W)
        return F.group_norm(x, cfg.num_groups, weight, bias, cfg.eps)
    return group_norm_frames(x, weight, bias, cfg.num_groups, cfg.eps, interleaved=True)


def res_block(x, w, prefix, cfg, checkpoint_semantics):
    """conv1 -> norm1 -> SiLU -> conv2 -> norm2 -> SiLU(x + residual)  (temporal.py:117-149)."""
    h = conv3d(x, w[prefix + ".conv1.weight"], w[prefix + ".conv1.bias"])
    h = F.silu(group_norm(h, w[prefix + ".norm1.weight"], w[prefix + ".norm1.bias"], cfg, checkpoint_semantics))
    h = conv3d(h, w[prefix + ".conv2.weight"], w[prefix + ".conv2.bias"])
    h = group_norm(h, w[prefix + ".norm2.weight"], w[prefix + ".norm2.bias"], cfg, checkpoint_semantics)
    return F.silu(h + x)


def temporal_pixel_shuffle(x, checkpoint_semantics=False):
    """(B, 2C, T, H, W) -> (B, C, 2T, H, W).  Reference (temporal.py:204-213): reshape (b, r, c_out, ...) -> out[c, 2t + p] =
    in[p * C + c, t].  Upstream rearrange "b (c p1) f h w -> b c (f p1) h w": out[c, 2t + p] = in[2c + p, t]."""
    b, c2, t, h, w = x.shape
    c = c2 // 2
    if checkpoint_semantics:
        return x.reshape(b, c, 2, t, h, w).permute(0, 1, 3, 2, 4, 5).reshape(b, c, 2 * t, h, w)
    return x.reshape(b, 2, c, t, h, w).permute(0, 2, 3, 1, 4, 5).reshape(b, c, 2 * t, h, w)


def forward(x, w, cfg: TemporalUpscalerConfig, checkpoint_semantics: bool = False):
    """TemporalUpscaler.__call__ (temporal.py:265-307): (B, C, F, H, W) -> (B, C, 2F - 1, H, W)."""
    x = conv3d(x, w["initial_conv.weight"], w["initial_conv.bias"])
    x = F.silu(group_norm(x, w["initial_norm.weight"], w["initial_norm.bias"], cfg, checkpoint_semantics))
    for i in range(cfg.num_res_blocks):
        x = res_block(x, w, f"res_blocks.{i}", cfg, checkpoint_semantics)
    x = conv3d(x, w["upsampler.0.weight"], w["upsampler.0.bias"])           # temporal.py:184
    x = temporal_pixel_shuffle(x, checkpoint_semantics)[:, :, 1:]           # temporal.py:188, 296: first frame dropped
    for i in range(cfg.num_res_blocks):
        x = res_block(x, w, f"post_upsample_res_blocks.{i}", cfg, checkpoint_semantics)
    return conv3d(x, w["final_conv.weight"], w["final_conv.bias"])


def upscale_latent_temporal(latent, w, cfg, mean, std, checkpoint_semantics: bool = False):
    """un-normalise -> upscale -> re-normalise (reference scripts/generate.py:2052-2066)."""
    m, s = mean.reshape(1, -1, 1, 1, 1), std.reshape(1, -1, 1, 1, 1)
    return (forward(latent * s + m, w, cfg, checkpoint_semantics) - m) / s
