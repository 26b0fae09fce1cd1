"""High-quality two-stage text/image-to-video on MI355X: the res_2s second-order sampler.

Mirrors reference LTX_2_MLX/pipelines/ti2vid_hq.py:52-97 (TI2VidHQConfig), :100-136 (constructor), :153-273 (the res_2s loop) and
:360-531 (__call__).  15 second-order steps do what the Euler pipelines need 30 for.
  stage 1: half resolution, LTX2Scheduler over num_inference_steps, classifier-free guidance in the HQ pipeline's own form
           (uncond + scale * (cond - uncond)) inside the res_2s step -- pipelines.common.res2s_denoise_loop: one C call per step or one
           captured graph;
  stage 2: un-normalise -> spatial upscaler -> normalise, image conditionings re-encoded at full size, noise at
           STAGE_2_DISTILLED_SIGMA_VALUES[0], the distilled refinement steps without guidance (the captured conditioned loop),
           optionally under a distilled LoRA fused into the touched weights for this stage only; then the (tiled) decode.
Video only: the joint audio branch of the res_2s loop is not built, audio_enabled=True raises NotImplementedError.  An AudioVideo
checkpoint runs through its video twin.  The reference constructs a Res2sDiffusionStep (SDE noise) and never calls it: not built.
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch

from ..components import STAGE_2_DISTILLED_SIGMA_VALUES, EulerDiffusionStep, GaussianNoiser, LTX2Scheduler, VideoLatentPatchifier
from ..loader.lora_loader import LoRAConfig, find_lora_keys_for_weight, fuse_lora_into_weights
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from .common import (ImageCondition, as_x0model, auto_tiling_config, conditioned_initial_state, create_image_conditionings, decode_video,
                     final_latent, joint_denoise_loop, res2s_denoise_loop, seeded_noiser, stage_callback, upscale_latent_x2, video_tools_for)


@dataclass
class TI2VidHQConfig:
    """Configuration of the HQ two-stage pipeline (reference pipelines/ti2vid_hq.py:52-97)."""
    height: int = 1088
    width: int = 1920
    num_frames: int = 97            # must be 8k + 1
    num_inference_steps: int = 15
    cfg_scale: float = 3.0
    audio_cfg_scale: float = 7.0
    guidance_rescale: float = 0.45
    seed: int = 42
    fps: float = 25.0
    distilled_lora_config: Optional[LoRAConfig] = None      # fused into the transformer for stage 2 only
    tiling_config: Optional[TilingConfig] = None
    dtype: torch.dtype = torch.float32      # (the reference's mx.float16: this engine steps fp32 latents)
    audio_enabled: bool = False
    use_internal_audio_branch: bool = True
    audio_vae_channels: int = 8
    audio_mel_bins: int = 16
    audio_sample_rate: int = 16000
    audio_hop_length: int = 160
    audio_downsample_factor: int = 4
    audio_output_sample_rate: int = 24000
    use_hip_graph: bool = True      # MI355X addition: replay each stage's loop from one captured graph (no callback, < 64 steps)

    def _get_tiling_config(self) -> Optional[TilingConfig]:
        return auto_tiling_config(self.tiling_config, self.num_frames, self.height, self.width)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}")
        if self.height % 64 != 0 or self.width % 64 != 0:
            raise ValueError(f"Resolution ({self.height}x{self.width}) must be divisible by 64.")


# ---------------------------------------------------------------------- the distilled LoRA of stage 2
_PACKED = {"to_qkv": ("to_q", "to_k", "to_v"), "to_kv": ("to_k", "to_v")}


def checkpoint_views(name: str, t: torch.Tensor) -> List[Tuple[str, torch.Tensor]]:
    """An engine-layout linear weight as (checkpoint key, row-slice view) pairs: LTXModel packs q/k/v (k/v) of an attention into one
    tensor, LoRA files address the parts."""
    mod, leaf = name.rsplit(".", 1)
    parent, last = mod.rsplit(".", 1) if "." in mod else ("", mod)
    parts = _PACKED.get(last)
    if parts is None:
        return [(name, t)]
    rows = t.shape[0] // len(parts)
    return [(f"{parent}.{p}.{leaf}", t[i * rows: (i + 1) * rows]) for i, p in enumerate(parts)]


def lora_touched(weights: Dict[str, torch.Tensor], lora_keys) -> Dict[str, List[Tuple[str, torch.Tensor]]]:
    """Engine-layout 2-D weights that `lora_keys` (the names in a LoRA file) address through at least one part."""
    names = dict.fromkeys(lora_keys)
    out = {}
    for name, t in weights.items():
        if t.dim() != 2 or not name.endswith(".weight"):
            continue
        views = checkpoint_views(name, t)
        if any(find_lora_keys_for_weight(names, k)[0] is not None for k, _ in views):
            out[name] = views
    return out


@contextmanager
def fused_lora(model, lora_config: Optional[LoRAConfig], fuse: Callable = fuse_lora_into_weights, lora_keys=None):
    """Within the block, `model` (an LTXModel) runs with `lora_config` fused into the linear weights it touches; on exit the original
    tensors are registered again (in a finally).  Only the touched tensors are kept aside, not a second copy of the model.
    `fuse` (default loader.fuse_lora_into_weights) and `lora_keys` (default: the names in the file) can be supplied by a caller that
    holds the adapter already."""
    if lora_config is None:
        yield
        return
    weights = model.weight_tensors()
    if any(t.dtype == torch.uint8 for t in weights.values()):
        raise NotImplementedError("LoRA fusion needs dequantised weights: drop fp8_resident")
    if lora_keys is None:
        from safetensors import safe_open
        with safe_open(lora_config.path, framework="pt") as f:
            lora_keys = list(f.keys())
    touched = lora_touched(weights, lora_keys)
    if not touched:
        yield
        return
    originals = {name: weights[name] for name in touched}
    parts = fuse({k: v for views in touched.values() for k, v in views}, [lora_config])
    model.replace_weights({name: torch.cat([parts[k] for k, _ in views], 0) if len(views) > 1 else parts[views[0][0]]
                           for name, views in touched.items()})
    try:
        yield
    finally:
        model.replace_weights(originals)


class TI2VidHQPipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder, video_decoder: Optional[SimpleVideoDecoder],
                 spatial_upscaler: Optional[Callable], audio_decoder=None, vocoder=None):
        self.transformer, self.is_av_model = as_x0model(transformer)
        self._velocity_model = self.transformer.velocity_model
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.spatial_upscaler = spatial_upscaler
        self.audio_decoder = audio_decoder          # accepted for the reference's signature; this pipeline is video-only
        self.vocoder = vocoder
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.euler_step = EulerDiffusionStep()

    def stage1_latent(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: TI2VidHQConfig,
                      images: Optional[List[ImageCondition]] = None, callback=None, *, initial_noise: Optional[torch.Tensor] = None,
                      noiser: Optional[GaussianNoiser] = None) -> torch.Tensor:
        """Stage 1 alone: the half-resolution latent (1, 128, F, H/64, W/64) after the guided res_2s loop."""
        if config.audio_enabled:
            raise NotImplementedError("TI2VidHQPipeline is video-only here: the joint audio branch of the res_2s loop is not built")
        dev = self._velocity_model.device
        noiser = noiser or seeded_noiser(dev, config.seed)
        h1, w1 = config.height // 2, config.width // 2
        tools = video_tools_for(self.patchifier, config.num_frames, h1, w1, config.fps)
        conds = create_image_conditionings(images or [], self.video_encoder, h1, w1, config.dtype)
        state = conditioned_initial_state(tools, conds, config.dtype, dev)
        sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
        state = noiser(state, noise_scale=1.0, noise=initial_noise)
        nctx = None if negative_encoding is None else negative_encoding.to(dev)
        state = res2s_denoise_loop(self.transformer, state, sigmas, positive_encoding.to(dev), nctx, config.cfg_scale, config.audio_cfg_scale,
                                   stage_callback(callback, "stage1_res2s"), config.use_hip_graph)
        return final_latent(tools, state)

    def denoise_latent(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: TI2VidHQConfig,
                       images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                       *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Both stages up to the final latent (1, 128, F, H/32, W/32).  initial_noise / stage2_noise (keyword-only, MI355X addition):
        supplied N(0,1) tensors of the patchified shapes, so results can be compared with a restatement."""
        if self.spatial_upscaler is None:
            raise ValueError("TI2VidHQPipeline requires spatial_upscaler to be provided")
        images = images or []
        dev = self._velocity_model.device
        ctx = positive_encoding.to(dev)
        noiser = seeded_noiser(dev, config.seed)
        latent = self.stage1_latent(ctx, negative_encoding, config, images, callback, initial_noise=initial_noise, noiser=noiser)

        upscaled = upscale_latent_x2(latent, self.spatial_upscaler, self.video_encoder, self.video_decoder)
        with fused_lora(self._velocity_model, config.distilled_lora_config):
            tools2 = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
            conds2 = create_image_conditionings(images, self.video_encoder, config.height, config.width, config.dtype)
            state2 = conditioned_initial_state(tools2, conds2, config.dtype, dev, initial_latent=upscaled)
            sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES]
            state2 = noiser(state2, noise_scale=sig2[0], noise=stage2_noise)
            # refinement without guidance (reference :321-358, :499-503): the existing conditioned loop, captured; no audio state, so an
            # AudioVideo model runs through its video twin
            state2 = joint_denoise_loop(self.transformer, self.is_av_model, state2, None, sig2, ctx, None, self.euler_step,
                                        stage_callback(callback, "stage2"), config.use_hip_graph)[0]
        return final_latent(tools2, state2)

    def __call__(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: TI2VidHQConfig,
                 images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                 positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None,
                 *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> uint8 frames (F, H, W, 3) (the final latent when no decoder is set).  The audio encodings are accepted for the reference's
        signature and unused: this pipeline is video-only."""
        latent = self.denoise_latent(positive_encoding, negative_encoding, config, images, callback, initial_noise=initial_noise,
                                     stage2_noise=stage2_noise)
        return decode_video(latent, self.video_decoder, config._get_tiling_config())


def create_ti2vid_hq_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder=None, vocoder=None) -> TI2VidHQPipeline:
    return TI2VidHQPipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder, vocoder)
