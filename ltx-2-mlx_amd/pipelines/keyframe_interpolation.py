"""Keyframe interpolation on MI355X: a video that passes through given images at given frames.

Mirrors reference LTX_2_MLX/pipelines/keyframe_interpolation.py:45-91 (KeyframeInterpolationConfig, Keyframe), :94-169 (the plain LANCZOS
loader, create_keyframe_conditionings), :223-296 (the guided loop) and :298-500 (__call__).  Every keyframe is encoded by the VAE encoder
and its tokens are APPENDED to the sequence (conditioning/keyframe.py), so the DiT runs on F*H*W + K*H*W tokens.
  stage 1: half resolution (full when use_two_stage=False), LTX2Scheduler over num_inference_steps, classifier-free guidance with
           CFGGuider(cfg_scale) on the video-only model -- pipelines.common.guided_denoise_loop: one C call per step or one captured graph;
  stage 2: un-normalise -> spatial upscaler -> normalise, keyframes re-encoded at full resolution and appended again, noise at
           STAGE_2_DISTILLED_SIGMA_VALUES[0], stage_2_steps steps without guidance (the captured conditioned loop), decode.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Union

import torch

from ..components import STAGE_2_DISTILLED_SIGMA_VALUES, CFGGuider, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier
from ..conditioning.keyframe import VideoConditionByKeyframeIndex
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from .common import (as_x0model, conditioned_initial_state, decode_video, final_latent, guided_denoise_loop, projected_denoise_loop, seeded_noiser, stage_callback,
                     upscale_latent_x2, video_tools_for)


@dataclass
class KeyframeInterpolationConfig:
    """Configuration of the keyframe interpolation pipeline (reference pipelines/keyframe_interpolation.py:45-82)."""
    height: int = 480
    width: int = 704
    num_frames: int = 97            # must be 8k + 1
    num_inference_steps: int = 30
    cfg_scale: float = 7.5
    seed: int = 42
    fps: float = 24.0
    use_two_stage: bool = True
    stage_2_steps: int = 3
    tiling_config: Optional[TilingConfig] = None
    dtype: torch.dtype = torch.float32
    use_hip_graph: bool = True      # MI355X addition: replay each stage's loop from one captured graph (no callback, < 64 steps)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}. Valid values: 1, 9, 17, 25, 33, ..., 121")
        if self.use_two_stage and (self.height % 64 != 0 or self.width % 64 != 0):
            raise ValueError(f"For two-stage pipeline, resolution ({self.height}x{self.width}) must be divisible by 64.")


@dataclass
class Keyframe:
    """An image the video passes through at `frame_index` (reference :85-91).  `image` may carry an already loaded tensor
    (1, 3, 1, H, W) in [-1, 1] instead of a path; it is resized to each stage's resolution."""
    image_path: Optional[str]
    frame_index: int
    strength: float = 0.95
    image: Optional[torch.Tensor] = None


def load_image_as_tensor(image_path: str, height: int, width: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """File -> (1, 3, 1, H, W) in [-1, 1]: RGB, a plain LANCZOS resize to (width, height) -- no aspect-preserving crop, unlike
    common.load_image_tensor (reference pipelines/keyframe_interpolation.py:94-126)."""
    import numpy as np
    from PIL import Image
    if not os.path.exists(image_path):
        raise FileNotFoundError(f"Image not found: {image_path}")
    img = Image.open(image_path).convert("RGB").resize((width, height), Image.Resampling.LANCZOS)
    arr = torch.from_numpy(np.array(img).astype(np.float32) / 127.5 - 1.0)
    return arr.permute(2, 0, 1)[None, :, None].to(dtype)


def _keyframe_image(kf: Keyframe, height: int, width: int, dtype: torch.dtype) -> torch.Tensor:
    if kf.image is None:
        return load_image_as_tensor(kf.image_path, height, width, dtype)
    img = kf.image.to(dtype)
    if img.dim() != 5 or img.shape[:3] != (1, 3, 1):
        raise ValueError(f"keyframe image must be (1, 3, 1, H, W), got {tuple(img.shape)}")
    if tuple(img.shape[-2:]) != (height, width):     # a preloaded tensor serves both stages: resized like the file would be
        img = torch.nn.functional.interpolate(img[:, :, 0], size=(height, width), mode="bilinear", align_corners=False, antialias=True)[:, :, None]
    return img


def create_keyframe_conditionings(keyframes: List[Keyframe], video_encoder, height: int, width: int,
                                  dtype: torch.dtype = torch.float32) -> List[VideoConditionByKeyframeIndex]:
    """Encode every keyframe with the VAE encoder into an appended-token conditioning (reference :129-169)."""
    if video_encoder is None:
        raise ValueError("keyframe conditioning needs a video_encoder")
    return [VideoConditionByKeyframeIndex(keyframes=video_encoder(_keyframe_image(kf, height, width, dtype)), frame_idx=kf.frame_index,
                                          strength=kf.strength) for kf in keyframes]


class KeyframeInterpolationPipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder, video_decoder: Optional[SimpleVideoDecoder],
                 spatial_upscaler: Optional[Callable] = None):
        self.transformer, _ = as_x0model(transformer)
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.spatial_upscaler = spatial_upscaler
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.diffusion_step = EulerDiffusionStep()
        self.token_counts: List[int] = []        # DiT tokens of each stage of the last call: F*H*W + K*H*W

    def _stage_state(self, keyframes, config, height, width, dev, initial_latent=None):
        tools = video_tools_for(self.patchifier, config.num_frames, height, width, config.fps)
        conds = create_keyframe_conditionings(keyframes, self.video_encoder, height, width, config.dtype)
        state = conditioned_initial_state(tools, conds, config.dtype, dev, initial_latent)
        self.token_counts.append(int(state.latent.shape[1]))
        return tools, state

    def denoise_latent(self, text_encoding: torch.Tensor, keyframes: List[Keyframe], config: KeyframeInterpolationConfig,
                       negative_text_encoding: Optional[torch.Tensor] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                       *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None, guider=None) -> torch.Tensor:
        """Both stages up to the final latent (1, 128, F, H/32, W/32).  initial_noise / stage2_noise (keyword-only, MI355X addition):
        supplied N(0,1) tensors of the patchified shapes INCLUDING the appended tokens, so results can be compared with a restatement.
        guider (keyword-only): replaces CFGGuider(config.cfg_scale) in stage 1 and runs through projected_denoise_loop."""
        for kf in keyframes:
            if not 0 <= kf.frame_index < config.num_frames:
                raise ValueError(f"keyframe frame_index {kf.frame_index} is outside [0, {config.num_frames})")
        if config.use_two_stage and self.spatial_upscaler is None:
            raise ValueError("Two-stage pipeline requires spatial_upscaler to be provided")
        dev = self.transformer.velocity_model.device
        ctx = text_encoding.to(dev)
        # no negative prompt: zeros of the context's shape (reference :326-330, create_null_text_encoding)
        nctx = torch.zeros_like(ctx) if negative_text_encoding is None else negative_text_encoding.to(dev)
        noiser = seeded_noiser(dev, config.seed)
        self.token_counts = []

        div = 2 if config.use_two_stage else 1
        tools, state = self._stage_state(keyframes, config, config.height // div, config.width // div, dev)
        sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
        state = noiser(state, noise_scale=1.0, noise=initial_noise)
        loop, stage1_guider = (guided_denoise_loop, CFGGuider(config.cfg_scale)) if guider is None else (projected_denoise_loop, guider)
        state = loop(self.transformer, state, sigmas, ctx, nctx, stage1_guider, self.diffusion_step, stage_callback(callback, "stage1"),
                     config.use_hip_graph)
        latent = final_latent(tools, state)
        if not config.use_two_stage:
            return latent

        upscaled = upscale_latent_x2(latent, self.spatial_upscaler, self.video_encoder, self.video_decoder)
        tools2, state2 = self._stage_state(keyframes, config, config.height, config.width, dev, initial_latent=upscaled)
        sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES[: config.stage_2_steps + 1]]
        state2 = noiser(state2, noise_scale=sig2[0], noise=stage2_noise)
        # refinement without guidance (reference :475-486, CFGGuider(1.0)): the existing conditioned loop, captured
        state2 = guided_denoise_loop(self.transformer, state2, sig2, ctx, None, CFGGuider(1.0), self.diffusion_step,
                                     stage_callback(callback, "stage2"), config.use_hip_graph)
        return final_latent(tools2, state2)

    def __call__(self, text_encoding: torch.Tensor, text_mask: Optional[torch.Tensor], keyframes: List[Keyframe],
                 config: KeyframeInterpolationConfig, negative_text_encoding: Optional[torch.Tensor] = None,
                 negative_text_mask: Optional[torch.Tensor] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                 *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None, guider=None) -> torch.Tensor:
        """-> uint8 frames (F, H, W, 3) (the final latent when no decoder is set).  The text masks are accepted and unused, as every loop
        here passes context_mask=None (reference pipelines/common.py:223-232).  guider (keyword-only): the guider of stage 1 instead of
        CFGGuider(config.cfg_scale), e.g. LtxAPGGuider."""
        latent = self.denoise_latent(text_encoding, keyframes, config, negative_text_encoding, callback, initial_noise=initial_noise,
                                     stage2_noise=stage2_noise, guider=guider)
        return decode_video(latent, self.video_decoder, config.tiling_config)           # no automatic tiling here


def create_keyframe_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler=None) -> KeyframeInterpolationPipeline:
    return KeyframeInterpolationPipeline(transformer, video_encoder, video_decoder, spatial_upscaler)
