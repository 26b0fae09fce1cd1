"""Two-stage text/image-to-video with sound on MI355X: CFG + modality-isolated guidance, then distilled refinement.

Mirrors reference LTX_2_MLX/pipelines/two_stage.py:88-141 (TwoStageCFGConfig), :158-199 (constructor), :314-401 (the joint guided loop) and
:495-804 (__call__): the reference CLI's `--pipeline two-stage` on an AudioVideo checkpoint.
  stage 1: half resolution, LTX2Scheduler over num_inference_steps, video and audio latent sampled jointly.  Per step the positive prompt, the
           negative prompt (CFG: cfg_scale on the video, audio_cfg_scale on the audio) and the positive prompt with every audio<->video
           cross-attention skipped (modality_scale on both), combined by MultiModalGuider.calculate and stepped by Euler --
           pipelines.common.multimodal_denoise_loop: one C call per step (that loop has no captured form);
  stage 2: un-normalise -> spatial upscaler -> normalise, image conditionings re-encoded at full size, both latents re-noised at
           STAGE_2_DISTILLED_SIGMA_VALUES[0] (the audio one is stage 1's: it is not upscaled), the distilled joint refinement steps without
           guidance, optionally under a distilled LoRA fused into the touched weights for this stage only; then the (tiled) decode, and with
           audio_enabled the audio VAE decoder and the vocoder.
An AudioVideo model is required: the reference's video-only branch (_denoise_loop_cfg) references an undefined `guider` and cannot run, so on
a video-only transformer this pipeline raises NotImplementedError rather than invent its behaviour.  With audio_enabled=False the audio latent
is still sampled (the reference's use_internal_audio_branch) and no waveform is returned.  rescale_scale (MI355X addition, default 0 as the
reference hardcodes) feeds both guiders; guidance_rescale is kept as a field and is unused on this path, as in the reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple, Union

import torch

from ..components import STAGE_2_DISTILLED_SIGMA_VALUES, AudioPatchifier, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier
from ..components.guiders import MultiModalGuider, MultiModalGuiderParams
from ..conditioning.tools import AudioLatentTools
from ..loader.lora_loader import LoRAConfig
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from ..types import AudioLatentShape, VideoPixelShape
from .common import (ImageCondition, as_x0model, auto_tiling_config, conditioned_initial_state, create_image_conditionings, decode_video,
                     final_latent, joint_denoise_loop, multimodal_denoise_loop, seeded_noiser, stage_callback, upscale_latent_x2, video_tools_for)
from .ti2vid_hq import fused_lora


@dataclass
class TwoStageCFGConfig:
    """Configuration of the two-stage CFG pipeline (reference pipelines/two_stage.py:88-141)."""
    height: int = 480
    width: int = 704
    num_frames: int = 97            # must be 8k + 1

    seed: int = 42
    fps: float = 25.0
    num_inference_steps: int = 30

    cfg_scale: float = 3.0
    audio_cfg_scale: float = 7.0
    guidance_rescale: float = 0.0   # unused on the AudioVideo path, as in the reference
    modality_scale: float = 3.0
    rescale_scale: float = 0.0      # MI355X addition: MultiModalGuiderParams.rescale_scale of both guiders (the reference hardcodes 0)

    distilled_lora_config: Optional[LoRAConfig] = None      # fused into the transformer for stage 2 only
    stage_2_sigmas: Optional[list] = None                   # None: STAGE_2_DISTILLED_SIGMA_VALUES
    tiling_config: Optional[TilingConfig] = None
    dtype: torch.dtype = torch.float32

    audio_enabled: bool = False
    use_internal_audio_branch: bool = True
    audio_vae_channels: int = 8
    audio_mel_bins: int = 16
    audio_sample_rate: int = 16000
    audio_hop_length: int = 160
    audio_downsample_factor: int = 4
    audio_output_sample_rate: int = 24000

    def _get_tiling_config(self) -> Optional[TilingConfig]:
        return auto_tiling_config(self.tiling_config, self.num_frames, self.height, self.width)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}. Valid values: 1, 9, 17, 25, 33, ..., 121")
        if self.height % 64 != 0 or self.width % 64 != 0:
            raise ValueError(f"Resolution ({self.height}x{self.width}) must be divisible by 64 for two-stage pipeline.")


class TwoStagePipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder, video_decoder: Optional[SimpleVideoDecoder],
                 spatial_upscaler: Optional[Callable], audio_decoder=None, vocoder=None):
        self.transformer, self.is_av_model = as_x0model(transformer)
        self._velocity_model = self.transformer.velocity_model
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.spatial_upscaler = spatial_upscaler
        self.audio_decoder = audio_decoder
        self.vocoder = vocoder
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.diffusion_step = EulerDiffusionStep()
        self.audio_latent: Optional[torch.Tensor] = None        # the final audio latent (1, 8, T_a, 16) of the last call

    def guiders(self, config: TwoStageCFGConfig) -> Tuple[MultiModalGuider, MultiModalGuider]:
        """(video guider, audio guider) as the reference builds them (:550-561), plus rescale_scale."""
        mk = lambda cfg: MultiModalGuider(params=MultiModalGuiderParams(cfg_scale=cfg, modality_scale=config.modality_scale,      # noqa: E731
                                                                        rescale_scale=config.rescale_scale))
        return mk(config.cfg_scale), mk(config.audio_cfg_scale)

    @staticmethod
    def _audio_tools(config: TwoStageCFGConfig, height: int, width: int) -> AudioLatentTools:
        pix = VideoPixelShape(batch=1, frames=config.num_frames, height=height, width=width, fps=config.fps)
        shape = AudioLatentShape.from_video_pixel_shape(pix, channels=config.audio_vae_channels, mel_bins=config.audio_mel_bins,
                                                        sample_rate=config.audio_sample_rate, hop_length=config.audio_hop_length,
                                                        audio_latent_downsample_factor=config.audio_downsample_factor)
        return AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=shape)

    def _check(self, config: TwoStageCFGConfig, positive_audio_encoding, negative_audio_encoding) -> None:
        if not self.is_av_model:
            raise NotImplementedError("TwoStagePipeline needs an AudioVideo model: the reference's video-only branch (_denoise_loop_cfg) references an "
                                      "undefined `guider` and cannot run, so there is no behaviour to reproduce on a video-only transformer")
        if positive_audio_encoding is None or negative_audio_encoding is None:
            raise ValueError("Audio encoding required for AudioVideo generation. Provide positive_audio_encoding and negative_audio_encoding.")
        if config.audio_enabled and (self.audio_decoder is None or self.vocoder is None):
            raise ValueError("Audio decoder and vocoder required when audio_enabled is True.")

    def stage1_latent(self, positive_encoding: torch.Tensor, negative_encoding: torch.Tensor, config: TwoStageCFGConfig,
                      images: Optional[List[ImageCondition]] = None, callback=None, positive_audio_encoding: Optional[torch.Tensor] = None,
                      negative_audio_encoding: Optional[torch.Tensor] = None, *, initial_noise: Optional[torch.Tensor] = None,
                      initial_audio_noise: Optional[torch.Tensor] = None, noiser=None, fused: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Stage 1 alone: (the half-resolution latent (1, 128, F, H/64, W/64), the audio latent (1, 8, T_a, 16)) after the joint guided loop
        (the audio is noised after the video, reference :601-618)."""
        self._check(config, positive_audio_encoding, negative_audio_encoding)
        dev = self._velocity_model.device
        noiser = noiser or seeded_noiser(dev, config.seed)
        h1, w1 = config.height // 2, config.width // 2
        tools = video_tools_for(self.patchifier, config.num_frames, h1, w1, config.fps)
        conds = create_image_conditionings(images or [], self.video_encoder, h1, w1, config.dtype)
        state = conditioned_initial_state(tools, conds, config.dtype, dev)
        sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
        state = noiser(state, noise_scale=1.0, noise=initial_noise)
        atools = self._audio_tools(config, h1, w1)
        astate = noiser(atools.create_initial_state(dtype=config.dtype, device=dev), noise_scale=1.0, noise=initial_audio_noise)
        vg, ag = self.guiders(config)
        state, astate = multimodal_denoise_loop(self.transformer, state, astate, sigmas, positive_encoding.to(dev), positive_audio_encoding.to(dev),
                                                negative_encoding.to(dev), negative_audio_encoding.to(dev), vg, ag, stage_callback(callback, "stage1"),
                                                fused=fused)
        return final_latent(tools, state), final_latent(atools, astate)

    def denoise_latent(self, positive_encoding: torch.Tensor, negative_encoding: torch.Tensor, config: TwoStageCFGConfig,
                       images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                       positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None, *,
                       initial_noise: Optional[torch.Tensor] = None, stage_2_noise: Optional[torch.Tensor] = None,
                       initial_audio_noise: Optional[torch.Tensor] = None, stage_2_audio_noise: Optional[torch.Tensor] = None,
                       fused: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Both stages up to (the final latent (1, 128, F, H/32, W/32), the final audio latent (1, 8, T_a, 16)).  initial_noise / stage_2_noise
        and their audio counterparts (keyword-only, MI355X addition): supplied N(0,1) tensors of the patchified shapes."""
        if self.spatial_upscaler is None:
            raise ValueError("TwoStagePipeline requires spatial_upscaler to be provided")
        self._check(config, positive_audio_encoding, negative_audio_encoding)
        images = images or []
        dev = self._velocity_model.device
        noiser = seeded_noiser(dev, config.seed)
        latent, audio_latent = self.stage1_latent(positive_encoding, negative_encoding, config, images, callback, positive_audio_encoding,
                                                  negative_audio_encoding, initial_noise=initial_noise, initial_audio_noise=initial_audio_noise,
                                                  noiser=noiser, fused=fused)
        print("  Upsampling latent 2x with spatial upscaler...")
        upscaled = upscale_latent_x2(latent, self.spatial_upscaler, self.video_encoder, self.video_decoder)
        with fused_lora(self._velocity_model, config.distilled_lora_config):
            tools2 = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
            conds2 = create_image_conditionings(images, self.video_encoder, config.height, config.width, config.dtype)
            state2 = conditioned_initial_state(tools2, conds2, config.dtype, dev, initial_latent=upscaled)
            sig2 = [float(s) for s in (config.stage_2_sigmas if config.stage_2_sigmas is not None else STAGE_2_DISTILLED_SIGMA_VALUES)]
            state2 = noiser(state2, noise_scale=sig2[0], noise=stage_2_noise)
            # no spatial upscaling for audio: stage 1's latent is re-noised (reference :737-754) and refined jointly, without guidance (:441-493)
            atools2 = self._audio_tools(config, config.height, config.width)
            astate2 = noiser(atools2.create_initial_state(dtype=config.dtype, device=dev, initial_latent=audio_latent), noise_scale=sig2[0],
                             noise=stage_2_audio_noise)
            state2, astate2 = joint_denoise_loop(self.transformer, True, state2, astate2, sig2, positive_encoding.to(dev), positive_audio_encoding.to(dev),
                                                 self.diffusion_step, stage_callback(callback, "stage2"), False)
        return final_latent(tools2, state2), final_latent(atools2, astate2)

    def __call__(self, positive_encoding: torch.Tensor, negative_encoding: torch.Tensor, config: TwoStageCFGConfig,
                 images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                 positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None, *,
                 initial_noise: Optional[torch.Tensor] = None, stage_2_noise: Optional[torch.Tensor] = None,
                 initial_audio_noise: Optional[torch.Tensor] = None, stage_2_audio_noise: Optional[torch.Tensor] = None, fused: bool = True):
        """-> (uint8 frames (F, H, W, 3), or the final latent when no decoder is set; the waveform (B, 2, samples) with config.audio_enabled,
        else None) (reference :790-804).  The final audio latent is kept in self.audio_latent either way."""
        latent, audio_latent = self.denoise_latent(positive_encoding, negative_encoding, config, images, callback, positive_audio_encoding,
                                                   negative_audio_encoding, initial_noise=initial_noise, stage_2_noise=stage_2_noise,
                                                   initial_audio_noise=initial_audio_noise, stage_2_audio_noise=stage_2_audio_noise, fused=fused)
        self.audio_latent = audio_latent
        video = decode_video(latent, self.video_decoder, config._get_tiling_config())
        return video, (self.vocoder(self.audio_decoder(audio_latent)) if config.audio_enabled else None)


def create_two_stage_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder=None, vocoder=None) -> TwoStagePipeline:
    return TwoStagePipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder, vocoder)
