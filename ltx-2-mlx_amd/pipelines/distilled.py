"""Distilled generation pipeline on MI355X (video path).

Mirrors reference LTX_2_MLX/pipelines/distilled.py:48-98 (DistilledConfig), :101-143
(constructor), :198-272 (_denoise_loop_av, video branch) and :274-505 (__call__): stage 1 at half
resolution with DISTILLED_SIGMA_VALUES (8 steps), optional latent 2x upscale + stage 2 with
STAGE_2_DISTILLED_SIGMA_VALUES (3 steps), then VAE decode (tiled above 4000 latent voxels).
The joint audio+video branch runs on AudioVideo transformers and returns the audio waveform when an audio_decoder and a
vocoder are given (model/audio_vae/), the audio latent otherwise.  Image conditioning encodes the image with the VAE encoder
and runs the per-token-sigma path of the DiT.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Union

import torch

from ..components import DISTILLED_SIGMA_VALUES, STAGE_2_DISTILLED_SIGMA_VALUES, AudioPatchifier, EulerDiffusionStep, VideoLatentPatchifier
from ..conditioning.tools import AudioLatentTools
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from ..types import AudioLatentShape, LatentState, VideoPixelShape
from .common import (as_x0model, auto_tiling_config, conditioned_initial_state, create_image_conditionings, decode_video, final_latent,
                     ancestral_denoise_loop, joint_denoise_loop, seeded_noiser, stage_callback, upscale_latent_x2, video_tools_for)


@dataclass
class DistilledConfig:
    height: int = 480
    width: int = 704
    num_frames: int = 97          # must be 8k + 1
    seed: int = 42
    fps: float = 25.0
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
    use_hip_graph: bool = False    # MI355X addition: replay the captured step loop (uniform sigma only)
    sampler: str = "euler"         # "euler_ancestral": stage 1 through EulerAncestralDiffusionStep's loop (reference pipelines/distilled.py:140-143);
    ancestral_eta: float = 1.0     #   stage 2 stays plain Euler, as the reference's constructor comments say.  The noise seed is `seed`.

    def _get_tiling_config(self) -> Optional[TilingConfig]:
        return auto_tiling_config(self.tiling_config, self.num_frames, self.height, self.width)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}. Valid values: 1, 9, 17, 25, 33, ..., 121")
        if self.height % 64 != 0 or self.width % 64 != 0:
            raise ValueError(f"Resolution ({self.height}x{self.width}) must be divisible by 64 for two-stage pipeline.")
        if self.sampler not in ("euler", "euler_ancestral"):
            raise ValueError(f"sampler={self.sampler!r}: the distilled pipeline runs 'euler' or 'euler_ancestral'")


class DistilledPipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder=None, video_decoder: Optional[SimpleVideoDecoder] = None,
                 spatial_upscaler: Optional[Callable] = None, audio_decoder=None, vocoder=None):
        self.transformer, self.is_av_model = as_x0model(transformer)
        self.audio_decoder = audio_decoder
        self.vocoder = vocoder
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.spatial_upscaler = spatial_upscaler
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.diffusion_step = EulerDiffusionStep()

    def _create_audio_tools(self, target_shape: AudioLatentShape) -> AudioLatentTools:
        return AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=target_shape)

    @staticmethod
    def _channelwise_normalize_audio(latent: torch.Tensor) -> torch.Tensor:
        """Length-invariant audio noise (reference pipelines/distilled.py:165-187): global zero-mean / unit-std
        (population std), then per-feature standardisation over the token axis."""
        x = (latent - latent.mean()) / (latent.std(unbiased=False) + 1e-8)
        return (x - x.mean(dim=1, keepdim=True)) / (x.std(dim=1, keepdim=True, unbiased=False) + 1e-8)

    def _denoise_loop_av(self, video_state: LatentState, audio_state: Optional[LatentState], sigmas: Sequence[float],
                         video_context: torch.Tensor, audio_context: Optional[torch.Tensor] = None,
                         stepper: Optional[EulerDiffusionStep] = None, callback: Optional[Callable[[int, int], None]] = None,
                         use_hip_graph: bool = False):
        """Joint audio+video loop (reference pipelines/distilled.py:198-271): see pipelines.common.joint_denoise_loop."""
        return joint_denoise_loop(self.transformer, self.is_av_model, video_state, audio_state, sigmas, video_context, audio_context,
                                  stepper or self.diffusion_step, callback, use_hip_graph)

    def __call__(self, text_encoding: torch.Tensor, text_mask: Optional[torch.Tensor], config: DistilledConfig,
                 images: Optional[List] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                 audio_encoding: Optional[torch.Tensor] = None, initial_noise: Optional[torch.Tensor] = None,
                 initial_audio_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None):
        """Returns the decoded video (uint8 frames, or the final latent when no decoder is set); with
        config.audio_enabled on an AudioVideo model, the tuple (video, audio): the waveform (B, 2, samples) when both audio_decoder and
        vocoder were given (the reference's _decode_audio, distilled.py:188-196), the (B, 8, T_a, 16) latent without them."""
        images = images or []
        dev = self.transformer.velocity_model.device
        noiser = seeded_noiser(dev, config.seed)
        audio_active = self.is_av_model and (config.use_internal_audio_branch or config.audio_enabled)
        if config.audio_enabled and not self.is_av_model:
            raise ValueError("audio_enabled needs an AudioVideo transformer")
        actx = audio_encoding.to(dev) if audio_encoding is not None else None

        def audio_shape(height: int, width: int) -> AudioLatentShape:
            pix = VideoPixelShape(batch=1, frames=config.num_frames, height=height, width=width, fps=config.fps)
            return AudioLatentShape.from_video_pixel_shape(pix, channels=config.audio_vae_channels, mel_bins=config.audio_mel_bins,
                                                           sample_rate=config.audio_sample_rate, hop_length=config.audio_hop_length,
                                                           audio_latent_downsample_factor=config.audio_downsample_factor)

        h1, w1 = config.height // 2, config.width // 2
        tools = video_tools_for(self.patchifier, config.num_frames, h1, w1, config.fps)
        # image conditioning at stage-1 resolution: encoded latent replaces the tokens of its latent frame and
        # lowers their denoise mask (reference pipelines/distilled.py:326-333)
        state = conditioned_initial_state(tools, create_image_conditionings(images, self.video_encoder, h1, w1, config.dtype), config.dtype, dev)
        state = noiser(state, noise_scale=1.0, noise=initial_noise)
        astate, atools = None, None
        if audio_active:
            atools = self._create_audio_tools(audio_shape(h1, w1))
            astate = noiser(atools.create_initial_state(dtype=config.dtype, device=dev), noise_scale=1.0, noise=initial_audio_noise)
            astate = astate.replace(latent=self._channelwise_normalize_audio(astate.latent))
        if config.sampler == "euler_ancestral":
            state, astate = ancestral_denoise_loop(self.transformer, state, astate, DISTILLED_SIGMA_VALUES, text_encoding.to(dev), actx,
                                                   eta=config.ancestral_eta, seed=config.seed, callback=stage_callback(callback, "stage1"),
                                                   use_hip_graph=config.use_hip_graph)
        else:
            state, astate = self._denoise_loop_av(state, astate, DISTILLED_SIGMA_VALUES, text_encoding.to(dev), actx,
                                                  callback=stage_callback(callback, "stage1"), use_hip_graph=config.use_hip_graph)
        latent = final_latent(tools, state)
        audio_latent = final_latent(atools, astate) if astate is not None else None

        if self.spatial_upscaler is not None:
            up = upscale_latent_x2(latent, self.spatial_upscaler, self.video_encoder, self.video_decoder)
            tools2 = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
            conds2 = create_image_conditionings(images, self.video_encoder, config.height, config.width, config.dtype)
            state2 = conditioned_initial_state(tools2, conds2, config.dtype, dev, initial_latent=up)
            sigma0 = float(STAGE_2_DISTILLED_SIGMA_VALUES[0])
            state2 = noiser(state2, noise_scale=sigma0, noise=stage2_noise)
            astate2, atools2 = None, None
            if audio_active:        # no spatial upscaling for audio: stage 1's latent is re-noised (reference :441-458)
                atools2 = self._create_audio_tools(audio_shape(config.height, config.width))
                astate2 = noiser(atools2.create_initial_state(dtype=config.dtype, initial_latent=audio_latent), noise_scale=sigma0)
            state2, astate2 = self._denoise_loop_av(state2, astate2, STAGE_2_DISTILLED_SIGMA_VALUES, text_encoding.to(dev), actx,
                                                    callback=stage_callback(callback, "stage2"), use_hip_graph=config.use_hip_graph)
            latent = final_latent(tools2, state2)
            if astate2 is not None:
                audio_latent = final_latent(atools2, astate2)

        video = decode_video(latent, self.video_decoder, config._get_tiling_config())
        if config.audio_enabled and audio_latent is not None:
            audio = self._decode_audio(audio_latent)
            return video, (audio if audio is not None else audio_latent)
        return (video, audio_latent) if config.audio_enabled else video

    def _decode_audio(self, audio_latent: torch.Tensor) -> Optional[torch.Tensor]:
        """Audio latent -> waveform (B, 2, samples) through the audio VAE decoder and the vocoder; None when either is missing."""
        if self.audio_decoder is None or self.vocoder is None:
            return None
        return self.vocoder(self.audio_decoder(audio_latent))


def create_distilled_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler=None, audio_decoder=None, vocoder=None):
    return DistilledPipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder, vocoder)
