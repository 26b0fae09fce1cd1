"""Audio-to-video two-stage pipeline on MI355X: a video generated TO a given audio track.

Mirrors reference LTX_2_MLX/pipelines/a2vid_two_stage.py:49-93 (A2VidConfig), :169-198 (constructor), :225-271 (the video-only loop) and
:273-464 (__call__).
  stage 1: half resolution, LTX2Scheduler over num_inference_steps on the AudioVideo model, the encoded audio latent frozen (denoise_mask = 0,
           never noised, never stepped), classifier-free guidance on the video alone -- pipelines.common.frozen_audio_guided_loop: one C call
           per step or one captured graph;
  stage 2: un-normalise -> spatial upscaler -> normalise, image conditionings re-encoded at full size, noise at
           STAGE_2_DISTILLED_SIGMA_VALUES[0], the distilled refinement steps without guidance (the captured frozen-audio loop), optionally
           under a distilled LoRA fused into the touched weights for this stage only; then the (tiled) decode.
Two differences from the reference, both on purpose:
  1. the audio is really encoded (AudioProcessor + AudioEncoder; the reference's _encode_audio_to_latent returns None and its fallback, audio
     noised once and never stepped, is not ported);
  2. stage 2 keeps the SAME encoded latent frozen (the reference builds an all-zero one there, a consequence of its missing encoder): the audio
     latent's shape depends on num_frames / fps alone, not on the resolution.
The waveform returned is the original one, never a VAE decode.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch

from ..components import STAGE_2_DISTILLED_SIGMA_VALUES, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier
from ..components.patchifiers import AudioPatchifier
from ..conditioning.tools import AudioLatentTools
from ..loader.lora_loader import LoRAConfig
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from ..types import AudioLatentShape, LatentState, VideoPixelShape
from .common import (ImageCondition, as_x0model, auto_tiling_config, conditioned_initial_state, create_image_conditionings, decode_video,
                     final_latent, frozen_audio_guided_loop, seeded_noiser, stage_callback, upscale_latent_x2, video_tools_for)
from .ti2vid_hq import fused_lora


@dataclass
class A2VidConfig:
    """Configuration of the audio-to-video pipeline (reference pipelines/a2vid_two_stage.py:49-93)."""
    height: int = 512
    width: int = 768
    num_frames: int = 97

    num_inference_steps: int = 30
    cfg_scale: float = 3.0
    seed: int = 42
    fps: float = 25.0

    distilled_lora_config: Optional[LoRAConfig] = None      # fused into the transformer for stage 2 only

    tiling_config: Optional[TilingConfig] = None
    dtype: torch.dtype = torch.float32      # (the reference's mx.float16: this engine steps fp32 latents)

    audio_vae_channels: int = 8
    audio_mel_bins: int = 16
    audio_sample_rate: int = 16000
    audio_hop_length: int = 160
    audio_downsample_factor: int = 4
    audio_output_sample_rate: int = 24000

    audio_start_time: float = 0.0
    audio_max_duration: Optional[float] = None
    use_hip_graph: bool = True      # MI355X addition: replay each stage's loop from one captured graph (no callback, < 64 steps)

    def _get_tiling_config(self) -> Optional[TilingConfig]:
        return auto_tiling_config(self.tiling_config, self.num_frames, self.height, self.width)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}")
        if self.height % 64 != 0 or self.width % 64 != 0:
            raise ValueError(f"Resolution ({self.height}x{self.width}) must be divisible by 64.")


def fit_audio_latent(latent: torch.Tensor, frames: int) -> torch.Tensor:
    """Encoded latent (1, C, T, F) -> exactly `frames` latent frames: a surplus trailing frame (the waveform's last, partly padded one) is
    cropped; a latent that comes out short is an error, it is not padded."""
    if latent.shape[2] < frames:
        raise ValueError(f"the encoded audio has {latent.shape[2]} latent frames, the video needs {frames}")
    return latent[:, :, :frames].contiguous()


def encode_audio_file(audio_path: str, num_frames: int, fps: float, audio_encoder, audio_processor=None, start_time: float = 0.0,
                      max_duration: Optional[float] = None, sample_rate: int = 16000) -> Tuple[torch.Tensor, np.ndarray, int]:
    """Audio file -> (audio latent (1, 8, T_a, 16) for a num_frames / fps video, the fitted waveform [C, samples], its rate): load_audio_file
    (start / duration trim, resample), cut or right-padded with silence to the video's length, AudioProcessor.waveform_to_mel, AudioEncoder."""
    from ..model.audio_vae import AudioProcessor, encode_audio, load_audio_file
    waveform, sr = load_audio_file(audio_path, sample_rate, start_time, max_duration)
    print(f"  Audio: {waveform.shape[1] / sr:.1f}s, {sr}Hz, {waveform.shape[0]}ch")
    proc = audio_processor or AudioProcessor(sample_rate=sr, device=audio_encoder.device)
    waveform = proc.fit_waveform(waveform[:2], proc.samples_for_video(num_frames, fps))
    latent = encode_audio(proc.waveform_to_mel(waveform, sr), audio_encoder)
    target = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=num_frames, height=32, width=32, fps=fps))
    return fit_audio_latent(latent, target.frames), waveform, sr


class A2VidPipelineTwoStage:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder, video_decoder: Optional[SimpleVideoDecoder],
                 spatial_upscaler: Optional[Callable], audio_decoder=None, vocoder=None, audio_encoder=None, audio_processor=None):
        self.transformer, self.is_av_model = as_x0model(transformer)
        self._velocity_model = self.transformer.velocity_model
        if not self.is_av_model:
            raise ValueError("A2Vid pipeline requires an audio-video (AV) model")
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.spatial_upscaler = spatial_upscaler
        self.audio_decoder = audio_decoder          # accepted for the reference's signature; the original waveform is returned, nothing is decoded
        self.vocoder = vocoder
        self.audio_encoder = audio_encoder          # MI355X addition: AudioEncoder (+ an AudioProcessor; built on demand) for audio_path
        self.audio_processor = audio_processor
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.stepper = EulerDiffusionStep()
        self.token_counts: List[int] = []
        self.audio_latent: Optional[torch.Tensor] = None        # the frozen latent (1, 8, T_a, 16) of the last call

    def _frozen_audio_state(self, latent: torch.Tensor, config: A2VidConfig, dev) -> Tuple[AudioLatentTools, LatentState]:
        pix = VideoPixelShape(batch=1, frames=config.num_frames, height=config.height // 2, width=config.width // 2, fps=config.fps)
        shape = AudioLatentShape.from_video_pixel_shape(pix, channels=config.audio_vae_channels, mel_bins=config.audio_mel_bins,
                                                        sample_rate=config.audio_sample_rate, hop_length=config.audio_hop_length,
                                                        audio_latent_downsample_factor=config.audio_downsample_factor)
        if tuple(latent.shape) != (1, shape.channels, shape.frames, shape.mel_bins):
            raise ValueError(f"audio_latent is {tuple(latent.shape)}, the video needs (1, {shape.channels}, {shape.frames}, {shape.mel_bins})")
        tools = AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=shape)
        state = tools.create_initial_state(dtype=config.dtype, initial_latent=latent.to(dev, config.dtype))
        return tools, state.replace(denoise_mask=torch.zeros_like(state.denoise_mask))       # frozen: never noised, never stepped

    def stage1_latent(self, audio_state: LatentState, positive_encoding, negative_encoding, config: A2VidConfig, images=None, callback=None,
                      positive_audio_encoding=None, negative_audio_encoding=None, *, initial_noise=None, noiser=None) -> torch.Tensor:
        """Stage 1 alone: the half-resolution latent (1, 128, F, H/64, W/64) after the guided loop over the frozen audio state."""
        dev = self._velocity_model.device
        noiser = noiser or seeded_noiser(dev, config.seed)
        h1, w1 = config.height // 2, config.width // 2
        tools = video_tools_for(self.patchifier, config.num_frames, h1, w1, config.fps)
        conds = create_image_conditionings(images or [], self.video_encoder, h1, w1, config.dtype)
        state = noiser(conditioned_initial_state(tools, conds, config.dtype, dev), noise_scale=1.0, noise=initial_noise)
        self.token_counts = [state.latent.shape[1]]
        sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
        to = lambda t: None if t is None else t.to(dev)          # noqa: E731
        state, _ = frozen_audio_guided_loop(self.transformer, state, audio_state, sigmas, to(positive_encoding), to(positive_audio_encoding),
                                            to(negative_encoding), to(negative_audio_encoding), config.cfg_scale, self.stepper,
                                            stage_callback(callback, "stage1_a2v"), config.use_hip_graph)
        return final_latent(tools, state)

    def denoise_latent(self, audio_latent: torch.Tensor, positive_encoding, negative_encoding, config: A2VidConfig, images=None, callback=None,
                       positive_audio_encoding=None, negative_audio_encoding=None, *, initial_noise=None, stage_2_noise=None) -> torch.Tensor:
        """Both stages up to the final latent (1, 128, F, H/32, W/32), over the audio latent (1, 8, T_a, 16) kept frozen in both."""
        if self.spatial_upscaler is None:
            raise ValueError("A2VidPipelineTwoStage requires spatial_upscaler to be provided")
        if positive_audio_encoding is None:
            raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
        images = images or []
        dev = self._velocity_model.device
        noiser = seeded_noiser(dev, config.seed)
        _, audio_state = self._frozen_audio_state(audio_latent, config, dev)
        latent = self.stage1_latent(audio_state, positive_encoding, negative_encoding, config, images, callback, positive_audio_encoding,
                                    negative_audio_encoding, initial_noise=initial_noise, noiser=noiser)

        upscaled = upscale_latent_x2(latent, self.spatial_upscaler, self.video_encoder, self.video_decoder)
        with fused_lora(self._velocity_model, config.distilled_lora_config):
            tools2 = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
            conds2 = create_image_conditionings(images, self.video_encoder, config.height, config.width, config.dtype)
            state2 = conditioned_initial_state(tools2, conds2, config.dtype, dev, initial_latent=upscaled)
            sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES]
            state2 = noiser(state2, noise_scale=sig2[0], noise=stage_2_noise)
            self.token_counts.append(state2.latent.shape[1])
            # refinement without guidance (reference :440-444) over the same frozen audio latent: the captured frozen-audio loop
            state2, _ = frozen_audio_guided_loop(self.transformer, state2, audio_state, sig2, positive_encoding.to(dev), positive_audio_encoding.to(dev),
                                                 None, None, 1.0, self.stepper, stage_callback(callback, "stage2_a2v"), config.use_hip_graph)
        return final_latent(tools2, state2)

    def __call__(self, audio_path: Optional[str], positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: A2VidConfig,
                 images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                 positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None, *,
                 initial_noise: Optional[torch.Tensor] = None, stage_2_noise: Optional[torch.Tensor] = None,
                 audio_latent: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[np.ndarray], Optional[int]]:
        """-> (uint8 frames (F, H, W, 3), or the final latent when no decoder is set; the original waveform [C, samples]; its sample rate).
        audio_latent (keyword-only, MI355X addition): a pre-encoded (1, 8, T_a, 16) latent that bypasses the file; waveform and rate are then
        None unless audio_path is given as well.  initial_noise / stage_2_noise: supplied N(0,1) tensors of the patchified shapes."""
        waveform = rate = None
        if audio_latent is None:
            if audio_path is None:
                raise ValueError("A2Vid pipeline needs audio_path or audio_latent")
            if self.audio_encoder is None:
                raise ValueError("A2Vid pipeline needs an audio_encoder to encode audio_path (or pass audio_latent)")
            print(f"  Loading audio: {audio_path}")
            audio_latent, waveform, rate = encode_audio_file(audio_path, config.num_frames, config.fps, self.audio_encoder, self.audio_processor,
                                                             config.audio_start_time, config.audio_max_duration, config.audio_sample_rate)
        elif audio_path is not None:
            from ..model.audio_vae import load_audio_file
            waveform, rate = load_audio_file(audio_path, config.audio_sample_rate, config.audio_start_time, config.audio_max_duration)
        self.audio_latent = audio_latent
        latent = self.denoise_latent(audio_latent, positive_encoding, negative_encoding, config, images, callback, positive_audio_encoding,
                                     negative_audio_encoding, initial_noise=initial_noise, stage_2_noise=stage_2_noise)
        return decode_video(latent, self.video_decoder, config._get_tiling_config()), waveform, rate


def create_a2vid_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder=None, vocoder=None, audio_encoder=None,
                          audio_processor=None) -> A2VidPipelineTwoStage:
    return A2VidPipelineTwoStage(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder, vocoder, audio_encoder, audio_processor)
