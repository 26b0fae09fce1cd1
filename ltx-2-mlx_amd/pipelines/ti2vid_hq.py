"""High-quality two-stage text/image-to-video on MI355X: the res_2s second-order sampler.

Mirrors reference LTX_2_MLX/pipelines/ti2vid_hq.py:52-97 (TI2VidHQConfig), :100-136 (constructor), :153-273 (the res_2s loop) and
:360-531 (__call__).  15 second-order steps do what the Euler pipelines need 30 for.
  stage 1: half resolution, LTX2Scheduler over num_inference_steps, classifier-free guidance in the HQ pipeline's own form
           (uncond + scale * (cond - uncond)) inside the res_2s step -- pipelines.common.res2s_denoise_loop: one C call per step or one
           captured graph; with audio_enabled on an AudioVideo model, pipelines.common.res2s_av_denoise_loop steps the audio latent
           jointly, guided by audio_cfg_scale, one C call per step (that loop has no captured form);
  stage 2: un-normalise -> spatial upscaler -> normalise, image conditionings re-encoded at full size, noise at
           STAGE_2_DISTILLED_SIGMA_VALUES[0], the distilled refinement steps without guidance (the captured conditioned loop),
           optionally under a distilled LoRA fused into the touched weights for this stage only; then the (tiled) decode.
With sound (audio_enabled=True, an AudioVideo model): stage 2 re-noises stage 1's audio latent and refines both modalities jointly, one C
call per step as well: with sound neither stage replays a captured graph, whatever use_hip_graph says.  The audio latent is decoded by the audio VAE decoder and the vocoder, and __call__ returns (frames, waveform or None).  audio_enabled=True on a
VideoOnly model raises NotImplementedError.  With audio_enabled=False an AudioVideo checkpoint runs through its video twin, whatever
use_internal_audio_branch says (accepted and unused, a deviation: the reference then samples an audio latent it never returns).  The
reference constructs a Res2sDiffusionStep (SDE noise) and never calls it: not built.
"""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch

from ..components import STAGE_2_DISTILLED_SIGMA_VALUES, AudioPatchifier, EulerDiffusionStep, GaussianNoiser, LTX2Scheduler, VideoLatentPatchifier
from ..conditioning.tools import AudioLatentTools
from ..loader.lora_loader import LoRAConfig, find_lora_keys_for_weight, fuse_lora_into_weights
from ..model.transformer import LTXModel, LTXModelType, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from ..types import AudioLatentShape, VideoPixelShape
from .common import (ImageCondition, as_x0model, auto_tiling_config, conditioned_initial_state, create_image_conditionings, decode_video,
                     final_latent, joint_denoise_loop, res2s_av_denoise_loop, res2s_denoise_loop, seeded_noiser, stage_callback, upscale_latent_x2,
                     video_tools_for)


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
    use_hip_graph: bool = True      # MI355X addition: replay each stage's loop from one captured graph (no callback, < 64 steps; not with audio_enabled)

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
        self.audio_decoder = audio_decoder          # with a vocoder: the joint path's audio latent becomes a waveform
        self.vocoder = vocoder
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.euler_step = EulerDiffusionStep()
        self.audio_latent = None

    def _joint(self, config: TI2VidHQConfig) -> bool:
        """Whether this call samples sound: audio_enabled on an AudioVideo model.  On any other model audio_enabled is refused."""
        if not config.audio_enabled:
            return False
        if getattr(self._velocity_model, "model_type", None) != LTXModelType.AudioVideo:
            raise NotImplementedError("TI2VidHQPipeline: audio_enabled=True needs an AudioVideo model; this one is video-only")
        return True

    @staticmethod
    def _audio_tools(config: TI2VidHQConfig, height: int, width: int) -> AudioLatentTools:
        pix = VideoPixelShape(batch=1, frames=config.num_frames, height=height, width=width, fps=config.fps)
        shape = AudioLatentShape.from_video_pixel_shape(pix, channels=config.audio_vae_channels, mel_bins=config.audio_mel_bins,
                                                        sample_rate=config.audio_sample_rate, hop_length=config.audio_hop_length,
                                                        audio_latent_downsample_factor=config.audio_downsample_factor)
        return AudioLatentTools(patchifier=AudioPatchifier(patch_size=1), target_shape=shape)

    def _decode_audio(self, audio_latent: torch.Tensor) -> Optional[torch.Tensor]:
        """Audio latent -> waveform (B, 2, samples) through the audio VAE decoder and the vocoder; None when either is missing."""
        if self.audio_decoder is None or self.vocoder is None:
            return None
        return self.vocoder(self.audio_decoder(audio_latent))

    def stage1_latent(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: TI2VidHQConfig,
                      images: Optional[List[ImageCondition]] = None, callback=None, *, initial_noise: Optional[torch.Tensor] = None,
                      noiser: Optional[GaussianNoiser] = None, positive_audio_encoding: Optional[torch.Tensor] = None,
                      negative_audio_encoding: Optional[torch.Tensor] = None, initial_audio_noise: Optional[torch.Tensor] = None):
        """Stage 1 alone: the half-resolution latent (1, 128, F, H/64, W/64) after the guided res_2s loop; with sound, the pair of it and
        the audio latent (1, 8, T_a, 16) the same loop stepped beside it (the audio is noised after the video, reference :397-412)."""
        joint = self._joint(config)
        dev = self._velocity_model.device
        noiser = noiser or seeded_noiser(dev, config.seed)
        h1, w1 = config.height // 2, config.width // 2
        tools = video_tools_for(self.patchifier, config.num_frames, h1, w1, config.fps)
        conds = create_image_conditionings(images or [], self.video_encoder, h1, w1, config.dtype)
        state = conditioned_initial_state(tools, conds, config.dtype, dev)
        sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
        state = noiser(state, noise_scale=1.0, noise=initial_noise)
        nctx = None if negative_encoding is None else negative_encoding.to(dev)
        if not joint:
            state = res2s_denoise_loop(self.transformer, state, sigmas, positive_encoding.to(dev), nctx, config.cfg_scale, config.audio_cfg_scale,
                                       stage_callback(callback, "stage1_res2s"), config.use_hip_graph)
            return final_latent(tools, state)
        atools = self._audio_tools(config, h1, w1)
        astate = noiser(atools.create_initial_state(dtype=config.dtype, device=dev), noise_scale=1.0, noise=initial_audio_noise)
        actx = None if positive_audio_encoding is None else positive_audio_encoding.to(dev)
        nactx = None if negative_audio_encoding is None else negative_audio_encoding.to(dev)
        state, astate = res2s_av_denoise_loop(self.transformer, state, astate, sigmas, positive_encoding.to(dev), actx, nctx, nactx, config.cfg_scale,
                                              config.audio_cfg_scale, stage_callback(callback, "stage1_res2s"), config.use_hip_graph)
        return final_latent(tools, state), final_latent(atools, astate)

    def denoise_latent(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: TI2VidHQConfig,
                       images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                       positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None,
                       *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None,
                       initial_audio_noise: Optional[torch.Tensor] = None, stage2_audio_noise: Optional[torch.Tensor] = None):
        """Both stages up to the final latent (1, 128, F, H/32, W/32); with sound, the pair of it and the audio latent (1, 8, T_a, 16).
        initial_noise / stage2_noise and their audio counterparts (keyword-only, MI355X addition): supplied N(0,1) tensors of the patchified
        shapes, so results can be compared with a restatement."""
        if self.spatial_upscaler is None:
            raise ValueError("TI2VidHQPipeline requires spatial_upscaler to be provided")
        joint = self._joint(config)
        images = images or []
        dev = self._velocity_model.device
        ctx = positive_encoding.to(dev)
        noiser = seeded_noiser(dev, config.seed)
        audio_latent = None
        if joint:
            latent, audio_latent = self.stage1_latent(ctx, negative_encoding, config, images, callback, initial_noise=initial_noise, noiser=noiser,
                                                      positive_audio_encoding=positive_audio_encoding, negative_audio_encoding=negative_audio_encoding,
                                                      initial_audio_noise=initial_audio_noise)
        else:
            latent = self.stage1_latent(ctx, negative_encoding, config, images, callback, initial_noise=initial_noise, noiser=noiser)

        upscaled = upscale_latent_x2(latent, self.spatial_upscaler, self.video_encoder, self.video_decoder)
        with fused_lora(self._velocity_model, config.distilled_lora_config):
            tools2 = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
            conds2 = create_image_conditionings(images, self.video_encoder, config.height, config.width, config.dtype)
            state2 = conditioned_initial_state(tools2, conds2, config.dtype, dev, initial_latent=upscaled)
            sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES]
            state2 = noiser(state2, noise_scale=sig2[0], noise=stage2_noise)
            if not joint:
                # refinement without guidance (reference :321-358, :499-503): the existing conditioned loop, captured; no audio state, so an
                # AudioVideo model runs through its video twin
                state2 = joint_denoise_loop(self.transformer, self.is_av_model, state2, None, sig2, ctx, None, self.euler_step,
                                            stage_callback(callback, "stage2"), config.use_hip_graph)[0]
                return final_latent(tools2, state2)
            # no spatial upscaling for audio: stage 1's latent is re-noised (reference :478-492) and refined jointly
            atools2 = self._audio_tools(config, config.height, config.width)
            astate2 = noiser(atools2.create_initial_state(dtype=config.dtype, device=dev, initial_latent=audio_latent), noise_scale=sig2[0],
                             noise=stage2_audio_noise)
            actx = None if positive_audio_encoding is None else positive_audio_encoding.to(dev)
            # per step, whatever config.use_hip_graph says: with sound no stage of this pipeline replays a captured graph
            state2, astate2 = joint_denoise_loop(self.transformer, True, state2, astate2, sig2, ctx, actx, self.euler_step,
                                                 stage_callback(callback, "stage2"), False)
        return final_latent(tools2, state2), final_latent(atools2, astate2)

    def __call__(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: TI2VidHQConfig,
                 images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                 positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None,
                 *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None,
                 initial_audio_noise: Optional[torch.Tensor] = None, stage2_audio_noise: Optional[torch.Tensor] = None):
        """-> uint8 frames (F, H, W, 3) (the final latent when no decoder is set); with config.audio_enabled on an AudioVideo model, the
        tuple (frames, waveform (B, 2, samples)), the second None unless both audio_decoder and vocoder were given (reference :523-531)."""
        out = self.denoise_latent(positive_encoding, negative_encoding, config, images, callback, positive_audio_encoding, negative_audio_encoding,
                                  initial_noise=initial_noise, stage2_noise=stage2_noise, initial_audio_noise=initial_audio_noise,
                                  stage2_audio_noise=stage2_audio_noise)
        if not config.audio_enabled:
            return decode_video(out, self.video_decoder, config._get_tiling_config())
        latent, audio_latent = out
        self.audio_latent = audio_latent             # (1, 8, T_a, 16): kept for a caller that decodes or stores it itself
        return decode_video(latent, self.video_decoder, config._get_tiling_config()), self._decode_audio(audio_latent)


def create_ti2vid_hq_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder=None, vocoder=None) -> TI2VidHQPipeline:
    return TI2VidHQPipeline(transformer, video_encoder, video_decoder, spatial_upscaler, audio_decoder, vocoder)
