"""Single-stage generation pipeline on MI355X: the Euler branches of the reference's OneStagePipeline, with or without classifier-free guidance.

Mirrors reference LTX_2_MLX/pipelines/one_stage.py:52-110 (OneStageCFGConfig, field names and defaults verbatim),
:113-160 (constructor), :224-330 / :466-568 (`_denoise_loop_cfg`, `_denoise_loop_cfg_av` with `need_cfg == False`) and
:731-1011 (`__call__`): LTX2Scheduler sigma schedule over `num_inference_steps`, optional image conditioning by latent
replacement, video-only or joint audio+video denoising on an AudioVideo transformer (LTX-2.3 always takes the joint
branch: `use_internal_audio_branch`), VAE decode (tiled above 4000 latent voxels).  This is the path the reference's CLI
takes for LTX-2.3 checkpoints and for `--generate-audio` (scripts/generate.py:1638-1735; distilled models run it with
cfg_scale = audio_cfg_scale = 1, i.e. one transformer evaluation per step).

Classifier-free guidance (round 3): `cfg_scale` / `audio_cfg_scale` != 1 evaluate the negative prompt too (a second engine context over the same
weights) and combine the two predictions with CFGGuider or, for `rescale_scale > 0`, CFGStarRescalingGuider -- per modality, as :793-807.
`guider_override` (one of CFGGuider, CFGStarRescalingGuider, LtxAPGGuider, LegacyStatefulAPGGuider) becomes the video guider; audio keeps its
standard one (:795-805).  Without an audio state an enabled projected guider runs through pipelines.common.projected_denoise_loop.
The joint audio+video branch -- the route of an LTX-2.3 dev checkpoint and of `--generate-audio --model-variant dev`, by default a
CFGStarRescalingGuider per modality -- stays on the eager loop (two X0Model calls, the guiders in torch).  Its device form exists,
pipelines.common.joint_projected_denoise_loop (one C call per step: both evaluations, one sums kernel, one step kernel over both latents; one
captured graph per loop), but measured at the bench geometry it is not faster (profiles/joint_projected_step.md: 204.1 ms per step as C calls
and 219.6 with the capture against 202.4 eager), so this pipeline does not take it.

Spatio-temporal guidance: `stg_scale` > 0 adds, while (step + 1) / steps <= `stg_cutoff`, a third evaluation of the positive prompt with the video
self-attention of `stg_blocks` (None: every block) skipped, and STGGuider pushes the guided video prediction away from it (:284-297, :516-526).
Without an audio state and with a plain CFGGuider (or none enabled) the loop is pipelines.common.stg_denoise_loop: one C call per step, one
captured graph per loop.  With CFG* (the config default) or a projected override, with or without an audio state, it is the eager loop: three
evaluations, the guiders in torch; there only the video is STG-guided.
With an audio state and a plain CFGGuider per modality (or none enabled) the loop is pipelines.common.joint_stg_denoise_loop: one C call per step
(LTXModel.stg_step_joint_av_: the evaluations, then one kernel over both latents), no captured form.  `stg_audio_scale` > 0 (this loop alone)
STG-guides the audio latent too: the perturbed evaluation also skips the audio self-attention of `stg_blocks`, and an STGGuider of that scale acts
on the CFG-guided audio prediction.  With `stg_audio_scale` 0 the audio gets plain CFG, as on the eager loop.

`sampler="heun"` runs the reference's predictor-corrector loops (:334-464, :570-729) and `ge_gamma` > 0 its GE velocity correction on the video's
guided prediction (:300-307), in either sampler.  Under a plain CFGGuider per modality (or none enabled) the loop is
pipelines.common.heun_denoise_loop / ge_denoise_loop's device form: one C call per step (the two pairs of evaluations, a predictor and a corrector
kernel), the video-only Heun loop one captured graph; the joint audio+video Heun loop has no captured form, and Euler + GE on the joint branch has no
device form.  With CFG* (the config default) or a projected override it is the eager form: the reference's statements through X0Model, the torch
guiders and HeunDiffusionStep.  An unknown `sampler` is a ValueError.

Outside the MI355X hot path, rejected with NotImplementedError: any other `guider_override`, the Heun sampler or GE velocity correction beside STG
(`stg_scale` > 0), cross-attention scaling, the temporal upscaler.
With `audio_enabled`, the audio waveform is returned when an audio_decoder and a vocoder are given (model/audio_vae/), the audio
LATENT otherwise.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple, Union

import torch

from ..components import (AudioPatchifier, CFGGuider, CFGStarRescalingGuider, EulerDiffusionStep, LegacyStatefulAPGGuider, LtxAPGGuider, LTX2Scheduler,
                          STGGuider, VideoLatentPatchifier, create_batched_stg_config)
from ..conditioning.tools import AudioLatentTools
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from ..types import AudioLatentShape, VideoPixelShape
from .common import (ImageCondition, ancestral_denoise_loop, as_x0model, auto_tiling_config, conditioned_initial_state, create_image_conditionings, decode_video,
                     final_latent, ge_denoise_loop, heun_denoise_loop, heun_device_form, joint_denoise_loop, joint_stg_denoise_loop, projected_denoise_loop, projected_guider_args, reset_guider, seeded_noiser, stg_denoise_loop, video_tools_for)


@dataclass
class OneStageCFGConfig:
    """Configuration of the single-stage pipeline (reference pipelines/one_stage.py:52-110)."""
    height: int = 480
    width: int = 704
    num_frames: int = 97            # must be 8k + 1
    seed: int = 42
    fps: float = 24.0
    num_inference_steps: int = 30
    cfg_scale: float = 3.0          # video text guidance (1.0: none, one transformer evaluation per step)
    audio_cfg_scale: float = 7.0    # audio text guidance
    rescale_scale: float = 0.7      # > 0: CFGStarRescalingGuider, else CFGGuider (one_stage.py:796-805)
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
    use_hip_graph: bool = False     # MI355X addition: replay the captured step loop (uniform sigma, no callback)

    def _get_tiling_config(self) -> Optional[TilingConfig]:
        return auto_tiling_config(self.tiling_config, self.num_frames, self.height, self.width)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}. Valid values: 1, 9, 17, 25, 33, ..., 121")
        if self.height % 32 != 0 or self.width % 32 != 0:
            raise ValueError(f"Resolution ({self.height}x{self.width}) must be divisible by 32 for single-stage pipeline.")


class OneStagePipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder=None, video_decoder: Optional[SimpleVideoDecoder] = None,
                 audio_decoder=None, vocoder=None):
        self.transformer, self.is_av_model = as_x0model(transformer)
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.audio_decoder = audio_decoder
        self.vocoder = vocoder
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.audio_patchifier = AudioPatchifier(patch_size=1)
        self.diffusion_step = EulerDiffusionStep()
        self.scheduler = LTX2Scheduler()

    def _create_audio_tools(self, target_shape: AudioLatentShape) -> AudioLatentTools:
        return AudioLatentTools(patchifier=self.audio_patchifier, target_shape=target_shape)

    @staticmethod
    def _require_no_guidance(stg_scale, guider_override, ge_gamma, sampler, temporal_upscaler, cross_attn_scale):
        """Everything beyond classifier-free guidance and the Euler step is not built here.  The reference enables STG / GE only for
        values > 0 (pipelines/one_stage.py:867, :301): a zero or negative value is a no-op there and passes here."""
        if guider_override is not None and type(guider_override) not in (CFGGuider, CFGStarRescalingGuider, LtxAPGGuider, LegacyStatefulAPGGuider):
            raise NotImplementedError("guider_override (APG / custom guiders) is outside the MI355X hot path")
        if stg_scale > 0:
            raise NotImplementedError("STG guidance is outside the MI355X hot path")
        if ge_gamma > 0:
            raise NotImplementedError("GE velocity correction is outside the MI355X hot path")
        if sampler != "euler":
            raise NotImplementedError(f"sampler={sampler!r}: only the Euler step is built")
        if temporal_upscaler is not None:
            raise NotImplementedError("the temporal upscaler is outside the MI355X hot path")
        if cross_attn_scale != 1.0:
            raise NotImplementedError("cross_attn_scale != 1.0 is outside the MI355X hot path")

    def __call__(self, positive_encoding: torch.Tensor, negative_encoding: Optional[torch.Tensor], config: OneStageCFGConfig,
                 images: Optional[List[ImageCondition]] = None, callback: Optional[Callable[[int, int], None]] = None,
                 positive_audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None,
                 stg_scale: float = 0.0, stg_blocks: Optional[List[int]] = None, stg_cutoff: float = 1.0, guider_override=None,
                 ge_gamma: float = 0.0, sampler: str = "euler", temporal_upscaler=None, cross_attn_scale: float = 1.0,
                 cross_attn_start_block: int = 40, *, stg_audio_scale: float = 0.0, initial_noise: Optional[torch.Tensor] = None,
                 initial_audio_noise: Optional[torch.Tensor] = None,
                 initial_audio_latent: Optional[torch.Tensor] = None,
                 ancestral_eta: float = 1.0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """-> (video, audio): video uint8 frames (F, H, W, 3) (or the final latent when no decoder is set); audio = the
        waveform (B, 2, samples) when config.audio_enabled and both audio_decoder and vocoder were given (the reference's
        _decode_audio), the audio LATENT (B, 8, T_a, 16) when config.audio_enabled without them, else None.
        The negative encodings are evaluated when a guider is enabled (cfg_scale / audio_cfg_scale != 1); unlike the reference
        (one_stage.py:776-780, which demands negative_audio_encoding whenever the audio branch runs) they may be None when no guider is.  initial_noise /
        initial_audio_noise (keyword-only, MI355X addition): supplied N(0,1) tensors of the patchified latent shapes, so
        results can be compared with the oracle loop (MLX's RNG stream is not reproducible here).
        initial_audio_latent (keyword-only): an encoded audio latent (1, 8, T_a, 16) (model/audio_vae AudioEncoder) the video is generated
        TO: the audio state starts from it with denoise_mask = 0 and is not noised, so every step leaves it as it is and only the video is
        denoised (reference pipelines/a2vid_two_stage.py:338-357).  Needs an AudioVideo transformer.  The returned audio is then this
        latent, never VAE-decoded (the reference returns the original waveform).
        stg_audio_scale (keyword-only, MI355X addition): > 0 adds an STG term of that scale to the AUDIO prediction, from the same perturbed
        evaluation, which then skips the audio self-attention of `stg_blocks` as well; stg_blocks / stg_cutoff hold for both modalities.  Needs
        an audio state (ValueError without one) and a plain CFGGuider per modality or none enabled (NotImplementedError under CFG* / APG).
        sampler="euler_ancestral" with ancestral_eta (keyword-only, MI355X addition): the reference's EulerAncestralDiffusionStep
        (components/diffusion_steps.py:70-129) through pipelines.common.ancestral_denoise_loop, the noise made in the step kernel under
        config.seed.  Runs under a plain CFGGuider per modality (rescale_scale = 0) or with no guidance; NotImplementedError beside CFG* / APG,
        STG, GE, cross_attn_scale and a temporal upscaler."""
        images = images or []
        internal_audio_active = self.is_av_model and (config.use_internal_audio_branch or config.audio_enabled)
        if config.audio_enabled or internal_audio_active:
            if positive_audio_encoding is None:
                raise ValueError("Audio encoding required for AudioVideo generation. Provide positive_audio_encoding and negative_audio_encoding.")
        if config.audio_enabled and not self.is_av_model:
            raise ValueError("audio_enabled needs an AudioVideo transformer")
        if initial_audio_latent is not None and not internal_audio_active:
            raise ValueError("initial_audio_latent needs an AudioVideo transformer (the audio branch carries the frozen latent)")
        # STG is validated here; the gate below then sees the remaining options (it refuses every stg_scale > 0 on its own)
        stg_guider = audio_stg_guider = None
        if stg_audio_scale > 0 and not internal_audio_active:
            raise ValueError("stg_audio_scale > 0 needs an audio state (an AudioVideo transformer with its audio branch active)")
        if stg_scale > 0 or stg_audio_scale > 0:
            layers = self.transformer.velocity_model.num_layers
            bad = [b for b in (stg_blocks or []) if not 0 <= int(b) < layers]
            if bad:
                raise ValueError(f"stg_blocks {bad} out of range: the model has {layers} layers")
            if not 0.0 <= stg_cutoff <= 1.0:
                raise ValueError(f"stg_cutoff={stg_cutoff} must lie in [0, 1]")
            stg_guider = STGGuider(scale=stg_scale) if stg_scale > 0 else None
            audio_stg_guider = STGGuider(scale=stg_audio_scale) if stg_audio_scale > 0 else None
        if sampler not in ("euler", "heun", "euler_ancestral"):
            raise ValueError(f"sampler={sampler!r}: 'euler', 'heun' or 'euler_ancestral'")
        # Heun and GE are built without STG; beside it they stay refused, so the gate sees them only then
        heun, ge, ancestral = sampler == "heun", ge_gamma > 0, sampler == "euler_ancestral"
        if ancestral:
            # the ancestral step is built for the Euler step under plain CFG alone: the gate sees every other option, then GE and the guider classes
            self._require_no_guidance(max(stg_scale, stg_audio_scale), guider_override, ge_gamma, "euler", temporal_upscaler, cross_attn_scale)
            if guider_override is not None and type(guider_override) is not CFGGuider:
                raise NotImplementedError("sampler='euler_ancestral' beside CFG* / APG (a projected guider_override) is outside the MI355X hot path")
            if config.rescale_scale > 0 and guider_override is None and (config.cfg_scale != 1.0 or (internal_audio_active and config.audio_cfg_scale != 1.0)):
                raise NotImplementedError("sampler='euler_ancestral' beside CFG* (rescale_scale > 0) is outside the MI355X hot path: it runs under a plain "
                                          "CFGGuider per modality (rescale_scale = 0) or with no guidance")
            if ancestral_eta < 0:
                raise ValueError(f"ancestral_eta={ancestral_eta} must be >= 0")
        elif stg_guider is None and audio_stg_guider is None:
            self._require_no_guidance(0.0, guider_override, 0.0, "euler", temporal_upscaler, cross_attn_scale)
        else:
            self._require_no_guidance(0.0, guider_override, ge_gamma, sampler, temporal_upscaler, cross_attn_scale)

        dev = self.transformer.velocity_model.device
        noiser = seeded_noiser(dev, config.seed)
        video_tools = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
        conditionings = create_image_conditionings(images, self.video_encoder, config.height, config.width, config.dtype)
        video_state = conditioned_initial_state(video_tools, conditionings, config.dtype, dev)
        sigmas = self.scheduler.execute(steps=config.num_inference_steps)        # no latent: the MAX_SHIFT_ANCHOR schedule (one_stage.py:837)
        video_state = noiser(video_state, noise_scale=1.0, noise=initial_noise)

        audio_state, audio_tools = None, None
        if internal_audio_active:
            pixel_shape = VideoPixelShape(batch=1, frames=config.num_frames, height=config.height, width=config.width, fps=config.fps)
            audio_shape = AudioLatentShape.from_video_pixel_shape(
                pixel_shape, channels=config.audio_vae_channels, mel_bins=config.audio_mel_bins, sample_rate=config.audio_sample_rate,
                hop_length=config.audio_hop_length, audio_latent_downsample_factor=config.audio_downsample_factor)
            audio_tools = self._create_audio_tools(audio_shape)
            if initial_audio_latent is not None:
                # frozen: denoise_mask = 0, no noise (a2vid_two_stage.py:347-357); the loops' non-uniform path carries it
                audio_state = audio_tools.create_initial_state(dtype=config.dtype, initial_latent=initial_audio_latent.to(dev, config.dtype))
                audio_state = audio_state.replace(denoise_mask=torch.zeros_like(audio_state.denoise_mask))
            else:
                audio_state = noiser(audio_tools.create_initial_state(dtype=config.dtype, device=dev), noise_scale=1.0, noise=initial_audio_noise)

        actx = positive_audio_encoding.to(dev) if (internal_audio_active and positive_audio_encoding is not None) else None
        # one guider per modality (one_stage.py:793-807)
        mk = CFGStarRescalingGuider if config.rescale_scale > 0 else CFGGuider
        video_guider, audio_guider = mk(scale=config.cfg_scale), mk(scale=config.audio_cfg_scale)
        if guider_override is not None:
            video_guider = guider_override      # audio keeps its standard guider (one_stage.py:795-805)
            reset_guider(video_guider)
        need_cfg = video_guider.enabled() or (internal_audio_active and audio_guider.enabled())
        if need_cfg and (negative_encoding is None or (internal_audio_active and negative_audio_encoding is None)):
            raise ValueError("cfg_scale / audio_cfg_scale != 1 need the negative prompt's encoding(s)")
        nactx = negative_audio_encoding.to(dev) if (need_cfg and internal_audio_active) else None
        if ancestral:
            # one kernel per step steps to sigma_down and adds the Philox noise; both latents when there is an audio state
            video_state, audio_state = ancestral_denoise_loop(
                self.transformer, video_state, audio_state, sigmas, positive_encoding.to(dev), actx, negative_encoding.to(dev) if need_cfg else None,
                nactx, video_guider.scale if video_guider.enabled() else 1.0,
                audio_guider.scale if (audio_state is not None and audio_guider.enabled()) else 1.0, ancestral_eta, config.seed, callback,
                config.use_hip_graph)
        elif heun or ge:
            # on the device under plain CFG (or none); CFG* and the projected overrides through the eager statements.  Euler + GE has no device form
            # of the joint loop
            loop = heun_denoise_loop if heun else ge_denoise_loop
            fused = heun_device_form(video_guider, audio_guider if audio_state is not None else None) and (heun or audio_state is None)
            video_state, audio_state = loop(self.transformer, video_state, audio_state, sigmas, positive_encoding.to(dev), actx,
                                            negative_encoding.to(dev) if need_cfg else None, nactx, video_guider,
                                            audio_guider if audio_state is not None else None, max(float(ge_gamma), 0.0), callback, config.use_hip_graph, fused)
        elif (stg_guider is not None or audio_stg_guider is not None) and audio_state is not None and heun_device_form(video_guider, audio_guider):
            # both latents: forward_av x 2 or 3 (one of them perturbed) and one kernel over both per step, on the device
            video_state, audio_state = joint_stg_denoise_loop(self.transformer, video_state, audio_state, sigmas, positive_encoding.to(dev), actx,
                                                              negative_encoding.to(dev) if need_cfg else None, nactx, video_guider, audio_guider,
                                                              stg_guider, audio_stg_guider, stg_blocks, stg_cutoff, callback, config.use_hip_graph)
        elif audio_stg_guider is not None:
            raise NotImplementedError("stg_audio_scale > 0 runs under a plain CFGGuider per modality (rescale_scale = 0, no projected guider_override) or "
                                      "none enabled: beside CFG* / APG the eager loop STG-guides the video alone")
        elif stg_guider is not None and audio_state is None and (type(video_guider) is CFGGuider or not video_guider.enabled()):
            # forward x 2 or 3 and one kernel per step, on the device
            video_state = stg_denoise_loop(self.transformer, video_state, sigmas, positive_encoding.to(dev),
                                           negative_encoding.to(dev) if video_guider.enabled() else None, video_guider, stg_guider, stg_blocks, stg_cutoff,
                                           self.diffusion_step, callback, config.use_hip_graph)
        elif stg_guider is None and guider_override is not None and audio_state is None and video_guider.enabled() and projected_guider_args(video_guider) is not None:
            # the override's sums and step on the device; the default guiders stay on the eager loop below
            video_state = projected_denoise_loop(self.transformer, video_state, sigmas, positive_encoding.to(dev), negative_encoding.to(dev),
                                                 video_guider, self.diffusion_step, callback, config.use_hip_graph)
        else:
            video_state, audio_state = joint_denoise_loop(self.transformer, self.is_av_model, video_state, audio_state, sigmas,
                                                          positive_encoding.to(dev), actx, self.diffusion_step, callback, config.use_hip_graph,
                                                          negative_video_context=negative_encoding.to(dev) if need_cfg else None,
                                                          negative_audio_context=nactx, video_guider=video_guider, audio_guider=audio_guider,
                                                          **(dict(stg_guider=stg_guider, stg_perturbations=create_batched_stg_config(1, blocks=stg_blocks),
                                                                  stg_cutoff=stg_cutoff) if stg_guider is not None else {}))

        video = decode_video(final_latent(video_tools, video_state), self.video_decoder, config._get_tiling_config())
        audio = None
        if initial_audio_latent is not None:
            audio = final_latent(audio_tools, audio_state)          # the latent given, kept by every step
        elif config.audio_enabled and audio_state is not None:
            audio = final_latent(audio_tools, audio_state)
            if self.audio_decoder is not None and self.vocoder is not None:
                audio = self._decode_audio(audio)
        return video, audio

    def _decode_audio(self, audio_latent: torch.Tensor) -> torch.Tensor:
        """Audio latent (B, 8, T, 16) -> waveform (B, 2, samples) through the audio VAE decoder and the vocoder (reference
        one_stage.py:184-205)."""
        if self.audio_decoder is None or self.vocoder is None:
            raise ValueError("Audio decoder and vocoder required for audio decoding")
        return self.vocoder(self.audio_decoder(audio_latent))


def create_one_stage_pipeline(transformer, video_encoder, video_decoder, audio_decoder=None, vocoder=None) -> OneStagePipeline:
    return OneStagePipeline(transformer, video_encoder, video_decoder, audio_decoder, vocoder)
