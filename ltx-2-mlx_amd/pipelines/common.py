"""Loop and conditioning helpers shared by the pipelines.  Mirrors reference LTX_2_MLX/pipelines/common.py:23-262.
Additions of this codebase, without a counterpart there: the stage helpers (as_x0model, seeded_noiser, video_tools_for, conditioned_initial_state,
stage_callback, final_latent, upscale_latent_x2, auto_tiling_config, decode_video) and the three device-resident loops with their helpers."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

from ..components import GaussianNoiser
from ..conditioning.latent import VideoConditionByLatentIndex
from ..conditioning.tools import VideoLatentTools
from ..model.transformer import LTXModelType, Modality, X0Model
from ..model.upscaler import SpatialUpscaler, upscale_latent
from ..model.video_vae import TilingConfig, decode_latent, decode_tiled
from ..types import LatentState, VideoLatentShape, VideoPixelShape


@dataclass
class ImageCondition:
    """An image that replaces the latent at one latent frame (reference pipelines/common.py:23-29).  `image` may
    carry an already loaded tensor (1, 3, 1, H, W) in [-1, 1] instead of a path."""
    image_path: Optional[str]
    frame_index: int
    strength: float = 0.95
    image: Optional[torch.Tensor] = None


def load_image_tensor(image_path: str, height: int, width: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """File -> (1, 3, 1, H, W) in [-1, 1]: RGB, aspect-preserving LANCZOS resize + centre crop
    (reference pipelines/common.py:32-102)."""
    import numpy as np
    from PIL import Image
    if not os.path.exists(image_path):
        raise FileNotFoundError(f"Image not found: {image_path}")
    try:
        img = Image.open(image_path)
    except Exception as e:  # noqa: BLE001
        raise ValueError(f"Failed to open image {image_path}: {e}")
    if img.mode not in ("RGB", "RGBA", "L"):
        raise ValueError(f"Unsupported image format: {img.mode}. Supported formats: RGB, RGBA, L")
    img = img.convert("RGB")
    sw, sh = img.size
    if abs(sw / sh - width / height) < 0.01:
        img = img.resize((width, height), Image.Resampling.LANCZOS)
    else:
        if sw / sh > width / height:
            nh, nw = height, int(sw * (height / sh))
        else:
            nw, nh = width, int(sh * (width / sw))
        img = img.resize((nw, nh), Image.Resampling.LANCZOS)
        left, top = (nw - width) // 2, (nh - height) // 2
        img = img.crop((left, top, left + width, top + height))
    arr = torch.from_numpy(np.array(img).astype(np.float32) / 127.5 - 1.0)
    return arr.permute(2, 0, 1)[None, :, None].to(dtype)


def create_image_conditionings(images: List[ImageCondition], video_encoder, height: int, width: int,
                               dtype: torch.dtype = torch.float32) -> List[VideoConditionByLatentIndex]:
    """Encode every image with the VAE encoder into a latent-index conditioning (reference pipelines/common.py:105-146)."""
    out = []
    for ic in images:
        img = ic.image if ic.image is not None else load_image_tensor(ic.image_path, height, width, dtype)
        if tuple(img.shape[-2:]) != (height, width):
            raise ValueError(f"image is {tuple(img.shape[-2:])}, expected ({height}, {width})")
        if video_encoder is None:
            raise ValueError("image conditioning needs a video_encoder")
        out.append(VideoConditionByLatentIndex(latent=video_encoder(img), strength=ic.strength, latent_idx=ic.frame_index))
    return out


def apply_conditionings(latent_state: LatentState, conditionings, video_tools: VideoLatentTools) -> LatentState:
    for c in conditionings:
        latent_state = c.apply_to(latent_state, video_tools)
    return latent_state


# ---------------------------------------------------------------------- the scaffolding of a stage, one copy for every pipeline
def as_x0model(transformer) -> Tuple[X0Model, bool]:
    """-> (the transformer as an X0Model, whether it is an AudioVideo model)."""
    x0 = transformer if isinstance(transformer, X0Model) else X0Model(transformer)
    return x0, getattr(x0.velocity_model, "model_type", None) == LTXModelType.AudioVideo


def seeded_noiser(device, seed: int) -> GaussianNoiser:
    """The one generator of a call: every stage draws from it in turn."""
    return GaussianNoiser(generator=torch.Generator(device=device).manual_seed(seed))


def video_tools_for(patchifier, num_frames: int, height: int, width: int, fps: float) -> VideoLatentTools:
    """The latent tools of a stage that renders num_frames pixel frames of height x width."""
    pix = VideoPixelShape(batch=1, frames=num_frames, height=height, width=width, fps=fps)
    return VideoLatentTools(patchifier=patchifier, target_shape=VideoLatentShape.from_pixel_shape(pix, latent_channels=128), fps=fps)


def conditioned_initial_state(tools: VideoLatentTools, conditionings, dtype: torch.dtype, device, initial_latent=None) -> LatentState:
    """The patchified start of a stage, zeros on `device` or `initial_latent` (a second stage), with the conditionings applied in order."""
    return apply_conditionings(tools.create_initial_state(dtype=dtype, initial_latent=initial_latent, device=device), conditionings, tools)


def stage_callback(callback: Optional[Callable[[str, int, int], None]], name: str) -> Optional[Callable[[int, int], None]]:
    """A pipeline's (stage, step, total) callback as the (step, total) callback of one stage's loop."""
    return (lambda s, t: callback(name, s, t)) if callback else None


def final_latent(tools, state: LatentState) -> torch.Tensor:
    """The latent of a stage's last state: appended conditioning tokens cut off, unpatchified (video or audio tools)."""
    return tools.unpatchify(tools.clear_conditioning(state)).latent


def upscale_latent_x2(latent: torch.Tensor, spatial_upscaler, video_encoder, video_decoder) -> torch.Tensor:
    """un_normalize -> spatial upscaler -> normalize (reference pipelines/distilled.py:394-405).  The statistics ship with the VAE weights:
    the encoder's only when it actually carries loaded weights (an unloaded SimpleVideoEncoder holds the identity placeholder zeros / ones,
    which would silently mis-scale stage 2), else the decoder's, which also serves when no encoder object is passed."""
    stats = getattr(video_encoder, "per_channel_statistics", None)
    if stats is not None and not getattr(video_encoder, "_loaded", True):
        stats = None
    stats = stats or getattr(video_decoder, "per_channel_statistics", None)
    if stats is None:
        raise ValueError("spatial_upscaler needs per_channel_statistics (un_normalize/normalize) from the video VAE")
    if isinstance(spatial_upscaler, SpatialUpscaler):
        return upscale_latent(latent, spatial_upscaler, stats.mean_of_means, stats.std_of_means)
    return stats.normalize(spatial_upscaler(stats.un_normalize(latent)))


def auto_tiling_config(tiling_config: Optional[TilingConfig], num_frames: int, height: int, width: int) -> Optional[TilingConfig]:
    """The given tiling, or the default one above 4000 latent voxels (reference pipelines/distilled.py:86-98)."""
    if tiling_config is not None:
        return tiling_config
    latent_frames = (num_frames - 1) // 8 + 1
    if latent_frames * (height // 32) * (width // 32) > 4000:
        return TilingConfig.default()
    return None


def decode_video(latent: torch.Tensor, video_decoder, tiling: Optional[TilingConfig]) -> torch.Tensor:
    """The final decode: the latent itself without a decoder, the tiled decode's chunks joined in time with `tiling`, else decode_latent."""
    if video_decoder is None:
        return latent
    if tiling:
        chunks = list(decode_tiled(latent, video_decoder, tiling))
        return torch.cat(chunks, dim=2) if len(chunks) > 1 else chunks[0]
    return decode_latent(latent, video_decoder)


def post_process_latent(denoised: torch.Tensor, denoise_mask: torch.Tensor, clean_latent: torch.Tensor) -> torch.Tensor:
    """Blend denoised output with the clean state: denoised*mask + clean*(1-mask)."""
    if denoise_mask.ndim == 2 and denoised.ndim == 3:
        denoise_mask = denoise_mask[..., None]
    return (denoised * denoise_mask + clean_latent * (1 - denoise_mask)).to(denoised.dtype)


def timesteps_from_mask(denoise_mask: torch.Tensor, sigma: float) -> torch.Tensor:
    return denoise_mask * sigma


def modality_from_state(state: LatentState, context: torch.Tensor, sigma: float, enabled: bool = True, uniform: bool = False) -> Modality:
    """uniform=True: the caller KNOWS the denoise mask is all ones (checked once per loop, not per step), so the timesteps are
    the scalar sigma -- the broadcast AdaLN path, identical arithmetic, N x fewer AdaLN MLP rows."""
    # context_mask is always None (reference pipelines/common.py:223-232)
    sg = torch.full((1,), float(sigma), device=state.latent.device)
    ts = sg if uniform else timesteps_from_mask(state.denoise_mask, sigma)
    return Modality(enabled=enabled, latent=state.latent, timesteps=ts,
                    positions=state.positions, context=context, context_mask=None, sigma=sg)


def audio_modality_from_state(state: LatentState, context: torch.Tensor, sigma: float, enabled: bool = True, uniform: bool = False) -> Modality:
    """Same record for the audio modality (reference pipelines/common.py:235-262)."""
    return modality_from_state(state, context, sigma, enabled, uniform)


_eager_noted = set()


def _note_eager_once(why: str) -> None:
    """use_hip_graph=True but the loop cannot be replayed from the captured graph (say so once per reason)."""
    if why not in _eager_noted:
        _eager_noted.add(why)
        import sys
        print(f"  note: hipGraph replay skipped, the sampling loop runs eagerly: {why}", file=sys.stderr)


def capture_and_replay(capture: Callable[[], None], replay: Callable[[], None]) -> None:
    """Capture a loop's graph on a side stream (capture needs a non-default one) and replay it there once, ordered after the work already
    queued on the current stream and before whatever follows."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        capture()
        replay()
    torch.cuda.current_stream().wait_stream(side)


def _video_loop_inputs(model, video_state: LatentState, video_only: bool = True):
    """What the device-resident video loops step: -> (the video-only model, or with video_only=False the model as it is, whether the mask is
    all ones, the fp32 latent (N, C), cloned as it is stepped in place: never the caller's tensor, and the fp32 mask (N,) / clean latent
    (N, C), None when uniform)."""
    if model.is_av and video_only:
        model = model._video_twin()
    uniform = bool((video_state.denoise_mask == 1).all())
    lat = video_state.latent[0].float().clone(memory_format=torch.contiguous_format)
    mask = None if uniform else video_state.denoise_mask[0].reshape(-1).float().contiguous()
    clean = None if uniform else video_state.clean_latent[0].float().contiguous()
    return model, uniform, lat, mask, clean


def _with_latent(state: LatentState, lat: torch.Tensor) -> LatentState:
    """The state with the stepped fp32 latent (N, C) written back in its own dtype."""
    return state.replace(latent=lat[None].to(state.latent.dtype))


def _prepare_contexts(model, guided: bool, per_token: bool, positions, context, negative_context, audio_positions=None, audio_context=None,
                      negative_audio_context=None):
    """What every device-resident loop prepares: the positive context on `model` and, when guided, the negative one on a clone over the same
    weights, both with the same per_token.  -> the clone, or None."""
    neg = model.clone_sharing_weights() if guided else None
    model.prepare(context, positions, per_token=per_token, audio_context=audio_context, audio_positions=audio_positions)
    if guided:
        neg.prepare(negative_context, positions, per_token=per_token, audio_context=negative_audio_context, audio_positions=audio_positions)
    return neg


def _run_steps(n: int, callback, use_hip_graph: bool, capture: Optional[Callable[[], None]], replay: Optional[Callable[[], None]],
               step: Callable[[int], None], final: Optional[Callable[[int], bool]] = None) -> None:
    """How every device-resident loop runs its n steps: with no callback and fewer than 64 of them as one captured graph, replayed once
    (capture None: the loop has no captured form); otherwise step(i) and the callback n times.  final(i): step i is the loop's last one
    (res_2s), after it the loop ends without a callback."""
    if capture is not None and use_hip_graph and callback is None and n < 64:
        capture_and_replay(capture, replay)
        return
    for i in range(n):
        step(i)
        if final is not None and final(i):
            break
        if callback:
            callback(i + 1, n)


def _res2s_sigmas(sigmas) -> Tuple[int, List[float]]:
    """The res_2s loops' sigma handling, the reference's verbatim: -> (the step count len(sigmas) - 1, taken BEFORE a trailing 0.0 is
    replaced by [0.0011, 0.0]; the sigma_0 .. sigma_n those steps read, rounded to fp32, the engine's scalar type)."""
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    if sig[-1] == 0.0:
        sig = sig[:-1] + [0.0011, 0.0]
    return n, torch.tensor(sig[: n + 1], dtype=torch.float32).tolist()


def _res2s_final(sig: List[float], i: int) -> bool:
    """Step i takes the reference's final-step branch: latent = denoised, no sub-sigma evaluation."""
    return sig[i + 1] <= 0.001 or sig[i + 1] == sig[i]


def joint_denoise_loop(transformer, is_av_model: bool, video_state: LatentState, audio_state: Optional[LatentState], sigmas,
                       video_context: torch.Tensor, audio_context: Optional[torch.Tensor], stepper, callback=None,
                       use_hip_graph: bool = False, *, negative_video_context: Optional[torch.Tensor] = None,
                       negative_audio_context: Optional[torch.Tensor] = None, video_guider=None, audio_guider=None, stg_guider=None,
                       stg_perturbations=None, stg_cutoff: float = 1.0):
    """The guidance-free sampling loop every pipeline here shares (reference pipelines/distilled.py:198-271 and the
    `need_cfg == False` branch of pipelines/one_stage.py:466-568 / :224-330).  Per step and modality:
    Modality(timesteps = denoise_mask * sigma) -> X0Model -> post_process_latent -> EulerDiffusionStep.
    Two equivalent executions: (a) API-faithful, one X0Model call + stepper.step per step; (b) hipGraph replay of the fused
    steps (ltx2_dit_graph_*) when the denoise masks are uniform and no callback needs intermediate states.
    stg_guider / stg_perturbations / stg_cutoff (pipelines/one_stage.py:289-297, :516-526): while (step + 1) / n <= stg_cutoff a further
    evaluation of the positive prompt with `stg_perturbations` (a BatchedPerturbationConfig) and STGGuider.guide on the guided VIDEO
    prediction; the perturbed audio output is dropped.  Always the eager execution.
    `transformer` is an X0Model; returns (video_state, audio_state)."""
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model = transformer.velocity_model
    stg = stg_guider is not None and stg_guider.enabled() and stg_perturbations is not None
    if stg and use_hip_graph:
        _note_eager_once("STG guidance on the eager loop (a projected video guider, or joint audio+video)")
        use_hip_graph = False
    joint = is_av_model and audio_state is not None
    if joint and audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    if is_av_model and not joint:
        model = model._video_twin()        # no audio tokens: the video half alone (reference model.py:829-840), same weights
    states = [video_state] + ([audio_state] if joint else [])
    # a modality whose mask is all ones takes the uniform form (one timestep, the broadcast AdaLN path) in both executions below, whatever the
    # other modality's mask is: the per-token AdaLN path rounds differently, so graph == eager needs the same choice per modality
    unif = [bool((st.denoise_mask == 1).all()) for st in states] + [True]
    uniform = all(unif)                                                       # no conditioning tokens
    # classifier-free guidance (pipelines/one_stage.py:224-330 video, :466-568 joint): a second evaluation with the negative prompt whenever a
    # guider is enabled(); BOTH modalities are then guided by their own guider (a guider at scale 1 returns cond).  The negative prompt runs
    # through a second engine context over the same weights, so each context keeps its own per-prompt text K / V.
    need_cfg = (video_guider is not None and video_guider.enabled()) or (joint and audio_guider is not None and audio_guider.enabled())
    neg = None
    if need_cfg:
        if negative_video_context is None or (joint and negative_audio_context is None):
            raise ValueError("guidance needs the negative prompt's encoding(s)")
        neg = X0Model(model.clone_sharing_weights())
    if use_hip_graph and not (callback is None and not need_cfg):
        _note_eager_once("a step callback" if callback is not None else "classifier-free guidance (two evaluations per step)")
    if use_hip_graph and callback is None and not need_cfg:
        lat = video_state.latent[0].float().contiguous()
        alat = audio_state.latent[0].float().contiguous() if joint else None
        # conditioning tokens (image-to-video): the captured steps form timesteps = denoise_mask * sigma_i on the device and blend x0 with the
        # clean latent (reference pipelines/common.py:193-232); a modality whose mask is all ones takes the uniform form
        cond = {}
        if not uniform:
            for key, st_ in (("", video_state),) + ((("audio_", audio_state),) if joint else ()):
                if not bool((st_.denoise_mask == 1).all()):
                    cond[key + "denoise_mask"] = st_.denoise_mask[0].reshape(-1).float().contiguous()
                    cond[key + "clean_latent"] = st_.clean_latent[0].float().contiguous()
        if joint:
            model.prepare(video_context, video_state.positions, per_token=not uniform, audio_context=audio_context, audio_positions=audio_state.positions)
        else:
            model.prepare(video_context, video_state.positions, per_token=not uniform)
        capture_and_replay(lambda: model.capture_denoise_graph(lat, sig, audio_latent=alat, **cond), model.replay_denoise_graph)
        return _with_latent(video_state, lat), (_with_latent(audio_state, alat) if joint else audio_state)
    for i in range(n):
        vm = modality_from_state(video_state, video_context, sig[i], uniform=unif[0])
        am = audio_modality_from_state(audio_state, audio_context, sig[i], uniform=unif[1]) if joint else None
        if joint:
            vx0, ax0 = transformer(vm, am)
        else:
            out = transformer(vm)
            vx0, ax0 = (out[0] if isinstance(out, tuple) else out), None
        if need_cfg:
            nvm = modality_from_state(video_state, negative_video_context, sig[i], uniform=unif[0])
            if joint:
                nvx0, nax0 = neg(nvm, audio_modality_from_state(audio_state, negative_audio_context, sig[i], uniform=unif[1]))
                ax0 = audio_guider.guide(ax0, nax0) if audio_guider is not None else ax0
            else:
                nvx0 = neg(nvm)
            vx0 = video_guider.guide(vx0, nvx0) if video_guider is not None else vx0
        if stg and (i + 1) / n <= stg_cutoff:
            pout = transformer(vm, am, perturbations=stg_perturbations) if joint else transformer(vm, perturbations=stg_perturbations)
            vx0 = stg_guider.guide(vx0, pout[0] if isinstance(pout, tuple) else pout)
        vx0 = post_process_latent(vx0, video_state.denoise_mask, video_state.clean_latent)
        video_state = video_state.replace(latent=stepper.step(sample=video_state.latent, denoised_sample=vx0, sigmas=sig, step_index=i))
        if joint:
            ax0 = post_process_latent(ax0, audio_state.denoise_mask, audio_state.clean_latent)
            audio_state = audio_state.replace(latent=stepper.step(sample=audio_state.latent, denoised_sample=ax0, sigmas=sig, step_index=i))
        if callback:
            callback(i + 1, n)
    return video_state, audio_state


def guided_denoise_loop(transformer, video_state: LatentState, sigmas, context: torch.Tensor, negative_context: Optional[torch.Tensor],
                        guider, stepper, callback=None, use_hip_graph: bool = True) -> LatentState:
    """Classifier-free guidance on the video-only model that does not leave the device (the reference's keyframe stage 1,
    pipelines/keyframe_interpolation.py:223-296, and the video branch of pipelines/one_stage.py:224-330).  With a plain CFGGuider that is
    enabled(), every step is ONE C call -- forward(positive), forward(negative), then x0 x 2 + guide + post_process_latent + Euler in one
    kernel (LTXModel.guided_step_) -- and with no callback and fewer than 64 steps the whole loop is one captured graph.  A guider that is
    not enabled, or any other guider class (CFGStarRescalingGuider's projection is a reduction over the latent), goes through
    joint_denoise_loop.  `transformer` is an X0Model; an AudioVideo model is used through its video twin.  Returns the video state."""
    from ..components.guiders import CFGGuider
    model = transformer.velocity_model
    if type(guider) is not CFGGuider or not guider.enabled():
        return joint_denoise_loop(transformer, model.is_av, video_state, None, sigmas, context, None, stepper, callback, use_hip_graph,
                                  negative_video_context=negative_context, video_guider=guider)[0]
    if negative_context is None:
        raise ValueError("guidance needs the negative prompt's encoding")
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state)
    neg = _prepare_contexts(model, True, not uniform, video_state.positions, context, negative_context)
    cond = dict(denoise_mask=mask, clean_latent=clean)
    vm = lambda i: modality_from_state(video_state.replace(latent=lat[None]), context, sig[i], uniform=uniform)      # noqa: E731
    _run_steps(n, callback, use_hip_graph, lambda: model.capture_guided_graph(neg, lat, sig, guider.scale, **cond), model.replay_guided_graph,
               lambda i: model.guided_step_(neg, lat, vm(i), sig[i], sig[i + 1], guider.scale, **cond))
    return _with_latent(video_state, lat)


def rescale_noise_cfg(noise_cfg: torch.Tensor, noise_pred_text: torch.Tensor, guidance_rescale: float = 0.7) -> torch.Tensor:
    """The reference's rescale_noise_cfg (scripts/generate.py:688-727) on token-layout predictions (B, N, C): per channel, over the tokens (its
    axes 2, 3, 4 of (B, C, F, H, W)), the guided prediction is given the conditional one's mean and standard deviation, then blended with
    itself by guidance_rescale.  Its statements in order."""
    cfg_mean = noise_cfg.mean(dim=1, keepdim=True)
    cfg_std = torch.sqrt(((noise_cfg - cfg_mean) ** 2).mean(dim=1, keepdim=True) + 1e-8)
    text_mean = noise_pred_text.mean(dim=1, keepdim=True)
    text_std = torch.sqrt(((noise_pred_text - text_mean) ** 2).mean(dim=1, keepdim=True) + 1e-8)
    rescaled = (noise_cfg - cfg_mean) / cfg_std * text_std + text_mean
    return guidance_rescale * rescaled + (1 - guidance_rescale) * noise_cfg


def standard_cfg_denoise_loop(transformer, video_state: LatentState, sigmas, context: torch.Tensor, negative_context: Optional[torch.Tensor],
                              cfg_scale: float, guidance_rescale: float, callback=None, use_hip_graph: bool = True, fused: bool = True,
                              first_block_cache: float = 0.0) -> LatentState:
    """The guided branch of the reference's standard one-stage loop (scripts/generate.py:1895-1976: the dev video-only model under classifier-free
    guidance): per step the positive and the negative prompt, g = uncond + cfg_scale*(cond - uncond) on the x0 predictions, with
    guidance_rescale > 0 rescale_noise_cfg(g, cond, guidance_rescale), then the x0 Euler step.  fused=True: every step is ONE C call
    (LTXModel.rescaled_guided_step_: the two forwards, the per-channel statistics, the step kernel) and with no callback and fewer than 64
    steps the loop is one captured graph.  fused=False: the reference's statements one by one in torch through X0Model, the comparison form.
    cfg_scale <= 1 is the unguided loop (joint_denoise_loop), as the reference guides only above 1.  The route has no conditioning: the
    denoise mask must be all ones.  `transformer` is an X0Model of a video-only model.  Returns the video state.
    first_block_cache = t > 0 (an MI355X addition): the fused loop with every evaluation through the first-block cache at
    threshold t, the positive pass in slot 0 and the negative one in slot 1 -- eager, one C call per step, as each evaluation reads its decision
    back; with cfg_scale <= 1 the plain loop through slot 0.  The model's cache is left off afterwards; first_block_cache_last_stats() holds the
    loop's counts.  A negative threshold is a ValueError."""
    from ..components import EulerDiffusionStep
    model = transformer.velocity_model
    if not float(first_block_cache) >= 0.0:
        raise ValueError(f"first_block_cache={first_block_cache!r} must be >= 0 (0: off)")
    if model.is_av:
        if first_block_cache > 0:
            raise NotImplementedError("first_block_cache is built for the video-only model alone (AudioVideo / LTX-2.3 joint models are outside it)")
        raise ValueError("standard_cfg_denoise_loop runs the video-only model (AudioVideo models are guided by OneStagePipeline)")
    if first_block_cache > 0:
        if not fused:
            raise NotImplementedError("first_block_cache runs the fused loop (fused=False is the torch comparison form)")
        if not bool((video_state.denoise_mask == 1).all()):
            raise ValueError("standard_cfg_denoise_loop has no conditioning (the reference's standard loop has none): the denoise mask must be all ones")
        if cfg_scale > 1.0 and negative_context is None:
            raise ValueError("guidance needs the negative prompt's encoding")
        return _first_block_cache_loop(model, video_state, sigmas, context, negative_context if cfg_scale > 1.0 else None, cfg_scale,
                                       guidance_rescale, float(first_block_cache), callback, use_hip_graph)
    if not cfg_scale > 1.0:
        return joint_denoise_loop(transformer, False, video_state, None, sigmas, context, None, EulerDiffusionStep(), callback, use_hip_graph)[0]
    if negative_context is None:
        raise ValueError("guidance needs the negative prompt's encoding")
    if not bool((video_state.denoise_mask == 1).all()):
        raise ValueError("standard_cfg_denoise_loop has no conditioning (the reference's standard loop has none): the denoise mask must be all ones")
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    if not fused:
        from .. import kernels as K
        neg = X0Model(model.clone_sharing_weights())
        c = video_state.latent.shape[-1]
        for i in range(n):
            cond = transformer(modality_from_state(video_state, context, sig[i], uniform=True))
            uncond = neg(modality_from_state(video_state, negative_context, sig[i], uniform=True))
            denoised = uncond + cfg_scale * (cond - uncond)
            if guidance_rescale > 0:
                denoised = rescale_noise_cfg(denoised, cond, guidance_rescale)
            lat = video_state.latent
            video_state = video_state.replace(latent=K.euler_step(lat.reshape(-1, c).float(), denoised.reshape(-1, c).float(), sig[i], sig[i + 1])
                                              .reshape(lat.shape).to(lat.dtype))
            if callback:
                callback(i + 1, n)
        return video_state
    model, _, lat, _, _ = _video_loop_inputs(model, video_state)
    neg = _prepare_contexts(model, True, False, video_state.positions, context, negative_context)
    vm = lambda i: modality_from_state(video_state.replace(latent=lat[None]), context, sig[i], uniform=True)      # noqa: E731
    _run_steps(n, callback, use_hip_graph, lambda: model.capture_rescaled_guided_graph(neg, lat, sig, cfg_scale, guidance_rescale),
               model.replay_rescaled_guided_graph, lambda i: model.rescaled_guided_step_(neg, lat, vm(i), sig[i], sig[i + 1], cfg_scale, guidance_rescale))
    return _with_latent(video_state, lat)


_fbc_last_stats: List[dict] = []


def first_block_cache_last_stats() -> List[dict]:
    """Per slot, the counts of the last loop that ran with first_block_cache > 0 (LTXModel.first_block_cache_stats() at its end)."""
    return [dict(d) for d in _fbc_last_stats]


def first_block_cache_summary(stats: List[dict], threshold: float) -> str:
    """The one line a run with the cache on prints."""
    k, m = sum(d["skips"] for d in stats), sum(d["evaluations"] for d in stats)
    return f"first-block cache: {k} of {m} evaluations reused the tail (threshold {threshold:g})"


def _first_block_cache_loop(model, video_state: LatentState, sigmas, context, negative_context, cfg_scale: float, guidance_rescale: float,
                            threshold: float, callback, use_hip_graph: bool) -> LatentState:
    """The standard loop with the first-block cache on: negative_context None is the plain loop (slot 0), otherwise the guided one (slots 0 and
    1).  The driver's three rules: every slot is reset at the start, the last step is forced to compute (the first one computes anyway: its
    slots are not valid), and the counts are read at the end.  The cache is configured on the positive context alone."""
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    guided = negative_context is not None
    if use_hip_graph:
        _note_eager_once("the first-block cache reads a decision back per evaluation")
    model, _, lat, _, _ = _video_loop_inputs(model, video_state)
    neg = _prepare_contexts(model, guided, False, video_state.positions, context, negative_context)
    vm = lambda i: modality_from_state(video_state.replace(latent=lat[None]), context, sig[i], uniform=True)      # noqa: E731
    model.enable_first_block_cache(threshold, slots=2 if guided else 1)
    try:
        model.reset_first_block_cache()
        for i in range(n):
            if i == n - 1:
                model.force_first_block_cache(-1)
            if guided:
                model.rescaled_guided_step_cached_(neg, lat, vm(i), sig[i], sig[i + 1], cfg_scale, guidance_rescale, slots=(0, 1))
            else:
                model.denoise_step_cached_(lat, vm(i), sig[i], sig[i + 1], slot=0)
            if callback:
                callback(i + 1, n)
        torch.cuda.synchronize()
        _fbc_last_stats[:] = model.first_block_cache_stats()
    finally:
        model.enable_first_block_cache(0.0, slots=0)
    return _with_latent(video_state, lat)


def stg_denoise_loop(transformer, video_state: LatentState, sigmas, context: torch.Tensor, negative_context: Optional[torch.Tensor], guider,
                     stg_guider, stg_blocks: Optional[List[int]], stg_cutoff: float, stepper, callback=None, use_hip_graph: bool = True) -> LatentState:
    """guided_denoise_loop with spatio-temporal guidance on top (pipelines/one_stage.py:267-326): while (step + 1) / n <= stg_cutoff a third
    evaluation of the positive prompt with the video self-attention of `stg_blocks` (None: every block) skipped, and STGGuider.guide on the
    CFG-guided prediction.  With a plain CFGGuider, or a guider that is not enabled (then no negative evaluation), every step is ONE C call
    -- the two or three evaluations, then x0 x 3 + both guiders + post_process_latent + Euler in one kernel (LTXModel.stg_step_) -- and with
    no callback and fewer than 64 steps the whole loop is one captured graph.  The perturbed pass runs on the positive context itself.  Any
    other enabled guider class goes through joint_denoise_loop's eager STG path; an STG guider that is not enabled through
    guided_denoise_loop.  `transformer` is an X0Model; an AudioVideo model is used through its video twin.  Returns the video state."""
    from ..components.guiders import CFGGuider
    from ..components.perturbations import create_batched_stg_config
    model = transformer.velocity_model
    if stg_guider is None or not stg_guider.enabled():
        return guided_denoise_loop(transformer, video_state, sigmas, context, negative_context, guider, stepper, callback, use_hip_graph)
    cfg = guider is not None and guider.enabled()
    if cfg and type(guider) is not CFGGuider:
        return joint_denoise_loop(transformer, model.is_av, video_state, None, sigmas, context, None, stepper, callback, use_hip_graph,
                                  negative_video_context=negative_context, video_guider=guider, stg_guider=stg_guider,
                                  stg_perturbations=create_batched_stg_config(1, blocks=stg_blocks), stg_cutoff=stg_cutoff)[0]
    if cfg and negative_context is None:
        raise ValueError("guidance needs the negative prompt's encoding")
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state)
    model.set_stg_blocks(stg_blocks)
    neg = _prepare_contexts(model, cfg, not uniform, video_state.positions, context, negative_context)
    cfg_scale = guider.scale if cfg else 1.0
    vel_p = torch.empty_like(lat)
    cond = dict(denoise_mask=mask, clean_latent=clean)

    def step(i):
        vm = modality_from_state(video_state.replace(latent=lat[None]), context, sig[i], uniform=uniform)
        if (i + 1) / n <= stg_cutoff:
            model.stg_step_(neg, lat, vm, sig[i], sig[i + 1], cfg_scale, stg_guider.scale, vel_p, **cond)
        elif cfg:
            model.guided_step_(neg, lat, vm, sig[i], sig[i + 1], cfg_scale, **cond)
        else:
            model.denoise_step_(lat, vm, sig[i], sig[i + 1], **cond)

    _run_steps(n, callback, use_hip_graph, lambda: model.capture_stg_graph(neg, lat, sig, cfg_scale, stg_guider.scale, vel_p, stg_cutoff, **cond),
               model.replay_stg_graph, step)
    return _with_latent(video_state, lat)


def joint_stg_perturbations(stg_blocks: Optional[List[int]], video: bool, audio: bool):
    """The BatchedPerturbationConfig (batch 1) of the joint STG loop: the video and / or the audio self-attention of `stg_blocks` (None: every
    block) skipped."""
    from ..components.perturbations import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType as PT
    kinds = ([PT.SKIP_VIDEO_SELF_ATTN] if video else []) + ([PT.SKIP_AUDIO_SELF_ATTN] if audio else [])
    return BatchedPerturbationConfig([PerturbationConfig([Perturbation(k, stg_blocks) for k in kinds])])


def joint_stg_denoise_loop(transformer, video_state: LatentState, audio_state: LatentState, sigmas, video_context: torch.Tensor,
                           audio_context: torch.Tensor, negative_video_context: Optional[torch.Tensor],
                           negative_audio_context: Optional[torch.Tensor], video_guider, audio_guider, stg_guider, audio_stg_guider,
                           stg_blocks: Optional[List[int]], stg_cutoff: float, callback=None, use_hip_graph: bool = True,
                           fused: bool = True) -> Tuple[LatentState, LatentState]:
    """Spatio-temporal guidance over BOTH modalities of an AudioVideo model (the joint branch of OneStagePipeline, pipelines/one_stage.py:466-568
    with :516-526, and an STG term on the audio as the two-stage pipeline's multimodal guider applies one): while (step + 1) / n <= stg_cutoff --
    decided in double on the host, as stg_denoise_loop decides it -- a third evaluation of the positive prompts with the video self-attention of
    `stg_blocks` (None: every block) skipped when stg_guider is enabled and the audio self-attention of the same blocks when audio_stg_guider
    is, and each enabled STG guider pushes its modality's CFG-guided prediction away from it.  video_guider / audio_guider: a plain CFGGuider,
    None or not enabled, per modality; when neither is enabled there is no negative evaluation.  At least one STG guider is enabled.
    fused=True: every step is ONE C call (LTXModel.stg_step_joint_av_: the two or three evaluations, then one kernel over both latents); the
    steps past the cutoff are guided_step_joint_av_, or the plain joint step without CFG.  There is no captured form of this loop:
    use_hip_graph is accepted for the signature the other loops share and answered with the usual one-time note.
    fused=False: the same loop from the existing parts, the comparison form -- the X0Model calls through the same forward entries, the
    guiders, post_process_latent and EulerDiffusionStep in torch.
    Both latents are held in fp32 across the loop in either form; each modality takes the uniform or the per-token form by its own mask.
    `transformer` is an X0Model over an AudioVideo model.  Returns (video_state, audio_state)."""
    from ..components import EulerDiffusionStep
    model = transformer.velocity_model
    if not model.is_av or audio_state is None:
        raise ValueError("joint_stg_denoise_loop requires an audio-video (AV) model and an audio state")
    if audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    guiders, stg_guiders = (video_guider, audio_guider), (stg_guider, audio_stg_guider)
    if not heun_device_form(*guiders):
        raise ValueError("joint_stg_denoise_loop runs under a plain CFGGuider (or none) per modality")
    stg = [g.scale if (g is not None and g.enabled()) else 0.0 for g in stg_guiders]
    if not any(stg):
        raise ValueError("joint_stg_denoise_loop: neither STG guider is enabled; that loop is joint_projected_denoise_loop")
    on = [g is not None and g.enabled() for g in guiders]
    need_cfg = any(on)
    if need_cfg and (negative_video_context is None or negative_audio_context is None):
        raise ValueError("guidance needs the negative prompt's encoding(s)")
    scale = [g.scale if e else 1.0 for g, e in zip(guiders, on)]
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=False)
    _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
    states = lambda: (video_state.replace(latent=lat[None]), audio_state.replace(latent=alat[None]))      # noqa: E731
    modalities = lambda st, ast, vc, ac, s: (modality_from_state(st, vc, s, uniform=uniform),      # noqa: E731
                                             audio_modality_from_state(ast, ac, s, uniform=a_uniform))
    if not fused:
        neg = X0Model(model.clone_sharing_weights()) if need_cfg else None
        perturbations = joint_stg_perturbations(stg_blocks, stg[0] != 0.0, stg[1] != 0.0)
        stepper = EulerDiffusionStep()
        for i in range(n):
            st, ast = states()
            pair = modalities(st, ast, video_context, audio_context, sig[i])
            x0 = list(transformer(*pair))
            if need_cfg:
                nx0 = neg(*modalities(st, ast, negative_video_context, negative_audio_context, sig[i]))
                x0 = [g.guide(p, q) if e else p for g, e, p, q in zip(guiders, on, x0, nx0)]
            if (i + 1) / n <= stg_cutoff:
                px0 = transformer(*pair, perturbations=perturbations)
                x0 = [g.guide(p, q) if s != 0.0 else p for g, s, p, q in zip(stg_guiders, stg, x0, px0)]
            lat = stepper.step(sample=st.latent, denoised_sample=post_process_latent(x0[0], st.denoise_mask, st.clean_latent), sigmas=sig, step_index=i)[0]
            alat = stepper.step(sample=ast.latent, denoised_sample=post_process_latent(x0[1], ast.denoise_mask, ast.clean_latent), sigmas=sig, step_index=i)[0]
            if callback:
                callback(i + 1, n)
        return _with_latent(video_state, lat), _with_latent(audio_state, alat)
    for k in (0, 1):
        model.set_stg_blocks(stg_blocks if stg[k] != 0.0 else [], k)
    neg = _prepare_contexts(model, need_cfg, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                            audio_state.positions, audio_context, negative_audio_context)
    cond = dict(denoise_mask=mask, clean_latent=clean, audio_denoise_mask=amask, audio_clean_latent=aclean)
    vel_p, avel_p = torch.empty_like(lat), torch.empty_like(alat)
    if use_hip_graph:
        _note_eager_once("the joint audio+video STG loop has no captured form")

    def step(i):
        vm, am = modalities(*states(), video_context, audio_context, sig[i])
        if (i + 1) / n <= stg_cutoff:
            model.stg_step_joint_av_(neg, lat, alat, vm, am, sig[i], sig[i + 1], scale[0], scale[1], stg[0], stg[1], vel_p, avel_p, **cond)
        elif need_cfg:
            model.guided_step_joint_av_(neg, lat, alat, vm, am, sig[i], sig[i + 1], scale[0], scale[1], **cond)
        else:
            model.denoise_step_(lat, vm, sig[i], sig[i + 1], audio_latent=alat, audio=am, **cond)

    _run_steps(n, callback, use_hip_graph, None, None, step)
    return _with_latent(video_state, lat), _with_latent(audio_state, alat)


def frozen_audio_guided_loop(transformer, video_state: LatentState, audio_state: LatentState, sigmas, video_context: torch.Tensor,
                             audio_context: torch.Tensor, negative_video_context: Optional[torch.Tensor],
                             negative_audio_context: Optional[torch.Tensor], cfg_scale: float, stepper, callback=None,
                             use_hip_graph: bool = True) -> Tuple[LatentState, LatentState]:
    """Audio-to-video sampling on the AudioVideo model (the reference's _video_only_denoise_loop, pipelines/a2vid_two_stage.py:225-271): the
    audio state is a given latent with an all-zero denoise mask, fed to every evaluation and never stepped; classifier-free guidance,
    post_process_latent and the Euler step act on the video alone.  With cfg_scale > 1 and a negative video context every step is ONE C call
    -- both modalities through the positive and through the negative context, then the guided Euler kernel on the video latent
    (LTXModel.guided_step_av_) -- and with no callback and fewer than 64 steps the whole loop is one captured graph.  The negative pass
    takes `negative_audio_context or audio_context`, as the reference does.  Without guidance the loop is joint_denoise_loop's frozen-audio
    path, unchanged.  `transformer` is an X0Model over an AudioVideo model.  Returns (video_state, the audio_state object it was given)."""
    if not bool((audio_state.denoise_mask == 0).all()):
        raise ValueError("frozen_audio_guided_loop: the audio state's denoise mask must be all zero (the audio latent is given, not sampled)")
    model = transformer.velocity_model
    if not model.is_av:
        raise ValueError("frozen_audio_guided_loop requires an audio-video (AV) model")
    if audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    if not (cfg_scale > 1.0 and negative_video_context is not None):
        video_state, _ = joint_denoise_loop(transformer, True, video_state, audio_state, sigmas, video_context, audio_context, stepper, callback, use_hip_graph)
        return video_state, audio_state
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=False)
    alat = audio_state.latent[0].float().contiguous()
    amask = audio_state.denoise_mask[0].reshape(-1).float().contiguous()
    negative_audio_context = negative_audio_context if negative_audio_context is not None else audio_context
    neg = _prepare_contexts(model, True, True, video_state.positions, video_context, negative_video_context, audio_state.positions, audio_context,
                            negative_audio_context)
    cond = dict(denoise_mask=mask, clean_latent=clean)
    vm = lambda i: modality_from_state(video_state.replace(latent=lat[None]), video_context, sig[i], uniform=uniform)      # noqa: E731
    _run_steps(n, callback, use_hip_graph, lambda: model.capture_guided_av_graph(neg, lat, alat, sig, cfg_scale, audio_denoise_mask=amask, **cond),
               model.replay_guided_av_graph,
               lambda i: model.guided_step_av_(neg, lat, alat, vm(i), audio_modality_from_state(audio_state, audio_context, sig[i]), sig[i], sig[i + 1],
                                               cfg_scale, **cond))
    return _with_latent(video_state, lat), audio_state


def joint_guided_denoise_loop(transformer, video_state: LatentState, audio_state: LatentState, sigmas, video_context: torch.Tensor,
                              audio_context: torch.Tensor, negative_video_context: Optional[torch.Tensor],
                              negative_audio_context: Optional[torch.Tensor], cfg_scale: float, audio_cfg_scale: float, stepper, callback=None,
                              use_hip_graph: bool = True) -> Tuple[LatentState, LatentState]:
    """Classifier-free guidance over BOTH modalities of an AudioVideo model without leaving the device (the reference's RetakePipeline._denoise_loop,
    pipelines/retake.py:234-291, run with an audio state): per step both modalities through the positive and through the negative contexts,
    then CFGGuider.guide, post_process_latent and the Euler step on both latents, the video under cfg_scale and the audio under
    audio_cfg_scale.  Every step is ONE C call (LTXModel.guided_step_joint_av_: the evaluations, then one kernel over both latents) and with no
    callback and fewer than 64 steps the whole loop is one captured graph.  Each modality takes the uniform or the per-token form by its
    own mask.  The guidance is CFGGuider's a + (s - 1)*(a - b), as guided_denoise_loop forms it; the reference's line writes the same
    quantity as b + s*(a - b).  When neither scale exceeds 1, or a negative context is missing, there is no negative pass: the loop is
    joint_denoise_loop's, captured for the masked joint case.  `transformer` is an X0Model over an AudioVideo model.  Returns (video_state,
    audio_state)."""
    model = transformer.velocity_model
    if not model.is_av or audio_state is None:
        raise ValueError("joint_guided_denoise_loop requires an audio-video (AV) model and an audio state")
    if audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    if not (cfg_scale > 1.0 or audio_cfg_scale > 1.0) or negative_video_context is None or negative_audio_context is None:
        return joint_denoise_loop(transformer, True, video_state, audio_state, sigmas, video_context, audio_context, stepper, callback, use_hip_graph)
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=False)
    _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
    neg = _prepare_contexts(model, True, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                            audio_state.positions, audio_context, negative_audio_context)
    cond = dict(denoise_mask=mask, clean_latent=clean, audio_denoise_mask=amask, audio_clean_latent=aclean)

    def step(i):
        st, ast = video_state.replace(latent=lat[None]), audio_state.replace(latent=alat[None])
        model.guided_step_joint_av_(neg, lat, alat, modality_from_state(st, video_context, sig[i], uniform=uniform),
                                    audio_modality_from_state(ast, audio_context, sig[i], uniform=a_uniform), sig[i], sig[i + 1], cfg_scale,
                                    audio_cfg_scale, **cond)

    _run_steps(n, callback, use_hip_graph, lambda: model.capture_guided_joint_graph(neg, lat, alat, sig, cfg_scale, audio_cfg_scale, **cond),
               model.replay_guided_joint_graph, step)
    return _with_latent(video_state, lat), _with_latent(audio_state, alat)


def projected_guider_args(guider) -> Optional[dict]:
    """The (mode, scale, eta, norm_threshold, momentum) of LTXModel.projected_step_ for a guider whose scalars are sums over the latent; None
    for every other object."""
    from ..components.guiders import CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider
    if type(guider) is CFGStarRescalingGuider:
        return dict(mode=0, scale=guider.scale, eta=1.0, norm_threshold=0.0, momentum=0.0)
    if type(guider) is LtxAPGGuider:
        return dict(mode=1, scale=guider.scale, eta=guider.eta, norm_threshold=guider.norm_threshold, momentum=0.0)
    if type(guider) is LegacyStatefulAPGGuider:
        return dict(mode=2, scale=guider.scale, eta=guider.eta, norm_threshold=guider.norm_threshold, momentum=guider.momentum)
    return None


def reset_guider(guider) -> None:
    """A stateful guider starts every loop without its running state (LegacyStatefulAPGGuider.reset; the reference never clears it)."""
    if hasattr(guider, "reset"):
        guider.reset()


def projected_denoise_loop(transformer, video_state: LatentState, sigmas, context: torch.Tensor, negative_context: Optional[torch.Tensor],
                           guider, stepper, callback=None, use_hip_graph: bool = True) -> LatentState:
    """guided_denoise_loop for the guiders whose scalars are sums over the whole latent: an enabled CFGStarRescalingGuider, LtxAPGGuider or
    LegacyStatefulAPGGuider runs every step as ONE C call -- forward(positive), forward(negative), the sums kernel, the projected step kernel
    (LTXModel.projected_step_) -- and with no callback and fewer than 64 steps the whole loop is one captured graph.  The sums run over all
    tokens of the state, appended conditioning tokens included, as the reference's guider sees the whole denoised tensor.  A stateful
    guider's running guidance lives on the device for the loop and starts cleared.  A plain CFGGuider is handed to guided_denoise_loop;
    anything else, or a guider that is not enabled, goes to joint_denoise_loop.  Returns the video state."""
    from ..components.guiders import CFGGuider
    reset_guider(guider)
    model = transformer.velocity_model
    if type(guider) is CFGGuider:
        return guided_denoise_loop(transformer, video_state, sigmas, context, negative_context, guider, stepper, callback, use_hip_graph)
    args = projected_guider_args(guider)
    if args is None or not guider.enabled():
        return joint_denoise_loop(transformer, model.is_av, video_state, None, sigmas, context, None, stepper, callback, use_hip_graph,
                                  negative_video_context=negative_context, video_guider=guider)[0]
    if negative_context is None:
        raise ValueError("guidance needs the negative prompt's encoding")
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state)
    neg = _prepare_contexts(model, True, not uniform, video_state.positions, context, negative_context)
    cond = dict(denoise_mask=mask, clean_latent=clean, **args)
    vm = lambda i: modality_from_state(video_state.replace(latent=lat[None]), context, sig[i], uniform=uniform)      # noqa: E731
    _run_steps(n, callback, use_hip_graph, lambda: model.capture_projected_graph(neg, lat, sig, **cond), model.replay_projected_graph,
               lambda i: model.projected_step_(neg, lat, vm(i), sig[i], sig[i + 1], first=(i == 0), **cond))
    return _with_latent(video_state, lat)


def joint_guider_args(guider) -> Optional[dict]:
    """One modality's guider of LTXModel.projected_step_joint_av_: projected_guider_args for the guiders it knows, mode 3 for a plain CFGGuider,
    mode 4 for a guider that is None or not enabled (whatever its class); None for an enabled guider of any other class."""
    from ..components.guiders import CFGGuider
    if guider is None or not guider.enabled():
        return dict(mode=4, scale=1.0)
    if type(guider) is CFGGuider:
        return dict(mode=3, scale=guider.scale)
    return projected_guider_args(guider)


def joint_projected_denoise_loop(transformer, video_state: LatentState, audio_state: LatentState, sigmas, video_context: torch.Tensor,
                                 audio_context: torch.Tensor, negative_video_context: Optional[torch.Tensor],
                                 negative_audio_context: Optional[torch.Tensor], video_guider, audio_guider, stepper, callback=None,
                                 use_hip_graph: bool = True) -> Tuple[LatentState, LatentState]:
    """joint_guided_denoise_loop with a guider object per modality (the reference's _denoise_loop_cfg_av, pipelines/one_stage.py:466-568, whose
    default guiders are a CFGStarRescalingGuider each): per step both modalities through the positive and through the negative contexts, then each
    modality's guider, post_process_latent and the Euler step on both latents.  Every step is ONE C call (LTXModel.projected_step_joint_av_: the
    evaluations, one sums kernel over the modalities whose guider reads sums, one step kernel over both latents) and with no callback and fewer
    than 64 steps the whole loop is one captured graph.  Each guider is a CFGGuider, a guider projected_guider_args knows
    (CFGStarRescalingGuider, LtxAPGGuider, LegacyStatefulAPGGuider) or not enabled; a stateful guider's running guidance lives on the device
    for the loop and starts cleared.  The sums run over all tokens of a modality, on the device in fp64 (the torch guiders reduce in fp32).
    When neither guider is enabled, or a negative context is missing, the loop is joint_denoise_loop's; an enabled guider of another class is
    a ValueError.  `transformer` is an X0Model over an AudioVideo model.  Returns (video_state, audio_state)."""
    model = transformer.velocity_model
    if not model.is_av or audio_state is None:
        raise ValueError("joint_projected_denoise_loop requires an audio-video (AV) model and an audio state")
    if audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    guiders = (video_guider, audio_guider)
    for g in guiders:
        reset_guider(g)
    args = [joint_guider_args(g) for g in guiders]
    if any(a is None for a in args):
        raise ValueError("joint_projected_denoise_loop: a guider is a CFGGuider, a CFGStarRescalingGuider, an LtxAPGGuider, a LegacyStatefulAPGGuider or not enabled")
    if all(a["mode"] == 4 for a in args) or negative_video_context is None or negative_audio_context is None:
        return joint_denoise_loop(transformer, True, video_state, audio_state, sigmas, video_context, audio_context, stepper, callback, use_hip_graph,
                                  negative_video_context=negative_video_context, negative_audio_context=negative_audio_context,
                                  video_guider=video_guider, audio_guider=audio_guider)
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=False)
    _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
    neg = _prepare_contexts(model, True, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                            audio_state.positions, audio_context, negative_audio_context)
    run, arun = (torch.zeros_like(t) if a.get("momentum") else None for a, t in zip(args, (lat, alat)))
    cond = dict(video_guider=args[0], audio_guider=args[1], running=run, audio_running=arun, denoise_mask=mask, clean_latent=clean,
                audio_denoise_mask=amask, audio_clean_latent=aclean)

    def step(i):
        st, ast = video_state.replace(latent=lat[None]), audio_state.replace(latent=alat[None])
        model.projected_step_joint_av_(neg, lat, alat, modality_from_state(st, video_context, sig[i], uniform=uniform),
                                       audio_modality_from_state(ast, audio_context, sig[i], uniform=a_uniform), sig[i], sig[i + 1], first=(i == 0), **cond)

    _run_steps(n, callback, use_hip_graph, lambda: model.capture_projected_joint_graph(neg, lat, alat, sig, **cond), model.replay_projected_joint_graph, step)
    return _with_latent(video_state, lat), _with_latent(audio_state, alat)


def res2s_denoise_loop(transformer, video_state: LatentState, sigmas, context: torch.Tensor, negative_context: Optional[torch.Tensor],
                       cfg_scale: float, audio_cfg_scale: float = 7.0, callback=None, use_hip_graph: bool = True) -> LatentState:
    """The HQ pipeline's res_2s loop on the video-only model (reference pipelines/ti2vid_hq.py:153-273), without leaving the device: every
    step is ONE C call -- two pairs of evaluations, the midpoint and the combine kernel (LTXModel.res2s_step_) -- and with no callback
    and fewer than 64 steps the whole loop is one captured graph.
    The reference's sigma handling is kept verbatim: the step count is len(sigmas) - 1, taken BEFORE a trailing 0.0 is replaced by
    [0.0011, 0.0], so a scheduler table's last step lands on sigma = 0.0011 and the final-step branch (sigma_next <= 0.001 or h == 0:
    latent = denoised, loop ends, no callback) is reached only by tables that end otherwise.  The negative evaluation runs under the
    reference's condition, (cfg_scale > 1 or audio_cfg_scale > 1) and negative_context is not None.  The sigmas are rounded to fp32 (the
    engine's scalar type, 0.0011 included) and the latent is held in fp32 across the loop, as guided_denoise_loop holds it; the
    reference's per-step cast to the state dtype is not reproduced.  `transformer` is an X0Model; an AudioVideo model is used through its
    video twin (res2s_av_denoise_loop steps both modalities).  Returns the video state."""
    n, sig = _res2s_sigmas(sigmas)
    model, uniform, lat, mask, clean = _video_loop_inputs(transformer.velocity_model, video_state)
    guide = (cfg_scale > 1.0 or audio_cfg_scale > 1.0) and negative_context is not None
    neg = _prepare_contexts(model, guide, not uniform, video_state.positions, context, negative_context)
    cond = dict(denoise_mask=mask, clean_latent=clean)
    final = lambda i: _res2s_final(sig, i)      # noqa: E731

    def step(i):
        st = video_state.replace(latent=lat[None])
        sub = None if final(i) else modality_from_state(st, context, math.sqrt(sig[i] * sig[i + 1]), uniform=uniform)
        model.res2s_step_(neg, lat, modality_from_state(st, context, sig[i], uniform=uniform), sub, sig[i], sig[i + 1], cfg_scale, **cond)

    _run_steps(n, callback, use_hip_graph, lambda: model.capture_res2s_graph(neg, lat, sig, cfg_scale, **cond), model.replay_res2s_graph, step, final)
    return _with_latent(video_state, lat)


def res2s_av_denoise_loop(transformer, video_state: LatentState, audio_state: LatentState, sigmas, video_context: torch.Tensor,
                          audio_context: torch.Tensor, negative_video_context: Optional[torch.Tensor],
                          negative_audio_context: Optional[torch.Tensor], cfg_scale: float, audio_cfg_scale: float, callback=None,
                          use_hip_graph: bool = True) -> Tuple[LatentState, LatentState]:
    """The HQ pipeline's res_2s loop over BOTH modalities of an AudioVideo model (reference pipelines/ti2vid_hq.py:153-319): every step is ONE C
    call -- two pairs of AudioVideo evaluations, the midpoint and the combine kernel over both latents in one launch each
    (LTXModel.res2s_step_av_).  There is no captured form of this loop: use_hip_graph is accepted for the signature the other loops share,
    changes nothing and is answered with the usual one-time note.  The video is guided by
    cfg_scale and the audio by audio_cfg_scale, both as uncond + s * (cond - uncond), under the reference's condition
    (cfg_scale > 1 or audio_cfg_scale > 1) and negative_video_context is not None.  A missing negative audio context falls back to the
    negative video context (reference :303) where the two modalities' contexts have the same width; otherwise that is a ValueError.  Sigma
    handling, step count, final-step break and the fp32-held latents are res2s_denoise_loop's.  Each modality takes the uniform or the
    per-token form by its own mask.  `transformer` is an X0Model over an AudioVideo model.  Returns (video_state, audio_state)."""
    model = transformer.velocity_model
    if not model.is_av or audio_state is None:
        raise ValueError("res2s_av_denoise_loop requires an audio-video (AV) model and an audio state")
    if audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    n, sig = _res2s_sigmas(sigmas)
    guide = (cfg_scale > 1.0 or audio_cfg_scale > 1.0) and negative_video_context is not None
    if guide and negative_audio_context is None:
        if negative_video_context.shape[-1] != audio_context.shape[-1]:
            raise ValueError(f"negative_audio_context is missing and the negative video context (width {negative_video_context.shape[-1]}) cannot "
                             f"stand in for it: the audio context has width {audio_context.shape[-1]}")
        negative_audio_context = negative_video_context
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=False)
    _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
    neg = _prepare_contexts(model, guide, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                            audio_state.positions, audio_context, negative_audio_context)
    cond = dict(denoise_mask=mask, clean_latent=clean, audio_denoise_mask=amask, audio_clean_latent=aclean)
    final = lambda i: _res2s_final(sig, i)      # noqa: E731
    if use_hip_graph:
        _note_eager_once("the joint audio+video res_2s loop has no captured form")

    def step(i):
        st, ast = video_state.replace(latent=lat[None]), audio_state.replace(latent=alat[None])
        sub = asub = None
        if not final(i):
            s_sub = math.sqrt(sig[i] * sig[i + 1])
            sub = modality_from_state(st, video_context, s_sub, uniform=uniform)
            asub = audio_modality_from_state(ast, audio_context, s_sub, uniform=a_uniform)
        model.res2s_step_av_(neg, lat, alat, modality_from_state(st, video_context, sig[i], uniform=uniform),
                             audio_modality_from_state(ast, audio_context, sig[i], uniform=a_uniform), sub, asub, sig[i], sig[i + 1], cfg_scale,
                             audio_cfg_scale, **cond)

    _run_steps(n, callback, use_hip_graph, None, None, step, final)
    return _with_latent(video_state, lat), _with_latent(audio_state, alat)


def _ancestral_parts(x, vel_cond, vel_uncond, ts, cfg_scale, mask, clean, sigma, sigma_up, sigma_down, noise):
    """One modality's Euler-ancestral step from separate ops, the statements ltx2_ancestral_euler_step fuses, on fp32 (N, C): under guidance
    every fp32 torch op on its own; without, x0_from_velocity and euler_step (the plain step's kernels) with the blend in torch."""
    import numpy as np
    from .. import kernels as K
    m = None if mask is None else mask.reshape(-1, 1)
    blend = lambda d: d if m is None else d * m + clean * (1 - m)      # noqa: E731
    if vel_uncond is None:
        stepped = K.euler_step(x, blend(K.x0_from_velocity(x, vel_cond, ts)), sigma, sigma_down)
    else:
        t = ts.reshape(-1, 1) if ts.numel() > 1 else ts.reshape(1, 1)
        a, b = x - t * vel_cond, x - t * vel_uncond
        d = blend(a + float(np.float32(cfg_scale) - np.float32(1)) * (a - b))      # the kernel's fp32 scalars: cfg_scale - 1, 1/sigma, sigma_down - sigma
        inv, dt = float(np.float32(1) / np.float32(sigma)), float(np.float32(sigma_down) - np.float32(sigma))
        stepped = x + ((x - d) * inv) * dt
    if sigma_up == 0:
        return stepped
    scaled = noise.reshape(x.shape) * float(np.float32(sigma_up))
    return stepped + (scaled if m is None else scaled * m)


def ancestral_denoise_loop(transformer, video_state: LatentState, audio_state: Optional[LatentState], sigmas, video_context: torch.Tensor,
                           audio_context: Optional[torch.Tensor] = None, negative_video_context: Optional[torch.Tensor] = None,
                           negative_audio_context: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, audio_cfg_scale: float = 1.0,
                           eta: float = 1.0, seed: int = 0, callback=None, use_hip_graph: bool = True,
                           fused: bool = True) -> Tuple[LatentState, Optional[LatentState]]:
    """The Euler-ancestral sampler (the reference's EulerAncestralDiffusionStep, components/diffusion_steps.py:70-129, as its DistilledPipeline
    runs stage 1) without leaving the device: per step the Euler step to sigma_down, then sigma_up * N(0,1) on top, with (sigma_up, sigma_down) =
    _get_ancestral_step(sigma_i, sigma_{i+1}, eta) in double on the host.  The noise is made INSIDE the step kernel: Philox4x32-10 under (seed,
    step, modality, element index), the video latent from stream 0 and the audio latent from stream 1, scaled by the denoise mask so that
    conditioned tokens stay clean (the reference would add noise to them too; with an all-ones mask the arithmetic is the reference's).
    Video alone (audio_state None; an AudioVideo model through its video twin) or both latents of an AudioVideo model.  Classifier-free guidance
    (CFGGuider's arithmetic, as guided_denoise_loop / joint_guided_denoise_loop) when a scale is not 1 and the negative context(s) are given.
    fused=True: every step is ONE C call (LTXModel.ancestral_step_) and with no callback and fewer than 64 steps the loop is one captured graph
    that reads the seed from device memory.  fused=False: the comparison form -- the same forwards, then separate ops and
    kernels.philox_normal; it gives the same bits.  eta = 0 gives the Euler loops' bits (joint_denoise_loop; under guidance
    guided_denoise_loop / joint_guided_denoise_loop).  `transformer` is an X0Model.  Returns (video_state, audio_state or None)."""
    from .. import kernels as K
    from ..components import EulerAncestralDiffusionStep
    model = transformer.velocity_model
    joint = audio_state is not None
    if joint and not model.is_av:
        raise ValueError("an audio state needs an audio-video (AV) model")
    if joint and audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    if eta < 0:
        raise ValueError(f"eta={eta} must be >= 0")
    guided = (cfg_scale != 1.0 or (joint and audio_cfg_scale != 1.0)) and negative_video_context is not None and (not joint or negative_audio_context is not None)
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    steps = [EulerAncestralDiffusionStep._get_ancestral_step(sig[i], sig[i + 1], eta) for i in range(n)]
    up, down = [s[0] for s in steps], [s[1] for s in steps]
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=not joint)
    a_uniform, alat, amask, aclean = True, None, None, None
    if joint:
        _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
    seed_dev = K.seed_word(seed, lat.device)
    neg = _prepare_contexts(model, guided, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                            audio_state.positions if joint else None, audio_context if joint else None, negative_audio_context if joint else None)
    cond = dict(denoise_mask=mask, clean_latent=clean)
    if joint:
        cond.update(audio_denoise_mask=amask, audio_clean_latent=aclean)

    def modalities(vc, ac, s):
        vm = modality_from_state(video_state.replace(latent=lat[None]), vc, s, uniform=uniform)
        return (vm, audio_modality_from_state(audio_state.replace(latent=alat[None]), ac, s, uniform=a_uniform)) if joint else (vm,)

    if fused:
        def step(i):
            mods = modalities(video_context, audio_context, sig[i])
            model.ancestral_step_(neg, lat, mods[0], sig[i], up[i], down[i], seed_dev, i, cfg_scale, audio_latent=alat,
                                  audio=mods[1] if joint else None, audio_cfg_scale=audio_cfg_scale, **cond)

        _run_steps(n, callback, use_hip_graph, lambda: model.capture_ancestral_graph(neg, lat, sig, up, down, seed_dev, cfg_scale, audio_latent=alat,
                                                                                      audio_cfg_scale=audio_cfg_scale, **cond),
                   model.replay_ancestral_graph, step)
    else:
        def velocities(m, mods):
            out = m(*mods)
            return [v[0] for v in (out if isinstance(out, tuple) else (out,))][:len(mods)]

        segments = [(lat, cfg_scale, mask, clean, 0)] + ([(alat, audio_cfg_scale, amask, aclean, 1)] if joint else [])
        for i in range(n):
            mods = modalities(video_context, audio_context, sig[i])
            vc = velocities(model, mods)
            vu = velocities(neg, modalities(negative_video_context, negative_audio_context, sig[i])) if guided else [None, None]
            for k, (x, scale, mk, cl, stream_id) in enumerate(segments):
                noise = K.philox_normal(x.numel(), seed_dev, i, stream_id) if up[i] != 0 else None
                x.copy_(_ancestral_parts(x, vc[k], vu[k], mods[k].timesteps.reshape(-1).float(), scale, mk, cl, sig[i], up[i], down[i], noise))
            if callback:
                callback(i + 1, n)
    return _with_latent(video_state, lat), (_with_latent(audio_state, alat) if joint else None)


def heun_device_form(video_guider, audio_guider=None) -> bool:
    """Whether the Heun / GE loops can run their device form under these guiders: each a plain CFGGuider, None or not enabled."""
    from ..components.guiders import CFGGuider
    return all(g is None or not g.enabled() or type(g) is CFGGuider for g in (video_guider, audio_guider))


def _heun_ge_loop(heun: bool, transformer, video_state: LatentState, audio_state: Optional[LatentState], sigmas, video_context: torch.Tensor,
                  audio_context: Optional[torch.Tensor], negative_video_context: Optional[torch.Tensor], negative_audio_context: Optional[torch.Tensor],
                  video_guider, audio_guider, ge_gamma: float, callback, use_hip_graph: bool, fused: bool):
    """heun_denoise_loop (heun=True) and ge_denoise_loop (heun=False)."""
    from ..components import EulerDiffusionStep, HeunDiffusionStep
    model = transformer.velocity_model
    joint = audio_state is not None
    if joint and not model.is_av:
        raise ValueError("an audio state needs an audio-video (AV) model")
    if joint and audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    if ge_gamma < 0 or (not heun and not ge_gamma > 0):
        raise ValueError(f"ge_gamma={ge_gamma}: the GE loop needs ge_gamma > 0, the Heun loop ge_gamma >= 0")
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    guiders = [video_guider] + ([audio_guider] if joint else [])
    need_cfg = any(g is not None and g.enabled() for g in guiders)
    if need_cfg and (negative_video_context is None or (joint and negative_audio_context is None)):
        raise ValueError("guidance needs the negative prompt's encoding(s)")
    for g in guiders:
        reset_guider(g)
    if fused:
        if not heun_device_form(*guiders):
            raise ValueError("the device form runs under a plain CFGGuider (or none) per modality; call with fused=False for any other guider")
        if joint and not heun:
            raise ValueError("Euler + GE has no device form on the joint audio+video loop; call with fused=False")
        scale = [g.scale if (g is not None and g.enabled()) else 1.0 for g in guiders]
        model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=not joint)
        cond = dict(denoise_mask=mask, clean_latent=clean)
        modality = lambda st, ctx, s, u: None if s == 0 else modality_from_state(st, ctx, s, uniform=u)       # noqa: E731  (sigma_next == 0: no second evaluation)
        if not joint:
            neg = _prepare_contexts(model, need_cfg, not uniform, video_state.positions, video_context, negative_video_context)

            def step(i):
                st = video_state.replace(latent=lat[None])
                vm = modality_from_state(st, video_context, sig[i], uniform=uniform)
                if heun:
                    model.heun_step_(neg, lat, vm, modality(st, video_context, sig[i + 1], uniform), sig[i], sig[i + 1], scale[0], ge_gamma, i == 0, **cond)
                else:
                    model.ge_step_(neg, lat, vm, sig[i], sig[i + 1], scale[0], ge_gamma, i == 0, **cond)

            capture = (lambda: model.capture_heun_graph(neg, lat, sig, scale[0], ge_gamma, **cond)) if heun else None
            _run_steps(n, callback, use_hip_graph, capture, model.replay_heun_graph if heun else None, step)
            return _with_latent(video_state, lat), None
        _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
        neg = _prepare_contexts(model, need_cfg, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                                audio_state.positions, audio_context, negative_audio_context)
        cond.update(audio_denoise_mask=amask, audio_clean_latent=aclean)
        if use_hip_graph:
            _note_eager_once("the joint audio+video Heun loop has no captured form")

        def step(i):
            st, ast = video_state.replace(latent=lat[None]), audio_state.replace(latent=alat[None])
            model.heun_step_av_(neg, lat, alat, modality_from_state(st, video_context, sig[i], uniform=uniform),
                                audio_modality_from_state(ast, audio_context, sig[i], uniform=a_uniform), modality(st, video_context, sig[i + 1], uniform),
                                modality(ast, audio_context, sig[i + 1], a_uniform), sig[i], sig[i + 1], scale[0], scale[1], ge_gamma, i == 0, **cond)

        _run_steps(n, callback, use_hip_graph, None, None, step)
        return _with_latent(video_state, lat), _with_latent(audio_state, alat)

    # the eager form: the reference's statements one by one
    if model.is_av and not joint:
        model = model._video_twin()
    pos_model, neg_model = transformer, (X0Model(model.clone_sharing_weights()) if need_cfg else None)
    states = [video_state] + ([audio_state] if joint else [])
    contexts, neg_contexts = [video_context, audio_context], [negative_video_context, negative_audio_context]
    unif = [bool((st.denoise_mask == 1).all()) for st in states]
    euler, heun_stepper = EulerDiffusionStep(), HeunDiffusionStep()
    prev_velocity = None

    def denoised(sts, s):
        """the guided x0 of every state at sigma s, before post_process_latent"""
        mods = [modality_from_state(st, c, s, uniform=u) for st, c, u in zip(sts, contexts, unif)]
        out = pos_model(*mods)
        out = list(out) if isinstance(out, tuple) else [out]
        if need_cfg:
            nout = neg_model(*[modality_from_state(st, c, s, uniform=u) for st, c, u in zip(sts, neg_contexts, unif)])
            nout = list(nout) if isinstance(nout, tuple) else [nout]
            out = [g.guide(p, q) if g is not None else p for g, p, q in zip(guiders, out, nout)]
        return out[:len(sts)]

    blend = lambda ds: [post_process_latent(d, st.denoise_mask, st.clean_latent) for d, st in zip(ds, states)]       # noqa: E731
    for i in range(n):
        s, sn = sig[i], sig[i + 1]
        d = denoised(states, s)
        if ge_gamma > 0 and s > 0:
            cur = (states[0].latent - d[0]) / s
            if prev_velocity is not None:
                d[0] = states[0].latent - (ge_gamma * (cur - prev_velocity) + prev_velocity) * s
            prev_velocity = cur
        d = blend(d)
        if not heun:
            states = [st.replace(latent=euler.step(sample=st.latent, denoised_sample=x0, sigmas=sig, step_index=i)) for st, x0 in zip(states, d)]
        elif sn == 0:
            states = [st.replace(latent=x0) for st, x0 in zip(states, d)]
        else:
            predicted = [st.replace(latent=heun_stepper.step(sample=st.latent, denoised_sample=x0, sigmas=sig, step_index=i)) for st, x0 in zip(states, d)]
            d2 = blend(denoised(predicted, sn))
            states = [st.replace(latent=heun_stepper.step(sample=st.latent, denoised_sample=x0, sigmas=sig, step_index=i, denoised_at_predicted=x2))
                      for st, x0, x2 in zip(states, d, d2)]
        if callback:
            callback(i + 1, n)
    return states[0], (states[1] if joint else None)


def heun_denoise_loop(transformer, video_state: LatentState, audio_state: Optional[LatentState], sigmas, video_context: torch.Tensor,
                      audio_context: Optional[torch.Tensor], negative_video_context: Optional[torch.Tensor],
                      negative_audio_context: Optional[torch.Tensor], video_guider, audio_guider=None, ge_gamma: float = 0.0, callback=None,
                      use_hip_graph: bool = True, fused: bool = True) -> Tuple[LatentState, Optional[LatentState]]:
    """OneStagePipeline's Heun loops (the reference's _denoise_loop_heun and _denoise_loop_heun_av, pipelines/one_stage.py:334-464, 570-729): per
    step the guided x0 at sigma, on the video the GE velocity correction when ge_gamma > 0, post_process_latent, the Euler predictor, and unless
    sigma_next == 0 (then latent = x0) a second guided evaluation of the predicted latent at sigma_next and HeunDiffusionStep's corrector.
    audio_state None: the video-only loop (an AudioVideo model through its video twin); otherwise both latents are stepped, each under its own
    guider, GE on the video alone.  The negative prompt is evaluated when either guider is enabled().
    fused=True: each guider is a plain CFGGuider, None or not enabled (heun_device_form).  Every step is ONE C call (LTXModel.heun_step_ /
    heun_step_av_: the evaluations, the predictor and the corrector kernel), the latents held in fp32 across the loop; the video-only loop with
    no callback and fewer than 64 steps is one captured graph.  The joint loop has no captured form.
    fused=False: the reference's statements one by one, for any guider: X0Model calls, the torch guiders, post_process_latent and
    HeunDiffusionStep.  `transformer` is an X0Model.  Returns (video_state, audio_state or None)."""
    return _heun_ge_loop(True, transformer, video_state, audio_state, sigmas, video_context, audio_context, negative_video_context, negative_audio_context,
                         video_guider, audio_guider, ge_gamma, callback, use_hip_graph, fused)


def ge_denoise_loop(transformer, video_state: LatentState, audio_state: Optional[LatentState], sigmas, video_context: torch.Tensor,
                    audio_context: Optional[torch.Tensor], negative_video_context: Optional[torch.Tensor],
                    negative_audio_context: Optional[torch.Tensor], video_guider, audio_guider=None, ge_gamma: float = 0.0, callback=None,
                    use_hip_graph: bool = True, fused: bool = True) -> Tuple[LatentState, Optional[LatentState]]:
    """OneStagePipeline's Euler loops with the GE velocity correction (ge_gamma > 0; the reference's _denoise_loop_cfg and _denoise_loop_cfg_av,
    pipelines/one_stage.py:224-330, 466-568): from the second step on the video's guided x0 is rebuilt from ge_gamma * (v - v_prev) + v_prev.
    fused=True: the video-only loop under a plain CFGGuider (or none), every step ONE C call (LTXModel.ge_step_); there is no captured form
    (use_hip_graph changes nothing) and no device form of the joint loop.  fused=False: the reference's statements one by one, for any guider
    and for the joint loop.  Arguments and result as heun_denoise_loop."""
    return _heun_ge_loop(False, transformer, video_state, audio_state, sigmas, video_context, audio_context, negative_video_context, negative_audio_context,
                         video_guider, audio_guider, ge_gamma, callback, use_hip_graph, fused)


def multimodal_denoise_loop(transformer, video_state: LatentState, audio_state: LatentState, sigmas, video_context: torch.Tensor,
                            audio_context: torch.Tensor, negative_video_context: Optional[torch.Tensor],
                            negative_audio_context: Optional[torch.Tensor], video_guider, audio_guider, callback=None,
                            fused: bool = True) -> Tuple[LatentState, LatentState]:
    """Stage 1 of the two-stage pipeline on the AudioVideo model (the reference's _denoise_loop_cfg_av, pipelines/two_stage.py:314-401): per step
    up to four evaluations of both modalities -- the positive prompt; the negative prompt when either MultiModalGuider
    do_unconditional_generation(); the positive prompt with the self-attentions of the guiders' stg_blocks skipped when either
    do_perturbed_generation() (the reference's loop never asks for it; its guider has the term); the positive prompt with every cross-modal
    attention skipped when either do_isolated_modality_generation() -- then MultiModalGuider.calculate, post_process_latent and the Euler
    step on both latents.  A pass that ran contributes its term to BOTH modalities, whatever their scales, as the reference hands both
    guiders the same predictions.
    fused=True: every step is ONE C call (LTXModel.mm_guided_step_av_): the evaluations, then one kernel over both latents (with
    rescale_scale != 0, a sums and a step kernel per modality).  There is no captured form of this loop.  The latents are held in fp32
    across the loop, as the other device-resident loops hold them.
    fused=False: the eager composition, the reference's statements one by one: X0Model calls through the C entries, calculate,
    post_process_latent and EulerDiffusionStep.
    skip_step is not read (the reference's loop does not call should_skip_step).  `transformer` is an X0Model over an AudioVideo model.
    Returns (video_state, audio_state)."""
    from ..components import EulerDiffusionStep
    model = transformer.velocity_model
    if not model.is_av or audio_state is None:
        raise ValueError("multimodal_denoise_loop requires an audio-video (AV) model and an audio state")
    if audio_context is None:
        raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
    sig = [float(s) for s in sigmas]
    n = len(sig) - 1
    guiders = (video_guider, audio_guider)
    need_u = any(g.do_unconditional_generation() for g in guiders)
    need_p = any(g.do_perturbed_generation() for g in guiders)
    need_m = any(g.do_isolated_modality_generation() for g in guiders)
    if need_u and (negative_video_context is None or negative_audio_context is None):
        raise ValueError("guidance needs the negative prompt's encoding(s)")
    if need_p:
        blocks = [g.params.stg_blocks for g in guiders]
        if all(b is not None and len(b) == 0 for b in blocks):
            raise ValueError("stg_scale != 0 needs stg_blocks on at least one guider (None: every block)")
        for k, b in enumerate(blocks):
            model.set_stg_blocks(b, modality=k)
    if not fused:
        from ..components.perturbations import BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType as PT
        stepper = EulerDiffusionStep()
        neg = X0Model(model.clone_sharing_weights()) if need_u else None
        ptb = None
        if need_p:
            kinds = (PT.SKIP_VIDEO_SELF_ATTN, PT.SKIP_AUDIO_SELF_ATTN)
            ptb = BatchedPerturbationConfig([PerturbationConfig([Perturbation(type=kinds[k], blocks=g.params.stg_blocks) for k, g in enumerate(guiders)
                                                                 if g.params.stg_blocks is None or len(g.params.stg_blocks)])])
        unif = [bool((st.denoise_mask == 1).all()) for st in (video_state, audio_state)]
        for i in range(n):
            vm = modality_from_state(video_state, video_context, sig[i], uniform=unif[0])
            am = audio_modality_from_state(audio_state, audio_context, sig[i], uniform=unif[1])
            cond = transformer(vm, am)
            unc = ptd = mod = (0.0, 0.0)
            if need_u:
                unc = neg(modality_from_state(video_state, negative_video_context, sig[i], uniform=unif[0]),
                          audio_modality_from_state(audio_state, negative_audio_context, sig[i], uniform=unif[1]))
            if need_p:
                ptd = transformer(vm, am, perturbations=ptb)
            if need_m:
                mod = transformer.forward_isolated(vm, am)
            states = []
            for k, st in enumerate((video_state, audio_state)):
                d = post_process_latent(guiders[k].calculate(cond[k], unc[k], ptd[k], mod[k]), st.denoise_mask, st.clean_latent)
                states.append(st.replace(latent=stepper.step(sample=st.latent, denoised_sample=d, sigmas=sig, step_index=i)))
            video_state, audio_state = states
            if callback:
                callback(i + 1, n)
        return video_state, audio_state
    model, uniform, lat, mask, clean = _video_loop_inputs(model, video_state, video_only=False)
    _, a_uniform, alat, amask, aclean = _video_loop_inputs(model, audio_state, video_only=False)
    neg = _prepare_contexts(model, need_u, not (uniform and a_uniform), video_state.positions, video_context, negative_video_context,
                            audio_state.positions, audio_context, negative_audio_context)
    scratch = lambda: (lat.new_empty(lat.shape[0], model.out_channels), alat.new_empty(alat.shape[0], model.AUDIO_OUT_CHANNELS))      # noqa: E731
    cond = dict(isolated=scratch() if need_m else None, perturbed=scratch() if need_p else None, denoise_mask=mask, clean_latent=clean,
                audio_denoise_mask=amask, audio_clean_latent=aclean)

    def step(i):
        st, ast = video_state.replace(latent=lat[None]), audio_state.replace(latent=alat[None])
        model.mm_guided_step_av_(neg, lat, alat, modality_from_state(st, video_context, sig[i], uniform=uniform),
                                 audio_modality_from_state(ast, audio_context, sig[i], uniform=a_uniform), sig[i], sig[i + 1], video_guider.params,
                                 audio_guider.params, **cond)

    _run_steps(n, callback, False, None, None, step)
    return _with_latent(video_state, lat), _with_latent(audio_state, alat)
