"""Retake on MI355X: keep a clip, regenerate one time window of it from a prompt.

Mirrors reference LTX_2_MLX/pipelines/retake.py:47-64 (RetakeConfig), :67-138 (get_video_metadata, load_video_frames), :141-196
(TemporalRegionMask) and :199-408 (RetakePipeline).  The whole source clip is encoded by the VAE encoder; the tokens of the latent frames the
window touches get denoise_mask 1 and are noised, all others keep mask 0 and their encoded value, and the conditioned sampling loops
(timesteps = mask * sigma, x0 blended with the clean latent) regenerate the first and carry the second through unchanged, bit for bit.
  distilled: the 8 steps of the distilled sigma table without guidance (pipelines.common.joint_denoise_loop);
  otherwise: LTX2Scheduler over num_inference_steps with CFGGuider(cfg_scale) (pipelines.common.guided_denoise_loop).
Both are one captured graph when there is no callback.  The source stays on the device: uint8 frames -> kernels.frames_to_patches ->
SimpleVideoEncoder.encode_patches -> kernels.retake_prepare (patchify, mask and noise blend in one pass); with composite_source the
frames outside the window are put back from the source by kernels.retake_composite.  The reference reads the file with ffmpeg and resizes
nothing; load_control_frames reads arrays, image directories and (through an ffmpeg binary) video files, at the source's own size.
Retake with sound (MI355X addition; the reference's audio state is always None, its _denoise_loop :234-291 is written for one): given the clip's
sound track (audio_path= / audio_latent=) on an AudioVideo model, the track is encoded by the audio VAE encoder, kernels.retake_prepare_audio
builds its state with the mask on the audio tokens whose seconds meet the window, and BOTH latents run through the joint loops
(joint_denoise_loop distilled, joint_guided_denoise_loop otherwise: one C call per step or one captured graph); decoded, the waveform outside the
window can be put back from the source by kernels.retake_composite_audio.  Without an audio argument nothing here changes.
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
from dataclasses import dataclass
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch

from .. import kernels as K
from ..components import DISTILLED_SIGMA_VALUES, CFGGuider, EulerDiffusionStep, LTX2Scheduler, VideoLatentPatchifier
from ..components.patchifiers import AudioPatchifier
from ..conditioning.tools import AudioLatentTools, VideoLatentTools
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from ..types import AudioLatentShape, LatentState, VideoLatentShape, VideoPixelShape
from .common import (as_x0model, decode_video, final_latent, guided_denoise_loop, joint_denoise_loop, joint_guided_denoise_loop,
                     projected_denoise_loop, stage_callback)
from .ic_lora import IMAGE_SUFFIXES, load_control_frames, load_control_signal_tensor


@dataclass
class RetakeConfig:
    """Configuration of the retake pipeline (reference :47-64).  Without a sound track (no audio_path= / audio_latent=): regenerate_audio is
    kept for the signature and has no effect, as in the reference, whose audio state is always None, and regenerate_video=False leaves the
    mask all ones, as create_initial_state makes it: the whole clip is regenerated.
    With a sound track the two flags mean what they say, which differs on purpose from that quirk: regenerate_video=False FREEZES the whole
    picture (mask 0: the window is re-dubbed), regenerate_audio=False freezes the whole track, both False is a ValueError."""
    start_time: float               # seconds, inclusive
    end_time: float                 # seconds, exclusive
    regenerate_video: bool = True
    regenerate_audio: bool = True
    distilled: bool = False
    num_inference_steps: int = 40
    cfg_scale: float = 3.0
    seed: int = 42
    tiling_config: Optional[TilingConfig] = None
    dtype: torch.dtype = torch.float32
    # MI355X additions
    fps: Optional[float] = None     # the source's frame rate: required for arrays and image directories, overrides ffprobe's for a video file
    use_hip_graph: bool = True      # replay the loop from one captured graph (no callback; the guided loop: fewer than 64 steps)
    composite_source: bool = False  # put the source's own frames back outside the window (kernels.retake_composite)
    composite_ramp: int = 4         # frames of linear fade on each side, OUTSIDE the window
    audio_cfg_scale: Optional[float] = None     # guidance scale of the audio latent; None: cfg_scale, the reference's single scale
    composite_source_audio: bool = False        # put the source track's own samples back outside the window (kernels.retake_composite_audio)
    audio_composite_ramp_ms: float = 20.0       # milliseconds of linear fade on each side, OUTSIDE the window

    def __post_init__(self):
        if self.start_time >= self.end_time:
            raise ValueError(f"start_time ({self.start_time}) must be < end_time ({self.end_time})")
        if self.composite_ramp < 0:
            raise ValueError(f"composite_ramp ({self.composite_ramp}) must be >= 0")
        if self.audio_composite_ramp_ms < 0:
            raise ValueError(f"audio_composite_ramp_ms ({self.audio_composite_ramp_ms}) must be >= 0")


def _is_array_or_dir(path: str) -> bool:
    return os.path.isdir(path) or path.lower().endswith((".npy", ".npz"))


def get_video_metadata(video_path: str, fps: Optional[float] = None) -> Tuple[float, int, int, int]:
    """-> (fps, num_frames, width, height) of the source (reference :67-94).  A video file is asked through ffprobe, as in the reference;
    an array (.npy / .npz) or a directory of image frames carries no frame rate, so `fps` is required for those (MI355X addition; given
    for a video file it replaces ffprobe's)."""
    if not os.path.exists(video_path):
        raise FileNotFoundError(f"Source video not found: {video_path}")
    if _is_array_or_dir(video_path):
        if fps is None:
            raise ValueError(f"{video_path} is an array or an image directory and carries no frame rate: set RetakeConfig.fps")
        if os.path.isdir(video_path):
            from PIL import Image
            names = sorted(n for n in os.listdir(video_path) if n.lower().endswith(IMAGE_SUFFIXES))
            if not names:
                raise ValueError(f"Could not read any frames from {video_path}: no image files ({', '.join(IMAGE_SUFFIXES)})")
            with Image.open(os.path.join(video_path, names[0])) as im:
                w, h = im.size
            return float(fps), len(names), w, h
        if video_path.lower().endswith(".npy"):
            shape = np.load(video_path, mmap_mode="r").shape
        else:
            with np.load(video_path) as z:
                shape = z[z.files[0]].shape
        if len(shape) not in (3, 4):
            raise ValueError(f"{video_path}: frames must be (F, H, W, 3) or (F, H, W), got {tuple(shape)}")
        return float(fps), int(shape[0]), int(shape[2]), int(shape[1])
    if shutil.which("ffprobe") is None:
        raise RuntimeError(f"reading the video file {video_path} needs the ffprobe and ffmpeg binaries, and ffprobe was not found: pass the "
                           "source as a .npy / .npz array of uint8 frames (F, H, W, 3) or as a directory of image frames, with RetakeConfig.fps")
    r = subprocess.run(["ffprobe", "-v", "quiet", "-print_format", "json", "-show_streams", "-show_format", video_path], capture_output=True,
                       text=True)
    data = json.loads(r.stdout or "{}")
    for stream in data.get("streams", []):
        if stream.get("codec_type") == "video":
            parts = stream.get("r_frame_rate", "24/1").split("/")
            rate = float(parts[0]) / float(parts[1]) if len(parts) == 2 else float(parts[0])
            n = int(stream.get("nb_frames", 0) or 0)
            if n == 0:
                n = int(float(data.get("format", {}).get("duration", 0)) * rate)
            return (float(fps) if fps is not None else rate), n, int(stream["width"]), int(stream["height"])
    raise ValueError(f"No video stream found in {video_path}")


def load_video_frames(video_path: str, height: int, width: int, num_frames: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Source -> (1, 3, F, H, W) in [-1, 1] on the host (reference :97-138): the API-faithful form.  The pipeline itself keeps the uint8
    frames of load_control_frames and normalises them on the device (kernels.frames_to_patches)."""
    return load_control_signal_tensor(load_control_frames(video_path, height, width, num_frames), dtype)


class TemporalRegionMask:
    """denoise_mask = 1 inside a time range, 0 outside (reference :141-196): only the masked tokens are regenerated, the others keep the
    clean latent.  start_time inclusive, end_time exclusive, in seconds; fps converts them to frames."""

    def __init__(self, start_time: float, end_time: float, fps: float):
        self.start_time = start_time
        self.end_time = end_time
        self.fps = fps

    def frame_window(self, latent_frames: int) -> Tuple[int, int]:
        """The latent frames [f0, f1) the range touches, by the reference's arithmetic (:168-173); f0 >= f1 when it touches none."""
        start_pixel_frame = int(self.start_time * self.fps)
        end_pixel_frame = int(self.end_time * self.fps)
        return max(0, (start_pixel_frame - 1) // 8), min(latent_frames, (end_pixel_frame - 1) // 8 + 1)

    def pixel_window(self, latent_frames: int, pixel_frames: int) -> Tuple[int, int]:
        """The pixel frames [p0, p1) those latent frames cover: latent frame 0 is pixel frame 0, latent frame k >= 1 the pixel frames
        8(k-1)+1 .. 8k."""
        f0, f1 = self.frame_window(latent_frames)
        if f0 >= f1:
            return 0, 0
        first = lambda k: 0 if k == 0 else 8 * (k - 1) + 1
        return min(first(f0), pixel_frames), min(first(f1), pixel_frames)

    def apply_to(self, latent_state: LatentState, latent_tools: VideoLatentTools) -> LatentState:
        """The state with this mask, in plain torch: the yardstick of kernels.retake_prepare's mask."""
        shape = latent_tools.target_shape
        f0, f1 = self.frame_window(shape.frames)
        per_frame = shape.height * shape.width
        old = latent_state.denoise_mask
        mask = torch.zeros((1, shape.frames * per_frame, 1), dtype=old.dtype, device=old.device)
        if f0 < f1:
            mask[:, f0 * per_frame: f1 * per_frame] = 1
        return latent_state.replace(denoise_mask=mask)


def end_of_clip(num_frames: int, fps: float) -> float:
    """An end_time that reaches the clip's last frame: half a frame past it.  num_frames / fps itself does not always do: the window's end is
    int(end_time * fps) frames, and the float round trip n / fps * fps truncates to n - 1 for, e.g., 57 frames at 25 fps or 97 at 23.976,
    which would leave the last latent frame out without a word."""
    return (num_frames + 0.5) / fps


def audio_token_window(t0: float, t1: float, tokens: int, sample_rate: int = 16000, hop_length: int = 160, downsample: int = 4) -> Tuple[int, int]:
    """The contiguous audio tokens [a0, a1) whose [start, end) seconds (AudioPatchifier.get_patch_grid_bounds: causal, token k spans
    max(4k - 3, 0) .. 4k + 1 mel frames of hop_length / sample_rate seconds each) intersect [t0, t1), on the host in double precision.
    A token that only touches the window with its end (end == t0) or its start (start == t1) is outside.  (0, 0) when none is touched."""
    sec = lambda k: max(downsample * k + 1 - downsample, 0) * hop_length / sample_rate      # noqa: E731
    hit = [k for k in range(tokens) if sec(k) < t1 and sec(k + 1) > t0]
    return (hit[0], hit[-1] + 1) if hit else (0, 0)


def _snap(num_frames: int) -> int:
    return ((num_frames - 1) // 8) * 8 + 1


class RetakePipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder, video_decoder: Optional[SimpleVideoDecoder], audio_decoder=None,
                 vocoder=None, audio_encoder=None, audio_processor=None):
        """audio_decoder / vocoder turn the retaken audio latent into a waveform; audio_encoder (+ an AudioProcessor, built on demand;
        MI355X additions, as in create_a2vid_pipeline) encodes audio_path.  All four are unused without a sound track."""
        self.transformer, self.is_av_model = as_x0model(transformer)
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.audio_decoder = audio_decoder
        self.vocoder = vocoder
        self.audio_encoder = audio_encoder
        self.audio_processor = audio_processor
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.stepper = EulerDiffusionStep()
        # of the last call: the source on the device (uint8), its frame rate, the latent-frame and pixel-frame windows, the DiT tokens
        self.source_frames: Optional[torch.Tensor] = None
        self.fps: Optional[float] = None
        self.frame_window: Optional[Tuple[int, int]] = None
        self.pixel_window: Optional[Tuple[int, int]] = None
        self.token_count: int = 0
        # of the last call with a sound track: the audio tokens [a0, a1) regenerated, the same span in samples of the decoded waveform, the latent
        self.audio_window: Optional[Tuple[int, int]] = None
        self.audio_sample_window: Optional[Tuple[int, int]] = None
        self.audio_latent: Optional[torch.Tensor] = None

    def _load_source(self, video_path: Optional[str], frames, config: RetakeConfig) -> Tuple[torch.Tensor, float]:
        """-> (uint8 (8k+1, H, W, 3) on the encoder's device, fps).  The frame count is snapped down to 8k + 1 (reference :327); the size
        is the source's own and must be divisible by 32."""
        dev = self.video_encoder.device
        if frames is not None:
            if config.fps is None:
                raise ValueError("frames= carries no frame rate: set RetakeConfig.fps")
            x = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
            if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
                raise ValueError(f"frames must be uint8 (F, H, W, 3), got {x.dtype} {tuple(x.shape)}")
            fps, n, w, h = float(config.fps), int(x.shape[0]), int(x.shape[2]), int(x.shape[1])
        else:
            fps, n, w, h = get_video_metadata(video_path, config.fps)
        if n < 1:
            raise ValueError(f"Could not read any frames from {video_path if frames is None else 'frames='}")
        if h % 32 or w % 32:
            raise ValueError(f"Source resolution ({w}x{h}) must be divisible by 32 (the source is not resized)")
        n = _snap(n)
        if frames is None:
            x = torch.from_numpy(load_control_frames(video_path, h, w, n))
        return x[:n].to(dev).contiguous(), fps

    def _audio_state(self, audio_path, audio_latent, n_pix: int, fps: float, seconds: Tuple[float, float], config: RetakeConfig,
                     initial_audio_noise, gen, dev) -> Tuple[AudioLatentTools, LatentState]:
        """The sound track's state: the track encoded for the clip's snapped length (or audio_latent as given), the mask on the tokens whose
        seconds meet `seconds`, noise at scale 1 on those (kernels.retake_prepare_audio), the positions of AudioLatentTools."""
        shape = AudioLatentShape.from_video_pixel_shape(VideoPixelShape(batch=1, frames=n_pix, height=32, width=32, fps=fps))
        if audio_latent is None:
            if self.audio_encoder is None:
                raise ValueError("RetakePipeline needs an audio_encoder to encode audio_path (or pass audio_latent)")
            from .a2vid_two_stage import encode_audio_file
            print(f"  Loading audio: {audio_path}")
            audio_latent = encode_audio_file(audio_path, n_pix, fps, self.audio_encoder, self.audio_processor)[0]
        if tuple(audio_latent.shape) != shape.to_tuple():
            raise ValueError(f"audio_latent is {tuple(audio_latent.shape)}, the clip ({n_pix} frames at {fps:g} fps) needs {shape.to_tuple()}")
        encoded = audio_latent.to(dev, torch.float32).contiguous()
        patchifier = AudioPatchifier(patch_size=1)
        a0, a1 = (0, 0)
        if config.regenerate_audio:
            a0, a1 = audio_token_window(seconds[0], seconds[1], shape.frames, patchifier.sample_rate, patchifier.hop_length,
                                        patchifier.audio_latent_downsample_factor)
            if a0 >= a1:
                raise ValueError(f"the retake window {seconds[0]:.3f}s - {seconds[1]:.3f}s touches no audio token of the source track: it has "
                                 f"{shape.frames} latent frames, {n_pix / fps:.3f} s")
        width = shape.channels * shape.mel_bins
        if initial_audio_noise is None:
            initial_audio_noise = torch.randn((1, shape.frames, width), generator=gen(), device=dev, dtype=torch.float32)
        if tuple(initial_audio_noise.shape) != (1, shape.frames, width):
            raise ValueError(f"initial_audio_noise must be (1, {shape.frames}, {width}), got {tuple(initial_audio_noise.shape)}")
        clean, mask, latent = K.retake_prepare_audio(encoded, initial_audio_noise[0].to(dev, torch.float32).contiguous(), a0, a1, noise_scale=1.0)
        tools = AudioLatentTools(patchifier=patchifier, target_shape=shape)
        positions = tools.create_initial_state(dtype=torch.float32, device=dev).positions
        self.audio_window = (a0, a1)
        return tools, LatentState(latent=latent[None].to(config.dtype), denoise_mask=mask[None, :, None], positions=positions,
                                  clean_latent=clean[None].to(config.dtype))

    def denoise_latent(self, video_path: Optional[str], text_encoding: torch.Tensor, config: RetakeConfig,
                       negative_text_encoding: Optional[torch.Tensor] = None, callback: Optional[Callable[[str, int, int], None]] = None, *,
                       frames=None, initial_noise: Optional[torch.Tensor] = None, guider=None, audio_path: Optional[str] = None,
                       audio_latent: Optional[torch.Tensor] = None, initial_audio_noise: Optional[torch.Tensor] = None,
                       audio_encoding: Optional[torch.Tensor] = None, negative_audio_encoding: Optional[torch.Tensor] = None):
        """Up to the final latent (1, 128, F, H/32, W/32).  frames (keyword-only, MI355X addition): already loaded uint8 frames
        (F, H, W, 3) instead of a path.  initial_noise: a supplied N(0, 1) tensor (1, F*H*W/1024, 128) of the patchified shape, so results
        can be compared with a restatement.  guider (keyword-only): replaces CFGGuider(config.cfg_scale) in the guided (not distilled) mode
        and runs through projected_denoise_loop.
        audio_path / audio_latent (keyword-only): the clip's sound track, a file or its encoded latent (1, 8, T_a, 16); with one of them, on
        an AudioVideo model with audio_encoding, both modalities are retaken and the result is (video latent, audio latent (1, 8, T_a, 16)).
        The audio window is the tokens whose seconds meet those of the widened pixel window (p0 / fps, p1 / fps) when the video is
        regenerated, so picture and sound change over the same seconds, else (start_time, end_time).  Here regenerate_video=False freezes
        the whole picture and regenerate_audio=False the whole track (RetakeConfig).  initial_audio_noise: (1, T_a, 128)."""
        with_audio = audio_path is not None or audio_latent is not None
        if with_audio:
            if not self.is_av_model:
                raise ValueError("a retake with a sound track requires an audio-video (AV) model")
            if audio_encoding is None:
                raise ValueError("AudioVideo model: audio_encoding (the audio text context) is required")
            if guider is not None:
                raise NotImplementedError("a guider override on the joint audio+video retake loop is not built (plain classifier-free guidance only)")
            if not (config.regenerate_video or config.regenerate_audio):
                raise ValueError("regenerate_video and regenerate_audio are both False: nothing to retake")
        if self.video_encoder is None:
            raise ValueError("RetakePipeline needs a video_encoder")
        src, fps = self._load_source(video_path, frames, config)
        n_pix, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
        encoded = self.video_encoder.encode_patches(K.frames_to_patches(src))              # (1, 128, F, h/32, w/32) fp32
        shape = VideoLatentShape.from_pixel_shape(VideoPixelShape(batch=1, frames=n_pix, height=h, width=w, fps=fps), latent_channels=128)
        region = TemporalRegionMask(config.start_time, config.end_time, fps)
        if config.regenerate_video:
            f0, f1 = region.frame_window(shape.frames)
            if f0 >= f1:                                                                   # not 40 steps that change nothing
                raise ValueError(f"the retake window {config.start_time}s - {config.end_time}s touches no frame of the source: it has "
                                 f"{n_pix} frames at {fps:g} fps, {n_pix / fps:.3f} s")
            p0, p1 = region.pixel_window(shape.frames, n_pix)
        elif with_audio:
            (f0, f1), (p0, p1) = (0, 0), (0, 0)                                            # the picture is frozen: the window is re-dubbed
        else:
            (f0, f1), (p0, p1) = (0, shape.frames), (0, n_pix)
        dev = encoded.device
        tokens = shape.frames * shape.height * shape.width
        seeded = []

        def gen():                                                                         # the one generator of a call: video noise first, then audio
            if not seeded:
                seeded.append(torch.Generator(device=dev).manual_seed(config.seed))
            return seeded[0]

        if initial_noise is None:
            initial_noise = torch.randn((1, tokens, 128), generator=gen(), device=dev, dtype=torch.float32)
        if tuple(initial_noise.shape) != (1, tokens, 128):
            raise ValueError(f"initial_noise must be (1, {tokens}, 128), got {tuple(initial_noise.shape)}")
        clean, mask, latent = K.retake_prepare(encoded, initial_noise[0].to(dev, torch.float32).contiguous(), f0, f1, noise_scale=1.0)
        tools = VideoLatentTools(patchifier=self.patchifier, target_shape=shape, fps=fps)      # the source's own size and frame rate
        positions = tools.create_initial_state(dtype=torch.float32, device=dev).positions
        state = LatentState(latent=latent[None].to(config.dtype), denoise_mask=mask[None, :, None], positions=positions,
                            clean_latent=clean[None].to(config.dtype))
        self.source_frames, self.fps, self.frame_window, self.pixel_window, self.token_count = src, fps, (f0, f1), (p0, p1), tokens

        ctx = text_encoding.to(dev)
        cb = stage_callback(callback, "retake")
        if with_audio:
            seconds = (p0 / fps, p1 / fps) if config.regenerate_video else (float(config.start_time), float(config.end_time))
            atools, astate = self._audio_state(audio_path, audio_latent, n_pix, fps, seconds, config, initial_audio_noise, gen, dev)
            actx = audio_encoding.to(dev)
            if config.distilled:
                state, astate = joint_denoise_loop(self.transformer, True, state, astate, [float(s) for s in DISTILLED_SIGMA_VALUES], ctx, actx,
                                                   self.stepper, cb, config.use_hip_graph)
            else:
                sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
                # no negative prompt: zeros of the context's shape, for either modality (reference :387-388)
                nctx = torch.zeros_like(ctx) if negative_text_encoding is None else negative_text_encoding.to(dev)
                nactx = torch.zeros_like(actx) if negative_audio_encoding is None else negative_audio_encoding.to(dev)
                audio_cfg = config.cfg_scale if config.audio_cfg_scale is None else config.audio_cfg_scale
                state, astate = joint_guided_denoise_loop(self.transformer, state, astate, sigmas, ctx, actx, nctx, nactx, config.cfg_scale, audio_cfg,
                                                          self.stepper, cb, config.use_hip_graph)
            return final_latent(tools, state), final_latent(atools, astate)
        if config.distilled:
            state = joint_denoise_loop(self.transformer, self.is_av_model, state, None, [float(s) for s in DISTILLED_SIGMA_VALUES], ctx, None,
                                       self.stepper, cb, config.use_hip_graph)[0]
        else:
            sigmas = LTX2Scheduler().execute(steps=config.num_inference_steps)
            # no negative prompt: zeros of the context's shape (reference :387-388); cfg_scale <= 1: no negative pass (:261)
            nctx = torch.zeros_like(ctx) if negative_text_encoding is None else negative_text_encoding.to(dev)
            loop = guided_denoise_loop if guider is None else projected_denoise_loop
            guider = CFGGuider(config.cfg_scale if config.cfg_scale > 1.0 else 1.0) if guider is None else guider
            state = loop(self.transformer, state, sigmas, ctx, nctx, guider, self.stepper, cb, config.use_hip_graph)
        return final_latent(tools, state)

    def _decode_audio(self, audio_latent: torch.Tensor, audio_path: Optional[str], config: RetakeConfig) -> torch.Tensor:
        """The retaken audio latent -> waveform (2, S) fp32 at the vocoder's output_sample_rate; with composite_source_audio the source track,
        loaded at that rate and cut or right-padded with silence to S, is put back outside the audio window's samples."""
        from ..model.audio_vae import AudioProcessor, load_audio_file
        waveform = self.vocoder(self.audio_decoder(audio_latent))[0].contiguous()
        rate, samples = int(self.vocoder.output_sample_rate), int(waveform.shape[1])
        a0, a1 = self.audio_window
        p = AudioPatchifier(patch_size=1)
        sec = lambda k: max(p.audio_latent_downsample_factor * k + 1 - p.audio_latent_downsample_factor, 0) * p.hop_length / p.sample_rate      # noqa: E731
        self.audio_sample_window = (min(samples, int(round(sec(a0) * rate))), min(samples, int(round(sec(a1) * rate)))) if a0 < a1 else (0, 0)
        if not config.composite_source_audio:
            return waveform
        if audio_path is None:
            raise ValueError("composite_source_audio needs the source track itself: pass audio_path (audio_latent alone carries no waveform)")
        source, _ = load_audio_file(audio_path, rate)
        source = AudioProcessor.fit_waveform(np.asarray(source, dtype=np.float32)[:2], samples)
        if source.shape[0] < waveform.shape[0]:                                            # mono: the one channel on both
            source = np.repeat(source[:1], waveform.shape[0], axis=0)
        source = torch.from_numpy(np.ascontiguousarray(source)).to(waveform.device)
        ramp = int(round(config.audio_composite_ramp_ms * rate / 1000.0))
        return K.retake_composite_audio(waveform, source, *self.audio_sample_window, ramp)

    def __call__(self, video_path: Optional[str], text_encoding: torch.Tensor, text_mask: Optional[torch.Tensor], config: RetakeConfig,
                 negative_text_encoding: Optional[torch.Tensor] = None, audio_encoding: Optional[torch.Tensor] = None,
                 negative_audio_encoding: Optional[torch.Tensor] = None, callback: Optional[Callable[[str, int, int], None]] = None, *,
                 frames=None, initial_noise: Optional[torch.Tensor] = None, guider=None, audio_path: Optional[str] = None,
                 audio_latent: Optional[torch.Tensor] = None, initial_audio_noise: Optional[torch.Tensor] = None):
        """-> uint8 frames (T, H, W, 3) (the final latent when no decoder is set).  text_mask is accepted and unused, as every loop here
        passes context_mask=None (reference pipelines/common.py:223-232); so are the audio encodings without a sound track.  guider
        (keyword-only): the guider of the guided mode instead of CFGGuider(config.cfg_scale), e.g. LtxAPGGuider.
        audio_path / audio_latent (keyword-only): the clip's sound track (denoise_latent) -> (frames, audio): the audio is the waveform
        (2, S) fp32 at the vocoder's output_sample_rate when audio_decoder and vocoder are set, else the audio latent (1, 8, T_a, 16).
        audio_window, audio_sample_window and audio_latent of the call are kept as attributes."""
        with_audio = audio_path is not None or audio_latent is not None
        self.audio_window = self.audio_sample_window = self.audio_latent = None
        out = self.denoise_latent(video_path, text_encoding, config, negative_text_encoding, callback, frames=frames, initial_noise=initial_noise,
                                  guider=guider, audio_path=audio_path, audio_latent=audio_latent, initial_audio_noise=initial_audio_noise,
                                  audio_encoding=audio_encoding, negative_audio_encoding=negative_audio_encoding)
        latent, audio = out if with_audio else (out, None)
        self.audio_latent = audio
        if with_audio and self.audio_decoder is not None and self.vocoder is not None:
            audio = self._decode_audio(audio, audio_path, config)
        if self.video_decoder is None:
            return (latent, audio) if with_audio else latent
        video = decode_video(latent, self.video_decoder, config.tiling_config)             # no automatic tiling here
        if video.dtype != torch.uint8:                                                     # decode_tiled: float (1, 3, T, H, W) in [-1, 1]
            video = K.video_to_uint8(video[0] if video.dim() == 5 else video)
        if config.composite_source:
            video = K.retake_composite(video.contiguous(), self.source_frames, *self.pixel_window, config.composite_ramp)
        return (video, audio) if with_audio else video


def create_retake_pipeline(transformer, video_encoder, video_decoder, audio_decoder=None, vocoder=None, audio_encoder=None,
                           audio_processor=None) -> RetakePipeline:
    return RetakePipeline(transformer, video_encoder, video_decoder, audio_decoder, vocoder, audio_encoder, audio_processor)
