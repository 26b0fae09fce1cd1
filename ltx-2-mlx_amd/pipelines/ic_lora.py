"""IC-LoRA on MI355X: video-to-video generation steered by a control video (depth, pose, edges).

Mirrors reference LTX_2_MLX/pipelines/ic_lora.py:49-53 (ControlType), :241-287 (ICLoraConfig, VideoCondition), :345-411
(create_video_conditionings) and :414-753 (ICLoraPipeline).  The control video is encoded by the VAE encoder and its tokens are APPENDED to
the sequence at frame 0 (conditioning/keyframe.py: nothing there assumes one latent frame), so stage 1 runs the DiT on 2 * F*H*W tokens.
  stage 1: half resolution, image conditionings first and control conditionings after them, noise 1.0, the first stage_1_steps steps of
           the distilled sigma table without guidance (the existing conditioned loop, captured when there is no callback), under the IC-LoRA
           fused into the touched weights for this stage only (ti2vid_hq.fused_lora);
  stage 2: appended tokens cut off, un-normalise -> spatial upscaler -> normalise, the BASE weights, image conditionings only, noise at
           STAGE_2_DISTILLED_SIGMA_VALUES[0], stage_2_steps steps, decode.
The control path stays on the device: uint8 frames -> kernels.canny (ControlType.CANNY) -> kernels.frames_to_patches ->
SimpleVideoEncoder.encode_patches.  The reference does both the file reading and the edges with OpenCV, which this project does not depend
on; load_control_frames reads arrays, image directories and (through an ffmpeg binary) video files instead.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
from dataclasses import dataclass
from enum import Enum
from typing import Callable, Dict, List, Optional, Union

import numpy as np
import torch

from .. import kernels as K
from ..components import DISTILLED_SIGMA_VALUES, STAGE_2_DISTILLED_SIGMA_VALUES, EulerDiffusionStep, GaussianNoiser, VideoLatentPatchifier
from ..conditioning.keyframe import VideoConditionByKeyframeIndex
from ..loader.lora_loader import LoRAConfig
from ..model.transformer import LTXModel, X0Model
from ..model.video_vae import SimpleVideoDecoder, TilingConfig
from .common import (ImageCondition, as_x0model, conditioned_initial_state, create_image_conditionings, decode_video, final_latent,
                     joint_denoise_loop, seeded_noiser, stage_callback, upscale_latent_x2, video_tools_for)
from .ti2vid_hq import fused_lora

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")


class ControlType(Enum):
    """How a control video is preprocessed (reference :49-53)."""
    CANNY = "canny"
    RAW = "raw"         # used as it is, e.g. a pre-made depth or pose video


@dataclass
class ICLoraConfig:
    """Configuration of the IC-LoRA pipeline (reference :241-273).  The default 480x704 fails the multiple-of-64 check, as the reference's does."""
    height: int = 480
    width: int = 704
    num_frames: int = 97            # must be 8k + 1
    stage_1_steps: int = 7          # of the distilled table's 8: the reference's default stops at sigma 0.421875, short of 0
    stage_2_steps: int = 3
    seed: int = 42
    fps: float = 24.0
    tiling_config: Optional[TilingConfig] = None
    dtype: torch.dtype = torch.float32
    use_hip_graph: bool = True      # MI355X addition: replay each stage's loop from one captured graph (no callback)

    def __post_init__(self):
        if self.num_frames % 8 != 1:
            raise ValueError(f"num_frames must be 8*k + 1, got {self.num_frames}. Valid values: 1, 9, 17, 25, 33, ..., 121")
        if self.height % 64 != 0 or self.width % 64 != 0:
            raise ValueError(f"Resolution ({self.height}x{self.width}) must be divisible by 64.")


@dataclass
class VideoCondition:
    """A control video for IC-LoRA (reference :276-287).  `frames` may carry already loaded uint8 frames (F, H, W, 3) instead of a path;
    they are resized to the stage's resolution like a file's would be."""
    video_path: Optional[str]
    strength: float = 0.95
    control_type: ControlType = ControlType.RAW
    canny_low: int = 100
    canny_high: int = 200
    save_control: bool = False
    frames: Optional[Union[np.ndarray, torch.Tensor]] = None


def _fit_frames(frames: np.ndarray, height: int, width: int, num_frames: int, what: str) -> np.ndarray:
    """(n, h, w, 3) or (n, h, w) uint8 -> exactly (num_frames, height, width, 3): cut, plain LANCZOS resize, last frame repeated."""
    from PIL import Image
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = np.repeat(frames[..., None], 3, axis=-1)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
        raise ValueError(f"{what}: control frames must be uint8 (F, H, W, 3) or (F, H, W), got {frames.dtype} {frames.shape}")
    if frames.shape[0] == 0:
        raise ValueError(f"Could not read any frames from {what}")
    frames = frames[:num_frames]
    if frames.shape[1:3] != (height, width):
        frames = np.stack([np.array(Image.fromarray(f).resize((width, height), Image.Resampling.LANCZOS)) for f in frames])
    if frames.shape[0] < num_frames:
        frames = np.concatenate([frames, np.repeat(frames[-1:], num_frames - frames.shape[0], axis=0)])
    return np.ascontiguousarray(frames)


def _ppm_frames(stream: bytes) -> np.ndarray:
    """A concatenation of binary PPM images (P6, maxval 255, one size) -> uint8 (n, h, w, 3).  Every image carries its own width and height,
    so the size is what the decoder produced (rotation and sample aspect ratio applied), not what a stream header printed."""
    frames, at = [], 0
    while at < len(stream):
        m = re.compile(rb"P6\s+(\d+)\s+(\d+)\s+(\d+)\s").match(stream, at)
        if m is None or int(m.group(3)) != 255:
            raise ValueError("not a stream of 8-bit binary PPM images")
        w, h = int(m.group(1)), int(m.group(2))
        if m.end() + h * w * 3 > len(stream):
            break                                    # a cut-off last image
        frames.append(np.frombuffer(stream, dtype=np.uint8, count=h * w * 3, offset=m.end()).reshape(h, w, 3))
        at = m.end() + h * w * 3
    if not frames or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("no frames, or frames of several sizes")
    return np.stack(frames)


def _ffmpeg_frames(path: str, num_frames: int) -> np.ndarray:
    """The first num_frames frames of a video file's first video stream at their decoded size, piped out of one ffmpeg run as PPM images:
    the reverse of scripts/generate.py's save_video.  The resize is done afterwards, the same way for every source."""
    r = subprocess.run(["ffmpeg", "-v", "error", "-i", path, "-map", "0:v:0", "-frames:v", str(num_frames), "-f", "image2pipe", "-c:v", "ppm",
                        "-"], capture_output=True)
    try:
        if r.returncode != 0:
            raise ValueError("ffmpeg failed")
        return _ppm_frames(r.stdout)
    except ValueError as e:
        raise ValueError(f"Could not read any frames from {path}: {e}: {r.stderr.decode('utf-8', 'replace')[-300:]}") from None


def load_control_frames(path: str, height: int, width: int, num_frames: int) -> np.ndarray:
    """A control video -> uint8 (num_frames, height, width, 3).  `path` is a .npy / .npz array of uint8 frames ((F, H, W, 3) or (F, H, W);
    the first array of an .npz), a directory of image frames (sorted by name), or a video file when an ffmpeg binary exists.  Frames of
    another size get the plain PIL LANCZOS resize of load_image_as_tensor (the reference: OpenCV's LANCZOS4); a short clip is padded with
    its last frame (reference :108-113)."""
    from PIL import Image
    if not os.path.exists(path):
        raise FileNotFoundError(f"Control video not found: {path}")
    low = path.lower()
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_SUFFIXES))[:num_frames]
        if not names:
            raise ValueError(f"Could not read any frames from {path}: no image files ({', '.join(IMAGE_SUFFIXES)})")
        frames = [Image.open(os.path.join(path, n)).convert("RGB") for n in names]
        if any(f.size != frames[0].size for f in frames):
            frames = [f.resize((width, height), Image.Resampling.LANCZOS) for f in frames]
        frames = np.stack([np.array(f) for f in frames])
    elif low.endswith(".npy"):
        frames = np.load(path)
    elif low.endswith(".npz"):
        with np.load(path) as z:
            frames = z[z.files[0]]
    elif shutil.which("ffmpeg") is not None:
        frames = _ffmpeg_frames(path, num_frames)
    else:
        raise RuntimeError(f"reading the video file {path} needs an ffmpeg binary, and none was found: pass the control video as a .npy / .npz "
                           "array of uint8 frames (F, H, W, 3), or as a directory of image frames")
    return _fit_frames(frames, height, width, num_frames, path)


def load_control_signal_tensor(control_signal: np.ndarray, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """uint8 (F, H, W, 3) in [0, 255] -> (1, 3, F, H, W) in [-1, 1] (reference :216-238): the host form of what
    kernels.frames_to_patches computes on the device; kept as the yardstick of that kernel."""
    v = torch.from_numpy(np.asarray(control_signal).astype(np.float32) / 127.5 - 1.0)
    return v.permute(3, 0, 1, 2)[None].to(dtype)


def create_video_conditionings(videos: List[VideoCondition], video_encoder, height: int, width: int, num_frames: int,
                               dtype: torch.dtype = torch.float32, save_video: Optional[Callable] = None,
                               fps: float = 24.0, save_dir: Optional[str] = None) -> List[VideoConditionByKeyframeIndex]:
    """Encode every control video into an appended-token conditioning at frame 0 (reference :345-411).  Frames go to the device as uint8;
    ControlType.CANNY runs kernels.canny there, and save_control writes the edges as `<stem>_canny.mp4` through `save_video(frames, path,
    fps=)` (scripts/generate.py's; `<stem>_canny.npz` without one); kernels.frames_to_patches and encode_patches do the rest.
    The sidecar goes into save_dir under the control video's base name (generate_video passes the output's directory, so a read-only
    input directory does not matter); with save_dir=None it lands beside the control video, as the reference's does ("control" in the
    working directory when only `frames` is given)."""
    if videos and video_encoder is None:
        raise ValueError("control-video conditioning needs a video_encoder")
    out = []
    for vc in videos:
        if vc.frames is not None:
            src = vc.frames.cpu().numpy() if isinstance(vc.frames, torch.Tensor) else vc.frames
            frames = _fit_frames(src, height, width, num_frames, "VideoCondition.frames")
        else:
            frames = load_control_frames(vc.video_path, height, width, num_frames)
        x = torch.from_numpy(frames).to(video_encoder.device)
        if vc.control_type == ControlType.CANNY:
            x = K.canny(x, vc.canny_low, vc.canny_high)                      # (F, H, W): white edges on black, replicated to RGB below
            if vc.save_control:
                stem = os.path.splitext(vc.video_path.rstrip("/"))[0] if vc.video_path else "control"
                if save_dir is not None:
                    stem = os.path.join(save_dir, os.path.basename(stem))
                rgb = x[..., None].expand(-1, -1, -1, 3).cpu().numpy()
                if save_video is not None:
                    save_video(rgb, f"{stem}_canny.mp4", fps=int(round(fps)))
                else:
                    np.savez_compressed(f"{stem}_canny.npz", frames=rgb)
        elif vc.control_type != ControlType.RAW:
            raise ValueError(f"Unknown control type: {vc.control_type}")
        latent = video_encoder.encode_patches(K.frames_to_patches(x)).to(dtype)
        out.append(VideoConditionByKeyframeIndex(keyframes=latent, frame_idx=0, strength=vc.strength))
    return out


class ICLoraPipeline:
    def __init__(self, transformer: Union[LTXModel, X0Model], video_encoder, video_decoder: Optional[SimpleVideoDecoder],
                 spatial_upscaler: Optional[Callable], base_transformer_weights: Optional[Dict[str, torch.Tensor]] = None,
                 lora_configs: Optional[List[LoRAConfig]] = None, save_video: Optional[Callable] = None, save_dir: Optional[str] = None):
        """base_transformer_weights is accepted for the reference's signature and unused: fused_lora keeps the touched tensors aside itself
        and registers them again after stage 1.  save_video / save_dir (MI355X additions): the writer and the directory of the save_control
        sidecar (create_video_conditionings)."""
        self.transformer, self.is_av_model = as_x0model(transformer)
        self._velocity_model = self.transformer.velocity_model
        self.video_encoder = video_encoder
        self.video_decoder = video_decoder
        self.spatial_upscaler = spatial_upscaler
        self.base_transformer_weights = base_transformer_weights
        self.lora_configs = lora_configs or []
        self.save_video, self.save_dir = save_video, save_dir
        self.patchifier = VideoLatentPatchifier(patch_size=1)
        self.diffusion_step = EulerDiffusionStep()
        self.token_counts: List[int] = []        # DiT tokens of each stage of the last call

    def _loop(self, state, sigmas, ctx, callback, config):
        # no guidance (reference :503-558): the existing conditioned loop; an AudioVideo model runs through its video twin
        return joint_denoise_loop(self.transformer, self.is_av_model, state, None, sigmas, ctx, None, self.diffusion_step, callback,
                                  config.use_hip_graph)[0]

    def stage1_latent(self, text_encoding: torch.Tensor, config: ICLoraConfig, images: Optional[List[ImageCondition]] = None,
                      video_conditioning: Optional[List[VideoCondition]] = None, callback=None, *,
                      initial_noise: Optional[torch.Tensor] = None, noiser: Optional[GaussianNoiser] = None) -> torch.Tensor:
        """Stage 1 alone: the half-resolution latent (1, 128, F, H/64, W/64) of the run under the IC-LoRA.  initial_noise covers the
        appended control tokens too."""
        if len(self.lora_configs) > 1:               # before anything is encoded
            raise NotImplementedError("more than one IC-LoRA at a time is not built: fused_lora fuses one adapter")
        dev = self._velocity_model.device
        noiser = noiser or seeded_noiser(dev, config.seed)
        h1, w1 = config.height // 2, config.width // 2
        tools = video_tools_for(self.patchifier, config.num_frames, h1, w1, config.fps)
        # image conditionings first, control conditionings after them (reference :635)
        conds = create_image_conditionings(images or [], self.video_encoder, h1, w1, config.dtype) + \
            create_video_conditionings(video_conditioning or [], self.video_encoder, h1, w1, config.num_frames, config.dtype,
                                       save_video=self.save_video, fps=config.fps, save_dir=self.save_dir)
        state = conditioned_initial_state(tools, conds, config.dtype, dev)
        self.token_counts.append(int(state.latent.shape[1]))
        sigmas = [float(s) for s in DISTILLED_SIGMA_VALUES[: config.stage_1_steps + 1]]
        state = noiser(state, noise_scale=1.0, noise=initial_noise)
        lora = self.lora_configs
        with fused_lora(self._velocity_model, lora[0] if lora else None):
            state = self._loop(state, sigmas, text_encoding.to(dev), stage_callback(callback, "stage1_iclora"), config)
        return final_latent(tools, state)

    def stage2_latent(self, stage1: torch.Tensor, text_encoding: torch.Tensor, config: ICLoraConfig,
                      images: Optional[List[ImageCondition]] = None, callback=None, *, stage2_noise: Optional[torch.Tensor] = None,
                      noiser: Optional[GaussianNoiser] = None) -> torch.Tensor:
        """Stage 2 from a stage-1 latent: x2 upscale, the base weights, image conditionings only -> (1, 128, F, H/32, W/32)."""
        dev = self._velocity_model.device
        noiser = noiser or seeded_noiser(dev, config.seed)
        tools = video_tools_for(self.patchifier, config.num_frames, config.height, config.width, config.fps)
        upscaled = upscale_latent_x2(stage1, self.spatial_upscaler, self.video_encoder, self.video_decoder)
        conds = create_image_conditionings(images or [], self.video_encoder, config.height, config.width, config.dtype)
        state = conditioned_initial_state(tools, conds, config.dtype, dev, initial_latent=upscaled)
        self.token_counts.append(int(state.latent.shape[1]))
        sig2 = [float(s) for s in STAGE_2_DISTILLED_SIGMA_VALUES[: config.stage_2_steps + 1]]
        state = noiser(state, noise_scale=sig2[0], noise=stage2_noise)
        state = self._loop(state, sig2, text_encoding.to(dev), stage_callback(callback, "stage2_refine"), config)
        return final_latent(tools, state)

    def denoise_latent(self, text_encoding: torch.Tensor, config: ICLoraConfig, images: Optional[List[ImageCondition]] = None,
                       video_conditioning: Optional[List[VideoCondition]] = None, callback: Optional[Callable[[str, int, int], None]] = None,
                       *, initial_noise: Optional[torch.Tensor] = None, stage2_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Both stages up to the final latent (1, 128, F, H/32, W/32).  initial_noise / stage2_noise (keyword-only, MI355X addition):
        supplied N(0,1) tensors of the patchified shapes, stage 1's INCLUDING the appended tokens, so results can be compared with a
        restatement."""
        if self.spatial_upscaler is None:
            raise ValueError("ICLoraPipeline requires spatial_upscaler to be provided")
        dev = self._velocity_model.device
        noiser = seeded_noiser(dev, config.seed)
        self.token_counts = []
        latent = self.stage1_latent(text_encoding, config, images, video_conditioning, callback, initial_noise=initial_noise, noiser=noiser)
        return self.stage2_latent(latent, text_encoding, config, images, callback, stage2_noise=stage2_noise, noiser=noiser)

    def __call__(self, text_encoding: torch.Tensor, text_mask: Optional[torch.Tensor], config: ICLoraConfig,
                 images: Optional[List[ImageCondition]] = None, video_conditioning: Optional[List[VideoCondition]] = None,
                 callback: Optional[Callable[[str, int, int], None]] = None, *, initial_noise: Optional[torch.Tensor] = None,
                 stage2_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> uint8 frames (F, H, W, 3) (the final latent when no decoder is set).  text_mask is accepted and unused, as every loop here
        passes context_mask=None (reference pipelines/common.py:223-232)."""
        latent = self.denoise_latent(text_encoding, config, images, video_conditioning, callback, initial_noise=initial_noise,
                                     stage2_noise=stage2_noise)
        return decode_video(latent, self.video_decoder, config.tiling_config)           # no automatic tiling here


def create_ic_lora_pipeline(transformer, video_encoder, video_decoder, spatial_upscaler, base_transformer_weights=None,
                            lora_configs: Optional[List[LoRAConfig]] = None, save_video: Optional[Callable] = None,
                            save_dir: Optional[str] = None) -> ICLoraPipeline:
    return ICLoraPipeline(transformer, video_encoder, video_decoder, spatial_upscaler, base_transformer_weights, lora_configs, save_video, save_dir)
