"""Keyframe conditioning (keyframe interpolation): the encoded keyframe's tokens are APPENDED after the F*H*W video tokens, with
positions of their own and a denoise mask of 1 - strength; no latent frame is overwritten.  VideoLatentTools.clear_conditioning cuts
them off again after the loop.  Mirrors reference LTX_2_MLX/conditioning/keyframe.py:10-87."""
from __future__ import annotations

import torch

from ..components.patchifiers import get_pixel_coords
from ..types import LatentState, VideoLatentShape
from .tools import VideoLatentTools


class VideoConditionByKeyframeIndex:
    def __init__(self, keyframes: torch.Tensor, frame_idx: int, strength: float):
        """keyframes: encoded keyframe latent (B, C, 1, H, W); frame_idx: the PIXEL frame the keyframe sits at; strength: 1 keeps the
        appended tokens clean (mask 0), 0 leaves them free."""
        self.keyframes, self.frame_idx, self.strength = keyframes, frame_idx, strength

    def apply_to(self, latent_state: LatentState, latent_tools: VideoLatentTools) -> LatentState:
        lat = latent_state.latent
        tokens = latent_tools.patchifier.patchify(self.keyframes).to(lat.device, lat.dtype)
        bounds = latent_tools.patchifier.get_patch_grid_bounds(VideoLatentShape.from_shape(self.keyframes.shape), device=lat.device)
        # the causal first-frame shift belongs to a keyframe at frame 0 only (keyframe.py:62-63)
        pos = get_pixel_coords(bounds, latent_tools.scale_factors, causal_fix=latent_tools.causal_fix if self.frame_idx == 0 else False).float()
        pos = torch.cat([(pos[:, 0:1] + self.frame_idx) / latent_tools.fps, pos[:, 1:]], dim=1)
        mask = torch.full((tokens.shape[0], tokens.shape[1], 1), 1.0 - self.strength, dtype=latent_state.denoise_mask.dtype,
                          device=latent_state.denoise_mask.device)
        return LatentState(latent=torch.cat([lat, tokens], dim=1), denoise_mask=torch.cat([latent_state.denoise_mask, mask], dim=1),
                           positions=torch.cat([latent_state.positions, pos.to(latent_state.positions.device)], dim=2),
                           clean_latent=torch.cat([latent_state.clean_latent, tokens.to(latent_state.clean_latent.dtype)], dim=1))
