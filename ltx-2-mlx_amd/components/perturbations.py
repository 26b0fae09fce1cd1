"""Attention perturbations for spatio-temporal guidance (reference LTX_2_MLX/components/perturbations.py).

A perturbation names one attention of the transformer block and the blocks in which a perturbed forward skips it.  The engine builds the two
self-attention kinds: LTXModel.__call__(..., perturbations=...) turns a config into per-layer skip flags (ltx2_dit_set_stg_blocks) and runs
ltx2_dit_forward_perturbed.  The cross-modal kinds exist by name only and raise NotImplementedError there."""
from __future__ import annotations

from dataclasses import dataclass
from enum import Enum
from typing import List, Optional

import torch


class PerturbationType(Enum):
    SKIP_A2V_CROSS_ATTN = "skip_a2v_cross_attn"
    SKIP_V2A_CROSS_ATTN = "skip_v2a_cross_attn"
    SKIP_VIDEO_SELF_ATTN = "skip_video_self_attn"
    SKIP_AUDIO_SELF_ATTN = "skip_audio_self_attn"


@dataclass(frozen=True)
class Perturbation:
    """One attention kind and the block indices it is skipped in; blocks None: every block."""
    type: PerturbationType
    blocks: Optional[List[int]] = None

    def is_perturbed(self, perturbation_type: PerturbationType, block: int) -> bool:
        if self.type != perturbation_type:
            return False
        return self.blocks is None or block in self.blocks


@dataclass(frozen=True)
class PerturbationConfig:
    """The perturbations of one sample; None or an empty list: none."""
    perturbations: Optional[List[Perturbation]] = None

    def is_perturbed(self, perturbation_type: PerturbationType, block: int) -> bool:
        if self.perturbations is None:
            return False
        return any(p.is_perturbed(perturbation_type, block) for p in self.perturbations)

    @staticmethod
    def empty() -> "PerturbationConfig":
        return PerturbationConfig(perturbations=[])


@dataclass(frozen=True)
class BatchedPerturbationConfig:
    """One PerturbationConfig per sample of the batch."""
    perturbations: List[PerturbationConfig]

    def mask(self, perturbation_type: PerturbationType, block: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """(batch,) tensor: 1 = the attention runs, 0 = it is skipped."""
        return torch.tensor([0.0 if p.is_perturbed(perturbation_type, block) else 1.0 for p in self.perturbations], dtype=dtype)

    def mask_like(self, perturbation_type: PerturbationType, block: int, values: torch.Tensor) -> torch.Tensor:
        """mask() in the dtype and on the device of `values`, shaped (batch, 1, ..., 1) to broadcast against it."""
        m = self.mask(perturbation_type, block, values.dtype).to(values.device)
        return m.reshape((-1,) + (1,) * (values.dim() - 1))

    def any_in_batch(self, perturbation_type: PerturbationType, block: int) -> bool:
        return any(p.is_perturbed(perturbation_type, block) for p in self.perturbations)

    def all_in_batch(self, perturbation_type: PerturbationType, block: int) -> bool:
        return all(p.is_perturbed(perturbation_type, block) for p in self.perturbations)

    @staticmethod
    def empty(batch_size: int) -> "BatchedPerturbationConfig":
        return BatchedPerturbationConfig(perturbations=[PerturbationConfig.empty() for _ in range(batch_size)])


def create_stg_perturbation(skip_video_self_attn: bool = True, blocks: Optional[List[int]] = None) -> PerturbationConfig:
    """The usual STG config: video self-attention skipped in `blocks` (None: all)."""
    perturbations = []
    if skip_video_self_attn:
        perturbations.append(Perturbation(type=PerturbationType.SKIP_VIDEO_SELF_ATTN, blocks=blocks))
    return PerturbationConfig(perturbations=perturbations)


def create_batched_stg_config(batch_size: int, skip_video_self_attn: bool = True, blocks: Optional[List[int]] = None) -> BatchedPerturbationConfig:
    """Every sample of the batch with the same STG config."""
    config = create_stg_perturbation(skip_video_self_attn, blocks)
    return BatchedPerturbationConfig(perturbations=[config] * batch_size)
