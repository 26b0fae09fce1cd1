"""Classifier-free guidance on the denoised prediction (reference LTX_2_MLX/components/guiders.py:26-77, 105-205, 290-306).

Host-side glue of the guided single-stage loops: two x0 predictions (positive / negative prompt) per step are combined here in
fp32 on the device (element-wise ops and dot products over a (B, N, C) tensor).  pipelines.common.projected_denoise_loop runs the
same guiders as two kernels per step (csrc/sampler.hip).  STGGuider (:80-102) pushes the guided prediction away from one made with chosen
self-attentions skipped (components/perturbations.py); pipelines.common.stg_denoise_loop runs it inside one kernel per step."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import torch


def projection_coef(to_project: torch.Tensor, project_onto: torch.Tensor) -> torch.Tensor:
    """<to_project, project_onto> / (|project_onto|^2 + 1e-8) per batch element, shape (B, 1) (guiders.py:290-306)."""
    b = to_project.shape[0]
    p, n = to_project.reshape(b, -1), project_onto.reshape(b, -1)
    return (p * n).sum(dim=1, keepdim=True) / ((n * n).sum(dim=1, keepdim=True) + 1e-8)


@dataclass(frozen=True)
class CFGGuider:
    """cond + (scale - 1) (cond - uncond)  (guiders.py:26-47)."""
    scale: float

    def delta(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        return (self.scale - 1) * (cond - uncond)

    def guide(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        return cond + self.delta(cond, uncond)

    def enabled(self) -> bool:
        return self.scale != 1.0


@dataclass(frozen=True)
class CFGStarRescalingGuider:
    """CFG with the unconditioned sample rescaled onto the conditioned one first (guiders.py:51-76): the coefficient (B, 1) multiplies a
    (B, N, C) tensor exactly as the reference's broadcast does."""
    scale: float

    def delta(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        rescaled_neg = projection_coef(cond, uncond) * uncond
        return (self.scale - 1) * (cond - rescaled_neg)

    def guide(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        return cond + self.delta(cond, uncond)

    def enabled(self) -> bool:
        return self.scale != 1.0


@dataclass(frozen=True)
class STGGuider:
    """pos + scale (pos - perturbed)  (guiders.py:80-102): `perturbed` is the prediction of a pass whose chosen attentions acted as a
    passthrough.  scale 0 disables it."""
    scale: float

    def delta(self, pos_denoised: torch.Tensor, perturbed_denoised: torch.Tensor) -> torch.Tensor:
        return self.scale * (pos_denoised - perturbed_denoised)

    def guide(self, pos_denoised: torch.Tensor, perturbed_denoised: torch.Tensor) -> torch.Tensor:
        return pos_denoised + self.delta(pos_denoised, perturbed_denoised)

    def enabled(self) -> bool:
        return self.scale != 0.0


def _apg_delta(guidance: torch.Tensor, cond: torch.Tensor, eta: float, norm_threshold: float) -> torch.Tensor:
    """The part the two APG guiders share (guiders.py:132-144 / :186-197): the guidance clipped to norm_threshold over the last three axes,
    split into its components parallel and orthogonal to cond, the parallel one weighted by eta."""
    if norm_threshold > 0:
        guidance_norm = torch.sqrt((guidance * guidance).sum(dim=(-1, -2, -3), keepdim=True))
        guidance = guidance * torch.minimum(torch.ones_like(guidance), norm_threshold / guidance_norm)
    g_parallel = projection_coef(guidance, cond) * cond
    return g_parallel * eta + (guidance - g_parallel)


@dataclass(frozen=True)
class LtxAPGGuider:
    """Adaptive projected guidance (guiders.py:105-152): cond - uncond, norm-clipped, its component parallel to cond weighted by eta, the
    whole scaled by scale - 1."""
    scale: float
    eta: float = 1.0
    norm_threshold: float = 0.0

    def delta(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        return _apg_delta(cond - uncond, cond, self.eta, self.norm_threshold) * (self.scale - 1)

    def guide(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        return cond + self.delta(cond, uncond)

    def enabled(self) -> bool:
        return self.scale != 1.0


@dataclass(frozen=False)
class LegacyStatefulAPGGuider:
    """APG with a running sum of the guidance (guiders.py:155-205): with momentum != 0 the first call keeps cond - uncond, every later one
    momentum * running_avg + (cond - uncond); the result is scaled by `scale`, not scale - 1.  reset() forgets the running state: every
    loop here calls it before its first step (the reference never does)."""
    scale: float
    eta: float
    norm_threshold: float = 5.0
    momentum: float = 0.0
    running_avg: Optional[torch.Tensor] = field(default=None, repr=False)

    def reset(self) -> None:
        self.running_avg = None

    def delta(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        guidance = cond - uncond
        if self.momentum != 0:
            self.running_avg = guidance if self.running_avg is None else self.momentum * self.running_avg + guidance
            guidance = self.running_avg
        return _apg_delta(guidance, cond, self.eta, self.norm_threshold) * self.scale

    def guide(self, cond: torch.Tensor, uncond: torch.Tensor) -> torch.Tensor:
        return cond + self.delta(cond, uncond)

    def enabled(self) -> bool:
        return self.scale != 0.0


@dataclass(frozen=True)
class MultiModalGuiderParams:
    """One modality's scales of the multi-modal guider (guiders.py:211-224)."""
    cfg_scale: float = 1.0
    stg_scale: float = 0.0
    stg_blocks: Optional[list] = field(default_factory=list)
    rescale_scale: float = 0.0
    modality_scale: float = 1.0
    skip_step: int = 0


@dataclass(frozen=True)
class MultiModalGuider:
    """CFG + STG + modality-isolated guidance on one modality's prediction (guiders.py:227-287).  Up to four transformer passes per step: cond,
    uncond (negative prompt), ptb (self-attentions skipped), mod (cross-modal attentions skipped).  pipelines.common.multimodal_denoise_loop
    runs calculate, post_process_latent and the Euler step of both modalities as one kernel per step (csrc/sampler.hip)."""
    params: MultiModalGuiderParams
    negative_context: Optional[torch.Tensor] = None

    def calculate(self, cond: torch.Tensor, uncond_text, uncond_perturbed, uncond_modality) -> torch.Tensor:
        """Separate fp32 ops in the reference's order.  A float (0.0) in place of a prediction: that pass did not run and its term is left
        out; a pass that ran contributes its term whatever its scale."""
        p = self.params
        pred = cond
        if isinstance(uncond_text, torch.Tensor):
            pred = pred + (p.cfg_scale - 1) * (cond - uncond_text)
        if isinstance(uncond_perturbed, torch.Tensor):
            pred = pred + p.stg_scale * (cond - uncond_perturbed)
        if isinstance(uncond_modality, torch.Tensor):
            pred = pred + (p.modality_scale - 1) * (cond - uncond_modality)
        if p.rescale_scale != 0:
            factor = torch.sqrt(cond.var(unbiased=False) + 1e-8) / torch.sqrt(pred.var(unbiased=False) + 1e-8)
            pred = pred * (p.rescale_scale * factor + (1 - p.rescale_scale))
        return pred

    def do_unconditional_generation(self) -> bool:
        return not math.isclose(self.params.cfg_scale, 1.0)

    def do_perturbed_generation(self) -> bool:
        return not math.isclose(self.params.stg_scale, 0.0)

    def do_isolated_modality_generation(self) -> bool:
        return not math.isclose(self.params.modality_scale, 1.0)

    def should_skip_step(self, step: int) -> bool:
        if self.params.skip_step == 0:
            return False
        return step % (self.params.skip_step + 1) != 0
