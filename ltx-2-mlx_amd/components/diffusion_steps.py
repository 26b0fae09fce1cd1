"""Euler stepping through the C ABI (ltx2_euler_step).  Mirrors reference
LTX_2_MLX/components/diffusion_steps.py:24-67 and core_utils.py:34-94."""
from __future__ import annotations

from typing import Optional, Union

import torch

from .. import kernels as K


def _sig(s) -> float:
    return float(s.item()) if isinstance(s, torch.Tensor) else float(s)


def to_velocity(sample: torch.Tensor, sigma: Union[float, torch.Tensor], denoised_sample: torch.Tensor) -> torch.Tensor:
    s = _sig(sigma)
    if s == 0:
        raise ValueError("Sigma can't be 0.0")
    return ((sample.float() - denoised_sample.float()) / s).to(sample.dtype)


def to_denoised(sample: torch.Tensor, velocity: torch.Tensor, sigma: Union[float, torch.Tensor]) -> torch.Tensor:
    return (sample.float() - velocity.float() * (sigma.float() if isinstance(sigma, torch.Tensor) else sigma)).to(sample.dtype)


class EulerDiffusionStep:
    """sample + (sample - denoised)/sigma * (sigma_next - sigma), computed in fp32 on the GPU."""

    def step(self, sample: torch.Tensor, denoised_sample: torch.Tensor, sigmas, step_index: int) -> torch.Tensor:
        sigma, sigma_next = _sig(sigmas[step_index]), _sig(sigmas[step_index + 1])
        shp = sample.shape
        c = shp[-1]
        out = K.euler_step(sample.float().reshape(-1, c), denoised_sample.float().reshape(-1, c), sigma, sigma_next)
        return out.reshape(shp).to(sample.dtype)


class HeunDiffusionStep:
    """The reference's second-order predictor-corrector step (components/diffusion_steps.py:132-190), its statements one by one in torch:
    without denoised_at_predicted the Euler predictor, with it sample + 0.5*(v + v_at_predicted)*dt.  This is the eager form, on whatever device
    the tensors live; the device loops run the same step as ltx2_heun_predict / ltx2_heun_correct."""

    def step(self, sample: torch.Tensor, denoised_sample: torch.Tensor, sigmas, step_index: int,
             denoised_at_predicted: Optional[torch.Tensor] = None) -> torch.Tensor:
        sigma, sigma_next = _sig(sigmas[step_index]), _sig(sigmas[step_index + 1])
        dt = sigma_next - sigma
        velocity = to_velocity(sample, sigma, denoised_sample).float()
        sample_f32 = sample.float()
        predicted = sample_f32 + velocity * dt
        if denoised_at_predicted is None:
            return predicted.to(sample.dtype)
        velocity_at_predicted = to_velocity(predicted.to(sample.dtype), sigma_next, denoised_at_predicted).float()
        return (sample_f32 + (0.5 * (velocity + velocity_at_predicted)) * dt).to(sample.dtype)


class EulerAncestralDiffusionStep:
    """The reference's stochastic sampler (components/diffusion_steps.py:70-129, its note: ComfyUI's euler_ancestral_cfg_pp): the Euler step to
    sigma_down, then sigma_up * N(0,1) on top.  Without `noise` the step is ONE kernel (ltx2_ancestral_euler_step_x0) whose noise is Philox4x32-10
    under (seed, step_index, stream_id, element index) -- no host generator, the same values however the step is launched.  With a given `noise`
    tensor the step is the reference's statements in torch, on whatever device the tensors live.  `eta` scales the noise (the reference's step
    always takes 1.0); eta = 0 is the Euler step."""

    def __init__(self, eta: float = 1.0, seed: int = 0):
        self.eta = float(eta)
        self.seed = int(seed)
        self._seed_word = None

    @staticmethod
    def _get_ancestral_step(sigma_from: float, sigma_to: float, eta: float = 1.0):
        """(sigma_up, sigma_down) of a step from sigma_from to sigma_to, in double: sigma_up = min(sigma_to, eta * sigma_to *
        sqrt(1 - sigma_to^2 / sigma_from^2)) written as the reference writes it, sigma_down^2 = sigma_to^2 - sigma_up^2; (0, 0) at sigma_to = 0."""
        if sigma_to == 0.0:
            return 0.0, 0.0
        variance = sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2
        sigma_up = min(sigma_to, eta * variance ** 0.5)
        return sigma_up, (sigma_to ** 2 - sigma_up ** 2) ** 0.5

    def step(self, sample: torch.Tensor, denoised_sample: torch.Tensor, sigmas, step_index: int, noise: Optional[torch.Tensor] = None,
             stream_id: int = 0) -> torch.Tensor:
        sigma, sigma_next = _sig(sigmas[step_index]), _sig(sigmas[step_index + 1])
        sigma_up, sigma_down = self._get_ancestral_step(sigma, sigma_next, self.eta)
        if noise is not None:
            result = sample.float() + to_velocity(sample, sigma, denoised_sample).float() * (sigma_down - sigma)
            if sigma_up > 0:
                result = result + noise.float() * sigma_up
            return result.to(sample.dtype)
        if self._seed_word is None or self._seed_word.device != sample.device:
            self._seed_word = K.seed_word(self.seed, sample.device)
        shp = sample.shape
        c = shp[-1]
        out = K.ancestral_euler_step_x0(sample.float().reshape(-1, c).contiguous(), denoised_sample.float().reshape(-1, c).contiguous(), sigma, sigma_up,
                                        sigma_down, self._seed_word, step_index, stream_id)
        return out.reshape(shp).to(sample.dtype)
