from .diffusion_steps import EulerAncestralDiffusionStep, EulerDiffusionStep, HeunDiffusionStep, to_denoised, to_velocity
from .guiders import (CFGGuider, CFGStarRescalingGuider, LegacyStatefulAPGGuider, LtxAPGGuider, MultiModalGuider, MultiModalGuiderParams, STGGuider,
                      projection_coef)
from .noisers import GaussianNoiser
from .perturbations import (BatchedPerturbationConfig, Perturbation, PerturbationConfig, PerturbationType, create_batched_stg_config,
                            create_stg_perturbation)
from .res2s import get_res2s_coefficients, phi
from .patchifiers import AudioPatchifier, VideoLatentPatchifier, get_pixel_coords
from .schedulers import (DISTILLED_SIGMA_VALUES, STAGE_2_DISTILLED_SIGMA_VALUES, LTX2Scheduler,
                         get_sigma_schedule)

__all__ = ["CFGGuider", "CFGStarRescalingGuider", "LtxAPGGuider", "LegacyStatefulAPGGuider", "STGGuider", "MultiModalGuider", "MultiModalGuiderParams", "projection_coef", "PerturbationType", "Perturbation", "PerturbationConfig",
           "BatchedPerturbationConfig", "create_stg_perturbation", "create_batched_stg_config", "EulerDiffusionStep", "EulerAncestralDiffusionStep", "HeunDiffusionStep", "to_denoised", "to_velocity", "GaussianNoiser", "AudioPatchifier", "VideoLatentPatchifier",
           "get_pixel_coords", "DISTILLED_SIGMA_VALUES", "STAGE_2_DISTILLED_SIGMA_VALUES", "LTX2Scheduler",
           "get_sigma_schedule", "phi", "get_res2s_coefficients"]
