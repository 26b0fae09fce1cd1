from .a2vid_two_stage import A2VidConfig, A2VidPipelineTwoStage, create_a2vid_pipeline, encode_audio_file
from .common import (ImageCondition, apply_conditionings, audio_modality_from_state, create_image_conditionings, frozen_audio_guided_loop, ge_denoise_loop, guided_denoise_loop, heun_denoise_loop, joint_denoise_loop, joint_guided_denoise_loop, joint_projected_denoise_loop, joint_stg_denoise_loop, multimodal_denoise_loop, projected_denoise_loop, stg_denoise_loop,
                     res2s_av_denoise_loop, res2s_denoise_loop, load_image_tensor, modality_from_state, post_process_latent, timesteps_from_mask,
                     rescale_noise_cfg, standard_cfg_denoise_loop)
from .distilled import DistilledConfig, DistilledPipeline, create_distilled_pipeline
from .ic_lora import (ControlType, ICLoraConfig, ICLoraPipeline, VideoCondition, create_ic_lora_pipeline, create_video_conditionings,
                      load_control_frames, load_control_signal_tensor)
from .keyframe_interpolation import (Keyframe, KeyframeInterpolationConfig, KeyframeInterpolationPipeline, create_keyframe_conditionings,
                                     create_keyframe_pipeline, load_image_as_tensor)
from .one_stage import OneStageCFGConfig, OneStagePipeline, create_one_stage_pipeline
from .retake import RetakeConfig, RetakePipeline, TemporalRegionMask, audio_token_window, create_retake_pipeline, end_of_clip, get_video_metadata, load_video_frames
from .ti2vid_hq import TI2VidHQConfig, TI2VidHQPipeline, create_ti2vid_hq_pipeline
from .two_stage import TwoStageCFGConfig, TwoStagePipeline, create_two_stage_pipeline

__all__ = ["ImageCondition", "apply_conditionings", "create_image_conditionings", "load_image_tensor", "joint_denoise_loop",
           "audio_modality_from_state", "modality_from_state", "post_process_latent", "timesteps_from_mask", "DistilledConfig", "DistilledPipeline",
           "create_distilled_pipeline", "OneStageCFGConfig", "OneStagePipeline", "create_one_stage_pipeline", "guided_denoise_loop", "projected_denoise_loop", "stg_denoise_loop", "joint_stg_denoise_loop", "Keyframe",
           "KeyframeInterpolationConfig", "KeyframeInterpolationPipeline", "create_keyframe_conditionings", "create_keyframe_pipeline",
           "load_image_as_tensor", "res2s_denoise_loop", "TI2VidHQConfig", "TI2VidHQPipeline", "create_ti2vid_hq_pipeline", "ControlType", "ICLoraConfig",
           "ICLoraPipeline", "VideoCondition", "create_ic_lora_pipeline", "create_video_conditionings", "load_control_frames",
           "load_control_signal_tensor", "RetakeConfig", "RetakePipeline", "TemporalRegionMask", "create_retake_pipeline", "end_of_clip", "get_video_metadata",
           "load_video_frames", "A2VidConfig", "A2VidPipelineTwoStage", "create_a2vid_pipeline", "encode_audio_file", "frozen_audio_guided_loop", "res2s_av_denoise_loop",
           "multimodal_denoise_loop", "TwoStageCFGConfig", "TwoStagePipeline", "create_two_stage_pipeline", "joint_guided_denoise_loop", "audio_token_window", "joint_projected_denoise_loop",
           "heun_denoise_loop", "ge_denoise_loop", "standard_cfg_denoise_loop", "rescale_noise_cfg"]
