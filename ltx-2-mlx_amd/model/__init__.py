from . import transformer, video_vae
from .upscaler import (SpatialUpscaler, TemporalUpscaler, load_spatial_upscaler_weights, load_temporal_upscaler_weights, upscale_latent,
                       upscale_latent_temporal)

__all__ = ["transformer", "video_vae", "SpatialUpscaler", "TemporalUpscaler", "load_spatial_upscaler_weights",
           "load_temporal_upscaler_weights", "upscale_latent", "upscale_latent_temporal"]
