"""Text-side per-prompt path: Gemma feature extractors + Embeddings1DConnector on the MI355X kernels.
Mirrors LTX_2_MLX/model/text_encoder/__init__.py for the classes on this path, Gemma-3 (gemma3.py) included."""
from .connector import Embeddings1DConnector
from .encoder import (AudioVideoGemmaEncoderOutput, AudioVideoGemmaTextEncoderModel, VideoGemmaEncoderOutput, VideoGemmaTextEncoderModel,
                      create_av_text_encoder_v2, create_av_text_encoder_v2_from_checkpoint, create_text_encoder,
                      load_av_text_encoder_v2_weights, load_text_encoder_weights)
from .feature_extractor import GemmaFeaturesExtractorProjLinear, GemmaFeaturesExtractorV2, norm_and_concat_padded_batch
from .gemma3 import Gemma3Config, Gemma3Model, create_gemma3_model, load_gemma3_weights, load_gemma_tokenizer, tokenize_prompt

__all__ = ["Embeddings1DConnector", "GemmaFeaturesExtractorProjLinear", "GemmaFeaturesExtractorV2", "norm_and_concat_padded_batch",
           "VideoGemmaTextEncoderModel", "AudioVideoGemmaTextEncoderModel", "VideoGemmaEncoderOutput", "AudioVideoGemmaEncoderOutput",
           "create_text_encoder", "load_text_encoder_weights", "create_av_text_encoder_v2", "create_av_text_encoder_v2_from_checkpoint",
           "load_av_text_encoder_v2_weights", "Gemma3Config", "Gemma3Model", "create_gemma3_model", "load_gemma3_weights",
           "load_gemma_tokenizer", "tokenize_prompt"]
