"""Audio VAE decoder + vocoders on the MI355X (reference LTX_2_MLX/model/audio_vae/): latent -> log-mel -> waveform, fp32 HIP kernels
(csrc/audio.hip).  The audio encoder (AudioEncoder, load_audio_encoder_weights, encode_audio) is not built."""
from .decoder import AudioDecoder, PerChannelStatistics, load_audio_decoder_weights
from .vocoder import MelSTFT, Vocoder, VocoderWithBWE, load_vocoder_weights, load_vocoder_with_bwe_weights

__all__ = [
    "AudioDecoder",
    "PerChannelStatistics",
    "MelSTFT",
    "Vocoder",
    "VocoderWithBWE",
    "load_audio_decoder_weights",
    "load_vocoder_weights",
    "load_vocoder_with_bwe_weights",
]
