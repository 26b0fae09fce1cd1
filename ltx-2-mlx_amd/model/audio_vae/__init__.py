"""Audio VAE on the MI355X (reference LTX_2_MLX/model/audio_vae/), fp32 HIP kernels (csrc/audio.hip): the decoder + vocoders
(latent -> log-mel -> waveform), the encoder (log-mel -> latent: AudioEncoder, load_audio_encoder_weights, encode_audio) and, beyond the
reference, the waveform -> log-mel front end the encoder needs (AudioProcessor, load_audio_file)."""
from .decoder import AudioDecoder, PerChannelStatistics, load_audio_decoder_weights
from .encoder import AudioEncoder, encode_audio, load_audio_encoder_weights
from .processor import AudioProcessor, load_audio_file
from .vocoder import MelSTFT, Vocoder, VocoderWithBWE, load_vocoder_weights, load_vocoder_with_bwe_weights

__all__ = [
    "AudioDecoder",
    "AudioEncoder",
    "AudioProcessor",
    "PerChannelStatistics",
    "MelSTFT",
    "Vocoder",
    "VocoderWithBWE",
    "encode_audio",
    "load_audio_decoder_weights",
    "load_audio_encoder_weights",
    "load_audio_file",
    "load_vocoder_weights",
    "load_vocoder_with_bwe_weights",
]
