"""Text-side per-prompt path behind the reference's API (LTX_2_MLX/model/text_encoder/encoder.py:13-32 output records,
:65-253 VideoGemmaTextEncoderModel, :255-370 AudioVideoGemmaTextEncoderModel, :373-413 create_text_encoder,
:415-560 load_text_encoder_weights, :717-913 the LTX-2.3 "V2" encoder: create_av_text_encoder_v2, ..._from_checkpoint,
load_av_text_encoder_v2_weights).  Gemma itself is gemma3.py; the entry points here take its hidden states
(`encode_from_hidden_states`) or already-projected features (`encode_projected`).  The caption projection
3840 -> 4096 stays in the transformer (`ltx2_dit_prepare`), as in the reference."""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .connector import Embeddings1DConnector
from .feature_extractor import GemmaFeaturesExtractorProjLinear, GemmaFeaturesExtractorV2

CONNECTOR_PREFIX = "model.diffusion_model.video_embeddings_connector."
AUDIO_CONNECTOR_PREFIX = "model.diffusion_model.audio_embeddings_connector."
FEATURE_EXTRACTOR_PREFIX = "text_embedding_projection."


@dataclass
class VideoGemmaEncoderOutput:
    video_encoding: torch.Tensor       # [B, T, D]
    attention_mask: torch.Tensor       # [B, T]


@dataclass
class AudioVideoGemmaEncoderOutput:
    video_encoding: torch.Tensor
    audio_encoding: torch.Tensor
    attention_mask: torch.Tensor


def _additive_mask(attention_mask: torch.Tensor) -> torch.Tensor:
    """binary [B, T] (1 = attend) -> additive [B,1,1,T] (encoder.py:103-134)."""
    am = attention_mask.float()
    return ((am - 1) * 3.40e38).reshape(am.shape[0], 1, 1, am.shape[-1])


def _binary_mask(output_mask: torch.Tensor) -> torch.Tensor:
    return (output_mask.squeeze(1).squeeze(1) >= -0.5).to(torch.int32)


class VideoGemmaTextEncoderModel:
    def __init__(self, feature_extractor: Optional[GemmaFeaturesExtractorProjLinear] = None,
                 embeddings_connector: Optional[Embeddings1DConnector] = None):
        self.feature_extractor = feature_extractor or GemmaFeaturesExtractorProjLinear()
        self.embeddings_connector = embeddings_connector or Embeddings1DConnector()

    def encode_projected(self, projected_features: torch.Tensor, attention_mask: torch.Tensor) -> VideoGemmaEncoderOutput:
        encoded, output_mask = self.embeddings_connector(projected_features, _additive_mask(attention_mask).to(projected_features.device))
        binary = _binary_mask(output_mask)
        return VideoGemmaEncoderOutput(video_encoding=encoded * binary[:, :, None], attention_mask=binary)

    def encode_from_hidden_states(self, hidden_states: List[torch.Tensor], attention_mask: torch.Tensor,
                                  padding_side: str = "left") -> VideoGemmaEncoderOutput:
        feats = self.feature_extractor.extract_from_hidden_states(hidden_states=hidden_states, attention_mask=attention_mask,
                                                                  padding_side=padding_side)
        return self.encode_projected(feats, attention_mask)

    __call__ = encode_from_hidden_states


class AudioVideoGemmaTextEncoderModel:
    def __init__(self, feature_extractor=None, embeddings_connector: Optional[Embeddings1DConnector] = None,
                 audio_embeddings_connector: Optional[Embeddings1DConnector] = None):
        self.feature_extractor = feature_extractor or GemmaFeaturesExtractorProjLinear()
        self.embeddings_connector = embeddings_connector or Embeddings1DConnector()
        self.audio_embeddings_connector = audio_embeddings_connector or Embeddings1DConnector()

    def encode_from_hidden_states(self, hidden_states: List[torch.Tensor], attention_mask: torch.Tensor,
                                  padding_side: str = "left") -> AudioVideoGemmaEncoderOutput:
        feats = self.feature_extractor.extract_from_hidden_states(hidden_states=hidden_states, attention_mask=attention_mask,
                                                                  padding_side=padding_side)
        video_in, audio_in = feats if isinstance(self.feature_extractor, GemmaFeaturesExtractorV2) else (feats, feats)
        add = _additive_mask(attention_mask).to(video_in.device)
        video, output_mask = self.embeddings_connector(video_in, add)
        binary = _binary_mask(output_mask)
        audio, _ = self.audio_embeddings_connector(audio_in, add)
        return AudioVideoGemmaEncoderOutput(video_encoding=video * binary[:, :, None], audio_encoding=audio, attention_mask=binary)

    __call__ = encode_from_hidden_states


def create_text_encoder(hidden_dim: int = 3840, num_gemma_layers: int = 49, connector_heads: int = 30, connector_head_dim: int = 128,
                        connector_layers: int = 2, num_registers: int = 128, device="cuda") -> VideoGemmaTextEncoderModel:
    return VideoGemmaTextEncoderModel(
        feature_extractor=GemmaFeaturesExtractorProjLinear(hidden_dim=hidden_dim, num_layers=num_gemma_layers, device=device),
        embeddings_connector=Embeddings1DConnector(attention_head_dim=connector_head_dim, num_attention_heads=connector_heads,
                                                   num_layers=connector_layers, num_learnable_registers=num_registers, device=device))


def _strip(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def load_text_encoder_weights(encoder, weights_path: str) -> int:
    """Feature extractor (`text_embedding_projection.*`) and connector(s) (`model.diffusion_model.video_embeddings_connector.*`,
    `…audio_embeddings_connector.*` for the AV encoder) from the LTX-2 safetensors checkpoint (reference
    encoder.py:415-560).  Caption-projection weights belong to the transformer and are not read here.  Returns the number
    of tensors consumed."""
    from safetensors import safe_open
    want = (FEATURE_EXTRACTOR_PREFIX, CONNECTOR_PREFIX, AUDIO_CONNECTOR_PREFIX)
    sd: Dict[str, torch.Tensor] = {}
    with safe_open(weights_path, framework="pt") as f:
        for k in f.keys():
            if k.startswith(want):
                sd[k] = f.get_tensor(k)
    n = 0
    fe = _strip(sd, FEATURE_EXTRACTOR_PREFIX)
    if fe:
        encoder.feature_extractor.load_state_dict(fe)
        n += len(fe)
    conn = _strip(sd, CONNECTOR_PREFIX)
    if conn:
        encoder.embeddings_connector.load_state_dict(conn)
        n += len(conn)
    aconn = _strip(sd, AUDIO_CONNECTOR_PREFIX)
    if aconn and hasattr(encoder, "audio_embeddings_connector"):
        encoder.audio_embeddings_connector.load_state_dict(aconn)
        n += len(aconn)
    if n == 0:
        raise KeyError(f"no text-encoder tensors under {want} in {weights_path}")
    return n


# ---------------------------------------------------------------------------------------------------------------- LTX-2.3 ("V2")
def _read_transformer_config_from_checkpoint(weights_path: str) -> dict:
    """The `transformer` record of the safetensors metadata's JSON `config`; {} when absent or unreadable (encoder.py:717-729)."""
    from safetensors import safe_open
    try:
        with safe_open(weights_path, framework="pt") as f:
            metadata = f.metadata() or {}
        config = json.loads(metadata.get("config", "{}"))
    except Exception:
        return {}
    transformer_config = config.get("transformer", {}) if isinstance(config, dict) else {}
    return transformer_config if isinstance(transformer_config, dict) else {}


def _parse_rope_type(value) -> str:
    """"split" / "interleaved" (a string in any case, or an enum with such a value); anything else is interleaved (encoder.py:732-740)."""
    value = getattr(value, "value", value)
    if isinstance(value, str) and value.strip().lower() in ("split", "interleaved"):
        return value.strip().lower()
    return "interleaved"


def _normalize_positional_embedding_max_pos(value) -> List[int]:
    """A non-empty int list: None -> [1], a number -> [int], a non-empty list -> ints, anything else -> [1] (encoder.py:743-751)."""
    if value is None:
        return [1]
    if isinstance(value, (int, float)):
        return [int(value)]
    if isinstance(value, (list, tuple)) and value:
        return [int(v) for v in value]
    return [1]


def create_av_text_encoder_v2(hidden_dim: int = 3840, num_gemma_layers: int = 49, video_inner_dim: int = 4096, audio_inner_dim: int = 2048,
                              video_connector_heads: int = 32, video_connector_head_dim: int = 128, audio_connector_heads: int = 32,
                              audio_connector_head_dim: int = 64, connector_layers: int = 8, num_registers: int = 128,
                              positional_embedding_max_pos: Optional[List[int]] = None, rope_type="interleaved",
                              connector_apply_gated_attention: bool = True, double_precision_rope: bool = False,
                              device="cuda") -> AudioVideoGemmaTextEncoderModel:
    """The LTX-2.3 text encoder (encoder.py:754-808): per-token RMS feature extractor with one biased projection per modality, straight
    to the transformer widths, and one connector per modality."""
    def connector(heads, head_dim):
        return Embeddings1DConnector(attention_head_dim=head_dim, num_attention_heads=heads, num_layers=connector_layers,
                                     num_learnable_registers=num_registers, positional_embedding_max_pos=positional_embedding_max_pos,
                                     rope_type=rope_type, apply_gated_attention=connector_apply_gated_attention,
                                     double_precision_rope=double_precision_rope, device=device)
    return AudioVideoGemmaTextEncoderModel(
        feature_extractor=GemmaFeaturesExtractorV2(hidden_dim=hidden_dim, num_layers=num_gemma_layers, video_inner_dim=video_inner_dim,
                                                   audio_inner_dim=audio_inner_dim, device=device),
        embeddings_connector=connector(video_connector_heads, video_connector_head_dim),
        audio_embeddings_connector=connector(audio_connector_heads, audio_connector_head_dim))


def create_av_text_encoder_v2_from_checkpoint(weights_path: str, hidden_dim: int = 3840, num_gemma_layers: int = 49, video_inner_dim: int = 4096,
                                              audio_inner_dim: int = 2048, num_registers: int = 128,
                                              device="cuda") -> AudioVideoGemmaTextEncoderModel:
    """create_av_text_encoder_v2 with the connector settings of the checkpoint's metadata (encoder.py:811-871)."""
    cfg = _read_transformer_config_from_checkpoint(weights_path)
    video_heads = int(cfg.get("connector_num_attention_heads", 32))
    video_head_dim = int(cfg.get("connector_attention_head_dim", 128))
    layers = int(cfg.get("connector_num_layers", 8))
    audio_heads = int(cfg.get("audio_connector_num_attention_heads", video_heads))
    audio_head_dim = int(cfg.get("audio_connector_attention_head_dim", 64))
    max_pos = _normalize_positional_embedding_max_pos(cfg.get("connector_positional_embedding_max_pos"))
    rope_type = _parse_rope_type(cfg.get("rope_type", cfg.get("split_rope")))
    gated = bool(cfg.get("connector_apply_gated_attention", True))
    double_precision_rope = cfg.get("frequencies_precision", "") == "float64"
    print("  AV text encoder config: "
          f"video_heads={video_heads}x{video_head_dim}, audio_heads={audio_heads}x{audio_head_dim}, layers={layers}, rope={rope_type}, "
          f"max_pos={max_pos}, gated={'on' if gated else 'off'}, double_precision_rope={'on' if double_precision_rope else 'off'}")
    return create_av_text_encoder_v2(hidden_dim=hidden_dim, num_gemma_layers=num_gemma_layers, video_inner_dim=video_inner_dim,
                                     audio_inner_dim=audio_inner_dim, video_connector_heads=video_heads, video_connector_head_dim=video_head_dim,
                                     audio_connector_heads=audio_heads, audio_connector_head_dim=audio_head_dim, connector_layers=layers,
                                     num_registers=num_registers, positional_embedding_max_pos=max_pos, rope_type=rope_type,
                                     connector_apply_gated_attention=gated, double_precision_rope=double_precision_rope, device=device)


V2_FEATURE_EXTRACTOR_KEYS = tuple(f"{FEATURE_EXTRACTOR_PREFIX}{n}.{p}" for n in ("video_aggregate_embed", "audio_aggregate_embed")
                                  for p in ("weight", "bias"))


def load_av_text_encoder_v2_weights(encoder: AudioVideoGemmaTextEncoderModel, weights_path: str) -> int:
    """`text_embedding_projection.{video,audio}_aggregate_embed.{weight,bias}` and both connectors from an LTX-2.3 checkpoint
    (encoder.py:874-913).  Nothing else is read: `caption_projection.*` and the DiT's own tensors stay where they are.  Returns the
    number of tensors consumed; KeyError when the checkpoint holds none of them."""
    from safetensors import safe_open
    print(f"Loading AV text encoder V2 weights from {weights_path}...")
    want = (FEATURE_EXTRACTOR_PREFIX, CONNECTOR_PREFIX, AUDIO_CONNECTOR_PREFIX)
    fe: Dict[str, torch.Tensor] = {}
    conn: Dict[str, torch.Tensor] = {}
    aconn: Dict[str, torch.Tensor] = {}
    with safe_open(weights_path, framework="pt") as f:
        for k in f.keys():
            if k in V2_FEATURE_EXTRACTOR_KEYS:
                fe[k[len(FEATURE_EXTRACTOR_PREFIX):]] = f.get_tensor(k)
            elif k.startswith(CONNECTOR_PREFIX):
                conn[k[len(CONNECTOR_PREFIX):]] = f.get_tensor(k)
            elif k.startswith(AUDIO_CONNECTOR_PREFIX):
                aconn[k[len(AUDIO_CONNECTOR_PREFIX):]] = f.get_tensor(k)
    n = len(fe) + len(conn) + len(aconn)
    if n == 0:
        raise KeyError(f"no V2 text-encoder tensors under {want} in {weights_path}")
    if fe:
        encoder.feature_extractor.load_state_dict(fe)
    if conn:
        encoder.embeddings_connector.load_state_dict(conn)
    if aconn:
        encoder.audio_embeddings_connector.load_state_dict(aconn)
    print(f"  Loaded {n} AV text encoder V2 weight tensors")
    return n
