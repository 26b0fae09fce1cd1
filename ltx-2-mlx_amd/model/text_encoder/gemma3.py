"""Gemma-3 12B as LTX-2's text encoder: prefill only, all hidden states out, on the MI355X kernels.

Keeps the reference's names (LTX_2_MLX/model/text_encoder/gemma3.py: Gemma3Config :36-55, Gemma3Model :296-406,
load_gemma3_weights :409-520, create_gemma3_model :523-540) so a caller switches imports.  Semantics followed:

* layer i is full attention when i % 6 == 5, sliding otherwise (:30-33); sliding layers: window 1024, RoPE theta 1e4, no scaling;
  full layers: theta 1e6, positions / 8 (:79-114); RoPE in rotate-half form over head_dim 256 (:117-138);
* RMSNorm = rms_norm(x) * (1 + w), eps 1e-6 (:58-63), four per layer: x += post_attn(attn(input(x))), x += post_ff(mlp(pre_ff(x)))
  (:258-293); per-head q_norm / k_norm before RoPE (:206-210); GQA: query head h reads kv head h // (heads / kv_heads) (:228-229);
  scale 256 ** -0.5;
* masks (:362-382): causal and key not padding, sliding layers also (i - j) < window; attention_mask=None means NO mask (bidirectional);
* embedding * sqrt(hidden) with the scale in fp32 (:312, :352), positions arange(T) over the padded sequence (:338-341);
* hidden states [embedding, out(layer 0) ... out(layer L-2), final_norm(out(layer L-1))] (:388-406);
* MLP down(act(gate(x)) * up(x)) (:244-255).  The reference's act is SiLU; the released checkpoints were trained with
  gelu_pytorch_tanh (HF Gemma3TextConfig.hidden_activation).  The default here is the reference's SiLU, for parity;
  Gemma3Config.hidden_activation = "gelu_pytorch_tanh" selects the other.

Only the real tokens are computed: with left padding a valid row never reads a padded one (padded keys are masked), so the forward
runs the contiguous run of valid rows alone, each at its ABSOLUTE position (RoPE), under plain causal + window masking.  Padded rows
of the returned hidden states are zero (the feature extractors mask them out).  A mask whose valid positions are not one contiguous
run is refused.

Gemma runs on the bfloat16 library whatever the DiT's compute dtype: bf16 operands with an fp32 residual stream, HF's native
precision (the reference runs fp32 because fp16 overflows, scripts/generate.py:376-378).  Per layer: fused QKV GEMM ->
ltx2_gemma_qknorm_rope -> ltx2_gemma_attn -> o_proj GEMM -> ltx2_gemma_resid_norm (residual + next pre-norm) -> gate|up GEMM ->
ltx2_gemma_gated_act -> down GEMM -> ltx2_gemma_resid_norm, which writes the layer's output straight into its slot of the
[L + 1][T][hidden] fp32 hidden-state buffer.
"""
from __future__ import annotations

import glob
import json
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from ... import _native as nv
from ... import kernels as K

BF16 = torch.bfloat16
ACTIVATIONS = {"silu": nv.GEMMA_ACT_SILU, "gelu_pytorch_tanh": nv.GEMMA_ACT_GELU_TANH}


def default_layer_types(num_layers: int) -> List[str]:
    """Every 6th layer (5, 11, ...) is full attention (reference gemma3.py:30-33)."""
    return ["sliding_attention" if (i % 6 != 5) else "full_attention" for i in range(num_layers)]


GEMMA3_LAYER_TYPES = default_layer_types(48)


@dataclass
class Gemma3Config:
    """Gemma 3 12B text decoder (reference gemma3.py:36-55) plus `hidden_activation` ("silu" = the reference, default;
    "gelu_pytorch_tanh" = the checkpoints' own)."""
    vocab_size: int = 262208
    hidden_size: int = 3840
    intermediate_size: int = 15360
    num_hidden_layers: int = 48
    num_attention_heads: int = 16
    num_key_value_heads: int = 8
    head_dim: int = 256
    rms_norm_eps: float = 1e-6
    max_position_embeddings: int = 131072
    sliding_window: int = 1024
    sliding_rope_theta: float = 10000.0
    sliding_rope_scaling_factor: float = 1.0
    full_rope_theta: float = 1000000.0
    full_rope_scaling_factor: float = 8.0
    layer_types: Optional[List[str]] = None
    hidden_activation: str = "silu"

    def __post_init__(self):
        if self.layer_types is None:
            self.layer_types = default_layer_types(self.num_hidden_layers)
        if len(self.layer_types) != self.num_hidden_layers:
            raise ValueError(f"layer_types has {len(self.layer_types)} entries for {self.num_hidden_layers} layers")
        bad = [t for t in self.layer_types if t not in ("sliding_attention", "full_attention")]
        if bad:
            raise ValueError(f"unknown layer type {bad[0]!r}")
        if self.hidden_activation not in ACTIVATIONS:
            raise ValueError(f"hidden_activation {self.hidden_activation!r}: one of {sorted(ACTIVATIONS)}")

    @classmethod
    def from_dict(cls, d: dict, **overrides) -> "Gemma3Config":
        """An HF config.json (`text_config` of the multimodal checkpoint, or the top level of a text-only one): dimensions, layer types,
        window and RoPE parameters.  `hidden_activation` is NOT taken from the file (the reference's SiLU stays the default); pass it
        as an override."""
        tc = d.get("text_config", d)
        base = cls()
        kw = {}
        for name in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
                     "head_dim", "rms_norm_eps", "max_position_embeddings", "sliding_window"):
            if tc.get(name) is not None:
                kw[name] = type(getattr(base, name))(tc[name])
        n = kw.get("num_hidden_layers", base.num_hidden_layers)
        if tc.get("layer_types"):
            kw["layer_types"] = list(tc["layer_types"])
        elif tc.get("sliding_window_pattern"):
            p = int(tc["sliding_window_pattern"])
            kw["layer_types"] = ["sliding_attention" if (i + 1) % p else "full_attention" for i in range(n)]
        else:
            kw["layer_types"] = default_layer_types(n)
        rp = tc.get("rope_parameters")
        if isinstance(rp, dict) and ("full_attention" in rp or "sliding_attention" in rp):   # newer transformers: per layer type
            full, slide = rp.get("full_attention", {}), rp.get("sliding_attention", {})
            if "rope_theta" in full:
                kw["full_rope_theta"] = float(full["rope_theta"])
            kw["full_rope_scaling_factor"] = float(full.get("factor", 1.0)) if full.get("rope_type", "default") == "linear" else 1.0
            if "rope_theta" in slide:
                kw["sliding_rope_theta"] = float(slide["rope_theta"])
            kw["sliding_rope_scaling_factor"] = float(slide.get("factor", 1.0)) if slide.get("rope_type", "default") == "linear" else 1.0
        else:
            if tc.get("rope_theta") is not None:
                kw["full_rope_theta"] = float(tc["rope_theta"])
            if tc.get("rope_local_base_freq") is not None:
                kw["sliding_rope_theta"] = float(tc["rope_local_base_freq"])
            rs = tc.get("rope_scaling")
            if isinstance(rs, dict) and rs.get("rope_type", rs.get("type")) == "linear":
                kw["full_rope_scaling_factor"] = float(rs["factor"])
            elif "rope_scaling" in tc:
                kw["full_rope_scaling_factor"] = 1.0
        kw.update(overrides)
        return cls(**kw)

    @classmethod
    def from_pretrained(cls, path: str, **overrides) -> "Gemma3Config":
        """config.json of a checkpoint directory when present, else the defaults."""
        cfg = os.path.join(path, "config.json") if os.path.isdir(path) else path
        if os.path.isfile(cfg):
            with open(cfg) as f:
                return cls.from_dict(json.load(f), **overrides)
        return cls(**overrides)


def rope_cos_sin(positions: torch.Tensor, head_dim: int, theta: float, scaling_factor: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos, sin [T, head_dim / 2] of the rotate-half RoPE at absolute `positions` (reference gemma3.py:79-114), built on the host in
    float64 and returned as fp32."""
    inv_freq = 1.0 / (float(theta) ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    freqs = (positions.to(torch.float64).cpu() / float(scaling_factor))[:, None] * inv_freq[None, :]
    return torch.cos(freqs).float(), torch.sin(freqs).float()


def valid_run(attention_mask: torch.Tensor) -> Tuple[int, int]:
    """(start, count) of the one contiguous run of valid (non-zero) positions of a [T] mask; ValueError when they are not contiguous.
    Left-padded, right-padded and unpadded masks all qualify."""
    m = torch.as_tensor(attention_mask).reshape(-1).cpu() != 0
    idx = torch.nonzero(m).reshape(-1)
    if idx.numel() == 0:
        return 0, 0
    s, e = int(idx[0]), int(idx[-1]) + 1
    if e - s != idx.numel():
        raise ValueError(f"attention_mask: the valid positions must form one contiguous run (left, right or no padding); got "
                         f"{idx.numel()} valid positions spread over [{s}, {e})")
    return s, idx.numel()


LAYER_TENSORS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                 "self_attn.q_norm.weight", "self_attn.k_norm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight",
                 "input_layernorm.weight", "post_attention_layernorm.weight", "pre_feedforward_layernorm.weight",
                 "post_feedforward_layernorm.weight")


class Gemma3Model:
    """Gemma 3 decoder stack on the GPU; __call__ mirrors the reference's (last_hidden_state, all_hidden_states) return (:320-406).

    Weights: fused QKV [(H + 2 Hkv) * hd, hidden], o_proj, gate|up concatenated [2 * intermediate, hidden] and down_proj, all bf16;
    the embedding table bf16; norm weights fp32.  set_weight() / load_state_dict() take the HF names without prefix
    (`embed_tokens.weight`, `norm.weight`, `layers.{i}.self_attn.q_proj.weight`, ...)."""

    def __init__(self, config: Optional[Gemma3Config] = None, device: Union[str, torch.device] = "cuda"):
        self.config = config or Gemma3Config()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Gemma3Model runs on the MI355X only (no CPU fallback)")
        c = self.config
        if c.head_dim != 256:
            raise ValueError(f"head_dim {c.head_dim}: the attention kernel is built for head_dim 256 (Gemma 3)")
        if c.num_attention_heads % c.num_key_value_heads:
            raise ValueError(f"num_attention_heads {c.num_attention_heads} is not a multiple of num_key_value_heads {c.num_key_value_heads}")
        self.embed_scale = c.hidden_size ** 0.5
        self.act = ACTIVATIONS[c.hidden_activation]
        self._loaded: set = set()
        self._alloc()

    # ------------------------------------------------------------------------------------------------------------------ weights
    def _alloc(self):
        c, dev = self.config, self.device
        hd, h, hkv, d, inter = c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.hidden_size, c.intermediate_size
        e = lambda *s: torch.empty(*s, device=dev, dtype=BF16)          # noqa: E731
        f = lambda n: torch.empty(n, device=dev, dtype=torch.float32)   # noqa: E731
        self.embed_tokens = e(c.vocab_size, d)
        self.norm = f(d)
        self.layers = []
        for _ in range(c.num_hidden_layers):
            self.layers.append(dict(qkv=e((h + 2 * hkv) * hd, d), o=e(d, h * hd), gu=e(2 * inter, d), down=e(d, inter), q_norm=f(hd), k_norm=f(hd),
                                    input=f(d), post_attn=f(d), pre_ff=f(d), post_ff=f(d)))

    def required_weights(self) -> List[str]:
        return required_tensor_names(self.config)

    def _target(self, name: str) -> Tuple[torch.Tensor, tuple]:
        """(destination view, expected source shape) of a tensor name."""
        c = self.config
        hd, h, hkv, d, inter = c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.hidden_size, c.intermediate_size
        if name == "embed_tokens.weight":
            return self.embed_tokens, (c.vocab_size, d)
        if name == "norm.weight":
            return self.norm, (d,)
        parts = name.split(".", 2)
        if len(parts) == 3 and parts[0] == "layers" and parts[1].isdigit() and int(parts[1]) < c.num_hidden_layers:
            L, t = self.layers[int(parts[1])], parts[2]
            q0, k0, v0 = 0, h * hd, (h + hkv) * hd
            table = {"self_attn.q_proj.weight": (L["qkv"][q0:k0], (h * hd, d)), "self_attn.k_proj.weight": (L["qkv"][k0:v0], (hkv * hd, d)),
                     "self_attn.v_proj.weight": (L["qkv"][v0:], (hkv * hd, d)), "self_attn.o_proj.weight": (L["o"], (d, h * hd)),
                     "self_attn.q_norm.weight": (L["q_norm"], (hd,)), "self_attn.k_norm.weight": (L["k_norm"], (hd,)),
                     "mlp.gate_proj.weight": (L["gu"][:inter], (inter, d)), "mlp.up_proj.weight": (L["gu"][inter:], (inter, d)),
                     "mlp.down_proj.weight": (L["down"], (d, inter)), "input_layernorm.weight": (L["input"], (d,)),
                     "post_attention_layernorm.weight": (L["post_attn"], (d,)), "pre_feedforward_layernorm.weight": (L["pre_ff"], (d,)),
                     "post_feedforward_layernorm.weight": (L["post_ff"], (d,))}
            if t in table:
                return table[t]
        raise KeyError(f"unknown Gemma-3 tensor {name!r}")

    def set_weight(self, name: str, tensor: torch.Tensor) -> None:
        dst, shape = self._target(name)
        if tuple(tensor.shape) != shape:
            raise ValueError(f"{name}: shape {tuple(tensor.shape)} != {shape}")
        dst.copy_(tensor)               # straight into the fused device matrix: a bf16 file tensor goes to HBM as bf16
        self._loaded.add(name)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for k, v in sd.items():
            self.set_weight(k, v)
        self.check_loaded()

    def check_loaded(self) -> None:
        missing = [k for k in self.required_weights() if k not in self._loaded]
        if missing:
            raise KeyError(f"Gemma-3 weights missing: {missing[0]!r}" + (f" and {len(missing) - 1} more" if len(missing) > 1 else ""))

    def free(self) -> None:
        """Drop the weights (~23.5 GB at 12B) so the DiT can load (reference scripts/generate.py:631-640)."""
        self.embed_tokens = self.norm = None
        self.layers = []
        self._loaded = set()

    # ------------------------------------------------------------------------------------------------------------------ forward
    def _tables(self, positions: torch.Tensor) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        c = self.config
        out = {}
        for kind, theta, fac in (("sliding_attention", c.sliding_rope_theta, c.sliding_rope_scaling_factor),
                                 ("full_attention", c.full_rope_theta, c.full_rope_scaling_factor)):
            cos, sin = rope_cos_sin(positions, c.head_dim, theta, fac)
            out[kind] = (cos.to(self.device).contiguous(), sin.to(self.device).contiguous())
        return out

    def forward_rows(self, ids: torch.Tensor, positions: torch.Tensor, hidden: torch.Tensor, causal: bool = True) -> None:
        """Run the stack over n rows (int32 ids [n] on the GPU, absolute positions [n]); writes slots 0..L of `hidden`
        ([L + 1, n, D] fp32 view, row-contiguous)."""
        c = self.config
        if not self.layers or self.embed_tokens is None:
            raise RuntimeError("Gemma3Model: weights freed or never loaded")
        n, d = ids.shape[0], c.hidden_size
        if n == 0:
            return
        hd, h, hkv, inter = c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.intermediate_size
        tabs = self._tables(positions)
        K.gemma_embed(ids, self.embed_tokens, self.embed_scale, out=hidden[0])
        x_mid = torch.empty(n, d, device=self.device, dtype=torch.float32)
        hbuf = torch.empty(n, d, device=self.device, dtype=BF16)
        K.gemma_resid_norm(hidden[0], None, None, self.layers[0]["input"], h_out=hbuf, eps=c.rms_norm_eps)
        last = c.num_hidden_layers - 1
        for i, L in enumerate(self.layers):
            sliding = c.layer_types[i] == "sliding_attention"
            cos, sin = tabs[c.layer_types[i]]
            qkv = K.gemm(hbuf, L["qkv"])
            K.gemma_qknorm_rope_(qkv, h, hkv, L["q_norm"], L["k_norm"], cos, sin, eps=c.rms_norm_eps)
            att = K.gemma_attn(qkv[:, :h * hd], qkv[:, h * hd:(h + hkv) * hd], qkv[:, (h + hkv) * hd:], h, hkv, causal=causal,
                               window=c.sliding_window if (sliding and causal) else 0, scale=hd ** -0.5)
            y = K.gemm(att, L["o"])
            K.gemma_resid_norm(hidden[i], y, L["post_attn"], L["pre_ff"], x_out=x_mid, h_out=hbuf, eps=c.rms_norm_eps)
            a = K.gemma_gated_act(K.gemm(hbuf, L["gu"]), inter, self.act)
            y = K.gemm(a, L["down"])
            if i < last:
                K.gemma_resid_norm(x_mid, y, L["post_ff"], self.layers[i + 1]["input"], x_out=hidden[i + 1], h_out=hbuf, eps=c.rms_norm_eps)
            else:   # the list's last entry is final_norm(out(last layer)) (:396-406)
                K.gemma_resid_norm(x_mid, y, L["post_ff"], self.norm, hf_out=hidden[i + 1], eps=c.rms_norm_eps)

    def __call__(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                 output_hidden_states: bool = True) -> Tuple[torch.Tensor, Optional[List[torch.Tensor]]]:
        """input_ids [B, T] -> (final-normed last hidden state [B, T, D], [L + 1] hidden states [B, T, D] fp32 or None).
        attention_mask [B, T] (1 = real): causal + sliding window over the valid run; None: no mask at all (reference :362-382)."""
        c = self.config
        ids = torch.as_tensor(input_ids)
        if ids.dim() == 1:
            ids = ids[None]
        b, t = ids.shape
        if int(ids.min()) < 0 or int(ids.max()) >= c.vocab_size:
            raise ValueError(f"token id outside [0, {c.vocab_size})")
        pos_all = torch.arange(t) if position_ids is None else torch.as_tensor(position_ids).reshape(-1, t)[0].cpu()
        hidden = torch.zeros(b, c.num_hidden_layers + 1, t, c.hidden_size, device=self.device, dtype=torch.float32)
        for bi in range(b):
            if attention_mask is None:
                s, n, causal = 0, t, False
            else:
                s, n = valid_run(torch.as_tensor(attention_mask).reshape(b, t)[bi])
                causal = True
            rows = ids[bi, s:s + n].to(self.device, torch.int32).contiguous()
            self.forward_rows(rows, pos_all[s:s + n], hidden[bi, :, s:s + n], causal=causal)
        states = [hidden[:, l] for l in range(c.num_hidden_layers + 1)]
        return states[-1], (states if output_hidden_states else None)


def _shards(weights_dir: str) -> List[str]:
    files = sorted(glob.glob(os.path.join(weights_dir, "model-*.safetensors")))
    if not files:
        files = sorted(glob.glob(os.path.join(weights_dir, "model.safetensors")))
    return files


# checkpoint key prefixes of the text decoder: the multimodal checkpoint as the reference reads it (:455-520), the newer HF layout, and
# a text-only Gemma3ForCausalLM; tensors of the other towers are not the text encoder's and are skipped
TEXT_PREFIXES = ("language_model.model.", "model.language_model.", "model.")
OTHER_PREFIXES = ("vision_tower.", "multi_modal_projector.", "model.vision_tower.", "model.multi_modal_projector.", "lm_head.",
                  "language_model.lm_head.")


def checkpoint_key_to_name(key: str) -> Optional[str]:
    """Checkpoint key -> Gemma3Model tensor name; None for tensors of the other towers / the LM head."""
    if key.startswith(OTHER_PREFIXES):
        return None
    for p in TEXT_PREFIXES:
        if key.startswith(p):
            return key[len(p):]
    raise KeyError(f"unknown Gemma-3 checkpoint tensor {key!r}")


def required_tensor_names(config: Gemma3Config) -> List[str]:
    return ["embed_tokens.weight", "norm.weight"] + [f"layers.{i}.{t}" for i in range(config.num_hidden_layers) for t in LAYER_TENSORS]


def scan_gemma3_checkpoint(weights_dir: str, config: Gemma3Config) -> Dict[str, Tuple[str, str]]:
    """{model tensor name: (shard path, checkpoint key)} of a checkpoint directory, read from the shard headers only; raises FileNotFoundError
    without shards, KeyError naming an unknown or a missing tensor."""
    from safetensors import safe_open
    shards = _shards(weights_dir)
    if not shards:
        raise FileNotFoundError(f"No safetensors files found in {weights_dir}")
    found: Dict[str, Tuple[str, str]] = {}
    need = set(required_tensor_names(config))
    for path in shards:
        with safe_open(path, framework="pt") as f:
            for key in f.keys():
                name = checkpoint_key_to_name(key)
                if name is None:
                    continue
                if name not in need:
                    raise KeyError(f"unknown Gemma-3 checkpoint tensor {key!r} (config: {config.num_hidden_layers} layers)")
                found[name] = (path, key)
    missing = [n for n in required_tensor_names(config) if n not in found]
    if missing:
        raise KeyError(f"Gemma-3 checkpoint {weights_dir} lacks {missing[0]!r}" + (f" and {len(missing) - 1} more" if len(missing) > 1 else ""))
    return found


def load_gemma3_weights(model: Gemma3Model, weights_dir: str, use_fp16: bool = True) -> int:
    """Load `model-*.safetensors` shards (reference :409-520; keys `language_model.model.*` or text-only `model.*`).  q / k / v land in
    the fused QKV matrix and gate / up in the fused gate|up matrix as they are read; 16-bit tensors go to HBM without an fp32 copy.
    `use_fp16` is accepted for the reference's signature: the weights are bf16 on the GPU whatever it says.  A missing or unknown tensor
    raises with its name.  Returns the number of tensors loaded."""
    from safetensors import safe_open
    plan = scan_gemma3_checkpoint(weights_dir, model.config)       # every name checked before a byte moves
    by_shard: Dict[str, List[Tuple[str, str]]] = {}
    for name, (path, key) in plan.items():
        by_shard.setdefault(path, []).append((name, key))
    n = 0
    for path, items in by_shard.items():
        with safe_open(path, framework="pt") as f:
            for name, key in items:
                model.set_weight(name, f.get_tensor(key))
                n += 1
    model.check_loaded()
    torch.cuda.synchronize(model.device)
    return n


def create_gemma3_model(weights_dir: Optional[str] = None, device: Union[str, torch.device] = "cuda", hidden_activation: str = "silu",
                        config: Optional[Gemma3Config] = None) -> Gemma3Model:
    """Gemma3Model from `weights_dir`'s config.json (the defaults when absent), loaded from its shards when given (reference :523-540)."""
    if config is None:
        config = Gemma3Config.from_pretrained(weights_dir, hidden_activation=hidden_activation) if weights_dir else \
            Gemma3Config(hidden_activation=hidden_activation)
    model = Gemma3Model(config, device=device)
    if weights_dir:
        load_gemma3_weights(model, weights_dir)
    return model


# ---------------------------------------------------------------------------------------------------------------------- tokenizer
def load_gemma_tokenizer(gemma_path: str):
    """The checkpoint directory's tokenizer, from local files only (never the network), set up as the reference uses it
    (scripts/generate.py:368-372): left padding, pad token = EOS when the tokenizer has none."""
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(gemma_path, local_files_only=True)
    tok.padding_side = "left"
    if tok.pad_token is None:
        tok.pad_token = tok.eos_token
    return tok


def tokenize_prompt(tokenizer, prompt: str, max_length: int = 1024) -> Tuple[np.ndarray, np.ndarray]:
    """Raw prompt, no chat template; padding to max_length, truncation (scripts/generate.py:384-393).  -> (input_ids, attention_mask)
    int64 [1, max_length]."""
    enc = tokenizer(prompt, return_tensors="np", padding="max_length", truncation=True, max_length=max_length)
    return np.asarray(enc["input_ids"], dtype=np.int64), np.asarray(enc["attention_mask"], dtype=np.int64)


__all__ = ["Gemma3Config", "Gemma3Model", "GEMMA3_LAYER_TYPES", "load_gemma3_weights", "create_gemma3_model", "load_gemma_tokenizer",
           "tokenize_prompt", "rope_cos_sin", "valid_run", "checkpoint_key_to_name", "default_layer_types", "scan_gemma3_checkpoint"]
