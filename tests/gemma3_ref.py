"""fp32 PyTorch restatement of the reference's Gemma-3 text encoder (LTX_2_MLX/model/text_encoder/gemma3.py) -- the checker of
ltx_2_mlx_amd.model.text_encoder.gemma3, runnable on the CPU or, for the production-width tests, on the GPU -- plus a seeded weight
maker.  Line numbers cite the reference file.  Not part of the product (and not under oracle/, which stays as it is)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

LAYER_TENSORS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                 "self_attn.q_norm.weight", "self_attn.k_norm.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight",
                 "input_layernorm.weight", "post_attention_layernorm.weight", "pre_feedforward_layernorm.weight",
                 "post_feedforward_layernorm.weight")


def make_gemma3_weights(cfg, seed: int = 0, norm_scale: float = 0.5, device="cpu") -> Dict[str, torch.Tensor]:
    """Seeded fp32 weights under the HF names without prefix.  Projections ~ N(0, 1 / fan_in); norm weights ~ norm_scale * N(0, 1)
    (the (1 + w) form makes w = 0 the identity); embedding ~ N(0, 1) / sqrt(hidden), so embedding * sqrt(hidden) is O(1).
    device="cuda" draws them on the GPU (production width: 11 G parameters)."""
    g = torch.Generator(device=device).manual_seed(seed)
    d, hd, h, hkv, inter = cfg.hidden_size, cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.intermediate_size

    def lin(o, i):
        return torch.randn(o, i, generator=g, device=device) / math.sqrt(i)

    def nrm(n):
        return norm_scale * torch.randn(n, generator=g, device=device)

    w = {"embed_tokens.weight": torch.randn(cfg.vocab_size, d, generator=g, device=device) / math.sqrt(d)}
    for i in range(cfg.num_hidden_layers):
        p = f"layers.{i}."
        w[p + "self_attn.q_proj.weight"] = lin(h * hd, d)
        w[p + "self_attn.k_proj.weight"] = lin(hkv * hd, d)
        w[p + "self_attn.v_proj.weight"] = lin(hkv * hd, d)
        w[p + "self_attn.o_proj.weight"] = lin(d, h * hd)
        w[p + "self_attn.q_norm.weight"] = nrm(hd)
        w[p + "self_attn.k_norm.weight"] = nrm(hd)
        w[p + "mlp.gate_proj.weight"] = lin(inter, d)
        w[p + "mlp.up_proj.weight"] = lin(inter, d)
        w[p + "mlp.down_proj.weight"] = lin(d, inter)
        for t in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            w[p + t + ".weight"] = nrm(d)
    w["norm.weight"] = nrm(d)
    return w


def rms_norm(x, w, eps):
    """rms_norm(x) * (1 + w) (:58-63)."""
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (1 + w)


def rope(x, positions, theta, factor):
    """rotate-half RoPE (:79-138): positions / factor, inv_freq over head_dim, halves [0, hd/2) and [hd/2, hd)."""
    hd = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64, device=x.device) / hd))
    f = (positions.to(torch.float64)[:, None] / factor) * inv[None, :]
    cos, sin = torch.cos(f).float(), torch.sin(f).float()
    x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def act(x, kind):
    """the MLP's gate activation: the reference's silu_mul (:244-255) or the checkpoints' gelu_pytorch_tanh."""
    return F.silu(x) if kind == "silu" else F.gelu(x, approximate="tanh")


def forward(input_ids: torch.Tensor, w: Dict[str, torch.Tensor], cfg, attention_mask: Optional[torch.Tensor] = None,
            positions: Optional[torch.Tensor] = None, activation: Optional[str] = None) -> List[torch.Tensor]:
    """input_ids [B, T] -> the 49 (L + 1) hidden states [B, T, D] fp32 (:320-406).  A query row whose keys are all masked (a padded
    row of a left-padded prompt) gets zero attention output; valid rows never see padded keys, so they are unaffected."""
    dev = w["norm.weight"].device
    kind = activation or getattr(cfg, "hidden_activation", "silu")
    b, t = input_ids.shape
    d, hd, h, hkv = cfg.hidden_size, cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads
    eps = cfg.rms_norm_eps
    pos = torch.arange(t, device=dev) if positions is None else positions.to(dev)          # arange over the padded sequence (:338-341)
    x = F.embedding(input_ids.to(dev), w["embed_tokens.weight"]) * torch.tensor(d ** 0.5, dtype=torch.float32)   # (:312, :352)
    full = slide = None
    if attention_mask is not None:                                                       # boolean masks (:362-382)
        causal = torch.tril(torch.ones(t, t, dtype=torch.bool, device=dev))
        pad = attention_mask.to(dev).bool()[:, None, None, :]
        full = causal[None, None] & pad
        i = torch.arange(t, device=dev)
        slide = full & ((i[:, None] - i[None, :]) < cfg.sliding_window)[None, None]
    states = []
    for li in range(cfg.num_hidden_layers):
        states.append(x)                                                                 # hidden state BEFORE each layer (:391-393)
        p = f"layers.{li}."
        sliding = cfg.layer_types[li] == "sliding_attention"
        theta = cfg.sliding_rope_theta if sliding else cfg.full_rope_theta
        factor = cfg.sliding_rope_scaling_factor if sliding else cfg.full_rope_scaling_factor
        r = x
        y = rms_norm(x, w[p + "input_layernorm.weight"], eps)
        q = (y @ w[p + "self_attn.q_proj.weight"].T).reshape(b, t, h, hd)
        k = (y @ w[p + "self_attn.k_proj.weight"].T).reshape(b, t, hkv, hd)
        v = (y @ w[p + "self_attn.v_proj.weight"].T).reshape(b, t, hkv, hd)
        q = rms_norm(q, w[p + "self_attn.q_norm.weight"], eps).transpose(1, 2)           # per-head norms before RoPE (:206-210)
        k = rms_norm(k, w[p + "self_attn.k_norm.weight"], eps).transpose(1, 2)
        v = v.transpose(1, 2)
        q, k = rope(q, pos, theta, factor), rope(k, pos, theta, factor)
        k = torch.repeat_interleave(k, h // hkv, dim=1)                                   # mx.repeat: query head i reads kv head i // 2 (:228-229)
        v = torch.repeat_interleave(v, h // hkv, dim=1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        m = slide if sliding else full
        if m is not None:
            s = s.masked_fill(~m, float("-inf"))
        pr = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
        o = (pr @ v).transpose(1, 2).reshape(b, t, h * hd) @ w[p + "self_attn.o_proj.weight"].T
        x = r + rms_norm(o, w[p + "post_attention_layernorm.weight"], eps)              # (:276-281)
        r = x
        y = rms_norm(x, w[p + "pre_feedforward_layernorm.weight"], eps)
        y = (act(y @ w[p + "mlp.gate_proj.weight"].T, kind) * (y @ w[p + "mlp.up_proj.weight"].T)) @ w[p + "mlp.down_proj.weight"].T
        x = r + rms_norm(y, w[p + "post_feedforward_layernorm.weight"], eps)             # (:283-290)
    states.append(rms_norm(x, w["norm.weight"], eps))                                    # final norm, appended (:396-404)
    return states


def bf16_weights(w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The weights as the kernels hold them: matrices and the embedding rounded to bf16, norm vectors fp32."""
    return {k: (v.to(torch.bfloat16).float() if v.dim() == 2 else v) for k, v in w.items()}


def round_bf16_(w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """bf16_weights in place (no second copy of a production-width set)."""
    for v in w.values():
        if v.dim() == 2:
            v.copy_(v.to(torch.bfloat16))
    return w


def write_wordlevel_tokenizer(path, words, with_pad=False):
    """A WordLevel tokenizer with a Gemma-like special set (<pad> optional, <eos>, <bos>, <unk>; <bos> prepended to every prompt),
    saved in the HF layout: the tokenizer path of the encoder without the 262k-entry Gemma vocabulary."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    specials = (["<pad>"] if with_pad else []) + ["<eos>", "<bos>", "<unk>"]
    vocab = {w: i for i, w in enumerate(specials + list(words))}
    tk = Tokenizer(models.WordLevel(vocab=vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    tk.post_processor = processors.TemplateProcessing(single="<bos> $A", special_tokens=[("<bos>", vocab["<bos>"])])
    kw = dict(tokenizer_object=tk, eos_token="<eos>", bos_token="<bos>", unk_token="<unk>")
    if with_pad:
        kw["pad_token"] = "<pad>"
    PreTrainedTokenizerFast(**kw).save_pretrained(str(path))
    return vocab


def write_gemma_checkpoint(path, cfg, w, shards: int = 2, prefix: str = "language_model.model."):
    """config.json (HF text_config form) + `model-0000i-of-0000n.safetensors` shards of the weights `w` (bf16) under `prefix`."""
    import json
    import os
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    tc = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
              num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
              head_dim=cfg.head_dim, sliding_window=cfg.sliding_window, layer_types=cfg.layer_types, rope_theta=cfg.full_rope_theta,
              rope_local_base_freq=cfg.sliding_rope_theta, rope_scaling={"rope_type": "linear", "factor": cfg.full_rope_scaling_factor})
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "gemma3", "text_config": tc}, f)
    keys = sorted(w)
    for i in range(shards):
        part = {prefix + k: w[k].to(torch.bfloat16).cpu().contiguous() for k in keys[i::shards]}
        save_file(part, os.path.join(path, f"model-{i + 1:05d}-of-{shards:05d}.safetensors"))
