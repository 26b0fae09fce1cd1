"""Generate tests/golden/gemma3_tiny.npz by executing the REFERENCE'S OWN Gemma-3 (LTX_2_MLX/model/text_encoder/gemma3.py) through the
throw-away mlx->torch shim (tools/mlx_shim.py), on the seeded weights of tests/gemma3_ref.py.  Needs a checkout of the reference
(the directory that holds LTX_2_MLX/); the GPU is not used:

    python tools/pin_gemma_against_reference.py REFERENCE_DIR

The shim lacks a few pieces this model needs; they are patched in HERE (the shim itself, and the eight fixtures it pins, stay as they are):
a real nn.Embedding, mx.tril / mx.split / `&` on arrays, boolean masks in SDPA (where-masking, not addition), and the Metal
kernel silu_mul, restated as silu(a) * b.  Only inputs, the valid rows' hidden states and the config are stored.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "LTX_2_MLX")):
    sys.exit("usage: python tools/pin_gemma_against_reference.py REFERENCE_DIR   (the directory that holds LTX_2_MLX/)")
REFERENCE = os.path.abspath(sys.argv[1])
sys.path.insert(0, REFERENCE)

from tools import mlx_shim as shim  # noqa: E402

mx, nn = shim.install()
A = shim.Arr

# ---- the pieces the shim lacks
mx.tril = lambda a, k=0: A(torch.tril(shim._t(a), diagonal=k))
mx.split = lambda a, n, axis=0: [A(t) for t in torch.chunk(shim._t(a), n, dim=axis)]
A.__and__ = lambda a, b: A(torch.logical_and(shim._t(a), shim._t(b)))


class Embedding(shim.Module):
    def __init__(self, num_embeddings, dims):
        self.weight = mx.zeros((num_embeddings, dims))

    def __call__(self, ids):
        return A(F.embedding(shim._t(ids).long(), shim._t(self.weight)))


nn.Embedding = Embedding


def _sdpa(q, k, v, scale=None, mask=None):
    q, k, v = shim._t(q), shim._t(k), shim._t(v)
    s = (q @ k.transpose(-1, -2)) * (scale if scale is not None else q.shape[-1] ** -0.5)
    if mask is not None:
        m = shim._t(mask)
        s = s.masked_fill(~m, float("-inf")) if m.dtype == torch.bool else s + m
    return A(torch.nan_to_num(torch.softmax(s.float(), dim=-1), nan=0.0).to(q.dtype) @ v)


mx.fast.scaled_dot_product_attention = _sdpa

import types  # noqa: E402

kern = types.ModuleType("LTX_2_MLX.kernels")
kern.silu_mul = lambda a, b: A(F.silu(shim._t(a)) * shim._t(b))
sys.modules["LTX_2_MLX.kernels"] = kern

import importlib.util  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gemma3", os.path.join(REFERENCE, "LTX_2_MLX", "model", "text_encoder", "gemma3.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

import gemma3_ref  # noqa: E402

# tiny config: head_dim 256 (the kernel's), 4 / 2 heads, hidden 256, intermediate 512, 6 layers (layer 5 = full attention), window 24,
# T = 64 with 40 valid tokens left-padded (the window binds)
TINY = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=6, num_attention_heads=4, num_key_value_heads=2,
            head_dim=256, sliding_window=24)
T, VALID, SEED = 64, 40, 1234


def main():
    cfg = ref.Gemma3Config(**TINY, layer_types=["sliding_attention" if (i % 6 != 5) else "full_attention" for i in range(6)])
    w = gemma3_ref.make_gemma3_weights(cfg, SEED)
    model = ref.Gemma3Model(cfg)
    model.embed_tokens.weight = A(w["embed_tokens.weight"].clone())
    model.norm.weight = A(w["norm.weight"].clone())
    for i, layer in enumerate(model.layers):
        for name in gemma3_ref.LAYER_TENSORS:
            obj = layer
            parts = name.split(".")
            for p in parts[:-1]:
                obj = getattr(obj, p)
            setattr(obj, parts[-1], A(w[f"layers.{i}.{name}"].clone()))
    g = torch.Generator().manual_seed(SEED + 1)
    ids = torch.randint(1, TINY["vocab_size"], (1, T), generator=g)
    ids[:, :T - VALID] = 0
    mask = torch.zeros(1, T, dtype=torch.int64)
    mask[:, T - VALID:] = 1
    _, states = model(A(ids), attention_mask=A(mask))
    hs = np.stack([np.asarray(shim._t(s)[0, T - VALID:], dtype=np.float32) for s in states])       # [L + 1, VALID, D]
    out = os.path.join(ROOT, "tests", "golden", "gemma3_tiny.npz")
    np.savez_compressed(out, input_ids=ids.numpy().astype(np.int32), attention_mask=mask.numpy().astype(np.int32), hidden_states=hs,
                        seed=np.int64(SEED), config=np.array([TINY[k] for k in sorted(TINY)], dtype=np.int64),
                        config_keys=np.array(sorted(TINY)))
    print(f"wrote {out}: hidden_states {hs.shape}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
