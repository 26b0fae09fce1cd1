"""For anyone with real Gemma-3 weights: the HIP encode against the fp32 restatement (tests/gemma3_ref.py) run on the GPU, on one prompt.
Prints rel-L2 and the minimum / mean per-token cosine of every hidden state, and of the final text encoding (feature extractor +
connector) when an LTX-2 checkpoint is given.  Not run in the test suite: no checkpoint of the real model is available there.

    python tools/gemma_compare.py GEMMA_DIR "a red fox runs through the snow" [--ltx-weights ltx2.safetensors] [--gelu]
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gemma3_ref  # noqa: E402
from ltx_2_mlx_amd.model.text_encoder.gemma3 import (create_gemma3_model, load_gemma_tokenizer, scan_gemma3_checkpoint,  # noqa: E402
                                                     tokenize_prompt)


def report(tag, got, ref, mask):
    g, r = got[0][mask], ref[0][mask]
    rel = float((g - r).double().norm() / r.double().norm())
    cos = F.cosine_similarity(g.double(), r.double(), dim=-1)
    print(f"{tag:>22}: rel-L2 {rel:.3e}   per-token cosine min {float(cos.min()):.6f} mean {float(cos.mean()):.6f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("gemma_dir")
    ap.add_argument("prompt")
    ap.add_argument("--ltx-weights", default=None)
    ap.add_argument("--gelu", action="store_true", help="hidden_activation gelu_pytorch_tanh (the checkpoints') instead of the reference's silu")
    ap.add_argument("--max-length", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    act = "gelu_pytorch_tanh" if a.gelu else "silu"
    tok = load_gemma_tokenizer(a.gemma_dir)
    ids, mask = tokenize_prompt(tok, a.prompt, a.max_length)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    m = create_gemma3_model(a.gemma_dir, device=dev, hidden_activation=act)
    cfg = m.config
    _, hip = m(ids, attention_mask=mask)
    hip = [h.cpu() for h in hip]
    m.free()
    torch.cuda.empty_cache()
    from safetensors import safe_open
    w = {}
    for name, (path, key) in scan_gemma3_checkpoint(a.gemma_dir, cfg).items():       # the weights as stored, in fp32, on the GPU
        with safe_open(path, framework="pt") as f:
            w[name] = f.get_tensor(key).to(dev, torch.float32)
    with torch.no_grad():
        ref = [h.cpu() for h in gemma3_ref.forward(ids, w, cfg, attention_mask=mask, activation=act)]
    del w
    torch.cuda.empty_cache()
    valid = mask[0].bool()
    print(f"{int(valid.sum())} valid tokens of {ids.shape[1]}; activation {act}")
    for i in (0, 1, len(hip) // 2, len(hip) - 2, len(hip) - 1):
        report(f"hidden state {i}", hip[i], ref[i], valid)
    if a.ltx_weights:
        import generate
        enc = generate._gemma_text_encoder(cfg, a.ltx_weights, dev)
        outs = [enc.encode_from_hidden_states([h.to(dev) for h in hs], mask.to(dev), padding_side="left") for hs in (hip, ref)]
        om = outs[1].attention_mask[0].bool().cpu()
        report("text encoding", outs[0].video_encoding.cpu(), outs[1].video_encoding.cpu(), om)


if __name__ == "__main__":
    main()
