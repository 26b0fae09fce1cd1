"""Gemma-3 12B encode timing on the MI355X: per-kernel times of one layer's ops and the whole 48-layer encode, at 1024 valid rows
(compute: fraction of the ~2.5 PF/s bf16 MFMA roof) and at 128 valid rows (weight stream: fraction of the 8 TB/s HBM peak for the
21.5 GB of layer weights).  Random weights (vocab 4096: the embedding table is not part of either figure).

    python tools/gemma_time.py [out.md]        (default profiles/gemma_encode.md)
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemma3_ref  # noqa: E402
from ltx_2_mlx_amd import kernels as K  # noqa: E402
from ltx_2_mlx_amd.model.text_encoder.gemma3 import Gemma3Config, Gemma3Model, rope_cos_sin  # noqa: E402

DEV = torch.device("cuda:0")
MFMA_ROOF = 2.5e15          # bf16 dense, spec
HBM_PEAK = 8.0e12           # spec; ~6.3e12 achievable (float4 copy)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def layer_ops(m, n):
    c = m.config
    hd, h, hkv, d, inter = c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.hidden_size, c.intermediate_size
    L = m.layers[0]
    x = torch.randn(n, d, device=DEV)
    hb = torch.randn(n, d, device=DEV).to(torch.bfloat16)
    qkv = K.gemm(hb, L["qkv"])
    cos, sin = (t.to(DEV) for t in rope_cos_sin(torch.arange(n), hd, 1e4, 1.0))
    att = torch.empty(n, h * hd, device=DEV, dtype=torch.bfloat16)
    gu = K.gemm(hb, L["gu"])
    a = K.gemma_gated_act(gu, inter, m.act)
    y = K.gemm(att, L["o"])
    xo = torch.empty_like(x)
    ops = [
        ("gemm qkv (N 8192, K 3840)", 48, lambda: K.gemm(hb, L["qkv"], out=qkv)),
        ("qknorm + rope", 48, lambda: K.gemma_qknorm_rope_(qkv, h, hkv, L["q_norm"], L["k_norm"], cos, sin)),
        ("attention, sliding (window 1024)", 40, lambda: K.gemma_attn(qkv[:, :h * hd], qkv[:, h * hd:(h + hkv) * hd], qkv[:, (h + hkv) * hd:], h, hkv,
                                                                       True, c.sliding_window, out=att)),
        ("attention, full", 8, lambda: K.gemma_attn(qkv[:, :h * hd], qkv[:, h * hd:(h + hkv) * hd], qkv[:, (h + hkv) * hd:], h, hkv, True, 0, out=att)),
        ("gemm o_proj (N 3840, K 4096)", 48, lambda: K.gemm(att, L["o"], out=y)),
        ("resid + norm (x2 per layer)", 96, lambda: K.gemma_resid_norm(x, y, L["post_attn"], L["pre_ff"], x_out=xo, h_out=hb)),
        ("gemm gate|up (N 30720, K 3840)", 48, lambda: K.gemm(hb, L["gu"], out=gu)),
        ("gated act", 48, lambda: K.gemma_gated_act(gu, inter, m.act, out=a)),
        ("gemm down (N 3840, K 15360)", 48, lambda: K.gemm(a, L["down"], out=y)),
    ]
    return [(name, cnt, timed(fn)) for name, cnt, fn in ops]


def main():
    out_md = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gemma_encode.md")
    cfg = Gemma3Config(vocab_size=4096)
    t0 = time.time()
    w = gemma3_ref.make_gemma3_weights(cfg, 0, device=DEV)
    m = Gemma3Model(cfg, device=DEV)
    m.load_state_dict(w)
    del w
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    print(f"random 48-layer Gemma built in {time.time() - t0:.1f} s")
    d, inter = cfg.hidden_size, cfg.intermediate_size
    gemm_mac_per_row = 8192 * d + d * 4096 + 2 * inter * d + d * inter
    weight_bytes = 2 * gemm_mac_per_row * cfg.num_hidden_layers
    lines = ["# Gemma-3 12B encode on one MI355X (bf16 operands, fp32 residual stream)", "",
             "Measured by `tools/gemma_time.py` (random weights, 48 layers, 3840 hidden, 16/8 x 256 heads, 15360 intermediate).",
             f"Layer weights streamed per encode: {weight_bytes / 1e9:.1f} GB.  Roofs: bf16 MFMA ~2.5 PF/s dense (spec), HBM 8 TB/s (spec; ~6.3 achievable).", ""]
    for n in (1024, 128):
        ids = torch.randint(0, cfg.vocab_size, (1, n))
        mask = torch.ones(1, n, dtype=torch.long)
        m(ids, attention_mask=mask)
        torch.cuda.synchronize()
        reps = 5
        t0 = time.time()
        for _ in range(reps):
            m(ids, attention_mask=mask)
        torch.cuda.synchronize()
        whole = (time.time() - t0) / reps
        gemm_flops = 2.0 * n * gemm_mac_per_row * cfg.num_hidden_layers
        attn_flops = sum(4.0 * cfg.num_attention_heads * cfg.head_dim * sum(min(i + 1, cfg.sliding_window if t == "sliding_attention" else n)
                                                                            for i in range(n)) for t in cfg.layer_types)
        ops = layer_ops(m, n)
        kern = sum(cnt * t for _, cnt, t in ops)
        lines += [f"## {n} valid rows", "", "| op | per launch (us) | launches | per encode (ms) |", "|---|---:|---:|---:|"]
        lines += [f"| {name} | {t * 1e6:.1f} | {cnt} | {cnt * t * 1e3:.2f} |" for name, cnt, t in ops]
        lines += ["", f"* whole encode (`Gemma3Model.__call__`, host included): **{whole * 1e3:.1f} ms**; sum of the kernels above {kern * 1e3:.1f} ms",
                  f"* GEMM flops {gemm_flops / 1e12:.1f} TFLOP + attention {attn_flops / 1e12:.2f} TFLOP: "
                  f"{(gemm_flops + attn_flops) / whole / 1e12:.0f} TF/s = **{(gemm_flops + attn_flops) / whole / MFMA_ROOF * 100:.1f} % of the bf16 MFMA roof**",
                  f"* weight stream {weight_bytes / 1e9:.1f} GB in {whole * 1e3:.1f} ms = {weight_bytes / whole / 1e12:.2f} TB/s = "
                  f"**{weight_bytes / whole / HBM_PEAK * 100:.1f} % of HBM peak**", ""]
        print(f"{n} rows: whole encode {whole * 1e3:.1f} ms, kernels {kern * 1e3:.1f} ms")
    os.makedirs(os.path.dirname(out_md), exist_ok=True)
    with open(out_md, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
