"""Tensor-level wrappers over the per-kernel C-ABI entry points (counterpart of the reference's
LTX_2_MLX/kernels/ + the mx.fast.* / mx.conv2d leaf calls).  Used by the unit-parity tests and
by host glue; the full DiT step and VAE pass go through the engine calls instead
(ltx2_dit_* / ltx2_vae_*), which sequence the same kernels in C++.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _native as nv

BF16 = torch.bfloat16
F16 = torch.float16
ACT16 = (BF16, F16)         # the 16-bit activation / weight type: bfloat16 (libltx2hip.so) or IEEE half (libltx2hip_f16.so, -DLTX2_F16)


def _L(*tensors, dtype=None):
    """The library build for these tensors' 16-bit type (the first bf16 / f16 tensor decides; `dtype` when there is none)."""
    for t in tensors:
        if t is not None and t.dtype in ACT16:
            return nv.lib(t.dtype)
    return nv.lib(dtype)


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = nv.EPI_BF16,
         out: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
         gate_table: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T + bias).  a, w bf16; bias/gate fp32."""
    assert a.dtype in ACT16 and w.dtype == a.dtype and a.dim() == 2 and w.dim() == 2
    a, w = _c(a), _c(w)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        odt = torch.float32 if epilogue in (nv.EPI_F32, nv.EPI_RESID_GATE_F32) else a.dtype
        assert epilogue != nv.EPI_RESID_GATE_F32, "RESID_GATE accumulates into `out`; pass it"
        out = torch.empty(M, N, device=a.device, dtype=odt)
    gs = 0
    if gate is not None:
        gate = _c(gate)
        gs = 0 if gate.shape[0] == 1 else gate.stride(0)
    nv.check(_L(a).ltx2_gemm_bf16(nv.ptr(a), a.stride(0), nv.ptr(w), nv.ptr(bias), nv.ptr(out), out.stride(0), M, N, K,
                                     epilogue, nv.ptr(gate), gs, nv.ptr(gate_table), nv.ptr(res),
                                     res.stride(0) if res is not None else 0, nv.stream()))
    return out


def gemm_qkv_vt(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], heads: int, head_dim: int = 128):
    """Fused QKV projection: returns (qkv [M, 3D] bf16 -- V columns only written on the unfused path --, vt [H, hd, Npad], fused)."""
    assert a.dtype in ACT16 and w.dtype == a.dtype
    a, w = _c(a), _c(w)
    M, K = a.shape
    N = w.shape[0]
    D = heads * head_dim
    assert N == 3 * D
    npad = (M + 63) // 64 * 64
    out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    vt = torch.empty(heads, head_dim, npad, device=a.device, dtype=a.dtype)
    import ctypes
    fused = ctypes.c_int(0)
    nv.check(_L(a).ltx2_gemm_qkv_vt(nv.ptr(a), a.stride(0), nv.ptr(w), nv.ptr(bias), nv.ptr(out), out.stride(0), M, N, K,
                                       nv.ptr(vt), 2 * D, npad, head_dim, ctypes.byref(fused), nv.stream()))
    return out, vt, bool(fused.value)


def adaln_rmsnorm2(x: torch.Tensor, scale0, shift0, scale1, shift1, eps: float = 1e-6, dtype: torch.dtype = BF16):
    """(rms_norm(x) * (1 + scale0) + shift0, rms_norm(x) * (1 + scale1) + shift1) from one read of x [rows, D] fp32."""
    x = _c(x.float())
    o0 = torch.empty(x.shape, device=x.device, dtype=dtype)
    o1 = torch.empty_like(o0)
    nv.check(nv.lib(dtype).ltx2_adaln_rmsnorm2(nv.ptr(x), x.stride(0), nv.ptr(o0), nv.ptr(o1), o0.stride(0), x.shape[0], x.shape[1], eps,
                                               nv.ptr(scale0), nv.ptr(shift0), nv.ptr(scale1), nv.ptr(shift1), nv.stream()))
    return o0, o1


def gemm_rowss(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """out = a @ w^T + bias (16-bit) plus the row partial sums of squares of out over 64-column strips -> (out, rowss [M, N/64] fp32 or None
    when the shape does not run on the kernel that writes them)."""
    assert a.dtype in ACT16 and w.dtype == a.dtype
    a, w = _c(a), _c(w)
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    rowss = torch.zeros(M, max(N // 64, 1), device=a.device, dtype=torch.float32)
    import ctypes
    written = ctypes.c_int(0)
    nv.check(_L(a).ltx2_gemm_bf16_rowss(nv.ptr(a), a.stride(0), nv.ptr(w), nv.ptr(bias), nv.ptr(out), out.stride(0), M, N, K, nv.ptr(rowss),
                                        ctypes.byref(written), nv.stream()))
    return out, (rowss if written.value else None)


def gemm_fold(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], epilogue: int, out: Optional[torch.Tensor] = None,
              gate_table: Optional[torch.Tensor] = None, shadow: Optional[torch.Tensor] = None, shadow_scale: Optional[torch.Tensor] = None,
              rf_parts: Optional[torch.Tensor] = None, rf_dim: int = 0, eps: float = 1e-6):
    """ltx2_gemm_bf16_fold (include/ltx2hip.h): the producer / consumer half of an RMS norm folded around two GEMMs.
    Producer (epilogue RESID_GATE_F32, `out` = the fp32 residual stream, updated in place; shadow = 16-bit [M, N]): returns (out, shadow_ss [N/256, ld]),
    the partial sums of squares of the new rows per 256-column tile, tile-major.
    Consumer (BF16 / GELU_BF16; rf_parts = a producer's shadow_ss over rf_dim columns): returns out [M, N].
    None when the 4-wave kernel does not take the problem."""
    import ctypes
    assert a.dtype in ACT16 and w.dtype == a.dtype
    a, w = _c(a), _c(w)
    M, K = a.shape
    N = w.shape[0]
    prod = epilogue == nv.EPI_RESID_GATE_F32
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=a.dtype)
    ss = torch.zeros(max(N // 256, 1), (M + 255) // 256 * 256 + 256, device=a.device, dtype=torch.float32) if (prod and shadow is not None) else None
    sup = ctypes.c_int(0)
    nv.check(_L(a).ltx2_gemm_bf16_fold(nv.ptr(a), a.stride(0), nv.ptr(w), nv.ptr(bias), nv.ptr(out), out.stride(0), M, N, K, epilogue, nv.ptr(gate_table),
                                       nv.ptr(shadow), shadow.stride(0) if shadow is not None else 0, nv.ptr(shadow_scale), nv.ptr(ss),
                                       ss.stride(0) if ss is not None else 0,
                                       nv.ptr(rf_parts), rf_parts.stride(0) if rf_parts is not None else 0, rf_parts.shape[0] if rf_parts is not None else 0,
                                       rf_dim, eps, ctypes.byref(sup), nv.stream()))
    if not sup.value:
        return None
    return (out, ss) if prod else out


def flash_attn_rowscale(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, nkv: int, q_ss: torch.Tensor, eps: float = 1e-6,
                        scale: Optional[float] = None) -> torch.Tensor:
    """flash_attn with q's RMS normalisation over its FULL width folded in as a per-row softmax scale (q_ss: partial sums of squares [Nq, P])."""
    assert q.dtype in ACT16 and q_ss.dtype == torch.float32 and q_ss.is_contiguous()
    nq, hd = q.shape[0], vt.shape[1]
    out = torch.empty(nq, heads * hd, device=q.device, dtype=q.dtype)
    if scale is None:
        scale = 1.0 / math.sqrt(float(hd))
    nv.check(_L(q).ltx2_flash_attn_rowscale(nv.ptr(q), q.stride(0), nv.ptr(k), k.stride(0), nv.ptr(vt), vt.shape[2], nv.ptr(out), out.stride(0), nq, nkv,
                                            heads, hd, scale, nv.ptr(q_ss), q_ss.shape[1], heads * hd, eps, nv.stream()))
    return out


def flash_attn_gated(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, nkv: int, gate_logits: torch.Tensor,
                     scale: Optional[float] = None) -> torch.Tensor:
    """flash_attn with per-head output gates 2*sigmoid(gate_logits[q, h]) applied in the epilogue (fp32, before the rounding)."""
    assert q.dtype in ACT16 and gate_logits.dtype == torch.float32 and gate_logits.stride(1) == 1
    nq, hd = q.shape[0], vt.shape[1]
    out = torch.empty(nq, heads * hd, device=q.device, dtype=q.dtype)
    if scale is None:
        scale = 1.0 / math.sqrt(float(hd))
    nv.check(_L(q).ltx2_flash_attn_gated(nv.ptr(q), q.stride(0), nv.ptr(k), k.stride(0), nv.ptr(vt), vt.shape[2], nv.ptr(out), out.stride(0), nq, nkv,
                                         heads, hd, scale, nv.ptr(gate_logits), gate_logits.stride(0), nv.stream()))
    return out


def flash_attn_gated_parts(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, nkv: int, x: torch.Tensor, gate_w: torch.Tensor,
                           gate_b: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """The engine's many-row form of flash_attn_gated: gate logits x @ gate_w^T as 8 K-slice partial sums, added (with gate_b) in the attention epilogue."""
    assert q.dtype in ACT16 and x.dtype == q.dtype and gate_w.dtype == q.dtype and x.stride(1) == 1
    nq, hd = q.shape[0], vt.shape[1]
    out = torch.empty(nq, heads * hd, device=q.device, dtype=q.dtype)
    parts = torch.empty(8, nq, heads, device=q.device, dtype=torch.float32)
    if scale is None:
        scale = 1.0 / math.sqrt(float(hd))
    nv.check(_L(q).ltx2_flash_attn_gated_parts(nv.ptr(q), q.stride(0), nv.ptr(k), k.stride(0), nv.ptr(vt), vt.shape[2], nv.ptr(out), out.stride(0), nq, nkv,
                                               heads, hd, scale, nv.ptr(x), x.stride(0), nv.ptr(_c(gate_w)), nv.ptr(_c(gate_b.float())), x.shape[1], nv.ptr(parts),
                                               nv.stream()))
    return out


def flash_attn_keymask(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, nkv: int, mask: torch.Tensor,
                       scale: Optional[float] = None) -> torch.Tensor:
    """flash_attn with a key mask: mask [Nkv] bool / 0-1 (True = attend) -- the boolean context mask of the reference's text
    cross-attention (model.py:163-201, attention.py:38-70)."""
    assert q.dtype in ACT16 and mask.numel() == nkv
    nq, hd = q.shape[0], vt.shape[1]
    out = torch.empty(nq, heads * hd, device=q.device, dtype=q.dtype)
    f = (mask.reshape(-1).to(q.device) != 0).to(torch.float32).contiguous()
    words = torch.empty(vt.shape[2] // 64, device=q.device, dtype=torch.int64)
    if scale is None:
        scale = 1.0 / math.sqrt(float(hd))
    nv.check(_L(q).ltx2_flash_attn_keymask(nv.ptr(q), q.stride(0), nv.ptr(k), k.stride(0), nv.ptr(vt), vt.shape[2], nv.ptr(out), out.stride(0), nq, nkv,
                                           heads, hd, scale, nv.ptr(f), nv.ptr(words), nv.stream()))
    return out


def gemm_w8a16(a: torch.Tensor, w8: torch.Tensor, wscale: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = nv.EPI_BF16,
               out: Optional[torch.Tensor] = None, gate_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epilogue(a[M,K] @ dequant(w8)[N,K]^T + bias) with fp8-RESIDENT weights: w8 = float8_e4m3fn codes (uint8 view
    accepted), wscale fp32 [N]; bit-identical to gemm() on bf16(f32(w8) * wscale[:, None])."""
    assert a.dtype in ACT16 and w8.element_size() == 1 and wscale.dtype == torch.float32 and a.dim() == 2 and w8.dim() == 2
    a, w8, wscale = _c(a), _c(w8), _c(wscale)
    M, K = a.shape
    N = w8.shape[0]
    assert wscale.numel() == N
    if out is None:
        assert epilogue != nv.EPI_RESID_GATE_F32, "RESID_GATE accumulates into `out`; pass it"
        out = torch.empty(M, N, device=a.device, dtype=torch.float32 if epilogue == nv.EPI_F32 else a.dtype)
    nv.check(_L(a).ltx2_gemm_w8a16(nv.ptr(a), a.stride(0), nv.ptr(w8), nv.ptr(wscale), nv.ptr(bias), nv.ptr(out), out.stride(0), M, N, K,
                                      epilogue, None, 0, nv.ptr(gate_table), nv.stream()))
    return out


def quantize_rows_fp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 [R, K] -> (float8_e4m3fn codes as uint8 [R, K], fp32 scale [R]): scale = max|row| / 448 (1 for a zero row),
    code = e4m3fn_rne(x * (1 / scale)).  The quantiser of the fp8 compute path (activations per token, weights per output channel)."""
    assert x.dtype in ACT16 and x.dim() == 2
    x = _c(x)
    R, K = x.shape
    codes = torch.empty(R, K, device=x.device, dtype=torch.uint8)
    scale = torch.empty(R, device=x.device, dtype=torch.float32)
    nv.check(_L(x).ltx2_quantize_rows_fp8(nv.ptr(x), x.stride(0), R, K, nv.ptr(codes), K, nv.ptr(scale), nv.stream()))
    return codes, scale


def gemm_fp8(a8: torch.Tensor, ascale: torch.Tensor, w8: torch.Tensor, wscale: torch.Tensor, bias: Optional[torch.Tensor] = None,
             epilogue: int = nv.EPI_BF16, out: Optional[torch.Tensor] = None, gate: Optional[torch.Tensor] = None,
             gate_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M,N] = epilogue(ascale[m] * wscale[n] * (f32(a8)[M,K] @ f32(w8)[N,K]^T) + bias) on the fp8 MFMA (a8, w8: float8_e4m3fn codes,
    uint8 views accepted)."""
    assert a8.element_size() == 1 and w8.element_size() == 1 and a8.dim() == 2 and w8.dim() == 2
    assert ascale.dtype == torch.float32 and wscale.dtype == torch.float32
    a8, w8, ascale, wscale = _c(a8), _c(w8), _c(ascale), _c(wscale)
    M, K = a8.shape
    N = w8.shape[0]
    assert ascale.numel() == M and wscale.numel() == N and w8.shape[1] == K
    if out is None:
        assert epilogue != nv.EPI_RESID_GATE_F32, "RESID_GATE accumulates into `out`; pass it"
        out = torch.empty(M, N, device=a8.device, dtype=torch.float32 if epilogue == nv.EPI_F32 else BF16)
    gs = 0
    if gate is not None:
        gate = _c(gate)
        gs = 0 if gate.shape[0] == 1 else gate.stride(0)
    nv.check(nv.lib().ltx2_gemm_fp8(nv.ptr(a8), a8.stride(0), nv.ptr(ascale), nv.ptr(w8), nv.ptr(wscale), nv.ptr(bias), nv.ptr(out), out.stride(0),
                                    M, N, K, epilogue, nv.ptr(gate), gs, nv.ptr(gate_table), nv.stream()))
    return out


def gemm_fp8_qkv_vt(a8, ascale, w8, wscale, bias, heads: int, head_dim: int = 128):
    """gemm_qkv_vt on the fp8 compute path -> (qkv [M, 3D] bf16, vt [H, hd, Npad], fused)."""
    a8, w8, ascale, wscale = _c(a8), _c(w8), _c(ascale), _c(wscale)
    M, K = a8.shape
    N = w8.shape[0]
    D = heads * head_dim
    assert N == 3 * D
    npad = (M + 63) // 64 * 64
    out = torch.empty(M, N, device=a8.device, dtype=BF16)
    vt = torch.empty(heads, head_dim, npad, device=a8.device, dtype=BF16)
    import ctypes
    fused = ctypes.c_int(0)
    nv.check(nv.lib().ltx2_gemm_fp8_qkv_vt(nv.ptr(a8), a8.stride(0), nv.ptr(ascale), nv.ptr(w8), nv.ptr(wscale), nv.ptr(bias), nv.ptr(out),
                                           out.stride(0), M, N, K, nv.ptr(vt), 2 * D, npad, head_dim, ctypes.byref(fused), nv.stream()))
    return out, vt, bool(fused.value)


def gemv(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act_in: int = 0, act_out: int = 0) -> torch.Tensor:
    assert a.dtype == torch.float32 and w.dtype in ACT16
    a, w = _c(a), _c(w)
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    nv.check(_L(w).ltx2_gemv_f32(nv.ptr(a), a.stride(0), nv.ptr(w), nv.ptr(bias), nv.ptr(out), N, M, N, K, act_in,
                                    act_out, nv.stream()))
    return out


def conv_weight_to_engine(w: torch.Tensor, d2s_stride: Optional[Tuple[int, int, int]] = None, dtype: torch.dtype = BF16) -> torch.Tensor:
    """PyTorch conv3d weight (Cout, Cin, 3, 3, 3) -> engine layout bf16 [Cout][27][Cin]
    (tap = (kt*3+kh)*3+kw).  For depth-to-space convs the output rows are permuted from
    ch = c*sp + s to n' = s*Cf + c so one contiguous channel run lands on one output voxel."""
    cout, cin = w.shape[0], w.shape[1]
    e = w.permute(0, 2, 3, 4, 1).reshape(cout, 27, cin)
    if d2s_stride is not None:
        sp = d2s_stride[0] * d2s_stride[1] * d2s_stride[2]
        cf = cout // sp
        e = e.reshape(cf, sp, 27, cin).permute(1, 0, 2, 3).reshape(cout, 27, cin)
    return e.to(dtype).contiguous()


def conv_bias_to_engine(b: torch.Tensor, d2s_stride: Optional[Tuple[int, int, int]] = None) -> torch.Tensor:
    if d2s_stride is not None:
        sp = d2s_stride[0] * d2s_stride[1] * d2s_stride[2]
        b = b.reshape(-1, sp).t().reshape(-1)
    return b.float().contiguous()


def conv3d(x: torch.Tensor, w_engine: torch.Tensor, bias: Optional[torch.Tensor], causal: bool = False, mode: int = 0,
           res: Optional[torch.Tensor] = None, stride: Tuple[int, int, int] = (1, 1, 1), residual: bool = False,
           pad_zero: int = 0) -> torch.Tensor:
    """x bf16 [T,H,W,Cin] channels-last; w_engine [Cout][27 or 9][Cin] from conv_weight_to_engine /
    conv2d_weight_to_engine (9 taps = per-frame 3x3 conv).  pad_zero: 0 reflect H/W + replicate T (VAE decoder),
    1 / True zero padding in T/H/W (spatial upscaler), 2 zero padding in H/W + replicate T (VAE encoder)."""
    assert x.dtype in ACT16 and x.dim() == 4 and w_engine.dtype == x.dtype
    x = _c(x)
    T, H, W, Cin = x.shape
    Cout = w_engine.shape[0]
    kt = w_engine.shape[1] // 9
    ft, fh, fw = stride
    if mode == 2:
        sp = ft * fh * fw
        out = torch.empty(T * ft - (1 if ft > 1 else 0), H * fh, W * fw, Cout // sp, device=x.device, dtype=x.dtype)
    else:
        out = torch.empty(T, H, W, Cout, device=x.device, dtype=x.dtype)
    nv.check(_L(x).ltx2_conv3d_fused(nv.ptr(x), nv.ptr(w_engine), nv.ptr(bias), nv.ptr(out), T, H, W, Cin, Cout,
                                        int(causal), mode, nv.ptr(res), ft, fh, fw, int(residual), int(pad_zero), kt,
                                        nv.stream()))
    return out


def conv2d_weight_to_engine(w: torch.Tensor, pixel_shuffle: int = 0, dtype: torch.dtype = BF16) -> torch.Tensor:
    """PyTorch conv2d weight (Cout, Cin, 3, 3) -> engine layout bf16 [Cout][9][Cin] (tap = kh*3+kw).  With
    pixel_shuffle = r the output rows are permuted from ch = c*r*r + s (PyTorch pixel_shuffle packing
    (C, r_h, r_w)) to n' = s*Cf + c for the depth-to-space epilogue."""
    cout, cin = w.shape[0], w.shape[1]
    e = w.permute(0, 2, 3, 1).reshape(cout, 9, cin)
    if pixel_shuffle:
        sp = pixel_shuffle * pixel_shuffle
        e = e.reshape(cout // sp, sp, 9, cin).permute(1, 0, 2, 3).reshape(cout, 9, cin)
    return e.to(dtype).contiguous()


def groupnorm_silu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-5,
                   res: Optional[torch.Tensor] = None, act: bool = True) -> torch.Tensor:
    """y = [silu](GroupNorm(x over (C/groups, T, H, W)) * gamma + beta + res) on channels-last bf16 [..., C]."""
    assert x.dtype in ACT16 and x.is_contiguous()
    C = x.shape[-1]
    P = x.numel() // C
    y = torch.empty_like(x)
    sums = torch.empty(2 * groups * (1 + (P + 15) // 16), device=x.device, dtype=torch.float32)
    nv.check(_L(x).ltx2_groupnorm_silu(nv.ptr(x), nv.ptr(res), nv.ptr(y), P, C, groups, eps, nv.ptr(_c(gamma.float())),
                                          nv.ptr(_c(beta.float())), nv.ptr(sums), int(act), nv.stream()))
    return y


def groupnorm_frames_silu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-5,
                          res: Optional[torch.Tensor] = None, act: bool = True, interleaved: bool = True) -> torch.Tensor:
    """y = [silu](GroupNorm(x[f] over (group, H, W)) * gamma + beta + res) per frame f of channels-last 16-bit x [F, ..., C]
    (temporal upscaler, upscaler/temporal.py:128-147).  interleaved: group of channel c is c % groups (mlx.nn.GroupNorm's
    default, what the reference runs); otherwise c // (C // groups) as in torch.nn.GroupNorm."""
    assert x.dtype in ACT16 and x.is_contiguous() and x.dim() >= 2
    assert res is None or (res.dtype == x.dtype and res.shape == x.shape and res.is_contiguous())
    frames, C = x.shape[0], x.shape[-1]
    y = torch.empty_like(x)
    nv.check(_L(x).ltx2_groupnorm_frames_silu(nv.ptr(x), nv.ptr(res), nv.ptr(y), frames, x.numel() // (frames * C), C, groups, int(interleaved), eps,
                                              nv.ptr(_c(gamma.float())), nv.ptr(_c(beta.float())), None, int(act), nv.stream()))
    return y


def s2d_downsample(y: torch.Tensor, x: torch.Tensor, stride: Tuple[int, int, int]) -> torch.Tensor:
    """space_to_depth(y) + group_mean(space_to_depth(x)) on channels-last bf16 [T,H,W,C] (VAE encoder downsample)."""
    assert y.dtype in ACT16 and x.dtype == y.dtype and y.shape[:3] == x.shape[:3]
    y, x = _c(y), _c(x)
    T, H, W, Cc = y.shape
    st, sh, sw = stride
    out = torch.empty(T // st, H // sh, W // sw, Cc * st * sh * sw, device=y.device, dtype=y.dtype)
    nv.check(_L(y).ltx2_s2d_downsample(nv.ptr(y), nv.ptr(x), nv.ptr(out), T, H, W, Cc, x.shape[3], st, sh, sw, nv.stream()))
    return out


def latent_unnormalize_nhwc(latent: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, dtype: torch.dtype = BF16) -> torch.Tensor:
    """latent fp32 [C,T,H,W] -> bf16 [T,H,W,C] = latent * std[c] + mean[c]  (PerChannelStatistics.un_normalize,
    video_vae/ops.py:158-171; same kernel as the VAE decoder's input stage)."""
    assert latent.dtype == torch.float32 and latent.dim() == 4
    latent = _c(latent)
    C, T, H, W = latent.shape
    out = torch.empty(T, H, W, C, device=latent.device, dtype=dtype)
    nv.check(nv.lib(dtype).ltx2_vae_prepare_latent(nv.ptr(latent), nv.ptr(_c(std.float())), nv.ptr(_c(mean.float())), None, 0.0,
                                              nv.ptr(out), C, T * H * W, nv.stream()))
    return out


def latent_normalize_nchw(x: torch.Tensor, mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """x bf16 [T,H,W,C] -> fp32 [C,T,H,W] = (x - mean[c]) / std[c]."""
    assert x.dtype in ACT16 and x.dim() == 4 and x.is_contiguous()
    T, H, W, C = x.shape
    out = torch.empty(C, T, H, W, device=x.device, dtype=torch.float32)
    nv.check(_L(x).ltx2_latent_normalize_nchw(nv.ptr(x), nv.ptr(_c(mean.float())), nv.ptr(_c(std.float())), nv.ptr(out), C,
                                                 T * H * W, nv.stream()))
    return out


def adaln_rmsnorm(x: torch.Tensor, eps: float = 1e-6, layer_norm: bool = False,
                  scale_tab: Optional[torch.Tensor] = None, shift_tab: Optional[torch.Tensor] = None,
                  scale_emb: Optional[torch.Tensor] = None, shift_emb: Optional[torch.Tensor] = None,
                  emb_stride: int = 0, dtype: torch.dtype = BF16) -> torch.Tensor:
    assert x.dtype == torch.float32 and x.dim() == 2
    x = _c(x)
    rows, D = x.shape
    out = torch.empty(rows, D, device=x.device, dtype=dtype)
    nv.check(nv.lib(dtype).ltx2_adaln_rmsnorm(nv.ptr(x), D, nv.ptr(out), D, rows, D, eps, int(layer_norm), nv.ptr(scale_tab),
                                         nv.ptr(shift_tab), nv.ptr(scale_emb), nv.ptr(shift_emb), emb_stride, nv.stream()))
    return out


def adaln_rmsnorm_fp8(x: torch.Tensor, eps: float = 1e-6, layer_norm: bool = False, scale_tab: Optional[torch.Tensor] = None,
                      shift_tab: Optional[torch.Tensor] = None, scale_emb: Optional[torch.Tensor] = None,
                      shift_emb: Optional[torch.Tensor] = None, emb_stride: int = 0, want_bf16: bool = True):
    """adaln_rmsnorm with the per-token e4m3fn quantiser fused in -> (bf16 out or None, codes uint8 [rows, D], scale fp32 [rows])."""
    assert x.dtype == torch.float32 and x.dim() == 2
    x = _c(x)
    rows, D = x.shape
    out = torch.empty(rows, D, device=x.device, dtype=BF16) if want_bf16 else None
    codes = torch.empty(rows, D, device=x.device, dtype=torch.uint8)
    scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    nv.check(nv.lib().ltx2_adaln_rmsnorm_fp8(nv.ptr(x), D, nv.ptr(out), D, nv.ptr(codes), D, nv.ptr(scale), rows, D, eps, int(layer_norm),
                                             nv.ptr(scale_tab), nv.ptr(shift_tab), nv.ptr(scale_emb), nv.ptr(shift_emb), emb_stride, nv.stream()))
    return out, codes, scale


def qknorm_rope_(buf: torch.Tensor, D: int, head_dim: int, q_off: int, q_weight: torch.Tensor,
                 k_off: int = 0, k_weight: Optional[torch.Tensor] = None, eps: float = 1e-6,
                 cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert buf.dtype in ACT16 and buf.dim() == 2 and buf.is_contiguous()
    nv.check(_L(buf).ltx2_qknorm_rope(nv.ptr(buf), buf.stride(0), buf.shape[0], D, head_dim, q_off, nv.ptr(q_weight),
                                       k_off, nv.ptr(k_weight), eps, nv.ptr(cos), nv.ptr(sin), nv.stream()))
    return buf


def vt_transpose(v: torch.Tensor, heads: int, head_dim: int = 128) -> torch.Tensor:
    """v bf16 [Nkv, >= heads*head_dim] (a strided column view is fine) -> VT [H,head_dim,Npad]."""
    assert v.dtype in ACT16 and v.dim() == 2 and v.stride(1) == 1
    nkv = v.shape[0]
    npad = (nkv + 63) // 64 * 64
    vt = torch.empty(heads, head_dim, npad, device=v.device, dtype=v.dtype)
    nv.check(_L(v).ltx2_vt_transpose(nv.ptr(v), v.stride(0), nv.ptr(vt), nkv, npad, heads, head_dim, nv.stream()))
    return vt


def flash_attn(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, nkv: int,
               scale: Optional[float] = None) -> torch.Tensor:
    """q [Nq, H*hd], k [Nkv, H*hd] bf16 (row-strided views allowed), vt [H,hd,Npad] from vt_transpose (hd 128 or 64)."""
    assert q.dtype in ACT16 and k.dtype == q.dtype and vt.dtype == q.dtype and q.stride(1) == 1 and k.stride(1) == 1
    nq, hd = q.shape[0], vt.shape[1]
    out = torch.empty(nq, heads * hd, device=q.device, dtype=q.dtype)
    if scale is None:
        scale = 1.0 / math.sqrt(float(hd))
    nv.check(_L(q).ltx2_flash_attn(nv.ptr(q), q.stride(0), nv.ptr(k), k.stride(0), nv.ptr(vt), vt.shape[2], nv.ptr(out),
                                      out.stride(0), nq, nkv, heads, hd, scale, nv.stream()))
    return out


def attn_head_gate_(att: torch.Tensor, x: torch.Tensor, gate_w: torch.Tensor, gate_b: torch.Tensor, heads: int) -> torch.Tensor:
    """In place: att [rows, H*hd] bf16 *= 2*sigmoid(x @ gate_w^T + gate_b) per head; returns the fp32 logits."""
    assert att.dtype in ACT16 and x.dtype == att.dtype and gate_w.dtype == att.dtype and att.is_contiguous() and x.stride(1) == 1
    rows, hd = att.shape[0], att.shape[1] // heads
    logits = torch.empty(rows, heads, device=att.device, dtype=torch.float32)
    nv.check(_L(att).ltx2_attn_head_gate(nv.ptr(att), att.stride(0), nv.ptr(x), x.stride(0), nv.ptr(_c(gate_w)), nv.ptr(_c(gate_b.float())),
                                          nv.ptr(logits), rows, x.shape[1], heads, hd, nv.stream()))
    return logits


def rope_tables(positions: torch.Tensor, dim: int, theta: float, max_pos) -> Tuple[torch.Tensor, torch.Tensor]:
    """positions (1, n_dims, N, 2) on the GPU -> SPLIT-RoPE cos, sin fp32 [N, dim/2] (slot h*(d/2)+j for head h)."""
    pos = _c(positions[0].float())
    n_dims, N = pos.shape[0], pos.shape[1]
    if n_dims != len(max_pos):
        raise ValueError(f"Number of position dimensions ({n_dims}) must match max_pos length ({len(max_pos)})")
    n_freq = dim // (2 * n_dims)
    grid = (torch.tensor(float(theta)) ** torch.linspace(0.0, 1.0, n_freq, dtype=torch.float32) * (math.pi / 2)).float().to(pos.device)
    mp = torch.tensor([float(m) for m in max_pos], device=pos.device)
    cos = torch.empty(N, dim // 2, device=pos.device, dtype=torch.float32)
    sin = torch.empty_like(cos)
    nv.check(nv.lib().ltx2_rope_tables(nv.ptr(pos), nv.ptr(grid), nv.ptr(mp), N, n_dims, n_freq, dim // 2, nv.ptr(cos), nv.ptr(sin),
                                       nv.stream()))
    return cos, sin


def timestep_sinusoid(t: torch.Tensor, mult: float, dim: int = 256) -> torch.Tensor:
    t = _c(t.float())
    out = torch.empty(t.numel(), dim, device=t.device, dtype=torch.float32)
    nv.check(nv.lib().ltx2_timestep_sinusoid(nv.ptr(t), 1, mult, t.numel(), dim, nv.ptr(out), None, nv.stream()))
    return out


def dequant_fp8(w: torch.Tensor, scale: float, dtype: torch.dtype = BF16) -> torch.Tensor:
    """fp8 e4m3fn weight (device tensor, torch.float8_e4m3fn or its uint8 view) * scale -> bf16."""
    raw = w.view(torch.uint8) if w.dtype != torch.uint8 else w
    raw = _c(raw)
    out = torch.empty(raw.shape, device=raw.device, dtype=dtype)
    nv.check(nv.lib(dtype).ltx2_dequant_fp8_e4m3fn(nv.ptr(raw), float(scale), nv.ptr(out), raw.numel(), nv.stream()))
    return out


def cast_bf16(x: torch.Tensor, dtype: torch.dtype = BF16) -> torch.Tensor:
    x = _c(x.float())
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    nv.check(nv.lib(dtype).ltx2_cast_f32_bf16(nv.ptr(x), nv.ptr(out), x.numel(), nv.stream()))
    return out


def x0_from_velocity(latent: torch.Tensor, velocity: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
    """latent/velocity fp32 [N,C]; timesteps fp32 with 1 or N elements."""
    latent, velocity, timesteps = _c(latent), _c(velocity), _c(timesteps.float())
    n, c = latent.shape
    out = torch.empty_like(latent)
    stride = 0 if timesteps.numel() == 1 else 1
    nv.check(nv.lib().ltx2_x0_from_velocity(nv.ptr(latent), nv.ptr(velocity), nv.ptr(timesteps), stride, 0.0, nv.ptr(out),
                                            n, c, nv.stream()))
    return out


def euler_step(x: torch.Tensor, x0: torch.Tensor, sigma: float, sigma_next: float,
               mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None) -> torch.Tensor:
    x, x0 = _c(x), _c(x0)
    n, c = x.shape
    out = torch.empty_like(x)
    nv.check(nv.lib().ltx2_euler_step(nv.ptr(x), nv.ptr(x0), nv.ptr(mask), nv.ptr(clean), float(sigma), float(sigma_next),
                                      nv.ptr(out), n, c, nv.stream()))
    return out


def _step_operands(x, timesteps, operands, mask=None):
    """The checks the sampler-step wrappers share -> (N, C, timesteps as contiguous fp32): timesteps has 1 or N elements, every operand that is
    given (None: an optional one left out) is fp32, contiguous and shaped like x, and a mask has N fp32 elements."""
    n, c = x.shape
    timesteps = _c(timesteps.float())
    if timesteps.numel() not in (1, n):
        raise ValueError(f"timesteps has {timesteps.numel()} elements; expected 1 or N={n}")
    for t in (x,) + tuple(operands):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape)
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous() and mask.numel() == n)
    return n, c, timesteps


def _segment(seg: dict, layout: tuple, required: tuple = ("vel_cond",), outputs: tuple = ("out",), null: tuple = (), like: str = "x",
             both: bool = True):
    """One latent's share of a C entry's arguments from its operands by name.  `layout`: the entry's per-segment arguments in ABI order, up to
    (N, C), which follow: a str names a [N, C] fp32 tensor -- "timesteps" stands for the pointer and its stride, "mask" for the [N] mask --
    and a tuple (key, cast[, default]) any other argument (no default: seg must hold it).  A tensor that seg leaves out is NULL, unless it is
    in `required` (asserted) or in `outputs`: those are made like seg[like], except the ones in `null`, which stay NULL.  both: mask and
    clean go together; else a mask needs its clean latent.  -> (arguments, {output name: tensor}, the tensors to keep alive across the call:
    _step_operands may have made a contiguous fp32 copy of the timesteps, and the arguments hold its address only)."""
    x = seg[like]
    outs = {k: None if k in null else seg[k] if seg.get(k) is not None else torch.empty_like(x) for k in outputs}
    tensors = {k: outs[k] if k in outs else seg.get(k) for k in layout if isinstance(k, str) and k != "timesteps"}
    mask, clean = tensors.get("mask"), tensors.get("clean")
    assert all(tensors[k] is not None for k in required) and ((mask is None) == (clean is None) if both else (mask is None or clean is not None))
    n, c, ts = _step_operands(x, seg["timesteps"], tuple(t for k, t in tensors.items() if k not in (like, "mask")), mask)
    args = []
    for k in layout:
        if k == "timesteps":
            args += [nv.ptr(ts), 0 if ts.numel() == 1 else 1]
        elif isinstance(k, str):
            args.append(nv.ptr(tensors[k]))
        else:
            args.append(k[1](seg[k[0]] if len(k) == 2 else seg.get(k[0], k[2])))
    return args + [n, c], outs, ts


def _segments(segs, layout: tuple, **kw):
    """_segment over the (video, audio) pair of a *_pair wrapper -> (the flat argument list, [outputs of each], the tensors to keep alive)."""
    packed = [_segment(seg, layout, **kw) for seg in segs]
    return [a for p in packed for a in p[0]], [p[1] for p in packed], [p[2] for p in packed]


_GUIDED = ("x", "vel_cond", "vel_uncond", "timesteps", "mask", "clean", ("cfg_scale", float), "out")


def guided_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: torch.Tensor, timesteps: torch.Tensor, cfg_scale: float, sigma: float,
                      sigma_next: float, mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """One classifier-free-guided step over fp32 [N, C] (ltx2_guided_euler_step): x0 of both velocities, CFGGuider.guide, the mask / clean
    blend and the Euler update in one pass, every operation individually rounded.  timesteps: 1 or N elements; `out` may be `x`;
    `dtype` picks the library build (the kernel is fp32 in both)."""
    if out is None:
        out = torch.empty_like(x)
    assert vel_cond is not None and vel_uncond is not None and (mask is None or clean is not None)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, clean, out), mask)
    nv.check(nv.lib(dtype).ltx2_guided_euler_step(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                                  nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(sigma), float(sigma_next), nv.ptr(out), n, c,
                                                  nv.stream()))
    return out


def guided_euler_step_pair(video: dict, audio: dict, sigma: float, sigma_next: float, dtype: Optional[torch.dtype] = None):
    """guided_euler_step over two latents in ONE launch (ltx2_guided_euler_step_pair): `video` and `audio` each hold the single form's
    operands by name -- x, vel_cond, vel_uncond, timesteps, cfg_scale and optionally mask, clean, out.  -> (video out, audio out), each
    equal to guided_euler_step's bit for bit."""
    args, outs, _held = _segments((video, audio), _GUIDED, required=("vel_cond", "vel_uncond"))
    nv.check(nv.lib(dtype).ltx2_guided_euler_step_pair(*args, float(sigma), float(sigma_next), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


def seed_word(seed: int, device) -> torch.Tensor:
    """The noise seed as the kernels read it: one 64-bit word on the device (the low 64 bits of `seed`, stored as int64)."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device=device)


def _seed_ptr(seed: torch.Tensor):
    assert seed.dtype == torch.int64 and seed.numel() == 1 and seed.is_cuda, "seed: one int64 word on the device (kernels.seed_word)"
    return nv.ptr(seed)


def philox_bits(n_quads: int, seed: torch.Tensor, step: int, stream_id: int, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The raw Philox4x32-10 words (ltx2_philox_bits) -> (n_quads, 4) int32, to be read as uint32: row q has the counter
    (lo32(q), hi32(q), step, stream_id) and the key (lo32(seed), hi32(seed))."""
    out = torch.empty(int(n_quads), 4, dtype=torch.int32, device=seed.device)
    nv.check(nv.lib(dtype).ltx2_philox_bits(nv.ptr(out), int(n_quads), _seed_ptr(seed), int(step), int(stream_id), nv.stream()))
    return out


def philox_normal(n: int, seed: torch.Tensor, step: int, stream_id: int, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """n fp32 N(0,1) values (ltx2_philox_normal): element e is lane e & 3 of quad e >> 2, Box-Muller on the quad's uniforms.  A function of
    (seed, step, stream_id, e) alone: the noise the ancestral step kernels add, bit for bit."""
    out = torch.empty(int(n), dtype=torch.float32, device=seed.device)
    nv.check(nv.lib(dtype).ltx2_philox_normal(nv.ptr(out), int(n), _seed_ptr(seed), int(step), int(stream_id), nv.stream()))
    return out


def ancestral_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], timesteps: torch.Tensor, cfg_scale: float,
                         sigma: float, sigma_up: float, sigma_down: float, seed: torch.Tensor, step: int, mask: Optional[torch.Tensor] = None,
                         clean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """One Euler-ancestral step over fp32 [N, C] (ltx2_ancestral_euler_step): guided_euler_step to sigma_down, then + (z * sigma_up) * mask with
    z = philox_normal(N*C, seed, step, 0) made inside the kernel.  vel_uncond None: no guidance, the plain step's arithmetic (x0_from_velocity,
    euler_step).  `out` may be `x`."""
    if out is None:
        out = torch.empty_like(x)
    assert vel_cond is not None and (mask is None) == (clean is None)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, clean, out), mask)
    nv.check(nv.lib(dtype).ltx2_ancestral_euler_step(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                                     nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(sigma), float(sigma_up), float(sigma_down),
                                                     _seed_ptr(seed), int(step), nv.ptr(out), n, c, nv.stream()))
    return out


def ancestral_euler_step_pair(video: dict, audio: dict, sigma: float, sigma_up: float, sigma_down: float, seed: torch.Tensor, step: int,
                              dtype: Optional[torch.dtype] = None):
    """ancestral_euler_step over two latents in ONE launch (ltx2_ancestral_euler_step_pair): `video` (noise stream 0) and `audio` (stream 1) each
    hold x, vel_cond, timesteps, cfg_scale and optionally vel_uncond, mask, clean, out.  -> (video out, audio out), each the single launch's
    bits (the audio's: a single launch on stream 1, which philox_normal(..., stream_id=1) and the torch ops restate)."""
    args, outs, _held = _segments((video, audio), _GUIDED)
    nv.check(nv.lib(dtype).ltx2_ancestral_euler_step_pair(*args, float(sigma), float(sigma_up), float(sigma_down), _seed_ptr(seed), int(step), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


def ancestral_euler_step_x0(x: torch.Tensor, x0: torch.Tensor, sigma: float, sigma_up: float, sigma_down: float, seed: torch.Tensor, step: int,
                            stream_id: int = 0, mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The Euler-ancestral step from a ready x0 over fp32 [N, C] (ltx2_ancestral_euler_step_x0), every operation individually rounded.  With
    `clean`, x0 is blended by `mask` first; a mask WITHOUT clean scales the noise alone (x0 is taken as already blended)."""
    if out is None:
        out = torch.empty_like(x)
    assert x0 is not None and (clean is None or mask is not None)
    n, c = x.shape
    for t in (x, x0, clean, out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape)
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous() and mask.numel() == n)
    nv.check(nv.lib(dtype).ltx2_ancestral_euler_step_x0(nv.ptr(x), nv.ptr(x0), nv.ptr(mask), nv.ptr(clean), float(sigma), float(sigma_up), float(sigma_down),
                                                        _seed_ptr(seed), int(step), int(stream_id), nv.ptr(out), n, c, nv.stream()))
    return out


def stg_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], vel_perturbed: torch.Tensor, timesteps: torch.Tensor,
                   cfg_scale: float, stg_scale: float, sigma: float, sigma_next: float, mask: Optional[torch.Tensor] = None,
                   clean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """guided_euler_step with STGGuider.guide on top (ltx2_stg_euler_step): x0 of the three velocities, CFGGuider.guide (vel_uncond None: no CFG),
    g + stg_scale * (g - perturbed), the mask / clean blend and the Euler update in one pass, every operation individually rounded.
    timesteps: 1 or N elements; `out` may be any input; `dtype` picks the library build (the kernel is fp32 in both)."""
    if out is None:
        out = torch.empty_like(x)
    assert vel_cond is not None and vel_perturbed is not None and (mask is None or clean is not None)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, vel_perturbed, clean, out), mask)
    nv.check(nv.lib(dtype).ltx2_stg_euler_step(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(vel_perturbed), nv.ptr(timesteps),
                                               0 if timesteps.numel() == 1 else 1, nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(stg_scale),
                                               float(sigma), float(sigma_next), nv.ptr(out), n, c, nv.stream()))
    return out


def stg_euler_step_pair(video: dict, audio: dict, sigma: float, sigma_next: float, dtype: Optional[torch.dtype] = None):
    """stg_euler_step over two latents in ONE launch (ltx2_stg_euler_step_pair): `video` and `audio` each hold the single form's operands by
    name -- x, vel_cond, timesteps, cfg_scale, stg_scale and optionally vel_uncond (None: no CFG on that modality), vel_perturbed (None: no
    STG term, guided_euler_step's arithmetic), mask, clean, out.  -> (video out, audio out), each equal to the single launch's bit for bit."""
    layout = ("x", "vel_cond", "vel_uncond", "vel_perturbed", "timesteps", "mask", "clean", ("cfg_scale", float), ("stg_scale", float), "out")
    args, outs, _held = _segments((video, audio), layout)
    nv.check(nv.lib(dtype).ltx2_stg_euler_step_pair(*args, float(sigma), float(sigma_next), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


def channel_guidance_stats_blocks(rows: int, c: int, dtype: Optional[torch.dtype] = None) -> int:
    """Rows of the fp64 [rows, 4, C] workspace that channel_guidance_stats fills for an [N, C] latent (ltx2_channel_guidance_stats_blocks)."""
    return int(nv.lib(dtype).ltx2_channel_guidance_stats_blocks(int(rows), int(c)))


def channel_guidance_stats(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: torch.Tensor, timesteps: torch.Tensor, cfg_scale: float,
                           partials: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                           dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The per-channel statistics of the standard loop's guidance rescale over fp32 [N, C] (ltx2_channel_guidance_stats): with a = x - t*vc,
    b = x - t*vu, g = b + cfg_scale*(a - b), over all rows the mean and sqrt(mean((. - mean)^2) + 1e-8) of g and of a per channel, accumulated
    in fp64 without atomics.  -> stats, fp32 [4, C] = mean_g, std_g, mean_a, std_a.  `partials`: the fp64 workspace
    [channel_guidance_stats_blocks(N, C), 4, C]; `dtype` picks the library build (the kernels are fp32 / fp64 in both)."""
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond))
    assert vel_cond is not None and vel_uncond is not None
    if partials is None:
        partials = torch.empty(channel_guidance_stats_blocks(n, c, dtype), 4, c, device=x.device, dtype=torch.float64)
    if stats is None:
        stats = torch.empty(4, c, device=x.device, dtype=torch.float32)
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 4 * c * channel_guidance_stats_blocks(n, c, dtype)
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 4 * c
    nv.check(nv.lib(dtype).ltx2_channel_guidance_stats(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps),
                                                       0 if timesteps.numel() == 1 else 1, float(cfg_scale), nv.ptr(partials), nv.ptr(stats), n, c,
                                                       nv.stream()))
    return stats


def rescaled_guided_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: torch.Tensor, timesteps: torch.Tensor, cfg_scale: float,
                               guidance_rescale: float, sigma: float, sigma_next: float, stats: Optional[torch.Tensor] = None,
                               out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """One guided step of the standard one-stage loop over fp32 [N, C] (ltx2_rescaled_guided_euler_step): g = b + cfg_scale*(a - b), with `stats`
    (channel_guidance_stats) gr = ((g - mean_g)/std_g)*std_a + mean_a and g = r*gr + (1 - r)*g, then the Euler update, every operation
    individually rounded.  stats None: guidance without rescale.  timesteps: 1 or N elements; `out` may be `x`."""
    if out is None:
        out = torch.empty_like(x)
    assert vel_cond is not None and vel_uncond is not None
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, out))
    assert stats is None or (stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 4 * c)
    nv.check(nv.lib(dtype).ltx2_rescaled_guided_euler_step(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps),
                                                           0 if timesteps.numel() == 1 else 1, nv.ptr(stats), float(cfg_scale), float(guidance_rescale),
                                                           float(sigma), float(sigma_next), nv.ptr(out), n, c, nv.stream()))
    return out


def _fbc_operands(*ts: Optional[torch.Tensor]) -> int:
    n = ts[0].numel()
    for t in ts:
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n)
    return n


def fbc_head_metric(h0: torch.Tensor, h1: torch.Tensor, head_prev: Optional[torch.Tensor], threshold: float, r: Optional[torch.Tensor] = None,
                    h1_save: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, float, float, int]:
    """The first-block cache's metric over fp32 tensors of one shape (ltx2_fbc_head_metric): r = h1 - h0, num = sum |r - head_prev| and
    den = sum |head_prev| in fp64 in a fixed order without atomics, skip = (threshold > 0 and den > 0 and num < threshold*den).  head_prev None
    reads as zeros; h1_save receives a copy of h1 and may be h0 itself.  -> (r, num, den, skip); reading the record back waits for the stream."""
    if r is None:
        r = torch.empty_like(h0)
    n = _fbc_operands(h0, h1, head_prev, r, h1_save)
    L = nv.lib(dtype)
    partials = torch.empty(int(L.ltx2_fbc_metric_blocks(n)), 2, device=h0.device, dtype=torch.float64)
    rec = torch.zeros(3, device=h0.device, dtype=torch.float64)
    nv.check(L.ltx2_fbc_head_metric(nv.ptr(h0), nv.ptr(h1), nv.ptr(head_prev), nv.ptr(r), nv.ptr(h1_save), nv.ptr(partials), nv.ptr(rec),
                                    float(threshold), n, nv.stream()))
    host = rec.cpu()
    return r, float(host[0]), float(host[1]), int(host[2:3].view(torch.int32)[0])


def fbc_store_tail(h_last: torch.Tensor, h1: torch.Tensor, tail: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """tail = h_last - h1 over fp32 tensors of one shape (ltx2_fbc_store_tail), one rounded subtraction per element."""
    if tail is None:
        tail = torch.empty_like(h_last)
    n = _fbc_operands(h_last, h1, tail)
    nv.check(nv.lib(dtype).ltx2_fbc_store_tail(nv.ptr(h_last), nv.ptr(h1), nv.ptr(tail), n, nv.stream()))
    return tail


def fbc_apply_tail(h: torch.Tensor, tail: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """h += tail in place over fp32 tensors of one shape (ltx2_fbc_apply_tail), one rounded addition per element."""
    n = _fbc_operands(h, tail)
    nv.check(nv.lib(dtype).ltx2_fbc_apply_tail(nv.ptr(h), nv.ptr(tail), n, nv.stream()))
    return h


GUIDANCE_MODES = {"cfg_star": 0, "apg": 1, "legacy_apg": 2}    # `mode` of ltx2_projected_euler_step / ltx2_dit_projected_step


def guidance_sums_blocks(rows: int, c: int, dtype: Optional[torch.dtype] = None) -> int:
    """Rows of the fp64 [rows, 5] partials buffer that guidance_sums fills for an [N, C] latent (ltx2_guidance_sums_blocks)."""
    return int(nv.lib(dtype).ltx2_guidance_sums_blocks(int(rows), int(c)))


def guidance_sums(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: torch.Tensor, timesteps: torch.Tensor, partials: Optional[torch.Tensor] = None,
                  running: Optional[torch.Tensor] = None, first: bool = True, momentum: float = 0.0, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """First pass of a projected guidance step over fp32 [N, C] (ltx2_guidance_sums): a = x - t*vc, b = x - t*vu, g = a - b (with `running`:
    g = momentum*running + g unless `first`, stored back to running), and S_aa, S_ab, S_bb, S_gg, S_ga in fp64, one row per block.
    -> partials, fp64 [guidance_sums_blocks(N, C), 5].  `dtype` picks the library build (the kernel is fp32 / fp64 in both)."""
    if partials is None:
        partials = torch.empty(guidance_sums_blocks(*x.shape, dtype=dtype), 5, device=x.device, dtype=torch.float64)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, running))
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 5 * guidance_sums_blocks(n, c, dtype)
    nv.check(nv.lib(dtype).ltx2_guidance_sums(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                              nv.ptr(running), int(bool(first)), float(momentum), nv.ptr(partials), n, c, nv.stream()))
    return partials


def projected_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: torch.Tensor, timesteps: torch.Tensor, partials: torch.Tensor, mode: int,
                         scale: float, eta: float, norm_threshold: float, sigma: float, sigma_next: float, mask: Optional[torch.Tensor] = None,
                         clean: Optional[torch.Tensor] = None, running: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         scalars_out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Second pass (ltx2_projected_euler_step): the sums of `partials` added in every block, the guider's scalars from them (mode 0: CFG*'s coef;
    1 / 2: APG's sf and proj), then x0 of both velocities, the guider, the mask / clean blend and the Euler update, every fp32 operation
    individually rounded.  `out` may be `x`; `scalars_out` (fp32, 2 elements) receives the scalars used; `running` (mode 2): the guidance
    guidance_sums left."""
    if out is None:
        out = torch.empty_like(x)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, clean, running, out), mask)
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 5 * guidance_sums_blocks(n, c, dtype)
    assert (mask is None) == (clean is None)
    assert scalars_out is None or (scalars_out.dtype == torch.float32 and scalars_out.numel() >= 2)
    nv.check(nv.lib(dtype).ltx2_projected_euler_step(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                                     nv.ptr(mask), nv.ptr(clean), nv.ptr(running), nv.ptr(partials), int(mode), float(scale), float(eta),
                                                     float(norm_threshold), float(sigma), float(sigma_next), nv.ptr(out), nv.ptr(scalars_out), n, c,
                                                     nv.stream()))
    return out


PAIR_GUIDANCE_MODES = dict(GUIDANCE_MODES, cfg=3, off=4)         # a segment's `mode` in ltx2_projected_euler_step_pair: two guiders without sums on top


def guidance_sums_pair(video: dict, audio: dict, dtype: Optional[torch.dtype] = None):
    """guidance_sums over two latents in ONE launch (ltx2_guidance_sums_pair): `video` and `audio` each hold the single form's operands by name
    -- x, vel_cond, vel_uncond, timesteps and optionally partials, running, first (True), momentum (0.0).  A segment given as None is left out
    (its guider reads no sums; not both).  -> (video partials, audio partials), each equal to guidance_sums's bit for bit (None for a segment
    left out)."""
    layout = ("x", "vel_cond", "vel_uncond", "timesteps", "running", ("first", lambda f: int(bool(f)), True), ("momentum", float, 0.0), ("partials", nv.ptr))
    args, parts, held = [], [], []
    for seg in (video, audio):
        if seg is None:
            args += [None, None, None, None, 0, None, 1, 0.0, None, 0, 0]
            parts.append(None)
            continue
        part = seg.get("partials")
        if part is None:
            part = torch.empty(guidance_sums_blocks(*seg["x"].shape, dtype=dtype), 5, device=seg["x"].device, dtype=torch.float64)
        a, _, ts = _segment(dict(seg, partials=part), layout, required=("vel_cond", "vel_uncond"), outputs=())
        assert part.dtype == torch.float64 and part.is_contiguous() and part.numel() >= 5 * guidance_sums_blocks(a[-2], a[-1], dtype)
        args += a
        parts.append(part)
        held.append(ts)
    nv.check(nv.lib(dtype).ltx2_guidance_sums_pair(*args, nv.stream()))
    return parts[0], parts[1]


def projected_euler_step_pair(video: dict, audio: dict, sigma: float, sigma_next: float, dtype: Optional[torch.dtype] = None):
    """projected_euler_step over two latents in ONE launch (ltx2_projected_euler_step_pair): `video` and `audio` each hold the single form's
    operands by name -- x, vel_cond, timesteps, mode, scale and optionally vel_uncond (mode 4 alone does without), partials (modes 0 - 2), eta
    (1.0), norm_threshold (0.0), mask, clean, running, out, scalars_out.  mode: 0 - 2 as projected_euler_step, 3 = CFGGuider's
    a + (scale - 1)*(a - b), 4 = not guided.  -> (video out, audio out), each equal to the single-launch step's bit for bit."""
    layout = ("x", "vel_cond", "vel_uncond", "timesteps", "mask", "clean", "running", ("partials", nv.ptr, None), ("mode", int), ("scale", float),
              ("eta", float, 1.0), ("norm_threshold", float, 0.0), "out", ("scalars_out", nv.ptr, None))
    args, outs, _held = _segments((video, audio), layout)
    for seg in (video, audio):
        part, sc, (n, c) = seg.get("partials"), seg.get("scalars_out"), seg["x"].shape
        assert part is None or (part.dtype == torch.float64 and part.is_contiguous() and part.numel() >= 5 * guidance_sums_blocks(n, c, dtype))
        assert sc is None or (sc.dtype == torch.float32 and sc.numel() >= 2)
    nv.check(nv.lib(dtype).ltx2_projected_euler_step_pair(*args, float(sigma), float(sigma_next), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


_MM = ("x", "vel_cond", "vel_uncond", "vel_perturbed", "vel_isolated", "timesteps", "mask", "clean")


def _mm_args(seg: dict):
    """One latent's operands of the multi-modal guided steps, by name -- x, vel_cond, timesteps and optionally vel_uncond, vel_perturbed,
    vel_isolated, mask, clean, out -- as the C entries take them -> (pointer / stride arguments up to `clean`, out, N, C, the tensors to keep)."""
    (*args, _out, n, c), outs, ts = _segment(seg, _MM + ("out",))
    return args, outs["out"], n, c, ts


def mm_guided_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, timesteps: torch.Tensor, cfg_scale: float, stg_scale: float, modality_scale: float,
                         sigma: float, sigma_next: float, vel_uncond: Optional[torch.Tensor] = None, vel_perturbed: Optional[torch.Tensor] = None,
                         vel_isolated: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """One step under MultiModalGuider.calculate without rescale over fp32 [N, C] (ltx2_mm_guided_euler_step): x0 of the velocities given, the
    CFG / STG / modality terms of those that are not None, the mask / clean blend and the Euler update in one pass, every operation
    individually rounded.  timesteps: 1 or N elements; `out` may be any input; `dtype` picks the library build (the kernel is fp32 in both)."""
    args, out, n, c, _ts = _mm_args(dict(x=x, vel_cond=vel_cond, vel_uncond=vel_uncond, vel_perturbed=vel_perturbed, vel_isolated=vel_isolated,
                                         timesteps=timesteps, mask=mask, clean=clean, out=out))
    nv.check(nv.lib(dtype).ltx2_mm_guided_euler_step(*args, float(cfg_scale), float(stg_scale), float(modality_scale), float(sigma), float(sigma_next),
                                                     nv.ptr(out), n, c, nv.stream()))
    return out


def mm_guided_euler_step_pair(video: dict, audio: dict, sigma: float, sigma_next: float, dtype: Optional[torch.dtype] = None):
    """mm_guided_euler_step over two latents in ONE launch (ltx2_mm_guided_euler_step_pair): `video` and `audio` each hold the single form's
    operands by name -- x, vel_cond, timesteps, cfg_scale, stg_scale, modality_scale and optionally vel_uncond, vel_perturbed, vel_isolated,
    mask, clean, out.  -> (video out, audio out), each equal to mm_guided_euler_step's bit for bit."""
    args, outs, _held = _segments((video, audio), _MM + (("cfg_scale", float), ("stg_scale", float), ("modality_scale", float), "out"))
    nv.check(nv.lib(dtype).ltx2_mm_guided_euler_step_pair(*args, float(sigma), float(sigma_next), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


def mm_guidance_sums(x: torch.Tensor, vel_cond: torch.Tensor, timesteps: torch.Tensor, cfg_scale: float, stg_scale: float, modality_scale: float,
                     vel_uncond: Optional[torch.Tensor] = None, vel_perturbed: Optional[torch.Tensor] = None, vel_isolated: Optional[torch.Tensor] = None,
                     partials: Optional[torch.Tensor] = None, pred_out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """First pass of the rescaled multi-modal step (ltx2_mm_guidance_sums): the fp64 sums of a, a*a, pred, pred*pred, one row per block.
    -> partials, fp64 [guidance_sums_blocks(N, C), 4]; `pred_out` (fp32 [N, C]) receives MultiModalGuider.calculate's un-rescaled prediction."""
    if partials is None:
        partials = torch.empty(guidance_sums_blocks(*x.shape, dtype=dtype), 4, device=x.device, dtype=torch.float64)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, vel_perturbed, vel_isolated, pred_out))
    assert vel_cond is not None and partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 4 * guidance_sums_blocks(n, c, dtype)
    nv.check(nv.lib(dtype).ltx2_mm_guidance_sums(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(vel_perturbed), nv.ptr(vel_isolated), nv.ptr(timesteps),
                                                 0 if timesteps.numel() == 1 else 1, float(cfg_scale), float(stg_scale), float(modality_scale), nv.ptr(partials),
                                                 nv.ptr(pred_out), n, c, nv.stream()))
    return partials


def mm_rescaled_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, timesteps: torch.Tensor, partials: torch.Tensor, cfg_scale: float, stg_scale: float,
                           modality_scale: float, rescale_scale: float, sigma: float, sigma_next: float, vel_uncond: Optional[torch.Tensor] = None,
                           vel_perturbed: Optional[torch.Tensor] = None, vel_isolated: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                           clean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, scalars_out: Optional[torch.Tensor] = None,
                           dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Second pass (ltx2_mm_rescaled_euler_step): the sums of `partials` added in every block, the rescale factor f from them in fp64, then
    mm_guided_euler_step's pass with pred * f.  `scalars_out` (fp32, 1 element) receives f; `out` may be `x`."""
    args, out, n, c, _ts = _mm_args(dict(x=x, vel_cond=vel_cond, vel_uncond=vel_uncond, vel_perturbed=vel_perturbed, vel_isolated=vel_isolated,
                                         timesteps=timesteps, mask=mask, clean=clean, out=out))
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 4 * guidance_sums_blocks(n, c, dtype)
    assert scalars_out is None or (scalars_out.dtype == torch.float32 and scalars_out.numel() >= 1)
    nv.check(nv.lib(dtype).ltx2_mm_rescaled_euler_step(*args, nv.ptr(partials), float(cfg_scale), float(stg_scale), float(modality_scale), float(rescale_scale),
                                                       float(sigma), float(sigma_next), nv.ptr(out), nv.ptr(scalars_out), n, c, nv.stream()))
    return out


def res2s_midpoint(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], timesteps: torch.Tensor, cfg_scale: float, c: float,
                   n_bong: int, mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None, x_mid: Optional[torch.Tensor] = None,
                   anchor: Optional[torch.Tensor] = None, eps1: Optional[torch.Tensor] = None, final: bool = False,
                   dtype: Optional[torch.dtype] = None):
    """First pass of a res_2s step over fp32 [N, C] (ltx2_res2s_midpoint): the guided, blended x0 `d` of the two velocities, then
    anchor = x, eps1 = d - anchor, x_mid = anchor + c*eps1 and n_bong "bong" iterations, every operation individually rounded.
    -> (x_mid, anchor, eps1); `x_mid` may be `x`.  final=True: the reference's final-step branch, x_mid = d -> (x_mid, None, None).
    vel_uncond None: no guidance.  timesteps: 1 or N elements; `dtype` picks the library build (the kernel is fp32 in both)."""
    if x_mid is None:
        x_mid = torch.empty_like(x)
    if not final:
        anchor = torch.empty_like(x) if anchor is None else anchor
        eps1 = torch.empty_like(x) if eps1 is None else eps1
    else:
        anchor = eps1 = None
    assert vel_cond is not None and (mask is None or clean is not None)
    n, ch, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, clean, x_mid, anchor, eps1), mask)
    nv.check(nv.lib(dtype).ltx2_res2s_midpoint(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                               nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(c), int(n_bong), nv.ptr(x_mid), nv.ptr(anchor),
                                               nv.ptr(eps1), n, ch, nv.stream()))
    return x_mid, anchor, eps1


def res2s_combine(x_mid: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], timesteps: torch.Tensor, cfg_scale: float,
                  anchor: torch.Tensor, eps1: torch.Tensor, h: float, b1: float, b2: float, mask: Optional[torch.Tensor] = None,
                  clean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Second pass of a res_2s step (ltx2_res2s_combine): d2 from (x_mid, velocities at the sub-sigma) as in res2s_midpoint,
    e2 = d2 - anchor, out = anchor + h*(b1*eps1 + b2*e2), every operation individually rounded.  `out` may be any [N, C] operand."""
    if out is None:
        out = torch.empty_like(x_mid)
    assert vel_cond is not None and anchor is not None and eps1 is not None and (mask is None or clean is not None)
    n, ch, timesteps = _step_operands(x_mid, timesteps, (vel_cond, vel_uncond, clean, anchor, eps1, out), mask)
    nv.check(nv.lib(dtype).ltx2_res2s_combine(nv.ptr(x_mid), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                              nv.ptr(mask), nv.ptr(clean), float(cfg_scale), nv.ptr(anchor), nv.ptr(eps1), float(h), float(b1), float(b2),
                                              nv.ptr(out), n, ch, nv.stream()))
    return out


def res2s_midpoint_pair(video: dict, audio: dict, c: float, n_bong: int, final: bool = False, dtype: Optional[torch.dtype] = None):
    """res2s_midpoint over two latents in ONE launch (ltx2_res2s_midpoint_pair): `video` and `audio` each hold the single form's operands by
    name -- x, vel_cond, timesteps, cfg_scale and optionally vel_uncond, mask, clean, x_mid, anchor, eps1 -- with shapes, scales, timesteps and
    conditioning of their own; c, n_bong and `final` are shared.  -> ((x_mid, anchor, eps1) of the video, the same of the audio), each equal
    to res2s_midpoint's bit for bit."""
    names = ("x_mid", "anchor", "eps1")
    args, outs, _held = _segments((video, audio), _GUIDED[:-1] + names, outputs=names, null=names[1:] if final else (), both=False)
    nv.check(nv.lib(dtype).ltx2_res2s_midpoint_pair(*args, float(c), int(n_bong), nv.stream()))
    return tuple(outs[0][k] for k in names), tuple(outs[1][k] for k in names)


def res2s_combine_pair(video: dict, audio: dict, h: float, b1: float, b2: float, dtype: Optional[torch.dtype] = None):
    """res2s_combine over two latents in ONE launch (ltx2_res2s_combine_pair): `video` and `audio` each hold x_mid, vel_cond, timesteps,
    cfg_scale, anchor, eps1 and optionally vel_uncond, mask, clean, out; h, b1, b2 are shared.  -> (video out, audio out), each equal to
    res2s_combine's bit for bit; `out` may be any [N, C] operand of its segment."""
    layout = ("x_mid",) + _GUIDED[1:-1] + ("anchor", "eps1", "out")
    args, outs, _held = _segments((video, audio), layout, required=("vel_cond", "anchor", "eps1"), like="x_mid", both=False)
    nv.check(nv.lib(dtype).ltx2_res2s_combine_pair(*args, float(h), float(b1), float(b2), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


def heun_predict(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], timesteps: torch.Tensor, cfg_scale: float, sigma: float,
                 sigma_next: float, ge_gamma: float = 0.0, prev: Optional[torch.Tensor] = None, first: bool = True,
                 mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None, d: Optional[torch.Tensor] = None,
                 xp: Optional[torch.Tensor] = None, final: bool = False, dtype: Optional[torch.dtype] = None):
    """First pass of a Heun step over fp32 [N, C] (ltx2_heun_predict): the CFG-guided x0 of the two velocities (vel_uncond None: no
    guidance), the GE velocity correction where `prev` is given (ge_gamma > 0; read unless `first`, then overwritten with the uncorrected
    velocity), the mask / clean blend `d` and the Euler predictor `xp`, every operation individually rounded.  -> (d, xp); final=True: the
    sigma_next == 0 form -> (d, None).  d / xp may be `x`.  timesteps: 1 or N elements; `dtype` picks the library build."""
    d = torch.empty_like(x) if d is None else d
    xp = None if final else (torch.empty_like(x) if xp is None else xp)
    assert vel_cond is not None and (mask is None or clean is not None)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, clean, prev, d, xp), mask)
    nv.check(nv.lib(dtype).ltx2_heun_predict(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                             nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(ge_gamma), nv.ptr(prev), int(bool(first)), float(sigma),
                                             float(sigma_next), nv.ptr(d), nv.ptr(xp), n, c, nv.stream()))
    return d, xp


def heun_correct(x: torch.Tensor, d: torch.Tensor, xp: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], timesteps: torch.Tensor,
                 cfg_scale: float, sigma: float, sigma_next: float, mask: Optional[torch.Tensor] = None, clean: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Second pass of a Heun step (ltx2_heun_correct): d2 from (xp, velocities and timesteps at sigma_next) as in heun_predict without GE,
    out = x + (0.5*((x - d)/sigma + (xp - d2)/sigma_next))*(sigma_next - sigma), every operation individually rounded.  `out` may be any
    [N, C] operand."""
    out = torch.empty_like(x) if out is None else out
    assert d is not None and xp is not None and vel_cond is not None and (mask is None or clean is not None)
    n, c, timesteps = _step_operands(x, timesteps, (d, xp, vel_cond, vel_uncond, clean, out), mask)
    nv.check(nv.lib(dtype).ltx2_heun_correct(nv.ptr(x), nv.ptr(d), nv.ptr(xp), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps),
                                             0 if timesteps.numel() == 1 else 1, nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(sigma),
                                             float(sigma_next), nv.ptr(out), n, c, nv.stream()))
    return out


def ge_euler_step(x: torch.Tensor, vel_cond: torch.Tensor, vel_uncond: Optional[torch.Tensor], timesteps: torch.Tensor, cfg_scale: float, ge_gamma: float,
                  prev: torch.Tensor, first: bool, sigma: float, sigma_next: float, mask: Optional[torch.Tensor] = None,
                  clean: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """One guided Euler step with the GE velocity correction over fp32 [N, C] (ltx2_ge_euler_step): heun_predict's pass with the predictor
    as the new latent.  `prev` (fp32 [N, C]) is read unless `first` and overwritten with the uncorrected velocity; `out` may be `x`."""
    out = torch.empty_like(x) if out is None else out
    assert vel_cond is not None and prev is not None and (mask is None or clean is not None)
    n, c, timesteps = _step_operands(x, timesteps, (vel_cond, vel_uncond, clean, prev, out), mask)
    nv.check(nv.lib(dtype).ltx2_ge_euler_step(nv.ptr(x), nv.ptr(vel_cond), nv.ptr(vel_uncond), nv.ptr(timesteps), 0 if timesteps.numel() == 1 else 1,
                                              nv.ptr(mask), nv.ptr(clean), float(cfg_scale), float(ge_gamma), nv.ptr(prev), int(bool(first)), float(sigma),
                                              float(sigma_next), nv.ptr(out), n, c, nv.stream()))
    return out


_GE = (("ge_gamma", float), "prev", ("first", lambda f: int(bool(f))))     # the video's GE arguments, behind cfg_scale: dict(video, ge_gamma=..., first=...)


def heun_predict_pair(video: dict, audio: dict, sigma: float, sigma_next: float, ge_gamma: float = 0.0, first: bool = True, final: bool = False,
                      dtype: Optional[torch.dtype] = None):
    """heun_predict over two latents in ONE launch (ltx2_heun_predict_pair): `video` and `audio` each hold x, vel_cond, timesteps, cfg_scale
    and optionally vel_uncond, mask, clean, d, xp; the video alone may hold `prev` (GE acts on it alone).  -> ((d, xp) of the video, the same
    of the audio), each equal to heun_predict's bit for bit; final=True: xp is None in both."""
    kw = dict(outputs=("d", "xp"), null=("xp",) if final else ())
    va, v, _vts = _segment(dict(video, ge_gamma=ge_gamma, first=first), _GUIDED[:-1] + _GE + ("d", "xp"), **kw)
    aa, a, _ats = _segment(audio, _GUIDED[:-1] + ("d", "xp"), **kw)
    nv.check(nv.lib(dtype).ltx2_heun_predict_pair(*va, *aa, float(sigma), float(sigma_next), nv.stream()))
    return (v["d"], v["xp"]), (a["d"], a["xp"])


def heun_correct_pair(video: dict, audio: dict, sigma: float, sigma_next: float, dtype: Optional[torch.dtype] = None):
    """heun_correct over two latents in ONE launch (ltx2_heun_correct_pair): `video` and `audio` each hold x, d, xp, vel_cond, timesteps,
    cfg_scale and optionally vel_uncond, mask, clean, out.  -> (video out, audio out), each equal to heun_correct's bit for bit."""
    args, outs, _held = _segments((video, audio), ("x", "d", "xp") + _GUIDED[1:], required=("d", "xp", "vel_cond"))
    nv.check(nv.lib(dtype).ltx2_heun_correct_pair(*args, float(sigma), float(sigma_next), nv.stream()))
    return outs[0]["out"], outs[1]["out"]


def ge_euler_step_pair(video: dict, audio: dict, ge_gamma: float, first: bool, sigma: float, sigma_next: float, dtype: Optional[torch.dtype] = None):
    """ge_euler_step over the video latent and the plain guided Euler step over the audio latent in ONE launch (ltx2_ge_euler_step_pair):
    `video` holds x, vel_cond, timesteps, cfg_scale, prev and optionally vel_uncond, mask, clean, out; `audio` the same without prev.
    -> (video out, audio out), each equal to the single launch's bit for bit."""
    va, v, _vts = _segment(dict(video, ge_gamma=ge_gamma, first=first), _GUIDED[:-1] + _GE + ("out",), required=("vel_cond", "prev"))
    aa, a, _ats = _segment(audio, _GUIDED)
    nv.check(nv.lib(dtype).ltx2_ge_euler_step_pair(*va, *aa, float(sigma), float(sigma_next), nv.stream()))
    return v["out"], a["out"]


def pixnorm_mod_silu(x: torch.Tensor, table: torch.Tensor, te: Optional[torch.Tensor], shift_row: int, scale_row: int,
                     eps: float = 1e-6) -> torch.Tensor:
    assert x.dtype in ACT16
    x = _c(x)
    C_ = x.shape[-1]
    P = x.numel() // C_
    y = torch.empty_like(x)
    nv.check(_L(x).ltx2_pixnorm_mod_silu(nv.ptr(x), nv.ptr(y), P, C_, eps, nv.ptr(table), nv.ptr(te), shift_row,
                                            scale_row, nv.stream()))
    return y


def video_chunk_to_uint8(cur: torch.Tensor, frames: torch.Tensor, t_dst0: int, prev: Optional[torch.Tensor] = None,
                         ramp: Optional[torch.Tensor] = None) -> None:
    """One temporal chunk `cur` fp32 [3,Tc,H,W] -> frames uint8 [T,H,W,3] at frame t_dst0, cross-faded with the tail of the previous
    chunk `prev` over len(ramp) frames, trimmed at T (reference simple_decoder.py:760-798) -- one pass instead of cat / blend / cat /
    convert over fp32 volumes."""
    cur = _c(cur.float())
    _, Tc, H, W = cur.shape
    ov = 0 if prev is None else int(ramp.numel())
    if prev is not None:
        prev, ramp = _c(prev.float()), _c(ramp.float())
    nv.check(nv.lib().ltx2_video_chunk_to_uint8(nv.ptr(cur), nv.ptr(prev), nv.ptr(ramp), nv.ptr(frames), Tc, 0 if prev is None else prev.shape[1], ov,
                                                H, W, int(t_dst0), frames.shape[0], nv.stream()))


def tile_blend_accumulate(tile: torch.Tensor, nt: int, nh: int, nw: int, mt: torch.Tensor, mh: torch.Tensor, mw: torch.Tensor,
                          out: torch.Tensor, wsum: torch.Tensor, t0: int, h0: int, w0: int) -> None:
    """out[3,OT,OH,OW] += tile[3,dt,dh,dw][:, :nt, :nh, :nw] * (mt x mh x mw); wsum[OT,OH,OW] += mask (reference tiling.py:380-404)."""
    tile = _c(tile.float())
    _, dt, dh, dw = tile.shape
    _, OT, OH, OW = out.shape
    nv.check(nv.lib().ltx2_tile_blend_accumulate(nv.ptr(tile), dt, dh, dw, nt, nh, nw, nv.ptr(_c(mt.float())), nv.ptr(_c(mh.float())),
                                                 nv.ptr(_c(mw.float())), nv.ptr(out), nv.ptr(wsum), OT, OH, OW, t0, h0, w0, nv.stream()))


def tile_blend_finish(out: torch.Tensor, wsum: torch.Tensor) -> None:
    """out /= clamp(wsum, 1e-8) in place (reference tiling.py:410-412)."""
    nv.check(nv.lib().ltx2_tile_blend_finish(nv.ptr(out), nv.ptr(wsum), wsum.numel(), nv.stream()))


def video_to_uint8(video: torch.Tensor) -> torch.Tensor:
    """video fp32 [3,T,H,W] -> uint8 [T,H,W,3] (reference simple_decoder.py:792-798)."""
    video = _c(video.float())
    _, T, H, W = video.shape
    out = torch.empty(T, H, W, 3, device=video.device, dtype=torch.uint8)
    nv.check(nv.lib().ltx2_video_to_uint8(nv.ptr(video), nv.ptr(out), T, H, W, nv.stream()))
    return out


# ---------------------------------------------------------------------- control-video path (IC-LoRA): Canny edges, uint8 -> patchified operand
CANNY_TILE = (nv.CANNY_TILE_H, nv.CANNY_TILE_W)          # the hysteresis kernel's tile (rows, columns): tests size their maps from it


def _u8_frames(t: torch.Tensor, name: str, dims) -> torch.Tensor:
    if t.dtype != torch.uint8 or t.dim() not in dims:
        raise ValueError(f"{name}: expected a uint8 tensor of {' or '.join(str(d) for d in dims)} dimensions, got {t.dtype} {tuple(t.shape)}")
    return _c(t)


def _out_like(out: Optional[torch.Tensor], name: str, shape, dtype: torch.dtype, device) -> torch.Tensor:
    """A caller's output buffer must be exactly what the kernel writes: the kernel trusts the shape it is given."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if out.device != device or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}" + ("" if out.is_contiguous() else " (not contiguous)"))
    return out


def canny_hysteresis(cmap: torch.Tensor, out: Optional[torch.Tensor] = None, return_passes: bool = False):
    """Second stage of Canny alone: map uint8 (F, H, W) of {0, 1 = weak, 2 = strong} -> edges uint8 (F, H, W), 255 on every strong pixel and
    every weak pixel 8-connected to one.  Synchronises the stream (one flag read per pass); RuntimeError past H * W relaunches."""
    cmap = _u8_frames(cmap, "canny_hysteresis", (3,))
    F, H, W = cmap.shape
    out = _out_like(out, "canny_hysteresis", cmap.shape, torch.uint8, cmap.device)
    ws = torch.empty(nv.CANNY_FLAG_BYTES, device=cmap.device, dtype=torch.uint8)
    n = nv.i32(0)
    nv.check(nv.lib().ltx2_canny_hysteresis(nv.ptr(cmap), F, H, W, nv.ptr(out), nv.ptr(ws), ws.numel(), nv.C.byref(n), nv.stream()))
    return (out, n.value) if return_passes else out


def canny(frames: torch.Tensor, low: float = 100.0, high: float = 200.0, out: Optional[torch.Tensor] = None, return_passes: bool = False):
    """uint8 RGB frames (F, H, W, 3) -> edges uint8 (F, H, W), 255 / 0: the Canny definition written out in include/ltx2hip.h (OpenCV's with
    apertureSize 3, L2gradient false).  Synchronises the stream, as canny_hysteresis does."""
    frames = _u8_frames(frames, "canny", (4,))
    F, H, W, ch = frames.shape
    if ch != 3:
        raise ValueError(f"canny: expected RGB frames (F, H, W, 3), got {tuple(frames.shape)}")
    out = _out_like(out, "canny", (F, H, W), torch.uint8, frames.device)
    ws = torch.empty(nv.CANNY_FLAG_BYTES + F * H * W, device=frames.device, dtype=torch.uint8)
    n = nv.i32(0)
    nv.check(nv.lib().ltx2_canny_u8(nv.ptr(frames), F, H, W, float(low), float(high), nv.ptr(out), nv.ptr(ws), ws.numel(), nv.C.byref(n), nv.stream()))
    return (out, n.value) if return_passes else out


def frames_to_patches(frames: torch.Tensor, dtype: torch.dtype = BF16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames (F, H, W, 3), (F, H, W, 1) or (F, H, W) -> the VAE encoder's patchified operand [F, H/4, W/4, 64] in `dtype`:
    patchify_video(frames / 127.5 - 1) in one pass, bit for bit; a single channel is replicated to three."""
    frames = _u8_frames(frames, "frames_to_patches", (3, 4))
    F, H, W = frames.shape[:3]
    cin = frames.shape[3] if frames.dim() == 4 else 1
    if dtype not in ACT16:
        raise ValueError(f"frames_to_patches: dtype {dtype} (bfloat16 or float16: the library builds)")
    if H % 4 or W % 4:
        raise ValueError(f"frames_to_patches: H {H} and W {W} must be multiples of 4")
    out = _out_like(out, "frames_to_patches", (F, H // 4, W // 4, 64), dtype, frames.device)
    nv.check(nv.lib(dtype).ltx2_frames_to_patches(nv.ptr(frames), F, H, W, cin, nv.ptr(out), nv.stream()))
    return out


# ---------------------------------------------------------------------- source-clip glue of the retake pipeline (control.hip)
def _dense(t: torch.Tensor, name: str, what: str, dtype: torch.dtype, shape, device) -> torch.Tensor:
    """An operand the kernel reads as it lies: exactly this dtype, shape and device, contiguous (no silent copy or cast)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)} on {t.device}" + ("" if t.is_contiguous() else " (not contiguous)") if isinstance(t, torch.Tensor) else repr(type(t))
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got {got}")
    return t


def retake_prepare(encoded: torch.Tensor, noise: torch.Tensor, f0: int, f1: int, noise_scale: float = 1.0,
                   out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """The retake pipeline's state from the encoded source clip in one pass (ltx2_retake_prepare): encoded fp32 (1, C, F, H, W), noise fp32
    (N, C) with N = F*H*W, the latent-frame window 0 <= f0 <= f1 <= F -> (clean (N, C), mask (N,), latent (N, C)), fp32:
    clean = VideoLatentPatchifier(1).patchify(encoded), mask = 1 on the tokens of frames [f0, f1) (TemporalRegionMask), latent =
    noise*sm + clean*(1 - sm) with sm = mask*noise_scale (GaussianNoiser), bit for bit what those torch statements give.
    out: the three output tensors, exactly those shapes; nothing may overlap."""
    if not isinstance(encoded, torch.Tensor) or encoded.dim() != 5 or encoded.shape[0] != 1 or not encoded.is_cuda:
        raise ValueError(f"retake_prepare: encoded must be a GPU tensor (1, C, F, H, W), got "
                         f"{tuple(encoded.shape)} on {encoded.device}" if isinstance(encoded, torch.Tensor) else "retake_prepare: encoded must be a tensor")
    _, ch, F, H, W = encoded.shape
    dev, n = encoded.device, F * H * W
    _dense(encoded, "retake_prepare", "encoded", torch.float32, encoded.shape, dev)
    _dense(noise, "retake_prepare", "noise", torch.float32, (n, ch), dev)
    f0, f1 = int(f0), int(f1)
    if not 0 <= f0 <= f1 <= F:
        raise ValueError(f"retake_prepare: latent-frame window [{f0}, {f1}) is not within 0 <= f0 <= f1 <= F = {F}")
    if out is not None and len(out) != 3:
        raise ValueError("retake_prepare: out must be the three tensors (clean, mask, latent)")
    oc, om, ol = out if out is not None else (None, None, None)
    oc = _out_like(oc, "retake_prepare (clean)", (n, ch), torch.float32, dev)
    om = _out_like(om, "retake_prepare (mask)", (n,), torch.float32, dev)
    ol = _out_like(ol, "retake_prepare (latent)", (n, ch), torch.float32, dev)
    nv.check(nv.lib().ltx2_retake_prepare(nv.ptr(encoded), nv.ptr(noise), ch, F, H, W, f0, f1, float(noise_scale), nv.ptr(oc), nv.ptr(om),
                                          nv.ptr(ol), nv.stream()))
    return oc, om, ol


def retake_composite(decoded: torch.Tensor, source: torch.Tensor, p0: int, p1: int, ramp: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 clips (T, H, W, 3) -> uint8 (T, H, W, 3): `decoded` on the pixel frames [p0, p1), a linear fade into `source` over `ramp`
    frames outside the window and the source's own bytes beyond it (ltx2_retake_composite, integer arithmetic).  out may not alias an input."""
    for name, t in (("decoded", decoded), ("source", source)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or not t.is_cuda:
            raise ValueError(f"retake_composite: {name} must be a uint8 GPU tensor (T, H, W, 3), got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else f"retake_composite: {name} must be a tensor")
    dev = decoded.device
    _dense(decoded, "retake_composite", "decoded", torch.uint8, decoded.shape, dev)
    _dense(source, "retake_composite", "source", torch.uint8, decoded.shape, dev)
    T, H, W, _ = decoded.shape
    p0, p1, ramp = int(p0), int(p1), int(ramp)
    if not 0 <= p0 <= p1 <= T:
        raise ValueError(f"retake_composite: pixel-frame window [{p0}, {p1}) is not within 0 <= p0 <= p1 <= T = {T}")
    if not 0 <= ramp <= nv.RETAKE_MAX_RAMP:
        raise ValueError(f"retake_composite: ramp {ramp} (0 .. {nv.RETAKE_MAX_RAMP})")
    out = _out_like(out, "retake_composite", decoded.shape, torch.uint8, dev)
    nv.check(nv.lib().ltx2_retake_composite(nv.ptr(decoded), nv.ptr(source), T, H, W, p0, p1, ramp, nv.ptr(out), nv.stream()))
    return out


def retake_prepare_audio(encoded: torch.Tensor, noise: torch.Tensor, a0: int, a1: int, noise_scale: float = 1.0,
                         out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """retake_prepare for the clip's sound track (ltx2_retake_prepare_audio): the audio encoder's latent fp32 (1, C, T, M), noise fp32
    (T, C*M), the latent-frame window 0 <= a0 <= a1 <= T -> (clean (T, C*M), mask (T,), latent (T, C*M)), fp32:
    clean = AudioPatchifier.patchify(encoded), mask = 1 on the frames [a0, a1), latent = noise*sm + clean*(1 - sm) with sm = mask*noise_scale,
    bit for bit what those torch statements give.  out: the three output tensors, exactly those shapes; nothing may overlap."""
    if not isinstance(encoded, torch.Tensor):
        raise ValueError("retake_prepare_audio: encoded must be a tensor")
    if encoded.dim() != 4 or encoded.shape[0] != 1 or not encoded.is_cuda:
        raise ValueError(f"retake_prepare_audio: encoded must be a GPU tensor (1, C, T, M), got {tuple(encoded.shape)} on {encoded.device}")
    _, ch, T, M = encoded.shape
    dev = encoded.device
    _dense(encoded, "retake_prepare_audio", "encoded", torch.float32, encoded.shape, dev)
    _dense(noise, "retake_prepare_audio", "noise", torch.float32, (T, ch * M), dev)
    a0, a1 = int(a0), int(a1)
    if not 0 <= a0 <= a1 <= T:
        raise ValueError(f"retake_prepare_audio: latent-frame window [{a0}, {a1}) is not within 0 <= a0 <= a1 <= T = {T}")
    if out is not None and len(out) != 3:
        raise ValueError("retake_prepare_audio: out must be the three tensors (clean, mask, latent)")
    oc, om, ol = out if out is not None else (None, None, None)
    oc = _out_like(oc, "retake_prepare_audio (clean)", (T, ch * M), torch.float32, dev)
    om = _out_like(om, "retake_prepare_audio (mask)", (T,), torch.float32, dev)
    ol = _out_like(ol, "retake_prepare_audio (latent)", (T, ch * M), torch.float32, dev)
    nv.check(nv.lib().ltx2_retake_prepare_audio(nv.ptr(encoded), nv.ptr(noise), ch, T, M, a0, a1, float(noise_scale), nv.ptr(oc), nv.ptr(om),
                                                nv.ptr(ol), nv.stream()))
    return oc, om, ol


def retake_composite_audio(decoded: torch.Tensor, source: torch.Tensor, s0: int, s1: int, ramp: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 waveforms (channels, S) at one rate -> fp32 (channels, S): `decoded` on the samples [s0, s1), a linear fade into `source` over
    `ramp` samples outside the window and the source's own bits beyond it (ltx2_retake_composite_audio; individually rounded fp32
    arithmetic).  out may not alias an input."""
    for name, t in (("decoded", decoded), ("source", source)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"retake_composite_audio: {name} must be a tensor")
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_cuda:
            raise ValueError(f"retake_composite_audio: {name} must be a float32 GPU tensor (channels, S), got {t.dtype} {tuple(t.shape)} on {t.device}")
    dev = decoded.device
    _dense(decoded, "retake_composite_audio", "decoded", torch.float32, decoded.shape, dev)
    _dense(source, "retake_composite_audio", "source", torch.float32, decoded.shape, dev)
    ch, S = decoded.shape
    s0, s1, ramp = int(s0), int(s1), int(ramp)
    if ch < 1 or S < 1:
        raise ValueError(f"retake_composite_audio: empty waveform {tuple(decoded.shape)}")
    if not 0 <= s0 <= s1 <= S:
        raise ValueError(f"retake_composite_audio: sample window [{s0}, {s1}) is not within 0 <= s0 <= s1 <= S = {S}")
    if not 0 <= ramp <= nv.RETAKE_AUDIO_MAX_RAMP:
        raise ValueError(f"retake_composite_audio: ramp {ramp} (0 .. {nv.RETAKE_AUDIO_MAX_RAMP})")
    out = _out_like(out, "retake_composite_audio", decoded.shape, torch.float32, dev)
    nv.check(nv.lib().ltx2_retake_composite_audio(nv.ptr(decoded), nv.ptr(source), ch, S, s0, s1, ramp, nv.ptr(out), nv.stream()))
    return out


# ---------------------------------------------------------------------------------------------- Gemma-3 text encoder (gemma.hip)
# Gemma always runs on the bfloat16 build (model/text_encoder/gemma3.py), whatever the DiT's compute dtype.

def gemma_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, kv_heads: int, causal: bool = True, window: int = 0,
               scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [Tq, >= heads*256], k / v [Tkv, >= kv_heads*256] bf16 (row-strided column views of the fused QKV rows are fine) ->
    out [Tq, heads*256] bf16: causal (window > 0: sliding) or, causal=False, unmasked GQA attention at head_dim 256."""
    assert q.dtype == BF16 and k.dtype == BF16 and v.dtype == BF16 and q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    tq, tkv = q.shape[0], k.shape[0]
    if out is None:
        out = torch.empty(tq, heads * 256, device=q.device, dtype=BF16)
    if scale is None:
        scale = 256 ** -0.5
    nv.check(nv.lib().ltx2_gemma_attn(nv.ptr(q), q.stride(0), nv.ptr(k), k.stride(0), nv.ptr(v), v.stride(0), nv.ptr(out), out.stride(0),
                                      tq, tkv, heads, kv_heads, int(bool(causal)), int(window), float(scale), nv.stream()))
    return out


def gemma_qknorm_rope_(qkv: torch.Tensor, q_heads: int, kv_heads: int, q_w: torch.Tensor, k_w: torch.Tensor, cos: torch.Tensor,
                       sin: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """In place on the fused QKV rows [T, >= (q_heads + kv_heads)*256] bf16: per-head RMSNorm(1 + w) then rotate-half RoPE
    (cos / sin fp32 [T, 128]); the V columns are not touched."""
    assert qkv.dtype == BF16 and qkv.stride(1) == 1 and cos.dtype == torch.float32 and sin.dtype == torch.float32
    assert cos.shape == (qkv.shape[0], 128) and sin.shape == cos.shape and cos.is_contiguous() and sin.is_contiguous()
    nv.check(nv.lib().ltx2_gemma_qknorm_rope(nv.ptr(qkv), qkv.stride(0), qkv.shape[0], q_heads, kv_heads, nv.ptr(_c(q_w.float())),
                                             nv.ptr(_c(k_w.float())), float(eps), nv.ptr(cos), nv.ptr(sin), nv.stream()))
    return qkv


def gemma_resid_norm(x_in: torch.Tensor, y: Optional[torch.Tensor], w_post: Optional[torch.Tensor], w_next: Optional[torch.Tensor],
                     x_out: Optional[torch.Tensor] = None, h_out: Optional[torch.Tensor] = None, hf_out: Optional[torch.Tensor] = None,
                     eps: float = 1e-6) -> None:
    """x = x_in + rms_norm(y) * (1 + w_post) (y None: x = x_in); n = rms_norm(x) * (1 + w_next); writes x_out (fp32) = x,
    h_out (bf16) = n, hf_out (fp32) = n -- whichever are given."""
    assert x_in.dtype == torch.float32 and x_in.stride(1) == 1
    rows, d = x_in.shape
    for t in (x_out, hf_out):
        assert t is None or (t.dtype == torch.float32 and t.shape == (rows, d) and t.stride(1) == 1)
    assert h_out is None or (h_out.dtype == BF16 and h_out.shape == (rows, d) and h_out.stride(1) == 1)
    assert y is None or (y.dtype == BF16 and y.shape == (rows, d) and y.stride(1) == 1)
    nv.check(nv.lib().ltx2_gemma_resid_norm(nv.ptr(x_in), x_in.stride(0), nv.ptr(y), y.stride(0) if y is not None else 0, nv.ptr(w_post),
                                            nv.ptr(w_next), nv.ptr(x_out), x_out.stride(0) if x_out is not None else 0, nv.ptr(h_out),
                                            h_out.stride(0) if h_out is not None else 0, nv.ptr(hf_out),
                                            hf_out.stride(0) if hf_out is not None else 0, rows, d, float(eps), nv.stream()))


def gemma_gated_act(gu: torch.Tensor, inter: int, act: int = nv.GEMMA_ACT_SILU, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gu [rows, >= 2*inter] bf16 (gate columns [0, inter), up columns [inter, 2*inter)) -> act(gate) * up, bf16 [rows, inter]."""
    assert gu.dtype == BF16 and gu.stride(1) == 1
    if out is None:
        out = torch.empty(gu.shape[0], inter, device=gu.device, dtype=BF16)
    nv.check(nv.lib().ltx2_gemma_gated_act(nv.ptr(gu), gu.stride(0), nv.ptr(out), out.stride(0), gu.shape[0], inter, int(act), nv.stream()))
    return out


def gemma_embed(ids: torch.Tensor, table: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ids int32 [rows] -> fp32 [rows, D] = table[ids] * scale (table bf16 [vocab, D])."""
    assert table.dtype == BF16 and table.is_contiguous() and ids.dtype == torch.int32 and ids.is_contiguous()
    vocab, d = table.shape
    if out is None:
        out = torch.empty(ids.shape[0], d, device=table.device, dtype=torch.float32)
    nv.check(nv.lib().ltx2_gemma_embed(nv.ptr(ids), ids.shape[0], nv.ptr(table), vocab, d, float(scale), nv.ptr(out), out.stride(0), nv.stream()))
    return out


def _layer_strides(states) -> Optional[Tuple[int, int]]:
    """(layer stride, row stride) in elements when the L [T, D] fp32 tensors are equally spaced rows of one buffer (the views
    Gemma3Model returns, sliced or not); None when they are not and have to be stacked."""
    s0 = states[0]
    if any(s.shape != s0.shape or s.dtype != torch.float32 or s.device != s0.device or s.stride() != s0.stride() for s in states):
        return None
    if s0.stride(1) != 1 or s0.stride(0) % 4 or s0.stride(0) < s0.shape[1]:
        return None
    if len(states) == 1:
        return 0, s0.stride(0)
    step = states[1].data_ptr() - s0.data_ptr()
    if step <= 0 or step % 16 or any(states[i + 1].data_ptr() - states[i].data_ptr() != step for i in range(len(states) - 1)):
        return None
    same = s0.untyped_storage().data_ptr()
    if any(s.untyped_storage().data_ptr() != same for s in states):
        return None
    return step // 4, s0.stride(0)


def gemma_features_rms(hidden_states, valid: Optional[torch.Tensor] = None, eps: float = 1e-6, dtype: torch.dtype = BF16,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The V2 feature extractor's GEMM operand: hidden_states = L fp32 [T, D] tensors (or one [L, T, D] tensor), valid [T] (non-zero = a
    real token; None = all) -> 16-bit [T, L * D], column l * D + d = x[l, t, d] * rsqrt(mean_d(x[l, t]^2) + eps), pad rows zero.  The
    list is read in place when its entries are equally spaced views of one buffer, and stacked once otherwise."""
    states = list(hidden_states.unbind(0)) if isinstance(hidden_states, torch.Tensor) else list(hidden_states)
    assert states and all(s.dim() == 2 and s.is_cuda for s in states)
    strides = _layer_strides(states)
    if strides is None:
        stacked = torch.stack([s.float() for s in states])
        states, strides = list(stacked.unbind(0)), (stacked.stride(0), stacked.stride(1))
    nl, (t, d) = len(states), states[0].shape
    if out is None:
        out = torch.empty(t, nl * d, device=states[0].device, dtype=dtype)
    assert out.dtype == dtype and dtype in ACT16 and out.shape == (t, nl * d) and out.stride(1) == 1
    if valid is not None:
        valid = _c(valid.to(states[0].device, torch.int32).reshape(-1))
        assert valid.shape[0] == t
    nv.check(nv.lib(dtype).ltx2_gemma_features_rms(nv.ptr(states[0]), strides[0], strides[1], nv.ptr(valid), nv.ptr(out), out.stride(0), t, nl, d,
                                                   float(eps), nv.stream()))
    return out


# ---- audio VAE decoder / vocoder (fp32, csrc/audio.hip).  Channels-last fp32 tensors: [T, C] (1-D) or [H, W, C] (2-D); the row stride is
# the stride of the position dimension.  Weights come packed by pack_conv_weight / pack_conv_transpose_weight.

def _f32(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_cuda and t.stride(-1) == 1), "audio kernels take CUDA fp32 tensors with unit channel stride"


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """PyTorch conv weight (out, in, k) or (out, in, kh, kw) -> fp32 [kh * kw * in, round_up(out, 4)] (k = (i * kw + j) * in + c)."""
    w = w.float()
    if w.dim() == 3:
        w = w[:, :, None, :]
    cout, cin, kh, kw = w.shape
    packed = torch.zeros(kh * kw * cin, (cout + 3) // 4 * 4, device=w.device, dtype=torch.float32)
    packed[:, :cout] = w.permute(2, 3, 1, 0).reshape(kh * kw * cin, cout)
    return packed


def pack_conv_transpose_weight(w: torch.Tensor, rate: int) -> torch.Tensor:
    """PyTorch ConvTranspose1d weight (in, out, k) -> the polyphase layout [rate][ceil(k / rate)][in][round_up(out, 4)]:
    phase ph, tap t holds kernel index ph + rate * (ntaps - 1 - t) (zero past k)."""
    w = w.float()
    cin, cout, k = w.shape
    ntaps = (k + rate - 1) // rate
    packed = torch.zeros(rate, ntaps, cin, (cout + 3) // 4 * 4, device=w.device, dtype=torch.float32)
    for ph in range(rate):
        for t in range(ntaps):
            j = ph + rate * (ntaps - 1 - t)
            if j < k:
                packed[ph, t, :, :cout] = w[:, :, j]
    return packed


def audio_conv1d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], c_out: int, k: int, *, stride: int = 1, dilation: int = 1,
                 padding: int = 0, t_out: Optional[int] = None, out: Optional[torch.Tensor] = None, prologue: int = nv.AUDIO_PRO_NONE,
                 slope: float = 0.0, res: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 0.0, act: int = nv.AUDIO_ACT_NONE,
                 c_in: Optional[int] = None) -> torch.Tensor:
    """x [T, >= C_in] -> out [T_out, c_out]: zero-padded (left `padding`) conv1d with the packed weight w [k * C_in, ldw] and the fused
    prologue / epilogue of ltx2_audio_conv.  T_out defaults to the usual (T + 2 padding - dilation (k - 1) - 1) // stride + 1."""
    c_in = x.shape[1] if c_in is None else c_in
    T = x.shape[0]
    if t_out is None:
        t_out = (T + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    if out is None:
        out = torch.empty(t_out, c_out, device=x.device, dtype=torch.float32)
    _f32(x, w, bias, out, res)
    assert w.shape[0] == k * c_in and out.shape[0] >= t_out
    nv.check(nv.lib().ltx2_audio_conv(nv.ptr(x), x.stride(0), 1, T, c_in, nv.ptr(w), w.stride(0), nv.ptr(bias), nv.ptr(out), out.stride(0), 1, t_out,
                                      c_out, 1, k, stride, dilation, 0, padding, 0, int(prologue), float(slope), nv.ptr(res),
                                      res.stride(0) if res is not None else 0, float(alpha), float(beta), int(act), nv.stream()))
    return out


def audio_conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], c_out: int, kh: int, kw: int, pad_h: int, pad_w: int, *,
                 upsample: bool = False, out: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [H, W, C_in] -> out [H_out, W_out, c_out] (stride 1), padded as CausalConv2d pads (pad_h rows on top only, pad_w columns each
    side): [H, W] for 3x3 / 1x1; upsample=True reads the nearest x2 image and drops the first output row (Upsample2d): [2H - 1, 2W]."""
    H, W, c_in = x.shape
    if upsample:
        h_out, w_out = 2 * H + pad_h - kh, 2 * W + 2 * pad_w - kw + 1
    else:
        h_out, w_out = H + pad_h - kh + 1, W + 2 * pad_w - kw + 1
    if out is None:
        out = torch.empty(h_out, w_out, c_out, device=x.device, dtype=torch.float32)
    assert x.is_contiguous() and out.is_contiguous() and (res is None or res.is_contiguous())
    _f32(x, w, bias, out, res)
    nv.check(nv.lib().ltx2_audio_conv(nv.ptr(x), c_in, H, W, c_in, nv.ptr(w), w.stride(0), nv.ptr(bias), nv.ptr(out), c_out, h_out, w_out, c_out,
                                      kh, kw, 1, 1, pad_h, pad_w, 1 if upsample else 0, nv.AUDIO_PRO_NONE, 0.0, nv.ptr(res),
                                      c_out if res is not None else 0, 1.0, 0.0, nv.AUDIO_ACT_NONE, nv.stream()))
    return out


def audio_conv2d_strided(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], c_out: int, kh: int, kw: int, pad_h: int, pad_w: int, *,
                         stride: Tuple[int, int] = (1, 1), out: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                         act: int = nv.AUDIO_ACT_NONE) -> torch.Tensor:
    """x [H, W, C_in] -> out [H_out, W_out, c_out] with stride (stride_h, stride_w), padded as CausalConv2d pads (pad_h rows on top only,
    pad_w columns each side): only the kept outputs are computed.  Downsample2d is kh = kw = 3, pad (2, 1), stride (2, 2):
    [(H - 1) // 2 + 1, (W - 1) // 2 + 1].  act: AUDIO_ACT_NONE or AUDIO_ACT_SILU (after bias and res)."""
    H, W, c_in = x.shape
    sh, sw = stride
    h_out, w_out = (H + pad_h - kh) // sh + 1, (W + 2 * pad_w - kw) // sw + 1
    if out is None:
        out = torch.empty(h_out, w_out, c_out, device=x.device, dtype=torch.float32)
    assert x.is_contiguous() and out.is_contiguous() and (res is None or res.is_contiguous())
    assert tuple(out.shape) == (h_out, w_out, c_out) and (res is None or tuple(res.shape) == (h_out, w_out, c_out)) and w.shape[0] == kh * kw * c_in
    _f32(x, w, bias, out, res)
    nv.check(nv.lib().ltx2_audio_conv2d_strided(nv.ptr(x), c_in, H, W, c_in, nv.ptr(w), w.stride(0), nv.ptr(bias), nv.ptr(out), c_out, h_out, w_out,
                                                c_out, kh, kw, sh, sw, pad_h, pad_w, nv.ptr(res), c_out if res is not None else 0, int(act),
                                                nv.stream()))
    return out


def audio_latent_normalize(h: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, z: int) -> torch.Tensor:
    """Encoder conv_out h [T, F, ld] (channels-last, ld >= z) -> (z, T, F): (h[t, f, c] - mean[c * F + f]) / std[c * F + f]."""
    T, F, ld = h.shape
    assert h.is_contiguous() and mean.is_contiguous() and std.is_contiguous() and mean.numel() == z * F == std.numel() and ld >= z
    out = torch.empty(z, T, F, device=h.device, dtype=torch.float32)
    _f32(h, mean, std, out)
    nv.check(nv.lib().ltx2_audio_latent_normalize(nv.ptr(h), ld, nv.ptr(mean), nv.ptr(std), nv.ptr(out), T, F, z, nv.stream()))
    return out


def audio_conv_transpose1d(x: torch.Tensor, w_phase: torch.Tensor, bias: Optional[torch.Tensor], c_out: int, k: int, rate: int, padding: int,
                           prologue: int = nv.AUDIO_PRO_NONE, slope: float = 0.0) -> torch.Tensor:
    """ConvTranspose1d(stride=rate, padding) of x [T, C_in] -> [(T - 1) rate + k - 2 padding, c_out] through the polyphase kernel."""
    T, c_in = x.shape
    t_out = (T - 1) * rate + k - 2 * padding
    out = torch.empty(t_out, c_out, device=x.device, dtype=torch.float32)
    _f32(x, w_phase, bias, out)
    assert w_phase.is_contiguous() and tuple(w_phase.shape[:3]) == (rate, (k + rate - 1) // rate, c_in)
    nv.check(nv.lib().ltx2_audio_conv_transpose1d(nv.ptr(x), x.stride(0), T, c_in, nv.ptr(w_phase), nv.ptr(bias), nv.ptr(out), out.stride(0), t_out,
                                                  c_out, k, rate, padding, int(prologue), float(slope), nv.stream()))
    return out


def audio_pixnorm_silu(x: torch.Tensor, eps: float = 1e-6, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(PixelNorm(x)) over the last dimension of a contiguous fp32 tensor."""
    assert x.is_contiguous()
    _f32(x)
    c = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    nv.check(nv.lib().ltx2_audio_pixnorm_silu(nv.ptr(x), c, nv.ptr(out), c, x.numel() // c, c, float(eps), nv.stream()))
    return out


def audio_snake_aa(x: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor, up_filter: torch.Tensor, down_filter: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Activation1d(SnakeBeta) of x [T, C] (x2 up / down with the given filters) -> [T, C]."""
    T, c = x.shape
    if out is None:
        out = torch.empty(T, c, device=x.device, dtype=torch.float32)
    _f32(x, alpha, beta, up_filter, down_filter, out)
    nv.check(nv.lib().ltx2_audio_snake_aa(nv.ptr(x), x.stride(0), T, c, nv.ptr(alpha), nv.ptr(beta), nv.ptr(up_filter), up_filter.numel(),
                                          nv.ptr(down_filter), down_filter.numel(), nv.ptr(out), out.stride(0), nv.stream()))
    return out


def audio_upsample(x: torch.Tensor, filt: torch.Tensor, ratio: int, pad: int, pad_left: int, t_out: int) -> torch.Tensor:
    """UpSample1d of x [T, C] -> [t_out, C]."""
    T, c = x.shape
    out = torch.empty(t_out, c, device=x.device, dtype=torch.float32)
    _f32(x, filt, out)
    nv.check(nv.lib().ltx2_audio_upsample(nv.ptr(x), x.stride(0), T, c, nv.ptr(filt), filt.numel(), ratio, pad, pad_left, nv.ptr(out), out.stride(0),
                                          t_out, nv.stream()))
    return out
