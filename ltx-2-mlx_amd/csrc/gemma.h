// Gemma-3 text-encoder prefill (model/text_encoder/gemma3.py): host launchers of the kernels in gemma.hip.
// Every launcher returns LTX2_OK / LTX2_E_INVALID / LTX2_E_HIP and sets the thread's error message on failure.
#pragma once
#include "common.h"

// Causal / sliding-window / non-causal GQA flash attention at head_dim 256 (Gemma3Attention, reference gemma3.py:186-241):
//   O[q, h*256:(h+1)*256] = softmax(scale * Q_h K_{h/ratio}^T + mask) V_{h/ratio}
// with key j visible from query i when j < Tkv and, for causal != 0, j <= i and (window == 0 or i - j < window).
// causal == 0 is the reference's attention_mask=None case (no mask at all; window must then be 0).  Q, K, V are row-major bf16 with
// 16-byte aligned rows (ld % 8 == 0, base 16-byte aligned): query head h at columns h*256 of Q, kv head g at columns g*256 of K and V.
// A query row that sees no key writes zeros.
int gemma_attn_launch(const bf16* Q, long ldq, const bf16* K, long ldk, const bf16* V, long ldv, bf16* O, long ldo, int Tq, int Tkv,
                      int heads, int kv_heads, int causal, int window, float scale, hipStream_t stream);

// In place on the fused QKV rows [rows][ld]: for each of the q_heads + kv_heads 256-wide heads at columns [0, (q_heads + kv_heads) * 256):
//   y = x * rsqrt(mean(x^2) + eps) * (1 + w)           (w = q_w for the first q_heads heads, k_w for the next kv_heads; fp32 [256])
//   y = [y1 * cos - y2 * sin, y2 * cos + y1 * sin]     (rotate-half, halves [0,128) and [128,256); cos / sin fp32 [rows][128])
int gemma_qknorm_rope_launch(bf16* qkv, long ld, int rows, int q_heads, int kv_heads, const float* q_w, const float* k_w, float eps,
                             const float* cos, const float* sin, hipStream_t stream);

// One row pass: x = x_in + rms(y) * (1 + w_post)   (y == null: x = x_in), then with n = rms(x) * (1 + w_next):
//   x_out (fp32, may be null) = x;  h_out (bf16, may be null) = n;  hf_out (fp32, may be null) = n.   D % 4 == 0, D <= 8192.
int gemma_resid_norm_launch(const float* x_in, long ldx, const bf16* y, long ldy, const float* w_post, const float* w_next, float* x_out,
                            long ldxo, bf16* h_out, long ldh, float* hf_out, long ldhf, int rows, int D, float eps, hipStream_t stream);

// out[r][i] = act(gu[r][i]) * gu[r][inter + i] (bf16), act 0 = silu, 1 = gelu (tanh form).  inter % 8 == 0.
int gemma_gated_act_launch(const bf16* gu, long ldgu, bf16* out, long ldo, int rows, int inter, int act, hipStream_t stream);

// x[r][:] = table[ids[r]][:] * scale (fp32 out); an id outside [0, vocab) writes zeros.  D % 4 == 0.
int gemma_embed_launch(const int* ids, int rows, const bf16* table, int vocab, int D, float scale, float* x, long ldx, hipStream_t stream);

// The V2 (LTX-2.3) feature extractor's GEMM operand (reference feature_extractor.py:160-181), one pass over Gemma's hidden states:
//   out[t][l * D + d] = valid[t] ? hs[l * layer_stride + t * row_stride + d] * rsqrt(mean_d(hs[l, t, :]^2) + eps) : 0
// hs fp32 (strides in elements, multiples of 4, 16-byte aligned base), valid int32 [T] or null (every token valid), out 16-bit
// [T][ldo], ldo >= L * D, ldo % 8 == 0.  fp32 sum, one rounding.  D % 8 == 0, D <= 8192.
int gemma_features_rms_launch(const float* hs, long layer_stride, long row_stride, const int* valid, bf16* out, long ldo, int T, int L, int D,
                              float eps, hipStream_t stream);
