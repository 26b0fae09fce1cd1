/*
 * ltx2hip.h -- C ABI of libltx2hip.so: the MI355X (gfx950) implementation of the LTX-2
 * denoise (DiT) + CausalVideoVAE decode hot path.
 *
 * This is the drop-in boundary.  The reference (Acelogic/LTX-2-MLX) is pure Python over
 * Apple MLX; the entry points below are what its Python layer would bind (via ctypes, see
 * INTEGRATION.md) in place of the MLX calls cited next to each function.  All paths are
 * relative to /root/reference.
 *
 * Conventions
 *   - every function returns int: 0 = LTX2_OK, negative = LTX2_E_* ; nothing throws across the
 *     boundary; ltx2_last_error() returns a thread-local message for the last failure.
 *   - all pointers are DEVICE pointers (HBM) unless named host_*; the library never allocates or
 *     frees caller memory and never retains input/output pointers beyond the call, except
 *     weights (owned by the caller for the lifetime of the context) and the bound workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only
 *     enqueues work on that stream; no internal threads; one context per GPU / process.
 *   - activations: bf16 = raw uint16 bfloat16; fp32 where stated.  Batch is 1 (the reference
 *     hard-wires batch = 1: pipelines/distilled.py:314, scripts/generate.py:1768).
 */
#ifndef LTX2HIP_H
#define LTX2HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LTX2_OK 0
#define LTX2_E_INVALID (-1) /* bad argument / unsupported shape  (Python side raises ValueError) */
#define LTX2_E_HIP (-2)     /* HIP runtime error                   (RuntimeError) */
#define LTX2_E_STATE (-3)   /* call order, missing weight, small workspace (RuntimeError) */
#define LTX2_E_UNSUPPORTED (-4) /* a valid request for a form that is not built  (NotImplementedError) */

#define LTX2_DTYPE_BF16 0
#define LTX2_DTYPE_F32 1
#define LTX2_DTYPE_FP8_E4M3FN 2   /* ltx2_dit_set_weight: codes of a fp8-resident linear weight; `<name>_scale` (fp32 [out]) must be set too */

/* Version of THIS header's signatures.  ltx2_abi_version() returns the version the library was built with; a caller compares the
 * two before its first compute call (the Python binding refuses to load a library that reports another version).  History:
 * 1 = round 1;  2 = round 2 added the `sigma` / `sigma_dev` argument to ltx2_dit_forward / ltx2_dit_denoise_step (in the middle of
 * the list: an old caller's arguments would shift silently), round 3 added ltx2_dit_health; round 4 added entry points only
 * (ltx2_clear_error, ltx2_adaln_rmsnorm2, ltx2_flash_attn_gated, ltx2_flash_attn_form, ltx2_dit_graph_capture_cond[_av], the
 * "adaln_combine" option) without bumping the version -- a round-3 library then passed the check and failed later on a symbol lookup;
 * 3 = round 5: the round-4 additions are part of the version, ltx2_flash_attn_form (the 64-rows-per-wave experiment's entry), ltx2_flash_attn_ws /
 * ltx2_flash_attn_workspace_bytes (the stream-K launch form) and ltx2_dit_health (its timeout flag) are REMOVED with their kernels, and
 * ltx2_dit_graph_capture_cond[_av] take the element counts of the mask / clean-latent buffers they replay from.  Rule from here on: any change
 * of the exported symbol set or of a signature bumps the version. */
#define LTX2_ABI_VERSION 3

const char* ltx2_last_error(void);
/* forget the calling thread's message (a binding that loads several builds of the library reads every build's message after a failure and
 * clears them all, so a stale message of one build is never reported for a failure in another; round 4, additive) */
void ltx2_clear_error(void);
int ltx2_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Per-kernel entry points (unit parity against the oracle)
 * ------------------------------------------------------------------------------------------ */

/* GEMM epilogues */
#define LTX2_EPI_BF16 0            /* out_bf16 = acc + bias */
#define LTX2_EPI_GELU_BF16 1       /* out_bf16 = gelu_tanh(acc + bias) */
#define LTX2_EPI_SILU_BF16 2       /* out_bf16 = silu(acc + bias) */
#define LTX2_EPI_F32 3             /* out_f32  = acc + bias */
#define LTX2_EPI_RESID_GATE_F32 4  /* out_f32 += gate * (acc + bias) */
#define LTX2_EPI_ADD_BF16 5        /* out_bf16 = acc + bias + res_bf16 */

/* out[M,N] = epilogue(A[M,K] @ W[N,K]^T + bias).  Replaces mlx nn.Linear on the DiT path:
 * model/transformer/attention.py:225-228,253 (to_q/k/v/out), feed_forward.py:23,49 (FFN),
 * model.py:49-56 (caption projection), model.py:242 (patchify_proj), model.py:757 (proj_out),
 * and the fused helpers transformer.py:35-46 (_compiled_residual_gate: epilogue 4) and
 * feed_forward.py:26 (gelu_approx: epilogue 1).
 * gate (epilogue 4): gate[m*gate_stride + n] (+ gate_table[n]); both NULL -> 1.            */
int ltx2_gemm_bf16(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M,
                   int N, int K, int epilogue, const float* gate, int64_t gate_stride, const float* gate_table,
                   const void* res, int64_t ldres, void* stream);

/* Fused QKV projection (attention.py:196-214: to_q / to_k / to_v on the same input): out[M][N] = A @ W^T + bias for the columns
 * < vt_col0 (Q and K), while the columns >= vt_col0 (V, heads of head_dim) leave as attention's V^T operand vt[H][head_dim][Npad]
 * with the key order ltx2_vt_transpose produces (rows >= M zero up to Npad) -- written by the GEMM's epilogue on the shapes the
 * 4-wave kernel takes (M >= 1024, N % 256 == 0, vt_col0 % 256 == 0, K % 128 == 0; *fused = 1), else by a transpose pass after
 * the GEMM (*fused = 0; the V columns of `out` are then written too).  Bit-identical to ltx2_gemm_bf16 + ltx2_vt_transpose. */
int ltx2_gemm_qkv_vt(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M, int N, int K,
                     void* vt, int vt_col0, int Npad, int head_dim, int* fused, void* stream);

/* fp8-RESIDENT weights (reference loader/fp8_loader.py:14-51,54-130 dequantises at load; BASELINE config 3): W8 = float8_e4m3fn
 * codes [N][K], wscale[N] fp32 = the checkpoint's per-tensor `weight_scale` repeated per output row (fused q/k/v carry one
 * value per part).  The kernel expands bf16(f32(code) * wscale[n]) on the way from LDS to the MFMA -- exactly
 * ltx2_dequant_fp8_e4m3fn's arithmetic -- so out is BIT-IDENTICAL to ltx2_gemm_bf16 on the dequantised weights.
 * N % 256 == 0, K % 128 == 0, K >= 256; epilogues BF16 / GELU_BF16 / F32 / RESID_GATE_F32.                          */
int ltx2_gemm_w8a16(const void* A, int64_t lda, const void* W8, const float* wscale, const float* bias, void* out, int64_t ldo, int M,
                    int N, int K, int epilogue, const float* gate, int64_t gate_stride, const float* gate_table, void* stream);

/* Text cross-attention with q_norm folded in (attention.py:231-237 applied as arithmetic instead of a pass over q; round 3).
 * ltx2_gemm_bf16_rowss: out = A @ W^T + bias (bf16) and, where the 4-wave kernel takes the shape (*written = 1), rowss[m][N / 64] = the
 * sums of squares of out's ROUNDED values over each 64-column strip of row m; *written = 0: plain GEMM, rowss untouched.
 * ltx2_flash_attn_rowscale: ltx2_flash_attn with a per-query-row scale: row q uses scale * rsqrt(sum_j q_ss[q][j] / q_norm_dim + q_eps),
 * i.e. softmax((rms_norm(Q) K'^T) * scale) V for K' carrying q_norm.weight * k_norm.weight -- identical to normalising Q first up to the
 * rounding of the normalised Q to 16 bits (which this form does not do).  head_dim 128, q_ss_ld % 16 == 0 (ABI 3: the row's four lanes read f32x4 quarters; rows 64-byte aligned).                     */
int ltx2_gemm_bf16_rowss(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M, int N, int K, float* rowss,
                         int* written, void* stream);
int ltx2_flash_attn_rowscale(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                             int H, int head_dim, float scale, const float* q_ss, int q_ss_ld, int q_norm_dim, float q_eps, void* stream);

/* An RMS norm folded around two GEMMs (round 6; rms_norm + nn.Linear, transformer.py:217-226, as arithmetic instead of a pass over x):
 * rms_norm(x) (1 + s) in front of a projection (W, b) equals r (x (1 + s)) W^T + b, r[m] = rsqrt(mean_j x[m][j]^2 + eps).
 * ltx2_gemm_bf16_fold: ltx2_gemm_bf16 with the producer / consumer half of that identity:
 *   epilogue RESID_GATE_F32 (x += gate_table * (acc + bias), row-invariant gate): shadow[m][n] = 16-bit(x_new[m][n] * (1 + shadow_scale[n]))
 *     (row stride ld_shadow; shadow_scale null: * 1) and shadow_ss[(n / 256) * ld_ss + m] = the sum of x_new[m][n]^2 over each 256-column tile
 *     (ld_ss >= the row tiles' extent: M rounded up to a multiple of 256 is always enough; % 4 == 0); shadow_scale 16-byte aligned (the epilogue loads
 *     four floats at a time) and ld_shadow >= N (narrower rows would overlap), else *supported = 0;
 *   epilogue BF16 / GELU_BF16: out = epilogue(r[m] * acc + bias) with r[m] = rsqrt(sum_{j < rf_nparts} rf_parts[j * rf_ld + m] / rf_dim + rf_eps)
 *     formed inside the kernel (rf_parts = a producer's shadow_ss, rf_nparts <= 24).
 *   *supported = 0 (nothing launched) when the 4-wave layout-3 kernel does not take the problem (M >= 1024, N % 256 == 0, K % 128 == 0, dense 16-bit
 *   weights, the bfloat16 build) or neither half is asked for.                                                                                      */
int ltx2_gemm_bf16_fold(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M, int N, int K, int epilogue,
                        const float* gate_table, void* shadow, int64_t ld_shadow, const float* shadow_scale, float* shadow_ss, int64_t ld_ss,
                        const float* rf_parts, int64_t rf_ld, int rf_nparts, int rf_dim, float rf_eps, int* supported, void* stream);

/* flash attention with a key mask (attention.py:38-70 with the additive mask model.py:163-201 builds from a boolean (B, S) context
 * mask): mask fp32 [Nkv], non-zero = the key may be attended; a masked key takes no weight unless every key is masked (then the
 * row averages V over all keys, as the reference's -finfo.max bias does).  words: scratch of Npad / 8 bytes on the device.        */
int ltx2_flash_attn_keymask(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo,
                            int Nq, int Nkv, int H, int head_dim, float scale, const float* mask, void* words, void* stream);

/* Which kernel ltx2_gemm_bf16 / ltx2_gemm_w8a16 / ltx2_gemm_fp8 (weights = 0 / 1 / 2) would run for a dense M x N x K problem with
 * this epilogue -- host logic only, nothing is launched, no GPU needed.  Returns LTX2_ROUTE_* (negative: unsupported), OR-ed with
 * 0x100 when has_vt != 0 and the fused-QKV V^T output (ltx2_gemm_qkv_vt with N = 3 * inner_dim) would come from the GEMM's own epilogue.
 * The dispatch is a parity surface: tests pin the route of every GEMM the models issue.                                  */
#define LTX2_ROUTE_SKINNY 0     /* gemm_skinny.hip: M <= 128 rows, weight streaming                         */
#define LTX2_ROUTE_V4_224 1     /* gemm_v4.hip, generated asm K loop, 224 x 256 tiles                       */
#define LTX2_ROUTE_V4_256 2     /*                                    256 x 256 tiles                       */
#define LTX2_ROUTE_V4_W8_224 3  /* ... fp8-resident weights expanded to bf16 in the loop                     */
#define LTX2_ROUTE_V4_W8_256 4
#define LTX2_ROUTE_V4_F8_224 5  /* ... fp8 compute (v_mfma_f32_32x32x64_f8f6f4)                             */
#define LTX2_ROUTE_V4_F8_256 6
#define LTX2_ROUTE_PP 7         /* gemm_pp.hip: 256 x 256 ping-pong                                         */
#define LTX2_ROUTE_SMALL 8      /* gemm.hip: 128 x 128                                                      */
#define LTX2_ROUTE_NARROW 9     /* gemm.hip: 128 x 64 (N <= 64)                                             */
int ltx2_gemm_route(int M, int N, int K, int epilogue, int weights, int has_vt);

/* fp8 COMPUTE (BASELINE config 3, "fp8 weights (CDNA4 fp8 MFMA)"; opt-in, not the parity-exact default): both operands are
 * float8_e4m3fn codes, the products run on v_mfma_f32_32x32x64_f8f6f4 at twice the bf16 MFMA rate, fp32 accumulation;
 *   out = epilogue(ascale[m] * wscale[n] * sum_k f32(A8[m][k]) * f32(W8[n][k]) + bias[n]).
 * ltx2_quantize_rows_fp8 is the quantiser of both sides: scale[r] = max_k |x[r][k]| / 448 (1 for an all-zero row), codes[r][k] =
 * e4m3fn_rne(x[r][k] * (1 / scale[r])) -- per TOKEN for activations, per OUTPUT CHANNEL for weights quantised at load (an fp8
 * checkpoint's codes + per-tensor `weight_scale`, reference loader/fp8_loader.py:14-51, are used as they are).
 * N % 256 == 0, K % 256 == 0, K >= 512, lda % 16 == 0; epilogues BF16 / GELU_BF16 / F32 / RESID_GATE_F32.                    */
int ltx2_quantize_rows_fp8(const void* x_bf16, int64_t ldx, int rows, int K, void* codes, int64_t ldo, float* scale, void* stream);
int ltx2_gemm_fp8(const void* A8, int64_t lda, const float* ascale, const void* W8, const float* wscale, const float* bias, void* out,
                  int64_t ldo, int M, int N, int K, int epilogue, const float* gate, int64_t gate_stride, const float* gate_table,
                  void* stream);

/* ltx2_gemm_qkv_vt on the fp8 compute path (same contract: V columns leave as attention's V^T operand). */
int ltx2_gemm_fp8_qkv_vt(const void* A8, int64_t lda, const float* ascale, const void* W8, const float* wscale, const float* bias, void* out,
                         int64_t ldo, int M, int N, int K, void* vt, int vt_col0, int Npad, int head_dim, int* fused, void* stream);

/* Skinny fp32-activation path (M <= 16): out_f32 = act_out(act_in(a) @ W^T + bias); act: 0 none,
 * 1 silu, 2 gelu_tanh.  Replaces TimestepEmbedding / AdaLayerNormSingle linears for a scalar
 * sigma (model/transformer/timestep_embedding.py:112-124,187-202) and the VAE TimestepEmbedder
 * (model/video_vae/simple_decoder.py:54-59).                                                 */
int ltx2_gemv_f32(const float* a, int64_t lda, const void* W, const float* bias, float* out, int64_t ldo, int M,
                  int N, int K, int act_in, int act_out, void* stream);

/* 3x3x3 stride-1 conv3d on channels-last bf16 activations x[T][H][W][Cin], weights
 * w[Cout][27][Cin] (tap = (kt*3+kh)*3+kw), reflect pad H/W, replicate pad T (causal: 2 front).
 * Replaces Conv3dSimple.__call__ (model/video_vae/simple_decoder.py:90-180).
 *   mode 0: out[T][H][W][Cout] = conv + bias
 *   mode 1: out = conv + bias + res          (ResBlock3d skip, simple_decoder.py:240)
 *   mode 2: depth-to-space upsample epilogue (DepthToSpaceUpsample3d, simple_decoder.py:287-313):
 *           weight rows must be pre-permuted to n' = s*Cf + c (s = (a*fh+b)*fw+d, Cf = Cout/(ft*fh*fw));
 *           out[T*ft - (ft>1)][H*fh][W*fw][Cf]; residual != 0 adds tile(d2s(x)).                */
int ltx2_conv3d_fused(const void* x, const void* w, const float* bias, void* out, int T, int H, int W, int Cin,
                      int Cout, int causal, int mode, const void* res, int ft, int fh, int fw, int residual,
                      int pad_zero, int kt, void* stream);
/* pad_zero = 1: zero padding in T/H/W instead of reflect/replicate (spatial upscaler, upscaler/spatial.py:20-87);
 * pad_zero = 2: zero padding in H/W, replicated temporal edge (VAE encoder Conv3dSimple, simple_encoder.py:44-75);
 * kt = 1: per-frame 3x3 conv2d (weight [Cout][9*Cin]); with mode 2, ft=1, fh=fw=2 the epilogue is
 * PixelShuffle(2) (SpatialRationalResampler, upscaler/spatial.py:267-323).                               */

/* GroupNorm over (C/groups, T, H, W) on channels-last bf16 x[P][C] (upscaler/spatial.py:89-128), fused with the
 * affine, an optional residual add and SiLU:  y = silu(gn(x) * gamma + beta + res).  scratch: 2*groups*(1 +
 * ceil(P/16)) floats (two-level reduction without atomics: bit-reproducible).  act = 0 skips the SiLU.   */
int ltx2_groupnorm_silu(const void* x, const void* res, void* y, int64_t P, int C, int groups, float eps,
                        const float* gamma, const float* beta, float* scratch, int act, void* stream);

/* Per-frame GroupNorm of the temporal upscaler (upscaler/temporal.py:128-147, 278-285: reshape to (B*T, H, W, C), then
 * mlx.nn.GroupNorm): x[frames][P_frame][C] channels-last 16-bit, statistics per (frame, group), fused with the affine, an
 * optional residual add and SiLU as above.  interleaved != 0: group of channel c is c % groups (mlx.nn.GroupNorm without
 * pytorch_compatible, what the reference constructs); interleaved == 0: c / (C/groups) (torch.nn.GroupNorm).  One launch;
 * a frame's slab of groups stays in registers between the sums and the apply where it fits, otherwise x is read twice.
 * Statistics and the affine are fp64, in a fixed order without atomics (bit-reproducible).  scratch is unused (may be
 * null): it keeps the call shape of ltx2_groupnorm_silu.  Accepts every (C, groups) that entry accepts.          */
int ltx2_groupnorm_frames_silu(const void* x, const void* res, void* y, int frames, int64_t P_frame, int C, int groups,
                               int interleaved, float eps, const float* gamma, const float* beta, float* scratch, int act,
                               void* stream);

/* VAE encoder SpaceToDepthDownsample3d tail (simple_encoder.py:183-257): y = conv(x') [T][H][W][Cc] and the conv
 * input x' [T][H][W][Cin] (first frame already duplicated when st = 2) ->
 * out[T/st][H/sh][W/sw][Cc*sp] = space_to_depth(y) + group_mean(space_to_depth(x')), sp = st*sh*sw,
 * channel c*sp + (a*sh + b)*sw + d, groups of Cin*sp / (Cc*sp) consecutive space-to-depth channels.      */
int ltx2_s2d_downsample(const void* y, const void* x, void* out, int T, int H, int W, int Cc, int Cin, int st, int sh,
                        int sw, void* stream);

/* Upscaler output: x bf16 [P][C] -> out fp32 [C][P] = (x - mean[c]) / std[c]  (PerChannelStatistics.normalize,
 * video_vae/ops.py:173-186).                                                                             */
int ltx2_latent_normalize_nchw(const void* x, const float* mean, const float* std, float* out, int C, int64_t P,
                               void* stream);

/* out_bf16 = norm(x_f32) * (1 + scale) + shift ; scale = scale_tab[d] + scale_emb[row*emb_stride+d].
 * layer_norm = 0: RMS  (transformer.py:16-31 _compiled_adaln_forward; attention.py:88-100 rms_norm)
 * layer_norm = 1: LayerNorm without affine (model.py:553,744-758).  NULL pointers contribute 0.   */
int ltx2_adaln_rmsnorm(const float* x, int64_t ldx, void* out, int64_t ldo, int rows, int D, float eps,
                       int layer_norm, const float* scale_tab, const float* shift_tab, const float* scale_emb,
                       const float* shift_emb, int64_t emb_stride, void* stream);
/* Two modulations of ONE RMS-normalised stream from one read of x (round 4; the cross-modal attention's a2v / v2a inputs, transformer.py:556-620):
 * out_g = rms_norm(x) * (1 + scale_g) + shift_g, g = 0, 1 (row-invariant fp32 vectors [D], any may be null).  D <= 4096.            */
int ltx2_adaln_rmsnorm2(const float* x, int64_t ldx, void* out0, void* out1, int64_t ldo, int rows, int D, float eps, const float* scale0,
                        const float* shift0, const float* scale1, const float* shift1, void* stream);

/* The same with the fp8 compute path's per-token quantiser fused in: codes[rows][ldq] + scale[rows] = ltx2_quantize_rows_fp8 of the
 * bf16-rounded outputs, bit for bit; out_bf16 may be NULL (the GEMM that follows reads only the codes).                    */
int ltx2_adaln_rmsnorm_fp8(const float* x, int64_t ldx, void* out_bf16, int64_t ldo, void* codes, int64_t ldq, float* scale, int rows, int D,
                           float eps, int layer_norm, const float* scale_tab, const float* shift_tab, const float* scale_emb,
                           const float* shift_emb, int64_t emb_stride, void* stream);

/* In place on bf16 rows: RMSNorm(weight) over the full inner dim of q (and k), then SPLIT RoPE
 * (cos/sin fp32 [rows][D/2], slot h*hd/2 + j) if cos != NULL.
 * Replaces attention.py:231-237 + rope.py:92-144.  k_* may be NULL/absent (nseg = 1).        */
int ltx2_qknorm_rope(void* buf, int64_t ld, int rows, int D, int head_dim, int q_off, const float* q_weight,
                     int k_off, const float* k_weight, float eps, const float* cos, const float* sin, void* stream);

/* V[Nkv][ld] (head h at columns h*hd) -> VT[H][hd][Npad], keys permuted inside each block of 32
 * to match the MFMA accumulator layout of the attention kernel (ABI 3: position 8g + 4h + r of a block holds key 16h + 4g + r -- the
 * 16x16x32 kernel's order; a V^T written by an ABI-2 library is NOT valid for this one); padded keys are zero.
 * head_dim hd = 128 (video streams) or 64 (audio streams, audio<->video attention).          */
int ltx2_vt_transpose(const void* V, int64_t ld, void* VT, int Nkv, int Npad, int H, int head_dim, void* stream);

/* out[q][h*hd..] = softmax(Q_h K_h^T * scale) V_h, non-causal, no mask, head_dim 128 or 64; ldq, ldk, ldo multiples of 8 (16-byte rows).
 * Replaces _compiled_attention_core_no_mask (attention.py:12-34).                             */
int ltx2_flash_attn(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out,
                    int64_t ldo, int Nq, int Nkv, int H, int head_dim, float scale, void* stream);


/* Per-head attention gates (V2.3, attention.py:241-249): logits[rows][H] (fp32 scratch, also returned)
 * = x[rows][Dq] @ gate_w[H][Dq]^T + gate_b ; att[:, h*hd:(h+1)*hd] *= 2*sigmoid(logits[:, h]).  H <= 32. */
int ltx2_attn_head_gate(void* att, int64_t ld, const void* x, int64_t ldx, const void* gate_w, const float* gate_b,
                        float* logits, int rows, int Dq, int H, int head_dim, void* stream);

/* ltx2_flash_attn with the per-head gates applied in the kernel's epilogue (round 4: the engine's form -- the gate multiplies the fp32 result
 * before it is rounded, instead of a pass over the rounded output): out[q, h*hd:(h+1)*hd] = 2*sigmoid(gate_logits[q*gate_ld + h]) * attention. */
int ltx2_flash_attn_gated(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                          int H, int head_dim, float scale, const float* gate_logits, int gate_ld, void* stream);

/* The engine's form of the gated attention for many rows (round 5): the gate logits x[Nq][Dq] @ gate_w[H][Dq]^T leave as 8 partial sums over K slices
 * (parts: fp32 scratch [8][Nq][H]; H <= 32, Dq % 256 == 0, ldx % 8 == 0), and the attention kernel's epilogue adds the 8 values and gate_b in slice order before
 * 2 * sigmoid(.) multiplies the fp32 result -- ltx2_attn_head_gate's logits up to the summation order.                                              */
int ltx2_flash_attn_gated_parts(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                                int H, int head_dim, float scale, const void* x, int64_t ldx, const void* gate_w, const float* gate_b, int Dq, float* parts,
                                void* stream);

/* SPLIT-RoPE tables (precompute_freqs_cis with use_middle_indices_grid, rope.py:214-328,365-418): positions fp32
 * [n_dims][N][2] = [start, end) per axis, freq_grid [n_freq] = theta^linspace(0,1,n_freq)*pi/2 (host-computed, exact),
 * max_pos [n_dims]; writes cos/sin fp32 [N][half_dim], slot = pad + f*n_dims + d, pad = half_dim - n_dims*n_freq
 * identity slots in FRONT.  Replaces the per-step table rebuild of model.py:203-229.                    */
int ltx2_rope_tables(const float* positions, const float* freq_grid, const float* max_pos, int N, int n_dims, int n_freq,
                     int half_dim, float* cos_out, float* sin_out, void* stream);

/* [cos | sin] sinusoid, dim 256 (timestep_embedding.py:10-60 with flip_sin_to_cos, shift 0;
 * simple_decoder.py:12-39).  Either output may be NULL.                                       */
int ltx2_timestep_sinusoid(const float* t, int64_t t_stride, float mult, int T, int dim, float* out_f32,
                           void* out_bf16, void* stream);

/* Load-time dequantisation of fp8 checkpoints: out_bf16[i] = bf16(f32(e4m3fn in[i]) * weight_scale)
 * (loader/weight_converter.py:391-395, loader/fp8_loader.py:14-51).                            */
int ltx2_dequant_fp8_e4m3fn(const void* in, float scale, void* out_bf16, int64_t n, void* stream);
int ltx2_cast_f32_bf16(const float* in, void* out, int64_t n, void* stream);

/* x0 = latent - ts * velocity  (X0Model.__call__, model.py:912-918); ts_ptr NULL -> ts_scalar. */
int ltx2_x0_from_velocity(const float* latent, const float* velocity, const float* ts_ptr, int64_t ts_stride,
                          float ts_scalar, float* x0, int rows, int C, void* stream);

/* post_process_latent + EulerDiffusionStep.step fused (pipelines/common.py:169-190,
 * components/diffusion_steps.py:36-67, scripts/generate.py:905-930).  sigma == 0 -> LTX2_E_INVALID
 * with message "Sigma can't be 0.0" (core_utils.py:54-55).  mask/clean may both be NULL.      */
int ltx2_euler_step(const float* x, const float* x0, const float* mask, const float* clean, float sigma,
                    float sigma_next, float* out, int rows, int C, void* stream);

/* One classifier-free-guided sampling step in ONE pass over [rows][C] fp32 (pipelines/one_stage.py:224-330 with CFGGuider): the two
 * x0_from_velocity launches, the guider's three ops, post_process_latent's four and the Euler update.  Per element, every operation
 * individually rounded (no FMA contraction), so the result equals the separate fp32 torch ops bit for bit:
 *   t = ts[row * ts_stride];  a = x - t*vel_cond;  b = x - t*vel_uncond;  g = a + (cfg_scale - 1)*(a - b);
 *   d = mask ? g*mask[row] + clean*(1 - mask[row]) : g;  out = x + ((x - d) * (1/sigma)) * (sigma_next - sigma)
 * ts_stride: 0 = one timestep, 1 = one per row.  mask [rows] and clean [rows][C] are both NULL or both set.  out may equal x.
 * sigma == 0 -> LTX2_E_INVALID with message "Sigma can't be 0.0".  (additive entry of ABI version 3)                          */
int ltx2_guided_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride,
                           const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next,
                           float* out, int rows, int C, void* stream);

/* ltx2_guided_euler_step over TWO latents in ONE launch (the video and the audio latent of a joint guided step; the audio one is ~100 rows, a
 * launch of its own nearly all latency): v_ then a_, each with its own operands, cfg_scale, timesteps, mask / clean and shape; sigma and
 * sigma_next are shared.  The per-element arithmetic is ltx2_guided_euler_step's, so each segment's output equals the single launch's bit for
 * bit.  16-byte accesses only when both segments allow them.  sigma == 0 -> LTX2_E_INVALID with message "Sigma can't be 0.0".
 * (additive entry of ABI version 3)                                                                                                      */
int ltx2_guided_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                                const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                                const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next,
                                void* stream);

/* Counter-based noise for the stochastic sampler: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85).
 * Quad q has the counter (lo32(q), hi32(q), step, stream_id) and the key (lo32(seed), hi32(seed)); its four words r0..r3 serve the elements
 * 4q .. 4q+3 of a latent.  seed_dev: a device pointer to one 64-bit word (8-byte aligned), read when the kernel runs -- a captured graph serves
 * any seed.  stream_id: 0 the video latent, 1 the audio latent.
 *   ltx2_philox_bits:   out[n_quads][4], the raw words (the hook for the Random123 known-answer vectors).
 *   ltx2_philox_normal: out[n] fp32 N(0,1): u_k = ((r_k >> 9) + 0.5)*2^-23 (exact, inside (0, 1)); z0 = sqrt(-2 ln u0)*cos(2 pi u1),
 *                       z1 = sqrt(-2 ln u0)*sin(2 pi u1), z2 / z3 from (u2, u3); accurate logf / sincospif, every operation rounded on its own.
 * The values are a function of (seed, step, stream_id, element index) alone: not of the grid, the access width or n.
 * (additive entries of ABI version 3)                                                                                                      */
int ltx2_philox_bits(uint32_t* out, int64_t n_quads, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, void* stream);
int ltx2_philox_normal(float* out, int64_t n, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, void* stream);

/* The Euler-ancestral step (EulerAncestralDiffusionStep, reference components/diffusion_steps.py:70-129) in ONE pass with the noise made in the
 * kernel.  sigma_up / sigma_down: _get_ancestral_step(sigma, sigma_next, eta) evaluated by the caller in double.  Per element:
 *   d as ltx2_guided_euler_step forms it;  r = x + ((x - d) * (1/sigma)) * (sigma_down - sigma);  out = r + ((z * sigma_up) * m)
 * with z = the ltx2_philox_normal value of element row*C + c under (seed, step, stream 0) and m = mask[row] (1 without a mask).  The mask on the
 * noise is a departure from the reference, which adds noise to conditioned tokens too; with m = 1 the arithmetic is the reference's.
 * vel_uncond NULL: no guidance, and r in the arithmetic of ltx2_x0_from_velocity + ltx2_euler_step.  sigma_up == 0: no noise is evaluated and
 * out = r, ltx2_guided_euler_step's bits for sigma_next = sigma_down.  out may equal any input.  LTX2_E_INVALID: sigma == 0 ("Sigma can't be
 * 0.0"), a negative sigma_up / sigma_down, seed_dev NULL or off its 8-byte boundary, and the rules of ltx2_guided_euler_step.
 * _pair: the video latent (stream 0) then the audio latent (stream 1) in one launch, each segment the single launch's bits.
 * _x0: from a ready x0; d = clean ? x0*m + clean*(1 - m) : x0.  A mask WITHOUT a clean latent scales the noise alone (the caller has blended x0).
 * (additive entries of ABI version 3)                                                                                                      */
int ltx2_ancestral_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                              const float* clean, float cfg_scale, float sigma, float sigma_up, float sigma_down, const uint64_t* seed_dev,
                              uint32_t step, float* out, int rows, int C, void* stream);
int ltx2_ancestral_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                                   const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                   const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                                   const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_up,
                                   float sigma_down, const uint64_t* seed_dev, uint32_t step, void* stream);
int ltx2_ancestral_euler_step_x0(const float* x, const float* x0, const float* mask, const float* clean, float sigma, float sigma_up, float sigma_down,
                                 const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, float* out, int rows, int C, void* stream);

/* ltx2_guided_euler_step with spatio-temporal guidance (STG) on top: STGGuider.guide applied to the CFG-guided x0 (pipelines/one_stage.py:284-297).
 * vel_perturbed is the velocity of a forward whose chosen self-attentions were skipped (ltx2_dit_forward_perturbed).  Per element, every
 * operation individually rounded, so the result equals the separate fp32 torch ops bit for bit:
 *   t = ts[row * ts_stride];  a = x - t*vel_cond;  b = x - t*vel_uncond;  g = vel_uncond ? a + (cfg_scale - 1)*(a - b) : a
 *   p = x - t*vel_perturbed;  s = g + stg_scale*(g - p)
 *   d = mask ? s*mask[row] + clean*(1 - mask[row]) : s;  out = x + ((x - d) * (1/sigma)) * (sigma_next - sigma)
 * vel_uncond may be NULL (the guider is not enabled: no CFG).  ts_stride, mask / clean as above; out may equal any input.  16-byte accesses when
 * C % 4 == 0 and every [rows][C] operand is 16-byte aligned, element-wise otherwise.  sigma == 0 -> LTX2_E_INVALID with message
 * "Sigma can't be 0.0".  (additive entry of ABI version 3)                                                                              */
int ltx2_stg_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* ts,
                        int64_t ts_stride, const float* mask, const float* clean, float cfg_scale, float stg_scale, float sigma, float sigma_next,
                        float* out, int rows, int C, void* stream);

/* ltx2_stg_euler_step over TWO latents in ONE launch (the video and the audio latent of a joint STG step), on the two-segment scaffold of
 * ltx2_guided_euler_step_pair: v_ then a_, each with its own operands, cfg_scale, stg_scale, timesteps, mask / clean and shape; sigma and sigma_next
 * are shared.  The per-element arithmetic is ltx2_stg_euler_step's, so each segment's output equals the single launch's bit for bit.  Per segment,
 * independently: vel_uncond may be NULL (no CFG on that modality) and vel_perturbed may be NULL -- then s = g, ltx2_guided_euler_step's arithmetic
 * (a modality that is not STG-guided, a step past the cutoff); both NULL: out = x + ((x - d) * (1/sigma)) * (sigma_next - sigma) with d from
 * a = x - t*vel_cond alone.  16-byte accesses only when both segments allow them, element-wise otherwise.  sigma == 0 -> LTX2_E_INVALID with message
 * "Sigma can't be 0.0".  (additive entry of ABI version 3)                                                                                */
int ltx2_stg_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed, const float* v_ts,
                             int64_t v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float v_stg_scale, float* v_out,
                             int v_rows, int v_C, const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed,
                             const float* a_ts, int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float a_stg_scale,
                             float* a_out, int a_rows, int a_C, float sigma, float sigma_next, void* stream);

/* The res_2s second-order exponential-integrator step (pipelines/ti2vid_hq.py:153-273) as two passes over [rows][C] fp32, every operation
 * individually rounded (no FMA contraction), so each equals the separate fp32 array ops of the reference bit for bit.  The guided, blended
 * x0 of a pair of velocities, in the HQ pipeline's own order (:315, not CFGGuider's):
 *   t = ts[row * ts_stride];  a = x - t*vel_cond;  b = x - t*vel_uncond;  g = b + cfg_scale*(a - b)   (g = a when vel_uncond is NULL)
 *   d = mask ? g*mask[row] + clean*(1 - mask[row]) : g
 * ltx2_res2s_midpoint:  an = x;  e = d - an;  xm = an + c*e;  n_bong times { an = xm - c*e;  e = d - an };  x_mid = xm, anchor = an, eps1 = e.
 *   c = fp32(h * a21), n_bong = 100 when h < 0.5 and sigma > 0.03 else 0 (the caller decides; any n_bong >= 0).  x_mid may equal x.
 *   anchor == eps1 == NULL: the reference's final-step branch (h == 0 or sigma_next <= 0.001): x_mid = d and nothing else is written.
 * ltx2_res2s_combine:   d2 as d from (x_mid, velocities, ts at the sub-sigma);  e2 = d2 - anchor;  out = anchor + h*(b1*eps1 + b2*e2).
 *   out may equal any [rows][C] operand.
 * ts_stride: 0 = one timestep, 1 = one per row.  mask [rows] and clean [rows][C] are both NULL or both set.  16-byte accesses when C % 4 == 0
 * and every [rows][C] operand is 16-byte aligned, element-wise otherwise.  (additive entries of ABI version 3)                          */
int ltx2_res2s_midpoint(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                        const float* clean, float cfg_scale, float c, int n_bong, float* x_mid, float* anchor, float* eps1, int rows, int C,
                        void* stream);
int ltx2_res2s_combine(const float* x_mid, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                       const float* clean, float cfg_scale, const float* anchor, const float* eps1, float h, float b1, float b2, float* out,
                       int rows, int C, void* stream);
/* The same two passes over TWO latents in ONE launch -- the video and the audio latent of a joint step (pipelines/ti2vid_hq.py:217-268), the
 * audio one about a hundred rows.  The single forms' operands twice, v_ then a_; each segment has its own cfg_scale, ts / ts_stride,
 * mask / clean and rows / C, while c / n_bong and h / b1 / b2 are shared.  Each segment's output equals the single entry's bit for bit.
 * 16-byte accesses only when BOTH segments qualify.  The final-step form (anchor == eps1 == NULL) applies to both segments together.
 * (additive entries of ABI version 3)                                                                                                  */
int ltx2_res2s_midpoint_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                             const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_x_mid, float* v_anchor, float* v_eps1, int v_rows,
                             int v_C, const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride,
                             const float* a_mask, const float* a_clean, float a_cfg_scale, float* a_x_mid, float* a_anchor, float* a_eps1, int a_rows,
                             int a_C, float c, int n_bong, void* stream);
int ltx2_res2s_combine_pair(const float* v_x_mid, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                            const float* v_mask, const float* v_clean, float v_cfg_scale, const float* v_anchor, const float* v_eps1, float* v_out,
                            int v_rows, int v_C, const float* a_x_mid, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts,
                            int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, const float* a_anchor,
                            const float* a_eps1, float* a_out, int a_rows, int a_C, float h, float b1, float b2, void* stream);

/* The Heun sampler of OneStagePipeline (pipelines/one_stage.py:334-464, components/diffusion_steps.py:132-190) as two passes over [rows][C] fp32,
 * with the GE velocity correction (:300-307) in the first.  Every operation individually rounded (no FMA contraction), so each equals the separate
 * fp32 torch ops bit for bit.  With inv = 1/sigma, inv_next = 1/sigma_next, dt = sigma_next - sigma formed in fp32 on the host:
 * ltx2_heun_predict:
 *   t = ts[row * ts_stride];  a = x - t*vel_cond;  b = x - t*vel_uncond;  g = a + (cfg_scale - 1)*(a - b)   (g = a when vel_uncond is NULL)
 *   prev != NULL (GE; goes with ge_gamma > 0):  cur = (x - g)*inv;  first == 0: g = x - (ge_gamma*(cur - prev) + prev)*sigma;  then prev = cur
 *     (the UNcorrected velocity; first != 0: the old content of prev is not read)
 *   d = mask ? g*mask[row] + clean*(1 - mask[row]) : g;  xp = x + ((x - d)*inv)*dt
 *   xp == NULL: the final-step form (sigma_next == 0: the step ends with d), d alone is written.  d == NULL: xp alone, which is the Euler step
 *   with GE -- ltx2_ge_euler_step is that form, `out` being xp.  d / xp may equal x.
 * ltx2_heun_correct:  d2 as d, without GE, from (xp, the velocities and ts at sigma_next);  v1 = (x - d)*inv;  v2 = (xp - d2)*inv_next;
 *   out = x + (0.5*(v1 + v2))*dt.  out may equal any [rows][C] operand.
 * ts_stride: 0 = one timestep, 1 = one per row.  mask [rows] and clean [rows][C] are both NULL or both set.  16-byte accesses when C % 4 == 0
 * and every [rows][C] operand is 16-byte aligned, element-wise otherwise.  LTX2_E_INVALID: sigma <= 0, for the corrector sigma_next <= 0,
 * ge_gamma < 0, a GE state without ge_gamma > 0 or the reverse.
 * The _pair entries: the same over TWO latents in ONE launch (the video and the audio latent of the joint loop, :570-729), v_ then a_, each
 * with its own cfg_scale, ts / ts_stride, mask / clean and rows / C; GE acts on the video alone, as the reference keeps prev_velocity for the
 * video alone.  Each segment's output equals the single entry's bit for bit; 16-byte accesses only when BOTH segments qualify; the
 * predictor's form (d, xp or both) applies to both segments together.  (additive entries of ABI version 3)                              */
int ltx2_heun_predict(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                      const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* d, float* xp,
                      int rows, int C, void* stream);
int ltx2_heun_correct(const float* x, const float* d, const float* xp, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride,
                      const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, float* out, int rows, int C, void* stream);
int ltx2_ge_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                       const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* out, int rows,
                       int C, void* stream);
int ltx2_heun_predict_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride, const float* v_mask,
                           const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_d, float* v_xp, int v_rows, int v_C,
                           const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                           const float* a_clean, float a_cfg_scale, float* a_d, float* a_xp, int a_rows, int a_C, float sigma, float sigma_next,
                           void* stream);
int ltx2_heun_correct_pair(const float* v_x, const float* v_d, const float* v_xp, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts,
                           int64_t v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C,
                           const float* a_x, const float* a_d, const float* a_xp, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts,
                           int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma,
                           float sigma_next, void* stream);
int ltx2_ge_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride, const float* v_mask,
                            const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_out, int v_rows, int v_C,
                            const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                            const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next, void* stream);

/* Guiders whose scalars are sums over the whole latent -- CFGStarRescalingGuider, LtxAPGGuider, LegacyStatefulAPGGuider (components/guiders.py:51-76,
 * 105-205) -- as two passes over [rows][C] fp32.  Every fp32 operation is individually rounded (no FMA contraction); the sums are fp64.
 * ltx2_guidance_sums, per element:
 *   t = ts[row * ts_stride];  a = x - t*vel_cond;  b = x - t*vel_uncond;  g = a - b
 *   running != NULL (momentum): first == 0: g = momentum*running + g;  then running = g   (first != 0: running = g, the old content is not read)
 *   S_aa = sum a*a, S_ab = sum a*b, S_bb = sum b*b, S_gg = sum g*g, S_ga = sum g*a, each product exact in fp64, over ALL rows.
 *   Order: per thread in loop order, across the wave, across the block; partials[block][5] fp64 in that order of sums, one row per block.
 *   The number of blocks is ltx2_guidance_sums_blocks(rows, C), a function of the shape alone; partials is 8-byte aligned.
 * ltx2_projected_euler_step: every block adds the partial rows in index order (all blocks hold the same sums), derives the scalars in fp64 and
 * rounds each once to fp32:
 *   mode 0 (CFG*):        coef = fp32(S_ab / (S_bb + 1e-8));                              g_out = a + (scale - 1)*(a - coef*b)
 *   mode 1 (APG):         sf = norm_threshold > 0 ? min(1, norm_threshold / sqrt(S_gg)) : 1;  proj = fp32(sf*S_ga / (S_aa + 1e-8)) with the fp64 sf;
 *                         sf = fp32(sf);  gs = g*sf;  par = proj*a;  apg = par*eta + (gs - par);   g_out = a + apg*(scale - 1)
 *   mode 2 (legacy APG):  as mode 1 with the multiplier `scale`, and g read from `running` when it is set (running is refused in modes 0 and 1).
 *   scale - 1 is formed in fp32.  proj comes from sf*S_ga; the reference reduces the fp32-rounded g*sf again, a relative difference of order 2^-24.
 *   d = mask ? g_out*mask[row] + clean*(1 - mask[row]) : g_out;  out = x + ((x - d) * (1/sigma)) * (sigma_next - sigma)
 * out may equal x.  scalars_out (may be NULL): block 0 stores the fp32 scalars it used, [0] = coef (mode 0), or [0] = sf, [1] = proj.
 * 16-byte accesses when C % 4 == 0 and every [rows][C] operand is 16-byte aligned, element-wise otherwise.  ts_stride, mask and clean as in
 * ltx2_guided_euler_step.  sigma == 0 -> LTX2_E_INVALID with message "Sigma can't be 0.0".  (additive entries of ABI version 3)           */
int ltx2_guidance_sums_blocks(int rows, int C);
int ltx2_guidance_sums(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, float* running, int first,
                       float momentum, double* partials, int rows, int C, void* stream);
int ltx2_projected_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                              const float* clean, const float* running, const double* partials, int mode, float scale, float eta,
                              float norm_threshold, float sigma, float sigma_next, float* out, float* scalars_out, int rows, int C, void* stream);
/* The same two passes over TWO latents in ONE launch each -- the video and the audio latent of a joint guided step, the audio one about a hundred
 * rows.  The single forms' operands twice, v_ then a_: each segment has its own operands, ts / ts_stride, running / first / momentum and partials
 * region partials[ltx2_guidance_sums_blocks(rows, C)][5], and in the step its own mode, scale, eta, norm_threshold, mask / clean, scalars_out and
 * rows / C; sigma and sigma_next are shared.  A segment's blocks number their partial rows from 0 and add their own rows in index order, the
 * scalars are derived in fp64 and rounded once, every fp32 operation is individually rounded: each segment's partials, running, scalars_out and
 * out equal the single entries' bit for bit at the same access width.  16-byte accesses only when BOTH segments qualify (the order of the
 * fp64 sums, and so their last bits, depends on the access width; the step's element-wise part does not).
 * ltx2_guidance_sums_pair: a segment with partials == NULL is left out (its guider reads no sums); both NULL -> LTX2_E_INVALID.
 * ltx2_projected_euler_step_pair: a segment's mode is 0, 1, 2 as in ltx2_projected_euler_step, or one of two guiders without sums, for which
 *   partials may be NULL, nothing is stored to scalars_out and running is refused:
 *   mode 3 (CFG):  g_out = a + (scale - 1)*(a - b), ltx2_guided_euler_step's arithmetic;   mode 4 (off): g_out = a (vel_uncond may be NULL).
 *   The single entry keeps refusing modes 3 and 4.  sigma == 0 -> LTX2_E_INVALID with message "Sigma can't be 0.0".
 * (additive entries of ABI version 3)                                                                                                   */
int ltx2_guidance_sums_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                            float* v_running, int v_first, float v_momentum, double* v_partials, int v_rows, int v_C, const float* a_x,
                            const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, float* a_running, int a_first,
                            float a_momentum, double* a_partials, int a_rows, int a_C, void* stream);
int ltx2_projected_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                                   const float* v_mask, const float* v_clean, const float* v_running, const double* v_partials, int v_mode,
                                   float v_scale, float v_eta, float v_norm_threshold, float* v_out, float* v_scalars_out, int v_rows, int v_C,
                                   const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride,
                                   const float* a_mask, const float* a_clean, const float* a_running, const double* a_partials, int a_mode,
                                   float a_scale, float a_eta, float a_norm_threshold, float* a_out, float* a_scalars_out, int a_rows, int a_C,
                                   float sigma, float sigma_next, void* stream);

/* MultiModalGuider.calculate (components/guiders.py:244-273) and the Euler step behind it, the stage-1 step of the two-stage pipeline
 * (pipelines/two_stage.py:366-390), over [rows][C] fp32.  Every fp32 operation is individually rounded, in the reference's order, so the
 * un-rescaled step equals the separate fp32 array ops bit for bit.  Per element, t = ts[row * ts_stride]:
 *   a = x - t*vel_cond;  u, p, m the same from vel_uncond (negative prompt), vel_perturbed (self-attentions skipped: ltx2_dit_forward_perturbed_av)
 *   and vel_isolated (cross-modal attentions skipped: ltx2_dit_forward_isolated_av)
 *   pred = a;  vel_uncond:    pred = pred + (cfg_scale - 1)*(a - u)
 *              vel_perturbed: pred = pred + stg_scale*(a - p)
 *              vel_isolated:  pred = pred + (modality_scale - 1)*(a - m)
 *   d = mask ? pred*mask[row] + clean*(1 - mask[row]) : pred;  out = x + ((x - d) * (1/sigma)) * (sigma_next - sigma)
 * A term is there exactly when its velocity is non-NULL, whatever its scale (the reference adds the term of every pass that ran).  The scale
 * differences are formed in fp32.  ltx2_mm_guided_euler_step_pair: two latents in ONE launch, v_ then a_, each with its own operands, scales and
 * shape; each segment's output equals the single entry's bit for bit; 16-byte accesses only when BOTH segments qualify.
 * With MultiModalGuiderParams.rescale_scale != 0 the step is two passes:
 * ltx2_mm_guidance_sums: S_a = sum a, S_aa = sum a*a, S_p = sum pred, S_pp = sum pred*pred in fp64 over ALL rows, in the order of
 *   ltx2_guidance_sums, into partials[ltx2_guidance_sums_blocks(rows, C)][4] (8-byte aligned); pred_out (may be NULL) receives pred.
 * ltx2_mm_rescaled_euler_step: every block adds the partial rows in index order and derives in fp64, n = rows*C,
 *   var = (S2 - S1*S1/n)/n (the population variance, as mx.var);  f = rescale_scale*sqrt((var_a + 1e-8)/(var_p + 1e-8)) + (1 - rescale_scale),
 *   rounded once to fp32; block 0 stores f to scalars_out (may be NULL); then the step above with pred*f in place of pred.
 * out may equal x (any input).  ts_stride, mask / clean, the access width and sigma == 0 as in ltx2_guided_euler_step.
 * (additive entries of ABI version 3)                                                                                                  */
int ltx2_mm_guided_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                              const float* ts, int64_t ts_stride, const float* mask, const float* clean, float cfg_scale, float stg_scale,
                              float modality_scale, float sigma, float sigma_next, float* out, int rows, int C, void* stream);
int ltx2_mm_guided_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed,
                                   const float* v_vel_isolated, const float* v_ts, int64_t v_ts_stride, const float* v_mask, const float* v_clean,
                                   float v_cfg_scale, float v_stg_scale, float v_modality_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                   const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed, const float* a_vel_isolated,
                                   const float* a_ts, int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale,
                                   float a_stg_scale, float a_modality_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next,
                                   void* stream);
int ltx2_mm_guidance_sums(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                          const float* ts, int64_t ts_stride, float cfg_scale, float stg_scale, float modality_scale, double* partials, float* pred_out,
                          int rows, int C, void* stream);
int ltx2_mm_rescaled_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                                const float* ts, int64_t ts_stride, const float* mask, const float* clean, const double* partials, float cfg_scale,
                                float stg_scale, float modality_scale, float rescale_scale, float sigma, float sigma_next, float* out,
                                float* scalars_out, int rows, int C, void* stream);

/* Classifier-free guidance with the per-channel rescale of the reference's standard one-stage loop (scripts/generate.py:1926-1931, rescale_noise_cfg
 * :688-727) over fp32 [rows][C] (rows = F*H*W tokens: the reference's [1, C, F, H, W] with statistics over axes 2, 3, 4).  Every fp32 operation is
 * rounded on its own, in the reference's statement order.  With a = x - t*vc, b = x - t*vu, g = b + cfg_scale*(a - b) (from the unconditional side:
 * another rounding than ltx2_guided_euler_step's a + (cfg_scale - 1)*(a - b)):
 * ltx2_channel_guidance_stats: per channel c, over all rows, mean and sqrt(mean((. - mean)^2) + 1e-8) of g[:, c] and of a[:, c], accumulated in
 *   fp64 and rounded once, into fp32 stats[4][C] = mean_g, std_g, mean_a, std_a.  Two launches and no atomics: per block of rows the sums of
 *   (v - v0) and (v - v0)^2, v0 the channel's value in row 0, into partials[ltx2_channel_guidance_stats_blocks(rows, C)][4][C] (fp64, 8-byte
 *   aligned; the last row holds the shifts), then one thread per channel adds the rows in index order: mean = v0 + S1/n,
 *   var = max((S2 - S1*S1/n)/n, 0).  The result is the same bits from run to run.  DESIGN.md derives the bound against the fp64 two-pass formula.
 * ltx2_rescaled_guided_euler_step: gr = ((g - mean_g)/std_g)*std_a + mean_a, g' = r*gr + (1 - r)*g with r = fp32(guidance_rescale) and
 *   (1 - r) = fp32(1 - guidance_rescale), out = x + ((x - g')*(1/sigma))*(sigma_next - sigma).  stats == NULL: g' = g (guidance without rescale, in
 *   this route's operation order).  out may equal x.  There is no mask / clean operand: the route has no conditioning.
 * ts_stride, the access width and sigma == 0 as in ltx2_guided_euler_step (stats and partials are read and written element-wise at any width).
 * (additive entries of ABI version 3)                                                                                                      */
int ltx2_channel_guidance_stats_blocks(int rows, int C);
int ltx2_channel_guidance_stats(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, float cfg_scale,
                                double* partials, float* stats, int rows, int C, void* stream);
int ltx2_rescaled_guided_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride,
                                    const float* stats, float cfg_scale, double guidance_rescale, float sigma, float sigma_next, float* out, int rows,
                                    int C, void* stream);

/* First-block cache: the three kernels over the fp32 residual stream, taken as n elements.
 * ltx2_fbc_head_metric: r = h1 - h0 (one fp32 subtraction per element), num = sum |r - head_prev| and den = sum |head_prev| in fp64, and
 *   record = {double num, double den, int32 skip, int32 0} (24 bytes of device memory, 8-byte aligned) with
 *   skip = (threshold > 0 && den > 0 && num < (double)threshold * den): no division, den == 0 and threshold == 0 never skip, +inf always does.
 *   Two launches and no atomics: ltx2_fbc_metric_blocks(n) blocks (one per 8192 elements, 1024 at the most) of 256 threads, thread t of block b adding
 *   the quads (4 consecutive elements) b*256 + t, + blocks*256, ... in index order, a fixed binary tree over the block into partials[block][2]
 *   (fp64, 8-byte aligned), then one block of 256 threads that adds the partials t, t + 256, ... and runs the same tree.  The same inputs give the
 *   same record on every run; 16-byte accesses where every operand is 16-byte aligned, element-wise ones otherwise, with the same sums.
 *   head_prev NULL reads as zeros.  h1_save (may be NULL) receives a copy of h1 and may be the buffer h0 itself; nothing else may alias.
 * ltx2_fbc_store_tail: tail = hL - h1.   ltx2_fbc_apply_tail: h = h + tail in place.  One rounded fp32 operation per element.
 * (additive entries of ABI version 3)                                                                                                      */
int ltx2_fbc_metric_blocks(int64_t n);
int ltx2_fbc_head_metric(const float* h0, const float* h1, const float* head_prev, float* r, float* h1_save, double* partials, void* record,
                         float threshold, int64_t n, void* stream);
int ltx2_fbc_store_tail(const float* hL, const float* h1, float* tail, int64_t n, void* stream);
int ltx2_fbc_apply_tail(float* h, const float* tail, int64_t n, void* stream);

/* VAE elementwise glue (simple_decoder.py:492-498, 228-238/339-342, ops.py:109-125, :792-798)  */
int ltx2_vae_prepare_latent(const float* latent, const float* std, const float* mean, const float* noise,
                            float noise_scale, void* out_bf16, int C, int64_t P, void* stream);
int ltx2_pixnorm_mod_silu(const void* x, void* y, int64_t P, int C, float eps, const float* table, const float* te,
                          int shift_row, int scale_row, void* stream);
int ltx2_vae_unpatchify(const void* x, float* video, int T, int H, int W, void* stream);
int ltx2_video_to_uint8(const float* video, uint8_t* frames, int T, int H, int W, void* stream);
/* decode_latent's chunk cross-fade, trim and uint8 conversion in one pass (simple_decoder.py:760-798): frame j of the chunk
 * `cur` [3][Tc][H][W] lands on output frame t_dst0 + j of `frames` [T_out][H][W][3]; with `prev` (the previous chunk,
 * [3][prev_T][H][W]) the first `ov` frames are prev_tail * (1 - ramp[j]) + cur * ramp[j] (ramp = torch.linspace(0, 1, ov) on the
 * device), rounded like the separate reference ops.                                                                  */
int ltx2_video_chunk_to_uint8(const float* cur, const float* prev, const float* ramp, uint8_t* frames, int Tc, int prev_T, int ov, int H,
                              int W, int t_dst0, int T_out, void* stream);
/* decode_tiled's trapezoid blend (video_vae/tiling.py:380-412): out[3][OT][OH][OW] += tile[3][dt][dh][dw](cropped to nt,nh,nw) *
 * mt[t] mh[h] mw[w] and wsum += mask at offset (t0,h0,w0); ltx2_tile_blend_finish divides by clamp(wsum, 1e-8).       */
int ltx2_tile_blend_accumulate(const float* tile, int dt, int dh, int dw, int nt, int nh, int nw, const float* mt, const float* mh,
                               const float* mw, float* out, float* wsum, int OT, int OH, int OW, int t0, int h0, int w0, void* stream);
int ltx2_tile_blend_finish(float* out, const float* wsum, int64_t plane, void* stream);

/* ------------------------------------------------------------------------------------------
 * DiT engine: LTXModel forward behind one call, VideoOnly or AudioVideo, 19B-style blocks or the
 * 22B "V2.3" variant (cross_attention_adaln + apply_gated_attention).
 * Replaces X0Model(LTXModel(...)).__call__ (model/transformer/model.py:776-881,895-936),
 * BasicTransformerBlock.__call__ (transformer.py:191-238) and BasicAVTransformerBlock.__call__
 * (transformer.py:457-648) x num_layers.
 * ------------------------------------------------------------------------------------------ */
#define LTX2_MODEL_VIDEO_ONLY 0
#define LTX2_MODEL_AUDIO_VIDEO 1

typedef struct ltx2_dit ltx2_dit;

typedef struct ltx2_dit_config {
    int num_layers;        /* 48 */
    int num_heads;         /* 32 */
    int head_dim;          /* 128 */
    int in_channels;       /* 128 */
    int out_channels;      /* 128 */
    int caption_channels;  /* 3840; 0 = no caption_projection (context already inner_dim wide) */
    float norm_eps;        /* 1e-6 */
    float timestep_scale;  /* 1000 */
    /* --- fields below default to 0 for the 19B VideoOnly model --- */
    int model_type;             /* LTX2_MODEL_VIDEO_ONLY / LTX2_MODEL_AUDIO_VIDEO (model.py:436) */
    int audio_heads;            /* 32  (LTXModel.AUDIO_ATTENTION_HEADS, model.py:429); must equal num_heads */
    int audio_head_dim;         /* 64  (AUDIO_HEAD_DIM, model.py:430) */
    int audio_in_channels;      /* 128 */
    int audio_out_channels;     /* 128 */
    int cross_attention_adaln;  /* V2.3: 9 AdaLN rows, prompt_adaln_single, prompt_scale_shift_table (transformer.py:427-455) */
    int apply_gated_attention;  /* V2.3: to_gate_logits, out *= 2*sigmoid(.) per head (attention.py:241-249) */
    float av_ca_timestep_scale; /* 1 (av_ca_timestep_scale_multiplier, model.py:452) */
} ltx2_dit_config;

int ltx2_dit_create(const ltx2_dit_config* cfg, ltx2_dit** out);
void ltx2_dit_destroy(ltx2_dit* ctx);

/* Register a weight (caller keeps it alive).  Names are the checkpoint keys after stripping
 * "model.diffusion_model." (loader/weight_converter.py:277-315), with these load-time fusions:
 *   transformer_blocks.{i}.attn1.to_qkv.{weight,bias}  = cat(to_q, to_k, to_v)   [3D, D]
 *   transformer_blocks.{i}.attn2.to_kv.{weight,bias}   = cat(to_k, to_v)         [2D, D]
 * Linear weights: bf16 [out, in]; biases, norm weights, scale_shift_tables: fp32.           */
int ltx2_dit_set_weight(ltx2_dit* ctx, const char* name, const void* ptr, int dtype, int64_t numel);

/* Workspace (activations + per-prompt caches).  per_token != 0 sizes the per-token AdaLN path.
 * AudioVideo models use the *_av forms (Na audio tokens, Sa audio-text tokens).               */
int64_t ltx2_dit_workspace_bytes(const ltx2_dit* ctx, int N, int S, int per_token);
int ltx2_dit_bind_workspace(ltx2_dit* ctx, void* ptr, int64_t bytes, int N, int S, int per_token);
int64_t ltx2_dit_workspace_bytes_av(const ltx2_dit* ctx, int N, int S, int Na, int Sa, int per_token);
int ltx2_dit_bind_workspace_av(ltx2_dit* ctx, void* ptr, int64_t bytes, int N, int S, int Na, int Sa, int per_token);

/* Per-prompt, step-invariant work hoisted out of the loop (the reference recomputes it every
 * step: model.py:262-271): caption projection (model.py:142-161), per-layer cross-attention
 * K (k_norm applied) and V^T of the projected context (attention.py:227-232), and the RoPE
 * tables cos/sin fp32 [N][D/2] computed by the caller from positions (rope.py:365-418).     */
int ltx2_dit_prepare(ltx2_dit* ctx, const float* context, int S, const float* rope_cos, const float* rope_sin,
                     void* stream);
/* AudioVideo: per modality the text context, the self-attention RoPE tables [N][D/2] and the
 * cross-modal tables [N][Da/2] (temporal axis only, audio inner dim; model.py:320-344).  With
 * cross_attention_adaln the text K/V depend on sigma and are recomputed per step instead.    */
int ltx2_dit_prepare_av(ltx2_dit* ctx, const float* v_context, int S, const float* v_cos, const float* v_sin,
                        const float* v_cross_cos, const float* v_cross_sin, const float* a_context, int Sa,
                        const float* a_cos, const float* a_sin, const float* a_cross_cos, const float* a_cross_sin,
                        void* stream);

/* velocity[N][out_channels] (fp32) = LTXModel(latent[N][in_channels] fp32, timesteps).
 * n_timesteps = 1: one sigma for all tokens (Modality.timesteps shape (B,), scripts/generate.py:1946);
 * n_timesteps = N: per-token sigma (pipelines/common.py:193-232).                           */
int ltx2_dit_forward(ltx2_dit* ctx, const float* latent, const float* timesteps, int n_timesteps, const float* sigma,
                     float* velocity, void* stream);
/* AudioVideo forward (model.py:776-881).  *_sigma: one device float per modality = Modality.sigma
 * (drives the prompt AdaLN of its own modality and the cross-modal AdaLN of the OTHER one,
 * model.py:151-161,392-404).  The VideoOnly entries take it as `sigma` / `sigma_dev` (one device float; NULL =
 * timesteps[0], which is only right when no token carries a conditioning mask: with image conditioning
 * timesteps = mask * sigma, model.py:151-158).                                                 */
int ltx2_dit_forward_av(ltx2_dit* ctx, const float* v_latent, const float* v_timesteps, int n_v_timesteps,
                        const float* v_sigma, const float* a_latent, const float* a_timesteps, int n_a_timesteps,
                        const float* a_sigma, float* v_velocity, float* a_velocity, void* stream);

/* Spatio-temporal guidance (STG): the layers whose SELF-attention a perturbed forward skips, per modality (0 = video, 1 = audio: the reference's
 * SKIP_VIDEO_SELF_ATTN / SKIP_AUDIO_SELF_ATTN, model/transformer/transformer.py:485-515, 538-543).  flags: a HOST array of n_layers bytes,
 * non-zero = skip; n_layers must equal the model's; NULL clears the set.  A skipped self-attention is launches that do not happen (the residual
 * stream is unchanged); the text cross-attention, the cross-modal attention and the feed-forward of that layer run as always.  On a VideoOnly
 * context (and the video twin of an AudioVideo model) this is the AudioVideo block's video branch with audio absent.  The A2V / V2A cross-modal
 * perturbations are not built.  The set is read by the perturbed entries alone: every other entry ignores it.
 * ltx2_dit_forward_perturbed[_av]: the arguments and the program of ltx2_dit_forward[_av] with the stored set applied (an empty set: the same
 * result bit for bit).  With "fold_norms" = 1 a layer whose self-attention is skipped runs its text cross-attention's pre-norm as a pass of
 * its own (the skipped out-projection was the fold's producer); the AudioVideo stream / event schedule is that of the plain forward.
 * (additive entries of ABI version 3)                                                                                                  */
int ltx2_dit_set_stg_blocks(ltx2_dit* ctx, int modality, const unsigned char* flags, int n_layers);
/* The reference's set_cross_attn_scale (scripts/generate.py:1174-1176): in every forward of ctx from now on, the output of the text cross-attention of
 * the layers l >= start_layer enters the residual stream multiplied by `scale` -- a row-invariant gate table of the out-projection's gated-residual
 * epilogue, no further kernel.  scale == 1 removes it.  Per context: set it on the negative prompt's context as well.  LTX2_E_UNSUPPORTED on a gated
 * text cross-attention (cross_attention_adaln: LTX-2.3) and on AudioVideo contexts, whose gate is per row.  It synchronises the device (a copy of
 * the table) and is not for use while a stream is capturing.  (additive entry of ABI version 3)                                            */
int ltx2_dit_set_cross_attn_scale(ltx2_dit* ctx, float scale, int start_layer);
int ltx2_dit_forward_perturbed(ltx2_dit* ctx, const float* latent, const float* timesteps, int n_timesteps, const float* sigma,
                               float* velocity, void* stream);
int ltx2_dit_forward_perturbed_av(ltx2_dit* ctx, const float* v_latent, const float* v_timesteps, int n_v_timesteps,
                                  const float* v_sigma, const float* a_latent, const float* a_timesteps, int n_a_timesteps,
                                  const float* a_sigma, float* v_velocity, float* a_velocity, void* stream);
/* The modality-isolated forward (the reference's SKIP_A2V_CROSS_ATTN and SKIP_V2A_CROSS_ATTN over every block together, pipelines/two_stage.py:356-364):
 * the arguments and the program of ltx2_dit_forward_av with the cross-modal attention of EVERY layer left out -- launches that do not happen, both
 * residual streams unchanged there -- so each modality's velocity depends on its own latent alone.  Both stream joins per layer, the early text
 * K / V and the output heads are those of the plain forward.  A per-layer set or a single direction is not built.  LTX2_E_INVALID on a VideoOnly
 * context.  (additive entry of ABI version 3)                                                                                           */
int ltx2_dit_forward_isolated_av(ltx2_dit* ctx, const float* v_latent, const float* v_timesteps, int n_v_timesteps,
                                 const float* v_sigma, const float* a_latent, const float* a_timesteps, int n_a_timesteps,
                                 const float* a_sigma, float* v_velocity, float* a_velocity, void* stream);

/* One sampling step: forward -> x0 = latent - ts*v -> post_process -> Euler, latent updated in
 * place (pipelines/distilled.py:214-253; scripts/generate.py:1942-1979).  x0_out may be NULL.  */
int ltx2_dit_denoise_step(ltx2_dit* ctx, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                          const float* mask, const float* clean, float sigma, float sigma_next, float* x0_out, void* stream);
/* Joint audio+video step (pipelines/distilled.py:198-271): both latents updated in place;
 * sigma_dev = device copy of sigma.                                                          */
int ltx2_dit_denoise_step_av(ltx2_dit* ctx, float* v_latent, float* a_latent, const float* v_timesteps,
                             int n_v_timesteps, const float* a_timesteps, int n_a_timesteps, const float* sigma_dev,
                             const float* v_mask, const float* v_clean, const float* a_mask, const float* a_clean,
                             float sigma, float sigma_next, float* v_x0_out, float* a_x0_out, void* stream);

/* hipGraph: capture n_steps of ltx2_dit_denoise_step over host_sigmas[n_steps+1] with a uniform
 * sigma per step (timesteps = sigma for every token), then replay.  latent is updated in place. */
int ltx2_dit_graph_capture(ltx2_dit* ctx, float* latent, const float* host_sigmas, int n_steps, void* stream);
/* The same for CONDITIONED loops (image-to-video; reference pipelines/common.py:193-232, pipelines/distilled.py:214-253): mask fp32 [N] = the
 * denoise mask (1 = free token), clean fp32 [N][C] = the clean latent of the conditioned tokens.  Step i runs with per-token timesteps
 * mask * sigma_i (formed on the device inside the captured step) and blends x0 with `clean` before the Euler update, exactly as
 * ltx2_dit_denoise_step with n_timesteps = N, mask and clean.  The workspace must be bound with per_token = 1.  A null mask (per modality in
 * the _av form) = no conditioning tokens there.  n_mask / n_clean: ELEMENT counts of the two buffers, checked against the bound token count
 * and N * out_channels (the replay reads exactly that much on every step).  (round 4; the counts: round 5, ABI 3)                       */
int ltx2_dit_graph_capture_cond(ltx2_dit* ctx, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask, const float* clean,
                                int64_t n_clean, void* stream);
int ltx2_dit_graph_capture_cond_av(ltx2_dit* ctx, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps, const float* v_mask, int64_t n_v_mask,
                                   const float* v_clean, int64_t n_v_clean, const float* a_mask, int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, void* stream);

/* One classifier-free-guided step on the VideoOnly engine (keyframe interpolation's stage 1; pipelines/one_stage.py:224-330): forward(ctx)
 * and forward(neg) from the same latent and the same timestep pointer, each into its own context's velocity buffer, then
 * ltx2_guided_euler_step in place on `latent` -- enqueued one after the other on the caller's stream (no fork: each evaluation fills the
 * device).  `neg` is a second context over the same weights, prepared with the negative prompt.  LTX2_E_INVALID when either context is
 * AudioVideo or not prepared, ctx == neg, the two differ in N or out_channels, or n_timesteps > 1 and either workspace was not bound with
 * per_token = 1.  sigma_dev as in ltx2_dit_denoise_step.  (additive entries of ABI version 3)                                          */
int ltx2_dit_guided_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                         const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, void* stream);
/* ltx2_dit_graph_capture_cond with that step as its body: a linear chain of n_steps guided steps.  mask may be NULL (the uniform form, clean
 * then NULL too); otherwise the per-token timesteps mask * sigma_i are formed into ctx's buffer and both contexts read them.  The graph
 * belongs to ctx: ltx2_dit_graph_launch(ctx) replays it.                                                                               */
int ltx2_dit_graph_capture_guided(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps,
                                  const float* mask, int64_t n_mask, const float* clean, int64_t n_clean, float cfg_scale, void* stream);
/* ltx2_dit_guided_step in the standard one-stage loop's form (scripts/generate.py:1895-1976): forward(ctx), forward(neg), with guidance_rescale > 0
 * ltx2_channel_guidance_stats into ctx's own workspace (allocated before anything is enqueued, for the bound shape, and freed with ctx), then
 * ltx2_rescaled_guided_euler_step in place on `latent`.  No mask / clean: that loop has no conditioning.  Validity as ltx2_dit_guided_step.
 * ltx2_dit_graph_capture_rescaled_guided: n_steps of it as one captured linear chain owned by ctx, with uniform timesteps sigma_i.
 * (additive entries of ABI version 3)                                                                                                      */
int ltx2_dit_rescaled_guided_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                                  float cfg_scale, double guidance_rescale, float sigma, float sigma_next, void* stream);
int ltx2_dit_graph_capture_rescaled_guided(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, float cfg_scale,
                                           double guidance_rescale, void* stream);
/* First-block cache on the VideoOnly engine (opt-in).  A slot belongs to one kind of evaluation within a step (the positive
 * or the negative pass) and holds head_prev and tail, [N][D] fp32 each, and a valid flag; the context holds two more buffers (the scratch r, the
 * saved h1), so (2*n_slots + 2) * N*D*4 bytes in all, allocated by the first cached pass for the bound shape.  A cached pass in slot s: h0 enters
 * block 0, which gives h1; ltx2_fbc_head_metric forms r = h1 - h0 and, with a valid slot, the decision against head_prev; the record is read back
 * by one 24-byte copy on the pass's stream and a wait for it.  Skip: h = h1 + tail, the slot unchanged.  Otherwise blocks 1..L-1 run, then
 * tail = hL - h1, head_prev = r (a pointer swap) and valid = 1.  Then the output head.  A pass whose slot is not valid, or was named by
 * ltx2_dit_fbc_force_next since its last pass, computes in full and reads nothing back.  A cached pass cannot be captured (LTX2_E_STATE).
 * ltx2_dit_fbc_configure: n_slots 0..8 (0: off, the buffers freed) and threshold >= 0; every slot starts invalid with zero counts.  The cache's
 *   state is kept beside the context, not in it: a caller that turned it on calls ltx2_dit_fbc_configure(ctx, 0, 0) before ltx2_dit_destroy(ctx).
 * ltx2_dit_fbc_reset: every slot invalid, counts zero, forcing cleared -- a loop calls it at its start.
 * ltx2_dit_fbc_force_next: the next pass in `slot` (-1: in every slot) computes in full -- a loop calls it before its last step.
 * ltx2_dit_fbc_stats: the slot's passes and skips since the reset, and the sums of its last pass that read a record (any output may be NULL).
 * ltx2_dit_forward_fbc: ltx2_dit_forward through ctx's slot.  pass_kind other than LTX2_FBC_PASS_PLAIN, and an AudioVideo context, return
 *   LTX2_E_UNSUPPORTED: the perturbed (STG) and the modality-isolated pass have no cached form.
 * ltx2_dit_denoise_step_fbc: ltx2_dit_denoise_step without mask / clean / x0_out through ctx's slot.
 * ltx2_dit_rescaled_guided_step_fbc: ltx2_dit_rescaled_guided_step with forward(ctx) in ctx's slot_pos and forward(neg) in ctx's slot_neg (the
 *   slots of `neg` itself are not touched).  With the cache off none of this runs and every other entry is what it was.
 * (additive entries of ABI version 3)                                                                                                      */
#define LTX2_FBC_PASS_PLAIN 0
#define LTX2_FBC_PASS_PERTURBED 1
#define LTX2_FBC_PASS_ISOLATED 2
int ltx2_dit_fbc_configure(ltx2_dit* ctx, int n_slots, float threshold);
int ltx2_dit_fbc_reset(ltx2_dit* ctx);
int ltx2_dit_fbc_force_next(ltx2_dit* ctx, int slot);
int ltx2_dit_fbc_stats(const ltx2_dit* ctx, int slot, int64_t* evaluations, int64_t* skips, double* last_num, double* last_den);
int ltx2_dit_forward_fbc(ltx2_dit* ctx, int slot, int pass_kind, const float* latent, const float* timesteps, int n_timesteps, const float* sigma,
                         float* velocity, void* stream);
int ltx2_dit_denoise_step_fbc(ltx2_dit* ctx, int slot, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, float sigma,
                              float sigma_next, void* stream);
int ltx2_dit_rescaled_guided_step_fbc(ltx2_dit* ctx, ltx2_dit* neg, int slot_pos, int slot_neg, float* latent, const float* timesteps,
                                      int n_timesteps, const float* sigma_dev, float cfg_scale, double guidance_rescale, float sigma,
                                      float sigma_next, void* stream);
/* One STG step on the VideoOnly engine (pipelines/one_stage.py:267-326 with a CFGGuider and an STGGuider): forward(ctx), forward(neg) when neg is
 * given (NULL: no CFG), a perturbed forward on ctx ITSELF (ltx2_dit_forward_perturbed: the set of ltx2_dit_set_stg_blocks) into vel_perturbed, the
 * caller's [N][out_channels] fp32 scratch, then ltx2_stg_euler_step in place on `latent` -- in order on the caller's stream.  There is no third
 * context: the perturbed pass reads ctx's per-prompt text K / V.  Validity as ltx2_dit_guided_step (with neg NULL the same rules on ctx alone).
 * ltx2_dit_graph_capture_stg: n_steps as one captured linear chain owned by ctx, built like ltx2_dit_graph_capture_guided.  Step i is an STG step
 * iff (i + 1) / n_steps <= stg_cutoff (decided on the host at capture, in double); later steps are the guided step, or the plain step when neg
 * is NULL.  n_vel: the ELEMENT count of vel_perturbed, checked against N * out_channels.  (additive entries of ABI version 3)             */
int ltx2_dit_stg_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* mask,
                      const float* clean, float* vel_perturbed, float cfg_scale, float stg_scale, float sigma, float sigma_next, void* stream);
int ltx2_dit_graph_capture_stg(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                               const float* clean, int64_t n_clean, float* vel_perturbed, int64_t n_vel, float cfg_scale, float stg_scale,
                               double stg_cutoff, void* stream);
/* The guided step on the AudioVideo engine with the audio latent FROZEN (audio-to-video; pipelines/a2vid_two_stage.py:225-271): what
 * ltx2_dit_forward_av does on ctx and then on neg, both from the same latents and timestep pointers (sigma_dev is both modalities' sigma), each into
 * its own context's velocity buffers, then ltx2_guided_euler_step in place on the VIDEO latent -- in order on the caller's stream, the audio stream's
 * kernels on each context's side stream as in every AudioVideo forward.  a_latent is only read; the audio velocities are not read.
 * LTX2_E_INVALID, before anything is launched, when either context is VideoOnly or not prepared, ctx == neg, the two differ in N, Na or
 * out_channels, a timestep count is neither 1 nor its modality's token count, or one is > 1 and either workspace was not bound with per_token = 1.
 * (additive entries of ABI version 3)                                                                                                     */
int ltx2_dit_guided_step_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, const float* a_latent, const float* v_timesteps, int n_v_timesteps,
                            const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                            float cfg_scale, float sigma, float sigma_next, void* stream);
/* n_steps of that step as one captured graph owned by ctx (ltx2_dit_graph_launch(ctx) replays it), built like ltx2_dit_graph_capture_cond_av: a
 * modality with a mask gets per-token timesteps mask * sigma_i formed on the device into ctx's buffer, which both contexts read.  The frozen audio
 * passes its all-zero mask (no clean latent: it is never blended or stepped); v_mask may be NULL (v_clean then NULL too).                      */
int ltx2_dit_graph_capture_guided_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, const float* a_latent, const float* host_sigmas, int n_steps,
                                     const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                     int64_t n_a_mask, float cfg_scale, void* stream);
/* The guided step on the AudioVideo engine with BOTH latents stepped (a retake with sound; the reference's pipelines/retake.py:234-291 run with an
 * audio state): forward_av on ctx, then on neg, exactly as ltx2_dit_guided_step_av builds them, then ONE ltx2_guided_euler_step_pair in place on both
 * latents, the video under cfg_scale and the audio under audio_cfg_scale.  Each modality may carry a denoise mask with its clean latent (both or
 * neither).  LTX2_E_INVALID, before anything is launched: the rules of ltx2_dit_guided_step_av, a mask without its clean latent (or the reverse),
 * sigma == 0.
 * ltx2_dit_graph_capture_guided_joint_av: n_steps (< 64) of that step as one captured graph owned by ctx (ltx2_dit_graph_launch(ctx) replays it),
 * built like ltx2_dit_graph_capture_guided_av: a modality with a mask gets per-token timesteps mask * sigma_i formed on the device into ctx's buffer,
 * which both contexts read, and its x0 blended with its clean latent; n_*: ELEMENT counts, checked against the bound shapes.
 * (additive entries of ABI version 3)                                                                                                       */
int ltx2_dit_guided_step_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                                  const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                                  const float* a_mask, const float* a_clean, float cfg_scale, float audio_cfg_scale, float sigma, float sigma_next,
                                  void* stream);
int ltx2_dit_graph_capture_guided_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                                           const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                           int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, float cfg_scale, float audio_cfg_scale,
                                           void* stream);
/* The Euler-ancestral step on the engine: ltx2_dit_guided_step (VideoOnly contexts) and ltx2_dit_guided_step_joint_av (AudioVideo contexts, both
 * latents stepped) with ltx2_ancestral_euler_step / _pair in place of the guided Euler kernel.  neg NULL: no guidance, one evaluation.  The same
 * forwards and the same validity rules; besides, LTX2_E_INVALID for a negative sigma_up / sigma_down and a NULL or misaligned seed_dev.
 * ltx2_dit_graph_capture_ancestral / _joint_av: n_steps (< 64) as one captured linear chain owned by ctx; step i bakes in step = i and
 * host_sigma_up[i] / host_sigma_down[i] (n_steps values each), seed_dev stays a pointer: writing another seed and replaying gives that seed's
 * result.  (additive entries of ABI version 3)                                                                                            */
int ltx2_dit_ancestral_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                            const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_up, float sigma_down,
                            const uint64_t* seed_dev, uint32_t step, void* stream);
int ltx2_dit_ancestral_step_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                                     const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                                     const float* a_mask, const float* a_clean, float cfg_scale, float audio_cfg_scale, float sigma, float sigma_up,
                                     float sigma_down, const uint64_t* seed_dev, uint32_t step, void* stream);
int ltx2_dit_graph_capture_ancestral(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                                     const float* clean, int64_t n_clean, float cfg_scale, const float* host_sigma_up, const float* host_sigma_down,
                                     const uint64_t* seed_dev, void* stream);
int ltx2_dit_graph_capture_ancestral_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                                              const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                              int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, float cfg_scale, float audio_cfg_scale,
                                              const float* host_sigma_up, const float* host_sigma_down,
                                              const uint64_t* seed_dev, void* stream);
/* The STG step on the AudioVideo engine with BOTH latents stepped and an STG term per modality (OneStagePipeline's joint branch with stg_scale and / or
 * stg_audio_scale): forward_av on ctx and, when neg is given (NULL: neither modality has CFG), on neg, exactly as ltx2_dit_guided_step_joint_av builds
 * them; then ltx2_dit_forward_perturbed_av on ctx ITSELF (the sets of ltx2_dit_set_stg_blocks, per modality; no third context) into the caller's
 * scratch pair, v_vel_perturbed [N][out_channels] and a_vel_perturbed [Na][audio_out_channels] fp32, both required; then ONE
 * ltx2_stg_euler_step_pair in place on both latents, the video under cfg_scale / stg_scale and the audio under audio_cfg_scale / audio_stg_scale.
 * A modality whose STG scale is 0 hands the kernel no perturbed velocity: it takes the guided step's arithmetic.  n_v_vel / n_a_vel: the ELEMENT
 * counts of the scratch buffers.  LTX2_E_INVALID, before anything is launched: the rules of ltx2_dit_guided_step_joint_av (with neg NULL the same
 * rules on ctx alone), a missing scratch or one whose element count is not N * out_channels / Na * audio_out_channels, a non-zero STG scale on a
 * modality whose set is empty, both STG scales 0 (that is ltx2_dit_guided_step_joint_av).  There is no captured form: the loop is one C call per
 * step.  (additive entry of ABI version 3)                                                                                                  */
int ltx2_dit_stg_step_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                               const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                               const float* a_mask, const float* a_clean, float* v_vel_perturbed, int64_t n_v_vel, float* a_vel_perturbed, int64_t n_a_vel,
                               float cfg_scale, float audio_cfg_scale, float stg_scale, float audio_stg_scale, float sigma, float sigma_next, void* stream);
/* ltx2_dit_guided_step with a guider whose scalars are sums over the whole latent: forward(ctx), forward(neg), ltx2_guidance_sums and
 * ltx2_projected_euler_step in place on `latent`, in order on the caller's stream.  mode / scale / eta / norm_threshold as in
 * ltx2_projected_euler_step; momentum != 0 (mode 2 only) keeps the running guidance in a [N][out_channels] fp32 buffer owned by ctx: first != 0
 * starts it (the first step of a loop), first == 0 continues it and is LTX2_E_STATE when no first step has run for the bound N.  That buffer
 * and the partials are allocated on first use for the bound N and freed with ctx.  The sums run over all N rows, appended conditioning tokens
 * included.  Otherwise the validity rules of ltx2_dit_guided_step.  (additive entries of ABI version 3)                                  */
int ltx2_dit_projected_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                            const float* mask, const float* clean, int mode, float scale, float eta, float norm_threshold, float momentum, int first,
                            float sigma, float sigma_next, void* stream);
/* n_steps of that step as one captured linear chain, built like ltx2_dit_graph_capture_guided; first is 1 in step 0 only, and with momentum a
 * memset node at the head of the chain clears the running guidance, so every replay starts alike.  The graph belongs to ctx.              */
int ltx2_dit_graph_capture_projected(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask,
                                     int64_t n_mask, const float* clean, int64_t n_clean, int mode, float scale, float eta, float norm_threshold,
                                     float momentum, void* stream);
/* The projected step on the AudioVideo engine with BOTH latents stepped, each modality under its own guider (OneStagePipeline's joint branch:
 * a CFGStarRescalingGuider per modality by default, pipelines/one_stage.py:466-568).  In order on the caller's stream: forward_av on ctx, then on
 * neg, scheduled exactly as ltx2_dit_guided_step_joint_av schedules them; ONE ltx2_guidance_sums_pair over the modalities whose guider reads
 * sums (none does: no launch); ONE ltx2_projected_euler_step_pair in place on both latents.  v_mode / a_mode and their scale / eta /
 * norm_threshold as in ltx2_projected_euler_step_pair (3: plain CFG, 4: the modality is not guided).  momentum != 0 (mode 2 only) keeps that
 * modality's running guidance in the CALLER's buffer, [N][out_channels] resp. [Na][audio_out_channels] fp32 (n_*_running: its ELEMENT count,
 * checked against the bound shape); without momentum the buffer is NULL.  first != 0 starts the running guidance (the first step of a loop).
 * The partials are allocated on first use for the bound shapes, before anything is enqueued, and freed with ctx.  The sums run over all rows
 * of a modality, appended conditioning tokens included.  LTX2_E_INVALID, before anything is launched: the rules of
 * ltx2_dit_guided_step_joint_av, a mode outside 0..4, momentum outside mode 2, a running buffer that is missing, unasked for or of another length.
 * ltx2_dit_graph_capture_projected_joint_av: n_steps (< 64) of that step as one captured graph owned by ctx (ltx2_dit_graph_launch(ctx) replays
 * it), built like ltx2_dit_graph_capture_guided_joint_av; first is 1 in step 0 only, and a memset node at the head of the chain clears each
 * running buffer, so every replay starts alike.  (additive entries of ABI version 3)                                                       */
int ltx2_dit_projected_step_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                                     const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                                     const float* a_mask, const float* a_clean, int v_mode, float v_scale, float v_eta, float v_norm_threshold,
                                     float v_momentum, float* v_running, int64_t n_v_running, int a_mode, float a_scale, float a_eta,
                                     float a_norm_threshold, float a_momentum, float* a_running, int64_t n_a_running, int first, float sigma,
                                     float sigma_next, void* stream);
int ltx2_dit_graph_capture_projected_joint_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                                              const float* v_mask, int64_t n_v_mask, const float* v_clean, int64_t n_v_clean, const float* a_mask,
                                              int64_t n_a_mask, const float* a_clean, int64_t n_a_clean, int v_mode, float v_scale, float v_eta,
                                              float v_norm_threshold, float v_momentum, float* v_running, int64_t n_v_running, int a_mode,
                                              float a_scale, float a_eta, float a_norm_threshold, float a_momentum, float* a_running,
                                              int64_t n_a_running, void* stream);
/* One res_2s step on the VideoOnly engine (pipelines/ti2vid_hq.py:185-273), enqueued in order on the caller's stream: forward(ctx) and
 * forward(neg) from `latent` at `timesteps`, ltx2_res2s_midpoint into workspaces owned by ctx, forward(ctx) and forward(neg) from x_mid at
 * `ts_sub` (the timesteps of the sub-sigma sqrt(sigma * sigma_next)), ltx2_res2s_combine into `latent`.  neg may be NULL: no guidance, two
 * evaluations.  h = -log(sigma_next / sigma) and (a21, b1, b2) are computed on the host in double exactly as components/res2s.py does;
 * n_bong = 100 when h < 0.5 and sigma > 0.03.  When h == 0 or sigma_next <= 0.001 the step is the reference's final one: one pair of
 * evaluations and latent = d (ts_sub is not read).  n_timesteps (1 or N) counts both `timesteps` and `ts_sub`; sigma_dev / sub_sigma_dev as
 * sigma_dev in ltx2_dit_denoise_step (NULL: the first timestep).  The three [N][out_channels] fp32 workspaces are allocated on first use
 * for the bound N and freed with ctx.  LTX2_E_INVALID as ltx2_dit_guided_step, and when sigma <= 0 or sigma_next < 0.
 * (additive entries of ABI version 3)                                                                                                  */
int ltx2_dit_res2s_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                        const float* ts_sub, const float* sub_sigma_dev, const float* mask, const float* clean, float cfg_scale, float sigma,
                        float sigma_next, void* stream);
/* n_steps res_2s steps as one captured linear chain (it ends after a final step).  The sub-sigmas are uploaded beside the sigmas; with a mask
 * the per-token timesteps mask * sigma_i are formed into ctx's buffer before the first pair of evaluations and mask * sub_sigma_i into the
 * same buffer after the midpoint kernel.  The graph belongs to ctx: ltx2_dit_graph_launch(ctx) replays it.                              */
int ltx2_dit_graph_capture_res2s(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask,
                                 int64_t n_mask, const float* clean, int64_t n_clean, float cfg_scale, void* stream);
/* One JOINT res_2s step on the AudioVideo engine (pipelines/ti2vid_hq.py:153-319): both latents are stepped.  In order on the caller's stream:
 * forward(ctx) and forward(neg) on both modalities (built as in ltx2_dit_guided_step_av), ltx2_res2s_midpoint_pair into workspaces owned by
 * ctx, both contexts again from the two midpoint latents at the sub-sigma timesteps, ltx2_res2s_combine_pair into both latents in place.
 * The video is guided by cfg_scale and the audio by audio_cfg_scale, both as uncond + s*(cond - uncond).  neg may be NULL: no guidance, two
 * evaluations.  The plan (h, a21, b1, b2, n_bong, the final step) is that of ltx2_dit_res2s_step; on the final step both latents take d.
 * n_v_timesteps (1 or N) counts v_timesteps and v_ts_sub, n_a_timesteps (1 or Na) a_timesteps and a_ts_sub; sigma_dev / sub_sigma_dev: one
 * float each, shared by the modalities (sub_sigma_dev NULL: the first of v_ts_sub).  Workspace: 3 x (N*C + Na*Ca) fp32, allocated on first
 * use for the bound shapes.  The step is enqueued eagerly only: there is no captured form of the joint loop.
 * LTX2_E_INVALID, before anything is launched: the rules of ltx2_dit_guided_step_av (with neg NULL the same rules on ctx alone), a mask
 * without its clean latent, sigma <= 0, sigma_next < 0.
 * (additive entry of ABI version 3)                                                                                                    */
int ltx2_dit_res2s_step_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                           const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_ts_sub, const float* a_ts_sub,
                           const float* sub_sigma_dev, const float* v_mask, const float* v_clean, const float* a_mask, const float* a_clean,
                           float cfg_scale, float audio_cfg_scale, float sigma, float sigma_next, void* stream);
/* One Heun step on the VideoOnly engine (pipelines/one_stage.py:366-459 under a CFGGuider, or none), enqueued in order on the caller's stream:
 * forward(ctx) and forward(neg) from `latent` at `timesteps`, ltx2_heun_predict into workspaces owned by ctx, forward(ctx) and forward(neg) from
 * the predictor xp at `ts_next` (the timesteps of sigma_next), ltx2_heun_correct into `latent`.  neg may be NULL: no guidance, two evaluations.
 * sigma_next == 0: the reference's last step, one pair of evaluations and latent = d (ts_next is not read).  ge_gamma > 0: the GE velocity
 * correction on the first evaluation, its state kept in ctx's workspace; first != 0 starts it (the first step of a loop), first == 0 continues it
 * and is LTX2_E_STATE unless one of these step entries has run on ctx with ge_gamma > 0 and first != 0 since the workspace was allocated for the
 * bound shapes (a step without GE, or a capture, allocates it and fills no velocity).  n_timesteps (1 or N) counts both `timesteps` and `ts_next`; sigma_dev /
 * sigma_next_dev as sigma_dev in ltx2_dit_denoise_step (NULL: the first timestep).  The workspace (3 x N*C fp32; on an AudioVideo context
 * 2 x Na*Ca more) is allocated on first use for the bound shapes, before anything is enqueued, and freed with ctx.
 * LTX2_E_INVALID, before anything is launched: the rules of ltx2_dit_guided_step (with neg NULL the same rules on ctx alone), sigma <= 0,
 * sigma_next < 0, ge_gamma < 0, ts_next missing while sigma_next > 0.
 * ltx2_dit_heun_step_av: the JOINT step on the AudioVideo engine (:600-724): both latents are stepped, each pass ONE launch over both
 * (ltx2_heun_predict_pair / ltx2_heun_correct_pair), the video under cfg_scale and the audio under audio_cfg_scale; GE acts on the video alone.
 * sigma_dev / sigma_next_dev: one float each, shared by the modalities (sigma_next_dev NULL: the first of v_ts_next).  Enqueued eagerly only:
 * there is no captured form of the joint loop.
 * ltx2_dit_ge_step: the Euler step with GE on the VideoOnly engine (:267-326): the evaluations of ltx2_dit_guided_step (neg NULL: one), then
 * ONE ltx2_ge_euler_step in place on `latent`; ge_gamma > 0, `first` as above.
 * ltx2_dit_graph_capture_heun: n_steps (< 64) Heun steps as one captured linear chain owned by ctx (ltx2_dit_graph_launch(ctx) replays it), built
 * like ltx2_dit_graph_capture_guided.  sigma_{i+1} is read on the device beside sigma_i; with a mask, mask * sigma_i is formed into ctx's buffer
 * before the first pair of evaluations and mask * sigma_{i+1} into the same buffer after the predictor.  A step whose sigma_next is 0 takes the
 * final-step form, decided on the host at capture.  first is 1 in step 0 only, and with ge_gamma > 0 a memset node at the head of the chain
 * clears the GE velocity, so every replay starts alike.  (additive entries of ABI version 3)                                             */
int ltx2_dit_heun_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev,
                       const float* ts_next, const float* sigma_next_dev, const float* mask, const float* clean, float cfg_scale, float ge_gamma,
                       int first, float sigma, float sigma_next, void* stream);
int ltx2_dit_heun_step_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                          const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_ts_next, const float* a_ts_next,
                          const float* sigma_next_dev, const float* v_mask, const float* v_clean, const float* a_mask, const float* a_clean,
                          float cfg_scale, float audio_cfg_scale, float ge_gamma, int first, float sigma, float sigma_next, void* stream);
int ltx2_dit_ge_step(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* timesteps, int n_timesteps, const float* sigma_dev, const float* mask,
                     const float* clean, float cfg_scale, float ge_gamma, int first, float sigma, float sigma_next, void* stream);
int ltx2_dit_graph_capture_heun(ltx2_dit* ctx, ltx2_dit* neg, float* latent, const float* host_sigmas, int n_steps, const float* mask, int64_t n_mask,
                                const float* clean, int64_t n_clean, float cfg_scale, float ge_gamma, void* stream);
/* One step of the two-stage pipeline's stage 1 on the AudioVideo engine (pipelines/two_stage.py:314-401): BOTH latents are stepped under
 * MultiModalGuider.calculate, each modality with its own scales.  In order on the caller's stream: forward(ctx) and, with neg, forward(neg) on both
 * modalities (as ltx2_dit_guided_step_av builds them); with the perturbed scratch pair, ltx2_dit_forward_perturbed_av on ctx into it; with the
 * isolated scratch pair, ltx2_dit_forward_isolated_av on ctx into it; then the element-wise passes in place: when both rescale scales are 0 ONE
 * ltx2_mm_guided_euler_step_pair, otherwise per modality ltx2_mm_guided_euler_step or ltx2_mm_guidance_sums + ltx2_mm_rescaled_euler_step.  A
 * pass that did not run contributes no term: neg NULL, a NULL scratch pair.  The scratch buffers are the caller's, [N][out_channels] and
 * [Na][audio_out_channels] fp32, a pair both NULL or both set; n_*: their ELEMENT counts, checked against the bound shapes.  The partials of a
 * modality that rescales are allocated on first use for the bound shapes, before anything is enqueued, and freed with ctx.  The step is
 * enqueued eagerly only: there is no captured form of the joint loop.
 * LTX2_E_INVALID, before anything is launched: the rules of ltx2_dit_guided_step_av (with neg NULL the same rules on ctx alone), a mask without
 * its clean latent, sigma == 0, a scratch of the wrong length or half a pair, a perturbed scratch with both sets of ltx2_dit_set_stg_blocks empty.
 * (additive entry of ABI version 3)                                                                                                    */
int ltx2_dit_mm_guided_step_av(ltx2_dit* ctx, ltx2_dit* neg, float* v_latent, float* a_latent, const float* v_timesteps, int n_v_timesteps,
                               const float* a_timesteps, int n_a_timesteps, const float* sigma_dev, const float* v_mask, const float* v_clean,
                               const float* a_mask, const float* a_clean, float* v_vel_isolated, int64_t n_v_isolated, float* a_vel_isolated,
                               int64_t n_a_isolated, float* v_vel_perturbed, int64_t n_v_perturbed, float* a_vel_perturbed, int64_t n_a_perturbed,
                               float v_cfg_scale, float v_stg_scale, float v_modality_scale, float v_rescale_scale, float a_cfg_scale, float a_stg_scale,
                               float a_modality_scale, float a_rescale_scale, float sigma, float sigma_next, void* stream);
int ltx2_dit_graph_capture_av(ltx2_dit* ctx, float* v_latent, float* a_latent, const float* host_sigmas, int n_steps,
                              void* stream);
int ltx2_dit_graph_launch(ltx2_dit* ctx, void* stream);

/* Text-context key mask of one modality (0 = video, 1 = audio): Modality.context_mask as the reference's boolean (B, S) mask
 * (model.py:163-201 turns it into the additive -finfo.max mask of attention.py:38-70): mask fp32 [S] on the device, non-zero = the key may
 * be attended; NULL clears it.  Applies to the text cross-attention of every block until changed; call after binding the workspace
 * (binding clears it).  Every pipeline of the reference passes context_mask = None (pipelines/common.py:223-232).                  */
int ltx2_dit_set_context_mask(ltx2_dit* ctx, int modality, const float* mask, int S, void* stream);

/* Engine options, by name (unknown names -> LTX2_E_INVALID):
 *   "fp8_compute" = 1 (before ltx2_dit_bind_workspace): every linear of the VIDEO stream whose weight is registered fp8-resident (LTX2_DTYPE_FP8_E4M3FN codes +
 *   `<name>_scale`) and whose GEMM has M >= 1024 rows runs as ltx2_gemm_fp8 on activations quantised per token
 *   (ltx2_quantize_rows_fp8).  Default 0: fp8-resident weights are expanded to bf16 inside the GEMM (bit-identical to the
 *   reference's dequantise-at-load).
 *   "adaln_combine" = 0 (any time): tables and timestep embeddings reach every kernel separately, as in round 3.  Default 1: with one
 *   timestep per modality the sums of all layers are formed by one launch at the top of the step (bit-identical results).
 *   "fold_norms" = 0 / 1 (any time; default 1; VideoOnly non-V2.3 models on dense 16-bit weights in the bfloat16 build, one timestep per modality):
 *   1: the text cross-attention's plain RMS pre-norm rides on attn1.to_out's epilogue and attn2.to_q's accumulators (ltx2_gemm_bf16_fold) instead of
 *   running as a pass over the residual stream; 0: round 5's form.  Same mathematics; the operand is rounded before the row factor instead of after it.
 *   "text_kv_ahead" = 0 (any time; AudioVideo models with cross_attention_adaln only): the video stream projects its sigma-modulated text K / V
 *   inline, in front of its text cross-attention (round 4's schedule).  Default 1 (round 5): they are a function of the prompt and sigma only,
 *   so layer l's are projected on the side stream at the top of layer l, beside the main stream's norm / QKV projection (bit-identical
 *   results; -1.4 ... -1.8 ms per LTX-2.3 step).  Ignored with fp8_compute (that projection shares the video stream's activation scratch).  */
int ltx2_dit_set_option(ltx2_dit* ctx, const char* name, int value);


/* Measurement aid: bracket every launch of one GEMM kernel instantiation (epilogue id, or -1 for
 * every GEMM) issued by this thread's ltx2_dit_* calls with HIP events on the launch stream;
 * profile_end synchronises and returns the summed kernel time, launch count and 2*M*N*K flops. */
int ltx2_dit_profile_begin(ltx2_dit* ctx, int epilogue);
int ltx2_dit_profile_end(ltx2_dit* ctx, double* total_ms, int64_t* launches, double* flops);

/* ------------------------------------------------------------------------------------------
 * VAE decoder engine: SimpleVideoDecoder.__call__ (model/video_vae/simple_decoder.py:446-563)
 * ------------------------------------------------------------------------------------------ */
typedef struct ltx2_vae ltx2_vae;

#define LTX2_VAE_MAX_BLOCKS 16
#define LTX2_VAE_RES 0
#define LTX2_VAE_UPSAMPLE 1

typedef struct ltx2_vae_config {
    int n_blocks;                             /* up_blocks in execution order (reversed decoder_blocks) */
    int kind[LTX2_VAE_MAX_BLOCKS];            /* LTX2_VAE_RES | LTX2_VAE_UPSAMPLE */
    int num_layers[LTX2_VAE_MAX_BLOCKS];      /* res: number of ResBlock3d */
    int stride[LTX2_VAE_MAX_BLOCKS][3];       /* upsample: (ft, fh, fw) */
    int multiplier[LTX2_VAE_MAX_BLOCKS];      /* upsample: out_channels_reduction_factor */
    int residual[LTX2_VAE_MAX_BLOCKS];
    int base_channels;                        /* 128 -> first feature width 1024 */
    int latent_channels;                      /* 128 */
    int timestep_conditioning;
    float decode_noise_scale;                 /* 0.025 */
} ltx2_vae_config;

int ltx2_vae_create(const ltx2_vae_config* cfg, ltx2_vae** out);
void ltx2_vae_destroy(ltx2_vae* ctx);
/* Names = checkpoint keys (simple_decoder.py:592-671).  conv weights: bf16 [Cout][27][Cin]
 * (upsample convs row-permuted for the depth-to-space epilogue); linear weights bf16 [out,in];
 * everything else fp32.                                                                       */
int ltx2_vae_set_weight(ltx2_vae* ctx, const char* name, const void* ptr, int dtype, int64_t numel);
/* value of the checkpoint scalar vae.decoder.timestep_scale_multiplier (default 1000) */
int ltx2_vae_set_timestep_multiplier(ltx2_vae* ctx, float multiplier);
int64_t ltx2_vae_workspace_bytes(const ltx2_vae* ctx, int T, int H, int W);
int ltx2_vae_bind_workspace(ltx2_vae* ctx, void* ptr, int64_t bytes);
/* latent fp32 [C][T][H][W] -> video fp32 [3][To][32H][32W] in [-1, 1].  timestep < 0 disables
 * timestep conditioning for this call; noise (fp32, latent-shaped, N(0,1)) may be NULL (zeros). */
int ltx2_vae_decode(ltx2_vae* ctx, const float* latent, int T, int H, int W, float timestep, const float* noise,
                    int causal, float* video, void* stream);
/* output frame count of one decode call for T latent frames */
int ltx2_vae_out_frames(const ltx2_vae* ctx, int T);

/* ---- Gemma-3 text encoder (prefill only; model/text_encoder/gemma3.py).  Additive entries: the DiT / VAE ABI above is unchanged.
 * Gemma runs on the bfloat16 build for both compute dtypes (the reference runs it in fp32; fp16 overflows, scripts/generate.py:376-378).
 * Causal / sliding-window / non-causal GQA flash attention at head_dim 256 (gemma3.py:186-241, masks :362-382):
 *   out[q, h*256:(h+1)*256] = softmax(scale * Q_h K_{h / (heads / kv_heads)}^T + mask) V_{h / (heads / kv_heads)}
 * key j visible from query i when j < Tkv and, with causal != 0, j <= i and (window == 0 or i - j < window).  causal == 0: no mask at
 * all (the reference's attention_mask=None); window must then be 0.  Q / K / V / out: bf16 row-major, query head h at columns h*256 of q,
 * kv head g at columns g*256 of k and v; 16-byte aligned rows.  A query row that sees no key is written as zeros. */
int ltx2_gemma_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo, int Tq,
                    int Tkv, int heads, int kv_heads, int causal, int window, float scale, void* stream);
/* In place on the fused QKV rows (q heads then kv heads, 256 wide, from column 0): per head y = rms_norm(x) * (1 + w) (w = q_w for the
 * q heads, k_w for the k heads; fp32 [256]), then rotate-half RoPE with cos / sin fp32 [rows][128] (gemma3.py:117-138, :206-224). */
int ltx2_gemma_qknorm_rope(void* qkv, int64_t ld, int rows, int q_heads, int kv_heads, const float* q_w, const float* k_w, float eps,
                           const float* cos, const float* sin, void* stream);
/* One row pass (gemma3.py:258-293): x = x_in + rms_norm(y) * (1 + w_post) (y NULL: x = x_in); n = rms_norm(x) * (1 + w_next);
 * x_out (fp32) = x, h_out (bf16) = n, hf_out (fp32) = n -- each output may be NULL.  D % 4 == 0, D <= 8192. */
int ltx2_gemma_resid_norm(const float* x_in, int64_t ldx, const void* y, int64_t ldy, const float* w_post, const float* w_next, float* x_out,
                          int64_t ld_xout, void* h_out, int64_t ldh, float* hf_out, int64_t ldhf, int rows, int D, float eps, void* stream);
/* out[r][i] = act(gu[r][i]) * gu[r][inter + i] (bf16; gate | up of one GEMM, gemma3.py:244-255); act 0 = silu (the reference),
 * 1 = gelu_pytorch_tanh (the released checkpoints' hidden_activation).  inter % 8 == 0. */
#define LTX2_GEMMA_ACT_SILU 0
#define LTX2_GEMMA_ACT_GELU_TANH 1
int ltx2_gemma_gated_act(const void* gu, int64_t ldgu, void* out, int64_t ldo, int rows, int inter, int act, void* stream);
/* x[r][:] = fp32(table[ids[r]][:]) * scale (gemma3.py:312, :352); an id outside [0, vocab) gives a zero row.  D % 4 == 0. */
int ltx2_gemma_embed(const int32_t* ids, int rows, const void* table, int vocab, int D, float scale, float* x, int64_t ldx, void* stream);
/* The LTX-2.3 (V2) feature extractor's GEMM operand in one pass over the L hidden states (feature_extractor.py:160-181):
 *   out[t][l * D + d] = valid[t] ? hs[l * layer_stride + t * row_stride + d] * rsqrt(mean_d(hs[l, t, :]^2) + eps) : 0
 * hs fp32 (strides in elements: the [L][T][D] buffer Gemma fills, or any such set of rows), valid int32 [T] or NULL (all valid), out in the
 * build's 16-bit type [T][ldo] with layer l at columns [l * D, (l + 1) * D) -- the column order of the re-ordered aggregate_embed weights.
 * fp32 sum, rounded once; pad rows are exact zeros; deterministic.  D % 8 == 0, D <= 8192, strides % 4 == 0, ldo % 8 == 0, ldo >= L * D. */
int ltx2_gemma_features_rms(const float* hs, int64_t layer_stride, int64_t row_stride, const int32_t* valid, void* out, int64_t ldo, int T, int L,
                            int D, float eps, void* stream);

/* ---- audio VAE decoder / vocoder (model/audio_vae/: AudioDecoder, Vocoder, VocoderWithBWE).  Additive entries; fp32 end to end
 * (operands, accumulation, activations), the same code in both builds.  Tensors are channels-last fp32: one row of C channels per time
 * step (1-D) or per (h, w) pixel (2-D, h-major); ld* are row strides in elements.
 * Convolution on the exact-f32 MFMA, M = h_out * w_out positions, N = c_out, K = kh * kw * c_in:
 *   y[p][n] = act(alpha * (bias[n] + res[p][n] + sum_{i,j,c} pro(x[src(p,i,j)][c]) * w[(i*kw + j)*c_in + c][n]) + beta * y[p][n])
 * p = (h, w) reads row h + upsample - pad_h + i and column w*stride + j*dilation - pad_w (zero outside the input); upsample != 0 reads
 * the nearest x2 image of x and drops the first output row (Upsample2d, decoder.py:223-244).  w: [K][ldw], ldw % 4 == 0, ldw >= c_out,
 * 16-byte aligned.  bias / res may be NULL; res may alias y.  1-D: h_in = h_out = kh = 1, pad_h = 0. */
#define LTX2_AUDIO_PRO_NONE 0
#define LTX2_AUDIO_PRO_LEAKY_RELU 1      /* v < 0 ? slope * v : v, on the operand as it is staged */
#define LTX2_AUDIO_PRO_MAGNITUDE 2       /* sqrt(x[c]^2 + x[c + c_in]^2): |STFT| from its real | imaginary halves (ldx >= 2 c_in) */
#define LTX2_AUDIO_ACT_NONE 0
#define LTX2_AUDIO_ACT_TANH 1
#define LTX2_AUDIO_ACT_CLIP 2            /* clip(v, -1, 1) */
#define LTX2_AUDIO_ACT_LOG 3             /* log(max(v, 1e-5)) */
int ltx2_audio_conv(const float* x, int64_t ldx, int h_in, int w_in, int c_in, const float* w, int64_t ldw, const float* bias, float* y,
                    int64_t ldy, int h_out, int w_out, int c_out, int kh, int kw, int stride, int dilation, int pad_h, int pad_w, int upsample,
                    int prologue, float slope, const float* res, int64_t ldres, float alpha, float beta, int act, void* stream);
/* Audio VAE encoder (model/audio_vae/encoder.py).  The same convolution strided along both axes: p = (h, w) reads row h*stride_h - pad_h + i
 * and column w*stride_w - pad_w + j, so Downsample2d (CausalConv2d(k = 3, stride = 2), encoder.py:23-33: pad_h = 2, pad_w = 1,
 * h_out = (h_in - 1) / 2 + 1, w_out = (w_in - 1) / 2 + 1) computes only the outputs it keeps.  No prologue, dilation 1, alpha 1, beta 0;
 * act: NONE or SILU (applied after bias and res: the encoder's silu(h) before conv_out, folded into mid.block_2.conv2).  ltx2_audio_conv
 * itself accepts acts 0..3 only. */
#define LTX2_AUDIO_ACT_SILU 4            /* v * sigmoid(v) */
int ltx2_audio_conv2d_strided(const float* x, int64_t ldx, int h_in, int w_in, int c_in, const float* w, int64_t ldw, const float* bias, float* y,
                              int64_t ldy, int h_out, int w_out, int c_out, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                              const float* res, int64_t ldres, int act, void* stream);
/* Encoder latent normalisation (encoder.py:172-203, patchify -> normalize -> unpatchify on the mean half) in one pass: channels-last
 * h [t][f][ld] (ld >= z; ld = 2z with double_z) -> out (z, t, f) fp32, out[c][t][f] = (h[t][f][c] - mean[c*f_dim + f]) / std[c*f_dim + f].
 * One IEEE subtract and one IEEE divide per element: equal to fp32 torch bit for bit. */
int ltx2_audio_latent_normalize(const float* h, int64_t ld, const float* mean, const float* std, float* out, int t, int f, int z, void* stream);
/* ConvTranspose1d(stride = rate, padding) as `rate` polyphase convolutions (vocoder.py:66-116); output length t_out.  w_phase:
 * [rate][ceil(k / rate)][c_in][round_up(c_out, 4)], phase ph = (o + padding) % rate, tap t = kernel index ph + rate * (ntaps - 1 - t)
 * (zero past k).  prologue: NONE or LEAKY_RELU. */
int ltx2_audio_conv_transpose1d(const float* x, int64_t ldx, int t_in, int c_in, const float* w_phase, const float* bias, float* y, int64_t ldy,
                                int t_out, int c_out, int k, int rate, int padding, int prologue, float slope, void* stream);
/* y[r][:] = silu(x[r][:] / sqrt(mean(x[r][:]^2) + eps)): PixelNorm + SiLU (decoder.py:29-55).  c % 4 == 0, 16-byte aligned rows. */
int ltx2_audio_pixnorm_silu(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int c, float eps, void* stream);
/* Activation1d(SnakeBeta) in one pass (vocoder.py:162-412): replicate pad, x2 upsample with up_filter, x + sin(x e^alpha)^2 / (e^beta + 1e-9),
 * replicate pad, low-pass with down_filter, decimate by 2.  [t][c] -> [t][c], out of place.  up_k even, up_k and down_k <= 16. */
int ltx2_audio_snake_aa(const float* x, int64_t ldx, int t, int c, const float* alpha, const float* beta, const float* up_filter, int up_k,
                        const float* down_filter, int down_k, float* y, int64_t ldy, void* stream);
/* UpSample1d (vocoder.py:304-367): y[u][c] = ratio * sum_k f[k] x[clamp((u + pad_left - k) / ratio - pad, 0, t_in - 1)][c] over the k with
 * (u + pad_left - k) % ratio == 0, u < t_out.  Out of place. */
int ltx2_audio_upsample(const float* x, int64_t ldx, int t_in, int c, const float* filter, int k, int ratio, int pad, int pad_left, float* y,
                        int64_t ldy, int t_out, void* stream);

/* ---- control-video path of the IC-LoRA pipeline (pipelines/ic_lora.py).  Additive entries; integer arithmetic except frames_to_patches.
 * Canny edges of F uint8 RGB frames: edges[f][y][x] = 255 on an edge, 0 elsewhere.  The definition is OpenCV's Canny with apertureSize 3 and
 * L2gradient false, written out (no OpenCV binary was at hand to check it against: the gray weights and the tie rules are unverified):
 *   gray = (R*9798 + G*19235 + B*3735 + 16384) >> 15;  gx, gy = the 3x3 Sobel operators on gray with a replicated border, in integers;
 *   mag = |gx| + |gy|, 0 outside the image;  low, high are floored to integers and swapped if low > high.
 *   A pixel with mag > low is kept if it passes non-maximum suppression along its quantised direction: x = |gx|, y = |gy| << 15,
 *   t22 = x * 13573;  y < t22: horizontal, keep when mag > left && mag >= right;  else t67 = t22 + (x << 16);  y > t67: vertical, keep when
 *   mag > up && mag >= down;  otherwise diagonal with s = -1 if (gx ^ gy) < 0 else +1, keep when mag > mag[y-1][x-s] && mag > mag[y+1][x+s].
 *   A kept pixel with mag > high is strong (2), any other kept pixel weak (1).  Hysteresis: 255 for every strong pixel and for every weak
 *   pixel 8-connected to a strong one through weak or strong pixels; frames are independent.
 * ltx2_canny_hysteresis is the second stage alone on a given map of {0, 1, 2}.  It runs passes over LTX2_CANNY_TILE_H x LTX2_CANNY_TILE_W
 * tiles (a fixpoint per tile in LDS; no block waits on another) and reads one int back per pass until a pass promotes nothing on a tile
 * rim; more than H * W relaunches is LTX2_E_STATE.  Both calls therefore synchronise `stream` and cannot be captured into a graph.
 * *passes (may be NULL) receives the number of passes.  workspace: device memory, 4-byte aligned, LTX2_CANNY_FLAG_BYTES for the hysteresis
 * alone, LTX2_CANNY_FLAG_BYTES + F * H * W for ltx2_canny_u8 (the map).  map and edges must not alias. */
#define LTX2_CANNY_TILE_H 32
#define LTX2_CANNY_TILE_W 64
#define LTX2_CANNY_FLAG_BYTES 16
int ltx2_canny_u8(const uint8_t* rgb, int F, int H, int W, float low, float high, uint8_t* edges, void* workspace, int64_t workspace_bytes,
                  int* passes, void* stream);
int ltx2_canny_hysteresis(const uint8_t* map, int F, int H, int W, uint8_t* edges, void* workspace, int64_t workspace_bytes, int* passes,
                          void* stream);
/* uint8 frames [F][H][W][Cin] (Cin 3, or 1 replicated to three colours) -> the VAE encoder's patchified operand [F][H/4][W/4][64] in the
 * build's 16-bit type: channel (c*4 + r_w)*4 + r_h = pixel (4 hq + r_h, 4 wq + r_w) of colour c as x / 127.5f - 1.0f (one IEEE divide and
 * one subtract in fp32, rounded once), channels 48..63 zero: what patchify_video makes of the fp32 clip, in one pass.  H, W multiples of 4;
 * frames 4-byte and out 16-byte aligned. */
int ltx2_frames_to_patches(const uint8_t* frames, int F, int H, int W, int Cin, void* out, void* stream);

/* ---- source-clip glue of the retake pipeline (pipelines/retake.py).  Additive entries.
 * encoded: the VAE encoder's latent, channel-major fp32 [C][F][H][W]; noise: token-major fp32 [F*H*W][C].  One pass writes
 *   clean[p][c]  = encoded[c][p]                                   (VideoLatentPatchifier(patch_size = 1).patchify),
 *   mask[p]      = 1.0f for the tokens of the latent frames [f0, f1), 0.0f elsewhere   (TemporalRegionMask),
 *   latent[p][c] = noise[p][c] * sm + clean[p][c] * (1.0f - sm),  sm = mask[p] * noise_scale   (GaussianNoiser),
 * each multiplication, the subtraction and the addition rounded on its own (no FMA), so the three outputs equal the separate fp32 torch
 * statements bit for bit.  0 <= f0 <= f1 <= F; out of place: no output may overlap an input or another output. */
int ltx2_retake_prepare(const float* encoded, const float* noise, int C, int F, int H, int W, int f0, int f1, float noise_scale, float* clean,
                        float* mask, float* latent, void* stream);
/* uint8 clips [T][H][W][3]: out = decoded on the pixel frames [p0, p1).  A frame t outside the window lies at distance d = p0 - t (before)
 * or t - p1 + 1 (after); with R = ramp + 1 and a = max(R - d, 0) every byte of it is (decoded * a + source * (R - a) + R / 2) / R in
 * integers: a linear fade over `ramp` frames OUTSIDE the window, the source's own bytes beyond it (ramp = 0: on every frame outside).
 * 0 <= p0 <= p1 <= T, 0 <= ramp <= LTX2_RETAKE_MAX_RAMP; out may not overlap an input.  16 bytes per lane when all three clips are
 * 16-byte aligned, one byte per lane otherwise and for the last T*H*W*3 % 16 bytes. */
#define LTX2_RETAKE_MAX_RAMP 65535
int ltx2_retake_composite(const uint8_t* decoded, const uint8_t* source, int T, int H, int W, int p0, int p1, int ramp, uint8_t* out, void* stream);
/* The same glue for the clip's sound track.  encoded: the audio VAE encoder's latent, fp32 [C][T][M] (checkpoints: C = 8, M = 16); noise: token-major
 * fp32 [T][C*M].  One pass writes
 *   clean[t][c*M + m] = encoded[c][t][m]                             (AudioPatchifier.patchify),
 *   mask[t]           = 1.0f on the latent frames [a0, a1), 0.0f elsewhere,
 *   latent[t][j]      = noise[t][j] * sm + clean[t][j] * (1.0f - sm),  sm = mask[t] * noise_scale,
 * rounded as ltx2_retake_prepare rounds (no FMA): the separate fp32 torch statements, bit for bit.  0 <= a0 <= a1 <= T; out of place. */
int ltx2_retake_prepare_audio(const float* encoded, const float* noise, int C, int T, int M, int a0, int a1, float noise_scale, float* clean,
                              float* mask, float* latent, void* stream);
/* fp32 waveforms [channels][S] at one rate: out = decoded on the samples [s0, s1).  A sample outside the window lies at distance d = s0 - s
 * (before) or s - s1 + 1 (after), as in ltx2_retake_composite; with R = ramp + 1 and a = max(R - d, 0) it is
 *   (decoded * (float)a + source * (float)(R - a)) / (float)R
 * as two multiplies, one add and one IEEE divide, each rounded on its own (no FMA); a == 0 (ramp = 0: every sample outside) is the source's own
 * bits.  0 <= s0 <= s1 <= S, 0 <= ramp <= LTX2_RETAKE_AUDIO_MAX_RAMP (R stays exact in fp32); out may not overlap an input. */
#define LTX2_RETAKE_AUDIO_MAX_RAMP 16777215
int ltx2_retake_composite_audio(const float* decoded, const float* source, int channels, int64_t S, int64_t s0, int64_t s1, int ramp, float* out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LTX2HIP_H */
