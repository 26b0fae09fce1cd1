// C ABI (include/ltx2hip.h): error channel + thin extern "C" wrappers over the kernel launchers.
// The DiT / VAE engine entry points live in dit_engine.hip / vae_engine.hip.
#include <stdarg.h>
#include <stdio.h>

#include "../../include/ltx2hip.h"
#include "attention.h"
#include "fbc.h"
#include "gemm.h"
#include "gemma.h"
#include "rowops.h"
#include "sampler.h"

static thread_local char g_err[512] = "";

void ltx2_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// The shared tail of the two *_qkv_vt entries: the V columns as attention's V^T operand from the GEMM's epilogue where the route can, else by a transpose pass behind it
static int gemm_qkv_vt(GemmParams& p, void* vt, int vt_col0, int Npad, int head_dim, int* fused, hipStream_t stream) {
    gemm_set_vt(p, vt, vt_col0, Npad, head_dim);
    const bool f = gemm_vt_fused(p, EPI_BF16);
    if (fused) *fused = f ? 1 : 0;
    if (!f) p.vt = nullptr;
    const int rc = gemm_launch(p, EPI_BF16, false, stream);
    if (rc != LTX2_OK || f) return rc;
    return vt_transpose_launch((const bf16*)p.out + vt_col0, p.ldo, (bf16*)vt, p.M, Npad, (p.N - vt_col0) / head_dim, stream, head_dim);
}

extern "C" {

const char* ltx2_last_error(void) { return g_err; }
void ltx2_clear_error(void) { g_err[0] = 0; }
int ltx2_abi_version(void) { return LTX2_ABI_VERSION; }

int ltx2_gemm_bf16(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M,
                   int N, int K, int epilogue, const float* gate, int64_t gate_stride, const float* gate_table,
                   const void* res, int64_t ldres, void* stream) {
    LTX2_CHECK_ARG(epilogue >= 0 && epilogue <= LTX2_EPI_ADD_BF16, "gemm: epilogue %d out of range", epilogue);
    LTX2_CHECK_ARG(epilogue != LTX2_EPI_ADD_BF16 || res, "gemm: epilogue ADD_BF16 needs res");
    GemmParams p = gemm_dense_params((const bf16*)A, lda, (const bf16*)W, bias, out, ldo, M, N, K);
    gemm_set_gate(p, gate, gate_stride, gate_table);
    p.res = (const bf16*)res;
    p.ldres = ldres;
    return gemm_launch(p, epilogue, false, (hipStream_t)stream);
}

int ltx2_adaln_rmsnorm2(const float* x, int64_t ldx, void* out0, void* out1, int64_t ldo, int rows, int D, float eps, const float* scale0,
                        const float* shift0, const float* scale1, const float* shift1, void* stream) {
    LTX2_CHECK_ARG(x && out0 && out1, "adaln_rmsnorm2: null operand");
    const float* sct[2] = {scale0, scale1};
    const float* sht[2] = {shift0, shift1};
    const float* none[2] = {nullptr, nullptr};
    return norm_mod2_launch(x, ldx, (bf16*)out0, (bf16*)out1, ldo, rows, D, eps, sct, sht, none, none, (hipStream_t)stream);
}

int ltx2_gemm_bf16_rowss(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M, int N, int K, float* rowss,
                         int* written, void* stream) {
    LTX2_CHECK_ARG(A && W && out && rowss && written, "gemm_bf16_rowss: null argument");
    GemmParams p = gemm_dense_params((const bf16*)A, lda, (const bf16*)W, bias, out, ldo, M, N, K);
    *written = gemm_rowss_supported(p, EPI_BF16) ? 1 : 0;
    if (*written) p.rowss = rowss;
    return gemm_launch(p, EPI_BF16, false, (hipStream_t)stream);
}

int ltx2_gemm_bf16_fold(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M, int N, int K, int epilogue,
                        const float* gate_table, void* shadow, int64_t ld_shadow, const float* shadow_scale, float* shadow_ss, int64_t ld_ss,
                        const float* rf_parts, int64_t rf_ld, int rf_nparts, int rf_dim, float rf_eps, int* supported, void* stream) {
    LTX2_CHECK_ARG(A && W && out && supported, "gemm_bf16_fold: null argument");
    LTX2_CHECK_ARG(epilogue == LTX2_EPI_BF16 || epilogue == LTX2_EPI_GELU_BF16 || epilogue == LTX2_EPI_RESID_GATE_F32, "gemm_bf16_fold: epilogue %d (BF16, GELU_BF16 or RESID_GATE_F32)", epilogue);
    GemmParams p = gemm_dense_params((const bf16*)A, lda, (const bf16*)W, bias, out, ldo, M, N, K);
    gemm_set_gate(p, nullptr, 0, gate_table);
    gemm_set_fold_producer(p, shadow, ld_shadow, shadow_scale, shadow_ss, ld_ss);
    gemm_set_fold_consumer(p, rf_parts, rf_ld, rf_nparts, rf_dim, rf_eps);
    *supported = ((p.shadow || p.rf_parts) && gemm_fold_supported(p, epilogue)) ? 1 : 0;
    if (!*supported) return LTX2_OK;
    return gemm_launch(p, epilogue, false, (hipStream_t)stream);
}

int ltx2_flash_attn_rowscale(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                             int H, int head_dim, float scale, const float* q_ss, int q_ss_ld, int q_norm_dim, float q_eps, void* stream) {
    LTX2_CHECK_ARG(Q && K && VT && out && q_ss, "flash_attn_rowscale: null operand");
    LTX2_CHECK_ARG(head_dim == 128, "flash_attn_rowscale: head_dim=%d, only 128 is implemented", head_dim);
    AttnParams a = attn_params(Q, ldq, K, ldk, VT, Npad, out, ldo, Nq, Nkv, H, head_dim, scale * 1.4426950408889634f);
    attn_set_rowscale(a, q_ss, q_ss_ld, q_norm_dim, q_eps);
    return attn_launch(a, (hipStream_t)stream);
}

int ltx2_flash_attn_keymask(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                            int H, int head_dim, float scale, const float* mask, void* words, void* stream) {
    LTX2_CHECK_ARG(Q && K && VT && out && mask && words, "flash_attn_keymask: null operand");
    if (const int rc = keymask_words_launch(mask, Nkv, (unsigned long long*)words, Npad / 64, (hipStream_t)stream)) return rc;
    AttnParams a = attn_params(Q, ldq, K, ldk, VT, Npad, out, ldo, Nq, Nkv, H, head_dim, scale * 1.4426950408889634f);
    a.kmask = (const unsigned long long*)words;
    return attn_launch(a, (hipStream_t)stream);
}

int ltx2_gemm_route(int M, int N, int K, int epilogue, int weights, int has_vt) {
    // host logic only: addresses are never dereferenced (16-byte aligned dummies satisfy the alignment checks)
    static const long dummy[2] = {0, 0};
    GemmParams p = gemm_dense_params((const bf16*)dummy, K, (const bf16*)dummy, nullptr, (void*)dummy, N, M, N, K);
    if (weights >= 1) gemm_set_w8(p, dummy, (const float*)dummy);
    if (weights == 2) gemm_set_a8(p, dummy, (const float*)dummy, K);
    const int r = gemm_route(p, epilogue, false);
    if (!has_vt || r < 0) return r;
    gemm_set_vt(p, (void*)dummy, 2 * (N / 3), (M + 63) / 64 * 64, (N / 3) % 128 == 0 ? 128 : 64);
    return r | (gemm_vt_fused(p, epilogue) ? 0x100 : 0);
}

int ltx2_quantize_rows_fp8(const void* x, int64_t ldx, int rows, int K, void* codes, int64_t ldo, float* scale, void* stream) {
    LTX2_CHECK_ARG(x && codes && scale, "quantize_rows_fp8: null argument");
    return quant_rows_fp8_launch((const bf16*)x, ldx, rows, K, (unsigned char*)codes, ldo, scale, (hipStream_t)stream);
}

int ltx2_gemm_fp8(const void* A8, int64_t lda, const float* ascale, const void* W8, const float* wscale, const float* bias, void* out,
                  int64_t ldo, int M, int N, int K, int epilogue, const float* gate, int64_t gate_stride, const float* gate_table,
                  void* stream) {
    LTX2_CHECK_ARG(A8 && ascale && W8 && wscale && out, "gemm_fp8: null operand");
    GemmParams p = gemm_dense_params(nullptr, lda, nullptr, bias, out, ldo, M, N, K);
    gemm_set_w8(p, W8, wscale);
    gemm_set_a8(p, A8, ascale, lda);
    gemm_set_gate(p, gate, gate_stride, gate_table);
    return gemm_launch(p, epilogue, false, (hipStream_t)stream);
}

int ltx2_gemm_qkv_vt(const void* A, int64_t lda, const void* W, const float* bias, void* out, int64_t ldo, int M, int N, int K,
                     void* vt, int vt_col0, int Npad, int head_dim, int* fused, void* stream) {
    LTX2_CHECK_ARG(A && W && out && vt, "gemm_qkv_vt: null operand");
    LTX2_CHECK_ARG(head_dim == 64 || head_dim == 128, "gemm_qkv_vt: head_dim=%d, only 128 and 64 are implemented", head_dim);
    LTX2_CHECK_ARG(vt_col0 > 0 && vt_col0 < N && (N - vt_col0) % head_dim == 0 && Npad % 64 == 0 && Npad >= M, "gemm_qkv_vt: bad V column range / Npad");
    GemmParams p = gemm_dense_params((const bf16*)A, lda, (const bf16*)W, bias, out, ldo, M, N, K);
    return gemm_qkv_vt(p, vt, vt_col0, Npad, head_dim, fused, (hipStream_t)stream);
}

int ltx2_gemm_fp8_qkv_vt(const void* A8, int64_t lda, const float* ascale, const void* W8, const float* wscale, const float* bias, void* out,
                         int64_t ldo, int M, int N, int K, void* vt, int vt_col0, int Npad, int head_dim, int* fused, void* stream) {
    LTX2_CHECK_ARG(A8 && ascale && W8 && wscale && out && vt, "gemm_fp8_qkv_vt: null operand");
    LTX2_CHECK_ARG(head_dim == 64 || head_dim == 128, "gemm_fp8_qkv_vt: head_dim=%d, only 128 and 64 are implemented", head_dim);
    LTX2_CHECK_ARG(vt_col0 > 0 && vt_col0 < N && (N - vt_col0) % head_dim == 0 && Npad % 64 == 0 && Npad >= M, "gemm_fp8_qkv_vt: bad V column range / Npad");
    GemmParams p = gemm_dense_params(nullptr, lda, nullptr, bias, out, ldo, M, N, K);
    gemm_set_w8(p, W8, wscale);
    gemm_set_a8(p, A8, ascale, lda);
    return gemm_qkv_vt(p, vt, vt_col0, Npad, head_dim, fused, (hipStream_t)stream);
}

int ltx2_gemm_w8a16(const void* A, int64_t lda, const void* W8, const float* wscale, const float* bias, void* out, int64_t ldo, int M,
                    int N, int K, int epilogue, const float* gate, int64_t gate_stride, const float* gate_table, void* stream) {
    LTX2_CHECK_ARG(A && W8 && wscale && out, "gemm_w8a16: null operand");
    GemmParams p = gemm_dense_params((const bf16*)A, lda, nullptr, bias, out, ldo, M, N, K);
    gemm_set_w8(p, W8, wscale);
    gemm_set_gate(p, gate, gate_stride, gate_table);
    return gemm_launch(p, epilogue, false, (hipStream_t)stream);
}

int ltx2_gemv_f32(const float* a, int64_t lda, const void* W, const float* bias, float* out, int64_t ldo, int M,
                  int N, int K, int act_in, int act_out, void* stream) {
    LTX2_CHECK_ARG(a && W && out, "gemv: null operand");
    return gemv_launch(a, lda, (const bf16*)W, bias, out, ldo, M, N, K, act_in, act_out, (hipStream_t)stream);
}

int ltx2_adaln_rmsnorm(const float* x, int64_t ldx, void* out, int64_t ldo, int rows, int D, float eps,
                       int layer_norm, const float* scale_tab, const float* shift_tab, const float* scale_emb,
                       const float* shift_emb, int64_t emb_stride, void* stream) {
    LTX2_CHECK_ARG(x && out, "adaln_rmsnorm: null operand");
    return norm_mod_launch(x, ldx, (bf16*)out, ldo, rows, D, eps, layer_norm, scale_tab, shift_tab, scale_emb, shift_emb,
                           emb_stride, (hipStream_t)stream);
}

int ltx2_adaln_rmsnorm_fp8(const float* x, int64_t ldx, void* out_bf16, int64_t ldo, void* codes, int64_t ldq, float* scale, int rows, int D,
                           float eps, int layer_norm, const float* scale_tab, const float* shift_tab, const float* scale_emb,
                           const float* shift_emb, int64_t emb_stride, void* stream) {
    LTX2_CHECK_ARG(x && codes && scale, "adaln_rmsnorm_fp8: null operand");
    return norm_mod_launch(x, ldx, (bf16*)out_bf16, ldo, rows, D, eps, layer_norm, scale_tab, shift_tab, scale_emb, shift_emb, emb_stride,
                           (hipStream_t)stream, (unsigned char*)codes, ldq, scale);
}

int ltx2_qknorm_rope(void* buf, int64_t ld, int rows, int D, int head_dim, int q_off, const float* q_weight,
                     int k_off, const float* k_weight, float eps, const float* cos, const float* sin, void* stream) {
    LTX2_CHECK_ARG(buf && q_weight, "qknorm_rope: null operand");
    const int offs[2] = {q_off, k_off};
    const float* wts[2] = {q_weight, k_weight};
    return qknorm_rope_launch((bf16*)buf, ld, rows, D, head_dim, k_weight ? 2 : 1, offs, wts, eps, cos, sin,
                              (hipStream_t)stream);
}

int ltx2_vt_transpose(const void* V, int64_t ld, void* VT, int Nkv, int Npad, int H, int head_dim, void* stream) {
    LTX2_CHECK_ARG(V && VT, "vt_transpose: null operand");
    return vt_transpose_launch((const bf16*)V, ld, (bf16*)VT, Nkv, Npad, H, (hipStream_t)stream, head_dim);
}

int ltx2_attn_head_gate(void* att, int64_t ld, const void* x, int64_t ldx, const void* gate_w, const float* gate_b,
                        float* logits, int rows, int Dq, int H, int head_dim, void* stream) {
    LTX2_CHECK_ARG(att && x && gate_w && gate_b && logits, "attn_head_gate: null operand");
    int rc = gate_logits_launch((const bf16*)x, ldx, (const bf16*)gate_w, gate_b, logits, H, rows, Dq, H, (hipStream_t)stream);
    if (rc != LTX2_OK) return rc;
    return head_gate_launch((bf16*)att, ld, logits, H, rows, H, head_dim, (hipStream_t)stream);
}

int ltx2_flash_attn_gated(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                          int H, int head_dim, float scale, const float* gate_logits, int gate_ld, void* stream) {
    LTX2_CHECK_ARG(Q && K && VT && out && gate_logits && gate_ld >= H, "flash_attn_gated: null operand / gate_ld < H");
    LTX2_CHECK_ARG(head_dim == 128 || head_dim == 64, "flash_attn_gated: head_dim=%d, only 128 and 64 are implemented", head_dim);
    AttnParams a = attn_params(Q, ldq, K, ldk, VT, Npad, out, ldo, Nq, Nkv, H, head_dim, scale * 1.4426950408889634f);
    attn_set_gate(a, gate_logits, gate_ld);
    return attn_launch(a, (hipStream_t)stream);
}

int ltx2_flash_attn_gated_parts(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out, int64_t ldo, int Nq, int Nkv,
                                int H, int head_dim, float scale, const void* x, int64_t ldx, const void* gate_w, const float* gate_b, int Dq, float* parts,
                                void* stream) {
    LTX2_CHECK_ARG(Q && K && VT && out && x && gate_w && gate_b && parts, "flash_attn_gated_parts: null operand");
    LTX2_CHECK_ARG(head_dim == 128 || head_dim == 64, "flash_attn_gated_parts: head_dim=%d, only 128 and 64 are implemented", head_dim);
    if (const int rc = gate_logits_parts_launch((const bf16*)x, ldx, (const bf16*)gate_w, parts, Nq, Dq, H, (hipStream_t)stream)) return rc;
    AttnParams a = attn_params(Q, ldq, K, ldk, VT, Npad, out, ldo, Nq, Nkv, H, head_dim, scale * 1.4426950408889634f);
    attn_set_gate(a, parts, H, GATE_LOGIT_PARTS, gate_b);
    return attn_launch(a, (hipStream_t)stream);
}

int ltx2_flash_attn(const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* VT, int Npad, void* out,
                    int64_t ldo, int Nq, int Nkv, int H, int head_dim, float scale, void* stream) {
    LTX2_CHECK_ARG(Q && K && VT && out, "flash_attn: null operand");
    LTX2_CHECK_ARG(head_dim == 128 || head_dim == 64, "flash_attn: head_dim=%d, only 128 and 64 are implemented", head_dim);
    AttnParams a = attn_params(Q, ldq, K, ldk, VT, Npad, out, ldo, Nq, Nkv, H, head_dim, scale * 1.4426950408889634f);
    return attn_launch(a, (hipStream_t)stream);
}

int ltx2_timestep_sinusoid(const float* t, int64_t t_stride, float mult, int T, int dim, float* out_f32,
                           void* out_bf16, void* stream) {
    LTX2_CHECK_ARG(t && (out_f32 || out_bf16), "timestep_sinusoid: null operand");
    return timestep_sinusoid_launch(t, t_stride, 0.f, mult, T, dim, out_f32, (bf16*)out_bf16, (hipStream_t)stream);
}

int ltx2_dequant_fp8_e4m3fn(const void* in, float scale, void* out_bf16, int64_t n, void* stream) {
    return dequant_fp8_launch((const unsigned char*)in, scale, (bf16*)out_bf16, n, (hipStream_t)stream);
}

int ltx2_groupnorm_silu(const void* x, const void* res, void* y, int64_t P, int C, int groups, float eps,
                        const float* gamma, const float* beta, float* scratch, int act, void* stream) {
    return groupnorm_silu_launch((const bf16*)x, (const bf16*)res, (bf16*)y, P, C, groups, eps, gamma, beta, scratch, act, (hipStream_t)stream);
}

int ltx2_groupnorm_frames_silu(const void* x, const void* res, void* y, int frames, int64_t P_frame, int C, int groups, int interleaved,
                               float eps, const float* gamma, const float* beta, float* scratch, int act, void* stream) {
    return groupnorm_frames_silu_launch((const bf16*)x, (const bf16*)res, (bf16*)y, frames, P_frame, C, groups, interleaved, eps, gamma, beta,
                                        scratch, act, (hipStream_t)stream);
}

int ltx2_s2d_downsample(const void* y, const void* x, void* out, int T, int H, int W, int Cc, int Cin, int st, int sh,
                        int sw, void* stream) {
    return s2d_downsample_launch((const bf16*)y, (const bf16*)x, (bf16*)out, T, H, W, Cc, Cin, st, sh, sw, (hipStream_t)stream);
}

int ltx2_latent_normalize_nchw(const void* x, const float* mean, const float* std, float* out, int C, int64_t P, void* stream) {
    return latent_normalize_nchw_launch((const bf16*)x, mean, std, out, C, P, (hipStream_t)stream);
}

int ltx2_rope_tables(const float* positions, const float* freq_grid, const float* max_pos, int N, int n_dims, int n_freq,
                     int half_dim, float* cos_out, float* sin_out, void* stream) {
    return rope_tables_launch(positions, freq_grid, max_pos, N, n_dims, n_freq, half_dim, cos_out, sin_out, (hipStream_t)stream);
}

int ltx2_cast_f32_bf16(const float* in, void* out, int64_t n, void* stream) {
    LTX2_CHECK_ARG(in && out, "cast: null operand");
    return cast_f32_bf16_launch(in, (bf16*)out, n, (hipStream_t)stream);
}

int ltx2_x0_from_velocity(const float* latent, const float* velocity, const float* ts_ptr, int64_t ts_stride,
                          float ts_scalar, float* x0, int rows, int C, void* stream) {
    LTX2_CHECK_ARG(latent && velocity && x0, "x0_from_velocity: null operand");
    return x0_from_velocity_launch(latent, velocity, ts_ptr, ts_stride, ts_scalar, x0, rows, C, (hipStream_t)stream);
}

int ltx2_euler_step(const float* x, const float* x0, const float* mask, const float* clean, float sigma,
                    float sigma_next, float* out, int rows, int C, void* stream) {
    LTX2_CHECK_ARG(x && x0 && out, "euler_step: null operand");
    return euler_step_launch(x, x0, mask, clean, sigma, sigma_next, out, rows, C, (hipStream_t)stream);
}

int ltx2_guided_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride,
                           const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next,
                           float* out, int rows, int C, void* stream) {
    return guided_euler_step_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, sigma, sigma_next, out, rows, C,
                                    (hipStream_t)stream);
}

int ltx2_guided_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                                const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                                const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next,
                                void* stream) {
    return guided_euler_step_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, v_out, v_rows, v_C, a_x,
                                         a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_out, a_rows, a_C, sigma,
                                         sigma_next, (hipStream_t)stream);
}

int ltx2_philox_bits(uint32_t* out, int64_t n_quads, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, void* stream) {
    return philox_bits_launch(out, (long)n_quads, seed_dev, step, stream_id, (hipStream_t)stream);
}

int ltx2_philox_normal(float* out, int64_t n, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, void* stream) {
    return philox_normal_launch(out, (long)n, seed_dev, step, stream_id, (hipStream_t)stream);
}

int ltx2_ancestral_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                              const float* clean, float cfg_scale, float sigma, float sigma_up, float sigma_down, const uint64_t* seed_dev,
                              uint32_t step, float* out, int rows, int C, void* stream) {
    return ancestral_euler_step_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, sigma, sigma_up, sigma_down, seed_dev, step,
                                       out, rows, C, (hipStream_t)stream);
}

int ltx2_ancestral_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                                   const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                   const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                                   const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_up,
                                   float sigma_down, const uint64_t* seed_dev, uint32_t step, void* stream) {
    return ancestral_euler_step_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, v_out, v_rows, v_C, a_x,
                                            a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_out, a_rows, a_C, sigma,
                                            sigma_up, sigma_down, seed_dev, step, (hipStream_t)stream);
}

int ltx2_ancestral_euler_step_x0(const float* x, const float* x0, const float* mask, const float* clean, float sigma, float sigma_up, float sigma_down,
                                 const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, float* out, int rows, int C, void* stream) {
    return ancestral_euler_step_x0_launch(x, x0, mask, clean, sigma, sigma_up, sigma_down, seed_dev, step, stream_id, out, rows, C, (hipStream_t)stream);
}

int ltx2_stg_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* ts, int64_t ts_stride,
                        const float* mask, const float* clean, float cfg_scale, float stg_scale, float sigma, float sigma_next, float* out, int rows,
                        int C, void* stream) {
    return stg_euler_step_launch(x, vel_cond, vel_uncond, vel_perturbed, ts, (long)ts_stride, mask, clean, cfg_scale, stg_scale, sigma, sigma_next, out,
                                 rows, C, (hipStream_t)stream);
}

int ltx2_stg_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed, const float* v_ts,
                             int64_t v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float v_stg_scale, float* v_out,
                             int v_rows, int v_C, const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed,
                             const float* a_ts, int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float a_stg_scale,
                             float* a_out, int a_rows, int a_C, float sigma, float sigma_next, void* stream) {
    return stg_euler_step_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_vel_perturbed, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, v_stg_scale,
                                      v_out, v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_vel_perturbed, a_ts, (long)a_ts_stride, a_mask, a_clean,
                                      a_cfg_scale, a_stg_scale, a_out, a_rows, a_C, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_res2s_midpoint(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                        const float* clean, float cfg_scale, float c, int n_bong, float* x_mid, float* anchor, float* eps1, int rows, int C,
                        void* stream) {
    return res2s_midpoint_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, c, n_bong, x_mid, anchor, eps1, rows, C,
                                 (hipStream_t)stream);
}

int ltx2_res2s_combine(const float* x_mid, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                       const float* clean, float cfg_scale, const float* anchor, const float* eps1, float h, float b1, float b2, float* out,
                       int rows, int C, void* stream) {
    return res2s_combine_launch(x_mid, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, anchor, eps1, h, b1, b2, out, rows, C,
                                (hipStream_t)stream);
}

int ltx2_res2s_midpoint_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                             const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_x_mid, float* v_anchor, float* v_eps1, int v_rows,
                             int v_C, const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride,
                             const float* a_mask, const float* a_clean, float a_cfg_scale, float* a_x_mid, float* a_anchor, float* a_eps1, int a_rows,
                             int a_C, float c, int n_bong, void* stream) {
    return res2s_midpoint_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, v_x_mid, v_anchor, v_eps1,
                                      v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_x_mid,
                                      a_anchor, a_eps1, a_rows, a_C, c, n_bong, (hipStream_t)stream);
}

int ltx2_res2s_combine_pair(const float* v_x_mid, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                            const float* v_mask, const float* v_clean, float v_cfg_scale, const float* v_anchor, const float* v_eps1, float* v_out,
                            int v_rows, int v_C, const float* a_x_mid, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts,
                            int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, const float* a_anchor,
                            const float* a_eps1, float* a_out, int a_rows, int a_C, float h, float b1, float b2, void* stream) {
    return res2s_combine_pair_launch(v_x_mid, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, v_anchor, v_eps1, v_out,
                                     v_rows, v_C, a_x_mid, a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_anchor,
                                     a_eps1, a_out, a_rows, a_C, h, b1, b2, (hipStream_t)stream);
}

int ltx2_heun_predict(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                      const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* d, float* xp,
                      int rows, int C, void* stream) {
    return heun_predict_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, ge_gamma, prev, first, sigma, sigma_next, d, xp, rows, C,
                               (hipStream_t)stream);
}

int ltx2_heun_correct(const float* x, const float* d, const float* xp, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride,
                      const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, float* out, int rows, int C, void* stream) {
    return heun_correct_launch(x, d, xp, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, sigma, sigma_next, out, rows, C,
                               (hipStream_t)stream);
}

int ltx2_ge_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                       const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* out, int rows,
                       int C, void* stream) {
    return ge_euler_step_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, cfg_scale, ge_gamma, prev, first, sigma, sigma_next, out, rows, C,
                                (hipStream_t)stream);
}

int ltx2_heun_predict_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride, const float* v_mask,
                           const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_d, float* v_xp, int v_rows, int v_C,
                           const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                           const float* a_clean, float a_cfg_scale, float* a_d, float* a_xp, int a_rows, int a_C, float sigma, float sigma_next,
                           void* stream) {
    return heun_predict_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, ge_gamma, v_prev, first, v_d, v_xp,
                                    v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_d, a_xp, a_rows, a_C,
                                    sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_heun_correct_pair(const float* v_x, const float* v_d, const float* v_xp, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts,
                           int64_t v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C,
                           const float* a_x, const float* a_d, const float* a_xp, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts,
                           int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma,
                           float sigma_next, void* stream) {
    return heun_correct_pair_launch(v_x, v_d, v_xp, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, v_out, v_rows, v_C, a_x,
                                    a_d, a_xp, a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_out, a_rows, a_C, sigma,
                                    sigma_next, (hipStream_t)stream);
}

int ltx2_ge_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride, const float* v_mask,
                            const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_out, int v_rows, int v_C,
                            const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, const float* a_mask,
                            const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next, void* stream) {
    return ge_euler_step_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_cfg_scale, ge_gamma, v_prev, first, v_out,
                                     v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_out, a_rows, a_C,
                                     sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_guidance_sums_blocks(int rows, int C) { return guidance_sums_blocks(rows, C); }

int ltx2_guidance_sums(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, float* running, int first,
                       float momentum, double* partials, int rows, int C, void* stream) {
    return guidance_sums_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, running, first, momentum, partials, rows, C, (hipStream_t)stream);
}

int ltx2_projected_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, const float* mask,
                              const float* clean, const float* running, const double* partials, int mode, float scale, float eta,
                              float norm_threshold, float sigma, float sigma_next, float* out, float* scalars_out, int rows, int C, void* stream) {
    return projected_euler_step_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, mask, clean, running, partials, mode, scale, eta, norm_threshold,
                                       sigma, sigma_next, out, scalars_out, rows, C, (hipStream_t)stream);
}

int ltx2_guidance_sums_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride, float* v_running,
                            int v_first, float v_momentum, double* v_partials, int v_rows, int v_C, const float* a_x, const float* a_vel_cond,
                            const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride, float* a_running, int a_first, float a_momentum,
                            double* a_partials, int a_rows, int a_C, void* stream) {
    return guidance_sums_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_running, v_first, v_momentum, v_partials, v_rows, v_C, a_x,
                                     a_vel_cond, a_vel_uncond, a_ts, (long)a_ts_stride, a_running, a_first, a_momentum, a_partials, a_rows, a_C,
                                     (hipStream_t)stream);
}

int ltx2_projected_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, int64_t v_ts_stride,
                                   const float* v_mask, const float* v_clean, const float* v_running, const double* v_partials, int v_mode,
                                   float v_scale, float v_eta, float v_norm_threshold, float* v_out, float* v_scalars_out, int v_rows, int v_C,
                                   const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, int64_t a_ts_stride,
                                   const float* a_mask, const float* a_clean, const float* a_running, const double* a_partials, int a_mode,
                                   float a_scale, float a_eta, float a_norm_threshold, float* a_out, float* a_scalars_out, int a_rows, int a_C,
                                   float sigma, float sigma_next, void* stream) {
    return projected_euler_step_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, (long)v_ts_stride, v_mask, v_clean, v_running, v_partials, v_mode, v_scale,
                                            v_eta, v_norm_threshold, v_out, v_scalars_out, v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_ts,
                                            (long)a_ts_stride, a_mask, a_clean, a_running, a_partials, a_mode, a_scale, a_eta, a_norm_threshold, a_out,
                                            a_scalars_out, a_rows, a_C, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_mm_guided_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                              const float* ts, int64_t ts_stride, const float* mask, const float* clean, float cfg_scale, float stg_scale,
                              float modality_scale, float sigma, float sigma_next, float* out, int rows, int C, void* stream) {
    return mm_guided_euler_step_launch(x, vel_cond, vel_uncond, vel_perturbed, vel_isolated, ts, (long)ts_stride, mask, clean, cfg_scale, stg_scale,
                                       modality_scale, sigma, sigma_next, out, rows, C, (hipStream_t)stream);
}

int ltx2_mm_guided_euler_step_pair(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed,
                                   const float* v_vel_isolated, const float* v_ts, int64_t v_ts_stride, const float* v_mask, const float* v_clean,
                                   float v_cfg_scale, float v_stg_scale, float v_modality_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                   const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed, const float* a_vel_isolated,
                                   const float* a_ts, int64_t a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale,
                                   float a_stg_scale, float a_modality_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next,
                                   void* stream) {
    return mm_guided_euler_step_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_vel_perturbed, v_vel_isolated, v_ts, (long)v_ts_stride, v_mask, v_clean,
                                            v_cfg_scale, v_stg_scale, v_modality_scale, v_out, v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_vel_perturbed,
                                            a_vel_isolated, a_ts, (long)a_ts_stride, a_mask, a_clean, a_cfg_scale, a_stg_scale, a_modality_scale, a_out,
                                            a_rows, a_C, sigma, sigma_next, (hipStream_t)stream);
}

int ltx2_mm_guidance_sums(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                          const float* ts, int64_t ts_stride, float cfg_scale, float stg_scale, float modality_scale, double* partials, float* pred_out,
                          int rows, int C, void* stream) {
    return mm_guidance_sums_launch(x, vel_cond, vel_uncond, vel_perturbed, vel_isolated, ts, (long)ts_stride, cfg_scale, stg_scale, modality_scale, partials,
                                   pred_out, rows, C, (hipStream_t)stream);
}

int ltx2_mm_rescaled_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                                const float* ts, int64_t ts_stride, const float* mask, const float* clean, const double* partials, float cfg_scale,
                                float stg_scale, float modality_scale, float rescale_scale, float sigma, float sigma_next, float* out,
                                float* scalars_out, int rows, int C, void* stream) {
    return mm_rescaled_euler_step_launch(x, vel_cond, vel_uncond, vel_perturbed, vel_isolated, ts, (long)ts_stride, mask, clean, partials, cfg_scale,
                                         stg_scale, modality_scale, rescale_scale, sigma, sigma_next, out, scalars_out, rows, C, (hipStream_t)stream);
}

int ltx2_channel_guidance_stats_blocks(int rows, int C) { return channel_guidance_stats_blocks(rows, C); }

int ltx2_channel_guidance_stats(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride, float cfg_scale,
                                double* partials, float* stats, int rows, int C, void* stream) {
    return channel_guidance_stats_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, cfg_scale, partials, stats, rows, C, (hipStream_t)stream);
}

int ltx2_rescaled_guided_euler_step(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, int64_t ts_stride,
                                    const float* stats, float cfg_scale, double guidance_rescale, float sigma, float sigma_next, float* out, int rows,
                                    int C, void* stream) {
    return rescaled_guided_euler_step_launch(x, vel_cond, vel_uncond, ts, (long)ts_stride, stats, cfg_scale, guidance_rescale, sigma, sigma_next, out, rows,
                                             C, (hipStream_t)stream);
}

int ltx2_fbc_metric_blocks(int64_t n) { return fbc_metric_blocks((long)n); }

int ltx2_fbc_head_metric(const float* h0, const float* h1, const float* head_prev, float* r, float* h1_save, double* partials, void* record,
                         float threshold, int64_t n, void* stream) {
    return fbc_head_metric_launch(h0, h1, head_prev, r, h1_save, partials, (FbcRecord*)record, threshold, (long)n, (hipStream_t)stream);
}

int ltx2_fbc_store_tail(const float* hL, const float* h1, float* tail, int64_t n, void* stream) {
    return fbc_store_tail_launch(hL, h1, tail, (long)n, (hipStream_t)stream);
}

int ltx2_fbc_apply_tail(float* h, const float* tail, int64_t n, void* stream) { return fbc_apply_tail_launch(h, tail, (long)n, (hipStream_t)stream); }

int ltx2_vae_prepare_latent(const float* latent, const float* std, const float* mean, const float* noise,
                            float noise_scale, void* out_bf16, int C, int64_t P, void* stream) {
    LTX2_CHECK_ARG(latent && std && mean && out_bf16, "vae_prepare_latent: null operand");
    return vae_prepare_latent_launch(latent, std, mean, noise, noise_scale, (bf16*)out_bf16, C, P, (hipStream_t)stream);
}

int ltx2_pixnorm_mod_silu(const void* x, void* y, int64_t P, int C, float eps, const float* table, const float* te,
                          int shift_row, int scale_row, void* stream) {
    LTX2_CHECK_ARG(x && y && table, "pixnorm_mod_silu: null operand");
    return pixnorm_mod_silu_launch((const bf16*)x, (bf16*)y, P, C, eps, table, te, shift_row, scale_row,
                                   (hipStream_t)stream);
}

int ltx2_vae_unpatchify(const void* x, float* video, int T, int H, int W, void* stream) {
    LTX2_CHECK_ARG(x && video, "vae_unpatchify: null operand");
    return vae_unpatchify_launch((const bf16*)x, video, T, H, W, (hipStream_t)stream);
}

int ltx2_video_chunk_to_uint8(const float* cur, const float* prev, const float* ramp, uint8_t* frames, int Tc, int prev_T, int ov, int H,
                              int W, int t_dst0, int T_out, void* stream) {
    LTX2_CHECK_ARG(cur && frames, "video_chunk_to_uint8: null operand");
    return video_chunk_to_uint8_launch(cur, prev, ramp, frames, Tc, prev_T, ov, H, W, t_dst0, T_out, (hipStream_t)stream);
}

int ltx2_tile_blend_accumulate(const float* tile, int dt, int dh, int dw, int nt, int nh, int nw, const float* mt, const float* mh,
                               const float* mw, float* out, float* wsum, int OT, int OH, int OW, int t0, int h0, int w0, void* stream) {
    LTX2_CHECK_ARG(tile && mt && mh && mw && out && wsum, "tile_blend_accumulate: null operand");
    return tile_blend_accumulate_launch(tile, dt, dh, dw, nt, nh, nw, mt, mh, mw, out, wsum, OT, OH, OW, t0, h0, w0, (hipStream_t)stream);
}

int ltx2_tile_blend_finish(float* out, const float* wsum, int64_t plane, void* stream) {
    LTX2_CHECK_ARG(out && wsum && plane > 0, "tile_blend_finish: bad argument");
    return tile_blend_finish_launch(out, wsum, (long)plane, (hipStream_t)stream);
}

int ltx2_video_to_uint8(const float* video, uint8_t* frames, int T, int H, int W, void* stream) {
    LTX2_CHECK_ARG(video && frames, "video_to_uint8: null operand");
    return video_to_uint8_launch(video, frames, T, H, W, (hipStream_t)stream);
}

int ltx2_gemma_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo, int Tq,
                    int Tkv, int heads, int kv_heads, int causal, int window, float scale, void* stream) {
    return gemma_attn_launch((const bf16*)q, (long)ldq, (const bf16*)k, (long)ldk, (const bf16*)v, (long)ldv, (bf16*)out, (long)ldo, Tq, Tkv,
                             heads, kv_heads, causal, window, scale, (hipStream_t)stream);
}

int ltx2_gemma_qknorm_rope(void* qkv, int64_t ld, int rows, int q_heads, int kv_heads, const float* q_w, const float* k_w, float eps,
                           const float* cos, const float* sin, void* stream) {
    return gemma_qknorm_rope_launch((bf16*)qkv, (long)ld, rows, q_heads, kv_heads, q_w, k_w, eps, cos, sin, (hipStream_t)stream);
}

int ltx2_gemma_resid_norm(const float* x_in, int64_t ldx, const void* y, int64_t ldy, const float* w_post, const float* w_next, float* x_out,
                          int64_t ld_xout, void* h_out, int64_t ldh, float* hf_out, int64_t ldhf, int rows, int D, float eps, void* stream) {
    return gemma_resid_norm_launch(x_in, (long)ldx, (const bf16*)y, (long)ldy, w_post, w_next, x_out, (long)ld_xout, (bf16*)h_out, (long)ldh,
                                   hf_out, (long)ldhf, rows, D, eps, (hipStream_t)stream);
}

int ltx2_gemma_gated_act(const void* gu, int64_t ldgu, void* out, int64_t ldo, int rows, int inter, int act, void* stream) {
    return gemma_gated_act_launch((const bf16*)gu, (long)ldgu, (bf16*)out, (long)ldo, rows, inter, act, (hipStream_t)stream);
}

int ltx2_gemma_embed(const int32_t* ids, int rows, const void* table, int vocab, int D, float scale, float* x, int64_t ldx, void* stream) {
    return gemma_embed_launch((const int*)ids, rows, (const bf16*)table, vocab, D, scale, x, (long)ldx, (hipStream_t)stream);
}

int ltx2_gemma_features_rms(const float* hs, int64_t layer_stride, int64_t row_stride, const int32_t* valid, void* out, int64_t ldo, int T, int L,
                            int D, float eps, void* stream) {
    return gemma_features_rms_launch(hs, (long)layer_stride, (long)row_stride, (const int*)valid, (bf16*)out, (long)ldo, T, L, D, eps,
                                     (hipStream_t)stream);
}

}  // extern "C"
