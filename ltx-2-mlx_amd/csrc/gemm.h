// bf16 MFMA GEMM / implicit-GEMM conv3d for gfx950: parameter block + host launchers.
#pragma once
#include "common.h"

enum GemmEpilogue {
    EPI_BF16 = 0,            // out_bf16 = acc + bias
    EPI_GELU_BF16 = 1,       // out_bf16 = gelu_tanh(acc + bias)
    EPI_SILU_BF16 = 2,       // out_bf16 = silu(acc + bias)
    EPI_F32 = 3,             // out_f32  = acc + bias
    EPI_RESID_GATE_F32 = 4,  // out_f32[m][n] += (gate[m*gate_stride+n] + gate_table[n]) * (acc + bias)
    EPI_ADD_BF16 = 5,        // out_bf16 = acc + bias + res_bf16[m*ldres + n]
    EPI_D2S_BF16 = 6,        // conv only: depth-to-space scatter (+ tiled d2s(x) residual)
    EPI_COUNT = 7
};

struct GemmParams {
    const bf16* A;       // dense: [M][lda];  conv: activations [T][H][W][Cin] (channels-last)
    const bf16* W;       // [N][K]  (K contiguous; conv: K = tap*Cin + c, tap = (kt*3+kh)*3+kw)
    const unsigned char* W8;  // fp8-resident weights (gemm_v4.hip): e4m3fn codes [N][K] instead of W, with
    const float* wscale;      //   one dequantisation scale per output column: w = bf16(f32(code) * wscale[n])
    const unsigned char* A8;  // fp8 COMPUTE (gemm_v4.hip layout 5): e4m3fn activation codes [M][lda] instead of A, with one scale per
    const float* ascale;      //   row; needs W8 / wscale too: out = epilogue(ascale[m] * wscale[n] * sum_k a8[m][k] * w8[n][k] + bias)
    const float* bias;   // [N] or null
    void* out;           // bf16 or f32, [M][ldo]  (D2S: [To][Ho][Wo][Cf])
    const float* gate;   // EPI_RESID_GATE_F32: per-row part  gate[m*gate_stride + n]  (may be null)
    const float* gate_table;  // EPI_RESID_GATE_F32: broadcast part gate_table[n]  (may be null; both null -> 1)
    const bf16* res;     // EPI_ADD_BF16
    long lda, ldo, gate_stride, ldres;
    int M, N, K;
    // conv geometry (implicit GEMM): M = T*H*Wd output positions, stride 1, 3x3x3
    int T, H, Wd, Cin, cin_shift, pad_front;
    int taps_t;          // temporal kernel size: 3 (3x3x3) or 1 (per-frame 3x3); K = 9*taps_t*Cin
    int pad_zero;        // 0: reflect H/W + replicate T (VAE decoder); 1: zero padding in T/H/W (spatial upscaler);
                         // 2: zero padding in H/W + replicate T (VAE encoder)
    // depth-to-space epilogue: column n = s*Cf + c, s = (a*fh + b)*fw + d
    int ft, fh, fw, Cf, cf_shift, drop_first, d2s_residual, c_d2s;
    // gemm_v4.hip, EPI_BF16, dense, layout 3: output columns >= vt_col0 (the V third of a fused QKV projection) are written
    // TRANSPOSED and key-permuted as attention's V^T operand vt[h][vt_hd][vt_npad] (attention.hip, vt_transpose_kernel's
    // layout: rows >= M zero-filled up to vt_npad) instead of into `out`; null = off.  gemm_v4_vt_supported() says when.
    bf16* vt;
    long vt_head_stride;
    int vt_col0, vt_npad, vt_hd;
    // gemm_v4.hip, EPI_BF16, dense, layouts 3 / 5: rowss[m * (N / 64) + n / 64] = sum over the 64-column strip of out[m][n]^2 (of the
    // ROUNDED outputs): the partial sums of a row's squared norm, for a consumer that folds an RMS normalisation of `out` into its own
    // arithmetic (text cross-attention: q_norm as a per-row softmax scale).  null = off.  gemm_rowss_supported() says when.
    float* rowss;
    // ---- round 6: the plain RMS normalisation in front of a projection folded around the GEMMs (gemm_v4.hip layout 3, dense bf16 weights; gemm_fold_supported()) ----
    // rms_norm(x) W^T + b equals r[m] (x W^T) + b with r[m] = rsqrt(mean x[m]^2 + eps): the PRODUCER of x (the gated-residual epilogue that forms the new
    // residual row) also leaves y = bf16(x_new) and the partial sums of squares of x_new (one per 256-column tile); the CONSUMER forms the row factors of its
    // tile's rows from those partials (fetched into LDS in front of its K loop) and multiplies its accumulators by them -- the stand-alone norm pass and the
    // fp32 re-read of x between the two GEMMs are gone.  (A scale (1 + s) rides on the shadow; a shift t would need t W^T per step: measured, not kept -- DESIGN.md.)
    // Producer (EPI_RESID_GATE_F32, row-invariant gate):
    bf16* shadow;              //   shadow[m][n] = bf16(x_new[m][n] * (1 + shadow_scale[n])), row stride ld_shadow; null = off
    const float* shadow_scale; //   [N] or null (plain RMS norm: * 1)
    float* shadow_ss;          //   shadow_ss[(n / 256) * ld_ss + m] = sum of x_new[m][n]^2 over the 256-column tile (fp32, before the scale; the tile's four waves added in wave order)
    long ld_shadow, ld_ss;     //   ld_ss >= the row tiles' extent (ceil(M / tile rows) * tile rows), % 4 == 0
    // Consumer (EPI_BF16 / EPI_GELU_BF16): out = epilogue(r[m] * acc + bias), r[m] = rsqrt(sum_{j < rf_nparts} rf_parts[j * rf_ld + m] / rf_dim + rf_eps)
    const float* rf_parts;     //   a producer's shadow_ss (rf_ld = its ld_ss); null: r = 1
    long rf_ld;
    int rf_nparts, rf_dim;     //   rf_nparts <= GEMM_RF_MAX_PARTS
    float rf_eps;
    int splitk;          // gemm_v4.hip: K split over this many blocks per tile (fp32 slabs + reduce); 0 / 1 = off
    void* dbg;           // ping-pong kernel: optional device buffer for interval timestamps (debug)
};

// ---- filling a GemmParams: dense operands and shape first, then what the call adds (everything else is set field by field) ----
inline GemmParams gemm_dense_params(const bf16* A, long lda, const bf16* W, const float* bias, void* out, long ldo, int M, int N, int K) {
    GemmParams p{};
    p.A = A;
    p.lda = lda;
    p.W = W;
    p.bias = bias;
    p.out = out;
    p.ldo = ldo;
    p.M = M;
    p.N = N;
    p.K = K;
    return p;
}
// fp8-resident weight: e4m3fn codes + one scale per output column in place of W
inline void gemm_set_w8(GemmParams& p, const void* W8, const float* wscale) {
    p.W = nullptr;
    p.W8 = (const unsigned char*)W8;
    p.wscale = wscale;
}
// fp8 compute: per-row quantised activations (codes [M][lda] + one scale per row) in place of A; needs gemm_set_w8 too
inline void gemm_set_a8(GemmParams& p, const void* A8, const float* ascale, long lda) {
    p.A = nullptr;
    p.A8 = (const unsigned char*)A8;
    p.ascale = ascale;
    p.lda = lda;
}
// columns >= col0 go to vt[h][hd][npad] as attention's V^T operand (ask gemm_vt_fused() before the launch)
inline void gemm_set_vt(GemmParams& p, void* vt, int col0, int npad, int hd) {
    p.vt = (bf16*)vt;
    p.vt_col0 = col0;
    p.vt_npad = npad;
    p.vt_hd = hd;
    p.vt_head_stride = (long)hd * npad;
}
// EPI_RESID_GATE_F32: per-row part gate[m * gate_stride + n] and broadcast part gate_table[n] (either may be null)
inline void gemm_set_gate(GemmParams& p, const float* gate, long gate_stride, const float* gate_table) {
    p.gate = gate;
    p.gate_stride = gate_stride;
    p.gate_table = gate_table;
}
// a folded norm's producer half (EPI_RESID_GATE_F32): the new rows' 16-bit shadow and their partial sums of squares (ask gemm_fold_supported())
inline void gemm_set_fold_producer(GemmParams& p, void* shadow, long ld_shadow, const float* shadow_scale, float* shadow_ss, long ld_ss) {
    p.shadow = (bf16*)shadow;
    p.ld_shadow = ld_shadow;
    p.shadow_scale = shadow_scale;
    p.shadow_ss = shadow_ss;
    p.ld_ss = ld_ss;
}
// ... and its consumer half (EPI_BF16 / EPI_GELU_BF16): row factors from a producer's shadow_ss (rf_ld = its ld_ss)
inline void gemm_set_fold_consumer(GemmParams& p, const float* rf_parts, long rf_ld, int rf_nparts, int rf_dim, float rf_eps) {
    p.rf_parts = rf_parts;
    p.rf_ld = rf_ld;
    p.rf_nparts = rf_nparts;
    p.rf_dim = rf_dim;
    p.rf_eps = rf_eps;
}

int gemm_launch(const GemmParams& p, int epilogue, bool conv, hipStream_t stream);
inline bool gemm_v4_prefer_224(const GemmParams& p) {
    const long nt = p.N / 256, cus = 256;
    const long t256 = ((long)(p.M + 255) / 256) * nt, t224 = ((long)(p.M + 223) / 224) * nt;
    const long cost256 = (t256 + cus - 1) / cus * 256, cost224 = (t224 + cus - 1) / cus * 224;
    return p.A8 ? cost224 * 100 <= cost256 * 108 : cost224 < cost256;
}
// Which kernel gemm_launch hands this problem to (host logic only, nothing is launched): gemm_route() is the only place that decides,
// gemm_launch and the gemm_*_supported / gemm_vt_fused queries follow it.  The dispatch is a parity surface, so tests/test_host_cpu.py
// enumerates every GEMM the three models issue and pins its route, and compares a grid of 47 520 problems with a recorded table.
enum GemmRoute {
    ROUTE_INVALID = -1,
    ROUTE_SKINNY = 0,      // gemm_skinny.hip: M <= 128 rows (the audio stream), weight-streaming
    ROUTE_V4_224 = 1,      // gemm_v4.hip layout 3, 224-row tiles (the DiT's big GEMMs)
    ROUTE_V4_256 = 2,      // gemm_v4.hip layout 3, 256-row tiles
    ROUTE_V4_W8_224 = 3,   // ... with fp8-resident weights expanded in the loop
    ROUTE_V4_W8_256 = 4,
    ROUTE_V4_F8_224 = 5,   // gemm_v4.hip fp8 compute: layout 6 (16x16x128 blocks)
    ROUTE_V4_F8_256 = 6,   //   layout 5 (32x32x64 blocks)
    ROUTE_PP = 7,          // gemm_pp.hip: 256x256 ping-pong (big grids the asm-loop kernel does not take; convs of the upscaler / encoder)
    ROUTE_SMALL = 8,       // gemm.hip 128x128
    ROUTE_NARROW = 9       // gemm.hip 128x64 (N <= 64)
};
// The 4-wave kernel of a ROUTE_V4_* route: gemm_v4_kernel<EPI, layout, bm, false, var> (bm = 0: not a 4-wave route).  var 30 = the
// instantiations that implement a folded norm's producer / consumer half, var 20 = fp8-resident weights expanded in the K loop.
struct GemmV4Kernel {
    int layout, bm, var;
};
#ifndef LTX2_F8_FORCE_L5
#define LTX2_F8_FORCE_L5 0          // (A/B builds: gemm.hip=-DLTX2_F8_FORCE_L5=1 keeps every fp8 GEMM on layout 5)
#endif
inline GemmV4Kernel gemm_v4_kernel_of(int route, const GemmParams& p) {
    switch (route) {
        case ROUTE_V4_224: return {3, 224, (p.shadow || p.rf_parts) ? 30 : 0};
        case ROUTE_V4_256: return {3, 256, (p.shadow || p.rf_parts) ? 30 : 0};
        case ROUTE_V4_W8_224: return {3, 224, 20};
        case ROUTE_V4_W8_256: return {3, 256, 20};
        // 224-row tiles: the 16x16x128 form (+16 % FLOP per joule on random e4m3 operands, tools/micro/mfma_fp8_power.hip)
        case ROUTE_V4_F8_224: return {LTX2_F8_FORCE_L5 ? 5 : 6, 224, 0};
        case ROUTE_V4_F8_256: return {5, 256, 0};
        default: return {0, 0, 0};
    }
}
int gemm_route(const GemmParams& p, int epilogue, bool conv);
// p.vt set: will gemm_launch route this problem to the kernel that writes V^T from its epilogue?  (false: clear p.vt and run
// vt_transpose_launch after the GEMM; gemm_launch rejects a p.vt it cannot honour.)
bool gemm_vt_fused(const GemmParams& p, int epilogue);
// p.rowss set: will gemm_launch route this problem to a kernel that writes the row partial sums?  (false: the caller must not set it)
bool gemm_rowss_supported(const GemmParams& p, int epilogue);
// p.shadow / p.rf_parts set: will gemm_launch route this problem to the kernel that implements them (the 4-wave layout-3 kernel on dense bf16 weights)?
// gemm_launch rejects what it cannot honour.
bool gemm_fold_supported(const GemmParams& p, int epilogue);
constexpr int GEMM_RF_MAX_PARTS = 24;      // partial sums per row the consumer stages in LDS (a producer of up to 6144 columns)
// fp8 compute (p.A8 / p.ascale / p.W8 / p.wscale set): can the fp8-MFMA kernel (gemm_v4.hip layouts 5 / 6) take this problem?
bool gemm_v4_f8_supported(const GemmParams& p, int epilogue);

// Skinny path (M <= 16 rows, fp32 activations, bf16 weights): out_f32 = act_out(in_act(a) @ W^T + b)
// act codes: 0 none, 1 silu, 2 gelu_tanh
int gemv_launch(const float* a, long lda, const bf16* W, const float* bias, float* out, long ldo,
                int M, int N, int K, int in_act, int out_act, hipStream_t stream);
