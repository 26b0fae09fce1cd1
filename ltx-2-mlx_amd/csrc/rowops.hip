// HBM-bound row / elementwise kernels of the DiT step, for gfx950.  All loads are 8/16-byte vectors; reductions use wave64 shuffles.
//   norm_mod (per-row, row-invariant, two-modulation forms), adaln_combine, qknorm_rope, ctx_mod, gate_logits (+ parts), head_gate
//   rope_tables, timestep_sinusoid
//   cast_f32_bf16, keymask_words, quant_rows_fp8, dequant_fp8
// The three norm kernels are one row body (norm_row_load / norm_row_stats / norm_mod_at / norm_row_apply) under three grid walks; the
// fused norm -> fp8 path and the stand-alone quantiser share block_max_256 / fp8_row_scale / pack4_fp8, which is why they agree bit for bit.
// The upscalers' GroupNorms are in groupnorm.hip, the VAE's glue kernels in vae_glue.hip; rowops.h declares the launchers of all three.
//
// Reference semantics restated (paths under the reference's LTX_2_MLX):
//   norm_mod          model/transformer/transformer.py:16-31 (_compiled_adaln_forward),
//                     attention.py:88-100 (rms_norm), model.py:744-758 (LayerNorm + shift/scale)
//   norm_mod2         transformer.py:556-620 (the a2v and v2a scale / shift rows of one normalised stream)
//   qknorm_rope       attention.py:231-237 (q_norm/k_norm over the FULL inner dim),
//                     rope.py:92-144 (apply_split_rotary_emb)
//   ctx_mod           transformer.py:441-451
//   gate_logits, head_gate   attention.py:241-249
//   rope_tables       rope.py:214-328,365-418
//   timestep_sinusoid timestep_embedding.py:10-60 with flip_sin_to_cos=True, shift 0;
//                     video_vae/simple_decoder.py:12-39
//   dequant_fp8       loader/fp8_loader.py:14-51; weight_converter.py:391-395
#include "rowops.h"

// ---- build switches (A/B builds: tools/ab_build.py NAME rowops.hip='-DLTX2_...=value') ----
#ifndef LTX2_NORM_BLOCKS
#define LTX2_NORM_BLOCKS 1024       // blocks of the row-invariant form (each loads the combined tables once); A/B builds: -DLTX2_NORM_BLOCKS=512 / 2048
#endif
#ifndef LTX2_QK_BLOCKS
#define LTX2_QK_BLOCKS 2048         // up to this many blocks; beyond that a block takes several rows (each block loads the norm weights once; 512 .. 4096 measured the same)
#endif
#ifndef LTX2_GATE_X_FIRST
#define LTX2_GATE_X_FIRST 1     // (A/B) the first DEPTH activation fragments are requested BEFORE the weight slice is staged: the two memory round trips overlap
#endif

namespace {

// ---- per-row e4m3fn quantisation of the fp8 compute path: amax = max |x| over the row (block_max_256), then ----
// scale = amax / 448 (1 when the row is all zeros), inv = 1 / scale (IEEE)
__device__ __forceinline__ float fp8_row_scale(float amax, float& inv) {
    const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
    inv = 1.0f / scale;
    return scale;
}
// code[k] = e4m3fn_rne(x[k] * inv), four codes to a word.  v_cvt_pk_fp8_f32 is the OCP conversion (round to nearest even, subnormals
// kept); |x * inv| <= 448 (1 + 2^-23) never reaches the overflow threshold (464).
__device__ __forceinline__ unsigned pack4_fp8(float x0, float x1, float x2, float x3, float inv) {
    unsigned c = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
    c = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(x0 * inv, x1 * inv, (int)c, false);
    c = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(x2 * inv, x3 * inv, (int)c, true);
#endif
    return c;
}

// fp8 compute path: the block's row (already rounded to bf16: the values the bf16 path would hand the GEMM) leaves as per-token
// e4m3fn codes + scale -- ltx2_quantize_rows_fp8's arithmetic on the same bf16 values, so fused and unfused agree bit for bit.
template <int NV>
__device__ __forceinline__ void row_to_fp8(const bf16x4 (&o)[NV], int D, float* red, unsigned char* qrow, float* qscale_row) {
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int d = threadIdx.x * 4 + i * 1024;
        if (d < D)
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fabsf(bf2f(o[i][e])));
    }
    amax = block_max_256<true>(amax, red);      // `red` still holds the row's sums for the block's other waves
    float inv;
    const float scale = fp8_row_scale(amax, inv);
    if (threadIdx.x == 0) *qscale_row = scale;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int d = threadIdx.x * 4 + i * 1024;
        if (d >= D) continue;
        *(unsigned*)(qrow + d) = pack4_fp8(bf2f(o[i][0]), bf2f(o[i][1]), bf2f(o[i][2]), bf2f(o[i][3]), inv);
    }
}

// ---- the row body of the three norm kernels ----
// Thread t of the block's 256 owns the 4-vectors at columns d = 4 t + 1024 i, i < NV, of a row of D <= 1024 NV floats; the row is read
// ONCE and held in registers.  The expressions are written as hipcc contracts them into FMAs: keep their shape.
// SUM1 false: s1 is left alone (the RMS-only kernel has no use for the mean).
template <int NV, bool SUM1 = true>
__device__ __forceinline__ void norm_row_load(const float* xr, int D, f32x4 (&v)[NV], float& s1, float& s2) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int d = threadIdx.x * 4 + i * 1024;
        v[i] = (d < D) ? *(const f32x4*)(xr + d) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (SUM1) s1 += v[i][0] + v[i][1] + v[i][2] + v[i][3];
        s2 += v[i][0] * v[i][0] + v[i][1] * v[i][1] + v[i][2] * v[i][2] + v[i][3] * v[i][3];
    }
}
// the row's block sums -> rstd, and the mean (0 for the RMS norm)
__device__ __forceinline__ float norm_row_stats(float s1, float s2, int D, float eps, int layer_norm, float& mean) {
    mean = layer_norm ? s1 / (float)D : 0.f;
    const float ms = s2 / (float)D;
    const float var = layer_norm ? fmaxf(ms - mean * mean, 0.f) : ms;
    return rsqrtf(var + eps);
}
// (1 + scale, shift) of the four columns at d.  1 + (table + embedding): the same rounding whether the sum arrives combined
// (adaln_combine) or in two parts; a null pointer counts 0, and a vector beyond the row (in_row false) reads nothing.
struct RowMod {
    f32x4 sc1, sh;
};
__device__ __forceinline__ RowMod norm_mod_at(int d, bool in_row, const float* scale_tab, const float* shift_tab, const float* scale_emb,
                                              const float* shift_emb) {
    f32x4 sc = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};
    if (in_row) {
        if (scale_tab) sc += *(const f32x4*)(scale_tab + d);
        if (scale_emb) sc += *(const f32x4*)(scale_emb + d);
        if (shift_tab) h += *(const f32x4*)(shift_tab + d);
        if (shift_emb) h += *(const f32x4*)(shift_emb + d);
    }
    return {1.f + sc, h};
}
// row-invariant modulation: the thread's NV vectors once per block
template <int NV>
__device__ __forceinline__ void norm_mod_rows(int D, const float* scale_tab, const float* shift_tab, const float* scale_emb,
                                              const float* shift_emb, RowMod (&m)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int d = threadIdx.x * 4 + i * 1024;
        m[i] = norm_mod_at(d, d < D, scale_tab, shift_tab, scale_emb, shift_emb);
    }
}
// out = (v - mean) * rstd * (1 + scale) + shift, rounded to the 16-bit type; stored to orow (may be null) and kept in ov for the fp8 path.
// mod(i, d) gives the RowMod of vector i.
template <int NV, class Mod>
__device__ __forceinline__ void norm_row_apply(const f32x4 (&v)[NV], int D, float mean, float rstd, Mod mod, bf16* orow, bf16x4 (&ov)[NV]) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int d = threadIdx.x * 4 + i * 1024;
        if (d >= D) continue;
        const RowMod m = mod(i, d);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf((v[i][e] - mean) * rstd * m.sc1[e] + m.sh[e]);
        if (orow) *(bf16x4*)(orow + d) = o;
        ov[i] = o;
    }
}

// One block per row: per-token modulation (read beside the row) and the plain norm.
template <int NV>
__global__ __launch_bounds__(256) void norm_mod_kernel(const float* __restrict__ x, long ldx, bf16* __restrict__ out,
                                                       long ldo, int D, float eps, int layer_norm,
                                                       const float* __restrict__ scale_tab,
                                                       const float* __restrict__ shift_tab,
                                                       const float* __restrict__ scale_emb,
                                                       const float* __restrict__ shift_emb, long emb_stride,
                                                       unsigned char* __restrict__ q8, long ldq, float* __restrict__ qscale) {
    __shared__ float red[8];
    const long row = blockIdx.x;
    f32x4 v[NV];
    float s1 = 0.f, s2 = 0.f;
    norm_row_load<NV>(x + row * ldx, D, v, s1, s2);
    block_sum2_256(s1, s2, red);
    float mean;
    const float rstd = norm_row_stats(s1, s2, D, eps, layer_norm, mean);
    const float* se = scale_emb ? scale_emb + row * emb_stride : nullptr;
    const float* he = shift_emb ? shift_emb + row * emb_stride : nullptr;
    bf16x4 ov[NV];
    norm_row_apply<NV>(v, D, mean, rstd, [&](int, int d) { return norm_mod_at(d, true, scale_tab, shift_tab, se, he); },
                       out ? out + row * ldo : nullptr, ov);
    if (q8) row_to_fp8<NV>(ov, D, red, q8 + row * ldq, qscale + row);
}

// Row-invariant modulation (emb_stride == 0: the scalar-sigma case).  A block walks rows blockIdx.x, +gridDim.x, ..
// with the combined (1 + scale) and shift vectors in registers -- read per row, the four 16-KiB tables are 64 KiB of
// L2->L1 traffic beside 24 KiB of data (21.5 -> 18.8 us at 3456 x 4096).  The per-row kernel above stays for per-token
// modulation and for the plain norm, where more blocks in flight matter more (28.5 vs 32.5 us, 14.0 vs 14.5).
template <int NV>
__global__ __launch_bounds__(256) void norm_mod_shared_kernel(const float* __restrict__ x, long ldx, bf16* __restrict__ out,
                                                              long ldo, int rows, int D, float eps, int layer_norm,
                                                              const float* __restrict__ scale_tab,
                                                              const float* __restrict__ shift_tab,
                                                              const float* __restrict__ scale_emb,
                                                              const float* __restrict__ shift_emb,
                                                              unsigned char* __restrict__ q8, long ldq, float* __restrict__ qscale) {
    __shared__ float red[8];
    RowMod m[NV];
    norm_mod_rows<NV>(D, scale_tab, shift_tab, scale_emb, shift_emb, m);
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        f32x4 v[NV];
        float s1 = 0.f, s2 = 0.f;
        norm_row_load<NV>(x + row * ldx, D, v, s1, s2);
        block_sum2_256(s1, s2, red);
        float mean;
        const float rstd = norm_row_stats(s1, s2, D, eps, layer_norm, mean);
        bf16x4 ov[NV];
        norm_row_apply<NV>(v, D, mean, rstd, [&](int i, int) { return m[i]; }, out ? out + row * ldo : nullptr, ov);
        if (q8) row_to_fp8<NV>(ov, D, red, q8 + row * ldq, qscale + row);
    }
}

// Two modulations of ONE normalised row (row-invariant tables): out_g = norm(x) * (1 + scale_g) + shift_g, g = 0, 1.  The AudioVideo block's
// cross-modal attention reads the SAME pre-update RMS-normalised stream twice (transformer.py:556-620: the a2v and the v2a scale / shift rows),
// which two norm_mod launches re-read and re-reduced (round 4: one read of x, one reduction, two stores).
struct NormMod2Tabs {
    const float* scale_tab[2];
    const float* shift_tab[2];
    const float* scale_emb[2];
    const float* shift_emb[2];
};
template <int NV>
__global__ __launch_bounds__(256) void norm_mod_shared2_kernel(const float* __restrict__ x, long ldx, bf16* __restrict__ out0, bf16* __restrict__ out1,
                                                               long ldo, int rows, int D, float eps, NormMod2Tabs t) {
    __shared__ float red[8];
    RowMod m[2][NV];
#pragma unroll
    for (int g = 0; g < 2; ++g) norm_mod_rows<NV>(D, t.scale_tab[g], t.shift_tab[g], t.scale_emb[g], t.shift_emb[g], m[g]);
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        f32x4 v[NV];
        float s1 = 0.f, s2 = 0.f;       // RMS only: s1 rides through the two-value reduction as a zero
        norm_row_load<NV, false>(x + row * ldx, D, v, s1, s2);
        block_sum2_256(s1, s2, red);
        float mean;
        const float rstd = norm_row_stats(s1, s2, D, eps, 0, mean);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            bf16x4 ov[NV];
            norm_row_apply<NV>(v, D, mean, rstd, [&](int i, int) { return m[g][i]; }, (g ? out1 : out0) + row * ldo, ov);
        }
    }
}

struct QKSegs {
    int off[2];
    const float* w[2];
};

// One block per row, D/2 <= 2048 rotation pairs: thread t owns pairs [8t, 8t+8) of EVERY segment
// (q and k share the cos/sin row), everything register-resident, one read + one write per element.
template <int NSEG>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(bf16* __restrict__ buf, long ld, int rows, int D, int head_dim,
                                                          QKSegs segs, float eps, const float* __restrict__ cosp,
                                                          const float* __restrict__ sinp) {
    __shared__ float red[8];
    const int half = head_dim >> 1;
    const int p0 = threadIdx.x * 8;
    const bool act = p0 < D / 2;
    const int ia = act ? (p0 / half) * head_dim + (p0 % half) : 0;
    const int ib = ia + half;
    // the norm weights do not depend on the row: once per block, in registers (a block walks rows blockIdx.x, +gridDim.x, ..)
    float wa[NSEG][8], wb[NSEG][8];
#pragma unroll
    for (int g = 0; g < NSEG; ++g) {
        const float* wt = segs.w[g];
        const f32x4 a0 = *(const f32x4*)(wt + ia), a1 = *(const f32x4*)(wt + ia + 4);
        const f32x4 b0 = *(const f32x4*)(wt + ib), b1 = *(const f32x4*)(wt + ib + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wa[g][e] = a0[e];
            wa[g][4 + e] = a1[e];
            wb[g][e] = b0[e];
            wb[g][4 + e] = b1[e];
        }
    }
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
        bf16x8 va[NSEG], vb[NSEG];
        float ss[2] = {0.f, 0.f};
#pragma unroll
        for (int g = 0; g < NSEG; ++g) {
            bf16* xr = buf + row * ld + segs.off[g];
            if (act) {
                va[g] = *(const bf16x8*)(xr + ia);
                vb[g] = *(const bf16x8*)(xr + ib);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = bf2f(va[g][e]), b = bf2f(vb[g][e]);
                    ss[g] += a * a + b * b;
                }
            }
        }
        block_sum2_256(ss[0], ss[1], red);
        if (!act) continue;
        f32x4 c4[2], s4[2];
        if (cosp) {
            c4[0] = *(const f32x4*)(cosp + row * (D / 2) + p0);
            c4[1] = *(const f32x4*)(cosp + row * (D / 2) + p0 + 4);
            s4[0] = *(const f32x4*)(sinp + row * (D / 2) + p0);
            s4[1] = *(const f32x4*)(sinp + row * (D / 2) + p0 + 4);
        }
#pragma unroll
        for (int g = 0; g < NSEG; ++g) {
            bf16* xr = buf + row * ld + segs.off[g];
            const float rstd = rsqrtf(ss[g] / (float)D + eps);
            bf16x8 oa, ob;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = bf2f(va[g][e]) * rstd * wa[g][e];
                const float b = bf2f(vb[g][e]) * rstd * wb[g][e];
                if (cosp) {
                    const float c = e < 4 ? c4[0][e & 3] : c4[1][e & 3];
                    const float sn = e < 4 ? s4[0][e & 3] : s4[1][e & 3];
                    oa[e] = f2bf(a * c - b * sn);
                    ob[e] = f2bf(b * c + a * sn);
                } else {
                    oa[e] = f2bf(a);
                    ob[e] = f2bf(b);
                }
            }
            *(bf16x8*)(xr + ia) = oa;
            *(bf16x8*)(xr + ib) = ob;
        }
    }
}

__global__ void ctx_mod_kernel(const bf16* __restrict__ ctx, bf16* __restrict__ out, long n4, int D,
                               const float* __restrict__ scale_tab, const float* __restrict__ shift_tab,
                               const float* __restrict__ scale_emb, const float* __restrict__ shift_emb) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)((i * 4) % D);
        const bf16x4 v = *(const bf16x4*)(ctx + i * 4);
        const f32x4 sc = *(const f32x4*)(scale_tab + d) + *(const f32x4*)(scale_emb + d);
        const f32x4 sh = *(const f32x4*)(shift_tab + d) + *(const f32x4*)(shift_emb + d);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(bf2f(v[e]) * (1.f + sc[e]) + sh[e]);
        *(bf16x4*)(out + i * 4) = o;
    }
}

// Tall-skinny gate-logit GEMM (attention.py:241-243): logits[M][H] = X[M][K] @ Wg[H][K]^T + bg, H <= 32.
// One block per 16 rows; the 4 waves split K and reduce through LDS.  v_mfma_f32_16x16x32_bf16:
// A/B lane l holds row/col l&15, k = 8*(l>>4)..+7; D lane l holds rows 4*(l>>4)+r, col l&15.
__global__ __launch_bounds__(256) void gate_logits_kernel(const bf16* __restrict__ X, long ldx, const bf16* __restrict__ Wg,
                                                          const float* __restrict__ bg, float* __restrict__ out, long ldo,
                                                          int M, int K, int H) {
    __shared__ float part[4][16][33];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int row = min((int)blockIdx.x * 16 + r16, M - 1);
    const int kw = K / 4;                                   // this wave's K range
    const bf16* xp = X + (long)row * ldx + wv * kw + kq * 8;
    const bf16* w0 = Wg + (long)min(r16, H - 1) * K + wv * kw + kq * 8;
    const bf16* w1 = Wg + (long)min(16 + r16, H - 1) * K + wv * kw + kq * 8;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // 216 blocks x 4 waves is 3.4 waves per CU: the kernel is bound by the bytes each wave keeps in flight, so a wave requests DEPTH
    // k-steps (3 x 1 KiB each) before it consumes the first (round 4: DEPTH 4 ran the 28 MB of X at 1.4 TB/s, 20 us at 3456 x 4096)
    constexpr int DEPTH = 16;
    int k = 0;
    for (; k + 32 * DEPTH <= kw; k += 32 * DEPTH) {
        bf16x8 a[DEPTH], b0[DEPTH], b1[DEPTH];
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            a[j] = *(const bf16x8*)(xp + k + 32 * j);
            b0[j] = *(const bf16x8*)(w0 + k + 32 * j);
            b1[j] = *(const bf16x8*)(w1 + k + 32 * j);
        }
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            acc0 = LTX2_MFMA_16x16x32(a[j], b0[j], acc0, 0, 0, 0);
            acc1 = LTX2_MFMA_16x16x32(a[j], b1[j], acc1, 0, 0, 0);
        }
    }
#pragma unroll 4
    for (; k < kw; k += 32) {
        const bf16x8 a = *(const bf16x8*)(xp + k);
        const bf16x8 b0 = *(const bf16x8*)(w0 + k);
        const bf16x8 b1 = *(const bf16x8*)(w1 + k);
        acc0 = LTX2_MFMA_16x16x32(a, b0, acc0, 0, 0, 0);
        acc1 = LTX2_MFMA_16x16x32(a, b1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        part[wv][4 * kq + r][r16] = acc0[r];
        part[wv][4 * kq + r][16 + r16] = acc1[r];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * 32; i += 256) {
        const int rr = i >> 5, cc = i & 31;
        const int grow = blockIdx.x * 16 + rr;
        if (grow < M && cc < H) out[(long)grow * ldo + cc] = part[0][rr][cc] + part[1][rr][cc] + part[2][rr][cc] + part[3][rr][cc] + bg[cc];
    }
}

// The same product for many rows (round 5): the kernel above re-reads the whole 32 x K gate weight (256 KiB at K = 4096) from L2 in every 16-row block -- 55 MB of
// weight traffic beside 28 MB of activations at 3456 x 4096, 14-20 us.  Here a block takes 64 rows x ONE K slice (K / KS columns): the slice of the weight
// (32 x K/KS, 32 KiB at K = 4096 with KS = GATE_LOGIT_PARTS = 8; a 4-slice form measured no faster than the round-4 kernel) is staged in LDS once and shared by the block's four waves (16 rows each); X streams from global memory.  The KS partial
// sums are NOT reduced here: parts[ks][M][H] (fp32, no bias) -- the consumer (the attention kernel's epilogue) adds the KS values and the bias in a fixed order.
template <int KS>
__global__ __launch_bounds__(256) void gate_logits_parts_kernel(const bf16* __restrict__ X, long ldx, const bf16* __restrict__ Wg, float* __restrict__ parts,
                                                                int M, int K, int H) {
    extern __shared__ __attribute__((aligned(16))) char gl_smem[];
    const int Kc = K / KS, ks = blockIdx.y, ROWB = (Kc + 8) * 2;       // padded LDS row: 16 rows x 16 B land on 16 different bank groups
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * 64 + wv * 16;
    const bf16* xp = X + (long)min(row0 + r16, M - 1) * ldx + (long)ks * Kc + kq * 8;
    const char* w0 = gl_smem + r16 * ROWB + kq * 16;
    const char* w1 = gl_smem + (16 + r16) * ROWB + kq * 16;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    constexpr int DEPTH = 16;
    bf16x8 a[DEPTH];
    if (LTX2_GATE_X_FIRST) {
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) a[j] = (32 * j < Kc) ? *(const bf16x8*)(xp + 32 * j) : bf16x8{};
    }
    // stage the weight slice: 32 rows x Kc columns as 16-byte pieces (rows >= H repeat row H - 1: their products are never stored)
    const int pieces_per_row = Kc / 8;
    for (int i = tid; i < 32 * pieces_per_row; i += 256) {
        const int h = i / pieces_per_row, c = i - h * pieces_per_row;
        const bf16x8 v = *(const bf16x8*)(Wg + (long)min(h, H - 1) * K + (long)ks * Kc + c * 8);
        *(bf16x8*)(gl_smem + h * ROWB + c * 16) = v;
    }
    __syncthreads();
    for (int k = 0; k < Kc; k += 32 * DEPTH) {
        if (!LTX2_GATE_X_FIRST || k > 0) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) a[j] = (k + 32 * j < Kc) ? *(const bf16x8*)(xp + k + 32 * j) : bf16x8{};
        }
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            if (k + 32 * j < Kc) {
                const bf16x8 b0 = *(const bf16x8*)(w0 + (k + 32 * j) * 2), b1 = *(const bf16x8*)(w1 + (k + 32 * j) * 2);
                acc0 = LTX2_MFMA_16x16x32(a[j], b0, acc0, 0, 0, 0);
                acc1 = LTX2_MFMA_16x16x32(a[j], b1, acc1, 0, 0, 0);
            }
        }
    }
    float* out = parts + (long)ks * M * H;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * kq + r;
        if (row < M) {
            if (r16 < H) out[(long)row * H + r16] = acc0[r];
            if (16 + r16 < H) out[(long)row * H + 16 + r16] = acc1[r];
        }
    }
}

__global__ void head_gate_kernel(bf16* __restrict__ att, long ld, const float* __restrict__ logits, long ldl, long n8,
                                 int per_row8, int hd) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const long row = i / per_row8;
        const int col = (int)(i - row * per_row8) * 8;
        const float g = 2.f / (1.f + __expf(-logits[row * ldl + col / hd]));
        bf16x8* p = (bf16x8*)(att + row * ld + col);
        bf16x8 v = *p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = f2bf(bf2f(v[e]) * g);
        *p = v;
    }
}

// SPLIT-RoPE tables on the GPU (rope.py:214-328,365-418): cos/sin fp32 [N][half], slot pad + f*n_dims + d, identity
// padding at the FRONT; freq = grid[f] * (2*mid_d/max_pos[d] - 1), mid = (start + end) / 2.  cosf/sinf are the
// accurate (range-reducing) versions: the argument reaches ~1.6e4 rad.
__global__ void rope_tables_kernel(const float* __restrict__ pos, const float* __restrict__ grid, const float* __restrict__ max_pos,
                                   int N, int n_dims, int n_freq, int half, float* __restrict__ cosb, float* __restrict__ sinb) {
    const long total = (long)N * half;
    const int pad = half - n_dims * n_freq;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / half), slot = (int)(i - (long)n * half);
        float c = 1.f, s = 0.f;
        if (slot >= pad) {
            const int j = slot - pad, f = j / n_dims, d = j - f * n_dims;
            const float mid = (pos[((long)d * N + n) * 2] + pos[((long)d * N + n) * 2 + 1]) * 0.5f;
            const float arg = grid[f] * ((mid / max_pos[d]) * 2.f - 1.f);
            c = cosf(arg);
            s = sinf(arg);
        }
        cosb[i] = c;
        sinb[i] = s;
    }
}

__global__ void timestep_sinusoid_kernel(const float* __restrict__ t, long t_stride, float t_scalar, float mult, int T,
                                         int dim, float* __restrict__ of, bf16* __restrict__ ob) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim >> 1;
    if (idx >= T * half) return;
    const int row = idx / half, i = idx - row * half;
    const float freq = __expf(-9.210340371976184f * (float)i / (float)half);   // ln(10000)
    const float arg = (t ? t[row * t_stride] : t_scalar) * mult * freq;
    const float c = cosf(arg), s = sinf(arg);
    if (of) {
        of[(long)row * dim + i] = c;
        of[(long)row * dim + half + i] = s;
    }
    if (ob) {
        ob[(long)row * dim + i] = f2bf(c);
        ob[(long)row * dim + half + i] = f2bf(s);
    }
}

// fp8 e4m3fn (OCP: bias 7, no inf, 0x7f/0xff = NaN) -> fp32, exact (loader/fp8_loader.py:14-51)
// out_bf16[i] = bf16( f32(fp8[i]) * scale )   (weight_converter.py:391-395: fp8 -> f32 * weight_scale -> target dtype)
__global__ void dequant_fp8_kernel(const unsigned char* __restrict__ in, float scale, bf16* __restrict__ out, long n) {
    const long stride = (long)gridDim.x * blockDim.x * 8;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n; i += stride) {
        if (i + 7 < n) {
            const u32x2 w = *(const u32x2*)(in + i);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(e4m3fn_to_f32((w[e >> 2] >> (8 * (e & 3))) & 0xffu) * scale);
            *(bf16x8*)(out + i) = o;
        } else {
            for (long j = i; j < n; ++j) out[j] = f2bf(e4m3fn_to_f32(in[j]) * scale);
        }
    }
}

// Per-row e4m3fn quantiser of the fp8 compute path: one workgroup per row, the arithmetic of fp8_row_scale / pack4_fp8 above.
// The row stays in registers between the two passes (K <= 32768: NIT = 2, 8 or 16 x 16 bytes per thread).
template <int NIT>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const bf16* __restrict__ x, long ldx, int K, unsigned char* __restrict__ out, long ldo,
                                                             float* __restrict__ scale_out) {
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const bf16* xr = x + (long)row * ldx;
    bf16x8 v[NIT];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int k = (i * 256 + tid) * 8;
        if (k < K) {
            v[i] = *(const bf16x8*)(xr + k);
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(v[i][e])));
        }
    }
    amax = block_max_256(amax, red);
    float inv;
    const float scale = fp8_row_scale(amax, inv);
    if (tid == 0) scale_out[row] = scale;
    unsigned char* orow = out + (long)row * ldo;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int k = (i * 256 + tid) * 8;
        if (k < K) {
            const u32x2 c = {pack4_fp8(bf2f(v[i][0]), bf2f(v[i][1]), bf2f(v[i][2]), bf2f(v[i][3]), inv),
                             pack4_fp8(bf2f(v[i][4]), bf2f(v[i][5]), bf2f(v[i][6]), bf2f(v[i][7]), inv)};
            *(u32x2*)(orow + k) = c;
        }
    }
}

// key mask fp32 [S] (non-zero = attend) -> one 64-bit word per 64 keys (bit i of word t = key 64 t + i); keys >= S read as masked
__global__ void keymask_words_kernel(const float* __restrict__ mask, int S, unsigned long long* __restrict__ words, int nwords) {
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= nwords) return;
    const int k = w * 64 + lane;
    const unsigned long long b = __ballot(k < S && mask[k] != 0.f);
    if (lane == 0) words[w] = b;
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ in, bf16* __restrict__ out, long n) {
    const long stride = (long)gridDim.x * blockDim.x * 4;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            const float4 v = *(const float4*)(in + i);
            bf16x4 o = {f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)};
            *(bf16x4*)(out + i) = o;
        } else {
            for (long j = i; j < n; ++j) out[j] = f2bf(in[j]);
        }
    }
}

// grid of a row-walking kernel: at most `blocks` blocks, every block with the same number of rows to walk (the last may fall short)
int row_walk_grid(int rows, int blocks) {
    const int per_block = (rows + blocks - 1) / blocks;
    return (rows + per_block - 1) / per_block;
}

}  // namespace

// the norm kernels hold a row of D <= 1024 * NV floats in registers: NV = 4 up to D = 4096, 8 up to the launchers' limit of 8192
#define NORM_LAUNCH(kernel, grid, ...)                                                                       \
    do {                                                                                                     \
        if (D <= 4096) hipLaunchKernelGGL((kernel<4>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__);       \
        else hipLaunchKernelGGL((kernel<8>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__);                 \
    } while (0)

int norm_mod_launch(const float* x, long ldx, bf16* out, long ldo, int rows, int D, float eps, int layer_norm,
                    const float* scale_tab, const float* shift_tab, const float* scale_emb, const float* shift_emb,
                    long emb_stride, hipStream_t stream, unsigned char* q8, long ldq, float* qscale) {
    LTX2_CHECK_ARG(rows > 0 && D > 0 && D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0, "norm_mod: D, ldx, ldo must be multiples of 4");
    LTX2_CHECK_ARG((out || q8) && (!q8 || (qscale && ldq % 4 == 0)), "norm_mod: no output / fp8 output without a scale vector");
    LTX2_CHECK_ARG(D <= 8192 && emb_stride % 4 == 0, "norm_mod: D=%d exceeds 8192 or emb_stride not a multiple of 4", D);
    const bool shared_mod = emb_stride == 0 && (scale_tab || shift_tab || scale_emb || shift_emb) && rows > 1024;
    if (shared_mod)
        NORM_LAUNCH(norm_mod_shared_kernel, row_walk_grid(rows, LTX2_NORM_BLOCKS), x, ldx, out, ldo, rows, D, eps, layer_norm, scale_tab,
                    shift_tab, scale_emb, shift_emb, q8, ldq, qscale);
    else
        NORM_LAUNCH(norm_mod_kernel, rows, x, ldx, out, ldo, D, eps, layer_norm, scale_tab, shift_tab, scale_emb, shift_emb, emb_stride, q8,
                    ldq, qscale);
    LTX2_CHECK_LAUNCH("norm_mod_kernel");
    return LTX2_OK;
}

// comb[l][i] = tab[l][i] + emb[i]: the AdaLN rows of EVERY layer for this step in one launch (row-invariant modulation: one sigma per step).  The norm
// kernels then read two vectors per row set instead of four and the gated-residual GEMMs take their gate as a table (no per-row gate loads).
static __global__ __launch_bounds__(256) void adaln_combine_kernel(const float* __restrict__ tab, const float* __restrict__ emb, float* __restrict__ out, long n, long total) {
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (long)gridDim.x * 1024) {
        const f32x4 a = *(const f32x4*)(tab + i), e = *(const f32x4*)(emb + i % n);
        *(f32x4*)(out + i) = a + e;
    }
}
int adaln_combine_launch(const float* tab, const float* emb, float* out, int layers, long n, hipStream_t stream) {
    LTX2_CHECK_ARG(tab && emb && out && layers > 0 && n > 0 && n % 4 == 0, "adaln_combine: bad operand");
    const long total = (long)layers * n;
    hipLaunchKernelGGL(adaln_combine_kernel, dim3(grid_for(total / 4, 256, 2048)), dim3(256), 0, stream, tab, emb, out, n, total);
    LTX2_CHECK_LAUNCH("adaln_combine_kernel");
    return LTX2_OK;
}

int norm_mod2_launch(const float* x, long ldx, bf16* out0, bf16* out1, long ldo, int rows, int D, float eps, const float* const* scale_tab,
                     const float* const* shift_tab, const float* const* scale_emb, const float* const* shift_emb, hipStream_t stream) {
    // the two norm_mod launches this replaced took D <= 8192
    LTX2_CHECK_ARG(x && out0 && out1 && rows > 0 && D > 0 && D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && D <= 8192, "norm_mod2: bad operand (D <= 8192, multiples of 4)");
    NormMod2Tabs t{};
    for (int g = 0; g < 2; ++g) {
        t.scale_tab[g] = scale_tab[g];
        t.shift_tab[g] = shift_tab[g];
        t.scale_emb[g] = scale_emb[g];
        t.shift_emb[g] = shift_emb[g];
    }
    NORM_LAUNCH(norm_mod_shared2_kernel, row_walk_grid(rows, LTX2_NORM_BLOCKS), x, ldx, out0, out1, ldo, rows, D, eps, t);
    LTX2_CHECK_LAUNCH("norm_mod_shared2_kernel");
    return LTX2_OK;
}
#undef NORM_LAUNCH

int qknorm_rope_launch(bf16* buf, long ld, int rows, int D, int head_dim, int nseg, const int* seg_off,
                       const float* const* weights, float eps, const float* cos, const float* sin, hipStream_t stream) {
    LTX2_CHECK_ARG(nseg >= 1 && nseg <= 2, "qknorm_rope: nseg must be 1 or 2");
    LTX2_CHECK_ARG(head_dim % 16 == 0 && D % head_dim == 0 && ld % 8 == 0, "qknorm_rope: head_dim %% 16, D %% head_dim, ld %% 8");
    LTX2_CHECK_ARG((cos == nullptr) == (sin == nullptr), "qknorm_rope: cos and sin must both be set or both null");
    QKSegs s{};
    for (int i = 0; i < nseg; ++i) {
        LTX2_CHECK_ARG(seg_off[i] % 8 == 0 && weights[i], "qknorm_rope: bad segment");
        s.off[i] = seg_off[i];
        s.w[i] = weights[i];
    }
    LTX2_CHECK_ARG(D <= 4096, "qknorm_rope: inner dim %d exceeds 4096", D);
    const int grid = row_walk_grid(rows, LTX2_QK_BLOCKS);
    if (nseg == 2)
        hipLaunchKernelGGL((qknorm_rope_kernel<2>), dim3(grid), dim3(256), 0, stream, buf, ld, rows, D, head_dim, s, eps, cos, sin);
    else
        hipLaunchKernelGGL((qknorm_rope_kernel<1>), dim3(grid), dim3(256), 0, stream, buf, ld, rows, D, head_dim, s, eps, cos, sin);
    LTX2_CHECK_LAUNCH("qknorm_rope_kernel");
    return LTX2_OK;
}

int ctx_mod_launch(const bf16* ctx, bf16* out, int rows, int D, const float* scale_tab, const float* shift_tab,
                   const float* scale_emb, const float* shift_emb, hipStream_t stream) {
    LTX2_CHECK_ARG(rows > 0 && D > 0 && D % 4 == 0, "ctx_mod: D must be a multiple of 4");
    LTX2_CHECK_ARG(scale_tab && shift_tab && scale_emb && shift_emb, "ctx_mod: null table");
    const long n4 = (long)rows * D / 4;
    hipLaunchKernelGGL(ctx_mod_kernel, dim3(grid_for(n4, 256, 4096)), dim3(256), 0, stream, ctx, out, n4, D, scale_tab, shift_tab, scale_emb, shift_emb);
    LTX2_CHECK_LAUNCH("ctx_mod_kernel");
    return LTX2_OK;
}

int gate_logits_launch(const bf16* X, long ldx, const bf16* Wg, const float* bg, float* out, long ldo, int M, int K, int H,
                       hipStream_t stream) {
    LTX2_CHECK_ARG(M > 0 && H > 0 && H <= 32 && K % 128 == 0 && ldx % 8 == 0, "gate_logits: need H <= 32, K %% 128 == 0, ldx %% 8 == 0");
    hipLaunchKernelGGL(gate_logits_kernel, dim3((M + 15) / 16), dim3(256), 0, stream, X, ldx, Wg, bg, out, ldo, M, K, H);
    LTX2_CHECK_LAUNCH("gate_logits_kernel");
    return LTX2_OK;
}

int gate_logits_parts_launch(const bf16* X, long ldx, const bf16* Wg, float* parts, int M, int K, int H, hipStream_t stream) {
    LTX2_CHECK_ARG(M > 0 && H > 0 && H <= 32 && K % (GATE_LOGIT_PARTS * 32) == 0 && ldx % 8 == 0, "gate_logits_parts: need H <= 32, K %% %d == 0, ldx %% 8 == 0", GATE_LOGIT_PARTS * 32);
    const int lds = 32 * (K / GATE_LOGIT_PARTS + 8) * 2;
    LTX2_CHECK_ARG(lds <= 160 * 1024, "gate_logits_parts: K=%d too wide for the LDS-resident weight slice", K);
    static PerDeviceOnce once;
    if (once.first()) (void)hipFuncSetAttribute((const void*)gate_logits_parts_kernel<GATE_LOGIT_PARTS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(gate_logits_parts_kernel<GATE_LOGIT_PARTS>, dim3((M + 63) / 64, GATE_LOGIT_PARTS), dim3(256), lds, stream, X, ldx, Wg, parts, M, K, H);
    LTX2_CHECK_LAUNCH("gate_logits_parts_kernel");
    return LTX2_OK;
}

int head_gate_launch(bf16* att, long ld, const float* logits, long ldl, int rows, int H, int hd, hipStream_t stream) {
    LTX2_CHECK_ARG(rows > 0 && H > 0 && hd > 0 && hd % 8 == 0 && ld % 8 == 0, "head_gate: head_dim and ld must be multiples of 8");
    const int per_row8 = H * hd / 8;
    const long n8 = (long)rows * per_row8;
    hipLaunchKernelGGL(head_gate_kernel, dim3(grid_for(n8, 256, 4096)), dim3(256), 0, stream, att, ld, logits, ldl, n8, per_row8, hd);
    LTX2_CHECK_LAUNCH("head_gate_kernel");
    return LTX2_OK;
}

int rope_tables_launch(const float* pos, const float* grid, const float* max_pos, int N, int n_dims, int n_freq, int half,
                       float* cosb, float* sinb, hipStream_t stream) {
    LTX2_CHECK_ARG(pos && grid && max_pos && cosb && sinb && N > 0, "rope_tables: null operand");
    LTX2_CHECK_ARG(n_dims >= 1 && n_freq >= 1 && n_dims * n_freq <= half, "rope_tables: n_dims*n_freq=%d exceeds D/2=%d", n_dims * n_freq, half);
    hipLaunchKernelGGL(rope_tables_kernel, dim3(grid_for((long)N * half, 256, 8192)), dim3(256), 0, stream, pos, grid, max_pos, N, n_dims,
                       n_freq, half, cosb, sinb);
    LTX2_CHECK_LAUNCH("rope_tables_kernel");
    return LTX2_OK;
}

int timestep_sinusoid_launch(const float* t, long t_stride, float t_scalar, float mult, int T, int dim, float* out_f32,
                             bf16* out_bf16, hipStream_t stream) {
    LTX2_CHECK_ARG(T > 0 && dim % 2 == 0, "timestep_sinusoid: bad shape");
    const int n = T * (dim / 2);
    hipLaunchKernelGGL(timestep_sinusoid_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, t, t_stride, t_scalar, mult, T,
                       dim, out_f32, out_bf16);
    LTX2_CHECK_LAUNCH("timestep_sinusoid_kernel");
    return LTX2_OK;
}

int dequant_fp8_launch(const unsigned char* in, float scale, bf16* out, long n, hipStream_t stream) {
    LTX2_CHECK_ARG(in && out && n > 0, "dequant_fp8: bad argument");
    LTX2_CHECK_ARG((((uintptr_t)in) & 7) == 0 && (((uintptr_t)out) & 15) == 0, "dequant_fp8: pointers must be 8/16-byte aligned");
    hipLaunchKernelGGL(dequant_fp8_kernel, dim3(grid_for(n / 8, 256, 8192)), dim3(256), 0, stream, in, scale, out, n);
    LTX2_CHECK_LAUNCH("dequant_fp8_kernel");
    return LTX2_OK;
}

int quant_rows_fp8_launch(const bf16* x, long ldx, int rows, int K, unsigned char* out, long ldo, float* scale, hipStream_t stream) {
    LTX2_CHECK_ARG(rows > 0 && K > 0 && K % 8 == 0 && K <= 16 * 2048 && ldx % 8 == 0 && ldo % 8 == 0, "quant_rows_fp8: rows=%d K=%d (K %% 8 == 0, K <= 32768, 16-byte rows)", rows, K);
    const int nit = (K + 2047) / 2048;
    if (nit <= 2)
        hipLaunchKernelGGL(quant_rows_fp8_kernel<2>, dim3(rows), dim3(256), 0, stream, x, ldx, K, out, ldo, scale);
    else if (nit <= 8)
        hipLaunchKernelGGL(quant_rows_fp8_kernel<8>, dim3(rows), dim3(256), 0, stream, x, ldx, K, out, ldo, scale);
    else
        hipLaunchKernelGGL(quant_rows_fp8_kernel<16>, dim3(rows), dim3(256), 0, stream, x, ldx, K, out, ldo, scale);
    LTX2_CHECK_LAUNCH("quant_rows_fp8_kernel");
    return LTX2_OK;
}

int keymask_words_launch(const float* mask, int S, unsigned long long* words, int nwords, hipStream_t stream) {
    LTX2_CHECK_ARG(mask && words && S > 0 && nwords * 64 >= S, "keymask_words: bad argument");
    hipLaunchKernelGGL(keymask_words_kernel, dim3((nwords + 3) / 4), dim3(256), 0, stream, mask, S, words, nwords);
    LTX2_CHECK_LAUNCH("keymask_words_kernel");
    return LTX2_OK;
}

int cast_f32_bf16_launch(const float* in, bf16* out, long n, hipStream_t stream) {
    LTX2_CHECK_ARG(n > 0, "cast: empty");
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, stream, in, out, n);
    LTX2_CHECK_LAUNCH("cast_f32_bf16_kernel");
    return LTX2_OK;
}
