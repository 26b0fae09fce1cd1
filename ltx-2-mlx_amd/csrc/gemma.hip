// Gemma-3 12B prefill kernels for gfx950 / CDNA4 (the text encoder, model/text_encoder/gemma3.py).  Its GEMMs run on ltx2_gemm_bf16;
// what is Gemma-specific lives here, in a translation unit of its own so that no pre-existing kernel's code changes.
//
//  * gemma_attn_kernel: causal / sliding-window / non-causal GQA flash attention at head_dim 256 (reference gemma3.py:186-241, masks
//    :362-382).  Workgroup = 4 wave64 = 64 query rows of one query head; each wave owns 16 rows.  KV tile = 64 keys: K [64][256] and
//    V^T [256][64] take 64 KiB of data per stage (70.6 KiB with the bank-spreading row pads), so ONE LDS stage per workgroup and two
//    workgroups per CU (141 KiB of the 160 KiB); the next tile is fetched into registers while the current one is computed, and the
//    workgroup's SIMD partner covers the LDS fill.  v_mfma_f32_16x16x32 in the "swapped" orientation (S^T = K Q^T, O^T = V^T P^T) so that
//    a query's softmax statistics sit in the four lanes {c, c+16, c+32, c+48}; P stays in registers: V^T is written to LDS with its keys
//    permuted inside each 32-key block (ga_vpos) so that the P accumulators ARE the B fragment of the P.V product.
//    Tiles wholly above the diagonal or wholly outside the window are never visited (workgroup range) or skipped per wave; scores are
//    masked element by element only on edge tiles.  A row that sees no key writes zeros (l == 0), never NaN.
//  * gemma_qknorm_rope_kernel: per-head q / k RMSNorm(1 + w) + rotate-half RoPE, in place on the fused QKV rows (:117-138, :206-224).
//  * gemma_resid_norm_kernel: residual add of a post-norm'ed sublayer output, then the next pre-norm, in one row pass (:258-293);
//    writes the fp32 residual straight into the [49][T][D] hidden-state buffer.
//  * gemma_gated_act_kernel: act(gate) * up of the fused gate|up GEMM (:244-255), SiLU (the reference) or tanh-GELU (the checkpoints).
//  * gemma_embed_kernel: embedding gather * sqrt(hidden) (:312, :352).
//  * gemma_features_rms_kernel: the [49][T][D] hidden states -> the LTX-2.3 feature extractor's per-token RMS-normalised, layer-major
//    16-bit GEMM operand [T][49 * D] in one pass (feature_extractor.py:160-181).
#include "gemma.h"

namespace {

constexpr int GA_HD = 256;                              // head_dim
constexpr int GA_KVB = 64;                              // keys per tile
constexpr int GA_QB = 64;                               // query rows per workgroup (4 waves x 16)
constexpr int GA_KLD = GA_HD + 8;                       // K tile row: 528 B (16 B pad spreads the 16 rows of a fragment read over the banks)
constexpr int GA_VLD = GA_KVB + 8;                      // V^T tile row: 144 B
constexpr int GA_K_BYTES = GA_KVB * GA_KLD * 2;         // 33 792
constexpr int GA_V_BYTES = GA_HD * GA_VLD * 2;          // 36 864
constexpr int GA_LDS = GA_K_BYTES + GA_V_BYTES;         // 70 656: two workgroups per CU

struct GemmaAttnParams {
    const bf16* Q;
    const bf16* K;
    const bf16* V;
    bf16* O;
    long ldq, ldk, ldv, ldo;
    int Tq, Tkv, ratio, causal, window;
    float scale_log2e;
};

// position of key kl (< 64) inside the V^T tile row: in each 32-key block, key 16h + 4g + i sits at 8g + 4h + i -- the k-slot at which
// the P.V MFMA's B fragment (lane group g: elements 0-3 = the S^T accumulators of key block 2kk, 4-7 = of key block 2kk+1) holds it
__device__ __forceinline__ int ga_vpos(int kl) {
    const int r = kl & 31;
    return (kl & 32) + 8 * ((r >> 2) & 3) + 4 * (r >> 4) + (r & 3);
}

__device__ __forceinline__ unsigned ga_half(const u32x4& v, int e) { return e & 1 ? v[e >> 1] >> 16 : v[e >> 1] & 0xffffu; }

__global__ __launch_bounds__(256, 2) void gemma_attn_kernel(const GemmaAttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Ks = (bf16*)smem;
    bf16* Vt = (bf16*)(smem + GA_K_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int head = blockIdx.y, kvh = head / p.ratio;            // mx.repeat interleaves: query head h reads kv head h / ratio (:228-229)
    const int qb0 = blockIdx.x * GA_QB;
    const int qb1 = min(qb0 + GA_QB, p.Tq);
    const int q0w = qb0 + wv * 16;
    const int qi = q0w + c;
    const bf16* Kg = p.K + (long)kvh * GA_HD;
    const bf16* Vg = p.V + (long)kvh * GA_HD;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    // key tiles this workgroup can see at all: causal ends at the last query's diagonal, the window starts at the first query's edge
    const int ntile = (p.Tkv + GA_KVB - 1) / GA_KVB;
    int kt0 = 0, kt1 = ntile;
    if (p.causal) {
        kt1 = min(ntile, (qb1 - 1) / GA_KVB + 1);
        if (p.window > 0) kt0 = max(0, qb0 - p.window + 1) / GA_KVB;
    }

    bf16x8 qf[GA_HD / 32];
    {
        const bool ok = qi < p.Tq;
        const bf16* qrow = p.Q + (long)(ok ? qi : 0) * p.ldq + (long)head * GA_HD + 8 * g;
#pragma unroll
        for (int ks = 0; ks < GA_HD / 32; ++ks) qf[ks] = as_bf16x8(ok ? *(const u32x4*)(qrow + 32 * ks) : zero);
    }

    // the next tile travels in registers while the current one is computed: K as 8 x 16 B per thread (rows of 512 B, coalesced), V as
    // 4 key pairs x 2 x 16 B (a pair lands in one 32-bit LDS word of the transposed tile)
    u32x4 kr[8], vr[4][2];
    auto fetch = [&](int kt) {
        const int k0 = kt * GA_KVB;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = i * 256 + tid, key = k0 + (ch >> 5);
            kr[i] = key < p.Tkv ? *(const u32x4*)(Kg + (long)key * p.ldk + (ch & 31) * 8) : zero;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = i * 256 + tid, key = k0 + 2 * (u & 31);
            const bf16* src = Vg + (long)key * p.ldv + (u >> 5) * 8;
            vr[i][0] = key < p.Tkv ? *(const u32x4*)src : zero;
            vr[i][1] = key + 1 < p.Tkv ? *(const u32x4*)(src + p.ldv) : zero;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int ch = i * 256 + tid;
            *(u32x4*)(Ks + (ch >> 5) * GA_KLD + (ch & 31) * 8) = kr[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = i * 256 + tid, pos = ga_vpos(2 * (u & 31)), d0 = (u >> 5) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(unsigned*)(Vt + (d0 + e) * GA_VLD + pos) = ga_half(vr[i][0], e) | (ga_half(vr[i][1], e) << 16);
        }
    };

    f32x4 o[GA_HD / 16];
#pragma unroll
    for (int db = 0; db < GA_HD / 16; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1.0e30f, l = 0.f;          // finite start: a tile whose scores are all masked (-inf) leaves alpha = 1 and P = 0
    const float sl2 = p.scale_log2e;

    if (kt0 < kt1) fetch(kt0);
    for (int kt = kt0; kt < kt1; ++kt) {
        const int k0 = kt * GA_KVB;
        __syncthreads();                  // every wave is done with the previous tile
        stash();
        __syncthreads();
        if (kt + 1 < kt1) fetch(kt + 1);

        // per wave (uniform): a tile that none of this wave's 16 rows can see is not computed
        bool skip = q0w >= p.Tq;
        bool edge = k0 + GA_KVB > p.Tkv;
        if (p.causal) {
            skip = skip || k0 > q0w + 15 || (p.window > 0 && q0w - (k0 + GA_KVB - 1) >= p.window);
            edge = edge || k0 + GA_KVB - 1 > q0w || (p.window > 0 && q0w + 15 - k0 >= p.window);
        }
        if (skip) continue;

        f32x4 s[4];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < GA_HD / 32; ++ks) {
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                const u32x4 kf = *(const u32x4*)(Ks + (16 * kb + c) * GA_KLD + 32 * ks + 8 * g);
                s[kb] = LTX2_MFMA_16x16x32(as_bf16x8(kf), qf[ks], s[kb], 0, 0, 0);
            }
        }
        // S^T[kb][i] = score of key k0 + 16 kb + 4 g + i for query qi
        float mt = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = s[kb][i] * sl2;
                if (edge) {
                    const int kj = k0 + 16 * kb + 4 * g + i;
                    bool ok = kj < p.Tkv;
                    if (p.causal) ok = ok && kj <= qi && (p.window <= 0 || qi - kj < p.window);
                    v = ok ? v : -INFINITY;
                }
                s[kb][i] = v;
                mt = fmaxf(mt, v);
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float alpha = exp2f(m - mn);
        m = mn;
        float ls = 0.f;
        bf16x8 pf[2];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float pv = exp2f(s[kb][i] - mn);
                ls += pv;
                pf[kb >> 1][(kb & 1) * 4 + i] = f2bf(pv);
            }
        }
        l = l * alpha + ls;
#pragma unroll
        for (int db = 0; db < GA_HD / 16; ++db) o[db] *= alpha;
#pragma unroll
        for (int db = 0; db < GA_HD / 16; ++db) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const u32x4 vf = *(const u32x4*)(Vt + (16 * db + c) * GA_VLD + 32 * kk + 8 * g);
                o[db] = LTX2_MFMA_16x16x32(as_bf16x8(vf), pf[kk], o[db], 0, 0, 0);
            }
        }
    }

    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    if (qi < p.Tq) {
        bf16* orow = p.O + (long)qi * p.ldo + (long)head * GA_HD + 4 * g;
#pragma unroll
        for (int db = 0; db < GA_HD / 16; ++db) {
            const bf16x4 w = {f2bf(o[db][0] * inv), f2bf(o[db][1] * inv), f2bf(o[db][2] * inv), f2bf(o[db][3] * inv)};
            *(bf16x4*)(orow + 16 * db) = w;
        }
    }
}

// one wave per (row, head); lane holds elements 4 lane .. 4 lane + 3, so the rotate-half partner of lane L is lane L ^ 32
__global__ __launch_bounds__(256) void gemma_qknorm_rope_kernel(bf16* __restrict__ qkv, long ld, int rows, int q_heads, int nheads,
                                                                const float* __restrict__ q_w, const float* __restrict__ k_w, float eps,
                                                                const float* __restrict__ cos, const float* __restrict__ sin) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)rows * nheads) return;
    const int row = (int)(item / nheads), h = (int)(item % nheads);
    bf16* x = qkv + (long)row * ld + (long)h * GA_HD + 4 * lane;
    const float* w = (h < q_heads ? q_w : k_w) + 4 * lane;
    const bf16x4 xv = *(const bf16x4*)x;
    float y[4], ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        y[e] = bf2f(xv[e]);
        ss += y[e] * y[e];
    }
    const float r = rsqrtf(wave_sum(ss) * (1.0f / GA_HD) + eps);
    const int j = (4 * lane) & (GA_HD / 2 - 1);
    const float* cr = cos + (long)row * (GA_HD / 2) + j;
    const float* sr = sin + (long)row * (GA_HD / 2) + j;
    bf16x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        y[e] = y[e] * r * (1.0f + w[e]);
        const float other = __shfl_xor(y[e], 32);
        const float rot = lane < 32 ? y[e] * cr[e] - other * sr[e] : y[e] * cr[e] + other * sr[e];
        out[e] = f2bf(rot);
    }
    *(bf16x4*)x = out;
}

__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

constexpr int GR_NV = 8;          // float4 per thread: D <= 8192

__global__ __launch_bounds__(256) void gemma_resid_norm_kernel(const float* __restrict__ x_in, long ldx, const bf16* __restrict__ y, long ldy,
                                                               const float* __restrict__ w_post, const float* __restrict__ w_next,
                                                               float* __restrict__ x_out, long ldxo, bf16* __restrict__ h_out, long ldh,
                                                               float* __restrict__ hf_out, long ldhf, int D, float eps) {
    __shared__ float red[2][4];
    const int row = blockIdx.x, tid = threadIdx.x, n4 = D / 4;
    float4 xv[GR_NV];
    const float4* xr = (const float4*)(x_in + (long)row * ldx);
    if (y) {
        const bf16* yr = y + (long)row * ldy;
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < GR_NV; ++k) {
            const int i = tid + 256 * k;
            if (i < n4) {
                const bf16x4 v = *(const bf16x4*)(yr + 4 * i);
                xv[k] = make_float4(bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3]));
                ss += xv[k].x * xv[k].x + xv[k].y * xv[k].y + xv[k].z * xv[k].z + xv[k].w * xv[k].w;
            }
        }
        const float ry = rsqrtf(block_sum256(ss, red[0]) / (float)D + eps);
#pragma unroll
        for (int k = 0; k < GR_NV; ++k) {
            const int i = tid + 256 * k;
            if (i < n4) {
                const float4 a = xr[i], wp = ((const float4*)w_post)[i];
                xv[k] = make_float4(a.x + xv[k].x * ry * (1.0f + wp.x), a.y + xv[k].y * ry * (1.0f + wp.y),
                                    a.z + xv[k].z * ry * (1.0f + wp.z), a.w + xv[k].w * ry * (1.0f + wp.w));
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < GR_NV; ++k) {
            const int i = tid + 256 * k;
            if (i < n4) xv[k] = xr[i];
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < GR_NV; ++k) {
        const int i = tid + 256 * k;
        if (i < n4) ss += xv[k].x * xv[k].x + xv[k].y * xv[k].y + xv[k].z * xv[k].z + xv[k].w * xv[k].w;
    }
    const float rx = rsqrtf(block_sum256(ss, red[1]) / (float)D + eps);
#pragma unroll
    for (int k = 0; k < GR_NV; ++k) {
        const int i = tid + 256 * k;
        if (i >= n4) continue;
        if (x_out) ((float4*)(x_out + (long)row * ldxo))[i] = xv[k];
        if (h_out || hf_out) {
            const float4 wn = ((const float4*)w_next)[i];
            const float4 n = make_float4(xv[k].x * rx * (1.0f + wn.x), xv[k].y * rx * (1.0f + wn.y), xv[k].z * rx * (1.0f + wn.z),
                                         xv[k].w * rx * (1.0f + wn.w));
            if (h_out) {
                const bf16x4 b = {f2bf(n.x), f2bf(n.y), f2bf(n.z), f2bf(n.w)};
                *(bf16x4*)(h_out + (long)row * ldh + 4 * i) = b;
            }
            if (hf_out) ((float4*)(hf_out + (long)row * ldhf))[i] = n;
        }
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void gemma_gated_act_kernel(const bf16* __restrict__ gu, long ldgu, bf16* __restrict__ out, long ldo, int rows,
                                                              int inter) {
    const int n8 = inter / 8;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)rows * n8) return;
    const int row = (int)(idx / n8), i = (int)(idx % n8) * 8;
    const bf16* gr = gu + (long)row * ldgu + i;
    const bf16x8 gv = *(const bf16x8*)gr, uv = *(const bf16x8*)(gr + inter);
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float a = bf2f(gv[e]);
        r[e] = f2bf((ACT == 0 ? silu_f(a) : gelu_tanh(a)) * bf2f(uv[e]));
    }
    *(bf16x8*)(out + (long)row * ldo + i) = r;
}

__global__ __launch_bounds__(256) void gemma_embed_kernel(const int* __restrict__ ids, const bf16* __restrict__ table, int vocab, int D, float scale,
                                                          float* __restrict__ x, long ldx) {
    const int row = blockIdx.x, id = ids[row];
    const bool ok = id >= 0 && id < vocab;
    const bf16* src = table + (long)(ok ? id : 0) * D;
    float4* dst = (float4*)(x + (long)row * ldx);
    for (int i = threadIdx.x; i < D / 4; i += 256) {
        const bf16x4 v = *(const bf16x4*)(src + 4 * i);
        dst[i] = ok ? make_float4(bf2f(v[0]) * scale, bf2f(v[1]) * scale, bf2f(v[2]) * scale, bf2f(v[3]) * scale) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// The V2 feature extractor's GEMM operand in one pass over the hidden states (reference feature_extractor.py:160-181): one wave per
// (token, layer) row of D floats, held in registers between the sum of squares and the scale, so every fp32 element is read once and
// every 16-bit element written once (two 16-byte loads and one 16-byte store per lane and chunk of 8).  No LDS, no barrier; the
// reduction order is fixed by the butterfly, so two runs agree bit for bit.  A pad token's rows are written as zeros without a read.
template <int NV>          // chunks of 8 per lane: D <= 512 * NV
__global__ __launch_bounds__(256) void gemma_features_rms_kernel(const float* __restrict__ hs, long layer_stride, long row_stride,
                                                                 const int* __restrict__ valid, bf16* __restrict__ out, long ldo, int T, int L,
                                                                 int D, float eps) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)T * L) return;
    const int lane = threadIdx.x & 63, t = (int)(item / L), l = (int)(item % L), n8 = D / 8;
    bf16* orow = out + (long)t * ldo + (long)l * D;
    if (valid && valid[t] == 0) {
        const bf16x8 z = {};
        for (int c = lane; c < n8; c += 64) *(bf16x8*)(orow + 8 * c) = z;
        return;
    }
    const float4* xr = (const float4*)(hs + (long)l * layer_stride + (long)t * row_stride);
    float4 xa[NV], xb[NV];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        if (c < n8) {
            xa[k] = xr[2 * c];
            xb[k] = xr[2 * c + 1];
            ss += xa[k].x * xa[k].x + xa[k].y * xa[k].y + xa[k].z * xa[k].z + xa[k].w * xa[k].w;
            ss += xb[k].x * xb[k].x + xb[k].y * xb[k].y + xb[k].z * xb[k].z + xb[k].w * xb[k].w;
        }
    }
    const float r = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        if (c < n8) {
            const bf16x8 o = {f2bf(xa[k].x * r), f2bf(xa[k].y * r), f2bf(xa[k].z * r), f2bf(xa[k].w * r),
                              f2bf(xb[k].x * r), f2bf(xb[k].y * r), f2bf(xb[k].z * r), f2bf(xb[k].w * r)};
            *(bf16x8*)(orow + 8 * c) = o;
        }
    }
}

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

}  // namespace

int gemma_features_rms_launch(const float* hs, long layer_stride, long row_stride, const int* valid, bf16* out, long ldo, int T, int L, int D,
                              float eps, hipStream_t stream) {
    LTX2_CHECK_ARG(hs && out, "gemma_features_rms: null operand");
    LTX2_CHECK_ARG(T >= 0 && L > 0 && D > 0 && D % 8 == 0 && D <= 8192, "gemma_features_rms: T %d, L %d, D %d (a multiple of 8, at most 8192)", T, L,
                   D);
    LTX2_CHECK_ARG(row_stride >= D && row_stride % 4 == 0 && layer_stride >= 0 && layer_stride % 4 == 0 && ldo >= (long)L * D && ldo % 8 == 0 &&
                       aligned16(hs) && aligned16(out),
                   "gemma_features_rms: 16-byte rows needed (layer stride %ld, row stride %ld, ldo %ld for L * D = %ld)", layer_stride, row_stride, ldo,
                   (long)L * D);
    const long items = (long)T * L;
    if (items == 0) return LTX2_OK;
    LTX2_CHECK_ARG((items + 3) / 4 <= 0x7fffffffL, "gemma_features_rms: T * L = %ld rows exceed the grid", items);
    const dim3 grid((unsigned)((items + 3) / 4));
    if (D <= 512 * 2)
        hipLaunchKernelGGL(gemma_features_rms_kernel<2>, grid, dim3(256), 0, stream, hs, layer_stride, row_stride, valid, out, ldo, T, L, D, eps);
    else if (D <= 512 * 8)
        hipLaunchKernelGGL(gemma_features_rms_kernel<8>, grid, dim3(256), 0, stream, hs, layer_stride, row_stride, valid, out, ldo, T, L, D, eps);
    else
        hipLaunchKernelGGL(gemma_features_rms_kernel<16>, grid, dim3(256), 0, stream, hs, layer_stride, row_stride, valid, out, ldo, T, L, D, eps);
    LTX2_CHECK_LAUNCH("gemma_features_rms");
    return LTX2_OK;
}

int gemma_attn_launch(const bf16* Q, long ldq, const bf16* K, long ldk, const bf16* V, long ldv, bf16* O, long ldo, int Tq, int Tkv,
                      int heads, int kv_heads, int causal, int window, float scale, hipStream_t stream) {
    LTX2_CHECK_ARG(Q && K && V && O, "gemma_attn: null operand");
    LTX2_CHECK_ARG(Tq >= 0 && Tkv >= 0 && heads > 0 && kv_heads > 0 && heads % kv_heads == 0 && heads <= 65535,
                   "gemma_attn: heads %d / kv_heads %d (heads must be a multiple of kv_heads), Tq %d, Tkv %d", heads, kv_heads, Tq, Tkv);
    LTX2_CHECK_ARG(window >= 0 && (causal || window == 0), "gemma_attn: window %d needs causal mode (causal = %d)", window, causal);
    LTX2_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0 && aligned16(Q) && aligned16(K) && aligned16(V) && ((uintptr_t)O & 7) == 0,
                   "gemma_attn: rows must be 16-byte aligned (ldq %ld ldk %ld ldv %ld ldo %ld)", ldq, ldk, ldv, ldo);
    LTX2_CHECK_ARG(ldq >= (long)heads * GA_HD && ldo >= (long)heads * GA_HD && ldk >= (long)kv_heads * GA_HD && ldv >= (long)kv_heads * GA_HD,
                   "gemma_attn: a row stride is narrower than its heads x 256");
    if (Tq == 0) return LTX2_OK;
    static PerDeviceOnce once;
    if (once.first()) (void)hipFuncSetAttribute((const void*)gemma_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GA_LDS);
    GemmaAttnParams p{};
    p.Q = Q;
    p.K = K;
    p.V = V;
    p.O = O;
    p.ldq = ldq;
    p.ldk = ldk;
    p.ldv = ldv;
    p.ldo = ldo;
    p.Tq = Tq;
    p.Tkv = Tkv;
    p.ratio = heads / kv_heads;
    p.causal = causal ? 1 : 0;
    p.window = window;
    p.scale_log2e = scale * 1.4426950408889634f;
    hipLaunchKernelGGL(gemma_attn_kernel, dim3((Tq + GA_QB - 1) / GA_QB, heads), dim3(256), GA_LDS, stream, p);
    LTX2_CHECK_LAUNCH("gemma_attn");
    return LTX2_OK;
}

int gemma_qknorm_rope_launch(bf16* qkv, long ld, int rows, int q_heads, int kv_heads, const float* q_w, const float* k_w, float eps,
                             const float* cos, const float* sin, hipStream_t stream) {
    LTX2_CHECK_ARG(qkv && q_w && k_w && cos && sin, "gemma_qknorm_rope: null operand");
    LTX2_CHECK_ARG(rows >= 0 && q_heads > 0 && kv_heads >= 0 && ld >= (long)(q_heads + kv_heads) * GA_HD && ld % 4 == 0 && ((uintptr_t)qkv & 7) == 0,
                   "gemma_qknorm_rope: rows %d, q_heads %d, kv_heads %d, ld %ld", rows, q_heads, kv_heads, ld);
    const long items = (long)rows * (q_heads + kv_heads);
    if (items == 0) return LTX2_OK;
    hipLaunchKernelGGL(gemma_qknorm_rope_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, stream, qkv, ld, rows, q_heads,
                       q_heads + kv_heads, q_w, k_w, eps, cos, sin);
    LTX2_CHECK_LAUNCH("gemma_qknorm_rope");
    return LTX2_OK;
}

int gemma_resid_norm_launch(const float* x_in, long ldx, const bf16* y, long ldy, const float* w_post, const float* w_next, float* x_out,
                            long ldxo, bf16* h_out, long ldh, float* hf_out, long ldhf, int rows, int D, float eps, hipStream_t stream) {
    LTX2_CHECK_ARG(x_in && (!y || w_post) && (!(h_out || hf_out) || w_next), "gemma_resid_norm: null operand");
    LTX2_CHECK_ARG(rows >= 0 && D > 0 && D % 4 == 0 && D <= 256 * 4 * GR_NV, "gemma_resid_norm: D %d (a multiple of 4, at most %d)", D, 256 * 4 * GR_NV);
    LTX2_CHECK_ARG(ldx % 4 == 0 && (!y || ldy % 4 == 0) && ldxo % 4 == 0 && ldh % 4 == 0 && ldhf % 4 == 0 && aligned16(x_in) && aligned16(w_post) &&
                       aligned16(w_next) && aligned16(x_out) && aligned16(hf_out) && ((uintptr_t)y & 7) == 0 && ((uintptr_t)h_out & 7) == 0,
                   "gemma_resid_norm: misaligned operand");
    if (rows == 0) return LTX2_OK;
    hipLaunchKernelGGL(gemma_resid_norm_kernel, dim3(rows), dim3(256), 0, stream, x_in, ldx, y, ldy, w_post, w_next, x_out, ldxo, h_out, ldh,
                       hf_out, ldhf, D, eps);
    LTX2_CHECK_LAUNCH("gemma_resid_norm");
    return LTX2_OK;
}

int gemma_gated_act_launch(const bf16* gu, long ldgu, bf16* out, long ldo, int rows, int inter, int act, hipStream_t stream) {
    LTX2_CHECK_ARG(gu && out, "gemma_gated_act: null operand");
    LTX2_CHECK_ARG(act == 0 || act == 1, "gemma_gated_act: act %d (0 = silu, 1 = gelu_pytorch_tanh)", act);
    LTX2_CHECK_ARG(rows >= 0 && inter > 0 && inter % 8 == 0 && ldgu % 8 == 0 && ldo % 8 == 0 && ldgu >= 2L * inter && ldo >= inter && aligned16(gu) &&
                       aligned16(out),
                   "gemma_gated_act: inter %d (a multiple of 8), ldgu %ld, ldo %ld", inter, ldgu, ldo);
    const long n = (long)rows * (inter / 8);
    if (n == 0) return LTX2_OK;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (act == 0)
        hipLaunchKernelGGL(gemma_gated_act_kernel<0>, grid, dim3(256), 0, stream, gu, ldgu, out, ldo, rows, inter);
    else
        hipLaunchKernelGGL(gemma_gated_act_kernel<1>, grid, dim3(256), 0, stream, gu, ldgu, out, ldo, rows, inter);
    LTX2_CHECK_LAUNCH("gemma_gated_act");
    return LTX2_OK;
}

int gemma_embed_launch(const int* ids, int rows, const bf16* table, int vocab, int D, float scale, float* x, long ldx, hipStream_t stream) {
    LTX2_CHECK_ARG(ids && table && x, "gemma_embed: null operand");
    LTX2_CHECK_ARG(rows >= 0 && vocab > 0 && D > 0 && D % 4 == 0 && ldx % 4 == 0 && aligned16(x) && ((uintptr_t)table & 7) == 0,
                   "gemma_embed: D %d (a multiple of 4), ldx %ld", D, ldx);
    if (rows == 0) return LTX2_OK;
    hipLaunchKernelGGL(gemma_embed_kernel, dim3(rows), dim3(256), 0, stream, ids, table, vocab, D, scale, x, ldx);
    LTX2_CHECK_LAUNCH("gemma_embed");
    return LTX2_OK;
}
