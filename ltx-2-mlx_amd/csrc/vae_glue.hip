// Norm / activation / layout glue around the VAE decoder's and encoder's convolutions, for gfx950 (HBM-bound, 8/16-byte vectors):
//   vae_prepare_latent                 latent fp32 [C][P] -> de-normalised (+ noise) channels-last 16-bit [P][C]
//   pixnorm_mod_silu (plain, padded)   pixel norm + timestep modulation + SiLU, optionally into the padded volume of the implicit-GEMM conv
//   pad_volume                         the same padded volume without arithmetic
//   vae_unpatchify, video_to_uint8, video_chunk_to_uint8, tile_blend_accumulate / finish   decoder output: pixels, chunk cross-fade, tiled blend
//   s2d_downsample, latent_normalize_nchw                                                  encoder: downsample tail, latent statistics
// padded_src_pos() is the one statement of the padding rule the padded pixel norm, pad_volume and the conv's tap offsets agree on.
//
// Reference semantics restated (paths under the reference's LTX_2_MLX):
//   vae_*, pixnorm    video_vae/simple_decoder.py:339-342,228-238,492-498,528-553; ops.py:109-125
//   padding           video_vae/simple_decoder.py:105-134
//   chunk cross-fade  video_vae/simple_decoder.py:760-798
//   tile blend        tiling.py:380-412
#include "rowops.h"

namespace {

// out[t'][h'][w'][co] = y_s2d[co] + mean_{q in group co} x_s2d[q]   (VAE encoder downsample, see ltx2hip.h)
__global__ __launch_bounds__(256) void s2d_downsample_kernel(const bf16* __restrict__ y, const bf16* __restrict__ x,
                                                             bf16* __restrict__ out, int T, int H, int W, int Cc, int Cin,
                                                             int st, int sh, int sw, long n) {
    const int sp = st * sh * sw, Cout = Cc * sp, gs = Cin / Cc;
    const int To = T / st, Ho = H / sh, Wo = W / sw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        long pos = i / Cout;
        const int wo = (int)(pos % Wo);
        pos /= Wo;
        const int ho = (int)(pos % Ho), to = (int)(pos / Ho);
        (void)To;
        auto src_pos = [&](int s) {
            const int a = s / (sh * sw), b = (s / sw) % sh, d = s % sw;
            return ((long)(to * st + a) * H + (ho * sh + b)) * W + (wo * sw + d);
        };
        float v = bf2f(y[src_pos(co % sp) * Cc + co / sp]);
        float m = 0.f;
        for (int q = co * gs; q < (co + 1) * gs; ++q) m += bf2f(x[src_pos(q % sp) * Cin + q / sp]);
        out[i] = f2bf(v + m / (float)gs);
    }
}

// x bf16 [P][C] -> out fp32 [C][P] = (x - mean[c]) / std[c]
__global__ __launch_bounds__(256) void latent_normalize_nchw_kernel(const bf16* __restrict__ x, const float* __restrict__ mean,
                                                                    const float* __restrict__ stdv, float* __restrict__ out,
                                                                    int C, long P) {
    __shared__ float tile[64][65];
    const long p0 = (long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int pr = i >> 6, cc = i & 63;
        tile[pr][cc] = (p0 + pr < P && c0 + cc < C) ? bf2f(x[(p0 + pr) * C + c0 + cc]) : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int cc = i >> 6, pr = i & 63;
        if (p0 + pr < P && c0 + cc < C) out[(long)(c0 + cc) * P + p0 + pr] = (tile[pr][cc] - mean[c0 + cc]) / stdv[c0 + cc];
    }
}

__global__ void vae_prepare_latent_kernel(const float* __restrict__ latent, const float* __restrict__ stdv,
                                          const float* __restrict__ meanv, const float* __restrict__ noise,
                                          float ns, bf16* __restrict__ out, int C, long P) {
    // out[p][c] <- latent[c][p]; tile transpose through LDS (32 positions x 32 channels)
    __shared__ float tile[32][33];
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: ty 0..7
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        const long pp = p0 + tx;
        float v = 0.f;
        if (c < C && pp < P) {
            v = latent[(long)c * P + pp] * stdv[c] + meanv[c];
            if (ns > 0.f) v = (noise ? noise[(long)c * P + pp] : 0.f) * ns + (1.f - ns) * v;
        }
        tile[k][tx] = v;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const long pp = p0 + k;
        const int c = c0 + tx;
        if (c < C && pp < P) out[pp * C + c] = f2bf(tile[tx][k]);
    }
}

// Position `pos` of the PADDED channels-last volume [T+2][H+2][W+2] -> the position of [T][H][W] it shows: replicate in T with
// `pad_front` leading frames, reflect in H / W (reference simple_decoder.py:105-134).  The implicit-GEMM conv of gemm_v4.hip reads
// volumes padded by this rule, whichever kernel wrote them.
__device__ __forceinline__ long padded_src_pos(long pos, int T, int H, int W, int pad_front) {
    const int Hp = H + 2, Wp = W + 2;
    const int tp = (int)(pos / ((long)Hp * Wp)), r2 = (int)(pos - (long)tp * Hp * Wp), hp = r2 / Wp, wp = r2 - hp * Wp;
    const int t = min(max(tp - pad_front, 0), T - 1);
    int h = hp - 1, w = wp - 1;
    h = h < 0 ? -h : (h >= H ? 2 * H - 2 - h : h);
    w = w < 0 ? -w : (w >= W ? 2 * W - 2 - w : w);
    return ((long)t * H + h) * W + w;
}

// LP lanes per position, each lane owns C/LP contiguous channels (8 or 16).  A thread keeps its channels' (1+scale) and
// shift values in registers and walks positions with a grid stride: loaded per position, the four 16-byte table reads
// per 16 bytes of data made the kernel VMEM-issue-bound (3.85 TB/s at C = 128).
// PAD: the output is the padded volume of padded_src_pos(): the loop walks padded positions and normalises the source
// position each one mirrors (a few % more rows than the interior).
template <int E, bool PAD>
__global__ __launch_bounds__(256) void pixnorm_mod_silu_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, long P,
                                                               int C, int lp_shift, float eps,
                                                               const float* __restrict__ tab,
                                                               const float* __restrict__ te, int shift_row,
                                                               int scale_row, int T, int H, int W, int pad_front) {
    const int LP = 1 << lp_shift;
    const long gthread = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long pos_stride = ((long)gridDim.x * blockDim.x) >> lp_shift;
    const int sub = (int)(gthread & (LP - 1));
    const int c0 = sub * E;
    float sc1[E], sh[E];
#pragma unroll
    for (int q4 = 0; q4 < E / 4; ++q4) {
        const int c = c0 + q4 * 4;
        f32x4 a = *(const f32x4*)(tab + shift_row * C + c), b = *(const f32x4*)(tab + scale_row * C + c);
        if (te) {
            a += *(const f32x4*)(te + shift_row * C + c);
            b += *(const f32x4*)(te + scale_row * C + c);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sh[q4 * 4 + e] = a[e];
            sc1[q4 * 4 + e] = 1.f + b[e];
        }
    }
    const float inv_c = 1.f / (float)C;
    // the LP lanes of a position share `pos`, so a shuffle group is always wholly inside or wholly outside the loop
    for (long pos = gthread >> lp_shift; pos < P; pos += pos_stride) {
        const long src = PAD ? padded_src_pos(pos, T, H, W, pad_front) : pos;
        float v[E];
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < E / 8; ++i) {
            const bf16x8 t8 = *(const bf16x8*)(x + src * C + c0 + i * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[i * 8 + e] = bf2f(t8[e]);
                s2 += v[i * 8 + e] * v[i * 8 + e];
            }
        }
        for (int o = LP >> 1; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
        const float rstd = rsqrtf(s2 * inv_c + eps);
#pragma unroll
        for (int i = 0; i < E / 8; ++i) {
            bf16x8 o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) o8[e] = f2bf(silu_f(v[i * 8 + e] * rstd * sc1[i * 8 + e] + sh[i * 8 + e]));
            *(bf16x8*)(y + pos * C + c0 + i * 8) = o8;
        }
    }
}

__global__ void vae_unpatchify_kernel(const bf16* __restrict__ x, float* __restrict__ video, int T, int H, int W) {
    // video[c][t][h*4+rh][w*4+rw] = x[t][h][w][c*16 + rw*4 + rh]
    const int HO = H * 4, WO = W * 4;
    const long n = (long)3 * T * HO * WO;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int xo = (int)(i % WO);
        long r = i / WO;
        const int yo = (int)(r % HO);
        r /= HO;
        const int t = (int)(r % T);
        const int c = (int)(r / T);
        const int w = xo >> 2, rw = xo & 3, h = yo >> 2, rh = yo & 3;
        video[i] = bf2f(x[(((long)t * H + h) * W + w) * 48 + c * 16 + rw * 4 + rh]);
    }
}

__global__ void video_to_uint8_kernel(const float* __restrict__ video, unsigned char* __restrict__ frames, int T, int H,
                                      int W) {
    const long plane = (long)T * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (video[c * plane + i] + 1.f) * 0.5f;
            v = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
            frames[i * 3 + c] = (unsigned char)v;
        }
    }
}

// One temporal chunk of decode_latent -> uint8 frames, cross-faded with the previous chunk on the first `ov` frames
// (simple_decoder.py:760-798): frame j of `cur` lands on output frame t_dst0 + j; for j < ov the value is
// prev[prev_T - ov + j] * (1 - ramp[j]) + cur[j] * ramp[j] with torch.linspace's ramp, rounded exactly like the separate torch
// ops it replaces (no FMA contraction); frames at or beyond T_out are dropped (the final trim).
__global__ void video_chunk_to_uint8_kernel(const float* __restrict__ cur, const float* __restrict__ prev, const float* __restrict__ ramp,
                                            unsigned char* __restrict__ frames, int Tc, int prev_T, int ov, int H, int W,
                                            int t_dst0, int T_out) {
    const long hw = (long)H * W, plane = (long)Tc * hw, pplane = (long)prev_T * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i / hw);
        const long px = i - (long)j * hw;
        const int t = t_dst0 + j;
        if (t >= T_out) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = cur[c * plane + i];
            if (prev && j < ov) {
                const float r = ramp[j];
                const float a = prev[c * pplane + (long)(prev_T - ov + j) * hw + px];
                v = add_rn(mul_rn(a, sub_rn(1.0f, r)), mul_rn(v, r));
            }
            v = (v + 1.f) * 0.5f;
            v = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
            frames[((long)t * hw + px) * 3 + c] = (unsigned char)v;
        }
    }
}

// decode_tiled (tiling.py:380-412): out[c][t0+t][h0+h][w0+w] += tile[c][t][h][w] * m, wsum[...] += m with the separable
// trapezoid mask m = mt[t] * mh[h] * mw[w], one pass over the tile instead of three torch passes over volume slices.
__global__ void tile_blend_accumulate_kernel(const float* __restrict__ tile, int dt, int dh, int dw, int nt, int nh, int nw,
                                             const float* __restrict__ mt, const float* __restrict__ mh, const float* __restrict__ mw,
                                             float* __restrict__ out, float* __restrict__ wsum, int OT, int OH, int OW, int t0, int h0, int w0) {
    const long n = (long)nt * nh * nw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int w = (int)(i % nw);
        const long r = i / nw;
        const int h = (int)(r % nh), t = (int)(r / nh);
        const float m = mul_rn(mul_rn(mt[t], mh[h]), mw[w]);
        const long o = ((long)(t0 + t) * OH + (h0 + h)) * OW + (w0 + w);
        wsum[o] = add_rn(wsum[o], m);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long oc = (long)c * OT * OH * OW + o;
            out[oc] = add_rn(out[oc], mul_rn(tile[((long)c * dt + t) * dh * dw + (long)h * dw + w], m));
        }
    }
}

__global__ void tile_blend_finish_kernel(float* __restrict__ out, const float* __restrict__ wsum, long plane) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (long)gridDim.x * blockDim.x) {
        const float d = fmaxf(wsum[i], 1e-8f);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c * plane + i] = __fdiv_rn(out[c * plane + i], d);
    }
}

}  // namespace

int s2d_downsample_launch(const bf16* y, const bf16* x, bf16* out, int T, int H, int W, int Cc, int Cin, int st, int sh, int sw,
                          hipStream_t stream) {
    LTX2_CHECK_ARG(y && x && out && T > 0 && H > 0 && W > 0, "s2d_downsample: bad argument");
    LTX2_CHECK_ARG(st >= 1 && sh >= 1 && sw >= 1 && T % st == 0 && H % sh == 0 && W % sw == 0, "s2d_downsample: dims must divide by the stride");
    LTX2_CHECK_ARG(Cc > 0 && Cin % Cc == 0, "s2d_downsample: Cin=%d must be a multiple of the conv width %d", Cin, Cc);
    const long n = (long)(T / st) * (H / sh) * (W / sw) * Cc * st * sh * sw;
    hipLaunchKernelGGL(s2d_downsample_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, stream, y, x, out, T, H, W, Cc, Cin, st, sh, sw, n);
    LTX2_CHECK_LAUNCH("s2d_downsample_kernel");
    return LTX2_OK;
}

int latent_normalize_nchw_launch(const bf16* x, const float* mean, const float* stdv, float* out, int C, long P, hipStream_t stream) {
    LTX2_CHECK_ARG(x && mean && stdv && out && C > 0 && P > 0, "latent_normalize: bad argument");
    hipLaunchKernelGGL(latent_normalize_nchw_kernel, dim3((int)((P + 63) / 64), (C + 63) / 64), dim3(256), 0, stream, x, mean, stdv, out, C, P);
    LTX2_CHECK_LAUNCH("latent_normalize_nchw_kernel");
    return LTX2_OK;
}

int vae_prepare_latent_launch(const float* latent, const float* std, const float* mean, const float* noise,
                              float noise_scale, bf16* out, int C, long P, hipStream_t stream) {
    dim3 grid((unsigned)((P + 31) / 32), (C + 31) / 32);
    hipLaunchKernelGGL(vae_prepare_latent_kernel, grid, dim3(256), 0, stream, latent, std, mean, noise, noise_scale, out, C, P);
    LTX2_CHECK_LAUNCH("vae_prepare_latent_kernel");
    return LTX2_OK;
}

static int pixnorm_launch_impl(const bf16* x, bf16* y, long P, int C, float eps, const float* tab, const float* te,
                               int shift_row, int scale_row, bool pad, int T, int H, int W, int pad_front, hipStream_t stream) {
    LTX2_CHECK_ARG(P > 0 && C >= 64 && (C & (C - 1)) == 0 && C <= 1024, "pixnorm: P=%ld must be positive, C=%d a power of two in [64,1024]", P, C);
    const int E = (C >= 1024) ? 16 : 8;
    const int LP = C / E;
    int lp_shift = 0;
    while ((1 << lp_shift) < LP) ++lp_shift;
    const int grid = grid_for(P * LP, 256, 8192);        // 32 blocks per CU; the kernel walks the rest
#define PIX_LAUNCH(EE, PP) \
    hipLaunchKernelGGL((pixnorm_mod_silu_kernel<EE, PP>), dim3(grid), dim3(256), 0, stream, x, y, P, C, lp_shift, eps, tab, te, shift_row, scale_row, T, H, W, pad_front)
    if (E == 16) {
        if (pad) PIX_LAUNCH(16, true);
        else PIX_LAUNCH(16, false);
    } else {
        if (pad) PIX_LAUNCH(8, true);
        else PIX_LAUNCH(8, false);
    }
#undef PIX_LAUNCH
    LTX2_CHECK_LAUNCH("pixnorm_mod_silu_kernel");
    return LTX2_OK;
}

int pixnorm_mod_silu_launch(const bf16* x, bf16* y, long P, int C, float eps, const float* tab, const float* te,
                            int shift_row, int scale_row, hipStream_t stream) {
    return pixnorm_launch_impl(x, y, P, C, eps, tab, te, shift_row, scale_row, false, 0, 0, 0, 0, stream);
}

// y = the padded volume [T+2][H+2][W+2][C] (see the kernel comment)
int pixnorm_mod_silu_padded_launch(const bf16* x, bf16* y, int T, int H, int W, int C, float eps, const float* tab, const float* te,
                                   int shift_row, int scale_row, int pad_front, hipStream_t stream) {
    LTX2_CHECK_ARG(H >= 2 && W >= 2 && T >= 1 && (pad_front == 1 || pad_front == 2), "pixnorm (padded): reflect padding needs H, W >= 2");
    return pixnorm_launch_impl(x, y, (long)(T + 2) * (H + 2) * (W + 2), C, eps, tab, te, shift_row, scale_row, true, T, H, W, pad_front, stream);
}

// y = x copied into the padded volume of padded_src_pos(), no arithmetic: the input of the depth-to-space upsample convs, which no
// norm precedes
__global__ __launch_bounds__(256) void pad_volume_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, long P, int cshift, int T, int H, int W,
                                                         int pad_front) {
    const int C8 = 1 << cshift;            // 16-byte chunks per position
    const long total = P << cshift;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long pos = i >> cshift;
        const int c = (int)(i & (C8 - 1));
        const long src = padded_src_pos(pos, T, H, W, pad_front);
        *(u32x4*)(y + (pos << (cshift + 3)) + c * 8) = *(const u32x4*)(x + (src << (cshift + 3)) + c * 8);
    }
}
int pad_volume_launch(const bf16* x, bf16* y, int T, int H, int W, int C, int pad_front, hipStream_t stream) {
    LTX2_CHECK_ARG(H >= 2 && W >= 2 && T >= 1 && (pad_front == 1 || pad_front == 2) && C >= 8 && (C & (C - 1)) == 0, "pad_volume: reflect padding needs H, W >= 2; C a power of two >= 8");
    int cshift = 0;
    while ((8 << cshift) < C) ++cshift;
    const long P = (long)(T + 2) * (H + 2) * (W + 2);
    hipLaunchKernelGGL(pad_volume_kernel, dim3(grid_for(P << cshift, 256, 16384)), dim3(256), 0, stream, x, y, P, cshift, T, H, W, pad_front);
    LTX2_CHECK_LAUNCH("pad_volume_kernel");
    return LTX2_OK;
}

int vae_unpatchify_launch(const bf16* x, float* video, int T, int H, int W, hipStream_t stream) {
    const long n = (long)3 * T * H * 4 * W * 4;
    hipLaunchKernelGGL(vae_unpatchify_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, stream, x, video, T, H, W);
    LTX2_CHECK_LAUNCH("vae_unpatchify_kernel");
    return LTX2_OK;
}

int video_to_uint8_launch(const float* video, unsigned char* frames, int T, int H, int W, hipStream_t stream) {
    const long n = (long)T * H * W;
    hipLaunchKernelGGL(video_to_uint8_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, stream, video, frames, T, H, W);
    LTX2_CHECK_LAUNCH("video_to_uint8_kernel");
    return LTX2_OK;
}

int video_chunk_to_uint8_launch(const float* cur, const float* prev, const float* ramp, unsigned char* frames, int Tc, int prev_T, int ov,
                                int H, int W, int t_dst0, int T_out, hipStream_t stream) {
    LTX2_CHECK_ARG(Tc > 0 && H > 0 && W > 0 && (!prev || (ov >= 1 && ov <= Tc && ov <= prev_T && ramp)), "video_chunk_to_uint8: bad overlap");
    const long n = (long)Tc * H * W;
    hipLaunchKernelGGL(video_chunk_to_uint8_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, stream, cur, prev, ramp, frames, Tc, prev_T, ov,
                       H, W, t_dst0, T_out);
    LTX2_CHECK_LAUNCH("video_chunk_to_uint8_kernel");
    return LTX2_OK;
}

int tile_blend_accumulate_launch(const float* tile, int dt, int dh, int dw, int nt, int nh, int nw, const float* mt, const float* mh,
                                 const float* mw, float* out, float* wsum, int OT, int OH, int OW, int t0, int h0, int w0, hipStream_t stream) {
    LTX2_CHECK_ARG(nt <= dt && nh <= dh && nw <= dw && t0 + nt <= OT && h0 + nh <= OH && w0 + nw <= OW, "tile_blend_accumulate: tile outside the volume");
    const long n = (long)nt * nh * nw;
    hipLaunchKernelGGL(tile_blend_accumulate_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, stream, tile, dt, dh, dw, nt, nh, nw, mt, mh, mw,
                       out, wsum, OT, OH, OW, t0, h0, w0);
    LTX2_CHECK_LAUNCH("tile_blend_accumulate_kernel");
    return LTX2_OK;
}

int tile_blend_finish_launch(float* out, const float* wsum, long plane, hipStream_t stream) {
    hipLaunchKernelGGL(tile_blend_finish_kernel, dim3(grid_for(plane, 256, 16384)), dim3(256), 0, stream, out, wsum, plane);
    LTX2_CHECK_LAUNCH("tile_blend_finish_kernel");
    return LTX2_OK;
}
