// Audio VAE decoder + vocoders (model/audio_vae/): the fp32 kernels and their ltx2_audio_* C entry points (declared in include/ltx2hip.h).
// Everything here is fp32 end to end (operands, accumulation, activations in HBM), as the reference forces for this path: the
// convolutions run on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32).  Tensors are channels-last: one row of C channels per time step
// (1-D) or per (h, w) pixel (2-D, rows h-major).  Nothing here depends on LTX2_F16: both library builds carry the same code.
#include <math.h>

#include "../../include/ltx2hip.h"
#include "common.h"

namespace {

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------------------------
// Implicit-GEMM convolution.  M = output positions (h_out * w_out), N = c_out, K = ntaps * c_in with k = tap * c_in + c and
// tap = i * kw + j.  Output position p = (h, w) reads source row vh = h * stride_h + up - pad_h + i and column
// vw = w * stride + j * dil - pad_w (stride_h = 1 everywhere but the encoder's Downsample2d, which keeps every second row and column: only
// the kept outputs are rows of M); with up != 0 the source is the nearest x2 image of the input (Upsample2d, whose first output row is
// dropped: the `+ up`).
// Block: 256 threads = 2 x 2 waves over a (32 FM) x (32 FN) tile, each wave FM x FN 16x16 MFMA blocks; K steps of 16.
// ------------------------------------------------------------------------------------------------------------------------------
struct AudioConvParams {
    const float* x;
    long ldx;
    int h_in, w_in, c_in;
    const float* w;
    long ldw;
    const float* bias;
    float* y;
    long ldy;
    long M;
    int w_out, c_out, K;
    int kw, ntaps, stride, stride_h, dil, pad_h, pad_w, up;
    int pro;
    float slope;
    const float* res;
    long ldres;
    float alpha, beta;
    int act;
};

constexpr int AC_BK = 16;
constexpr int AC_LDA = AC_BK + 4;   // A tile [BM][20]: 16-byte rows, and the 16x16x4 operand reads (row = lane & 15) hit distinct banks

template <int FM, int FN, bool VEC>
__global__ __launch_bounds__(256) void audio_conv_kernel(AudioConvParams p) {
    constexpr int BM = 32 * FM, BN = 32 * FN, LDB = BN + 16;
    constexpr int AR = BM / 64;                          // A rows staged per thread (one 4-wide k group each)
    constexpr int BQ = 16 * BN / 4;                      // float4 groups of one B tile
    constexpr int BV = (BQ + 255) / 256;
    constexpr int NE = VEC ? 1 : 4;                      // k counters per thread: one float4 group, or four scalars
    __shared__ __attribute__((aligned(16))) float As[BM * AC_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[AC_BK * LDB];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int kq = tid & 3;

    int vh0[AR], vw0[AR];
    bool rok[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        const long m = m0 + (tid >> 2) + 64 * i;
        rok[i] = m < p.M;
        const long mm = rok[i] ? m : 0;
        const int h = (int)(mm / p.w_out), w = (int)(mm - (long)h * p.w_out);
        vh0[i] = h * p.stride_h + p.up - p.pad_h;
        vw0[i] = w * p.stride - p.pad_w;
    }
    int tap[NE], cc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int k = 4 * kq + e;
        tap[e] = k / p.c_in;
        cc[e] = k - tap[e] * p.c_in;
    }

    // source of row slot i at (tap t, channel c); null where the convolution reads padding
    auto a_src = [&](int i, int t, int c) -> const float* {
        if (!rok[i] || t >= p.ntaps) return nullptr;
        const int ti = t / p.kw, tj = t - ti * p.kw;
        int vh = vh0[i] + ti, vw = vw0[i] + tj * p.dil;
        if (p.up) {
            if (vh < 0 || vh >= 2 * p.h_in || vw < 0 || vw >= 2 * p.w_in) return nullptr;
            vh >>= 1;
            vw >>= 1;
        } else if (vh < 0 || vh >= p.h_in || vw < 0 || vw >= p.w_in) {
            return nullptr;
        }
        return p.x + ((long)vh * p.w_in + vw) * p.ldx + c;
    };

    f32x4 ra[AR];
    f32x4 rb[BV];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {
                const float* s = a_src(i, tap[0], cc[0]);
                if (s) v = *(const f32x4*)s;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* s = a_src(i, tap[e], cc[e]);
                    if (s) {
                        float a = s[0];
                        if (p.pro == 2) {
                            const float b = s[p.c_in];
                            a = sqrtf(a * a + b * b);
                        }
                        v[e] = a;
                    }
                }
            }
            if (p.pro == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? v[e] * p.slope : v[e];
            }
            ra[i] = v;
        }
#pragma unroll
        for (int j = 0; j < BV; ++j) {
            const int idx = tid + 256 * j;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (idx < BQ) {
                const int kr = idx / (BN / 4), n = n0 + 4 * (idx % (BN / 4));
                const int k = k0 + kr;
                if (k < p.K && n < p.ldw) v = *(const f32x4*)(p.w + (long)k * p.ldw + n);
            }
            rb[j] = v;
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int q = cc[e] + AC_BK, d = q / p.c_in;
            tap[e] += d;
            cc[e] = q - d * p.c_in;
        }
    };

    f32x4 acc[FM][FN];
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int b = 0; b < FN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nk = (p.K + AC_BK - 1) / AC_BK;
    load(0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int i = 0; i < AR; ++i) *(f32x4*)&As[((tid >> 2) + 64 * i) * AC_LDA + 4 * kq] = ra[i];
#pragma unroll
        for (int j = 0; j < BV; ++j) {
            const int idx = tid + 256 * j;
            if (idx < BQ) *(f32x4*)&Bs[(idx / (BN / 4)) * LDB + 4 * (idx % (BN / 4))] = rb[j];
        }
        __syncthreads();
        if (kt + 1 < nk) load((kt + 1) * AC_BK);       // the next tile's global reads are in flight under this tile's MFMAs
#pragma unroll
        for (int s = 0; s < AC_BK / 4; ++s) {
            float fa[FM], fb[FN];
#pragma unroll
            for (int a = 0; a < FM; ++a) fa[a] = As[(wm * 16 * FM + a * 16 + (lane & 15)) * AC_LDA + 4 * s + (lane >> 4)];
#pragma unroll
            for (int b = 0; b < FN; ++b) fb[b] = Bs[(4 * s + (lane >> 4)) * LDB + wn * 16 * FN + b * 16 + (lane & 15)];
#pragma unroll
            for (int a = 0; a < FM; ++a)
#pragma unroll
                for (int b = 0; b < FN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: C/D map col = lane & 15, row = 4 * (lane >> 4) + r
#pragma unroll
    for (int a = 0; a < FM; ++a)
#pragma unroll
        for (int b = 0; b < FN; ++b) {
            const int n = n0 + wn * 16 * FN + b * 16 + (lane & 15);
            if (n >= p.c_out) continue;
            const float bn = p.bias ? p.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wm * 16 * FM + a * 16 + 4 * (lane >> 4) + r;
                if (m >= p.M) continue;
                float v = acc[a][b][r] + bn;
                if (p.res) v += p.res[m * p.ldres + n];
                v *= p.alpha;
                float* dst = p.y + m * p.ldy + n;
                if (p.beta != 0.f) v += p.beta * *dst;
                if (p.act == 1) v = tanhf(v);
                else if (p.act == 2) v = fminf(fmaxf(v, -1.f), 1.f);
                else if (p.act == 3) v = logf(fmaxf(v, 1e-5f));
                else if (p.act == 4) v = v * (1.f / (1.f + expf(-v)));
                *dst = v;
            }
        }
}

template <int FM, int FN>
void conv_dispatch_vec(const AudioConvParams& p, bool vec, dim3 grid, hipStream_t stream) {
    if (vec)
        hipLaunchKernelGGL((audio_conv_kernel<FM, FN, true>), grid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL((audio_conv_kernel<FM, FN, false>), grid, dim3(256), 0, stream, p);
}

// Tile per shape: the N tile follows c_out (32 / 64 / 128 wide, so the last vocoder stages' 32 and the stereo 2 channels waste
// little); the M tile is 128 rows when the grid then still fills a round of the 256 CUs, 64 otherwise.
int conv_launch(AudioConvParams p, hipStream_t stream) {
    if (p.M == 0) return LTX2_OK;
    const int fn = p.c_out > 64 ? 4 : (p.c_out > 32 ? 2 : 1);
    const long tiles_n = (p.c_out + 32 * fn - 1) / (32 * fn);
    const int fm = ((p.M + 127) / 128) * tiles_n >= 256 ? 4 : 2;
    const bool vec = p.pro != 2 && p.c_in % 4 == 0 && p.ldx % 4 == 0 && aligned16(p.x);
    const dim3 grid((unsigned)((p.M + 32 * fm - 1) / (32 * fm)), (unsigned)tiles_n);
    if (fm == 4) {
        if (fn == 4) conv_dispatch_vec<4, 4>(p, vec, grid, stream);
        else if (fn == 2) conv_dispatch_vec<4, 2>(p, vec, grid, stream);
        else conv_dispatch_vec<4, 1>(p, vec, grid, stream);
    } else {
        if (fn == 4) conv_dispatch_vec<2, 4>(p, vec, grid, stream);
        else if (fn == 2) conv_dispatch_vec<2, 2>(p, vec, grid, stream);
        else conv_dispatch_vec<2, 1>(p, vec, grid, stream);
    }
    LTX2_CHECK_LAUNCH("audio_conv");
    return LTX2_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Activation1d(SnakeBeta), fused: a block owns 64 output steps x 64 channels.  It computes the 2 * 64 + down_k - 2 snake values the
// low-pass reads (replicate-clamped indices of the x2 signal, each from up_k / 2 taps of the replicate-padded input) into LDS, then
// filters and decimates.  Upsample: pad = up_k / 2 - 1, pad_left = 2 * pad + (up_k - 2) / 2 (UpSample1d(2, up_k)); low-pass
// pad_left = down_k / 2 - (down_k even) (LowPassFilter1d).
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int SN_T = 64, SN_C = 64;

__global__ __launch_bounds__(256) void audio_snake_aa_kernel(const float* __restrict__ x, long ldx, int T, int C, const float* __restrict__ alpha,
                                                             const float* __restrict__ beta, const float* __restrict__ fu, int ku,
                                                             const float* __restrict__ fd, int kd, float* __restrict__ y, long ldy) {
    __shared__ float zs[(2 * SN_T + 16) * SN_C];
    __shared__ float su[16], sd[16];
    const int tid = threadIdx.x, cl = tid & (SN_C - 1), r = tid >> 6;
    if (tid < ku) su[tid] = fu[tid];
    if (tid < kd) sd[tid] = fd[tid];
    __syncthreads();
    const int c = blockIdx.y * SN_C + cl;
    const bool cok = c < C;
    const int t0 = blockIdx.x * SN_T;
    const float ea = cok ? expf(alpha[c]) : 0.f, ib = cok ? 1.f / (expf(beta[c]) + 1e-9f) : 0.f;
    const int pu = ku / 2 - 1, pul = 2 * pu + (ku - 2) / 2;
    const int pdl = kd / 2 - ((kd & 1) == 0 ? 1 : 0);
    const int nz = 2 * SN_T + kd - 2;
    for (int j = r; j < nz; j += 4) {
        const int u = min(max(2 * t0 - pdl + j, 0), 2 * T - 1);
        float v = 0.f;
        if (cok) {
            for (int k = (u + pul) & 1; k < ku; k += 2) {
                const int i = min(max((u + pul - k) / 2 - pu, 0), T - 1);
                v += su[k] * x[(long)i * ldx + c];
            }
            v *= 2.f;
            const float s = sinf(v * ea);
            v += ib * (s * s);
        }
        zs[j * SN_C + cl] = v;
    }
    __syncthreads();
    if (!cok) return;
    for (int o = r; o < SN_T; o += 4) {
        const int t = t0 + o;
        if (t >= T) break;
        float a = 0.f;
        for (int k = 0; k < kd; ++k) a += sd[k] * zs[(2 * o + k) * SN_C + cl];
        y[(long)t * ldy + c] = a;
    }
}

// UpSample1d (any ratio): y[u][c] = ratio * sum_k f[k] x[clamp((u + pad_left - k) / ratio - pad)][c], (u + pad_left - k) % ratio == 0
__global__ __launch_bounds__(256) void audio_upsample_kernel(const float* __restrict__ x, long ldx, int T, int C, const float* __restrict__ f, int K,
                                                             int ratio, int pad, int pad_left, float* __restrict__ y, long ldy, int t_out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)t_out * C) return;
    const int u = (int)(idx / C), c = (int)(idx - (long)u * C);
    float v = 0.f;
    for (int k = 0; k < K; ++k) {
        const int q = u + pad_left - k;
        if (q < 0 || q % ratio) continue;
        const int i = min(max(q / ratio - pad, 0), T - 1);
        v += f[k] * x[(long)i * ldx + c];
    }
    y[(long)u * ldy + c] = (float)ratio * v;
}

// PixelNorm + SiLU: one wave per row of C channels
__global__ __launch_bounds__(256) void audio_pixnorm_silu_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y, long ldy, long rows,
                                                                 int C, float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const f32x4* xr = (const f32x4*)(x + row * ldx);
    f32x4* yr = (f32x4*)(y + row * ldy);
    float ss = 0.f;
    for (int i = lane; i < C / 4; i += 64) {
        const f32x4 v = xr[i];
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float d = sqrtf(ss / (float)C + eps);
    for (int i = lane; i < C / 4; i += 64) {
        f32x4 v = xr[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = v[e] / d;
            v[e] = t * (1.f / (1.f + expf(-t)));
        }
        yr[i] = v;
    }
}

// Encoder latent normalisation (encoder.py:172-203: patchify -> (x - mean) / std -> unpatchify on the mean half of conv_out) in one pass:
// channels-last h [T][F][ld] -> out (z, T, F), statistic index c * F + f.  One IEEE subtract and one IEEE divide per element, as torch does.
__global__ __launch_bounds__(256) void audio_latent_normalize_kernel(const float* __restrict__ h, long ld, const float* __restrict__ mean,
                                                                     const float* __restrict__ stdv, float* __restrict__ out, int T, int F, int z) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long tf = (long)T * F;
    if (idx >= tf * z) return;
    const int c = (int)(idx / tf);
    const long r = idx - (long)c * tf;                  // t * F + f
    const int f = (int)(r % F);
    const float d = h[r * ld + c] - mean[c * F + f];
    out[idx] = d / stdv[c * F + f];
}

// the argument checks and parameter block shared by ltx2_audio_conv (stride_h = 1, act <= LOG) and ltx2_audio_conv2d_strided
int audio_conv_checked(const float* x, int64_t ldx, int h_in, int w_in, int c_in, const float* w, int64_t ldw, const float* bias, float* y,
                       int64_t ldy, int h_out, int w_out, int c_out, int kh, int kw, int stride_h, int stride, int dilation, int pad_h, int pad_w,
                       int upsample, int prologue, float slope, const float* res, int64_t ldres, float alpha, float beta, int act, int act_max,
                       void* stream) {
    LTX2_CHECK_ARG(x && w && y, "audio_conv: null operand");
    LTX2_CHECK_ARG(h_in > 0 && w_in > 0 && c_in > 0 && h_out >= 0 && w_out >= 0 && c_out > 0 && kh > 0 && kw > 0 && stride > 0 && dilation > 0,
                   "audio_conv: h_in %d w_in %d c_in %d h_out %d w_out %d c_out %d kh %d kw %d stride %d dilation %d", h_in, w_in, c_in, h_out,
                   w_out, c_out, kh, kw, stride, dilation);
    LTX2_CHECK_ARG((long)kh * kw * c_in < (1L << 30) && (long)h_out * w_out < (1L << 37), "audio_conv: problem too large");
    LTX2_CHECK_ARG(prologue >= 0 && prologue <= 2 && act >= 0 && act <= act_max, "audio_conv: prologue %d (0..2) / act %d (0..%d)", prologue, act, act_max);
    LTX2_CHECK_ARG(ldw % 4 == 0 && ldw >= c_out && aligned16(w), "audio_conv: the weight rows must be 16-byte aligned with ldw %ld >= c_out %d",
                   (long)ldw, c_out);
    LTX2_CHECK_ARG(ldx >= (prologue == 2 ? 2L * c_in : (long)c_in) && ldy >= c_out && (!res || ldres >= c_out),
                   "audio_conv: a row stride is narrower than its channels (ldx %ld, ldy %ld, ldres %ld)", (long)ldx, (long)ldy, (long)ldres);
    LTX2_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0 && ((uintptr_t)res & 3) == 0 && ((uintptr_t)bias & 3) == 0,
                   "audio_conv: misaligned fp32 operand");
    AudioConvParams p{};
    p.x = x;
    p.ldx = ldx;
    p.h_in = h_in;
    p.w_in = w_in;
    p.c_in = c_in;
    p.w = w;
    p.ldw = ldw;
    p.bias = bias;
    p.y = y;
    p.ldy = ldy;
    p.M = (long)h_out * w_out;
    p.w_out = w_out > 0 ? w_out : 1;
    p.c_out = c_out;
    p.K = kh * kw * c_in;
    p.kw = kw;
    p.ntaps = kh * kw;
    p.stride = stride;
    p.stride_h = stride_h;
    p.dil = dilation;
    p.pad_h = pad_h;
    p.pad_w = pad_w;
    p.up = upsample ? 1 : 0;
    p.pro = prologue;
    p.slope = slope;
    p.res = res;
    p.ldres = ldres;
    p.alpha = alpha;
    p.beta = beta;
    p.act = act;
    return conv_launch(p, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int ltx2_audio_conv(const float* x, int64_t ldx, int h_in, int w_in, int c_in, const float* w, int64_t ldw, const float* bias, float* y,
                    int64_t ldy, int h_out, int w_out, int c_out, int kh, int kw, int stride, int dilation, int pad_h, int pad_w, int upsample,
                    int prologue, float slope, const float* res, int64_t ldres, float alpha, float beta, int act, void* stream) {
    return audio_conv_checked(x, ldx, h_in, w_in, c_in, w, ldw, bias, y, ldy, h_out, w_out, c_out, kh, kw, 1, stride, dilation, pad_h, pad_w, upsample,
                              prologue, slope, res, ldres, alpha, beta, act, LTX2_AUDIO_ACT_LOG, stream);
}

int ltx2_audio_conv2d_strided(const float* x, int64_t ldx, int h_in, int w_in, int c_in, const float* w, int64_t ldw, const float* bias, float* y,
                              int64_t ldy, int h_out, int w_out, int c_out, int kh, int kw, int stride_h, int stride_w, int pad_h, int pad_w,
                              const float* res, int64_t ldres, int act, void* stream) {
    LTX2_CHECK_ARG(stride_h > 0 && stride_w > 0, "audio_conv2d_strided: stride_h %d stride_w %d", stride_h, stride_w);
    // every source row and column an output reads lies inside the padded image: the last output's first tap starts at or before the last row
    LTX2_CHECK_ARG((long)(h_out - 1) * stride_h - pad_h < h_in && (long)(w_out - 1) * stride_w - pad_w < w_in,
                   "audio_conv2d_strided: h_out %d / w_out %d reach past the %d x %d input at stride (%d, %d), pad (%d, %d)", h_out, w_out, h_in, w_in,
                   stride_h, stride_w, pad_h, pad_w);
    LTX2_CHECK_ARG(act == LTX2_AUDIO_ACT_NONE || act == LTX2_AUDIO_ACT_SILU, "audio_conv2d_strided: act %d (NONE or SILU)", act);
    return audio_conv_checked(x, ldx, h_in, w_in, c_in, w, ldw, bias, y, ldy, h_out, w_out, c_out, kh, kw, stride_h, stride_w, 1, pad_h, pad_w, 0,
                              LTX2_AUDIO_PRO_NONE, 0.f, res, ldres, 1.f, 0.f, act, LTX2_AUDIO_ACT_SILU, stream);
}

int ltx2_audio_latent_normalize(const float* h, int64_t ld, const float* mean, const float* std, float* out, int t, int f, int z, void* stream) {
    LTX2_CHECK_ARG(h && mean && std && out, "audio_latent_normalize: null operand");
    LTX2_CHECK_ARG(t >= 0 && f > 0 && z > 0 && ld >= z && (long)t * f * z < (1L << 40), "audio_latent_normalize: t %d f %d z %d ld %ld", t, f, z, (long)ld);
    LTX2_CHECK_ARG(((uintptr_t)h & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)mean & 3) == 0 && ((uintptr_t)std & 3) == 0,
                   "audio_latent_normalize: misaligned fp32 operand");
    const long n = (long)t * f * z;
    if (n == 0) return LTX2_OK;
    hipLaunchKernelGGL(audio_latent_normalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h, (long)ld, mean, std, out, t,
                       f, z);
    LTX2_CHECK_LAUNCH("audio_latent_normalize");
    return LTX2_OK;
}

int ltx2_audio_conv_transpose1d(const float* x, int64_t ldx, int t_in, int c_in, const float* w_phase, const float* bias, float* y, int64_t ldy,
                                int t_out, int c_out, int k, int rate, int padding, int prologue, float slope, void* stream) {
    LTX2_CHECK_ARG(x && w_phase && y, "audio_conv_transpose1d: null operand");
    LTX2_CHECK_ARG(t_in > 0 && c_in > 0 && t_out >= 0 && c_out > 0 && k > 0 && rate > 0 && padding >= 0 && (prologue == 0 || prologue == 1),
                   "audio_conv_transpose1d: t_in %d c_in %d t_out %d c_out %d k %d rate %d padding %d prologue %d", t_in, c_in, t_out, c_out, k,
                   rate, padding, prologue);
    LTX2_CHECK_ARG(t_out <= (long)(t_in - 1) * rate + k - 2 * padding, "audio_conv_transpose1d: t_out %d exceeds (t_in - 1) * rate + k - 2 * padding",
                   t_out);
    LTX2_CHECK_ARG(ldx >= c_in && ldy >= c_out && aligned16(w_phase) && ((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0 && ((uintptr_t)bias & 3) == 0,
                   "audio_conv_transpose1d: misaligned operand or narrow row stride");
    const int ntaps = (k + rate - 1) / rate;
    const int ldw = (c_out + 3) / 4 * 4;
    for (int ph = 0; ph < rate; ++ph) {
        const int o0 = ((ph - padding) % rate + rate) % rate;          // first output of this phase
        if (o0 >= t_out) continue;
        const int q0 = (o0 + padding) / rate;                          // input index of tap m = 0 for output o0
        AudioConvParams p{};
        p.x = x;
        p.ldx = ldx;
        p.h_in = 1;
        p.w_in = t_in;
        p.c_in = c_in;
        p.w = w_phase + (long)ph * ntaps * c_in * ldw;
        p.ldw = ldw;
        p.bias = bias;
        p.y = y + (long)o0 * ldy;
        p.ldy = ldy * rate;
        p.M = (t_out - o0 + rate - 1) / rate;
        p.w_out = (int)p.M;
        p.c_out = c_out;
        p.K = ntaps * c_in;
        p.kw = ntaps;
        p.ntaps = ntaps;
        p.stride = 1;
        p.stride_h = 1;
        p.dil = 1;
        p.pad_h = 0;
        p.pad_w = ntaps - 1 - q0;                                      // tap t reads input n + t - (ntaps - 1 - q0)
        p.pro = prologue;
        p.slope = slope;
        p.alpha = 1.f;
        const int rc = conv_launch(p, (hipStream_t)stream);
        if (rc != LTX2_OK) return rc;
    }
    return LTX2_OK;
}

int ltx2_audio_pixnorm_silu(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int c, float eps, void* stream) {
    LTX2_CHECK_ARG(x && y, "audio_pixnorm_silu: null operand");
    LTX2_CHECK_ARG(rows >= 0 && c > 0 && c % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= c && ldy >= c && aligned16(x) && aligned16(y),
                   "audio_pixnorm_silu: c %d (a multiple of 4) and 16-byte aligned rows (ldx %ld, ldy %ld)", c, (long)ldx, (long)ldy);
    if (rows == 0) return LTX2_OK;
    hipLaunchKernelGGL(audio_pixnorm_silu_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, y, (long)ldy,
                       (long)rows, c, eps);
    LTX2_CHECK_LAUNCH("audio_pixnorm_silu");
    return LTX2_OK;
}

int ltx2_audio_snake_aa(const float* x, int64_t ldx, int t, int c, const float* alpha, const float* beta, const float* up_filter, int up_k,
                        const float* down_filter, int down_k, float* y, int64_t ldy, void* stream) {
    LTX2_CHECK_ARG(x && alpha && beta && up_filter && down_filter && y, "audio_snake_aa: null operand");
    LTX2_CHECK_ARG(t >= 0 && c > 0 && ldx >= c && ldy >= c && up_k >= 2 && up_k <= 16 && up_k % 2 == 0 && down_k >= 1 && down_k <= 16,
                   "audio_snake_aa: t %d c %d up_k %d (even, <= 16) down_k %d (<= 16)", t, c, up_k, down_k);
    LTX2_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "audio_snake_aa: misaligned fp32 operand");
    LTX2_CHECK_ARG(x != y, "audio_snake_aa: in place is not supported (blocks read a halo of neighbouring rows)");
    if (t == 0) return LTX2_OK;
    hipLaunchKernelGGL(audio_snake_aa_kernel, dim3((unsigned)((t + SN_T - 1) / SN_T), (unsigned)((c + SN_C - 1) / SN_C)), dim3(256), 0,
                       (hipStream_t)stream, x, (long)ldx, t, c, alpha, beta, up_filter, up_k, down_filter, down_k, y, (long)ldy);
    LTX2_CHECK_LAUNCH("audio_snake_aa");
    return LTX2_OK;
}

int ltx2_audio_upsample(const float* x, int64_t ldx, int t_in, int c, const float* filter, int k, int ratio, int pad, int pad_left, float* y,
                        int64_t ldy, int t_out, void* stream) {
    LTX2_CHECK_ARG(x && filter && y, "audio_upsample: null operand");
    LTX2_CHECK_ARG(t_in > 0 && c > 0 && k > 0 && ratio > 0 && pad >= 0 && pad_left >= 0 && t_out >= 0 && ldx >= c && ldy >= c && x != y,
                   "audio_upsample: t_in %d c %d k %d ratio %d pad %d pad_left %d t_out %d (out of place)", t_in, c, k, ratio, pad, pad_left, t_out);
    LTX2_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "audio_upsample: misaligned fp32 operand");
    const long n = (long)t_out * c;
    if (n == 0) return LTX2_OK;
    hipLaunchKernelGGL(audio_upsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, t_in, c, filter, k,
                       ratio, pad, pad_left, y, (long)ldy, t_out);
    LTX2_CHECK_LAUNCH("audio_upsample");
    return LTX2_OK;
}

}  // extern "C"
