// GroupNorm (+ residual, + SiLU) of the latent upscalers on channels-last 16-bit activations, for gfx950:
//   groupnorm_silu         spatial upscaler: statistics per group over all positions (stats -> finish -> apply, fp32)
//   groupnorm_frames_silu  temporal upscaler: statistics per (frame, group), contiguous or interleaved groups (one launch, fp64 in LDS;
//                          the slab form and the element-wise form for what it cannot tile)
// No atomics and a fixed summation order in both: repeated launches are bit-identical.  The reference runs mlx.nn.GroupNorm
// (interleaved groups by default); rowops.h states what each launcher computes.
#include "rowops.h"

namespace {

// ---- GroupNorm (spatial upscaler): statistics over (C/G channels x all positions) per group ----
// Deterministic two-level reduction (no atomics, fixed summation order => bit-reproducible statistics):
// block b reduces rows [16b, 16b+16) to per-channel sums in LDS (every channel has exactly one owner thread),
// then to per-group partials partial[b][2G]; groupnorm_finish_kernel folds the partials in a fixed tree.
__global__ __launch_bounds__(256) void groupnorm_stats_kernel(const bf16* __restrict__ x, float* __restrict__ partial, long P,
                                                              int C, int G, int rows_per_block) {
    __shared__ float ch1[2048], ch2[2048];
    const int cpg = C / G;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = r0 + rows_per_block < P ? r0 + rows_per_block : P;
    const int vec_per_row = C / 4;
    for (int v = threadIdx.x; v < vec_per_row; v += 256) {
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        for (long r = r0; r < r1; ++r) {
            const bf16x4 q = *(const bf16x4*)(x + r * C + v * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float f = bf2f(q[e]);
                s1[e] += f;
                s2[e] += f * f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ch1[v * 4 + e] = s1[e];
            ch2[v * 4 + e] = s2[e];
        }
    }
    __syncthreads();
    if (threadIdx.x < G) {
        float a = 0.f, b = 0.f;
        for (int c = threadIdx.x * cpg; c < (threadIdx.x + 1) * cpg; ++c) {
            a += ch1[c];
            b += ch2[c];
        }
        partial[(long)blockIdx.x * 2 * G + threadIdx.x] = a;
        partial[(long)blockIdx.x * 2 * G + G + threadIdx.x] = b;
    }
}

// sums[k] = sum_b partial[b][k], k < 2G: one block per k, strided serial sums + fixed-order LDS tree
__global__ __launch_bounds__(256) void groupnorm_finish_kernel(const float* __restrict__ partial, float* __restrict__ sums,
                                                               int nblk, int G2) {
    __shared__ float red[256];
    const int k = blockIdx.x;
    float a = 0.f;
    for (int b = threadIdx.x; b < nblk; b += 256) a += partial[(long)b * G2 + k];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[k] = red[0];
}

__global__ __launch_bounds__(256) void groupnorm_apply_kernel(const bf16* __restrict__ x, const bf16* __restrict__ res,
                                                              bf16* __restrict__ y, const float* __restrict__ sums,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              long n4, int C, int G, float inv_count, float eps, int act) {
    const int cpg = C / G;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)((i * 4) % C);
        float mean[4], rstd[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int g = (c + e) / cpg;
            mean[e] = sums[g] * inv_count;
            rstd[e] = rsqrtf(fmaxf(sums[G + g] * inv_count - mean[e] * mean[e], 0.f) + eps);
        }
        const bf16x4 q = *(const bf16x4*)(x + i * 4);
        const f32x4 ga = *(const f32x4*)(gamma + c), be = *(const f32x4*)(beta + c);
        bf16x4 r4 = {f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
        if (res) r4 = *(const bf16x4*)(res + i * 4);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = (bf2f(q[e]) - mean[e]) * rstd[e] * ga[e] + be[e] + bf2f(r4[e]);
            o[e] = f2bf(act ? silu_f(v) : v);
        }
        *(bf16x4*)(y + i * 4) = o;
    }
}

// ---- per-frame GroupNorm (temporal upscaler): statistics per (frame, group), contiguous or interleaved groups ----
// x[frames][P][C]; group of channel c = c % G (interleaved, mlx.nn.GroupNorm's default) or c / (C/G) (contiguous).
// One launch, one workgroup per (frame, slab).  A slab is a set of whole groups whose channels are, at every position,
// `nvec` aligned V-element vectors `vstride` channels apart starting at channel slab * slab_c:
//   contiguous : slab_c consecutive channels (a multiple of lcm(C/G, V)), vstride = V
//   interleaved: the V groups slab*V .. slab*V + V-1, i.e. channels j*G + slab*V + e (j < C/G), vstride = G
// Thread t owns vector i = t % nvec of the positions r, r + R, r + 2R, ... (r = t / nvec, R = 256 / nvec), so the group of
// each of its V elements is fixed.  REG: the thread's <= GNF_NV vectors stay in registers between the sums and the apply (one
// HBM read); otherwise x is read twice.  Sums, mean, rstd and the affine run in fp64 on the 16-bit inputs: every x and x^2
// is exact there and the sums round at 2^-53 (not at all while a group's magnitudes span less than ~2^15), so E[x^2] - mean^2
// keeps ~1e-16 * mean^2 / var and v = x*a + b + res carries ~1e-16 into the one rounding on store, whatever beta + res cancels:
// the one-ulp bound of the 16-bit output needs |error before rounding| < ulp / 2 also where |v| is 1e-4 of its terms, which
// fp32 statistics (mean good to 6e-8 |mean|) cannot give.  The kernel stays bound by its loads and stores (rowops_time / DESIGN.md).  Fixed summation order, no atomics: repeated launches are bit-identical.
constexpr int GNF_NV = 24;

template <int V>
struct GnfVec {
    typedef bf16 type __attribute__((ext_vector_type(V)));
};

struct GnfParams {
    const bf16* x;
    const bf16* res;
    bf16* y;
    const float* gamma;
    const float* beta;
    long P;            // positions per frame
    int C, G, cpg, interleaved, act;
    int slabs, slab_c, nvec, vstride, R;
    float eps;
};

template <int V, bool REG>
__global__ __launch_bounds__(256) void groupnorm_frames_kernel(const GnfParams p) {
    typedef typename GnfVec<V>::type vec_t;
    __shared__ double part1[2048], part2[2048];      // [r][i*V + e], R * nvec <= 256
    __shared__ double g_mean[64], g_rstd[64];
    // the slabs of one frame are neighbours in the logical order: on one XCD they share an L2 (interleaved slabs share every cache line)
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int frame = bid / p.slabs, slab = bid % p.slabs;
    const int i = threadIdx.x % p.nvec, r = threadIdx.x / p.nvec;
    const bool active = r < p.R;
    const int c_first = slab * p.slab_c + i * p.vstride;                    // channel of element 0 of this thread's vectors
    const long base = (long)frame * p.P * p.C + c_first;
    const int W = p.nvec * V;                                               // channels of the slab

    vec_t xv[REG ? GNF_NV : 1];
    double s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s1[e] = s2[e] = 0.0;
    if (active) {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < GNF_NV; ++k) {
                const long pos = r + (long)k * p.R;
                if (pos < p.P) {
                    xv[k] = *(const vec_t*)(p.x + base + pos * p.C);
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const double f = (double)bf2f(xv[k][e]);
                        s1[e] += f;
                        s2[e] += f * f;
                    }
                }
            }
        } else {
            for (long pos = r; pos < p.P; pos += p.R) {
                const vec_t q = *(const vec_t*)(p.x + base + pos * p.C);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const double f = (double)bf2f(q[e]);
                    s1[e] += f;
                    s2[e] += f * f;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            part1[r * W + i * V + e] = s1[e];
            part2[r * W + i * V + e] = s2[e];
        }
    }
    __syncthreads();
    // per-channel sums: column j of part[r][j] folded over r in order, left in row 0
    for (int j = threadIdx.x; j < W; j += 256) {
        double a = part1[j], b = part2[j];
        for (int rr = 1; rr < p.R; ++rr) {
            a += part1[rr * W + j];
            b += part2[rr * W + j];
        }
        part1[j] = a;
        part2[j] = b;
    }
    __syncthreads();
    // per-group statistics: local group lg owns slab columns lg*cpg + q (contiguous) or q*V + lg (interleaved), q < cpg
    const int lgroups = W / p.cpg;
    if (threadIdx.x < lgroups) {
        const int lg = threadIdx.x;
        double a = 0.0, b = 0.0;
        for (int q = 0; q < p.cpg; ++q) {
            const int j = p.interleaved ? q * V + lg : lg * p.cpg + q;
            a += part1[j];
            b += part2[j];
        }
        const double n = (double)p.P * (double)p.cpg;
        const double mean = a / n;
        const double var = fmax(b / n - mean * mean, 0.0);
        g_mean[lg] = mean;
        g_rstd[lg] = 1.0 / sqrt(var + (double)p.eps);
    }
    __syncthreads();
    if (!active) return;
    double ca[V], cb[V];                                                    // v = x * ca + cb (+ res)
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int lg = p.interleaved ? e : (i * V + e) / p.cpg;
        ca[e] = g_rstd[lg] * (double)p.gamma[c_first + e];
        cb[e] = (double)p.beta[c_first + e] - g_mean[lg] * ca[e];
    }
    auto apply = [&](const vec_t q, long off) {
        vec_t o;
        if (p.res) {
            const vec_t rq = *(const vec_t*)(p.res + off);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float v = (float)(fma((double)bf2f(q[e]), ca[e], cb[e]) + (double)bf2f(rq[e]));
                o[e] = f2bf(p.act ? silu_f(v) : v);
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float v = (float)fma((double)bf2f(q[e]), ca[e], cb[e]);
                o[e] = f2bf(p.act ? silu_f(v) : v);
            }
        }
        *(vec_t*)(p.y + off) = o;
    };
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < GNF_NV; ++k) {
            const long pos = r + (long)k * p.R;
            if (pos < p.P) apply(xv[k], base + pos * p.C);
        }
    } else {
        for (long pos = r; pos < p.P; pos += p.R) apply(*(const vec_t*)(p.x + base + pos * p.C), base + pos * p.C);
    }
}

// Any (C, G, mode) the slab form cannot tile (e.g. interleaved groups with G % 4 != 0): one workgroup per (frame, group),
// element-wise 16-bit accesses, x read twice.  Same arithmetic and the same fixed order.
__global__ __launch_bounds__(256) void groupnorm_frames_scalar_kernel(const GnfParams p) {
    __shared__ double red[8];
    const int frame = blockIdx.x / p.G, g = blockIdx.x % p.G;
    const long base = (long)frame * p.P * p.C;
    const long n = p.P * p.cpg;
    auto offset = [&](long idx) {
        const long pos = idx / p.cpg;
        const int q = (int)(idx % p.cpg);
        return base + pos * p.C + (p.interleaved ? q * p.G + g : g * p.cpg + q);
    };
    double a = 0.0, b = 0.0;
    for (long idx = threadIdx.x; idx < n; idx += 256) {
        const double f = (double)bf2f(p.x[offset(idx)]);
        a += f;
        b += f * f;
    }
    block_sum2_256<false>(a, b, red);
    const double mean = a / (double)n;
    const double rstd = 1.0 / sqrt(fmax(b / (double)n - mean * mean, 0.0) + (double)p.eps);
    for (long idx = threadIdx.x; idx < n; idx += 256) {
        const long off = offset(idx);
        const int c = (int)((off - base) % p.C);
        const double ca = rstd * (double)p.gamma[c];
        double v = fma((double)bf2f(p.x[off]), ca, (double)p.beta[c] - mean * ca);
        if (p.res) v += (double)bf2f(p.res[off]);
        p.y[off] = f2bf(p.act ? silu_f((float)v) : (float)v);
    }
}

}  // namespace

int groupnorm_silu_launch(const bf16* x, const bf16* res, bf16* y, long P, int C, int G, float eps, const float* gamma,
                          const float* beta, float* scratch, int act, hipStream_t stream) {
    LTX2_CHECK_ARG(x && y && gamma && beta && scratch && P > 0, "groupnorm: null operand");
    LTX2_CHECK_ARG(G >= 1 && G <= 64 && C % G == 0 && C % 4 == 0 && C <= 2048, "groupnorm: need groups <= 64, C %% groups == 0, C %% 4 == 0, C <= 2048 (C=%d, groups=%d)", C, G);
    const int rows_per_block = 16;
    const int nblk = (int)((P + rows_per_block - 1) / rows_per_block);
    float* sums = scratch;                 // [2G]
    float* partial = scratch + 2 * G;      // [nblk][2G]
    hipLaunchKernelGGL(groupnorm_stats_kernel, dim3(nblk), dim3(256), 0, stream, x, partial, P, C, G, rows_per_block);
    LTX2_CHECK_LAUNCH("groupnorm_stats_kernel");
    hipLaunchKernelGGL(groupnorm_finish_kernel, dim3(2 * G), dim3(256), 0, stream, partial, sums, nblk, 2 * G);
    LTX2_CHECK_LAUNCH("groupnorm_finish_kernel");
    const long n4 = P * C / 4;
    hipLaunchKernelGGL(groupnorm_apply_kernel, dim3(grid_for(n4, 256, 8192)), dim3(256), 0, stream, x, res, y, sums, gamma, beta, n4, C, G,
                       1.0f / ((float)P * (float)(C / G)), eps, act);
    LTX2_CHECK_LAUNCH("groupnorm_apply_kernel");
    return LTX2_OK;
}

int groupnorm_frames_silu_launch(const bf16* x, const bf16* res, bf16* y, int frames, long P_frame, int C, int G, int interleaved,
                                 float eps, const float* gamma, const float* beta, float* scratch, int act, hipStream_t stream) {
    (void)scratch;      // every reduction of this entry lives in LDS; the argument keeps the call shape of groupnorm_silu_launch
    LTX2_CHECK_ARG(x && y && gamma && beta && P_frame > 0 && frames > 0, "groupnorm_frames: null operand");
    LTX2_CHECK_ARG(G >= 1 && G <= 64 && C % G == 0 && C % 4 == 0 && C <= 2048, "groupnorm_frames: need groups <= 64, C %% groups == 0, C %% 4 == 0, C <= 2048 (C=%d, groups=%d)", C, G);
    GnfParams p;
    p.x = x, p.res = res, p.y = y, p.gamma = gamma, p.beta = beta;
    p.P = P_frame, p.C = C, p.G = G, p.cpg = C / G, p.interleaved = interleaved ? 1 : 0, p.act = act, p.eps = eps;
    // slab geometry (see groupnorm_frames_kernel); V = 0: no aligned tiling, element-wise form
    int V = 0;
    if (p.interleaved) {
        V = (C % 8 == 0 && G % 8 == 0) ? 8 : (G % 4 == 0 ? 4 : 0);
        if (V) p.slabs = G / V, p.slab_c = V, p.nvec = p.cpg, p.vstride = G;
    } else {
        V = C % 8 == 0 ? 8 : 4;
        int a = p.cpg, b = V;
        while (b) { const int t = a % b; a = b; b = t; }
        const int lcm = p.cpg / a * V;              // divides C: C is a multiple of both
        int m = 1;
        for (int d = 1; d <= C / lcm && lcm * d <= 64; ++d)
            if ((C / lcm) % d == 0) m = d;          // widest slab of <= 64 channels (128 bytes per position) that divides C
        p.slab_c = lcm * m, p.slabs = C / p.slab_c, p.nvec = p.slab_c / V, p.vstride = V;
    }
    if (V && p.nvec > 256) V = 0;
    if (!V) {
        LTX2_CHECK_ARG((long)frames * G <= 0x7fffffffL, "groupnorm_frames: frames * groups = %ld workgroups exceed the grid", (long)frames * G);
        hipLaunchKernelGGL(groupnorm_frames_scalar_kernel, dim3(frames * G), dim3(256), 0, stream, p);
        LTX2_CHECK_LAUNCH("groupnorm_frames_scalar_kernel");
        return LTX2_OK;
    }
    p.R = 256 / p.nvec;
    LTX2_CHECK_ARG((long)frames * p.slabs <= 0x7fffffffL, "groupnorm_frames: frames * slabs = %ld workgroups exceed the grid", (long)frames * p.slabs);
    const dim3 grid(frames * p.slabs), block(256);
    const bool reg = (P_frame + p.R - 1) / p.R <= GNF_NV;
    if (V == 8) {
        if (reg) hipLaunchKernelGGL((groupnorm_frames_kernel<8, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((groupnorm_frames_kernel<8, false>), grid, block, 0, stream, p);
    } else {
        if (reg) hipLaunchKernelGGL((groupnorm_frames_kernel<4, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((groupnorm_frames_kernel<4, false>), grid, block, 0, stream, p);
    }
    LTX2_CHECK_LAUNCH("groupnorm_frames_kernel");
    return LTX2_OK;
}
