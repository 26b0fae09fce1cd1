// Guiders whose scalars are reductions over the whole latent (CFGStarRescalingGuider, LtxAPGGuider, LegacyStatefulAPGGuider; reference
// components/guiders.py:51-76, 105-205) as two passes over [rows][C] fp32: ltx2_guidance_sums leaves five fp64 sums per block,
// ltx2_projected_euler_step adds them up in every block and runs the guided step.  All arithmetic is fp32 and fp64, so the file compiles to
// the same code in both library builds.  The definitions are written out in include/ltx2hip.h.
#include <hip/hip_runtime.h>

#include "common.h"
#include "rowops.h"

namespace {

// Individually rounded fp32 operations, as in rowops.hip: operators compiled under contract(off) are never fused into FMAs.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

constexpr int BLOCK = 256, WAVES = BLOCK / 64, NSUM = 5;      // S_aa, S_ab, S_bb, S_gg, S_ga
constexpr int SUMS_CAP = 1024;                                  // every block of the second pass reads all the rows of the first
constexpr int STEP_CAP = 4096;                                  // rowops.hip's grid_for cap

inline int grid_for(long n, int block, int cap) {
    long g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// rows of `partials`: a function of (rows, C) alone, whichever access width the operands' alignment allows
inline int sums_blocks(long n) { return grid_for((n + 3) / 4, BLOCK, SUMS_CAP); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a = x - t*vc, b = x - t*vu, g = a - b, with momentum g = momentum*running + g (not on the first step) stored back to running; the five sums
// per thread in loop order, then across the wave (xor tree), then across the block's waves in order.  V elements per thread (V divides C).
template <int V>
__global__ __launch_bounds__(BLOCK) void guidance_sums_kernel(const float* __restrict__ x, const float* __restrict__ vc, const float* __restrict__ vu,
                                                              const float* __restrict__ ts, long ts_stride, float* running, int first,
                                                              float momentum, double* __restrict__ partials, long n, int C) {
    __shared__ double part[WAVES][NSUM];
    const long nv = n / V;
    double s[NSUM] = {0, 0, 0, 0, 0};
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        const long e = i * V, row = e / C;
        const float t = ts[row * ts_stride];
        alignas(16) float xs[V], cs[V], us[V], rn[V], gs[V];
        if constexpr (V == 4) {
            *(float4*)xs = *(const float4*)(x + e);
            *(float4*)cs = *(const float4*)(vc + e);
            *(float4*)us = *(const float4*)(vu + e);
            *(float4*)rn = (running && !first) ? *(const float4*)(running + e) : float4{0.f, 0.f, 0.f, 0.f};
        } else {
            xs[0] = x[e];
            cs[0] = vc[e];
            us[0] = vu[e];
            rn[0] = (running && !first) ? running[e] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float a = sub_rn(xs[j], mul_rn(t, cs[j]));
            const float b = sub_rn(xs[j], mul_rn(t, us[j]));
            float g = sub_rn(a, b);
            if (running && !first) g = add_rn(mul_rn(momentum, rn[j]), g);
            gs[j] = g;
            const double da = a, db = b, dg = g;                   // each product of two fp32 values is exact in fp64
            s[0] += da * da;
            s[1] += da * db;
            s[2] += db * db;
            s[3] += dg * dg;
            s[4] += dg * da;
        }
        if (running) {
            if constexpr (V == 4) *(float4*)(running + e) = *(const float4*)gs;
            else running[e] = gs[0];
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        const double w = wave_sum_f64(s[k]);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < NSUM) {
        double acc = part[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) acc += part[w][threadIdx.x];
        partials[(long)blockIdx.x * NSUM + threadIdx.x] = acc;
    }
}

struct StepArgs {
    int mode;             // 0 CFG*, 1 APG, 2 legacy APG
    float mult;           // scale - 1 (modes 0, 1) or scale (mode 2)
    float eta, thr, inv, dt;
    int nb;               // rows of partials
};

// g_out of one element from (a, b, g) and the block's fp32 scalars: k0 = coef (mode 0) or sf (modes 1, 2), k1 = proj
__device__ __forceinline__ float projected_one(int mode, float a, float b, float g, float k0, float k1, float mult, float eta) {
    if (mode == 0) return add_rn(a, mul_rn(mult, sub_rn(a, mul_rn(k0, b))));
    const float gsc = mul_rn(g, k0), par = mul_rn(k1, a);
    const float apg = add_rn(mul_rn(par, eta), sub_rn(gsc, par));
    return add_rn(a, mul_rn(apg, mult));
}

// No __restrict__ on x / out: they may be one buffer.  A thread reads its own V elements of every operand before it stores any.
template <int V>
__global__ __launch_bounds__(BLOCK) void projected_euler_step_kernel(const float* x, const float* __restrict__ vc, const float* __restrict__ vu,
                                                                     const float* __restrict__ ts, long ts_stride, const float* __restrict__ mask,
                                                                     const float* __restrict__ clean, const float* __restrict__ running,
                                                                     const double* __restrict__ partials, StepArgs p, float* out, float* scalars_out,
                                                                     long n, int C) {
    __shared__ double sums[NSUM];
    __shared__ float sc[2];
    if (threadIdx.x < NSUM) {                                      // the partial rows in index order: every block holds the same five sums
        double acc = 0.0;
        for (int r = 0; r < p.nb; ++r) acc += partials[(long)r * NSUM + threadIdx.x];
        sums[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                        // fp64 throughout, each scalar rounded once
        float k0, k1 = 0.f;
        if (p.mode == 0) {
            k0 = (float)(sums[1] / (sums[2] + 1e-8));
        } else {
            double sf = 1.0;
            if (p.thr > 0.f) sf = fmin(1.0, (double)p.thr / sqrt(sums[3]));
            k0 = (float)sf;
            k1 = (float)(sf * sums[4] / (sums[0] + 1e-8));
        }
        sc[0] = k0;
        sc[1] = k1;
        if (blockIdx.x == 0 && scalars_out) {
            scalars_out[0] = k0;
            if (p.mode != 0) scalars_out[1] = k1;
        }
    }
    __syncthreads();
    const float k0 = sc[0], k1 = sc[1];
    const bool blend = mask != nullptr;
    const long nv = n / V;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        const long e = i * V, row = e / C;
        const float t = ts[row * ts_stride];
        const float m = blend ? mask[row] : 1.f, om = sub_rn(1.0f, m);
        alignas(16) float xs[V], cs[V], us[V], cl[V], rn[V], o[V];
        if constexpr (V == 4) {
            *(float4*)xs = *(const float4*)(x + e);
            *(float4*)cs = *(const float4*)(vc + e);
            *(float4*)us = *(const float4*)(vu + e);
            *(float4*)cl = blend ? *(const float4*)(clean + e) : float4{0.f, 0.f, 0.f, 0.f};
            *(float4*)rn = running ? *(const float4*)(running + e) : float4{0.f, 0.f, 0.f, 0.f};
        } else {
            xs[0] = x[e];
            cs[0] = vc[e];
            us[0] = vu[e];
            cl[0] = blend ? clean[e] : 0.f;
            rn[0] = running ? running[e] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float a = sub_rn(xs[j], mul_rn(t, cs[j]));
            const float b = sub_rn(xs[j], mul_rn(t, us[j]));
            const float g = running ? rn[j] : sub_rn(a, b);
            float d = projected_one(p.mode, a, b, g, k0, k1, p.mult, p.eta);
            if (blend) d = add_rn(mul_rn(d, m), mul_rn(cl[j], om));
            o[j] = add_rn(xs[j], mul_rn(mul_rn(sub_rn(xs[j], d), p.inv), p.dt));
        }
        if constexpr (V == 4) *(float4*)(out + e) = *(const float4*)o;
        else out[e] = o[0];
    }
}

}  // namespace

int guidance_sums_blocks(int rows, int C) { return (rows > 0 && C > 0) ? sums_blocks((long)rows * C) : 0; }

int guidance_sums_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, float* running, int first,
                         float momentum, double* partials, int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(x && vel_cond && vel_uncond && ts && partials && rows > 0 && C > 0, "guidance_sums: null operand or empty shape");
    LTX2_CHECK_ARG(ts_stride == 0 || ts_stride == 1, "guidance_sums: ts_stride is 0 (one timestep) or 1 (one per row)");
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "guidance_sums: partials must be 8-byte aligned");
    const long n = (long)rows * C;
    const int nb = sums_blocks(n);
    // 16-byte accesses need every [rows][C] operand on a 16-byte boundary as well as C % 4 == 0 (a NULL operand contributes no bits)
    const uintptr_t al = (uintptr_t)x | (uintptr_t)vel_cond | (uintptr_t)vel_uncond | (uintptr_t)running;
    if (C % 4 == 0 && (al & 15) == 0)
        hipLaunchKernelGGL(guidance_sums_kernel<4>, dim3(nb), dim3(BLOCK), 0, stream, x, vel_cond, vel_uncond, ts, ts_stride, running, first, momentum,
                           partials, n, C);
    else
        hipLaunchKernelGGL(guidance_sums_kernel<1>, dim3(nb), dim3(BLOCK), 0, stream, x, vel_cond, vel_uncond, ts, ts_stride, running, first, momentum,
                           partials, n, C);
    LTX2_CHECK_LAUNCH("guidance_sums_kernel");
    return LTX2_OK;
}

int projected_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                                const float* clean, const float* running, const double* partials, int mode, float scale, float eta,
                                float norm_threshold, float sigma, float sigma_next, float* out, float* scalars_out, int rows, int C,
                                hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    LTX2_CHECK_ARG(x && vel_cond && vel_uncond && ts && partials && out && rows > 0 && C > 0, "projected_euler_step: null operand or empty shape");
    LTX2_CHECK_ARG(ts_stride == 0 || ts_stride == 1, "projected_euler_step: ts_stride is 0 (one timestep) or 1 (one per row)");
    LTX2_CHECK_ARG((mask == nullptr) == (clean == nullptr), "projected_euler_step: mask and clean go together");
    LTX2_CHECK_ARG(mode >= 0 && mode <= 2, "projected_euler_step: mode=%d is 0 (CFG*), 1 (APG) or 2 (legacy APG)", mode);
    LTX2_CHECK_ARG(running == nullptr || mode == 2, "projected_euler_step: only mode 2 (legacy APG with momentum) reads a running buffer");
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "projected_euler_step: partials must be 8-byte aligned");
    const long n = (long)rows * C;
    const StepArgs p = {mode, mode == 2 ? scale : scale - 1.0f, eta, norm_threshold, 1.0f / sigma, sigma_next - sigma, sums_blocks(n)};
    const uintptr_t al = (uintptr_t)x | (uintptr_t)vel_cond | (uintptr_t)vel_uncond | (uintptr_t)clean | (uintptr_t)running | (uintptr_t)out;
    if (C % 4 == 0 && (al & 15) == 0)
        hipLaunchKernelGGL(projected_euler_step_kernel<4>, dim3(grid_for(n / 4, BLOCK, STEP_CAP)), dim3(BLOCK), 0, stream, x, vel_cond, vel_uncond, ts,
                           ts_stride, mask, clean, running, partials, p, out, scalars_out, n, C);
    else
        hipLaunchKernelGGL(projected_euler_step_kernel<1>, dim3(grid_for(n, BLOCK, STEP_CAP)), dim3(BLOCK), 0, stream, x, vel_cond, vel_uncond, ts,
                           ts_stride, mask, clean, running, partials, p, out, scalars_out, n, C);
    LTX2_CHECK_LAUNCH("projected_euler_step_kernel");
    return LTX2_OK;
}
