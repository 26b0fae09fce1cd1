// First-block cache: the metric over block 0's residual and the two kernels that store and re-apply the residual of blocks 1..L-1.  All three are
// bandwidth-bound passes over the fp32 residual stream; arithmetic is fp32 (one rounded operation per element) and fp64 (the sums), so the file
// compiles to the same code in both library builds.  The definitions are written out in fbc.h and include/ltx2hip.h.
#include <hip/hip_runtime.h>

#include "common.h"
#include "fbc.h"

namespace {

constexpr int BLOCK = 256;
constexpr long QUADS_PER_BLOCK = 2048;          // 8 quads per thread before the grid is capped

// the block's 256 (a, b) pairs added by a fixed binary tree; the result is thread 0's
__device__ __forceinline__ void block_tree_sum2(double& a, double& b, double (*red)[BLOCK]) {
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
#pragma unroll
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[1][0];
}

// V = 4: every operand is 16-byte aligned, a full quad is one float4 access; V = 1: element-wise accesses.  Which thread adds which element, and in
// which order, is the same in both.
template <int V>
__global__ __launch_bounds__(BLOCK) void fbc_head_metric_kernel(const float* h0, const float* __restrict__ h1, const float* __restrict__ head_prev,
                                                                float* __restrict__ r, float* h1_save, double* __restrict__ partials, long n) {
    __shared__ double red[2][BLOCK];
    const long nq = (n + 3) / 4;
    double num = 0.0, den = 0.0;
    for (long q = (long)blockIdx.x * BLOCK + threadIdx.x; q < nq; q += (long)gridDim.x * BLOCK) {
        const long e = q * 4;
        const int cnt = (n - e) >= 4 ? 4 : (int)(n - e);
        alignas(16) float a[4] = {}, b[4] = {}, p[4] = {}, d[4];
        if (V == 4 && cnt == 4) {
            *(float4*)a = *(const float4*)(h0 + e);
            *(float4*)b = *(const float4*)(h1 + e);
            if (head_prev) *(float4*)p = *(const float4*)(head_prev + e);
        } else {
            for (int j = 0; j < cnt; ++j) {
                a[j] = h0[e + j];
                b[j] = h1[e + j];
                if (head_prev) p[j] = head_prev[e + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = sub_rn(b[j], a[j]);
            if (j < cnt) {
                num += fabs((double)d[j] - (double)p[j]);
                den += fabs((double)p[j]);
            }
        }
        if (V == 4 && cnt == 4) {
            *(float4*)(r + e) = *(const float4*)d;
            if (h1_save) *(float4*)(h1_save + e) = *(const float4*)b;
        } else {
            for (int j = 0; j < cnt; ++j) {
                r[e + j] = d[j];
                if (h1_save) h1_save[e + j] = b[j];
            }
        }
    }
    block_tree_sum2(num, den, red);
    if (threadIdx.x == 0) {
        partials[2L * blockIdx.x] = num;
        partials[2L * blockIdx.x + 1] = den;
    }
}

// one block: thread t adds the partials t, t + 256, ... in index order, then the tree
__global__ __launch_bounds__(BLOCK) void fbc_decide_kernel(const double* __restrict__ partials, int nb, float threshold, FbcRecord* __restrict__ rec) {
    __shared__ double red[2][BLOCK];
    double num = 0.0, den = 0.0;
    for (int b = threadIdx.x; b < nb; b += BLOCK) {
        num += partials[2L * b];
        den += partials[2L * b + 1];
    }
    block_tree_sum2(num, den, red);
    if (threadIdx.x == 0) {
        rec->num = num;
        rec->den = den;
        rec->skip = (threshold > 0.f && den > 0.0 && num < (double)threshold * den) ? 1 : 0;
        rec->pad = 0;
    }
}

// out = a - b (SUB) or a + b; out may be a
template <int V, bool SUB>
__global__ __launch_bounds__(BLOCK) void fbc_combine_kernel(const float* a, const float* __restrict__ b, float* out, long n) {
    const long nv = n / V;
    for (long i = (long)blockIdx.x * BLOCK + threadIdx.x; i < nv; i += (long)gridDim.x * BLOCK) {
        if constexpr (V == 4) {
            const float4 x = *(const float4*)(a + i * 4), y = *(const float4*)(b + i * 4);
            float4 o;
            o.x = SUB ? sub_rn(x.x, y.x) : add_rn(x.x, y.x);
            o.y = SUB ? sub_rn(x.y, y.y) : add_rn(x.y, y.y);
            o.z = SUB ? sub_rn(x.z, y.z) : add_rn(x.z, y.z);
            o.w = SUB ? sub_rn(x.w, y.w) : add_rn(x.w, y.w);
            *(float4*)(out + i * 4) = o;
        } else {
            out[i] = SUB ? sub_rn(a[i], b[i]) : add_rn(a[i], b[i]);
        }
    }
}

template <bool SUB>
int combine_launch(const char* who, const float* a, const float* b, float* out, long n, hipStream_t stream) {
    LTX2_CHECK_ARG(a && b && out && n > 0, "%s: null operand or empty shape", who);
    LTX2_CHECK_ARG((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3) == 0, "%s: operands must be 4-byte aligned", who);
    const bool v4 = n % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0;
    if (v4) hipLaunchKernelGGL((fbc_combine_kernel<4, SUB>), dim3(grid_for(n / 4, BLOCK)), dim3(BLOCK), 0, stream, a, b, out, n);
    else hipLaunchKernelGGL((fbc_combine_kernel<1, SUB>), dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, stream, a, b, out, n);
    LTX2_CHECK_LAUNCH(who);
    return LTX2_OK;
}

}  // namespace

int fbc_metric_blocks(long n) {
    if (n <= 0) return 0;
    const long nq = (n + 3) / 4, nb = (nq + QUADS_PER_BLOCK - 1) / QUADS_PER_BLOCK;
    return (int)(nb > FBC_MAX_BLOCKS ? FBC_MAX_BLOCKS : nb);
}

int fbc_head_metric_launch(const float* h0, const float* h1, const float* head_prev, float* r, float* h1_save, double* partials, FbcRecord* rec,
                           float threshold, long n, hipStream_t stream) {
    LTX2_CHECK_ARG(h0 && h1 && r && partials && rec && n > 0, "fbc_head_metric: null operand or empty shape");
    LTX2_CHECK_ARG(threshold >= 0.f, "fbc_head_metric: threshold=%g must be >= 0", threshold);
    uintptr_t bits = (uintptr_t)h0 | (uintptr_t)h1 | (uintptr_t)head_prev | (uintptr_t)r | (uintptr_t)h1_save;
    LTX2_CHECK_ARG((bits & 3) == 0 && (((uintptr_t)partials | (uintptr_t)rec) & 7) == 0,
                   "fbc_head_metric: fp32 operands must be 4-byte, partials and the record 8-byte aligned");
    const int nb = fbc_metric_blocks(n);
    if ((bits & 15) == 0)
        hipLaunchKernelGGL((fbc_head_metric_kernel<4>), dim3(nb), dim3(BLOCK), 0, stream, h0, h1, head_prev, r, h1_save, partials, n);
    else
        hipLaunchKernelGGL((fbc_head_metric_kernel<1>), dim3(nb), dim3(BLOCK), 0, stream, h0, h1, head_prev, r, h1_save, partials, n);
    LTX2_CHECK_LAUNCH("fbc_head_metric_kernel");
    hipLaunchKernelGGL(fbc_decide_kernel, dim3(1), dim3(BLOCK), 0, stream, partials, nb, threshold, rec);
    LTX2_CHECK_LAUNCH("fbc_decide_kernel");
    return LTX2_OK;
}

int fbc_store_tail_launch(const float* hL, const float* h1, float* tail, long n, hipStream_t stream) {
    return combine_launch<true>("fbc_store_tail", hL, h1, tail, n, stream);
}

int fbc_apply_tail_launch(float* h, const float* tail, long n, hipStream_t stream) { return combine_launch<false>("fbc_apply_tail", h, tail, h, n, stream); }
