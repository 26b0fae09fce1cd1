// The device code of the sampling step over fp32 [rows][C] latents: the plain x0 / Euler pair, and the steps that replace a sequence of separate
// fp32 torch ops bit for bit -- the classifier-free-guided Euler step (pipelines/one_stage.py:224-330), the same with STG guidance on top, the two passes of the res_2s second-order
// step (reference pipelines/ti2vid_hq.py:153-273; over one latent, or over the video and the audio latent of the joint step in one launch) and the two passes of the guiders whose scalars are reductions over the whole latent
// (CFGStarRescalingGuider, LtxAPGGuider, LegacyStatefulAPGGuider; reference components/guiders.py:51-76, 105-205), and the multi-modal guided step
// (MultiModalGuider.calculate, :244-273: CFG, STG and modality-isolated terms, with or without the variance rescale), and the two passes of the Heun
// sampler with the GE velocity correction (pipelines/one_stage.py:300-307, 334-464), and the guided step of the standard one-stage loop with its
// per-channel rescale and the two kernels of its statistics (reference scripts/generate.py:688-727, 1895-1976).  All arithmetic is fp32 and
// fp64, so the file compiles to the same code in both library builds.  The definitions are written out in include/ltx2hip.h.
#include <hip/hip_runtime.h>

#include "common.h"
#include "sampler.h"

namespace {

// ---------------------------------- the plain step: contracted arithmetic, bounded (not bit-exact) against its reference ----------------------------------
// Its two fused operations, written out so that no compiler decision stands between the kernels below and the unguided ancestral step, which
// shares them: x0 = fma(-t, v, x) and x + ((x - d)*inv)*dt with the last product and sum fused.  The mask / clean blend is rounded per operation.
__device__ __forceinline__ float plain_denoised(float x, float v, float t) { return fmaf(-t, v, x); }
__device__ __forceinline__ float plain_euler(float x, float d, float inv, float dt) { return fmaf(mul_rn(sub_rn(x, d), inv), dt, x); }

__global__ void x0_from_velocity_kernel(const float* __restrict__ latent, const float* __restrict__ vel,
                                        const float* __restrict__ ts_ptr, long ts_stride, float ts_scalar,
                                        float* __restrict__ x0, int rows, int C) {
    const long n = (long)rows * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C;
        const float ts = ts_ptr ? ts_ptr[row * ts_stride] : ts_scalar;
        x0[i] = plain_denoised(latent[i], vel[i], ts);
    }
}

__global__ void euler_step_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                  const float* __restrict__ mask, const float* __restrict__ clean, float inv_sigma,
                                  float dt, float* __restrict__ out, int rows, int C) {
    const long n = (long)rows * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float d = x0[i];
        if (mask) {
            const float m = mask[i / C];
            d = add_rn(mul_rn(d, m), mul_rn(clean[i], sub_rn(1.f, m)));
        }
        out[i] = plain_euler(x[i], d, inv_sigma, dt);
    }
}

// ---------------------------------- the individually rounded steps: one scaffold ----------------------------------
// A step is an Op: NIN operands `in` and NOUT operands `out`, all [rows][C], and one(): the arithmetic of one element, a[k] read from in[k] and
// o[k] stored to out[k], every operation rounded on its own (mul_rn / add_rn / sub_rn) in the order of the torch statements it replaces.  A NULL
// `in` reads as zeros and a NULL `out` is not stored.  begin() / end() run once per thread around the loop with the thread's State and the block's
// index within its own grid (a segment's index in a two-segment launch).
//
// Aliasing: any `out` may be the same buffer as any `in` (the engine updates the latent in place).  So no [rows][C] operand is __restrict__, and a
// thread loads its V elements of EVERY operand before it stores any; V divides C, so a vector never straddles a row.
constexpr int BLOCK = 256, WAVES = BLOCK / 64;

struct Rows {           // what every step reads per row, and the shape
    const float* ts;    // t = ts[row * ts_stride]
    long ts_stride;
    const float* mask;  // m = mask[row], or NULL: m = 1 and no blend
    long n;             // rows * C
    int C;
};
struct Row {
    float t, m, one_minus_m;
    bool blend;
    int col;            // the element's channel (only the step with per-channel statistics reads it)
    long e;             // the element's index row*C + col (only the steps with noise read it)
};

template <int V>
__device__ __forceinline__ void load(const float* p, long e, float (&v)[V]) {
    if constexpr (V == 4) *(float4*)v = p ? *(const float4*)(p + e) : float4{0.f, 0.f, 0.f, 0.f};
    else v[0] = p ? p[e] : 0.f;
}
template <int V>
__device__ __forceinline__ void store(float* p, long e, const float (&v)[V]) {
    if (!p) return;
    if constexpr (V == 4) *(float4*)(p + e) = *(const float4*)v;
    else p[e] = v[0];
}

// the loop of one block over the vectors of r, as block `block` of `blocks`
template <int V, class Op>
__device__ __forceinline__ void step_rows(const Op& op, const Rows& r, long block, long blocks) {
    typename Op::State st;
    op.begin(st, block);
    const bool blend = r.mask != nullptr;
    const long nv = r.n / V;
    for (long i = block * blockDim.x + threadIdx.x; i < nv; i += blocks * blockDim.x) {
        const long e = i * V, row = e / r.C;
        const float m = blend ? r.mask[row] : 1.f;
        Row rw = {Op::reads_t ? r.ts[row * r.ts_stride] : 0.f, m, sub_rn(1.0f, m), blend, 0, 0};
        const int col = (int)(e - row * r.C);
        alignas(16) float in[Op::NIN][V], out[Op::NOUT][V];
#pragma unroll
        for (int k = 0; k < Op::NIN; ++k) load<V>(op.in[k], e, in[k]);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float a[Op::NIN], o[Op::NOUT] = {};
#pragma unroll
            for (int k = 0; k < Op::NIN; ++k) a[k] = in[k][j];
            rw.col = col + j;
            rw.e = e + j;
            op.one(st, rw, a, o);
#pragma unroll
            for (int k = 0; k < Op::NOUT; ++k) out[k][j] = o[k];
        }
#pragma unroll
        for (int k = 0; k < Op::NOUT; ++k) store<V>(op.out[k], e, out[k]);
    }
    op.end(st, block);
}

template <int V, class Op>
__global__ __launch_bounds__(BLOCK) void step_rows_kernel(const Op op, const Rows r) {
    step_rows<V>(op, r, blockIdx.x, gridDim.x);
}

// Two segments in one launch (the video and the audio latent of a joint step; the audio one is ~100 rows, a launch of its own nearly all latency):
// blocks [0, blocks_a) are the grid of segment a, the rest the grid of segment b.  Each segment's elements see exactly what a launch of its own
// gives them -- begin() / end() included, which take the block's index within its segment -- so its output is the single launch's bit for bit.
template <int V, class Op>
__global__ __launch_bounds__(BLOCK) void step_rows2_kernel(const Op a, const Rows ra, const Op b, const Rows rb, const int blocks_a) {
    if ((int)blockIdx.x < blocks_a) step_rows<V>(a, ra, blockIdx.x, blocks_a);
    else step_rows<V>(b, rb, (int)blockIdx.x - blocks_a, (int)gridDim.x - blocks_a);
}

struct StepOp {         // the defaults: no per-thread state, no prologue, no epilogue; the row's timestep is loaded
    struct State {};
    static constexpr bool reads_t = true;
    template <class S>
    __device__ __forceinline__ void begin(S&, long) const {}
    template <class S>
    __device__ __forceinline__ void end(S&, long) const {}
};

// The shared formulas.  x0 of one velocity at the row's timestep:
__device__ __forceinline__ float denoised(float x, float v, float t) { return sub_rn(x, mul_rn(t, v)); }
// CFGGuider.guide, from the conditional side: a + (cfg - 1)*(a - b)
__device__ __forceinline__ float guide_from_cond(float a, float b, float cfg_minus_1) { return add_rn(a, mul_rn(cfg_minus_1, sub_rn(a, b))); }
// the HQ pipeline's order (ti2vid_hq.py:315), from the unconditional side: b + cfg*(a - b) -- another rounding than the line above
__device__ __forceinline__ float guide_from_uncond(float a, float b, float cfg) { return add_rn(b, mul_rn(cfg, sub_rn(a, b))); }
// post_process_latent: d*m + clean*(1 - m) on a conditioned latent
__device__ __forceinline__ float blend_clean(float d, float clean, const Row& r) {
    return r.blend ? add_rn(mul_rn(d, r.m), mul_rn(clean, r.one_minus_m)) : d;
}
// x + ((x - d)/sigma)*(sigma_next - sigma) with inv = 1/sigma, dt = sigma_next - sigma
__device__ __forceinline__ float euler(float x, float d, float inv, float dt) { return add_rn(x, mul_rn(mul_rn(sub_rn(x, d), inv), dt)); }

struct GuidedEuler : StepOp {
    enum { X, VC, VU, CLEAN, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float s1, inv, dt;          // cfg_scale - 1, 1/sigma, sigma_next - sigma
    __device__ __forceinline__ void one(State&, const Row& r, const float* a, float* o) const {
        const float g = guide_from_cond(denoised(a[X], a[VC], r.t), denoised(a[X], a[VU], r.t), s1);
        o[OUT] = euler(a[X], blend_clean(g, a[CLEAN], r), inv, dt);
    }
};

// STGGuider.guide on top of the CFG-guided x0 (pipelines/one_stage.py:284-297): g as GuidedEuler forms it (g = a with no vu: the guider is not
// enabled), p = x - t*vp from the pass whose self-attentions were skipped, s = g + stg*(g - p).  No vp (the pair form alone allows it: a modality
// that is not STG-guided, a step past the cutoff): s = g, GuidedEuler's arithmetic
struct StgEuler : StepOp {
    enum { X, VC, VU, VP, CLEAN, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float s1, stg, inv, dt;     // cfg_scale - 1, stg_scale, 1/sigma, sigma_next - sigma
    __device__ __forceinline__ void one(State&, const Row& r, const float* a, float* o) const {
        float g = denoised(a[X], a[VC], r.t);
        if (in[VU]) g = guide_from_cond(g, denoised(a[X], a[VU], r.t), s1);
        if (in[VP]) g = add_rn(g, mul_rn(stg, sub_rn(g, denoised(a[X], a[VP], r.t))));
        o[OUT] = euler(a[X], blend_clean(g, a[CLEAN], r), inv, dt);
    }
};

// the guided, mask-blended x0 of one pair of velocities as the res_2s step forms it; no vu: no guidance
__device__ __forceinline__ float res2s_denoised(const Row& r, float x, float vc, float vu, bool guide, float cfg, float clean) {
    float d = denoised(x, vc, r.t);
    if (guide) d = guide_from_uncond(d, denoised(x, vu, r.t), cfg);
    return blend_clean(d, clean, r);
}

// anchor = x, eps1 = d - anchor, x_mid = anchor + c*eps1, then the "bong" iteration (:232-238) n_bong times in registers:
// anchor = x_mid - c*eps1, eps1 = d - anchor.  No anchor / eps1 to store: the final-step form, x_mid = d and nothing else.
struct Res2sMidpoint : StepOp {
    enum { X, VC, VU, CLEAN, NIN };
    enum { X_MID, ANCHOR, EPS1, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float cfg, c;
    int n_bong;
    __device__ __forceinline__ void one(State&, const Row& r, const float* a, float* o) const {
        const float d = res2s_denoised(r, a[X], a[VC], a[VU], in[VU] != nullptr, cfg, a[CLEAN]);
        if (!out[ANCHOR]) {
            o[X_MID] = d;
            return;
        }
        float an = a[X], e = sub_rn(d, an);
        const float xm = add_rn(an, mul_rn(c, e));
        for (int k = 0; k < n_bong; ++k) {
            an = sub_rn(xm, mul_rn(c, e));
            e = sub_rn(d, an);
        }
        o[X_MID] = xm;
        o[ANCHOR] = an;
        o[EPS1] = e;
    }
};

// d2 from (x_mid, velocities at the sub-sigma) as above, e2 = d2 - anchor, out = anchor + h*(b1*eps1 + b2*e2)
struct Res2sCombine : StepOp {
    enum { X_MID, VC, VU, CLEAN, ANCHOR, EPS1, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float cfg, h, b1, b2;
    __device__ __forceinline__ void one(State&, const Row& r, const float* a, float* o) const {
        const float d2 = res2s_denoised(r, a[X_MID], a[VC], a[VU], in[VU] != nullptr, cfg, a[CLEAN]);
        const float e2 = sub_rn(d2, a[ANCHOR]);
        o[OUT] = add_rn(a[ANCHOR], mul_rn(h, add_rn(mul_rn(b1, a[EPS1]), mul_rn(b2, e2))));
    }
};

// The Heun sampler's first pass (reference pipelines/one_stage.py:334-424), and with no `d` stored the Euler step with the GE velocity correction
// (:300-326): g as GuidedEuler forms it (g = a with no vu).  GE, where the state `prev` is given (out[PREV_OUT]): cur = (x - g)/sigma, and unless
// the step is the loop's first (in[PREV] NULL) tot = gamma*(cur - prev) + prev, g = x - tot*sigma; prev = cur, the UNcorrected velocity.  Then
// d = the mask / clean blend of g and the predictor xp = x + ((x - d)/sigma)*dt, which is GuidedEuler's output.  No xp to store: the final-step
// form (sigma_next == 0), d alone.
struct HeunPredict : StepOp {
    enum { X, VC, VU, CLEAN, PREV, NIN };
    enum { D, XP, PREV_OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float s1, inv, dt, sigma, gamma;    // cfg_scale - 1, 1/sigma, sigma_next - sigma, sigma, ge_gamma
    __device__ __forceinline__ void one(State&, const Row& r, const float* a, float* o) const {
        float g = denoised(a[X], a[VC], r.t);
        if (in[VU]) g = guide_from_cond(g, denoised(a[X], a[VU], r.t), s1);
        if (out[PREV_OUT]) {
            const float cur = mul_rn(sub_rn(a[X], g), inv);
            if (in[PREV]) g = sub_rn(a[X], mul_rn(add_rn(mul_rn(gamma, sub_rn(cur, a[PREV])), a[PREV]), sigma));
            o[PREV_OUT] = cur;
        }
        const float d = blend_clean(g, a[CLEAN], r);
        o[D] = d;
        o[XP] = euler(a[X], d, inv, dt);
    }
};

// The Heun corrector (:426-453; HeunDiffusionStep.step): d2 from (xp, velocities at sigma_next) as above, without GE, v1 = (x - d)/sigma,
// v2 = (xp - d2)/sigma_next, out = x + (0.5*(v1 + v2))*dt
struct HeunCorrect : StepOp {
    enum { X, D, XP, VC, VU, CLEAN, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float s1, inv, inv_next, dt;        // cfg_scale - 1, 1/sigma, 1/sigma_next, sigma_next - sigma
    __device__ __forceinline__ void one(State&, const Row& r, const float* a, float* o) const {
        float g = denoised(a[XP], a[VC], r.t);
        if (in[VU]) g = guide_from_cond(g, denoised(a[XP], a[VU], r.t), s1);
        const float v1 = mul_rn(sub_rn(a[X], a[D]), inv), v2 = mul_rn(sub_rn(a[XP], blend_clean(g, a[CLEAN], r)), inv_next);
        o[OUT] = add_rn(a[X], mul_rn(mul_rn(0.5f, add_rn(v1, v2)), dt));
    }
};

constexpr int NSUM = 5;               // S_aa, S_ab, S_bb, S_gg, S_ga
constexpr int SUMS_CAP = 1024;        // every block of the second pass reads all the rows of the first

// rows of `partials`: a function of (rows, C) alone, whichever access width the operands' alignment allows
inline int sums_blocks(long n) { return grid_for((n + 3) / 4, BLOCK, SUMS_CAP); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The N sums of a block in the order every sums pass shares -- per thread in loop order (s), across the wave (xor tree), across the block's waves in
// order -- into row `block` of partials[blocks][N]
template <int N>
__device__ __forceinline__ void block_sums_store(const double (&s)[N], double* partials, long block) {
    __shared__ double part[WAVES][N];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double w = wave_sum_f64(s[k]);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double acc = part[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) acc += part[w][threadIdx.x];
        partials[block * N + threadIdx.x] = acc;
    }
}

// The nb rows of partials[nb][N] added in index order into sums[N] (shared memory; the caller synchronises): every block holds the same sums
template <int N>
__device__ __forceinline__ void partial_rows_sum(const double* partials, int nb, double* sums) {
    if (threadIdx.x < N) {
        double acc = 0.0;
        for (int r = 0; r < nb; ++r) acc += partials[(long)r * N + threadIdx.x];
        sums[threadIdx.x] = acc;
    }
}

// a = x - t*vc, b = x - t*vu, g = a - b, with momentum g = momentum*running + g (in[RUN]: NULL on the first step) stored back to running; the five
// sums per thread in loop order, then across the wave (xor tree), then across the block's waves in order.
struct GuidanceSums : StepOp {
    enum { X, VC, VU, RUN, NIN };
    enum { RUN_OUT, NOUT };
    struct State {
        double s[NSUM];
    };
    const float* in[NIN];
    float* out[NOUT];
    float momentum;
    double* partials;
    __device__ __forceinline__ void begin(State& st, long) const {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) st.s[k] = 0.0;
    }
    __device__ __forceinline__ void one(State& st, const Row& r, const float* v, float* o) const {
        const float a = denoised(v[X], v[VC], r.t), b = denoised(v[X], v[VU], r.t);
        float g = sub_rn(a, b);
        if (in[RUN]) g = add_rn(mul_rn(momentum, v[RUN]), g);
        o[RUN_OUT] = g;
        const double da = a, db = b, dg = g;                   // each product of two fp32 values is exact in fp64
        st.s[0] += da * da;
        st.s[1] += da * db;
        st.s[2] += db * db;
        st.s[3] += dg * dg;
        st.s[4] += dg * da;
    }
    __device__ __forceinline__ void end(State& st, long block) const { block_sums_store<NSUM>(st.s, partials, block); }
};

// g_out of one element from (a, b, g) and the block's fp32 scalars: k0 = coef (mode 0) or sf (modes 1, 2), k1 = proj
__device__ __forceinline__ float projected_one(int mode, float a, float b, float g, float k0, float k1, float mult, float eta) {
    if (mode == 0) return add_rn(a, mul_rn(mult, sub_rn(a, mul_rn(k0, b))));
    const float gsc = mul_rn(g, k0), par = mul_rn(k1, a);
    const float apg = add_rn(mul_rn(par, eta), sub_rn(gsc, par));
    return add_rn(a, mul_rn(apg, mult));
}

// Every block adds the partial rows in index order, so every block holds the same five sums and derives the same scalars; then the guided step
// with g read from `running` (mode 2 with momentum) or formed as a - b.  The two-segment launch also takes a segment whose guider has no sums:
// PROJECTED_CFG (CFGGuider.guide, GuidedEuler's arithmetic) and PROJECTED_OFF (d = a); such a segment reads no partials and reports no scalars.
struct ProjectedEuler : StepOp {
    enum { X, VC, VU, CLEAN, RUN, NIN };
    enum { OUT, NOUT };
    struct State {
        float k0, k1;
    };
    const float* in[NIN];
    float* out[NOUT];
    const double* partials;
    float* scalars_out;
    int mode;             // 0 CFG*, 1 APG, 2 legacy APG, PROJECTED_CFG, PROJECTED_OFF
    float mult;           // scale - 1 (modes 0, 1, PROJECTED_CFG) or scale (mode 2)
    float eta, thr, inv, dt;
    int nb;               // rows of partials
    __device__ __forceinline__ void begin(State& st, long block) const {
        __shared__ double sums[NSUM];
        __shared__ float sc[2];
        if (mode >= PROJECTED_CFG) {                                   // the same in every thread of the block: no barrier is skipped by some
            st.k0 = st.k1 = 0.f;
            return;
        }
        partial_rows_sum<NSUM>(partials, nb, sums);
        __syncthreads();
        if (threadIdx.x == 0) {                                        // fp64 throughout, each scalar rounded once
            float k0, k1 = 0.f;
            if (mode == 0) {
                k0 = (float)(sums[1] / (sums[2] + 1e-8));
            } else {
                double sf = 1.0;
                if (thr > 0.f) sf = fmin(1.0, (double)thr / sqrt(sums[3]));
                k0 = (float)sf;
                k1 = (float)(sf * sums[4] / (sums[0] + 1e-8));
            }
            sc[0] = k0;
            sc[1] = k1;
            if (block == 0 && scalars_out) {
                scalars_out[0] = k0;
                if (mode != 0) scalars_out[1] = k1;
            }
        }
        __syncthreads();
        st.k0 = sc[0];
        st.k1 = sc[1];
    }
    __device__ __forceinline__ void one(State& st, const Row& r, const float* v, float* o) const {
        const float a = denoised(v[X], v[VC], r.t), b = denoised(v[X], v[VU], r.t);
        const float g = in[RUN] ? v[RUN] : sub_rn(a, b);
        const float d = mode == PROJECTED_OFF ? a : mode == PROJECTED_CFG ? guide_from_cond(a, b, mult) : projected_one(mode, a, b, g, st.k0, st.k1, mult, eta);
        o[OUT] = euler(v[X], blend_clean(d, v[CLEAN], r), inv, dt);
    }
};

// MultiModalGuider.calculate (reference components/guiders.py:244-273) from the conditional x0 `a` and the x0 of the passes that ran: u (negative prompt),
// p (self-attentions skipped), m (cross-modal attentions skipped); a term is there exactly when its velocity is
struct MmTerms {
    float cfg1, stg, mod1;      // cfg_scale - 1, stg_scale, modality_scale - 1
};
__device__ __forceinline__ float mm_pred(const MmTerms& k, const Row& r, float x, float a, float vu, float vp, float vm, bool has_u, bool has_p, bool has_m) {
    float pred = a;
    if (has_u) pred = add_rn(pred, mul_rn(k.cfg1, sub_rn(a, denoised(x, vu, r.t))));
    if (has_p) pred = add_rn(pred, mul_rn(k.stg, sub_rn(a, denoised(x, vp, r.t))));
    if (has_m) pred = add_rn(pred, mul_rn(k.mod1, sub_rn(a, denoised(x, vm, r.t))));
    return pred;
}

// the multi-modal guided step without rescale: pred, the mask / clean blend, Euler
struct MmGuidedEuler : StepOp {
    enum { X, VC, VU, VP, VM, CLEAN, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    MmTerms k;
    float inv, dt;              // 1/sigma, sigma_next - sigma
    __device__ __forceinline__ void one(State&, const Row& r, const float* v, float* o) const {
        const float a = denoised(v[X], v[VC], r.t);
        const float pred = mm_pred(k, r, v[X], a, v[VU], v[VP], v[VM], in[VU] != nullptr, in[VP] != nullptr, in[VM] != nullptr);
        o[OUT] = euler(v[X], blend_clean(pred, v[CLEAN], r), inv, dt);
    }
};

constexpr int NMM = 4;                // S_a, S_aa, S_p, S_pp

// with rescale, pass 1: the fp64 sums of a, a*a, pred, pred*pred over ALL rows in GuidanceSums' order; pred is stored where the caller asks for it
struct MmGuidanceSums : StepOp {
    enum { X, VC, VU, VP, VM, NIN };
    enum { PRED, NOUT };
    struct State {
        double s[NMM];
    };
    const float* in[NIN];
    float* out[NOUT];
    MmTerms k;
    double* partials;
    __device__ __forceinline__ void begin(State& st, long) const {
#pragma unroll
        for (int j = 0; j < NMM; ++j) st.s[j] = 0.0;
    }
    __device__ __forceinline__ void one(State& st, const Row& r, const float* v, float* o) const {
        const float a = denoised(v[X], v[VC], r.t);
        const float pred = mm_pred(k, r, v[X], a, v[VU], v[VP], v[VM], in[VU] != nullptr, in[VP] != nullptr, in[VM] != nullptr);
        o[PRED] = pred;
        const double da = a, dp = pred;                        // each product of two fp32 values is exact in fp64
        st.s[0] += da;
        st.s[1] += da * da;
        st.s[2] += dp;
        st.s[3] += dp * dp;
    }
    __device__ __forceinline__ void end(State& st, long block) const { block_sums_store<NMM>(st.s, partials, block); }
};

// pass 2: every block adds the partial rows in index order and derives, in fp64, the population variances var = (S2 - S1*S1/n)/n (as mx.var) and
// f = rescale*sqrt((var_a + 1e-8)/(var_p + 1e-8)) + (1 - rescale), rounded once to fp32; then the step with pred*f
struct MmRescaledEuler : StepOp {
    enum { X, VC, VU, VP, VM, CLEAN, NIN };
    enum { OUT, NOUT };
    struct State {
        float f;
    };
    const float* in[NIN];
    float* out[NOUT];
    MmTerms k;
    const double* partials;
    float* scalars_out;
    double rescale, n;          // rescale_scale; rows * C
    float inv, dt;
    int nb;                     // rows of partials
    __device__ __forceinline__ void begin(State& st, long block) const {
        __shared__ double sums[NMM];
        __shared__ float sf;
        partial_rows_sum<NMM>(partials, nb, sums);
        __syncthreads();
        if (threadIdx.x == 0) {
            const double var_a = (sums[1] - sums[0] * sums[0] / n) / n, var_p = (sums[3] - sums[2] * sums[2] / n) / n;
            sf = (float)(rescale * sqrt((var_a + 1e-8) / (var_p + 1e-8)) + (1.0 - rescale));
            if (block == 0 && scalars_out) scalars_out[0] = sf;
        }
        __syncthreads();
        st.f = sf;
    }
    __device__ __forceinline__ void one(State& st, const Row& r, const float* v, float* o) const {
        const float a = denoised(v[X], v[VC], r.t);
        const float pred = mm_pred(k, r, v[X], a, v[VU], v[VP], v[VM], in[VU] != nullptr, in[VP] != nullptr, in[VM] != nullptr);
        o[OUT] = euler(v[X], blend_clean(mul_rn(pred, st.f), v[CLEAN], r), inv, dt);
    }
};

// ---------------------------------- classifier-free guidance with the per-channel rescale (the standard one-stage loop) ----------------------------------
// rescale_noise_cfg of the reference's scripts/generate.py:688-727: statistics over the rows (the tokens) per channel, not over the whole latent.
__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

constexpr int NCS = 4;                // per channel: the sums S1_g, S2_g, S1_a, S2_a, and the statistics mean_g, std_g, mean_a, std_a
constexpr int CS_ROWS = 64, CS_CAP = 256;       // a block takes at least CS_ROWS rows, and there are at most CS_CAP blocks

// blocks along the rows: a function of the shape alone, whichever access width the operands' alignment allows
inline int channel_blocks(int rows) { return grid_for(rows, CS_ROWS, CS_CAP); }

// Pass 1.  Block (bx, by) takes the rows [rows*bx/nb, rows*(bx+1)/nb) and the `lanes` column groups (V channels each) from by*lanes on: a thread
// owns one column group and every (BLOCK / lanes)-th row of the chunk.  With a = x - t*vc, b = x - t*vu, g = b + cfg*(a - b) as the step forms them
// and the shifts g0, a0 = the channel's values in row 0, it adds (v - v0) and (v - v0)^2 in fp64 in row order, then the block's row lanes in lane
// order, into partials[bx][4][C].  Block row 0 also stores the shifts into partials[nb][0][C] (g0) and partials[nb][2][C] (a0).  No atomics.
template <int V>
__global__ __launch_bounds__(BLOCK) void channel_sums_kernel(const float* __restrict__ x, const float* __restrict__ vc, const float* __restrict__ vu,
                                                             const float* __restrict__ ts, long ts_stride, float cfg, double* __restrict__ partials,
                                                             int rows, int C, int lanes) {
    __shared__ double part[BLOCK * V];
    const int cl = threadIdx.x % lanes, rl = threadIdx.x / lanes, row_lanes = BLOCK / lanes;
    const int col = ((int)blockIdx.y * lanes + cl) * V;
    const bool active = col < C;
    const int nb = gridDim.x;
    const long r0 = (long)rows * blockIdx.x / nb, r1 = (long)rows * (blockIdx.x + 1) / nb;
    double s[NCS][V] = {}, g0[V] = {}, a0[V] = {};
    auto form = [&](long row, float (&g)[V], float (&a)[V]) {
        const float t = ts[row * ts_stride];
        alignas(16) float xv[V], cv[V], uv[V];
        load<V>(x, row * C + col, xv);
        load<V>(vc, row * C + col, cv);
        load<V>(vu, row * C + col, uv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            a[j] = denoised(xv[j], cv[j], t);
            g[j] = guide_from_uncond(a[j], denoised(xv[j], uv[j], t), cfg);
        }
    };
    if (active) {
        float g[V], a[V];
        form(0, g, a);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            g0[j] = g[j];
            a0[j] = a[j];
        }
        for (long row = r0 + rl; row < r1; row += row_lanes) {
            form(row, g, a);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double dg = (double)g[j] - g0[j], da = (double)a[j] - a0[j];
                s[0][j] += dg;
                s[1][j] += dg * dg;
                s[2][j] += da;
                s[3][j] += da * da;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NCS; ++k) {
#pragma unroll
        for (int j = 0; j < V; ++j) part[threadIdx.x * V + j] = s[k][j];
        __syncthreads();
        if (active && rl == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double acc = part[cl * V + j];
                for (int q = 1; q < row_lanes; ++q) acc += part[(q * lanes + cl) * V + j];
                partials[((long)blockIdx.x * NCS + k) * C + col + j] = acc;
            }
        }
        __syncthreads();
    }
    if (active && rl == 0 && blockIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            partials[((long)nb * NCS + 0) * C + col + j] = g0[j];
            partials[((long)nb * NCS + 2) * C + col + j] = a0[j];
        }
    }
}

// Pass 2, one thread per channel: the nb partial rows added in index order, then in fp64 mean = v0 + S1/n, var = max((S2 - S1*S1/n)/n, 0),
// std = sqrt(var + 1e-8), each rounded once to fp32 into stats[4][C] = mean_g, std_g, mean_a, std_a
__global__ __launch_bounds__(BLOCK) void channel_stats_kernel(const double* __restrict__ partials, float* __restrict__ stats, int nb, int rows, int C) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= C) return;
    double s[NCS];
#pragma unroll
    for (int k = 0; k < NCS; ++k) {
        double acc = 0.0;
        for (int b = 0; b < nb; ++b) acc += partials[((long)b * NCS + k) * C + c];
        s[k] = acc;
    }
    const double n = rows;
#pragma unroll
    for (int k = 0; k < NCS; k += 2) {
        const double v0 = partials[((long)nb * NCS + k) * C + c];
        stats[(long)k * C + c] = (float)(v0 + s[k] / n);
        stats[(long)(k + 1) * C + c] = (float)sqrt(fmax((s[k + 1] - s[k] * s[k] / n) / n, 0.0) + 1e-8);
    }
}

// The guided step with the rescale, the reference's statements in order (scripts/generate.py:1935-1960, rescale_noise_cfg :715-725, euler_step_x0):
// a = x - t*vc, b = x - t*vu, g = b + cfg*(a - b); with stats: gr = ((g - mean_g)/std_g)*std_a + mean_a, g = r*gr + (1 - r)*g; then the Euler step
struct RescaledGuidedEuler : StepOp {
    enum { X, VC, VU, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    const float* stats;         // [4][C], or NULL: no rescale
    float cfg, r, one_minus_r, inv, dt;     // cfg_scale, guidance_rescale, 1 - guidance_rescale, 1/sigma, sigma_next - sigma
    int C;
    __device__ __forceinline__ void one(State&, const Row& rw, const float* v, float* o) const {
        const float a = denoised(v[X], v[VC], rw.t);
        float g = guide_from_uncond(a, denoised(v[X], v[VU], rw.t), cfg);
        if (stats) {
            const float* s = stats + rw.col;
            const float gr = add_rn(mul_rn(div_rn(sub_rn(g, s[0]), s[C]), s[3L * C]), s[2L * C]);
            g = add_rn(mul_rn(r, gr), mul_rn(one_minus_r, g));
        }
        o[OUT] = euler(v[X], g, inv, dt);
    }
};

// ---------------------------------- counter-based noise and the Euler-ancestral step ----------------------------------
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"; the Random123 known-answer vectors): ten rounds of two 32x32->64
// multiplies, the key bumped by the Weyl constants between rounds.
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// Where a latent's noise comes from: a pure function of (seed, step, stream, element index).  seed: one 64-bit word in device memory, read when the
// kernel runs, so one captured graph serves any seed; stream: 0 the video latent, 1 the audio latent
struct Noise {
    const uint64_t* seed;
    uint32_t step, stream;
};

// The four words of quad q: counter (lo32(q), hi32(q), step, stream), key (lo32(seed), hi32(seed)); they serve the elements 4q .. 4q+3
__device__ __forceinline__ void philox_quad(long q, uint64_t seed, const Noise& nz, uint32_t (&r)[4]) {
    r[0] = (uint32_t)(uint64_t)q;
    r[1] = (uint32_t)((uint64_t)q >> 32);
    r[2] = nz.step;
    r[3] = nz.stream;
    philox4x32_10(r, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// The four N(0,1) values of quad q, the ONE function every caller shares (the fill and the fused step give the same bits): uniforms
// u_k = ((r_k >> 9) + 0.5)*2^-23, exact in fp32 and inside (0, 1); Box-Muller on (u0, u1) and on (u2, u3) with the accurate logf / sincospif
// (the angle 2*u is exact, so no rounded 2*pi*u enters), every operation rounded on its own
__device__ __forceinline__ void philox_normal_quad(long q, uint64_t seed, const Noise& nz, float (&z)[4]) {
#pragma clang fp contract(off)
    uint32_t r[4];
    philox_quad(q, seed, nz, r);
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = ((float)(r[k] >> 9) + 0.5f) * 0x1p-23f;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const float rad = sqrtf(-2.0f * logf(u[k]));
        float sn, cs;
        sincospif(2.0f * u[k + 1], &sn, &cs);
        z[k] = rad * cs;
        z[k + 1] = rad * sn;
    }
}

__global__ __launch_bounds__(BLOCK) void philox_bits_kernel(uint32_t* __restrict__ out, long n_quads, const Noise nz) {
    const uint64_t seed = *nz.seed;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += (long)gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox_quad(q, seed, nz, r);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[4 * q + k] = r[k];
    }
}

__global__ __launch_bounds__(BLOCK) void philox_normal_kernel(float* __restrict__ out, long n, const Noise nz) {
    const uint64_t seed = *nz.seed;
    const long n_quads = (n + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += (long)gridDim.x * blockDim.x) {
        float z[4];
        philox_normal_quad(q, seed, nz, z);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * q + k < n) out[4 * q + k] = z[k];
    }
}

// The stochastic part of EulerAncestralDiffusionStep (reference components/diffusion_steps.py:70-129): r, the Euler step to sigma_down, plus
// z*sigma_up scaled by the row's mask -- a conditioned token (m = 0) stays on its clean value, where the reference would add noise to it too;
// with m = 1 the arithmetic is the reference's.  A thread keeps the quad it evaluated last: with 16-byte accesses that is one Philox per four
// elements; an element-wise thread evaluates quad e >> 2 and keeps lane e & 3, so the values do not depend on the access width or the grid.
// up == 0: no Philox is evaluated and r comes back as it is.
struct NoiseState {
    uint64_t seed;
    long q;
    float z[4];
};
struct AncestralOp : StepOp {
    using State = NoiseState;
    __device__ __forceinline__ void begin_noise(State& st, const Noise& nz, float up) const {
        st.seed = up != 0.f ? *nz.seed : 0;
        st.q = -1;
    }
    __device__ __forceinline__ float ancestral(State& st, const Noise& nz, const Row& r, float stepped, float up) const {
        if (up == 0.f) return stepped;
        const long q = r.e >> 2;
        if (q != st.q) {
            philox_normal_quad(q, st.seed, nz, st.z);
            st.q = q;
        }
        const int lane = (int)(r.e & 3);
        const float z = lane == 0 ? st.z[0] : lane == 1 ? st.z[1] : lane == 2 ? st.z[2] : st.z[3];
        return add_rn(stepped, mul_rn(mul_rn(z, up), r.m));
    }
};

// g as GuidedEuler forms it and its Euler step with dt = sigma_down - sigma, then the noise.  No vu: the plain step's arithmetic, through the
// helpers x0_from_velocity_kernel and euler_step_kernel are written with (plain_denoised, plain_euler), so the unguided step at sigma_up == 0 is
// the plain denoise step's bit for bit
struct AncestralEuler : AncestralOp {
    enum { X, VC, VU, CLEAN, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float s1, inv, dt, up;      // cfg_scale - 1, 1/sigma, sigma_down - sigma, sigma_up
    Noise nz;
    __device__ __forceinline__ void begin(State& st, long) const { begin_noise(st, nz, up); }
    __device__ __forceinline__ void one(State& st, const Row& r, const float* a, float* o) const {
        float stepped;
        if (in[VU]) {
            const float g = guide_from_cond(denoised(a[X], a[VC], r.t), denoised(a[X], a[VU], r.t), s1);
            stepped = euler(a[X], blend_clean(g, a[CLEAN], r), inv, dt);
        } else {
            stepped = plain_euler(a[X], blend_clean(plain_denoised(a[X], a[VC], r.t), a[CLEAN], r), inv, dt);
        }
        o[OUT] = ancestral(st, nz, r, stepped, up);
    }
};

// The same from a ready x0 (EulerAncestralDiffusionStep.step).  A mask without a clean latent: x0 is taken as it is -- the caller has blended
// it already -- and the mask scales the noise alone
struct AncestralFromX0 : AncestralOp {
    static constexpr bool reads_t = false;      // no velocity, no timestep: Rows.ts stays NULL
    enum { X, X0, CLEAN, NIN };
    enum { OUT, NOUT };
    const float* in[NIN];
    float* out[NOUT];
    float inv, dt, up;
    Noise nz;
    __device__ __forceinline__ void begin(State& st, long) const { begin_noise(st, nz, up); }
    __device__ __forceinline__ void one(State& st, const Row& r, const float* a, float* o) const {
        const float d = in[CLEAN] ? blend_clean(a[X0], a[CLEAN], r) : a[X0];
        o[OUT] = ancestral(st, nz, r, euler(a[X], d, inv, dt), up);
    }
};

// The checks every step shares, under the caller's name, and the launch.  present: the caller's required operands are all there.  16-byte accesses
// need every [rows][C] operand on a 16-byte boundary as well as C % 4 == 0 (a NULL operand contributes no bits).  sums_grid: the grid of the sums
// pass, which does not depend on the access width; 0: a step, one thread per vector under grid_for's cap.
// mask_alone: the ancestral step from a ready x0 -- it also takes a mask without a clean latent, and reads no timesteps (Op::reads_t is false)
inline int check_rows(const char* who, bool present, const float* ts, long ts_stride, const float* mask, const float* clean, int rows, int C,
                      bool mask_alone = false) {
    LTX2_CHECK_ARG(present && (ts || mask_alone) && rows > 0 && C > 0, "%s: null operand or empty shape", who);
    LTX2_CHECK_ARG(ts_stride == 0 || ts_stride == 1, "%s: ts_stride is 0 (one timestep) or 1 (one per row)", who);
    LTX2_CHECK_ARG(mask_alone ? (mask || !clean) : (mask == nullptr) == (clean == nullptr), "%s: %s", who,
                   mask_alone ? "a clean latent needs its mask" : "mask and clean go together");
    return LTX2_OK;
}

template <class Op>
bool vec4_ok(const Op& op, int C) {
    uintptr_t al = 0;
    for (const float* p : op.in) al |= (uintptr_t)p;
    for (const float* p : op.out) al |= (uintptr_t)p;
    return C % 4 == 0 && (al & 15) == 0;
}

template <class Op>
int launch_rows(const char* who, bool present, const Op& op, const float* ts, long ts_stride, const float* mask, const float* clean, int rows, int C,
                int sums_grid, hipStream_t stream, bool mask_alone = false) {
    if (const int rc = check_rows(who, present, ts, ts_stride, mask, clean, rows, C, mask_alone); rc != LTX2_OK) return rc;
    const Rows r = {ts, ts_stride, mask, (long)rows * C, C};
    if (vec4_ok(op, C))
        hipLaunchKernelGGL((step_rows_kernel<4, Op>), dim3(sums_grid ? sums_grid : grid_for(r.n / 4, BLOCK)), dim3(BLOCK), 0, stream, op, r);
    else
        hipLaunchKernelGGL((step_rows_kernel<1, Op>), dim3(sums_grid ? sums_grid : grid_for(r.n, BLOCK)), dim3(BLOCK), 0, stream, op, r);
    LTX2_CHECK_LAUNCH(who);
    return LTX2_OK;
}

// One modality of a two-segment step: what launch_rows takes per call
struct Seg {
    const float* ts;
    long ts_stride;
    const float* mask;
    const float* clean;
    int rows, C;
};

// Both segments are checked as launch_rows checks one, before the one launch; 16-byte accesses only where BOTH segments allow them.
// sums_a / sums_b: each segment's grid in a sums pass (launch_rows' sums_grid); 0: a step
template <class Op>
int launch_rows2(const char* who, bool present, const Op& a, const Seg& sa, const Op& b, const Seg& sb, hipStream_t stream, int sums_a = 0,
                 int sums_b = 0) {
    if (const int rc = check_rows(who, present, sa.ts, sa.ts_stride, sa.mask, sa.clean, sa.rows, sa.C); rc != LTX2_OK) return rc;
    if (const int rc = check_rows(who, present, sb.ts, sb.ts_stride, sb.mask, sb.clean, sb.rows, sb.C); rc != LTX2_OK) return rc;
    const Rows ra = {sa.ts, sa.ts_stride, sa.mask, (long)sa.rows * sa.C, sa.C}, rb = {sb.ts, sb.ts_stride, sb.mask, (long)sb.rows * sb.C, sb.C};
    if (vec4_ok(a, sa.C) && vec4_ok(b, sb.C)) {
        const int ga = sums_a ? sums_a : grid_for(ra.n / 4, BLOCK), gb = sums_b ? sums_b : grid_for(rb.n / 4, BLOCK);
        hipLaunchKernelGGL((step_rows2_kernel<4, Op>), dim3(ga + gb), dim3(BLOCK), 0, stream, a, ra, b, rb, ga);
    } else {
        const int ga = sums_a ? sums_a : grid_for(ra.n, BLOCK), gb = sums_b ? sums_b : grid_for(rb.n, BLOCK);
        hipLaunchKernelGGL((step_rows2_kernel<1, Op>), dim3(ga + gb), dim3(BLOCK), 0, stream, a, ra, b, rb, ga);
    }
    LTX2_CHECK_LAUNCH(who);
    return LTX2_OK;
}

}  // namespace

int x0_from_velocity_launch(const float* latent, const float* vel, const float* ts_ptr, long ts_stride, float ts_scalar,
                            float* x0, int rows, int C, hipStream_t stream) {
    hipLaunchKernelGGL(x0_from_velocity_kernel, dim3(grid_for((long)rows * C, 256)), dim3(256), 0, stream, latent, vel,
                       ts_ptr, ts_stride, ts_scalar, x0, rows, C);
    LTX2_CHECK_LAUNCH("x0_from_velocity_kernel");
    return LTX2_OK;
}

int euler_step_launch(const float* x, const float* x0, const float* mask, const float* clean, float sigma,
                      float sigma_next, float* out, int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    LTX2_CHECK_ARG((mask == nullptr) == (clean == nullptr), "euler_step: mask and clean go together");
    hipLaunchKernelGGL(euler_step_kernel, dim3(grid_for((long)rows * C, 256)), dim3(256), 0, stream, x, x0, mask, clean,
                       1.0f / sigma, sigma_next - sigma, out, rows, C);
    LTX2_CHECK_LAUNCH("euler_step_kernel");
    return LTX2_OK;
}

int guided_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride,
                             const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, float* out,
                             int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const GuidedEuler op = {{}, {x, vel_cond, vel_uncond, clean}, {out}, cfg_scale - 1.0f, 1.0f / sigma, sigma_next - sigma};
    return launch_rows("guided_euler_step", x && vel_cond && vel_uncond && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int guided_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride,
                                  const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                  const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                                  const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next,
                                  hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const float inv = 1.0f / sigma, dt = sigma_next - sigma;
    const GuidedEuler v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_clean}, {v_out}, v_cfg_scale - 1.0f, inv, dt};
    const GuidedEuler a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_clean}, {a_out}, a_cfg_scale - 1.0f, inv, dt};
    return launch_rows2("guided_euler_step_pair", v_x && v_vel_cond && v_vel_uncond && v_out && a_x && a_vel_cond && a_vel_uncond && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int stg_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* ts, long ts_stride,
                          const float* mask, const float* clean, float cfg_scale, float stg_scale, float sigma, float sigma_next, float* out, int rows,
                          int C, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const StgEuler op = {{}, {x, vel_cond, vel_uncond, vel_perturbed, clean}, {out}, cfg_scale - 1.0f, stg_scale, 1.0f / sigma, sigma_next - sigma};
    return launch_rows("stg_euler_step", x && vel_cond && vel_perturbed && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int stg_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed, const float* v_ts,
                               long v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float v_stg_scale, float* v_out, int v_rows,
                               int v_C, const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed,
                               const float* a_ts, long a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float a_stg_scale,
                               float* a_out, int a_rows, int a_C, float sigma, float sigma_next, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const float inv = 1.0f / sigma, dt = sigma_next - sigma;
    const StgEuler v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_vel_perturbed, v_clean}, {v_out}, v_cfg_scale - 1.0f, v_stg_scale, inv, dt};
    const StgEuler a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_vel_perturbed, a_clean}, {a_out}, a_cfg_scale - 1.0f, a_stg_scale, inv, dt};
    return launch_rows2("stg_euler_step_pair", v_x && v_vel_cond && v_out && a_x && a_vel_cond && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int res2s_midpoint_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                          const float* clean, float cfg_scale, float c, int n_bong, float* x_mid, float* anchor, float* eps1, int rows, int C,
                          hipStream_t stream) {
    LTX2_CHECK_ARG((anchor == nullptr) == (eps1 == nullptr), "res2s_midpoint: anchor and eps1 go together (both NULL: the final-step form)");
    LTX2_CHECK_ARG(n_bong >= 0, "res2s_midpoint: n_bong=%d", n_bong);
    const Res2sMidpoint op = {{}, {x, vel_cond, vel_uncond, clean}, {x_mid, anchor, eps1}, cfg_scale, c, n_bong};
    return launch_rows("res2s_midpoint", x && vel_cond && x_mid, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int res2s_combine_launch(const float* x_mid, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                         const float* clean, float cfg_scale, const float* anchor, const float* eps1, float h, float b1, float b2, float* out,
                         int rows, int C, hipStream_t stream) {
    const Res2sCombine op = {{}, {x_mid, vel_cond, vel_uncond, clean, anchor, eps1}, {out}, cfg_scale, h, b1, b2};
    return launch_rows("res2s_combine", x_mid && vel_cond && anchor && eps1 && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int res2s_midpoint_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                               const float* v_clean, float v_cfg_scale, float* v_x_mid, float* v_anchor, float* v_eps1, int v_rows, int v_C,
                               const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                               const float* a_clean, float a_cfg_scale, float* a_x_mid, float* a_anchor, float* a_eps1, int a_rows, int a_C,
                               float c, int n_bong, hipStream_t stream) {
    LTX2_CHECK_ARG((v_anchor == nullptr) == (v_eps1 == nullptr) && (a_anchor == nullptr) == (a_eps1 == nullptr),
                   "res2s_midpoint_pair: anchor and eps1 go together (both NULL: the final-step form)");
    LTX2_CHECK_ARG((v_anchor == nullptr) == (a_anchor == nullptr), "res2s_midpoint_pair: the final-step form (anchor == eps1 == NULL) applies to both segments together");
    LTX2_CHECK_ARG(n_bong >= 0, "res2s_midpoint_pair: n_bong=%d", n_bong);
    const Res2sMidpoint v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_clean}, {v_x_mid, v_anchor, v_eps1}, v_cfg_scale, c, n_bong};
    const Res2sMidpoint a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_clean}, {a_x_mid, a_anchor, a_eps1}, a_cfg_scale, c, n_bong};
    return launch_rows2("res2s_midpoint_pair", v_x && v_vel_cond && v_x_mid && a_x && a_vel_cond && a_x_mid, v, {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C},
                        a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int res2s_combine_pair_launch(const float* v_x_mid, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                              const float* v_clean, float v_cfg_scale, const float* v_anchor, const float* v_eps1, float* v_out, int v_rows, int v_C,
                              const float* a_x_mid, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                              const float* a_clean, float a_cfg_scale, const float* a_anchor, const float* a_eps1, float* a_out, int a_rows, int a_C,
                              float h, float b1, float b2, hipStream_t stream) {
    const Res2sCombine v = {{}, {v_x_mid, v_vel_cond, v_vel_uncond, v_clean, v_anchor, v_eps1}, {v_out}, v_cfg_scale, h, b1, b2};
    const Res2sCombine a = {{}, {a_x_mid, a_vel_cond, a_vel_uncond, a_clean, a_anchor, a_eps1}, {a_out}, a_cfg_scale, h, b1, b2};
    return launch_rows2("res2s_combine_pair", v_x_mid && v_vel_cond && v_anchor && v_eps1 && v_out && a_x_mid && a_vel_cond && a_anchor && a_eps1 && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int guidance_sums_blocks(int rows, int C) { return (rows > 0 && C > 0) ? sums_blocks((long)rows * C) : 0; }

int guidance_sums_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, float* running, int first,
                         float momentum, double* partials, int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "guidance_sums: partials must be 8-byte aligned");
    const GuidanceSums op = {{}, {x, vel_cond, vel_uncond, first ? nullptr : running}, {running}, momentum, partials};
    return launch_rows("guidance_sums", x && vel_cond && vel_uncond && partials, op, ts, ts_stride, nullptr, nullptr, rows, C,
                       guidance_sums_blocks(rows, C), stream);
}

int projected_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                                const float* clean, const float* running, const double* partials, int mode, float scale, float eta,
                                float norm_threshold, float sigma, float sigma_next, float* out, float* scalars_out, int rows, int C,
                                hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    LTX2_CHECK_ARG(mode >= 0 && mode <= 2, "projected_euler_step: mode=%d is 0 (CFG*), 1 (APG) or 2 (legacy APG)", mode);
    LTX2_CHECK_ARG(running == nullptr || mode == 2, "projected_euler_step: only mode 2 (legacy APG with momentum) reads a running buffer");
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "projected_euler_step: partials must be 8-byte aligned");
    const ProjectedEuler op = {{}, {x, vel_cond, vel_uncond, clean, running}, {out}, partials, scalars_out, mode, mode == 2 ? scale : scale - 1.0f,
                               eta, norm_threshold, 1.0f / sigma, sigma_next - sigma, guidance_sums_blocks(rows, C)};
    return launch_rows("projected_euler_step", x && vel_cond && vel_uncond && partials && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int guidance_sums_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, float* v_running,
                              int v_first, float v_momentum, double* v_partials, int v_rows, int v_C, const float* a_x, const float* a_vel_cond,
                              const float* a_vel_uncond, const float* a_ts, long a_ts_stride, float* a_running, int a_first, float a_momentum,
                              double* a_partials, int a_rows, int a_C, hipStream_t stream) {
    LTX2_CHECK_ARG(v_partials || a_partials, "guidance_sums_pair: both partials are NULL (a segment without sums passes NULL, not both)");
    // a segment whose guider reads no sums: the other segment's single launch, which is what its blocks of the pair launch would be
    if (!a_partials)
        return guidance_sums_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, v_ts_stride, v_running, v_first, v_momentum, v_partials, v_rows, v_C, stream);
    if (!v_partials)
        return guidance_sums_launch(a_x, a_vel_cond, a_vel_uncond, a_ts, a_ts_stride, a_running, a_first, a_momentum, a_partials, a_rows, a_C, stream);
    LTX2_CHECK_ARG((((uintptr_t)v_partials | (uintptr_t)a_partials) & 7) == 0, "guidance_sums_pair: partials must be 8-byte aligned");
    const GuidanceSums v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_first ? nullptr : v_running}, {v_running}, v_momentum, v_partials};
    const GuidanceSums a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_first ? nullptr : a_running}, {a_running}, a_momentum, a_partials};
    return launch_rows2("guidance_sums_pair", v_x && v_vel_cond && v_vel_uncond && a_x && a_vel_cond && a_vel_uncond, v,
                        {v_ts, v_ts_stride, nullptr, nullptr, v_rows, v_C}, a, {a_ts, a_ts_stride, nullptr, nullptr, a_rows, a_C}, stream,
                        guidance_sums_blocks(v_rows, v_C), guidance_sums_blocks(a_rows, a_C));
}

namespace {
// one segment of projected_euler_step_pair: the single form's checks, with the two guiders that read no sums admitted
int projected_segment(const char* seg, const float* vel_uncond, const float* running, const double* partials, int mode, float scale, float eta,
                      float norm_threshold, float inv, float dt, int rows, int C, ProjectedEuler& op) {
    LTX2_CHECK_ARG(mode >= 0 && mode <= PROJECTED_OFF, "projected_euler_step_pair: %s mode=%d is 0 (CFG*), 1 (APG), 2 (legacy APG), 3 (CFG) or 4 (off)", seg, mode);
    LTX2_CHECK_ARG(running == nullptr || mode == 2, "projected_euler_step_pair: only mode 2 (legacy APG with momentum) reads a running buffer (%s)", seg);
    LTX2_CHECK_ARG(mode >= PROJECTED_CFG || partials, "projected_euler_step_pair: %s mode=%d reads partials", seg, mode);
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "projected_euler_step_pair: partials must be 8-byte aligned");
    LTX2_CHECK_ARG(mode == PROJECTED_OFF || vel_uncond, "projected_euler_step_pair: null operand or empty shape");
    op.partials = mode >= PROJECTED_CFG ? nullptr : partials;
    if (mode >= PROJECTED_CFG) op.scalars_out = nullptr;
    op.mode = mode;
    op.mult = mode == 2 ? scale : scale - 1.0f;
    op.eta = eta;
    op.thr = norm_threshold;
    op.inv = inv;
    op.dt = dt;
    op.nb = guidance_sums_blocks(rows, C);
    return LTX2_OK;
}
}  // namespace

int projected_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride,
                                     const float* v_mask, const float* v_clean, const float* v_running, const double* v_partials, int v_mode,
                                     float v_scale, float v_eta, float v_norm_threshold, float* v_out, float* v_scalars_out, int v_rows, int v_C,
                                     const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride,
                                     const float* a_mask, const float* a_clean, const float* a_running, const double* a_partials, int a_mode,
                                     float a_scale, float a_eta, float a_norm_threshold, float* a_out, float* a_scalars_out, int a_rows, int a_C,
                                     float sigma, float sigma_next, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const float inv = 1.0f / sigma, dt = sigma_next - sigma;
    ProjectedEuler v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_clean, v_running}, {v_out}, nullptr, v_scalars_out};
    ProjectedEuler a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_clean, a_running}, {a_out}, nullptr, a_scalars_out};
    if (const int rc = projected_segment("video", v_vel_uncond, v_running, v_partials, v_mode, v_scale, v_eta, v_norm_threshold, inv, dt, v_rows, v_C, v); rc != LTX2_OK) return rc;
    if (const int rc = projected_segment("audio", a_vel_uncond, a_running, a_partials, a_mode, a_scale, a_eta, a_norm_threshold, inv, dt, a_rows, a_C, a); rc != LTX2_OK) return rc;
    return launch_rows2("projected_euler_step_pair", v_x && v_vel_cond && v_out && a_x && a_vel_cond && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int mm_guided_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                                const float* ts, long ts_stride, const float* mask, const float* clean, float cfg_scale, float stg_scale,
                                float modality_scale, float sigma, float sigma_next, float* out, int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const MmGuidedEuler op = {{}, {x, vel_cond, vel_uncond, vel_perturbed, vel_isolated, clean}, {out}, {cfg_scale - 1.0f, stg_scale, modality_scale - 1.0f},
                              1.0f / sigma, sigma_next - sigma};
    return launch_rows("mm_guided_euler_step", x && vel_cond && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int mm_guided_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed,
                                     const float* v_vel_isolated, const float* v_ts, long v_ts_stride, const float* v_mask, const float* v_clean,
                                     float v_cfg_scale, float v_stg_scale, float v_modality_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                     const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed, const float* a_vel_isolated,
                                     const float* a_ts, long a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float a_stg_scale,
                                     float a_modality_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    const float inv = 1.0f / sigma, dt = sigma_next - sigma;
    const MmGuidedEuler v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_vel_perturbed, v_vel_isolated, v_clean}, {v_out},
                             {v_cfg_scale - 1.0f, v_stg_scale, v_modality_scale - 1.0f}, inv, dt};
    const MmGuidedEuler a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_vel_perturbed, a_vel_isolated, a_clean}, {a_out},
                             {a_cfg_scale - 1.0f, a_stg_scale, a_modality_scale - 1.0f}, inv, dt};
    return launch_rows2("mm_guided_euler_step_pair", v_x && v_vel_cond && v_out && a_x && a_vel_cond && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int mm_guidance_sums_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                            const float* ts, long ts_stride, float cfg_scale, float stg_scale, float modality_scale, double* partials, float* pred_out,
                            int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "mm_guidance_sums: partials must be 8-byte aligned");
    const MmGuidanceSums op = {{}, {x, vel_cond, vel_uncond, vel_perturbed, vel_isolated}, {pred_out}, {cfg_scale - 1.0f, stg_scale, modality_scale - 1.0f},
                               partials};
    return launch_rows("mm_guidance_sums", x && vel_cond && partials, op, ts, ts_stride, nullptr, nullptr, rows, C, guidance_sums_blocks(rows, C), stream);
}

int mm_rescaled_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                                  const float* ts, long ts_stride, const float* mask, const float* clean, const double* partials, float cfg_scale,
                                  float stg_scale, float modality_scale, float rescale_scale, float sigma, float sigma_next, float* out,
                                  float* scalars_out, int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0, "mm_rescaled_euler_step: partials must be 8-byte aligned");
    const MmRescaledEuler op = {{}, {x, vel_cond, vel_uncond, vel_perturbed, vel_isolated, clean}, {out},
                                {cfg_scale - 1.0f, stg_scale, modality_scale - 1.0f}, partials, scalars_out, (double)rescale_scale, (double)rows * C,
                                1.0f / sigma, sigma_next - sigma, guidance_sums_blocks(rows, C)};
    return launch_rows("mm_rescaled_euler_step", x && vel_cond && partials && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int channel_guidance_stats_blocks(int rows, int C) { return (rows > 0 && C > 0) ? channel_blocks(rows) + 1 : 0; }

int channel_guidance_stats_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, float cfg_scale,
                                  double* partials, float* stats, int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(x && vel_cond && vel_uncond && ts && partials && stats && rows > 0 && C > 0, "channel_guidance_stats: null operand or empty shape");
    LTX2_CHECK_ARG(ts_stride == 0 || ts_stride == 1, "channel_guidance_stats: ts_stride is 0 (one timestep) or 1 (one per row)");
    LTX2_CHECK_ARG(((uintptr_t)partials & 7) == 0 && ((uintptr_t)stats & 3) == 0, "channel_guidance_stats: partials must be 8-byte and stats 4-byte aligned");
    const bool v4 = C % 4 == 0 && (((uintptr_t)x | (uintptr_t)vel_cond | (uintptr_t)vel_uncond) & 15) == 0;
    const int groups = v4 ? C / 4 : C, nb = channel_blocks(rows);
    int lanes = 1;              // column groups per block: the power of two that covers them, BLOCK at the most; the other threads are row lanes
    while (lanes < groups && lanes < BLOCK) lanes <<= 1;
    const dim3 grid(nb, (groups + lanes - 1) / lanes);
    if (v4)
        hipLaunchKernelGGL((channel_sums_kernel<4>), grid, dim3(BLOCK), 0, stream, x, vel_cond, vel_uncond, ts, ts_stride, cfg_scale, partials, rows, C, lanes);
    else
        hipLaunchKernelGGL((channel_sums_kernel<1>), grid, dim3(BLOCK), 0, stream, x, vel_cond, vel_uncond, ts, ts_stride, cfg_scale, partials, rows, C, lanes);
    LTX2_CHECK_LAUNCH("channel_sums_kernel");
    hipLaunchKernelGGL(channel_stats_kernel, dim3((C + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, partials, stats, nb, rows, C);
    LTX2_CHECK_LAUNCH("channel_stats_kernel");
    return LTX2_OK;
}

int rescaled_guided_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* stats,
                                      float cfg_scale, double guidance_rescale, float sigma, float sigma_next, float* out, int rows, int C,
                                      hipStream_t stream) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    LTX2_CHECK_ARG(((uintptr_t)stats & 3) == 0, "rescaled_guided_euler_step: stats must be 4-byte aligned");
    const RescaledGuidedEuler op = {{}, {x, vel_cond, vel_uncond}, {out}, stats, cfg_scale, (float)guidance_rescale, (float)(1.0 - guidance_rescale),
                                    1.0f / sigma, sigma_next - sigma, C};
    return launch_rows("rescaled_guided_euler_step", x && vel_cond && vel_uncond && out, op, ts, ts_stride, nullptr, nullptr, rows, C, 0, stream);
}

namespace {
// one segment of the predictor: the checks of its outputs and GE state, and the Op.  d NULL: the Euler step with GE (xp is the new latent)
int heun_predict_segment(const char* who, const float* x, const float* vel_cond, const float* vel_uncond, const float* clean, float cfg_scale,
                         float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* d, float* xp, HeunPredict& op) {
    LTX2_CHECK_ARG(d || xp, "%s: d and xp are both NULL", who);
    LTX2_CHECK_ARG(ge_gamma >= 0.f && (prev != nullptr) == (ge_gamma > 0.f), "%s: a GE state goes with ge_gamma > 0 (ge_gamma=%g)", who, ge_gamma);
    op = {{}, {x, vel_cond, vel_uncond, clean, first ? nullptr : prev}, {d, xp, prev}, cfg_scale - 1.0f, 1.0f / sigma, sigma_next - sigma, sigma, ge_gamma};
    return LTX2_OK;
}
}  // namespace

int heun_predict_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                        const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* d, float* xp,
                        int rows, int C, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma > 0.f, "heun_predict: sigma=%g must be > 0", sigma);
    HeunPredict op;
    if (const int rc = heun_predict_segment("heun_predict", x, vel_cond, vel_uncond, clean, cfg_scale, ge_gamma, prev, first, sigma, sigma_next, d, xp, op); rc != LTX2_OK) return rc;
    return launch_rows("heun_predict", x && vel_cond, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int heun_predict_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                             const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_d, float* v_xp, int v_rows, int v_C,
                             const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                             const float* a_clean, float a_cfg_scale, float* a_d, float* a_xp, int a_rows, int a_C, float sigma, float sigma_next,
                             hipStream_t stream) {
    LTX2_CHECK_ARG(sigma > 0.f, "heun_predict_pair: sigma=%g must be > 0", sigma);
    LTX2_CHECK_ARG((v_d == nullptr) == (a_d == nullptr) && (v_xp == nullptr) == (a_xp == nullptr),
                   "heun_predict_pair: the form (d, xp, or both) applies to both segments together");
    HeunPredict v, a;
    if (const int rc = heun_predict_segment("heun_predict_pair", v_x, v_vel_cond, v_vel_uncond, v_clean, v_cfg_scale, ge_gamma, v_prev, first, sigma, sigma_next, v_d, v_xp, v); rc != LTX2_OK) return rc;
    if (const int rc = heun_predict_segment("heun_predict_pair", a_x, a_vel_cond, a_vel_uncond, a_clean, a_cfg_scale, 0.f, nullptr, 1, sigma, sigma_next, a_d, a_xp, a); rc != LTX2_OK) return rc;
    return launch_rows2("heun_predict_pair", v_x && v_vel_cond && a_x && a_vel_cond, v, {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a,
                        {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int heun_correct_launch(const float* x, const float* d, const float* xp, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride,
                        const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, float* out, int rows, int C,
                        hipStream_t stream) {
    LTX2_CHECK_ARG(sigma > 0.f && sigma_next > 0.f, "heun_correct: sigma=%g and sigma_next=%g must be > 0 (sigma_next == 0: the step ends with d)", sigma, sigma_next);
    const HeunCorrect op = {{}, {x, d, xp, vel_cond, vel_uncond, clean}, {out}, cfg_scale - 1.0f, 1.0f / sigma, 1.0f / sigma_next, sigma_next - sigma};
    return launch_rows("heun_correct", x && d && xp && vel_cond && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int heun_correct_pair_launch(const float* v_x, const float* v_d, const float* v_xp, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts,
                             long v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C,
                             const float* a_x, const float* a_d, const float* a_xp, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts,
                             long a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma,
                             float sigma_next, hipStream_t stream) {
    LTX2_CHECK_ARG(sigma > 0.f && sigma_next > 0.f, "heun_correct_pair: sigma=%g and sigma_next=%g must be > 0 (sigma_next == 0: the step ends with d)", sigma, sigma_next);
    const float inv = 1.0f / sigma, inv_next = 1.0f / sigma_next, dt = sigma_next - sigma;
    const HeunCorrect v = {{}, {v_x, v_d, v_xp, v_vel_cond, v_vel_uncond, v_clean}, {v_out}, v_cfg_scale - 1.0f, inv, inv_next, dt};
    const HeunCorrect a = {{}, {a_x, a_d, a_xp, a_vel_cond, a_vel_uncond, a_clean}, {a_out}, a_cfg_scale - 1.0f, inv, inv_next, dt};
    return launch_rows2("heun_correct_pair", v_x && v_d && v_xp && v_vel_cond && v_out && a_x && a_d && a_xp && a_vel_cond && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int ge_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                         const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* out, int rows,
                         int C, hipStream_t stream) {
    LTX2_CHECK_ARG(out && prev, "ge_euler_step: null operand or empty shape");
    return heun_predict_launch(x, vel_cond, vel_uncond, ts, ts_stride, mask, clean, cfg_scale, ge_gamma, prev, first, sigma, sigma_next, nullptr, out, rows, C,
                               stream);
}

int ge_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                              const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_out, int v_rows, int v_C,
                              const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                              const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next, hipStream_t stream) {
    LTX2_CHECK_ARG(v_out && a_out && v_prev, "ge_euler_step_pair: null operand or empty shape");
    return heun_predict_pair_launch(v_x, v_vel_cond, v_vel_uncond, v_ts, v_ts_stride, v_mask, v_clean, v_cfg_scale, ge_gamma, v_prev, first, nullptr, v_out,
                                    v_rows, v_C, a_x, a_vel_cond, a_vel_uncond, a_ts, a_ts_stride, a_mask, a_clean, a_cfg_scale, nullptr, a_out, a_rows, a_C, sigma,
                                    sigma_next, stream);
}

namespace {
// what the ancestral steps check of their scalars and their seed
int ancestral_check(const char* who, float sigma, float sigma_up, float sigma_down, const uint64_t* seed_dev) {
    LTX2_CHECK_ARG(sigma != 0.f, "Sigma can't be 0.0");   // reference core_utils.py:54-55
    LTX2_CHECK_ARG(sigma_up >= 0.f && sigma_down >= 0.f, "%s: sigma_up=%g and sigma_down=%g must be >= 0", who, sigma_up, sigma_down);
    LTX2_CHECK_ARG(seed_dev && ((uintptr_t)seed_dev & 7) == 0, "%s: seed_dev is a device pointer to one 8-byte aligned 64-bit word", who);
    return LTX2_OK;
}
}  // namespace

int philox_bits_launch(uint32_t* out, long n_quads, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, hipStream_t stream) {
    LTX2_CHECK_ARG(out && n_quads > 0 && seed_dev && ((uintptr_t)seed_dev & 7) == 0, "philox_bits: null operand, empty shape or a seed off its 8-byte boundary");
    hipLaunchKernelGGL(philox_bits_kernel, dim3(grid_for(n_quads, BLOCK)), dim3(BLOCK), 0, stream, out, n_quads, Noise{seed_dev, step, stream_id});
    LTX2_CHECK_LAUNCH("philox_bits_kernel");
    return LTX2_OK;
}

int philox_normal_launch(float* out, long n, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, hipStream_t stream) {
    LTX2_CHECK_ARG(out && n > 0 && seed_dev && ((uintptr_t)seed_dev & 7) == 0, "philox_normal: null operand, empty shape or a seed off its 8-byte boundary");
    hipLaunchKernelGGL(philox_normal_kernel, dim3(grid_for((n + 3) / 4, BLOCK)), dim3(BLOCK), 0, stream, out, n, Noise{seed_dev, step, stream_id});
    LTX2_CHECK_LAUNCH("philox_normal_kernel");
    return LTX2_OK;
}

int ancestral_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                                const float* clean, float cfg_scale, float sigma, float sigma_up, float sigma_down, const uint64_t* seed_dev,
                                uint32_t step, float* out, int rows, int C, hipStream_t stream) {
    if (const int rc = ancestral_check("ancestral_euler_step", sigma, sigma_up, sigma_down, seed_dev); rc != LTX2_OK) return rc;
    const AncestralEuler op = {{}, {x, vel_cond, vel_uncond, clean}, {out}, cfg_scale - 1.0f, 1.0f / sigma, sigma_down - sigma, sigma_up, {seed_dev, step, 0}};
    return launch_rows("ancestral_euler_step", x && vel_cond && out, op, ts, ts_stride, mask, clean, rows, C, 0, stream);
}

int ancestral_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride,
                                     const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                     const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                                     const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_up,
                                     float sigma_down, const uint64_t* seed_dev, uint32_t step, hipStream_t stream) {
    if (const int rc = ancestral_check("ancestral_euler_step_pair", sigma, sigma_up, sigma_down, seed_dev); rc != LTX2_OK) return rc;
    const float inv = 1.0f / sigma, dt = sigma_down - sigma;
    const AncestralEuler v = {{}, {v_x, v_vel_cond, v_vel_uncond, v_clean}, {v_out}, v_cfg_scale - 1.0f, inv, dt, sigma_up, {seed_dev, step, 0}};
    const AncestralEuler a = {{}, {a_x, a_vel_cond, a_vel_uncond, a_clean}, {a_out}, a_cfg_scale - 1.0f, inv, dt, sigma_up, {seed_dev, step, 1}};
    return launch_rows2("ancestral_euler_step_pair", v_x && v_vel_cond && v_out && a_x && a_vel_cond && a_out, v,
                        {v_ts, v_ts_stride, v_mask, v_clean, v_rows, v_C}, a, {a_ts, a_ts_stride, a_mask, a_clean, a_rows, a_C}, stream);
}

int ancestral_euler_step_x0_launch(const float* x, const float* x0, const float* mask, const float* clean, float sigma, float sigma_up, float sigma_down,
                                   const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, float* out, int rows, int C, hipStream_t stream) {
    if (const int rc = ancestral_check("ancestral_euler_step_x0", sigma, sigma_up, sigma_down, seed_dev); rc != LTX2_OK) return rc;
    const AncestralFromX0 op = {{}, {x, x0, clean}, {out}, 1.0f / sigma, sigma_down - sigma, sigma_up, {seed_dev, step, stream_id}};
    static_assert(!AncestralFromX0::reads_t, "the launch below passes no timesteps");
    return launch_rows("ancestral_euler_step_x0", x && x0 && out, op, nullptr, 0, mask, clean, rows, C, 0, stream, true);
}
