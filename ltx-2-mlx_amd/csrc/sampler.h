// The sampling step over fp32 [rows][C] latents: host launchers (sampler.hip; the definitions: include/ltx2hip.h).
#pragma once
#include "common.h"

// x0[row][c] = latent[row][c] - ts(row) * vel[row][c]   (ts = ts_ptr[row*ts_stride] if ts_ptr else ts_scalar)
int x0_from_velocity_launch(const float* latent, const float* vel, const float* ts_ptr, long ts_stride, float ts_scalar,
                            float* x0, int rows, int C, hipStream_t stream);

// x0' = mask ? x0*mask(row) + clean*(1-mask(row)) : x0 ;  out = x + (x - x0')/sigma * (sigma_next - sigma)
int euler_step_launch(const float* x, const float* x0, const float* mask, const float* clean, float sigma,
                      float sigma_next, float* out, int rows, int C, hipStream_t stream);

// The steps below round every operation individually (the separate fp32 torch ops, bit for bit), read t = ts[row * ts_stride] with ts_stride 0 or
// 1, blend with `clean` where `mask` is given (both or neither), and may write any output over any [rows][C] input.

// One classifier-free-guided step in one pass:
// a = x - t*vc, b = x - t*vu, g = a + (cfg_scale - 1)*(a - b), d = mask ? g*m + clean*(1 - m) : g, out = x + ((x - d)/sigma)*(sigma_next - sigma)
int guided_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride,
                             const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, float* out,
                             int rows, int C, hipStream_t stream);

// The same step over the video and the audio latent in ONE launch (the joint guided loop of a retake with sound), v_ then a_, each with its own
// operands, cfg_scale, timesteps, mask / clean and shape; sigma / sigma_next are shared.  Each segment's output is the single launch's bit for bit.
int guided_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride,
                                  const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                  const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                                  const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next,
                                  hipStream_t stream);

// The same step with spatio-temporal guidance on top (STGGuider.guide applied to the CFG-guided x0; vel_perturbed: the velocity of the pass whose
// self-attentions were skipped): g as above (g = a when vel_uncond is NULL), p = x - t*vp, s = g + stg_scale*(g - p), then d and out from s
int stg_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* ts, long ts_stride,
                          const float* mask, const float* clean, float cfg_scale, float stg_scale, float sigma, float sigma_next, float* out, int rows,
                          int C, hipStream_t stream);

// The same step over the video and the audio latent in ONE launch (the joint STG loop), v_ then a_ as in guided_euler_step_pair_launch, each with its
// own cfg_scale and stg_scale.  Per segment vel_uncond may be NULL (no CFG) and vel_perturbed may be NULL (no STG term: s = g, the guided step's
// arithmetic).  Each segment's output is the single launch's bit for bit.
int stg_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed, const float* v_ts,
                               long v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float v_stg_scale, float* v_out, int v_rows,
                               int v_C, const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed,
                               const float* a_ts, long a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float a_stg_scale,
                               float* a_out, int a_rows, int a_C, float sigma, float sigma_next, hipStream_t stream);

// The res_2s second-order step as two passes; d(x, vc, vu) = the guided, mask-blended x0 in the HQ pipeline's order:
// a = x - t*vc, b = x - t*vu, g = b + cfg*(a - b) (g = a when vu is NULL), d = mask ? g*m + clean*(1 - m) : g.
// midpoint: an = x, e = d - an, xm = an + c*e, n_bong x {an = xm - c*e, e = d - an}; stores x_mid, anchor, eps1.
// anchor == eps1 == NULL: the final-step form, x_mid = d and nothing else.
int res2s_midpoint_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                          const float* clean, float cfg_scale, float c, int n_bong, float* x_mid, float* anchor, float* eps1, int rows, int C,
                          hipStream_t stream);
// combine: e2 = d(x_mid, vc, vu) - anchor, out = anchor + h*(b1*eps1 + b2*e2)
int res2s_combine_launch(const float* x_mid, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                         const float* clean, float cfg_scale, const float* anchor, const float* eps1, float h, float b1, float b2, float* out,
                         int rows, int C, hipStream_t stream);

// Both passes over TWO latents in one launch (the video and the audio latent of a joint step): the single forms' operands given twice, v_ then
// a_, each with its own cfg_scale, timesteps, mask / clean and shape; c / n_bong and h / b1 / b2 are shared.  Each segment's output is the single
// launch's bit for bit.  16-byte accesses only when both segments allow them; the final-step form applies to both segments together.
int res2s_midpoint_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                               const float* v_clean, float v_cfg_scale, float* v_x_mid, float* v_anchor, float* v_eps1, int v_rows, int v_C,
                               const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                               const float* a_clean, float a_cfg_scale, float* a_x_mid, float* a_anchor, float* a_eps1, int a_rows, int a_C,
                               float c, int n_bong, hipStream_t stream);
int res2s_combine_pair_launch(const float* v_x_mid, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                              const float* v_clean, float v_cfg_scale, const float* v_anchor, const float* v_eps1, float* v_out, int v_rows, int v_C,
                              const float* a_x_mid, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                              const float* a_clean, float a_cfg_scale, const float* a_anchor, const float* a_eps1, float* a_out, int a_rows, int a_C,
                              float h, float b1, float b2, hipStream_t stream);

// The Heun sampler as two passes (reference pipelines/one_stage.py:334-464), with the GE velocity correction (:300-307) in the first; inv = 1/sigma:
// predict: a = x - t*vc, b = x - t*vu, g = a + (cfg_scale - 1)*(a - b) (g = a when vu is NULL); with a GE state `prev` (ge_gamma > 0, else NULL):
//   cur = (x - g)*inv, unless `first` g = x - (ge_gamma*(cur - prev) + prev)*sigma, prev = cur; d = mask ? g*m + clean*(1 - m) : g,
//   xp = x + ((x - d)*inv)*(sigma_next - sigma); stores d, xp, prev.  xp NULL: the final-step form (sigma_next == 0: the step ends with d), d alone.
//   d NULL: the Euler step with GE, xp being the new latent (ge_euler_step_launch).
int heun_predict_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                        const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* d, float* xp,
                        int rows, int C, hipStream_t stream);
// correct: d2 = the guided, mask-blended x0 of (xp, vc, vu at sigma_next; ts = its timesteps), v1 = (x - d)*inv, v2 = (xp - d2)*(1/sigma_next),
//   out = x + (0.5*(v1 + v2))*(sigma_next - sigma)
int heun_correct_launch(const float* x, const float* d, const float* xp, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride,
                        const float* mask, const float* clean, float cfg_scale, float sigma, float sigma_next, float* out, int rows, int C,
                        hipStream_t stream);
int ge_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                         const float* clean, float cfg_scale, float ge_gamma, float* prev, int first, float sigma, float sigma_next, float* out, int rows,
                         int C, hipStream_t stream);
// The three over the video and the audio latent in ONE launch, v_ then a_; GE acts on the video alone (the reference keeps prev_velocity for it only).
// Each segment's output is the single launch's bit for bit; the predictor's form (d, xp or both) applies to both segments together.
int heun_predict_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                             const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_d, float* v_xp, int v_rows, int v_C,
                             const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                             const float* a_clean, float a_cfg_scale, float* a_d, float* a_xp, int a_rows, int a_C, float sigma, float sigma_next,
                             hipStream_t stream);
int heun_correct_pair_launch(const float* v_x, const float* v_d, const float* v_xp, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts,
                             long v_ts_stride, const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C,
                             const float* a_x, const float* a_d, const float* a_xp, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts,
                             long a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma,
                             float sigma_next, hipStream_t stream);
int ge_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, const float* v_mask,
                              const float* v_clean, float v_cfg_scale, float ge_gamma, float* v_prev, int first, float* v_out, int v_rows, int v_C,
                              const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                              const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next, hipStream_t stream);

// Guiders whose scalars are sums over the whole latent.  sums: five fp64 sums per block into partials[guidance_sums_blocks(rows, C)][5], and with
// `running` the momentum update of the guidance; step: every block adds the partial rows in index order, derives the fp32 scalars and runs the
// guided, mask-blended Euler step.
int guidance_sums_blocks(int rows, int C);
int guidance_sums_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, float* running, int first,
                         float momentum, double* partials, int rows, int C, hipStream_t stream);
int projected_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                                const float* clean, const float* running, const double* partials, int mode, float scale, float eta,
                                float norm_threshold, float sigma, float sigma_next, float* out, float* scalars_out, int rows, int C,
                                hipStream_t stream);

// Both passes over TWO latents in one launch (the video and the audio latent of a joint step), v_ then a_, each segment with its own operands,
// timesteps, running / first / momentum, partials region partials[guidance_sums_blocks(rows, C)][5], and in the step its own mode, scale, eta,
// norm_threshold, mask / clean and scalars_out; sigma / sigma_next are shared.  A segment's blocks index its own partials from 0 and add its own
// rows in index order, so its partials, running, scalars and output are the single launch's bit for bit at the same access width (16-byte only
// when both segments allow it; the order of the fp64 sums depends on the width).  The step's segments also take two guiders without sums,
// which read no partials (NULL) and report no scalars: PROJECTED_CFG, g_out = a + (scale - 1)*(a - b) as guided_euler_step, and PROJECTED_OFF,
// g_out = a (vel_uncond may be NULL).  sums: a segment with partials == NULL is left out (the other one's single launch); not both.
constexpr int PROJECTED_CFG = 3, PROJECTED_OFF = 4;
int guidance_sums_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride, float* v_running,
                              int v_first, float v_momentum, double* v_partials, int v_rows, int v_C, const float* a_x, const float* a_vel_cond,
                              const float* a_vel_uncond, const float* a_ts, long a_ts_stride, float* a_running, int a_first, float a_momentum,
                              double* a_partials, int a_rows, int a_C, hipStream_t stream);
int projected_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride,
                                     const float* v_mask, const float* v_clean, const float* v_running, const double* v_partials, int v_mode,
                                     float v_scale, float v_eta, float v_norm_threshold, float* v_out, float* v_scalars_out, int v_rows, int v_C,
                                     const float* a_x, const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride,
                                     const float* a_mask, const float* a_clean, const float* a_running, const double* a_partials, int a_mode,
                                     float a_scale, float a_eta, float a_norm_threshold, float* a_out, float* a_scalars_out, int a_rows, int a_C,
                                     float sigma, float sigma_next, hipStream_t stream);

// MultiModalGuider.calculate (reference components/guiders.py:244-273) and the step behind it.  With a = x - t*vc and u, p, m formed the same way from
// vel_uncond (negative prompt), vel_perturbed (self-attentions skipped) and vel_isolated (cross-modal attentions skipped), each term present exactly
// when its velocity is non-NULL:
//   pred = a [+ (cfg_scale - 1)*(a - u)] [+ stg_scale*(a - p)] [+ (modality_scale - 1)*(a - m)];  d = mask ? pred*m + clean*(1 - m) : pred;  out = euler(x, d)
int mm_guided_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                                const float* ts, long ts_stride, const float* mask, const float* clean, float cfg_scale, float stg_scale,
                                float modality_scale, float sigma, float sigma_next, float* out, int rows, int C, hipStream_t stream);
// the same over the video and the audio latent in one launch, each with its own scales; each segment's output is the single launch's bit for bit
int mm_guided_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_vel_perturbed,
                                     const float* v_vel_isolated, const float* v_ts, long v_ts_stride, const float* v_mask, const float* v_clean,
                                     float v_cfg_scale, float v_stg_scale, float v_modality_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                     const float* a_vel_cond, const float* a_vel_uncond, const float* a_vel_perturbed, const float* a_vel_isolated,
                                     const float* a_ts, long a_ts_stride, const float* a_mask, const float* a_clean, float a_cfg_scale, float a_stg_scale,
                                     float a_modality_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_next, hipStream_t stream);
// With rescale_scale != 0, two passes.  sums: the fp64 sums of a, a*a, pred, pred*pred per block into partials[guidance_sums_blocks(rows, C)][4]
// (pred_out, may be NULL: pred itself).  step: every block adds the partial rows in index order, var = (S2 - S1*S1/n)/n,
// f = fp32(rescale_scale*sqrt((var_a + 1e-8)/(var_p + 1e-8)) + (1 - rescale_scale)) in fp64, block 0 stores f to scalars_out; then the step above with pred*f
int mm_guidance_sums_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                            const float* ts, long ts_stride, float cfg_scale, float stg_scale, float modality_scale, double* partials, float* pred_out,
                            int rows, int C, hipStream_t stream);
int mm_rescaled_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* vel_perturbed, const float* vel_isolated,
                                  const float* ts, long ts_stride, const float* mask, const float* clean, const double* partials, float cfg_scale,
                                  float stg_scale, float modality_scale, float rescale_scale, float sigma, float sigma_next, float* out,
                                  float* scalars_out, int rows, int C, hipStream_t stream);

// Classifier-free guidance with the per-channel rescale of the standard one-stage loop (reference scripts/generate.py:688-727, :1935-1960).  With
// a = x - t*vc, b = x - t*vu, g = b + cfg_scale*(a - b), every operation rounded on its own:
// stats: per channel c, over all rows, mean and sqrt(mean((. - mean)^2) + 1e-8) of g[:, c] and of a[:, c] into fp32 stats[4][C] = mean_g, std_g,
//   mean_a, std_a.  Two launches: fp64 sums of (v - v0) and (v - v0)^2 (v0: the channel's value in row 0) per block of rows into
//   partials[channel_guidance_stats_blocks(rows, C)][4][C] (the last row holds the shifts), then one thread per channel adds the rows in index
//   order: mean = v0 + S1/n, var = max((S2 - S1*S1/n)/n, 0).  No atomics: the same bits from run to run.
// step: gr = ((g - mean_g)/std_g)*std_a + mean_a, g' = r*gr + (1 - r)*g with r = fp32(guidance_rescale) and (1 - r) = fp32(1 - guidance_rescale)
//   (stats NULL: g' = g), out = x + ((x - g')*(1/sigma))*(sigma_next - sigma).  out may be x.  No mask / clean: the route has no conditioning.
int channel_guidance_stats_blocks(int rows, int C);
int channel_guidance_stats_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, float cfg_scale,
                                  double* partials, float* stats, int rows, int C, hipStream_t stream);
int rescaled_guided_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* stats,
                                      float cfg_scale, double guidance_rescale, float sigma, float sigma_next, float* out, int rows, int C,
                                      hipStream_t stream);

// Counter-based noise: Philox4x32-10 with counter (lo32(q), hi32(q), step, stream_id) and key (lo32(seed), hi32(seed)) for quad q, whose four
// words serve the elements 4q .. 4q+3; seed_dev: one 64-bit word in device memory, read when the kernel runs.  bits: out[n_quads][4], the raw
// words.  normal: out[n], u_k = ((r_k >> 9) + 0.5)*2^-23, z0 = sqrt(-2 ln u0)*cos(2 pi u1), z1 = sqrt(-2 ln u0)*sin(2 pi u1), z2 / z3 from
// (u2, u3).  The values depend on (seed, step, stream_id, element index) alone.
int philox_bits_launch(uint32_t* out, long n_quads, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, hipStream_t stream);
int philox_normal_launch(float* out, long n, const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, hipStream_t stream);

// The Euler-ancestral step (reference components/diffusion_steps.py:70-129; sigma_up / sigma_down from _get_ancestral_step on the host):
// d as guided_euler_step_launch forms it, r = x + ((x - d)/sigma)*(sigma_down - sigma), out = r + ((z*sigma_up)*m) with z the element's
// philox_normal value (stream 0) and m the row's mask (1 without one).  vel_uncond NULL: no guidance, and r in the plain step's arithmetic
// (x0_from_velocity_launch, euler_step_launch).  sigma_up == 0: no noise is evaluated, out = r.
int ancestral_euler_step_launch(const float* x, const float* vel_cond, const float* vel_uncond, const float* ts, long ts_stride, const float* mask,
                                const float* clean, float cfg_scale, float sigma, float sigma_up, float sigma_down, const uint64_t* seed_dev,
                                uint32_t step, float* out, int rows, int C, hipStream_t stream);
// over the video (stream 0) and the audio latent (stream 1) in ONE launch, v_ then a_; each segment's output is the single launch's bit for bit
int ancestral_euler_step_pair_launch(const float* v_x, const float* v_vel_cond, const float* v_vel_uncond, const float* v_ts, long v_ts_stride,
                                     const float* v_mask, const float* v_clean, float v_cfg_scale, float* v_out, int v_rows, int v_C, const float* a_x,
                                     const float* a_vel_cond, const float* a_vel_uncond, const float* a_ts, long a_ts_stride, const float* a_mask,
                                     const float* a_clean, float a_cfg_scale, float* a_out, int a_rows, int a_C, float sigma, float sigma_up,
                                     float sigma_down, const uint64_t* seed_dev, uint32_t step, hipStream_t stream);
// from a ready x0, every operation rounded on its own: d = clean ? x0*m + clean*(1 - m) : x0.  A mask without a clean latent scales the noise alone.
int ancestral_euler_step_x0_launch(const float* x, const float* x0, const float* mask, const float* clean, float sigma, float sigma_up, float sigma_down,
                                   const uint64_t* seed_dev, uint32_t step, uint32_t stream_id, float* out, int rows, int C, hipStream_t stream);
