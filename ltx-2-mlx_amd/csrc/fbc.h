// First-block cache: the three element-wise kernels over the fp32 residual stream [N][D], taken as n = N*D elements.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// What fbc_head_metric leaves in device memory: the two sums and the decision (1: skip).  24 bytes, 8-byte aligned.
struct FbcRecord {
    double num, den;
    int skip, pad;
};

constexpr int FBC_MAX_BLOCKS = 1024;

// blocks of the metric's first launch, a function of n alone: one block per 2048 quads (8192 elements), FBC_MAX_BLOCKS at the most
int fbc_metric_blocks(long n);

// r = h1 - h0 (one fp32 subtraction per element) into `r`; num = sum |r - head_prev|, den = sum |head_prev| in fp64: every thread adds its quads
// (4 consecutive elements, quad q to thread q % (blocks*256)) in index order, the block's 256 values are added by a fixed tree into
// partials[block][2], and ONE finishing block adds those in a fixed order and writes `rec`: num, den, skip = (threshold > 0 && den > 0 &&
// num < threshold*den).  No atomics: the same inputs give the same record on every run, and the 16-byte and the element-wise form of the loads
// (chosen by the pointers' alignment) give the same record too.  head_prev NULL reads as zeros (den = 0: never a skip).  h1_save, may be NULL,
// receives a copy of h1; it may be the buffer h0 itself (each thread reads its elements of h0 before it writes them), nothing else may alias.
// partials: fbc_metric_blocks(n)*2 doubles.
int fbc_head_metric_launch(const float* h0, const float* h1, const float* head_prev, float* r, float* h1_save, double* partials, FbcRecord* rec,
                           float threshold, long n, hipStream_t stream);
// tail = hL - h1
int fbc_store_tail_launch(const float* hL, const float* h1, float* tail, long n, hipStream_t stream);
// h += tail, in place
int fbc_apply_tail_launch(float* h, const float* tail, long n, hipStream_t stream);
