// The Eigen-2014 depth metrics (hem/models/paper_cgan.py:447-478) stated once: the per-element terms, the block reduction
// and the eight values of one set.  Shared by tdg_cgan_metrics (tdg_cgan.hip) and the fused dataset evaluation
// (tdg_cgan_eval.hip), so that both give the same bits on the same data.
#pragma once
#include "tdg_cgan_common.h"

namespace {

constexpr int kMetricBlocks = 256;

struct MetricPartial {
  double s[5];
  unsigned long long hits[3];
};

// blocks of 256 threads, each striding over the n * hw elements: the partition both kernels use
inline int metric_blocks(size_t total) {
  const size_t b = (total + 1023) / 1024;
  return (int)(b < 1 ? 1 : (b > (size_t)kMetricBlocks ? (size_t)kMetricBlocks : b));
}

// per element (a = y / 10, p = pred / 10): |a-p|/p, (a-p)^2/p, (a-p)^2, d^2, d with d = log(a+1e-8) - log(p+1e-8);
// threshold hits: max(a/p, p/a) < 1.25^k with tf.maximum's NaN rule (x < y ? y : x).  f32 as the formulas are written,
// summed in f64.
__device__ __forceinline__ void metric_terms(float y10, float p10, double* s, unsigned long long* h) {
  const float a = y10 / 10.f;
  const float p = p10 / 10.f;
  const float e = a - p;
  const float d = logf(a + 1e-8f) - logf(p + 1e-8f);
  s[0] += (double)(fabsf(e) / p);
  s[1] += (double)(e * e / p);
  s[2] += (double)(e * e);
  s[3] += (double)(d * d);
  s[4] += (double)d;
  const float q1 = a / p, q2 = p / a;
  const float delta = q1 < q2 ? q2 : q1;
  h[0] += delta < 1.25f;
  h[1] += delta < 1.5625f;
  h[2] += delta < 1.953125f;
}

// a thread's sums to per-wave sums in LDS (256 threads: four waves); __syncthreads() before metric_block_total
__device__ __forceinline__ void metric_wave_sums(const double* s, const unsigned long long* h, double (*shd)[4],
                                                 unsigned long long (*shh)[4]) {
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double v = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) shd[k][wv] = v;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    unsigned long long v = h[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) shh[k][wv] = v;
  }
}

__device__ __forceinline__ MetricPartial metric_block_total(double (*shd)[4], unsigned long long (*shh)[4]) {
  MetricPartial m;
  for (int k = 0; k < 5; ++k) m.s[k] = block_total(shd[k]);
  for (int k = 0; k < 3; ++k) m.hits[k] = block_total(shh[k]);
  return m;
}

// The eight values of one set (METRIC_KEYS order) from its block partials, summed in block order; the streaming threshold
// totals counts[0..2] (hits) and counts[3] (elements) are advanced first, so v[5..7] are the running percentages.
__device__ __forceinline__ void metric_values(const MetricPartial* __restrict__ part, int nblk, unsigned long long total,
                                              unsigned long long* __restrict__ counts, double* v) {
  double s[5] = {0, 0, 0, 0, 0};
  unsigned long long h[3] = {0, 0, 0};
  for (int b = 0; b < nblk; ++b) {
    for (int k = 0; k < 5; ++k) s[k] += part[b].s[k];
    for (int k = 0; k < 3; ++k) h[k] += part[b].hits[k];
  }
  const double n = (double)total;
  v[0] = s[0] / n;
  v[1] = s[1] / n;
  v[2] = sqrt(s[2] / n);
  v[3] = sqrt(s[3] / n);
  v[4] = s[3] / n - s[4] * s[4] / (n * n);
  counts[3] += total;
  for (int k = 0; k < 3; ++k) {
    counts[k] += h[k];
    v[5 + k] = (double)counts[k] / (double)counts[3];
  }
}

}  // namespace
