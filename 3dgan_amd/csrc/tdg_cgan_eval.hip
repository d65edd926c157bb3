// paper_cgan dataset evaluation (paper/paper_metrics.py and the mean / variance image pre-pass of paper/paper_train.py:43-60,
// 130-132 of the thesis code): per batch, the Eigen-2014 metrics of up to three predictors from ONE read of the depth crop
// and of y_hat, and the per-pixel batch moments; everything is added into a device-resident f64 accumulator block, which one
// finish launch turns into the sweep's results.  No float atomics: per-block f64 partials finished in block order, so two
// runs are bit-equal.  All of these are memory-bound; wave64 throughout.
//
// Accumulator block (doubles), hw = pixels of one image:
//   [set * 9 + k]  k < 8: sum over batches of value k of set `set` (METRIC_KEYS order); k = 8: batches added to that set
//   [27]           batches added to the moments
//   [28 + p]       sum over batches of the batch mean of pixel p;  [28 + hw + p]  of its batch variance
#include "tdg_cgan_metrics.h"

namespace {

constexpr int kSets = 3, kSetStride = 9, kMomBatches = kSets * kSetStride, kMomBase = kMomBatches + 1;
constexpr int kScalars = 12;                                // per set: 8 means, 3 final percentages, batches

// ---- fused batch evaluation: the block partition of cgan_metrics_kernel, up to three sets per element ---------------
// set 0: pred[i];  set 1: offset[i / hw] (nullable: 0);  set 2: image[i % hw] * image_scale (f32)
__global__ void __launch_bounds__(256) eval_batch_kernel(const float* __restrict__ y, const float* __restrict__ pred,
                                                         const float* __restrict__ offset, const float* __restrict__ image,
                                                         float image_scale, int n, int hw, int sets, MetricPartial* __restrict__ part) {
  __shared__ double shd[kSets][5][4];
  __shared__ unsigned long long shh[kSets][3][4];
  double s[kSets][5] = {};
  unsigned long long h[kSets][3] = {};
  const size_t total = (size_t)n * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / hw), p = (int)(i - (size_t)b * hw);
    const float yv = y[i];
    if (sets & 1) metric_terms(yv, pred[i] + 0.f, s[0], h[0]);
    if (sets & 2) metric_terms(yv, 0.f + (offset ? offset[b] : 0.f), s[1], h[1]);
    if (sets & 4) metric_terms(yv, image[p] * image_scale + 0.f, s[2], h[2]);
  }
#pragma unroll
  for (int k = 0; k < kSets; ++k)
    if (sets >> k & 1) metric_wave_sums(s[k], h[k], shd[k], shh[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < kSets; ++k)
      if (sets >> k & 1) part[k * kMetricBlocks + blockIdx.x] = metric_block_total(shd[k], shh[k]);
  }
}

// one thread per set: this batch's eight values, added to the set's sums
__global__ void eval_batch_finish_kernel(const MetricPartial* __restrict__ part, int nblk, unsigned long long total, int sets,
                                         unsigned long long* __restrict__ counts, double* __restrict__ acc) {
  const int k = threadIdx.x;
  if (k >= kSets || !(sets >> k & 1)) return;
  double v[8];
  metric_values(part + k * kMetricBlocks, nblk, total, counts + k * 4, v);
  double* a = acc + k * kSetStride;
  for (int j = 0; j < 8; ++j) a[j] += v[j];
  a[8] += 1.0;
}

// ---- per-pixel batch moments (tf.nn.moments(y, axes=0)): a block owns 64 consecutive pixels, slice_moments does the rest
__global__ void __launch_bounds__(64 * kSlices) eval_moments_kernel(const float* __restrict__ y, int n, int hw,
                                                                    double* __restrict__ acc) {
  __shared__ double sh[kSlices][64];
  const int p = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool ok = p < hw;
  const double mean = slice_moments(y, n, hw, p, ok, sh);
  if (threadIdx.x < 64 && ok) {
    acc[kMomBase + p] += mean;
    acc[kMomBase + hw + p] += slice_total(sh) / (double)n;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) acc[kMomBatches] += 1.0;
}

// ---- finish: the accumulators to results ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) eval_finish_kernel(const double* __restrict__ acc, const unsigned long long* __restrict__ counts,
                                                          int hw, double unit, double* __restrict__ scalars,
                                                          float* __restrict__ mean_img, float* __restrict__ var_img) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < kSets) {
    const double* a = acc + t * kSetStride;
    double* o = scalars + t * kScalars;
    for (int j = 0; j < 8; ++j) o[j] = a[j] / a[8];
    for (int j = 0; j < 3; ++j) o[8 + j] = (double)counts[t * 4 + j] / (double)counts[t * 4 + 3];
    o[11] = a[8];
  }
  if (t < hw && mean_img) {
    const double nb = acc[kMomBatches];
    mean_img[t] = (float)(acc[kMomBase + t] / nb / unit);
    var_img[t] = (float)(acc[kMomBase + hw + t] / nb / (unit * unit));
  }
}

}  // namespace

extern "C" size_t tdg_cgan_eval_workspace_bytes(void) { return (size_t)kSets * kMetricBlocks * sizeof(MetricPartial); }

extern "C" size_t tdg_cgan_eval_acc_bytes(int hw) { return hw > 0 ? (size_t)(kMomBase + 2 * (size_t)hw) * sizeof(double) : 0; }

extern "C" int tdg_cgan_eval_batch(const float* y, const float* pred, const float* offset, const float* image, float image_scale,
                                   int n, int hw, int sets, unsigned long long* counts, double* acc, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(y && counts && acc && workspace && n > 0 && hw > 0 && sets > 0 && sets < (1 << kSets) && (!(sets & 1) || pred) &&
                    (!(sets & 4) || image),
                "tdg_cgan_eval_batch: bad argument (n %d, hw %d, sets %d)", n, hw, sets);
  if (workspace_bytes < tdg_cgan_eval_workspace_bytes()) {
    tdg_set_error("tdg_cgan_eval_batch: workspace of %zu bytes, %zu needed", workspace_bytes, tdg_cgan_eval_workspace_bytes());
    return TDG_EWORKSPACE;
  }
  const size_t total = (size_t)n * hw;
  const int nblk = metric_blocks(total);
  MetricPartial* part = static_cast<MetricPartial*>(workspace);
  tdg_timing_start("cgan_eval_batch", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(eval_batch_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, y, pred, offset, image, image_scale, n, hw,
                     sets, part);
  hipLaunchKernelGGL(eval_batch_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, nblk, (unsigned long long)total, sets,
                     counts, acc);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_eval_batch");
  return TDG_OK;
}

extern "C" int tdg_cgan_eval_moments(const float* y, int n, int hw, double* acc, void* stream) {
  TDG_CHECK_ARG(y && acc && n > 0 && hw > 0, "tdg_cgan_eval_moments: bad argument (n %d, hw %d)", n, hw);
  tdg_timing_start("cgan_eval_moments", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(eval_moments_kernel, dim3(tdg_ceil_div(hw, 64)), dim3(64 * kSlices), 0, (hipStream_t)stream, y, n, hw, acc);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_eval_moments");
  return TDG_OK;
}

extern "C" int tdg_cgan_eval_finish(const double* acc, const unsigned long long* counts, int hw, float unit, double* scalars,
                                    float* mean_img, float* var_img, void* stream) {
  TDG_CHECK_ARG(acc && counts && scalars && hw > 0 && unit > 0.f && (!mean_img == !var_img),
                "tdg_cgan_eval_finish: bad argument (hw %d, unit %g)", hw, (double)unit);
  tdg_timing_start("cgan_eval_finish", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(tdg_ceil_div(hw, 256)), dim3(256), 0, (hipStream_t)stream, acc, counts, hw, (double)unit,
                     scalars, mean_img, var_img);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_eval_finish");
  return TDG_OK;
}
