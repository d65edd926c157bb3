// paper_sampler's per-set statistics beyond the eight Eigen values (hem/models/paper_sampler.py:337-342): the per-image mean
// absolute error (mean and min over the batch) and tf.nn.moments(., axes=0) of g and y_hat averaged over the pixels, plus the
// per-pixel mean / variance images of y_hat (the uncertainty map of sample()).  y_hat is rounded in f32 the way the head stores
// it; everything after that is f64, the variance two-pass.  No float atomics: per-block partials, finished in block, slice and
// image order, so two launches are bit-equal.  Memory-bound; wave64 throughout.
#include "tdg_cgan_common.h"

namespace {

constexpr int kMomCols = 4;                                  // block partials behind the n per-image ones: mean g, var g, mean y_hat, var y_hat

// the prediction forms of tdg_cgan_eval_batch: image[p] * scale, or pred[b, p] + offset[b] (either nullable: 0), f32
__device__ __forceinline__ float prediction(const float* pred, const float* offset, const float* image, float scale, int b, int p,
                                            int hw) {
  if (image) return image[p] * scale + 0.f;
  return (pred ? pred[(size_t)b * hw + p] : 0.f) + (offset ? offset[b] : 0.f);
}

// A block owns 64 consecutive pixels, wave w the images b = w, w + 8, ...: every load of a wave is one contiguous run of an
// image -- the recipe of slice_moments (tdg_cgan_common.h), written out here because the first pass also carries the per-image
// error sums and g and y_hat share its barriers.  part[blk][b] (b < n) = that image's sum of |y - y_hat| over the block's
// pixels; part[blk][n + k] = the block's sum over its pixels of the batch mean / variance of g (k = 0, 1) and y_hat (k = 2, 3).
__global__ void __launch_bounds__(64 * kSlices) sample_stats_kernel(const float* __restrict__ y, const float* __restrict__ g,
                                                                    const float* __restrict__ pred, const float* __restrict__ offset,
                                                                    const float* __restrict__ image, float scale, int n, int hw,
                                                                    double unit, double* __restrict__ part,
                                                                    float* __restrict__ mean_img, float* __restrict__ var_img) {
  __shared__ double sh[2][kSlices][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int p = blockIdx.x * 64 + lane;
  const bool ok = p < hw;
  double* pb = part + (size_t)blockIdx.x * (n + kMomCols);
  double sg = 0.0, sy = 0.0;
  for (int b = sl; b < n; b += kSlices) {                    // (uniform per wave)
    double a = 0.0;
    if (ok) {
      const double yh = (double)prediction(pred, offset, image, scale, b, p, hw);
      sy += yh;
      if (g) sg += (double)g[(size_t)b * hw + p];
      a = fabs((double)y[(size_t)b * hw + p] - yh);
    }
    a = wave_sum(a);
    if (lane == 0) pb[b] = a;
  }
  sh[0][sl][lane] = sg;
  sh[1][sl][lane] = sy;
  __syncthreads();
  double mg = 0.0, my = 0.0;
  for (int k = 0; k < kSlices; ++k) { mg += sh[0][k][lane]; my += sh[1][k][lane]; }     // every wave: the same order
  mg /= (double)n;
  my /= (double)n;
  __syncthreads();
  double qg = 0.0, qy = 0.0;
  if (ok)
    for (int b = sl; b < n; b += kSlices) {
      const double dy = (double)prediction(pred, offset, image, scale, b, p, hw) - my;
      qy += dy * dy;
      if (g) {
        const double dg = (double)g[(size_t)b * hw + p] - mg;
        qg += dg * dg;
      }
    }
  sh[0][sl][lane] = qg;
  sh[1][sl][lane] = qy;
  __syncthreads();
  if (sl != 0) return;
  double vg = 0.0, vy = 0.0;
  for (int k = 0; k < kSlices; ++k) { vg += sh[0][k][lane]; vy += sh[1][k][lane]; }
  vg /= (double)n;
  vy /= (double)n;
  if (ok && mean_img) {
    mean_img[p] = (float)(my / unit);
    var_img[p] = (float)(vy / (unit * unit));
  }
  const double t0 = wave_sum(ok ? mg : 0.0), t1 = wave_sum(ok ? vg : 0.0), t2 = wave_sum(ok ? my : 0.0), t3 = wave_sum(ok ? vy : 0.0);
  if (lane == 0) {
    pb[n] = t0;
    pb[n + 1] = t1;
    pb[n + 2] = t2;
    pb[n + 3] = t3;
  }
}

// one block: thread t sums the images b = t, t + 256, ... (each over the blocks in block order), thread 0 combines the
// threads in thread order; out = per_image_rmse/mean, /min, g_moments/mean, /var, y_hat_moments/mean, /var
__global__ void __launch_bounds__(256) sample_stats_finish_kernel(const double* __restrict__ part, int nblk, int n, int hw, double unit,
                                                                  float* __restrict__ out) {
  __shared__ double sum_sh[256], min_sh[256];
  const int t = threadIdx.x, cols = n + kMomCols;
  double s = 0.0, m = INFINITY;
  for (int b = t; b < n; b += 256) {
    double a = 0.0;
    for (int k = 0; k < nblk; ++k) a += part[(size_t)k * cols + b];
    a /= (double)hw;
    s += a;
    m = fmin(m, a);
  }
  sum_sh[t] = s;
  min_sh[t] = m;
  __syncthreads();
  if (t == 0) {
    s = 0.0;
    m = INFINITY;
    for (int k = 0; k < 256; ++k) { s += sum_sh[k]; m = fmin(m, min_sh[k]); }
    out[0] = (float)(s / (double)n / unit);
    out[1] = (float)(m / unit);
  } else if (t <= kMomCols) {
    const int c = t - 1;
    double a = 0.0;
    for (int k = 0; k < nblk; ++k) a += part[(size_t)k * cols + n + c];
    out[2 + c] = (float)(a / (double)hw / ((c & 1) ? unit * unit : unit));
  }
}

}  // namespace

extern "C" size_t tdg_cgan_sample_stats_workspace_bytes(int n, int hw) {
  return n > 0 && hw > 0 ? (size_t)tdg_ceil_div(hw, 64) * (size_t)(n + kMomCols) * sizeof(double) : 0;
}

extern "C" int tdg_cgan_sample_stats(const float* y, const float* g, const float* pred, const float* offset, const float* image,
                                     float image_scale, int n, int hw, float unit, float* out, float* mean_img, float* var_img,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(y && out && workspace && n > 0 && hw > 0 && unit > 0.f && (!mean_img == !var_img) && (!image || (!pred && !offset)),
                "tdg_cgan_sample_stats: bad argument (n %d, hw %d, unit %g)", n, hw, (double)unit);
  if (workspace_bytes < tdg_cgan_sample_stats_workspace_bytes(n, hw)) {
    tdg_set_error("tdg_cgan_sample_stats: workspace of %zu bytes, %zu needed", workspace_bytes,
                  tdg_cgan_sample_stats_workspace_bytes(n, hw));
    return TDG_EWORKSPACE;
  }
  const int nblk = tdg_ceil_div(hw, 64);
  double* part = static_cast<double*>(workspace);
  tdg_timing_start("cgan_sample_stats", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(sample_stats_kernel, dim3(nblk), dim3(64 * kSlices), 0, (hipStream_t)stream, y, g, pred, offset, image,
                     image_scale, n, hw, (double)unit, part, mean_img, var_img);
  hipLaunchKernelGGL(sample_stats_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nblk, n, hw, (double)unit, out);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_sample_stats");
  return TDG_OK;
}
