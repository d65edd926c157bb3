// Whole-frame sampling of paper_sampler / paper_noise (SamplerReplica.sample_full): the window grid of tdg_cgan_full.hip with
// every window repeated `rep` times in the staging buffers -- the sampler set's batch of copies of ONE image, one noise draw per
// copy (hem/models/paper_sampler.py:88-101) -- and the reduction of each group of draws to the per-pixel mean and variance that
// the frame blend takes.  y_hat is read as the head stored it (f32); everything after that is f64, the variance two-pass.  No
// float atomics: fixed slice and draw order, so two launches are bit-equal.  Memory- and latency-bound; wave64 throughout.
#include <math.h>

#include "tdg_common.h"

namespace {

constexpr int kSrc = 65, kCrop = 29, kCrop2 = kCrop * kCrop;
constexpr int kMinSide = kSrc + kCrop - 1;               // 93: a side needs more than this for one window
constexpr int kSlices = 8;                               // waves of a block: each takes every 8th draw
constexpr int kColBlocks = (kCrop2 + 63) / 64;           // 14 blocks of 64 pixels
constexpr int kRow = kSrc * 3 + kSrc;                    // a staged row: 195 image floats, then 65 depth floats
constexpr int kWindow = kSrc * kRow;

inline int grid_for(size_t n) {
  const size_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

inline int grid_count(int side, int s) { return (side - kMinSide) / s; }

__device__ __forceinline__ double wsum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- repeated patch gather: window c = chunk * G + g into rows [g rep, g rep + rep) of x [B,65,65,3] / y [B,65,65,1] ---------
// One thread per (window, staged float, copy slice): it reads its float once and writes the copies j = slice, slice + nsl, ...
// Consecutive lanes hold consecutive floats of a staged row, contiguous in the frame and in every copy.
__global__ void __launch_bounds__(256) full_gather_rep_kernel(const float* __restrict__ image, const float* __restrict__ depth, int W,
                                                              int s, int cols, int P, const int* __restrict__ chunk, int G, int rep,
                                                              int nsl, float* __restrict__ x, float* __restrict__ y) {
  const long long base = (long long)*chunk * G;
  const size_t total = (size_t)G * nsl * kWindow;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int gs = (int)(i / kWindow);                      // (window, slice), slice fastest
    const int rem = (int)(i - (size_t)gs * kWindow);
    const int g = gs / nsl, sl = gs - g * nsl;
    const int r = rem / kRow, k = rem - r * kRow;
    const long long c = base + g;
    const bool rgb = k < kSrc * 3;
    float v = 0.f;
    if (c >= 0 && c < P) {                                  // slots past the grid are zero, as the reference pads
      const int n = (int)c / cols, m = (int)c - n * cols;
      const size_t row = (size_t)(m * s + r) * W + n * s;
      v = rgb ? image[row * 3 + k] : (depth ? depth[row + (k - kSrc * 3)] : 0.f);
    }
    for (int j = sl; j < rep; j += nsl) {
      const size_t b = (size_t)g * rep + j;
      if (rgb) x[(b * kSrc + r) * (kSrc * 3) + k] = v;
      else y[(b * kSrc + r) * kSrc + (k - kSrc * 3)] = v;
    }
  }
}

// ---- sample store: group k (rows [k draws, k draws + draws)) to slot chunk * groups + k ------------------------------------
// blockIdx.y is the group.  Blocks x < 14 own 64 consecutive pixels, wave w the draws d = w, w + 8, ...: every load of a wave is
// one contiguous run of a draw; the slices meet in LDS in slice order.  Block x == 14 (launched only with a crop) owns the
// group's per-draw errors: wave w sums |crop - y_hat| of its draws over all the pixels, keeps their sum and min in draw order,
// and wave 0 combines the slices in slice order.
__global__ void __launch_bounds__(64 * kSlices) full_sample_store_kernel(const float* __restrict__ yhat, const float* __restrict__ ybar,
                                                                         const float* __restrict__ crop, int draws, int groups,
                                                                         long long slots, const int* __restrict__ chunk,
                                                                         float* __restrict__ st_yhat, float* __restrict__ st_var,
                                                                         float* __restrict__ st_ybar, float* __restrict__ st_err) {
  __shared__ double sh[kSlices][64];
  const long long base = (long long)*chunk * groups;
  if (base < 0 || base + groups > slots) return;            // a store past its slots writes nothing (uniform: before any barrier)
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int k = blockIdx.y;
  const size_t slot = (size_t)base + k;
  const float* yh = yhat + (size_t)k * draws * kCrop2;
  if (blockIdx.x == kColBlocks) {                           // ---- the group's per-draw mean absolute errors
    const float* cr = crop + (size_t)k * draws * kCrop2;
    double s = 0.0, m = INFINITY;
    for (int d = sl; d < draws; d += kSlices) {             // (uniform per wave)
      double a = 0.0;
#pragma unroll
      for (int it = 0; it < kColBlocks; ++it) {
        const int p = it * 64 + lane;
        if (p < kCrop2) a += fabs((double)cr[(size_t)d * kCrop2 + p] - (double)yh[(size_t)d * kCrop2 + p]);
      }
      a = wsum64(a) / (double)kCrop2;                       // (lane 0 holds the draw's value)
      s += a;
      m = fmin(m, a);
    }
    if (lane == 0) {
      sh[sl][0] = s;
      sh[sl][1] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      s = 0.0;
      m = INFINITY;
      for (int w = 0; w < kSlices; ++w) { s += sh[w][0]; m = fmin(m, sh[w][1]); }
      st_err[slot * 2] = (float)(s / (double)draws / 10.0);
      st_err[slot * 2 + 1] = (float)(m / 10.0);
    }
    return;
  }
  const int p = blockIdx.x * 64 + lane;
  const bool ok = p < kCrop2;
  double sy = 0.0;
  if (ok)
    for (int d = sl; d < draws; d += kSlices) sy += (double)yh[(size_t)d * kCrop2 + p];
  sh[sl][lane] = sy;
  __syncthreads();
  double my = 0.0;
  for (int w = 0; w < kSlices; ++w) my += sh[w][lane];      // every wave: the same order
  my /= (double)draws;
  __syncthreads();
  double qy = 0.0;
  if (ok)
    for (int d = sl; d < draws; d += kSlices) {
      const double dy = (double)yh[(size_t)d * kCrop2 + p] - my;
      qy += dy * dy;
    }
  sh[sl][lane] = qy;
  __syncthreads();
  if (sl != 0) return;
  double vy = 0.0;
  for (int w = 0; w < kSlices; ++w) vy += sh[w][lane];
  vy /= (double)draws;
  if (ok) {
    st_yhat[slot * kCrop2 + p] = (float)my;                 // 10x depth, as tdg_cgan_full_store writes
    st_var[slot * kCrop2 + p] = (float)(vy / 100.0);        // [0, 1] units
  }
  if (blockIdx.x == 0 && lane == 0) st_ybar[slot] = ybar ? ybar[(size_t)k * draws] : 0.f;
}

__global__ void full_sample_next_chunk_kernel(int* chunk) {
  if (threadIdx.x == 0) chunk[0] += 1;
}

}  // namespace

extern "C" int tdg_cgan_full_gather_rep(const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch,
                                        int rep, float* x_stage, float* y_stage, void* stream) {
  TDG_CHECK_ARG(image && chunk && x_stage && y_stage && H > kMinSide && W > kMinSide && stride >= 1 && batch > 0,
                "tdg_cgan_full_gather_rep: bad argument (H %d, W %d, stride %d, batch %d)", H, W, stride, batch);
  TDG_CHECK_ARG(rep >= 1 && batch % rep == 0, "tdg_cgan_full_gather_rep: rep %d must be at least 1 and divide batch %d", rep, batch);
  const int cols = grid_count(H, stride), rows = grid_count(W, stride);
  const int G = batch / rep, nsl = rep < kSlices ? rep : kSlices;
  tdg_timing_start("cgan_full_gather_rep", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(full_gather_rep_kernel, dim3(grid_for((size_t)G * nsl * kWindow)), dim3(256), 0, (hipStream_t)stream, image, depth,
                     W, stride, cols > 0 ? cols : 1, cols * rows, chunk, G, rep, nsl, x_stage, y_stage);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_gather_rep");
  return TDG_OK;
}

extern "C" int tdg_cgan_full_sample_store(const float* yhat, const float* ybar, const float* crop, int batch, int draws, long long slots,
                                          int* chunk, float* store_yhat, float* store_var, float* store_ybar, float* store_err,
                                          void* stream) {
  TDG_CHECK_ARG(yhat && chunk && store_yhat && store_var && store_ybar && batch > 0,
                "tdg_cgan_full_sample_store: bad argument (batch %d, draws %d, slots %lld)", batch, draws, slots);
  TDG_CHECK_ARG(draws >= 1 && batch % draws == 0, "tdg_cgan_full_sample_store: draws %d must be at least 1 and divide batch %d", draws,
                batch);
  TDG_CHECK_ARG(!crop == !store_err, "tdg_cgan_full_sample_store: crop and store_err must both be given or both be null");
  const int groups = batch / draws;
  TDG_CHECK_ARG(groups <= 65535 && slots >= groups, "tdg_cgan_full_sample_store: %d groups, the store holds %lld slots", groups, slots);
  tdg_timing_start("cgan_full_sample_store", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(full_sample_store_kernel, dim3(kColBlocks + (crop ? 1 : 0), groups), dim3(64 * kSlices), 0, (hipStream_t)stream,
                     yhat, ybar, crop, draws, groups, slots, chunk, store_yhat, store_var, store_ybar, store_err);
  hipLaunchKernelGGL(full_sample_next_chunk_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, chunk);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_sample_store");
  return TDG_OK;
}
