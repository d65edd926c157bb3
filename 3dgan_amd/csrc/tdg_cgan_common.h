// What the depth models' .hip files (tdg_cgan*.hip) and tdg_cgan_metrics.h share, stated once: the window geometry, the
// grid of a one-thread-per-element launch, the 64-lane wave sum, the four-wave block total and the per-pixel batch moments
// of a block of eight slices.  Every combination has a fixed order, so two launches are bit-equal.
#pragma once
#include <math.h>

#include "tdg_common.h"

namespace {

constexpr int kSrc = 65, kCrop = 29, kCrop2 = kCrop * kCrop;      // the window, the generator's output, its 841 pixels
constexpr int kOff = 17;                                 // paper_cgan.py:93-94: crop_to_bounding_box(y * 10, 17, 17, 29, 29)
constexpr int kMinSide = kSrc + kCrop - 1;               // 93: a frame side needs more than this for one window
constexpr int kSlices = 8;                               // waves of a moments block: each takes every 8th image

// blocks of 256 threads, one element per thread, grid-stride beyond 2048 blocks
inline int grid_for(size_t n) {
  const size_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// the wave's sum in lane 0 (f32, f64 and the u64 hit counts)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// a 256-thread block's total from its four wave sums in LDS, in wave order
template <typename T>
__device__ __forceinline__ T block_total(const T* sh) {
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// the lane's column of the eight slices' values in LDS, added in slice order
__device__ __forceinline__ double slice_total(const double (*sh)[64]) {
  double t = 0.0;
  for (int k = 0; k < kSlices; ++k) t += sh[k][threadIdx.x & 63];
  return t;
}

// Per-pixel batch moments (tf.nn.moments(., axes=0)) in a block of 64 * kSlices threads that owns 64 consecutive pixels:
// lane's pixel p (ok: it exists) of the n images y [n, hw], wave sl taking the images b = sl, sl + 8, ... so that every
// load of a wave is one contiguous run of an image.  Two passes in f64: the batch mean, then the sum of the squared
// deviations from it; the slices meet in LDS in slice order.  Three barriers, which every thread of the block must reach.
// Returns the mean in every wave and leaves the slices' sums of squared deviations in sh, behind the third barrier:
// slice_total(sh) / n is the variance.
__device__ __forceinline__ double slice_moments(const float* __restrict__ y, int n, int hw, int p, bool ok, double (*sh)[64]) {
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  double s = 0.0;
  if (ok)
    for (int b = sl; b < n; b += kSlices) s += (double)y[(size_t)b * hw + p];
  sh[sl][lane] = s;
  __syncthreads();
  const double mean = slice_total(sh) / (double)n;                 // every wave: the same order
  __syncthreads();
  double q = 0.0;
  if (ok)
    for (int b = sl; b < n; b += kSlices) {
      const double d = (double)y[(size_t)b * hw + p] - mean;
      q += d * d;
    }
  sh[sl][lane] = q;
  __syncthreads();
  return mean;
}

}  // namespace
