// Activation montages for the training event files: what hem.summarize_layers(..., montage=True) (hem/ops/summaries.py:31-48)
// records per layer -- hem.montage (:139-181) of image 0's channel planes, encoded by tf.summary.image -- for a whole table
// of activations (jobs) in one batched entry.
//
// Layout.  A job is image 0 of an NHWC activation: h x w pixels of c live channels, pixel stride cs.  With
// (m, n) = factorization(c) -- m the largest divisor of c that is <= sqrt(c), n = c / m -- the montage is n*h rows by m*w
// columns of one byte each, channel j*m + i at block row j, block column i.
//
// Values: TensorFlow's rule for a float image (NormalizeFloatImage, summary_image_op.cc), restated in include/tdg.h: lo / hi
// over the finite elements, one f32 divide for the scale, then per pixel one f32 multiply, one f32 add (never fused), a
// minimum with 255 and truncation.  Non-finite pixels are 255.
//
// Scheme: two launches whatever njobs is.  montage_range_kernel, one block per job: thread t takes the live elements t,
// t + 256, ... (consecutive threads read consecutive channels), min / max and the finite count go through the wave shuffle and
// then the four waves through LDS in wave order; the job's (lo, hi) goes to the result block.  montage_paint_kernel, grid
// (kPaintBlocks, njobs): one thread per output byte, grid-stride within the job; consecutive threads write consecutive bytes of
// an output row and read one channel of consecutive pixels.  No atomics; min and max do not depend on the order, so two
// launches are bit-equal.  Reads: only the c live channels of each pixel, nothing behind the last live element of the last
// pixel.  Writes: only each job's n*h*m*w bytes.
//
// Like tdg_tensor_summary the entry reads the job table back (one stream-ordered copy, one stream synchronisation): a bad job
// must be a status and not a fault.  It runs eagerly between training steps, never inside a captured body.
#include <float.h>

#include <algorithm>
#include <vector>

#include "tdg_cgan_common.h"

namespace {

constexpr int kThreads = 256, kPaintBlocks = 16;
constexpr unsigned long long kMaxImageElems = 1ull << 30;          // h * w * cs of one job: every index fits an int

static_assert(sizeof(TdgMontageJob) == 40, "ActivationMontages (kernels.py) builds this layout");

// hem.factorization's first member: the largest i <= sqrt(c) that divides c
__host__ __device__ inline int montage_m(int c) {
  int i = 1;
  while ((long long)(i + 1) * (i + 1) <= (long long)c) ++i;
  while (c % i) --i;
  return i;
}

__host__ __device__ inline unsigned long long montage_bytes(const TdgMontageJob& j) {
  return (unsigned long long)j.h * (unsigned long long)j.w * (unsigned long long)j.c;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
  return v;
}

template <typename T>
__device__ __forceinline__ void range_scan(const TdgMontageJob& job, float& mn, float& mx, uint32_t& fin) {
  const T* __restrict__ p = static_cast<const T*>(job.ptr);
  const int total = job.h * job.w * job.c;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int px = e / job.c, ch = e - px * job.c;
    const float v = to_f32<T>(p[(size_t)px * job.cs + ch]);
    if (fabsf(v) <= FLT_MAX) {                                     // false for NaN and +-Inf
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
      ++fin;
    }
  }
}

__global__ void __launch_bounds__(kThreads) montage_range_kernel(const TdgMontageJob* __restrict__ jobs, float* __restrict__ res) {
  __shared__ float sh_mn[4], sh_mx[4];
  __shared__ uint32_t sh_fin[4];
  const TdgMontageJob job = jobs[blockIdx.x];
  float mn = INFINITY, mx = -INFINITY;
  uint32_t fin = 0;
  if (job.dtype == TDG_BF16) range_scan<bf16_t>(job, mn, mx, fin);
  else range_scan<float>(job, mn, mx, fin);
  mn = wave_min(mn), mx = wave_max(mx), fin = wave_sum(fin);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    sh_mn[w] = mn, sh_mx[w] = mx, sh_fin[w] = fin;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const bool any = block_total(sh_fin) > 0;
  float lo = any ? fminf(fminf(sh_mn[0], sh_mn[1]), fminf(sh_mn[2], sh_mn[3])) : 0.f;
  float hi = any ? fmaxf(fmaxf(sh_mx[0], sh_mx[1]), fmaxf(sh_mx[2], sh_mx[3])) : 0.f;
  if (lo == 0.f) lo = 0.f;                                         // one zero: which of -0 / +0 a minimum keeps is not defined
  if (hi == 0.f) hi = 0.f;
  res[2 * blockIdx.x] = lo;
  res[2 * blockIdx.x + 1] = hi;
}

template <typename T>
__device__ __forceinline__ void paint(const TdgMontageJob& job, float scale, float offset, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
  const T* __restrict__ p = static_cast<const T*>(job.ptr);
  const int m = montage_m(job.c), mw = m * job.w;
  const int total = job.h * job.w * job.c;                         // = n*h rows of m*w bytes
  uint8_t* __restrict__ dst = out + job.out_offset;
  for (int o = blockIdx.x * kThreads + threadIdx.x; o < total; o += kPaintBlocks * kThreads) {
    const int row = o / mw, col = o - row * mw;
    const int j = row / job.h, y = row - j * job.h;
    const int i = col / job.w, x = col - i * job.w;
    const float v = to_f32<T>(p[(size_t)(y * job.w + x) * job.cs + (j * m + i)]);
    uint8_t b = 255;
    if (fabsf(v) <= FLT_MAX) {
      const float t = v * scale;
      const float u = t + offset;
      b = (uint8_t)fminf(u, 255.0f);
    }
    dst[o] = b;
  }
}

__global__ void __launch_bounds__(kThreads) montage_paint_kernel(const TdgMontageJob* __restrict__ jobs, const float* __restrict__ res,
                                                                 uint8_t* __restrict__ out) {
  const TdgMontageJob job = jobs[blockIdx.y];
  const float lo = res[2 * blockIdx.y], hi = res[2 * blockIdx.y + 1];
  float scale, offset;
  if (lo < 0.f) {
    const float big = fmaxf(fabsf(lo), fabsf(hi));
    scale = big < 1e-6f ? 0.f : 127.0f / big;
    offset = 128.0f;
  } else {
    scale = hi < 1e-6f ? 0.f : 255.0f / hi;
    offset = 0.f;
  }
  if (job.dtype == TDG_BF16) paint<bf16_t>(job, scale, offset, out);
  else paint<float>(job, scale, offset, out);
}

}  // namespace

extern "C" int tdg_activation_montage(const TdgMontageJob* jobs_dev, int njobs, void* out_dev, size_t out_bytes, float* results_dev,
                                      void* stream) {
  TDG_CHECK_ARG(jobs_dev && out_dev && results_dev && njobs > 0 && njobs <= 65535,
                "tdg_activation_montage: bad argument (jobs %p, njobs %d, out %p, results %p)", (const void*)jobs_dev, njobs, out_dev,
                (const void*)results_dev);
  TDG_CHECK_ARG(((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)results_dev & 3) == 0, "tdg_activation_montage: misaligned job table or results");
  hipStream_t s = (hipStream_t)stream;
  std::vector<TdgMontageJob> jobs((size_t)njobs);
  hipError_t e = hipMemcpyAsync(jobs.data(), jobs_dev, (size_t)njobs * sizeof(TdgMontageJob), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    tdg_set_error("tdg_activation_montage: reading the job table back failed: %s (it does not run inside a captured body)",
                  hipGetErrorString(e));
    return TDG_EHIP;
  }
  std::vector<std::pair<unsigned long long, unsigned long long>> regions;      // (first byte, one past the last)
  for (int j = 0; j < njobs; ++j) {
    const TdgMontageJob& b = jobs[(size_t)j];
    TDG_CHECK_ARG(b.dtype == TDG_F32 || b.dtype == TDG_BF16, "tdg_activation_montage: job %d: bad dtype %d", j, b.dtype);
    TDG_CHECK_ARG(b.ptr && b.h >= 1 && b.w >= 1 && b.c >= 1 && b.cs >= b.c &&
                      (unsigned long long)b.h * (unsigned long long)b.w <= kMaxImageElems / (unsigned long long)b.cs,
                  "tdg_activation_montage: job %d: bad activation (ptr %p, h %d, w %d, c %d, cs %d)", j, b.ptr, b.h, b.w, b.c, b.cs);
    TDG_CHECK_ARG(((uintptr_t)b.ptr & (uintptr_t)(tdg_dtype_size(b.dtype) - 1)) == 0, "tdg_activation_montage: job %d: misaligned activation", j);
    const unsigned long long n = montage_bytes(b);
    TDG_CHECK_ARG(b.out_offset <= out_bytes && n <= out_bytes - b.out_offset,
                  "tdg_activation_montage: job %d: bytes [%llu, +%llu) run past the output of %zu bytes", j, (unsigned long long)b.out_offset, n,
                  out_bytes);
    regions.emplace_back((unsigned long long)b.out_offset, (unsigned long long)b.out_offset + n);
  }
  std::sort(regions.begin(), regions.end());
  for (size_t k = 1; k < regions.size(); ++k)
    TDG_CHECK_ARG(regions[k].first >= regions[k - 1].second, "tdg_activation_montage: the output regions [%llu, %llu) and [%llu, %llu) overlap",
                  regions[k - 1].first, regions[k - 1].second, regions[k].first, regions[k].second);
  tdg_timing_start("activation_montage", 0.0, s);
  hipLaunchKernelGGL(montage_range_kernel, dim3(njobs), dim3(kThreads), 0, s, jobs_dev, results_dev);
  hipLaunchKernelGGL(montage_paint_kernel, dim3(kPaintBlocks, njobs), dim3(kThreads), 0, s, jobs_dev, (const float*)results_dev,
                     static_cast<uint8_t*>(out_dev));
  tdg_timing_stop(s);
  TDG_HIP_LAUNCH_CHECK("activation_montage");
  return TDG_OK;
}
