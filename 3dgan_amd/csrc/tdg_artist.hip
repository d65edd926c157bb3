// artist pieces that are not GEMMs (hem/models/artist.py): the whole-image mean squared error of a decoder output against
// the staged batch, with its seed, in ONE pass over both (include/tdg.h states the arithmetic).  Memory-bound; wave64.
//
// A 256-thread block takes tiles of kTile = 1024 consecutive pixels, grid-stride.  Per tile the compact target (c floats per
// pixel, 12 bytes at c = 3) is brought into LDS with 16-byte loads where its base is 16-byte aligned (a tile starts 4096 c
// bytes behind the base, so every full tile is aligned with it) and with 4-byte loads otherwise or in the last, partial tile;
// then thread t takes the pixels t, t + 256, t + 512, t + 768 of the tile: one 16-byte load of h per pixel (consecutive lanes,
// consecutive pixels), the c target values from LDS (stride c words: no bank conflict at c = 1, 3), the squares into an f64
// sum of its own, and the seed's c channels with the widest stores that stay inside them.
// The sum has a fixed order -- thread, wave shuffle, the four waves, one f64 partial per block, then the partials by one
// block in the same shape -- and there are no atomics: two launches are bit-equal.
#include "tdg_cgan_common.h"

namespace {

constexpr int kTile = 1024;          // pixels of one block and trip
constexpr int kMaxBlocks = 1024;     // the cap on the grid = the partials the workspace holds

// channels 0..3 of one pixel by ONE 16-byte load (bf16: the load brings eight, four are kept).  The empty asm names all four
// registers as used, so that the compiler does not narrow the load to the channels a small c reads: adjacent lanes then cover
// whole lines with one request each instead of 2 or 4 bytes at a 16-byte stride.
__device__ __forceinline__ i32x4 load_px16(const void* p) {
  i32x4 q = *reinterpret_cast<const i32x4*>(p);
  asm("" : "+v"(q));
  return q;
}
template <typename T>
__device__ __forceinline__ void load_px(const T* p, float* v);
template <>
__device__ __forceinline__ void load_px<bf16_t>(const bf16_t* p, float* v) {
  const i32x4 q = load_px16(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(((unsigned)q[i >> 1] >> (16 * (i & 1))) << 16);      // bf16 -> f32: exact
}
template <>
__device__ __forceinline__ void load_px<float>(const float* p, float* v) {
  const i32x4 q = load_px16(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __int_as_float(q[i]);
}

template <typename T>
struct PxVec;
template <>
struct PxVec<bf16_t> { using v4 = bf16x4; using v2 = bf16x2; };
template <>
struct PxVec<float> { using v4 = f32x4; using v2 = f32x2; };

// channels 0..C-1 of one pixel (p is 16-byte aligned); channels [C, cs) are never written
template <typename T, int C>
__device__ __forceinline__ void store_px(T* p, const float* v) {
  using V4 = typename PxVec<T>::v4;
  using V2 = typename PxVec<T>::v2;
  if constexpr (C == 4) {
    V4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = from_f32<T>(v[i]);
    *reinterpret_cast<V4*>(p) = a;
  } else {
    if constexpr (C >= 2) {
      V2 a;
      a[0] = from_f32<T>(v[0]);
      a[1] = from_f32<T>(v[1]);
      *reinterpret_cast<V2*>(p) = a;
    }
    if constexpr (C & 1) p[C - 1] = from_f32<T>(v[C - 1]);
  }
}

template <typename T, int C, bool SEED>
__global__ void __launch_bounds__(256) artist_mse_kernel(const float* __restrict__ target, const T* __restrict__ h, int rows, int cs,
                                                         float k, bool tvec, T* __restrict__ seed, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float tsh[kTile * C];
  __shared__ double sh[4];
  const int ntiles = (rows + kTile - 1) / kTile;
  double s = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t p0 = (size_t)tile * kTile;
    const int np = rows - p0 < (size_t)kTile ? (int)(rows - p0) : kTile;
    const float* tg = target + p0 * C;
    if (tvec && np == kTile) {
      for (int i = threadIdx.x; i < kTile * C / 4; i += 256) reinterpret_cast<f32x4*>(tsh)[i] = reinterpret_cast<const f32x4*>(tg)[i];
    } else {
      for (int i = threadIdx.x; i < np * C; i += 256) tsh[i] = tg[i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTile / 256; ++j) {
      const int p = j * 256 + threadIdx.x;
      if (p < np) {
        const size_t o = (p0 + p) * cs;
        float hv[4], sv[C];
        load_px<T>(h + o, hv);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          // hem.rescale, every operation rounded once: the target's round trip [0,1] -> [-1,1] -> [0,1], then h to [0,1]
          const float tm = __fsub_rn(__fmul_rn(2.f, tsh[p * C + ch]), 1.f);
          const float t01 = __fmul_rn(__fadd_rn(tm, 1.f), 0.5f);
          const float h01 = __fmul_rn(__fadd_rn(hv[ch], 1.f), 0.5f);
          const float d = __fsub_rn(h01, t01);
          s += (double)d * (double)d;
          sv[ch] = __fmul_rn(d, k);
        }
        if constexpr (SEED) store_px<T, C>(seed + o, sv);
      }
    }
    __syncthreads();                                         // the next trip overwrites tsh
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = block_total(sh);
}

// the partials by one block: thread t takes t, t + 256, ..., then the wave sums, then the four waves in wave order
__global__ void __launch_bounds__(256) artist_mse_finish_kernel(const double* __restrict__ partial, int nblk, double n,
                                                                float* __restrict__ scal) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 256) s += partial[b];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double mean = block_total(sh) / n;
    scal[0] = (float)mean;
    scal[1] = (float)sqrt(mean);
  }
}

// four blocks per compute unit of the current device, at most kMaxBlocks (asked once per process)
int artist_grid_cap() {
  static const int cap = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = kMaxBlocks / 4;
    return 4 * cus < kMaxBlocks ? 4 * cus : kMaxBlocks;
  }();
  return cap;
}

template <typename T, int C>
void artist_mse_launch(const float* target, const void* h, int rows, int cs, float k, bool tvec, void* seed, double* partial, int nblk,
                       hipStream_t stream) {
  if (seed)
    hipLaunchKernelGGL((artist_mse_kernel<T, C, true>), dim3(nblk), dim3(256), 0, stream, target, static_cast<const T*>(h), rows, cs, k,
                       tvec, static_cast<T*>(seed), partial);
  else
    hipLaunchKernelGGL((artist_mse_kernel<T, C, false>), dim3(nblk), dim3(256), 0, stream, target, static_cast<const T*>(h), rows, cs, k,
                       tvec, static_cast<T*>(nullptr), partial);
}

}  // namespace

extern "C" size_t tdg_artist_mse_workspace_bytes(void) { return kMaxBlocks * sizeof(double); }

extern "C" int tdg_artist_mse(int dtype, const float* target, const void* h, int rows, int c, int cs, void* seed, float* scal,
                              void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(target && h && scal && workspace && rows > 0 && c >= 1 && c <= 4 && c <= cs && cs % 8 == 0,
                "tdg_artist_mse: bad argument (rows %d, c %d of 1..4, cs %d, a multiple of 8)", rows, c, cs);
  TDG_CHECK_ARG((((uintptr_t)h | (uintptr_t)seed) & 15) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
                "tdg_artist_mse: h and seed must be 16-byte aligned, target 4-byte, the workspace 8-byte");
  if (workspace_bytes < tdg_artist_mse_workspace_bytes()) {
    tdg_set_error("tdg_artist_mse: workspace of %zu bytes, %zu needed", workspace_bytes, tdg_artist_mse_workspace_bytes());
    return TDG_EWORKSPACE;
  }
  const double n = (double)rows * (double)c;
  const float k = 1.f / (float)n;                            // IEEE on the host: fl(1 / fl(rows c))
  const bool tvec = ((uintptr_t)target & 15) == 0;
  const int ntiles = tdg_ceil_div(rows, kTile), cap = artist_grid_cap();
  const int nblk = ntiles < cap ? ntiles : cap;
  double* partial = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  tdg_timing_start("artist_mse", 0.0, s);
  DISPATCH_T(dtype, {
    switch (c) {
      case 1: artist_mse_launch<T, 1>(target, h, rows, cs, k, tvec, seed, partial, nblk, s); break;
      case 2: artist_mse_launch<T, 2>(target, h, rows, cs, k, tvec, seed, partial, nblk, s); break;
      case 3: artist_mse_launch<T, 3>(target, h, rows, cs, k, tvec, seed, partial, nblk, s); break;
      default: artist_mse_launch<T, 4>(target, h, rows, cs, k, tvec, seed, partial, nblk, s); break;
    }
  })
  hipLaunchKernelGGL(artist_mse_finish_kernel, dim3(1), dim3(256), 0, s, partial, nblk, n, scal);
  tdg_timing_stop(s);
  TDG_HIP_LAUNCH_CHECK("artist_mse");
  return TDG_OK;
}
