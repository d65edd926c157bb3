// paper_standalone's pieces that are not GEMMs (hem/models/paper_standalone.py): the RMSE regression loss with its gradient
// (:244-253) and the fed y_bar channel of g_mean_provided (:176-207).  Memory-bound; wave64 throughout.
//
// tdg_cgan_rmse_loss: loss = sqrt(mean((yhat/10 - y/10)^2)) over all N = n * hw elements, one scalar per launch, and
// d(loss)/d(yhat) = d / (10 sqrt(N S)) with d = yhat - y and S = sum d^2.  Differences, squares and sums are f64 and every
// combination has a fixed order (wave shuffle -> LDS in wave order -> block partials in block order), no atomics: two
// launches are bit-equal.  Two equally wide launches: the first writes one f64 partial per block of 1024 elements (16-byte
// loads), the second has EVERY block re-sum the few hundred partials in the same order -- the same S in every block -- and
// scale and store its own 1024 elements; block 0 writes the scalar.  No serial one-block finish.
// DEVIATION: S == 0 (yhat == y everywhere) gives loss 0 and an all-zero gradient; TensorFlow's sqrt gradient gives NaN there.
#include "tdg_cgan_common.h"

namespace {

constexpr int kTile = 1024;                                  // elements per block: 256 threads x one 16-byte load of each input
constexpr int kMaxBlocks = 1024;                             // beyond that many tiles a block takes several (grid stride)

inline int rmse_blocks(long long total) {
  const long long b = (total + kTile - 1) / kTile;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

// the block's sum, the same value in every thread: wave shuffle, then the four wave sums from LDS in wave order
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();                                           // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return block_total(sh);
}

// d[0..3] = yhat - y (f64) of the four elements from i on; elements at or past `total` are 0.  VEC: both pointers are
// 16-byte aligned, so a whole group is one load of each.
template <bool VEC>
__device__ __forceinline__ void diff4(const float* __restrict__ y, const float* __restrict__ yhat, long long i, long long total,
                                      double* d) {
  if (VEC && i + 4 <= total) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(y + i), b = *reinterpret_cast<const f32x4*>(yhat + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = (double)b[k] - (double)a[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = i + k < total ? (double)yhat[i + k] - (double)y[i + k] : 0.0;
}

template <bool VEC>
__global__ void __launch_bounds__(256) rmse_partial_kernel(const float* __restrict__ y, const float* __restrict__ yhat,
                                                           long long total, double* __restrict__ part) {
  __shared__ double sh[4];
  double s = 0.0;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (long long)gridDim.x * kTile) {
    double d[4];
    diff4<VEC>(y, yhat, i, total, d);
    s += ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256) rmse_grad_kernel(const float* __restrict__ y, const float* __restrict__ yhat, long long total,
                                                        const double* __restrict__ part, T* __restrict__ dg, int dg_cs,
                                                        float* __restrict__ scal) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int k = threadIdx.x; k < (int)gridDim.x; k += 256) s += part[k];      // thread t: partials t, t + 256, ... in that order
  const double S = block_sum(s, sh);
  const double N = (double)total;
  const double inv = S > 0.0 ? 1.0 / (10.0 * sqrt(N * S)) : (S == 0.0 ? 0.0 : S);      // (NaN stays NaN: the finite check's)
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[0] = (float)(sqrt(S / N) / 10.0);
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < total; i += (long long)gridDim.x * kTile) {
    double d[4];
    diff4<VEC>(y, yhat, i, total, d);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < total) dg[(size_t)(i + k) * dg_cs] = from_f32<T>((float)(d[k] * inv));
  }
}

template <typename T>
__global__ void __launch_bounds__(256) bar_fill_kernel(const float* __restrict__ ybar, long long total, int hw2, T* __restrict__ win,
                                                       int win_cs, float* __restrict__ plane) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const float m = ybar[i / hw2];
    win[(size_t)i * win_cs] = from_f32<T>(m);
    if (plane) plane[i] = m;
  }
}

}  // namespace

extern "C" size_t tdg_cgan_rmse_loss_workspace_bytes(int n, int hw) {
  return n > 0 && hw > 0 ? (size_t)rmse_blocks((long long)n * hw) * sizeof(double) : 0;
}

extern "C" int tdg_cgan_rmse_loss(int dtype, const float* y, const float* yhat, int n, int hw, void* dg, int dg_cs, float* scal,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(y && yhat && dg && scal && workspace && n > 0 && hw > 0 && dg_cs > 0 && (dtype == TDG_F32 || dtype == TDG_BF16),
                "tdg_cgan_rmse_loss: bad argument (dtype %d, n %d, hw %d, dg_cs %d)", dtype, n, hw, dg_cs);
  if (workspace_bytes < tdg_cgan_rmse_loss_workspace_bytes(n, hw)) {
    tdg_set_error("tdg_cgan_rmse_loss: workspace of %zu bytes, %zu needed", workspace_bytes, tdg_cgan_rmse_loss_workspace_bytes(n, hw));
    return TDG_EWORKSPACE;
  }
  const long long total = (long long)n * hw;
  const int nblk = rmse_blocks(total);
  const bool vec = (((uintptr_t)y | (uintptr_t)yhat) & 15) == 0;
  double* part = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  tdg_timing_start("cgan_rmse_loss", 0.0, s);
  if (vec) hipLaunchKernelGGL(rmse_partial_kernel<true>, dim3(nblk), dim3(256), 0, s, y, yhat, total, part);
  else hipLaunchKernelGGL(rmse_partial_kernel<false>, dim3(nblk), dim3(256), 0, s, y, yhat, total, part);
  DISPATCH_T(dtype, {
    if (vec)
      hipLaunchKernelGGL((rmse_grad_kernel<T, true>), dim3(nblk), dim3(256), 0, s, y, yhat, total, part, static_cast<T*>(dg), dg_cs, scal);
    else
      hipLaunchKernelGGL((rmse_grad_kernel<T, false>), dim3(nblk), dim3(256), 0, s, y, yhat, total, part, static_cast<T*>(dg), dg_cs, scal);
  })
  tdg_timing_stop(s);
  TDG_HIP_LAUNCH_CHECK("cgan_rmse_loss");
  return TDG_OK;
}

extern "C" int tdg_cgan_bar_fill(int dtype, const float* ybar, int n, int hw2, void* win, int win_cs, float* plane, void* stream) {
  TDG_CHECK_ARG(ybar && win && n > 0 && hw2 > 0 && win_cs > 0 && (dtype == TDG_F32 || dtype == TDG_BF16),
                "tdg_cgan_bar_fill: bad argument (dtype %d, n %d, hw2 %d, win_cs %d)", dtype, n, hw2, win_cs);
  const long long total = (long long)n * hw2;
  hipStream_t s = (hipStream_t)stream;
  tdg_timing_start("cgan_bar_fill", 0.0, s);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(bar_fill_kernel<T>, dim3(grid_for((size_t)total)), dim3(256), 0, s, ybar, total, hw2, static_cast<T*>(win), win_cs, plane);
  })
  tdg_timing_stop(s);
  TDG_HIP_LAUNCH_CHECK("cgan_bar_fill");
  return TDG_OK;
}
