// mean_depth_estimator's one piece that is not a GEMM (hem/models/mean_depth_estimator.py:136-147): the loss
//   mean_i = mean over the hw pixels of image i of y_full,   loss = (1/n) sum_i |mean_i - m_i|
// with m the network's sigmoid output, and the gradient seed dL/dm_i = sign(m_i - mean_i) / n.
//
// The seed is dL/dm, the gradient with respect to the sigmoid's OUTPUT, not dL/dlogit: +-f32(1/n) rounded to the dtype, or
// 0.  The executor's last layer turns it into dL/dlogit with the activation's derivative (tdg_act_bwd on the stored output).
// DEVIATION: the reference writes sqrt(square(d)), whose TensorFlow gradient at d == 0 is NaN; here sign(0) = 0.
//
// Memory-bound on n * hw * 4 bytes (7.6 MB at n = 512, hw = 3710: a few microseconds of HBM time), so the two launch
// latencies dominate.  Launch 1: one 256-thread block per image (grid-stride beyond kMaxBlocks); thread t adds the elements
// t VW, t VW + 256 VW, ... in that order (VW = 4 / 2 / 1 floats per load, by the row alignment), then wave shuffle, then
// the four wave sums from LDS in wave order; ONE f64 division and ONE rounding to f32 per image; the block also writes
// the image's seed and its f64 term |mean_i - m_i| into the workspace.  Launch 2: one block stages the n terms through LDS
// 256 at a time and thread 0 adds them in image order (n is a batch size: 512 dependent f64 adds), divides once and rounds
// once.  No atomics and a fixed order everywhere: two launches on the same input are bit-equal.  wave64 throughout.
#include "tdg_cgan_common.h"

namespace {

constexpr int kMaxBlocks = 4096;

template <int VW>
__device__ __forceinline__ double row_sum(const float* __restrict__ row, int hw) {
  double s = 0.0;
  for (int i = threadIdx.x * VW; i < hw; i += 256 * VW) {          // hw % VW == 0: a group never straddles the row's end
    if constexpr (VW == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + i);
      s += (((double)v[0] + (double)v[1]) + (double)v[2]) + (double)v[3];
    } else if constexpr (VW == 2) {
      const f32x2 v = *reinterpret_cast<const f32x2*>(row + i);
      s += (double)v[0] + (double)v[1];
    } else {
      s += (double)row[i];
    }
  }
  return s;
}

template <typename T, int VW>
__global__ void __launch_bounds__(256) mde_image_kernel(const float* __restrict__ y, int n, int hw, const T* __restrict__ m, int m_cs,
                                                        float* __restrict__ mean_out, T* __restrict__ seed, int seed_cs,
                                                        double* __restrict__ term) {
  __shared__ double sh[4];
  for (int img = blockIdx.x; img < n; img += gridDim.x) {
    double s = wave_sum(row_sum<VW>(y + (size_t)img * hw, hw));
    __syncthreads();                                               // (sh may still be read for the previous image)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double mean = block_total(sh) / (double)hw;
      const double d = (double)to_f32<T>(m[(size_t)img * m_cs]) - mean;
      const float step = (float)(1.0 / (double)n);
      mean_out[img] = (float)mean;
      term[img] = fabs(d);
      seed[(size_t)img * seed_cs] = from_f32<T>(d > 0.0 ? step : (d < 0.0 ? -step : (d == 0.0 ? 0.f : (float)d)));   // (NaN stays NaN)
    }
  }
}

__global__ void __launch_bounds__(256) mde_finish_kernel(const double* __restrict__ term, int n, float* __restrict__ scal) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    __syncthreads();
    sh[threadIdx.x] = i0 + (int)threadIdx.x < n ? term[i0 + threadIdx.x] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int k = n - i0 < 256 ? n - i0 : 256;
      for (int j = 0; j < k; ++j) s += sh[j];
    }
  }
  if (threadIdx.x == 0) scal[0] = (float)(s / (double)n);
}

}  // namespace

extern "C" size_t tdg_mde_loss_workspace_bytes(int n) { return n > 0 ? (size_t)n * sizeof(double) : 0; }

extern "C" int tdg_mde_loss(int dtype, const float* y_full, int n, int hw, const void* m, int m_cs, float* mean_out, void* seed,
                            int seed_cs, float* scal, void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(y_full && m && mean_out && seed && scal && workspace && n > 0 && hw > 0 && m_cs > 0 && seed_cs > 0 &&
                    (dtype == TDG_F32 || dtype == TDG_BF16),
                "tdg_mde_loss: bad argument (dtype %d, n %d, hw %d, m_cs %d, seed_cs %d)", dtype, n, hw, m_cs, seed_cs);
  TDG_CHECK_ARG(((uintptr_t)y_full & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "tdg_mde_loss: misaligned y_full or workspace");
  if (workspace_bytes < tdg_mde_loss_workspace_bytes(n)) {
    tdg_set_error("tdg_mde_loss: workspace of %zu bytes, %zu needed", workspace_bytes, tdg_mde_loss_workspace_bytes(n));
    return TDG_EWORKSPACE;
  }
  // every row starts hw floats after the one before: the widest load that keeps each row's groups aligned and whole
  const int vw = (hw % 4 == 0 && ((uintptr_t)y_full & 15) == 0) ? 4 : ((hw % 2 == 0 && ((uintptr_t)y_full & 7) == 0) ? 2 : 1);
  const int nblk = n < kMaxBlocks ? n : kMaxBlocks;
  double* term = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  tdg_timing_start("mde_loss", 0.0, s);
  DISPATCH_T(dtype, {
    const T* mp = static_cast<const T*>(m);
    T* sp = static_cast<T*>(seed);
    if (vw == 4)
      hipLaunchKernelGGL((mde_image_kernel<T, 4>), dim3(nblk), dim3(256), 0, s, y_full, n, hw, mp, m_cs, mean_out, sp, seed_cs, term);
    else if (vw == 2)
      hipLaunchKernelGGL((mde_image_kernel<T, 2>), dim3(nblk), dim3(256), 0, s, y_full, n, hw, mp, m_cs, mean_out, sp, seed_cs, term);
    else
      hipLaunchKernelGGL((mde_image_kernel<T, 1>), dim3(nblk), dim3(256), 0, s, y_full, n, hw, mp, m_cs, mean_out, sp, seed_cs, term);
  })
  hipLaunchKernelGGL(mde_finish_kernel, dim3(1), dim3(256), 0, s, term, n, scal);
  tdg_timing_stop(s);
  TDG_HIP_LAUNCH_CHECK("mde_loss");
  return TDG_OK;
}
