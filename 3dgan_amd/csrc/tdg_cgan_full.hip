// paper_cgan full-frame inference (paper_fullimage.py of the thesis code): the 65x65 window slid over an H x W frame at
// stride s, the generator's 29x29 outputs blended back into frame-sized canvases, and the frame RMSE.
//
// Grid (build_batch): cols = (H - 93) / s windows down, rows = (W - 93) / s across; patch c = n * cols + m (n < rows
// outer, m < cols inner: column-major, the window moves down first) has its top-left corner at (m s, n s).  Its 29x29
// output lands at (m s + off, n s + off) of the canvas.  All of these are memory-bound; wave64 throughout.
#include <math.h>

#include "tdg_common.h"

namespace {

constexpr int kSrc = 65, kCrop = 29, kCrop2 = kCrop * kCrop;
constexpr int kMinSide = kSrc + kCrop - 1;               // 93: a side needs more than this for one window
constexpr int kRmseBlocks = 256;
constexpr int kRmseLo = 18, kRmseHi = 46;               // rmse region: [18, H - 46) x [18, W - 46)

inline int grid_for(size_t n) {
  const size_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

inline int grid_count(int side, int s) { return (side - kMinSide) / s; }

__device__ __forceinline__ double wsum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- patch gather: the chunk's windows of image [H,W,3] and depth [H,W] into x [B,65,65,3] / y [B,65,65,1] ----------
// One thread per staged float; a staged row is 195 image floats then 65 depth floats, both contiguous in the frame.
__global__ void __launch_bounds__(256) full_gather_kernel(const float* __restrict__ image, const float* __restrict__ depth, int W,
                                                          int s, int cols, int P, const int* __restrict__ chunk, int B,
                                                          float* __restrict__ x, float* __restrict__ y) {
  constexpr int kRow = kSrc * 3 + kSrc;
  const long long base = (long long)*chunk * B;
  const size_t total = (size_t)B * kSrc * kRow;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / (kSrc * kRow));
    const int rem = (int)(i - (size_t)b * (kSrc * kRow));
    const int r = rem / kRow, k = rem - r * kRow;
    const long long c = base + b;
    float v = 0.f;
    if (c >= 0 && c < P) {                                  // slots past the grid are zero, as the reference pads
      const int n = (int)c / cols, m = (int)c - n * cols;
      const size_t row = (size_t)(m * s + r) * W + n * s;
      v = k < kSrc * 3 ? image[row * 3 + k] : depth[row + (k - kSrc * 3)];
    }
    if (k < kSrc * 3) x[((size_t)b * kSrc + r) * (kSrc * 3) + k] = v;
    else y[((size_t)b * kSrc + r) * kSrc + (k - kSrc * 3)] = v;
  }
}

// ---- patch store: the chunk's y_hat [B,29,29] / y_bar [B] to slots [chunk B, chunk B + B) of the frame store -------
__global__ void __launch_bounds__(256) full_store_kernel(const float* __restrict__ yhat, const float* __restrict__ ybar, int B,
                                                         long long slots, const int* __restrict__ chunk,
                                                         float* __restrict__ st_yhat, float* __restrict__ st_ybar) {
  const long long base = (long long)*chunk * B;
  if (base < 0 || base + B > slots) return;                 // a store past its slots writes nothing
  const size_t total = (size_t)B * (kCrop2 + 1);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    if (i < (size_t)B * kCrop2) st_yhat[(size_t)base * kCrop2 + i] = yhat[i];
    else {
      const size_t b = i - (size_t)B * kCrop2;
      st_ybar[base + b] = ybar ? ybar[b] : 0.f;
    }
  }
}

__global__ void full_next_chunk_kernel(int* chunk) {
  if (threadIdx.x == 0) chunk[0] += 1;
}

// ---- ordered blend: one thread per canvas pixel, a wave on 64 consecutive pixels of one row ------------------------
// The covering windows of pixel (py, px) are m in [m_lo, m_hi] (from py) and n in [n_lo, n_hi] (from px).  m's range is
// the same for the whole wave; the wave walks the union of its lanes' n ranges in ascending order, each lane taking the
// n that cover it, so every load is one contiguous run of a patch row.  Per lane the order is ascending c = n cols + m,
// the reference's visiting order, and the recurrence v = (isnan(v) ? d : v + d) / 2 runs in float64.
__device__ __forceinline__ void cover_range(int p, int off, int s, int count, int& lo, int& hi) {
  const int t = p - off;                                   // window k covers p iff k s <= t <= k s + 28
  if (t < 0) {
    lo = 0;
    hi = -1;
    return;
  }
  lo = t <= kCrop - 1 ? 0 : (t - (kCrop - 1) + s - 1) / s;
  hi = t / s;
  if (hi > count - 1) hi = count - 1;
}

__global__ void __launch_bounds__(256) full_blend_kernel(const float* __restrict__ st_yhat, const float* __restrict__ st_ybar,
                                                         int H, int W, int s, int off, int cols, int rows,
                                                         float* __restrict__ out_yhat, float* __restrict__ out_g) {
  const int lane = threadIdx.x & 63;
  const int py = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x0 = blockIdx.x * 64, px = x0 + lane;
  if (py >= H) return;
  int m_lo, m_hi, n_lo, n_hi, na, nb, dummy;
  cover_range(py, off, s, cols, m_lo, m_hi);
  cover_range(px, off, s, rows, n_lo, n_hi);
  cover_range(x0, off, s, rows, na, dummy);                // wave-uniform n range: from the first lane's low end ...
  cover_range(min(x0 + 63, W - 1), off, s, rows, dummy, nb);   // ... to the last lane's high end
  double vy = NAN, vg = NAN;
  for (int n = na; n <= nb; ++n) {
    if (n < n_lo || n > n_hi) continue;
    const int q = px - n * s - off;
    for (int m = m_lo; m <= m_hi; ++m) {
      const int c = n * cols + m;
      const float d = st_yhat[(size_t)c * kCrop2 + (py - m * s - off) * kCrop + q];
      const float g = d - st_ybar[c];                      // g = y_hat - y_bar (f32), exactly y_hat for baseline
      vy = (isnan(vy) ? (double)d : vy);
      vg = (isnan(vg) ? (double)g : vg);
      vy = (vy + (double)d) / 2.0;
      vg = (vg + (double)g) / 2.0;
    }
  }
  if (px < W) {
    out_yhat[(size_t)py * W + px] = (float)(isnan(vy) ? 0.0 : vy);    // nan_to_num: uncovered pixels are 0
    out_g[(size_t)py * W + px] = (float)(isnan(vg) ? 0.0 : vg);
  }
}

// ---- frame RMSE: sqrt(mean((10 depth - canvas)^2)) over [18, H-46) x [18, W-46), float64 block partials ------------
__global__ void __launch_bounds__(256) full_rmse_kernel(const float* __restrict__ depth, const float* __restrict__ canvas, int H,
                                                        int W, double* __restrict__ part) {
  __shared__ double sh[4];
  const int ch = W - kRmseLo - kRmseHi;
  const size_t total = (size_t)(H - kRmseLo - kRmseHi) * ch;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int r = (int)(i / ch) + kRmseLo, c = (int)(i % ch) + kRmseLo;
    const size_t p = (size_t)r * W + c;
    const double e = (double)(depth[p] * 10.f) - (double)canvas[p];   // the reference scales the f32 depth in f32
    acc += e * e;
  }
  acc = wsum_d(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void full_rmse_finish_kernel(const double* __restrict__ part, int nblk, double count, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[b];
  out[0] = sqrt(s / count);
}

}  // namespace

extern "C" int tdg_cgan_full_gather(const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch,
                                    float* x_stage, float* y_stage, void* stream) {
  TDG_CHECK_ARG(image && depth && chunk && x_stage && y_stage && H > kMinSide && W > kMinSide && stride >= 1 && batch > 0,
                "tdg_cgan_full_gather: bad argument (H %d, W %d, stride %d, batch %d)", H, W, stride, batch);
  const int cols = grid_count(H, stride), rows = grid_count(W, stride);
  const size_t total = (size_t)batch * kSrc * (kSrc * 4);
  tdg_timing_start("cgan_full_gather", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(full_gather_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, image, depth, W, stride,
                     cols > 0 ? cols : 1, cols * rows, chunk, batch, x_stage, y_stage);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_gather");
  return TDG_OK;
}

extern "C" int tdg_cgan_full_store(const float* yhat, const float* ybar, int batch, long long slots, int* chunk, float* store_yhat,
                                   float* store_ybar, void* stream) {
  TDG_CHECK_ARG(yhat && chunk && store_yhat && store_ybar && batch > 0 && slots >= batch,
                "tdg_cgan_full_store: bad argument (batch %d, slots %lld)", batch, slots);
  tdg_timing_start("cgan_full_store", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(full_store_kernel, dim3(grid_for((size_t)batch * (kCrop2 + 1))), dim3(256), 0, (hipStream_t)stream, yhat, ybar,
                     batch, slots, chunk, store_yhat, store_ybar);
  hipLaunchKernelGGL(full_next_chunk_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, chunk);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_store");
  return TDG_OK;
}

extern "C" int tdg_cgan_full_blend(const float* store_yhat, const float* store_ybar, long long slots, int H, int W, int stride,
                                   int offset, float* canvas_yhat, float* canvas_g, void* stream) {
  TDG_CHECK_ARG(store_yhat && store_ybar && canvas_yhat && canvas_g && H > kMinSide && W > kMinSide && stride >= 1 &&
                    offset >= 0 && offset <= kSrc - kCrop,
                "tdg_cgan_full_blend: bad argument (H %d, W %d, stride %d, offset %d)", H, W, stride, offset);
  const int cols = grid_count(H, stride), rows = grid_count(W, stride);
  if ((long long)cols * rows > slots) {
    tdg_set_error("tdg_cgan_full_blend: %d patches, the store holds %lld", cols * rows, slots);
    return TDG_EINVAL;
  }
  tdg_timing_start("cgan_full_blend", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(full_blend_kernel, dim3(tdg_ceil_div(W, 64), tdg_ceil_div(H, 4)), dim3(256), 0, (hipStream_t)stream, store_yhat,
                     store_ybar, H, W, stride, offset, cols, rows, canvas_yhat, canvas_g);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_blend");
  return TDG_OK;
}

extern "C" int tdg_cgan_full_rmse(const float* depth, const float* canvas, int H, int W, double* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(depth && canvas && out && workspace && H > kMinSide && W > kMinSide, "tdg_cgan_full_rmse: bad argument (H %d, W %d)",
                H, W);
  if (workspace_bytes < kRmseBlocks * sizeof(double)) {
    tdg_set_error("tdg_cgan_full_rmse: workspace of %zu bytes, %zu needed", workspace_bytes, kRmseBlocks * sizeof(double));
    return TDG_EWORKSPACE;
  }
  const size_t total = (size_t)(H - kRmseLo - kRmseHi) * (W - kRmseLo - kRmseHi);
  int nblk = (int)((total + 1023) / 1024);
  nblk = nblk < 1 ? 1 : (nblk > kRmseBlocks ? kRmseBlocks : nblk);
  double* part = static_cast<double*>(workspace);
  tdg_timing_start("cgan_full_rmse", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(full_rmse_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, depth, canvas, H, W, part);
  hipLaunchKernelGGL(full_rmse_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, nblk, (double)total, out);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_rmse");
  return TDG_OK;
}
