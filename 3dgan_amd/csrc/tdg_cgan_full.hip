// paper_cgan full-frame inference (paper_fullimage.py of the thesis code): the 65x65 window slid over an H x W frame at
// stride s, the generator's 29x29 outputs blended back into frame-sized canvases, and the frame RMSE.
//
// Grid (build_batch): cols = (H - 93) / s windows down, rows = (W - 93) / s across; patch c = n * cols + m (n < rows
// outer, m < cols inner: column-major, the window moves down first) has its top-left corner at (m s, n s).  Its 29x29
// output lands at (m s + off, n s + off) of the canvas.
//
// Whole-frame sampling of paper_sampler / paper_noise (SamplerReplica.sample_full) runs on the same grid with every window
// repeated `rep` times in the staging buffers -- the sampler set's batch of copies of ONE image, one noise draw per copy
// (hem/models/paper_sampler.py:88-101) -- and reduces each group of draws to the per-pixel mean and variance that the frame
// blend takes.  y_hat is read as the head stored it (f32); everything after that is f64, the variance two-pass.  No float
// atomics: fixed slice and draw order, so two launches are bit-equal.  All of these are memory- or latency-bound; wave64
// throughout.
#include "tdg_cgan_common.h"

namespace {

constexpr int kRmseBlocks = 256;
constexpr int kRmseLo = 18, kRmseHi = 46;               // rmse region: [18, H - 46) x [18, W - 46)
constexpr int kColBlocks = (kCrop2 + 63) / 64;           // 14 blocks of 64 pixels
constexpr int kRow = kSrc * 3 + kSrc;                    // a staged row: 195 image floats, then 65 depth floats
constexpr int kWindow = kSrc * kRow;

inline int grid_count(int side, int s) { return (side - kMinSide) / s; }

// ---- patch gather: window c = chunk * G + g into rows [g rep, g rep + rep) of x [B,65,65,3] / y [B,65,65,1] ----------------
// One thread per (window, staged float, copy slice): it reads its float once and writes the copies j = slice, slice + nsl, ...
// Consecutive lanes hold consecutive floats of a staged row, contiguous in the frame and in every copy.  REP = false is
// tdg_cgan_full_gather: one copy, one slice, a depth that is never null.
template <bool REP>
__global__ void __launch_bounds__(256) full_gather_kernel(const float* __restrict__ image, const float* __restrict__ depth, int W,
                                                          int s, int cols, int P, const int* __restrict__ chunk, int G, int rep_,
                                                          int nsl_, float* __restrict__ x, float* __restrict__ y) {
  const int rep = REP ? rep_ : 1, nsl = REP ? nsl_ : 1;
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
      v = rgb ? image[row * 3 + k] : (!REP || depth ? depth[row + (k - kSrc * 3)] : 0.f);
    }
    for (int j = sl; j < rep; j += nsl) {
      const size_t b = (size_t)g * rep + j;
      if (rgb) x[(b * kSrc + r) * (kSrc * 3) + k] = v;
      else y[(b * kSrc + r) * kSrc + (k - kSrc * 3)] = v;
    }
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

// ---- sample store: group k (rows [k draws, k draws + draws)) to slot chunk * groups + k ------------------------------------
// blockIdx.y is the group.  Blocks x < 14 own 64 consecutive pixels and take the draws' moments with slice_moments.  Block
// x == 14 (launched only with a crop) owns the group's per-draw errors: wave w sums |crop - y_hat| of its draws d = w, w + 8,
// ... over all the pixels, keeps their sum and min in draw order, and wave 0 combines the slices in slice order.
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
      a = wave_sum(a) / (double)kCrop2;                     // (lane 0 holds the draw's value)
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
  const double my = slice_moments(yh, draws, kCrop2, p, ok, sh);
  if (sl != 0) return;
  const double vy = slice_total(sh) / (double)draws;
  if (ok) {
    st_yhat[slot * kCrop2 + p] = (float)my;                 // 10x depth, as tdg_cgan_full_store writes
    st_var[slot * kCrop2 + p] = (float)(vy / 100.0);        // [0, 1] units
  }
  if (blockIdx.x == 0 && lane == 0) st_ybar[slot] = ybar ? ybar[(size_t)k * draws] : 0.f;
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
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = block_total(sh);
}

__global__ void full_rmse_finish_kernel(const double* __restrict__ part, int nblk, double count, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[b];
  out[0] = sqrt(s / count);
}

}  // namespace

// both gathers: REP = false is tdg_cgan_full_gather's single copy (rep = 1)
template <bool REP>
static int full_gather(const char* what, const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch,
                       int rep, float* x_stage, float* y_stage, hipStream_t stream) {
  const int cols = grid_count(H, stride), rows = grid_count(W, stride);
  const int G = batch / rep, nsl = rep < kSlices ? rep : kSlices;
  tdg_timing_start(what, 0.0, stream);
  hipLaunchKernelGGL(full_gather_kernel<REP>, dim3(grid_for((size_t)G * nsl * kWindow)), dim3(256), 0, stream, image, depth, W, stride,
                     cols > 0 ? cols : 1, cols * rows, chunk, G, rep, nsl, x_stage, y_stage);
  tdg_timing_stop(stream);
  TDG_HIP_LAUNCH_CHECK(what);
  return TDG_OK;
}

extern "C" int tdg_cgan_full_gather(const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch,
                                    float* x_stage, float* y_stage, void* stream) {
  TDG_CHECK_ARG(image && depth && chunk && x_stage && y_stage && H > kMinSide && W > kMinSide && stride >= 1 && batch > 0,
                "tdg_cgan_full_gather: bad argument (H %d, W %d, stride %d, batch %d)", H, W, stride, batch);
  return full_gather<false>("cgan_full_gather", image, depth, H, W, stride, chunk, batch, 1, x_stage, y_stage, (hipStream_t)stream);
}

extern "C" int tdg_cgan_full_gather_rep(const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch,
                                        int rep, float* x_stage, float* y_stage, void* stream) {
  TDG_CHECK_ARG(image && chunk && x_stage && y_stage && H > kMinSide && W > kMinSide && stride >= 1 && batch > 0,
                "tdg_cgan_full_gather_rep: bad argument (H %d, W %d, stride %d, batch %d)", H, W, stride, batch);
  TDG_CHECK_ARG(rep >= 1 && batch % rep == 0, "tdg_cgan_full_gather_rep: rep %d must be at least 1 and divide batch %d", rep, batch);
  return full_gather<true>("cgan_full_gather_rep", image, depth, H, W, stride, chunk, batch, rep, x_stage, y_stage, (hipStream_t)stream);
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
  hipLaunchKernelGGL(full_next_chunk_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, chunk);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_full_sample_store");
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
