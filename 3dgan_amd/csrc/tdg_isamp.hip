// improved_sampler pieces that are not GEMMs (hem/models/improved_sampler.py): the input assembly of tdg_xsamp_prep made general
// in the number of planes, the source side and the crop; generator A1's head, whose 1x1 conv passes through a one-channel batch
// norm before tanh, with its backward pass; the gradient of the RMSE term of `--g_rmse`; and tf.nn.zero_fraction for
// `--g_sparsity`.  All of them are memory-bound; wave64 throughout.  The head keeps tdg_xsamp_head's lane layout (TPP threads
// per pixel, eight channels each) and its per-image partials.  Every sum has a fixed order and there are no atomics: two
// launches are bit-equal.
#include "tdg_cgan_common.h"

namespace {

// eight consecutive channels as f32 (16-byte loads for bf16, two for f32)
template <typename T>
__device__ __forceinline__ void load8(const T* p, float* v);
template <>
__device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float* v) {
  const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)q[i];
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float* v) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float* v);
template <>
__device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float* v) {
  bf16x8 q;
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = (bf16_t)v[i];
  *reinterpret_cast<bf16x8*>(p) = q;
}
template <>
__device__ __forceinline__ void store8<float>(float* p, const float* v) {
  f32x4 a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) { a[i] = v[i]; b[i] = v[4 + i]; }
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}

template <typename T>
struct Vec;
template <>
struct Vec<bf16_t> { using v4 = bf16x4; using v2 = bf16x2; };
template <>
struct Vec<float> { using v4 = f32x4; using v2 = f32x2; };

// channels 0..P-1 of one pixel: where the channel stride keeps them aligned (cs % 4 == 0: every activation buffer of the
// engine) a 4-channel store and what is left of P behind it (P = 3: a 2-channel store and one channel), single channels
// otherwise.  Channel P and the padding are never written.
template <typename T, int P>
__device__ __forceinline__ void store_planes(T* p, const float* v, bool vec) {
  using V4 = typename Vec<T>::v4;
  using V2 = typename Vec<T>::v2;
  if (!vec) {
#pragma unroll
    for (int i = 0; i < P; ++i) p[i] = from_f32<T>(v[i]);
    return;
  }
  int at = 0;
  if constexpr (P >= 4) {
    V4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = from_f32<T>(v[i]);
    *reinterpret_cast<V4*>(p) = a;
    at = 4;
  }
  if constexpr (P - (P >= 4 ? 4 : 0) >= 2) {
    V2 b;
    b[0] = from_f32<T>(v[at]);
    b[1] = from_f32<T>(v[at + 1]);
    *reinterpret_cast<V2*>(p + at) = b;
    at += 2;
  }
  if (at < P) p[at] = from_f32<T>(v[at]);
}

__device__ __forceinline__ int mapped_row(const int* rows, int b, int n) {
  const int r = rows ? rows[b] : b;
  return r < 0 ? 0 : (r >= n ? n - 1 : r);                   // a map entry outside [0, n) must not become an address
}

// ---- input assembly: one thread per pixel of the S x S window of output row b ---------------------------------------
// The thread of a pixel inside the T x T crop also writes that pixel's depth target, so the batch is read once.
template <typename T, int P>
__global__ void __launch_bounds__(256) isamp_prep_kernel(const float* __restrict__ x, const float* __restrict__ xl,
                                                         const float* __restrict__ yl, const float* __restrict__ mv,
                                                         const float* __restrict__ y, const int* __restrict__ x_rows,
                                                         const int* __restrict__ y_rows, int n, int S, int Tc, int off,
                                                         T* __restrict__ gin, int gcs, T* __restrict__ rin, int rcs,
                                                         T* __restrict__ dreal, int dcs, float* __restrict__ target) {
  const size_t ss = (size_t)S * S, total = (size_t)n * ss;
  const bool gvec = (gcs & 3) == 0, rvec = (rcs & 3) == 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / ss), p = (int)(i - (size_t)b * ss);
    const int r = mapped_row(x_rows, b, n);
    const size_t src = (size_t)r * ss + p;
    float v[P];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fsub_rn(__fmul_rn(2.f, x[src * 3 + c]), 1.f);       // hem.rescale: 2x exact, one rounding
    if constexpr (P >= 5) {
      v[3] = xl[src];
      v[4] = yl[src];
    }
    if constexpr (P >= 6) v[5] = mv[src];
    if (gin) store_planes<T, P>(gin + i * gcs, v, gvec);
    if (rin) store_planes<T, P>(rin + i * rcs, v, rvec);
    if (y) {
      const int row = p / S, col = p - row * S;
      const int tr = row - off, tc = col - off;
      if (tr >= 0 && tr < Tc && tc >= 0 && tc < Tc) {
        const int q = mapped_row(y_rows, b, n);
        const float d = __fsub_rn(__fmul_rn(2.f, y[(size_t)q * ss + p]), 1.f);
        const size_t o = ((size_t)b * Tc + tr) * Tc + tc;
        if (dreal) dreal[o * dcs] = from_f32<T>(d);
        if (target) target[o] = d;
      }
    }
  }
}

// ---- the batch's two f64 sums from the per-image partials part[b][2], by every thread of a 256-thread block in one fixed order:
// thread t takes the images t, t + 256, ..., then the wave sums, then the four waves in wave order.  sh: 2 x 4 doubles.
__device__ __forceinline__ void batch_sums(const double* __restrict__ part, int n, double (*sh)[4], double* s0, double* s1) {
  double a = 0.0, c = 0.0;
  for (int b = threadIdx.x; b < n; b += 256) {
    a += part[2 * b];
    c += part[2 * b + 1];
  }
  a = wave_sum(a);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  *s0 = block_total(sh[0]);
  *s1 = block_total(sh[1]);
}

// ---- A1's head, forward, phase 1: z = w . cat + b per pixel (tdg_xsamp_head_fwd's accumulation) into zbuf, and the image's
// f64 sums of z and z z into part[b][2].  One block per image: group grp takes the pixels grp, grp + G, ...; the groups meet in
// LDS in group order.
template <typename T, int TPP>
__global__ void __launch_bounds__(256) isamp_head_z_kernel(const T* __restrict__ cat, int hw, int cs, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ zbuf,
                                                           double* __restrict__ part) {
  constexpr int G = 256 / TPP;
  __shared__ double s_sh[G], q_sh[G];
  const int b = blockIdx.x, lane = threadIdx.x % TPP, grp = threadIdx.x / TPP;
  float wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wv[i] = w[lane * 8 + i];
  const float b0 = bias[0];
  const int npix = hw * hw;
  double s = 0.0, q = 0.0;
  for (int p = grp; p < npix; p += G) {
    float v[8];
    load8<T>(cat + ((size_t)b * npix + p) * cs + lane * 8, v);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) d = fmaf(v[i], wv[i], d);
#pragma unroll
    for (int o = TPP / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    const float z = d + b0;                                  // the butterfly leaves the same sum in every lane of the group
    if (lane == 0) zbuf[(size_t)b * npix + p] = z;
    s += (double)z;
    q += (double)z * (double)z;
  }
  if (lane == 0) {
    s_sh[grp] = s;
    q_sh[grp] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = 0.0, tq = 0.0;
    for (int g = 0; g < G; ++g) {
      ts += s_sh[g];
      tq += q_sh[g];
    }
    part[2 * b] = ts;
    part[2 * b + 1] = tq;
  }
}

// ---- forward, phase 2: finish the statistics (every block, the same order), then one thread per value:
// zhat = fl(fl(z - mean) * rstd), g = tanhf(fl(zhat + beta)).
template <typename T>
__global__ void __launch_bounds__(256) isamp_head_bn_apply_kernel(const double* __restrict__ part, int n, int npix, float eps,
                                                                  const float* __restrict__ beta, float* __restrict__ zbuf,
                                                                  float* __restrict__ g32, T* __restrict__ fake, int fcs,
                                                                  float* __restrict__ stats) {
  __shared__ double sh[2][4];
  double s, q;
  batch_sums(part, n, sh, &s, &q);
  const double N = (double)n * (double)npix, mean_d = s / N;
  double var = q / N - mean_d * mean_d;                      // biased, as tf.nn.moments
  var = var < 0.0 ? 0.0 : var;
  const float mean = (float)mean_d, rstd = (float)(1.0 / sqrt(var + (double)eps)), be = beta[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = rstd;
  }
  const size_t total = (size_t)n * npix;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const float zh = __fmul_rn(__fsub_rn(zbuf[i], mean), rstd);
    const float g = tanhf(__fadd_rn(zh, be));
    zbuf[i] = zh;
    g32[i] = g;
    fake[i * fcs] = from_f32<T>(g);
  }
}

// dy = dL/dg * fl(1 - fl(g g)): the derivative of tanh from the stored f32 g, as tdg_xsamp_head_bwd takes it
template <typename T>
__device__ __forceinline__ float tanh_seed(const T* dfake, int fcs, const float* g32, size_t pix) {
  const float gv = g32[pix];
  return to_f32<T>(dfake[pix * fcs]) * __fsub_rn(1.f, __fmul_rn(gv, gv));
}

// ---- A1's head, backward, phase 1: the image's f64 sums of dy and dy zhat into part[b][2].  One block per image, thread t the
// pixels t, t + 256, ...
template <typename T>
__global__ void __launch_bounds__(256) isamp_head_bn_sums_kernel(const T* __restrict__ dfake, int fcs, const float* __restrict__ g32,
                                                                 const float* __restrict__ zhat, int npix, double* __restrict__ part) {
  __shared__ double sh[2][4];
  const int b = blockIdx.x;
  double a = 0.0, c = 0.0;
  for (int p = threadIdx.x; p < npix; p += 256) {
    const size_t pix = (size_t)b * npix + p;
    const float dy = tanh_seed<T>(dfake, fcs, g32, pix);
    a += (double)dy;
    c += (double)dy * (double)zhat[pix];
  }
  a = wave_sum(a);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) {
    sh[0][threadIdx.x >> 6] = a;
    sh[1][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * b] = block_total(sh[0]);
    part[2 * b + 1] = block_total(sh[1]);
  }
}

// ---- backward, phase 2: m1 = mean(dy), m2 = mean(dy zhat) from the partials, dz = fl(rstd * fl(fl(dy - m1) - fl(zhat m2))),
// then tdg_xsamp_head_bwd's arithmetic from dz on: dcat = dz (x) w * mask(cat), per-image partials of dW and db.
template <typename T, int TPP>
__global__ void __launch_bounds__(256) isamp_head_bn_bwd_kernel(const T* __restrict__ dfake, int fcs, const float* __restrict__ g32,
                                                                const float* __restrict__ zhat, const float* __restrict__ stats,
                                                                const double* __restrict__ part, int n, const T* __restrict__ cat,
                                                                int hw, int cs, const float* __restrict__ w, int mmode, float leak,
                                                                T* __restrict__ dcat, float* __restrict__ partial,
                                                                float* __restrict__ dbeta) {
  constexpr int G = 256 / TPP, CIN = 8 * TPP, COLS = CIN + 1;
  __shared__ float acc_sh[G][CIN];
  __shared__ float db_sh[G];
  __shared__ double sh[2][4];
  const int b = blockIdx.x, lane = threadIdx.x % TPP, grp = threadIdx.x / TPP, npix = hw * hw;
  double s1, s2;
  batch_sums(part, n, sh, &s1, &s2);
  const double N = (double)n * (double)npix;
  const float m1 = (float)(s1 / N), m2 = (float)(s2 / N), rstd = stats[1];
  if (b == 0 && threadIdx.x == 0) dbeta[0] = (float)s1;
  float wv[8], acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { wv[i] = w[lane * 8 + i]; acc[i] = 0.f; }
  float dbacc = 0.f;
  for (int p = grp; p < npix; p += G) {
    const size_t pix = (size_t)b * npix + p, o = pix * cs + lane * 8;
    const float dy = tanh_seed<T>(dfake, fcs, g32, pix);
    const float d = __fmul_rn(rstd, __fsub_rn(__fsub_rn(dy, m1), __fmul_rn(zhat[pix], m2)));
    float v[8], out[8];
    load8<T>(cat + o, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc[i] = fmaf(d, v[i], acc[i]);
      out[i] = d * wv[i] * mask_factor(v[i], mmode, leak);
    }
    dbacc += d;
    store8<T>(dcat + o, out);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc_sh[grp][lane * 8 + i] = acc[i];
  if (lane == 0) db_sh[grp] = dbacc;
  __syncthreads();
  float* pi = partial + (size_t)b * COLS;
  for (int ch = threadIdx.x; ch < COLS; ch += 256) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += ch < CIN ? acc_sh[g][ch] : db_sh[g];
    pi[ch] = s;
  }
}

__global__ void __launch_bounds__(256) isamp_head_finish_kernel(const float* __restrict__ partial, int n, int cols,
                                                                float* __restrict__ dw, float* __restrict__ db) {
  for (int ch = blockIdx.x * 256 + threadIdx.x; ch < cols; ch += gridDim.x * 256) {
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += partial[(size_t)b * cols + ch];
    if (ch < cols - 1) dw[ch] = s;
    else db[0] = s;
  }
}

// ---- d rmse / d g added to dL/dg: one thread per row ------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) isamp_rmse_grad_kernel(const T* __restrict__ g, const T* __restrict__ y, int rows, int cs,
                                                              const float* __restrict__ rmse, T* __restrict__ dfake, int dgs) {
  const float k = __fdiv_rn(1.f, __fmul_rn(__fmul_rn(4.f, (float)rows), rmse[0]));
  for (size_t r = (size_t)blockIdx.x * 256 + threadIdx.x; r < (size_t)rows; r += (size_t)gridDim.x * 256) {
    const float t = __fmul_rn(__fsub_rn(to_f32<T>(g[r * cs]), to_f32<T>(y[r * cs])), k);
    dfake[r * dgs] = from_f32<T>(__fadd_rn(to_f32<T>(dfake[r * dgs]), t));
  }
}

// ---- zero_fraction: per-block counts of the exact zeros (v == 0 holds for -0.0), then one block adds them in block order -----
constexpr int kZeroBlocks = 256;

template <typename T>
__global__ void __launch_bounds__(256) isamp_zero_count_kernel(const T* __restrict__ x, int rows, int c, int cs,
                                                               unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long sh[4];
  const size_t total = (size_t)rows * c;
  unsigned long long k = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t r = i / c, col = i - r * c;
    k += to_f32<T>(x[r * cs + col]) == 0.f ? 1ull : 0ull;
  }
  k = wave_sum(k);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = block_total(sh);
}

__global__ void __launch_bounds__(256) isamp_zero_finish_kernel(const unsigned long long* __restrict__ counts, int nblk, double total,
                                                                float* __restrict__ out) {
  __shared__ unsigned long long sh[4];
  unsigned long long k = 0;
  for (int b = threadIdx.x; b < nblk; b += 256) k += counts[b];
  k = wave_sum(k);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((double)block_total(sh) / total);
}

}  // namespace

extern "C" int tdg_isamp_prep(int dtype, const float* x, const float* x_loc, const float* y_loc, const float* mean_vec, const float* y,
                              const int* x_rows, const int* y_rows, int n, int S, int T_side, int off, int planes, void* g_in, int g_cs,
                              void* rgb_in, int rgb_cs, void* depth_real, int depth_cs, float* target, void* stream) {
  TDG_CHECK_ARG(x && (planes == 3 || planes == 5 || planes == 6) && (planes < 5 || (x_loc && y_loc)) && (planes < 6 || mean_vec) &&
                    n > 0 && S > 0 && S <= 32768 && T_side > 0 && off >= 0 && off + T_side <= S && (!g_in || g_cs >= planes + 1) &&
                    (!rgb_in || rgb_cs >= planes) && (!depth_real || depth_cs >= 1) && (y || (!depth_real && !target)),
                "tdg_isamp_prep: bad argument (planes %d of 3, 5, 6, n %d, S %d, T %d, off %d, g_cs %d, rgb_cs %d, depth_cs %d)", planes,
                n, S, T_side, off, g_cs, rgb_cs, depth_cs);
  tdg_timing_start("isamp_prep", 0.0, (hipStream_t)stream);
#define ISAMP_PREP_LAUNCH(P)                                                                                                        \
  hipLaunchKernelGGL((isamp_prep_kernel<T, P>), dim3(grid_for((size_t)n * S * S)), dim3(256), 0, (hipStream_t)stream, x, x_loc, y_loc, \
                     mean_vec, y, x_rows, y_rows, n, S, T_side, off, static_cast<T*>(g_in), g_cs, static_cast<T*>(rgb_in), rgb_cs,   \
                     static_cast<T*>(depth_real), depth_cs, target)
  DISPATCH_T(dtype, {
    if (planes == 3) ISAMP_PREP_LAUNCH(3);
    else if (planes == 5) ISAMP_PREP_LAUNCH(5);
    else ISAMP_PREP_LAUNCH(6);
  })
#undef ISAMP_PREP_LAUNCH
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("isamp_prep");
  return TDG_OK;
}

static inline bool head_cin_ok(int cin) { return cin == 64 || cin == 128 || cin == 256 || cin == 512; }

#define ISAMP_TPP_DISPATCH(cin, ...)                        \
  switch ((cin) / 8) {                                      \
    case 8: { constexpr int TPP = 8; __VA_ARGS__ } break;   \
    case 16: { constexpr int TPP = 16; __VA_ARGS__ } break; \
    case 32: { constexpr int TPP = 32; __VA_ARGS__ } break; \
    case 64: { constexpr int TPP = 64; __VA_ARGS__ } break; \
    default: tdg_set_error("tdg_isamp_head_bn: cin %d is not 64, 128, 256 or 512", (cin)); return TDG_EINVAL; \
  }

extern "C" size_t tdg_isamp_head_bn_workspace_bytes(int n, int cin) {
  return n > 0 && cin > 0 ? (size_t)n * 2 * sizeof(double) + (size_t)n * (cin + 1) * sizeof(float) : 0;
}

extern "C" int tdg_isamp_head_bn_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, const float* w, const float* b,
                                     const float* beta, float eps, float* g, float* zhat, float* stats, void* fake, int fake_cs,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(cat && w && b && beta && g && zhat && stats && fake && workspace && n > 0 && hw > 0 && hw <= 4096 && head_cin_ok(cin) &&
                    cs >= cin && cs % 8 == 0 && fake_cs > 0 && eps > 0.f && ((uintptr_t)workspace & 7) == 0,
                "tdg_isamp_head_bn_fwd: bad argument (n %d, hw %d, cin %d of 64, 128, 256, 512, cs %d, eps %g)", n, hw, cin, cs,
                (double)eps);
  if (workspace_bytes < (size_t)n * 2 * sizeof(double)) {
    tdg_set_error("tdg_isamp_head_bn_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)n * 2 * sizeof(double));
    return TDG_EWORKSPACE;
  }
  double* part = static_cast<double*>(workspace);
  tdg_timing_start("isamp_head_bn_fwd", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    ISAMP_TPP_DISPATCH(cin, {
      hipLaunchKernelGGL((isamp_head_z_kernel<T, TPP>), dim3(n), dim3(256), 0, (hipStream_t)stream, static_cast<const T*>(cat), hw, cs,
                         w, b, zhat, part);
    })
    hipLaunchKernelGGL(isamp_head_bn_apply_kernel<T>, dim3(grid_for((size_t)n * hw * hw)), dim3(256), 0, (hipStream_t)stream, part, n,
                       hw * hw, eps, beta, zhat, g, static_cast<T*>(fake), fake_cs, stats);
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("isamp_head_bn_fwd");
  return TDG_OK;
}

extern "C" int tdg_isamp_head_bn_bwd(int dtype, const void* dfake, int fake_cs, const float* g, const float* zhat, const float* stats,
                                     const void* cat, int n, int hw, int cin, int cs, const float* w, int mask_mode, float leak,
                                     void* dcat, float* dw, float* db, float* dbeta, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  TDG_CHECK_ARG(dfake && g && zhat && stats && cat && w && dcat && dw && db && dbeta && workspace && n > 0 && hw > 0 && hw <= 4096 &&
                    head_cin_ok(cin) && cs >= cin && cs % 8 == 0 && fake_cs > 0 && ((uintptr_t)workspace & 7) == 0,
                "tdg_isamp_head_bn_bwd: bad argument (n %d, hw %d, cin %d of 64, 128, 256, 512, cs %d)", n, hw, cin, cs);
  const int cols = cin + 1;
  if (workspace_bytes < tdg_isamp_head_bn_workspace_bytes(n, cin)) {
    tdg_set_error("tdg_isamp_head_bn_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, tdg_isamp_head_bn_workspace_bytes(n, cin));
    return TDG_EWORKSPACE;
  }
  double* part = static_cast<double*>(workspace);
  float* colp = reinterpret_cast<float*>(part + (size_t)n * 2);
  tdg_timing_start("isamp_head_bn_bwd", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(isamp_head_bn_sums_kernel<T>, dim3(n), dim3(256), 0, (hipStream_t)stream, static_cast<const T*>(dfake), fake_cs, g,
                       zhat, hw * hw, part);
    ISAMP_TPP_DISPATCH(cin, {
      hipLaunchKernelGGL((isamp_head_bn_bwd_kernel<T, TPP>), dim3(n), dim3(256), 0, (hipStream_t)stream, static_cast<const T*>(dfake),
                         fake_cs, g, zhat, stats, part, n, static_cast<const T*>(cat), hw, cs, w, mask_mode, leak, static_cast<T*>(dcat),
                         colp, dbeta);
    })
  })
  hipLaunchKernelGGL(isamp_head_finish_kernel, dim3(tdg_ceil_div(cols, 256)), dim3(256), 0, (hipStream_t)stream, colp, n, cols, dw, db);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("isamp_head_bn_bwd");
  return TDG_OK;
}

extern "C" int tdg_isamp_rmse_grad(int dtype, const void* g, const void* y, int rows, int cs, const float* rmse, void* dfake, int dgs,
                                   void* stream) {
  TDG_CHECK_ARG(g && y && rmse && dfake && rows > 0 && cs > 0 && dgs > 0, "tdg_isamp_rmse_grad: bad argument (rows %d, cs %d, dgs %d)",
                rows, cs, dgs);
  tdg_timing_start("isamp_rmse_grad", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(isamp_rmse_grad_kernel<T>, dim3(grid_for((size_t)rows)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const T*>(g), static_cast<const T*>(y), rows, cs, rmse, static_cast<T*>(dfake), dgs);
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("isamp_rmse_grad");
  return TDG_OK;
}

extern "C" size_t tdg_isamp_zero_fraction_workspace_bytes(void) { return kZeroBlocks * sizeof(unsigned long long); }

extern "C" int tdg_isamp_zero_fraction(int dtype, const void* x, int rows, int c, int cs, float* out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(x && out && workspace && rows > 0 && c > 0 && cs >= c && ((uintptr_t)workspace & 7) == 0,
                "tdg_isamp_zero_fraction: bad argument (rows %d, c %d, cs %d)", rows, c, cs);
  if (workspace_bytes < tdg_isamp_zero_fraction_workspace_bytes()) {
    tdg_set_error("tdg_isamp_zero_fraction: workspace of %zu bytes, %zu needed", workspace_bytes, tdg_isamp_zero_fraction_workspace_bytes());
    return TDG_EWORKSPACE;
  }
  const size_t total = (size_t)rows * c;
  const int nblk = (int)((total + 255) / 256 < (size_t)kZeroBlocks ? (total + 255) / 256 : (size_t)kZeroBlocks);
  unsigned long long* counts = static_cast<unsigned long long*>(workspace);
  tdg_timing_start("isamp_zero_fraction", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(isamp_zero_count_kernel<T>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, static_cast<const T*>(x), rows, c, cs,
                       counts);
  })
  hipLaunchKernelGGL(isamp_zero_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, counts, nblk, (double)total, out);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("isamp_zero_fraction");
  return TDG_OK;
}
