// experimental_sampler pieces that are not GEMMs (hem/models/experimental_sampler.py): the one pass that assembles every input
// of a generator and critic pass from the staged f32 batch, and the 1x1 one-output-channel tanh head on the FULL plane of the
// last concat with its backward pass.  All of them are memory-bound; wave64 throughout.  The head kernels keep the lane layout,
// the accumulation order and the per-image partials of tdg_cgan.hip's head, so that with g == 0 (tanh' == 1) the backward pass
// is tdg_cgan_head_bwd's at crop == hw bit for bit.  No atomics: two launches are bit-equal.
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

// channels 0..5 of one pixel: one 4-channel and one 2-channel store where the channel stride keeps them aligned (cs % 4 == 0:
// every activation buffer of the engine), six scalar stores otherwise.  Channel 6 and the padding are never written.
template <typename T>
__device__ __forceinline__ void store6(T* p, const float* v, bool vec);
template <>
__device__ __forceinline__ void store6<bf16_t>(bf16_t* p, const float* v, bool vec) {
  if (vec) {
    bf16x4 a;
    bf16x2 b;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = (bf16_t)v[i];
    b[0] = (bf16_t)v[4];
    b[1] = (bf16_t)v[5];
    *reinterpret_cast<bf16x4*>(p) = a;
    *reinterpret_cast<bf16x2*>(p + 4) = b;
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = (bf16_t)v[i];
  }
}
template <>
__device__ __forceinline__ void store6<float>(float* p, const float* v, bool vec) {
  if (vec) {
    f32x4 a;
    f32x2 b;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = v[i];
    b[0] = v[4];
    b[1] = v[5];
    *reinterpret_cast<f32x4*>(p) = a;
    *reinterpret_cast<f32x2*>(p + 4) = b;
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = v[i];
  }
}

__device__ __forceinline__ int mapped_row(const int* rows, int b, int n) {
  const int r = rows ? rows[b] : b;
  return r < 0 ? 0 : (r >= n ? n - 1 : r);                   // a map entry outside [0, n) must not become an address
}

// ---- input assembly: one thread per pixel of the S x S window of output row b ---------------------------------------
// The thread of a pixel inside the T x T crop also writes that pixel's depth target, so the batch is read once.
template <typename T>
__global__ void __launch_bounds__(256) xsamp_prep_kernel(const float* __restrict__ x, const float* __restrict__ xl,
                                                         const float* __restrict__ yl, const float* __restrict__ m,
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
    float v[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __fsub_rn(__fmul_rn(2.f, x[src * 3 + c]), 1.f);       // hem.rescale: 2x exact, one rounding
    v[3] = xl[src];
    v[4] = yl[src];
    v[5] = m[r];
    if (gin) store6<T>(gin + i * gcs, v, gvec);
    if (rin) store6<T>(rin + i * rcs, v, rvec);
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

// ---- generator head: g = tanh(w . cat + b) on every pixel of the hw x hw concat ----------------------------------
// TPP threads per pixel, eight channels each (cin = 8 * TPP); the dot product is finished by a butterfly in the group, as
// tdg_cgan_head_fwd finishes it.  The forward pass has no reduction over pixels, so blockIdx.y splits an image's pixels.
template <typename T, int TPP>
__global__ void __launch_bounds__(256) xsamp_head_fwd_kernel(const T* __restrict__ cat, int hw, int cs, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ g32,
                                                             T* __restrict__ fake, int fcs) {
  const int b = blockIdx.x, lane = threadIdx.x % TPP, grp = threadIdx.x / TPP;
  constexpr int G = 256 / TPP;
  float wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wv[i] = w[lane * 8 + i];
  const float b0 = bias[0];
  const int npix = hw * hw;
  for (int p = blockIdx.y * G + grp; p < npix; p += gridDim.y * G) {
    float v[8];
    load8<T>(cat + ((size_t)b * npix + p) * cs + lane * 8, v);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(v[i], wv[i], s);
#pragma unroll
    for (int o = TPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      const float g = tanhf(s + b0);
      g32[(size_t)b * npix + p] = g;
      fake[((size_t)b * npix + p) * fcs] = from_f32<T>(g);
    }
  }
}

// ---- generator head backward: dz = dL/dg * (1 - g * g) from the stored f32 g, then tdg_cgan_head_bwd's arithmetic at
// crop == hw: dcat = dz (x) w * mask(cat) on every pixel; per-image partials of dW = sum dz * cat and db = sum dz, finished in
// image order by xsamp_head_finish_kernel.
template <typename T, int TPP>
__global__ void __launch_bounds__(256) xsamp_head_bwd_kernel(const T* __restrict__ dfake, int fcs, const float* __restrict__ g32,
                                                             const T* __restrict__ cat, int hw, int cs, const float* __restrict__ w,
                                                             int mmode, float leak, T* __restrict__ dcat, float* __restrict__ partial) {
  constexpr int G = 256 / TPP, CIN = 8 * TPP, COLS = CIN + 1;
  __shared__ float acc_sh[G][CIN];
  __shared__ float db_sh[G];
  const int b = blockIdx.x, lane = threadIdx.x % TPP, grp = threadIdx.x / TPP;
  float wv[8], acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { wv[i] = w[lane * 8 + i]; acc[i] = 0.f; }
  float dbacc = 0.f;
  for (int p = grp; p < hw * hw; p += G) {
    const size_t pix = (size_t)b * hw * hw + p, o = pix * cs + lane * 8;
    const float gv = g32[pix];
    const float d = to_f32<T>(dfake[pix * fcs]) * __fsub_rn(1.f, __fmul_rn(gv, gv));       // two roundings in the factor, one here
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

__global__ void __launch_bounds__(256) xsamp_head_finish_kernel(const float* __restrict__ partial, int n, int cols,
                                                                float* __restrict__ dw, float* __restrict__ db) {
  for (int ch = blockIdx.x * 256 + threadIdx.x; ch < cols; ch += gridDim.x * 256) {
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += partial[(size_t)b * cols + ch];
    if (ch < cols - 1) dw[ch] = s;
    else db[0] = s;
  }
}

}  // namespace

extern "C" int tdg_xsamp_prep(int dtype, const float* x, const float* x_loc, const float* y_loc, const float* m, const float* y,
                              const int* x_rows, const int* y_rows, int n, int S, int T_side, int off, void* g_in, int g_cs,
                              void* rgb_in, int rgb_cs, void* depth_real, int depth_cs, float* target, void* stream) {
  TDG_CHECK_ARG(x && x_loc && y_loc && m && n > 0 && S > 0 && S <= 32768 && T_side > 0 && off >= 0 && off + T_side <= S &&
                    (!g_in || g_cs >= 7) && (!rgb_in || rgb_cs >= 6) && (!depth_real || depth_cs >= 1) &&
                    (y || (!depth_real && !target)),
                "tdg_xsamp_prep: bad argument (n %d, S %d, T %d, off %d, g_cs %d, rgb_cs %d, depth_cs %d)", n, S, T_side, off, g_cs,
                rgb_cs, depth_cs);
  tdg_timing_start("xsamp_prep", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(xsamp_prep_kernel<T>, dim3(grid_for((size_t)n * S * S)), dim3(256), 0, (hipStream_t)stream, x, x_loc, y_loc, m,
                       y, x_rows, y_rows, n, S, T_side, off, static_cast<T*>(g_in), g_cs, static_cast<T*>(rgb_in), rgb_cs,
                       static_cast<T*>(depth_real), depth_cs, target);
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("xsamp_prep");
  return TDG_OK;
}

static inline bool head_cin_ok(int cin) { return cin == 64 || cin == 128 || cin == 256 || cin == 512; }

#define XSAMP_TPP_DISPATCH(cin, ...)                        \
  switch ((cin) / 8) {                                      \
    case 8: { constexpr int TPP = 8; __VA_ARGS__ } break;   \
    case 16: { constexpr int TPP = 16; __VA_ARGS__ } break; \
    case 32: { constexpr int TPP = 32; __VA_ARGS__ } break; \
    case 64: { constexpr int TPP = 64; __VA_ARGS__ } break; \
    default: tdg_set_error("tdg_xsamp_head: cin %d is not 64, 128, 256 or 512", (cin)); return TDG_EINVAL; \
  }

extern "C" int tdg_xsamp_head_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, const float* w, const float* b, float* g,
                                  void* fake, int fake_cs, void* stream) {
  TDG_CHECK_ARG(cat && w && b && g && fake && n > 0 && hw > 0 && hw <= 4096 && head_cin_ok(cin) && cs >= cin && cs % 8 == 0 && fake_cs > 0,
                "tdg_xsamp_head_fwd: bad argument (n %d, hw %d, cin %d of 64, 128, 256, 512, cs %d)", n, hw, cin, cs);
  tdg_timing_start("xsamp_head_fwd", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    XSAMP_TPP_DISPATCH(cin, {
      const int chunks = tdg_ceil_div((long long)hw * hw, 256 / TPP);
      hipLaunchKernelGGL((xsamp_head_fwd_kernel<T, TPP>), dim3(n, chunks < 8 ? chunks : 8), dim3(256), 0, (hipStream_t)stream,
                         static_cast<const T*>(cat), hw, cs, w, b, g, static_cast<T*>(fake), fake_cs);
    })
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("xsamp_head_fwd");
  return TDG_OK;
}

extern "C" int tdg_xsamp_head_bwd(int dtype, const void* dfake, int fake_cs, const float* g, const void* cat, int n, int hw, int cin,
                                  int cs, const float* w, int mask_mode, float leak, void* dcat, float* dw, float* db, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(dfake && g && cat && w && dcat && dw && db && workspace && n > 0 && hw > 0 && hw <= 4096 && head_cin_ok(cin) && cs >= cin &&
                    cs % 8 == 0 && fake_cs > 0,
                "tdg_xsamp_head_bwd: bad argument (n %d, hw %d, cin %d of 64, 128, 256, 512, cs %d)", n, hw, cin, cs);
  const int cols = cin + 1;
  if (workspace_bytes < (size_t)n * cols * sizeof(float)) {
    tdg_set_error("tdg_xsamp_head_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, (size_t)n * cols * sizeof(float));
    return TDG_EWORKSPACE;
  }
  float* part = static_cast<float*>(workspace);
  tdg_timing_start("xsamp_head_bwd", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    XSAMP_TPP_DISPATCH(cin, {
      hipLaunchKernelGGL((xsamp_head_bwd_kernel<T, TPP>), dim3(n), dim3(256), 0, (hipStream_t)stream, static_cast<const T*>(dfake),
                         fake_cs, g, static_cast<const T*>(cat), hw, cs, w, mask_mode, leak, static_cast<T*>(dcat), part);
    })
  })
  hipLaunchKernelGGL(xsamp_head_finish_kernel, dim3(tdg_ceil_div(cols, 256)), dim3(256), 0, (hipStream_t)stream, part, n, cols, dw, db);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("xsamp_head_bwd");
  return TDG_OK;
}
