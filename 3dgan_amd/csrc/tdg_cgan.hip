// paper_cgan pieces that are not GEMMs (hem/models/paper_cgan.py): the depth target's crop / rescale / per-image mean,
// the 1x1 one-output-channel generator head with its top-left crop, the D input join of the shared rgb path, the WGAN
// loss on sigmoid outputs and the Eigen-2014 depth metrics.  All of them are memory-bound; wave64 throughout.
#include "tdg_cgan_metrics.h"

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

// ---- target prep: one workgroup (256 threads) per image ------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cgan_prep_kernel(const float* __restrict__ y, int version, T* __restrict__ dreal, int dcs,
                                                        T* __restrict__ dfake, float* __restrict__ ybar, float* __restrict__ crop,
                                                        T* __restrict__ gones, int gcs, T* __restrict__ rgbbar, int rcs) {
  __shared__ float sh[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* yi = y + (size_t)b * kSrc * kSrc;
  float* ci = crop + (size_t)b * kCrop * kCrop;
  float s = 0.f;
  for (int p = t; p < kCrop * kCrop; p += 256) {
    const int r = p / kCrop, c = p - r * kCrop;
    const float v = yi[(r + kOff) * kSrc + c + kOff] * 10.f;
    ci[p] = v;
    s += v;
  }
  s = wave_sum(s);
  if ((t & 63) == 0) sh[t >> 6] = s;
  __syncthreads();
  const float m = block_total(sh) / (float)(kCrop * kCrop);     // every thread: the same order
  if (t == 0) ybar[b] = m;
  const size_t d0 = (size_t)b * kCrop * kCrop * dcs;
  for (int p = t; p < kCrop * kCrop; p += 256) {
    const float v = ci[p];
    dreal[d0 + (size_t)p * dcs] = from_f32<T>(version == 0 ? v : v - m);
    if (version == 2) {
      dreal[d0 + (size_t)p * dcs + 1] = from_f32<T>(m);
      dfake[d0 + (size_t)p * dcs + 1] = from_f32<T>(m);
    }
  }
  if (gones || rgbbar) {
    const T one = from_f32<T>(1.f), mb = from_f32<T>(m);
    for (int p = t; p < kSrc * kSrc; p += 256) {
      if (gones) gones[((size_t)b * kSrc * kSrc + p) * gcs] = one;
      if (rgbbar) rgbbar[((size_t)b * kSrc * kSrc + p) * rcs] = mb;
    }
  }
}

// ---- generator head: G = w . cat + b on the top-left crop x crop pixels of the hw x hw concat -------------------
// TPP threads per pixel, eight channels each (cin = 8 * TPP); the dot product is finished by a butterfly in the group.
// NOISE (paper_sampler --noise_layer d4): the head is a cin + 1 -> 1 conv whose last input channel is the f32 draw
// u [n,hw,hw], read in place of a widened concat: g = w . cat + w[cin] * u + b.  g32 (nullable): g as f32 [n,crop,crop].
template <typename T, int TPP, bool NOISE>
__global__ void __launch_bounds__(256) cgan_head_fwd_kernel(const T* __restrict__ cat, int hw, int cs, int crop,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ u, const float* __restrict__ ybar,
                                                            float* __restrict__ yhat, float* __restrict__ g32,
                                                            T* __restrict__ fake, int fcs) {
  const int b = blockIdx.x, lane = threadIdx.x % TPP, grp = threadIdx.x / TPP;
  constexpr int G = 256 / TPP;
  float wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wv[i] = w[lane * 8 + i];
  const float b0 = bias[0], off = ybar ? ybar[b] : 0.f;
  const float wn = NOISE ? w[8 * TPP] : 0.f;
  const int npix = crop * crop;
  for (int p = grp; p < npix; p += G) {
    const int r = p / crop, c = p - r * crop;
    float v[8];
    load8<T>(cat + ((size_t)b * hw * hw + (size_t)r * hw + c) * cs + lane * 8, v);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s = fmaf(v[i], wv[i], s);
#pragma unroll
    for (int o = TPP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      if constexpr (NOISE) s = fmaf(wn, u[(size_t)b * hw * hw + (size_t)r * hw + c], s);
      const float g = s + b0;
      yhat[(size_t)b * npix + p] = g + off;
      if (g32) g32[(size_t)b * npix + p] = g;
      fake[((size_t)b * npix + p) * fcs] = from_f32<T>(g);
    }
  }
}

// ---- generator head backward: dcat = delta (x) w * mask(cat) on every pixel (zero outside the crop); per-image
// partials of dW = sum delta * cat and db = sum delta, finished in a fixed order by cgan_head_finish_kernel.
// NOISE: one more partial column, dW[cin] = sum delta * u, between dW[0:cin] and db; the draw gets no gradient.
template <typename T, int TPP, bool NOISE>
__global__ void __launch_bounds__(256) cgan_head_bwd_kernel(const T* __restrict__ dfake, int fcs, const T* __restrict__ cat, int hw,
                                                            int cs, int crop, const float* __restrict__ w,
                                                            const float* __restrict__ u, int mmode, float leak,
                                                            T* __restrict__ dcat, float* __restrict__ partial) {
  constexpr int G = 256 / TPP, CIN = 8 * TPP, COLS = CIN + (NOISE ? 2 : 1);
  __shared__ float acc_sh[G][CIN];
  __shared__ float db_sh[G];
  __shared__ float dn_sh[G];
  const int b = blockIdx.x, lane = threadIdx.x % TPP, grp = threadIdx.x / TPP;
  float wv[8], acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { wv[i] = w[lane * 8 + i]; acc[i] = 0.f; }
  float dbacc = 0.f, dnacc = 0.f;
  for (int p = grp; p < hw * hw; p += G) {
    const int r = p / hw, c = p - r * hw;
    const size_t o = ((size_t)b * hw * hw + p) * cs + lane * 8;
    float out[8];
    if (r < crop && c < crop) {
      const float d = to_f32<T>(dfake[((size_t)b * crop * crop + r * crop + c) * fcs]);
      float v[8];
      load8<T>(cat + o, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        acc[i] = fmaf(d, v[i], acc[i]);
        out[i] = d * wv[i] * mask_factor(v[i], mmode, leak);
      }
      dbacc += d;
      if constexpr (NOISE) dnacc = fmaf(d, u[(size_t)b * hw * hw + p], dnacc);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) out[i] = 0.f;
    }
    store8<T>(dcat + o, out);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc_sh[grp][lane * 8 + i] = acc[i];
  if (lane == 0) { db_sh[grp] = dbacc; dn_sh[grp] = dnacc; }
  __syncthreads();
  float* pi = partial + (size_t)b * COLS;
  for (int ch = threadIdx.x; ch < COLS; ch += 256) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += ch < CIN ? acc_sh[g][ch] : (ch == COLS - 1 ? db_sh[g] : dn_sh[g]);
    pi[ch] = s;
  }
}

__global__ void __launch_bounds__(256) cgan_head_finish_kernel(const float* __restrict__ partial, int n, int cols,
                                                               float* __restrict__ dw, float* __restrict__ db) {
  for (int ch = blockIdx.x * 256 + threadIdx.x; ch < cols; ch += gridDim.x * 256) {
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += partial[(size_t)b * cols + ch];
    if (ch < cols - 1) dw[ch] = s;
    else db[0] = s;
  }
}

// ---- D input join: the rgb path ran once over n images, the depth path over 2n -------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cgan_join_kernel(int mode, int n_rgb, int rows, int c, T* __restrict__ comb, int ccs,
                                                        T* __restrict__ rgb, int rcs, T* __restrict__ depth, int dcs) {
  const int c8 = c / 8;
  const size_t total = (size_t)rows * c8;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int r = (int)(i / c8), k = (int)(i - (size_t)r * c8) * 8;
    T* cr = comb + (size_t)r * ccs;
    float v[8];
    if (mode == 0) {
      load8<T>(rgb + (size_t)(r % n_rgb) * rcs + k, v);
      store8<T>(cr + k, v);
      load8<T>(depth + (size_t)r * dcs + k, v);
      store8<T>(cr + c + k, v);
    } else {
      load8<T>(cr + c + k, v);
      store8<T>(depth + (size_t)r * dcs + k, v);
      if (rgb && r < n_rgb) {
        float u[8];
        load8<T>(cr + k, v);
        load8<T>(comb + (size_t)(r + n_rgb) * ccs + k, u);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += u[e];
        store8<T>(rgb + (size_t)r * rcs + k, v);
      }
    }
  }
}

// ---- WGAN loss on sigmoid outputs (paper_cgan.py:395-403) -------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cgan_wgan_kernel(const T* __restrict__ z, int rows, int cs, int mode, T* __restrict__ seed,
                                                        float* __restrict__ scal) {
  __shared__ float sh[2][4];
  float sr = 0.f, sf = 0.f;
  const float inv = 1.f / (float)rows;
  for (int i = threadIdx.x; i < rows; i += 256) {
    const float zr = to_f32<T>(z[(size_t)i * cs]), zf = to_f32<T>(z[(size_t)(rows + i) * cs]);
    const float pr = 1.f / (1.f + expf(-zr)), pf = 1.f / (1.f + expf(-zf));
    sr += pr;
    sf += pf;
    if (mode) {
      seed[(size_t)i * cs] = from_f32<T>(mode == 1 ? -pr * (1.f - pr) * inv : 0.f);
      seed[(size_t)(rows + i) * cs] = from_f32<T>(mode == 1 ? pf * (1.f - pf) * inv : -pf * (1.f - pf) * inv);
    }
  }
  sr = wave_sum(sr);
  sf = wave_sum(sf);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = sr; sh[1][threadIdx.x >> 6] = sf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float mr = block_total(sh[0]) * inv, mf = block_total(sh[1]) * inv;
    scal[0] = -mf;
    scal[1] = mf;
    scal[2] = mr;
    scal[3] = mf - mr;
  }
}

// ---- Eigen-2014 metrics (paper_cgan.py:447-478): the terms, the reduction and the values are tdg_cgan_metrics.h's ----
__global__ void __launch_bounds__(256) cgan_metrics_kernel(const float* __restrict__ y, const float* __restrict__ pred,
                                                           const float* __restrict__ offset, int n, int hw,
                                                           MetricPartial* __restrict__ part) {
  __shared__ double shd[5][4];
  __shared__ unsigned long long shh[3][4];
  double s[5] = {0, 0, 0, 0, 0};
  unsigned long long h[3] = {0, 0, 0};
  const size_t total = (size_t)n * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / hw);
    metric_terms(y[i], (pred ? pred[i] : 0.f) + (offset ? offset[b] : 0.f), s, h);
  }
  metric_wave_sums(s, h, shd, shh);
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = metric_block_total(shd, shh);
}

__global__ void cgan_metrics_finish_kernel(const MetricPartial* __restrict__ part, int nblk, unsigned long long total,
                                           unsigned long long* __restrict__ counts, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double v[8];
  metric_values(part, nblk, total, counts, v);
  for (int k = 0; k < 8; ++k) out[k] = (float)v[k];
}

}  // namespace

extern "C" int tdg_cgan_prep(int dtype, const float* y, int n, int version, void* depth_real, int depth_cs, void* depth_fake,
                             float* ybar, float* crop, void* g_ones, int g_cs, void* rgb_ybar, int rgb_cs, void* stream) {
  TDG_CHECK_ARG(y && n > 0 && depth_real && ybar && crop && version >= 0 && version <= 2 &&
                    depth_cs >= (version == 2 ? 2 : 1) && (version != 2 || depth_fake) && (!g_ones || g_cs > 0) &&
                    (!rgb_ybar || rgb_cs > 0),
                "tdg_cgan_prep: bad argument");
  tdg_timing_start("cgan_prep", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(cgan_prep_kernel<T>, dim3(n), dim3(256), 0, (hipStream_t)stream, y, version, static_cast<T*>(depth_real),
                       depth_cs, static_cast<T*>(depth_fake), ybar, crop, static_cast<T*>(g_ones), g_cs, static_cast<T*>(rgb_ybar),
                       rgb_cs);
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_prep");
  return TDG_OK;
}

#define CGAN_TPP_DISPATCH(cin, ...)                       \
  switch ((cin) / 8) {                                    \
    case 8: { constexpr int TPP = 8; __VA_ARGS__ } break;  \
    case 16: { constexpr int TPP = 16; __VA_ARGS__ } break; \
    case 32: { constexpr int TPP = 32; __VA_ARGS__ } break; \
    case 64: { constexpr int TPP = 64; __VA_ARGS__ } break; \
    default: tdg_set_error("tdg_cgan_head: cin %d is not 64, 128, 256 or 512", (cin)); return TDG_EINVAL; \
  }

// What the two dispatches below would reject, rejected with the other argument checks: before the timing window opens, so
// that a refused head call records nothing -- and with cin compared as a whole (cin / 8 let 65 .. 71 pass as 64).
#define CGAN_HEAD_CHECK(what, dtype, cin)                                                                               \
  do {                                                                                                                  \
    TDG_CHECK_ARG((dtype) == TDG_BF16 || (dtype) == TDG_F32, "%s: bad dtype %d", (what), (int)(dtype));                 \
    TDG_CHECK_ARG((cin) == 64 || (cin) == 128 || (cin) == 256 || (cin) == 512, "%s: cin %d is not 64, 128, 256 or 512", \
                  (what), (int)(cin));                                                                                  \
  } while (0)

// both head forwards: u == nullptr is the cin -> 1 head, else the cin + 1 -> 1 head of --noise_layer d4
static int head_fwd(const char* what, int dtype, const void* cat, int n, int hw, int cin, int cs, int crop, const float* w,
                    const float* b, const float* u, const float* ybar, float* yhat, float* g32, void* fake, int fake_cs,
                    hipStream_t stream) {
  CGAN_HEAD_CHECK(what, dtype, cin);
  tdg_timing_start(what, 0.0, stream);
  DISPATCH_T(dtype, {
    CGAN_TPP_DISPATCH(cin, {
      if (u)
        hipLaunchKernelGGL((cgan_head_fwd_kernel<T, TPP, true>), dim3(n), dim3(256), 0, stream, static_cast<const T*>(cat), hw, cs,
                           crop, w, b, u, ybar, yhat, g32, static_cast<T*>(fake), fake_cs);
      else
        hipLaunchKernelGGL((cgan_head_fwd_kernel<T, TPP, false>), dim3(n), dim3(256), 0, stream, static_cast<const T*>(cat), hw, cs,
                           crop, w, b, u, ybar, yhat, g32, static_cast<T*>(fake), fake_cs);
    })
  })
  tdg_timing_stop(stream);
  TDG_HIP_LAUNCH_CHECK(what);
  return TDG_OK;
}

static int head_bwd(const char* what, int dtype, const void* dfake, int fake_cs, const void* cat, int n, int hw, int cin, int cs,
                    int crop, const float* w, const float* u, int mask_mode, float leak, void* dcat, float* dw, float* db,
                    void* workspace, size_t workspace_bytes, hipStream_t stream) {
  CGAN_HEAD_CHECK(what, dtype, cin);
  const int cols = cin + (u ? 2 : 1);
  if (workspace_bytes < (size_t)n * cols * sizeof(float)) {
    tdg_set_error("%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, (size_t)n * cols * sizeof(float));
    return TDG_EWORKSPACE;
  }
  float* part = static_cast<float*>(workspace);
  tdg_timing_start(what, 0.0, stream);
  DISPATCH_T(dtype, {
    CGAN_TPP_DISPATCH(cin, {
      if (u)
        hipLaunchKernelGGL((cgan_head_bwd_kernel<T, TPP, true>), dim3(n), dim3(256), 0, stream, static_cast<const T*>(dfake), fake_cs,
                           static_cast<const T*>(cat), hw, cs, crop, w, u, mask_mode, leak, static_cast<T*>(dcat), part);
      else
        hipLaunchKernelGGL((cgan_head_bwd_kernel<T, TPP, false>), dim3(n), dim3(256), 0, stream, static_cast<const T*>(dfake), fake_cs,
                           static_cast<const T*>(cat), hw, cs, crop, w, u, mask_mode, leak, static_cast<T*>(dcat), part);
    })
  })
  hipLaunchKernelGGL(cgan_head_finish_kernel, dim3(tdg_ceil_div(cols, 256)), dim3(256), 0, stream, part, n, cols, dw, db);
  tdg_timing_stop(stream);
  TDG_HIP_LAUNCH_CHECK(what);
  return TDG_OK;
}

extern "C" int tdg_cgan_head_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, int crop, const float* w,
                                 const float* b, const float* ybar, float* yhat, void* fake, int fake_cs, void* stream) {
  TDG_CHECK_ARG(cat && w && b && yhat && fake && n > 0 && crop > 0 && crop <= hw && cs >= cin && cs % 8 == 0 && fake_cs > 0,
                "tdg_cgan_head_fwd: bad argument");
  return head_fwd("cgan_head_fwd", dtype, cat, n, hw, cin, cs, crop, w, b, nullptr, ybar, yhat, nullptr, fake, fake_cs,
                  (hipStream_t)stream);
}

extern "C" int tdg_cgan_head_noise_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, int crop, const float* w,
                                       const float* b, const float* u, const float* ybar, float* yhat, float* g, void* fake,
                                       int fake_cs, void* stream) {
  TDG_CHECK_ARG(cat && w && b && yhat && fake && n > 0 && crop > 0 && crop <= hw && cs >= cin && cs % 8 == 0 && fake_cs > 0,
                "tdg_cgan_head_noise_fwd: bad argument");
  return head_fwd("cgan_head_noise_fwd", dtype, cat, n, hw, cin, cs, crop, w, b, u, ybar, yhat, g, fake, fake_cs,
                  (hipStream_t)stream);
}

extern "C" int tdg_cgan_head_bwd(int dtype, const void* dfake, int fake_cs, const void* cat, int n, int hw, int cin, int cs, int crop,
                                 const float* w, int mask_mode, float leak, void* dcat, float* dw, float* db, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(dfake && cat && w && dcat && dw && db && workspace && n > 0 && crop > 0 && crop <= hw && cs >= cin && cs % 8 == 0 &&
                    fake_cs > 0,
                "tdg_cgan_head_bwd: bad argument");
  return head_bwd("cgan_head_bwd", dtype, dfake, fake_cs, cat, n, hw, cin, cs, crop, w, nullptr, mask_mode, leak, dcat, dw, db,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int tdg_cgan_head_noise_bwd(int dtype, const void* dfake, int fake_cs, const void* cat, int n, int hw, int cin, int cs,
                                       int crop, const float* w, const float* u, int mask_mode, float leak, void* dcat, float* dw,
                                       float* db, void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(dfake && cat && w && dcat && dw && db && workspace && n > 0 && crop > 0 && crop <= hw && cs >= cin && cs % 8 == 0 &&
                    fake_cs > 0,
                "tdg_cgan_head_noise_bwd: bad argument");
  return head_bwd("cgan_head_noise_bwd", dtype, dfake, fake_cs, cat, n, hw, cin, cs, crop, w, u, mask_mode, leak, dcat, dw, db,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int tdg_cgan_join(int dtype, int mode, int n_rgb, int rows, int c, void* comb, int comb_cs, void* rgb, int rgb_cs, void* depth,
                             int depth_cs, void* stream) {
  TDG_CHECK_ARG(comb && depth && (mode == 1 || rgb) && (mode == 0 || mode == 1) && n_rgb > 0 && rows > 0 && c > 0 && c % 8 == 0 &&
                    comb_cs >= 2 * c && comb_cs % 8 == 0 && (!rgb || (rgb_cs >= c && rgb_cs % 8 == 0)) && depth_cs >= c &&
                    depth_cs % 8 == 0 && (mode == 0 || !rgb || rows >= 2 * n_rgb),
                "tdg_cgan_join: bad argument");
  tdg_timing_start("cgan_join", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(cgan_join_kernel<T>, dim3(grid_for((size_t)rows * (c / 8))), dim3(256), 0, (hipStream_t)stream, mode, n_rgb,
                       rows, c, static_cast<T*>(comb), comb_cs, static_cast<T*>(rgb), rgb_cs, static_cast<T*>(depth), depth_cs);
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_join");
  return TDG_OK;
}

extern "C" int tdg_cgan_wgan_loss(int dtype, const void* logits, int rows, int cs, int mode, void* seed, float* scal, void* stream) {
  TDG_CHECK_ARG(logits && scal && rows > 0 && cs > 0 && mode >= 0 && mode <= 2 && (mode == 0 || seed), "tdg_cgan_wgan_loss: bad argument");
  tdg_timing_start("cgan_wgan_loss", 0.0, (hipStream_t)stream);
  DISPATCH_T(dtype, {
    hipLaunchKernelGGL(cgan_wgan_kernel<T>, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<const T*>(logits), rows, cs, mode,
                       static_cast<T*>(seed), scal);
  })
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_wgan_loss");
  return TDG_OK;
}

extern "C" size_t tdg_cgan_metrics_workspace_bytes(void) { return kMetricBlocks * sizeof(MetricPartial); }

extern "C" int tdg_cgan_metrics(const float* y, const float* pred, const float* offset, int n, int hw, unsigned long long* counts,
                                float* out, void* workspace, size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(y && counts && out && workspace && n > 0 && hw > 0, "tdg_cgan_metrics: bad argument");
  if (workspace_bytes < kMetricBlocks * sizeof(MetricPartial)) {
    tdg_set_error("tdg_cgan_metrics: workspace too small");
    return TDG_EWORKSPACE;
  }
  const size_t total = (size_t)n * hw;
  const int nblk = metric_blocks(total);
  MetricPartial* part = static_cast<MetricPartial*>(workspace);
  tdg_timing_start("cgan_metrics", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(cgan_metrics_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, y, pred, offset, n, hw, part);
  hipLaunchKernelGGL(cgan_metrics_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, nblk, (unsigned long long)total,
                     counts, out);
  tdg_timing_stop((hipStream_t)stream);
  TDG_HIP_LAUNCH_CHECK("cgan_metrics");
  return TDG_OK;
}
