// Tensor summaries for the training event files: what hem.summarize_layers / summarize_gradients /
// summarize_weights_biases (hem/ops/summaries.py:31-75) ask TensorFlow for per tensor -- tf.summary.histogram,
// tf.nn.zero_fraction and tf.reduce_mean -- for a whole table of tensors (jobs) in one batched entry.
//
// Buckets: TensorFlow's default histogram (tensorflow/core/lib/histogram/histogram.cc, InitDefaultBucketsInner), restated:
// positive limits v = 1e-12, v *= 1.1 while v < 1e20 (774 values, repeated f64 multiplication); the table is
// [-DBL_MAX, -pos reversed, 0, pos, DBL_MAX] (1551 limits) and an element goes to bucket b = the number of limits <= (double)v.
// tdg_tensor_summary_limits builds the table on the host; the kernel only ever compares against the caller's copy of it: a
// log2 guess of the bucket (v_log_f32, approximate) is corrected with the table until limits[b-1] <= v < limits[b] holds, so
// the answer is the table's upper_bound whatever the guess was.
//
// Scheme.  A job's live elements (rows x c, row stride cs) are cut into chunks of kChunkBytes bytes' worth (1024 f32, 2048 bf16:
// one 16-byte group per thread); the chunks of all jobs form one list that the blocks of ONE launch walk grid-stride, each
// finding its chunk's job by walking the job table (chunk indices of a block only grow).  Per chunk: thread t takes the
// elements t VW, t VW + 256 VW, ... (VW = 16 bytes' worth where the base, c and cs allow it -- a contiguous tensor takes whole
// 16-byte groups plus a scalar tail -- else 1), accumulates sum and sum of squares in f64, min / max, the zero and non-finite
// counts; then wave shuffle, then the four waves through LDS in wave order; the chunk's partial goes to the workspace.  A
// second launch (one block per job) adds a job's partials the same way: thread t the chunks t, t + 256, ..., then wave, then
// block.  No float atomics, a fixed order everywhere: two launches on the same input are bit-equal.
// Histogram: a per-block u32 histogram in LDS, flushed into the job's u64 buckets with integer atomics when the block's
// next chunk belongs to another job (and at the end): a large job costs each block one flush, not one per chunk.
// A relu layer sends half its elements to bucket 776 and an all-equal tensor everything to one bucket, so lanes first agree
// within the wave: the zero bucket, then up to kPeels times the first waiting lane's bucket (while those groups are not
// tiny), take ONE add of the matching lanes' count; what is left after that is spread and adds itself.  Reads: only the c live elements of each row, nothing
// behind the last live element of the last row.
//
// The job table lives in device memory (the caller builds it once per replica), but a bad job must be a status and not a
// fault, and the grid and the workspace depend on the jobs' sizes: the entry reads the table back (njobs x 32 bytes, one
// stream-ordered copy and one stream synchronisation).  It is the one entry of the library that synchronises; it runs
// eagerly between training steps, right before its caller reads the results, and never inside a captured body.
#include <float.h>

#include <vector>

#include "tdg_cgan_common.h"

namespace {

constexpr int kLimits = 1551, kPos = 774, kZeroBucket = 776;
constexpr int kChunkBytes = 4096;          // live elements per chunk, in bytes: one 16-byte group per thread
constexpr int kThreads = 256, kMaxBlocks = 2048;     // 8 blocks of 18.3 KB LDS per CU
constexpr int kFlushChunks = 1 << 20;      // chunks a block may gather in its u32 histogram: 2^20 * 2048 elements < 2^32
constexpr int kPeels = 3, kSmallGroup = 4;
constexpr unsigned long long kMaxElems = 1ull << 48;       // rows * cs of one job: far beyond any HBM, far below 2^64

struct Result {
  uint64_t num, zeros, nonfinite;
  float mn, mx;
  double sum, sum_squares;
  uint64_t bucket[kLimits];
};
static_assert(sizeof(Result) == 48 + 8 * kLimits, "TensorSummaries (kernels.py) parses this layout");

struct Partial {                           // one chunk
  double sum, sumsq;
  float mn, mx;
  uint32_t zeros, nonfinite;
};
static_assert(sizeof(Partial) == 32 && sizeof(TdgSummaryJob) == 32, "layout");

struct Acc {
  double s = 0.0, q = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  uint32_t zeros = 0, nonfinite = 0;
};

__host__ __device__ inline unsigned long long job_elems(const TdgSummaryJob& j) { return (unsigned long long)j.rows * (unsigned long long)j.c; }
__host__ __device__ inline int job_chunk(const TdgSummaryJob& j) { return kChunkBytes / (j.dtype == TDG_BF16 ? 2 : 4); }      // elements
__host__ __device__ inline long long job_chunks(const TdgSummaryJob& j) {
  const unsigned long long ch = (unsigned long long)job_chunk(j);
  return (long long)((job_elems(j) + ch - 1) / ch);
}

// upper_bound of a finite v in the table: the number of limits <= v, in [1, 1550]
__device__ __forceinline__ int bucket_of(float v, const double* lim) {
  if (v == 0.f) return kZeroBucket;
  // |v| ~ 1e-12 * 1.1^k:  k = (log2|v| + log2(1e12)) / log2(1.1); a denormal's log may come out as -inf: clamped
  const float kf = fminf(fmaxf((__log2f(fabsf(v)) + 39.863137f) * 7.2725409f, -1.f), (float)(kPos - 1));
  const int k1 = (int)floorf(kf) + 1;                              // ~ how many positive limits are <= |v|: 0 .. 774
  int b = v > 0.f ? kZeroBucket + k1 : kZeroBucket - 1 - k1;
  const double d = (double)v, lo = lim[b - 1], hi = lim[b];        // (two independent LDS loads; the guess is mostly right)
  if (hi <= d && b < kLimits - 1) {                                // (b stays in [0, 1550] whatever table the caller handed in)
    do ++b; while (b < kLimits - 1 && lim[b] <= d);
  } else if (lo > d) {
    do --b; while (b > 1 && lim[b - 1] > d);
  }
  return b;
}

// hist[b] += 1 for every active lane, with one add per group of lanes that agree (see the head of the file).  Every lane of
// the wave calls this together.
__device__ __forceinline__ void hist_add(uint32_t* hist, int b, bool active) {
  unsigned long long todo = __ballot(active);
  if (!todo) return;
  const int lane = threadIdx.x & 63;
  unsigned long long same = __ballot(active && b == kZeroBucket);
  if (same) {
    if (lane == __ffsll((long long)same) - 1) atomicAdd(&hist[kZeroBucket], (uint32_t)__popcll(same));
    todo &= ~same;
  }
  for (int p = 0; p < kPeels && todo; ++p) {
    const int lead = __ffsll((long long)todo) - 1;
    const int lb = __builtin_amdgcn_readlane(b, lead);
    same = __ballot(active && b == lb);                            // (all of them still wait: an earlier leader would have taken them)
    if (lane == lead) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
    todo &= ~same;
    if (__popcll(same) < kSmallGroup) break;                       // the waiting lanes look spread: no more leaders
  }
  if ((todo >> lane) & 1) atomicAdd(&hist[b], 1u);
}

__device__ __forceinline__ void take(float x, bool ok, float scale, const double* lim, uint32_t* hist, Acc& a) {
  const float v = x * scale;
  const bool fin = ok && fabsf(v) <= FLT_MAX;                      // false for NaN and +-Inf
  int b = 0;
  if (ok && !fin) ++a.nonfinite;
  if (fin) {
    const double d = (double)v;
    a.s += d;
    a.q += d * d;
    a.mn = fminf(a.mn, v);
    a.mx = fmaxf(a.mx, v);
    if (v == 0.f) ++a.zeros;
    b = bucket_of(v, lim);
  }
  hist_add(hist, b, fin);
}

// live elements [i0, i1) of the chunk that starts at live element e0 of the job (VW > 1: i0, i1, e0, c and cs are multiples of VW
// and every group is 16-byte aligned)
template <typename T, int VW>
__device__ __forceinline__ void scan(const TdgSummaryJob& job, unsigned long long e0, int i0, int i1, const double* lim, uint32_t* hist,
                                     Acc& a) {
  const T* __restrict__ p = static_cast<const T*>(job.ptr);
  const bool flat = job.cs == job.c;
  const uint32_t c = (uint32_t)job.c;
  const unsigned long long row0 = flat ? 0 : e0 / c;
  const uint32_t col0 = flat ? 0 : (uint32_t)(e0 - row0 * c);
  for (int base = i0; base < i1; base += kThreads * VW) {          // (the same trip count in every lane: hist_add is wave-wide)
    const int i = base + (int)threadIdx.x * VW;
    const bool ok = i < i1;
    size_t addr = 0;
    if (ok) {
      if (flat) {
        addr = (size_t)(e0 + (unsigned long long)i);
      } else {
        const uint32_t t = col0 + (uint32_t)i, r = t / c;
        addr = (size_t)((row0 + r) * (unsigned long long)job.cs + (t - r * c));
      }
    }
    if constexpr (VW == 1) {
      take(ok ? to_f32<T>(p[addr]) : 0.f, ok, job.scale, lim, hist, a);
    } else if constexpr (std::is_same_v<T, float>) {
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (ok) x = *reinterpret_cast<const f32x4*>(p + addr);
#pragma unroll
      for (int k = 0; k < 4; ++k) take(x[k], ok, job.scale, lim, hist, a);
    } else {
      bf16x8 x = {};
      if (ok) x = *reinterpret_cast<const bf16x8*>(p + addr);
#pragma unroll
      for (int k = 0; k < 8; ++k) take((float)x[k], ok, job.scale, lim, hist, a);
    }
  }
}

template <typename T>
__device__ __forceinline__ void scan_chunk(const TdgSummaryJob& job, unsigned long long e0, int n, const double* lim, uint32_t* hist, Acc& a) {
  constexpr int VW = 16 / (int)sizeof(T);
  const bool flat = job.cs == job.c;
  const bool wide = ((uintptr_t)job.ptr & 15) == 0 && (flat || (job.c % VW == 0 && job.cs % VW == 0));
  const int nw = wide ? (flat ? n - n % VW : n) : 0;               // (a chunk starts at a multiple of the chunk size, so of VW)
  if (nw > 0) scan<T, VW>(job, e0, 0, nw, lim, hist, a);
  if (nw < n) scan<T, 1>(job, e0, nw, n, lim, hist, a);
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

__global__ void __launch_bounds__(kThreads) summary_kernel(const TdgSummaryJob* __restrict__ jobs, int njobs, const double* __restrict__ limits,
                                                           Result* __restrict__ res, Partial* __restrict__ part, long long total_chunks) {
  __shared__ double lim[kLimits];
  __shared__ uint32_t hist[kLimits];
  __shared__ double sh_s[4], sh_q[4];
  __shared__ float sh_mn[4], sh_mx[4];
  __shared__ uint32_t sh_z[4], sh_nf[4];
  for (int i = threadIdx.x; i < kLimits; i += kThreads) {
    lim[i] = limits[i];
    hist[i] = 0;
  }
  __syncthreads();
  int j = 0, held = -1, gathered = 0;                              // held: the job whose counts hist holds (-1: it is empty)
  long long base = 0;
  TdgSummaryJob job = jobs[0];
  long long nch = job_chunks(job);
  auto flush = [&]() {                                             // (behind a barrier: every wave's adds are in)
    for (int i = threadIdx.x; i < kLimits; i += kThreads) {
      const uint32_t cnt = hist[i];
      if (cnt) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&res[held].bucket[i]), (unsigned long long)cnt);
        hist[i] = 0;
      }
    }
    held = -1, gathered = 0;
    __syncthreads();
  };
  for (long long v = blockIdx.x; v < total_chunks; v += gridDim.x) {
    while (v >= base + nch && j + 1 < njobs) {
      base += nch;
      job = jobs[++j];
      nch = job_chunks(job);
    }
    if (v >= base + nch) break;                                    // (cannot happen: total_chunks is the table's own total)
    if (held >= 0 && (held != j || gathered >= kFlushChunks)) flush();
    held = j, ++gathered;
    const int chunk = job_chunk(job);
    const unsigned long long e0 = (unsigned long long)(v - base) * (unsigned long long)chunk, left = job_elems(job) - e0;
    const int n = left < (unsigned long long)chunk ? (int)left : chunk;
    Acc a;
    if (job.dtype == TDG_BF16) scan_chunk<bf16_t>(job, e0, n, lim, hist, a);
    else scan_chunk<float>(job, e0, n, lim, hist, a);
    const double s = wave_sum(a.s), q = wave_sum(a.q);
    const float mn = wave_min(a.mn), mx = wave_max(a.mx);
    const uint32_t z = wave_sum(a.zeros), nf = wave_sum(a.nonfinite);
    if ((threadIdx.x & 63) == 0) {
      const int w = threadIdx.x >> 6;
      sh_s[w] = s, sh_q[w] = q, sh_mn[w] = mn, sh_mx[w] = mx, sh_z[w] = z, sh_nf[w] = nf;
    }
    __syncthreads();                                               // the wave results, and every wave's adds into hist
    if (threadIdx.x == 0) {
      Partial p;
      p.sum = block_total(sh_s);
      p.sumsq = block_total(sh_q);
      p.mn = fminf(fminf(sh_mn[0], sh_mn[1]), fminf(sh_mn[2], sh_mn[3]));
      p.mx = fmaxf(fmaxf(sh_mx[0], sh_mx[1]), fmaxf(sh_mx[2], sh_mx[3]));
      p.zeros = block_total(sh_z);
      p.nonfinite = block_total(sh_nf);
      part[v] = p;
    }
    __syncthreads();                                               // (sh_* are written again by the next chunk)
  }
  if (held >= 0) flush();
}

// one block per job: thread t adds the partials of the job's chunks t, t + 256, ... in that order, then wave shuffle, then the
// four waves in wave order (the loads of a large job's partials run in parallel; a fixed order all the same)
__global__ void __launch_bounds__(kThreads) summary_finish_kernel(const TdgSummaryJob* __restrict__ jobs, const Partial* __restrict__ part,
                                                                  Result* __restrict__ res) {
  __shared__ long long sh_before[4];
  __shared__ double sh_s[4], sh_q[4];
  __shared__ float sh_mn[4], sh_mx[4];
  __shared__ unsigned long long sh_z[4], sh_nf[4];
  const int j = blockIdx.x, w = threadIdx.x >> 6;
  long long before = 0;
  for (int i = threadIdx.x; i < j; i += kThreads) before += job_chunks(jobs[i]);
  before = wave_sum(before);
  if ((threadIdx.x & 63) == 0) sh_before[w] = before;
  __syncthreads();
  before = block_total(sh_before);
  const TdgSummaryJob job = jobs[j];
  const long long nch = job_chunks(job);
  double s = 0.0, q = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  unsigned long long z = 0, nf = 0;
  for (long long k = threadIdx.x; k < nch; k += kThreads) {
    const Partial p = part[before + k];
    s += p.sum;
    q += p.sumsq;
    mn = fminf(mn, p.mn);
    mx = fmaxf(mx, p.mx);
    z += p.zeros;
    nf += p.nonfinite;
  }
  s = wave_sum(s), q = wave_sum(q), mn = wave_min(mn), mx = wave_max(mx), z = wave_sum(z), nf = wave_sum(nf);
  if ((threadIdx.x & 63) == 0) sh_s[w] = s, sh_q[w] = q, sh_mn[w] = mn, sh_mx[w] = mx, sh_z[w] = z, sh_nf[w] = nf;
  __syncthreads();
  if (threadIdx.x != 0) return;
  Result* r = res + j;
  r->num = job_elems(job);
  r->zeros = block_total(sh_z);
  r->nonfinite = block_total(sh_nf);
  const bool any = r->nonfinite < r->num;                          // a finite element
  r->mn = any ? fminf(fminf(sh_mn[0], sh_mn[1]), fminf(sh_mn[2], sh_mn[3])) : 0.f;
  r->mx = any ? fmaxf(fmaxf(sh_mx[0], sh_mx[1]), fmaxf(sh_mx[2], sh_mx[3])) : 0.f;
  r->sum = block_total(sh_s);
  r->sum_squares = block_total(sh_q);
}

}  // namespace

extern "C" int tdg_tensor_summary_limits(double* out) {
  TDG_CHECK_ARG(out, "tdg_tensor_summary_limits: null output");
  double pos[kPos + 1];
  int n = 0;
  for (double v = 1.0e-12; v < 1.0e20; v *= 1.1) {
    if (n == kPos) {
      tdg_set_error("tdg_tensor_summary_limits: more than %d positive limits", kPos);
      return TDG_EINVAL;
    }
    pos[n++] = v;
  }
  if (n != kPos) {
    tdg_set_error("tdg_tensor_summary_limits: %d positive limits, %d expected", n, kPos);
    return TDG_EINVAL;
  }
  out[0] = -DBL_MAX;
  for (int i = 0; i < kPos; ++i) out[1 + i] = -pos[kPos - 1 - i];
  out[1 + kPos] = 0.0;
  for (int i = 0; i < kPos; ++i) out[kZeroBucket + i] = pos[i];
  out[kLimits - 1] = DBL_MAX;
  return TDG_OK;
}

extern "C" size_t tdg_tensor_summary_result_bytes() { return sizeof(Result); }

extern "C" size_t tdg_tensor_summary_workspace_bytes(int njobs, uint64_t total_elems) {
  // sum_j ceil(e_j / chunk_j) chunks at most, whatever the dtypes: an f32 chunk is the smaller one
  return njobs > 0 ? ((size_t)njobs + (size_t)(total_elems / (kChunkBytes / 4))) * sizeof(Partial) : 0;
}

extern "C" int tdg_tensor_summary(const TdgSummaryJob* jobs_dev, int njobs, const double* limits_dev, void* results_dev, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  TDG_CHECK_ARG(jobs_dev && limits_dev && results_dev && workspace && njobs > 0,
                "tdg_tensor_summary: bad argument (jobs %p, njobs %d, limits %p, results %p, workspace %p)", (const void*)jobs_dev, njobs,
                (const void*)limits_dev, results_dev, workspace);
  TDG_CHECK_ARG(((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)limits_dev & 7) == 0 && ((uintptr_t)results_dev & 7) == 0 &&
                    ((uintptr_t)workspace & 7) == 0,
                "tdg_tensor_summary: misaligned job table, limits, results or workspace");
  hipStream_t s = (hipStream_t)stream;
  std::vector<TdgSummaryJob> jobs((size_t)njobs);
  hipError_t e = hipMemcpyAsync(jobs.data(), jobs_dev, (size_t)njobs * sizeof(TdgSummaryJob), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    tdg_set_error("tdg_tensor_summary: reading the job table back failed: %s (it does not run inside a captured body)", hipGetErrorString(e));
    return TDG_EHIP;
  }
  long long total_chunks = 0;
  for (int j = 0; j < njobs; ++j) {
    const TdgSummaryJob& b = jobs[(size_t)j];
    TDG_CHECK_ARG(b.dtype == TDG_F32 || b.dtype == TDG_BF16, "tdg_tensor_summary: job %d: bad dtype %d", j, b.dtype);
    TDG_CHECK_ARG(b.ptr && b.rows >= 1 && b.c >= 1 && b.cs >= b.c && b.rows <= kMaxElems / (unsigned long long)b.cs,
                  "tdg_tensor_summary: job %d: bad tensor (ptr %p, rows %llu, c %d, cs %d)", j, b.ptr, (unsigned long long)b.rows, b.c, b.cs);
    TDG_CHECK_ARG(((uintptr_t)b.ptr & (uintptr_t)(tdg_dtype_size(b.dtype) - 1)) == 0, "tdg_tensor_summary: job %d: misaligned tensor", j);
    total_chunks += job_chunks(b);
  }
  const size_t need = (size_t)total_chunks * sizeof(Partial);
  if (workspace_bytes < need) {
    tdg_set_error("tdg_tensor_summary: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return TDG_EWORKSPACE;
  }
  const int nblk = (int)(total_chunks < kMaxBlocks ? total_chunks : kMaxBlocks);
  Result* res = static_cast<Result*>(results_dev);
  tdg_timing_start("tensor_summary", 0.0, s);
  e = hipMemsetAsync(res, 0, (size_t)njobs * sizeof(Result), s);    // the buckets are added into
  if (e == hipSuccess) {
    hipLaunchKernelGGL(summary_kernel, dim3(nblk), dim3(kThreads), 0, s, jobs_dev, njobs, limits_dev, res, static_cast<Partial*>(workspace),
                       total_chunks);
    hipLaunchKernelGGL(summary_finish_kernel, dim3(njobs), dim3(kThreads), 0, s, jobs_dev, static_cast<const Partial*>(workspace), res);
  }
  tdg_timing_stop(s);
  if (e != hipSuccess) {
    tdg_set_error("tdg_tensor_summary: clearing the results failed: %s", hipGetErrorString(e));
    return TDG_EHIP;
  }
  TDG_HIP_LAUNCH_CHECK("tensor_summary");
  return TDG_OK;
}
