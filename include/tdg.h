/* tdg.h -- C ABI of lib3dgan_hip.so: the MI355X (gfx950) kernels behind the
 * 3dgan training hot path (models/gan.py + ops/layers.py of algoterranean/3dgan).
 *
 * The reference has no native boundary: every op below is a TensorFlow-1.x op that the
 * reference's Python graph builders instantiate, and `sess.run` executes inside the TF C++
 * runtime.  Each entry point cites the reference call site (file:line under /root/reference)
 * whose TF op (forward and/or the autodiff ops TF derives from it) it replaces.
 *
 * Conventions
 *  - Plain C: pointers are device pointers (HBM) owned by the caller; the library allocates
 *    nothing persistent and never synchronises.  All work is enqueued on `stream`
 *    (a hipStream_t passed as void*).
 *  - Every function returns 0 on success, a negative TDG_E* code otherwise, and never
 *    throws; `tdg_last_error()` returns a thread-local message.
 *  - Activations are NHWC with an explicit channel stride `cs` (elements) >= channels;
 *    padding channels must hold zeros.  dtype selects the storage/compute type of
 *    activations and packed filters: TDG_F32 (exact f32 MFMA, parity path) or TDG_BF16
 *    (bf16 MFMA, f32 accumulate).  Master weights, gradients, optimizer state, biases,
 *    BN parameters and all reductions are always f32.
 */
#ifndef TDG_H_
#define TDG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDG_OK 0
#define TDG_EINVAL (-1)      /* invalid descriptor / argument            */
#define TDG_EUNSUPPORTED (-2)/* valid but not implemented for this shape */
#define TDG_EHIP (-3)        /* a HIP runtime call failed                */
#define TDG_EWORKSPACE (-4)  /* workspace too small                      */

#define TDG_F32 0
#define TDG_BF16 1

/* activations (fused epilogues / elementwise) */
#define TDG_ACT_NONE 0
#define TDG_ACT_RELU 1    /* models/gan.py:245 tf.nn.relu     */
#define TDG_ACT_LRELU 2   /* ops/activations.py:28 max(leak*x, x) */
#define TDG_ACT_TANH 3    /* models/gan.py:252 tf.tanh        */
#define TDG_ACT_SIGMOID 4 /* models/gan.py:275 tf.nn.sigmoid  */

/* mask applied by an epilogue: out *= act'(mask_src) evaluated from the POST-activation
 * (lrelu) or PRE-activation (relu after BN) tensor stored at the same offsets as `out`. */
#define TDG_MASK_NONE 0
#define TDG_MASK_LRELU 1  /* slope 1 where mask_src > 0 else leak (TF MaximumGrad, App. A-6) */
#define TDG_MASK_RELU 2   /* 1 where mask_src > 0 else 0 */

/* One strided 2-D convolution with TF 'SAME'/'VALID' geometry between a "big" tensor
 * x [n, h, w, c] (conv input / conv2d_transpose output) and a "small" tensor
 * y [n, oh, ow, k] (conv output / conv2d_transpose input), filter master layout
 * [kh, kw, c, k] f32 (HWIO for conv2d, ops/layers.py:96; [k,k,Cout,Cin] for deconv2d,
 * ops/layers.py:135 -- same memory order with c = deconv Cout, k = deconv Cin). */
typedef struct TdgConvDesc {
  int32_t n, h, w, c, cs;   /* big side: dims, channels, channel stride   */
  int32_t oh, ow, k, ks;    /* small side                                  */
  int32_t kh, kw, stride;
  int32_t pad_t, pad_l;     /* TF pad_before             */
  int32_t dtype;            /* TDG_F32 | TDG_BF16                          */
} TdgConvDesc;

/* Fused epilogue of the two conv GEMM forms. */
typedef struct TdgEpilogue {
  const float* bias;        /* per output channel, may be NULL (tf.nn.bias_add, ops/layers.py:102,143) */
  int32_t act;              /* TDG_ACT_*                                     */
  float leak;               /* lrelu leak                                    */
  int32_t mask_mode;        /* TDG_MASK_*                                    */
  const void* mask_src;     /* tensor with the geometry of the output, dtype = desc.dtype */
  int32_t accumulate;       /* 1: out = (act(acc + bias) + out) * mask  -- sums a second gradient path (U-Net skips) */
  /* Column partials of the STORED tile, emitted by the epilogue that holds it anyway (instead of a separate pass over
   * the tensor): per workgroup row tile b,  col_partial[(b*2 + 0)*N + n] = sum over its rows,  [(b*2 + 1)*N + n] = the
   * second moment (TDG_COL_BN).  TDG_COL_SUM: sum of the stored values (after activation and mask) = the bias gradient
   * of the layer that owns the tensor (autodiff of tf.nn.bias_add, ops/layers.py:102).  TDG_COL_BN: sum (v - bias[n]) and
   * sum (v - bias[n])^2 of the stored pre-activation = the batch statistics of tf.contrib.layers.batch_norm
   * (ops/layers.py:103,144).  Only rows of images < col_images count (0: all).  The launch reports how many row
   * tiles it wrote in *col_nblk_out (host memory, written before the call returns); 0 = this launch's kernel
   * variant does not provide partials (f32 tiles, accumulating epilogues, thin layers -- the thin-input, one-output-channel
   * and register-staged kernels --, and launches cut along K, whose tiles are not the stored tile): run the separate pass.
   * Finish with tdg_col_finalize_sum / tdg_bn_fwd_from_partials. */
  float* col_partial;
  size_t col_partial_bytes;
  int32_t col_mode;         /* TDG_COL_*                                     */
  int32_t col_images;
  int32_t* col_nblk_out;
  /* Optional scratch for split-K (caller-owned, like every buffer): a forward-type GEMM whose grid would leave most CUs
   * idle (few output rows, long K: pix2pix's 1x1 ... 8x8 bottleneck layers) is cut along K into f32 partial tiles here
   * and finished by a second kernel in a fixed order.  NULL: never split. */
  void* splitk_ws;
  size_t splitk_ws_bytes;
} TdgEpilogue;
enum { TDG_COL_NONE = 0, TDG_COL_SUM = 1, TDG_COL_BN = 2 };

const char* tdg_last_error(void);
int tdg_version(void);
/* Name of the GEMM kernel variant chosen by this thread's most recent tdg_conv2d_* call (profiling aid:
 * lets a caller attribute HIP-event timings to the kernel symbols rocprofv3 reports). */
const char* tdg_last_kernel(void);

/* Diagnostics (bench.py's roofline leg): between tdg_timing_begin() and tdg_timing_end() every conv GEMM kernel
 * launch is bracketed by HIP events on its own stream; tdg_timing_end() waits for them and returns one record per
 * launch: the kernel (as rocprofv3 names it, template arguments included), its duration and the algorithmic FLOPs
 * of the columns/rows it covered.  `count` receives the number of launches even when it exceeds `capacity`.
 * Not for use during stream capture. */
typedef struct TdgLaunchRecord {
  char kernel[64];
  double ms;
  double flops;
} TdgLaunchRecord;
int tdg_timing_begin(void);
int tdg_timing_end(TdgLaunchRecord* out, int capacity, int* count);

/* ---- filter packing: f32 master -> GEMM operand layout in desc.dtype ------------------
 * FWD form  : rows = k (small-side channels), K = (tap, c)        -> used by tdg_conv2d_fwd
 * BWD form  : per output-parity class, rows = c, K = (tap', k)    -> used by tdg_conv2d_bwd_data
 * Sizes in bytes via the *_bytes queries. */
size_t tdg_packed_filter_fwd_bytes(const TdgConvDesc* d);
size_t tdg_packed_filter_bwd_bytes(const TdgConvDesc* d);
int tdg_pack_filter_fwd(const TdgConvDesc* d, const float* w, void* packed, void* stream);
int tdg_pack_filter_bwd(const TdgConvDesc* d, const float* w, void* packed, void* stream);

/* Every filter of a network in one call (after an optimizer step the reference's variables change all at
 * once: tf.train.Optimizer.apply_gradients, models/gan.py:80-81): same results as calling the two functions
 * above per job, in as few launches as the jobs fit.  All jobs must share one dtype.  A null destination
 * skips that form. */
typedef struct TdgPackJob {
  TdgConvDesc desc;
  const float* w;          /* f32 master filter [kh][kw][c][k] */
  void* packed_fwd;
  void* packed_bwd;
} TdgPackJob;
int tdg_pack_filters(const TdgPackJob* jobs, int n_jobs, void* stream);

/* ---- conv GEMMs -------------------------------------------------------------------------
 * tdg_conv2d_fwd      : y = epi(conv2d(x, W))            tf.nn.conv2d, ops/layers.py:101;
 *                       also d(conv2d_transpose)/d(input) (autodiff of ops/layers.py:142)
 *                       and the tangent pass of the gradient penalty (models/gan.py:228)
 * tdg_conv2d_bwd_data : x = epi(conv2d_backprop_input(W, y))   autodiff of ops/layers.py:101;
 *                       also IS tf.nn.conv2d_transpose, ops/layers.py:142
 * tdg_conv2d_bwd_filter: dW (+)= conv2d_backprop_filter(x, y)  autodiff of ops/layers.py:101,142
 *                       dw = beta*dw + sum over rows; deterministic two-stage reduction.
 * `n_images` lets a call cover a leading sub-batch of the buffers (desc.n is the capacity
 * used for bounds only).  */
int tdg_conv2d_fwd(const TdgConvDesc* d, int n_images, const void* x, const void* w_packed_fwd,
                   void* y, const TdgEpilogue* epi, void* stream);
int tdg_conv2d_bwd_data(const TdgConvDesc* d, int n_images, const void* y, const void* w_packed_bwd,
                        void* x, const TdgEpilogue* epi, void* stream);
size_t tdg_conv2d_bwd_filter_workspace_bytes(const TdgConvDesc* d, int n_images);
int tdg_conv2d_bwd_filter(const TdgConvDesc* d, int n_images, const void* x, const void* y,
                          float* dw, float beta, void* workspace, size_t workspace_bytes, void* stream);
/* The same sum with the big-side rows coming from TWO tensors: images [0, n_first) from x, images [n_first, n_images)
 * from x2 (its image 0 first); y holds all n_images.  One launch instead of two plus one slab reduction less: the
 * critic's filter gradient of the iwgan D step = first-order rows (layer inputs of D(x), D(g)) + tangent-pass rows
 * (tangents of the penalty's double backward, models/gan.py:228) against one delta tensor. */
int tdg_conv2d_bwd_filter2(const TdgConvDesc* d, int n_images, const void* x, int n_first, const void* x2, const void* y,
                           float* dw, float beta, void* workspace, size_t workspace_bytes, void* stream);
/* Host-only query: the kernel variant a conv launch would take.  Runs the validation, plan and choice of the entry point
 * that `form` names and writes into `name` what tdg_last_kernel() would return after that call; nothing is enqueued.
 * Of `epi` only the scalar fields, the sizes and whether each pointer is NULL are read.  n_first: TDG_FORM_BWD_FILTER only --
 * 0 asks about tdg_conv2d_bwd_filter, anything else about tdg_conv2d_bwd_filter2 with that n_first.  Returns the status
 * the call's argument checks would return, assuming non-NULL, 16-byte aligned buffers and a large enough workspace. */
enum { TDG_FORM_FWD = 0, TDG_FORM_BWD_DATA = 1, TDG_FORM_BWD_FILTER = 2 };
int tdg_conv2d_dispatch(const TdgConvDesc* d, int n_images, int form, const TdgEpilogue* epi, int n_first, char* name,
                        size_t name_bytes);

/* ---- dense fc2-style row ops (tf.matmul with one output unit, ops/layers.py:57 via
 *      models/gan.py:285, and its autodiff) --------------------------------------------- */
/* out[r] = act(dot(x[r, :cols], w) + bias[0]) */
int tdg_rowdot(int dtype, const void* x, int rows, int cols, const float* w, const float* bias,
               int act, float* out, void* stream);
/* dx[r, c] = (dout[r] * w[c]) * mask(mask_src[r, c]) */
int tdg_rowouter(int dtype, const float* dout, const float* w, int rows, int cols, int mask_mode,
                 float leak, const void* mask_src, void* dx, void* stream);
/* Finish column partials written by a conv epilogue (TdgEpilogue.col_partial, nblk row tiles, c columns):
 * out[n] = beta*out[n] + sum_b partial[(b*2)*c + n], fixed summation order. */
int tdg_col_finalize_sum(const float* partial, int nblk, int c, float* out, float beta, void* stream);
/* dw[c] = beta*dw[c] + sum_r coef[r] * x[r, c]   (coef NULL -> 1); deterministic */
int tdg_colsum_weighted(int dtype, const void* x, int rows, int cols, int cs, const float* coef,
                        float* dw, float beta, void* workspace, size_t workspace_bytes, void* stream);
size_t tdg_colsum_workspace_bytes(int rows, int cols);

/* ---- batch norm, training mode, no gamma (tf.contrib.layers.batch_norm defaults,
 *      ops/layers.py:58,103,144) ------------------------------------------
 * fwd : pre = (u - mean) * rsqrt(var + eps) + beta ; h = act(pre)   (u over `rows` x c)
 *       stats[0:c] = mean, stats[c:2c] = rstd (saved for backward).  u/pre use channel stride cs, h uses
 *       h_cs (h may be a channel window of a wider concat buffer); likewise dh uses dh_cs in bwd.
 * bwd : dpre = dh * act'(pre); du = rstd * (dpre - mean(dpre) - xhat * mean(dpre*xhat));
 *       dbeta = beta_acc*dbeta + sum(dpre)                                                */
size_t tdg_bn_workspace_bytes(int rows, int c);
int tdg_bn_fwd(int dtype, const void* u, int rows, int c, int cs, const float* beta, float eps,
               int act, float leak, void* pre, void* h, int h_cs, float* stats, void* workspace,
               size_t workspace_bytes, void* stream);
/* tdg_bn_fwd over `ngroups` batches of rows_per_group rows that lie behind each other in u / pre / h, each normalised with
 * ITS OWN batch statistics (stats [ngroups][2][c]; workspace >= ngroups * tdg_bn_workspace_bytes): the generator passes of
 * the n_disc_train critic runs of one iteration (models/gan.py:150-155,169-173 -- `sess.run(d_train_op)` n_disc_train times,
 * each drawing its own z through the same generator variables) taken as ONE pass; batch_norm (ops/layers.py:103,144)
 * normalises per run, i.e. per group.  pre may be null (no backward pass follows). */
int tdg_bn_fwd_groups(int dtype, const void* u, int rows_per_group, int ngroups, int c, int cs, const float* beta,
                      float eps, int act, float leak, void* pre, void* h, int h_cs, float* stats, void* workspace,
                      size_t workspace_bytes, void* stream);
/* ---- instance norm of the gen-2 layer surface (hem/ops/images.py:73-89; `use_instance_norm=True`,
 *      hem/ops/layers.py:123,200): per (image, channel) moments over the hw positions, biased variance, eps 1e-3,
 *      learned per-channel scale (init 1) and shift (init 0); fused with the layer's activation.
 *      stats [n][2][c] = (mu, rstd) are kept for the backward. */
int tdg_instance_norm_fwd(int dtype, const void* u, int n, int hw, int c, int cs, const float* scale, const float* shift,
                          float eps, int act, float leak, void* h, int h_cs, float* stats, void* stream);
/* du = d/du of act(scale * xhat + shift) given dh; dscale / dshift = beta * old + sums over images and positions
 * (deterministic); workspace >= n * 2 * c floats. */
int tdg_instance_norm_bwd(int dtype, const void* dh, int dh_cs, const void* u, int n, int hw, int c, int cs, const float* scale,
                          const float* shift, const float* stats, int act, float leak, void* du, float* dscale, float* dshift,
                          float beta, void* workspace, size_t workspace_bytes, void* stream);
/* out = act(a + b), flat, one layout: the shortcut sum of `residual` (hem/ops/layers.py:297-304); TDG_ACT_NONE = add */
int tdg_add_act(int dtype, const void* a, const void* b, size_t n, int act, float leak, void* out, void* stream);
/* tdg_bn_fwd with the batch statistics taken from TDG_COL_BN partials of the producing conv (pivot = that conv's
 * bias, may be NULL) instead of a pass over u: stats, then pre = (u - mean) * rstd + beta and h = act(pre).
 * pre may be NULL when no backward pass will follow this forward pass (the generator pass of a critic step): only h is written. */
int tdg_bn_fwd_from_partials(int dtype, const void* u, int rows, int c, int cs, const float* beta, float eps, int act,
                             float leak, void* pre, void* h, int h_cs, float* stats, const float* partial, int nblk,
                             const float* pivot_bias, void* stream);
/* dbias (optional): += / = the column sums of the stored du, i.e. the bias gradient of the conv in front of the batch
 * norm (BiasAddGrad of ops/layers.py:102 under :103), taken from the pass that writes du instead of a pass of its own. */
int tdg_bn_bwd(int dtype, const void* dh, int dh_cs, const void* pre, int rows, int c, int cs,
               const float* beta, const float* stats, int act, float leak, void* du, float* dbeta,
               float beta_acc, float* dbias, float dbias_acc, void* workspace, size_t workspace_bytes, void* stream);

/* ---- elementwise ------------------------------------------------------------------------ */
/* y = act(x + bias[c]) over rows x c (tf.nn.bias_add + activation) */
int tdg_bias_act(int dtype, const void* x, int rows, int c, int cs, const float* bias, int act,
                 float leak, void* y, void* stream);
/* dx = dy * act'(.) given the post-activation tensor (tanh/sigmoid/lrelu) */
int tdg_act_bwd(int dtype, const void* dy, const void* post, size_t n, int act, float leak, void* dx,
                void* stream);
/* out = scale * (in + shift), f32 in -> dtype out   (models/gan.py:50: 2*(x-0.5)) */
int tdg_affine_cast(int dtype, const float* in, size_t n, float scale, float shift, void* out, void* stream);
/* Two 4-channel activations from two compact f32 row sets (ca + cb == 4): out_ab[r] = scale * ([a[r] | b[r]] + shift) and
 * out_a0[r] = the same with zeros in b's channels -- pix2pix's critic inputs [x | y] and [x | G(x) to come]
 * (hem/models/pix2pix.py:103-104 rescale + the concat of :236) in one pass. */
int tdg_affine_cast_pair(int dtype, const float* a, int ca, const float* b, int cb, size_t rows, float scale, float shift,
                         void* out_ab, void* out_a0, void* stream);
/* out[r*cs + ch] = scale * (in[r*c + ch] + shift), ch < c: compact f32 rows -> channel-padded activation */
int tdg_affine_cast_rows(int dtype, const float* in, int rows, int c, int cs, float scale, float shift, void* out,
                         void* stream);
int tdg_cast_to_f32(int dtype, const void* in, size_t n, float* out, void* stream);
int tdg_cast_from_f32(int dtype, const float* in, size_t n, void* out, void* stream);
/* xhat[r,:] = x[r,:] + alpha[r] * (g[r,:] - x[r,:])   (models/gan.py:225-226) */
int tdg_gp_interp(int dtype, const void* x, const void* g, const float* alpha, int rows, int cols,
                  void* xhat, void* stream);
/* acc[0] = beta*acc[0] + sum(x^2) over n elements (models/gan.py:229); deterministic.
 * ONE-STREAM RULE: the kernel hands its last block a ticket from a per-process device-global slot, so launches of this entry point must not overlap on the device; the library returns TDG_EINVAL if it is launched on a second (non-capturing) stream of the process. */
int tdg_sumsq(int dtype, const void* x, size_t n, float* acc, float beta, void* workspace,
              size_t workspace_bytes, void* stream);
size_t tdg_reduce_workspace_bytes(size_t n);
/* out[0] = mean(x[0:n]) f32 input (tf.reduce_mean of D outputs, models/gan.py:196-204) */
int tdg_mean_f32(const float* x, int n, float* out, void* stream);
/* out[0] = beta * out[0] + sum of n floats, one launch (the bias gradient of a dense layer with one output: ops/layers.py:56-57) */
int tdg_sum_f32(const float* x, int n, float* out, float beta, void* stream);
/* out[s] = mean(x[s*seglen : (s+1)*seglen]) for s < nseg, one launch (the means of D(x) and D(g), :196-197) */
int tdg_mean_segments_f32(const float* x, int nseg, int seglen, float* out, void* stream);
/* Vanilla-GAN losses on post-sigmoid scores (models/gan.py:193-194) and their gradients w.r.t. the LOGITS:
 *   scal[0] = d_loss = mean(-log(dr+1e-8) - log(1-df+1e-8)),  scal[1] = g_loss = mean(-log(df+1e-8))
 *   seed_real = d d_loss/d logit_real, seed_fake_d = d d_loss/d logit_fake, seed_fake_g = d g_loss/d logit_fake */
int tdg_gan_logloss(const float* d_real, const float* d_fake, int n, float* seed_real, float* seed_fake_d,
                    float* seed_fake_g, float* scal, void* stream);
/* ---- pix2pix losses (hem/models/pix2pix.py:263-304) -------------------------------------------------
 * Sigmoid cross-entropy terms on the PatchGAN logits (channel 0, row stride cs) of the real pass
 * (rows [0, rows)) and the fake pass (rows [rows, 2*rows)):
 *   scal[0] = d_real = mean xent(z_real, 1), scal[1] = d_fake = mean xent(z_fake, 0),
 *   scal[2] = g_fake = mean xent(z_fake, 1)      (xent(z,l) = max(z,0) - z*l + log(1+exp(-|z|)), App. A-7)
 * mode 1 (D step): seed = d(d_real + d_fake)/dz for both passes; mode 2 (G step): seed_fake = d g_fake/dz,
 * seed_real = 0; mode 0: losses only.  seed has the layout of logits. */
int tdg_p2p_xent(int dtype, const void* logits, int rows, int cs, int mode, void* seed, float* scal, void* stream);
/* y, g: channel 0 of [-1,1] tensors with row stride cs.  scal[0] = l1 = mean|y01 - g01|, scal[1] = rmse (:285,299,
 * hem/ops/losses.py:10-11) after rescaling both to [0,1].  If dg != NULL: dg[r*dgs] += weight * d l1 / d g. */
int tdg_p2p_l1(int dtype, const void* y, const void* g, int rows, int cs, float weight, void* dg, int dgs, float* scal,
               void* workspace, size_t workspace_bytes, void* stream);
/* ---- paper_cgan pieces (hem/models/paper_cgan.py; 3dgan_amd/csrc/tdg_cgan.hip) ------------------------------------
 * tdg_cgan_prep: one workgroup per image of the staged f32 depth y [n,65,65] (:90-96):
 *   crop[b] = 10 * y[b, 17:46, 17:46] (f32 [n,29,29]), ybar[b] = mean(crop[b]) (f32 [n]);
 *   depth_real (channel 0 of the real half of D's depth input [n,29,29,depth_cs]) = crop (version 0, baseline) or
 *   crop - ybar (1, mean_adjusted; 2, mean_provided2).  Version 2 also writes channel 1 = ybar of depth_real AND of
 *   depth_fake (the fake half, same layout).  g_ones (nullable): that channel of [n,65,65,g_cs] = 1 (mean_provided2's G
 *   input, :286); rgb_ybar (nullable): that channel of [n,65,65,rgb_cs] = ybar (mean_provided2's rgb D input, :323). */
int tdg_cgan_prep(int dtype, const float* y, int n, int version, void* depth_real, int depth_cs, void* depth_fake, float* ybar,
                  float* crop, void* g_ones, int g_cs, void* rgb_ybar, int rgb_cs, void* stream);
/* tdg_cgan_head_fwd: the generator head d4 (1x1 conv, cin -> 1, no activation) on the top-left crop x crop pixels of the
 * hw x hw concat [n,hw,hw,cs] only (:241-242): g = w . cat + b.  yhat = g + ybar[b] (ybar nullable: + 0), f32 [n,crop,crop];
 * fake (channel 0 of D's fake depth input, channel stride fake_cs, compute dtype) = g.  cin in {64,128,256,512}: any other
 * cin, like a bad dtype, is TDG_EINVAL for all four head entries, before anything is launched or timed. */
int tdg_cgan_head_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, int crop, const float* w, const float* b,
                      const float* ybar, float* yhat, void* fake, int fake_cs, void* stream);
/* tdg_cgan_head_bwd: from delta = dL/dg (channel 0 of dfake, [n,crop,crop,fake_cs]):
 *   dcat[p, c] = delta[p] * w[c] * mask(cat[p, c]) inside the crop, 0 outside it (the first writer of dcat);
 *   dw[c] = sum_p delta[p] * cat[p, c], db[0] = sum_p delta[p]  (f32, overwritten; per-image partials in the workspace of
 *   n * (cin + 1) floats, summed in image order: deterministic).  mask_mode / leak as in TdgEpilogue (TDG_MASK_LRELU: the
 *   derivative of the decoder's lrelu on its window; on the relu encoder window it is replaced by the relu mask the
 *   encoder's backward-data epilogue applies after adding the main path). */
int tdg_cgan_head_bwd(int dtype, const void* dfake, int fake_cs, const void* cat, int n, int hw, int cin, int cs, int crop,
                      const float* w, int mask_mode, float leak, void* dcat, float* dw, float* db, void* workspace,
                      size_t workspace_bytes, void* stream);
/* tdg_cgan_head_noise_fwd / _bwd: the head of paper_sampler --noise_layer d4, a (cin + 1) -> 1 conv whose last input channel is
 * a uniform draw (hem/models/paper_sampler.py:228-230).  The concat is not widened: u f32 [n,hw,hw] is read directly,
 *   g = w[0:cin] . cat + w[cin] * u + b,   dw[cin] = sum_p delta[p] * u[p]  (w and dw hold cin + 1 entries; workspace of
 *   n * (cin + 2) floats, the same per-image partials finished in image order); no gradient goes to u.
 * u nullable: then exactly tdg_cgan_head_fwd / _bwd (w and dw of cin entries, n * (cin + 1) floats), bit for bit.
 * g (nullable): g as f32 [n,crop,crop], before its rounding into `fake` (the sampler statistics read it). */
int tdg_cgan_head_noise_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, int crop, const float* w, const float* b,
                            const float* u, const float* ybar, float* yhat, float* g, void* fake, int fake_cs, void* stream);
int tdg_cgan_head_noise_bwd(int dtype, const void* dfake, int fake_cs, const void* cat, int n, int hw, int cin, int cs, int crop,
                            const float* w, const float* u, int mask_mode, float leak, void* dcat, float* dw, float* db,
                            void* workspace, size_t workspace_bytes, void* stream);
/* tdg_cgan_join: D's combined input [rows, comb_cs] = [rgb path output | depth path output] (:332) where the rgb path ran
 * ONCE over n_rgb images (it is the same for D(x,y) and D(x,yhat)) and the depth path over both halves.
 *   mode 0: comb[r, 0:c] = rgb[r % n_rgb], comb[r, c:2c] = depth[r]                                   (r < rows)
 *   mode 1: depth[r] = comb[r, c:2c]; if rgb: rgb[b] = comb[b, 0:c] + comb[n_rgb + b, 0:c]   (b < n_rgb, rows >= 2 n_rgb)
 * c, the strides and the pointers are multiples of 8 elements (16-byte vector access). */
int tdg_cgan_join(int dtype, int mode, int n_rgb, int rows, int c, void* comb, int comb_cs, void* rgb, int rgb_cs, void* depth,
                  int depth_cs, void* stream);
/* tdg_cgan_wgan_loss: WGAN losses on the SIGMOID outputs (:395-403) of the 1x1 logits (channel 0, row stride cs) of the
 * real pass (rows [0, rows)) and the fake pass (rows [rows, 2*rows)):
 *   scal[0] = g_fake = -mean s(z_fake), scal[1] = d_fake = mean s(z_fake), scal[2] = d_real = mean s(z_real),
 *   scal[3] = d_total = d_fake - d_real.
 * mode 1 (D step): seed_real = -s(1-s)/rows, seed_fake = +s(1-s)/rows; mode 2 (G step): seed_fake = -s(1-s)/rows,
 * seed_real = 0; mode 0: losses only.  seed has the layout of logits. */
int tdg_cgan_wgan_loss(int dtype, const void* logits, int rows, int cs, int mode, void* seed, float* scal, void* stream);
/* tdg_cgan_metrics: the Eigen-2014 metrics of one set (:447-478) on a = y / 10, p = pred / 10 over n images of hw pixels:
 * y f32 [n*hw] (10x depth), pred = pred[i] (nullable: 0) + offset[i / hw] (nullable: 0).
 *   out[0] abs_rel_diff = mean(|a-p|/p), out[1] squared_rel_diff = mean((a-p)^2/p), out[2] linear_rmse,
 *   out[3] log_rmse, out[4] scale_invariant_log_rmse = mean(d^2) - (sum d)^2/n^2  (d = log(a+1e-8) - log(p+1e-8)),
 *   out[5..7] threshold1..3: tf.metrics.percentage_below(max(a/p, p/a), 1.25^k) -- STREAMING: counts[0..2] (hits) and
 *   counts[3] (elements) are device-resident running totals, never reset, and out = counts[k] / counts[3].
 * Division by a non-positive p gives inf / NaN exactly where the formulas do.  Per-block f64 partials in the workspace
 * (tdg_cgan_metrics_workspace_bytes()), finished in block order by a second launch: deterministic. */
int tdg_cgan_metrics(const float* y, const float* pred, const float* offset, int n, int hw, unsigned long long* counts, float* out,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t tdg_cgan_metrics_workspace_bytes(void);
/* ---- paper_cgan dataset evaluation (paper/paper_metrics.py, paper/paper_train.py:43-60; 3dgan_amd/csrc/tdg_cgan_eval.hip) --
 * A sweep over a split adds every batch into device-resident accumulators and reads the host once, after tdg_cgan_eval_finish.
 * acc: tdg_cgan_eval_acc_bytes(hw) bytes of doubles, zeroed by the caller before a sweep:
 *   acc[set * 9 + k], k < 8: the sum over batches of value k (the order of tdg_cgan_metrics' out) of set `set`; k = 8: the
 *   batches added to that set;  acc[27]: the batches added to the moments;  acc[28 + p] / acc[28 + hw + p]: the sums over
 *   batches of pixel p's batch mean / batch variance.
 * counts: unsigned long long [3][4], per set the streaming threshold totals of tdg_cgan_metrics (hits 1..3, elements).
 * tdg_cgan_eval_batch: ONE read of y f32 [n*hw] (10x depth) and pred gives the eight values of tdg_cgan_metrics for every set
 *   in the bit mask `sets`:  1: prediction pred[i];  2: offset[i / hw] (nullable: 0);  4: image[i % hw] * image_scale (f32), a
 *   per-pixel image broadcast over the batch.  Each set's values are ADDED to its sums in acc and its batch count advances;
 *   out[5..7] enter as the RUNNING percentages after this batch.  Each set equals tdg_cgan_metrics on the same prediction
 *   bit for bit before its f32 rounding (same block partition, same arithmetic).  Workspace: tdg_cgan_eval_workspace_bytes(). */
int tdg_cgan_eval_batch(const float* y, const float* pred, const float* offset, const float* image, float image_scale, int n, int hw,
                        int sets, unsigned long long* counts, double* acc, void* workspace, size_t workspace_bytes, void* stream);
size_t tdg_cgan_eval_workspace_bytes(void);
size_t tdg_cgan_eval_acc_bytes(int hw);
/* tdg_cgan_eval_moments: tf.nn.moments(y, axes=0) of y f32 [n,hw] in float64, two passes: per pixel the batch mean and the mean
 *   of the squared deviations from it, added to acc[28 + p] and acc[28 + hw + p]; acc[27] += 1. */
int tdg_cgan_eval_moments(const float* y, int n, int hw, double* acc, void* stream);
/* tdg_cgan_sample_stats: what paper_sampler's metric_summaries adds to the eight Eigen values (hem/models/paper_sampler.py:337-342)
 *   for one set of n images of hw pixels.  y f32 [n,hw]; g f32 [n,hw] (nullable: 0); the prediction as tdg_cgan_eval_batch takes
 *   it: y_hat[b,p] = image[p] * image_scale (image given; pred and offset must be null) or pred[b,p] + offset[b] (either
 *   nullable: 0), rounded in f32; everything after that in f64.  out f32 [6], in units of `unit` (10: the reference's [0,1]):
 *   [0], [1] the mean and the min over the images of mean_p |y - y_hat| / unit;  [2], [3] the mean over the pixels of the
 *   batch mean of g / unit and of its population variance / unit^2 (tf.nn.moments(g, axes=0), two passes);  [4], [5] the same
 *   of y_hat.  mean_img / var_img (both or neither) f32 [hw]: the per-pixel batch mean / unit and variance / unit^2 of y_hat.
 *   Fixed-order f64 reductions (no atomics): two launches are bit-equal. */
int tdg_cgan_sample_stats(const float* y, const float* g, const float* pred, const float* offset, const float* image,
                          float image_scale, int n, int hw, float unit, float* out, float* mean_img, float* var_img,
                          void* workspace, size_t workspace_bytes, void* stream);
size_t tdg_cgan_sample_stats_workspace_bytes(int n, int hw);
/* ---- paper_standalone (hem/models/paper_standalone.py; 3dgan_amd/csrc/tdg_cgan_standalone.hip) ---------------------------
 * tdg_cgan_rmse_loss: the regression loss of :244-253 and its gradient for one batch.  y, yhat f32 [n,hw] in depth units (10x);
 *   d = yhat - y, S = sum d^2, N = n hw:  scal[0] = sqrt(S / N) / 10 = sqrt(mean((yhat/10 - y/10)^2)), one scalar, and
 *   dg[(b hw + p) dg_cs] = d / (10 sqrt(N S)) = d loss / d yhat in the compute dtype -- channel 0 of a buffer of channel
 *   stride dg_cs, what tdg_cgan_head_bwd / tdg_cgan_head_noise_bwd read as dfake; no other channel is written.
 *   Differences, squares and sums in f64, combined in a fixed order without atomics: two launches are bit-equal.  Two launches
 *   of ceil(N / 1024) blocks (at most 1024): block partials, then every block re-sums them and scales its slice.
 *   DEVIATION: S == 0 gives loss 0 and a zero gradient (TensorFlow: NaN).
 *   Workspace: tdg_cgan_rmse_loss_workspace_bytes(n, hw) = 8 min(ceil(n hw / 1024), 1024) bytes (0 for n or hw <= 0). */
int tdg_cgan_rmse_loss(int dtype, const float* y, const float* yhat, int n, int hw, void* dg, int dg_cs, float* scal,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t tdg_cgan_rmse_loss_workspace_bytes(int n, int hw);
/* tdg_cgan_bar_fill: the fed y_bar channel of g_mean_provided (:176-207).  win[(b hw2 + p) win_cs] = ybar[b] in the compute
 *   dtype for b < n, p < hw2 -- one channel of an NHWC window of channel stride win_cs -- and, when `plane` is given,
 *   plane[b hw2 + p] = ybar[b] (f32).  Nothing else is written. */
int tdg_cgan_bar_fill(int dtype, const float* ybar, int n, int hw2, void* win, int win_cs, float* plane, void* stream);
/* ---- mean_depth_estimator (hem/models/mean_depth_estimator.py:136-147; 3dgan_amd/csrc/tdg_mde.hip) ---------------------------
 * tdg_mde_loss: the scene mean-depth loss and its gradient seed for one batch.  y_full f32 [n,hw]; m [n] in the compute dtype,
 *   element i at m[i m_cs] (the network's sigmoid output).  mean_out[i] = f32(mean_p y_full[i,p]): the f64 sum of the image in a
 *   fixed order, divided once and rounded once.  scal[0] = f32((1/n) sum_i |mean_i - m_i|), every mean_i kept f64, m_i widened
 *   from its stored type, the n terms added in image order.  seed[i seed_cs] = sign(m_i - mean_i) * f32(1/n) in the compute
 *   dtype: dL/dm, the gradient with respect to the sigmoid's OUTPUT (the caller applies the activation's derivative).
 *   DEVIATION: sign(0) = 0 where the reference's sqrt(square(d)) has the gradient NaN.  No atomics: two launches are bit-equal.
 *   Two launches: one block per image (at most 4096 blocks), then a one-block finish over the n terms.
 *   Workspace: tdg_mde_loss_workspace_bytes(n) = 8 n bytes (0 for n <= 0), 8-byte aligned. */
int tdg_mde_loss(int dtype, const float* y_full, int n, int hw, const void* m, int m_cs, float* mean_out, void* seed, int seed_cs,
                 float* scal, void* workspace, size_t workspace_bytes, void* stream);
size_t tdg_mde_loss_workspace_bytes(int n);
/* ---- experimental_sampler (hem/models/experimental_sampler.py; 3dgan_amd/csrc/tdg_xsamp.hip) ---------------------------------
 * tdg_xsamp_prep: ONE pass over the staged f32 batch that writes every input tensor of a generator and critic pass (:107-149).
 *   x f32 [n,S,S,3], x_loc, y_loc f32 [n,S,S,1], m f32 [n] (the estimator's mean depth), y f32 [n,S,S,1] (nullable: no depth
 *   output may then be given); x_rows, y_rows int32 [n] (nullable: the identity), entries in [0, n) -- an entry outside is clamped
 *   into it, never dereferenced.  With r = x_rows[b], channels 0..5 of pixel p of output row b are
 *   [fl(2 x[r,p] - 1) (3) | x_loc[r,p] | y_loc[r,p] | m[r]], rounded to the compute dtype and written to g_in (channel stride
 *   g_cs >= 7) AND to rgb_in (channel stride rgb_cs >= 6), each nullable.  Channel 6 of g_in (the noise) and every padding channel
 *   are NOT written.  With q = y_rows[b] the depth target fl(2 y[q, off + i, off + j] - 1), i, j < T, goes to channel 0 of
 *   depth_real [n,T,T,depth_cs] (compute dtype, nullable) and to target f32 [n,T,T] (nullable).  off + T <= S.
 *   The row maps express the training pass (both null), the sampler set (both all-zero: row 0 broadcast) and the shuffled set
 *   (x_rows a permutation, y_rows null). */
int tdg_xsamp_prep(int dtype, const float* x, const float* x_loc, const float* y_loc, const float* m, const float* y, const int* x_rows,
                   const int* y_rows, int n, int S, int T, int off, void* g_in, int g_cs, void* rgb_in, int rgb_cs, void* depth_real,
                   int depth_cs, float* target, void* stream);
/* tdg_xsamp_head_fwd: the generator head d5 (1x1 conv, cin -> 1, tanh) on the FULL hw x hw plane of the last concat
 *   [n,hw,hw,cs] (:246-248; the reference's "31x31x1" comment is off, the plane is 32x32): z = w . cat + b, accumulated as
 *   tdg_cgan_head_fwd accumulates it, g = tanhf(z).  g f32 [n,hw,hw]; fake (channel 0 of D's fake depth input, channel stride
 *   fake_cs, compute dtype) = g rounded.  cin in {64,128,256,512}. */
int tdg_xsamp_head_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, const float* w, const float* b, float* g,
                       void* fake, int fake_cs, void* stream);
/* tdg_xsamp_head_bwd: from dL/dg (channel 0 of dfake, [n,hw,hw,fake_cs]) and the f32 g tdg_xsamp_head_fwd stored (NOT its
 *   rounding to the compute dtype): dz = dL/dg * fl(1 - fl(g g)), then the contract of tdg_cgan_head_bwd at crop == hw:
 *   dcat[p, c] = dz[p] * w[c] * mask(cat[p, c]) (the first writer of dcat); dw[c] = sum_p dz[p] * cat[p, c], db[0] = sum_p dz[p]
 *   (f32, overwritten; per-image partials in the workspace of n * (cin + 1) floats, summed in image order: deterministic).
 *   With g == 0 everywhere the three results are tdg_cgan_head_bwd's bit for bit. */
int tdg_xsamp_head_bwd(int dtype, const void* dfake, int fake_cs, const float* g, const void* cat, int n, int hw, int cin, int cs,
                       const float* w, int mask_mode, float leak, void* dcat, float* dw, float* db, void* workspace,
                       size_t workspace_bytes, void* stream);
/* ---- improved_sampler (hem/models/improved_sampler.py; 3dgan_amd/csrc/tdg_isamp.hip) ------------------------------------------
 * tdg_isamp_prep: tdg_xsamp_prep made general (:109-181).  planes P in {3, 5, 6}: [fl(2 x - 1) (3)], + [x_loc | y_loc], + a
 *   per-pixel mean_vec plane f32 [n,S,S] (x_loc / y_loc may be null for P = 3, mean_vec for P < 6).  Source side S, crop side T at
 *   offset off (off + T <= S); the row maps x_rows, y_rows as in tdg_xsamp_prep, an entry outside [0, n) clamped into it before it
 *   becomes an address.  Channels 0..P-1 go to g_in (channel stride g_cs >= P + 1) AND to rgb_in (rgb_cs >= P), each nullable;
 *   channel P of g_in (the noise) and every padding channel are NOT written.  The depth target fl(2 y[q, off + i, off + j] - 1)
 *   goes to channel 0 of depth_real [n,T,T,depth_cs] (nullable) and to target f32 [n,T,T] (nullable); without y neither may be
 *   given.  For P = 6 and mean_vec[b,:,:] == m[b] every written bit is tdg_xsamp_prep's. */
int tdg_isamp_prep(int dtype, const float* x, const float* x_loc, const float* y_loc, const float* mean_vec, const float* y,
                   const int* x_rows, const int* y_rows, int n, int S, int T, int off, int planes, void* g_in, int g_cs, void* rgb_in,
                   int rgb_cs, void* depth_real, int depth_cs, float* target, void* stream);
/* tdg_isamp_head_bn_fwd: generator A1's head d4 (:293 under the decoder's arg_scope: 1x1 conv cin -> 1, batch norm, tanh) on the
 *   hw x hw concat [n,hw,hw,cs].  Phase 1, one block per image: z = w . cat + b, accumulated as tdg_xsamp_head_fwd accumulates
 *   it, and the image's sums of z and z z in f64.  Phase 2: S, Q = the partials added in a fixed order (f64), N = n hw hw,
 *   mean = S / N, var = max(Q / N - mean mean, 0) (biased), stats[0] = f32(mean), stats[1] = rstd = f32(1 / sqrt(var + eps)); then
 *   in f32 zhat = fl(fl(z - stats[0]) * stats[1]), g = tanhf(fl(zhat + beta[0])) (no gamma).  g f32 [n,hw,hw], zhat f32 [n,hw,hw]
 *   (kept for the backward pass), fake (channel 0 of D's fake depth input, channel stride fake_cs) = g rounded to the compute
 *   dtype.  cin in {64,128,256,512}, cs % 8 == 0.  Workspace: 16 n bytes, 8-byte aligned (tdg_isamp_head_bn_workspace_bytes
 *   covers both passes).  No atomics: two launches are bit-equal. */
size_t tdg_isamp_head_bn_workspace_bytes(int n, int cin);
int tdg_isamp_head_bn_fwd(int dtype, const void* cat, int n, int hw, int cin, int cs, const float* w, const float* b, const float* beta,
                          float eps, float* g, float* zhat, float* stats, void* fake, int fake_cs, void* workspace,
                          size_t workspace_bytes, void* stream);
/* tdg_isamp_head_bn_bwd: from dL/dg (channel 0 of dfake) and the stored g, zhat and stats: dy = dL/dg * fl(1 - fl(g g));
 *   dbeta[0] = f32(sum dy) (overwritten; the sum in f64 from per-image partials, a fixed order); m1 = f32(sum dy / N),
 *   m2 = f32(sum dy zhat / N); dz = fl(rstd * fl(fl(dy - m1) - fl(zhat m2))) -- batch norm's backward pass without gamma --; then
 *   tdg_xsamp_head_bwd's contract from dz on: dcat[p, c] = dz[p] * w[c] * mask(cat[p, c]) (the first writer of dcat),
 *   dw[c] = sum_p dz[p] cat[p, c], db[0] = sum_p dz[p] (f32, overwritten; per-image partials summed in image order).
 *   Workspace: tdg_isamp_head_bn_workspace_bytes(n, cin) = 16 n + 4 n (cin + 1) bytes, 8-byte aligned. */
int tdg_isamp_head_bn_bwd(int dtype, const void* dfake, int fake_cs, const float* g, const float* zhat, const float* stats,
                          const void* cat, int n, int hw, int cin, int cs, const float* w, int mask_mode, float leak, void* dcat,
                          float* dw, float* db, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* tdg_isamp_rmse_grad: `--g_rmse` (:930-935): dfake[r dgs] += d rmse / d g[r], rmse = sqrt(mean(((g + 1) / 2 - (y + 1) / 2)^2)) over
 *   the `rows` values, read from the device scalar rmse[0] (scal[1] of tdg_p2p_l1 on the same tensors).  g, y: channel 0 of
 *   [-1,1] tensors of the compute dtype with row stride cs.  In f32, each operation rounded once, in this order:
 *   k = 1 / fl(fl(4 * f32(rows)) * rmse);  t = fl(fl(g[r] - y[r]) * k);  dfake[r dgs] = round_to_dtype(fl(dfake[r dgs] + t)).
 *   rmse == 0 is not guarded: k is then inf and the results are not finite, as the gradient of tf.sqrt at 0 is not. */
int tdg_isamp_rmse_grad(int dtype, const void* g, const void* y, int rows, int cs, const float* rmse, void* dfake, int dgs,
                        void* stream);
/* tdg_isamp_zero_fraction: tf.nn.zero_fraction (`--g_sparsity`, :928) of the rows x c entries of x with row stride cs >= c (the
 *   padding is not counted): out[0] = f32(count / (rows c)) with count the entries equal to zero (-0.0 counts), an exact integer,
 *   and the division in f64.  Workspace: tdg_isamp_zero_fraction_workspace_bytes(), 8-byte aligned. */
size_t tdg_isamp_zero_fraction_workspace_bytes(void);
int tdg_isamp_zero_fraction(int dtype, const void* x, int rows, int c, int cs, float* out, void* workspace, size_t workspace_bytes,
                            void* stream);
/* ---- artist (hem/models/artist.py:71-83; 3dgan_amd/csrc/tdg_artist.hip) -------------------------------------------------------
 * tdg_artist_mse: the whole-image loss of one decoder and its seed in ONE pass.  target: compact f32 [rows, c], the staged
 *   batch in [0, 1]; h, seed: [rows, cs] in dtype, h the decoder's tanh output in [-1, 1].  1 <= c <= 4 (image planes),
 *   cs % 8 == 0, h and seed 16-byte aligned (one 16-byte load of h per pixel), target 4-byte aligned: 16-byte loads of it
 *   where its base is 16-byte aligned, 4-byte loads otherwise.  Per element, in f32, each operation rounded once, in this
 *   order (hem.rescale: the target's round trip [0,1] -> [-1,1] -> [0,1], then h to [0,1]):
 *     tm = fl(fl(2 t) - 1);  t01 = fl(fl(tm + 1) * 0.5);  h01 = fl(fl(h + 1) * 0.5);  d = fl(h01 - t01);
 *     seed = round_to_dtype(fl(d * k)),  k = fl(1 / fl(rows c))   (the multiplications by 2 and 0.5 are exact)
 *   -- d loss / d h: the 2 of the square and the 1/2 of the rescale cancel.  seed == NULL (mode 0, evaluation): the loss alone.
 *   Channels [c, cs) of seed are NEVER written (as tdg_l1_loss leaves them).
 *   scal[0] = f32(S / (rows c)), scal[1] = f32(sqrt(S / (rows c))), with S = the sum of the EXACT squares d d in f64 (the
 *   product of two f32 fits f64), the division and the square root in f64: per thread, wave shuffle, the four waves, one f64
 *   partial per block (a grid-stride loop over 1024-pixel tiles, four blocks per compute unit, at most 1024), then the
 *   partials by one block in the same shape.  A fixed order and no atomics: two launches are bit-equal.  One launch plus the
 *   finish.  Workspace: tdg_artist_mse_workspace_bytes() = 8192 bytes, 8-byte aligned; a short one is TDG_EWORKSPACE, a null
 *   pointer, rows <= 0, c outside [1, min(4, cs)], cs % 8 != 0 or a misaligned pointer TDG_EINVAL, all before any launch. */
size_t tdg_artist_mse_workspace_bytes(void);
int tdg_artist_mse(int dtype, const float* target, const void* h, int rows, int c, int cs, void* seed, float* scal, void* workspace,
                   size_t workspace_bytes, void* stream);
/* tdg_cgan_eval_finish: scalars f64 [3][12], per set: the eight sums / batches, counts[k] / counts[3] for k < 3 (the final
 *   running percentages) and the batches (a set with no batch gives NaN).  mean_img / var_img f32 [hw] (both or neither):
 *   acc[28 + p] / acc[27] / unit and acc[28 + hw + p] / acc[27] / unit^2 -- unit = 10 turns the 10x depth into [0, 1]. */
int tdg_cgan_eval_finish(const double* acc, const unsigned long long* counts, int hw, float unit, double* scalars, float* mean_img,
                         float* var_img, void* stream);
/* ---- paper_cgan full-frame inference (paper_fullimage.py; 3dgan_amd/csrc/tdg_cgan_full.hip) ----------------------------
 * The 65x65 window slides over an H x W frame at stride s (build_batch, :90-110): cols = (H - 93) / s windows down,
 * rows = (W - 93) / s across, P = cols * rows; patch c = n * cols + m (n < rows outer, m < cols inner) has its top-left
 * corner at (m s, n s).  H, W >= 94 and s >= 1 or TDG_EINVAL.  The chunk index is a device int, so that a captured chunk
 * body (gather -> model -> store) replays as the next chunk.
 * tdg_cgan_full_gather: image f32 [H,W,3] and depth f32 [H,W] -> x_stage f32 [batch,65,65,3] and y_stage f32 [batch,65,65,1]:
 *   slot b holds patch c = chunk[0] * batch + b, zeros where c >= P (the reference's zero padding).  A pure copy. */
int tdg_cgan_full_gather(const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch,
                         float* x_stage, float* y_stage, void* stream);
/* tdg_cgan_full_store: yhat f32 [batch,29,29] and ybar f32 [batch] (nullable: zeros, the baseline's g = y_hat) to slots
 * [chunk[0] * batch, chunk[0] * batch + batch) of store_yhat f32 [slots,29,29] / store_ybar f32 [slots]; then chunk[0] += 1
 * (a second launch).  A chunk that would pass `slots` writes nothing but still advances. */
int tdg_cgan_full_store(const float* yhat, const float* ybar, int batch, long long slots, int* chunk, float* store_yhat,
                        float* store_ybar, void* stream);
/* tdg_cgan_full_blend: the ordered blend of reconstruct (:126-155), one launch.  Patch c's 29x29 block lands at
 * (m s + offset, n s + offset) (offset in [0, 36]; the reference places it at 18).  Per pixel, over the covering patches in
 * ascending c, in float64: the first sets v = d, every later one v = (v + d) / 2; uncovered pixels are 0 (nan_to_num).
 *   canvas_yhat f32 [H,W] from d = store_yhat; canvas_g f32 [H,W] from d = store_yhat - store_ybar (f32).
 * Each canvas is bit-equal to the float64 recurrence cast to f32.  P > slots is TDG_EINVAL. */
int tdg_cgan_full_blend(const float* store_yhat, const float* store_ybar, long long slots, int H, int W, int stride, int offset,
                        float* canvas_yhat, float* canvas_g, void* stream);
/* tdg_cgan_full_rmse: out[0] = sqrt(mean((double(10 depth) - canvas)^2)) (f64) over rows [18, H-46) and columns [18, W-46)
 * of depth f32 [H,W] (10 depth rounded in f32, as the reference) and canvas f32 [H,W] (:157-163).  Per-block f64 partials
 * in a workspace of at least 256 doubles, finished in block order by a second launch: deterministic. */
int tdg_cgan_full_rmse(const float* depth, const float* canvas, int H, int W, double* out, void* workspace, size_t workspace_bytes,
                       void* stream);
/* ---- whole-frame sampling of paper_sampler / paper_noise (3dgan_amd/csrc/tdg_cgan_full.hip) ------------------------------
 * The grid of tdg_cgan_full_gather with the sampler set's batching (hem/models/paper_sampler.py:88-101): a window's `rep` rows
 * are copies of that ONE window, one noise draw per copy.
 * tdg_cgan_full_gather_rep: tdg_cgan_full_gather with every window repeated: row b of x_stage f32 [batch,65,65,3] / y_stage
 *   f32 [batch,65,65,1] holds patch c = chunk[0] * (batch / rep) + b / rep, zeros where c >= P.  depth is nullable: y_stage
 *   is then zero.  rep < 1 or batch % rep != 0 is TDG_EINVAL.  With rep == 1 it writes what tdg_cgan_full_gather writes. */
int tdg_cgan_full_gather_rep(const float* image, const float* depth, int H, int W, int stride, const int* chunk, int batch, int rep,
                             float* x_stage, float* y_stage, void* stream);
/* tdg_cgan_full_sample_store: yhat f32 [batch,29,29] as batch / draws groups of `draws` consecutive rows; group k goes to slot
 *   s = chunk[0] * (batch / draws) + k:  store_yhat[s,p] = the f64 mean over the group's rows of yhat[b,p] as f32 (10x depth, as
 *   tdg_cgan_full_store writes);  store_var[s,p] = their two-pass f64 population variance / 100 as f32 ([0, 1] units);
 *   store_ybar[s] = ybar of the group's first row (ybar nullable: 0);  with crop f32 [batch,29,29] (crop and store_err both or
 *   neither), a_b = mean_p |crop[b,p] - yhat[b,p]| per row and store_err[s,0], [s,1] = the mean and the min of a_b over the
 *   group / 10 (per_image_rmse/mean and /min of tdg_cgan_sample_stats, per window).  Then chunk[0] += 1 (a second launch).  A
 *   call whose slots would pass `slots` writes nothing but still advances.  draws < 1 or batch % draws != 0 is TDG_EINVAL.
 *   Fixed-order f64 reductions (no atomics): two launches are bit-equal. */
int tdg_cgan_full_sample_store(const float* yhat, const float* ybar, const float* crop, int batch, int draws, long long slots,
                               int* chunk, float* store_yhat, float* store_var, float* store_ybar, float* store_err, void* stream);
/* ---- VAE pieces (models/vae.py:66-90,113-129) -------------------------------------------------------
 * heads = [z_mean | z_stddev] rows of 2L (channel stride hs); z = mean + stddev * eps (models/vae.py:128) */
int tdg_vae_reparam(int dtype, const void* heads, int hs, const void* eps, int es, int rows, int L, void* z, int zs,
                    void* stream);
/* dheads = [dz | dz * eps] */
int tdg_vae_reparam_bwd(int dtype, const void* dz, int zs, const void* eps, int es, int rows, int L, void* dheads, int hs,
                        void* stream);
/* --vae_full_elbo (SURVEY App. C-7 opt-in: the reference differentiates the reconstruction term alone, models/vae.py:41):
 * dheads = [dz + w*m | dz*eps + w*(s - s / (1e-8 + s^2))], the gradient of decoder_loss + w * latent_loss (:80-81) */
int tdg_vae_reparam_bwd_kl(int dtype, const void* dz, int zs, const void* eps, int es, const void* heads, int hs_in,
                           float kl_weight, int rows, int L, void* dheads, int hs, void* stream);
/* scal[0] = latent_loss = 0.5 * sum(mean^2 + std^2 - log(1e-8 + std^2) - 1)  (models/vae.py:80-81) */
int tdg_vae_kl(int dtype, const void* heads, int hs, int rows, int L, float* scal, void* workspace, size_t workspace_bytes,
               void* stream);
/* scal[0] = decoder_loss = -sum(x log(1e-8+d) + (1-x) log(1e-8+1-d)) (models/vae.py:76-77);
 * seed = d decoder_loss / d d.  x: compact f32 [rows, c] in [0,1]; d, seed: [rows, cs] in dtype. */
int tdg_vae_bce(int dtype, const float* x, const void* d, int rows, int c, int cs, void* seed, float* scal, void* workspace,
                size_t workspace_bytes, void* stream);
/* Convolutional autoencoder loss (models/cnn.py:31,75-79): with xs = scale * (x + shift) (the rescale to [-1,1]),
 * scal[0] = mean |xs - d|, seed = d loss / d d = sign(d - xs) / (rows * c)  (sign(0) = 0, TF AbsGrad).
 * x: compact f32 [rows, c]; d, seed: [rows, cs] in dtype. */
int tdg_l1_loss(int dtype, const float* x, const void* d, int rows, int c, int cs, float scale, float shift, void* seed,
                float* scal, void* workspace, size_t workspace_bytes, void* stream);
/* tf.nn.dropout(y, keep_prob) (hem/ops/layers.py:207) given the uniform draws u [rows, c] (compact f32):
 * y = y * floor(keep_prob + u) / keep_prob, in place on [rows, ycs]-strided y.  Applied to the incoming gradient with
 * the same u it is the layer's backward. */
int tdg_dropout(int dtype, void* y, int rows, int c, int ycs, const float* u, float keep, void* stream);
/* GP scalars from sumsq (device-resident, no host sync): slopes = sqrt(ss);
 * scal[0] = penalty = (slopes-1)^2 ; scal[1] = lambda * 2*(slopes-1)/slopes            */
int tdg_gp_scalars(const float* sumsq, float lambda, float* scal, void* stream);
/* tdg_sumsq (beta = 0) and tdg_gp_scalars in one launch (models/gan.py:229-230: slopes over the WHOLE batch tensor, penalty) */
int tdg_gp_sumsq(int dtype, const void* x, size_t n, float* sumsq, float lambda, float* scal, void* workspace,
                 size_t workspace_bytes, void* stream);
/* out = coef[0] * in   (u = d penalty / d v, coefficient read from device memory) */
int tdg_scale_by_dev(int dtype, const void* in, size_t n, const float* coef, void* out, void* stream);
/* --gp_per_sample (SURVEY App. C-4 opt-in: the reference takes ONE norm over the whole batch tensor, models/gan.py:229):
 * per row r of v [rows, cols]: slopes_r = |v_r|, pen_rows[r] = (slopes_r - 1)^2 and
 * u_r = lambda * 2 (slopes_r - 1) / (slopes_r * rows) * v_r  =  d(lambda * mean_r pen_r) / d v_r. */
int tdg_gp_rows(int dtype, const void* v, int rows, int cols, float lambda, float* pen_rows, void* u, void* stream);
/* x[i] = value for i < n (f32) */
int tdg_fill_f32(float* x, size_t n, float value, void* stream);
/* column sums of a rows x c activation: db[c] = beta*db[c] + sum_r dy[r,c] (bias gradient) */
int tdg_bias_grad(int dtype, const void* dy, int rows, int c, int cs, float* db, float beta,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimizers on flat f32 buckets (tf.train.*Optimizer via util.py:150-183) ----------- */
/* Adam: lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller */
int tdg_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr_t, float beta1,
                  float beta2, float eps, float grad_scale, void* stream);
/* Same update with the step count t kept in device memory (t_dev[0] = number of steps already applied):
 * lr_t is derived in-kernel, so a captured hipGraph can be replayed without re-baking arguments, and the kernel itself
 * counts the step (t_dev[0] += 1, by its last block).
 * ONE-STREAM RULE: the kernel hands its last block a ticket from a per-process device-global slot, so launches of this entry point must not overlap on the device; the library returns TDG_EINVAL if it is launched on a second (non-capturing) stream of the process. */
int tdg_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                      float beta2, float eps, float grad_scale, int32_t* t_dev, void* stream);
int tdg_add_i32(int32_t* x, int32_t inc, void* stream);
/* RMSProp (rms slot initialised to 1 by the caller), optional momentum, not centered */
int tdg_rmsprop_step(float* p, const float* g, float* rms, float* mom, size_t n, float lr,
                     float decay, float momentum, float eps, float grad_scale, void* stream);
/* RMSProp with centered=True (util.py:161-164 `centered = args.centered`): mg slot starts at 0 */
int tdg_rmsprop_centered_step(float* p, const float* g, float* mg, float* rms, float* mom, size_t n,
                              float lr, float decay, float momentum, float eps, float grad_scale,
                              void* stream);
/* tf.train.AdagradOptimizer / ProximalAdagradOptimizer with zero regularisation (util.py:167-168,
 * :173-174): acc slot starts at 0.1 */
int tdg_adagrad_step(float* p, const float* g, float* acc, size_t n, float lr, float grad_scale,
                     void* stream);
/* tf.train.AdadeltaOptimizer (util.py:165-166): rho 0.95, eps 1e-8 by default, slots start at 0 */
int tdg_adadelta_step(float* p, const float* g, float* acc, float* acc_update, size_t n, float lr,
                      float rho, float eps, float grad_scale, void* stream);
/* tf.train.FtrlOptimizer (util.py:182-183), lr_power -0.5: acc slot starts at 0.1, linear at 0 */
int tdg_ftrl_step(float* p, const float* g, float* acc, float* linear, size_t n, float lr, float l1,
                  float l2, float grad_scale, void* stream);
int tdg_sgd_momentum_step(float* p, const float* g, float* acc, size_t n, float lr, float momentum,
                          float grad_scale, void* stream);
/* p = clamp(p, lo, hi)  (models/gan.py:142-143; never executed by the reference, App. C-3) */
int tdg_clamp(float* p, size_t n, float lo, float hi, void* stream);
/* flag[0] = 1 if any element is NaN/Inf (hem/util/training.py:52-53 tf.check_numerics) */
int tdg_check_finite(const float* x, size_t n, int* flag, void* stream);

/* ---- RNG: Philox4x32-10 counter streams (tf.random_normal / tf.random_uniform,
 *      models/gan.py:246,224) -------------------------------------------------------------- */
int tdg_random_normal(int dtype, uint64_t seed, uint64_t stream_id, uint64_t offset, size_t n,
                      void* out, void* stream);
int tdg_random_uniform_f32(uint64_t seed, uint64_t stream_id, uint64_t offset, size_t n, float* out,
                           void* stream);
/* Graph-replayable forms: the counter offset is ((draw_dev[0] + 1) << 24), read from device memory, and the kernel
 * itself counts the draw (draw_dev[0] += 1, by its last block), so a replay of the same launch is a fresh draw.
 * ONE-STREAM RULE: the kernel hands its last block a ticket from a per-process device-global slot, so launches of this entry point must not overlap on the device; the library returns TDG_EINVAL if it is launched on a second (non-capturing) stream of the process.
 * DRAW WINDOW: each draw owns 2^24 counters, i.e. 2^26 values; n > 2^26 would run into the next draw's counters and
 * returns TDG_EINVAL (n == 2^26 is legal). */
int tdg_random_normal_dev(int dtype, uint64_t seed, uint64_t stream_id, int32_t* draw_dev, size_t n,
                          void* out, void* stream);
/* (the same window: n > 2^26 returns TDG_EINVAL) */
int tdg_random_uniform_f32_dev(uint64_t seed, uint64_t stream_id, int32_t* draw_dev, size_t n, float* out,
                               void* stream);

/* ---- tensor summaries for the training event files (hem/ops/summaries.py:31-75: per layer, gradient and weight a
 *      tf.summary.histogram, tf.nn.zero_fraction and tf.reduce_mean; called at hem/models/paper_cgan.py:166-177 and
 *      hem/models/artist.py:99-103) for a whole table of tensors at once.
 *      One job is one tensor of rows x c live elements with row stride cs (elements); a flat array is rows = 1, c = cs = n.
 *      Any base alignment the dtype allows is legal, and only live elements are read.  The element value is
 *      v = f32(x) * scale (one f32 multiply; gradients of a multi-rank run are summarised with scale = 1 / world size).
 *      Per job the result record of tdg_tensor_summary_result_bytes() bytes holds, in this order:
 *        uint64 num, zeros (v == 0, both signs), nonfinite (NaN, +-Inf);  float min, max;  double sum, sum_squares
 *        (of (double)v and (double)v * (double)v);  uint64 bucket[1551].
 *      Non-finite elements count in `nonfinite` only; with no finite element min, max and the sums are 0.
 *      Buckets are TensorFlow's default histogram: element v adds to bucket b = the number of limits <= (double)v of the
 *      1551 limits [-DBL_MAX, -pos reversed, 0, pos, DBL_MAX], pos = 1e-12 * 1.1^k by repeated f64 multiplication while
 *      below 1e20.  tdg_tensor_summary_limits (host, no GPU work) fills that table; the caller keeps a device copy and hands
 *      it to every launch.
 *      tdg_tensor_summary: `jobs_dev`, `limits_dev`, `results_dev` (njobs records) and `workspace` (at least
 *      tdg_tensor_summary_workspace_bytes(njobs, total live elements) bytes) are device memory.  Counts are exact; the sums
 *      are combined in a fixed order, so two launches on the same input are bit-equal in every field.  The entry reads the
 *      job table back to validate it and to size its grid -- it synchronises `stream`, unlike every other entry, and must not
 *      be called inside a captured body -- then enqueues a fixed three operations whatever njobs is.  A bad argument or job is
 *      a status, and nothing is written. */
typedef struct TdgSummaryJob {
  const void* ptr;
  uint64_t rows;
  int32_t c, cs;
  int32_t dtype;            /* TDG_F32 | TDG_BF16 */
  float scale;
} TdgSummaryJob;
int tdg_tensor_summary_limits(double* out);
size_t tdg_tensor_summary_result_bytes(void);
size_t tdg_tensor_summary_workspace_bytes(int njobs, uint64_t total_elems);
int tdg_tensor_summary(const TdgSummaryJob* jobs_dev, int njobs, const double* limits_dev, void* results_dev, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- activation montages for the training event files (hem.summarize_layers(..., montage=True), hem/ops/summaries.py:31-48:
 *      hem.montage (:139-181) of image 0 of a layer, through tf.summary.image) for a whole table of activations at once.
 *      One job is image 0 of an NHWC activation: `ptr` is pixel (0,0), channel 0 of the live window, h x w pixels of c live
 *      channels, pixel stride cs (elements, cs >= c).  Any base alignment the dtype allows is legal, only the live channels
 *      are read, and nothing behind the last live element of the last pixel.
 *      Layout: (m, n) = factorization(c), m the largest divisor of c with m * m <= c, n = c / m.  The job's montage is n*h rows
 *      by m*w columns of one byte each, row-major from `out_offset` of the packed output; channel j*m + i lands at block row j,
 *      block column i.
 *      Values (TensorFlow's NormalizeFloatImage): lo and hi are the min and max over the finite elements of the image (bf16
 *      widened to f32).  If lo < 0: M = max(|lo|, |hi|), scale = M < 1e-6f ? 0 : 127.0f / M, offset = 128.0f; otherwise
 *      scale = hi < 1e-6f ? 0 : 255.0f / hi, offset = 0.  A finite pixel v becomes (uint8) min(v * scale + offset, 255.0f): one
 *      IEEE f32 divide, one f32 multiply, one f32 add (not fused), truncation.  A non-finite pixel becomes 255; an image
 *      with no finite element is all 255 and reports lo = hi = 0.
 *      tdg_activation_montage: `jobs_dev`, `out_dev` (out_bytes bytes) and `results_dev` (njobs x {float lo, hi}) are device
 *      memory.  Bytes of the output outside every job's n*h*m*w region are not written.  Two launches on the same input are
 *      bit-equal.  Like tdg_tensor_summary the entry reads the job table back to validate it -- it synchronises `stream` and
 *      must not be called inside a captured body -- then enqueues two launches whatever njobs is.  A bad job (null pointer,
 *      non-positive dims, cs < c, unknown dtype, a region that overlaps another or runs past out_bytes) is a status, and
 *      nothing is written. */
typedef struct TdgMontageJob {
  const void* ptr;
  int32_t h, w, c, cs;
  int32_t dtype;            /* TDG_F32 | TDG_BF16 */
  int32_t reserved;
  uint64_t out_offset;
} TdgMontageJob;
int tdg_activation_montage(const TdgMontageJob* jobs_dev, int njobs, void* out_dev, size_t out_bytes, float* results_dev,
                           void* stream);

/* ---- input pipeline, host side (no GPU work): PNG scanline reconstruction (filter types 0-4 of the PNG
 *      specification) after the caller has inflated the IDAT stream -- what tf.image.decode_png does for the
 *      reference's nyuv2 / floorplan records (hem/data/nyuv2.py:152-153, data.py:15).  `filtered` holds `rows`
 *      scanlines of 1 + row_bytes bytes, `out` receives rows * row_bytes bytes; bpp = bytes per complete pixel. */
int tdg_png_unfilter(const unsigned char* filtered, int rows, int row_bytes, int bpp, unsigned char* out);

/* ---- tdg_jpeg_info / tdg_jpeg_decode: a JPEG file's bytes -> width x height x 3 RGB bytes (host memory, no device work).
 *      Replaces `tf.image.decode_image(..., channels=3)` on the reference's floorplan records, whose `image` feature is
 *      the raw bytes of the source file (data/floorplan_tfrecords.py:26-41 writes them, data.py:15 decodes them).
 *      Baseline and extended-sequential Huffman files, 8 bit, 1 (grayscale, replicated to 3 channels) or 3 components,
 *      sampling factors 1 and 2, restart intervals; libjpeg's default arithmetic (accurate integer inverse DCT, triangle
 *      chroma upsampling, 16-bit fixed-point YCbCr -> RGB).  Progressive / arithmetic / 12-bit / CMYK files: TDG_EINVAL
 *      with the reason in tdg_last_error(). */
int tdg_jpeg_info(const unsigned char* data, size_t nbytes, int* width, int* height, int* components);
int tdg_jpeg_decode(const unsigned char* data, size_t nbytes, unsigned char* rgb, size_t rgb_bytes);

/* ---- tdg_shuffle_draw / tdg_gather_rows: the host side of the streaming input pipeline (no device work) --------------
 *      `d.repeat().shuffle(buffer_size)` of the reference (data.py:56-57, train.py:171-174: buffer_size 10000) on example
 *      INDICES: `buf[0 .. buf_len)` holds the indices currently in the shuffle buffer, `*next_in` the next index of the
 *      repeated stream 0, 1, ..., n_total-1, 0, 1, ... to enter it.  Each of the `count` draws picks a uniformly random slot
 *      (xoshiro256** on state[4], Lemire's unbiased range reduction), writes its index to `out` and refills the slot from
 *      the stream -- tf.data's ShuffleDataset semantics: an example can appear at most ~buf_len draws before its stream
 *      position, never later than the buffer lets it wait.  The caller fills buf with the first min(buffer_size, ...)
 *      stream indices and sets *next_in behind them.
 *      tdg_gather_rows: out[i] = src[idx[i]] for rows of `row_bytes` bytes (the batch assembled in pinned host memory). */
int tdg_shuffle_draw(int64_t* buf, int64_t buf_len, uint64_t* state, int64_t* next_in, int64_t n_total, int64_t count,
                     int64_t* out);
int tdg_gather_rows(const unsigned char* src, int64_t n_rows, size_t row_bytes, const int64_t* idx, int64_t count,
                    unsigned char* out);

#ifdef __cplusplus
}
#endif
#endif /* TDG_H_ */
