"""Noise-injected RGB-to-depth cGAN of the thesis' experiment 2 on MI355X -- the reference's gen-2 plugin
`hem/models/paper_sampler.py` (arguments :14-58, __init__ :60-152, train :154-157, g_baseline :159-235, d_baseline :237-260,
loss :262-275, metric_summaries :304-342) on the HIP kernels.

The model is paper_cgan's `mean_adjusted` row (models/paper/paper_cgan.py: y = crop(10 y), y_hat = g + y_bar, the critic sees
(x, g) and (x, y - y_bar), g is written straight into D's fake depth input) with sigmoid cross-entropy and two Adam optimizers,
whose generator takes ONE channel of U(0,1) noise -- 512 at `e4-512` -- behind the node `--noise_layer` names:

    x    [x | u]      65x65x4   -> e1        e4      [e4 | u]        1x1x513  -> d1      d3  [d2 | e2 | u]  14x14x257 -> d3
    e1   [e1 | u]     31x31x65  -> e2        e4-512  [e4 | u(512)]   1x1x1024 -> d1      d4  [d3 | e1 | u]  31x31x129 -> d4 (head)
    e2   [e2 | u]     14x14x129 -> e3        d2      [d1 | e3 | u]   5x5x513  -> d2
    e3   [e3 | u]     5x5x257   -> e4

Every generator pass draws fresh noise (injection key 'noise_<node>').  The U-Net executor keeps each of these a zero-copy
channel window (unet.py); at `d4` the 1x1 head reads the f32 draw itself (tdg_cgan_head_noise_fwd / _bwd).

Reference-effective behaviour and what is opt-in:
  * `--e_bn` is `store_true` with the STRING default 'false' (:47-51), which is truthy: the reference's encoder has batch norm
    whether or not the flag is given.  Kept, flag and default; `--e_bn_off` (not in the reference) builds the encoder without
    batch norm, which is paper_noise's generator.
  * y_sampler is named 'tower_{}_g_sampler' a second time (:106,108); TF uniquifies the name, nothing reads it.  No tensor
    names exist here.
  * d_baseline's "14x14" comment (:251) is 13x13, as in paper_cgan.
  * the loss dict has the order of :274: g_fake, d_real, d_fake, d_total.

`metrics()`: `metrics_y_hat`, `metrics_y_0`, `metrics_y_mean` (while a mean image is set) and `metrics_y_sampler`, each the
eight Eigen values plus per_image_rmse/mean, /min, g_moments/mean, /var, y_hat_moments/mean, /var (tdg_cgan_sample_stats).
The sampler set (:88-108,146) broadcasts image 0 of the last loss fetch over the batch and runs the generator once more with
fresh noise, as one graph-replayed body; like infer() it writes the generator's activations and D's input buffers, which
every step rewrites, and leaves the variables, the optimizers and the last fetch's results alone.  `sample(x, y)` is the same
pass on an image of the caller's and returns the per-pixel mean and variance of the B predictions: an uncertainty map.

Not offered: infer_full and evaluate.  With encoder batch norm a window's output depends on its batch neighbours, so neither a
sliding window nor a dataset sweep means what it means for paper_cgan.  `sample_full(image, depth)` is the whole-frame entry
point: every window runs as the sampler set runs image 0 -- a batch of copies of that one window, one draw per copy -- and the
per-pixel mean and variance over the draws are blended into frame canvases (paper_sample_fullimage.py drives it).
"""
import torch

from ... import _lib
from ... import kernels as K
from ...ops.layers import conv2d, deconv2d, concat, arg_scope, variable_scope, random_uniform
from ...ops.activations import _lrelu, relu
from ...util import collection_to_dict
from ..ModelPlugin import ModelPlugin
from ..paper.paper_cgan import CganReplica, METRIC_KEYS, SRC, CROP, FULL_OFFSET, FULL_RMSE_BLOCKS, _FullBuffers, patch_grid  # noqa: F401

NODES = ['x', 'e1', 'e2', 'e3', 'e4', 'e4-512', 'd2', 'd3', 'd4']
STAT_KEYS = ('per_image_rmse/mean', 'per_image_rmse/min', 'g_moments/mean', 'g_moments/var', 'y_hat_moments/mean',
             'y_hat_moments/var')


def rate_arguments():
    """:16-40: the six rate / beta flags."""
    return {
        '--g_lr': {'type': float, 'default': 1e-3, 'help': 'Learning rate for generator.'},
        '--d_lr': {'type': float, 'default': 1e-3, 'help': 'Learning rate for discriminator.'},
        '--g_beta1': {'type': float, 'default': 0.9, 'help': 'Beta1 for generator'},
        '--d_beta1': {'type': float, 'default': 0.9, 'help': 'Beta1 for discriminator.'},
        '--g_beta2': {'type': float, 'default': 0.999, 'help': 'Beta2 for generator.'},
        '--d_beta2': {'type': float, 'default': 0.999, 'help': 'Beta2 for discriminator.'},
    }


class SamplerReplica(CganReplica):
    """paper_sampler and paper_noise: CganReplica's mean_adjusted model with the noisy generator, the reference's loss order,
    the six per-set statistics, the sampler pass and sample()."""

    @classmethod
    def _version_name(cls, args):
        return 'mean_adjusted'                                   # :110-113

    @staticmethod
    def noise_layer(args):
        return getattr(args, 'noise_layer', 'x')

    @staticmethod
    def encoder_batch_norm(args):
        """`args.e_bn` as the reference reads it -- any truthy value, its default string 'false' included -- unless
        `--e_bn_off` is given."""
        return bool(getattr(args, 'e_bn', 'false')) and not getattr(args, 'e_bn_off', False)

    @classmethod
    def generator(cls, x, args, reuse=False):
        """g_baseline (:159-235): x [B,65,65,3] -> the 31x31x1 head, cropped to 29x29 by the executor."""
        B, node = args.batch_size, cls.noise_layer(args)
        if node not in NODES:
            raise ValueError('--noise_layer %r is not one of %s' % (node, ', '.join(NODES)))

        def noisy(t, at, channels=1):
            if node != at:
                return t
            return concat([t, random_uniform([B, t.shape[1], t.shape[2], channels], minval=0, maxval=1)])
        with variable_scope('encoder'), arg_scope([conv2d], reuse=reuse, filter_size=5, stride=2, padding='VALID', init='xavier',
                                                  use_batch_norm=cls.encoder_batch_norm(args), activation=relu):
            h = noisy(x, 'x')
            e1 = conv2d(h, h.shape[-1], 64, name='e1')            # 31x31x64
            h = noisy(e1, 'e1')
            e2 = conv2d(h, h.shape[-1], 128, name='e2')           # 14x14x128
            h = noisy(e2, 'e2')
            e3 = conv2d(h, h.shape[-1], 256, name='e3')           # 5x5x256
            h = noisy(e3, 'e3')
            e4 = conv2d(h, h.shape[-1], 512, name='e4')           # 1x1x512
        with variable_scope('decoder'), arg_scope([deconv2d, conv2d], reuse=reuse, filter_size=5, stride=2, init='xavier',
                                                  padding='VALID', activation=_lrelu(0.2)):
            h = noisy(noisy(e4, 'e4'), 'e4-512', 512)
            y = deconv2d(h, h.shape[-1], 256, output_shape=(B, 256, 5, 5), name='d1')
            h = noisy(concat([y, e3]), 'd2')                      # 5x5x512
            y = deconv2d(h, h.shape[-1], 128, output_shape=(B, 128, 14, 14), name='d2')
            h = noisy(concat([y, e2]), 'd3')                      # 14x14x256
            y = deconv2d(h, h.shape[-1], 64, output_shape=(B, 64, 31, 31), name='d3')
            h = noisy(concat([y, e1]), 'd4')                      # 31x31x128
            y = conv2d(h, h.shape[-1], 1, stride=1, filter_size=1, padding='SAME', activation=None, name='d4')   # 31x31x1
        return y

    def __init__(self, x_y, args, sess=None):
        self.NOISE_KEYS = {'e4': 'noise_' + self.noise_layer(args)}          # the latent node has two forms: 'e4', 'e4-512'
        CganReplica.__init__(self, x_y, args, sess)
        B, dev = self.B, self.sess.device
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.g32, self.inf_g = f32(B, CROP, CROP), f32(B, CROP, CROP)          # g of the last loss fetch / of infer(), f32
        # the sampler pass: image 0 of the last loss fetch, its broadcast, and the pass's results
        self.x0, self.y0 = f32(1, SRC, SRC, 3), f32(1, SRC, SRC, 1)
        self.samp_x, self.samp_y = f32(B, SRC, SRC, 3), f32(B, SRC, SRC, 1)
        self.samp_ybar, self.samp_crop, self.samp_yhat, self.samp_g = f32(B), f32(B, CROP, CROP), f32(B, CROP, CROP), f32(B, CROP, CROP)
        self.samp_mean, self.samp_var = f32(CROP, CROP), f32(CROP, CROP)
        self.counts['y_sampler'] = torch.zeros(4, dtype=torch.int64, device=dev)
        self.sample_counts = torch.zeros(4, dtype=torch.int64, device=dev)
        self.samp_eigen = f32(8)
        self.stat_out = {k: f32(6) for k in ('y_hat', 'y_0', 'y_mean', 'y_sampler')}
        self.stat_ws = torch.zeros(_lib.load().tdg_cgan_sample_stats_workspace_bytes(B, CROP * CROP), dtype=torch.uint8, device=dev)
        self._full_sample = self._full                           # sample_full's frame buffers by (H, W, stride, draws): the one cache

    # ---- steps -------------------------------------------------------------------------------------------
    def _generate(self, ybar, yhat, g32=None):
        """Every pass keeps g in f32 beside y_hat: the statistics read it."""
        if g32 is None:
            g32 = self.g32 if yhat is self.yhat else self.inf_g
        CganReplica._generate(self, ybar, yhat, g32)

    def _g_grads(self):
        CganReplica._g_grads(self)
        self.x0.copy_(self.x_stage[:1])                          # x_sample / y_sample of :88-89, kept for metrics()
        self.y0.copy_(self.y_stage[:1])

    def _losses(self):
        d = CganReplica._losses(self)
        return {k: d[k] for k in ('g_fake', 'd_real', 'd_fake', 'd_total')}      # the order of :274

    def _train(self):
        """:154-157: one D step, then the G step and the loss fetch on the next batch."""
        self.d_step(self.x_y.next_batch())
        self.g_step(self.x_y.next_batch())
        return self._losses()

    # ---- statistics, sampler pass ----------------------------------------------------------------------------
    def _stats(self, name, crop, g, pred, offset, image, images=False):
        _lib.call('tdg_cgan_sample_stats', K.ptr(crop), K.ptr(g), K.ptr(pred), K.ptr(offset), K.ptr(image), 10.0, self.B, CROP * CROP,
                  10.0, K.ptr(self.stat_out[name]), K.ptr(self.samp_mean) if images else None,
                  K.ptr(self.samp_var) if images else None, K.ptr(self.stat_ws), self.stat_ws.numel(), K.stream())

    def _sampler_pass(self):
        """g_sampler (:99-101): the generator on the B copies in samp_x / samp_y with fresh noise; y_sampler = g_sampler +
        mean(y_sample)."""
        self._inputs(self.samp_ybar, self.samp_crop, self.samp_x, self.samp_y)
        self._generate(self.samp_ybar, self.samp_yhat, self.samp_g)

    def _eigen_sampler(self, counts):
        _lib.call('tdg_cgan_metrics', K.ptr(self.samp_crop), K.ptr(self.samp_yhat), None, self.B, CROP * CROP, K.ptr(counts),
                  K.ptr(self.samp_eigen), K.ptr(self.metric_ws), self.metric_ws.numel(), K.stream())

    def _metrics_sampler_body(self):
        B = self.B
        self.samp_x.copy_(self.x0.expand(B, SRC, SRC, 3))
        self.samp_y.copy_(self.y0.expand(B, SRC, SRC, 1))
        self._sampler_pass()
        self._eigen_sampler(self.counts['y_sampler'])
        self._stats('y_sampler', self.samp_crop, self.samp_g, self.samp_yhat, None, None)

    def _sample_body(self):
        self._sampler_pass()
        self._stats('y_sampler', self.samp_crop, self.samp_g, self.samp_yhat, None, None, images=True)

    def metrics(self):
        """`metrics_y_hat`, `metrics_y_0`, `metrics_y_mean` (while a mean image is set) of the last loss fetch's batch and
        `metrics_y_sampler` of its image 0 under B fresh noise draws (:143-146).  Each set: the eight Eigen values and
        STAT_KEYS, in the reference's [0, 1] units.  The streaming threshold totals are per set; each call is one
        evaluation."""
        out = CganReplica.metrics(self)
        self._stats('y_hat', self.crop, self.g32, self.yhat, None, None)
        self._stats('y_0', self.crop, None, None, self.ybar, None)                 # g_0 = 0, y_0 = y_bar
        if self.mean_image is not None:                                             # (g, 10 * mean image), :145
            self._stats('y_mean', self.crop, self.g32, None, None, self.mean_image)
        self._run('metrics_sampler', self._metrics_sampler_body)
        out['metrics_y_sampler'] = dict(zip(METRIC_KEYS, self.samp_eigen.cpu().tolist()))
        for name in ('y_hat', 'y_0', 'y_mean', 'y_sampler'):
            if 'metrics_' + name in out:
                out['metrics_' + name].update(zip(STAT_KEYS, self.stat_out[name].cpu().tolist()))
        return out

    def sample(self, x, y=None):
        """B predictions for ONE image under B noise draws.  x f32 [65,65,3] in [0, 1]; y (optional) its depth [65,65] or
        [65,65,1] in [0, 1].  Returns a dict: `y_hat` f32 [B,29,29] (device; 10x depth like infer(); without y, y_bar is 0 and
        the predictions are g), `mean` and `var` f32 [29,29] (device): the per-pixel mean and population variance of the
        predictions in [0, 1] units -- the uncertainty map -- and `metrics`: with y, the set's 14 values (thresholds of
        this call alone), else None."""
        dev = self.sess.device
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32)
        if tuple(x.shape) != (SRC, SRC, 3):
            raise ValueError('sample: x must be [%d,%d,3], got %s' % (SRC, SRC, tuple(x.shape)))
        if y is not None:
            y = torch.as_tensor(y).to(device=dev, dtype=torch.float32)
            if tuple(y.shape) not in ((SRC, SRC), (SRC, SRC, 1)):
                raise ValueError('sample: y must be [%d,%d] or [%d,%d,1], got %s' % (SRC, SRC, SRC, SRC, tuple(y.shape)))
            self.samp_y.copy_(y.reshape(1, SRC, SRC, 1).expand(self.B, SRC, SRC, 1))
        else:
            self.samp_y.zero_()
        self.samp_x.copy_(x.reshape(1, SRC, SRC, 3).expand(self.B, SRC, SRC, 3))
        self._run('sample', self._sample_body)
        out = {'y_hat': self.samp_yhat.clone(), 'mean': self.samp_mean.clone(), 'var': self.samp_var.clone(), 'metrics': None}
        if y is not None:
            self.sample_counts.zero_()
            self._eigen_sampler(self.sample_counts)
            out['metrics'] = dict(zip(METRIC_KEYS + STAT_KEYS, self.samp_eigen.cpu().tolist() + self.stat_out['y_sampler'].cpu().tolist()))
        return out

    # ---- whole-frame sampling --------------------------------------------------------------------------------
    def sample_full(self, image, depth=None, stride=10, offset=FULL_OFFSET, draws=None, windows=False):
        """Per-pixel mean and variance of the predictions over a whole frame: the 65x65 window slid at `stride` as infer_full
        of paper_cgan slides it, each window run through the sampler pass -- a batch of copies of that ONE window, one noise
        draw per copy (:88-101), the one batching of a sliding window that means the same with and without batch norm: a
        window's result depends on nothing but the window and the draws.

        image f32 [H,W,3], depth f32 [H,W] or [H,W,1] in [0, 1] or None (y_bar is then 0 and the predictions are g).  `draws`
        (default batch_size) must divide batch_size; with encoder batch norm it must equal batch_size (the batch statistics
        must be those of one window), without it batch_size / draws windows share a pass.  Per pass one graph-replayed body:
        tdg_cgan_full_gather_rep into samp_x / samp_y, the sampler pass, tdg_cgan_full_sample_store (the draws' f64 mean and
        variance per pixel).  Then the reference's blend recurrence, at the reference's +18 offset, on all three canvases.

        The variance canvas is that recurrence applied to the per-window variances -- a blend of variance maps, each over
        the draws of one window -- NOT a pooled variance of every prediction that covers a pixel.

        Returns a FullSample.  Like sample() it uses the sampler pass's buffers and leaves the variables, the optimizers,
        the last fetch's results and what metrics() reports for metrics_y_hat / metrics_y_0 alone."""
        B = self.B
        draws = B if draws is None else int(draws)
        if draws < 1 or B % draws:
            raise ValueError('sample_full: draws %d must divide the batch size %d' % (draws, B))
        if draws != B and self.encoder_batch_norm(self.args):
            raise ValueError('sample_full: with batch norm in the encoder a pass must hold ONE window, draws = batch_size = %d (got %d)'
                             % (B, draws))
        with_depth = depth is not None
        image = torch.as_tensor(image)
        image, depth = self._frame(image, depth if with_depth else torch.zeros(tuple(image.shape[:2])))
        H, W = int(image.shape[0]), int(image.shape[1])
        per_pass = B // draws
        # beside the common buffers: the variance store with its all-zero y_bar, the two error columns per slot, the variance canvases
        extras = lambda slots, f32: dict(n_passes=slots // per_pass, store_var=f32(slots, CROP, CROP), zero_ybar=f32(slots),
                                         store_err=f32(slots, 2), var=f32(H, W), var_g=f32(H, W))
        fb, grid = self._frame_sweep(
            'sample_full', image, depth, stride, offset, (H, W, stride, draws),
            'sample_full_%d_%d_%d_%d%s' % (H, W, stride, draws, '' if with_depth else '_g'), per_pass,
            lambda fb, H, W, stride: self._sample_full_pass(fb, H, W, stride, draws, with_depth), extras, rmse=with_depth)
        self._blend(fb, fb.store_var, fb.zero_ybar, H, W, stride, offset, fb.var, fb.var_g)
        P = grid.patches
        rmse = err_mean = err_min = None
        if with_depth:
            err_mean, err_min = fb.store_err[:P].double().mean(dim=0).cpu().tolist()
            rmse = float(fb.rmse.item())
        out = FullSample(fb.yhat.clone(), fb.g.clone(), fb.var.clone(), rmse, err_mean, err_min, P, (grid.cols, grid.rows), draws)
        if windows:
            out.window_y_hat, out.window_var, out.window_y_bar = fb.store_yhat[:P].clone(), fb.store_var[:P].clone(), fb.store_ybar[:P].clone()
        return out

    def _sample_full_pass(self, fb, H, W, stride, draws, with_depth):
        """One pass: its windows, `draws` copies each, into samp_x / samp_y, the sampler pass, the draws' mean / variance /
        errors into the stores; advances fb.chunk."""
        _lib.call('tdg_cgan_full_gather_rep', K.ptr(fb.image), K.ptr(fb.depth) if with_depth else None, H, W, stride, K.ptr(fb.chunk),
                  self.B, draws, K.ptr(self.samp_x), K.ptr(self.samp_y), K.stream())
        self._sampler_pass()
        _lib.call('tdg_cgan_full_sample_store', K.ptr(self.samp_yhat), K.ptr(self.samp_ybar), K.ptr(self.samp_crop) if with_depth else None,
                  self.B, draws, fb.slots, K.ptr(fb.chunk), K.ptr(fb.store_yhat), K.ptr(fb.store_var), K.ptr(fb.store_ybar),
                  K.ptr(fb.store_err) if with_depth else None, K.stream())

    # ---- not offered -----------------------------------------------------------------------------------------
    _WHY_NOT = ('%s is not offered by %s: with batch norm in the encoder a window\'s output depends on the other images of its '
                'batch, so the result would depend on how the windows are batched')

    def infer_full(self, *a, **kw):
        raise NotImplementedError(self._WHY_NOT % ('infer_full', self.name))

    def evaluate(self, *a, **kw):
        raise NotImplementedError(self._WHY_NOT % ('evaluate', self.name))


class FullSample:
    """sample_full's result: the y_hat, g and var canvases (device f32 [H,W]; y_hat and g in 10x depth like FullFrame's, var in
    [0, 1] units like sample()'s), rmse (the frame RMSE of the y_hat canvas), err_mean / err_min (the mean over the windows of
    each window's per_image_rmse/mean and /min over its draws) -- all three None without depth --, patches, grid (cols, rows)
    and draws.  With windows=True also window_y_hat, window_var [patches,29,29] and window_y_bar [patches]: what was blended."""

    window_y_hat = window_var = window_y_bar = None

    def __init__(self, y_hat, g, var, rmse, err_mean, err_min, patches, grid, draws):
        self.y_hat, self.g, self.var, self.rmse, self.err_mean, self.err_min = y_hat, g, var, rmse, err_mean, err_min
        self.patches, self.grid, self.draws = patches, grid, draws

    def __repr__(self):
        return 'FullSample(%dx%d, patches=%d, grid=%s, draws=%d, rmse=%s)' % (self.y_hat.shape[0], self.y_hat.shape[1], self.patches,
                                                                              self.grid, self.draws, self.rmse)


class paper_sampler(ModelPlugin, SamplerReplica):
    name = 'paper_sampler'

    @staticmethod
    def arguments():
        """hem/models/paper_sampler.py:14-58, plus the opt-in --e_bn_off."""
        a = rate_arguments()
        a['--noise_layer'] = {'type': str, 'choices': list(NODES), 'default': 'x',
                              'help': 'Which node to add noise to. See generator code for the node names.'}
        a['--e_bn'] = {'action': 'store_true', 'default': 'false',
                       'help': 'Use batchnorm in encoder (the reference\'s default, the string \'false\', is truthy: on either way).'}
        a['--e_bn_off'] = {'action': 'store_true', 'default': False,
                           'help': 'Build the encoder without batch norm (not in the reference, whose --e_bn cannot be switched off).'}
        return a

    def train(self, sess=None, args=None, feed_dict=None):
        return self._train()
