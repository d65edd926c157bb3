"""RGB-to-depth conditional GAN of the thesis experiments on MI355X -- the reference's gen-2 plugin
`hem/models/paper_cgan.py` (arguments :14-57, __init__ :60-192, train :200-209, generators :212-310, discriminators
:312-388, loss :390-412, metrics :447-478) on the HIP kernels.

Kept: the plugin contract, the builders with the reference's variable names (`generator/encoder/vars/e1/weights`,
`discriminator/rgb_path/vars/hx1/weights`, `discriminator/combined_path/vars/h3/bias`), xavier init of weights and biases,
the optimizers of :64-69 (the global --optimizer / --lr do not apply), the per-version table below and the loss dict of
`collection_to_dict(losses)`:

    version          G output y_hat   D depth input real / fake   D builder
    baseline         g                y / g                       discriminator
    mean_adjusted    g + y_bar        y - y_bar / g               discriminator
    mean_provided2   g + y_bar        [y - y_bar | y_bar] / [g | y_bar]   discriminator with y_bar channels

The fake depth input is g itself where the reference computes (g + y_bar) - y_bar: one f32 rounding apart.
Reference-effective behaviour and what is opt-in:
  * `mean_provided` cannot be built by the reference (`tf.variablpe_scope`, :245): ValueError here too.
  * wgan: the real-pass mean is named 'd_fake' a second time (:403), so TF uniquifies it: keys g_fake, d_fake, d_fake_1, d_total.
  * wgan weight clipping (:181-187) never runs in the reference: no clip by default; with `--wgan_clip c`
    both D and G variables are clamped to [-c, c] before their steps.
  * the threshold metrics are tf.metrics.percentage_below: running totals since the model was built, never reset.

Dataset evaluation (paper/paper_metrics.py, the mean / variance image pre-pass of paper/paper_train.py:43-60,130-132 and
`metrics_y_mean`, :79,177): set_mean_image / dataset_moments / evaluate on the kernels of tdg_cgan_eval.hip; a sweep adds
every batch into device-resident f64 accumulators and reads the host once.

Classes: GeneratorReplica is everything here that needs no critic (the generator, its pass and backward pass, metrics, dataset
evaluation, full-frame inference; models/standalone/ trains it on a regression loss), CganReplica the critic on top of it.

MI355X-native: activations are NHWC; the generator runs on the skip U-Net executor (unet.py: zero-copy skip concats);
D's rgb path runs ONCE over the B images -- it is identical for D(x, y) and D(x, y_hat) -- and its output fills the left
window of both halves of the combined input (tdg_cgan_join), its backward sums the two halves' gradients first; the depth
path and the 1x1 combined path run as one batched pass over 2B images; the 1x1 one-channel head computes the 29x29 crop
only (tdg_cgan_head_fwd / _bwd) and writes g straight into D's fake depth input.
"""
import torch

from ... import _lib
from ... import kernels as K
from ... import engine
from ...ops.layers import conv2d, deconv2d, concat, arg_scope, variable_scope, placeholder, reset_graph
from ...ops.activations import _lrelu, relu
from ...unet import UNet
from ...util import tower_scope_range, collection_to_dict
from ..ModelPlugin import ModelPlugin

VERSIONS = {'baseline': 0, 'mean_adjusted': 1, 'mean_provided2': 2}
PREP_VERSION = (0, 1, 2, 1)     # tdg_cgan_prep's version per version code: 3 (y_bar fed behind e1) has mean_adjusted's target
SRC, CROP = 65, 29
FULL_OFFSET = 18                 # paper_fullimage.py:138 places the 29x29 output at +18 (training crops the target at +17)
FULL_MIN_SIDE = SRC + CROP       # 94: the smallest frame side with one window
FULL_RMSE_BLOCKS = 256           # tdg_cgan_full_rmse's workspace, in doubles
METRIC_KEYS = ('abs_rel_diff', 'squared_rel_diff', 'linear_rmse', 'log_rmse', 'scale_invariant_log_rmse',
               'threshold1', 'threshold2', 'threshold3')


class GeneratorReplica(engine.Replica):
    """The generator half of the thesis' depth plugins, with no critic: the generator builders, the replica's buffers, the
    generator pass and its backward pass from dL/dg, the Eigen metric sets, the dataset evaluation and the full-frame
    inference.  paper_standalone / paper_baseline_standalone (models/standalone/) train it on a regression loss; CganReplica
    puts the critic on top.  Without a critic g and dL/dg live in two small buffers of the replica's own, and tdg_cgan_prep
    writes its depth target into a scratch buffer.  Not a `ModelPlugin` subclass, so the plugin scan registers only the
    plugins themselves.  A plugin supplies `name`, `arguments()` and `train()`, and may override `generator`."""

    NOISE_KEYS = None                # injection keys of the generator's noise nodes (unet.UNet's `noise_keys`)
    VERSIONS = VERSIONS              # --model_version -> code; 3 (models/standalone/): mean_adjusted's target, y_bar fed behind e1

    # ------------------------------------------------------------------------------ builders
    @classmethod
    def _version_name(cls, args):
        """The row of the module docstring's table this plugin runs."""
        return args.model_version

    @classmethod
    def check_version(cls, version):
        if version == 'mean_provided':
            raise ValueError("paper_cgan --model_version mean_provided cannot be built: the reference's g_mean_provided "
                             "calls tf.variablpe_scope (hem/models/paper_cgan.py:245) and raises AttributeError")
        if version not in VERSIONS:
            raise ValueError('paper_cgan: unknown --model_version %r' % version)

    @staticmethod
    def generator(x, args, reuse=False):
        """g_baseline (:212-243) and g_mean_provided2 (:277-310): x [B,65,65,3|4] -> the 31x31x1 head, cropped to 29x29
        by the executor.  Returns (d4 output, the records of the decoder concats)."""
        B = args.batch_size
        with variable_scope('encoder'), arg_scope([conv2d], reuse=reuse, filter_size=5, stride=2, padding='VALID', init='xavier',
                                                  activation=relu):
            e1 = conv2d(x, x.shape[-1], 64, name='e1')          # 31x31x64
            e2 = conv2d(e1, 64, 128, name='e2')                 # 14x14x128
            e3 = conv2d(e2, 128, 256, name='e3')                # 5x5x256
            e4 = conv2d(e3, 256, 512, name='e4')                # 1x1x512
        with variable_scope('decoder'), arg_scope([deconv2d, conv2d], reuse=reuse, filter_size=5, stride=2, init='xavier',
                                                  padding='VALID', activation=_lrelu(0.2)):
            y = deconv2d(e4, 512, 256, output_shape=(B, 256, 5, 5), name='d1')
            c1 = y = concat([y, e3])                           # 5x5x512
            y = deconv2d(y, 512, 128, output_shape=(B, 128, 14, 14), name='d2')
            c2 = y = concat([y, e2])                           # 14x14x256
            y = deconv2d(y, 256, 64, output_shape=(B, 64, 31, 31), name='d3')
            c3 = y = concat([y, e1])                           # 31x31x128
            y = conv2d(y, 128, 1, stride=1, filter_size=1, padding='SAME', activation=None, name='d4')   # 31x31x1
        return y, (c1, c2, c3)

    @classmethod
    def record_critic(cls, xs, args, mp2):
        """The critic's networks behind the generator's, for the plugins that have one."""

    @classmethod
    def build_graph(cls, args):
        """Record the networks for `args` (no device work); returns the Nets by scope name."""
        cls.check_version(cls._version_name(args))
        mp2 = cls._version_name(args) == 'mean_provided2'
        reset_graph()
        xs = placeholder((None, SRC, SRC, 3))
        gx = concat([xs, placeholder((None, SRC, SRC, 1), 'ones')]) if mp2 else xs
        with variable_scope('generator'):
            cls.generator(gx, args)
        cls.record_critic(xs, args, mp2)
        from ...ops import layers as Lyr
        return {k: v for k, v in Lyr._nets.items() if v.passes}

    # ------------------------------------------------------------------------------ construction
    def __init__(self, x_y, args, sess=None):
        engine.Replica.__init__(self, args, sess)
        self.x_y, sess = x_y, self.sess
        for flag, default in self._defaults().items():
            if not hasattr(args, flag):
                setattr(args, flag, default)
        self.check_version(self._version_name(args))
        self.version = self.VERSIONS[self._version_name(args)]
        B = self.B = args.batch_size
        dev, dt = sess.device, sess.dtype
        for _ in tower_scope_range(None, args.n_gpus, B, sess):
            nets = self.build_graph(args)
        self.enet, self.dec_net = nets['generator/encoder'], nets['generator/decoder']

        self.ws = K.Workspace(dev)
        self.g_store = engine.ParamStore(dev)
        mp2 = self.version == 2
        self.rgb_x = self._build_critic(nets, args)          # the critic's rgb input (None: no critic)
        # G input: D's rgb input where the two are the same tensor (baseline, mean_adjusted)
        self.gx = K.Act(B, SRC, SRC, 4, dt, dev) if mp2 else (K.Act(B, SRC, SRC, 3, dt, dev) if self.rgb_x is None else self.rgb_x)
        # G: the U-Net hands over its last concat [d3 | e1]; the 1x1 head on the 29x29 crop is _generate / _g_backward
        self.G = UNet(self.enet, self.dec_net, B, dt, dev, self.g_store, self.ws, self.gx, sess=sess, noise_keys=self.NOISE_KEYS)
        self.head = self.dec_net.layers[-1]
        head_noise = 1 if self.G.head_u is not None else 0          # the head reads its draw / fed plane beside the concat
        if len(self.dec_net.layers) != self.G.nd + 1 or \
                (self.head.k, self.head.out_size, self.head.in_size) != (1, 1, self.G.top.c + head_noise):
            raise ValueError('the generator head must be a 1x1 conv from the last concat to one channel')
        self.head_ws = torch.zeros(B * (self.head.in_size + 1), dtype=torch.float32, device=dev)
        self.fake, self.dfake = self._g_buffers()
        self._allocate()
        gen = torch.Generator().manual_seed(sess.seed)
        self.G.init_variables(gen)
        self._setup(args, gen)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x_stage, self.y_stage = self.staging((B, SRC, SRC, 3), (B, SRC, SRC, 1))
        self.ybar, self.crop, self.yhat = f32(B), f32(B, CROP, CROP), f32(B, CROP, CROP)     # of the last loss fetch
        self.inf_ybar, self.inf_crop, self.inf_yhat = f32(B), f32(B, CROP, CROP), f32(B, CROP, CROP)   # infer()'s own
        self.scal = f32(8)
        # streaming threshold totals of tf.metrics.percentage_below, one per metric set: hits 1..3, elements
        self.counts = {k: torch.zeros(4, dtype=torch.int64, device=dev) for k in ('y_hat', 'y_0')}
        self.metric_out = f32(8)
        self.metric_ws = torch.zeros(_lib.load().tdg_cgan_metrics_workspace_bytes(), dtype=torch.uint8, device=dev)
        self._full = {}                                      # _frame_buffers' cache: (H, W, stride) of infer_full, (H, W, stride, draws) of sample_full
        # dataset evaluation (tdg_cgan_eval.hip): the mean image of metrics_y_mean with its own streaming totals (row 2 of
        # [set, 4]), and evaluate()'s accumulators, totals and results
        lib = _lib.load()
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
        self.mean_image = None
        self.mean_counts = torch.zeros(3, 4, dtype=torch.int64, device=dev)
        self.eval_acc = f64(lib.tdg_cgan_eval_acc_bytes(CROP * CROP) // 8)
        self.eval_counts = torch.zeros(3, 4, dtype=torch.int64, device=dev)
        self.eval_scalars = f64(3, 12)
        self.eval_mean, self.eval_var = f32(CROP, CROP), f32(CROP, CROP)
        self.eval_ws = torch.zeros(lib.tdg_cgan_eval_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.refresh()

    @classmethod
    def _defaults(cls):
        return {k.lstrip('-'): v['default'] for k, v in cls.arguments().items()}

    # ---- what a critic changes (CganReplica) -----------------------------------------------------------------
    def _build_critic(self, nets, args):
        """No critic: tdg_cgan_prep's depth target goes to a scratch buffer that nothing reads."""
        self.prep_scratch = K.Act(self.B, CROP, CROP, 2 if self.version == 2 else 1, self.sess.dtype, self.sess.device)
        return None

    def _g_buffers(self):
        """Where g lands and where dL/dg is read from, channel 0 of each: two small buffers of the replica's own."""
        B, dt, dev = self.B, self.sess.dtype, self.sess.device
        return K.Act(B, CROP, CROP, 1, dt, dev), K.Act(B, CROP, CROP, 1, dt, dev)

    def _allocate(self):
        self.g_store.allocate()

    def _setup(self, args, gen):
        """After the generator's variables are initialised from `gen`: further variables, the optimizers, register()."""
        raise NotImplementedError

    def _prep_targets(self):
        """tdg_cgan_prep's device targets: (depth_real, its channel stride, depth_fake, rgb y_bar channel, its stride)."""
        return self.prep_scratch.ptr(0), self.prep_scratch.cs, self.fake.ptr(0) if self.version == 2 else None, None, 0

    # ---- pieces ------------------------------------------------------------------------------------------
    def _inputs(self, ybar, crop, x_src=None, y_src=None):
        """x into G's (and D's rgb) input, the depth target and the constant channels (:83-96, :286, :323, :326);
        y_bar and the f32 crop into `ybar` / `crop`.  x_src / y_src: f32 batches other than the staged one."""
        B, dt = self.B, self.sess.dtype
        rows = B * SRC * SRC
        x = K.ptr(self.x_stage if x_src is None else x_src)
        if self.rgb_x is not None:
            _lib.call('tdg_affine_cast_rows', dt, x, rows, 3, self.rgb_x.cs, 1.0, 0.0, self.rgb_x.ptr(0), K.stream())
        if self.gx is not self.rgb_x:
            _lib.call('tdg_affine_cast_rows', dt, x, rows, 3, self.gx.cs, 1.0, 0.0, self.gx.ptr(0), K.stream())
        if self.G.xn is not None:                                # noise at x: the generator reads [x | noise] from its own buffer
            _lib.call('tdg_affine_cast_rows', dt, x, rows, 3, self.G.xn.cs, 1.0, 0.0, self.G.xn.ptr(0), K.stream())
        self._target(ybar, crop, y_src)
        for win in self.G.fed.get('y_bar', ()):                  # mean_provided's fed channel, and the plane the head reads
            _lib.call('tdg_cgan_bar_fill', dt, K.ptr(ybar), B, win.h * win.w, win.ptr(0), win.cs, K.ptr(self.G.head_u), K.stream())

    def _target(self, ybar, crop, y_src=None):
        """The depth half of _inputs: the staged y into the depth target, y_bar and the f32 crop."""
        B, dt, mp2 = self.B, self.sess.dtype, self.version == 2
        dreal, dcs, dfake, rgb_bar, rgb_cs = self._prep_targets()
        _lib.call('tdg_cgan_prep', dt, K.ptr(self.y_stage if y_src is None else y_src), B, PREP_VERSION[self.version], dreal, dcs,
                  dfake, K.ptr(ybar), K.ptr(crop), self.gx.window(3, 1).ptr(0) if mp2 else None, self.gx.cs, rgb_bar, rgb_cs,
                  K.stream())

    def _generate(self, ybar, yhat, g32=None):
        """g (the cropped 1x1 head of the U-Net's last concat) into channel 0 of D's fake depth input, y_hat = g (+ y_bar,
        :113-121) into `yhat` (f32).  g32: also g as f32 [B,29,29]; that, or a head with a noise channel, takes the head's
        other entry point."""
        self.G.forward()
        c3, st, name = self.G.top, self.g_store, self.dec_net.var_name
        if g32 is not None or self.G.head_u is not None:
            _lib.call('tdg_cgan_head_noise_fwd', self.sess.dtype, c3.ptr(), self.B, c3.h, c3.c, c3.cs, CROP,
                      K.ptr(st[name(self.head, 'weights')]), K.ptr(st[name(self.head, 'bias')]), K.ptr(self.G.head_u),
                      K.ptr(ybar if self.version != 0 else None), K.ptr(yhat), K.ptr(g32), self.fake.ptr(0), self.fake.cs, K.stream())
            return
        _lib.call('tdg_cgan_head_fwd', self.sess.dtype, c3.ptr(), self.B, c3.h, c3.c, c3.cs, CROP, K.ptr(st[name(self.head, 'weights')]),
                  K.ptr(st[name(self.head, 'bias')]), K.ptr(ybar if self.version != 0 else None), K.ptr(yhat), self.fake.ptr(0),
                  self.fake.cs, K.stream())

    def _g_backward(self):
        """From dL/dg in channel 0 of D's fake depth-input gradient: the head writes the last concat's gradient
        [delta of d3 | dL/de1 from the skip] (the lrelu mask of d3 applied here, its producer), the U-Net takes it from there."""
        c3, gc3, st, name = self.G.top, self.G.gtop, self.g_store, self.dec_net.var_name
        if self.G.head_u is not None:
            _lib.call('tdg_cgan_head_noise_bwd', self.sess.dtype, self.dfake.ptr(0), self.dfake.cs, c3.ptr(), self.B, c3.h, c3.c, c3.cs,
                      CROP, K.ptr(st[name(self.head, 'weights')]), K.ptr(self.G.head_u), K.MASK_LRELU, self.dec_net.layers[-2].act.leak,
                      gc3.ptr(), K.ptr(st.grad(name(self.head, 'weights'))), K.ptr(st.grad(name(self.head, 'bias'))),
                      K.ptr(self.head_ws), self.head_ws.numel() * 4, K.stream())
        else:
            _lib.call('tdg_cgan_head_bwd', self.sess.dtype, self.dfake.ptr(0), self.dfake.cs, c3.ptr(), self.B, c3.h, c3.c, c3.cs, CROP,
                      K.ptr(st[name(self.head, 'weights')]), K.MASK_LRELU, self.dec_net.layers[-2].act.leak, gc3.ptr(),
                      K.ptr(st.grad(name(self.head, 'weights'))), K.ptr(st.grad(name(self.head, 'bias'))),
                      K.ptr(self.head_ws), self.head_ws.numel() * 4, K.stream())
        self.G.backward()

    # ---- event files ---------------------------------------------------------------------------------------
    def summary_items(self):
        """engine.Replica's weights and gradients, and the generator's activations under `g_activations/<scope>/<layer>`
        (hem/models/paper_cgan.py:170,172): the U-Net's encoder and decoder outputs -- channel windows of its zero-copy concat
        buffers -- and the head's g, which exists as the 29x29 crop only.  They hold what the last generator pass left."""
        items = engine.Replica.summary_items(self)
        G = self.G
        items += [('g_activations/%s/%s' % (self.enet.name, self.enet.layers[k - 1].name), G.e_h[k], 1.0) for k in range(1, G.n + 1)]
        items += [('g_activations/%s/%s' % (self.dec_net.name, self.dec_net.layers[i - 1].name), G.d_h[i], 1.0) for i in range(1, G.nd + 1)]
        items.append(('g_activations/%s/%s' % (self.dec_net.name, self.head.name), self.fake.window(0, 1), 1.0))
        return items

    def montage_items(self):
        """hem.summarize_layers(..., montage=True) (hem/models/paper_cgan.py:172-173): image 0 of every activation of
        summary_items(), 1x1 layers included, under `<its tag>/montage`."""
        return self._activation_montage_items()

    # ---- evaluation ----------------------------------------------------------------------------------------
    def metrics(self):
        """The Eigen-2014 sets `metrics_y_hat` and `metrics_y_0` (:171-172, :447-478) of the last loss fetch's batch.
        Each call is one evaluation of the streaming threshold metrics."""
        out = {}
        y_0 = self.ybar if self.version != 0 else None          # y_0 = 0 (baseline) or y_bar
        for name, pred, off in (('y_hat', self.yhat, None), ('y_0', None, y_0)):
            _lib.call('tdg_cgan_metrics', K.ptr(self.crop), K.ptr(pred), K.ptr(off), self.B, CROP * CROP, K.ptr(self.counts[name]),
                      K.ptr(self.metric_out), K.ptr(self.metric_ws), self.metric_ws.numel(), K.stream())
            out['metrics_' + name] = dict(zip(METRIC_KEYS, self.metric_out.cpu().tolist()))
        if self.mean_image is not None:                          # metrics_y_mean (:79, :177): 10 * mean image, no y_bar added
            self.eval_acc.zero_()
            self._eval_batch(self.crop, None, None, self.mean_image, 4, self.mean_counts)
            out['metrics_y_mean'] = dict(zip(METRIC_KEYS, self.eval_acc[18:26].float().cpu().tolist()))
        return out

    def set_mean_image(self, img01):
        """The reference's mean_image_placeholder: a [29,29] or [1,29,29] depth image in [0, 1] (dataset_moments' mean), kept
        on the device; while one is set, metrics() also reports `metrics_y_mean`.  None clears it."""
        if img01 is None:
            self.mean_image = None
            return
        img = torch.as_tensor(img01).to(device=self.sess.device, dtype=torch.float32)
        if tuple(img.shape) not in ((CROP, CROP), (1, CROP, CROP)):
            raise ValueError('set_mean_image: expected [%d,%d] or [1,%d,%d], got %s' % (CROP, CROP, CROP, CROP, tuple(img.shape)))
        self.mean_image = img.reshape(CROP, CROP).contiguous().clone()

    def _eval_batch(self, crop, yhat, y_0, image01, sets, counts):
        """tdg_cgan_eval_batch of one batch into self.eval_acc: sets 1 (yhat), 2 (y_0, None: zero), 4 (10 * image01)."""
        _lib.call('tdg_cgan_eval_batch', K.ptr(crop), K.ptr(yhat), K.ptr(y_0), K.ptr(image01), 10.0, self.B, CROP * CROP, sets,
                  K.ptr(counts), K.ptr(self.eval_acc), K.ptr(self.eval_ws), self.eval_ws.numel(), K.stream())

    def _eval_finish(self, images):
        _lib.call('tdg_cgan_eval_finish', K.ptr(self.eval_acc), K.ptr(self.eval_counts), CROP * CROP, 10.0, K.ptr(self.eval_scalars),
                  K.ptr(self.eval_mean) if images else None, K.ptr(self.eval_var) if images else None, K.stream())

    def _eval_sweep(self, source, n_batches, name, body, both=True):
        """`body` once per batch of `source`, graph-replayed, on the batch staged at fixed addresses."""
        for _ in range(n_batches):
            batch = source.next_batch()
            if both:
                self._stage(batch)
            else:
                self.y_stage.copy_(batch[1].reshape(self.y_stage.shape))
            self._run(name, body)

    def _eval_model_body(self):
        """Sweep 1: infer()'s path, then y_hat, y_0 and the moments from one read of the crop."""
        self._inputs(self.inf_ybar, self.inf_crop)
        self._generate(self.inf_ybar, self.inf_yhat)
        self._eval_batch(self.inf_crop, self.inf_yhat, self.inf_ybar if self.version != 0 else None, None, 3, self.eval_counts)
        self._moments_body(prep=False)

    def _eval_mean_body(self):
        """Sweep 2: no generator pass; the mean image of sweep 1 against this batch's crop."""
        self._target(self.inf_ybar, self.inf_crop)
        self._eval_batch(self.inf_crop, None, None, self.eval_mean, 4, self.eval_counts)

    def _moments_body(self, prep=True):
        if prep:
            self._target(self.inf_ybar, self.inf_crop)
        _lib.call('tdg_cgan_eval_moments', K.ptr(self.inf_crop), self.B, CROP * CROP, K.ptr(self.eval_acc), K.stream())

    @staticmethod
    def _check_sweep(what, n_batches):
        if int(n_batches) < 1:
            raise ValueError('%s: n_batches must be at least 1, got %r' % (what, n_batches))
        return int(n_batches)

    def dataset_moments(self, source, n_batches):
        """(mean_img, var_img), NumPy f32 [29,29]: tf.nn.moments over the batch axis of the [0, 1] depth crop of each of
        `n_batches` batches of `source`, averaged over the batches (paper_train.py:43-50, :130-132)."""
        n_batches = self._check_sweep('dataset_moments', n_batches)
        self.eval_acc.zero_()
        self._eval_sweep(source, n_batches, 'eval_moments', self._moments_body, both=False)
        self._eval_finish(True)
        return self.eval_mean.cpu().numpy(), self.eval_var.cpu().numpy()

    def evaluate(self, source, n_batches):
        """paper_metrics.py's calculate_metrics over `n_batches` batches of `source`, twice: sweep 1 evaluates the model's
        y_hat (`model`) and y_0 = 0 / y_bar (`zero`) and takes the moments; sweep 2, on the next n_batches batches, evaluates
        the mean image of sweep 1 (`mean`).  Each set: METRIC_KEYS averaged over the batches (thresholds: the mean of the
        running percentage, :24-34,119-130) plus `threshold{1,2,3}_final`, the totals' percentages; the totals start at zero
        in every call.  Also `mean_image` / `var_image` (NumPy f32 [29,29], [0, 1] units), `n_batches`, `images`.
        One host read; training state, metrics() and its buffers are untouched."""
        n_batches = self._check_sweep('evaluate', n_batches)
        self.eval_acc.zero_()
        self.eval_counts.zero_()
        self._eval_sweep(source, n_batches, 'eval_model', self._eval_model_body)
        self._eval_finish(True)
        self._eval_sweep(source, n_batches, 'eval_mean', self._eval_mean_body, both=False)
        self._eval_finish(False)
        rows = self.eval_scalars.cpu().tolist()
        out = {}
        for name, r in zip(('model', 'zero', 'mean'), rows):
            out[name] = dict(zip(METRIC_KEYS, r[:8]))
            out[name].update({'threshold%d_final' % (k + 1): r[8 + k] for k in range(3)})
        out.update(mean_image=self.eval_mean.cpu().numpy(), var_image=self.eval_var.cpu().numpy(), n_batches=n_batches,
                   images=n_batches * self.B)
        return out

    def infer(self, batch):
        """y_hat [B,29,29,1] f32 of one (x, y) batch (y supplies y_bar for the mean-adjusted versions).  It has buffers of its
        own: metrics() keeps reporting the last loss fetch."""
        self._stage(batch)
        self._inputs(self.inf_ybar, self.inf_crop)
        self._generate(self.inf_ybar, self.inf_yhat)
        return self.inf_yhat.reshape(self.B, CROP, CROP, 1).clone()

    # ---- full-frame inference (paper_fullimage.py) -----------------------------------------------------------
    def infer_full(self, image, depth, stride=10, offset=FULL_OFFSET):
        """The 65x65 window slid over a whole frame at `stride` (build_batch / reconstruct / rmse of paper_fullimage.py:90-163).

        image f32 [H,W,3] and depth f32 [H,W] or [H,W,1] in [0, 1] (torch or NumPy).  Every window runs through infer()'s
        path (depth feeds y_bar only) in chunks of batch_size, one graph-replayed body per chunk; the 29x29 outputs are
        blended into frame canvases at +offset, in the reference's order.  Returns a FullFrame: y_hat and g canvases
        (device f32 [H,W]), the frame RMSE, the patch count and the grid (cols, rows)."""
        image, depth = self._frame(image, depth)
        H, W = int(image.shape[0]), int(image.shape[1])
        fb, grid = self._frame_sweep('infer_full', image, depth, stride, offset, (H, W, stride), 'full_%d_%d_%d' % (H, W, stride),
                                     self.B, self._full_chunk)
        return FullFrame(fb.yhat.clone(), fb.g.clone(), float(fb.rmse.item()), grid.patches, (grid.cols, grid.rows))

    def _frame(self, image, depth):
        dev = self.sess.device
        image = torch.as_tensor(image).to(device=dev, dtype=torch.float32)
        depth = torch.as_tensor(depth).to(device=dev, dtype=torch.float32)
        if depth.dim() == 3 and depth.shape[-1] == 1:
            depth = depth[..., 0]
        if image.dim() != 3 or image.shape[-1] != 3 or tuple(depth.shape) != tuple(image.shape[:2]):
            raise ValueError('infer_full: image must be [H,W,3] and depth [H,W] or [H,W,1], got %s and %s'
                             % (tuple(image.shape), tuple(depth.shape)))
        return image, depth

    def _frame_sweep(self, what, image, depth, stride, offset, key, name, per_chunk, body, extras=None, rmse=True):
        """The whole-frame sweep that infer_full and sample_full share, on a frame _frame() has checked: the grid and the
        offset check (errors prefixed `what`), the frame into its buffers, `body(fb, H, W, stride)` once per chunk of
        `per_chunk` windows as the graph `name`, the blend of the y_hat store into the y_hat / g canvases and (`rmse`) the
        frame RMSE.  Returns (buffers, grid); `key` and `extras` are _frame_buffers'."""
        H, W = int(image.shape[0]), int(image.shape[1])
        grid = patch_grid(H, W, stride)
        if grid.patches == 0:
            raise ValueError('%s: no %dx%d window fits a %dx%d frame at stride %d' % (what, SRC, SRC, H, W, stride))
        if not 0 <= offset <= SRC - CROP:
            raise ValueError('%s: offset %d outside [0, %d]' % (what, offset, SRC - CROP))
        fb = self._frame_buffers(key, H, W, grid, per_chunk, extras)
        fb.image.copy_(image)
        fb.depth.copy_(depth)
        fb.chunk.zero_()
        for _ in range(fb.n_chunks):
            self._run(name, lambda: body(fb, H, W, stride))
        self._blend(fb, fb.store_yhat, fb.store_ybar, H, W, stride, offset, fb.yhat, fb.g)
        if rmse:
            _lib.call('tdg_cgan_full_rmse', K.ptr(fb.depth), K.ptr(fb.yhat), H, W, K.ptr(fb.rmse), K.ptr(fb.rmse_ws),
                      fb.rmse_ws.numel() * 8, K.stream())
        return fb, grid

    @staticmethod
    def _blend(fb, store, store_bar, H, W, stride, offset, canvas, canvas_g):
        _lib.call('tdg_cgan_full_blend', K.ptr(store), K.ptr(store_bar), fb.slots, H, W, stride, offset, K.ptr(canvas), K.ptr(canvas_g),
                  K.stream())

    def _frame_buffers(self, key, H, W, grid, per_chunk, extras=None):
        """Frame-sized buffers, allocated once per `key`: the frame itself, the patch store of n_chunks * per_chunk slots, the
        two canvases and the RMSE workspace (fixed addresses: the chunk body is graph-captured), plus the caller's
        `extras(slots, f32)`: a dict of further fields."""
        if key in self._full:
            return self._full[key]
        dev = self.sess.device
        n_chunks = -(-grid.patches // per_chunk)
        slots = n_chunks * per_chunk
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        fb = self._full[key] = _FullBuffers(
            n_chunks=n_chunks, slots=slots, image=f32(H, W, 3), depth=f32(H, W), chunk=torch.zeros(1, dtype=torch.int32, device=dev),
            store_yhat=f32(slots, CROP, CROP), store_ybar=f32(slots), yhat=f32(H, W), g=f32(H, W),
            rmse=torch.zeros(1, dtype=torch.float64, device=dev), rmse_ws=torch.zeros(FULL_RMSE_BLOCKS, dtype=torch.float64, device=dev),
            **(extras(slots, f32) if extras else {}))
        return fb

    def _full_chunk(self, fb, H, W, stride):
        """One chunk: its windows into the staging buffers, infer()'s path, its outputs into the store; advances fb.chunk."""
        _lib.call('tdg_cgan_full_gather', K.ptr(fb.image), K.ptr(fb.depth), H, W, stride, K.ptr(fb.chunk), self.B,
                  K.ptr(self.x_stage), K.ptr(self.y_stage), K.stream())
        self._inputs(self.inf_ybar, self.inf_crop)
        self._generate(self.inf_ybar, self.inf_yhat)
        _lib.call('tdg_cgan_full_store', K.ptr(self.inf_yhat), K.ptr(self.inf_ybar) if self.version != 0 else None, self.B, fb.slots,
                  K.ptr(fb.chunk), K.ptr(fb.store_yhat), K.ptr(fb.store_ybar), K.stream())


class CganReplica(GeneratorReplica):
    """What the thesis' depth cGAN plugins share (paper_cgan here, paper_sampler / paper_noise in models/sampler/):
    GeneratorReplica with the critic on top -- D's builder and networks, the join, the losses, the D and G steps.  g lands in
    D's fake depth input and dL/dg is read from that input's gradient."""

    @staticmethod
    def discriminator(x, y, args, reuse=False):
        """d_baseline (:312-338) / d_mean_provided2 (:362-388, x and y already carry their y_bar channel).
        Returns the logits [B,1,1,1] and the two path outputs."""
        with arg_scope([conv2d], reuse=reuse, activation=_lrelu(0.2), init='xavier', padding='VALID', filter_size=5, stride=2):
            with variable_scope('rgb_path'):
                h1 = conv2d(x, x.shape[-1], 64, name='hx1')     # 31x31x64
                h1 = conv2d(h1, 64, 128, name='hx2')            # 14x14x128
                h1 = conv2d(h1, 128, 256, name='hx3')           # 5x5x256
                h1 = conv2d(h1, 256, 512, name='hx4')           # 1x1x512
            with variable_scope('depth_path'):
                h2 = conv2d(y, y.shape[-1], 128, name='hy1')    # 13x13x128 (the reference's "14x14" comment at :326 is off)
                h2 = conv2d(h2, 128, 256, name='hy2')           # 5x5x256
                h2 = conv2d(h2, 256, 512, name='hy3')           # 1x1x512
            with variable_scope('combined_path'):
                h = concat([h1, h2])                            # 1x1x1024
                h = conv2d(h, 1024, 1024, stride=1, filter_size=1, padding='SAME', name='h1')
                h = conv2d(h, 1024, 512, stride=1, filter_size=1, padding='SAME', name='h2')
                h = conv2d(h, 512, 1, stride=1, filter_size=1, padding='SAME', name='h3', activation=None)
        return h, h1, h2

    @classmethod
    def record_critic(cls, xs, args, mp2):
        rx = concat([xs, placeholder((None, SRC, SRC, 1), 'y_bar')]) if mp2 else xs
        dy = placeholder((None, CROP, CROP, 2 if mp2 else 1), 'y')
        with variable_scope('discriminator'):
            cls.discriminator(rx, dy, args, reuse=False)             # D(x, y_hat) first, as :123-136
            cls.discriminator(rx, dy, args, reuse=True)

    # ------------------------------------------------------------------------------ construction
    S_GFAKE, S_DFAKE, S_DREAL, S_DTOTAL = 0, 1, 2, 3

    def _build_critic(self, nets, args):
        B, dev, dt, mp2 = self.B, self.sess.device, self.sess.dtype, self.version == 2
        self.wgan = getattr(args, 'training_version', 'gan') == 'wgan'
        rgb_net, depth_net, comb_net = (nets['discriminator/' + s] for s in ('rgb_path', 'depth_path', 'combined_path'))
        self.d_store = engine.ParamStore(dev)
        # D: combined path over 2B (images [0,B) real, [B,2B) fake), depth path over 2B, rgb path over B
        self.Dc = engine.SeqNet(comb_net, 2 * B, (1, 1, 1024), dt, dev, self.d_store, need_input_grad=True, ws=self.ws)
        self.Dr = engine.SeqNet(rgb_net, B, (SRC, SRC, 4 if mp2 else 3), dt, dev, self.d_store, ws=self.ws)
        self.Dd = engine.SeqNet(depth_net, 2 * B, (CROP, CROP, 2 if mp2 else 1), dt, dev, self.d_store, need_input_grad=True,
                                ws=self.ws)
        for net in (self.Dr, self.Dd, self.Dc):
            net.declare_variables()
        self.rgb_g = self.Dr.layers[-1].gout                 # dL/d(rgb path output): both halves summed by tdg_cgan_join
        self.depth_g = self.Dd.layers[-1].gout
        return self.Dr.x

    def _g_buffers(self):
        return self.Dd.x.view(self.B, self.B), self.Dd.dx.view(self.B, self.B)      # g lands in D's fake depth input

    def _allocate(self):
        self.d_store.allocate()
        self.g_store.allocate()

    def _setup(self, args, gen):
        for net in (self.Dr, self.Dd, self.Dc):
            net.init_variables(gen)
        if self.wgan:                                        # :64-66
            self.g_opt = engine.RMSProp(self.g_store, args.g_lr, decay=0.9, momentum=0.0, eps=1e-10)
            self.d_opt = engine.Adam(self.d_store, args.d_lr)
        else:                                                # :67-69
            self.g_opt = engine.Adam(self.g_store, args.g_lr, args.g_beta1, args.g_beta2)
            self.d_opt = engine.Adam(self.d_store, args.d_lr, args.d_beta1, args.d_beta2)
        self.register('generator', self.g_store, self.g_opt, self.G.repack)
        self.register('discriminator', self.d_store, self.d_opt, self._repack_d)

    def _repack_d(self):
        for net in (self.Dr, self.Dd, self.Dc):
            net.repack()

    def _prep_targets(self):
        mp2 = self.version == 2
        return (self.Dd.x.ptr(0), self.Dd.x.cs, self.Dd.x.ptr(self.B) if mp2 else None,
                self.Dr.x.window(3, 1).ptr(0) if mp2 else None, self.Dr.x.cs)

    def summary_items(self):
        """GeneratorReplica's, and under `d_activations/<scope>/<layer>` every layer output of the critic's three paths
        (hem/models/paper_cgan.py:171,173): the rgb path over the B images, the depth and combined paths over the real and
        the fake half together."""
        items = GeneratorReplica.summary_items(self)
        for net in (self.Dr, self.Dd, self.Dc):
            items += [('d_activations/%s/%s' % (net.net.name, L.spec.name), L.out if L.rowdot else L.h, 1.0) for L in net.layers]
        return items

    # ---- pieces ------------------------------------------------------------------------------------------
    def _d_forward(self):
        B, dt = self.B, self.sess.dtype
        self.Dr.forward(0, B)
        self.Dd.forward(0, 2 * B)
        rh, dh = self.Dr.layers[-1].h, self.Dd.layers[-1].h
        _lib.call('tdg_cgan_join', dt, 0, B, 2 * B, 512, self.Dc.x.ptr(0), self.Dc.x.cs, rh.ptr(0), rh.cs, dh.ptr(0), dh.cs, K.stream())
        self.Dc.forward(0, 2 * B)

    def _loss(self, mode):
        last = self.Dc.layers[-1]
        if self.wgan:
            _lib.call('tdg_cgan_wgan_loss', self.sess.dtype, last.h.ptr(0), self.B, last.h.cs, mode, last.gout.ptr(0),
                      K.ptr(self.scal), K.stream())
        else:        # tdg_p2p_xent writes d_real, d_fake, g_fake to scal[0..2] of the pointer, here self.scal[4..6] (_losses)
            _lib.call('tdg_p2p_xent', self.sess.dtype, last.h.ptr(0), self.B, last.h.cs, mode, last.gout.ptr(0),
                      K.ptr(self.scal, 16), K.stream())

    def _clip(self, store, repack):
        """--wgan_clip c (opt-in; :181-187 never runs in the reference): clamp before the step."""
        c = float(getattr(self.args, 'wgan_clip', 0.0) or 0.0)
        if self.wgan and c > 0.0:
            _lib.call('tdg_clamp', K.ptr(store.params), store.size, -c, c, K.stream())
            repack()

    # ---- steps ---------------------------------------------------------------------------------------------
    def d_step(self, batch):
        self._stage(batch)
        self.optimizer_step(self.d_store, ('d_grads', self._d_grads), ('d_apply', self._d_apply), 'd_step')

    def _d_grads(self):
        B, dt = self.B, self.sess.dtype
        self._clip(self.d_store, self._repack_d)
        self._inputs(self.ybar, self.crop)
        self._generate(self.ybar, self.yhat)
        self._d_forward()
        self._loss(1)
        self.Dc.backward(0, 2 * B, want_params=True, want_dx=True)
        dx = self.Dc.dx
        _lib.call('tdg_cgan_join', dt, 1, B, 2 * B, 512, dx.ptr(0), dx.cs, self.rgb_g.ptr(0), self.rgb_g.cs, self.depth_g.ptr(0),
                  self.depth_g.cs, K.stream())
        self.Dd.backward(0, 2 * B, want_params=True)
        self.Dr.backward(0, B, want_params=True)

    def _d_apply(self):
        self.d_opt.step(self._scale)
        self._repack_d()

    def g_step(self, batch):
        self._stage(batch)
        self.optimizer_step(self.g_store, ('g_grads', self._g_grads), ('g_apply', self._g_apply), 'g_step')

    def _g_grads(self):
        """The G step and the loss fetch of one sess.run (:208): D runs on both halves, the losses are this batch's."""
        B, dt = self.B, self.sess.dtype
        self._clip(self.g_store, self.G.repack)
        self._inputs(self.ybar, self.crop)
        self._generate(self.ybar, self.yhat)
        self._d_forward()
        self._loss(2)
        self.Dc.backward(B, B, want_params=False, want_dx=True)
        dx = self.Dc.dx
        _lib.call('tdg_cgan_join', dt, 1, B, B, 512, dx.ptr(B), dx.cs, None, 0, self.depth_g.ptr(B), self.depth_g.cs, K.stream())
        self.Dd.backward(B, B, want_params=False, want_dx=True)
        self._g_backward()

    def _g_apply(self):
        self.g_opt.step(self._scale)
        self.G.repack()

    # ---- held-out batches (train.py --validation; hem.inference, hem/util/misc.py:85-93) ---------------------------
    _STEP_BODIES = ('d_step', 'g_step', '_d_grads', '_g_grads', '_d_forward', '_loss', '_losses')

    @classmethod
    def has_validation(cls):
        """validation_losses / observe are built from CganReplica's own step bodies: a subclass that replaces one of them
        (models/sampler/) has no validation pass until it states its own."""
        return all(getattr(cls, m) is getattr(CganReplica, m) for m in CganReplica._STEP_BODIES)

    def _need_validation(self, what):
        if not self.has_validation():
            raise NotImplementedError('model %s has no validation pass (%s): it replaces step bodies of the depth cGAN'
                                      % (self._model_name(), what))

    def _forward_losses(self):
        """_g_grads without its backward half: inputs, generator, critic on both halves, the loss kernel."""
        self._clip(self.g_store, self.G.repack)
        self._inputs(self.ybar, self.crop)
        self._generate(self.ybar, self.yhat)
        self._d_forward()
        self._loss(2)

    def validation_losses(self, batch):
        """The loss dict of _losses() for one held-out batch, from a forward-only captured body.  Variables, optimizer
        slots, packed filters and step counters stay as they are (--wgan_clip's clamp, where asked for, runs as in the G
        step: it is idempotent).  metrics() then reports this batch."""
        self._need_validation('validation_losses')
        self._stage(batch)
        self._run('v_losses', self._forward_losses)
        return self._losses()

    def observe(self, batch):
        """The reference's summary op on a fed batch: the D and then the G gradient body of one step on `batch`, without
        either optimizer half, without the exchange between ranks and without a global_step increment.  Afterwards the
        activation, gradient and metric buffers hold this batch's values for write_event; variables, optimizer slots, packed
        filters and step counters stay as they are (--wgan_clip as in validation_losses).  Returns the losses."""
        self._need_validation('observe')
        self._stage(batch)
        self._run('d_grads', self._d_grads)
        self._run('g_grads', self._g_grads)
        return self._losses()

    def _losses(self):
        s = self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()
        r = self.sess.world_size - 1
        if self.wgan:                    # :396-403: the real mean is named 'd_fake' again -> 'd_fake_1'
            items = [('loss/generator/g_fake', s[0]), ('loss/discriminator/d_fake', s[1]), ('loss/discriminator/d_fake_1', s[2]),
                     ('loss/discriminator/d_total', s[3])]
        else:                            # :398-407 (scal[4..6] = d_real, d_fake, g_fake of tdg_p2p_xent)
            items = [('loss/generator/g_fake', s[6]), ('loss/discriminator/d_fake', s[5]), ('loss/discriminator/d_real', s[4]),
                     ('loss/discriminator/d_total', s[4] + s[5])]
        return collection_to_dict([('tower_%d/%s:0' % (r, n), v) for n, v in items])


class paper_cgan(ModelPlugin, CganReplica):
    name = 'paper_cgan'

    @staticmethod
    def arguments():
        """hem/models/paper_cgan.py:14-57."""
        return {
            '--g_lr': {'type': float, 'default': 1e-3, 'help': 'Learning rate for generator.'},
            '--d_lr': {'type': float, 'default': 1e-3, 'help': 'Learning rate for discriminator.'},
            '--g_beta1': {'type': float, 'default': 0.9, 'help': 'Beta1 for generator'},
            '--d_beta1': {'type': float, 'default': 0.9, 'help': 'Beta1 for discriminator.'},
            '--g_beta2': {'type': float, 'default': 0.999, 'help': 'Beta2 for generator.'},
            '--d_beta2': {'type': float, 'default': 0.999, 'help': 'Beta2 for discriminator.'},
            '--model_version': {'type': str, 'default': 'baseline',
                                'choices': ['baseline', 'mean_adjusted', 'mean_provided', 'mean_provided2'],
                                'help': 'Which version of the model to run.'},
            '--training_version': {'type': str, 'default': 'gan', 'choices': ['gan', 'wgan'],
                                   'help': 'Whether to use standard GAN training of Wasserstein GAN training.'},
        }

    def train(self, sess=None, args=None, feed_dict=None):
        """:200-209: gan -- one D step, then the G step and the loss fetch on the next batch; wgan -- five D steps first."""
        for _ in range(5 if self.wgan else 1):
            self.d_step(self.x_y.next_batch())
        self.g_step(self.x_y.next_batch())
        return self._losses()


class _FullBuffers:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class FullFrame:
    """infer_full's result: y_hat / g canvases (device f32 [H,W]), rmse (float), patches (P) and grid (cols, rows)."""

    def __init__(self, y_hat, g, rmse, patches, grid):
        self.y_hat, self.g, self.rmse, self.patches, self.grid = y_hat, g, rmse, patches, grid

    def __repr__(self):
        return 'FullFrame(%dx%d, patches=%d, grid=%s, rmse=%.6g)' % (self.y_hat.shape[0], self.y_hat.shape[1], self.patches,
                                                                     self.grid, self.rmse)


class PatchGrid(tuple):
    """(cols, rows) of the window grid of paper_fullimage.py's build_batch (:90-110), with the patch count and corners."""

    def __new__(cls, cols, rows, stride):
        t = tuple.__new__(cls, (cols, rows))
        t.stride = stride
        return t

    cols = property(lambda self: self[0])
    rows = property(lambda self: self[1])
    patches = property(lambda self: self[0] * self[1])

    def corner(self, c):
        """(top, left) of patch c: c = n * cols + m with n over rows (outer) and m over cols (inner) -> (m s, n s)."""
        if not 0 <= c < self.patches:
            raise IndexError('patch %d of %d' % (c, self.patches))
        n, m = divmod(c, self.cols)
        return m * self.stride, n * self.stride


def patch_grid(H, W, stride):
    """cols = (H - 93) // s windows down, rows = (W - 93) // s across (the reference's int((side - 65 - 29 + 1) / s)).
    ValueError for a frame smaller than 94 x 94 or a stride below 1; a grid may be empty (stride beyond the frame)."""
    H, W, stride = int(H), int(W), int(stride)
    if H < FULL_MIN_SIDE or W < FULL_MIN_SIDE:
        raise ValueError('patch_grid: a %dx%d frame is smaller than %dx%d' % (H, W, FULL_MIN_SIDE, FULL_MIN_SIDE))
    if stride < 1:
        raise ValueError('patch_grid: stride %d < 1' % stride)
    span = SRC + CROP - 1
    return PatchGrid((H - span) // stride, (W - span) // stride, stride)
