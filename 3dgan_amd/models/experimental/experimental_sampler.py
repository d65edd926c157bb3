"""Depth cGAN fed by the scene mean-depth estimator on MI355X -- the reference's gen-2 plugin
`hem/models/experimental_sampler.py` (arguments :16-43, __init__ :67-196, train :198-209, generatorE2 :213-248, discriminatorE2
:252-281, loss :284-324, sampler_summaries :377-397), driven by the reference's top-level `experimental.py`, on the HIP kernels.

Inputs (:107-149).  The batch is the 6-tuple of nyuv2 `--random_crop 64 64 --include_location --include_originals 53 70`:
(x [B,64,64,3], y [B,64,64,1], x_loc, y_loc [B,64,64,1], x_full [B,53,70,3], y_full).  x <- 2x - 1 and y <- 2y - 1 as hem.rescale
computes them in f32 (2x is exact: one rounding); y is cropped at (16, 16) to 32x32; x_loc / y_loc are used as they come, in
[0, 1]; m = stop_gradient(estimator.output_layer), one number per image from x_full in the same run, stacked to a 64x64 plane.
The generator and the critic read X = [x | x_loc | y_loc | m], 6 channels (tdg_xsamp_prep: one pass writes every input tensor).

    generator E2   [X | u], u ~ U(-1, 1) [B,64,64,1]                                  64x64x7
      encoder      e1..e4  conv2d 5x5 stride 2 SAME xavier relu     32x32x64, 16x16x128, 8x8x256, 4x4x512
                   e5      conv2d 4x4 stride 2 VALID relu           1x1x1024
      decoder      d1      deconv2d 4x4 stride 2 VALID lrelu 0.2    4x4x512,   concat e4 -> 4x4x1024
                   d2..d4  deconv2d 5x5 stride 2 SAME lrelu 0.2     8x8x256, 16x16x128, 32x32x64, each concat e3, e2, e1
                   d5      conv2d 1x1, 128 -> 1, tanh               32x32x1 (the reference's "31x31x1" comment at :247 is off)
    critic E2      rgb_path       X: hx1..hx4 5x5 stride 2 SAME, hx5 4x4 VALID, lrelu 0.2        -> 1x1x1024
                   depth_path     depth 32x32x1: hy1..hy3 5x5 stride 2 SAME, hy4 4x4 VALID       -> 1x1x1024
                   combined_path  1x1 convs 2048 -> 1024 -> 512 -> 256 -> 128 -> 64 -> 1, lrelu 0.2, none on h6

Variables: `generator/{encoder,decoder}/vars/<layer>/{weights,bias}`, `discriminator/{rgb_path,depth_path,combined_path}/vars/...`
and, registered beside them, the estimator's `model/vars/l*/...`.

Loss (:284-324): sigmoid cross-entropy g_fake, d_real, d_fake, d_total = d_real + d_fake; G is trained on g_fake ALONE.  The loss
dict holds g_fake, d_real, d_fake, d_total, rmse, l1 in that order; rmse and l1 compare (g + 1) / 2 with (y + 1) / 2.
`--g_rmse` and `--g_sparsity` are parsed, but the code that read them is commented out in the reference (:297-308): no effect.
`--g_arch` / `--d_arch`: only E2 exists (a KeyError in the reference, a ValueError naming the choices here).
Optimizers (:70-71): two instances of init_optimizer(args): the global --optimizer / --lr / --beta1 apply.

train() (:198-209) is ONE sess.run of [d_train_op, g_train_op, all_losses]: one batch, one noise draw, one forward pass, both
gradient sets taken at the variables before either update, the losses those of that pass, global_step advanced by 2.  Here: the
batch into the staging buffers; ONE captured gradient body (estimator forward, prep, G forward, head, the critic over 2B, xent
mode 1, the critic's backward pass for its parameters over both halves, xent mode 2, a data-only backward pass through the fake
half to dL/dg, head backward, U-Net backward, tdg_p2p_l1); the finite check and the exchange on both stores; ONE captured apply
body with both optimizer steps and both repacks.

The estimator.  Its variables are in neither optimizer's list: train() never changes them, nor its optimizer's slots.  Its
forward pass runs inside this model's captured bodies on this model's own staged copy of x_full; its output feeds
tdg_xsamp_prep and nothing flows back.  With `estimator=None` the model builds a mean_depth_estimator of its own from the same
args and session.  DEVIATION: with several towers the reference feeds every tower the LAST tower's output_layer (:119 reads the
estimator object after its tower loop), a slicing bug; here each rank's replica uses its own estimator output on its own rows.

metrics() (:142-160, :377-397): three more generator passes, each with a fresh noise channel -- `sampler` (row 0 of X, its m
included, and row 0 of y broadcast over the batch), `shuffled` (tf.random_shuffle(X): all six planes permuted together,
compared against the UNpermuted y) and `noise` (X replaced by U(-1, 1) of X's shape, compared against the sampler set's y) --
and per set `moments/<set>/moments/mean`, `/var` (the mean over the pixels of tf.nn.moments(g, axes=[0])) and
`per_image_metrics/<set>/rmse/mean`, `/min` (10 * the per-image mean |y - g| on the [-1, 1] tensors as written), plus the six
losses of the last fetch.  One graph-replayed body; the permutation is drawn on the host per call (injection key `shuffle`), the
noise set's input on the device (injection key `x_noise`).  It leaves the variables, the optimizers and the last fetch alone.
"""
import numpy as np
import torch

from ... import _lib
from ... import kernels as K
from ... import engine
from ...ops.layers import conv2d, deconv2d, concat, arg_scope, variable_scope, placeholder, random_uniform, reset_graph
from ...ops.activations import _lrelu, relu, tanh
from ...unet import UNet
from ...util import tower_scope_range, init_optimizer, collection_to_dict
from ..ModelPlugin import ModelPlugin
from ..estimator.mean_depth_estimator import mean_depth_estimator

SRC, CROP, OFFSET, FULL = 64, 32, 16, (53, 70)
ARCHS = ('E2',)
SETS = ('sampler', 'shuffled', 'noise')
SET_KEYS = tuple(k % s for s in SETS for k in ('moments/%s/moments/mean', 'moments/%s/moments/var')) + \
    tuple(k % s for s in SETS for k in ('per_image_metrics/%s/rmse/mean', 'per_image_metrics/%s/rmse/min'))


class experimental_sampler(ModelPlugin, engine.Replica):
    name = 'experimental_sampler'

    @staticmethod
    def arguments():
        """:16-43."""
        return {
            '--g_sparsity': {'action': 'store_true', 'default': False,
                             'help': 'Parsed as in the reference, where the sparsity term it once added is commented out: no effect.'},
            '--g_rmse': {'action': 'store_true', 'default': False,
                         'help': 'Parsed as in the reference, where the RMSE term it once added is commented out: no effect.'},
            '--g_arch': {'type': str, 'default': 'E2', 'help': 'Architecture to use for the generator. Options are: E2.'},
            '--d_arch': {'type': str, 'default': 'E2', 'help': 'Architecture to use for the discriminator. Options are: E2.'},
            '--examples': {'type': int, 'default': 64, 'help': 'Number of image summary examples to use.'},
        }

    # ------------------------------------------------------------------------------ builders
    @staticmethod
    def generatorE2(x, args, reuse=False):
        """:213-248: X [B,64,64,6] -> the recorded 32x32x1 tanh head d5."""
        B = args.batch_size
        with variable_scope('encoder'), arg_scope([conv2d], reuse=reuse, stride=2, padding='SAME', filter_size=5, init='xavier',
                                                  activation=relu):
            h = concat([x, random_uniform([B, SRC, SRC, 1], minval=-1.0, maxval=1.0)])      # 64x64x7
            e1 = conv2d(h, 7, 64, name='e1')                        # 32x32x64
            e2 = conv2d(e1, 64, 128, name='e2')                     # 16x16x128
            e3 = conv2d(e2, 128, 256, name='e3')                    # 8x8x256
            e4 = conv2d(e3, 256, 512, name='e4')                    # 4x4x512
            e5 = conv2d(e4, 512, 1024, filter_size=4, padding='VALID', name='e5')           # 1x1x1024
        with variable_scope('decoder'), arg_scope([deconv2d, conv2d], reuse=reuse, stride=2, init='xavier', padding='SAME',
                                                  filter_size=5, activation=_lrelu(0.2)):
            y = deconv2d(e5, 1024, 512, output_shape=(B, 512, 4, 4), filter_size=4, padding='VALID', name='d1')
            y = concat([y, e4])                                     # 4x4x1024
            y = deconv2d(y, 1024, 256, output_shape=(B, 256, 8, 8), name='d2')
            y = concat([y, e3])                                     # 8x8x512
            y = deconv2d(y, 512, 128, output_shape=(B, 128, 16, 16), name='d3')
            y = concat([y, e2])                                     # 16x16x256
            y = deconv2d(y, 256, 64, output_shape=(B, 64, 32, 32), name='d4')
            y = concat([y, e1])                                     # 32x32x128
            y = conv2d(y, 128, 1, stride=1, filter_size=1, activation=tanh, name='d5')      # 32x32x1 (not 31x31, :247)
        return y

    @staticmethod
    def discriminatorE2(x, y, args, reuse=False):
        """:252-281: X [B,64,64,6], depth [B,32,32,1] -> the logits [B,1,1,1]."""
        with arg_scope([conv2d], reuse=reuse, activation=_lrelu(0.2), init='xavier', padding='SAME', filter_size=5, stride=2):
            with variable_scope('rgb_path'):
                h1 = conv2d(x, 6, 64, name='hx1')                   # 32x32x64
                h1 = conv2d(h1, 64, 128, name='hx2')                # 16x16x128
                h1 = conv2d(h1, 128, 256, name='hx3')               # 8x8x256
                h1 = conv2d(h1, 256, 512, name='hx4')               # 4x4x512
                h1 = conv2d(h1, 512, 1024, padding='VALID', filter_size=4, name='hx5')      # 1x1x1024
            with variable_scope('depth_path'):
                h2 = conv2d(y, 1, 128, name='hy1')                  # 16x16x128
                h2 = conv2d(h2, 128, 256, name='hy2')               # 8x8x256
                h2 = conv2d(h2, 256, 512, name='hy3')               # 4x4x512
                h2 = conv2d(h2, 512, 1024, filter_size=4, padding='VALID', name='hy4')      # 1x1x1024
            with variable_scope('combined_path'):
                h = concat([h1, h2])                                # 1x1x2048
                for i, (ci, co) in enumerate(((2048, 1024), (1024, 512), (512, 256), (256, 128), (128, 64)), 1):
                    h = conv2d(h, ci, co, stride=1, filter_size=1, padding='SAME', name='h%d' % i)
                h = conv2d(h, 64, 1, stride=1, filter_size=1, padding='SAME', name='h6', activation=None)
        return h

    @classmethod
    def check_arch(cls, args):
        for flag in ('g_arch', 'd_arch'):
            arch = getattr(args, flag, 'E2')
            if arch not in ARCHS:
                raise ValueError('experimental_sampler: unknown --%s %r (choices: %s)' % (flag, arch, ', '.join(ARCHS)))

    @classmethod
    def build_graph(cls, args):
        """Record the networks for `args` (no device work); returns the Nets by scope name."""
        cls.check_arch(args)
        reset_graph()
        X = placeholder((None, SRC, SRC, 6))
        dy = placeholder((None, CROP, CROP, 1), 'y')
        with variable_scope('generator'):
            cls.generatorE2(X, args)
        with variable_scope('discriminator'):
            cls.discriminatorE2(X, dy, args, reuse=False)          # D(x, y) first, as :163-164
            cls.discriminatorE2(X, dy, args, reuse=True)
        from ...ops import layers as Lyr
        return {k: v for k, v in Lyr._nets.items() if v.passes}

    # ------------------------------------------------------------------------------ construction
    def __init__(self, x_y, args, sess=None, estimator=None):
        engine.Replica.__init__(self, args, sess)
        self.x_y, sess = x_y, self.sess
        for flag, spec in self.arguments().items():
            if not hasattr(args, flag.lstrip('-')):
                setattr(args, flag.lstrip('-'), spec['default'])
        self.check_arch(args)
        B = self.B = args.batch_size
        dev, dt = sess.device, sess.dtype
        est = self.estimator = estimator if estimator is not None else mean_depth_estimator(x_y, args, sess)
        if est.B != B or est.sess is not sess or tuple(est.FULL) != FULL:
            raise ValueError('experimental_sampler: the estimator must share this model\'s session and batch size %d and read %dx%d '
                             'originals' % ((B,) + FULL))
        for _ in tower_scope_range(None, args.n_gpus, B, sess):
            nets = self.build_graph(args)
        self.enet, self.dec_net = nets['generator/encoder'], nets['generator/decoder']
        self.ws = K.Workspace(dev)
        self.g_store, self.d_store = engine.ParamStore(dev), engine.ParamStore(dev)
        # D: combined path over 2B (images [0,B) real, [B,2B) fake), depth path over 2B, rgb path over B
        self.Dc = engine.SeqNet(nets['discriminator/combined_path'], 2 * B, (1, 1, 2048), dt, dev, self.d_store, need_input_grad=True,
                                ws=self.ws)
        self.Dr = engine.SeqNet(nets['discriminator/rgb_path'], B, (SRC, SRC, 6), dt, dev, self.d_store, ws=self.ws)
        self.Dd = engine.SeqNet(nets['discriminator/depth_path'], 2 * B, (CROP, CROP, 1), dt, dev, self.d_store, need_input_grad=True,
                                ws=self.ws)
        for net in (self.Dr, self.Dd, self.Dc):
            net.declare_variables()
        self.rgb_g, self.depth_g = self.Dr.layers[-1].gout, self.Dd.layers[-1].gout
        self.fake, self.dfake = self.Dd.x.view(B, B), self.Dd.dx.view(B, B)        # g lands in D's fake depth input
        # G: the U-Net allocates [X | noise] and hands over its last concat [d4 | e1]; d5 is this module's head
        self.G = UNet(self.enet, self.dec_net, B, dt, dev, self.g_store, self.ws, self.Dr.x, sess=sess)
        self.head, top = self.dec_net.layers[-1], self.G.top
        if self.G.xn is None or list(self.G.noise) != ['noise_x'] or len(self.dec_net.layers) != self.G.nd + 1 or \
                (self.head.k, self.head.out_size, self.head.in_size, top.h, top.w) != (1, 1, top.c, CROP, CROP):
            raise ValueError('experimental_sampler: the generator must read [X | noise] and end in a 1x1 head on the %dx%d concat'
                             % (CROP, CROP))
        self.head_ws = torch.zeros(B * (self.head.in_size + 1), dtype=torch.float32, device=dev)
        self.d_store.allocate()
        self.g_store.allocate()
        gen = torch.Generator().manual_seed(sess.seed)
        self.G.init_variables(gen)
        for net in (self.Dr, self.Dd, self.Dc):
            net.init_variables(gen)
        self.g_opt, self.d_opt = init_optimizer(args, self.g_store), init_optimizer(args, self.d_store)      # :70-71
        self.register('generator', self.g_store, self.g_opt, self.G.repack)
        self.register('discriminator', self.d_store, self.d_opt, self._repack_d)
        self.register('model', est.store, est.opt, est.M.repack)                   # carried, never stepped
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x_stage, self.y_stage, self.xl_stage, self.yl_stage, self.xf_stage = self.staging(
            (B, SRC, SRC, 3), (B, SRC, SRC, 1), (B, SRC, SRC, 1), (B, SRC, SRC, 1), (B,) + FULL + (3,))
        self.m = est.last.out                                                      # f32 [B]: the estimator's output, in place
        self.g32, self.target, self.scal = f32(B, CROP, CROP), f32(B, CROP, CROP), f32(8)      # of the last loss fetch
        self.l1_ws = torch.zeros(2 * _lib.load().tdg_reduce_workspace_bytes(B * CROP * CROP), dtype=torch.uint8, device=dev)
        # infer() / the summary passes / sample(): buffers of their own
        self.inf_g = f32(B, CROP, CROP)
        self.set_g, self.set_y = f32(B, CROP, CROP), {'sampler': f32(B, CROP, CROP), 'shuffled': f32(B, CROP, CROP)}
        self.zero_rows = torch.zeros(B, dtype=torch.int32, device=dev)
        self.perm = torch.zeros(B, dtype=torch.int32, device=dev)
        self.x_noise_u = f32(B * SRC * SRC * 6)
        self.stat_out = {s: f32(6) for s in SETS}
        self.samp_mean, self.samp_var = f32(CROP, CROP), f32(CROP, CROP)
        self.samp = [f32(B, SRC, SRC, 3), f32(B, SRC, SRC, 1), f32(B, SRC, SRC, 1), f32(B, SRC, SRC, 1), f32((B,) + FULL + (3,))]
        self.stat_ws = torch.zeros(_lib.load().tdg_cgan_sample_stats_workspace_bytes(B, CROP * CROP), dtype=torch.uint8, device=dev)
        self.refresh()

    def _repack_d(self):
        for net in (self.Dr, self.Dd, self.Dc):
            net.repack()

    # ---- pieces ------------------------------------------------------------------------------------------
    def _batch(self, batch):
        """The five tensors this model reads of the 6-tuple, checked."""
        B, (fh, fw) = self.B, FULL
        want = [(B, SRC, SRC, 3), (B, SRC, SRC, 1), (B, SRC, SRC, 1), (B, SRC, SRC, 1), (B, fh, fw, 3), (B, fh, fw, 1)]
        ok = isinstance(batch, (tuple, list)) and len(batch) == 6 and [tuple(t.shape) for t in batch] == want
        if not ok:
            got = [tuple(t.shape) for t in batch] if isinstance(batch, (tuple, list)) else type(batch).__name__
            raise ValueError('experimental_sampler reads (x, y, x_loc, y_loc, x_full, y_full) with %dx%d crops and %dx%d originals: '
                             'run the dataset with --random_crop %d %d --include_location --include_originals %d %d (got %s)'
                             % (SRC, SRC, fh, fw, SRC, SRC, fh, fw, got))
        return batch[:5]

    def _prep(self, src=None, x_rows=None, y_rows=None, target=None, with_y=True, estimate=True):
        """Estimator forward (estimate=False: m of the last one stands), then tdg_xsamp_prep: X into G's and D's inputs, the depth
        target into D's real half and `target`."""
        x, y, xl, yl, xf = src if src is not None else (self.x_stage, self.y_stage, self.xl_stage, self.yl_stage, self.xf_stage)
        if estimate:
            self.estimator._forward(xf)
        xn, rx, dd = self.G.xn, self.Dr.x, self.Dd.x
        _lib.call('tdg_xsamp_prep', self.sess.dtype, K.ptr(x), K.ptr(xl), K.ptr(yl), K.ptr(self.m), K.ptr(y) if with_y else None,
                  K.ptr(x_rows), K.ptr(y_rows), self.B, SRC, CROP, OFFSET, xn.ptr(0), xn.cs, rx.ptr(0), rx.cs,
                  dd.ptr(0) if with_y else None, dd.cs, K.ptr(target) if with_y else None, K.stream())

    def _generate(self, g32):
        """The U-Net (fresh noise), then the tanh head: g f32 into `g32`, rounded into channel 0 of D's fake depth input."""
        self.G.forward()
        top, st, name = self.G.top, self.g_store, self.dec_net.var_name
        _lib.call('tdg_xsamp_head_fwd', self.sess.dtype, top.ptr(), self.B, top.h, top.c, top.cs, K.ptr(st[name(self.head, 'weights')]),
                  K.ptr(st[name(self.head, 'bias')]), K.ptr(g32), self.fake.ptr(0), self.fake.cs, K.stream())

    def _d_forward(self):
        B, dt = self.B, self.sess.dtype
        self.Dr.forward(0, B)
        self.Dd.forward(0, 2 * B)
        rh, dh = self.Dr.layers[-1].h, self.Dd.layers[-1].h
        _lib.call('tdg_cgan_join', dt, 0, B, 2 * B, 1024, self.Dc.x.ptr(0), self.Dc.x.cs, rh.ptr(0), rh.cs, dh.ptr(0), dh.cs, K.stream())
        self.Dc.forward(0, 2 * B)

    def _xent(self, mode):
        last = self.Dc.layers[-1]          # d_real, d_fake, g_fake to scal[4..6]
        _lib.call('tdg_p2p_xent', self.sess.dtype, last.h.ptr(0), self.B, last.h.cs, mode, last.gout.ptr(0), K.ptr(self.scal, 16),
                  K.stream())

    # ---- the step ------------------------------------------------------------------------------------------
    def _grads(self):
        B, dt = self.B, self.sess.dtype
        self._prep(target=self.target)
        self._generate(self.g32)
        self._d_forward()
        # D's gradients: both halves
        self._xent(1)
        self.Dc.backward(0, 2 * B, want_params=True, want_dx=True)
        dx = self.Dc.dx
        _lib.call('tdg_cgan_join', dt, 1, B, 2 * B, 1024, dx.ptr(0), dx.cs, self.rgb_g.ptr(0), self.rgb_g.cs, self.depth_g.ptr(0),
                  self.depth_g.cs, K.stream())
        self.Dd.backward(0, 2 * B, want_params=True)
        self.Dr.backward(0, B, want_params=True)
        # G's gradients from the same forward pass: data only through the fake half, D's parameter gradients stay
        self._xent(2)
        self.Dc.backward(B, B, want_params=False, want_dx=True)
        _lib.call('tdg_cgan_join', dt, 1, B, B, 1024, dx.ptr(B), dx.cs, None, 0, self.depth_g.ptr(B), self.depth_g.cs, K.stream())
        self.Dd.backward(B, B, want_params=False, want_dx=True)
        top, gtop, st, name = self.G.top, self.G.gtop, self.g_store, self.dec_net.var_name
        _lib.call('tdg_xsamp_head_bwd', dt, self.dfake.ptr(0), self.dfake.cs, K.ptr(self.g32), top.ptr(), B, top.h, top.c, top.cs,
                  K.ptr(st[name(self.head, 'weights')]), K.MASK_LRELU, self.dec_net.layers[-2].act.leak, gtop.ptr(),
                  K.ptr(st.grad(name(self.head, 'weights'))), K.ptr(st.grad(name(self.head, 'bias'))), K.ptr(self.head_ws),
                  self.head_ws.numel() * 4, K.stream())
        self.G.backward()
        # rmse and l1 on (g + 1) / 2 against (y + 1) / 2: the two halves of D's depth input share a row stride
        dd = self.Dd.x
        _lib.call('tdg_p2p_l1', dt, dd.ptr(0), dd.ptr(B), B * CROP * CROP, dd.cs, 0.0, None, 0, K.ptr(self.scal), K.ptr(self.l1_ws),
                  self.l1_ws.numel(), K.stream())

    def _apply(self):
        self.d_opt.step(self._scale_d)
        self.g_opt.step(self._scale_g)
        self._repack_d()
        self.G.repack()

    def _losses(self):
        s = self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()
        t = 'tower_%d/loss/' % (self.sess.world_size - 1)
        return collection_to_dict([(t + 'generator/g_fake:0', s[6]), (t + 'discriminator/d_real:0', s[4]),
                                   (t + 'discriminator/d_fake:0', s[5]), (t + 'discriminator/d_total:0', s[4] + s[5]),
                                   (t + 'rmse:0', s[1]), (t + 'l1:0', s[0])])

    def train(self, sess=None, args=None, feed_dict=None):
        """:198-209: one sess.run of both train ops and the losses."""
        self._stage(self._batch(self.x_y.next_batch()))
        self._run('xs_grads', self._grads)
        for store in (self.d_store, self.g_store):
            self.sess.assert_finite(store, 'train')
        self._scale_d = self.sess.allreduce_mean_scale(self.d_store.grads)
        self._scale_g = self.sess.allreduce_mean_scale(self.g_store.grads)
        self._run('xs_apply', self._apply)
        self.sess.global_step += 2
        return self._losses()

    # ---- inference and the summary sets ----------------------------------------------------------------------
    def infer(self, batch):
        """Depth in [0, 1], (g + 1) / 2, f32 [B,32,32,1] of one 6-tuple batch.  E2 has no batch norm: rows are independent.  It
        writes the generator's activations and D's input buffers, which every step rewrites, and no result of the last fetch."""
        self._stage(self._batch(batch))
        self._prep(with_y=False)
        self._generate(self.inf_g)
        return ((self.inf_g + 1.0) * 0.5).reshape(self.B, CROP, CROP, 1)

    def _stats(self, name, y, g, images=False):
        """tdg_cgan_sample_stats at unit 1 on the [-1, 1] tensors: [0], [1] the per-image mean |y - g| (mean, min), [2], [3] the
        moments of g."""
        _lib.call('tdg_cgan_sample_stats', K.ptr(y), K.ptr(g), K.ptr(g), None, None, 1.0, self.B, CROP * CROP, 1.0,
                  K.ptr(self.stat_out[name]), K.ptr(self.samp_mean) if images else None, K.ptr(self.samp_var) if images else None,
                  K.ptr(self.stat_ws), self.stat_ws.numel(), K.stream())

    def _metrics_body(self):
        B, dt = self.B, self.sess.dtype
        # sampler: row 0 of X (its m included) and of y, broadcast
        self._prep(x_rows=self.zero_rows, y_rows=self.zero_rows, target=self.set_y['sampler'])
        self._generate(self.set_g)
        self._stats('sampler', self.set_y['sampler'], self.set_g)
        # shuffled: X permuted, y as it is
        self._prep(x_rows=self.perm, target=self.set_y['shuffled'], estimate=False)
        self._generate(self.set_g)
        self._stats('shuffled', self.set_y['shuffled'], self.set_g)
        # noise: X <- U(-1, 1), against the sampler set's y
        xn, u = self.G.xn, self.x_noise_u
        self.sess.random_uniform(u, u.numel(), 'x_noise')
        _lib.call('tdg_affine_cast_rows', dt, K.ptr(u), B * SRC * SRC, 6, xn.cs, 2.0, -0.5, xn.ptr(0), K.stream())
        self._generate(self.set_g)
        self._stats('noise', self.set_y['sampler'], self.set_g)

    def metrics(self):
        """SET_KEYS of the three summary sets on the last staged batch, then the six losses of the last fetch."""
        inj = self.sess._injected('shuffle')
        perm = torch.randperm(self.B) if inj is None else torch.as_tensor(np.asarray(inj)).reshape(self.B)
        self.perm.copy_(perm.to(torch.int32))
        self._run('xs_metrics', self._metrics_body)
        s = {k: self.stat_out[k].cpu().tolist() for k in SETS}
        out = {}
        for k in SETS:
            out['moments/%s/moments/mean' % k], out['moments/%s/moments/var' % k] = s[k][2], s[k][3]
        for k in SETS:                               # per_image_statistics multiplies by 10 (:381)
            out['per_image_metrics/%s/rmse/mean' % k], out['per_image_metrics/%s/rmse/min' % k] = 10.0 * s[k][0], 10.0 * s[k][1]
        out.update(self._losses())
        return out

    def _sample_body(self):
        self._prep(src=self.samp, x_rows=self.zero_rows, y_rows=self.zero_rows, target=self.set_y['sampler'])
        self._generate(self.set_g)
        self._stats('sampler', self.set_y['sampler'], self.set_g, images=True)

    def sample(self, x, x_loc, y_loc, x_full, y=None):
        """B predictions for ONE window under B noise draws.  x f32 [64,64,3], x_loc, y_loc [64,64] or [64,64,1], x_full
        [53,70,3], y (optional) [64,64] or [64,64,1], all in [0, 1].  Returns a dict: `y_hat` f32 [B,32,32] (device, depth in
        [0, 1]), `mean` and `var` f32 [32,32]: the per-pixel mean and population variance of the predictions in [0, 1] units,
        and `metrics`: with y the set's four statistics (SET_KEYS of `sampler`), else None."""
        dev, B = self.sess.device, self.B
        shapes = [((SRC, SRC, 3),), ((SRC, SRC), (SRC, SRC, 1)), ((SRC, SRC), (SRC, SRC, 1)), ((SRC, SRC), (SRC, SRC, 1)), (FULL + (3,),)]
        given = [x, y if y is not None else torch.zeros(SRC, SRC), x_loc, y_loc, x_full]
        for buf, t, ok, what in zip(self.samp, given, shapes, ('x', 'y', 'x_loc', 'y_loc', 'x_full')):
            t = torch.as_tensor(t).to(device=dev, dtype=torch.float32)
            if tuple(t.shape) not in ok:
                raise ValueError('sample: %s must be %s, got %s' % (what, ' or '.join(str(list(s)) for s in ok), tuple(t.shape)))
            buf[0].copy_(t.reshape(buf.shape[1:]))
        self._run('xs_sample', self._sample_body)
        out = {'y_hat': (self.set_g + 1.0) * 0.5, 'mean': (self.samp_mean + 1.0) * 0.5, 'var': self.samp_var * 0.25, 'metrics': None}
        if y is not None:
            s = self.stat_out['sampler'].cpu().tolist()
            out['metrics'] = {'moments/sampler/moments/mean': s[2], 'moments/sampler/moments/var': s[3],
                              'per_image_metrics/sampler/rmse/mean': 10.0 * s[0], 'per_image_metrics/sampler/rmse/min': 10.0 * s[1]}
        return out
