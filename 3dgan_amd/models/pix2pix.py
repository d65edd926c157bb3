"""pix2pix conditional GAN on MI355X -- the reference's gen-2 plugin `hem/models/pix2pix.py`
(arguments :36-78, __init__ :81-148, train :151-156, generator :160-228, discriminator :232-259,
loss :263-304) on the HIP kernels.

Kept: the plugin contract (`name`, `arguments()`, `__init__(x_y, args)`, `train(sess, args, feed_dict)`
-> loss dict), the generator/discriminator written against conv2d/deconv2d + arg_scope with the
reference's variable names (`generator/enocder/vars/1/weights` -- sic --, `generator/decoder/vars/8/bias`,
`discriminator/vars/m5/weights`), init N(0, 0.02) for weights and biases, batch norm on every decoder
layer, the hard-coded L1 weight 10.0 (C-9), three fresh batches per `train()`.

MI355X-native: activations are NHWC; every skip `tf.concat([y, e_k], axis=1)` is a ZERO-COPY concat --
the decoder layer and the encoder layer each write their channel window of one buffer, and in the backward
pass the encoder's two gradient paths (next encoder layer + skip) are summed by the `accumulate` epilogue of
the backward-data GEMM; D(x,y) and D(x,G(x)) run as one batched pass over [x|y ; x|g]; G(x) lands directly
in channel 3 of D's input and dL/dG(x) is read from channel 3 of D's input gradient.

`--dropout` (keep probability of decoder layers 1-3, hem/models/pix2pix.py:204-208) and `--noise input|latent|end`
(a U(-1,1) channel concatenated to the generator input / the 1x1 bottleneck / the last decoder layer's input,
:183-186,204-206,223-225) are executed by the skip U-Net executor (unet.py), which also owns the concat buffers.
"""
import torch

from .. import _lib
from .. import kernels as K
from .. import engine
from ..ops.layers import conv2d, deconv2d, concat, arg_scope, variable_scope, placeholder, reset_graph, random_uniform
from ..ops.activations import _lrelu, tanh
from ..unet import UNet
from ..util import tower_scope_range, init_optimizer, collection_to_dict
from .ModelPlugin import ModelPlugin

L1_WEIGHT = 10.0            # l_term, hem/models/pix2pix.py:284 (the --lambda flag is ignored by the reference)


class pix2pix(ModelPlugin, engine.Replica):
    name = 'pix2pix'

    @staticmethod
    def arguments():
        """hem/models/pix2pix.py:36-78 (argparse kwargs per flag)."""
        return {
            '--skip_layers': {'action': 'store_true', 'default': 'false', 'help': 'Adds skip layers to the generator.'},
            '--noise': {'type': str, 'nargs': '*', 'choices': ['input', 'latent', 'end'], 'default': []},
            '--dropout': {'type': float, 'default': 0},
            '--batch_norm_disc': {'action': 'store_true', 'default': False},
            '--batch_norm_gen': {'action': 'store_true', 'default': False},
            '--examples': {'type': int, 'default': 64},
            '--n_disc_train': {'type': int, 'default': 1},
            '--add_l1': {'action': 'store_true', 'default': False},
            '--lambda': {'type': float, 'default': 10.0},
        }

    # ------------------------------------------------------------------------------ builders
    @staticmethod
    def generator(x, args, reuse=False):
        """hem/models/pix2pix.py:160-228 (NHWC; 256x256x3 -> 256x256x1)."""
        init = 'normal0.02'
        with arg_scope([conv2d], reuse=reuse, use_batch_norm=args.batch_norm_gen, filter_size=4, stride=2, init=init,
                       activation=_lrelu(0.2)):
            with variable_scope('enocder'):
                if 'input' in args.noise:                                                  # :183-186
                    noise = random_uniform([args.batch_size, 256, 256, 1], minval=-1.0, maxval=1.0)
                    e1 = conv2d(concat([x, noise]), 4, 64, name='1', use_batch_norm=False)
                else:
                    e1 = conv2d(x, 3, 64, name='1', use_batch_norm=False)
                e2 = conv2d(e1, 64, 128, name='2')
                e3 = conv2d(e2, 128, 256, name='3')
                e4 = conv2d(e3, 256, 512, name='4')
                e5 = conv2d(e4, 512, 512, name='5')
                e6 = conv2d(e5, 512, 512, name='6')
                e7 = conv2d(e6, 512, 512, name='7')
                e8 = conv2d(e7, 512, 512, name='8')
        with arg_scope([deconv2d, conv2d], reuse=reuse, use_batch_norm=True, filter_size=4, stride=2, init=init,
                       activation=_lrelu(0.0)):
            with variable_scope('decoder'):
                if 'latent' in args.noise:                                                 # :204-206
                    noise = random_uniform([args.batch_size, 1, 1, 512], minval=-1.0, maxval=1.0)
                    y = deconv2d(concat([e8, noise]), 1024, 512, name='1', dropout=args.dropout)
                else:
                    y = deconv2d(e8, 512, 512, name='1', dropout=args.dropout)
                y = concat([y, e7])
                y = deconv2d(y, 1024, 512, name='2', dropout=args.dropout)
                y = concat([y, e6])
                y = deconv2d(y, 1024, 512, name='3', dropout=args.dropout)
                y = concat([y, e5])
                y = deconv2d(y, 1024, 512, name='4')
                y = concat([y, e4])
                y = deconv2d(y, 1024, 256, name='5')
                y = concat([y, e3])
                y = deconv2d(y, 512, 128, name='6')
                y = concat([y, e2])
                y = deconv2d(y, 256, 64, name='7')
                y = concat([y, e1])
                if 'end' in args.noise:                                                    # :223-225
                    noise = random_uniform([args.batch_size, 128, 128, 1], minval=-1.0, maxval=1.0)
                    y = deconv2d(concat([y, noise]), 129, 1, name='8', activation=tanh)
                else:
                    y = deconv2d(y, 128, 1, name='8', activation=tanh)
        return y

    @staticmethod
    def discriminator(x, y, args, reuse=False):
        """hem/models/pix2pix.py:232-259 (PatchGAN); returns the logits [B, 8, 8, 1]."""
        with arg_scope([conv2d], reuse=reuse, use_batch_norm=args.batch_norm_disc, activation=_lrelu(0.2), init='normal0.02',
                       filter_size=4, stride=2):
            x_y = concat([x, y])
            h = conv2d(x_y, 4, 64, name='m1', use_batch_norm=False)
            h = conv2d(h, 64, 128, name='m2')
            h = conv2d(h, 128, 256, name='m3')
            h = conv2d(h, 256, 512, name='m4')
            h = conv2d(h, 512, 1, name='m5', activation=None)
        return h

    # ------------------------------------------------------------------------------ construction
    S_DREAL, S_DFAKE, S_GFAKE, S_L1, S_RMSE = 0, 1, 2, 3, 4

    def __init__(self, x_y, args, sess=None):
        engine.Replica.__init__(self, args, sess)
        self.x_y, sess = x_y, self.sess
        for flag, default in (('noise', []), ('dropout', 0), ('batch_norm_gen', False), ('batch_norm_disc', False), ('add_l1', False)):
            if not hasattr(args, flag):
                setattr(args, flag, default)
        B = self.B = args.batch_size
        H = W = 256
        dev, dt = sess.device, sess.dtype

        reset_graph()
        xs, ys = placeholder((None, H, W, 3)), placeholder((None, H, W, 1))
        for _xy, scope, gpu_id in tower_scope_range((xs, ys), args.n_gpus, B, sess):
            with variable_scope('generator'):
                g = pix2pix.generator(_xy[0], args, reuse=False)
            with variable_scope('discriminator') as dnet:
                d_real = pix2pix.discriminator(_xy[0], _xy[1], args, reuse=False)
                d_fake = pix2pix.discriminator(_xy[0], g, args, reuse=True)
        from ..ops import layers as Lyr
        self.enet, self.dec_net, self.dnet = Lyr._nets['generator/enocder'], Lyr._nets['generator/decoder'], dnet

        self.ws = K.Workspace(dev)
        self.g_store, self.d_store = engine.ParamStore(dev), engine.ParamStore(dev)
        # D input holds both passes: images [0,B) = [x | y], images [B,2B) = [x | G(x)]
        self.D = engine.SeqNet(dnet, 2 * B, (H, W, 4), dt, dev, self.d_store, n_bn_passes=(2 if args.batch_norm_disc else 1),
                               need_input_grad=True, ws=self.ws)
        self.D.declare_variables()
        self.U = UNet(self.enet, self.dec_net, B, dt, dev, self.g_store, self.ws,
                      x_in=self.D.x.view(0, B).window(0, 3),
                      g_out=self.D.x.view(B, B).window(3, 1),
                      g_grad=self.D.dx.view(B, B).window(3, 1), sess=sess,
                      noise_keys={'x': 'noise_input', 'e8': 'noise_latent', 'd8': 'noise_end'})
        self.d_store.allocate()
        self.g_store.allocate()
        gen = torch.Generator().manual_seed(sess.seed)
        self.U.init_variables(gen)
        self.D.init_variables(gen)
        self.g_opt, self.d_opt = init_optimizer(args, self.g_store), init_optimizer(args, self.d_store)
        self.register('generator', self.g_store, self.g_opt, self.U.repack)
        self.register('discriminator', self.d_store, self.d_opt, self.D.repack)
        self.x_stage, self.y_stage = self.staging((B, H, W, 3), (B, H, W, 1))
        self.scal = torch.zeros(8, dtype=torch.float32, device=dev)
        self.refresh()

    # ---- pieces ------------------------------------------------------------------------------------------
    def _rescale(self):
        """hem.rescale((0,1) -> (-1,1)) of both halves (hem/models/pix2pix.py:103-104) into D's input slots."""
        B, dt = self.B, self.sess.dtype
        rows, cs = B * 256 * 256, self.D.x.cs
        if cs == 4:                                # [x | y] and [x | (G(x): written by the generator pass)] in one pass
            _lib.call('tdg_affine_cast_pair', dt, K.ptr(self.x_stage), 3, K.ptr(self.y_stage), 1, rows, 2.0, -0.5, self.D.x.ptr(0),
                      self.D.x.ptr(B), K.stream())
        else:
            for img0 in (0, B):
                _lib.call('tdg_affine_cast_rows', dt, K.ptr(self.x_stage), rows, 3, cs, 2.0, -0.5, self.D.x.ptr(img0), K.stream())
            _lib.call('tdg_affine_cast_rows', dt, K.ptr(self.y_stage), rows, 1, cs, 2.0, -0.5, self.D.x.window(3, 1).ptr(0), K.stream())
        if self.U.xn is not None:                  # --noise input: the generator reads [x | noise] from its own buffer
            _lib.call('tdg_affine_cast_rows', dt, K.ptr(self.x_stage), rows, 3, self.U.xn.cs, 2.0, -0.5, self.U.xn.ptr(0), K.stream())

    def _load(self, batch):
        self._stage(batch)
        self._rescale()

    def _d_forward(self, first, count):
        B = self.B
        if self.args.batch_norm_disc:
            for s in range(first, first + count):
                self.D.forward(s * B, B, bn_pass=s)
        else:
            self.D.forward(first * B, count * B)
        return self.D.layers[-1].h

    def _xent(self, mode):
        last = self.D.layers[-1]
        rows = self.B * last.h.h * last.h.w
        _lib.call('tdg_p2p_xent', self.sess.dtype, last.h.ptr(0), rows, last.h.cs, mode, last.gout.ptr(0),
                  K.ptr(self.scal, 4 * self.S_DREAL), K.stream())

    def _l1(self, with_grad):
        B, dt = self.B, self.sess.dtype
        y = self.D.x.view(0, B).window(3, 1)
        g = self.D.x.view(B, B).window(3, 1)
        dg = self.D.dx.view(B, B).window(3, 1)
        w = self.ws.ensure(4096)
        _lib.call('tdg_p2p_l1', dt, y.ptr(0), g.ptr(0), B * 256 * 256, y.cs, L1_WEIGHT,
                  dg.ptr(0) if with_grad else None, dg.cs, K.ptr(self.scal, 4 * self.S_L1), K.ptr(w), w.numel(), K.stream())

    # ---- steps ---------------------------------------------------------------------------------------------
    def d_step(self, batch):
        self._stage(batch)
        self.optimizer_step(self.d_store, ('d_grads', self._d_grads), ('d_apply', self._d_apply), 'd_step')

    def _d_grads(self):
        B = self.B
        self._rescale()
        self.U.forward(backward_follows=False)
        self._d_forward(0, 2)
        self._xent(1)
        if self.args.batch_norm_disc:
            self.D.backward(0, B, bn_pass=0, want_params=True, acc=False)
            self.D.backward(B, B, bn_pass=1, want_params=True, acc=True)
        else:
            self.D.backward(0, 2 * B, want_params=True)

    def _d_apply(self):
        self.d_opt.step(self._scale)
        self.D.repack()

    def g_step(self, batch):
        self._stage(batch)
        self.optimizer_step(self.g_store, ('g_grads', self._g_grads), ('g_apply', self._g_apply), 'g_step')

    def _g_grads(self):
        B = self.B
        self._rescale()
        self.U.forward()
        self._d_forward(1, 1)                  # only D(x, G(x)): sess.run(g_train_op) evaluates nothing of the real pass
        self._xent(2)                          # (hem/models/pix2pix.py:153; the losses are fetched by report() on a third batch)
        if self.args.batch_norm_disc:
            self.D.backward(B, B, bn_pass=1, want_params=False, want_dx=True)
        else:
            self.D.backward(B, B, want_params=False, want_dx=True)
        if self.args.add_l1:
            self._l1(True)
        self.U.backward()

    def _g_apply(self):
        self.g_opt.step(self._scale)
        self.U.repack()

    def _report_body(self):
        self._rescale()
        self.U.forward(backward_follows=False)
        self._d_forward(0, 2)
        self._xent(0)
        self._l1(False)

    def report(self, batch):
        """sess.run(all_losses) on a third batch (hem/models/pix2pix.py:155)."""
        self._stage(batch)
        self._run('report', self._report_body)
        s = self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()
        r = self.sess.world_size - 1     # the dict keeps the LAST tower's tensors (util.py:187-193, App. C-11), as models/gan.py does
        g_total = s[self.S_GFAKE] + (L1_WEIGHT * s[self.S_L1] if self.args.add_l1 else 0.0)
        g_name = 'loss/generator/add:0' if self.args.add_l1 else 'loss/generator/g_fake:0'
        return collection_to_dict([('tower_%d/loss/generator/l1:0' % r, s[self.S_L1]), ('tower_%d/%s' % (r, g_name), g_total),
                                   ('tower_%d/loss/generator/total:0' % r, g_total),
                                   ('tower_%d/loss/discriminator/d_real:0' % r, s[self.S_DREAL]),
                                   ('tower_%d/loss/discriminator/d_fake:0' % r, s[self.S_DFAKE]),
                                   ('tower_%d/loss/discriminator/total:0' % r, s[self.S_DREAL] + s[self.S_DFAKE]),
                                   ('tower_%d/loss/rmse:0' % r, s[self.S_RMSE])])

    def train(self, sess=None, args=None, feed_dict=None):
        """hem/models/pix2pix.py:151-156."""
        args = args or self.args
        for _ in range(args.n_disc_train):
            self.d_step(self.x_y.next_batch())
        self.g_step(self.x_y.next_batch())
        return self.report(self.x_y.next_batch())
