"""Shared-encoder RGB and depth autoencoder at 256x256 on MI355X -- the reference's gen-2 plugin `hem/models/artist.py` (arguments
:11-19, __init__ :23-63, train :65-68, losses :71-83, summaries :86-98, encoder :114-129, decoder :132-153), driven by train.py,
on the HIP kernels.

Inputs (:31-32).  The batch is the dataset's pair (x [B,256,256,3], y [B,256,256,1]) in [0, 1] (nyuv2: `--random_crop 256 256`);
longer tuples are accepted and the two leading entries read.  x <- 2x - 1 as hem.rescale computes it in f32
(tdg_affine_cast_rows: 2 (x - 0.5) has the bits of fl(2x - 1)); y enters the loss only.

    encoder    e1..e6  conv2d 5x5 stride 2 VALID lrelu 0.2     256 -> 126 -> 61 -> 29 -> 13 -> 5 -> 1, widths 3 -> 6, 12, 24, 48, 192, 384
                       batch norm on e2..e6, not on e1
    decoder    d1..d6  deconv2d 5x5 stride 2 VALID             1 -> 5 -> 13 -> 29 -> 61 -> 126 -> 256, widths 384 -> 192, 48, 24, 12, 6, C
                       batch norm on all six; d1..d5 lrelu 0.2, d6 deconv, batch norm, tanh
               built twice on the one encoder output: scope `x_decoder` with C = 3, scope `y_decoder` with C = 1.

Variables: `encoder/vars/e1/weights` ... `x_decoder/vars/d6/bias`, `y_decoder/vars/d6/bias`; batch-norm betas
`encoder/BatchNorm[_i]/beta`, `x_decoder/BatchNorm[_i]/beta`, `y_decoder/BatchNorm[_i]/beta` (Net.bn_name).  Batch norm runs in
training mode in every pass, with beta only and eps 1e-3, and keeps no moving averages, like the project's other batch-norm
models.  Weights and biases are xavier-uniform, drawn in the reference's creation order: encoder, x_decoder, y_decoder.

Losses (:71-83, tdg_artist_mse): all four tensors go back to [0, 1] in f32; x_hat_loss = mean((x01 - xhat01)^2) over B 3 65536,
y_hat_loss the same over B 65536, y_hat_rmse = sqrt(y_hat_loss).  The target is the f32 staged batch taken through the
reference's round trip, not the compute-dtype copy the encoder reads.
Gradients (:48-49): y_hat_loss trains encoder + y_decoder with one optimizer; x_hat_loss trains x_decoder ONLY -- its pass runs
the encoder forward, no gradient enters the encoder.  Two instances of init_optimizer(args) (:24-25).

train() (:65-68) is two sess.runs on two consecutive batches.  The y step first: the batch into the staging buffers; ONE
captured gradient body (cast, encoder, y_decoder, tdg_artist_mse with its seed, y_decoder's backward pass down to the latent,
the encoder's); the finite check and the exchange (Replica.optimizer_step); ONE captured apply body (the optimizer step, the
repacks).  Then the x step on the next batch: cast, encoder (forward only), the 1x1x384 latent copied into x_decoder's input,
x_decoder, tdg_artist_mse, x_decoder's backward pass without an input gradient; the check, the exchange, the apply.  Each loss
is that of its own forward pass, before the update.  global_step advances by 2.
"""
import math
import os

import numpy as np
import torch

from ... import _lib
from ... import kernels as K
from ... import engine
from ... import summaries
from ...ops.layers import conv2d, deconv2d, arg_scope, variable_scope, placeholder, reset_graph
from ...ops.activations import _lrelu, tanh
from ...util import tower_scope_range, init_optimizer, collection_to_dict
from ..ModelPlugin import ModelPlugin

SIDE = 256
LATENT = 384
SCOPES = ('encoder', 'x_decoder', 'y_decoder')
LOSS_KEYS = ('x_hat_loss', 'y_hat_loss', 'y_hat_rmse')


class artist(ModelPlugin, engine.Replica):
    name = 'artist'

    @staticmethod
    def arguments():
        """:11-19."""
        return {'--examples': {'type': int, 'default': 64, 'help': 'Number of image summary examples to use.'}}

    # ------------------------------------------------------------------------------ builders
    @staticmethod
    def encoder(x, reuse=False):
        """:114-129: x [B,256,256,3] -> the recorded 1x1x384 latent."""
        with arg_scope([conv2d], reuse=reuse, filter_size=5, stride=2, padding='VALID', init='xavier', use_batch_norm=True,
                       activation=_lrelu(0.2)):
            h = conv2d(x, 3, 6, name='e1', use_batch_norm=False)       # 126x126x6
            h = conv2d(h, 6, 12, name='e2')                            # 61x61x12
            h = conv2d(h, 12, 24, name='e3')                           # 29x29x24
            h = conv2d(h, 24, 48, name='e4')                           # 13x13x48
            h = conv2d(h, 48, 192, name='e5')                          # 5x5x192
            h = conv2d(h, 192, LATENT, name='e6')                      # 1x1x384
        return h

    @staticmethod
    def decoder(x_rep, args, channel_output=3, reuse=False):
        """:132-153: the latent -> the recorded 256x256xC tanh output.  The explicit sides 126 and 256 are one more than the
        natural 125 and 255, as paper_cgan's 5 -> 14 is."""
        B = args.batch_size
        with arg_scope([conv2d, deconv2d], reuse=reuse, filter_size=5, stride=2, padding='VALID', init='xavier', use_batch_norm=True,
                       activation=_lrelu(0.2)):
            h = deconv2d(x_rep, LATENT, 192, output_shape=(B, 192, 5, 5), name='d1')
            h = deconv2d(h, 192, 48, output_shape=(B, 48, 13, 13), name='d2')
            h = deconv2d(h, 48, 24, output_shape=(B, 24, 29, 29), name='d3')
            h = deconv2d(h, 24, 12, output_shape=(B, 12, 61, 61), name='d4')
            h = deconv2d(h, 12, 6, output_shape=(B, 6, 126, 126), name='d5')
            h = deconv2d(h, 6, channel_output, activation=tanh, output_shape=(B, channel_output, SIDE, SIDE), name='d6')
        return h

    @classmethod
    def build_graph(cls, args):
        """Record the three networks for `args` (no device work); returns the Nets by scope name."""
        reset_graph()
        x = placeholder((None, SIDE, SIDE, 3))
        with variable_scope('encoder'):
            e = cls.encoder(x)
        with variable_scope('x_decoder'):
            cls.decoder(e, args, channel_output=3)
        with variable_scope('y_decoder'):
            cls.decoder(e, args, channel_output=1)
        from ...ops import layers as Lyr
        return {k: Lyr._nets[k] for k in SCOPES}

    # ------------------------------------------------------------------------------ construction
    def __init__(self, x_y, args, sess=None):
        engine.Replica.__init__(self, args, sess)
        self.x_y, sess = x_y, self.sess
        if not hasattr(args, 'examples'):
            args.examples = self.arguments()['--examples']['default']
        B = self.B = args.batch_size
        dev, dt = sess.device, sess.dtype
        for _ in tower_scope_range(None, args.n_gpus, B, sess):
            nets = self.build_graph(args)
        self.bind(nets, B, dt, dev, sess.seed)
        self.x_opt, self.y_opt = init_optimizer(args, self.x_store), init_optimizer(args, self.y_store)     # :24-25
        self.register('x', self.x_store, self.x_opt, self.Dx.repack)
        self.register('y', self.y_store, self.y_opt, self._repack_y)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.batch_shapes = [(B, SIDE, SIDE, 3), (B, SIDE, SIDE, 1)]
        self.x_stage, self.y_stage = self.staging(*self.batch_shapes)
        self.rows = B * SIDE * SIDE
        self.scal = f32(4)                                                  # of the last fetches: x_hat_loss, -, y_hat_loss, y_hat_rmse
        self.eval_scal, self.eval_acc = f32(4), torch.zeros(4, dtype=torch.float64, device=dev)
        self.mse_ws = torch.zeros(_lib.load().tdg_artist_mse_workspace_bytes(), dtype=torch.uint8, device=dev)
        self.refresh()

    def bind(self, nets, B, dtype, device, seed):
        """The two stores, the three nets bound to their buffers and the fresh variables (no kernel runs).  Two variable sets
        (:48-49): x_decoder alone; encoder + y_decoder together.  The encoder's output and its gradient ARE the y decoder's input
        and input gradient; the x decoder has an input of its own, filled by a copy of the latent."""
        self.ws = K.Workspace(device)
        self.x_store, self.y_store = engine.ParamStore(device), engine.ParamStore(device)
        self.Dy = engine.SeqNet(nets['y_decoder'], B, (1, 1, LATENT), dtype, device, self.y_store, need_input_grad=True, ws=self.ws)
        self.E = engine.SeqNet(nets['encoder'], B, (SIDE, SIDE, 3), dtype, device, self.y_store, ws=self.ws, out_act=self.Dy.x,
                               out_grad=self.Dy.dx)
        self.Dx = engine.SeqNet(nets['x_decoder'], B, (1, 1, LATENT), dtype, device, self.x_store, ws=self.ws)
        for net in (self.E, self.Dy, self.Dx):
            net.declare_variables()
        self.x_store.allocate()
        self.y_store.allocate()
        gen = torch.Generator().manual_seed(seed)
        for net in (self.E, self.Dx, self.Dy):                              # the reference's creation order
            net.init_variables(gen)

    def _repack_y(self):
        self.E.repack()
        self.Dy.repack()

    # ---- pieces ------------------------------------------------------------------------------------------
    def _batch(self, batch):
        """(x, y): the two leading tensors of the dataset's tuple, checked."""
        ok = isinstance(batch, (tuple, list)) and len(batch) >= 2 and [tuple(t.shape) for t in batch[:2]] == self.batch_shapes
        if not ok:
            got = [tuple(t.shape) for t in batch] if isinstance(batch, (tuple, list)) else type(batch).__name__
            raise ValueError('artist reads (x [B,%d,%d,3], y [B,%d,%d,1]) at batch size %d: run the dataset with --random_crop %d %d '
                             '(got %s)' % (SIDE, SIDE, SIDE, SIDE, self.B, SIDE, SIDE, got))
        return tuple(batch[:2])

    def _encode(self, keep_pre):
        """x <- fl(2x - 1) into the encoder's input, then the encoder: the latent lands in the y decoder's input."""
        x = self.E.x
        _lib.call('tdg_affine_cast_rows', self.sess.dtype, K.ptr(self.x_stage), self.rows, 3, x.cs, 2.0, -0.5, x.ptr(0), K.stream())
        self.E.forward(0, self.B, keep_pre=keep_pre)

    def _mse(self, net, target, c, scal, at, seed=True):
        """tdg_artist_mse of `net`'s output against the staged `target`: the loss into scal[at], its root into scal[at + 1], the
        seed (unless mode 0) into the last layer's incoming gradient."""
        last = net.layers[-1]
        _lib.call('tdg_artist_mse', self.sess.dtype, K.ptr(target), last.h.ptr(0), self.rows, c, last.h.cs,
                  last.gout.ptr(0) if seed else None, K.ptr(scal, 4 * at), K.ptr(self.mse_ws), self.mse_ws.numel(), K.stream())

    def _decode_x(self, keep_pre):
        self.Dx.x.buf.copy_(self.Dy.x.buf)                                  # 384 values per image
        self.Dx.forward(0, self.B, keep_pre=keep_pre)

    # ---- the steps -----------------------------------------------------------------------------------------
    def _y_grads(self):
        self._encode(True)
        self.Dy.forward(0, self.B)
        self._mse(self.Dy, self.y_stage, 1, self.scal, 2)
        self.Dy.backward(0, self.B, want_params=True, want_dx=True)
        self.E.backward(0, self.B, want_params=True)

    def _y_apply(self):
        self.y_opt.step(self._scale)
        self._repack_y()

    def _x_grads(self):
        self._encode(False)                                                 # forward only: no gradient enters the encoder
        self._decode_x(True)
        self._mse(self.Dx, self.x_stage, 3, self.scal, 0)
        self.Dx.backward(0, self.B, want_params=True)

    def _x_apply(self):
        self.x_opt.step(self._scale)
        self.Dx.repack()

    def y_step(self, batch):
        self._stage(self._batch(batch))
        self.optimizer_step(self.y_store, ('a_y_grads', self._y_grads), ('a_y_apply', self._y_apply), 'y_step')

    def x_step(self, batch):
        self._stage(self._batch(batch))
        self.optimizer_step(self.x_store, ('a_x_grads', self._x_grads), ('a_x_apply', self._x_apply), 'x_step')

    def _scalars(self):
        return self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()

    def losses(self):
        """The reference's `losses` collection (:79-82) of the last fetches: x_hat_loss of the last x step's batch, y_hat_loss
        and y_hat_rmse of the last y step's."""
        s = self._scalars()
        t = 'tower_%d/' % (self.sess.world_size - 1)
        return collection_to_dict([(t + 'x_hat_loss:0', s[0]), (t + 'y_hat_loss:0', s[2]), (t + 'y_hat_rmse:0', s[3])])

    def train(self, sess=None, args=None, feed_dict=None):
        """:65-68: the y step, then the x step on the next batch."""
        self.y_step(self.x_y.next_batch())
        self.x_step(self.x_y.next_batch())
        s = self._scalars()
        return {'x_loss': s[0], 'y_loss': s[2]}

    # ---- inference, evaluation, summaries --------------------------------------------------------------------
    def _forward_body(self):
        self._encode(False)
        self.Dy.forward(0, self.B, keep_pre=False)
        self._decode_x(False)

    def _outputs01(self):
        out = []
        for net, c in ((self.Dx, 3), (self.Dy, 1)):
            h = net.layers[-1].h
            out.append((h.buf.float().reshape(self.B, SIDE, SIDE, h.cs)[..., :c] + 1.0) * 0.5)
        return tuple(out)

    def infer(self, batch):
        """(xhat01, yhat01), f32 [B,256,256,3] and [B,256,256,1] in [0, 1], of one batch (the dataset's tuple; its y is staged but
        not read).  Every batch-norm layer normalises with THIS pass's batch statistics -- the reference has no inference mode
        and keeps no moving averages a later pass could use --, so the rows of a batch depend on each other.  It writes the
        staging buffers and the activations, which every step rewrites, and no result of the last fetch."""
        self._stage(self._batch(batch))
        self._run('a_forward', self._forward_body)
        return self._outputs01()

    def _eval_body(self):
        self._forward_body()
        self._mse(self.Dx, self.x_stage, 3, self.eval_scal, 0, seed=False)
        self._mse(self.Dy, self.y_stage, 1, self.eval_scal, 2, seed=False)
        self.eval_acc.add_(self.eval_scal)

    def evaluate(self, source, n_batches):
        """{'x_hat_loss', 'y_hat_loss', 'y_hat_rmse', 'images', 'n_batches'} over `n_batches` batches of `source`: the mean over
        the batches of each batch's losses, forward only (tdg_artist_mse in mode 0), accumulated on the device (f64) and read
        once.  Variables, optimizer state and losses() are untouched; the staging buffers and activations are not."""
        n_batches = int(n_batches)
        if n_batches < 1:
            raise ValueError('evaluate: n_batches must be at least 1, got %r' % n_batches)
        self.eval_acc.zero_()
        for _ in range(n_batches):
            self._stage(self._batch(source.next_batch()))
            self._run('a_evaluate', self._eval_body)
        a = (self.eval_acc / n_batches).cpu().tolist()
        return {'x_hat_loss': a[0], 'y_hat_loss': a[2], 'y_hat_rmse': a[3], 'images': n_batches * self.B, 'n_batches': n_batches}

    def montages(self):
        """[(name, image [H, W, C] in [0, 1])] of write_montages' four montages (also the image summaries of an event)."""
        self._run('a_forward', self._forward_body)
        x_hat, y_hat = self._outputs01()
        n = int(math.floor(math.sqrt(min(int(self.args.examples), self.B))))
        if n < 1:
            raise ValueError('write_montages: --examples %r leaves no image' % self.args.examples)
        out = []
        for name, t, colorize in (('x', self.x_stage, False), ('y', self.y_stage, True), ('x_hat', x_hat, False), ('y_hat', y_hat, True)):
            a = t[:n * n].cpu().numpy()
            out.append((name, summaries.montage(summaries.jet(a[..., 0]) if colorize else a, n, n)))
        return out

    def write_montages(self, directory, epoch):
        """The four montages of :86-98 -- x, y (jet colours), x_hat, y_hat (jet colours) -- of the first `--examples` images of
        the batch in the staging buffers (the last one fetched), in an n x n grid, n = floor(sqrt(examples)), as
        `montage-<name>-<epoch>.png`.  The reconstructions come from a forward pass of their own on that batch.  Returns the
        paths.  DEVIATION: the reference hands hem.montage all `examples` images with height = width = n; where examples is not
        a square the grid holds the first n n of them."""
        os.makedirs(directory, exist_ok=True)
        written = []
        for name, img in self.montages():
            path = os.path.join(directory, 'montage-%s-%04d.png' % (name, epoch))
            summaries.write_png(path, img)
            written.append(path)
        return written
