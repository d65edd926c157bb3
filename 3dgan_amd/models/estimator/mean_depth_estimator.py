"""Scene mean-depth regressor on MI355X -- the reference's gen-2 plugin `hem/models/mean_depth_estimator.py` (arguments :13-26,
__init__ :29-79, train :81-86, E2 :94-121, loss :136-147) on the HIP kernels: a whole frame resized to 53x70 -> one number in
[0, 1], trained on |mean(depth) - m|.  It is what produces a mean depth WITHOUT ground truth for the `mean_*` versions of the
depth models, and the `estimator` of the reference's experimental_sampler / improved_sampler.

    E2    l1..l6  conv2d 5x5 stride 2 SAME xavier relu   53x70x3 -> 27x35 -> 14x18 -> 7x9 -> 4x5 -> 2x3 -> 1x2, widths WIDTHS[:6]
          flatten                                        1x2x2048 -> 4096
          l7      dense 4096 -> 2048, no activation (the builder's default)
          l8      dense 2048 -> 1, sigmoid               m

Variables are `model/vars/l1/weights` ... `model/vars/l8/bias`.  One optimizer from the global --optimizer / --lr
(`init_optimizer`, :32), unlike the paper_* plugins.

Inputs: the LAST two tensors of the batch, the originals x_full [B,53,70,3] and y_full [B,53,70,1] of the nyuv2 flags
`--include_originals 53 70` (with the reference's flag set these are x_y[4], x_y[5], :46-49).  x is used as it comes, in [0, 1].

Flatten order: flatten here is the free NHWC reinterpretation, so l7's 4096 input rows are ordered (w, c) -- row w * 2048 + c
reads channel c of column w -- where the reference's NCHW flatten orders them (c, w).  A checkpoint exchanged with the
reference permutes l7's rows accordingly; the function computed is the same.

Loss (tdg_mde_loss): mean_i = mean of image i's 3710 depth values, loss = (1/B) sum_i |mean_i - m_i|.  DEVIATION: the reference
writes sqrt(square(d)), whose TensorFlow gradient at d == 0 is NaN; here the gradient there is 0.

Loss dict: {'Mean_1': value}, this batch's at the variables before the update.  The reference adds the unnamed tensor `l` to the
`losses` collection (:146) and `collection_to_dict` (hem/util/misc.py:19-25) keys it by the last component of its name.  The
loss is built inside tower_scope_range's `tf.name_scope('tower_0')` (hem/util/scoping.py:87) and holds two reduce_mean calls:
`tf.reduce_mean(y, axis=[2, 3])` is `tower_0/Mean`, so the second, the loss, is uniquified to `tower_0/Mean_1:0` -> 'Mean_1'.
(The model's own ops live under `tower_0/model/...` and take no name from this scope.)

One train(): the batch's originals into the staging buffers; ONE captured gradient body -- cast, six convs, two dense layers,
tdg_mde_loss, the sigmoid's derivative, the backward pass --; the finite check and the exchange; one optimizer step.
"""
import torch

from ... import _lib
from ... import kernels as K
from ... import engine
from ...ops.layers import conv2d, dense, flatten, arg_scope, variable_scope, placeholder, reset_graph
from ...ops.activations import relu, sigmoid
from ...util import tower_scope_range, init_optimizer, collection_to_dict
from ..ModelPlugin import ModelPlugin


class mean_depth_estimator(ModelPlugin, engine.Replica):
    name = 'mean_depth_estimator'
    WIDTHS = (64, 128, 256, 512, 1024, 2048, 2048)        # l1 .. l7; a test builds a narrow copy by overriding this alone
    FULL = (53, 70)                                       # rows, columns of the originals

    @staticmethod
    def arguments():
        """:13-26."""
        return {
            '--m_arch': {'type': str, 'default': 'E2', 'choices': ['E2'], 'help': 'Architecture to use.'},
            '--examples': {'type': int, 'default': 64, 'help': 'Number of image summary examples to use.'},
        }

    # ------------------------------------------------------------------------------ builders
    @classmethod
    def E2(cls, x, args, reuse=False):
        """:94-121."""
        w = cls.WIDTHS
        with arg_scope([conv2d], reuse=reuse, stride=2, padding='SAME', filter_size=5, init='xavier', activation=relu):
            l1 = conv2d(x, x.shape[-1], w[0], name='l1')   # 27x35
            l2 = conv2d(l1, w[0], w[1], name='l2')         # 14x18
            l3 = conv2d(l2, w[1], w[2], name='l3')         # 7x9
            l4 = conv2d(l3, w[2], w[3], name='l4')         # 4x5
            l5 = conv2d(l4, w[3], w[4], name='l5')         # 2x3
            l6 = conv2d(l5, w[4], w[5], name='l6')         # 1x2
            f = flatten(l6)                                # 2 * w[5], ordered (w, c)
            l7 = dense(f, f.shape[-1], w[6], name='l7')
            l8 = dense(l7, w[6], 1, activation=sigmoid, name='l8')
        return l8

    @classmethod
    def build_graph(cls, args):
        """Record the network for `args` (no device work); returns the Net `model`."""
        arch = getattr(args, 'm_arch', 'E2')
        if arch != 'E2':
            raise ValueError('mean_depth_estimator: unknown --m_arch %r' % arch)
        reset_graph()
        with variable_scope('model') as net:
            cls.E2(placeholder((None,) + cls.FULL + (3,)), args)
        return net

    # ------------------------------------------------------------------------------ construction
    def __init__(self, x_y, args, sess=None):
        engine.Replica.__init__(self, args, sess)
        self.x_y, sess = x_y, self.sess
        B = self.B = args.batch_size
        dev, dt = sess.device, sess.dtype
        (fh, fw), self.hw = self.FULL, self.FULL[0] * self.FULL[1]
        for _ in tower_scope_range(None, args.n_gpus, B, sess):
            self.net = self.build_graph(args)
        self.ws = K.Workspace(dev)
        self.store = engine.ParamStore(dev)
        self.M = engine.SeqNet(self.net, B, (fh, fw, 3), dt, dev, self.store, ws=self.ws)
        self.last = self.M.layers[-1]
        if not self.last.rowdot:
            raise ValueError('mean_depth_estimator: the last layer must be a dense layer with one output')
        self.M.declare_variables()
        self.store.allocate()
        self.M.init_variables(torch.Generator().manual_seed(sess.seed))
        self.opt = init_optimizer(args, self.store)                         # :32
        self.register('model', self.store, self.opt, self.M.repack)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.x_stage, self.y_stage = self.staging((B, fh, fw, 3), (B, fh, fw, 1))
        self.pred_x = f32(B, fh, fw, 3)                                     # predict()'s own input
        self.mean, self.gm, self.scal = f32(B), f32(B), f32(4)              # of the last loss fetch: mean_i, dL/dm_i, the loss
        self.eval_mean, self.eval_gm, self.eval_scal = f32(B), f32(B), f32(4)       # evaluate()'s own
        self.eval_acc = torch.zeros(1, dtype=torch.float64, device=dev)
        nbytes = _lib.load().tdg_mde_loss_workspace_bytes(B)
        self.loss_ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.refresh()

    # ---- pieces ------------------------------------------------------------------------------------------
    def _originals(self, batch):
        """(x_full, y_full): the last two tensors of the batch."""
        (fh, fw), ok = self.FULL, isinstance(batch, (tuple, list)) and len(batch) >= 2
        if ok:
            x, y = batch[-2], batch[-1]
            ok = tuple(x.shape) == (self.B, fh, fw, 3) and tuple(y.shape) == (self.B, fh, fw, 1)
        if not ok:
            got = [tuple(t.shape) for t in batch] if isinstance(batch, (tuple, list)) else type(batch).__name__
            raise ValueError('mean_depth_estimator reads the originals, [B,%d,%d,3] and [B,%d,%d,1], as the last two tensors of '
                             'the batch: run the dataset with --include_originals %d %d (got %s)' % (fh, fw, fh, fw, fh, fw, got))
        return x, y

    def _forward(self, x32):
        """m of the f32 batch `x32`, used as it comes (:46-49: no rescale), into the last layer's f32 output."""
        fh, fw = self.FULL
        _lib.call('tdg_affine_cast_rows', self.sess.dtype, K.ptr(x32), self.B * fh * fw, 3, self.M.x.cs, 1.0, 0.0, self.M.x.ptr(0),
                  K.stream())
        return self.M.forward(0, self.B)

    def _loss(self, mean, gm, scal):
        """tdg_mde_loss on the staged depth and the f32 m: the means, dL/dm and the loss."""
        _lib.call('tdg_mde_loss', K.F32, K.ptr(self.y_stage), self.B, self.hw, K.ptr(self.last.out), 1, K.ptr(mean), K.ptr(gm), 1,
                  K.ptr(scal), K.ptr(self.loss_ws), self.loss_ws.numel(), K.stream())

    # ---- the step ------------------------------------------------------------------------------------------
    def _grads(self):
        self._forward(self.x_stage)
        self._loss(self.mean, self.gm, self.scal)
        # the dense head takes dL/dlogit: dL/dm times the sigmoid's derivative from its stored output
        _lib.call('tdg_act_bwd', K.F32, K.ptr(self.gm), K.ptr(self.last.out), self.B, K.ACT_SIGMOID, 0.0, K.ptr(self.last.seed),
                  K.stream())
        self.M.backward(0, self.B, want_params=True)

    def _apply(self):
        self.opt.step(self._scale)
        self.M.repack()

    def _losses(self):
        s = self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()
        return collection_to_dict([('tower_%d/Mean_1:0' % (self.sess.world_size - 1), s[0])])

    def train(self, sess=None, args=None, feed_dict=None):
        """:81-86: one sess.run of the train op and the loss -- one batch, the loss at the variables before the update."""
        self._stage(self._originals(self.x_y.next_batch()))
        self.optimizer_step(self.store, ('m_grads', self._grads), ('m_apply', self._apply), 'train')
        return self._losses()

    # ---- inference and evaluation --------------------------------------------------------------------------
    def predict(self, x_full):
        """m, f32 [B], of a [B,53,70,3] batch in [0, 1] (torch or NumPy).  It has an input buffer of its own; training state and
        the last loss fetch are untouched."""
        x = torch.as_tensor(x_full).to(device=self.sess.device, dtype=torch.float32)
        if tuple(x.shape) != tuple(self.pred_x.shape):
            raise ValueError('predict: expected %s, got %s' % (tuple(self.pred_x.shape), tuple(x.shape)))
        self.pred_x.copy_(x)
        return self._forward(self.pred_x)[:self.B].clone()

    def _eval_body(self):
        self._forward(self.x_stage)
        self._loss(self.eval_mean, self.eval_gm, self.eval_scal)
        self.eval_acc.add_(self.eval_scal[:1])

    def evaluate(self, source, n_batches):
        """{'mean_abs_error', 'images', 'n_batches'} over `n_batches` batches of `source`: the mean over the batches of each
        batch's mean |mean_i - m_i|, accumulated on the device (f64) and read once.  Training state is untouched."""
        n_batches = int(n_batches)
        if n_batches < 1:
            raise ValueError('evaluate: n_batches must be at least 1, got %r' % n_batches)
        self.eval_acc.zero_()
        for _ in range(n_batches):
            self._stage(self._originals(source.next_batch()))
            self._run('evaluate', self._eval_body)
        return {'mean_abs_error': float(self.eval_acc.item()) / n_batches, 'images': n_batches * self.B, 'n_batches': n_batches}
