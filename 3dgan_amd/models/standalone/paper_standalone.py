"""The control experiment of the thesis' depth tables on MI355X -- the reference's gen-2 plugin `hem/models/paper_standalone.py`
(arguments :14-35, __init__ :37-134, train :136-138, generators :140-242, loss :244-253) on the HIP kernels: paper_cgan's
65x65 RGB -> 29x29 depth U-Net trained on the RMSE regression loss alone.  No critic, one Adam (:40; the global --optimizer /
--lr do not apply), one batch per train().

    version          generator                                                      y_hat
    baseline         g_baseline: paper_cgan's                                       g
    mean_adjusted    g_baseline                                                     g + y_bar
    mean_provided    g_mean_provided: [e1 | y_bar] 31x31x65 -> e2, and the head     g + y_bar
                     reads [d3 | e1 | y_bar] 31x31x129
    mean_provided2   g_mean_provided2: [x | 1] 65x65x4 -> e1                        g + y_bar

Inputs are paper_cgan's: y = crop(10 y01, 17, 17, 29, 29), y_bar its per-image mean (depth units).  The y_bar channel of
`mean_provided` is data, FED per pass: the U-Net executor keeps it the zero-copy channel window `--noise_layer e1` of
paper_sampler uses (unet.py), tdg_cgan_bar_fill writes it after tdg_cgan_prep has produced y_bar, and the 1x1 head reads it as an
f32 plane through tdg_cgan_head_noise_fwd / _bwd.  It takes part in no Philox draw and nobody reads its gradient.

Loss: rmse = sqrt(mean((y_hat/10 - y/10)^2)) over all B*841 elements of the replica's batch, one scalar (tdg_cgan_rmse_loss,
forward and gradient, f64 sums in a fixed order); the loss dict is {'rmse': value}, this batch's at the variables before the
update.  DEVIATION: a batch with y_hat == y everywhere gives loss 0 and a zero gradient where TensorFlow's sqrt gives NaN.

One train(): stage the batch; ONE captured gradient body -- prep, (bar_fill), U-Net forward, head, loss, head backward, U-Net
backward --; the finite check and the exchange; Adam on the one part `generator`.  metrics(), set_mean_image, dataset_moments,
evaluate, infer and infer_full are paper_cgan's (GeneratorReplica): the generator has no batch norm.
"""
import torch

from ... import _lib
from ... import kernels as K
from ... import engine
from ...ops.layers import conv2d, deconv2d, concat, arg_scope, variable_scope, placeholder
from ...ops.activations import _lrelu, relu
from ...util import collection_to_dict
from ..ModelPlugin import ModelPlugin
from ..paper.paper_cgan import GeneratorReplica, CROP

VERSIONS = {'baseline': 0, 'mean_adjusted': 1, 'mean_provided2': 2, 'mean_provided': 3}


def standalone_arguments(versions):
    """:14-35."""
    return {
        '--g_lr': {'type': float, 'default': 1e-3, 'help': 'Learning rate for generator.'},
        '--g_beta1': {'type': float, 'default': 0.9, 'help': 'Beta1 for generator'},
        '--g_beta2': {'type': float, 'default': 0.999, 'help': 'Beta2 for generator.'},
        '--model_version': {'type': str, 'default': 'baseline', 'choices': list(versions), 'help': 'Which version of the model to run.'},
    }


class StandaloneReplica(GeneratorReplica):
    """paper_standalone and paper_baseline_standalone: GeneratorReplica with the fed y_bar channel, the RMSE loss and one Adam."""

    VERSIONS = VERSIONS

    @classmethod
    def check_version(cls, version):
        if version not in [c for c in cls.arguments()['--model_version']['choices']]:
            raise ValueError('%s: unknown --model_version %r' % (cls.name, version))

    @classmethod
    def generator(cls, x, args, reuse=False):
        """g_baseline / g_mean_provided2 are GeneratorReplica's; g_mean_provided (:176-207) concatenates a 31x31 channel of
        y_bar behind e1, so e2 is a 65 -> 128 conv and the head a 129 -> 1 conv."""
        if cls._version_name(args) != 'mean_provided':
            return GeneratorReplica.generator(x, args, reuse)
        B = args.batch_size
        with variable_scope('encoder'), arg_scope([conv2d], reuse=reuse, filter_size=5, stride=2, padding='VALID', init='xavier',
                                                  activation=relu):
            e1 = conv2d(x, x.shape[-1], 64, name='e1')          # 31x31x64
            e1 = concat([e1, placeholder((None, 31, 31, 1), 'y_bar')])      # 31x31x65
            e2 = conv2d(e1, 65, 128, name='e2')                 # 14x14x128
            e3 = conv2d(e2, 128, 256, name='e3')                # 5x5x256
            e4 = conv2d(e3, 256, 512, name='e4')                # 1x1x512
        with variable_scope('decoder'), arg_scope([deconv2d, conv2d], reuse=reuse, filter_size=5, stride=2, init='xavier',
                                                  padding='VALID', activation=_lrelu(0.2)):
            y = deconv2d(e4, 512, 256, output_shape=(B, 256, 5, 5), name='d1')
            y = concat([y, e3])                                # 5x5x512
            y = deconv2d(y, 512, 128, output_shape=(B, 128, 14, 14), name='d2')
            y = concat([y, e2])                                # 14x14x256
            y = deconv2d(y, 256, 64, output_shape=(B, 64, 31, 31), name='d3')
            y = concat([y, e1])                                # 31x31x129
            y = conv2d(y, 129, 1, stride=1, filter_size=1, padding='SAME', activation=None, name='d4')   # 31x31x1
        return y

    def _setup(self, args, gen):
        """The one optimizer (:40) and the loss kernel's buffers."""
        self.g_opt = engine.Adam(self.g_store, args.g_lr, args.g_beta1, args.g_beta2)
        self.register('generator', self.g_store, self.g_opt, self.G.repack)
        nbytes = _lib.load().tdg_cgan_rmse_loss_workspace_bytes(self.B, CROP * CROP)
        self.rmse_ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.sess.device)

    # ---- the step ------------------------------------------------------------------------------------------
    def _grads(self):
        self._inputs(self.ybar, self.crop)
        self._generate(self.ybar, self.yhat)
        _lib.call('tdg_cgan_rmse_loss', self.sess.dtype, K.ptr(self.crop), K.ptr(self.yhat), self.B, CROP * CROP, self.dfake.ptr(0),
                  self.dfake.cs, K.ptr(self.scal), K.ptr(self.rmse_ws), self.rmse_ws.numel(), K.stream())
        self._g_backward()

    def _apply(self):
        self.g_opt.step(self._scale)
        self.G.repack()

    def _losses(self):
        s = self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()
        return collection_to_dict([('tower_%d/loss/rmse:0' % (self.sess.world_size - 1), s[0])])

    def _train(self):
        """:136-138: one sess.run of the train op and the loss -- one batch, the loss at the variables before the update."""
        self._stage(self.x_y.next_batch())
        self.optimizer_step(self.g_store, ('g_grads', self._grads), ('g_apply', self._apply), 'train')
        return self._losses()


class paper_standalone(ModelPlugin, StandaloneReplica):
    name = 'paper_standalone'

    @staticmethod
    def arguments():
        return standalone_arguments(['baseline', 'mean_adjusted', 'mean_provided', 'mean_provided2'])

    def train(self, sess=None, args=None, feed_dict=None):
        return self._train()
