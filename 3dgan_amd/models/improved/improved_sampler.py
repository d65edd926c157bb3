"""The depth sampler cGANs A1-A3, B2, D1 and E1 on MI355X -- the reference's gen-2 plugin `hem/models/improved_sampler.py`
(arguments :16-43, __init__ :67-246, train :248-259, generators :262-540, discriminators :638-808, loss :911-952,
sampler_summaries :1014-1034), driven by train.py, on the HIP kernels.  experimental_sampler is the E2 row of this family.

Inputs (:109-181).  The batch is the dataset's tuple: (x, y), (x, y, x_loc, y_loc) or (x, y, x_loc, y_loc, mean_vec); longer
tuples are accepted and only the leading entries read, as in the reference.  x <- 2x - 1 and y <- 2y - 1 as hem.rescale computes
them in f32; the location planes and mean_vec are used as they come.  tdg_isamp_prep writes every input tensor in one pass.

    g_arch  source  X                                   depth target                 nyuv2 flags of the reference's config
    A1-A3   65x65   rgb (3)                             31x31 at (17, 17)            --random_crop 65 65
    B2      64x64   rgb (3)                             32x32 at (16, 16)            --random_crop 64 64
    D1      64x64   rgb, x_loc, y_loc (5)               32x32 at (16, 16)            --random_crop 64 64 --include_location
    E1      64x64   rgb, x_loc, y_loc, mean_vec (6)     32x32 at (16, 16)            the latter plus --normalize

    (A1's target is hem.center_crop(y, 0.4769): int((65 - 65 * 0.4769) / 2) = 17 on either side, 65 - 34 = 31.)

Generators (:262-540).  Every one concatenates u ~ U(-1, 1) [B,S,S,1] behind X (U-Net node `x`, injection key `noise_x`).
    A1, A2, A3     e1..e4  conv2d 5x5 stride 2 VALID relu          31x31x64, 14x14x128, 5x5x256, 1x1x512
                   d1..d3  deconv2d 5x5 stride 2 VALID lrelu 0.2   5x5x256, 14x14x128, 31x31x64, each concat e3, e2, e1
                   d4      conv2d 1x1, 128 -> 1, tanh              31x31x1
                   batch norm: A1 on e2..e4, d1..d3 AND d4 (the decoder's arg_scope sets use_batch_norm for hem.conv2d too, so
                   d4 is conv, batch norm, tanh: tdg_isamp_head_bn_fwd / _bwd); A2 on e2, e3 only; A3 none.
    B2, D1, E1     experimental_sampler's generator E2 with e1 reading 3 + 1, 5 + 1 and 6 + 1 planes; no batch norm.
Critics (:638-808).
    A1             rgb_path hx1..hx4 on 65x65x3 and depth_path hy1..hy3 on 31x31x1, 5x5 stride 2 VALID lrelu 0.2 -> 1x1x512 each;
                   combined_path 1x1 convs 1024 -> 1024 -> 512 -> 1 (paper_cgan's critic shape).
    B2, D1, E1     experimental_sampler's critic E2 with 3, 5 and 6 rgb-path planes.
The pairs that fit are (A1 | A2 | A3, A1), (B2, B2), (D1, D1), (E1, E1); any other pair is a ValueError naming them (a shape
error deep in graph building in the reference).  B1 and C1 (66x66 crops, filters 4, 3 and 6) are NOT BUILT: their 6x6 layers have
36 taps and the conv kernels hold 32 (IG_MAX_TAPS).  E2 is `--model experimental_sampler`.

Variables: `generator/{encoder,decoder}/vars/<layer>/{weights,bias}`, `discriminator/{rgb_path,depth_path,combined_path}/vars/...`,
batch-norm betas `generator/{encoder,decoder}/BatchNorm[_i]/beta` (Net.bn_name).  E1's names are experimental_sampler's.
Batch norm runs in training mode everywhere (the reference has no inference mode) and keeps no moving averages, like the
project's other batch-norm models.  DEVIATION: contrib batch_norm makes a fresh `BatchNorm_i` scope per CALL, so the reference's
three summary passes read betas of their own that no gradient ever reaches (zeros); here every pass reads the trained betas.

Loss (:911-952): sigmoid cross-entropy g_fake, d_real, d_fake, d_total = d_real + d_fake; rmse and l1 compare (g + 1) / 2 with
(y + 1) / 2.  The dict holds g_fake, d_real, d_fake, d_total, rmse, l1; with `--g_sparsity` also g_total, sparsity_term; with
`--g_rmse` alone also g_total.
    --g_rmse       G trains on g_total = g_fake + rmse: d rmse / d g = (g - y) / (4 N rmse) on the [-1, 1] tensors, N = B T T per
                   replica, is added to dL/dg before the head's backward pass (tdg_isamp_rmse_grad; no guard at rmse == 0: as
                   in TF the gradient is then not finite and the finite check reports it).
    --g_sparsity   sparsity_term = tf.nn.zero_fraction of e5's relu output in the training pass (tdg_isamp_zero_fraction),
                   g_total = g_fake - sparsity_term (+ rmse).  zero_fraction has no gradient: the term is reported only, the
                   gradients are those of the run without the flag.  A1-A3 have no e5 (a NameError in the reference): a
                   ValueError at construction.  DEVIATION: with several towers the reference reads tower 0's e5 in every tower
                   (the first name match in the `conv_layers` collection); here each rank reads its own.
Optimizers (:70-71): two instances of init_optimizer(args).

train() (:248-259) is ONE sess.run of [d_train_op, g_train_op, all_losses], as experimental_sampler.train: the batch into the
staging buffers; ONE captured gradient body (prep, G forward, head, the critic over 2B, xent mode 1, the critic's backward pass
for its parameters over both halves, xent mode 2, a data-only backward pass through the fake half to dL/dg, [tdg_p2p_l1,
tdg_isamp_rmse_grad], head backward, U-Net backward, tdg_p2p_l1, [tdg_isamp_zero_fraction]); the finite check and the exchange
on both stores; ONE captured apply body with both optimizer steps and both repacks; global_step advanced by 2.

metrics() (:175-181, :1014-1034): three more generator passes, each with a fresh noise channel -- `sampler` (row 0 of X and of
y broadcast over the batch), `shuffled` (tf.random_shuffle(X): all planes of X permuted together, against the UNpermuted y) and
`noise` (X replaced by U(-1, 1) of X's shape, against the sampler set's y) -- and per set the four statistics of
tdg_cgan_sample_stats, plus the losses of the last fetch.  The permutation is drawn on the host per call (injection key
`shuffle`), the noise set's input on the device (injection key `x_noise`).
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

# g_arch -> (source side, crop side, crop offset, planes of X)
GEOMETRY = {'A1': (65, 31, 17, 3), 'A2': (65, 31, 17, 3), 'A3': (65, 31, 17, 3), 'B2': (64, 32, 16, 3), 'D1': (64, 32, 16, 5),
            'E1': (64, 32, 16, 6)}
D_ARCHS = ('A1', 'B2', 'D1', 'E1')
PAIRS = (('A1', 'A1'), ('A2', 'A1'), ('A3', 'A1'), ('B2', 'B2'), ('D1', 'D1'), ('E1', 'E1'))
PAIRS_TEXT = '(A1 | A2 | A3, A1), (B2, B2), (D1, D1), (E1, E1)'
NOT_BUILT = ('B1', 'C1')
# the batch-normed layers of generator A: (encoder, decoder incl. the head d4)
A_BATCH_NORM = {'A1': (('e2', 'e3', 'e4'), ('d1', 'd2', 'd3', 'd4')), 'A2': (('e2', 'e3'), ()), 'A3': ((), ())}
# the nyuv2 flags of the matching reference config (examples/improved_sampler/*.config)
DATA_FLAGS = {3: '--random_crop %d %d', 5: '--random_crop %d %d --include_location', 6: '--random_crop %d %d --include_location --normalize'}
TUPLES = {3: '(x, y)', 5: '(x, y, x_loc, y_loc)', 6: '(x, y, x_loc, y_loc, mean_vec)'}
BN_EPS = 1e-3                                     # tf.contrib.layers.batch_norm's default epsilon
SETS = ('sampler', 'shuffled', 'noise')
SET_KEYS = tuple(k % s for s in SETS for k in ('moments/%s/moments/mean', 'moments/%s/moments/var')) + \
    tuple(k % s for s in SETS for k in ('per_image_metrics/%s/rmse/mean', 'per_image_metrics/%s/rmse/min'))


class improved_sampler(ModelPlugin, engine.Replica):
    name = 'improved_sampler'

    @staticmethod
    def arguments():
        """:16-43."""
        return {
            '--g_sparsity': {'action': 'store_true', 'default': False,
                             'help': 'Set this to add a sparsity term (for the encoder output/activation) to the loss function.'},
            '--g_rmse': {'action': 'store_true', 'default': False,
                         'help': 'Setting this will add a RMSE loss term to the generator.'},
            '--g_arch': {'type': str, 'default': 'A1',
                         'help': 'Architecture to use for the generator. Options are: A1, A2, A3, B2, D1, E1.'},
            '--d_arch': {'type': str, 'default': 'A1',
                         'help': 'Architecture to use for the discriminator. Options are: A1, B2, D1, E1.'},
            '--examples': {'type': int, 'default': 64, 'help': 'Number of image summary examples to use.'},
        }

    # ------------------------------------------------------------------------------ builders
    @staticmethod
    def generatorA(x, args, arch, reuse=False):
        """:262-362: X [B,65,65,3] -> the recorded 31x31x1 tanh head d4; `arch` chooses the batch-normed layers."""
        B = args.batch_size
        bn_e, bn_d = A_BATCH_NORM[arch]
        with variable_scope('encoder'), arg_scope([conv2d], reuse=reuse, filter_size=5, stride=2, padding='VALID', init='xavier',
                                                  activation=relu):
            h = concat([x, random_uniform([B, 65, 65, 1], minval=-1.0, maxval=1.0)])       # 65x65x4
            e1 = conv2d(h, 4, 64, name='e1')                                               # 31x31x64
            e2 = conv2d(e1, 64, 128, use_batch_norm='e2' in bn_e, name='e2')               # 14x14x128
            e3 = conv2d(e2, 128, 256, use_batch_norm='e3' in bn_e, name='e3')              # 5x5x256
            e4 = conv2d(e3, 256, 512, use_batch_norm='e4' in bn_e, name='e4')              # 1x1x512
        with variable_scope('decoder'), arg_scope([deconv2d, conv2d], reuse=reuse, filter_size=5, stride=2, init='xavier',
                                                  padding='VALID', activation=_lrelu(0.2)):
            y = deconv2d(e4, 512, 256, output_shape=(B, 256, 5, 5), use_batch_norm='d1' in bn_d, name='d1')
            y = concat([y, e3])                                                            # 5x5x512
            y = deconv2d(y, 512, 128, output_shape=(B, 128, 14, 14), use_batch_norm='d2' in bn_d, name='d2')
            y = concat([y, e2])                                                            # 14x14x256
            y = deconv2d(y, 256, 64, output_shape=(B, 64, 31, 31), use_batch_norm='d3' in bn_d, name='d3')
            y = concat([y, e1])                                                            # 31x31x128
            y = conv2d(y, 128, 1, stride=1, filter_size=1, padding='SAME', activation=tanh, use_batch_norm='d4' in bn_d, name='d4')
        return y

    @staticmethod
    def generatorE(x, args, planes, reuse=False):
        """:395-431, :465-540: X [B,64,64,planes] -> the recorded 32x32x1 tanh head d5 (experimental_sampler's generatorE2)."""
        B = args.batch_size
        with variable_scope('encoder'), arg_scope([conv2d], reuse=reuse, stride=2, padding='SAME', filter_size=5, init='xavier',
                                                  activation=relu):
            h = concat([x, random_uniform([B, 64, 64, 1], minval=-1.0, maxval=1.0)])       # 64x64x(planes + 1)
            e1 = conv2d(h, planes + 1, 64, name='e1')                                      # 32x32x64
            e2 = conv2d(e1, 64, 128, name='e2')                                            # 16x16x128
            e3 = conv2d(e2, 128, 256, name='e3')                                           # 8x8x256
            e4 = conv2d(e3, 256, 512, name='e4')                                           # 4x4x512
            e5 = conv2d(e4, 512, 1024, filter_size=4, padding='VALID', name='e5')          # 1x1x1024
        with variable_scope('decoder'), arg_scope([deconv2d, conv2d], reuse=reuse, stride=2, init='xavier', padding='SAME',
                                                  filter_size=5, activation=_lrelu(0.2)):
            y = deconv2d(e5, 1024, 512, output_shape=(B, 512, 4, 4), filter_size=4, padding='VALID', name='d1')
            y = concat([y, e4])                                                            # 4x4x1024
            y = deconv2d(y, 1024, 256, output_shape=(B, 256, 8, 8), name='d2')
            y = concat([y, e3])                                                            # 8x8x512
            y = deconv2d(y, 512, 128, output_shape=(B, 128, 16, 16), name='d3')
            y = concat([y, e2])                                                            # 16x16x256
            y = deconv2d(y, 256, 64, output_shape=(B, 64, 32, 32), name='d4')
            y = concat([y, e1])                                                            # 32x32x128
            y = conv2d(y, 128, 1, stride=1, filter_size=1, activation=tanh, name='d5')     # 32x32x1
        return y

    @staticmethod
    def discriminatorA1(x, y, args, reuse=False):
        """:638-663: x [B,65,65,3], depth [B,31,31,1] -> the logits [B,1,1,1]."""
        with arg_scope([conv2d], reuse=reuse, activation=_lrelu(0.2), init='xavier', padding='VALID', filter_size=5, stride=2):
            with variable_scope('rgb_path'):
                h1 = conv2d(x, 3, 64, name='hx1')                   # 31x31x64
                h1 = conv2d(h1, 64, 128, name='hx2')                # 14x14x128
                h1 = conv2d(h1, 128, 256, name='hx3')               # 5x5x256
                h1 = conv2d(h1, 256, 512, name='hx4')               # 1x1x512
            with variable_scope('depth_path'):
                h2 = conv2d(y, 1, 128, name='hy1')                  # 14x14x128
                h2 = conv2d(h2, 128, 256, name='hy2')               # 5x5x256
                h2 = conv2d(h2, 256, 512, name='hy3')               # 1x1x512
            with variable_scope('combined_path'):
                h = concat([h1, h2])                                # 1x1x1024
                h = conv2d(h, 1024, 1024, stride=1, filter_size=1, padding='SAME', name='h1')
                h = conv2d(h, 1024, 512, stride=1, filter_size=1, padding='SAME', name='h2')
                h = conv2d(h, 512, 1, stride=1, filter_size=1, padding='SAME', name='h3', activation=None)
        return h

    @staticmethod
    def discriminatorE(x, y, args, planes, reuse=False):
        """:690-808: X [B,64,64,planes], depth [B,32,32,1] -> the logits [B,1,1,1] (experimental_sampler's discriminatorE2)."""
        with arg_scope([conv2d], reuse=reuse, activation=_lrelu(0.2), init='xavier', padding='SAME', filter_size=5, stride=2):
            with variable_scope('rgb_path'):
                h1 = conv2d(x, planes, 64, name='hx1')              # 32x32x64
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
        """The (g_arch, d_arch) pair, checked: what is out of scope, what lives elsewhere, what does not exist, what does not fit."""
        g, d = getattr(args, 'g_arch', 'A1'), getattr(args, 'd_arch', 'A1')
        for flag, arch, known in (('g_arch', g, GEOMETRY), ('d_arch', d, D_ARCHS)):
            if arch in NOT_BUILT:
                raise NotImplementedError('improved_sampler: --%s %s is not built: its 6x6 layers have 36 filter taps and the conv '
                                          'kernels hold 32 (IG_MAX_TAPS); the archs that are: %s' % (flag, arch, PAIRS_TEXT))
            if arch == 'E2':
                raise ValueError('improved_sampler: --%s E2 is --model experimental_sampler (the estimator-fed arch has a plugin of '
                                 'its own)' % flag)
            if arch not in known:
                raise ValueError('improved_sampler: unknown --%s %r; the (g_arch, d_arch) pairs are %s' % (flag, arch, PAIRS_TEXT))
        if (g, d) not in PAIRS:
            raise ValueError('improved_sampler: --g_arch %s does not fit --d_arch %s; the (g_arch, d_arch) pairs are %s'
                             % (g, d, PAIRS_TEXT))
        if getattr(args, 'g_sparsity', False) and g in A_BATCH_NORM:
            raise ValueError('improved_sampler: --g_sparsity reads the encoder layer e5, which --g_arch %s does not have (B2, D1 and '
                             'E1 do)' % g)
        return g, d

    @classmethod
    def build_graph(cls, args):
        """Record the networks for `args` (no device work); returns the Nets by scope name."""
        g, d = cls.check_arch(args)
        S, T, _, P = GEOMETRY[g]
        reset_graph()
        X = placeholder((None, S, S, P))
        dy = placeholder((None, T, T, 1), 'y')
        with variable_scope('generator'):
            cls.generatorA(X, args, g) if g in A_BATCH_NORM else cls.generatorE(X, args, P)
        with variable_scope('discriminator'):
            for reuse in (False, True):                            # D(x, y) first, as :212-213
                cls.discriminatorA1(X, dy, args, reuse) if d == 'A1' else cls.discriminatorE(X, dy, args, P, reuse)
        from ...ops import layers as Lyr
        return {k: v for k, v in Lyr._nets.items() if v.passes}

    # ------------------------------------------------------------------------------ construction
    def __init__(self, x_y, args, sess=None):
        engine.Replica.__init__(self, args, sess)
        self.x_y, sess = x_y, self.sess
        for flag, spec in self.arguments().items():
            if not hasattr(args, flag.lstrip('-')):
                setattr(args, flag.lstrip('-'), spec['default'])
        self.g_arch, self.d_arch = self.check_arch(args)
        S, T, off, P = self.geometry = GEOMETRY[self.g_arch]
        self.g_rmse, self.g_sparsity = bool(args.g_rmse), bool(args.g_sparsity)
        B = self.B = args.batch_size
        dev, dt = sess.device, sess.dtype
        for _ in tower_scope_range(None, args.n_gpus, B, sess):
            nets = self.build_graph(args)
        self.enet, self.dec_net = nets['generator/encoder'], nets['generator/decoder']
        self.ws = K.Workspace(dev)
        self.g_store, self.d_store = engine.ParamStore(dev), engine.ParamStore(dev)
        # D: combined path over 2B (images [0,B) real, [B,2B) fake), depth path over 2B, rgb path over B
        cnet, rnet, dnet = (nets['discriminator/' + k] for k in ('combined_path', 'rgb_path', 'depth_path'))
        self.path_c = rnet.layers[-1].out_size                                     # each path's width at the join
        self.Dc = engine.SeqNet(cnet, 2 * B, (1, 1, 2 * self.path_c), dt, dev, self.d_store, need_input_grad=True, ws=self.ws)
        self.Dr = engine.SeqNet(rnet, B, (S, S, P), dt, dev, self.d_store, ws=self.ws)
        self.Dd = engine.SeqNet(dnet, 2 * B, (T, T, 1), dt, dev, self.d_store, need_input_grad=True, ws=self.ws)
        for net in (self.Dr, self.Dd, self.Dc):
            net.declare_variables()
        self.rgb_g, self.depth_g = self.Dr.layers[-1].gout, self.Dd.layers[-1].gout
        self.fake, self.dfake = self.Dd.x.view(B, B), self.Dd.dx.view(B, B)        # g lands in D's fake depth input
        # G: the U-Net allocates [X | noise] and hands over its last concat; the recorded layer behind it is this module's head
        self.G = UNet(self.enet, self.dec_net, B, dt, dev, self.g_store, self.ws, self.Dr.x, sess=sess)
        self.head, top = self.dec_net.layers[-1], self.G.top
        if self.G.xn is None or list(self.G.noise) != ['noise_x'] or len(self.dec_net.layers) != self.G.nd + 1 or \
                (self.head.k, self.head.out_size, self.head.in_size, top.h, top.w) != (1, 1, top.c, T, T):
            raise ValueError('improved_sampler: the generator must read [X | noise] and end in a 1x1 head on the %dx%d concat' % (T, T))
        # the derivative mask the head applies for the last decoder layer: none when that layer's batch norm applies it itself
        below = self.dec_net.layers[-2]
        self.head_mask = K.MASK_NONE if below.use_bn else K.MASK_LRELU
        self.head_leak = below.act.leak
        self.head_beta = None
        lib = _lib.load()
        if self.head.use_bn:                                                       # A1: conv, batch norm, tanh
            self.head_beta = self.dec_net.bn_name(0, len(self.dec_net.layers) - 1)
            self.g_store.declare(self.head_beta, (1,))
            self.head_ws = torch.zeros(lib.tdg_isamp_head_bn_workspace_bytes(B, self.head.in_size), dtype=torch.uint8, device=dev)
        else:
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
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.n_read = {3: 2, 5: 4, 6: 5}[P]                                        # leading tuple entries this arch reads
        self.batch_shapes = [(B, S, S, 3), (B, S, S, 1), (B, S, S, 1), (B, S, S, 1), (B, S, S, 1)][:self.n_read]
        self.stage = self.staging(*self.batch_shapes)
        self.g32, self.target, self.scal = f32(B, T, T), f32(B, T, T), f32(8)      # of the last loss fetch
        self.zhat, self.head_stats = (f32(B, T, T), f32(2)) if self.head.use_bn else (None, None)
        self.l1_ws = torch.zeros(2 * lib.tdg_reduce_workspace_bytes(B * T * T), dtype=torch.uint8, device=dev)
        self.zero_ws = torch.zeros(lib.tdg_isamp_zero_fraction_workspace_bytes(), dtype=torch.uint8, device=dev)
        # infer() / the summary passes / sample(): buffers of their own
        self.inf_g = f32(B, T, T)
        self.set_g, self.set_y = f32(B, T, T), {'sampler': f32(B, T, T), 'shuffled': f32(B, T, T)}
        self.zero_rows = torch.zeros(B, dtype=torch.int32, device=dev)
        self.perm = torch.zeros(B, dtype=torch.int32, device=dev)
        self.x_noise_u = f32(B * S * S * P)
        self.stat_out = {s: f32(6) for s in SETS}
        self.samp_mean, self.samp_var = f32(T, T), f32(T, T)
        self.samp = [f32(*s) for s in self.batch_shapes]
        self.stat_ws = torch.zeros(lib.tdg_cgan_sample_stats_workspace_bytes(B, T * T), dtype=torch.uint8, device=dev)
        self.refresh()

    def _repack_d(self):
        for net in (self.Dr, self.Dd, self.Dc):
            net.repack()

    # ---- pieces ------------------------------------------------------------------------------------------
    def _batch(self, batch):
        """The leading tensors this arch reads of the dataset's tuple, checked."""
        S, _, _, P = self.geometry
        ok = isinstance(batch, (tuple, list)) and len(batch) >= self.n_read and \
            [tuple(t.shape) for t in batch[:self.n_read]] == self.batch_shapes
        if not ok:
            got = [tuple(t.shape) for t in batch] if isinstance(batch, (tuple, list)) else type(batch).__name__
            raise ValueError('improved_sampler --g_arch %s reads %s at %dx%d: run the dataset with %s (got %s)'
                             % (self.g_arch, TUPLES[P], S, S, DATA_FLAGS[P] % (S, S), got))
        return tuple(batch[:self.n_read])

    def _prep(self, src=None, x_rows=None, y_rows=None, target=None, with_y=True):
        """tdg_isamp_prep: X into G's and D's inputs, the depth target into D's real half and `target`."""
        S, T, off, P = self.geometry
        src = tuple(src if src is not None else self.stage) + (None,) * 3
        x, y, xl, yl, mv = src[:5]
        xn, rx, dd = self.G.xn, self.Dr.x, self.Dd.x
        _lib.call('tdg_isamp_prep', self.sess.dtype, K.ptr(x), K.ptr(xl), K.ptr(yl), K.ptr(mv), K.ptr(y) if with_y else None,
                  K.ptr(x_rows), K.ptr(y_rows), self.B, S, T, off, P, xn.ptr(0), xn.cs, rx.ptr(0), rx.cs,
                  dd.ptr(0) if with_y else None, dd.cs, K.ptr(target) if with_y else None, K.stream())

    def _generate(self, g32):
        """The U-Net (fresh noise), then the head: g f32 into `g32`, rounded into channel 0 of D's fake depth input."""
        self.G.forward()
        top, st, name = self.G.top, self.g_store, self.dec_net.var_name
        w, b = K.ptr(st[name(self.head, 'weights')]), K.ptr(st[name(self.head, 'bias')])
        if self.head.use_bn:
            _lib.call('tdg_isamp_head_bn_fwd', self.sess.dtype, top.ptr(), self.B, top.h, top.c, top.cs, w, b, K.ptr(st[self.head_beta]),
                      BN_EPS, K.ptr(g32), K.ptr(self.zhat), K.ptr(self.head_stats), self.fake.ptr(0), self.fake.cs, K.ptr(self.head_ws),
                      self.head_ws.numel(), K.stream())
        else:
            _lib.call('tdg_xsamp_head_fwd', self.sess.dtype, top.ptr(), self.B, top.h, top.c, top.cs, w, b, K.ptr(g32), self.fake.ptr(0),
                      self.fake.cs, K.stream())

    def _head_backward(self):
        """From dL/dg in channel 0 of D's fake depth-input gradient and the g, zhat and statistics of the training pass."""
        top, gtop, st, name, dt = self.G.top, self.G.gtop, self.g_store, self.dec_net.var_name, self.sess.dtype
        w = K.ptr(st[name(self.head, 'weights')])
        dw, db = K.ptr(st.grad(name(self.head, 'weights'))), K.ptr(st.grad(name(self.head, 'bias')))
        if self.head.use_bn:
            _lib.call('tdg_isamp_head_bn_bwd', dt, self.dfake.ptr(0), self.dfake.cs, K.ptr(self.g32), K.ptr(self.zhat),
                      K.ptr(self.head_stats), top.ptr(), self.B, top.h, top.c, top.cs, w, self.head_mask, self.head_leak, gtop.ptr(), dw,
                      db, K.ptr(st.grad(self.head_beta)), K.ptr(self.head_ws), self.head_ws.numel(), K.stream())
        else:
            _lib.call('tdg_xsamp_head_bwd', dt, self.dfake.ptr(0), self.dfake.cs, K.ptr(self.g32), top.ptr(), self.B, top.h, top.c,
                      top.cs, w, self.head_mask, self.head_leak, gtop.ptr(), dw, db, K.ptr(self.head_ws), self.head_ws.numel() * 4,
                      K.stream())

    def _d_forward(self):
        B, dt, c = self.B, self.sess.dtype, self.path_c
        self.Dr.forward(0, B)
        self.Dd.forward(0, 2 * B)
        rh, dh = self.Dr.layers[-1].h, self.Dd.layers[-1].h
        _lib.call('tdg_cgan_join', dt, 0, B, 2 * B, c, self.Dc.x.ptr(0), self.Dc.x.cs, rh.ptr(0), rh.cs, dh.ptr(0), dh.cs, K.stream())
        self.Dc.forward(0, 2 * B)

    def _xent(self, mode):
        last = self.Dc.layers[-1]          # d_real, d_fake, g_fake to scal[4..6]
        _lib.call('tdg_p2p_xent', self.sess.dtype, last.h.ptr(0), self.B, last.h.cs, mode, last.gout.ptr(0), K.ptr(self.scal, 16),
                  K.stream())

    def _l1(self):
        """rmse and l1 on (g + 1) / 2 against (y + 1) / 2 into scal[1], scal[0]: the two halves of D's depth input share a row stride."""
        dd, rows = self.Dd.x, self.B * self.geometry[1] ** 2
        _lib.call('tdg_p2p_l1', self.sess.dtype, dd.ptr(0), dd.ptr(self.B), rows, dd.cs, 0.0, None, 0, K.ptr(self.scal), K.ptr(self.l1_ws),
                  self.l1_ws.numel(), K.stream())

    # ---- the step ------------------------------------------------------------------------------------------
    def _grads(self):
        B, dt, c = self.B, self.sess.dtype, self.path_c
        self._prep(target=self.target)
        self._generate(self.g32)
        self._d_forward()
        # D's gradients: both halves
        self._xent(1)
        self.Dc.backward(0, 2 * B, want_params=True, want_dx=True)
        dx = self.Dc.dx
        _lib.call('tdg_cgan_join', dt, 1, B, 2 * B, c, dx.ptr(0), dx.cs, self.rgb_g.ptr(0), self.rgb_g.cs, self.depth_g.ptr(0),
                  self.depth_g.cs, K.stream())
        self.Dd.backward(0, 2 * B, want_params=True)
        self.Dr.backward(0, B, want_params=True)
        # G's gradients from the same forward pass: data only through the fake half, D's parameter gradients stay
        self._xent(2)
        self.Dc.backward(B, B, want_params=False, want_dx=True)
        _lib.call('tdg_cgan_join', dt, 1, B, B, c, dx.ptr(B), dx.cs, None, 0, self.depth_g.ptr(B), self.depth_g.cs, K.stream())
        self.Dd.backward(B, B, want_params=False, want_dx=True)
        if self.g_rmse:                    # g_total = g_fake + rmse: the rmse first, then its gradient on top of dL/dg
            self._l1()
            dd = self.Dd.x
            _lib.call('tdg_isamp_rmse_grad', dt, dd.ptr(B), dd.ptr(0), B * self.geometry[1] ** 2, dd.cs, K.ptr(self.scal, 4),
                      self.dfake.ptr(0), self.dfake.cs, K.stream())
        self._head_backward()
        self.G.backward()
        if not self.g_rmse:
            self._l1()
        if self.g_sparsity:                # tf.nn.zero_fraction(e5) of this pass into scal[7]
            e5 = self.G.e_h[self.G.n]
            _lib.call('tdg_isamp_zero_fraction', dt, e5.ptr(0), B * e5.h * e5.w, e5.c, e5.cs, K.ptr(self.scal, 28), K.ptr(self.zero_ws),
                      self.zero_ws.numel(), K.stream())

    def _apply(self):
        self.d_opt.step(self._scale_d)
        self.g_opt.step(self._scale_g)
        self._repack_d()
        self.G.repack()

    def _losses(self):
        s = self.sess.report_scalars(self.scal, mean=getattr(self.args, 'mean_loss', False)).cpu().tolist()
        t = 'tower_%d/loss/' % (self.sess.world_size - 1)
        out = [(t + 'generator/g_fake:0', s[6]), (t + 'discriminator/d_real:0', s[4]), (t + 'discriminator/d_fake:0', s[5]),
               (t + 'discriminator/d_total:0', s[4] + s[5]), (t + 'rmse:0', s[1]), (t + 'l1:0', s[0])]
        if self.g_sparsity:                # :924-933, lambda_term = 1.0
            out += [(t + 'generator/g_total:0', s[6] - s[7] + (s[1] if self.g_rmse else 0.0)), (t + 'generator/sparsity_term:0', s[7])]
        elif self.g_rmse:
            out += [(t + 'generator/g_total:0', s[6] + s[1])]
        return collection_to_dict(out)

    def train(self, sess=None, args=None, feed_dict=None):
        """:248-259: one sess.run of both train ops and the losses."""
        self._stage(self._batch(self.x_y.next_batch()))
        self._run('is_grads', self._grads)
        for store in (self.d_store, self.g_store):
            self.sess.assert_finite(store, 'train')
        self._scale_d = self.sess.allreduce_mean_scale(self.d_store.grads)
        self._scale_g = self.sess.allreduce_mean_scale(self.g_store.grads)
        self._run('is_apply', self._apply)
        self.sess.global_step += 2
        return self._losses()

    # ---- inference and the summary sets ----------------------------------------------------------------------
    def infer(self, batch):
        """Depth in [0, 1], (g + 1) / 2, f32 [B,T,T,1] of one batch (the dataset's tuple; its y is not read).  The batch-norm archs
        (A1, A2) normalise EVERY pass with that pass's own batch statistics -- the reference has no inference mode and keeps no
        moving averages a later pass could use --, so their rows depend on each other; the rows of A3, B2, D1 and E1 are
        independent.  It writes the generator's activations and D's input buffers, which every step rewrites, and no result of
        the last fetch."""
        self._stage(self._batch(batch))
        self._prep(with_y=False)
        self._generate(self.inf_g)
        T = self.geometry[1]
        return ((self.inf_g + 1.0) * 0.5).reshape(self.B, T, T, 1)

    def _stats(self, name, y, g, images=False):
        """tdg_cgan_sample_stats at unit 1 on the [-1, 1] tensors: [0], [1] the per-image mean |y - g| (mean, min), [2], [3] the
        moments of g."""
        T = self.geometry[1]
        _lib.call('tdg_cgan_sample_stats', K.ptr(y), K.ptr(g), K.ptr(g), None, None, 1.0, self.B, T * T, 1.0,
                  K.ptr(self.stat_out[name]), K.ptr(self.samp_mean) if images else None, K.ptr(self.samp_var) if images else None,
                  K.ptr(self.stat_ws), self.stat_ws.numel(), K.stream())

    def _metrics_body(self):
        B, dt = self.B, self.sess.dtype
        S, _, _, P = self.geometry
        # sampler: row 0 of X and of y, broadcast
        self._prep(x_rows=self.zero_rows, y_rows=self.zero_rows, target=self.set_y['sampler'])
        self._generate(self.set_g)
        self._stats('sampler', self.set_y['sampler'], self.set_g)
        # shuffled: X permuted, y as it is
        self._prep(x_rows=self.perm, target=self.set_y['shuffled'])
        self._generate(self.set_g)
        self._stats('shuffled', self.set_y['shuffled'], self.set_g)
        # noise: X <- U(-1, 1), against the sampler set's y
        xn, u = self.G.xn, self.x_noise_u
        self.sess.random_uniform(u, u.numel(), 'x_noise')
        _lib.call('tdg_affine_cast_rows', dt, K.ptr(u), B * S * S, P, xn.cs, 2.0, -0.5, xn.ptr(0), K.stream())
        self._generate(self.set_g)
        self._stats('noise', self.set_y['sampler'], self.set_g)

    def metrics(self):
        """SET_KEYS of the three summary sets on the last staged batch, then the losses of the last fetch."""
        inj = self.sess._injected('shuffle')
        perm = torch.randperm(self.B) if inj is None else torch.as_tensor(np.asarray(inj)).reshape(self.B)
        self.perm.copy_(perm.to(torch.int32))
        self._run('is_metrics', self._metrics_body)
        s = {k: self.stat_out[k].cpu().tolist() for k in SETS}
        out = {}
        for k in SETS:
            out['moments/%s/moments/mean' % k], out['moments/%s/moments/var' % k] = s[k][2], s[k][3]
        for k in SETS:                               # per_image_statistics multiplies by 10 (:1018)
            out['per_image_metrics/%s/rmse/mean' % k], out['per_image_metrics/%s/rmse/min' % k] = 10.0 * s[k][0], 10.0 * s[k][1]
        out.update(self._losses())
        return out

    def _sample_body(self):
        self._prep(src=self.samp, x_rows=self.zero_rows, y_rows=self.zero_rows, target=self.set_y['sampler'])
        self._generate(self.set_g)
        self._stats('sampler', self.set_y['sampler'], self.set_g, images=True)

    def sample(self, x, y=None, x_loc=None, y_loc=None, mean_vec=None):
        """B predictions for ONE window under B noise draws.  x f32 [S,S,3]; y (optional), x_loc, y_loc, mean_vec [S,S] or [S,S,1]
        -- the planes the arch reads are required --, all as the dataset yields them.  Returns a dict: `y_hat` f32 [B,T,T] (device,
        depth in [0, 1]), `mean` and `var` f32 [T,T]: the per-pixel mean and population variance of the predictions in [0, 1]
        units, and `metrics`: with y the set's four statistics (SET_KEYS of `sampler`), else None."""
        dev, S = self.sess.device, self.geometry[0]
        given = [x, y if y is not None else torch.zeros(S, S), x_loc, y_loc, mean_vec][:self.n_read]
        for buf, t, what in zip(self.samp, given, ('x', 'y', 'x_loc', 'y_loc', 'mean_vec')):
            ok = ((S, S, 3),) if what == 'x' else ((S, S), (S, S, 1))
            if t is None:
                raise ValueError('sample: --g_arch %s reads %s' % (self.g_arch, what))
            t = torch.as_tensor(t).to(device=dev, dtype=torch.float32)
            if tuple(t.shape) not in ok:
                raise ValueError('sample: %s must be %s, got %s' % (what, ' or '.join(str(list(s)) for s in ok), tuple(t.shape)))
            buf[0].copy_(t.reshape(buf.shape[1:]))
        self._run('is_sample', self._sample_body)
        out = {'y_hat': (self.set_g + 1.0) * 0.5, 'mean': (self.samp_mean + 1.0) * 0.5, 'var': self.samp_var * 0.25, 'metrics': None}
        if y is not None:
            s = self.stat_out['sampler'].cpu().tolist()
            out['metrics'] = {'moments/sampler/moments/mean': s[2], 'moments/sampler/moments/var': s[3],
                              'per_image_metrics/sampler/rmse/mean': 10.0 * s[0], 'per_image_metrics/sampler/rmse/min': 10.0 * s[1]}
        return out
