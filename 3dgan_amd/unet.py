"""The skip U-Net executor: an encoder `Net` of n conv2d layers and a decoder `Net` of deconv2d layers whose inputs are
`concat([y, e_k])` of the previous decoder output and the mirrored encoder output (hem/models/pix2pix.py:160-228,
hem/models/paper_cgan.py:212-310), bound to HBM and run as HIP kernels.  Depth, spatial sizes, filter size, stride, padding,
batch norm, activation, init and dropout are read off the recorded `LayerSpec`s.

Every skip concat is ZERO-COPY: the decoder layer and the encoder layer each write their channel window of one buffer, and
in the backward pass the encoder's two gradient paths (skip first, then the next encoder layer) are summed by the
`accumulate` epilogue of the backward-data GEMM.

The top of the decoder is one of two things.  With `g_out` / `g_grad` the decoder is as deep as the encoder and its last
layer writes into / reads its gradient from the caller's windows (pix2pix).  Without them the decoder is one layer
shallower: the last concat and its gradient are handed to the caller as `top` / `gtop`, and whatever `dnet` records behind
the executed layers is the caller's head (paper_cgan); the caller's head writes `gtop` with the activation derivative of
the last decoder layer already applied.

Noise (pix2pix `--noise input|latent|end`, hem/models/pix2pix.py:183-186,204-206,223-225; paper_sampler `--noise_layer`,
hem/models/paper_sampler.py:169-230) switches on from the recorded layer widths: a layer whose `in_size` is one more -- at the
1x1 latent also: twice -- what its producers provide reads one more channel window, filled per pass with
tf.random_uniform(minval, maxval) of the recorded draw (`spec.noise`) from the device Philox stream.  The nodes are 'x' (the
generator input), 'e1' .. 'e<n>' (behind that encoder output; 'e<n>' is the latent) and 'd2' .. 'd<n>' (behind that decoder
layer's skip concat); the injection key of a node is 'noise_<node>' unless `noise_keys` names another.  Every concat stays
zero-copy -- the layouts are in UNet's docstring.  A head of the caller's that reads a noise channel ('d<n>' without `g_out`)
gets its f32 draw in `head_u`; the concat is not widened for it.
The extra last channel of a layer is either DRAWN, as above, or FED: a recorded placeholder concatenated last (`spec.fed`;
paper_standalone `--model_version mean_provided`, hem/models/paper_standalone.py:176-207: y_bar behind e1 and in front of the
head).  A fed channel has the layout of a drawn one, takes part in no Philox draw and has no injection key; its windows are in
`fed[source]` and the caller fills them (and `head_u`, the f32 plane of a fed head channel) before forward().  The padding
channels behind it stay zero.
Dropout (`spec.dropout` = keep probability, hem/ops/layers.py:207) runs on the decoder layers that record it.
"""
import torch

from . import _lib
from . import kernels as K
from . import engine

_MASK = {K.ACT_LRELU: K.MASK_LRELU, K.ACT_RELU: K.MASK_RELU}


class UNet:
    """cat[i] (i = 2..n) is decoder layer i's input [d_{i-1} | e_{n+1-i}]; gcat[i] its gradient.  Encoder layer k (k < n)
    writes its activation into the right window of cat[n+1-k] and receives its gradient -- skip path first, main path
    accumulated on top -- in the right window of gcat[n+1-k].

    Noise windows.  cat[i] is allocated as [d | e | noise] when either of its readers takes a noise channel: decoder layer i
    ('d<i>') reads all cd + ce + 1 channels and the next encoder layer its own window (cd, ce); with 'e<k>' the next encoder
    layer reads the window (cd, ce + 1) and decoder layer i the window (0, cd + ce).  cd is a multiple of 8, so every window
    starts on a 16-byte boundary.  The backward-data GEMM of the noise's reader also writes a gradient for the noise
    channel; nothing reads it.  The latent is [e_n | noise] of 1 or e_n's width channels, the input [x | noise].

    Gradient bookkeeping as in engine.SeqNet: a layer with batch norm keeps its normalised pre-activation and a delta buffer
    of its own; a layer without has delta == the gradient of its output, because the GEMM that produces that gradient
    applies the (l)relu derivative in its epilogue."""

    def __init__(self, enet, dnet, B, dtype, device, store, ws, x_in, g_out=None, g_grad=None, sess=None, noise_keys=None):
        self.B, self.dtype, self.device, self.store, self.ws = B, dtype, device, store, ws
        self.sess = sess
        self.enet, self.dnet = enet, dnet
        E, Dc = enet.layers, dnet.layers
        n = self.n = len(E)
        nd = self.nd = n if g_out is not None else n - 1            # decoder layers run here
        if len(Dc) < n:
            raise ValueError('a %d-layer encoder needs %d recorded decoder layers, got %d' % (n, n, len(Dc)))
        for spec in E + Dc[:nd]:
            if not spec.use_bn and (spec.act is None or spec.act.code not in _MASK):
                raise NotImplementedError('layer %s: without batch norm only relu / lrelu (the derivative mask of the GEMM epilogue)' % spec.name)
        A = lambda h, w, c: K.Act(B, h, w, c, dtype, device)
        H, W = E[0].in_shape[:2]
        # noise channels each layer reads behind what its producers provide
        self.noise_ch = {}                         # node -> channels (drawn or fed: the layouts are the same)
        self.fed_src = {}                          # node -> placeholder source, for the nodes whose extra channel is fed, not drawn

        def extra(node, spec, provided, allowed=(0, 1)):
            ch = spec.in_size - provided
            if ch not in allowed:
                raise ValueError('layer %s expects %d input channels, its producers provide %d' % (spec.name, spec.in_size, provided))
            drawn = spec.noise is not None and spec.noise[0] == ch
            fed = not drawn and getattr(spec, 'fed', None) is not None and spec.fed[0] == ch
            if ch and not drawn and not fed:
                raise ValueError('layer %s reads %d channels more than its producers provide, and they are neither a recorded '
                                 'random_uniform draw nor a placeholder' % (spec.name, ch))
            if ch:
                self.noise_ch[node] = ch
            if ch and fed:
                self.fed_src[node] = spec.fed[1]
            return ch
        extra('x', E[0], x_in.c)
        for k in range(1, n):
            extra('e%d' % k, E[k], E[k - 1].out_size)
        extra('e%d' % n, Dc[0], E[n - 1].out_size, (0, 1, E[n - 1].out_size))
        for i in range(2, n + 1):
            extra('d%d' % i, Dc[i - 1], Dc[i - 2].out_size + E[n - i].out_size)
        self.xn = A(H, W, x_in.c + 1) if 'x' in self.noise_ch else None
        if self.xn is not None:
            x_in = self.xn
        self.x_in = x_in
        # cat[i]: the buffer; cat_in[i]: what decoder layer i reads of it; wide[i]: [e | noise], what encoder layer n + 2 - i reads
        self.cat, self.gcat, self.cat_in, self.gcat_in, self.wide, self.gwide = {}, {}, {}, {}, {}, {}
        noise_at = {}
        for i in range(2, n + 1):
            cd, ce = Dc[i - 2].out_size, E[n - i].out_size
            dn = 'd%d' % i in self.noise_ch and i <= nd          # (a caller's head reads its own draw)
            en = 'e%d' % (n + 1 - i) in self.noise_ch
            if dn and en:
                raise NotImplementedError('noise both behind encoder layer %d and behind its skip concat' % (n + 1 - i))
            h, w = E[n - i].out_shape[:2]
            c = cd + ce + (1 if dn or en else 0)
            self.cat[i], self.gcat[i] = A(h, w, c), A(h, w, c)
            self.cat_in[i], self.gcat_in[i] = (self.cat[i].window(0, cd + ce), self.gcat[i].window(0, cd + ce)) if en else \
                (self.cat[i], self.gcat[i])
            if en:
                self.wide[i], self.gwide[i] = self.cat[i].window(cd, ce + 1), self.gcat[i].window(cd, ce + 1)
            if dn or en:
                noise_at['d%d' % i if dn else 'e%d' % (n + 1 - i)] = self.cat[i].window(cd + ce, 1)
        self.top, self.gtop = (self.cat_in[n], self.gcat_in[n]) if g_out is None else (None, None)
        # encoder activations / gradients
        self.e_h, self.e_g, self.e_pre, self.e_delta, self.e_stats, self.e_bn_name = {}, {}, {}, {}, {}, {}
        for k in range(1, n + 1):
            spec = E[k - 1]
            h, w, co = spec.out_shape
            if k < n:
                cd = Dc[n - 1 - k].out_size
                self.e_h[k] = self.cat[n + 1 - k].window(cd, co)
                self.e_g[k] = self.gcat[n + 1 - k].window(cd, co)     # dL/d(e_k output); == delta when no batch norm
            elif 'e%d' % n in self.noise_ch:       # [e_n | noise]: e_n is the left window of decoder layer 1's input
                lc = co + self.noise_ch['e%d' % n]
                self.lat, self.glat = A(h, w, lc), A(h, w, lc)
                self.e_h[k], self.e_g[k] = self.lat.window(0, co), self.glat.window(0, co)
                noise_at['e%d' % n] = self.lat.window(co, lc - co)
            else:
                self.e_h[k], self.e_g[k] = A(h, w, co), A(h, w, co)
            if spec.use_bn:
                self.e_pre[k], self.e_delta[k] = A(h, w, co), A(h, w, co)
                self.e_stats[k] = torch.zeros(2 * co, dtype=torch.float32, device=device)
                self.e_bn_name[k] = enet.bn_name(0, k - 1)
            else:
                self.e_delta[k] = self.e_g[k]
        # decoder
        self.d_pre, self.d_delta, self.d_h, self.d_g, self.d_stats, self.d_bn_name = {}, {}, {}, {}, {}, {}
        for i in range(1, nd + 1):
            spec = Dc[i - 1]
            h, w, co = spec.out_shape
            if i < n:
                self.d_h[i], self.d_g[i] = self.cat[i + 1].window(0, co), self.gcat[i + 1].window(0, co)
            else:
                self.d_h[i], self.d_g[i] = g_out, g_grad
            if spec.use_bn:
                self.d_pre[i], self.d_delta[i] = A(h, w, co), A(h, w, co)
                self.d_stats[i] = torch.zeros(2 * co, dtype=torch.float32, device=device)
                self.d_bn_name[i] = dnet.bn_name(0, i - 1)
            else:
                self.d_delta[i] = self.d_g[i]
                if i < n and (E[n - i - 1].act is None or E[n - i - 1].act.code != K.ACT_RELU):
                    # the GEMM that writes gcat[i + 1] masks BOTH windows with act'(cat[i + 1]); on e's window that is only
                    # harmless when e's own relu mask zeroes whatever it scaled: where e > 0 the factor is 1, and where e == 0
                    # the relu derivative -- the epilogue mask on top of the accumulated main path, or the one inside the
                    # batch-norm backward pass -- zeroes the entry
                    raise NotImplementedError('decoder layer %s without batch norm beside an encoder layer that is not a relu' % spec.name)
        # convs (descriptors carry the strides of the buffers each GEMM form touches)
        self.e_conv, self.d_conv = {}, {}
        for k in range(1, n + 1):
            spec = E[k - 1]
            big = self._e_in(k)
            small = self.e_pre[k] if spec.use_bn else self.e_h[k]
            self.e_conv[k] = K.Conv(big, small, spec.k, spec.k, spec.stride, *engine.conv_pads(spec, big, small))
        for i in range(1, nd + 1):
            spec = Dc[i - 1]
            big, small = (self.d_pre[i] if spec.use_bn else self.d_h[i]), self._d_in(i)
            self.d_conv[i] = K.Conv(big, small, spec.k, spec.k, spec.stride, *engine.conv_pads(spec, big, small))
        # tf.nn.dropout(h, keep_prob=dropout) on decoder layers built with dropout > 0: the uniform draws of the pass, kept
        # for the backward
        self.d_keep = {i: float(getattr(Dc[i - 1], 'dropout', 0) or 0) for i in range(1, nd + 1)}
        self.d_u = {i: torch.zeros(B * self.d_h[i].h * self.d_h[i].w * Dc[i - 1].out_size, dtype=torch.float32, device=device)
                    for i in range(1, nd + 1) if self.d_keep[i] > 0}
        # noise channel windows in node order ('x', 'e1' .., 'd2' ..: the order of the draws), each with the f32 staging of its
        # uniform draw and the affine map of tdg_affine_cast_rows that turns U(0,1) into U(minval, maxval)
        if self.xn is not None:
            noise_at['x'] = self.xn.window(self.xn.c - 1, 1)
        reader = dict([('x', E[0])] + [('e%d' % k, E[k]) for k in range(1, n)] + [('e%d' % n, Dc[0])] +
                      [('d%d' % i, Dc[i - 1]) for i in range(2, n + 1)])
        self.noise, self.noise_map, self.head_u = {}, {}, None
        self.fed = {}                              # placeholder source -> its channel windows; the caller fills them per pass
        for node in reader:
            if node not in self.noise_ch:
                continue
            if node in self.fed_src:               # no draw, no key: the order and the keys of the drawn nodes are untouched
                if self.noise_ch[node] != 1:
                    raise NotImplementedError('a fed channel behind %s is one channel wide' % node)
                if node in noise_at:
                    self.fed.setdefault(self.fed_src[node], []).append(noise_at[node])
                else:                              # the caller's head reads the fed channel as an f32 plane [B, h, w] of its own
                    self.head_u = torch.zeros(B * self.top.h * self.top.w, dtype=torch.float32, device=device)
                continue
            key = (noise_keys or {}).get(node, 'noise_' + node)
            _, lo, hi = reader[node].noise
            if node in noise_at:
                self.noise[key], self.noise_map[key] = noise_at[node], (hi - lo, lo / (hi - lo))
            elif (lo, hi) != (0.0, 1.0):
                raise NotImplementedError("the head's noise channel is read as drawn: U(0,1), not U(%g,%g)" % (lo, hi))
            else:                                  # the caller's head: the f32 draw [B, h, w] itself
                self.noise[key] = None
        self.noise_u = {k: torch.zeros(B * (a.h * a.w * a.c if a is not None else self.top.h * self.top.w), dtype=torch.float32,
                                       device=device) for k, a in self.noise.items()}
        for k, a in self.noise.items():
            if a is None:
                self.head_u = self.noise_u[k]
        # variables: every recorded layer of both nets (a caller's head included), batch-norm betas beside their layer
        for net, bn_names in ((enet, self.e_bn_name), (dnet, self.d_bn_name)):
            for idx, spec in enumerate(net.layers):
                engine.declare_weights(store, net, [spec])
                if idx + 1 in bn_names:
                    store.declare(bn_names[idx + 1], (spec.out_size,))
        self._pack_jobs = None

    def init_variables(self, gen):
        for net in (self.enet, self.dnet):
            engine.init_weights(self.store, net, net.layers, gen)

    def _var(self, net, spec, which):
        return self.store[net.var_name(spec, which)]

    def _grad(self, net, spec, which):
        return self.store.grad(net.var_name(spec, which))

    def repack(self):
        if self._pack_jobs is None:
            jl = [self.e_conv[k].pack_job(self._var(self.enet, self.enet.layers[k - 1], 'weights')) for k in range(1, self.n + 1)]
            jl += [self.d_conv[i].pack_job(self._var(self.dnet, self.dnet.layers[i - 1], 'weights')) for i in range(1, self.nd + 1)]
            self._pack_jobs = K.make_pack_jobs(jl)
        K.pack_all(self._pack_jobs)

    def _d_in(self, i):
        """Input tensor of decoder layer i: [e_n (| noise)] for i = 1, the skip concat (| noise) otherwise."""
        if i > 1:
            return self.cat_in[i]
        return self.lat if 'e%d' % self.n in self.noise_ch else self.e_h[self.n]

    def _e_in(self, k):
        """Input tensor of encoder layer k: x (| noise) for k = 1, e_{k-1} (| noise) otherwise."""
        if k == 1:
            return self.x_in
        return self.wide.get(self.n + 2 - k, self.e_h[k - 1])

    def _e_gin(self, k):
        """Where encoder layer k's backward-data GEMM delivers its gradient: e_{k-1}'s window (| the unread noise gradient)."""
        return self.gwide.get(self.n + 2 - k, self.e_g[k - 1])

    def draw_noise(self):
        """tf.random_uniform(minval, maxval) into every noise window (one draw per generator pass, as in TF)."""
        for key, a in self.noise.items():
            u = self.noise_u[key]
            self.sess.random_uniform(u, u.numel(), key)
            if a is not None:
                scale, shift = self.noise_map[key]
                _lib.call('tdg_affine_cast_rows', self.dtype, K.ptr(u), self.B * a.h * a.w, a.c, a.cs, scale, shift, a.ptr(0),
                          K.stream())

    # ---- forward: the last executed decoder layer's output into g_out / the left window of `top` ------------------
    def forward(self, backward_follows=True):
        """backward_follows=False (the critic step's and the loss fetch's generator pass): batch-norm layers write only their
        activation, not the normalised pre-activation the backward pass would read."""
        B = self.B
        self._keep_pre = backward_follows
        self.draw_noise()
        for k in range(1, self.n + 1):
            spec = self.enet.layers[k - 1]
            src = self._e_in(k)
            self._layer_fwd(self.e_conv[k].fwd, src, spec, self._var(self.enet, spec, 'bias'), self.e_pre.get(k), self.e_h[k],
                            self.e_bn_name.get(k), self.e_stats.get(k))
        for i in range(1, self.nd + 1):
            spec = self.dnet.layers[i - 1]
            self._layer_fwd(self.d_conv[i].bwd_data, self._d_in(i), spec, self._var(self.dnet, spec, 'bias'), self.d_pre.get(i),
                            self.d_h[i], self.d_bn_name.get(i), self.d_stats.get(i))
            if self.d_keep[i] > 0:
                self.sess.random_uniform(self.d_u[i], self.d_u[i].numel(), 'dropout')
                self._dropout(self.d_h[i], i)

    def _layer_fwd(self, gemm, src, spec, bias, pre, h, bn_name, stats):
        """One layer: bias + activation in the GEMM epilogue, or -- batch norm -- the GEMM stores `pre` and emits the batch
        statistics' column partials when the launch can (else the separate statistics pass)."""
        if not spec.use_bn:
            gemm(src.ptr(), h.ptr(), self.B, K.epilogue(bias=bias, act=spec.act.code, leak=spec.act.leak))
            return
        epi = K.colsum_epilogue(self.ws, pre.rows, spec.out_size, K.COL_BN, bias=bias)
        gemm(src.ptr(), pre.ptr(), self.B, epi)
        beta = self.store[bn_name]
        if K.nblk(epi):
            K.bn_fwd_from_partials(epi, pre, spec.out_size, beta, spec.act.code, pre if self._keep_pre else None, h, stats, bias,
                                   leak=spec.act.leak)
        else:
            K.bn_fwd(self.ws, pre, spec.out_size, beta, spec.act.code, pre, h, stats, leak=spec.act.leak)

    def _dropout(self, act, i):
        rows = self.B * act.h * act.w
        _lib.call('tdg_dropout', self.dtype, act.ptr(), rows, self.dnet.layers[i - 1].out_size, act.cs, K.ptr(self.d_u[i]),
                  self.d_keep[i], K.stream())

    # ---- backward from the gradient in g_grad / the left window of `gtop` -----------------------------------------
    def backward(self):
        B = self.B
        for i in range(self.nd, 0, -1):
            spec, conv = self.dnet.layers[i - 1], self.d_conv[i]
            if self.d_keep[i] > 0:
                self._dropout(self.d_g[i], i)                                     # d(dropout)/dh = the same mask / keep
            delta = self._layer_delta(self.dnet, spec, self.d_g[i], self.d_pre.get(i), self.d_delta[i], self.d_bn_name.get(i),
                                      self.d_stats.get(i))
            conv.bwd_filter(delta.ptr(), self._d_in(i).ptr(), self._grad(self.dnet, spec, 'weights'), B, 0.0)
            if i > 1:                                                             # first writer of gcat[i] (both windows)
                conv.fwd(delta.ptr(), self.gcat_in[i].ptr(), B, self._into_decoder(i - 1))
            else:
                conv.fwd(delta.ptr(), self.e_g[self.n].ptr(), B, self._into_encoder(self.n, accumulate=False))
        for k in range(self.n, 0, -1):
            spec, conv = self.enet.layers[k - 1], self.e_conv[k]
            delta = self._layer_delta(self.enet, spec, self.e_g[k], self.e_pre.get(k), self.e_delta[k], self.e_bn_name.get(k),
                                      self.e_stats.get(k))
            conv.bwd_filter(self._e_in(k).ptr(), delta.ptr(), self._grad(self.enet, spec, 'weights'), B, 0.0)
            if k > 1:
                conv.bwd_data(delta.ptr(), self._e_gin(k).ptr(), B, self._into_encoder(k - 1, accumulate=True))

    def _layer_delta(self, net, spec, g, pre, delta, bn_name, stats):
        """dL/d(conv output incl. bias) of one layer and its bias gradient: batch norm's backward pass gives both; without
        batch norm `g` is delta already and the bias gradient is its column sums."""
        if spec.use_bn:
            K.bn_bwd(self.ws, g, pre, spec.out_size, self.store[bn_name], stats, spec.act.code, delta, self.store.grad(bn_name),
                     leak=spec.act.leak, dbias=self._grad(net, spec, 'bias'))
        else:
            K.bias_grad(self.ws, delta, spec.out_size, self._grad(net, spec, 'bias'))
        return delta

    def _into_decoder(self, i):
        """Epilogue of the GEMM that writes gcat[i + 1] = [dL/d(d_i output) | skip gradient of e_{n-i}]: without batch norm
        on decoder layer i it applies act'(cat[i + 1]) so that the left window is delta_i (see __init__ for the right one)."""
        spec = self.dnet.layers[i - 1]
        if spec.use_bn:
            return None
        return K.epilogue(mask_mode=_MASK[spec.act.code], leak=spec.act.leak, mask_src=self.cat[i + 1].ptr())

    def _into_encoder(self, k, accumulate):
        """Epilogue of the GEMM that delivers a gradient to encoder layer k's output: add to the skip gradient
        already there, and -- without batch norm -- apply act'(e_k) so the result is delta_k directly."""
        spec = self.enet.layers[k - 1]
        if spec.use_bn:
            return K.epilogue(accumulate=accumulate)
        return K.epilogue(mask_mode=_MASK[spec.act.code], leak=spec.act.leak, mask_src=self.e_h[k].ptr(), accumulate=accumulate)
