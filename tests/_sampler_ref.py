"""Float64 statements of paper_sampler (hem/models/paper_sampler.py) for the tests: the noisy generator and one batch's
losses on torch autograd (oracle/torch_ref.py's primitives; test infrastructure only), and the six per-set statistics of
metric_summaries (:337-342) in NumPy."""
import numpy as np
import torch

from oracle.torch_ref import conv2d_valid, conv2d_transpose_valid, conv2d_same, lrelu, batch_norm

NODES = ['x', 'e1', 'e2', 'e3', 'e4', 'e4-512', 'd2', 'd3', 'd4']
# [h, w, c] of the draw at each node (:170-229, NHWC) and the input width of the layer that reads it
NOISE_SHAPE = {'x': (65, 65, 1), 'e1': (31, 31, 1), 'e2': (14, 14, 1), 'e3': (5, 5, 1), 'e4': (1, 1, 1), 'e4-512': (1, 1, 512),
               'd2': (5, 5, 1), 'd3': (14, 14, 1), 'd4': (31, 31, 1)}
READER = {'x': ('encoder', 'e1', 4), 'e1': ('encoder', 'e2', 65), 'e2': ('encoder', 'e3', 129), 'e3': ('encoder', 'e4', 257),
          'e4': ('decoder', 'd1', 513), 'e4-512': ('decoder', 'd1', 1024), 'd2': ('decoder', 'd2', 513), 'd3': ('decoder', 'd3', 257),
          'd4': ('decoder', 'd4', 129)}
STAT_KEYS = ('per_image_rmse/mean', 'per_image_rmse/min', 'g_moments/mean', 'g_moments/var', 'y_hat_moments/mean',
             'y_hat_moments/var')


def bn_beta(k):
    """The encoder's k-th (1-based) batch-norm beta: contrib batch_norm's scopes BatchNorm, BatchNorm_1, ..."""
    return 'generator/encoder/BatchNorm%s/beta' % ('' if k == 1 else '_%d' % (k - 1))


def oracle_G(P, x, node, bn, noise, pres=None):
    """g_baseline (:159-235), NHWC: `noise` [B,h,w,c] is concatenated behind `node`; `bn`: batch norm in the encoder.
    pres: a list that receives every (l)relu's input."""
    def W(n):
        return P['generator/' + n]

    def cat(t, at):
        return torch.cat([t, noise], dim=-1) if node == at else t
    h = cat(x, 'x')
    e = []
    for k in range(1, 5):
        h = conv2d_valid(h, W('encoder/vars/e%d/weights' % k), 2) + W('encoder/vars/e%d/bias' % k)
        if bn:
            h = batch_norm(h, P[bn_beta(k)])
        if pres is not None:
            pres.append(h)
        h = torch.relu(h)
        e.append(h)
        if k < 4:
            h = cat(h, 'e%d' % k)
    y = cat(cat(e[3], 'e4'), 'e4-512')
    for i, hw in ((1, 5), (2, 14), (3, 31)):
        y = conv2d_transpose_valid(y, W('decoder/vars/d%d/weights' % i), (hw, hw)) + W('decoder/vars/d%d/bias' % i)
        if pres is not None:
            pres.append(y)
        y = lrelu(y, 0.2)
        y = cat(torch.cat([y, e[3 - i]], dim=-1), 'd%d' % (i + 1))
    y = conv2d_same(y, W('decoder/vars/d4/weights'), 1) + W('decoder/vars/d4/bias')
    return y[:, :29, :29, :]


def nearest_kink(variables, batch, node, bn, noise, max_positions=100):
    """The smallest |input| of the (l)relus of the generator's SMALL layers (at most `max_positions` outputs per channel in
    the whole batch: e3, e4 and d1 at B = 4) on this batch, in float64.  The derivative jumps at zero: an evaluation whose
    rounding puts such an input on the other side differs from the oracle by that position's whole contribution -- a tenth
    of a bias gradient entry where a channel has a hundred positions -- whatever its precision.  In the wide layers one
    position in thousands moves nothing by 1e-3."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in variables.items() if k.startswith('generator/')}
    x = torch.tensor(np.asarray(batch[0].cpu() if hasattr(batch[0], 'cpu') else batch[0]), dtype=torch.float64)
    pres = []
    with torch.no_grad():
        oracle_G(P, x, node, bn, torch.tensor(np.asarray(noise), dtype=torch.float64), pres)
    return min(float(p.abs().min()) for p in pres if p.shape[0] * p.shape[1] * p.shape[2] <= max_positions)


def encoder_kink_margin(variables, batch, node, noise):
    """With batch norm in the encoder, how far ALL its relu inputs stay from zero on this batch, in units of what float32
    does to them (as critic_kink_margin: min |input| / rms(float32 - float64 input) per layer, the minimum over e1 .. e4).
    Normalised inputs are of order 1 and carry float32 errors of some 1e-7, and the batch-norm backward pass spreads one
    flipped derivative over every position of its channel, so here the wide layers count too."""
    pres = {}
    for dtype in (torch.float64, torch.float32):
        P = {k: torch.tensor(np.asarray(v)).to(dtype) for k, v in variables.items() if k.startswith('generator/')}
        x = torch.tensor(np.asarray(batch[0].cpu() if hasattr(batch[0], 'cpu') else batch[0])).to(dtype)
        pres[dtype] = []
        with torch.no_grad():
            oracle_G(P, x, node, True, torch.tensor(np.asarray(noise)).to(dtype), pres[dtype])
    return min(float(a.abs().min()) / float((a - b.double()).pow(2).mean().sqrt())
               for a, b in list(zip(pres[torch.float64], pres[torch.float32]))[:4])


def critic_inputs(P, x, y, dtype):
    """The inputs of the critic's lrelus (d_baseline, :237-258) by layer name."""
    def W(n):
        return torch.as_tensor(np.asarray(P['discriminator/' + n])).to(dtype)
    out, h1, h2 = {}, x, y
    for k in range(1, 5):
        out['hx%d' % k] = conv2d_valid(h1, W('rgb_path/vars/hx%d/weights' % k), 2) + W('rgb_path/vars/hx%d/bias' % k)
        h1 = lrelu(out['hx%d' % k], 0.2)
    for k in range(1, 4):
        out['hy%d' % k] = conv2d_valid(h2, W('depth_path/vars/hy%d/weights' % k), 2) + W('depth_path/vars/hy%d/bias' % k)
        h2 = lrelu(out['hy%d' % k], 0.2)
    h = torch.cat([h1, h2], dim=-1)
    for k in (1, 2):
        out['h%d' % k] = conv2d_same(h, W('combined_path/vars/h%d/weights' % k), 1) + W('combined_path/vars/h%d/bias' % k)
        h = lrelu(out['h%d' % k], 0.2)
    return out


def critic_kink_margin(variables, batch, node, bn, noise, real, max_positions):
    """How far the critic's SMALL layers (at most `max_positions` outputs per channel in the batch: hx3, hx4, hy2, hy3, h1, h2)
    keep their lrelu inputs from zero on this batch, in units of what float32 does to them: the minimum over those layers of
    min |input| / rms(float32 input - float64 input), both evaluations the oracle's own.  D(x, g) always, D(x, y - y_bar) with
    `real`.  A ratio of 5 means an evaluation needs five times the typical float32 error at that very element to take the
    other side of the kink; one such flip in hy2 moves hy1/weights by 1.3e-3 of its largest entry."""
    pres = {}
    for dtype in (torch.float64, torch.float32):
        P = {k: torch.tensor(np.asarray(v)).to(dtype) for k, v in variables.items()}
        x, y = (torch.tensor(np.asarray(t.cpu() if hasattr(t, 'cpu') else t)).to(dtype) for t in batch)
        with torch.no_grad():
            g = oracle_G(P, x, node, bn, torch.tensor(np.asarray(noise)).to(dtype))
            yc = 10.0 * y[:, 17:46, 17:46, :]
            passes = [('fake', g)] + ([('real', yc - yc.mean(dim=(1, 2, 3), keepdim=True))] if real else [])
            for tag, depth in passes:
                for name, p in critic_inputs(P, x, depth, dtype).items():
                    if p.shape[0] * p.shape[1] * p.shape[2] <= max_positions:
                        pres[(dtype, tag, name)] = p.double()
    return min(float(p.abs().min()) / float((p - pres[(torch.float32,) + k[1:]]).pow(2).mean().sqrt())
               for k, p in pres.items() if k[0] == torch.float64)


def oracle_forward(P, x01, y01, node, bn, noise, oracle_D):
    """:73-121 and :262-275 for one batch; returns (losses in the order of :274, g_fake, d_total, y_hat, g)."""
    y = 10.0 * y01[:, 17:46, 17:46, :]
    ybar = y.mean(dim=(1, 2, 3), keepdim=True)
    g = oracle_G(P, x01, node, bn, noise)
    y_hat = g + ybar
    zf, zr = oracle_D(P, x01, y_hat - ybar), oracle_D(P, x01, y - ybar)
    sp = torch.nn.functional.softplus
    g_fake, d_real, d_fake = sp(-zf).mean(), sp(-zr).mean(), sp(zf).mean()
    d_total = d_real + d_fake
    return {'g_fake': g_fake, 'd_real': d_real, 'd_fake': d_fake, 'd_total': d_total}, g_fake, d_total, y_hat, g


def oracle_grads(variables, batch, node, bn, noise, which, oracle_D, dtype=torch.float64):
    """(losses, gradients of the D ('d') or G ('g') loss by variable name, y_hat) of one batch, in `dtype`."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in variables.items()}
    x, y = (torch.tensor(np.asarray(t.cpu() if hasattr(t, 'cpu') else t), dtype=dtype) for t in batch)
    losses, g_fake, d_total, y_hat, _ = oracle_forward(P, x, y, node, bn, torch.tensor(np.asarray(noise), dtype=dtype), oracle_D)
    names = [k for k in P if k.startswith('discriminator/' if which == 'd' else 'generator/')]
    grads = torch.autograd.grad(d_total if which == 'd' else g_fake, [P[k] for k in names])
    return ({k: float(v.detach()) for k, v in losses.items()}, {k: g.double().numpy() for k, g in zip(names, grads)},
            y_hat.detach().double().numpy())


def sample_stats(y10, g10, p10):
    """STAT_KEYS of one set in float64: y10, g10, p10 [n, hw] -- the depth crop, g and y_hat in 10x units -- to the
    reference's [0, 1] units (values / 10, variances / 100)."""
    y, g, p = (np.asarray(a, np.float64) / 10.0 for a in (y10, g10, p10))
    per_image = np.mean(np.abs(y - p), axis=1)
    return np.array([per_image.mean(), per_image.min(), g.mean(axis=0).mean(), g.var(axis=0).mean(), p.mean(axis=0).mean(),
                     p.var(axis=0).mean()])


def sample_stats_literal(y10, g10, p10):
    """hem/models/paper_sampler.py:308-310,337-342 and hem/ops/summaries.py:87-90 transcribed line by line on [n,1,29,29]."""
    g = g10 / 10.0
    y = y10 / 10.0
    y_hat = p10 / 10.0
    per_image_rmse = np.mean(np.sqrt(np.square(y - y_hat)), axis=(1, 2, 3))
    out = [np.mean(per_image_rmse), np.min(per_image_rmse)]
    for x in (g, y_hat):                                    # mean, var = tf.nn.moments(x, axes=[0])
        mean = np.mean(x, axis=0, keepdims=True)
        var = np.mean(np.square(x - mean), axis=0)
        out += [np.mean(mean), np.mean(var)]
    return np.array(out)
