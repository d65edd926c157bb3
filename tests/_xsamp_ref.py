"""Float64 statements of experimental_sampler (hem/models/experimental_sampler.py) for the tests, on torch autograd
(oracle/torch_ref.py's primitives; the estimator's m from tests/_mde_ref.forward): the input assembly (:107-149), generator and
critic E2 (:213-281), the six losses (:284-324), both gradient sets from ONE forward pass (:198-209), the four statistics of a
summary set in NumPy (:377-397), a 6-tuple batch source at 64x64 / 53x70 and the kink-margin helpers of this network.  Test
infrastructure only."""
import numpy as np
import torch

from oracle.torch_ref import conv2d_same, conv2d_transpose_same, conv2d_valid, conv2d_transpose_valid, lrelu
import _mde_ref as M

SRC, CROP, OFFSET, FULL = 64, 32, 16, (53, 70)
LOSS_KEYS = ('g_fake', 'd_real', 'd_fake', 'd_total', 'rmse', 'l1')
SETS = ('sampler', 'shuffled', 'noise')
G_NAMES = ['generator/encoder/vars/e%d/%s' % (k, w) for k in range(1, 6) for w in ('weights', 'bias')] + \
          ['generator/decoder/vars/d%d/%s' % (k, w) for k in range(1, 6) for w in ('weights', 'bias')]
D_NAMES = ['discriminator/rgb_path/vars/hx%d/%s' % (k, w) for k in range(1, 6) for w in ('weights', 'bias')] + \
          ['discriminator/depth_path/vars/hy%d/%s' % (k, w) for k in range(1, 5) for w in ('weights', 'bias')] + \
          ['discriminator/combined_path/vars/h%d/%s' % (k, w) for k in range(1, 7) for w in ('weights', 'bias')]
# channels in -> out per layer; a narrow copy for the differentiation check keeps the structure
WIDE = dict(e=(7, 64, 128, 256, 512, 1024), hx=(6, 64, 128, 256, 512, 1024), hy=(1, 128, 256, 512, 1024),
            h=(2048, 1024, 512, 256, 128, 64, 1))
NARROW = dict(e=(7, 4, 4, 6, 6, 8), hx=(6, 4, 4, 6, 6, 8), hy=(1, 4, 6, 6, 8), h=(16, 8, 6, 6, 4, 4, 1))


def shapes(widths=WIDE):
    """Variable name -> shape for the given widths (WIDE: the reference's)."""
    e, hx, hy, h = widths['e'], widths['hx'], widths['hy'], widths['h']
    out = {}
    for k in range(1, 6):
        f = 4 if k == 5 else 5
        out['generator/encoder/vars/e%d/weights' % k], out['generator/encoder/vars/e%d/bias' % k] = (f, f, e[k - 1], e[k]), (e[k],)
        out['discriminator/rgb_path/vars/hx%d/weights' % k], out['discriminator/rgb_path/vars/hx%d/bias' % k] = \
            (f, f, hx[k - 1], hx[k]), (hx[k],)
    # decoder: d_i [k, k, Cout, Cin]; Cin = the previous decoder width + the mirrored encoder width
    dout = (e[4], e[3], e[2], e[1])
    cin = e[5]
    for i in range(1, 5):
        f = 4 if i == 1 else 5
        out['generator/decoder/vars/d%d/weights' % i], out['generator/decoder/vars/d%d/bias' % i] = (f, f, dout[i - 1], cin), (dout[i - 1],)
        cin = dout[i - 1] + e[5 - i]
    out['generator/decoder/vars/d5/weights'], out['generator/decoder/vars/d5/bias'] = (1, 1, cin, 1), (1,)
    for k in range(1, 5):
        f = 4 if k == 4 else 5
        out['discriminator/depth_path/vars/hy%d/weights' % k], out['discriminator/depth_path/vars/hy%d/bias' % k] = \
            (f, f, hy[k - 1], hy[k]), (hy[k],)
    for k in range(1, 7):
        out['discriminator/combined_path/vars/h%d/weights' % k], out['discriminator/combined_path/vars/h%d/bias' % k] = \
            (1, 1, h[k - 1], h[k]), (h[k],)
    return out


def random_variables(widths, seed=0, scale=1.0):
    """Xavier-like float64 variables of the given widths (the differentiation check's narrow copy)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, s in shapes(widths).items():
        fan = np.prod(s[:-1]) + s[-1] if len(s) > 1 else 2 * s[0]
        out[k] = rng.uniform(-1, 1, s) * scale * np.sqrt(6.0 / fan)
    return out


# ------------------------------------------------------------------------------------------------ the model
def assemble(batch, m, dtype=torch.float64, x_rows=None, y_rows=None):
    """(X [B,64,64,6], y [B,32,32,1]) of :107-139: fl32(2x - 1) and fl32(2y - 1) as hem.rescale rounds them, y cropped at
    (16, 16), X = [x | x_loc | y_loc | m].  x_rows / y_rows: tdg_xsamp_prep's row maps."""
    x, y, xl, yl = (torch.as_tensor(np.asarray(t.cpu() if hasattr(t, 'cpu') else t), dtype=torch.float32) for t in batch[:4])
    m = torch.as_tensor(np.asarray(m), dtype=torch.float32)
    B = x.shape[0]
    xr = torch.arange(B) if x_rows is None else torch.as_tensor(np.asarray(x_rows), dtype=torch.long)
    yr = torch.arange(B) if y_rows is None else torch.as_tensor(np.asarray(y_rows), dtype=torch.long)
    X = torch.cat([2.0 * x[xr] - 1.0, xl[xr], yl[xr], m[xr].reshape(B, 1, 1, 1).expand(B, SRC, SRC, 1)], dim=-1)
    yc = (2.0 * y[yr] - 1.0)[:, OFFSET:OFFSET + CROP, OFFSET:OFFSET + CROP, :]
    return X.to(dtype), yc.to(dtype)


def noise_channel(u01):
    """The executor's map of a U(0,1) draw to U(-1,1), in f32 as tdg_affine_cast_rows computes it: 2 * (u + -0.5)."""
    u = np.asarray(u01, np.float32)
    return np.float32(2.0) * (u + np.float32(-0.5))


def oracle_G(P, X, noise, pres=None):
    """generatorE2 (:213-248), NHWC: `noise` [B,64,64,1] is concatenated behind X.  pres receives every (l)relu's input."""
    def W(n):
        return P['generator/' + n]
    h = torch.cat([X, noise], dim=-1)
    e = []
    for k in range(1, 6):
        w, b = W('encoder/vars/e%d/weights' % k), W('encoder/vars/e%d/bias' % k)
        h = (conv2d_same(h, w, 2) if k < 5 else conv2d_valid(h, w, 2)) + b
        if pres is not None:
            pres.append(('e%d' % k, h))
        h = torch.relu(h)
        e.append(h)
    y = e[4]
    for i in range(1, 5):
        w, b = W('decoder/vars/d%d/weights' % i), W('decoder/vars/d%d/bias' % i)
        y = (conv2d_transpose_valid(y, w, (4, 4)) if i == 1 else conv2d_transpose_same(y, w)) + b
        if pres is not None:
            pres.append(('d%d' % i, y))
        y = torch.cat([lrelu(y, 0.2), e[4 - i]], dim=-1)
    return torch.tanh(conv2d_same(y, W('decoder/vars/d5/weights'), 1) + W('decoder/vars/d5/bias'))       # [B,32,32,1]


def critic_inputs(P, X, depth):
    """The inputs of the critic's lrelus (discriminatorE2, :252-281) by layer name, and the logits as 'h6'."""
    def W(n):
        return P['discriminator/' + n]
    out, h1, h2 = {}, X, depth
    for k in range(1, 6):
        w, b = W('rgb_path/vars/hx%d/weights' % k), W('rgb_path/vars/hx%d/bias' % k)
        out['hx%d' % k] = (conv2d_same(h1, w, 2) if k < 5 else conv2d_valid(h1, w, 2)) + b
        h1 = lrelu(out['hx%d' % k], 0.2)
    for k in range(1, 5):
        w, b = W('depth_path/vars/hy%d/weights' % k), W('depth_path/vars/hy%d/bias' % k)
        out['hy%d' % k] = (conv2d_same(h2, w, 2) if k < 4 else conv2d_valid(h2, w, 2)) + b
        h2 = lrelu(out['hy%d' % k], 0.2)
    h = torch.cat([h1, h2], dim=-1)
    for k in range(1, 7):
        out['h%d' % k] = conv2d_same(h, W('combined_path/vars/h%d/weights' % k), 1) + W('combined_path/vars/h%d/bias' % k)
        h = lrelu(out['h%d' % k], 0.2)
    return out


def oracle_D(P, X, depth):
    return critic_inputs(P, X, depth)['h6']


def oracle_forward(P, X, y, noise):
    """:155-167 and :284-324 for one batch: (losses in the order of :316, g)."""
    g = oracle_G(P, X, noise)
    zr, zf = oracle_D(P, X, y), oracle_D(P, X, g)
    sp = torch.nn.functional.softplus
    g_fake, d_real, d_fake = sp(-zf).mean(), sp(-zr).mean(), sp(zf).mean()
    g01, y01 = (g + 1.0) / 2.0, (y + 1.0) / 2.0
    return {'g_fake': g_fake, 'd_real': d_real, 'd_fake': d_fake, 'd_total': d_real + d_fake,
            'rmse': torch.sqrt(torch.mean(torch.square(g01 - y01))), 'l1': torch.mean(torch.abs(y01 - g01))}, g


def estimator_m(est_variables, batch):
    """m [B] of the batch's x_full under the estimator's variables, float64 (tests/_mde_ref.forward)."""
    with torch.no_grad():
        return M.forward(M.tensors(est_variables), torch.tensor(M._np(batch[4]), dtype=torch.float64)).numpy()


def oracle_grads(variables, X, y, noise, dtype=torch.float64):
    """(losses, D gradients of d_total, G gradients of g_fake, g) from ONE forward pass at `variables` (:169-172, :208)."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in variables.items()
         if k.startswith(('generator/', 'discriminator/'))}
    X, y, noise = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (X, y, noise))
    losses, g = oracle_forward(P, X, y, noise)
    dn, gn = [k for k in P if k.startswith('discriminator/')], [k for k in P if k.startswith('generator/')]
    dg = torch.autograd.grad(losses['d_total'], [P[k] for k in dn], retain_graph=True)
    gg = torch.autograd.grad(losses['g_fake'], [P[k] for k in gn])
    return ({k: float(v.detach()) for k, v in losses.items()}, {k: t.double().numpy() for k, t in zip(dn, dg)},
            {k: t.double().numpy() for k, t in zip(gn, gg)}, g.detach().double().numpy())


# ------------------------------------------------------------------------------------------------ kinks
def nearest_kink(variables, X, noise, max_positions):
    """The smallest |input| of the (l)relus of the generator's SMALL layers (at most `max_positions` outputs per channel in the
    whole batch) in float64 -- tests/_sampler_ref.nearest_kink for this network."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in variables.items() if k.startswith('generator/')}
    pres = []
    with torch.no_grad():
        oracle_G(P, torch.as_tensor(np.asarray(X), dtype=torch.float64), torch.as_tensor(np.asarray(noise), dtype=torch.float64), pres)
    return min(float(p.abs().min()) for _, p in pres if p.shape[0] * p.shape[1] * p.shape[2] <= max_positions)


def critic_kink_margin(variables, X, y, noise, max_positions):
    """How far the critic's SMALL layers keep their lrelu inputs from zero on D(X, y) and D(X, g), in units of what float32 does
    to them: min |input| / rms(float32 input - float64 input) per layer, the minimum over the small layers -- the analogue of
    tests/_sampler_ref.critic_kink_margin.  Both evaluations are the oracle's own."""
    pres = {}
    for dtype in (torch.float64, torch.float32):
        P = {k: torch.tensor(np.asarray(v)).to(dtype) for k, v in variables.items() if k.startswith(('generator/', 'discriminator/'))}
        Xt, yt, nt = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (X, y, noise))
        with torch.no_grad():
            g = oracle_G(P, Xt, nt)
            for tag, depth in (('fake', g), ('real', yt)):
                for name, p in critic_inputs(P, Xt, depth).items():
                    if name != 'h6' and p.shape[0] * p.shape[1] * p.shape[2] <= max_positions:
                        pres[(dtype, tag, name)] = p.double()
    return min(float(p.abs().min()) / float((p - pres[(torch.float32,) + k[1:]]).pow(2).mean().sqrt())
               for k, p in pres.items() if k[0] == torch.float64)


# ------------------------------------------------------------------------------------------------ statistics
def set_stats(y, g):
    """(moments mean, moments var, rmse/mean, rmse/min) of one set: y, g [n, ...] on [-1, 1], float64."""
    y, g = np.asarray(y, np.float64).reshape(len(y), -1), np.asarray(g, np.float64).reshape(len(g), -1)
    per_image = 10.0 * np.mean(np.abs(y - g), axis=1)
    return np.array([g.mean(axis=0).mean(), g.var(axis=0).mean(), per_image.mean(), per_image.min()])


def set_stats_literal(y, g):
    """hem/models/experimental_sampler.py:378-383 and hem/ops/summaries.py:87-90 transcribed line by line on [n,1,32,32]."""
    y_hat = g
    rmse = np.mean(np.sqrt(np.square(y - y_hat)), axis=(1, 2, 3)) * 10.0
    mean = np.mean(g, axis=0, keepdims=True)                 # mean, var = tf.nn.moments(x, axes=[0])
    var = np.mean(np.square(g - mean), axis=0)
    return np.array([np.mean(mean), np.mean(var), np.mean(rmse), np.min(rmse)])


# ------------------------------------------------------------------------------------------------ data
class Batches:
    """6-tuple batches at 64x64 / 53x70: uniform x, y in (0.01, 0.99), the location ramps of a 64x64 frame cut whole, uniform
    x_full and a y_full around a per-image level."""

    def __init__(self, B, n, seed=0, device='cpu'):
        g = torch.Generator().manual_seed(seed)
        ramp = (torch.arange(SRC, dtype=torch.float64) / (SRC - 1)).float()
        self.x = [torch.rand(B, SRC, SRC, 3, generator=g).to(device) for _ in range(n)]
        self.y = [(torch.rand(B, SRC, SRC, 1, generator=g) * 0.98 + 0.01).to(device) for _ in range(n)]
        self.x_loc = ramp[None, None, :, None].expand(B, SRC, SRC, 1).contiguous().to(device)
        self.y_loc = ramp[None, :, None, None].expand(B, SRC, SRC, 1).contiguous().to(device)
        self.x_full = [torch.rand(B, FULL[0], FULL[1], 3, generator=g).to(device) for _ in range(n)]
        self.y_full = [(torch.rand(B, FULL[0], FULL[1], 1, generator=g) * 0.5 + 0.25).to(device) for _ in range(n)]
        self.i = 0

    def batch(self, k):
        return self.x[k], self.y[k], self.x_loc, self.y_loc, self.x_full[k], self.y_full[k]

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.batch(k)


def adam_ref(v, g, slots, key, lr, b1, b2, eps=1e-8):
    """One tf.train.AdamOptimizer step from zero slots (t = 1), float64."""
    m, s = (1.0 - b1) * g, (1.0 - b2) * g * g
    slots[key] = (m, s)
    return v - lr * np.sqrt(1.0 - b2) / (1.0 - b1) * m / (np.sqrt(s) + eps)
