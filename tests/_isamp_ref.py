"""Float64 statements of improved_sampler (hem/models/improved_sampler.py) for the tests, on torch autograd (oracle/torch_ref.py's
primitives, batch norm in training mode included): the input assembly per arch (:109-181), the six generators (:262-540, A1's
batch-normed head among them) and four critics (:638-808), every loss variant (:911-952), both gradient sets from ONE forward
pass (:216-221, :258), the statistics of a summary set, batch sources, a narrow-width copy for the differentiation check, the
variables a fresh model holds (the engine's draw order restated on the host) and the kink-margin helpers.  Test infrastructure
only."""
import numpy as np
import torch

from oracle.torch_ref import conv2d_same, conv2d_transpose_same, conv2d_valid, conv2d_transpose_valid, lrelu, batch_norm
from _xsamp_ref import noise_channel, set_stats                      # the family shares them

# g_arch -> source side, crop side, crop offset, planes of X, network kind, batch-normed layers (encoder, decoder)
ARCHS = {
    'A1': dict(S=65, T=31, off=17, P=3, kind='A', bn=(('e2', 'e3', 'e4'), ('d1', 'd2', 'd3', 'd4'))),
    'A2': dict(S=65, T=31, off=17, P=3, kind='A', bn=(('e2', 'e3'), ())),
    'A3': dict(S=65, T=31, off=17, P=3, kind='A', bn=((), ())),
    'B2': dict(S=64, T=32, off=16, P=3, kind='E', bn=((), ())),
    'D1': dict(S=64, T=32, off=16, P=5, kind='E', bn=((), ())),
    'E1': dict(S=64, T=32, off=16, P=6, kind='E', bn=((), ())),
}
PAIRS = (('A1', 'A1'), ('A2', 'A1'), ('A3', 'A1'), ('B2', 'B2'), ('D1', 'D1'), ('E1', 'E1'))
LOSS_KEYS = ('g_fake', 'd_real', 'd_fake', 'd_total', 'rmse', 'l1')
SETS = ('sampler', 'shuffled', 'noise')
ENTRIES = {3: 2, 5: 4, 6: 5}                       # planes -> entries of the dataset's tuple


def loss_keys(g_rmse=False, g_sparsity=False):
    return LOSS_KEYS + (('g_total', 'sparsity_term') if g_sparsity else (('g_total',) if g_rmse else ()))


def widths(g_arch, narrow=False):
    """Channels in -> out per layer; the narrow copy keeps the structure."""
    P = ARCHS[g_arch]['P']
    if ARCHS[g_arch]['kind'] == 'A':
        if narrow:
            return dict(e=(P + 1, 4, 4, 6, 8), hx=(P, 4, 4, 6, 8), hy=(1, 4, 6, 8), h=(16, 8, 6, 1))
        return dict(e=(P + 1, 64, 128, 256, 512), hx=(P, 64, 128, 256, 512), hy=(1, 128, 256, 512), h=(1024, 1024, 512, 1))
    if narrow:
        return dict(e=(P + 1, 4, 4, 6, 6, 8), hx=(P, 4, 4, 6, 6, 8), hy=(1, 4, 6, 6, 8), h=(16, 8, 6, 6, 4, 4, 1))
    return dict(e=(P + 1, 64, 128, 256, 512, 1024), hx=(P, 64, 128, 256, 512, 1024), hy=(1, 128, 256, 512, 1024),
                h=(2048, 1024, 512, 256, 128, 64, 1))


def bn_names(g_arch):
    """layer -> beta name by Net.bn_name: BatchNorm, BatchNorm_1, ... per scope in layer order."""
    out = {}
    for scope, layers in zip(('encoder', 'decoder'), ARCHS[g_arch]['bn']):
        for i, l in enumerate(layers):
            out[l] = 'generator/%s/BatchNorm%s/beta' % (scope, '' if i == 0 else '_%d' % i)
    return out


def shapes(g_arch, w=None):
    """Variable name -> shape in the model's declaration order per store (generator, then discriminator)."""
    w = w or widths(g_arch)
    e, hx, hy, h = w['e'], w['hx'], w['hy'], w['h']
    A = ARCHS[g_arch]['kind'] == 'A'
    n = len(e) - 1                                 # encoder depth: 4 (A) or 5 (E)
    fe = lambda k: 5 if A or k < n else 4          # encoder / rgb-path filter side of layer k
    out = {}
    for k in range(1, n + 1):
        out['generator/encoder/vars/e%d/weights' % k], out['generator/encoder/vars/e%d/bias' % k] = (fe(k), fe(k), e[k - 1], e[k]), (e[k],)
    cin = e[n]
    for i in range(1, n):                          # decoder d_i [k, k, Cout, Cin]; Cin = previous decoder width + mirrored encoder width
        f, co = (5 if A or i > 1 else 4), e[n - i]
        out['generator/decoder/vars/d%d/weights' % i], out['generator/decoder/vars/d%d/bias' % i] = (f, f, co, cin), (co,)
        cin = co + e[n - i]
    out['generator/decoder/vars/d%d/weights' % n], out['generator/decoder/vars/d%d/bias' % n] = (1, 1, cin, 1), (1,)
    for k in range(1, n + 1):
        out['discriminator/rgb_path/vars/hx%d/weights' % k], out['discriminator/rgb_path/vars/hx%d/bias' % k] = \
            (fe(k), fe(k), hx[k - 1], hx[k]), (hx[k],)
    for k in range(1, n):
        f = 5 if A or k < n - 1 else 4
        out['discriminator/depth_path/vars/hy%d/weights' % k], out['discriminator/depth_path/vars/hy%d/bias' % k] = \
            (f, f, hy[k - 1], hy[k]), (hy[k],)
    for k in range(1, len(h)):
        out['discriminator/combined_path/vars/h%d/weights' % k], out['discriminator/combined_path/vars/h%d/bias' % k] = \
            (1, 1, h[k - 1], h[k]), (h[k],)
    return out


def beta_shapes(g_arch, w=None):
    w = w or widths(g_arch)
    e, n = w['e'], len(w['e']) - 1
    size = {'e%d' % k: e[k] for k in range(1, n + 1)}
    size.update({'d%d' % i: e[n - i] for i in range(1, n)})
    size['d%d' % n] = 1
    return {name: (size[l],) for l, name in bn_names(g_arch).items()}


def random_variables(g_arch, w, seed=0, scale=1.0):
    """Xavier-like float64 variables of the given widths and betas in (-0.5, 0.5) (the differentiation check's narrow copy)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, s in shapes(g_arch, w).items():
        fan = np.prod(s[:-1]) + s[-1] if len(s) > 1 else 2 * s[0]
        out[k] = rng.uniform(-1, 1, s) * scale * np.sqrt(6.0 / fan)
    for k, s in beta_shapes(g_arch, w).items():
        out[k] = rng.uniform(-0.5, 0.5, s)
    return out


def initial_variables(g_arch, seed=0):
    """The float32 variables of a fresh full-width model of session seed `seed`: engine.init_weights' draws restated -- one
    torch.Generator, xavier-uniform weights then bias per layer, encoder, decoder, rgb_path, depth_path, combined_path; betas zero."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in shapes(g_arch).items():
        if len(s) == 1:
            fan_in = fan_out = s[0]
        else:
            rf = int(np.prod(s[:-2]))
            fan_in, fan_out = rf * s[-2], rf * s[-1]
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        out[k] = ((torch.rand(s, generator=gen, dtype=torch.float32) * 2 - 1) * lim).numpy()
    for k, s in beta_shapes(g_arch).items():
        out[k] = np.zeros(s, np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the model
def assemble(g_arch, batch, dtype=torch.float64, x_rows=None, y_rows=None):
    """(X [B,S,S,P], y [B,T,T,1]) of :109-173: fl32(2x - 1) and fl32(2y - 1) as hem.rescale rounds them, y cropped at (off, off),
    X = [x | x_loc | y_loc | mean_vec] as far as the arch reads.  x_rows / y_rows: tdg_isamp_prep's row maps."""
    a = ARCHS[g_arch]
    t = [torch.as_tensor(np.asarray(b.cpu() if hasattr(b, 'cpu') else b), dtype=torch.float32) for b in batch[:ENTRIES[a['P']]]]
    B = t[0].shape[0]
    xr = torch.arange(B) if x_rows is None else torch.as_tensor(np.asarray(x_rows), dtype=torch.long)
    yr = torch.arange(B) if y_rows is None else torch.as_tensor(np.asarray(y_rows), dtype=torch.long)
    X = torch.cat([2.0 * t[0][xr] - 1.0] + [p[xr] for p in t[2:]], dim=-1)
    o, T = a['off'], a['T']
    yc = (2.0 * t[1][yr] - 1.0)[:, o:o + T, o:o + T, :]
    return X.to(dtype), yc.to(dtype)


def oracle_G(g_arch, P, X, noise, pres=None, acts=None):
    """The generator of `g_arch`, NHWC: `noise` [B,S,S,1] is concatenated behind X.  pres receives every (l)relu's input (behind
    batch norm where there is one), acts the encoder's outputs by name."""
    def W(n):
        return P['generator/' + n]
    a, bn = ARCHS[g_arch], bn_names(g_arch)
    A = a['kind'] == 'A'
    n = 4 if A else 5
    norm = lambda l, h: batch_norm(h, P[bn[l]]) if l in bn else h
    h = torch.cat([X, noise], dim=-1)
    e = []
    for k in range(1, n + 1):
        w, b = W('encoder/vars/e%d/weights' % k), W('encoder/vars/e%d/bias' % k)
        h = norm('e%d' % k, (conv2d_valid(h, w, 2) if A or k == n else conv2d_same(h, w, 2)) + b)
        if pres is not None:
            pres.append(('e%d' % k, h))
        h = torch.relu(h)
        e.append(h)
        if acts is not None:
            acts['e%d' % k] = h
    y = e[n - 1]
    for i in range(1, n):
        w, b = W('decoder/vars/d%d/weights' % i), W('decoder/vars/d%d/bias' % i)
        side = e[n - 1 - i].shape[1]
        y = norm('d%d' % i, (conv2d_transpose_valid(y, w, (side, side)) if A or i == 1 else conv2d_transpose_same(y, w)) + b)
        if pres is not None:
            pres.append(('d%d' % i, y))
        y = torch.cat([lrelu(y, 0.2), e[n - 1 - i]], dim=-1)
    head = 'd%d' % n
    z = norm(head, conv2d_same(y, W('decoder/vars/%s/weights' % head), 1) + W('decoder/vars/%s/bias' % head))
    return torch.tanh(z)                                                               # [B,T,T,1]


def critic_inputs(g_arch, P, X, depth):
    """The inputs of the critic's lrelus by layer name, and the logits as the last combined layer's entry (`logits`)."""
    def W(n):
        return P['discriminator/' + n]
    A = ARCHS[g_arch]['kind'] == 'A'
    n = 4 if A else 5
    out, h1, h2 = {}, X, depth
    for k in range(1, n + 1):
        w, b = W('rgb_path/vars/hx%d/weights' % k), W('rgb_path/vars/hx%d/bias' % k)
        out['hx%d' % k] = (conv2d_valid(h1, w, 2) if A or k == n else conv2d_same(h1, w, 2)) + b
        h1 = lrelu(out['hx%d' % k], 0.2)
    for k in range(1, n):
        w, b = W('depth_path/vars/hy%d/weights' % k), W('depth_path/vars/hy%d/bias' % k)
        out['hy%d' % k] = (conv2d_valid(h2, w, 2) if A or k == n - 1 else conv2d_same(h2, w, 2)) + b
        h2 = lrelu(out['hy%d' % k], 0.2)
    h = torch.cat([h1, h2], dim=-1)
    nc = 3 if A else 6
    for k in range(1, nc + 1):
        out['h%d' % k] = conv2d_same(h, W('combined_path/vars/h%d/weights' % k), 1) + W('combined_path/vars/h%d/bias' % k)
        h = lrelu(out['h%d' % k], 0.2)
    out['logits'] = out.pop('h%d' % nc)
    return out


def oracle_D(g_arch, P, X, depth):
    return critic_inputs(g_arch, P, X, depth)['logits']


def oracle_forward(g_arch, P, X, y, noise, g_rmse=False, g_sparsity=False):
    """:204-216 and :911-952 for one batch: (losses in the dict's order, g, the loss G trains on)."""
    acts = {}
    g = oracle_G(g_arch, P, X, noise, acts=acts)
    zr, zf = oracle_D(g_arch, P, X, y), oracle_D(g_arch, P, X, g)
    sp = torch.nn.functional.softplus
    g_fake, d_real, d_fake = sp(-zf).mean(), sp(-zr).mean(), sp(zf).mean()
    g01, y01 = (g + 1.0) / 2.0, (y + 1.0) / 2.0
    rmse = torch.sqrt(torch.mean(torch.square(y01 - g01)))
    losses = {'g_fake': g_fake, 'd_real': d_real, 'd_fake': d_fake, 'd_total': d_real + d_fake, 'rmse': rmse,
              'l1': torch.mean(torch.abs(y01 - g01))}
    g_loss = g_fake
    if g_sparsity:
        sparsity = (acts['e5'].detach() == 0).to(g.dtype).mean()                      # tf.nn.zero_fraction: no gradient
        g_loss = g_fake - sparsity + (rmse if g_rmse else 0.0)
        losses['g_total'], losses['sparsity_term'] = g_loss, sparsity
    elif g_rmse:
        g_loss = losses['g_total'] = g_fake + rmse
    return losses, g, g_loss


def oracle_grads(g_arch, variables, X, y, noise, g_rmse=False, g_sparsity=False, dtype=torch.float64):
    """(losses, D gradients of d_total, G gradients of the loss G trains on, g) from ONE forward pass at `variables`."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in variables.items()
         if k.startswith(('generator/', 'discriminator/'))}
    X, y, noise = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (X, y, noise))
    losses, g, g_loss = oracle_forward(g_arch, P, X, y, noise, g_rmse, g_sparsity)
    dn, gn = [k for k in P if k.startswith('discriminator/')], [k for k in P if k.startswith('generator/')]
    dg = torch.autograd.grad(losses['d_total'], [P[k] for k in dn], retain_graph=True)
    gg = torch.autograd.grad(g_loss, [P[k] for k in gn])
    return ({k: float(v.detach()) for k, v in losses.items()}, {k: t.double().numpy() for k, t in zip(dn, dg)},
            {k: t.double().numpy() for k, t in zip(gn, gg)}, g.detach().double().numpy())


# ------------------------------------------------------------------------------------------------ kinks
def nearest_kink(g_arch, variables, X, noise, max_positions):
    """The smallest |input| of the (l)relus of the generator's SMALL layers (at most `max_positions` outputs per channel in the
    whole batch) in float64 -- tests/_xsamp_ref.nearest_kink for this family."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in variables.items() if k.startswith('generator/')}
    pres = []
    with torch.no_grad():
        oracle_G(g_arch, P, torch.as_tensor(np.asarray(X), dtype=torch.float64), torch.as_tensor(np.asarray(noise), dtype=torch.float64), pres)
    return min(float(p.abs().min()) for _, p in pres if p.shape[0] * p.shape[1] * p.shape[2] <= max_positions)


def critic_kink_margin(g_arch, variables, X, y, noise, max_positions):
    """min |input| / rms(float32 input - float64 input) per small critic layer on D(X, y) and D(X, g), the minimum over them --
    tests/_xsamp_ref.critic_kink_margin for this family.  Both evaluations are the oracle's own."""
    pres = {}
    for dtype in (torch.float64, torch.float32):
        P = {k: torch.tensor(np.asarray(v)).to(dtype) for k, v in variables.items() if k.startswith(('generator/', 'discriminator/'))}
        Xt, yt, nt = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (X, y, noise))
        with torch.no_grad():
            g = oracle_G(g_arch, P, Xt, nt)
            for tag, depth in (('fake', g), ('real', yt)):
                for name, p in critic_inputs(g_arch, P, Xt, depth).items():
                    if name != 'logits' and p.shape[0] * p.shape[1] * p.shape[2] <= max_positions:
                        pres[(dtype, tag, name)] = p.double()
    return min(float(p.abs().min()) / float((p - pres[(torch.float32,) + k[1:]]).pow(2).mean().sqrt())
               for k, p in pres.items() if k[0] == torch.float64)


# ------------------------------------------------------------------------------------------------ data
class Batches:
    """The tuple `g_arch` reads at S x S: uniform x, y in (0.01, 0.99), the location ramps of an S x S frame cut whole, mean_vec
    the per-image mean of y as a plane."""

    def __init__(self, g_arch, B, n, seed=0, device='cpu'):
        a = ARCHS[g_arch]
        S, self.entries = a['S'], ENTRIES[a['P']]
        g = torch.Generator().manual_seed(seed)
        ramp = (torch.arange(S, dtype=torch.float64) / (S - 1)).float()
        self.x = [torch.rand(B, S, S, 3, generator=g).to(device) for _ in range(n)]
        ys = [torch.rand(B, S, S, 1, generator=g) * 0.98 + 0.01 for _ in range(n)]
        self.y = [t.to(device) for t in ys]
        self.x_loc = ramp[None, None, :, None].expand(B, S, S, 1).contiguous().to(device)
        self.y_loc = ramp[None, :, None, None].expand(B, S, S, 1).contiguous().to(device)
        self.mean_vec = [t.mean(dim=(1, 2, 3), keepdim=True).expand(B, S, S, 1).contiguous().to(device) for t in ys]
        self.i = 0

    def batch(self, k):
        return (self.x[k], self.y[k], self.x_loc, self.y_loc, self.mean_vec[k])[:self.entries]

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.batch(k)
