"""Float64 statement of artist (hem/models/artist.py) for the tests, on torch autograd (oracle/torch_ref.py's primitives, batch
norm in training mode with beta only): the input rescale, the encoder and the two decoders, the three losses with the target's
float32 round trip, the gradients of the two variable sets (y_hat_loss: encoder + y_decoder; x_hat_loss: x_decoder ONLY), one
Adam step, the variables a fresh model holds (the engine's draw order restated on the host), the kink report and a batch source.
Written from the model's description (widths, sides, which layers are batch-normed, the operation order of hem.rescale), not from
the product's code.  Test infrastructure only."""
import numpy as np
import torch

from oracle.torch_ref import conv2d_valid, conv2d_transpose_valid, lrelu, batch_norm

SIDE = 256
E_WIDTHS = (3, 6, 12, 24, 48, 192, 384)                    # e1..e6: in -> out
E_SIDES = (126, 61, 29, 13, 5, 1)
D_WIDTHS = (384, 192, 48, 24, 12, 6)                       # d1..d6: in -> out, the last out = C
D_SIDES = (5, 13, 29, 61, 126, 256)
E_BN = ('e2', 'e3', 'e4', 'e5', 'e6')
D_BN = ('d1', 'd2', 'd3', 'd4', 'd5', 'd6')
CHANNELS = {'x_decoder': 3, 'y_decoder': 1}
LOSS_KEYS = ('x_hat_loss', 'y_hat_loss', 'y_hat_rmse')
X_SET = ('x_decoder/',)                                    # :48
Y_SET = ('encoder/', 'y_decoder/')                         # :49


def _bn(scope, i):
    return '%s/BatchNorm%s/beta' % (scope, '' if i == 0 else '_%d' % i)


def bn_names():
    """layer -> beta name per scope, by Net.bn_name: BatchNorm, BatchNorm_1, ... in layer order."""
    out = {('encoder', l): _bn('encoder', i) for i, l in enumerate(E_BN)}
    for scope in CHANNELS:
        out.update({(scope, l): _bn(scope, i) for i, l in enumerate(D_BN)})
    return out


def weight_shapes(scope):
    """name -> shape of one scope's weights and biases in layer order."""
    out = {}
    if scope == 'encoder':
        for k in range(1, 7):
            out['encoder/vars/e%d/weights' % k] = (5, 5, E_WIDTHS[k - 1], E_WIDTHS[k])
            out['encoder/vars/e%d/bias' % k] = (E_WIDTHS[k],)
        return out
    w = D_WIDTHS + (CHANNELS[scope],)
    for k in range(1, 7):
        out['%s/vars/d%d/weights' % (scope, k)] = (5, 5, w[k], w[k - 1])           # deconv2d: [k, k, Cout, Cin]
        out['%s/vars/d%d/bias' % (scope, k)] = (w[k],)
    return out


def beta_shapes():
    out = {}
    for (scope, l), name in bn_names().items():
        k = int(l[1])
        out[name] = (E_WIDTHS[k],) if scope == 'encoder' else ((D_WIDTHS + (CHANNELS[scope],))[k],)
    return out


def shapes():
    out = {}
    for scope in ('encoder', 'x_decoder', 'y_decoder'):
        out.update(weight_shapes(scope))
    out.update(beta_shapes())
    return out


def dead_biases():
    """The conv biases in front of a batch norm: no influence on any loss, a gradient of rounding noise."""
    return {'%s/vars/%s/bias' % (scope, l) for scope, l in bn_names()}


def initial_variables(seed=0):
    """The float32 variables of a fresh model of session seed `seed`: one torch.Generator, xavier-uniform weights then bias per
    layer, scopes in the reference's creation order encoder, x_decoder, y_decoder; betas zero."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for scope in ('encoder', 'x_decoder', 'y_decoder'):
        for k, s in weight_shapes(scope).items():
            if len(s) == 1:
                fan_in = fan_out = s[0]
            else:
                rf = int(np.prod(s[:-2]))
                fan_in, fan_out = rf * s[-2], rf * s[-1]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            out[k] = ((torch.rand(s, generator=gen, dtype=torch.float32) * 2 - 1) * lim).numpy()
    for k, s in beta_shapes().items():
        out[k] = np.zeros(s, np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the model
def f32(t):
    return torch.as_tensor(np.asarray(t.cpu() if hasattr(t, 'cpu') else t), dtype=torch.float32)


def rescale_in(t):
    """hem.rescale((0, 1), (-1, 1)) in float32: fl(fl(2 t) - 1), as float64."""
    return (2.0 * f32(t) - 1.0).double()


def target01(t):
    """The loss target: the staged float32 batch through the reference's round trip, fl(fl(fl(fl(2 t) - 1) + 1) / 2), as float64."""
    return (((2.0 * f32(t) - 1.0) + 1.0) / 2.0).double()


def encoder(P, X, pres=None):
    h, bn = X, bn_names()
    for k in range(1, 7):
        l = 'e%d' % k
        h = conv2d_valid(h, P['encoder/vars/%s/weights' % l], 2) + P['encoder/vars/%s/bias' % l]
        if l in E_BN:
            h = batch_norm(h, P[bn[('encoder', l)]])
        if pres is not None:
            pres.append(('encoder', l, h))
        h = lrelu(h, 0.2)
    return h


def decoder(P, scope, e, pres=None):
    h, bn = e, bn_names()
    for k in range(1, 7):
        l = 'd%d' % k
        side = D_SIDES[k - 1]
        h = conv2d_transpose_valid(h, P['%s/vars/%s/weights' % (scope, l)], (side, side)) + P['%s/vars/%s/bias' % (scope, l)]
        h = batch_norm(h, P[bn[(scope, l)]])
        if k < 6:
            if pres is not None:
                pres.append((scope, l, h))
            h = lrelu(h, 0.2)
    return torch.tanh(h)


def forward(P, x, y, pres=None):
    """(losses, xhat01, yhat01) of one batch (x, y in [0, 1], float32) at the float64 variables P."""
    e = encoder(P, rescale_in(x), pres)
    x_hat, y_hat = decoder(P, 'x_decoder', e, pres), decoder(P, 'y_decoder', e, pres)
    x01, y01 = (x_hat + 1.0) / 2.0, (y_hat + 1.0) / 2.0
    x_loss = torch.mean(torch.square(target01(x) - x01))
    y_loss = torch.mean(torch.square(target01(y) - y01))
    return {'x_hat_loss': x_loss, 'y_hat_loss': y_loss, 'y_hat_rmse': torch.sqrt(y_loss)}, x01, y01


def tensors(variables, grad=True):
    return {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=grad) for k, v in variables.items()}


def oracle_grads(variables, x, y):
    """(losses, gradients of y_hat_loss on encoder + y_decoder, gradients of x_hat_loss on x_decoder, xhat01, yhat01) from ONE
    forward pass at `variables`."""
    P = tensors(variables)
    losses, x01, y01 = forward(P, x, y)
    yn, xn = [k for k in P if k.startswith(Y_SET)], [k for k in P if k.startswith(X_SET)]
    yg = torch.autograd.grad(losses['y_hat_loss'], [P[k] for k in yn], retain_graph=True)
    xg = torch.autograd.grad(losses['x_hat_loss'], [P[k] for k in xn])
    return ({k: float(v.detach()) for k, v in losses.items()}, {k: t.numpy() for k, t in zip(yn, yg)},
            {k: t.numpy() for k, t in zip(xn, xg)}, x01.detach().numpy(), y01.detach().numpy())


def adam_step(v, g, lr, b1, b2, eps=1e-8):
    """One tf.train.AdamOptimizer step from zero slots (t = 1), float64."""
    m, s = (1.0 - b1) * g, (1.0 - b2) * g * g
    return v - lr * np.sqrt(1.0 - b2) / (1.0 - b1) * m / (np.sqrt(s) + eps)


def oracle_train(variables, batch_y, batch_x, lr, b1, b2):
    """train() (:65-68) under Adam: the y step on `batch_y`, then the x step on `batch_x` at the updated encoder.  Returns
    (variables after, {'x_loss', 'y_loss'}, the gradients each variable was updated with)."""
    V = {k: np.asarray(v, np.float64) for k, v in variables.items()}
    ly, yg, _, _, _ = oracle_grads(V, *batch_y)
    for k, g in yg.items():
        V[k] = adam_step(V[k], g, lr, b1, b2)
    lx, _, xg, _, _ = oracle_grads(V, *batch_x)
    for k, g in xg.items():
        V[k] = adam_step(V[k], g, lr, b1, b2)
    grads = dict(yg)
    grads.update(xg)
    return V, {'x_loss': lx['x_hat_loss'], 'y_loss': ly['y_hat_loss']}, grads


def float32_y_step(variables, batch_y, lr, b1, b2):
    """The variables after the y step when the REFERENCE evaluates that step in float32 (torch on the CPU: forward, loss and
    autograd in float32, the Adam step from those gradients, the result stored as float32, as a float32 model holds it).  Nothing
    of the product takes part: this is what the number format alone does to the first of train()'s two steps."""
    P = {k: torch.tensor(np.asarray(v), dtype=torch.float32, requires_grad=True) for k, v in variables.items()}
    x, y = batch_y
    y_hat = decoder(P, 'y_decoder', encoder(P, 2.0 * f32(x) - 1.0))
    loss = torch.mean(torch.square(((2.0 * f32(y) - 1.0) + 1.0) / 2.0 - (y_hat + 1.0) / 2.0))
    names = [k for k in P if k.startswith(Y_SET)]
    grads = torch.autograd.grad(loss, [P[k] for k in names])
    out = {k: np.asarray(v, np.float64) for k, v in variables.items()}
    for k, g in zip(names, grads):
        out[k] = adam_step(out[k], g.double().numpy(), lr, b1, b2).astype(np.float32).astype(np.float64)
    return out


def x_step_reference_error(variables, batch_y, batch_x, lr, b1, b2):
    """{variable: |update - update'|} of the x set: the float64 x step at the float64 y step's variables against the float64 x
    step at float32_y_step's variables -- how far the reference's own x updates move when only its FIRST step is held in
    float32."""
    V = {k: np.asarray(v, np.float64) for k, v in variables.items()}
    V64, _, grads = oracle_train(V, batch_y, batch_x, lr, b1, b2)
    _, _, xg32, _, _ = oracle_grads(float32_y_step(variables, batch_y, lr, b1, b2), *batch_x)
    return {k: np.abs((V64[k] - V[k]) - (adam_step(V[k], g, lr, b1, b2) - V[k])) for k, g in xg32.items()}, {k: grads[k] for k in xg32}


# ------------------------------------------------------------------------------------------------ kinks
def kink_report(variables, x, tol=1e-6):
    """Every lrelu input of the three nets, in float64, through tests/_kinks.py's recorder: (the entries it reports within `tol`
    of the kink, the smallest |input| over all layers, the number of inputs seen)."""
    from _kinks import Kinks
    rec, pres = Kinks(tol), []
    with torch.no_grad():
        forward(tensors(variables, grad=False), x, torch.zeros(x.shape[0], SIDE, SIDE, 1), pres)
    for scope, layer, p in pres:
        rec.mask(scope, layer, p.numpy(), None, 0.2)
    return rec.near, min(float(p.abs().min()) for _, _, p in pres), sum(p.numel() for _, _, p in pres)


# ------------------------------------------------------------------------------------------------ data
class Batches:
    """(x [B,256,256,3] uniform in [0, 1), y [B,256,256,1] uniform in (0.01, 0.99)) pairs."""

    def __init__(self, B, n, seed=0, device='cpu'):
        g = torch.Generator().manual_seed(seed)
        self.x = [torch.rand(B, SIDE, SIDE, 3, generator=g).to(device) for _ in range(n)]
        self.y = [(torch.rand(B, SIDE, SIDE, 1, generator=g) * 0.98 + 0.01).to(device) for _ in range(n)]
        self.i = 0

    def batch(self, k):
        return self.x[k], self.y[k]

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.batch(k)


class Pairs(Batches):
    """The given (x, y) batches in turn."""

    def __init__(self, batches):
        self.x, self.y, self.i = [b[0] for b in batches], [b[1] for b in batches], 0
