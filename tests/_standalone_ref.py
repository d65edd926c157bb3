"""Float64 statements of paper_standalone (hem/models/paper_standalone.py) for the tests: the four generators and the RMSE
loss on torch autograd (oracle/torch_ref.py's primitives; test infrastructure only), the loss's closed-form gradient, and one
Adam step."""
import numpy as np
import torch

from oracle.torch_ref import conv2d_valid, conv2d_transpose_valid, conv2d_same, lrelu

VERSIONS = ('baseline', 'mean_adjusted', 'mean_provided', 'mean_provided2')
# the input width of every encoder layer and of the head, per version (:140-242)
ENCODER_WIDTHS = {'baseline': [3, 64, 128, 256], 'mean_adjusted': [3, 64, 128, 256], 'mean_provided': [3, 65, 128, 256],
                  'mean_provided2': [4, 64, 128, 256]}
HEAD_WIDTH = {'baseline': 128, 'mean_adjusted': 128, 'mean_provided': 129, 'mean_provided2': 128}


def target(y01):
    """:54-66: y = crop(10 y01, 17, 17, 29, 29) and its per-image mean [B,1,1,1]."""
    y = 10.0 * y01[:, 17:46, 17:46, :]
    return y, y.mean(dim=(1, 2, 3), keepdim=True)


def oracle_G(P, x, version, ybar, pres=None):
    """g_baseline (:140-173), g_mean_provided (:176-207: e1's output and the last skip concat carry a channel of y_bar) and
    g_mean_provided2 (:209-242: x carries a channel of ones), NHWC; returns g [B,29,29,1].  pres: a list that receives every
    (l)relu's input."""
    def W(n):
        return P['generator/' + n]
    B = x.shape[0]
    h = torch.cat([x, torch.ones_like(x[..., :1])], dim=-1) if version == 'mean_provided2' else x
    bar = ybar.reshape(B, 1, 1, 1).expand(B, 31, 31, 1) if version == 'mean_provided' else None
    e = []
    for k in range(1, 5):
        h = conv2d_valid(h, W('encoder/vars/e%d/weights' % k), 2) + W('encoder/vars/e%d/bias' % k)
        if pres is not None:
            pres.append(h)
        h = torch.relu(h)
        if k == 1 and bar is not None:
            h = torch.cat([h, bar], dim=-1)
        e.append(h)
    y = e[3]
    for i, hw in ((1, 5), (2, 14), (3, 31)):
        y = conv2d_transpose_valid(y, W('decoder/vars/d%d/weights' % i), (hw, hw)) + W('decoder/vars/d%d/bias' % i)
        if pres is not None:
            pres.append(y)
        y = torch.cat([lrelu(y, 0.2), e[3 - i]], dim=-1)
    y = conv2d_same(y, W('decoder/vars/d4/weights'), 1) + W('decoder/vars/d4/bias')
    return y[:, :29, :29, :]


def rmse_literal(y, y_hat):
    """:244-253 as written: sqrt(mean((y_hat/10 - y/10)^2)) over every element of the batch."""
    return torch.sqrt(torch.mean(torch.square(y_hat / 10.0 - y / 10.0)))


def rmse_closed(y, y_hat):
    """(loss, d loss / d y_hat) in NumPy float64: sqrt(S / N) / 10 and d / (10 sqrt(N S)), d = y_hat - y, S = sum d^2."""
    d = np.asarray(y_hat, np.float64) - np.asarray(y, np.float64)
    S, N = float(np.sum(d * d)), d.size
    return np.sqrt(S / N) / 10.0, d / (10.0 * np.sqrt(N * S))


def _tensors(variables, batch, dtype, grad):
    P = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=grad) for k, v in variables.items() if k.startswith('generator/')}
    x, y01 = (torch.tensor(np.asarray(t.cpu() if hasattr(t, 'cpu') else t), dtype=dtype) for t in batch)
    return P, x, y01


def oracle_grads(variables, batch, version, dtype=torch.float64):
    """(rmse, its gradients by variable name, y_hat [B,29,29,1]) of one batch in `dtype`."""
    P, x, y01 = _tensors(variables, batch, dtype, True)
    y, ybar = target(y01)
    g = oracle_G(P, x, version, ybar)
    y_hat = g if version == 'baseline' else g + ybar
    loss = rmse_literal(y, y_hat)
    names = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in names])
    return float(loss.detach()), {k: g.double().numpy() for k, g in zip(names, grads)}, y_hat.detach().double().numpy()


def nearest_kink(variables, batch, version, max_positions=100):
    """The smallest |input| of the (l)relus of the generator's SMALL layers (at most `max_positions` outputs per channel in the
    whole batch: e3, e4 and d1 at B = 4) on this batch, in float64 -- see tests/_sampler_ref.nearest_kink."""
    P, x, y01 = _tensors(variables, batch, torch.float64, False)
    pres = []
    with torch.no_grad():
        oracle_G(P, x, version, target(y01)[1], pres)
    return min(float(p.abs().min()) for p in pres if p.shape[0] * p.shape[1] * p.shape[2] <= max_positions)


def adam_first_step(P, G, lr, b1, b2, eps=1e-8):
    """The first step of tf.train.AdamOptimizer in float64 on torch.optim.Adam: TF's lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) with
    eps outside the bias correction is torch's update with eps' = eps / sqrt(1 - b2^t), here at t = 1."""
    p = torch.tensor(np.asarray(P, np.float64), requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps / np.sqrt(1.0 - b2))
    p.grad = torch.tensor(np.asarray(G, np.float64))
    opt.step()
    return p.detach().numpy()
