"""Float64 statements of mean_depth_estimator (hem/models/mean_depth_estimator.py) for the tests, on torch autograd: the E2
network as six TF-SAME 5x5 stride-2 convs (explicit asymmetric F.pad, then a VALID F.conv2d), the (w, c) flatten of the NHWC
path, two dense layers, and the loss as the reference writes it; the tdg_mde_loss kernel's NumPy statement; TF-1.x bilinear
resize in NumPy.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

NARROW = (8, 8, 16, 16, 24, 32, 16)
FULL = (53, 70)
SHAPES = [(27, 35), (14, 18), (7, 9), (4, 5), (2, 3), (1, 2)]


def same_pads(n, k=5, s=2):
    """TF's SAME split for one axis: (before, after), the odd element after."""
    total = max((-(-n // s) - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def names(n_layers=8):
    return ['model/vars/l%d/%s' % (i, w) for i in range(1, n_layers + 1) for w in ('weights', 'bias')]


def forward(P, x, pres=None):
    """m [B] of x [B,53,70,3] (NHWC) under the variables P; pres receives every relu's input."""
    h = x.permute(0, 3, 1, 2)
    for i in range(1, 7):
        (pt, pb), (pl, pr) = same_pads(h.shape[2]), same_pads(h.shape[3])
        w = P['model/vars/l%d/weights' % i].permute(3, 2, 0, 1)                   # [5,5,ci,co] -> [co,ci,5,5]
        h = F.conv2d(F.pad(h, (pl, pr, pt, pb)), w, stride=2) + P['model/vars/l%d/bias' % i][None, :, None, None]
        if pres is not None:
            pres.append(h)
        h = torch.relu(h)
    flat = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)                          # (w, c): the NHWC reinterpretation
    l7 = flat @ P['model/vars/l7/weights'] + P['model/vars/l7/bias']
    return torch.sigmoid(l7 @ P['model/vars/l8/weights'] + P['model/vars/l8/bias'])[:, 0]


def loss_literal(m, y):
    """:136-147 as written, NHWC: reduce_mean(sqrt(square(mean_depth - m)))."""
    return torch.mean(torch.sqrt(torch.square(y.mean(dim=(1, 2, 3)) - m)))


def _np(t):
    return np.asarray(t.cpu() if hasattr(t, 'cpu') else t)


def tensors(variables, dtype=torch.float64, grad=False):
    return {k: torch.tensor(_np(v), dtype=dtype, requires_grad=grad) for k, v in variables.items()}


def oracle_grads(variables, x, y, dtype=torch.float64):
    """(loss, gradients by variable name, m, mean depths) of one batch in `dtype`, as float64 NumPy."""
    P = tensors(variables, dtype, True)
    x, y = (torch.tensor(_np(t), dtype=dtype) for t in (x, y))
    m = forward(P, x)
    loss = loss_literal(m, y)
    keys = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in keys])
    return (float(loss.detach()), {k: g.double().numpy() for k, g in zip(keys, grads)}, m.detach().double().numpy(),
            y.mean(dim=(1, 2, 3)).double().numpy())


def nearest_kink(variables, x, max_positions=100):
    """The smallest |input| of the relus of the SMALL layers (at most `max_positions` outputs per channel in the whole batch) on
    this batch, in float64 -- as tests/_standalone_ref.nearest_kink."""
    pres = []
    with torch.no_grad():
        forward(tensors(variables), torch.tensor(_np(x), dtype=torch.float64), pres)
    return min(float(p.abs().min()) for p in pres if p.shape[0] * p.shape[2] * p.shape[3] <= max_positions)


def adam_steps(variables, batches, lr, b1, b2, eps=1e-8, dtype=torch.float64):
    """The variables after one tf.train.AdamOptimizer step per batch, and the loss of each batch before its step.  TF's
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) with eps outside the bias correction, written out."""
    P = {k: torch.tensor(_np(v), dtype=dtype) for k, v in variables.items()}
    mom = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in P.items()}
    losses = []
    for t, (x, y) in enumerate(batches, 1):
        l, g, _, _ = oracle_grads({k: v.numpy() for k, v in P.items()}, x, y, dtype)
        losses.append(l)
        lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        for k in P:
            gk = torch.tensor(g[k], dtype=dtype)
            m1, v1 = mom[k]
            m1.mul_(b1).add_(gk, alpha=1.0 - b1)
            v1.mul_(b2).add_(gk * gk, alpha=1.0 - b2)
            P[k] = P[k] - lr_t * m1 / (v1.sqrt() + eps)
    return {k: v.double().numpy() for k, v in P.items()}, losses


# ------------------------------------------------------------------------------------------------ the loss kernel
def mde_loss_ref(y, m):
    """tdg_mde_loss in float64: y [n,hw] f32 values, m [n] as stored (widened).  Returns (mean_out f32, loss f32, sign [n])."""
    mean = np.asarray(y, np.float64).mean(axis=1)
    d = np.asarray(m, np.float64) - mean
    return mean.astype(np.float32), np.float32(np.abs(d).sum() / len(d)), np.sign(d)


# ------------------------------------------------------------------------------------------------ TF-1.x bilinear resize
def resize_tf1(a, out_h, out_w):
    """tf.image.resize_images of TF 1.x on [N,H,W,C] in float64 NumPy: bilinear, align_corners=False, no half-pixel centres:
    src = dst * in / out; the upper neighbour clamped to the last row / column."""
    a = np.asarray(a, np.float64)
    n, h, w, c = a.shape
    out = np.empty((n, out_h, out_w, c))
    for r in range(out_h):
        sy = r * h / out_h
        y0 = min(int(np.floor(sy)), h - 1)
        y1, fy = min(y0 + 1, h - 1), sy - y0
        for q in range(out_w):
            sx = q * w / out_w
            x0 = min(int(np.floor(sx)), w - 1)
            x1, fx = min(x0 + 1, w - 1), sx - x0
            top = a[:, y0, x0] * (1 - fx) + a[:, y0, x1] * fx
            bot = a[:, y1, x0] * (1 - fx) + a[:, y1, x1] * fx
            out[:, r, q] = top * (1 - fy) + bot * fy
    return out


# ------------------------------------------------------------------------------------------------ the parity test's inputs
PARITY_SEED, PARITY_B, PARITY_STEPS = 0, 4, 3
HP = dict(optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999)


def initial_variables(plugin_cls, seed):
    """The variables a fresh replica of `plugin_cls` starts from at session seed `seed`, drawn on the host exactly as
    SeqNet.init_variables draws them (layer by layer, weights then bias, one generator)."""
    from types import SimpleNamespace
    from conftest import pkg
    net = plugin_cls.build_graph(SimpleNamespace(batch_size=PARITY_B))
    store = {}
    for l in net.layers:
        store[net.var_name(l, 'weights')] = torch.empty(l.filter_shape)
        store[net.var_name(l, 'bias')] = torch.empty((l.out_size,))
    pkg('engine').init_weights(store, net, net.layers, torch.Generator().manual_seed(seed))
    return {k: v.numpy() for k, v in store.items()}


class Originals:
    """(x_full, y_full) batches whose per-image depth means lie in [0.05, 0.2] or [0.8, 0.95]: the estimator starts near
    m = 0.5, so every |mean_i - m_i| stays far from the kink of the absolute value."""

    def __init__(self, B, n, seed=0, device='cpu'):
        g = torch.Generator().manual_seed(seed)
        self.x, self.y = [], []
        for _ in range(n):
            low = torch.rand(B, 1, 1, 1, generator=g) * 0.11 + 0.07
            level = torch.where(torch.rand(B, 1, 1, 1, generator=g) < 0.5, low, 1.0 - low)
            self.x.append(torch.rand(B, FULL[0], FULL[1], 3, generator=g).to(device))
            self.y.append((level + (torch.rand(B, FULL[0], FULL[1], 1, generator=g) - 0.5) * 0.04).to(device))
        self.i = 0

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.x[k], self.y[k]


def trajectory(variables, batches, dtype=torch.float64):
    """Per step: (the variables before it, its loss, its gradients, m, the mean depths), then the variables after the last step."""
    steps, v = [], variables
    for t in range(1, len(batches) + 1):
        l, g, m, means = oracle_grads(v, *batches[t - 1], dtype=dtype)
        steps.append((v, l, g, m, means))
        v, _ = adam_steps(variables, batches[:t], HP['lr'], HP['beta1'], HP['beta2'], dtype=dtype)
    return steps, v
