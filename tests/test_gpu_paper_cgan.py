"""paper_cgan on the GPU (hem/models/paper_cgan.py): the new kernels of tdg_cgan.hip against float64 NumPy, and the model
against a float64 torch-autograd restatement of the reference (defined here), plus graph replay, determinism, bf16 runs,
checkpoint / resume and train.py end to end."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
from oracle.torch_ref import conv2d_valid, conv2d_transpose_valid, conv2d_same, lrelu

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TOL = {0: 2e-5, 1: 2e-2}                       # f32, bf16 (relative to the value scale)


def K():
    return pkg('kernels')


def L():
    return pkg('_lib')


def close(a, b, tol, what=''):
    """Max-norm check; inf / NaN entries of the reference must be matched exactly."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    odd = ~np.isfinite(b)
    assert np.array_equal(a[odd], b[odd], equal_nan=True), '%s: non-finite entries differ' % what
    a, b = a[~odd], b[~odd]
    err = np.max(np.abs(a - b)) if a.size else 0.0
    assert err <= tol * max(1.0, np.max(np.abs(b)) if b.size else 0.0), '%s: max err %g' % (what, err)


_KEEP = []


def dev(a, dtype=torch.float32):
    """A device copy that stays alive: the kernels receive raw pointers, and a freed temporary's block could be handed to
    the next allocation before the launch that reads it."""
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)
    _KEEP.append(t)
    del _KEEP[:-64]
    return t


def rnd(dt_code, *shape, seed=0, lo=-1.0, hi=1.0):
    """Values exactly representable in the compute dtype (the kernels read them as stored)."""
    a = np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)
    if dt_code == 1:
        a = torch.tensor(a).bfloat16().float().numpy()
    return a


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('version', [0, 1, 2])
def test_prep_kernel(dt, version):
    B = 3
    y = np.random.default_rng(1).uniform(0.01, 0.99, (B, 65, 65)).astype(np.float32)
    depth = K().Act(2 * B, 29, 29, 2 if version == 2 else 1, dt, DEV)
    cs = depth.cs
    gx, rx = K().Act(B, 65, 65, 4, dt, DEV), K().Act(B, 65, 65, 4, dt, DEV)
    ybar, crop = torch.zeros(B, device=DEV), torch.zeros(B, 29, 29, device=DEV)
    mp2 = version == 2
    L().call('tdg_cgan_prep', dt, K().ptr(dev(y)), B, version, depth.ptr(0), cs, depth.ptr(B) if mp2 else None, K().ptr(ybar),
             K().ptr(crop), gx.window(3, 1).ptr(0) if mp2 else None, gx.cs, rx.window(3, 1).ptr(0) if mp2 else None, rx.cs,
             K().stream())
    c = 10.0 * y[:, 17:46, 17:46].astype(np.float64)
    m = c.mean(axis=(1, 2))
    close(crop.cpu().numpy(), c, 1e-6, 'crop')
    close(ybar.cpu().numpy(), m, 1e-6, 'ybar')
    d = depth.get()
    real = c if version == 0 else c - m[:, None, None]
    close(d[:B, ..., 0], real, TOL[dt], 'depth real')
    assert np.all(d[B:, ..., 0] == 0)                           # the fake half's g channel is the head's
    if mp2:
        close(d[:, ..., 1], np.concatenate([m, m])[:, None, None] * np.ones((1, 29, 29)), TOL[dt], 'y_bar channel')
        assert np.all(gx.get()[..., 3] == 1.0)
        close(rx.get()[..., 3], m[:, None, None] * np.ones((1, 65, 65)), TOL[dt], 'rgb y_bar channel')
    else:
        assert np.all(gx.get() == 0) and np.all(rx.get() == 0)


@pytest.mark.parametrize('dt', [0, 1])
def test_head_forward_and_backward(dt):
    B, C = 3, 128
    cat = K().Act(B, 31, 31, C, dt, DEV).set(rnd(dt, B, 31, 31, C, seed=2))
    catv = cat.get().astype(np.float64)
    w = rnd(0, C, seed=3)
    b = np.array([0.3], np.float32)
    ybar = np.array([1.0, 2.0, 3.0], np.float32)
    yhat = torch.zeros(B, 29, 29, device=DEV)
    fake = K().Act(B, 29, 29, 1, dt, DEV)
    L().call('tdg_cgan_head_fwd', dt, cat.ptr(), B, 31, C, cat.cs, 29, K().ptr(dev(w)), K().ptr(dev(b)), K().ptr(dev(ybar)),
             K().ptr(yhat), fake.ptr(), fake.cs, K().stream())
    g = (catv @ w.astype(np.float64) + b[0])[:, :29, :29]          # the TOP-LEFT 29x29 of the 31x31 head output
    close(yhat.cpu().numpy(), g + ybar[:, None, None], 1e-5, 'y_hat')
    close(fake.get()[..., 0], g, TOL[dt], 'fake depth channel')
    # backward
    dfake = K().Act(B, 29, 29, 1, dt, DEV).set(rnd(dt, B, 29, 29, 1, seed=4))
    delta = dfake.get()[..., 0].astype(np.float64)
    dcat = K().Act(B, 31, 31, C, dt, DEV).set(np.full((B, 31, 31, C), 7.0, np.float32))      # must be overwritten everywhere
    dw, db = torch.zeros(C, device=DEV), torch.zeros(1, device=DEV)
    ws = torch.zeros(B * (C + 1), device=DEV)
    L().call('tdg_cgan_head_bwd', dt, dfake.ptr(), dfake.cs, cat.ptr(), B, 31, C, cat.cs, 29, K().ptr(dev(w)), K().MASK_LRELU, 0.2,
             dcat.ptr(), K().ptr(dw), K().ptr(db), K().ptr(ws), ws.numel() * 4, K().stream())
    full = np.zeros((B, 31, 31))
    full[:, :29, :29] = delta
    mask = np.where(catv > 0, 1.0, 0.2)
    ref = full[..., None] * w[None, None, None, :] * mask
    got = dcat.get()
    close(got, ref, TOL[dt], 'dcat')
    assert np.all(got[:, 29:, :, :] == 0) and np.all(got[:, :, 29:, :] == 0)
    close(dw.cpu().numpy(), np.einsum('bhw,bhwc->c', full, catv), TOL[dt] * 10, 'dW')
    close(db.cpu().numpy(), [full.sum()], TOL[dt] * 10, 'db')


@pytest.mark.parametrize('dt', [0, 1])
def test_wgan_loss_and_seeds(dt):
    B, cs = 5, 8
    z = rnd(dt, 2 * B, seed=5, lo=-3, hi=3)
    logits = K().Act(2 * B, 1, 1, 1, dt, DEV).set(z.reshape(2 * B, 1, 1, 1))
    s = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    sr, sf = s[:B], s[B:]
    for mode in (0, 1, 2):
        seed = K().Act(2 * B, 1, 1, 1, dt, DEV)
        scal = torch.zeros(4, device=DEV)
        L().call('tdg_cgan_wgan_loss', dt, logits.ptr(), B, cs, mode, seed.ptr(), K().ptr(scal), K().stream())
        close(scal.cpu().numpy(), [-sf.mean(), sf.mean(), sr.mean(), sf.mean() - sr.mean()], 1e-5, 'wgan losses')
        got = seed.get().ravel()
        if mode == 1:
            ref = np.concatenate([-sr * (1 - sr), sf * (1 - sf)]) / B
        elif mode == 2:
            ref = np.concatenate([np.zeros(B), -sf * (1 - sf)]) / B
        else:
            ref = np.zeros(2 * B)
        close(got, ref, TOL[dt], 'seeds mode %d' % mode)


def eigen_ref(y, p, counts):
    from test_host_paper_cgan import eigen_metrics
    out = eigen_metrics(y.astype(np.float64), p.astype(np.float64), counts)
    return np.array([out[k] for k in pkg('models.paper.paper_cgan').METRIC_KEYS])


def test_metrics_kernel_streaming_and_zero_prediction():
    n, hw = 6, 841
    rng = np.random.default_rng(6)
    y = rng.uniform(0.1, 10, (n, hw)).astype(np.float32)
    g = (y * rng.uniform(0.6, 1.6, (n, hw))).astype(np.float32) - 1.0
    off = rng.uniform(0.5, 1.5, n).astype(np.float32)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, device=DEV)
    ws = torch.zeros(L().load().tdg_cgan_metrics_workspace_bytes(), dtype=torch.uint8, device=DEV)
    ref_counts = [0, 0, 0, 0]

    def run(pred, offset):
        L().call('tdg_cgan_metrics', K().ptr(dev(y)), K().ptr(dev(pred) if pred is not None else None),
                 K().ptr(dev(offset) if offset is not None else None), n, hw, K().ptr(counts), K().ptr(out), K().ptr(ws), ws.numel(),
                 K().stream())
        return out.cpu().numpy()

    got = run(g, off)
    ref = eigen_ref(y, g + off[:, None], ref_counts)
    close(got, ref, 1e-4, 'metrics 1')
    got = run(None, off)                                         # y_0 = y_bar: a second evaluation, counts keep running
    ref = eigen_ref(y, np.broadcast_to(off[:, None], y.shape), ref_counts)
    close(got, ref, 1e-4, 'metrics 2')
    assert counts.cpu().tolist() == ref_counts and ref_counts[3] == 2 * n * hw
    got = run(None, None)                                        # baseline's y_0 = 0: inf / NaN exactly as the formulas
    ref = eigen_ref(y, np.zeros_like(y), ref_counts)
    assert np.isinf(got[0]) and np.isinf(got[1]) and np.isinf(ref[0])
    assert np.isnan(got[4]) == np.isnan(ref[4])
    close(got[5:], ref[5:], 1e-6, 'running thresholds')


# ------------------------------------------------------------------------------------------------ the float64 oracle
def oracle_G(P, x):
    def W(n):
        return P['generator/' + n]
    h = x
    e = []
    for k in range(1, 5):
        h = torch.relu(conv2d_valid(h, W('encoder/vars/e%d/weights' % k), 2) + W('encoder/vars/e%d/bias' % k))
        e.append(h)
    y = e[3]
    for i, hw in ((1, 5), (2, 14), (3, 31)):
        y = lrelu(conv2d_transpose_valid(y, W('decoder/vars/d%d/weights' % i), (hw, hw)) + W('decoder/vars/d%d/bias' % i), 0.2)
        y = torch.cat([y, e[3 - i]], dim=-1)
    y = conv2d_same(y, W('decoder/vars/d4/weights'), 1) + W('decoder/vars/d4/bias')
    return y[:, :29, :29, :]


def oracle_D(P, x, y):
    def W(n):
        return P['discriminator/' + n]
    h1 = x
    for k in range(1, 5):
        h1 = lrelu(conv2d_valid(h1, W('rgb_path/vars/hx%d/weights' % k), 2) + W('rgb_path/vars/hx%d/bias' % k), 0.2)
    h2 = y
    for k in range(1, 4):
        h2 = lrelu(conv2d_valid(h2, W('depth_path/vars/hy%d/weights' % k), 2) + W('depth_path/vars/hy%d/bias' % k), 0.2)
    h = torch.cat([h1, h2], dim=-1)
    h = lrelu(conv2d_same(h, W('combined_path/vars/h1/weights'), 1) + W('combined_path/vars/h1/bias'), 0.2)
    h = lrelu(conv2d_same(h, W('combined_path/vars/h2/weights'), 1) + W('combined_path/vars/h2/bias'), 0.2)
    return conv2d_same(h, W('combined_path/vars/h3/weights'), 1) + W('combined_path/vars/h3/bias')


def oracle_forward(P, x01, y01, version, wgan):
    """hem/models/paper_cgan.py:83-149 and :390-412 for one batch; returns (losses, g_loss, d_total, y_hat)."""
    B = x01.shape[0]
    y = 10.0 * y01[:, 17:46, 17:46, :]
    ybar = y.mean(dim=(1, 2, 3), keepdim=True)
    gin = torch.cat([x01, torch.ones_like(x01[..., :1])], -1) if version == 'mean_provided2' else x01
    g = oracle_G(P, gin)
    if version == 'baseline':
        y_hat, real, fake, xr = g, y, g, x01
    else:
        y_hat = g + ybar
        real, fake, xr = y - ybar, y_hat - ybar, x01
        if version == 'mean_provided2':
            real = torch.cat([real, torch.ones_like(real) * ybar], -1)
            fake = torch.cat([fake, torch.ones_like(fake) * ybar], -1)
            xr = torch.cat([x01, torch.ones(B, 65, 65, 1, dtype=x01.dtype) * ybar], -1)
    zf, zr = oracle_D(P, xr, fake), oracle_D(P, xr, real)
    sp = torch.nn.functional.softplus
    if wgan:
        sf, sr = torch.sigmoid(zf).mean(), torch.sigmoid(zr).mean()
        g_fake, d_fake, d_real = -sf, sf, sr
        d_total = d_fake - d_real
        losses = {'g_fake': g_fake, 'd_fake': d_fake, 'd_fake_1': d_real, 'd_total': d_total}
    else:
        g_fake, d_real, d_fake = sp(-zf).mean(), sp(-zr).mean(), sp(zf).mean()
        d_total = d_real + d_fake
        losses = {'g_fake': g_fake, 'd_fake': d_fake, 'd_real': d_real, 'd_total': d_total}
    return losses, g_fake, d_total, y_hat


def oracle_grads(variables, batch, version, wgan, which):
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in variables.items()}
    x, y = (torch.tensor(t.cpu().numpy(), dtype=torch.float64) for t in batch)
    losses, g_fake, d_total, y_hat = oracle_forward(P, x, y, version, wgan)
    target = d_total if which == 'd' else g_fake
    names = [k for k in P if k.startswith('discriminator/' if which == 'd' else 'generator/')]
    grads = torch.autograd.grad(target, [P[k] for k in names])
    return ({k: float(v.detach()) for k, v in losses.items()}, {k: g.numpy() for k, g in zip(names, grads)}, y_hat.detach().numpy())


class Batches:
    def __init__(self, B, n, seed=0, device=DEV):
        g = torch.Generator().manual_seed(seed)
        self.x = [torch.rand(B, 65, 65, 3, generator=g).to(device) for _ in range(n)]
        self.y = [(torch.rand(B, 65, 65, 1, generator=g) * 0.98 + 0.01).to(device) for _ in range(n)]
        self.i = 0

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.x[k], self.y[k]


DEFAULT_HP = dict(g_lr=1e-3, d_lr=1e-3, g_beta1=0.9, d_beta1=0.9, g_beta2=0.999, d_beta2=0.999)
# Small, distinct rates and betas: the sigmoid critic does not saturate within one train() (at 1e-3 its logits reach
# several hundred in a few steps, and every sigmoid-WGAN seed s(1-s)/B is then exactly 0 in f32), and a swapped
# optimizer, rate or beta changes the update
SMALL_HP = dict(g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)


def make(version, training, B=4, dtype=0, seed=0, use_graphs=True, n_batches=8, data_seed=None, hp=DEFAULT_HP, **kw):
    rt = pkg('runtime')
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version=version, training_version=training, seed=seed,
                           use_graphs=use_graphs, **dict(hp, **kw))
    sess = rt.Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    return pkg('models.paper.paper_cgan').paper_cgan(Batches(B, n_batches, seed if data_seed is None else data_seed), args, sess)


def grads_close(got, ref, what):
    """Every gradient of one store within 1e-3 of the store's largest reference entry -- which must itself be far above that
    tolerance's floor, so that an all-zero (saturated) comparison fails instead of passing."""
    scale = max(float(np.max(np.abs(r))) for r in ref.values())
    assert scale > 1e-4, '%s: reference gradients vanish (max %g): nothing would be compared' % (what, scale)
    for k, r in ref.items():
        close(got[k], r, 1e-3 * scale, '%s %s' % (what, k))
        assert np.any(r != 0), '%s %s: the reference gradient is identically zero' % (what, k)


@pytest.mark.parametrize('training', ['gan', 'wgan'])
@pytest.mark.parametrize('version', ['baseline', 'mean_adjusted', 'mean_provided2'])
def test_model_parity_f32(version, training):
    m = make(version, training, use_graphs=False, hp=SMALL_HP)
    wgan = training == 'wgan'
    # infer() against the oracle's y_hat on a fresh batch
    b0 = m.x_y.next_batch()
    _, _, yh = oracle_grads(m.variables(), b0, version, wgan, 'g')
    close(m.infer(b0)[..., 0].cpu().numpy(), yh[..., 0], 1e-3, 'infer')
    # one D step: every D gradient
    v0, b1 = m.variables(), m.x_y.next_batch()
    _, ref_d, _ = oracle_grads(v0, b1, version, wgan, 'd')
    m.d_step(b1)
    grads_close(m.gradients(), ref_d, 'D step')
    # a G step and its loss fetch on the next batch: every G gradient and the four losses (before the G update).  Right
    # after one D step, so that the wgan seeds s(1-s)/B are not zero (the full five-D-step schedule: test_train_parity_f32)
    v1, b2 = m.variables(), m.x_y.next_batch()
    ref_l, ref_g, _ = oracle_grads(v1, b2, version, wgan, 'g')
    m.g_step(b2)
    grads_close(m.gradients(), ref_g, 'G step')
    got = m._losses()
    assert list(got) == list(ref_l)
    for k in ref_l:
        close(got[k], ref_l[k], 1e-3, 'loss ' + k)
    if wgan:
        assert 1e-3 < ref_l['d_fake'] < 1 - 1e-3 and 1e-3 < ref_l['d_fake_1'] < 1 - 1e-3, ref_l      # not saturated


def adam_ref(P, G, slots, name, lr, b1, b2, eps=1e-8):
    """tf.train.AdamOptimizer, float64."""
    m, v, t = slots.setdefault(name, [0.0, 0.0, 0])
    t += 1
    m = b1 * m + (1 - b1) * G
    v = b2 * v + (1 - b2) * G * G
    slots[name] = [m, v, t]
    return P - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps)


def rmsprop_ref(P, G, slots, name, lr, decay=0.9, momentum=0.0, eps=1e-10):
    """tf.train.RMSPropOptimizer, float64: the rms slot starts at one."""
    ms, mom = slots.setdefault(name, [1.0, 0.0])
    ms = decay * ms + (1 - decay) * G * G
    mom = momentum * mom + lr * G / np.sqrt(ms + eps)
    slots[name] = [ms, mom]
    return P - mom


def oracle_train(v0, batches, version, wgan, hp):
    """hem/models/paper_cgan.py:60-69 + :200-209 in float64: gan -- one Adam(d_lr, d_beta1, d_beta2) D step on batch 0, then
    one Adam(g_lr, g_beta1, g_beta2) G step on batch 1; wgan -- five default-beta Adam(d_lr) D steps on batches 0..4, then one
    RMSProp(g_lr) G step on batch 5.  Returns the variables and, per variable, where some step's gradient was too close to zero
    for its Adam direction to be defined at f32 precision."""
    V = {k: v.astype(np.float64) for k, v in v0.items()}
    slots, fuzzy = {}, {k: np.zeros(v.shape, bool) for k, v in V.items()}
    n_d = 5 if wgan else 1
    for i in range(n_d + 1):
        which = 'd' if i < n_d else 'g'
        _, grads, _ = oracle_grads(V, batches[i], version, wgan, which)
        for k, G in grads.items():
            if which == 'd' or not wgan:
                fuzzy[k] |= (G != 0) & (np.abs(G) <= 1e-4 * np.max(np.abs(G)))     # (exact zeros: no step in either)
            if which == 'd':
                b1, b2 = (0.9, 0.999) if wgan else (hp['d_beta1'], hp['d_beta2'])
                V[k] = adam_ref(V[k], G, slots, k, hp['d_lr'], b1, b2)
            elif wgan:
                V[k] = rmsprop_ref(V[k], G, slots, k, hp['g_lr'])
            else:
                V[k] = adam_ref(V[k], G, slots, k, hp['g_lr'], hp['g_beta1'], hp['g_beta2'])
    return V, fuzzy


@pytest.mark.parametrize('training', ['gan', 'wgan'])
@pytest.mark.parametrize('version', ['baseline', 'mean_provided2'])
def test_train_parity_f32(version, training):
    """Variables after one full train() -- its batch order, optimizers, rates and betas -- against the float64 oracle.
    Compared as updates: Adam moves by about lr per step whatever the gradient's size, so where the gradients define its
    direction the update must match to 2 % of lr (99.9 % of the entries; every one within lr / 2), and stay within the
    steps' reach elsewhere; RMSProp's update is linear in
    the gradient and must match to 1e-3 of its largest entry, beyond the f32 rounding of the stored variable.  And the
    variables within 1e-3."""
    hp, wgan = SMALL_HP, training == 'wgan'
    m = make(version, training, use_graphs=False, hp=hp)
    v0 = m.variables()
    batches = [(m.x_y.x[i], m.x_y.y[i]) for i in range(6)]
    m.train()
    v1 = m.variables()
    ref, fuzzy = oracle_train(v0, batches, version, wgan, hp)
    steps = {'d': 5 if wgan else 1, 'g': 1}
    for store in ('generator/', 'discriminator/'):
        keys = [k for k in v0 if k.startswith(store)]
        d_ref = {k: ref[k] - v0[k] for k in keys}
        d_got = {k: v1[k].astype(np.float64) - v0[k] for k in keys}
        if store == 'generator/' and wgan:
            scale = max(float(np.max(np.abs(d_ref[k]))) for k in keys)
            assert scale > 1e-9, 'RMSProp update vanishes'
            for k in keys:                 # (+ one f32 rounding of the stored variable: the update is far below its ulp)
                excess = np.abs(d_got[k] - d_ref[k]) - np.spacing(np.abs(v1[k])).astype(np.float64)
                assert np.max(excess) <= 1e-3 * scale, 'update %s: max err %g (largest update %g)' % (k, np.max(excess), scale)
        else:
            lr = hp['d_lr'] if store == 'discriminator/' else hp['g_lr']
            n = steps[store[0]]
            sharp = np.concatenate([~fuzzy[k].ravel() for k in keys])
            assert sharp.mean() > 0.9, '%s: %.3f of the gradients are near (not at) zero' % (store, 1 - sharp.mean())
            assert max(float(np.max(np.abs(d_ref[k]))) for k in keys) > 0.5 * lr, '%s: no Adam step taken' % store
            err = np.concatenate([np.abs(d_got[k] - d_ref[k]).ravel() for k in keys])
            e_sharp = err[sharp]
            # a swapped optimizer, rate or schedule is off by about lr on most entries; f32 leaves a few isolated entries whose
            # step direction sits at a kink or near-zero gradient of some step (observed: one in 2e5 at 0.12 lr)
            assert np.quantile(e_sharp, 0.999) <= 0.02 * lr, '%s: 99.9 %% quantile of the update error %g (lr %g)' % (
                store, np.quantile(e_sharp, 0.999), lr)
            assert np.max(e_sharp) <= 0.5 * lr, '%s: max update error %g (lr %g)' % (store, np.max(e_sharp), lr)
            assert np.max(err) <= 2.0 * n * lr + 1e-12, '%s: an update out of the steps\' reach' % store
        for k in keys:
            close(v1[k], ref[k], 1e-3, 'variable ' + k)


@pytest.mark.parametrize('training', ['gan', 'wgan'])
def test_graph_replay_matches_eager_bit_for_bit(training):
    a, b = make('mean_adjusted', training, use_graphs=True), make('mean_adjusted', training, use_graphs=False)
    for _ in range(3):
        la, lb = a.train(), b.train()
        assert la == lb
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


def test_two_fresh_models_are_bit_equal():
    a, b = make('mean_provided2', 'gan', seed=3), make('mean_provided2', 'gan', seed=3)
    for _ in range(3):
        assert a.train() == b.train()
    ma, mb = a.metrics(), b.metrics()
    for k in ma:
        assert np.array_equal(list(ma[k].values()), list(mb[k].values()), equal_nan=True)


@pytest.mark.parametrize('training', ['gan', 'wgan'])
@pytest.mark.parametrize('version', ['baseline', 'mean_adjusted'])
def test_bf16_runs_finite(version, training):
    m = make(version, training, B=64, dtype=1, n_batches=4)
    for _ in range(10):
        losses = m.train()
        assert all(np.isfinite(v) for v in losses.values()), losses
        met = m.metrics()
        for k in ('threshold1', 'threshold2', 'threshold3'):
            assert 0.0 <= met['metrics_y_hat'][k] <= 1.0
        if version == 'mean_adjusted':                       # y_0 = y_bar > 0: every metric finite
            assert all(np.isfinite(v) for v in met['metrics_y_0'].values()), met
    assert np.all(np.isfinite(m.infer(m.x_y.next_batch()).cpu().numpy()))


def test_metrics_of_the_last_fetch_stream():
    m = make('mean_adjusted', 'gan')
    m.train()
    crop, yhat, ybar = m.crop.cpu().numpy(), m.yhat.cpu().numpy(), m.ybar.cpu().numpy()
    m.infer(m.x_y.next_batch())                                   # infer() does not touch the fetch's buffers
    counts = [0, 0, 0, 0]
    keys = pkg('models.paper.paper_cgan').METRIC_KEYS
    got = m.metrics()
    close([got['metrics_y_hat'][k] for k in keys], eigen_ref(crop, yhat, counts), 1e-4, 'y_hat set')
    got = m.metrics()                                             # a second evaluation of the same fetch: totals double
    ref = eigen_ref(crop, yhat, counts)
    close([got['metrics_y_hat'][k] for k in keys], ref, 1e-4, 'y_hat set, second evaluation')
    c0 = [0, 0, 0, 0]
    eigen_ref(crop, np.broadcast_to(ybar[:, None, None], crop.shape), c0)
    ref0 = eigen_ref(crop, np.broadcast_to(ybar[:, None, None], crop.shape), c0)
    close([got['metrics_y_0'][k] for k in keys], ref0, 1e-4, 'y_0 set')


def test_wgan_clip_clamps_both_nets():
    m = make('baseline', 'wgan', wgan_clip=0.01)
    m.train()
    # every D step clamps D before it runs and the G step clamps G: after one more Adam / RMSProp step each
    # variable lies within the clip range plus one update
    for k, v in m.variables().items():
        assert np.max(np.abs(v)) <= 0.01 + 5e-3, k


@pytest.mark.parametrize('training', ['gan', 'wgan'])
def test_checkpoint_resume_is_bit_identical(tmp_path, training):
    """Checkpoint after one train(), resume into a model with other initial variables and the SAME data stream, one more
    train(): bit-identical to the uninterrupted run, in a state whose gradients (and Adam / RMSProp slots) are non-zero."""
    ckpt = pkg('checkpoint')
    a = make('mean_provided2', training, hp=SMALL_HP)
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    pos = a.x_y.i
    la = a.train()
    for store in ('generator/', 'discriminator/'):
        assert max(float(np.max(np.abs(v))) for k, v in a.gradients().items() if k.startswith(store)) > 1e-6, store
    b = make('mean_provided2', training, seed=11, data_seed=0, hp=SMALL_HP)
    assert any(not np.array_equal(b.variables()[k], v) for k, v in a.variables().items())
    ckpt.restore(path, b, b.sess)
    b.x_y.i = pos
    lb = b.train()
    assert la == lb
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


def test_train_cli_synthetic(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_cgan', '--dataset', 'synthetic',
                        '--batch_size', '8', '--epoch_size', '2', '--epochs', '1', '--model_version', 'mean_adjusted',
                        '--dir', str(tmp_path / 'ws')], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = p.stdout + p.stderr
    assert '2/2' in out.replace(' ', ''), out[-1500:]
    assert os.path.exists(str(tmp_path / 'ws' / 'checkpoint-1.npz'))
