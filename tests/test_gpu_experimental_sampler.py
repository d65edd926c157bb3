"""experimental_sampler on the GPU (hem/models/experimental_sampler.py) at full widths (the architecture is fixed), B = 4, the
estimator a narrow copy (tests/_mde_ref.NARROW through its WIDTHS override): both gradient sets of ONE forward pass, the six
losses and infer() against the float64 torch-autograd oracle of tests/_xsamp_ref.py with the noise injected; one train()
against the oracle plus a float64 Adam; the estimator untouched by train(); the three summary sets; sample(); graph replay,
determinism, checkpoint / resume; a bf16 run; the driver experimental.py end to end on synthetic data."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _mde_ref as M
import _xsamp_ref as R
from test_gpu_paper_cgan import close, grads_close, DEV

pytestmark = pytest.mark.gpu
HP = dict(optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, decay=0.9, momentum=0.01, centered=False)
KINK_MARGIN = 5.0
# The parity batch: the first data seed whose batch 0 keeps, at the variables of session seed 0 and the noise of draws(),
# every (l)relu input of the generator's small layers (at most 25 B positions per channel: e4, e5, d1) 1e-6 from zero and those
# of the critic's small layers (hx4, hx5, hy3, hy4, h1 .. h5) KINK_MARGIN rms float32 deviations from zero, on D(X, y) and on
# D(X, g) -- properties of the ORACLE alone (tests/_xsamp_ref.nearest_kink / critic_kink_margin), asserted before anything is
# compared, for the reasons test_gpu_paper_sampler.py::test_model_parity_f32 records: at a kink a float32 evaluation may take
# either side, and the other side moves a small layer's gradient by that position's whole contribution.  Seed 0 puts an input of
# a small generator layer 9.1e-7 from zero; seed 1 keeps them 1.4e-6 away and the critic's 5.95 deviations away.
PARITY_DATA_SEED = 1


def plugin():
    return pkg('models.experimental.experimental_sampler').experimental_sampler


def narrow_estimator():
    mde = pkg('models.estimator.mean_depth_estimator').mean_depth_estimator
    return type('narrow_estimator', (mde,), {'WIDTHS': M.NARROW})


def make(B=4, dtype=0, seed=0, use_graphs=True, n_batches=4, data_seed=0):
    args = SimpleNamespace(batch_size=B, n_gpus=1, seed=seed, use_graphs=use_graphs, **HP)
    sess = pkg('runtime').Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    data = R.Batches(B, n_batches, data_seed, DEV)
    return plugin()(data, args, sess, estimator=narrow_estimator()(data, args, sess))


def draws(B, k, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1, (B, R.SRC, R.SRC, 1)).astype(np.float32) for _ in range(k)]


def split(variables):
    est = {k: v for k, v in variables.items() if k.startswith('model/')}
    return est, {k: v for k, v in variables.items() if not k.startswith('model/')}


def oracle_inputs(m, batch, **rows):
    est, _ = split(m.variables())
    return R.assemble(batch, R.estimator_m(est, batch), **rows)


def same(a, b):
    return list(a) == list(b) and np.array_equal(list(a.values()), list(b.values()), equal_nan=True)


# ------------------------------------------------------------------------------------------------ parity with the oracle
def test_model_parity_f32():
    """After the gradient body of one train(), before the apply: every D gradient, every G gradient (grads_close: 1e-3 of the
    store's largest entry, which must exceed 1e-4) and the six losses (1e-3) against the float64 oracle -- both gradient sets
    from the one forward pass, at the variables before either update; then infer() against the oracle's (g + 1) / 2."""
    B = 4
    m = make(B=B, use_graphs=False, data_seed=PARITY_DATA_SEED)
    u = draws(B, 2)
    m.sess.inject = {'noise_x': [a.copy() for a in u]}
    b0 = m.x_y.batch(0)
    v0 = m.variables()
    X, y = oracle_inputs(m, b0)
    noise = R.noise_channel(u[0])
    kink = R.nearest_kink(v0, X, noise, max_positions=25 * B)
    assert kink > 1e-6, 'the batch puts a small generator layer %g from a kink: choose other data' % kink
    margin = R.critic_kink_margin(v0, X, y, noise, max_positions=25 * B)
    assert margin >= KINK_MARGIN, 'the batch puts a small critic layer %.2f deviations from a kink: choose other data' % margin
    losses, dg, gg, g = R.oracle_grads(v0, X, y, noise)
    m._stage(m._batch(m.x_y.next_batch()))
    m._grads()
    got = m.gradients()
    grads_close({k: v for k, v in got.items() if k.startswith('discriminator/')}, dg, 'D gradients')
    grads_close({k: v for k, v in got.items() if k.startswith('generator/')}, gg, 'G gradients')
    assert all(not np.any(v) for k, v in got.items() if k.startswith('model/'))           # nothing flows back into the estimator
    have = m._losses()
    assert list(have) == list(R.LOSS_KEYS) == list(losses)
    for k in losses:
        close(have[k], losses[k], 1e-3, 'loss ' + k)
    close(m.g32.cpu().numpy(), g[..., 0], 1e-3, 'g')
    close(m.m.cpu().numpy()[:B], R.estimator_m(split(v0)[0], b0), 1e-5, 'm')
    # infer(): the next draw, the same batch
    ref = R.oracle_grads(v0, X, y, R.noise_channel(u[1]))[3]
    out = m.infer(b0)
    assert tuple(out.shape) == (B, 32, 32, 1) and float(out.min()) >= 0 and float(out.max()) <= 1
    close(out.cpu().numpy(), (ref + 1) / 2, 1e-3, 'infer')
    assert not m.sess.inject['noise_x']                                                  # one draw per generator pass


def test_train_parity_f32():
    """Variables after one train() -- ONE batch, both Adam steps from the gradients of the one forward pass at the variables
    before either -- against the float64 oracle, by the rule of tests/test_gpu_paper_cgan.py::test_train_parity_f32: where the
    gradients define Adam's direction the update matches to 2 % of lr on 99.9 % of the entries and to lr / 2 on all; every update
    stays within the step's reach.  global_step advances by 2; the estimator's variables do not move."""
    B, lr = 4, HP['lr']
    m = make(B=B, use_graphs=False, data_seed=PARITY_DATA_SEED)
    u = draws(B, 1)
    m.sess.inject = {'noise_x': [a.copy() for a in u]}
    v0 = m.variables()
    X, y = oracle_inputs(m, m.x_y.batch(0))
    _, dg, gg, _ = R.oracle_grads(v0, X, y, R.noise_channel(u[0]))
    m.train()
    assert m.sess.global_step == 2 and m.g_opt.t == 1 and m.d_opt.t == 1
    v1 = m.variables()
    slots = {}
    for store, grads in (('generator/', gg), ('discriminator/', dg)):
        V = {k: R.adam_ref(v0[k].astype(np.float64), G, slots, k, lr, HP['beta1'], HP['beta2']) for k, G in grads.items()}
        fuzzy = {k: (G != 0) & (np.abs(G) <= 1e-4 * np.max(np.abs(G))) for k, G in grads.items()}
        keys = list(grads)
        sharp = np.concatenate([~fuzzy[k].ravel() for k in keys])
        err = np.concatenate([np.abs((v1[k].astype(np.float64) - v0[k]) - (V[k] - v0[k])).ravel() for k in keys])
        assert sharp.mean() > 0.9 and max(float(np.max(np.abs(V[k] - v0[k]))) for k in keys) > 0.5 * lr
        print('%s update error 99.9 %% quantile %.3g lr, max %.3g lr' % (store, np.quantile(err[sharp], 0.999) / lr, np.max(err[sharp]) / lr))
        assert np.quantile(err[sharp], 0.999) <= 0.02 * lr and np.max(err[sharp]) <= 0.5 * lr
        assert np.max(err) <= 2.0 * lr + 1e-12
        for k in keys:
            close(v1[k], V[k], 1e-3, 'variable ' + k)
    assert all(np.array_equal(v0[k], v1[k]) for k in v0 if k.startswith('model/'))


# ------------------------------------------------------------------------------------------------ the estimator
def test_train_leaves_the_estimator_bit_identical():
    """The estimator's variables and its optimizer's slots and step count before and after train(), with and without graph
    replay; its own train() still moves them, and the sampler then reads the new m."""
    for use_graphs in (False, True):
        m = make(use_graphs=use_graphs)
        est = m.estimator
        est.train()                                                   # non-trivial slots
        before = {k: v.copy() for k, v in split(m.variables())[0].items()}
        slots = {k: t.clone() for k, t in est.opt.state_tensors().items()}
        t0, m0 = est.opt.t, None
        for _ in range(3):
            m.train()
        after = split(m.variables())[0]
        assert set(before) == set(M.names()) and all(np.array_equal(before[k], after[k]) for k in before)
        assert est.opt.t == t0 == 1 and all(torch.equal(slots[k], t) for k, t in est.opt.state_tensors().items())
        assert any(np.any(s.cpu().numpy()) for s in slots.values())
        m0 = m.m.clone()
        est.train()
        assert any(not np.array_equal(before[k], v) for k, v in split(m.variables())[0].items())
        m.x_y.i -= 1                                                  # the same batch again: only the estimator differs
        m.train()
        assert not torch.equal(m0, m.m)
    assert [p.name for p in m.parts] == ['generator', 'discriminator', 'model'] and 'optimizers/model' in m.optimizers()


def test_builds_its_own_estimator():
    """estimator=None, through the dispatch table train.py uses: `--model experimental_sampler` runs on its own."""
    args = SimpleNamespace(batch_size=2, n_gpus=1, seed=0, use_graphs=True, **HP)
    sess = pkg('runtime').Session(device=DEV, dtype=0, seed=0, rank=0, world_size=1)
    train_func = pkg('models').model_funcs()['experimental_sampler'](R.Batches(2, 2, 0, DEV), args, sess)
    m = train_func.replica
    assert type(m) is plugin() and type(m.estimator).__name__ == 'mean_depth_estimator' and m.estimator.WIDTHS[0] == 64
    losses = train_func(sess, args)
    assert list(losses) == list(R.LOSS_KEYS) and all(np.isfinite(v) for v in losses.values())
    assert {'model/vars/l1/weights', 'model/vars/l8/bias'} <= set(m.variables())
    with pytest.raises(ValueError, match='--include_originals 53 70'):
        m.infer((m.x_y.x[0], m.x_y.y[0]))
    with pytest.raises(ValueError, match='estimator'):
        plugin()(m.x_y, SimpleNamespace(batch_size=4, n_gpus=1, seed=0, **HP), m.sess, estimator=m.estimator)


# ------------------------------------------------------------------------------------------------ the summary sets
def test_metrics_sets_against_the_oracle():
    """The three sets with every draw injected (noise_x per generator pass, the permutation, the noise set's input): the four
    statistics of each against the oracle's g under the same draws (1e-3, the model's yardstick) and, to the f32 rounding of
    the results, against the float64 statistics of the device's own g; keys and order; nothing else changes."""
    B = 4
    m = make(B=B, use_graphs=False)
    m.train()
    v0, fetch = m.variables(), (m.g32.clone(), m.target.clone(), m.scal.clone())
    slots = {(n, k): t.clone() for n, o in m.optimizers().items() for k, t in o.state_tensors().items()}
    last = m._losses()
    batch = m.x_y.batch(0)
    u = draws(B, 3, seed=11)
    perm = np.array([2, 0, 3, 1])
    xn = np.random.default_rng(12).uniform(0, 1, (B, R.SRC, R.SRC, 6)).astype(np.float32)
    m.sess.inject = {'noise_x': [a.copy() for a in u], 'shuffle': [perm], 'x_noise': [xn]}
    got = m.metrics()
    keys = pkg('models.experimental.experimental_sampler').SET_KEYS
    assert list(got) == list(keys) + list(R.LOSS_KEYS) and len(keys) == 12
    assert {k: got[k] for k in R.LOSS_KEYS} == last
    zero = [0] * B
    Xs, ys = oracle_inputs(m, batch, x_rows=zero, y_rows=zero)
    Xp, yp = oracle_inputs(m, batch, x_rows=perm)
    Xn = torch.tensor(R.noise_channel(xn), dtype=torch.float64)
    assert all(torch.equal(Xs[0], Xs[i]) and torch.equal(ys[0], ys[i]) for i in range(B))
    _, v = split(v0)
    for name, X, y, ui in (('sampler', Xs, ys, u[0]), ('shuffled', Xp, yp, u[1]), ('noise', Xn, ys, u[2])):
        with torch.no_grad():
            P = {k: torch.tensor(a, dtype=torch.float64) for k, a in v.items()}
            g = R.oracle_G(P, X, torch.tensor(R.noise_channel(ui), dtype=torch.float64)).numpy()
        ref = R.set_stats(y.numpy(), g)
        have = [got['moments/%s/moments/mean' % name], got['moments/%s/moments/var' % name],
                got['per_image_metrics/%s/rmse/mean' % name], got['per_image_metrics/%s/rmse/min' % name]]
        # g within e = 1e-3 of the oracle's (the model's yardstick on g, |g| <= 1) moves a mean by at most e, ten times a mean
        # absolute error by 10 e, and a variance, pixel by pixel, by at most 2 std e + e^2 <= 2 sqrt(var) e + e^2 on average
        e = 1e-3
        for h, r, bound, what in zip(have, ref, (e, 2 * np.sqrt(ref[1]) * e + e * e, 10 * e, 10 * e), ('mean', 'var', 'rmse/mean', 'rmse/min')):
            assert abs(h - r) <= bound, '%s %s: %r vs %r' % (name, what, h, r)
        assert have[1] > 0 and have[3] <= have[2]
    # the last set's statistics from the device's own g: f64 arithmetic, one f32 rounding (and the host's x10)
    own = R.set_stats(m.set_y['sampler'].cpu().numpy(), m.set_g.cpu().numpy())
    assert np.all(np.abs(np.array(have) - own) <= 2.0 ** -22 * np.abs(own))
    assert all(np.array_equal(v0[k], a) for k, a in m.variables().items())
    assert len(slots) == 6 and all(torch.equal(slots[(n, k)], t) for n, o in m.optimizers().items() for k, t in o.state_tensors().items())
    assert all(torch.equal(a, b) for a, b in zip(fetch, (m.g32, m.target, m.scal))) and m.sess.global_step == 2
    # the same noise draw in every row of the sampler set: the B predictions coincide
    one = np.repeat(draws(1, 1)[0], B, axis=0)
    m.sess.inject = {'noise_x': [one, one, one], 'shuffle': [perm], 'x_noise': [xn]}
    assert m.metrics()['moments/sampler/moments/var'] == 0.0


def test_sample_returns_an_uncertainty_map():
    B = 4
    m = make(B=B)
    m.train()
    b = m.x_y.batch(1)
    out = m.sample(b[0][2], b[2][2], b[3][2], b[4][2], b[1][2])
    assert tuple(out['y_hat'].shape) == (B, 32, 32) and tuple(out['mean'].shape) == (32, 32) == tuple(out['var'].shape)
    yh = out['y_hat'].cpu().numpy().astype(np.float64).reshape(B, -1)
    assert yh.min() >= 0 and yh.max() <= 1 and float(out['var'].max()) > 0
    assert np.allclose(out['mean'].cpu().numpy().ravel(), yh.mean(axis=0), rtol=0, atol=2e-7)
    # y_hat = fl((g + 1) / 2) carries d = 2**-23 of rounding per value: a variance moves by at most 2 std d + d^2, plus its own store
    var, d = yh.var(axis=0), 2.0 ** -23
    assert np.all(np.abs(out['var'].cpu().numpy().ravel() - var) <= 2 * np.sqrt(var) * d + d * d + d * var)
    y01 = b[1][2].cpu().numpy()[16:48, 16:48, 0].reshape(1, -1).astype(np.float64)
    assert len(out['metrics']) == 4
    close(out['metrics']['per_image_metrics/sampler/rmse/mean'], 10 * np.mean(np.abs(2 * y01 - 2 * yh), axis=1).mean(), 1e-5, 'rmse/mean')
    assert m.sample(b[0][2], b[2][2], b[3][2], b[4][2])['metrics'] is None
    with pytest.raises(ValueError, match='x must be'):
        m.sample(b[0][2][:63], b[2][2], b[3][2], b[4][2])


# ------------------------------------------------------------------------------------------------ determinism and I/O
def test_graph_replay_matches_eager_bit_for_bit():
    a, b = make(use_graphs=True), make(use_graphs=False)
    for i in range(3):
        assert a.train() == b.train()
        torch.manual_seed(i)
        ma = a.metrics()
        torch.manual_seed(i)
        assert same(ma, b.metrics())
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va) and a.sess.global_step == 6
    assert torch.equal(a.infer(a.x_y.batch(0)), b.infer(b.x_y.batch(0)))


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint after one train(), resume into a fresh model with other variables (the estimator's too): the next train(),
    its noise draw included, is bit-identical; the file carries all three parts."""
    ckpt = pkg('checkpoint')
    a = make()
    a.estimator.train()
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    z = np.load(path)
    assert {'generator/encoder/vars/e1/weights', 'discriminator/combined_path/vars/h6/bias', 'model/vars/l8/weights',
            'optimizers/generator/m', 'optimizers/discriminator/v', 'optimizers/model/m'} <= set(z.files)
    pos, drawn = a.x_y.i, a.sess.rng_state()
    assert drawn > 0
    la = a.train()
    b = make()
    b.load_variables({k: 0.5 * v for k, v in b.variables().items()})
    ckpt.restore(path, b, b.sess)
    assert b.sess.rng_state() == drawn and b.sess.global_step == 3
    b.x_y.i = pos
    assert b.train() == la
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


def test_bf16_runs_finite():
    m = make(B=16, dtype=1, n_batches=2)
    for _ in range(3):
        losses = m.train()
        assert all(np.isfinite(v) for v in losses.values()), losses
    met = m.metrics()
    assert all(np.isfinite(v) for v in met.values()) and met['moments/sampler/moments/var'] > 0
    assert np.all(np.isfinite(m.infer(m.x_y.next_batch()).cpu().numpy()))


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_cli_synthetic(tmp_path):
    """experimental.py end to end: the estimator's epochs, then the sampler's, one data source, checkpoints of the coupled
    model."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'experimental.py'), '--dataset', 'synthetic', '--batch_size', '4',
                        '--epoch_size', '2', '--estimator_epochs', '1', '--epochs', '1', '--optimizer', 'sgd', '--lr', '1e-3',
                        '--g_arch', 'B2', '--dir', str(tmp_path / 'ws')], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = p.stdout + p.stderr
    assert out.replace(' ', '').count('2/2') >= 2, out[-1500:]
    z = np.load(str(tmp_path / 'ws' / 'checkpoint-2.npz'))
    assert int(z['global_epoch']) == 2 and int(z['global_step']) == 2 + 2 * 2
    assert {'model/vars/l1/weights', 'generator/decoder/vars/d5/weights', 'discriminator/rgb_path/vars/hx1/weights'} <= set(z.files)
    z1 = np.load(str(tmp_path / 'ws' / 'checkpoint-1.npz'))
    assert np.array_equal(z1['model/vars/l8/weights'], z['model/vars/l8/weights'])         # the sampler phase leaves the estimator alone
    assert not np.array_equal(z1['generator/decoder/vars/d5/weights'], z['generator/decoder/vars/d5/weights'])
