"""improved_sampler on the GPU (hem/models/improved_sampler.py) at full widths, B = 4: for each of the six arch pairs both
gradient sets of ONE forward pass, the losses and infer() against the float64 torch-autograd oracle of tests/_isamp_ref.py with
the noise injected; `--g_rmse` and `--g_sparsity`; one train() against the oracle plus a float64 Adam; the three summary sets;
E1 against experimental_sampler bit for bit; graph replay, checkpoint / resume; a bf16 run per arch; train.py end to end."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _isamp_ref as R
import _xsamp_ref as XR
from test_gpu_paper_cgan import close, grads_close, DEV
import test_gpu_experimental_sampler as XS

pytestmark = pytest.mark.gpu
HP = dict(optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, decay=0.9, momentum=0.01, centered=False)
KINK_MARGIN = XS.KINK_MARGIN
# The parity batch per arch: the first data seed whose batch 0 (of a 4-batch source) keeps, at the variables of session seed 0
# and the noise of draws(), every (l)relu input of the generator's small layers (at most 25 B positions per channel) 1e-6 from
# zero and those of the critic's small layers KINK_MARGIN rms float32 deviations from zero, on D(X, y) and on D(X, g) -- the
# margins tests/test_gpu_experimental_sampler.py demands, properties of the ORACLE alone (tests/_isamp_ref.nearest_kink /
# critic_kink_margin on initial_variables(), found on the CPU) and asserted before anything is compared.
# seed: (nearest generator kink, critic margin) as found
PARITY_DATA_SEED = {'A1': 0, 'A2': 0, 'A3': 0, 'B2': 10, 'D1': 6, 'E1': 7}
PARITY_FOUND = {'A1': (1.72e-5, 7.93), 'A2': (1.52e-6, 6.66), 'A3': (4.83e-6, 7.93), 'B2': (2.05e-6, 9.15), 'D1': (2.47e-6, 23.6),
                'E1': (5.53e-6, 8.33)}


def plugin():
    return pkg('models.improved.improved_sampler').improved_sampler


def make(g, d=None, B=4, dtype=0, seed=0, use_graphs=True, n_batches=4, data_seed=0, data=None, **flags):
    args = SimpleNamespace(batch_size=B, n_gpus=1, seed=seed, use_graphs=use_graphs, g_arch=g, d_arch=d or dict(R.PAIRS)[g], **flags, **HP)
    sess = pkg('runtime').Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    return plugin()(data if data is not None else R.Batches(g, B, n_batches, data_seed, DEV), args, sess)


def draws(B, k, S, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1, (B, S, S, 1)).astype(np.float32) for _ in range(k)]


def same(a, b):
    return list(a) == list(b) and np.array_equal(list(a.values()), list(b.values()), equal_nan=True)


def grads_of(m, u, **kw):
    """The gradient body of one train() on batch 0 with the noise `u` injected: (gradients, losses)."""
    m.sess.inject = {'noise_x': [u.copy()]}
    m.x_y.i = 0
    m._stage(m._batch(m.x_y.next_batch()))
    m._grads()
    return m.gradients(), m._losses()


# ------------------------------------------------------------------------------------------------ parity with the oracle
@pytest.mark.parametrize('g,d', R.PAIRS)
def test_model_parity_f32(g, d):
    """After the gradient body of one train(), before the apply: every D gradient, every G gradient (grads_close: 1e-3 of the
    store's largest entry, which must exceed 1e-4) and the six losses (1e-3) against the float64 oracle -- both gradient sets
    from the one forward pass, at the variables before either update; then infer() against the oracle's (g + 1) / 2."""
    B, a = 4, R.ARCHS[g]
    m = make(g, d, B=B, use_graphs=False, data_seed=PARITY_DATA_SEED[g])
    u = draws(B, 2, a['S'])
    m.sess.inject = {'noise_x': [x.copy() for x in u]}
    b0 = m.x_y.batch(0)
    v0 = m.variables()
    init = R.initial_variables(g, 0)
    assert set(v0) == set(init) and all(np.array_equal(v0[k], init[k]) for k in init)      # what the CPU search of the seed assumed
    X, y = R.assemble(g, b0)
    noise = R.noise_channel(u[0])
    kink = R.nearest_kink(g, v0, X, noise, max_positions=25 * B)
    assert kink > 1e-6, 'the batch puts a small generator layer %g from a kink: choose other data' % kink
    margin = R.critic_kink_margin(g, v0, X, y, noise, max_positions=25 * B)
    assert margin >= KINK_MARGIN, 'the batch puts a small critic layer %.2f deviations from a kink: choose other data' % margin
    print('%s: seed %d, kink %.3g, margin %.2f (found: %s)' % (g, PARITY_DATA_SEED[g], kink, margin, PARITY_FOUND[g]))
    losses, dg, gg, out = R.oracle_grads(g, v0, X, y, noise)
    m._stage(m._batch(m.x_y.next_batch()))
    m._grads()
    got = m.gradients()
    grads_close({k: v for k, v in got.items() if k.startswith('discriminator/')}, dg, 'D gradients')
    grads_close({k: v for k, v in got.items() if k.startswith('generator/')}, gg, 'G gradients')
    assert set(got) == set(dg) | set(gg)
    have = m._losses()
    assert list(have) == list(R.LOSS_KEYS) == list(losses)
    for k in losses:
        close(have[k], losses[k], 1e-3, 'loss ' + k)
    close(m.g32.cpu().numpy(), out[..., 0], 1e-3, 'g')
    assert np.array_equal(m.target.cpu().numpy(), y[..., 0].numpy().astype(np.float32))
    # infer(): the next draw, the same batch
    ref = R.oracle_grads(g, v0, X, y, R.noise_channel(u[1]))[3]
    res = m.infer(b0)
    assert tuple(res.shape) == (B, a['T'], a['T'], 1) and float(res.min()) >= 0 and float(res.max()) <= 1
    close(res.cpu().numpy(), (ref + 1) / 2, 1e-3, 'infer')
    assert not m.sess.inject['noise_x']                                                  # one draw per generator pass


def test_g_rmse_on_d1():
    """G's gradients against the oracle's g_total = g_fake + rmse; D's gradients bit-identical to the run without the flag; the
    loss dict gains g_total."""
    g, B = 'D1', 4
    u = draws(B, 1, 64)[0]
    plain = make(g, B=B, use_graphs=False, data_seed=PARITY_DATA_SEED[g])
    flagged = make(g, B=B, use_graphs=False, data_seed=PARITY_DATA_SEED[g], g_rmse=True)
    v0 = plain.variables()
    assert all(np.array_equal(v0[k], v) for k, v in flagged.variables().items())
    g0, l0 = grads_of(plain, u)
    g1, l1 = grads_of(flagged, u)
    assert list(l1) == list(R.loss_keys(g_rmse=True)) == list(R.LOSS_KEYS) + ['g_total'] and list(l0) == list(R.LOSS_KEYS)
    assert all(l1[k] == l0[k] for k in l0) and l1['g_total'] == l1['g_fake'] + l1['rmse']
    assert all(np.array_equal(g0[k], g1[k]) for k in g0 if k.startswith('discriminator/'))
    assert any(not np.array_equal(g0[k], g1[k]) for k in g0 if k.startswith('generator/'))
    X, y = R.assemble(g, plain.x_y.batch(0))
    losses, _, gg, _ = R.oracle_grads(g, v0, X, y, R.noise_channel(u), g_rmse=True)
    grads_close({k: v for k, v in g1.items() if k.startswith('generator/')}, gg, 'G gradients of g_total')
    for k in losses:
        close(l1[k], losses[k], 1e-3, 'loss ' + k)
    # the rmse term is a real share of the gradient: without it the comparison above fails
    plain_gg = R.oracle_grads(g, v0, X, y, R.noise_channel(u))[2]
    scale = max(float(np.max(np.abs(r))) for r in gg.values())
    assert max(float(np.max(np.abs(gg[k] - plain_gg[k]))) for k in gg) > 1e-2 * scale


def test_g_sparsity_on_e1():
    """zero_fraction has no gradient: every gradient bit-identical to the run without the flag, with and without --g_rmse;
    sparsity_term is the exact zero count of the model's own e5; the keys; A1 has no e5."""
    g, B = 'E1', 4
    u = draws(B, 1, 64)[0]
    for rmse in (False, True):
        plain = make(g, B=B, use_graphs=False, g_rmse=rmse)
        flagged = make(g, B=B, use_graphs=False, g_rmse=rmse, g_sparsity=True)
        g0, l0 = grads_of(plain, u)
        g1, l1 = grads_of(flagged, u)
        assert set(g0) == set(g1) and all(np.array_equal(g0[k], g1[k]) for k in g0)
        assert list(l1) == list(R.loss_keys(rmse, True)) == list(R.LOSS_KEYS) + ['g_total', 'sparsity_term']
        e5 = flagged.G.e_h[5]
        act = e5.buf.float().cpu().numpy().reshape(B, e5.cs)[:, :1024]
        want = np.float32(int((act == 0).sum()) / (B * 1024))
        assert l1['sparsity_term'] == float(want) and 0.0 < want < 1.0 and np.all(act >= 0)
        assert l1['g_total'] == l1['g_fake'] - l1['sparsity_term'] + (l1['rmse'] if rmse else 0.0)
        assert all(l1[k] == l0[k] for k in R.LOSS_KEYS)
    X, y = R.assemble(g, flagged.x_y.batch(0))
    ref = R.oracle_grads(g, flagged.variables(), X, y, R.noise_channel(u), True, True)[0]
    assert abs(l1['sparsity_term'] - ref['sparsity_term']) <= 8 / (B * 1024)            # a relu input within rounding of zero may flip
    for arch in ('A1', 'A2', 'A3'):
        with pytest.raises(ValueError, match='e5'):
            make(arch, g_sparsity=True)


@pytest.mark.parametrize('g', ['A1', 'D1'])
def test_train_parity_f32(g):
    """Variables after one train() against the float64 oracle plus a float64 Adam, by the rule of
    tests/test_gpu_paper_cgan.py::test_train_parity_f32 as tests/test_gpu_experimental_sampler.py states it: where the gradients
    define Adam's direction the update matches to 2 % of lr on 99.9 % of the entries and to lr / 2 on all; every update stays
    within the step's reach.  global_step advances by 2."""
    B, lr = 4, HP['lr']
    m = make(g, B=B, use_graphs=False, data_seed=PARITY_DATA_SEED[g])
    u = draws(B, 1, R.ARCHS[g]['S'])
    m.sess.inject = {'noise_x': [x.copy() for x in u]}
    v0 = m.variables()
    X, y = R.assemble(g, m.x_y.batch(0))
    _, dg, gg, _ = R.oracle_grads(g, v0, X, y, R.noise_channel(u[0]))
    m.train()
    assert m.sess.global_step == 2 and m.g_opt.t == 1 and m.d_opt.t == 1
    v1 = m.variables()
    slots = {}
    for store, grads in (('generator/', gg), ('discriminator/', dg)):
        V = {k: XR.adam_ref(v0[k].astype(np.float64), G, slots, k, lr, HP['beta1'], HP['beta2']) for k, G in grads.items()}
        fuzzy = {k: (G != 0) & (np.abs(G) <= 1e-4 * np.max(np.abs(G))) for k, G in grads.items()}
        # the bias in front of a batch norm has a gradient that is rounding noise in the oracle and on the device alike: Adam turns
        # the noise's sign into a full step, so it defines no direction
        dead = {'generator/%s/vars/%s/bias' % ('encoder' if l[0] == 'e' else 'decoder', l) for l in R.bn_names(g)}
        keys = [k for k in grads if k not in dead]
        sharp = np.concatenate([~fuzzy[k].ravel() for k in keys])
        err = np.concatenate([np.abs((v1[k].astype(np.float64) - v0[k]) - (V[k] - v0[k])).ravel() for k in keys])
        assert sharp.mean() > 0.9 and max(float(np.max(np.abs(V[k] - v0[k]))) for k in keys) > 0.5 * lr
        print('%s update error 99.9 %% quantile %.3g lr, max %.3g lr' % (store, np.quantile(err[sharp], 0.999) / lr, np.max(err[sharp]) / lr))
        assert np.quantile(err[sharp], 0.999) <= 0.02 * lr and np.max(err[sharp]) <= 0.5 * lr
        assert np.max(err) <= 2.0 * lr + 1e-12
        for k in keys:
            close(v1[k], V[k], 1e-3, 'variable ' + k)
        for k in dead & set(grads):
            assert np.max(np.abs(grads[k])) < 1e-12 and np.max(np.abs(v1[k].astype(np.float64) - v0[k])) <= 2.0 * lr + 1e-12


# ------------------------------------------------------------------------------------------------ the summary sets
def test_metrics_sets_against_the_oracle():
    """D1: the three sets with every draw injected (noise_x per generator pass, the permutation, the noise set's input -- all
    five planes of X permuted together and noised): the four statistics of each against the oracle's g under the same draws
    (the bounds of tests/test_gpu_experimental_sampler.py) and, to the f32 rounding of the results, against the float64
    statistics of the device's own g; keys and order; nothing else changes."""
    g, B = 'D1', 4
    m = make(g, B=B, use_graphs=False)
    m.train()
    v0, fetch = m.variables(), (m.g32.clone(), m.target.clone(), m.scal.clone())
    slots = {(n, k): t.clone() for n, o in m.optimizers().items() for k, t in o.state_tensors().items()}
    last = m._losses()
    batch = m.x_y.batch(0)
    u = draws(B, 3, 64, seed=11)
    perm = np.array([2, 0, 3, 1])
    xn = np.random.default_rng(12).uniform(0, 1, (B, 64, 64, 5)).astype(np.float32)
    m.sess.inject = {'noise_x': [a.copy() for a in u], 'shuffle': [perm], 'x_noise': [xn]}
    got = m.metrics()
    keys = pkg('models.improved.improved_sampler').SET_KEYS
    assert list(got) == list(keys) + list(R.LOSS_KEYS) and len(keys) == 12
    assert {k: got[k] for k in R.LOSS_KEYS} == last
    zero = [0] * B
    Xs, ys = R.assemble(g, batch, x_rows=zero, y_rows=zero)
    Xp, yp = R.assemble(g, batch, x_rows=perm)
    Xn = torch.tensor(R.noise_channel(xn), dtype=torch.float64)
    assert all(torch.equal(Xs[0], Xs[i]) and torch.equal(ys[0], ys[i]) for i in range(B)) and torch.equal(Xp[0, ..., 3:], Xs[0, ..., 3:])
    assert not torch.equal(Xp[0, ..., :3], Xs[0, ..., :3]) and tuple(Xn.shape) == tuple(Xs.shape)
    for name, X, y, ui in (('sampler', Xs, ys, u[0]), ('shuffled', Xp, yp, u[1]), ('noise', Xn, ys, u[2])):
        with torch.no_grad():
            P = {k: torch.tensor(a, dtype=torch.float64) for k, a in v0.items()}
            out = R.oracle_G(g, P, X, torch.tensor(R.noise_channel(ui), dtype=torch.float64)).numpy()
        ref = R.set_stats(y.numpy(), out)
        have = [got['moments/%s/moments/mean' % name], got['moments/%s/moments/var' % name],
                got['per_image_metrics/%s/rmse/mean' % name], got['per_image_metrics/%s/rmse/min' % name]]
        e = 1e-3
        for h, r, bound, what in zip(have, ref, (e, 2 * np.sqrt(ref[1]) * e + e * e, 10 * e, 10 * e), ('mean', 'var', 'rmse/mean', 'rmse/min')):
            assert abs(h - r) <= bound, '%s %s: %r vs %r' % (name, what, h, r)
        assert have[1] > 0 and have[3] <= have[2]
    own = R.set_stats(m.set_y['sampler'].cpu().numpy(), m.set_g.cpu().numpy())
    assert np.all(np.abs(np.array(have) - own) <= 2.0 ** -22 * np.abs(own))
    assert all(np.array_equal(v0[k], a) for k, a in m.variables().items())
    assert len(slots) == 4 and all(torch.equal(slots[(n, k)], t) for n, o in m.optimizers().items() for k, t in o.state_tensors().items())
    assert all(torch.equal(a, b) for a, b in zip(fetch, (m.g32, m.target, m.scal))) and m.sess.global_step == 2


def test_sample_returns_an_uncertainty_map():
    B = 4
    m = make('D1', B=B)
    m.train()
    b = m.x_y.batch(1)
    out = m.sample(b[0][2], b[1][2], b[2][2], b[3][2])
    assert tuple(out['y_hat'].shape) == (B, 32, 32) and tuple(out['mean'].shape) == (32, 32) == tuple(out['var'].shape)
    yh = out['y_hat'].cpu().numpy().astype(np.float64).reshape(B, -1)
    assert yh.min() >= 0 and yh.max() <= 1 and float(out['var'].max()) > 0 and len(out['metrics']) == 4
    assert np.allclose(out['mean'].cpu().numpy().ravel(), yh.mean(axis=0), rtol=0, atol=2e-7)
    assert m.sample(b[0][2], None, b[2][2], b[3][2])['metrics'] is None
    with pytest.raises(ValueError, match='reads x_loc'):
        m.sample(b[0][2])
    with pytest.raises(ValueError, match='x must be'):
        m.sample(b[0][2][:63], None, b[2][2], b[3][2])


# ------------------------------------------------------------------------------------------------ E1 is experimental_sampler
class _Tuples:
    def __init__(self, batches):
        self.batches, self.i = batches, 0

    def batch(self, k):
        return self.batches[k]

    def next_batch(self):
        k = self.i % len(self.batches)
        self.i += 1
        return self.batches[k]


@pytest.mark.parametrize('dtype', [0, 1])
def test_e1_is_experimental_sampler_bit_for_bit(dtype):
    """The same variables, the same injected noise and a dataset mean_vec equal to the estimator's m: the six losses and both
    gradient sets are bit-identical, in f32 and in bf16."""
    B = 4
    xs = XS.make(B=B, dtype=dtype, use_graphs=False)
    u = draws(B, 1, 64)[0]
    xs.sess.inject = {'noise_x': [u.copy()]}
    b = xs.x_y.batch(0)
    xs._stage(xs._batch(xs.x_y.next_batch()))
    xs._grads()
    want_g, want_l = xs.gradients(), xs._losses()
    mvec = xs.m[:B].clone().reshape(B, 1, 1, 1).expand(B, 64, 64, 1).contiguous()
    m = make('E1', B=B, dtype=dtype, use_graphs=False, data=_Tuples([(b[0], b[1], b[2], b[3], mvec)]))
    m.load_variables({k: v for k, v in xs.variables().items() if not k.startswith('model/')})
    got_g, got_l = grads_of(m, u)
    assert same(got_l, want_l) and all(np.isfinite(v) for v in got_l.values())
    assert set(got_g) == {k for k in want_g if not k.startswith('model/')}
    assert all(np.array_equal(got_g[k], want_g[k]) for k in got_g) and any(np.any(v) for v in got_g.values())
    assert torch.equal(m.g32, xs.g32) and torch.equal(m.target, xs.target)


# ------------------------------------------------------------------------------------------------ determinism and I/O
@pytest.mark.parametrize('g,flags', [('A1', {}), ('E1', dict(g_rmse=True, g_sparsity=True))])
def test_graph_replay_matches_eager_bit_for_bit(g, flags):
    a, b = make(g, use_graphs=True, **flags), make(g, use_graphs=False, **flags)
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
    """Checkpoint after one train(), resume into a fresh model with other variables: the next train(), its noise draw included,
    is bit-identical; the file carries both parts and A1's betas."""
    ckpt = pkg('checkpoint')
    a = make('A1')
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    z = np.load(path)
    assert {'generator/encoder/vars/e1/weights', 'generator/decoder/BatchNorm_3/beta', 'generator/encoder/BatchNorm/beta',
            'discriminator/combined_path/vars/h3/bias', 'optimizers/generator/m', 'optimizers/discriminator/v'} <= set(z.files)
    pos, drawn = a.x_y.i, a.sess.rng_state()
    assert drawn > 0
    la = a.train()
    b = make('A1')
    b.load_variables({k: 0.5 * v for k, v in b.variables().items()})
    ckpt.restore(path, b, b.sess)
    assert b.sess.rng_state() == drawn and b.sess.global_step == 2
    b.x_y.i = pos
    assert b.train() == la
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    assert np.any(va['generator/decoder/BatchNorm_3/beta'] != 0)                         # the head's beta trains


@pytest.mark.parametrize('g', list(R.ARCHS))
def test_bf16_runs_finite(g):
    m = make(g, B=16, dtype=1, n_batches=2)
    for _ in range(3):
        losses = m.train()
        assert all(np.isfinite(v) for v in losses.values()), losses
    met = m.metrics()
    assert all(np.isfinite(v) for v in met.values()) and met['moments/sampler/moments/var'] > 0
    assert np.all(np.isfinite(m.infer(m.x_y.next_batch()).cpu().numpy()))


def test_shape_errors_name_the_dataset_flags():
    m = make('E1', B=2, n_batches=1)
    with pytest.raises(ValueError, match='--random_crop 64 64 --include_location --normalize'):
        m.infer((m.x_y.x[0], m.x_y.y[0]))
    with pytest.raises(ValueError, match=r'\(A1 \| A2 \| A3, A1\)'):
        make('A1', 'B2')


# ------------------------------------------------------------------------------------------------ the command line
@pytest.mark.parametrize('g,extra', [('A1', []), ('E1', ['--g_rmse', '--g_sparsity'])])
def test_train_cli_synthetic(tmp_path, g, extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'improved_sampler', '--g_arch', g, '--d_arch',
                        dict(R.PAIRS)[g], '--dataset', 'synthetic', '--batch_size', '8', '--epoch_size', '2', '--epochs', '1',
                        '--optimizer', 'adam', '--lr', '1e-4', '--dir', str(tmp_path / 'ws')] + extra, env=env, timeout=600,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = p.stdout + p.stderr
    assert '2/2' in out.replace(' ', '') and 'Training complete' in out, out[-1500:]
    z = np.load(str(tmp_path / 'ws' / 'checkpoint-1.npz'))
    assert int(z['global_step']) == 4 and 'generator/encoder/vars/e1/weights' in z.files
    assert ('generator/decoder/BatchNorm_3/beta' in z.files) == (g == 'A1')
