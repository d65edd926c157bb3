"""paper_sampler / paper_noise on the GPU (hem/models/paper_sampler.py): the model against the float64 torch-autograd oracle
of tests/_sampler_ref.py with the noise injected at each node, the sampler pass and its statistics, graph replay, determinism,
checkpoint / resume, bf16 runs, train.py end to end, sample(), and a regression guard for paper_cgan and pix2pix."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _sampler_ref as R
from test_gpu_paper_cgan import close, grads_close, oracle_D, adam_ref, eigen_ref, Batches, DEFAULT_HP, SMALL_HP, DEV

pytestmark = pytest.mark.gpu
BN_FED = {'generator/encoder/vars/e%d/bias' % k for k in range(1, 5)}      # a bias in front of a batch norm: gradient exactly 0


def module():
    return pkg('models.sampler.paper_sampler')


def make(node='x', bn=False, B=4, dtype=0, seed=0, use_graphs=True, n_batches=8, data_seed=None, hp=DEFAULT_HP, model='paper_sampler'):
    args = SimpleNamespace(batch_size=B, n_gpus=1, noise_layer=node, e_bn='false', e_bn_off=not bn, seed=seed, use_graphs=use_graphs, **hp)
    if model == 'paper_noise':
        args = SimpleNamespace(batch_size=B, n_gpus=1, model_version='baseline', seed=seed, use_graphs=use_graphs, **hp)
    sess = pkg('runtime').Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    cls = getattr(pkg('models.sampler.' + model), model)
    return cls(Batches(B, n_batches, seed if data_seed is None else data_seed), args, sess)


def draws(node, B, k, seed=7):
    rng = np.random.default_rng([seed, R.NODES.index(node)])
    return [rng.uniform(0, 1, (B,) + R.NOISE_SHAPE[node]).astype(np.float32) for _ in range(k)]


def same_metrics(a, b):
    """Two metrics() results equal bit for bit (a NaN -- the log of a negative prediction -- equals a NaN)."""
    return list(a) == list(b) and all(list(a[k]) == list(b[k]) and np.array_equal(list(a[k].values()), list(b[k].values()), equal_nan=True)
                                      for k in a)


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------------------------ parity with the oracle
PARITY = [(n, False) for n in R.NODES] + [(n, True) for n in ('x', 'e2', 'd2', 'd4')]


def check_store(got, variables, batch, node, bn, u, which, what):
    """One store's gradients against the float64 oracle.  Without batch norm: grads_close (1e-3 of the store's largest entry,
    which must exceed 1e-4).  With batch norm in the encoder: per tensor, max |err| / max |ref| within max(1e-3, 3 x the
    oracle's own float32-vs-float64 deviation on that tensor), the yardstick of tests/test_gpu_headline_parity.py; the biases
    in front of a batch norm have a gradient of exactly zero, so theirs must stay within 1e-3 of the store's largest entry."""
    losses, ref, yhat = R.oracle_grads(variables, batch, node, bn, u, which, oracle_D)
    if not bn:
        grads_close(got, ref, what)
        return losses, yhat
    _, ref32, _ = R.oracle_grads(variables, batch, node, bn, u, which, oracle_D, dtype=torch.float32)
    scale = max(float(np.max(np.abs(r))) for k, r in ref.items() if k not in BN_FED)
    assert scale > 1e-4, '%s: reference gradients vanish (max %g)' % (what, scale)
    report = []
    for k, r in ref.items():
        if k in BN_FED:
            assert np.max(np.abs(got[k])) <= 1e-3 * scale, '%s %s: %g, not zero' % (what, k, np.max(np.abs(got[k])))
            continue
        assert np.any(r != 0), '%s %s: the reference gradient is identically zero' % (what, k)
        err, bound = relerr(got[k], r), max(1e-3, 3.0 * relerr(ref32[k], r))
        report.append('%s %.1e (%.1e)' % ('.'.join(k.split('/')[-3:]).replace('vars.', ''), err, bound))
        assert err <= bound, '%s %s: %g above %g' % (what, k, err, bound)
    print('%s %s bn, max |err| / max |ref| per tensor (bound): %s' % (what, node, ', '.join(report)))
    return losses, yhat


# The batches of each parity case: chosen by properties of the ORACLE alone, which the test asserts before it compares.
PARITY_DATA_SEED = {False: 6, True: {'x': 0, 'e2': 27, 'd2': 47, 'd4': 22}}
KINK_MARGIN = 5.0


@pytest.mark.parametrize('node,bn', PARITY)
def test_model_parity_f32(node, bn):
    """infer(), every D gradient after a D step, every G gradient and the four losses after a G step, noise injected.

    The data must not put a checked step at a kink of a small layer, where the (l)relu derivative jumps: any float32
    evaluation may land on either side, and the other side moves a gradient by that position's whole contribution.
      * G step, generator (_sampler_ref.nearest_kink): with the batches of seed 0, e3's input at image 1, (4, 2), channel 208
        is 1.5e-8 in float64 and 3.4e-8 in the oracle's float32; the other side moves e3/bias[208] by 1.9e-3 of the store's
        largest gradient.  Every such input must be 1e-6 away, 25 times the 4e-8 the oracle's own float32 inputs deviate.
      * With encoder batch norm each tensor is held to 1e-3 of its OWN largest entry, which one flip in the critic breaks:
        with the batches of seed 6 and noise at x, hy2's input on the real pass of the D step is 2.5e-8 at one position, and
        the float64 oracle with that one derivative flipped differs by 1.30e-3 on hy1/weights (5.8e-3 on hy2/weights) --
        the 1.297e-3 by which the device run missed it.  So there the critic's small layers must keep their inputs
        KINK_MARGIN times the rms float32 deviation of the layer away from zero (_sampler_ref.critic_kink_margin), in
        the D step and, with the variables after it, in the G step.
      * The batch-normalised encoder inputs are of order 1 with float32 errors of some 1e-7, and the batch-norm backward
        pass spreads one flipped derivative over its whole channel: with the batches of seed 3 and noise at e2 the device
        run was 1.97e-3 off on e1/weights while every other tensor of every batch-norm case agreed to 6e-6 or better.  So
        all four encoder layers must keep the same margin in the G step (_sampler_ref.encoder_kink_margin).
    The seeds are the first that meet all of these."""
    B = 8 if bn else 4
    m = make(node, bn, B=B, use_graphs=False, hp=SMALL_HP, data_seed=PARITY_DATA_SEED[True][node] if bn else PARITY_DATA_SEED[False])
    u = draws(node, B, 3)
    m.sess.inject = {'noise_' + node: [a.copy() for a in u]}
    b0 = m.x_y.next_batch()
    _, _, yh = R.oracle_grads(m.variables(), b0, node, bn, u[0], 'g', oracle_D)
    got = m.infer(b0)[..., 0].cpu().numpy()
    if bn:
        _, _, yh32 = R.oracle_grads(m.variables(), b0, node, bn, u[0], 'g', oracle_D, dtype=torch.float32)
        err, bound = relerr(got, yh[..., 0]), max(1e-3, 3.0 * relerr(yh32[..., 0], yh[..., 0]))
        print('infer %s bn: %.1e (%.1e)' % (node, err, bound))
        assert err <= bound
    else:
        close(got, yh[..., 0], 1e-3, 'infer')
    v0, b1 = m.variables(), m.x_y.next_batch()
    if bn:
        margin = R.critic_kink_margin(v0, b1, node, bn, u[1], True, 25 * B)
        assert margin >= KINK_MARGIN, 'the D step\'s batch puts a small critic layer %.2f deviations from a kink: choose other data' % margin
    m.d_step(b1)
    check_store({k: v for k, v in m.gradients().items() if k.startswith('discriminator/')}, v0, b1, node, bn, u[1], 'd', 'D step')
    v1, b2 = m.variables(), m.x_y.next_batch()
    kink = R.nearest_kink(v1, b2, node, bn, u[2], max_positions=25 * B)
    assert kink > 1e-6, 'the G step\'s batch puts a small layer %g from a kink: choose other data' % kink
    if bn:
        margin = min(R.critic_kink_margin(v1, b2, node, bn, u[2], False, 25 * B), R.encoder_kink_margin(v1, b2, node, u[2]))
        assert margin >= KINK_MARGIN, 'the G step\'s batch puts a layer %.2f deviations from a kink: choose other data' % margin
    m.g_step(b2)
    ref_l, _ = check_store({k: v for k, v in m.gradients().items() if k.startswith('generator/')}, v1, b2, node, bn, u[2], 'g', 'G step')
    got = m._losses()
    assert list(got) == ['g_fake', 'd_real', 'd_fake', 'd_total'] == list(ref_l)
    for k in ref_l:
        close(got[k], ref_l[k], 1e-3, 'loss ' + k)
    assert not m.sess.inject['noise_' + node]                    # one draw per generator pass: all three consumed
    scope, layer, width = R.READER[node]
    assert m.variables()['generator/%s/vars/%s/weights' % (scope, layer)].shape[3 if scope == 'decoder' and layer != 'd4' else 2] == width


@pytest.mark.parametrize('bn', [False, True])
def test_train_parity_f32(bn):
    """Variables after one full train() -- D step on batch 0, G step on batch 1, both Adam with their own rates and betas
    (:63-64,154-157) -- against the float64 oracle, compared as in tests/test_gpu_paper_cgan.py::test_train_parity_f32: where
    the gradients define Adam's direction the update matches to 2 % of lr on 99.9 % of the entries and to lr / 2 on all; every
    update stays within the steps' reach.  The biases in front of a batch norm have a zero gradient: Adam turns their
    rounding noise into steps of about lr, so they are only held to the reach."""
    node, hp, B = 'e2', SMALL_HP, 8 if bn else 4
    m = make(node, bn, B=B, use_graphs=False, hp=hp)
    u = draws(node, B, 2)
    m.sess.inject = {'noise_' + node: [a.copy() for a in u]}
    v0 = m.variables()
    batches = [(m.x_y.x[i], m.x_y.y[i]) for i in range(2)]
    m.train()
    v1 = m.variables()
    V = {k: v.astype(np.float64) for k, v in v0.items()}
    fuzzy, slots = {k: np.zeros(v.shape, bool) for k, v in V.items()}, {}
    for i, which in enumerate('dg'):
        _, grads, _ = R.oracle_grads(V, batches[i], node, bn, u[i], which, oracle_D)
        lr, b1, b2 = (hp['d_lr'], hp['d_beta1'], hp['d_beta2']) if which == 'd' else (hp['g_lr'], hp['g_beta1'], hp['g_beta2'])
        for k, G in grads.items():
            fuzzy[k] |= ((G != 0) & (np.abs(G) <= 1e-4 * np.max(np.abs(G)))) | (bn and k in BN_FED)
            V[k] = adam_ref(V[k], G, slots, k, lr, b1, b2)
    for store, lr in (('generator/', hp['g_lr']), ('discriminator/', hp['d_lr'])):
        keys = [k for k in v0 if k.startswith(store)]
        sharp = np.concatenate([~fuzzy[k].ravel() for k in keys])
        err = np.concatenate([np.abs((v1[k].astype(np.float64) - v0[k]) - (V[k] - v0[k])).ravel() for k in keys])
        assert sharp.mean() > 0.9 and max(float(np.max(np.abs(V[k] - v0[k]))) for k in keys) > 0.5 * lr
        print('%s bn %s: update error 99.9 %% quantile %.3g lr, max %.3g lr' % (store, bn, np.quantile(err[sharp], 0.999) / lr,
                                                                               np.max(err[sharp]) / lr))
        assert np.quantile(err[sharp], 0.999) <= 0.02 * lr and np.max(err[sharp]) <= 0.5 * lr
        assert np.max(err) <= 2.0 * lr + 1e-12
        for k in keys:
            close(v1[k], V[k], 1e-3, 'variable ' + k)


# ------------------------------------------------------------------------------------------------ the sampler pass
def stats_within(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.all(np.abs(got - ref) <= 2.0 ** -22 * np.abs(ref)), '%s: %r vs float64 %r' % (what, got, ref)


def test_metrics_y_sampler():
    keys, B, node = pkg('models.paper.paper_cgan').METRIC_KEYS, 4, 'e2'
    m = make(node, bn=False, B=B)
    m.train()
    x0 = m.x_y.x[1][0].cpu().numpy()                              # the G step's batch is the loss fetch's; its image 0
    v0 = m.variables()
    first = m.metrics()
    assert set(first) == {'metrics_y_hat', 'metrics_y_0', 'metrics_y_sampler'}
    for s in first.values():
        assert list(s) == list(keys) + list(R.STAT_KEYS)
    sx, u = m.samp_x.cpu().numpy(), m.G.noise_u['noise_' + node].cpu().numpy().reshape(B, -1)
    assert all(np.array_equal(sx[i], x0) for i in range(B))       # every row of the sampler's input is row 0
    assert all(not np.array_equal(u[i], u[j]) for i in range(B) for j in range(i))       # the noise rows differ
    crop, g, yhat = (t.cpu().numpy().reshape(B, -1) for t in (m.samp_crop, m.samp_g, m.samp_yhat))
    assert all(np.array_equal(crop[i], crop[0]) for i in range(B))
    got = first['metrics_y_sampler']
    close([got[k] for k in keys], eigen_ref(crop, yhat, [0, 0, 0, 0]), 1e-4, 'sampler set, Eigen values')
    stats_within([got[k] for k in R.STAT_KEYS], R.sample_stats(crop, g, yhat), 'sampler set, statistics')
    assert got['per_image_rmse/min'] <= got['per_image_rmse/mean'] and got['g_moments/var'] > 0
    # the y_hat and y_0 sets on the last fetch's own buffers
    fc, fg, fy, fb = (t.cpu().numpy().reshape(B, -1) for t in (m.crop, m.g32, m.yhat, m.ybar))
    stats_within([first['metrics_y_hat'][k] for k in R.STAT_KEYS], R.sample_stats(fc, fg, fy), 'y_hat statistics')
    s0 = [first['metrics_y_0'][k] for k in R.STAT_KEYS]
    assert s0[2] == 0.0 and s0[3] == 0.0
    ref0 = R.sample_stats(fc, np.zeros_like(fc), np.broadcast_to(fb, fc.shape))
    stats_within([s0[i] for i in (0, 1, 4, 5)], ref0[[0, 1, 4, 5]], 'y_0 statistics')
    # training variables and metrics_y_hat are unchanged by the call; a mean image adds its set
    second = m.metrics()
    assert same_metrics({'s': second['metrics_y_hat']}, {'s': first['metrics_y_hat']})
    v1 = m.variables()
    assert all(np.array_equal(v0[k], v1[k]) for k in v0)
    m.set_mean_image(np.full((29, 29), 0.5, np.float32))
    third = m.metrics()
    stats_within([third['metrics_y_mean'][k] for k in R.STAT_KEYS], R.sample_stats(fc, fg, np.full_like(fc, 5.0)), 'y_mean statistics')
    # the same draw in every row: the B predictions coincide
    one = draws(node, 1, 1)[0]
    m.sess.inject = {'noise_' + node: [np.repeat(one, B, axis=0)]}
    same = m.metrics()['metrics_y_sampler']
    assert same['g_moments/var'] == 0.0 and same['y_hat_moments/var'] == 0.0


def test_sample_returns_an_uncertainty_map():
    B = 4
    m = make('d3', bn=True, B=B)
    m.train()
    x, y = m.x_y.x[0][2], m.x_y.y[0][2]
    out = m.sample(x, y)
    assert tuple(out['y_hat'].shape) == (B, 29, 29) and tuple(out['mean'].shape) == (29, 29) == tuple(out['var'].shape)
    yh = out['y_hat'].cpu().numpy().astype(np.float64).reshape(B, -1)
    stats_within(out['var'].cpu().numpy().ravel(), yh.var(axis=0) / 100.0, 'variance image')
    stats_within(out['mean'].cpu().numpy().ravel(), yh.mean(axis=0) / 10.0, 'mean image')
    assert float(out['var'].max()) > 0 and len(out['metrics']) == 14
    crop = 10.0 * y.cpu().numpy()[17:46, 17:46, 0].reshape(1, -1).repeat(B, axis=0)
    stats_within([out['metrics'][k] for k in R.STAT_KEYS][:2], R.sample_stats(crop, yh, yh)[:2], 'per-image error')
    assert m.sample(x)['metrics'] is None
    with pytest.raises(ValueError):
        m.sample(x[:64])
    for call in (m.infer_full, m.evaluate):
        with pytest.raises(NotImplementedError, match='batch norm'):
            call(None, None)


# ------------------------------------------------------------------------------------------------ determinism and I/O
@pytest.mark.parametrize('node,bn', [('e2', True), ('d4', False)])
def test_graph_replay_matches_eager_bit_for_bit(node, bn):
    a, b = make(node, bn, B=8, use_graphs=True), make(node, bn, B=8, use_graphs=False)
    for _ in range(3):
        assert a.train() == b.train()
        assert same_metrics(a.metrics(), b.metrics())
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


def test_two_fresh_models_are_bit_equal():
    a, b = make('e4', True, B=8, seed=3), make('e4', True, B=8, seed=3)
    for _ in range(3):
        assert a.train() == b.train()
    assert same_metrics(a.metrics(), b.metrics())
    assert np.array_equal(a.sample(a.x_y.x[0][0])['var'].cpu().numpy(), b.sample(b.x_y.x[0][0])['var'].cpu().numpy())


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint after one train(), resume into a model of the same --seed (the Philox key) with other variables and the
    same data stream: the next train() -- its noise draws included, so the Philox counter came back too -- is bit-identical."""
    ckpt = pkg('checkpoint')
    a = make('e1', True, B=8, hp=SMALL_HP)
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    pos, drawn = a.x_y.i, a.sess.rng_state()
    assert drawn > 0
    la = a.train()
    b = make('e1', True, B=8, hp=SMALL_HP)
    b.load_variables({k: 0.5 * v for k, v in b.variables().items()})
    assert any(not np.array_equal(b.variables()[k], v) for k, v in a.variables().items()) and b.sess.rng_state() == 0
    ckpt.restore(path, b, b.sess)
    assert b.sess.rng_state() == drawn
    b.x_y.i = pos
    assert b.train() == la
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    assert any(k.endswith('BatchNorm_3/beta') for k in va)


@pytest.mark.parametrize('node', ['x', 'e4-512', 'd4'])
def test_bf16_runs_finite(node):
    m = make(node, True, B=64, dtype=1, n_batches=4)
    for _ in range(4):
        losses = m.train()
        assert all(np.isfinite(v) for v in losses.values()), losses
    met = m.metrics()
    for name in ('metrics_y_hat', 'metrics_y_0', 'metrics_y_sampler'):
        assert all(np.isfinite(v) for v in met[name].values()), (name, met[name])
    assert met['metrics_y_sampler']['g_moments/var'] > 0
    assert np.all(np.isfinite(m.infer(m.x_y.next_batch()).cpu().numpy()))


def test_paper_noise_trains():
    m = make(model='paper_noise', B=4)
    assert m.G.xn is not None and list(m.G.noise) == ['noise_x'] and not m.G.e_bn_name
    losses = m.train()
    assert list(losses) == ['g_fake', 'd_real', 'd_fake', 'd_total'] and all(np.isfinite(v) for v in losses.values())
    assert m.metrics()['metrics_y_sampler']['g_moments/var'] > 0


def test_train_cli_synthetic(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_sampler', '--noise_layer', 'e2', '--dataset',
                        'synthetic', '--random_crop', '65', '65', '--batch_size', '8', '--epoch_size', '2', '--epochs', '1',
                        '--dir', str(tmp_path / 'ws')], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = p.stdout + p.stderr
    assert '2/2' in out.replace(' ', ''), out[-1500:]
    assert os.path.exists(str(tmp_path / 'ws' / 'checkpoint-1.npz'))


# ------------------------------------------------------------------------------------------------ regression guard
def test_paper_cgan_and_pix2pix_variables_are_those_of_the_parent_commit():
    """One train() of paper_cgan --model_version mean_adjusted and of pix2pix --noise input latent end leaves every variable
    with the bytes it had before the executor learned its other noise nodes and paper_cgan's shared parts moved into a base
    class.  tests/golden/regression_digests.npz was written on the parent commit of that change by
    `python tools/regression_digest.py tests/golden/regression_digests.npz` (the tool, copied into that checkout, uses only
    what both trees have)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import regression_digest
    finally:
        sys.path.pop(0)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'regression_digests.npz'))
    want = {str(n): (str(h), float(s)) for n, h, s in zip(z['names'], z['sha256'], z['sums'])}
    got = regression_digest.digests(DEV)
    assert set(got) == set(want)
    assert any(k.startswith('pix2pix/') for k in got) and any(k.startswith('paper_cgan/') for k in got)
    bad = ['%s: sum %r, was %r' % (k, got[k][1], want[k][1]) for k in sorted(got) if got[k][0] != want[k][0]]
    assert not bad, '\n'.join(bad[:10])
