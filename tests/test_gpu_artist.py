"""artist on the GPU (hem/models/artist.py) at its full widths and 256x256, B = 4 (the geometry is fixed by the decoder's output
shapes, so the small axis is the batch; 4 is the smallest at which the 1x1 latent's batch norm still has a spread): the
gradient bodies of the y step and of the x step and the losses against the float64 torch-autograd oracle of
tests/_artist_ref.py; one train() against the oracle's two steps under a float64 Adam; infer() and evaluate(); graph replay,
checkpoint / resume; a bf16 run; the montages; train.py end to end."""
import functools
import os
import struct
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _artist_ref as R
from test_gpu_paper_cgan import close, grads_close, DEV

pytestmark = pytest.mark.gpu
HP = dict(optimizer='adam', lr=1e-3, beta1=0.9, beta2=0.999, decay=0.9, momentum=0.01, centered=False)
B = 4
# The parity batch: the first data seed (of 0..79, searched on the CPU) whose batch 0 keeps EVERY lrelu input of the three nets --
# 2 077 584 of them -- further than 1e-6 from its kink with the most room, at the variables of session seed 0: a property of the
# ORACLE alone (tests/_artist_ref.kink_report, through tests/_kinks.py's recorder), asserted before anything is compared.
PARITY_DATA_SEED = 8
PARITY_FOUND = 1.92e-6                               # the smallest |input| as found
# train(): the y step runs on the parity batch; the x step's batch is batch 0 of the data seed (of 0..79, the same search) that
# keeps every lrelu input 1e-6 from its kink with the most room at the ORACLE's variables after its y step.
TRAIN_X_SEED = 72
TRAIN_X_FOUND = 1.17e-6


def plugin():
    return pkg('models.artist.artist').artist


def train_pairs(device):
    return R.Pairs([R.Batches(B, 1, PARITY_DATA_SEED, device).batch(0), R.Batches(B, 1, TRAIN_X_SEED, device).batch(0)])


def make(dtype=0, seed=0, use_graphs=True, n_batches=4, data_seed=PARITY_DATA_SEED, examples=4, hp=HP, data=None):
    args = SimpleNamespace(batch_size=B, n_gpus=1, seed=seed, use_graphs=use_graphs, examples=examples, **hp)
    sess = pkg('runtime').Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    return plugin()(data if data is not None else R.Batches(B, n_batches, data_seed, DEV), args, sess)


def host(batch):
    return tuple(t.cpu() for t in batch)


@functools.lru_cache(maxsize=None)
def oracle(k):
    """oracle_grads at the initial variables on batch k of the parity source: computed once, shared, never modified."""
    return R.oracle_grads(R.initial_variables(0), *R.Batches(B, 4, PARITY_DATA_SEED).batch(k))


def same(a, b):
    return list(a) == list(b) and np.array_equal(list(a.values()), list(b.values()), equal_nan=True)


# ------------------------------------------------------------------------------------------------ parity with the oracle
def test_gradient_bodies_parity_f32():
    """After the gradient body of the y step, and then of the x step, before any apply: every gradient of the step's variable
    set (grads_close: 1e-3 of the set's largest entry, which must exceed 1e-4), the losses (1e-3), and every gradient of
    encoder + y_decoder exactly untouched by the x step."""
    m = make(use_graphs=False)
    v0, init = m.variables(), R.initial_variables(0)
    assert set(v0) == set(init) and all(np.array_equal(v0[k], init[k]) for k in init)      # what the CPU search of the seed assumed
    b0 = m.x_y.batch(0)
    near, kmin, count = R.kink_report(v0, b0[0].cpu())
    print('seed %d: %d lrelu inputs, the nearest %.3g from its kink (found: %.3g)' % (PARITY_DATA_SEED, count, kmin, PARITY_FOUND))
    assert not near and kmin > 1e-6 and count == 2077584, 'the batch puts %d lrelu inputs within 1e-6 of a kink: choose other data' % len(near)
    losses, yg, xg, _, _ = oracle(0)
    m._stage(m._batch(b0))
    assert not any(np.any(g) for g in m.gradients().values())
    m._y_grads()
    after_y = m.gradients()
    grads_close({k: v for k, v in after_y.items() if k.startswith(R.Y_SET)}, yg, 'y-step gradients')
    assert not any(np.any(after_y[k]) for k in after_y if k.startswith(R.X_SET)) and set(after_y) == set(yg) | set(xg)
    have = m.losses()
    assert list(have) == list(R.LOSS_KEYS)
    close(have['y_hat_loss'], losses['y_hat_loss'], 1e-3, 'y_hat_loss')
    close(have['y_hat_rmse'], losses['y_hat_rmse'], 1e-3, 'y_hat_rmse')
    m._x_grads()                                                                         # the same batch, the same variables
    after_x = m.gradients()
    grads_close({k: v for k, v in after_x.items() if k.startswith(R.X_SET)}, xg, 'x-step gradients')
    touched = [k for k in after_y if k.startswith(R.Y_SET) and not np.array_equal(after_x[k], after_y[k])]
    assert not touched, 'the x step changed the gradients of %s' % touched
    have = m.losses()
    for k in R.LOSS_KEYS:
        close(have[k], losses[k], 1e-3, 'loss ' + k)
    assert all(np.array_equal(v0[k], v) for k, v in m.variables().items()) and m.sess.global_step == 0


def sharp_entries(G):
    """(keys, {key: mask}) of the entries whose gradient defines Adam's direction: not a bias in front of a batch norm (its
    gradient is rounding noise in the oracle and on the device alike, and Adam turns the noise's sign into a full step), and
    not within 1e-4 of the variable's largest gradient of zero."""
    keys = [k for k in G if k not in R.dead_biases()]
    return keys, {k: ~((G[k] != 0) & (np.abs(G[k]) <= 1e-4 * np.max(np.abs(G[k])))) for k in keys}


def adam_rule(name, before, after, V, G, quantile=0.02, worst=0.5):
    """The rule of tests/test_gpu_improved_sampler.py::test_train_parity_f32 on one variable set: `before` -> `after` on the device
    against `before` -> V under the float64 Adam with the gradients G.  Where the gradients define Adam's direction the update
    matches to `quantile` lr (2 %) on 99.9 % of the entries and to `worst` lr (1 / 2) on all; every update stays within the step's
    reach (2 lr).  The two defaults presume that both sides took their gradients at the SAME variables."""
    lr, dead = HP['lr'], R.dead_biases()
    fuzzy = {k: (g != 0) & (np.abs(g) <= 1e-4 * np.max(np.abs(g))) for k, g in G.items()}
    # the bias in front of a batch norm has a gradient that is rounding noise in the oracle and on the device alike: Adam turns
    # the noise's sign into a full step, so it defines no direction
    keys = [k for k in G if k not in dead]
    sharp = np.concatenate([~fuzzy[k].ravel() for k in keys])
    errs = {k: np.abs((after[k].astype(np.float64) - before[k]) - (V[k] - before[k])) for k in keys}
    err = np.concatenate([errs[k].ravel() for k in keys])
    assert sharp.mean() > 0.9 and max(float(np.max(np.abs(V[k] - before[k]))) for k in keys) > 0.5 * lr
    print('%s update error 99.9 %% quantile %.3g lr, max %.3g lr' % (name, np.quantile(err[sharp], 0.999) / lr, np.max(err[sharp]) / lr))
    ranked = sorted(((float(np.max(errs[k][~fuzzy[k]])) / lr, k) for k in keys), reverse=True)
    print('   per variable, the largest sharp error in lr: ' + ', '.join('%s %.3g' % (k, e) for e, k in ranked[:4]))
    print('   bounds: %.3g lr at the quantile, %.3g lr at worst' % (quantile, worst))
    assert np.quantile(err[sharp], 0.999) <= quantile * lr and np.max(err[sharp]) <= worst * lr
    assert np.max(err) <= 2.0 * lr + 1e-12
    for k in keys:
        close(after[k], V[k], 1e-3, 'variable ' + k)
    for k in dead & set(G):
        assert np.max(np.abs(G[k])) < 1e-12 and np.max(np.abs(after[k].astype(np.float64) - before[k])) <= 2.0 * lr + 1e-12


@functools.lru_cache(maxsize=None)
def trained():
    """One train() of a fresh model on train_pairs and the oracle's two steps on the same batches: run once, shared, not modified."""
    m = make(use_graphs=False, data=train_pairs(DEV))
    v0 = m.variables()
    src = train_pairs('cpu')
    V, want, grads = R.oracle_train(v0, src.batch(0), src.batch(1), HP['lr'], HP['beta1'], HP['beta2'])
    got = m.train()
    return SimpleNamespace(m=m, v0=v0, v1=m.variables(), V=V, want=want, grads=grads, got=got, src=src)


@pytest.mark.parametrize('which', ['y set', 'x set'])
def test_train_parity_f32(which):
    """Variables after one train() against the oracle's two steps -- the y step on the parity batch, the x step on the next batch
    at the updated encoder -- under a float64 Adam, by adam_rule, per variable set.  The returned dict has exactly x_loss, y_loss;
    global_step advances by 2; both losses within 1e-3.

    The y set: both sides take their gradients at the same initial variables, and the rule holds as it stands (2 % of lr, lr / 2).
    The x set: the x step takes its gradients at the variables AFTER the y step, which differ between a float32 model and the
    float64 oracle by what the y set's rule admits, and the encoder carries that difference into every x gradient.  Its two
    bounds are therefore the reference's OWN error, computed here with the oracle alone (tests/_artist_ref.x_step_reference_error):
    how far the float64 x updates move when nothing but the reference's first step is evaluated and held in float32 (torch on the
    CPU) -- on this data 0.054 lr at the 99.9 % quantile and 1.2 lr at worst, against 0.02 lr and lr / 2, which the reference
    itself therefore misses.  Neither figure comes from the device; the reach of 2 lr that the model's issue names holds for
    every entry in both sets.  The rule at its unchanged bounds is held for the x step where its premise is true, against the
    oracle at the device's own variables after its y step (test_x_step_parity_at_the_device_variables_f32).

    MEASURED (one MI355X, f32): y set 1.35e-4 lr at the quantile, 2.2e-3 lr at worst; x set 0.0322 lr and 0.549 lr; the oracle's x
    gradients at its own variables against the oracle's at the device's give that same 0.0322 lr / 0.548 lr with no device
    arithmetic in the comparison, the two sets of variables differing by at most 5.9e-3 lr after the y step."""
    t = trained()
    m, v0, src = t.m, t.v0, t.src
    after_y = {k: (t.V[k] if k.startswith(R.Y_SET) else v0[k]) for k in v0}               # what the oracle's x step sees
    near, kmin, _ = R.kink_report(after_y, src.batch(1)[0])
    print('x-step batch (seed %d): the nearest lrelu input %.3g from its kink (found: %.3g)' % (TRAIN_X_SEED, kmin, TRAIN_X_FOUND))
    assert not near and kmin > 1e-6, 'the x step\'s batch puts %d lrelu inputs within 1e-6 of a kink: choose other data' % len(near)
    assert list(t.got) == ['x_loss', 'y_loss'] and m.sess.global_step == 2 and m.x_opt.t == 1 and m.y_opt.t == 1 and m.x_y.i == 2
    close(t.got['y_loss'], t.want['y_loss'], 1e-3, 'y_loss')
    close(t.got['x_loss'], t.want['x_loss'], 1e-3, 'x_loss')
    assert abs(t.want['y_loss'] - R.oracle_grads(v0, *src.batch(0))[0]['y_hat_loss']) < 1e-12      # the loss of the pass before the update
    if which == 'y set':
        adam_rule(which, v0, t.v1, t.V, {k: g for k, g in t.grads.items() if k.startswith(R.Y_SET)})
        return
    lr = HP['lr']
    ref_err, G = R.x_step_reference_error(v0, src.batch(0), src.batch(1), lr, HP['beta1'], HP['beta2'])
    keys, sharp = sharp_entries(G)
    ref = np.concatenate([ref_err[k][sharp[k]].ravel() for k in keys])
    q_ref, w_ref = float(np.quantile(ref, 0.999)) / lr, float(np.max(ref)) / lr
    print("the reference's own x-set error with its y step in float32: 99.9 %% quantile %.3g lr, max %.3g lr" % (q_ref, w_ref))
    assert 0.02 < q_ref < 0.2 and w_ref > 0.5                                            # the unchanged bounds are out of the reference's own reach
    adam_rule(which, v0, t.v1, t.V, G, quantile=q_ref, worst=min(w_ref, 2.0))


def test_x_step_parity_at_the_device_variables_f32():
    """The x step after the device's own y step, against the oracle evaluated at the device's variables after that y step: the
    whole of adam_rule on the x set, the x loss within 1e-3, and encoder + y_decoder bit-for-bit untouched by the x step."""
    m = make(use_graphs=False, data=train_pairs(DEV))
    src = train_pairs('cpu')
    m.y_step(m.x_y.next_batch())
    vy = m.variables()
    losses, _, xg, _, _ = R.oracle_grads(vy, *src.batch(1))
    m.x_step(m.x_y.next_batch())
    v1 = m.variables()
    close(m.losses()['x_hat_loss'], losses['x_hat_loss'], 1e-3, 'x_hat_loss')
    V = {k: R.adam_step(vy[k].astype(np.float64), g, HP['lr'], HP['beta1'], HP['beta2']) for k, g in xg.items()}
    adam_rule('x set at the device variables', vy, v1, V, xg)
    assert all(np.array_equal(vy[k], v1[k]) for k in vy if k.startswith(R.Y_SET)) and m.sess.global_step == 2


def test_infer_and_evaluate():
    """infer() against the oracle's forward pass (1e-3); evaluate() over 2 batches against the mean of the oracle's losses; it
    leaves variables, optimizer state, the step counters and losses() untouched."""
    m = make(use_graphs=False)
    m.train()
    v1, last = m.variables(), m.losses()
    slots = {(n, k): t.clone() for n, o in m.optimizers().items() for k, t in o.state_tensors().items()}
    src = R.Batches(B, 4, PARITY_DATA_SEED)
    ref = [R.oracle_grads(v1, *src.batch(k)) for k in (2, 3)]
    x01, y01 = m.infer(m.x_y.batch(2))
    assert tuple(x01.shape) == (B, 256, 256, 3) and tuple(y01.shape) == (B, 256, 256, 1) and x01.dtype == y01.dtype == torch.float32
    assert float(x01.min()) >= 0 and float(x01.max()) <= 1 and float(y01.min()) >= 0 and float(y01.max()) <= 1
    close(x01.cpu().numpy(), ref[0][3], 1e-3, 'infer x_hat')
    close(y01.cpu().numpy(), ref[0][4], 1e-3, 'infer y_hat')
    assert m.x_y.i == 2
    out = m.evaluate(m.x_y, 2)                                                           # batches 2 and 3
    assert list(out) == ['x_hat_loss', 'y_hat_loss', 'y_hat_rmse', 'images', 'n_batches'] and (out['images'], out['n_batches']) == (2 * B, 2)
    for k in R.LOSS_KEYS:
        close(out[k], np.mean([r[0][k] for r in ref]), 1e-3, 'evaluate ' + k)
    assert same(m.losses(), last) and m.sess.global_step == 2 and m.x_opt.t == 1 and m.y_opt.t == 1
    assert all(np.array_equal(v1[k], a) for k, a in m.variables().items())
    assert len(slots) == 4 and all(torch.equal(slots[(n, k)], t) for n, o in m.optimizers().items() for k, t in o.state_tensors().items())
    with pytest.raises(ValueError, match='n_batches must be at least 1'):
        m.evaluate(m.x_y, 0)
    with pytest.raises(ValueError, match='--random_crop 256 256'):
        m.infer((m.x_y.x[0][:, :65, :65], m.x_y.y[0][:, :65, :65]))


# ------------------------------------------------------------------------------------------------ determinism and I/O
def test_graph_replay_matches_eager_bit_for_bit():
    a, b = make(use_graphs=True), make(use_graphs=False)
    for _ in range(3):
        assert a.train() == b.train()
        assert same(a.losses(), b.losses())
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va) and a.sess.global_step == 6 and sorted(a._graphs) == ['a_x_apply', 'a_x_grads', 'a_y_apply', 'a_y_grads']
    for _ in range(3):                                                                   # eager, capture, replay
        ia, ib = a.infer(a.x_y.batch(0)), b.infer(b.x_y.batch(0))
        assert torch.equal(ia[0], ib[0]) and torch.equal(ia[1], ib[1])
    ea, eb = a.evaluate(a.x_y, 3), b.evaluate(b.x_y, 3)
    assert ea == eb and all(np.isfinite(v) for v in ea.values())


def test_checkpoint_resume_is_bit_identical(tmp_path):
    """Checkpoint after one train(), resume into a fresh model with other variables: the next train() is bit-identical; the file
    carries both parts, their betas and both optimizers' slots."""
    ckpt = pkg('checkpoint')
    a = make()
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    z = np.load(path)
    assert {'encoder/vars/e1/weights', 'x_decoder/vars/d6/bias', 'y_decoder/BatchNorm_5/beta', 'encoder/BatchNorm/beta', 'optimizers/x/m',
            'optimizers/y/v', 'optimizers/x/t'} <= set(z.files) and set(R.shapes()) <= set(z.files)
    pos = a.x_y.i
    la = a.train()
    b = make()
    b.load_variables({k: 0.5 * v for k, v in b.variables().items()})
    ckpt.restore(path, b, b.sess)
    assert b.sess.global_step == 2
    b.x_y.i = pos
    assert b.train() == la
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    assert np.any(va['y_decoder/BatchNorm_5/beta'] != 0) and np.any(va['encoder/BatchNorm/beta'] != 0) and np.any(va['x_decoder/BatchNorm/beta'] != 0)


def test_bf16_runs_finite():
    m = make(dtype=1, n_batches=2)
    for _ in range(3):
        losses = m.train()
        assert list(losses) == ['x_loss', 'y_loss'] and all(np.isfinite(v) and v > 0 for v in losses.values()), losses
    assert all(np.isfinite(v) for v in m.losses().values())
    assert all(np.all(np.isfinite(t.cpu().numpy())) for t in m.infer(m.x_y.next_batch()))


def png_header(path):
    raw = open(path, 'rb').read(26)
    assert raw[:8] == b'\x89PNG\r\n\x1a\n' and raw[12:16] == b'IHDR'
    return struct.unpack('>IIBB', raw[16:26])


def test_montages(tmp_path):
    """--examples 4: four PNGs, each a 2 x 2 grid of 256 x 256 images in 8-bit RGB (the depth maps in jet colours)."""
    m = make(examples=4)
    m.train()
    last, v1 = m.losses(), m.variables()
    files = m.write_montages(str(tmp_path), 3)
    assert [os.path.basename(f) for f in files] == ['montage-%s-0003.png' % n for n in ('x', 'y', 'x_hat', 'y_hat')]
    for f in files:
        assert png_header(f) == (512, 512, 8, 2) and os.path.getsize(f) > 1000
    assert same(m.losses(), last) and m.sess.global_step == 2 and all(np.array_equal(v1[k], a) for k, a in m.variables().items())


# ------------------------------------------------------------------------------------------------ the command line
def test_train_cli_synthetic(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    ws = tmp_path / 'ws'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'artist', '--dataset', 'synthetic', '--random_crop', '256', '256',
                        '--batch_size', '4', '--epoch_size', '2', '--optimizer', 'rmsprop', '--lr', '1e-4', '--dir', str(ws)],
                       env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = p.stdout + p.stderr
    assert '2/2' in out.replace(' ', '') and 'Training complete' in out, out[-1500:]
    rows = open(str(ws / 'summaries' / 'losses.csv')).read().split()                     # the default --epochs 3: a row per epoch
    assert rows[0] == 'epoch,x_loss,y_loss' and [r.split(',')[0] for r in rows[1:]] == ['1', '2', '3']
    assert all(np.isfinite(float(v)) and float(v) > 0 for r in rows[1:] for v in r.split(',')[1:])
    z = np.load(str(ws / 'checkpoint-3.npz'))
    assert int(z['global_step']) == 12 and 'encoder/vars/e1/weights' in z.files and 'x_decoder/BatchNorm_5/beta' in z.files
    assert sorted(os.listdir(str(ws / 'summaries'))) == ['losses.csv'] + sorted('montage-%s-%04d.png' % (n, e) for n in ('x', 'x_hat', 'y', 'y_hat')
                                                                                for e in (1, 2, 3))
