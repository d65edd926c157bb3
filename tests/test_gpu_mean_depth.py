"""mean_depth_estimator on the GPU (hem/models/mean_depth_estimator.py): a narrow copy (widths 8, 8, 16, 16, 24, 32, 16; same
names and structure) at B = 4 in f32 against the float64 torch oracle of tests/_mde_ref.py -- predict(), the loss, every
parameter gradient, the variables after three Adam steps --; the full-width model in bf16 through the captured graph;
evaluate(); checkpoint; train.py end to end on synthetic data and on hand-made nyuv2 PNG records."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _mde_frames as F
import _mde_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAME = 'mean_depth_estimator'


def plugin(narrow=True):
    cls = getattr(pkg('models.estimator.' + NAME), NAME)
    return type('narrow', (cls,), {'WIDTHS': R.NARROW}) if narrow else cls


def make(source, B=R.PARITY_B, dtype=0, seed=R.PARITY_SEED, use_graphs=False, narrow=True, hp=R.HP):
    args = SimpleNamespace(batch_size=B, n_gpus=1, seed=seed, use_graphs=use_graphs, m_arch='E2', decay=0.9, momentum=0.01,
                           centered=False, **hp)
    sess = pkg('runtime').Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    return plugin(narrow)(source, args, sess)


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / np.max(np.abs(b)))


def held(got, ref, ref32, what, report):
    """The standing rule of the depth models: max |err| / max |ref| within max(1e-3, 3 x the oracle's own float32 deviation)."""
    err, bound = relerr(got, ref), max(1e-3, 3.0 * relerr(ref32, ref))
    report.append('%s %.1e (%.1e)' % (what, err, bound))
    assert err <= bound, '%s: %g above %g' % (what, err, bound)


def short(k):
    return '.'.join(k.split('/')[-2:])


# ------------------------------------------------------------------------------------------------ parity with the oracle
def test_narrow_model_parity_f32():
    """predict() on batch 0; then three train() calls on batches 1..3: each returned loss, the gradients of the first step and the
    variables after the third against the float64 oracle, each tensor by the rule of `held`.  The oracle's own conditions -- every
    |mean_i - m_i| above 0.05, the small layers' relu inputs 1e-6 away from zero at every step -- are asserted first (and, without
    a GPU, by tests/test_host_mean_depth.py)."""
    src = R.Originals(R.PARITY_B, R.PARITY_STEPS + 1, R.PARITY_SEED, DEV)
    m = make(src)
    v0 = m.variables()
    want0 = R.initial_variables(plugin(), R.PARITY_SEED)
    assert list(v0) == R.names() and all(np.array_equal(v0[k], want0[k]) for k in v0)
    assert [p.name for p in m.parts] == ['model'] and type(m.opt).__name__ == 'Adam'
    batches = [(src.x[i], src.y[i]) for i in range(1, R.PARITY_STEPS + 1)]
    steps, v_end = R.trajectory(v0, batches)
    steps32, v_end32 = R.trajectory(v0, batches, dtype=torch.float32)
    for (v, _, _, mm, means), (x, _) in zip(steps, batches):
        assert np.abs(means - mm).min() > 0.05, 'a mean depth within 0.05 of the prediction: choose other data'
        assert R.nearest_kink(v, x) > 1e-6, 'a small layer at a relu kink: choose other data'
    report = []
    # predict
    x0 = src.next_batch()[0]
    assert R.nearest_kink(v0, x0) > 1e-6
    with torch.no_grad():
        p64 = R.forward(R.tensors(v0), x0.cpu().double()).numpy()
        p32 = R.forward(R.tensors(v0, torch.float32), x0.cpu()).double().numpy()
    got = m.predict(x0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (R.PARITY_B,)
    held(got.cpu().numpy(), p64, p32, 'predict', report)
    # the first step: loss and gradients
    losses = [m.train()]
    assert list(losses[0]) == ['Mean_1']
    grads = m.gradients()
    assert set(grads) == set(steps[0][2])
    for k, r in steps[0][2].items():
        assert np.any(r != 0), '%s: the reference gradient is identically zero' % k
        held(grads[k], r, steps32[0][2][k], 'd' + short(k), report)
    np.testing.assert_allclose(m.mean.cpu().numpy(), steps[0][4], rtol=1e-6, atol=0)
    # two more steps: the losses at the variables before each update, the variables after three
    losses += [m.train() for _ in range(R.PARITY_STEPS - 1)]
    for t, (l, s, s32) in enumerate(zip(losses, steps, steps32)):
        held(l['Mean_1'], np.float64(s[1]), np.float64(s32[1]), 'loss%d' % t, report)
    l_skipped = R.oracle_grads(v0, *batches[1])[0]
    assert abs(l_skipped - steps[1][1]) > 3e-3 * steps[1][1], 'the update does not show in the second loss: choose another --lr'
    v3 = m.variables()
    for k in v0:
        held(v3[k], v_end[k], v_end32[k], short(k), report)
        assert np.any(v3[k] != v0[k])
    assert m.opt.t == R.PARITY_STEPS and m.sess.global_step == R.PARITY_STEPS
    print('max |err| / max |ref| per tensor (bound): ' + ', '.join(report))


def test_graph_replay_matches_eager_bit_for_bit():
    a = make(R.Originals(4, 4, 1, DEV), use_graphs=True)
    b = make(R.Originals(4, 4, 1, DEV), use_graphs=False)
    for _ in range(4):                                           # eager, capture, two replays
        assert a.train() == b.train()
    assert 'm_grads' in a._graphs and 'm_apply' in a._graphs and not b._graphs
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


# ------------------------------------------------------------------------------------------------ the full-width model
def test_full_width_bf16_trains_through_the_captured_graph():
    """The real E2 (78 M parameters, filters up to 5x5x1024x2048) at B = 2 in bf16: the first train() runs eagerly, the second is
    captured and replayed; both losses are finite and lie in (0, 1), and the step count follows."""
    data = pkg('data')
    m = make(data.SyntheticEstimatorSource(2, 2, DEV), B=2, dtype=1, use_graphs=True, narrow=False)
    assert m.store.num_params() == 78_238_337
    first = m.train()
    assert not m._graphs
    second = m.train()
    assert 'm_grads' in m._graphs and 'm_apply' in m._graphs
    for l in (first, second):
        assert list(l) == ['Mean_1'] and np.isfinite(l['Mean_1']) and 0 < l['Mean_1'] < 1, l
    assert m.opt.t == 2 and bool(torch.isfinite(m.store.params).all()) and bool(torch.isfinite(m.last.out).all())


# ------------------------------------------------------------------------------------------------ evaluate, checkpoint
def test_evaluate_is_the_mean_of_the_batches_errors():
    data = pkg('data')
    m = make(data.SyntheticEstimatorSource(3, 4, DEV), use_graphs=True)
    v0 = m.variables()
    got = m.evaluate(data.SyntheticEstimatorSource(3, 4, DEV), 3)
    assert set(got) == {'mean_abs_error', 'images', 'n_batches'} and (got['images'], got['n_batches']) == (12, 3)
    twin, per_batch = data.SyntheticEstimatorSource(3, 4, DEV), []
    for _ in range(3):
        b = twin.next_batch()
        per_batch.append(float((b[5].double().mean(dim=(1, 2, 3)) - m.predict(b[4]).double()).abs().mean()))
    want = float(np.mean(per_batch))
    print('mean_abs_error %.9g, from predict() %.9g' % (got['mean_abs_error'], want))
    assert len(set(per_batch)) == 3 and abs(got['mean_abs_error'] - want) <= 1e-6 * want
    assert all(np.array_equal(v, v0[k]) for k, v in m.variables().items()) and m.sess.global_step == 0
    with pytest.raises(ValueError, match='n_batches'):
        m.evaluate(twin, 0)
    with pytest.raises(ValueError, match='--include_originals 53 70'):
        m.evaluate(pkg('data').SyntheticPairSource(1, 4, DEV, 65), 1)


def test_checkpoint_into_a_fresh_replica_predicts_bit_equal(tmp_path):
    ckpt = pkg('checkpoint')
    a = make(R.Originals(4, 4, 2, DEV))
    a.train()
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    x = a.x_y.x[3]
    b = make(R.Originals(4, 4, 2, DEV), seed=11)
    assert not torch.equal(a.predict(x), b.predict(x))
    ckpt.restore(path, b, b.sess)
    assert torch.equal(a.predict(x), b.predict(x)) and b.opt.t == 2 and b.sess.global_step == 2
    b.x_y.i = a.x_y.i
    assert a.train() == b.train()                                # the optimizer slots came along


# ------------------------------------------------------------------------------------------------ the command line
def _train(tmp_path, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    ws = str(tmp_path / 'ws')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', NAME, '--epoch_size', '2', '--batch_size', '8',
                        '--epochs', '1', '--dir', ws] + list(argv), env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    out = p.stdout + p.stderr
    assert '2/2' in out.replace(' ', '') and 'Training complete' in out, out[-1500:]
    rows = open(os.path.join(ws, 'summaries', 'losses.csv')).read().split()
    assert rows[0] == 'epoch,Mean_1' and len(rows) == 2 and 0 < float(rows[1].split(',')[1]) < 1, rows
    assert os.path.exists(os.path.join(ws, 'checkpoint-1.npz'))
    return out


def test_train_cli_on_synthetic_data(tmp_path):
    _train(tmp_path, '--dataset', 'synthetic')


def test_train_cli_on_nyuv2_png_records(tmp_path):
    rgb, depth = F.frames(10)
    F.write_tfrecords(str(tmp_path / 'datasets' / 'nyuv2.train.tfrecords'), rgb, depth)
    out = _train(tmp_path, '--dataset', 'nyuv2', '--dataset_dir', str(tmp_path / 'datasets'), '--random_crop', '65', '65',
                 '--include_location', '--include_originals', '53', '70')
    assert 'ignored' not in out
