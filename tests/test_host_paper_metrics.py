"""paper_cgan dataset evaluation without a GPU (paper/paper_metrics.py, the mean / variance image pre-pass of
paper/paper_train.py): the float64 NumPy restatement of a sweep that the GPU tests check the kernels and evaluate() against,
held to hand-computed values here; the new entry points' exports and argument checks; the paper_metrics.py command line and
its report."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT
from test_host_paper_cgan import eigen_metrics

KEYS = ('abs_rel_diff', 'squared_rel_diff', 'linear_rmse', 'log_rmse', 'scale_invariant_log_rmse', 'threshold1', 'threshold2',
        'threshold3')


# ------------------------------------------------------------------------------------------------ the restatement
def sweep_set(ys, preds):
    """One metric set over a sweep (paper_metrics.py:24-34,119-130): per batch the eight values of eigen_metrics with the
    threshold totals running from zero, then the plain mean over the batches -- for t1..t3 the mean of the RUNNING
    percentage; `threshold{k}_final` are the totals' percentages after the last batch.  Returns (dict, counts)."""
    counts = [0, 0, 0, 0]
    rows = []
    for y, p in zip(ys, preds):
        m = eigen_metrics(np.asarray(y, np.float64), np.asarray(p, np.float64), counts)
        rows.append([m[k] for k in KEYS])
    with np.errstate(invalid='ignore'):
        out = dict(zip(KEYS, np.mean(np.array(rows, np.float64), axis=0).tolist()))
    out.update({'threshold%d_final' % (k + 1): counts[k] / counts[3] for k in range(3)})
    return out, counts


def batch_moments(ys):
    """paper_train.py:43-50 on tf.nn.moments(y, axes=0): per batch the mean and the mean squared deviation from it over the
    batch axis, both averaged over the batches."""
    ys = [np.asarray(y, np.float64) for y in ys]
    return np.mean([y.mean(0) for y in ys], axis=0), np.mean([y.var(0) for y in ys], axis=0)


def sweep_reference(crops, yhats, ybars, version, crops2):
    """evaluate() restated: crops / crops2 f32 [B,29,29] (10x depth) of sweep 1 / sweep 2, yhats f32 [B,29,29], ybars f32 [B].
    zero: 0 for baseline (version 0), y_bar otherwise; mean: 10 * the f32 mean image of the [0, 1] crops, in f32."""
    mean, var = batch_moments([np.asarray(c, np.float64) / 10.0 for c in crops])
    y0 = [np.zeros_like(c) if version == 0 else np.broadcast_to(np.asarray(b)[:, None, None], c.shape) for c, b in zip(crops, ybars)]
    pm = np.float32(10.0) * mean.astype(np.float32)
    return {'model': sweep_set(crops, yhats)[0], 'zero': sweep_set(crops, y0)[0],
            'mean': sweep_set(crops2, [np.broadcast_to(pm, c.shape) for c in crops2])[0], 'mean_image': mean, 'var_image': var}


def test_running_percentage_mean_known_answer():
    """Batches with 1 of 2, then 2 of 2 elements below 1.25: the running percentage is 0.5, then 0.75: mean 0.625, final 0.75."""
    ys = [np.array([1.0, 1.0]), np.array([1.0, 1.0])]
    ps = [np.array([1.0, 2.0]), np.array([1.0, 1.1])]
    out, counts = sweep_set(ys, ps)
    assert out['threshold1'] == 0.625 and out['threshold1_final'] == 0.75
    assert counts == [3, 3, 3, 4]
    # ratio 2 is above 1.25^3 = 1.953 as well
    assert out['threshold3'] == 0.625 and out['threshold3_final'] == 0.75
    # the other five are plain means of the per-batch values: batch 1 |0.1-0.2|/0.2 = 0.5 on one of two elements
    assert math.isclose(out['abs_rel_diff'], (0.25 + (0.01 / 0.11) / 2) / 2, rel_tol=1e-12)
    a = np.array([0.1, 0.1])
    rm = [np.sqrt(np.mean((a - np.array(p) / 10) ** 2)) for p in ps]
    assert math.isclose(out['linear_rmse'], np.mean(rm), rel_tol=1e-12)


def test_key_order_is_the_plugins():
    assert KEYS == tuple(pkg('models.paper.paper_cgan').METRIC_KEYS)
    out, _ = sweep_set([np.ones(2)], [np.ones(2)])
    assert list(out) == list(KEYS) + ['threshold1_final', 'threshold2_final', 'threshold3_final']


def test_non_finite_values_stay_visible():
    """A zero prediction: inf where the formulas divide by it, in the batch and therefore in the mean (no Counter filter)."""
    out, _ = sweep_set([np.array([1.0, 2.0]), np.array([1.0, 2.0])], [np.array([1.0, 2.0]), np.zeros(2)])
    assert np.isinf(out['abs_rel_diff']) and np.isinf(out['squared_rel_diff'])
    d = np.log(np.array([0.1, 0.2]) + 1e-8) - np.log(1e-8)         # the log terms stay finite: log(0 + 1e-8)
    assert math.isclose(out['log_rmse'], np.sqrt(np.mean(d ** 2)) / 2, rel_tol=1e-12)
    assert math.isclose(out['scale_invariant_log_rmse'], (np.mean(d ** 2) - d.sum() ** 2 / 4) / 2, rel_tol=1e-9)
    assert out['threshold1'] == (1.0 + 0.5) / 2 and out['threshold1_final'] == 0.5
    assert math.isclose(out['linear_rmse'], np.sqrt((0.01 + 0.04) / 2) / 2)


def test_moments_known_answer():
    """tf.nn.moments on a 2-image batch: mean (a+b)/2, variance ((a-b)/2)^2; then the mean over two batches of each."""
    b1 = np.array([[1.0, 4.0], [3.0, 0.0]])
    b2 = np.array([[2.0, 2.0], [2.0, 6.0]])
    mean, var = batch_moments([b1])
    assert np.array_equal(mean, [2.0, 2.0]) and np.array_equal(var, [1.0, 4.0])
    mean, var = batch_moments([b1, b2])
    assert np.array_equal(mean, [2.0, 3.0]) and np.array_equal(var, [0.5, 4.0])


def test_sweep_reference_sets():
    rng = np.random.default_rng(0)
    crops = [rng.uniform(1, 9, (2, 29, 29)).astype(np.float32) for _ in range(2)]
    crops2 = [rng.uniform(1, 9, (2, 29, 29)).astype(np.float32) for _ in range(2)]
    yh = [c * np.float32(1.1) for c in crops]
    yb = [c.mean((1, 2)) for c in crops]
    r0, r1 = sweep_reference(crops, yh, yb, 0, crops2), sweep_reference(crops, yh, yb, 1, crops2)
    assert np.isinf(r0['zero']['abs_rel_diff']) and np.isfinite(r1['zero']['abs_rel_diff'])
    assert r0['model'] == r1['model'] and r0['mean'] == r1['mean']                # y_bar is never added to model / mean
    assert r0['model']['threshold1'] == 1.0 and math.isclose(r0['model']['abs_rel_diff'], 0.1 / 1.1, rel_tol=1e-5)
    assert r0['mean_image'].shape == (29, 29) and 0.1 < r0['mean_image'].min() and r0['mean_image'].max() < 0.9


# ------------------------------------------------------------------------------------------------ the library
NEW = ('tdg_cgan_eval_batch', 'tdg_cgan_eval_workspace_bytes', 'tdg_cgan_eval_acc_bytes', 'tdg_cgan_eval_moments',
       'tdg_cgan_eval_finish')


def test_library_exports_the_eval_entry_points():
    L = pkg('_lib')
    L.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tdg.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(tdg_[a-z0-9_]+)\s*\(', text))
    exported = set(re.findall(r' T (tdg_[a-z0-9_]+)', subprocess.check_output(['nm', '-D', '--defined-only', L.LIB_PATH]).decode()))
    assert set(NEW) <= declared and set(NEW) <= set(L.SIGNATURES) and set(NEW) <= exported
    assert declared == set(L.SIGNATURES)


def test_eval_sizes():
    lib = pkg('_lib').load()
    assert lib.tdg_cgan_eval_workspace_bytes() == 3 * lib.tdg_cgan_metrics_workspace_bytes()      # a partial per set and block
    assert lib.tdg_cgan_eval_acc_bytes(841) == (27 + 1 + 2 * 841) * 8
    assert lib.tdg_cgan_eval_acc_bytes(0) == 0


def test_eval_kernels_report_bad_arguments():
    """Status + tdg_last_error() before any launch."""
    lib = pkg('_lib').load()
    p = C.c_void_p(4096)                                         # never dereferenced: every call below fails its checks
    big = lib.tdg_cgan_eval_workspace_bytes()
    assert lib.tdg_cgan_eval_batch(p, p, p, p, 1.0, 4, 841, 0, p, p, p, big, None) == -1 and b'eval_batch' in lib.tdg_last_error()
    assert lib.tdg_cgan_eval_batch(p, p, p, p, 1.0, 4, 841, 8, p, p, p, big, None) == -1
    assert lib.tdg_cgan_eval_batch(p, None, p, p, 1.0, 4, 841, 1, p, p, p, big, None) == -1          # set 1 needs pred
    assert lib.tdg_cgan_eval_batch(p, p, p, None, 1.0, 4, 841, 4, p, p, p, big, None) == -1          # set 4 needs the image
    assert lib.tdg_cgan_eval_batch(None, p, p, p, 1.0, 4, 841, 7, p, p, p, big, None) == -1
    assert lib.tdg_cgan_eval_batch(p, p, p, p, 1.0, 0, 841, 7, p, p, p, big, None) == -1
    assert lib.tdg_cgan_eval_batch(p, p, p, p, 1.0, 4, 841, 7, p, p, p, big - 1, None) != 0 and b'workspace' in lib.tdg_last_error()
    assert lib.tdg_cgan_eval_moments(None, 4, 841, p, None) == -1 and b'moments' in lib.tdg_last_error()
    assert lib.tdg_cgan_eval_moments(p, 0, 841, p, None) == -1
    assert lib.tdg_cgan_eval_finish(p, p, 841, 10.0, p, p, None, None) == -1 and b'finish' in lib.tdg_last_error()
    assert lib.tdg_cgan_eval_finish(p, p, 841, 0.0, p, p, p, None) == -1
    assert lib.tdg_cgan_eval_finish(None, p, 841, 10.0, p, p, p, None) == -1


# ------------------------------------------------------------------------------------------------ the model surface
def test_model_has_the_evaluation_methods():
    cls = pkg('models.paper.paper_cgan').paper_cgan
    for name in ('set_mean_image', 'dataset_moments', 'evaluate'):
        assert callable(getattr(cls, name))


def test_nyuv2_source_takes_a_split():
    import inspect
    sig = inspect.signature(pkg('data_plugins.nyuv2').NYUv2Dataset.get_source)
    assert list(sig.parameters) == ['args', 'sess', 'split'] and sig.parameters['split'].default == 'train'


# ------------------------------------------------------------------------------------------------ the command line
def cli():
    return __import__('paper_metrics')


def test_cli_defaults_and_flags():
    a = cli().parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--dir', 'w'])
    assert a.splits == ['validate', 'train'] and a.n_batches is None and a.no_images is False and a.dir == 'w'
    a = cli().parse_args(['--model', 'paper_cgan', '--dataset', 'nyuv2', '--splits', 'test', '--n_batches', '3', '--no_images',
                          '--batch_size', '64', '--model_version', 'mean_adjusted'])
    assert (a.splits, a.n_batches, a.no_images, a.batch_size, a.model_version) == (['test'], 3, True, 64, 'mean_adjusted')
    assert cli().batches_of(a, 1000) == 3
    a.n_batches = None
    assert cli().batches_of(a, 1000) == 15 and cli().batches_of(a, 10) == 1


def test_cli_rejects():
    with pytest.raises(SystemExit, match='paper_metrics'):
        cli().parse_args(['--model', 'pix2pix', '--dataset', 'synthetic'])
    with pytest.raises(SystemExit):
        cli().parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--n_batches', '0'])
    with pytest.raises(SystemExit):
        cli().parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--splits', 'nowhere'])


def test_cli_reads_the_training_options(tmp_path):
    """`@<dir>/options.config` as train.py writes it rebuilds the trained model's arguments; flags after it win."""
    import train
    ws = str(tmp_path / 'ws')
    opts = str(tmp_path / 'options.config')
    args = train.parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--batch_size', '8', '--epoch_size', '2', '--epochs', '1',
                             '--model_version', 'mean_adjusted', '--precision', 'f32', '--seed', '5', '--dir', ws])
    with open(opts, 'w') as f:
        for k in vars(args):
            if k != 'config':
                f.write('{} {}\n'.format(k, getattr(args, k)))
    a = cli().parse_args(['@' + opts, '--dir', ws, '--splits', 'train', '--n_batches', '2'])
    assert (a.model, a.dataset, a.batch_size, a.model_version, a.precision, a.seed) == ('paper_cgan', 'synthetic', 8, 'mean_adjusted',
                                                                                        'f32', 5)
    assert (a.dir, a.splits, a.n_batches) == (ws, ['train'], 2)


def test_cli_without_checkpoint_exits(tmp_path):
    with pytest.raises(SystemExit, match='no checkpoint'):
        cli().main(['--model', 'paper_cgan', '--dataset', 'synthetic', '--dir', str(tmp_path)])


def test_report_format():
    """The reference's block (:128-130): t1, t2, t3, then the five others, a tab and three decimals; NaN / inf are printed."""
    vals = dict(zip(KEYS, [0.1234, 0.05, 1.0, 0.4446, float('nan'), 0.5, 0.75, 0.8756]))
    got = cli().format_block('Model metrics:', vals)
    assert got == ('Model metrics:\n\tt1: 0.500\n\tt2: 0.750\n\tt3: 0.876\n\tabs_rel_diff: 0.123\n\tsquared_rel_diff: 0.050\n'
                   '\tlinear_rmse: 1.000\n\tlog_rmse: 0.445\n\tscale_invariant_log_rmse: nan')
    rep = cli().format_report({'model': vals, 'mean': vals, 'zero': dict(vals, abs_rel_diff=float('inf'))})
    assert [l for l in rep.split('\n') if not l.startswith('\t')] == ['Model metrics:', 'Mean metrics:', 'Zero metrics:']
    assert '\tabs_rel_diff: inf' in rep.split('Zero metrics:')[1]


def test_record_holds_the_scalars():
    res = {'model': {'a': 1.0}, 'zero': {'a': 2.0}, 'mean': {'a': 3.0}, 'n_batches': 4, 'images': 32, 'mean_image': np.zeros((29, 29)),
           'var_image': np.zeros((29, 29))}
    rec = cli().record('validate', '/some/dir/checkpoint-7.npz', res)
    assert rec == {'split': 'validate', 'checkpoint': 'checkpoint-7.npz', 'n_batches': 4, 'images': 32, 'model': {'a': 1.0},
                   'zero': {'a': 2.0}, 'mean': {'a': 3.0}}
