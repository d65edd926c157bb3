"""paper_standalone / paper_baseline_standalone on the GPU (hem/models/paper_standalone.py): the model against the float64
torch-autograd oracle of tests/_standalone_ref.py, two consecutive train() calls against torch.optim.Adam, graph replay,
determinism, checkpoint / resume, bf16 runs, metrics(), evaluate(), infer_full(), the command line, and a regression guard
for the sampler plugins, whose executor the fed channel touches."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _standalone_ref as R
from test_gpu_paper_cgan import close, eigen_ref, Batches, DEV
from test_gpu_paper_metrics import source, crop_of, check_result
from test_host_paper_metrics import sweep_reference
from test_gpu_paper_cgan_fullimage import chunked_infer, reconstruct, rmse, frame, grid

pytestmark = pytest.mark.gpu
HP = dict(g_lr=1e-3, g_beta1=0.9, g_beta2=0.999)
KEYS = pkg('models.paper.paper_cgan').METRIC_KEYS


def make(version, B=4, dtype=0, seed=0, use_graphs=True, n_batches=8, data_seed=None, hp=HP, model='paper_standalone'):
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version=version, seed=seed, use_graphs=use_graphs, **hp)
    sess = pkg('runtime').Session(device=DEV, dtype=dtype, seed=seed, rank=0, world_size=1)
    cls = getattr(pkg('models.standalone.' + model), model)
    return cls(Batches(B, n_batches, seed if data_seed is None else data_seed), args, sess)


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / np.max(np.abs(b)))


# ------------------------------------------------------------------------------------------------ parity with the oracle
PARITY = [('paper_standalone', v) for v in R.VERSIONS] + [('paper_baseline_standalone', 'mean_provided')]
PARITY_DATA_SEED = 0             # the first seed whose batches keep e3, e4 and d1 1e-6 away from their kinks, for every version


@pytest.mark.parametrize('model,version', PARITY)
def test_model_parity_f32(model, version):
    """infer() on batch 0, then one train() on batch 1: the returned loss and every generator gradient against the float64
    oracle.  Per tensor, max |err| / max |ref| within max(1e-3, 3 x the oracle's own float32-vs-float64 deviation on that
    tensor), as tests/test_gpu_paper_sampler.py::test_model_parity_f32.  The batches must keep the small layers (e3, e4, d1: at
    most 100 positions per channel at B = 4) 1e-6 away from their relu / lrelu kinks (_standalone_ref.nearest_kink), 25 times
    what the oracle's float32 inputs deviate; asserted on the oracle alone."""
    m = make(version, use_graphs=False, data_seed=PARITY_DATA_SEED, model=model)
    v0 = m.variables()
    assert not any(k.startswith('discriminator/') for k in v0) and [p.name for p in m.parts] == ['generator']
    b0 = m.x_y.next_batch()
    assert R.nearest_kink(v0, b0, version) > 1e-6, 'batch 0 puts a small layer at a kink: choose other data'
    _, _, yh = R.oracle_grads(v0, b0, version)
    _, _, yh32 = R.oracle_grads(v0, b0, version, dtype=torch.float32)
    err, bound = relerr(m.infer(b0).cpu().numpy(), yh), max(1e-3, 3.0 * relerr(yh32, yh))
    print('%s %s infer: %.1e (%.1e)' % (model, version, err, bound))
    assert err <= bound
    b1 = (m.x_y.x[1], m.x_y.y[1])
    kink = R.nearest_kink(v0, b1, version)
    assert kink > 1e-6, 'the step\'s batch puts a small layer %g from a kink: choose other data' % kink
    losses = m.train()
    assert list(losses) == ['rmse']
    ref_l, ref, _ = R.oracle_grads(v0, b1, version)
    _, ref32, _ = R.oracle_grads(v0, b1, version, dtype=torch.float32)
    print('%s %s loss %.9g (oracle %.9g)' % (model, version, losses['rmse'], ref_l))
    assert abs(losses['rmse'] - ref_l) <= 1e-3 * ref_l
    got = m.gradients()
    assert set(got) == set(ref)
    report = []
    for k, r in ref.items():
        assert np.any(r != 0), '%s: the reference gradient is identically zero' % k
        err, bound = relerr(got[k], r), max(1e-3, 3.0 * relerr(ref32[k], r))
        report.append('%s %.1e (%.1e)' % ('.'.join(k.split('/')[-3:]).replace('vars.', ''), err, bound))
        assert err <= bound, '%s: %g above %g' % (k, err, bound)
    print('%s %s, max |err| / max |ref| per tensor (bound): %s' % (model, version, ', '.join(report)))
    if version == 'mean_provided':
        assert v0['generator/encoder/vars/e2/weights'].shape == (5, 5, 65, 128)
        assert v0['generator/decoder/vars/d4/weights'].shape == (1, 1, 129, 1)
        assert np.any(ref['generator/decoder/vars/d4/weights'][0, 0, 128] != 0)      # dW[128] = sum dg * y_bar


@pytest.mark.parametrize('version', ['mean_adjusted', 'mean_provided'])
def test_two_train_calls_update_and_fetch_order(version):
    """The first returned rmse is batch 1's at the initial variables, the second is batch 2's at the variables after ONE Adam
    step (torch.optim.Adam in float64), both within 1e-3 relative.  g_lr = 1e-3: on the oracle, skipping the update moves the
    second loss by at least ten times that bound, so a run without an optimizer step fails."""
    m = make(version, use_graphs=False)
    v0 = m.variables()
    b = [(m.x_y.x[i], m.x_y.y[i]) for i in range(2)]
    l1, g, _ = R.oracle_grads(v0, b[0], version)
    v1 = {k: R.adam_first_step(v0[k], g[k], HP['g_lr'], HP['g_beta1'], HP['g_beta2']) for k in v0}
    l2, _, _ = R.oracle_grads(v1, b[1], version)
    l2_skipped, _, _ = R.oracle_grads(v0, b[1], version)
    assert abs(l2_skipped - l2) >= 10 * 1e-3 * l2, 'the update does not show in the second loss: choose another --g_lr'
    got1, got2 = m.train()['rmse'], m.train()['rmse']
    print('%s: rmse %.9g, %.9g; oracle %.9g, %.9g (update skipped: %.9g)' % (version, got1, got2, l1, l2, l2_skipped))
    assert abs(got1 - l1) <= 1e-3 * l1
    assert abs(got2 - l2) <= 1e-3 * l2
    assert m.g_opt.t == 2 and m.sess.global_step == 2


# ------------------------------------------------------------------------------------------------ behaviour
@pytest.mark.parametrize('version', ['mean_adjusted', 'mean_provided'])
def test_graph_replay_matches_eager_bit_for_bit(version):
    a, b = make(version, use_graphs=True), make(version, use_graphs=False)
    for _ in range(4):                                           # eager, capture, two replays
        assert a.train() == b.train()
    assert 'g_grads' in a._graphs and 'g_apply' in a._graphs and not b._graphs
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


def test_two_fresh_models_are_bit_equal():
    a, b = make('mean_provided', seed=3), make('mean_provided', seed=3)
    for _ in range(3):
        assert a.train() == b.train()
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    ma, mb = a.metrics(), b.metrics()
    for k in ma:
        assert np.array_equal(list(ma[k].values()), list(mb[k].values()), equal_nan=True)


def test_checkpoint_resume_is_bit_identical(tmp_path):
    ckpt = pkg('checkpoint')
    a = make('mean_provided')
    a.train()
    path = str(tmp_path / 'checkpoint-1.npz')
    ckpt.save(path, a, a.sess)
    pos = a.x_y.i
    la = a.train()
    assert max(float(np.max(np.abs(v))) for v in a.gradients().values()) > 1e-6
    b = make('mean_provided', seed=11, data_seed=0)
    assert any(not np.array_equal(b.variables()[k], v) for k, v in a.variables().items())
    ckpt.restore(path, b, b.sess)
    b.x_y.i = pos
    assert b.train() == la
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)


@pytest.mark.parametrize('version', R.VERSIONS)
def test_bf16_runs_finite(version):
    m = make(version, B=8, dtype=1, n_batches=4)
    for _ in range(5):
        losses = m.train()
        assert np.isfinite(losses['rmse']) and losses['rmse'] > 0, losses
    assert all(np.all(np.isfinite(v)) for v in m.variables().values())
    assert np.all(np.isfinite(m.infer(m.x_y.next_batch()).cpu().numpy()))


@pytest.mark.parametrize('version', ['baseline', 'mean_provided'])
def test_metrics_sets(version):
    """metrics_y_hat and metrics_y_0 of the last loss fetch, metrics_y_mean once a mean image is set: tdg_cgan_metrics' NumPy
    statement (test_host_paper_cgan.eigen_metrics) on the fetched batch."""
    m = make(version)
    m.train()
    crop, yhat, ybar = m.crop.cpu().numpy(), m.yhat.cpu().numpy(), m.ybar.cpu().numpy()
    m.infer(m.x_y.next_batch())                                   # infer() does not touch the fetch's buffers
    got = m.metrics()
    assert list(got) == ['metrics_y_hat', 'metrics_y_0'] and list(got['metrics_y_hat']) == list(KEYS)
    counts, c0, cm = [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]
    close([got['metrics_y_hat'][k] for k in KEYS], eigen_ref(crop, yhat, counts), 1e-4, 'y_hat set')
    y_0 = np.zeros_like(crop) if version == 'baseline' else np.broadcast_to(ybar[:, None, None], crop.shape)
    close([got['metrics_y_0'][k] for k in KEYS], eigen_ref(crop, y_0, c0), 1e-4, 'y_0 set')
    img = np.random.default_rng(3).uniform(0.05, 0.95, (29, 29)).astype(np.float32)
    m.set_mean_image(img)
    got = m.metrics()
    assert list(got) == ['metrics_y_hat', 'metrics_y_0', 'metrics_y_mean']
    close([got['metrics_y_mean'][k] for k in KEYS], eigen_ref(crop, np.broadcast_to(np.float32(10.0) * img, crop.shape), cm), 1e-4, 'y_mean')


@pytest.mark.parametrize('version', ['mean_adjusted', 'mean_provided'])
def test_evaluate_against_infer_and_the_restatement(version):
    """As tests/test_gpu_paper_metrics.py checks paper_cgan: evaluate() over 2 + 2 batches of a seeded source, recomputed from
    infer()'s own y_hat of the same batches through the restatement."""
    B, n = 4, 2
    m = make(version, B=B)
    got = m.evaluate(source(B), n)
    assert (got['n_batches'], got['images']) == (n, n * B)
    twin = source(B)
    crops, yhats, ybars, crops2 = [], [], [], []
    for _ in range(n):
        x, y = twin.next_batch()
        yhats.append(m.infer((x, y))[..., 0].cpu().numpy())
        c, yb = crop_of(y)
        crops.append(c)
        ybars.append(yb)
    for _ in range(n):
        crops2.append(crop_of(twin.next_batch()[1])[0])
    check_result(got, sweep_reference(crops, yhats, ybars, 1, crops2), version)       # (1: y_0 = y_bar)
    assert all(np.isfinite(v) for v in got['zero'].values()) and all(np.isfinite(v) for v in got['mean'].values())


@pytest.mark.parametrize('version', ['mean_adjusted', 'mean_provided'])
def test_infer_full_matches_infer_f32(version):
    """As tests/test_gpu_paper_cgan_fullimage.py checks paper_cgan.  A 94 x 100 frame holds (94 - 93) // 3 = 0 windows down at
    stride 3 -- refused, as by paper_cgan -- so the canvases are checked on a 100 x 112 frame at stride 3 (2 x 6 windows)."""
    m = make(version, B=8)
    image, depth = frame(94, 100, 2)
    with pytest.raises(ValueError, match='no 65x65 window'):
        m.infer_full(image, depth, stride=3)
    assert m.infer_full(image, depth, stride=1).patches == 7
    H, W, s = 100, 112, 3
    image, depth = frame(H, W, 2)
    r = m.infer_full(image, depth, stride=s)
    assert r.patches == grid(H, W, s).patches == 12 and r.grid == (2, 6)
    yh, ybar, P, xb = chunked_infer(m, image, depth, s)
    assert np.array_equal(r.y_hat.cpu().numpy(), reconstruct(H, W, yh, s).astype(np.float32))
    assert np.array_equal(r.g.cpu().numpy(), reconstruct(H, W, yh - ybar[:, None, None], s).astype(np.float32))
    ref = rmse(depth[..., None], r.y_hat.cpu().numpy().astype(np.float64)[..., None])
    assert abs(r.rmse - ref) <= 1e-12 * ref


# ------------------------------------------------------------------------------------------------ the command line
def test_train_and_paper_metrics_cli(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    ws = str(tmp_path / 'ws')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_standalone', '--model_version', 'mean_provided',
                        '--dataset', 'synthetic', '--batch_size', '8', '--epoch_size', '2', '--epochs', '1', '--dir', ws],
                       env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    assert '2/2' in (p.stdout + p.stderr).replace(' ', ''), (p.stdout + p.stderr)[-1500:]
    assert os.path.exists(os.path.join(ws, 'checkpoint-1.npz'))
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'paper_metrics.py'), '@' + os.path.join(ws, 'options.config'), '--dir', ws,
                        '--no_images'], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert lines and all(d['checkpoint'] == 'checkpoint-1.npz' and d['images'] == d['n_batches'] * 8 for d in lines)
    assert all(np.isfinite(d['model']['linear_rmse']) for d in lines)


# ------------------------------------------------------------------------------------------------ regression guard
def test_sampler_plugins_compute_what_the_parent_commit_computed():
    """tests/golden/sampler_parent_digests.npz: the variables after one train() of paper_sampler (e1 and d4 with encoder
    batch norm, x without) and paper_noise at B = 4, f32, seed 0, written by tools/regression_digest.py --sampler on the commit
    before the executor learned fed channels.  Same SHA-256 of every variable's float32 bytes."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import regression_digest as RD
    finally:
        sys.path.remove(os.path.join(ROOT, 'tools'))
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'sampler_parent_digests.npz'))
    want = dict(zip(gold['names'].tolist(), gold['sha256'].tolist()))
    got = RD.sampler_digests(DEV)
    assert sorted(got) == sorted(want) and len({k.split('/')[0] for k in got}) == 4
    wrong = [k for k in want if got[k][0] != want[k]]
    assert not wrong, 'variables differ from the parent commit: %s' % wrong[:8]
