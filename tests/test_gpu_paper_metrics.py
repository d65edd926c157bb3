"""paper_cgan dataset evaluation on the GPU (paper/paper_metrics.py, paper/paper_train.py:43-60): the kernels of
tdg_cgan_eval.hip against the float64 NumPy restatement of tests/test_host_paper_metrics.py and against tdg_cgan_metrics,
then set_mean_image / metrics(), dataset_moments(), evaluate() and the paper_metrics.py command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
from test_gpu_paper_cgan import close, dev, make, DEV, K, L
from test_host_paper_metrics import sweep_set, batch_moments, sweep_reference, KEYS

pytestmark = pytest.mark.gpu
HW = 841
FINALS = ['threshold%d_final' % k for k in (1, 2, 3)]


class Eval:
    """The three entry points on buffers of their own."""

    def __init__(self, hw=HW):
        lib = L().load()
        self.hw = hw
        self.acc = torch.zeros(lib.tdg_cgan_eval_acc_bytes(hw) // 8, dtype=torch.float64, device=DEV)
        self.counts = torch.zeros(3, 4, dtype=torch.int64, device=DEV)
        self.ws = torch.zeros(lib.tdg_cgan_eval_workspace_bytes(), dtype=torch.uint8, device=DEV)
        self.scalars = torch.zeros(3, 12, dtype=torch.float64, device=DEV)
        self.mean, self.var = torch.zeros(hw, device=DEV), torch.zeros(hw, device=DEV)

    def batch(self, y, pred, off, image, scale, sets):
        p = lambda a: K().ptr(dev(a)) if a is not None else K().ptr(None)
        L().call('tdg_cgan_eval_batch', p(y), p(pred), p(off), p(image), scale, y.shape[0], self.hw, sets, K().ptr(self.counts),
                 K().ptr(self.acc), K().ptr(self.ws), self.ws.numel(), K().stream())

    def moments(self, y):
        L().call('tdg_cgan_eval_moments', K().ptr(dev(y)), y.shape[0], self.hw, K().ptr(self.acc), K().stream())

    def finish(self, unit=10.0, images=True):
        L().call('tdg_cgan_eval_finish', K().ptr(self.acc), K().ptr(self.counts), self.hw, unit, K().ptr(self.scalars),
                 K().ptr(self.mean if images else None), K().ptr(self.var if images else None), K().stream())
        return self.scalars.cpu().numpy()

    def set_values(self, k):
        """Set k's eight sums (of one batch: its values)."""
        return self.acc[k * 9:k * 9 + 8].cpu().numpy()


def data(B, k, positive=False):
    """Batch k: the crop in [0.1, 10], a prediction as in test_metrics_kernel_streaming_and_zero_prediction (g + offset, with
    negative entries; `positive`: without the -1, so that every value is finite), per-image offsets and a [0, 1] image."""
    rng = np.random.default_rng([6, B, k])
    y = rng.uniform(0.1, 10, (B, HW)).astype(np.float32)
    g = (y * rng.uniform(0.6, 1.6, (B, HW))).astype(np.float32) - np.float32(0.0 if positive else 1.0)
    off = rng.uniform(0.5, 1.5, B).astype(np.float32)
    img = rng.uniform(0.05, 0.95, HW).astype(np.float32)
    return y, (g + off[:, None]).astype(np.float32), off, img


def metrics_kernel(y, pred, off):
    """tdg_cgan_metrics on fresh totals: its eight f32 outputs."""
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, device=DEV)
    ws = torch.zeros(L().load().tdg_cgan_metrics_workspace_bytes(), dtype=torch.uint8, device=DEV)
    p = lambda a: K().ptr(dev(a)) if a is not None else K().ptr(None)
    L().call('tdg_cgan_metrics', p(y), p(pred), p(off), y.shape[0], HW, K().ptr(counts), K().ptr(out), K().ptr(ws), ws.numel(),
             K().stream())
    return out.cpu().numpy()


def set_rows(d):
    return [d[k] for k in KEYS], [d[k] for k in FINALS]


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('zero_form', ['zero', 'ybar'])
@pytest.mark.parametrize('positive', [False, True])
@pytest.mark.parametrize('B', [6, 512])
def test_fused_kernel_against_the_restatement(B, positive, zero_form):
    """Three batches accumulated, all three sets at once: the sweep means and the final percentages within 1e-4 (the bound
    tdg_cgan_metrics is held to), inf / NaN exactly where the restatement has them, the totals equal as integers."""
    e = Eval()
    ys, preds, y0s, pms = [], [], [], []
    for k in range(3):
        y, yh, off, img = data(B, k, positive)
        e.batch(y, yh, off if zero_form == 'ybar' else None, img, 10.0, 7)
        ys.append(y)
        preds.append(yh)
        y0s.append(np.broadcast_to(off[:, None], y.shape) if zero_form == 'ybar' else np.zeros_like(y))
        pms.append(np.broadcast_to(np.float32(10.0) * img, y.shape))
    got = e.finish(images=False)
    counts = e.counts.cpu().tolist()
    for k, (name, ps) in enumerate((('y_hat', preds), ('y_0', y0s), ('y_mean', pms))):
        ref, ref_counts = sweep_set(ys, ps)
        means, finals = set_rows(ref)
        print(name, 'got', got[k].tolist(), 'ref', means, finals, 'counts', counts[k], ref_counts)
        close(got[k, :8], means, 1e-4, name + ' means')
        close(got[k, 8:11], finals, 1e-4, name + ' finals')
        assert got[k, 11] == 3.0
        assert counts[k] == ref_counts and ref_counts[3] == 3 * B * HW
    if zero_form == 'zero':                                      # the pattern of the existing zero-prediction test
        assert np.isinf(got[1, 0]) and np.isinf(got[1, 1]) and np.all(got[1, 5:11] == 0)
    if positive:
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))


@pytest.mark.parametrize('B', [6, 512])
def test_fused_kernel_is_the_metrics_kernel_bit_for_bit(B):
    """The fused kernel keeps tdg_cgan_metrics' block partition and arithmetic: a batch's y_hat / y_0 values, rounded to f32,
    are that kernel's outputs on the same buffers bit for bit -- with the other sets running beside them or alone."""
    y, yh, off, img = data(B, 0)
    img10 = (np.float32(10.0) * img).astype(np.float32)
    tiled = np.ascontiguousarray(np.broadcast_to(img10, y.shape))
    want = {0: metrics_kernel(y, yh, None), 1: metrics_kernel(y, None, off), 2: metrics_kernel(y, tiled, None)}
    want_zero = metrics_kernel(y, None, None)
    e = Eval()
    e.batch(y, yh, off, img, 10.0, 7)
    for k in range(3):
        assert np.array_equal(e.set_values(k).astype(np.float32), want[k], equal_nan=True), k
    for sets, k, args in ((1, 0, (yh, None, None, 1.0)), (2, 1, (None, off, None, 1.0)), (4, 2, (None, None, img10, 1.0))):
        e = Eval()                                               # one set alone; the image form with scale 1 on the 10x image
        e.batch(y, *args, sets)
        assert np.array_equal(e.set_values(k).astype(np.float32), want[k], equal_nan=True), sets
        assert np.all(e.acc[:27].cpu().numpy()[[j for j in range(27) if j // 9 != k]] == 0)      # the other sets untouched
    e = Eval()
    e.batch(y, None, None, None, 1.0, 2)                         # y_0 = 0
    assert np.array_equal(e.set_values(1).astype(np.float32), want_zero, equal_nan=True)


def test_fused_kernel_runs_are_bit_equal():
    a, b = Eval(), Eval()
    for k in range(3):
        y, yh, off, img = data(64, k)
        for e in (a, b):
            e.batch(y, yh, off, img, 10.0, 7)
            e.moments(y)
    assert np.array_equal(a.acc.cpu().numpy(), b.acc.cpu().numpy(), equal_nan=True)
    assert a.counts.cpu().tolist() == b.counts.cpu().tolist()


@pytest.mark.parametrize('B', [6, 13, 512])
def test_moments_kernel(B):
    """tf.nn.moments over the batch axis per batch, averaged over three batches: 1e-6 of NumPy float64 (f64-summed f32 data,
    the bound of test_prep_kernel); unit 10 gives the [0, 1] images, unit 1 the 10x ones."""
    e = Eval()
    ys = [data(B, k)[0] for k in range(3)]
    for y in ys:
        e.moments(y)
    assert e.acc[27].item() == 3.0 and np.all(e.acc[:27].cpu().numpy() == 0)
    e.finish(unit=10.0)
    mean, var = batch_moments([y.astype(np.float64) / 10.0 for y in ys])
    print('moments B', B, 'max err', np.abs(e.mean.cpu().numpy() - mean).max(), np.abs(e.var.cpu().numpy() - var).max())
    close(e.mean.cpu().numpy(), mean, 1e-6, 'mean image')
    close(e.var.cpu().numpy(), var, 1e-6, 'variance image')
    e.finish(unit=1.0)
    mean, var = batch_moments(ys)
    close(e.mean.cpu().numpy(), mean, 1e-6, 'mean image, 10x')
    close(e.var.cpu().numpy(), var, 1e-6, 'variance image, 10x')


def test_moments_known_answer_on_the_device():
    """A 2-image batch: mean (a+b)/2, variance ((a-b)/2)^2, exactly."""
    e = Eval(hw=2)
    e.moments(np.array([[1.0, 4.0], [3.0, 0.0]], np.float32))
    e.finish(unit=1.0)
    assert e.mean.cpu().tolist() == [2.0, 2.0] and e.var.cpu().tolist() == [1.0, 4.0]
    e.moments(np.array([[2.0, 2.0], [2.0, 6.0]], np.float32))
    e.finish(unit=1.0)
    assert e.mean.cpu().tolist() == [2.0, 3.0] and e.var.cpu().tolist() == [0.5, 4.0]


# ------------------------------------------------------------------------------------------------ the model
def source(B, seed=21, n=4):
    return pkg('data').SyntheticPairSource(n, B, DEV, 65, seed)


def crop_of(y01):
    """The f32 crop (10x depth) and y_bar as tdg_cgan_prep makes them (test_prep_kernel holds that kernel to 1e-6)."""
    c = (y01.cpu().numpy()[:, 17:46, 17:46, 0] * np.float32(10.0)).astype(np.float32)
    return c, c.astype(np.float64).mean((1, 2)).astype(np.float32)


def check_result(got, ref, what):
    for name in ('model', 'zero', 'mean'):
        gm, gf = set_rows(got[name])
        rm, rf = set_rows(ref[name])
        print(what, name, 'got', gm, gf, 'ref', rm, rf)
        close(gm, rm, 1e-4, '%s %s means' % (what, name))
        close(gf, rf, 1e-4, '%s %s finals' % (what, name))
        assert list(got[name]) == list(KEYS) + FINALS
    close(got['mean_image'], ref['mean_image'], 1e-6, what + ' mean image')
    close(got['var_image'], ref['var_image'], 1e-6, what + ' variance image')


def same_result(a, b):
    for name in ('model', 'zero', 'mean'):
        assert np.array_equal(list(a[name].values()), list(b[name].values()), equal_nan=True), name
    assert np.array_equal(a['mean_image'], b['mean_image']) and np.array_equal(a['var_image'], b['var_image'])
    assert (a['n_batches'], a['images']) == (b['n_batches'], b['images'])


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('version', ['baseline', 'mean_adjusted', 'mean_provided2'])
def test_evaluate_against_infer_and_the_restatement(version, dt):
    """evaluate() over 3 + 3 batches of a seeded source, recomputed from infer()'s own y_hat of the same batches (a second
    source with the same seed) through the restatement."""
    B, n = 8, 3
    m = make(version, 'gan', B=B, dtype=dt)
    got = m.evaluate(source(B), n)
    assert (got['n_batches'], got['images']) == (n, n * B)
    assert got['mean_image'].shape == (29, 29) and got['mean_image'].dtype == np.float32 and got['var_image'].shape == (29, 29)
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
    ref = sweep_reference(crops, yhats, ybars, {'baseline': 0, 'mean_adjusted': 1, 'mean_provided2': 2}[version], crops2)
    check_result(got, ref, '%s dt %d' % (version, dt))
    if version == 'baseline':                                    # g = 0 against a positive depth: the formulas' inf, and no hit
        assert np.isinf(got['zero']['abs_rel_diff']) and got['zero']['threshold3_final'] == 0.0
    else:
        assert all(np.isfinite(v) for v in got['zero'].values())
    assert all(np.isfinite(v) for v in got['mean'].values())


def test_evaluate_replay_determinism_and_isolation():
    B, n = 8, 4                                                  # four batches: eager, capture, two replays per sweep
    a, e = make('mean_adjusted', 'gan', B=B, use_graphs=True), make('mean_adjusted', 'gan', B=B, use_graphs=False)
    ra, re_ = a.evaluate(source(B), n), e.evaluate(source(B), n)
    assert 'eval_model' in a._graphs and 'eval_mean' in a._graphs and not e._graphs
    same_result(ra, re_)                                         # graph replay equals the eager run bit for bit
    same_result(a.evaluate(source(B), n), ra)                    # a second call: totals restart at zero, all replayed
    # training, metrics() and variables() do not see an evaluation: a twin that never evaluated is bit-equal
    b, c = make('mean_adjusted', 'gan', B=B), make('mean_adjusted', 'gan', B=B)
    for m in (b, c):
        m.train()
    v0 = b.variables()
    b.evaluate(source(B), n)
    v1 = b.variables()
    assert all(np.array_equal(v0[k], v1[k]) for k in v0)
    mb, mc = b.metrics(), c.metrics()
    assert set(mb) == {'metrics_y_hat', 'metrics_y_0'}
    for k in mb:
        assert np.array_equal(list(mb[k].values()), list(mc[k].values()), equal_nan=True)
    assert b.train() == c.train()
    vb, vc = b.variables(), c.variables()
    assert all(np.array_equal(vb[k], vc[k]) for k in vb)
    with pytest.raises(ValueError):
        b.evaluate(source(B), 0)


def test_dataset_moments():
    B, n = 8, 3
    m = make('baseline', 'gan', B=B)
    mean, var = m.dataset_moments(source(B), n)
    twin = source(B)
    ref_m, ref_v = batch_moments([crop_of(twin.next_batch()[1])[0].astype(np.float64) / 10.0 for _ in range(n)])
    assert mean.shape == var.shape == (29, 29) and mean.dtype == var.dtype == np.float32
    close(mean, ref_m, 1e-6, 'mean image')
    close(var, ref_v, 1e-6, 'variance image')
    got = m.evaluate(source(B), n)                               # evaluate()'s sweep 1 takes the same moments
    assert np.array_equal(got['mean_image'], mean) and np.array_equal(got['var_image'], var)
    m.set_mean_image(mean)                                       # and the mean goes straight to set_mean_image
    assert np.array_equal(m.mean_image.cpu().numpy(), mean)


@pytest.mark.parametrize('version', ['baseline', 'mean_adjusted'])
def test_metrics_y_mean(version):
    """metrics(): the key set is unchanged without a mean image; with one, `metrics_y_mean` is the restatement on
    10 * image (f32; no y_bar added, for every version) and its threshold totals stream across calls."""
    m = make(version, 'gan')
    m.train()
    assert set(m.metrics()) == {'metrics_y_hat', 'metrics_y_0'}
    crop = m.crop.cpu().numpy()
    img = np.random.default_rng(3).uniform(0.05, 0.95, (29, 29)).astype(np.float32)
    m.set_mean_image(img[None])                                  # [1,29,29], as the reference's placeholder
    pred = np.broadcast_to(np.float32(10.0) * img, crop.shape)
    counts = [0, 0, 0, 0]
    from test_gpu_paper_cgan import eigen_ref
    got = m.metrics()
    assert list(got) == ['metrics_y_hat', 'metrics_y_0', 'metrics_y_mean'] and list(got['metrics_y_mean']) == list(KEYS)
    close([got['metrics_y_mean'][k] for k in KEYS], eigen_ref(crop, pred, counts), 1e-4, 'y_mean')
    m.train()
    crop2 = m.crop.cpu().numpy()
    got = m.metrics()                                            # a second fetch: the totals keep running
    close([got['metrics_y_mean'][k] for k in KEYS], eigen_ref(crop2, pred, counts), 1e-4, 'y_mean, second call')
    assert m.mean_counts[2].cpu().tolist() == counts and counts[3] == 2 * crop.size
    m.set_mean_image(None)
    assert set(m.metrics()) == {'metrics_y_hat', 'metrics_y_0'}
    with pytest.raises(ValueError):
        m.set_mean_image(np.zeros((30, 29), np.float32))


# ------------------------------------------------------------------------------------------------ the command line
def test_paper_metrics_cli(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    ws = str(tmp_path / 'ws')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_cgan', '--dataset', 'synthetic',
                        '--batch_size', '8', '--epoch_size', '2', '--epochs', '1', '--model_version', 'mean_adjusted',
                        '--dir', ws], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    argv = ['@' + os.path.join(ws, 'options.config'), '--dir', ws]
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'paper_metrics.py')] + argv, env=env, timeout=600,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert [d['split'] for d in lines] == ['validate', 'train']
    assert all(d['n_batches'] == 4 and d['images'] == 32 and d['checkpoint'] == 'checkpoint-1.npz' for d in lines)
    text = [l for l in p.stdout.splitlines() if not l.startswith('{')]
    assert text.count('Model metrics:') == 2 and text.count('Mean metrics:') == 2 and text.count('Zero metrics:') == 2
    assert sum(l.startswith('\tt1: ') for l in text) == 6
    png = pkg('png')
    pm = __import__('paper_metrics')
    args = pm.parse_args(argv)
    m, _ = __import__('paper_fullimage').build_model(args)
    for d in lines:
        split = d['split']
        with open(os.path.join(ws, 'metrics', split + '.json')) as f:
            on_disk = json.load(f)
        src, examples = pm.open_split(args, m.sess, split)
        rec = pm.record(split, 'checkpoint-1.npz', m.evaluate(src, pm.batches_of(args, examples)))
        for name in ('model', 'zero', 'mean'):                  # the file, the JSON line and an in-process evaluate() agree
            assert np.array_equal(list(on_disk[name].values()), list(rec[name].values()), equal_nan=True), (split, name)
            assert np.array_equal(list(d[name].values()), list(rec[name].values()), equal_nan=True), (split, name)
            assert list(on_disk[name]) == list(rec[name])
        assert {k: on_disk[k] for k in ('split', 'checkpoint', 'n_batches', 'images')} == \
            {k: rec[k] for k in ('split', 'checkpoint', 'n_batches', 'images')}
        for stem, ch in (('_mean', 1), ('_mean_colorized', 3), ('_var', 1)):
            with open(os.path.join(ws, 'metrics', split + stem + '.png'), 'rb') as f:
                img = png.decode(f.read())
            assert img.shape == (29, 29, ch), (stem, img.shape)
    assert lines[0]['model'] != lines[1]['model']                 # the splits are different streams
