"""SamplerReplica.sample_full on the GPU: every window's mean / variance / errors against sample() on that window with the same
noise draws, the three canvases against the reference's reconstruct (restated in tests/test_gpu_paper_cgan_fullimage.py) on
the returned windows, grouped passes without batch norm, live noise, isolation from training and metrics(), determinism, graph
replay, frames without depth and the paper_sample_fullimage.py command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import _sampler_ref as R
from test_gpu_paper_cgan import Batches, SMALL_HP                # noqa: F401  (Batches: make()'s data)
from test_gpu_paper_cgan_fullimage import frame, grid, reconstruct, rmse
from test_gpu_paper_sampler import make, draws, same_metrics, stats_within

pytestmark = pytest.mark.gpu


def within(got, ref, tol, what):
    assert abs(got - ref) <= tol * abs(ref), '%s: %r vs %r' % (what, got, ref)


def windows_of(g, image, depth):
    for c in range(g.patches):
        top, left = g.corner(c)
        yield c, image[top:top + 65, left:left + 65], depth[top:top + 65, left:left + 65]


def crop10(y):
    """The model's depth target of a window: 10 y rounded in f32, cropped at +17."""
    return (np.float32(10.0) * y[17:46, 17:46]).astype(np.float64).reshape(1, -1)


def canvases(r):
    return [t.cpu().numpy() for t in (r.y_hat, r.g, r.var)]


def check_canvases(r, H, W, s, depth):
    """y_hat, g and var are the reference's blend of the returned windows, bit for bit; rmse is the reference's; what no
    window covers is 0."""
    wy, wv, wb = (t.cpu().numpy() for t in (r.window_y_hat, r.window_var, r.window_y_bar))
    cy, cg, cv = canvases(r)
    assert np.array_equal(cy, reconstruct(H, W, wy, s).astype(np.float32)), 'y_hat canvas'
    assert np.array_equal(cg, reconstruct(H, W, wy - wb[:, None, None], s).astype(np.float32)), 'g canvas'
    assert np.array_equal(cv, reconstruct(H, W, wv, s).astype(np.float32)), 'variance canvas'
    within(r.rmse, rmse(depth[..., None], cy.astype(np.float64)[..., None]), 1e-6, 'rmse')
    cols, rows = r.grid
    outside = np.ones((H, W), bool)
    outside[18:(cols - 1) * s + 18 + 29, 18:(rows - 1) * s + 18 + 29] = False
    for c in (cy, cg, cv):
        assert np.all(c[outside] == 0)
    assert np.any(cy[~outside] != 0)


# ------------------------------------------------------------------------------------------------ one window per pass
BN = dict(node='d3', B=4, H=100, W=107, s=3)


@pytest.fixture(scope='module')
def bn_case():
    """A batch-norm model after one train(), its noise draws staged (so every pass, eager or replayed, sees the same four),
    and one sample_full of a 100 x 107 frame at stride 3: 8 windows, 8 passes."""
    node, B, H, W, s = (BN[k] for k in ('node', 'B', 'H', 'W', 's'))
    m = make(node, bn=True, B=B, hp=SMALL_HP)
    m.train()
    m.sess.stage_draws('noise_' + node, draws(node, B, 1)[0])
    image, depth = frame(H, W, 21)
    r = m.sample_full(image, depth, stride=s, windows=True)
    return m, image, depth, r


def test_windows_are_sample(bn_case):
    m, image, depth, r = bn_case
    g = grid(BN['H'], BN['W'], BN['s'])
    assert r.patches == g.patches == 8 and r.grid == (2, 4) and r.draws == BN['B']
    assert tuple(r.window_y_hat.shape) == (8, 29, 29) == tuple(r.window_var.shape)
    wy, wv = r.window_y_hat.cpu().numpy(), r.window_var.cpu().numpy()
    means, mins = [], []
    for c, x, y in windows_of(g, image, depth):
        out = m.sample(x, y)
        yh = out['y_hat'].cpu().numpy().astype(np.float64).reshape(BN['B'], -1)
        stats_within(wy[c].ravel(), yh.mean(axis=0), 'window %d, mean' % c)
        stats_within(wv[c].ravel(), yh.var(axis=0) / 100.0, 'window %d, variance' % c)
        means.append(out['metrics']['per_image_rmse/mean'])
        mins.append(out['metrics']['per_image_rmse/min'])
    assert float(wv.max()) > 0
    within(r.err_mean, np.mean(means), 1e-6, 'err_mean')
    within(r.err_min, np.mean(mins), 1e-6, 'err_min')
    assert r.err_min <= r.err_mean


def test_canvases_are_the_reference_blend(bn_case):
    m, image, depth, r = bn_case
    check_canvases(r, BN['H'], BN['W'], BN['s'], depth)
    assert tuple(r.y_hat.shape) == (BN['H'], BN['W']) == tuple(r.g.shape) == tuple(r.var.shape)
    assert not np.array_equal(r.y_hat.cpu().numpy(), r.g.cpu().numpy())          # y_bar is not 0 with a depth


def test_second_call_replays_the_captured_body(bn_case):
    m, image, depth, r = bn_case
    name = 'sample_full_%d_%d_%d_%d' % (BN['H'], BN['W'], BN['s'], BN['B'])
    assert name in m._graphs                                     # 8 passes: one eager, one captured, six replayed
    graph, buffers = m._graphs[name], dict(m._full_sample)
    r2 = m.sample_full(image, depth, stride=BN['s'])
    assert m._graphs[name] is graph and dict(m._full_sample) == buffers and r2.window_y_hat is None
    assert all(np.array_equal(a, b) for a, b in zip(canvases(r), canvases(r2)))
    assert (r2.rmse, r2.err_mean, r2.err_min) == (r.rmse, r.err_mean, r.err_min)


def test_no_depth(bn_case):
    m, image, depth, _ = bn_case
    r = m.sample_full(image, None, stride=BN['s'])
    assert r.rmse is None and r.err_mean is None and r.err_min is None and r.patches == 8
    cy, cg, cv = canvases(r)
    assert np.array_equal(cy, cg) and np.any(cy != 0) and np.any(cv > 0)


def test_bad_arguments(bn_case):
    m, image, depth, _ = bn_case
    with pytest.raises(ValueError, match='batch norm'):
        m.sample_full(image, depth, stride=BN['s'], draws=2)
    with pytest.raises(ValueError):
        m.sample_full(image, depth, stride=BN['s'], draws=3)
    with pytest.raises(ValueError):
        m.sample_full(image[:93], depth[:93], stride=1)
    with pytest.raises(ValueError):
        m.sample_full(image, depth, stride=0)
    with pytest.raises(ValueError):
        m.sample_full(image, depth, stride=8)                    # (100 - 93) // 8 == 0: no window fits
    with pytest.raises(ValueError):
        m.sample_full(image, depth, stride=BN['s'], offset=37)
    for call in (m.infer_full, m.evaluate):                      # the refusals stay
        with pytest.raises(NotImplementedError, match='batch norm'):
            call(None, None)


# ------------------------------------------------------------------------------------------------ several windows per pass
def test_grouped_passes():
    """No batch norm, B = 8, draws = 2: four windows share a pass, window k of a pass under rows 2k, 2k + 1 of the staged
    draws; 6 windows, so the second pass is half empty.  Without batch norm sample() at B = 8 gives each row's prediction
    on its own, so its rows 2k, 2k + 1 are the window's two draws."""
    node, B, D, H, W, s = 'e2', 8, 2, 100, 104, 3
    m = make(node, bn=False, B=B, hp=SMALL_HP)
    m.train()
    m.sess.stage_draws('noise_' + node, draws(node, B, 1)[0])
    image, depth = frame(H, W, 22)
    g = grid(H, W, s)
    assert g.patches == 6
    r = m.sample_full(image, depth, stride=s, draws=D, windows=True)
    assert r.patches == 6 and r.draws == D and m._full_sample[(H, W, s, D)].n_passes == 2
    wy, wv = r.window_y_hat.cpu().numpy(), r.window_var.cpu().numpy()
    means, mins = [], []
    for c, x, y in windows_of(g, image, depth):
        k = c % (B // D)
        yh = m.sample(x, y)['y_hat'].cpu().numpy().astype(np.float64).reshape(B, -1)[k * D:(k + 1) * D]
        stats_within(wy[c].ravel(), yh.mean(axis=0), 'window %d, mean' % c)
        stats_within(wv[c].ravel(), yh.var(axis=0) / 100.0, 'window %d, variance' % c)
        e = R.sample_stats(np.repeat(crop10(y), D, axis=0), yh, yh)
        means.append(e[0])
        mins.append(e[1])
    assert float(wv.max()) > 0
    within(r.err_mean, np.mean(means), 1e-6, 'err_mean')
    within(r.err_min, np.mean(mins), 1e-6, 'err_min')
    check_canvases(r, H, W, s, depth)
    with pytest.raises(ValueError):
        m.sample_full(image, depth, stride=s, draws=3)


# ------------------------------------------------------------------------------------------------ noise, isolation, determinism
def test_noise_is_live():
    node, B, H, W, s = 'e2', 4, 100, 104, 3
    m = make(node, bn=False, B=B, hp=SMALL_HP)
    m.train()
    image, depth = frame(H, W, 23)
    a, b = m.sample_full(image, depth, stride=s), m.sample_full(image, depth, stride=s)
    assert not np.array_equal(a.y_hat.cpu().numpy(), b.y_hat.cpu().numpy()) and not np.array_equal(a.var.cpu().numpy(), b.var.cpu().numpy())
    cols, rows = a.grid
    assert float(a.var[18:(cols - 1) * s + 47, 18:(rows - 1) * s + 47].max()) > 0
    # the same draw in every row (another `draws`, so that the body is captured with the staged copy): the predictions coincide
    m.sess.stage_draws('noise_' + node, np.repeat(draws(node, 1, 1)[0], B, axis=0))
    c = m.sample_full(image, depth, stride=s, draws=2)
    assert np.all(c.var.cpu().numpy() == 0.0) and np.any(c.y_hat.cpu().numpy() != 0.0)
    assert c.err_mean == c.err_min


def test_isolation_and_determinism():
    node, B, H, W, s = 'x', 4, 100, 107, 3
    image, depth = frame(H, W, 24)
    a = make(node, bn=True, B=B, seed=3, hp=SMALL_HP)
    a.train()
    v0, m0 = a.variables(), a.metrics()
    kept = [t.clone() for t in (a.crop, a.yhat, a.g32, a.ybar)]
    ra = a.sample_full(image, depth, stride=s)
    v1, m1 = a.variables(), a.metrics()
    assert all(np.array_equal(v0[k], v1[k]) for k in v0)
    assert same_metrics({k: m0[k] for k in ('metrics_y_hat', 'metrics_y_0')}, {k: m1[k] for k in ('metrics_y_hat', 'metrics_y_0')})
    assert all(np.array_equal(t.cpu().numpy(), u.cpu().numpy()) for t, u in zip(kept, (a.crop, a.yhat, a.g32, a.ybar)))
    # a fresh model of the same seed, with graphs and without: the same steps, so the same draws, so the same canvases
    for use_graphs in (True, False):
        b = make(node, bn=True, B=B, seed=3, hp=SMALL_HP, use_graphs=use_graphs)
        b.train()
        b.metrics()
        rb = b.sample_full(image, depth, stride=s)
        assert all(np.array_equal(p, q) for p, q in zip(canvases(ra), canvases(rb))), 'use_graphs=%s' % use_graphs
        assert (ra.rmse, ra.err_mean, ra.err_min) == (rb.rmse, rb.err_mean, rb.err_min)
        assert bool(b._graphs) == use_graphs


# ------------------------------------------------------------------------------------------------ the command line
def test_paper_sample_fullimage_cli(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    ws = str(tmp_path / 'ws')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_sampler', '--dataset', 'synthetic',
                        '--random_crop', '65', '65', '--batch_size', '8', '--epoch_size', '2', '--epochs', '1', '--dir', ws], env=env, timeout=600,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    argv = ['@' + os.path.join(ws, 'options.config'), '--frames', '0', '--strides', '40', '--no_images']
    p = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'paper_sample_fullimage.py')] + argv, env=env,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    d = lines[0]
    assert list(d) == ['split', 'frame', 'stride', 'patches', 'draws', 'rmse', 'err_mean', 'err_min', 'var_mean', 'ms']
    assert (d['split'], d['frame'], d['stride'], d['patches'], d['draws']) == ('validate', 0, 40, 88, 8)
    assert np.isfinite(d['rmse']) and d['rmse'] > 0 and np.isfinite(d['err_mean']) and d['err_min'] <= d['err_mean'] and d['var_mean'] >= 0
    assert not os.path.exists(os.path.join(ws, 'images'))
