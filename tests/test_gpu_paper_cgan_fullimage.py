"""paper_cgan full-frame inference on the GPU (paper_fullimage.py of the thesis code): the tdg_cgan_full.hip kernels against
NumPy restatements of the reference's build_batch / reconstruct / rmse (defined here, line by line), infer_full end to end
against infer() and the float64 generator oracle, graph replay, isolation from training, full NYUv2-size frames in bf16 and
the paper_fullimage.py command line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
from test_gpu_paper_cgan import DEV, K, L, close, dev, make, oracle_G

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the reference, restated
def build_batch(image, stride, channels):
    """paper_fullimage.py:90-110 for an [H, W, C] frame (NHWC rows instead of the reference's NCHW: a layout, not a value
    change), float64, zero-padded to a multiple of 1024."""
    y_lim = image.shape[0]
    x_lim = image.shape[1]
    cols = int((y_lim - 65 - 29 + 1) / stride)
    rows = int((x_lim - 65 - 29 + 1) / stride)
    n = math.ceil((cols * rows) / 1024)
    image_batch = np.zeros((n * 1024, 65, 65, channels))
    c = 0
    x_pos = 0
    y_pos = 0
    for n in range(rows):
        for m in range(cols):
            image_batch[c] = image[x_pos:x_pos + 65, y_pos:y_pos + 65, :]
            c += 1
            x_pos += stride
        x_pos = 0
        y_pos += stride
    return image_batch, cols * rows


def reconstruct(H, W, depth_batch, stride, offset=18):
    """paper_fullimage.py:126-155 (the depth canvas) for an H x W frame; depth_batch [>= P, 29, 29] f32."""
    reconstructed_depth = np.zeros((H, W, 1))
    reconstructed_depth[:] = np.nan
    cols = int((H - 65 - 29 + 1) / stride)
    rows = int((W - 65 - 29 + 1) / stride)
    c = 0
    x_pos = 0
    y_pos = 0
    for n in range(rows):
        for m in range(cols):
            d = depth_batch[c][..., None]
            current_depth = reconstructed_depth[x_pos + offset:x_pos + offset + 29, y_pos + offset:y_pos + offset + 29, :]
            new_depth = np.where(np.isnan(current_depth), d, current_depth)
            new_depth = (new_depth + d) / 2.0
            reconstructed_depth[x_pos + offset:x_pos + offset + 29, y_pos + offset:y_pos + offset + 29, :] = new_depth
            c += 1
            x_pos += stride
        x_pos = 0
        y_pos += stride
    return np.nan_to_num(reconstructed_depth)[..., 0]


def rmse(d1, d2):
    """paper_fullimage.py:157-163: d1 the f32 depth [H, W, 1] in [0, 1], d2 the float64 canvas [H, W, 1]."""
    x_lim = d2.shape[0] - (18 + 28)
    y_lim = d2.shape[1] - (18 + 28)
    d1 = d1 * 10.0
    d1 = d1[18:x_lim, 18:y_lim, :]
    d2 = d2[18:x_lim, 18:y_lim, :]
    return np.sqrt(np.mean(np.square(d1 - d2)))


def f32(*shape, fill=0.0):
    return torch.full(shape, fill, dtype=torch.float32, device=DEV)


def frame(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.random((H, W, 3), dtype=np.float32), (rng.random((H, W), dtype=np.float32) * 0.98 + 0.01).astype(np.float32)


def grid(H, W, s):
    return pkg('models.paper.paper_cgan').patch_grid(H, W, s)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('chunk', [1, 2])
def test_gather_is_build_batch(chunk):
    H, W, s, B = 150, 170, 7, 32
    image, depth = frame(H, W, 1)
    xb, P = build_batch(image, s, 3)
    yb, _ = build_batch(depth[..., None], s, 1)
    assert P == 88 and 2 * B < P < 3 * B                        # chunk 2 is the last, partial one
    x, y = f32(B, 65, 65, 3, fill=7.0), f32(B, 65, 65, 1, fill=7.0)
    ch = torch.tensor([chunk], dtype=torch.int32, device=DEV)
    L().call('tdg_cgan_full_gather', K().ptr(dev(image)), K().ptr(dev(depth)), H, W, s, K().ptr(ch), B, K().ptr(x), K().ptr(y),
             K().stream())
    gx, gy = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
    assert np.array_equal(gx, xb[chunk * B:(chunk + 1) * B]) and np.array_equal(gy, yb[chunk * B:(chunk + 1) * B])
    if chunk == 2:
        assert np.all(gx[P - 2 * B:] == 0) and np.all(gy[P - 2 * B:] == 0)
    assert int(ch.item()) == chunk                              # the gather reads the index, the store advances it


@pytest.mark.parametrize('s', [1, 3, 10, 29, 31])
def test_blend_is_reconstruct(s):
    H, W = 200, 230
    P = grid(H, W, s).patches
    slots = P + 5
    rng = np.random.default_rng(s)
    st = rng.uniform(-3, 8, (slots, 29, 29)).astype(np.float32)
    bar = rng.uniform(0, 5, slots).astype(np.float32)
    cy, cg = f32(H, W, fill=7.0), f32(H, W, fill=7.0)
    for off in ((18, 17) if s == 3 else (18,)):
        L().call('tdg_cgan_full_blend', K().ptr(dev(st)), K().ptr(dev(bar)), slots, H, W, s, off, K().ptr(cy), K().ptr(cg), K().stream())
        ry = reconstruct(H, W, st, s, off).astype(np.float32)
        rg = reconstruct(H, W, st - bar[:, None, None], s, off).astype(np.float32)
        assert np.array_equal(cy.cpu().numpy(), ry), 'y_hat canvas, stride %d offset %d' % (s, off)
        assert np.array_equal(cg.cpu().numpy(), rg), 'g canvas, stride %d offset %d' % (s, off)
    if s == 31:                                                 # two-pixel gaps between the windows stay 0
        assert np.all(ry[:, 18 + 29:18 + 31] == 0) and np.all(ry[18 + 29:18 + 31, :] == 0)


def test_blend_order_matters():
    """Three windows over one pixel, constants 1, 2, 6 in that order: ((1 + 2) / 2 + 6) / 2 = 3.75, not the mean 3 (and not
    2.5, the reverse order)."""
    H, W, s = 96, 94, 1
    assert tuple(grid(H, W, s)) == (3, 1)
    st = np.stack([np.full((29, 29), v, np.float32) for v in (1.0, 2.0, 6.0)])
    cy, cg = f32(H, W), f32(H, W)
    L().call('tdg_cgan_full_blend', K().ptr(dev(st)), K().ptr(dev(np.zeros(3, np.float32))), 3, H, W, s, 18, K().ptr(cy), K().ptr(cg),
             K().stream())
    got = cy.cpu().numpy()
    assert got[18 + 2, 30] == 3.75 and got[18, 30] == 1.0 and got[18 + 1, 30] == 1.5
    assert np.array_equal(got, reconstruct(H, W, st, s).astype(np.float32))
    assert np.array_equal(cg.cpu().numpy(), got)


@pytest.mark.parametrize('case', ['dense', 'gaps'])
def test_rmse_kernel(case):
    H, W = 200, 230
    rng = np.random.default_rng(5)
    depth = rng.random((H, W), dtype=np.float32)
    if case == 'dense':
        canvas = rng.uniform(0, 10, (H, W)).astype(np.float32)
    else:                                                       # a blended canvas with uncovered pixels (zeros) in the region
        s = 31
        st = rng.uniform(0, 10, (grid(H, W, s).patches, 29, 29)).astype(np.float32)
        canvas = reconstruct(H, W, st, s).astype(np.float32)
        assert np.any(canvas[18:H - 46, 18:W - 46] == 0)
    out, ws = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(256, dtype=torch.float64, device=DEV)
    L().call('tdg_cgan_full_rmse', K().ptr(dev(depth)), K().ptr(dev(canvas)), H, W, K().ptr(out), K().ptr(ws), 256 * 8, K().stream())
    ref = rmse(depth[..., None], canvas.astype(np.float64)[..., None])
    assert abs(out.item() - ref) <= 1e-12 * ref


# ------------------------------------------------------------------------------------------------ infer_full
def chunked_infer(m, image, depth, s):
    """The reference's path on infer(): host build_batch, chunks of B in slot order; (y_hat store, y_bar store, P)."""
    xb, P = build_batch(image, s, 3)
    yb, _ = build_batch(depth[..., None], s, 1)
    B = m.B
    n = -(-P // B)
    yh, yb_ = [], []
    for k in range(n):
        x = torch.tensor(xb[k * B:(k + 1) * B], dtype=torch.float32, device=DEV)
        y = torch.tensor(yb[k * B:(k + 1) * B], dtype=torch.float32, device=DEV)
        yh.append(m.infer((x, y))[..., 0].cpu().numpy())
        yb_.append(m.inf_ybar.cpu().numpy().copy())
    return np.concatenate(yh), np.concatenate(yb_), P, xb


@pytest.mark.parametrize('version', ['baseline', 'mean_adjusted', 'mean_provided2'])
def test_infer_full_matches_infer_f32(version):
    H, W, s = 120, 140, 5
    m = make(version, 'gan', B=16)
    image, depth = frame(H, W, 2)
    r = m.infer_full(image, depth, stride=s)
    g = grid(H, W, s)
    assert r.patches == g.patches == 45 and r.grid == (5, 9)
    yh, ybar, P, xb = chunked_infer(m, image, depth, s)
    assert np.array_equal(r.y_hat.cpu().numpy(), reconstruct(H, W, yh, s).astype(np.float32))
    gv = yh if version == 'baseline' else yh - ybar[:, None, None]
    assert np.array_equal(r.g.cpu().numpy(), reconstruct(H, W, gv, s).astype(np.float32))
    ref = rmse(depth[..., None], r.y_hat.cpu().numpy().astype(np.float64)[..., None])
    assert abs(r.rmse - ref) <= 1e-12 * ref
    if version == 'baseline':
        P64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in m.variables().items()}
        with torch.no_grad():
            go = oracle_G(P64, torch.tensor(xb[:P], dtype=torch.float64))[..., 0].numpy()
        close(r.y_hat.cpu().numpy(), reconstruct(H, W, go, s), 2e-5, 'canvas vs the float64 oracle')
        r17 = m.infer_full(torch.tensor(image), torch.tensor(depth[..., None]), stride=s, offset=17)
        assert np.array_equal(r17.y_hat.cpu().numpy(), reconstruct(H, W, yh, s, 17).astype(np.float32))


def test_infer_full_replay_and_isolation():
    H, W, s = 120, 140, 5
    image, depth = frame(H, W, 3)
    a = make('mean_adjusted', 'gan', B=16, use_graphs=True)
    e = make('mean_adjusted', 'gan', B=16, use_graphs=False)
    r1, r2, r3 = a.infer_full(image, depth, s), a.infer_full(image, depth, s), e.infer_full(image, depth, s)
    assert 'full_%d_%d_%d' % (H, W, s) in a._graphs                  # the chunk body is graph-replayed after warm-up
    for r in (r2, r3):
        assert np.array_equal(r.y_hat.cpu().numpy(), r1.y_hat.cpu().numpy())
        assert np.array_equal(r.g.cpu().numpy(), r1.g.cpu().numpy())
        assert r.rmse == r1.rmse
    # training is untouched: a twin that never ran infer_full trains and reports bit-equally
    b = make('mean_adjusted', 'gan', B=16, use_graphs=True)
    b.infer_full(image, depth, s)
    c = make('mean_adjusted', 'gan', B=16, use_graphs=True)
    for m in (b, c):
        m.train()
    b.infer_full(image, depth, s)
    lb, lc = b.train(), c.train()
    assert lb == lc
    mb, mc = b.metrics(), c.metrics()
    for k in mb:
        assert np.array_equal(list(mb[k].values()), list(mc[k].values()), equal_nan=True)
    vb, vc = b.variables(), c.variables()
    assert all(np.array_equal(vb[k], vc[k]) for k in vb)
    # and a replay after training uses the trained weights
    rb = b.infer_full(image, depth, s)
    assert not np.array_equal(rb.y_hat.cpu().numpy(), r1.y_hat.cpu().numpy())


def test_infer_full_rejects_bad_frames():
    m = make('baseline', 'gan', B=16)
    image, depth = frame(120, 140, 4)
    with pytest.raises(ValueError):
        m.infer_full(image[:93], depth[:93], 5)
    with pytest.raises(ValueError):
        m.infer_full(image, depth, 0)
    with pytest.raises(ValueError):
        m.infer_full(image, depth, 28)                              # (120 - 93) // 28 == 0: no window fits
    with pytest.raises(ValueError):
        m.infer_full(image, depth[:100], 5)


@pytest.mark.parametrize('s, P', [(10, 1518), (1, 156312)])
def test_full_size_bf16(s, P):
    pf = __import__('paper_fullimage')
    image, depth = pf.synthetic_frame('validate', 0)
    m = make('baseline', 'gan', B=512, dtype=1, n_batches=1)
    r = m.infer_full(image, depth, stride=s)
    H, W = 427, 561
    cols, rows = r.grid
    assert r.patches == P == cols * rows
    for c in (r.y_hat.cpu().numpy(), r.g.cpu().numpy()):
        assert np.all(np.isfinite(c))
        r0, r1 = 18, (cols - 1) * s + 18 + 29                       # covered rows [r0, r1), columns [c0, c1)
        c0, c1 = 18, (rows - 1) * s + 18 + 29
        outside = np.ones((H, W), bool)
        outside[r0:r1, c0:c1] = False
        assert np.all(c[outside] == 0)
        for edge in (c[r0, c0:c1], c[r1 - 1, c0:c1], c[r0:r1, c0], c[r0:r1, c1 - 1]):
            assert np.any(edge != 0)
    assert np.isfinite(r.rmse) and r.rmse > 0


def test_paper_fullimage_cli(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    ws = str(tmp_path / 'ws')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_cgan', '--dataset', 'synthetic',
                        '--batch_size', '8', '--epoch_size', '2', '--epochs', '1', '--model_version', 'mean_adjusted',
                        '--dir', ws], env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    argv = ['@' + os.path.join(ws, 'options.config'), '--dir', ws, '--strides', '10', '--frames', '0', '1']
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'paper_fullimage.py')] + argv, env=env, timeout=600,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert [(d['frame'], d['stride'], d['patches']) for d in lines] == [(0, 10, 1518), (1, 10, 1518)]
    for i in (0, 1):
        for kind in ('depth', 'variance', 'montage'):
            assert os.path.getsize(os.path.join(ws, 'images', 'validate_%d_s10_%s.png' % (i, kind))) > 0
    assert os.path.getsize(os.path.join(ws, 'images', 'full_montage_10.png')) > 0
    pf = __import__('paper_fullimage')
    args = pf.parse_args(argv)
    m, _ = pf.build_model(args)
    for (i, image, depth), line in zip(pf.load_frames(args), lines):
        assert m.infer_full(image, depth, stride=10).rmse == line['rmse']
