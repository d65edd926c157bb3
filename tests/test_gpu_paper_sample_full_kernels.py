"""The two kernels of whole-frame sampling (tdg_cgan_full.hip) on the GPU: tdg_cgan_full_gather_rep against NumPy slices
of the frame and against tdg_cgan_full_gather, tdg_cgan_full_sample_store against float64 NumPy and _sampler_ref.sample_stats."""
import numpy as np
import pytest
import torch

import _sampler_ref as R
from test_gpu_paper_cgan import DEV, K, L, dev
from test_gpu_paper_cgan_fullimage import frame, grid
from test_gpu_paper_sampler import stats_within

pytestmark = pytest.mark.gpu
HW = 29 * 29


def f32(*shape, fill=0.0):
    return torch.full(shape, fill, dtype=torch.float32, device=DEV)


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ gather
FRAMES = {(95, 101, 2): (1, 4), (100, 107, 3): (2, 4)}


@pytest.mark.parametrize('rep', [1, 2, 3, 6])
@pytest.mark.parametrize('shape', list(FRAMES))
def test_gather_rep_is_the_window_repeated(shape, rep):
    H, W, s = shape
    B = 6
    g = grid(H, W, s)
    assert tuple(g) == FRAMES[shape]
    P, G = g.patches, B // rep
    image, depth = frame(H, W, 11)
    d_image, d_depth = dev(image), dev(depth)
    chunks = sorted({0, (P - 1) // G, -(-P // G)})                # the first, the last (partial unless G divides P), one past the grid
    for chunk in chunks:
        x, y, y0 = f32(B, 65, 65, 3, fill=7.0), f32(B, 65, 65, 1, fill=7.0), f32(B, 65, 65, 1, fill=7.0)
        ch = i32(chunk)
        L().call('tdg_cgan_full_gather_rep', K().ptr(d_image), K().ptr(d_depth), H, W, s, K().ptr(ch), B, rep, K().ptr(x), K().ptr(y),
                 K().stream())
        gx, gy = x.cpu().numpy(), y.cpu().numpy()
        for b in range(B):
            c = chunk * G + b // rep
            if c < P:
                top, left = g.corner(c)
                assert np.array_equal(gx[b], image[top:top + 65, left:left + 65]), (chunk, b, c)
                assert np.array_equal(gy[b, ..., 0], depth[top:top + 65, left:left + 65]), (chunk, b, c)
            else:
                assert np.all(gx[b] == 0) and np.all(gy[b] == 0), (chunk, b, c)
        assert int(ch.item()) == chunk                           # the gather reads the index, the store advances it
        if chunk == chunks[-1]:
            assert np.all(gx == 0) and np.all(gy == 0)
        # a null depth: the same x, a zero y
        x.fill_(7.0)
        L().call('tdg_cgan_full_gather_rep', K().ptr(d_image), None, H, W, s, K().ptr(ch), B, rep, K().ptr(x), K().ptr(y0), K().stream())
        assert np.array_equal(x.cpu().numpy(), gx) and np.all(y0.cpu().numpy() == 0)
        if rep == 1:                                             # bit-equal to the entry point it generalises
            x1, y1 = f32(B, 65, 65, 3, fill=7.0), f32(B, 65, 65, 1, fill=7.0)
            L().call('tdg_cgan_full_gather', K().ptr(d_image), K().ptr(d_depth), H, W, s, K().ptr(ch), B, K().ptr(x1), K().ptr(y1),
                     K().stream())
            assert np.array_equal(x1.cpu().numpy(), gx) and np.array_equal(y1.cpu().numpy(), gy)


def test_gather_rep_fills_a_wide_batch():
    """More windows and copies than one block or one copy slice holds: 16 windows x 12 copies, every row checked."""
    H, W, s, B, rep = 100, 107, 3, 192, 12
    g = grid(H, W, s)
    image, depth = frame(H, W, 12)
    x, y = f32(B, 65, 65, 3, fill=7.0), f32(B, 65, 65, 1, fill=7.0)
    L().call('tdg_cgan_full_gather_rep', K().ptr(dev(image)), K().ptr(dev(depth)), H, W, s, K().ptr(i32(0)), B, rep, K().ptr(x), K().ptr(y),
             K().stream())
    gx, gy = x.cpu().numpy(), y.cpu().numpy()
    for b in range(B):
        c = b // rep
        if c < g.patches:
            top, left = g.corner(c)
            assert np.array_equal(gx[b], image[top:top + 65, left:left + 65]) and np.array_equal(gy[b, ..., 0], depth[top:top + 65, left:left + 65])
        else:
            assert np.all(gx[b] == 0) and np.all(gy[b] == 0)


# ------------------------------------------------------------------------------------------------ store
def run_store(yhat, ybar, crop, B, draws, slots, chunk, rows):
    """One call on stores of `rows` >= slots rows filled with a sentinel; (store_yhat, store_var, store_ybar, store_err, chunk)."""
    sy, sv, sb, se = f32(rows, HW, fill=-7.0), f32(rows, HW, fill=-7.0), f32(rows, fill=-7.0), f32(rows, 2, fill=-7.0)
    ch = i32(chunk)
    L().call('tdg_cgan_full_sample_store', K().ptr(yhat), K().ptr(ybar), K().ptr(crop), B, draws, slots, K().ptr(ch), K().ptr(sy), K().ptr(sv),
             K().ptr(sb), K().ptr(se) if crop is not None else None, K().stream())
    return sy.cpu().numpy(), sv.cpu().numpy(), sb.cpu().numpy(), se.cpu().numpy(), int(ch.item())


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('draws', [1, 3, 8, 9, 17])
def test_sample_store(draws, groups):
    B = draws * groups
    rng = np.random.default_rng([draws, groups])
    offs = rng.uniform(1.0, 8.0, (groups, 1, 1))
    yhat = (offs + 0.3 * rng.standard_normal((groups, draws, HW))).astype(np.float32).reshape(B, HW)
    crop = rng.uniform(0.1, 9.9, (B, HW)).astype(np.float32)
    ybar = rng.uniform(0.0, 9.0, B).astype(np.float32)
    d_yhat, d_crop, d_ybar = dev(yhat), dev(crop), dev(ybar)
    slots, rows, chunk = 2 * groups, 2 * groups + 2, 1           # chunk 1 fills slots [groups, 2 groups): the last that fit
    sy, sv, sb, se, after = run_store(d_yhat, d_ybar, d_crop, B, draws, slots, chunk, rows)
    assert after == chunk + 1
    y64 = yhat.astype(np.float64).reshape(groups, draws, HW)
    lo, hi = groups, 2 * groups
    stats_within(sy[lo:hi], y64.mean(axis=1), 'mean')
    stats_within(sv[lo:hi], y64.var(axis=1) / 100.0, 'variance')
    if draws == 1:
        assert np.all(sv[lo:hi] == 0.0) and np.array_equal(sy[lo:hi], yhat)
    else:
        assert np.all(sv[lo:hi] > 0.0)
    for k in range(groups):
        rows_k = slice(k * draws, (k + 1) * draws)
        stats_within(se[lo + k], R.sample_stats(crop[rows_k], yhat[rows_k], yhat[rows_k])[:2], 'errors of group %d' % k)
        assert sb[lo + k] == ybar[k * draws]
    for a in (sy, sv, sb, se):                                   # the slots before and after the call's range keep the sentinel
        assert np.all(a[:lo] == -7.0) and np.all(a[hi:] == -7.0)
    # two launches are bit-equal
    again = run_store(d_yhat, d_ybar, d_crop, B, draws, slots, chunk, rows)
    assert all(np.array_equal(a, b) for a, b in zip((sy, sv, sb, se), again[:4]))
    # a chunk whose slots pass `slots` writes nothing and still advances
    ny, nv, nb, ne, after = run_store(d_yhat, d_ybar, d_crop, B, draws, slots, 2, rows)
    assert after == 3 and all(np.all(a == -7.0) for a in (ny, nv, nb, ne))
    # no crop: the same mean and variance, no errors; no y_bar: zeros
    py, pv, pb, pe, _ = run_store(d_yhat, None, None, B, draws, slots, chunk, rows)
    assert np.array_equal(py, sy) and np.array_equal(pv, sv) and np.all(pe == -7.0)
    assert np.all(pb[lo:hi] == 0.0) and np.all(pb[:lo] == -7.0) and np.all(pb[hi:] == -7.0)
