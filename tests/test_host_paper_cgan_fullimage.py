"""paper_cgan full-frame inference without a GPU: the window grid of paper_fullimage.py's build_batch (patch_grid), the
argument checks of the tdg_cgan_full_* entry points and the paper_fullimage.py command line."""
import ctypes as C
import os

import pytest

from conftest import pkg, ROOT


def patch_grid(*a):
    return pkg('models.paper.paper_cgan').patch_grid(*a)


def reference_corners(H, W, stride):
    """paper_fullimage.py:90-110's loop without the copies: (cols, rows) and the (top, left) of every patch in order."""
    y_lim, x_lim = H, W
    cols = int((y_lim - 65 - 29 + 1) / stride)
    rows = int((x_lim - 65 - 29 + 1) / stride)
    out = []
    x_pos = 0
    y_pos = 0
    for n in range(rows):
        for m in range(cols):
            out.append((x_pos, y_pos))
            x_pos += stride
        x_pos = 0
        y_pos += stride
    return cols, rows, out


@pytest.mark.parametrize('H, W', [(427, 561), (94, 94), (95, 200), (150, 170), (300, 97), (201, 333)])
@pytest.mark.parametrize('s', list(range(1, 13)) + [29, 30])
def test_patch_grid_is_build_batch(H, W, s):
    cols, rows, corners = reference_corners(H, W, s)
    g = patch_grid(H, W, s)
    assert tuple(g) == (cols, rows) and (g.cols, g.rows, g.patches) == (cols, rows, len(corners))
    assert [g.corner(c) for c in range(g.patches)] == corners
    for top, left in corners:                                    # every window inside the frame
        assert top + 65 <= H and left + 65 <= W
    with pytest.raises(IndexError):
        g.corner(g.patches)


def test_patch_grid_nyuv2_counts():
    assert patch_grid(427, 561, 10).patches == 1518
    assert patch_grid(427, 561, 1).patches == 156312
    assert tuple(patch_grid(120, 140, 5)) == (5, 9)
    assert patch_grid(120, 300, 28).patches == 0                  # a 120-pixel side has no window at s >= 28


@pytest.mark.parametrize('H, W, s', [(93, 200, 1), (200, 93, 1), (50, 50, 1), (200, 200, 0), (200, 200, -3)])
def test_patch_grid_rejects(H, W, s):
    with pytest.raises(ValueError):
        patch_grid(H, W, s)


def test_full_kernels_report_bad_arguments():
    """Status + tdg_last_error() before any launch: frames below 94, strides below 1, null pointers, a short store."""
    lib = pkg('_lib').load()
    p = C.c_void_p(4096)                                         # never dereferenced: every call below fails its checks
    assert lib.tdg_cgan_full_gather(p, p, 93, 200, 1, p, 4, p, p, None) == -1 and b'gather' in lib.tdg_last_error()
    assert lib.tdg_cgan_full_gather(p, p, 200, 200, 0, p, 4, p, p, None) == -1
    assert lib.tdg_cgan_full_gather(None, p, 200, 200, 1, p, 4, p, p, None) == -1
    assert lib.tdg_cgan_full_store(None, p, 4, 8, p, p, p, None) == -1 and b'store' in lib.tdg_last_error()
    assert lib.tdg_cgan_full_store(p, None, 4, 2, p, p, p, None) == -1
    assert lib.tdg_cgan_full_blend(p, p, 10 ** 6, 200, 93, 1, 18, p, p, None) == -1
    assert lib.tdg_cgan_full_blend(p, p, 10 ** 6, 200, 200, 0, 18, p, p, None) == -1
    assert lib.tdg_cgan_full_blend(p, p, 10 ** 6, 200, 200, 1, 37, p, p, None) == -1
    assert lib.tdg_cgan_full_blend(p, p, 99, 200, 200, 10, 18, p, p, None) == -1 and b'store holds' in lib.tdg_last_error()
    assert lib.tdg_cgan_full_rmse(p, p, 200, 200, p, p, 8, None) != 0 and b'workspace' in lib.tdg_last_error()
    assert lib.tdg_cgan_full_rmse(p, None, 200, 200, p, p, 4096, None) == -1


# ------------------------------------------------------------------------------------------------ the command line
def cli():
    return __import__('paper_fullimage')


def write_options(path, argv):
    """An options.config as train.py writes it (train.py:208-213 of the reference: `key value` with Python reprs)."""
    import train
    args = train.parse_args(argv)
    with open(path, 'w') as f:
        for a in vars(args):
            if a != 'config':
                f.write('{} {}\n'.format(a, getattr(args, a)))


def test_cli_defaults():
    a = cli().parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--dir', 'w'])
    assert a.strides == [10, 8, 6, 4, 2, 1] and a.split == 'validate' and a.frames == list(range(8))
    assert a.offset == 18 and a.no_images is False and a.model_version == 'baseline' and a.dir == 'w'


def test_cli_flags():
    a = cli().parse_args(['--model', 'paper_cgan', '--dataset', 'nyuv2', '--strides', '4', '1', '--split', 'test', '--frames', '3',
                          '--offset', '17', '--no_images', '--batch_size', '64', '--model_version', 'mean_provided2'])
    assert (a.strides, a.split, a.frames, a.offset, a.no_images) == ([4, 1], 'test', [3], 17, True)
    assert (a.batch_size, a.model_version, a.dataset) == (64, 'mean_provided2', 'nyuv2')


def test_cli_rejects_other_models_and_strides():
    with pytest.raises(SystemExit):
        cli().parse_args(['--model', 'pix2pix', '--dataset', 'synthetic'])
    with pytest.raises(SystemExit):
        cli().parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--strides', '0'])


def test_cli_reads_the_training_options(tmp_path):
    """`@<dir>/options.config` rebuilds the trained model's arguments; flags after it win."""
    ws = str(tmp_path / 'ws')
    opts = str(tmp_path / 'options.config')
    write_options(opts, ['--model', 'paper_cgan', '--dataset', 'synthetic', '--batch_size', '8', '--epoch_size', '2', '--epochs', '1',
                         '--model_version', 'mean_adjusted', '--training_version', 'wgan', '--precision', 'f32', '--seed', '5',
                         '--dir', ws])
    a = cli().parse_args(['@' + opts, '--strides', '10', '--frames', '0', '1'])
    assert (a.model, a.dataset, a.batch_size, a.model_version, a.training_version) == ('paper_cgan', 'synthetic', 8,
                                                                                       'mean_adjusted', 'wgan')
    assert (a.precision, a.seed, a.dir, a.strides, a.frames) == ('f32', 5, ws, [10], [0, 1])
    b = cli().parse_args(['@' + opts, '--batch_size', '16'])
    assert b.batch_size == 16


def test_config_tokens(tmp_path):
    f = tmp_path / 'c.config'
    f.write_text('# a comment\nmodel paper_cgan\nresize [32, 48]\ncache_dir None\ncheck_numerics False\nprofile True\n'
                 'test_epochs []\nunknown_args []\ndir some/where\nlr 0.001\n\n')
    assert cli().config_tokens(str(f)) == ['--model', 'paper_cgan', '--resize', '32', '48', '--profile', '--dir', 'some/where',
                                           '--lr', '0.001']


def test_cli_without_checkpoint_exits(tmp_path):
    a = cli().parse_args(['--model', 'paper_cgan', '--dataset', 'synthetic', '--dir', str(tmp_path)])
    with pytest.raises(SystemExit, match='no checkpoint'):
        cli().build_model(a)


def test_synthetic_frames_are_seeded():
    import numpy as np
    i0, d0 = cli().synthetic_frame('validate', 0)
    i1, d1 = cli().synthetic_frame('validate', 0)
    i2, _ = cli().synthetic_frame('validate', 1)
    assert i0.shape == (427, 561, 3) and d0.shape == (427, 561) and i0.dtype == d0.dtype == np.float32
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1) and not np.array_equal(i0, i2)
    assert 0.0 < d0.min() and d0.max() < 1.0


def test_jet_and_images():
    import numpy as np
    j = cli().jet(np.array([0.0, 0.5, 1.0, 2.0, -1.0]))
    assert np.allclose(j[0], [0, 0, 0.5]) and np.allclose(j[1], [0.5, 1, 0.5]) and np.allclose(j[2], [0.5, 0, 0])
    assert np.array_equal(j[3], j[2]) and np.array_equal(j[4], j[0])
    img = np.zeros((100, 120, 3), np.float32)
    d = np.full((100, 120), 0.5, np.float32)
    yh = np.full((100, 120), 25.0, np.float32)                    # beyond 10: clipped, not wrapped
    g = np.zeros((100, 120), np.float32)
    pred, var, mont = cli().frame_images(img, d, yh, g)
    assert np.array_equal(pred, np.broadcast_to(cli().jet(1.0), pred.shape))
    assert np.all(var == 0) and mont.shape == (100, 480, 3)
