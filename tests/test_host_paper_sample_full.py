"""Whole-frame sampling of paper_sampler / paper_noise without a GPU: the argument checks of tdg_cgan_full_gather_rep and
tdg_cgan_full_sample_store (status TDG_EINVAL and a message naming the entry point -- a launch without a device would come
back as another status, so -1 also says that nothing was enqueued) and the paper_sample_fullimage.py command line."""
import ctypes as C

import pytest

from conftest import pkg

EINVAL = -1


def lib():
    return pkg('_lib').load()


P = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks


def gather(image=P, depth=P, H=200, W=200, stride=1, chunk=P, batch=8, rep=2, x=P, y=P):
    rc = lib().tdg_cgan_full_gather_rep(image, depth, H, W, stride, chunk, batch, rep, x, y, None)
    return rc, lib().tdg_last_error()


def store(yhat=P, ybar=P, crop=P, batch=8, draws=2, slots=64, chunk=P, st_yhat=P, st_var=P, st_ybar=P, st_err=P):
    rc = lib().tdg_cgan_full_sample_store(yhat, ybar, crop, batch, draws, slots, chunk, st_yhat, st_var, st_ybar, st_err, None)
    return rc, lib().tdg_last_error()


@pytest.mark.parametrize('kw', [{'image': None}, {'chunk': None}, {'x': None}, {'y': None}, {'H': 93}, {'W': 93}, {'H': 50}, {'stride': 0},
                                {'batch': 0}, {'rep': 0}, {'rep': -1}, {'batch': 8, 'rep': 3}])
def test_gather_rep_reports_bad_arguments(kw):
    rc, msg = gather(**kw)
    assert rc == EINVAL and b'tdg_cgan_full_gather_rep' in msg, (kw, rc, msg)
    if 'rep' in kw:
        assert b'rep' in msg.replace(b'tdg_cgan_full_gather_rep', b'')


@pytest.mark.parametrize('kw', [{'yhat': None}, {'chunk': None}, {'st_yhat': None}, {'st_var': None}, {'st_ybar': None}, {'batch': 0},
                                {'draws': 0}, {'batch': 8, 'draws': 3}, {'batch': 8, 'draws': 16}, {'crop': P, 'st_err': None},
                                {'crop': None, 'st_err': P}, {'batch': 8, 'draws': 2, 'slots': 3}])
def test_sample_store_reports_bad_arguments(kw):
    rc, msg = store(**kw)
    assert rc == EINVAL and b'tdg_cgan_full_sample_store' in msg, (kw, rc, msg)


def test_signatures_are_declared():
    S = pkg('_lib').SIGNATURES
    assert len(S['tdg_cgan_full_gather_rep'][1]) == len(S['tdg_cgan_full_gather'][1]) + 1
    assert len(S['tdg_cgan_full_sample_store'][1]) == 12


# ------------------------------------------------------------------------------------------------ the command line
def cli():
    return __import__('paper_sample_fullimage')


def test_cli_refuses_other_models():
    for model in ('paper_cgan', 'paper_standalone', 'pix2pix'):
        with pytest.raises(SystemExit, match='paper_sampler'):
            cli().parse_args(['--model', model, '--dataset', 'synthetic'])


@pytest.mark.parametrize('model', ['paper_sampler', 'paper_noise'])
def test_cli_accepts_the_sampler_models(model):
    a = cli().parse_args(['--model', model, '--dataset', 'synthetic', '--dir', 'w'])
    assert a.model == model and a.strides == [10] and a.split == 'validate' and a.frames == list(range(8))
    assert a.offset == 18 and a.draws is None and a.no_images is False and a.dir == 'w'
    b = cli().parse_args(['--model', model, '--dataset', 'synthetic', '--strides', '4', '1', '--split', 'test', '--frames', '3',
                          '--offset', '17', '--draws', '16', '--no_images', '--batch_size', '64'])
    assert (b.strides, b.split, b.frames, b.offset, b.draws, b.no_images, b.batch_size) == ([4, 1], 'test', [3], 17, 16, True, 64)


def test_cli_rejects_strides_and_draws():
    with pytest.raises(SystemExit, match='strides'):
        cli().parse_args(['--model', 'paper_sampler', '--dataset', 'synthetic', '--strides', '10', '0'])
    with pytest.raises(SystemExit, match='draws'):
        cli().parse_args(['--model', 'paper_sampler', '--dataset', 'synthetic', '--batch_size', '64', '--draws', '48'])


def test_cli_reads_the_training_options(tmp_path):
    from test_host_paper_cgan_fullimage import write_options
    ws, opts = str(tmp_path / 'ws'), str(tmp_path / 'options.config')
    write_options(opts, ['--model', 'paper_sampler', '--noise_layer', 'e2', '--e_bn_off', '--dataset', 'synthetic', '--batch_size', '8',
                         '--dir', ws])
    a = cli().parse_args(['@' + opts, '--strides', '40', '--frames', '0', '--draws', '4'])
    assert (a.model, a.noise_layer, a.e_bn_off, a.batch_size, a.dir, a.strides, a.frames, a.draws) == \
        ('paper_sampler', 'e2', True, 8, ws, [40], [0], 4)


def test_cli_without_checkpoint_exits(tmp_path):
    with pytest.raises(SystemExit, match='no checkpoint'):
        cli().main(['--model', 'paper_sampler', '--dataset', 'synthetic', '--dir', str(tmp_path), '--frames', '0', '--no_images'])


def test_frame_images():
    import numpy as np
    img = np.zeros((100, 120, 3), np.float32)
    d = np.full((100, 120), 0.5, np.float32)
    yh = np.full((100, 120), 25.0, np.float32)
    var = np.zeros((100, 120), np.float32)
    var[50, 60], var[10, 10] = 4.0, 1.0
    pred, grey, mont = cli().frame_images(img, d, yh, var)
    assert np.array_equal(pred, np.broadcast_to(cli().jet(1.0), pred.shape))
    assert grey[50, 60, 0] == 1.0 and grey[10, 10, 0] == 0.25 and grey[0, 0, 0] == 0.0 and mont.shape == (100, 480, 3)
    assert np.all(cli().frame_images(img, d, yh, np.zeros_like(var))[1] == 0)
