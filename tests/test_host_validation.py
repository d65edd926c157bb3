"""Host side of the validation / test passes and the activation montages: the montage oracle's known answers (the values of
TensorFlow's float-image rule, the layout of hem.montage), the new train.py flags and their refusals, and the base replica's
refusal by name."""
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import pkg, ROOT

import _montage_ref as M


def values(v):
    """The bytes of a 1 x n one-channel image."""
    out, lo, hi = M.montage(np.asarray(v, np.float32).reshape(1, -1, 1))
    return out.reshape(-1).tolist(), lo, hi


def test_known_answers_of_the_value_rule():
    assert values([0, .5, 1]) == ([0, 127, 255], 0.0, 1.0)
    assert values([-1, 0, 1]) == ([1, 128, 255], -1.0, 1.0)
    assert values([-2, 1]) == ([1, 191], -2.0, 1.0)
    assert values([0, 0, 0]) == ([0, 0, 0], 0.0, 0.0)
    assert values([0, 5e-7])[0] == [0, 0]                              # hi below 1e-6: scale 0
    assert values([-5e-7, 2e-7])[0] == [128, 128]                      # the signed branch keeps its offset
    assert values([-3, -1]) == ([1, 85], -3.0, -1.0)                   # all negative: 127 / 3 * -1 + 128 = 85.67


def test_non_finite_pixels_are_255_and_do_not_count():
    got, lo, hi = values([np.nan, 0.25, np.inf, 1.0, -np.inf])
    assert got == [255, 63, 255, 255, 255] and (lo, hi) == (0.25, 1.0)
    got, lo, hi = values([np.nan, np.inf])
    assert got == [255, 255] and (lo, hi) == (0.0, 0.0)


def test_layout_of_six_channels_is_hem_montage():
    S = pkg('summaries')
    assert S.factorization(6) == (2, 3)
    x = np.arange(2 * 2 * 6, dtype=np.float32).reshape(2, 2, 6)         # [h, w, c], hi = 23: integer bytes after truncation
    out, lo, hi = M.montage(x)
    assert out.shape == (3 * 2, 2 * 2) and (lo, hi) == (0.0, 23.0)
    byte = lambda v: int(np.float32(v) * (np.float32(255.0) / np.float32(23.0)))
    for ch in range(6):
        j, i = divmod(ch, 2)                                           # channel j*m + i: block row j, block column i
        block = out[2 * j:2 * j + 2, 2 * i:2 * i + 2]
        assert block.tolist() == [[byte(x[y, xx, ch]) for xx in range(2)] for y in range(2)], ch
    planes = np.transpose(x, (2, 0, 1))
    assert np.array_equal(S.montage(planes)[:, :, 0], S.montage(planes, 2, 3)[:, :, 0])
    assert S.montage(planes)[2:4, 2:4, 0].tolist() == x[:, :, 3].tolist()


def test_png_bytes_u8_keeps_the_samples():
    S, png = pkg('summaries'), pkg('png')
    img = (np.arange(7 * 5) * 7 % 256).astype(np.uint8).reshape(7, 5)
    assert np.array_equal(np.squeeze(png.decode(S.png_bytes_u8(img))), img)
    with pytest.raises(ValueError):
        S.png_bytes_u8(img.astype(np.float32))


def parse(*extra):
    sys.path.insert(0, ROOT)
    import train
    return train.parse_args(['--dataset', 'synthetic'] + list(extra))


def test_flags_parse_and_default_off():
    a = parse('--model', 'paper_cgan')
    assert (a.validation, a.event_montages, a.validation_batches, a.test_epochs) == (False, False, None, [])
    a = parse('--model', 'paper_cgan', '--validation', '--event_files', '--event_montages', '--validation_batches', '3', '--test_epochs', '2', '5')
    assert (a.validation, a.event_montages, a.validation_batches, a.test_epochs) == (True, True, 3, [2, 5])
    for version in ('gan', 'wgan'):
        assert parse('--model', 'paper_cgan', '--validation', '--training_version', version).validation is True


def test_refusals_name_the_flag_or_the_model():
    with pytest.raises(SystemExit) as e:
        parse('--model', 'paper_cgan', '--event_montages')
    assert '--event_files' in str(e.value)
    with pytest.raises(SystemExit) as e:
        parse('--model', 'cnn', '--validation')
    assert 'cnn' in str(e.value) and '\n' not in str(e.value)
    with pytest.raises(SystemExit) as e:
        parse('--model', 'paper_cgan', '--validation', '--n_gpus', '2')
    assert '--n_gpus' in str(e.value) and '\n' not in str(e.value)
    with pytest.raises(SystemExit) as e:
        parse('--model', 'paper_sampler', '--validation')               # it replaces the G step body
    assert 'paper_sampler' in str(e.value)
    with pytest.raises(SystemExit):
        parse('--model', 'paper_cgan', '--validation', '--validation_batches', '0')


def test_the_base_replica_refuses_by_name():
    engine = pkg('engine')
    rep = engine.Replica.__new__(engine.Replica)
    rep.args = SimpleNamespace(model='cnn')
    assert engine.Replica.has_validation() is False and rep.montage_items() == []
    for call in (rep.validation_losses, rep.observe):
        with pytest.raises(NotImplementedError) as e:
            call(None)
        assert 'cnn' in str(e.value)
    cgan = pkg('models.paper.paper_cgan')
    assert cgan.paper_cgan.has_validation() is True
    assert pkg('models.sampler.paper_sampler').paper_sampler.has_validation() is False
