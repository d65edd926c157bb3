"""mean_depth_estimator and the nyuv2 outputs it reads, without a GPU (hem/models/mean_depth_estimator.py,
hem/data/nyuv2.py:148-262): discovery, flags, the recorded E2 graph, the batch check, the exported loss entry point, the
three optional nyuv2 outputs on hand-made frames (tests/_mde_frames.py) and the synthetic 6-tuple."""
import ctypes
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _mde_frames as F
import _mde_ref as R

NAME = 'mean_depth_estimator'
CPU = SimpleNamespace(device=torch.device('cpu'), rank=0, world_size=1)


def plugin():
    return getattr(pkg('models.estimator.' + NAME), NAME)


# ------------------------------------------------------------------------------------------------ discovery and flags
def test_discovery_finds_the_estimator_and_leaves_the_pinned_scans():
    P = pkg('plugins')
    assert set(P.estimator_model_plugins()) == {NAME}
    assert P.get_model(NAME) is plugin() and pkg('models').get_model(NAME) is plugin() and NAME in pkg('models').model_funcs()
    assert set(P.all_model_plugins()) == {'pix2pix', 'paper_cgan', 'paper_sampler', 'paper_noise'}
    assert set(P.standalone_model_plugins()) == {'paper_standalone', 'paper_baseline_standalone'}
    assert set(P.every_model_plugin()) == set(P.all_model_plugins()) | set(P.standalone_model_plugins()) | {NAME}
    helps = [a.help for a in pkg('arguments').build_parser()._actions if '--model' in a.option_strings]
    assert NAME in helps[0]


def test_arguments_and_the_merged_command_line():
    a = plugin().arguments()
    assert set(a) == {'--m_arch', '--examples'}
    assert (a['--m_arch']['default'], a['--m_arch']['choices'], a['--examples']['default']) == ('E2', ['E2'], 64)
    parse = lambda *argv: pkg('arguments').parse_args(['--model', NAME] + list(argv), warn=lambda m: None)
    args = parse('--dataset', 'nyuv2', '--random_crop', '65', '65', '--include_location', '--include_originals', '53', '70',
                 '--optimizer', 'adam', '--lr', '3e-4', '--batch_size', '8')
    assert (args.m_arch, args.examples, args.optimizer, args.lr) == ('E2', 64, 'adam', 3e-4)
    assert (args.random_crop, args.include_location, args.normalize, args.include_originals) == ([65, 65], True, False, [53, 70])
    assert not args.unknown_args and not hasattr(args, 'g_lr')
    assert parse('--dataset', 'synthetic', '--examples', '16').examples == 16
    with pytest.raises(SystemExit):
        parse('--dataset', 'synthetic', '--m_arch', 'E1')


def test_nyuv2_help_no_longer_calls_the_flags_ignored():
    a = pkg('plugins').get_dataset('nyuv2').arguments()
    for flag in ('--include_location', '--normalize', '--include_originals'):
        assert 'ignored' not in a[flag]['help'].lower()


# ------------------------------------------------------------------------------------------------ the recorded graph
def test_recorded_graph_of_E2():
    net = plugin().build_graph(SimpleNamespace(batch_size=4, m_arch='E2'))
    assert net.name == 'model' and len(net.passes) == 1
    L = net.layers
    assert [l.name for l in L] == ['l%d' % i for i in range(1, 9)]
    assert [l.kind for l in L] == ['conv2d'] * 6 + ['dense'] * 2
    assert [l.out_shape for l in L[:6]] == [(27, 35, 64), (14, 18, 128), (7, 9, 256), (4, 5, 512), (2, 3, 1024), (1, 2, 2048)]
    assert [l.out_shape[:2] for l in L[:6]] == R.SHAPES
    assert [(l.k, l.stride, l.padding, l.init) for l in L[:6]] == [(5, 2, 'SAME', 'xavier')] * 6
    assert [l.filter_shape for l in L] == [(5, 5, 3, 64), (5, 5, 64, 128), (5, 5, 128, 256), (5, 5, 256, 512), (5, 5, 512, 1024),
                                           (5, 5, 1024, 2048), (4096, 2048), (2048, 1)]
    K = pkg('kernels')
    assert [l.act.code for l in L[:6]] == [K.ACT_RELU] * 6 and L[6].act is None and L[7].act.code == K.ACT_SIGMOID
    assert not any(l.use_bn or l.use_in or l.noise or l.fed for l in L)
    assert [net.var_name(l, w) for l in L for w in ('weights', 'bias')] == R.names()
    # TF's SAME split per axis, as the executor derives it (engine.conv_pads): rows 2/2 and columns 1/2 at the first layer
    pads, (h, w) = [], R.FULL
    for l in L[:6]:
        oh, ow = l.out_shape[:2]
        pads.append(pkg('engine').conv_pads(l, SimpleNamespace(h=h, w=w), SimpleNamespace(h=oh, w=ow)))
        h, w = oh, ow
    sizes, want = R.FULL, []
    for _ in range(6):
        want.append((R.same_pads(sizes[0])[0], R.same_pads(sizes[1])[0]))
        sizes = (-(-sizes[0] // 2), -(-sizes[1] // 2))
    assert pads == want and (R.same_pads(53), R.same_pads(70)) == ((2, 2), (1, 2))
    assert sum(int(np.prod(l.filter_shape)) + l.out_size for l in L) == 78_238_337


def test_a_narrow_copy_keeps_names_and_structure():
    narrow = type('narrow', (plugin(),), {'WIDTHS': R.NARROW})
    net = narrow.build_graph(SimpleNamespace(batch_size=4))
    assert [l.out_shape for l in net.layers[:6]] == [s + (c,) for s, c in zip(R.SHAPES, R.NARROW)]
    assert [l.filter_shape for l in net.layers[6:]] == [(64, 16), (16, 1)]
    assert [net.var_name(l, w) for l in net.layers for w in ('weights', 'bias')] == R.names()
    with pytest.raises(ValueError, match='m_arch'):
        plugin().build_graph(SimpleNamespace(batch_size=4, m_arch='E1'))


def test_batches_without_53x70_originals_are_refused():
    m = object.__new__(plugin())
    m.B = 2
    x, y = torch.zeros(2, 65, 65, 3), torch.zeros(2, 65, 65, 1)
    xf, yf = torch.zeros(2, 53, 70, 3), torch.zeros(2, 53, 70, 1)
    got = m._originals((x, y, y, y, xf, yf))
    assert got[0] is xf and got[1] is yf
    for bad in ((x, y), x, (x, y, torch.zeros(2, 70, 53, 3), torch.zeros(2, 70, 53, 1)), (x, y, xf, torch.zeros(2, 53, 70, 3)),
                (x, y, xf[:1], yf[:1])):
        with pytest.raises(ValueError, match='--include_originals 53 70'):
            m._originals(bad)


def test_loss_entry_point_is_exported_and_bound():
    L = pkg('_lib')
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ('tdg_mde_loss', 'tdg_mde_loss_workspace_bytes'):
        assert hasattr(lib, name) and name in L.SIGNATURES
    ws = L.load().tdg_mde_loss_workspace_bytes
    assert (ws(1), ws(512), ws(0), ws(-3)) == (8, 4096, 0, 0)
    assert len(L.SIGNATURES['tdg_mde_loss'][1]) == 13


def test_oracle_loss_is_the_mean_absolute_difference():
    rng = np.random.default_rng(0)
    y = torch.tensor(rng.uniform(0.1, 0.9, (5, 53, 70, 1)))
    m = torch.tensor(rng.uniform(0.1, 0.9, 5), requires_grad=True)
    loss = R.loss_literal(m, y)
    g, = torch.autograd.grad(loss, m)
    d = m.detach().numpy() - y.numpy().mean(axis=(1, 2, 3))
    np.testing.assert_allclose(float(loss.detach()), np.abs(d).mean(), rtol=1e-14)
    np.testing.assert_allclose(g.numpy(), np.sign(d) / 5, rtol=1e-12)
    mean32, l32, sign = R.mde_loss_ref(y.numpy().reshape(5, -1).astype(np.float32), m.detach().numpy().astype(np.float32))
    assert abs(float(l32) - float(loss.detach())) < 1e-6 and np.array_equal(sign, np.sign(d))


# ------------------------------------------------------------------------------------------------ nyuv2 outputs
FLAGS = list(itertools.product((False, True), repeat=3))             # (location, normalize, originals)
FULL = (13, 17)


def _expected_length(case, loc, norm, orig):
    return 2 + (2 if loc and F.CASES[case]['random_crop'] else 0) + (1 if norm else 0) + (2 if orig else 0)


@pytest.mark.parametrize('loc,norm,orig', FLAGS)
def test_tuple_length_order_and_values(loc, norm, orig):
    """Every flag combination on the crop case: (x, y [, x_loc, y_loc] [, mean_vec] [, x_full, y_full]); the pair is what the same
    seed gives with no flag set (the extras draw nothing), the ramps are c / (W - 1) and r / (H - 1) at the drawn window, mean_vec
    is the image's mean, the originals are TF-1.x bilinear resizes of the drawn frames."""
    flags = dict(location=loc, normalize=norm, originals=FULL if orig else None)
    rgb, depth = F.frames()
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'nyuv2_pairs_parent.npz'))
    src = F.source('crop', flags)
    for b in range(F.GOLDEN_BATCHES):
        t = [a.numpy() for a in src.next_batch()]
        assert len(t) == _expected_length('crop', loc, norm, orig) and all(a.dtype == np.float32 for a in t)
        x, y = t[0], t[1]
        assert np.array_equal(x, gold['crop/x%d' % b]) and np.array_equal(y, gold['crop/y%d' % b])
        ch, cw = F.CASES['crop']['random_crop']
        rest = t[2:]
        # which frame and window each pair came from: the depth crop is unique in the hand-made frames
        where = [_locate(depth, y[i, :, :, 0]) for i in range(F.GOLDEN_B)]
        if loc:
            x_loc, y_loc, rest = rest[0], rest[1], rest[2:]
            assert x_loc.shape == y_loc.shape == (F.GOLDEN_B, ch, cw, 1)
            for i, (_, top, left) in enumerate(where):
                want_x = np.float32((left + np.arange(cw)) / (F.W - 1))
                want_y = np.float32((top + np.arange(ch)) / (F.H - 1))
                assert np.array_equal(x_loc[i, :, :, 0], np.broadcast_to(want_x[None, :], (ch, cw)))
                assert np.array_equal(y_loc[i, :, :, 0], np.broadcast_to(want_y[:, None], (ch, cw)))
        if norm:
            mean_vec, rest = rest[0], rest[1:]
            assert mean_vec.shape == y.shape
            want = y.astype(np.float64).mean(axis=(1, 2, 3))
            assert np.array_equal(mean_vec, np.broadcast_to(mean_vec[:, :1, :1, :], y.shape))
            np.testing.assert_allclose(mean_vec[:, 0, 0, 0], want, rtol=1e-6, atol=0)
        if orig:
            x_full, y_full = rest
            assert x_full.shape == (F.GOLDEN_B,) + FULL + (3,) and y_full.shape == (F.GOLDEN_B,) + FULL + (1,)
            idx = [f for f, _, _ in where]
            np.testing.assert_allclose(x_full, R.resize_tf1(rgb[idx], *FULL) / 255.0, rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(y_full, R.resize_tf1(depth[idx][..., None], *FULL) / 65535.0, rtol=1e-6, atol=1e-7)
        else:
            assert not rest


def _locate(depth, crop01):
    """(frame, top, left) of a [ch, cw] depth crop in [0, 1] among the uint16 frames."""
    ch, cw = crop01.shape
    first = np.float32(depth.astype(np.float32) / np.float32(65535.0))
    hits = np.argwhere(first[:, :depth.shape[1] - ch + 1, :depth.shape[2] - cw + 1] == crop01[0, 0])
    found = [(int(f), int(r), int(c)) for f, r, c in hits if np.array_equal(first[f, r:r + ch, c:c + cw], crop01)]
    assert len(found) == 1, found
    return found[0]


@pytest.mark.parametrize('case', sorted(F.CASES))
def test_no_flag_set_is_bit_equal_to_the_parent_commit(case):
    """tests/golden/nyuv2_pairs_parent.npz (tests/golden/make_nyuv2_pairs.py, run on the commit before the three outputs
    existed): the same two tensors from the same generator draws, with no flag and with every flag set."""
    gold = np.load(os.path.join(ROOT, 'tests', 'golden', 'nyuv2_pairs_parent.npz'))
    for flags in (None, dict(location=True, normalize=True, originals=FULL)):
        src = F.source(case, flags)
        for b in range(F.GOLDEN_BATCHES):
            t = src.next_batch()
            assert isinstance(t, tuple) and len(t) == (2 if flags is None else _expected_length(case, True, True, True))
            assert np.array_equal(t[0].numpy(), gold['%s/x%d' % (case, b)]) and np.array_equal(t[1].numpy(), gold['%s/y%d' % (case, b)])


def test_location_follows_resize_and_needs_a_crop():
    """With --resize the ramps are resized like the pair before the window is cut (:188-190); without --random_crop no
    location channel is emitted (:245)."""
    t = F.source('resize', dict(location=True)).next_batch()
    assert len(t) == 2
    src = F.source('resize_crop', dict(location=True))
    x, y, x_loc, y_loc = (a.numpy() for a in src.next_batch())
    w, h = F.CASES['resize_crop']['resize']
    ch, cw = F.CASES['resize_crop']['random_crop']
    ramp_x = np.broadcast_to((np.arange(F.W) / (F.W - 1))[None, :], (F.H, F.W)).astype(np.float32)
    ramp_y = np.broadcast_to((np.arange(F.H) / (F.H - 1))[:, None], (F.H, F.W)).astype(np.float32)
    rx, ry = (R.resize_tf1(r[None, :, :, None], h, w)[0, :, :, 0] for r in (ramp_x, ramp_y))
    _, depth = F.frames()
    small = np.float32(R.resize_tf1(depth[..., None], h, w)[..., 0] / 65535.0)
    for i in range(F.GOLDEN_B):
        # the window: where this pair's location crop sits in the resized ramps (they are strictly increasing)
        left = int(np.argmin(np.abs(rx[0] - x_loc[i, 0, 0, 0])))
        top = int(np.argmin(np.abs(ry[:, 0] - y_loc[i, 0, 0, 0])))
        np.testing.assert_allclose(x_loc[i, :, :, 0], rx[top:top + ch, left:left + cw], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(y_loc[i, :, :, 0], ry[top:top + ch, left:left + cw], rtol=1e-6, atol=1e-7)
        errs = [np.abs(small[f, top:top + ch, left:left + cw] - y[i, :, :, 0]).max() for f in range(F.N)]
        assert min(errs) < 1e-6, 'the depth crop does not sit at the location crop\'s window'


def test_get_source_passes_the_flags_on(tmp_path):
    rgb, depth = F.frames()
    F.write_tfrecords(str(tmp_path / 'datasets' / 'nyuv2.train.tfrecords'), rgb, depth)
    args = SimpleNamespace(dataset_dir=str(tmp_path / 'datasets'), cache_dir=None, data_dir=str(tmp_path), batch_size=2, seed=1,
                           random_crop=[65, 65], resize=None, include_location=True, normalize=True, include_originals=[53, 70])
    src, n, shape = pkg('plugins').get_dataset('nyuv2').get_source(args, CPU)
    t = src.next_batch()
    assert (n, shape) == (F.N, (65, 65, 3))
    assert [tuple(a.shape) for a in t] == [(2, 65, 65, 3)] + [(2, 65, 65, 1)] * 4 + [(2, 53, 70, 3), (2, 53, 70, 1)]
    assert src.full[0].shape == (F.N, 53, 70, 3)                       # every frame resized once, when the source is built
    before = src.full[0].data_ptr()
    src.next_batch()
    assert src.full[0].data_ptr() == before


# ------------------------------------------------------------------------------------------------ synthetic source
def test_synthetic_dataset_serves_the_six_tuple():
    args = pkg('arguments').parse_args(['--model', NAME, '--dataset', 'synthetic', '--batch_size', '8'], warn=lambda m: None)
    source, n, shape = pkg('plugins').get_dataset('synthetic').get_source(args, CPU)
    assert (n, shape) == (32, (65, 65, 3))
    means = []
    for _ in range(4):
        t = source.next_batch()
        assert [tuple(a.shape) for a in t] == [(8, 65, 65, 3), (8, 65, 65, 1), (8, 65, 65, 1), (8, 65, 65, 1), (8, 53, 70, 3), (8, 53, 70, 1)]
        assert all(a.dtype == torch.float32 for a in t)
        assert float(t[1].min()) > 0 and float(t[1].max()) < 1 and float(t[5].min()) > 0 and float(t[5].max()) < 1
        assert np.array_equal(t[2][0, :, :, 0].numpy(), np.broadcast_to(np.float32(np.arange(65) / 64)[None, :], (65, 65)))
        assert np.array_equal(t[3][0, :, :, 0].numpy(), np.broadcast_to(np.float32(np.arange(65) / 64)[:, None], (65, 65)))
        means += t[5].mean(dim=(1, 2, 3)).tolist()
    assert min(means) > 0.08 and max(means) < 0.92 and max(means) - min(means) > 0.4 and len(set(means)) == len(means)
    other = pkg('data').SyntheticEstimatorSource(4, 8, 'cpu', rank=1).next_batch()
    assert not torch.equal(other[5], pkg('data').SyntheticEstimatorSource(4, 8, 'cpu', rank=0).next_batch()[5])


# ------------------------------------------------------------------------------------------------ the GPU parity test's inputs
def test_parity_inputs_keep_clear_of_every_kink_on_the_oracle_alone():
    """tests/test_gpu_mean_depth.py compares three Adam steps of a narrow copy against the float64 oracle.  On the oracle alone,
    at the variables of each step: every |mean_i - m_i| exceeds 0.05 (the absolute value's kink), the depth means lie in
    [0.05, 0.2] or [0.8, 0.95], and the small layers' relu inputs stay 1e-6 away from zero."""
    narrow = type('narrow', (plugin(),), {'WIDTHS': R.NARROW})
    v0 = R.initial_variables(narrow, R.PARITY_SEED)
    src = R.Originals(R.PARITY_B, R.PARITY_STEPS + 1, R.PARITY_SEED)
    batches = [(src.x[i], src.y[i]) for i in range(1, R.PARITY_STEPS + 1)]
    steps, _ = R.trajectory(v0, batches)
    for (v, loss, grads, m, means), (x, y) in zip(steps, batches):
        assert np.all((means > 0.05) & (means < 0.2) | (means > 0.8) & (means < 0.95)), means
        assert np.abs(means - m).min() > 0.05, (means, m)
        assert R.nearest_kink(v, x) > 1e-6
        assert all(np.any(g != 0) for g in grads.values())
    assert R.nearest_kink(v0, src.x[0]) > 1e-6
