"""experimental_sampler without a GPU (hem/models/experimental_sampler.py): discovery, flags and the reference's config file,
the recorded E2 graphs, the documented errors, the float64 oracle of tests/_xsamp_ref.py (it differentiates correctly; its
statistics equal a literal transcription) and the magnitude caps of the exact conv cases of tests/test_gpu_xsamp_convs.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _exact_conv as XC
import _xsamp_ref as R
import test_gpu_xsamp_convs as C
from test_host_conv_exact import test_caps_hold_for_every_gpu_case as caps_hold

NAME = 'experimental_sampler'


def plugin():
    return getattr(pkg('models.experimental.' + NAME), NAME)


# ------------------------------------------------------------------------------------------------ discovery and flags
def test_discovery_by_name_leaves_the_pinned_scans():
    P = pkg('plugins')
    assert set(P.experimental_model_plugins()) == {NAME}
    assert P.get_model(NAME) is plugin() and pkg('models').get_model(NAME) is plugin() and NAME in pkg('models').model_funcs()
    assert set(P.known_model_plugins()) == set(P.every_model_plugin()) | {NAME} and NAME not in P.every_model_plugin()
    helps = [a.help for a in pkg('arguments').build_parser()._actions if '--model' in a.option_strings]
    assert NAME in helps[0]


def test_arguments_and_the_reference_config_file():
    a = plugin().arguments()
    assert set(a) == {'--g_sparsity', '--g_rmse', '--g_arch', '--d_arch', '--examples'}
    assert (a['--g_arch']['default'], a['--d_arch']['default'], a['--examples']['default']) == ('E2', 'E2', 64)
    for flag in ('--g_sparsity', '--g_rmse'):
        assert a[flag]['default'] is False and 'no effect' in a[flag]['help']
    warned = []
    cfg = os.path.join(ROOT, 'tests', 'golden', 'experimental.config')
    args = pkg('arguments').parse_args(['@' + cfg, '--model', NAME], warn=warned.append)
    # one model's flags per parse, as in the reference: the estimator's m_arch is a warned leftover here, g_arch / d_arch below
    assert len(warned) == 1 and args.unknown_args == ['--m_arch', 'E2']
    assert (args.model, args.g_arch, args.d_arch, args.examples, args.g_rmse, args.g_sparsity) == (NAME, 'E2', 'E2', 64, False, False)
    assert (args.dataset, args.random_crop, args.include_originals, args.include_location) == ('nyuv2', [64, 64], [53, 70], True)
    assert (args.epochs, args.batch_size, args.n_gpus, args.optimizer, args.lr, args.beta1) == ('10', 64, 2, 'adam', 1e-5, 0.5)
    # the file names the estimator as its model: the estimator's own flag parses from it too
    est = pkg('arguments').parse_args(['@' + cfg], warn=warned.append)
    assert (est.model, est.m_arch) == ('mean_depth_estimator', 'E2') and '--g_arch' in est.unknown_args


def test_synthetic_dataset_serves_the_64x64_six_tuple():
    args = SimpleNamespace(model=NAME, batch_size=2)
    sess = SimpleNamespace(device=torch.device('cpu'), rank=0, world_size=1)
    src, count, shape = pkg('plugins').get_dataset('synthetic').get_source(args, sess)
    batch = src.next_batch()
    assert [tuple(t.shape) for t in batch] == [(2, 64, 64, 3), (2, 64, 64, 1), (2, 64, 64, 1), (2, 64, 64, 1), (2, 53, 70, 3), (2, 53, 70, 1)]
    assert shape == (64, 64, 3) and count == 8
    m = object.__new__(plugin())
    m.B = 2
    assert len(m._batch(batch)) == 5


# ------------------------------------------------------------------------------------------------ the recorded graph
def test_recorded_graph_has_the_reference_names_and_shapes():
    nets = plugin().build_graph(SimpleNamespace(batch_size=4))
    assert set(nets) == {'generator/encoder', 'generator/decoder', 'discriminator/rgb_path', 'discriminator/depth_path',
                         'discriminator/combined_path'}
    got = {net.var_name(l, w): (l.filter_shape if w == 'weights' else (l.out_size,)) for net in nets.values() for l in net.layers
           for w in ('weights', 'bias')}
    assert got == R.shapes(R.WIDE) and list(R.shapes()) != [] and set(got) == set(R.G_NAMES + R.D_NAMES)
    assert got['generator/encoder/vars/e1/weights'] == (5, 5, 7, 64) and got['generator/encoder/vars/e5/weights'] == (4, 4, 512, 1024)
    assert got['generator/decoder/vars/d1/weights'] == (4, 4, 512, 1024)               # [k, k, Cout, Cin]: 512 outputs from 1024
    assert got['discriminator/rgb_path/vars/hx1/weights'] == (5, 5, 6, 64)
    assert got['discriminator/combined_path/vars/h6/weights'] == (1, 1, 64, 1)
    E, D = nets['generator/encoder'].layers, nets['generator/decoder'].layers
    assert [l.out_shape for l in E] == [(32, 32, 64), (16, 16, 128), (8, 8, 256), (4, 4, 512), (1, 1, 1024)]
    assert [l.out_shape for l in D] == [(4, 4, 512), (8, 8, 256), (16, 16, 128), (32, 32, 64), (32, 32, 1)]       # the head is 32x32, not 31x31
    assert [(l.k, l.stride, l.padding) for l in E] == [(5, 2, 'SAME')] * 4 + [(4, 2, 'VALID')]
    assert [(l.kind, l.k, l.stride, l.padding) for l in D] == [('deconv2d', 4, 2, 'VALID')] + [('deconv2d', 5, 2, 'SAME')] * 3 + \
        [('conv2d', 1, 1, 'SAME')]
    K = pkg('kernels')
    assert [l.act.code for l in E] == [K.ACT_RELU] * 5 and [l.act.code for l in D] == [K.ACT_LRELU] * 4 + [K.ACT_TANH]
    assert E[0].noise == (1, -1.0, 1.0) and not any(l.noise for l in E[1:] + D) and not any(l.use_bn or l.fed for l in E + D)
    assert all(len(nets['discriminator/' + p].passes) == 2 for p in ('rgb_path', 'depth_path', 'combined_path'))
    comb = nets['discriminator/combined_path'].layers
    assert [l.act.code if l.act else None for l in comb] == [K.ACT_LRELU] * 5 + [None]
    assert [l.out_shape for l in nets['discriminator/depth_path'].layers] == [(16, 16, 128), (8, 8, 256), (4, 4, 512), (1, 1, 1024)]


def test_documented_errors():
    for flag in ('g_arch', 'd_arch'):
        with pytest.raises(ValueError, match='E2'):
            plugin().build_graph(SimpleNamespace(batch_size=4, **{flag: 'B2'}))
    m = object.__new__(plugin())
    m.B = 2
    x, y = torch.zeros(2, 64, 64, 3), torch.zeros(2, 64, 64, 1)
    xf, yf = torch.zeros(2, 53, 70, 3), torch.zeros(2, 53, 70, 1)
    x65, y65 = torch.zeros(2, 65, 65, 3), torch.zeros(2, 65, 65, 1)
    for bad in ((x, y), x, (x65, y65, y65, y65, xf, yf), (x, y, y, y, torch.zeros(2, 70, 53, 3), torch.zeros(2, 70, 53, 1)),
                (x[:1], y[:1], y[:1], y[:1], xf[:1], yf[:1])):
        with pytest.raises(ValueError, match='--random_crop 64 64 --include_location --include_originals 53 70'):
            m._batch(bad)


# ------------------------------------------------------------------------------------------------ the oracle
def _narrow_case(B=2, seed=3):
    V = R.random_variables(R.NARROW, seed, scale=0.5)
    rng = np.random.default_rng(seed)
    data = R.Batches(B, 1, seed)
    X, y = R.assemble(data.batch(0), rng.uniform(0.2, 0.8, B))
    return V, X, y, rng.uniform(-1, 1, (B, R.SRC, R.SRC, 1))


def test_oracle_differentiates_correctly():
    """Central differences in float64 on a narrow copy: along random directions in the critic's and the generator's variables
    the directional derivative of d_total / g_fake equals <gradient, direction>; the D gradients come from the SAME forward
    pass as the G gradients (one noise, one batch)."""
    V, X, y, noise = _narrow_case()
    losses, dg, gg, g = R.oracle_grads(V, X, y, noise)
    assert list(losses) == list(R.LOSS_KEYS) and g.shape == (2, 32, 32, 1) and 0.01 < np.abs(g).max() < 0.99
    assert abs(losses['d_total'] - (losses['d_real'] + losses['d_fake'])) < 1e-15
    rng = np.random.default_rng(5)
    for grads, key in ((dg, 'd_total'), (gg, 'g_fake')):
        assert all(np.any(v != 0) for v in grads.values())
        for _ in range(2):
            direction = {k: rng.standard_normal(v.shape) for k, v in grads.items()}
            analytic = sum(float((grads[k] * direction[k]).sum()) for k in grads)
            eps = 1e-6
            vals = []
            for s in (1.0, -1.0):
                Vs = dict(V)
                Vs.update({k: V[k] + s * eps * direction[k] for k in grads})
                vals.append(R.oracle_grads(Vs, X, y, noise)[0][key])
            numeric = (vals[0] - vals[1]) / (2 * eps)
            assert abs(numeric - analytic) <= 1e-6 * max(1.0, abs(analytic)), (key, numeric, analytic)


def test_oracle_losses_and_input_assembly():
    V, X, y, noise = _narrow_case()
    losses, _, _, g = R.oracle_grads(V, X, y, noise)
    g01, y01 = (g + 1) / 2, (y.numpy() + 1) / 2
    assert abs(losses['rmse'] - np.sqrt(np.mean((g01 - y01) ** 2))) < 1e-14 and abs(losses['l1'] - np.mean(np.abs(g01 - y01))) < 1e-14
    data = R.Batches(3, 1, 1)
    b = data.batch(0)
    m = np.array([0.25, 0.5, 0.75])
    X, y = R.assemble(b, m, x_rows=[2, 0, 2], y_rows=[0, 0, 0])
    x32 = b[0].numpy()
    assert np.array_equal(X[0, ..., :3].numpy(), (np.float32(2) * x32[2] - np.float32(1)).astype(np.float64))
    assert np.array_equal(X[..., 5].numpy(), np.broadcast_to(np.array([0.75, 0.25, 0.75])[:, None, None], (3, 64, 64)))
    assert np.array_equal(X[1, ..., 3].numpy(), b[2][0, ..., 0].numpy().astype(np.float64)) and tuple(y.shape) == (3, 32, 32, 1)
    assert np.array_equal(y[1].numpy(), y[0].numpy())
    assert np.array_equal(y[2, ..., 0].numpy(), (np.float32(2) * b[1][0, 16:48, 16:48, 0].numpy() - np.float32(1)).astype(np.float64))
    assert np.array_equal(R.noise_channel([0.0, 0.5, 1.0]), np.array([-1, 0, 1], np.float32))


def test_statistics_restatement_equals_the_literal_transcription():
    rng = np.random.default_rng(0)
    y, g = rng.uniform(-1, 1, (5, 1, 32, 32)), rng.uniform(-1, 1, (5, 1, 32, 32))
    assert np.allclose(R.set_stats(y, g), R.set_stats_literal(y, g), rtol=1e-13, atol=0)
    same = np.repeat(g[:1], 5, axis=0)
    assert R.set_stats(y, same)[1] < 1e-30 < R.set_stats(y, g)[1]               # identical predictions: no variance but the mean's rounding


# ------------------------------------------------------------------------------------------------ the exact conv cases
@pytest.mark.parametrize('case,padding', C.CASES)
def test_exact_conv_cases_satisfy_the_caps(case, padding):
    """The condition of tests/test_gpu_xsamp_convs.py on the oracle alone, at _exact_conv's own keep probability."""
    caps_hold(case, padding)
    assert XC.exact_inputs(case, 0, padding).q == XC.keep_prob(case)
