"""paper_sampler / paper_noise plugin surface without a GPU (hem/models/paper_sampler.py, paper_noise.py): discovery, flags,
the recorded graph of every --noise_layer, the exported symbols and the statistics' NumPy statement."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import pkg
import _sampler_ref as R


def plugin(name='paper_sampler'):
    return getattr(pkg('models.sampler.' + name), name)


def parse(*argv):
    return pkg('arguments').parse_args(['--model', 'paper_sampler', '--batch_size', '4'] + list(argv), warn=lambda m: None)


def test_discovery_finds_both_and_leaves_the_pinned_scans():
    P = pkg('plugins')
    assert P.get_model('paper_sampler') is plugin() and P.get_model('paper_noise') is plugin('paper_noise')
    assert set(P.sampler_model_plugins()) == {'paper_sampler', 'paper_noise'}
    assert set(P.model_plugins()) == {'pix2pix'} and set(P.paper_model_plugins()) == {'paper_cgan'}
    assert set(P.all_model_plugins()) == {'pix2pix', 'paper_cgan', 'paper_sampler', 'paper_noise'}
    funcs = pkg('models').model_funcs()
    assert 'paper_sampler' in funcs and 'paper_noise' in funcs and 'paper_cgan' in funcs


def test_arguments_as_the_reference():
    a = plugin().arguments()
    for k in ('g_lr', 'd_lr'):
        assert a['--' + k]['default'] == 1e-3 and a['--' + k]['type'] is float
    assert [a['--' + k]['default'] for k in ('g_beta1', 'd_beta1', 'g_beta2', 'd_beta2')] == [0.9, 0.9, 0.999, 0.999]
    assert a['--noise_layer']['choices'] == R.NODES and a['--noise_layer']['default'] == 'x'
    assert a['--e_bn'] == {'action': 'store_true', 'default': 'false', 'help': a['--e_bn']['help']}
    n = plugin('paper_noise').arguments()
    assert n['--model_version']['choices'] == ['baseline'] and set(n) == {'--g_lr', '--d_lr', '--g_beta1', '--d_beta1', '--g_beta2',
                                                                           '--d_beta2', '--model_version'}
    globals_ = {s for act in pkg('arguments').build_parser()._actions for s in act.option_strings}
    assert not set(a) & globals_ and not set(n) & globals_


def _encoder_bn(args):
    return [l.use_bn for l in plugin().build_graph(args)['generator/encoder'].layers]


def test_command_line_noise_layer_and_e_bn():
    args = parse('--noise_layer', 'e2')
    assert args.noise_layer == 'e2' and args.e_bn == 'false' and args.e_bn_off is False
    assert _encoder_bn(args) == [True] * 4                   # the string default is truthy: batch norm without the flag
    args = parse('--e_bn')
    assert args.e_bn is True and args.noise_layer == 'x' and _encoder_bn(args) == [True] * 4
    assert _encoder_bn(parse('--e_bn_off')) == [False] * 4
    assert _encoder_bn(parse('--e_bn', '--e_bn_off')) == [False] * 4
    with pytest.raises(SystemExit):
        parse('--noise_layer', 'd1')


@pytest.mark.parametrize('bn', [True, False])
@pytest.mark.parametrize('node', R.NODES)
def test_recorded_graph_per_noise_layer(node, bn):
    args = SimpleNamespace(batch_size=4, noise_layer=node, e_bn='false', e_bn_off=not bn)
    nets = plugin().build_graph(args)
    enc, dec = nets['generator/encoder'], nets['generator/decoder']
    plain = {'e1': 3, 'e2': 64, 'e3': 128, 'e4': 256, 'd1': 512, 'd2': 512, 'd3': 256, 'd4': 128}
    scope, layer, width = R.READER[node]
    for net, sc in ((enc, 'encoder'), (dec, 'decoder')):
        for l in net.layers:
            reads_noise = (sc, l.name) == (scope, layer)
            assert l.in_size == (width if reads_noise else plain[l.name]), (node, l.name)
            assert (l.noise is not None) == reads_noise
            if reads_noise:
                assert l.noise == (R.NOISE_SHAPE[node][2], 0.0, 1.0)         # tf.random_uniform(minval=0, maxval=1)
    assert [l.out_shape for l in enc.layers] == [(31, 31, 64), (14, 14, 128), (5, 5, 256), (1, 1, 512)]
    assert [l.out_shape for l in dec.layers] == [(5, 5, 256), (14, 14, 128), (31, 31, 64), (31, 31, 1)]
    assert [l.use_bn for l in enc.layers] == [bn] * 4 and not any(l.use_bn for l in dec.layers)
    assert [l.act.code for l in enc.layers] == [pkg('kernels').ACT_RELU] * 4
    reader = (enc if scope == 'encoder' else dec)
    spec = next(l for l in reader.layers if l.name == layer)
    assert reader.var_name(spec, 'weights') == 'generator/%s/vars/%s/weights' % (scope, layer)
    shape = spec.filter_shape
    assert shape == ((5, 5, 256, width) if node in ('e4', 'e4-512') else (5, 5, 128, 513) if node == 'd2' else
                     (5, 5, 64, 257) if node == 'd3' else (1, 1, 129, 1) if node == 'd4' else (5, 5, width, spec.out_size))
    if bn:
        assert [enc.bn_name(0, k) for k in range(4)] == [R.bn_beta(k + 1) for k in range(4)]
    # the critic is paper_cgan's, and D(x, y_hat) and D(x, y) share its variables
    rgb, dep, comb = (nets['discriminator/' + s] for s in ('rgb_path', 'depth_path', 'combined_path'))
    assert [l.in_size for l in rgb.layers + dep.layers + comb.layers] == [3, 64, 128, 256, 1, 128, 256, 1024, 1024, 512]
    assert len(rgb.passes) == len(dep.passes) == len(comb.passes) == 2


def test_e2_weights_have_the_reference_shape():
    nets = plugin().build_graph(SimpleNamespace(batch_size=4, noise_layer='e1', e_bn='false', e_bn_off=False))
    enc = nets['generator/encoder']
    assert enc.var_name(enc.layers[1], 'weights') == 'generator/encoder/vars/e2/weights'
    assert enc.layers[1].filter_shape == (5, 5, 65, 128)


def test_paper_noise_is_the_x_case_without_batch_norm():
    nets = plugin('paper_noise').build_graph(SimpleNamespace(batch_size=4, model_version='baseline'))
    enc = nets['generator/encoder']
    assert [l.in_size for l in enc.layers] == [4, 64, 128, 256] and not any(l.use_bn for l in enc.layers)
    assert enc.layers[0].noise == (1, 0.0, 1.0)


def test_new_entry_points_are_exported_and_bound():
    L = pkg('_lib')
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ('tdg_cgan_head_noise_fwd', 'tdg_cgan_head_noise_bwd', 'tdg_cgan_sample_stats',
                 'tdg_cgan_sample_stats_workspace_bytes'):
        assert hasattr(lib, name) and name in L.SIGNATURES
    ws = L.load().tdg_cgan_sample_stats_workspace_bytes
    assert ws(13, 841) == 14 * (13 + 4) * 8 and ws(13, 70) == 2 * 17 * 8 and ws(0, 841) == 0


def test_statistics_statement_agrees_with_the_literal_transcription():
    rng = np.random.default_rng(0)
    n = 7
    y = rng.uniform(0.1, 10, (n, 1, 29, 29))
    g = rng.normal(0, 1, (n, 1, 29, 29))
    p = g + y.mean(axis=(1, 2, 3), keepdims=True)
    got = R.sample_stats(y.reshape(n, -1), g.reshape(n, -1), p.reshape(n, -1))
    np.testing.assert_allclose(got, R.sample_stats_literal(y, g, p), rtol=1e-12, atol=0)
    assert got[1] <= got[0] and got[3] > 0 and got[5] > 0
    same = np.repeat(g[:1], n, axis=0)
    assert R.sample_stats(y.reshape(n, -1), same.reshape(n, -1), same.reshape(n, -1))[3] < 1e-30      # (float64 rounding of v / 10 only)
    assert list(R.STAT_KEYS) == list(pkg('models.sampler.paper_sampler').STAT_KEYS)


def test_infer_full_and_evaluate_are_refused_with_the_reason():
    m = plugin().__new__(plugin())
    for call in (m.infer_full, m.evaluate):
        with pytest.raises(NotImplementedError, match='batch norm'):
            call(None, None)
