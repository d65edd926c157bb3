"""paper_standalone / paper_baseline_standalone plugin surface without a GPU (hem/models/paper_standalone.py,
paper_baseline_standalone.py): discovery, flags, the recorded graph of every version, the exported symbols, and the float64
statements of tests/_standalone_ref.py against torch autograd and tests/_sampler_ref.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg
import _sampler_ref as S
import _standalone_ref as R

NAMES = ('paper_standalone', 'paper_baseline_standalone')


def plugin(name='paper_standalone'):
    return getattr(pkg('models.standalone.' + name), name)


def test_discovery_finds_both_and_leaves_the_pinned_scans():
    P = pkg('plugins')
    assert set(P.standalone_model_plugins()) == set(NAMES)
    for n in NAMES:
        assert P.get_model(n) is plugin(n) and n in pkg('models').model_funcs()
    assert set(P.model_plugins()) == {'pix2pix'} and set(P.paper_model_plugins()) == {'paper_cgan'}
    assert set(P.sampler_model_plugins()) == {'paper_sampler', 'paper_noise'}
    assert set(P.all_model_plugins()) == {'pix2pix', 'paper_cgan', 'paper_sampler', 'paper_noise'}


def test_arguments_as_the_reference():
    a, b = plugin().arguments(), plugin(NAMES[1]).arguments()
    for args in (a, b):
        assert set(args) == {'--g_lr', '--g_beta1', '--g_beta2', '--model_version'}
        assert [args['--' + k]['default'] for k in ('g_lr', 'g_beta1', 'g_beta2')] == [1e-3, 0.9, 0.999]
        assert all(args['--' + k]['type'] is float for k in ('g_lr', 'g_beta1', 'g_beta2'))
        assert args['--model_version']['default'] == 'baseline'
    assert a['--model_version']['choices'] == ['baseline', 'mean_adjusted', 'mean_provided', 'mean_provided2']
    assert b['--model_version']['choices'] == ['baseline', 'mean_adjusted', 'mean_provided']
    globals_ = {s for act in pkg('arguments').build_parser()._actions for s in act.option_strings}
    assert not set(a) & globals_


def test_command_line():
    parse = lambda *argv: pkg('arguments').parse_args(['--batch_size', '4'] + list(argv), warn=lambda m: None)
    args = parse('--model', 'paper_standalone', '--model_version', 'mean_provided2', '--g_lr', '3e-4')
    assert (args.model_version, args.g_lr, args.g_beta1, args.g_beta2) == ('mean_provided2', 3e-4, 0.9, 0.999)
    assert not hasattr(args, 'd_lr') and not hasattr(args, 'training_version')
    assert parse('--model', 'paper_baseline_standalone', '--model_version', 'mean_provided').model_version == 'mean_provided'
    with pytest.raises(SystemExit):
        parse('--model', 'paper_baseline_standalone', '--model_version', 'mean_provided2')


@pytest.mark.parametrize('version', R.VERSIONS)
def test_recorded_graph_per_version(version):
    nets = plugin().build_graph(SimpleNamespace(batch_size=4, model_version=version))
    assert set(nets) == {'generator/encoder', 'generator/decoder'}          # no discriminator/* net
    enc, dec = nets['generator/encoder'], nets['generator/decoder']
    assert [l.in_size for l in enc.layers] == R.ENCODER_WIDTHS[version]
    assert [l.in_size for l in dec.layers] == [512, 512, 256, R.HEAD_WIDTH[version]]
    assert [l.out_shape for l in enc.layers] == [(31, 31, 64), (14, 14, 128), (5, 5, 256), (1, 1, 512)]
    assert [l.out_shape for l in dec.layers] == [(5, 5, 256), (14, 14, 128), (31, 31, 64), (31, 31, 1)]
    assert not any(l.use_bn or l.use_in for l in enc.layers + dec.layers)
    assert not any(l.noise for l in enc.layers + dec.layers)               # nothing is drawn
    K = pkg('kernels')
    assert [l.act.code for l in enc.layers] == [K.ACT_RELU] * 4 and [l.act.code for l in dec.layers[:3]] == [K.ACT_LRELU] * 3
    assert dec.layers[3].act is None
    names = [net.var_name(l, w) for net in (enc, dec) for l in net.layers for w in ('weights', 'bias')]
    assert names == ['generator/%s/vars/%s/%s' % (s, l, w) for s, ls in (('encoder', ('e1', 'e2', 'e3', 'e4')), ('decoder', ('d1', 'd2', 'd3', 'd4')))
                     for l in ls for w in ('weights', 'bias')]
    fed = {l.name: l.fed for l in enc.layers[1:] + dec.layers if l.fed}
    if version == 'mean_provided':
        assert enc.layers[1].filter_shape == (5, 5, 65, 128) and dec.layers[3].filter_shape == (1, 1, 129, 1)
        assert fed == {'e2': (1, 'y_bar'), 'd4': (1, 'y_bar')}
    else:
        assert enc.layers[1].filter_shape == (5, 5, 64, 128) and dec.layers[3].filter_shape == (1, 1, 128, 1) and not fed


def test_baseline_standalone_refuses_the_fourth_version():
    with pytest.raises(ValueError, match='mean_provided2'):
        plugin(NAMES[1]).build_graph(SimpleNamespace(batch_size=4, model_version='mean_provided2'))
    nets = plugin(NAMES[1]).build_graph(SimpleNamespace(batch_size=4, model_version='mean_provided'))
    assert nets['generator/encoder'].layers[1].in_size == 65


def test_paper_cgan_still_refuses_mean_provided_and_records_its_critic():
    pc = pkg('models.paper.paper_cgan')
    with pytest.raises(ValueError, match='variablpe_scope'):
        pc.paper_cgan.build_graph(SimpleNamespace(batch_size=4, model_version='mean_provided'))
    nets = pc.paper_cgan.build_graph(SimpleNamespace(batch_size=4, model_version='mean_provided2'))
    assert {'discriminator/rgb_path', 'discriminator/depth_path', 'discriminator/combined_path'} <= set(nets)
    assert issubclass(pc.CganReplica, pc.GeneratorReplica) and not hasattr(pc.GeneratorReplica, 'd_step')


def test_new_entry_points_are_exported_and_bound():
    L = pkg('_lib')
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ('tdg_cgan_rmse_loss', 'tdg_cgan_rmse_loss_workspace_bytes', 'tdg_cgan_bar_fill'):
        assert hasattr(lib, name) and name in L.SIGNATURES
    ws = L.load().tdg_cgan_rmse_loss_workspace_bytes
    # one f64 partial per block of 1024 elements, at most 1024 blocks (include/tdg.h)
    assert ws(1, 841) == 8 and ws(512, 841) == 8 * 421 and ws(0, 841) == 0 and ws(4096, 841) == 8 * 1024


def test_drivers_accept_the_standalone_models_and_refuse_the_rest():
    import paper_fullimage as pf
    import paper_metrics as pm
    for name in NAMES:
        a = pf.parse_args(['--model', name, '--dataset', 'synthetic', '--model_version', 'mean_provided'])
        assert (a.model, a.model_version) == (name, 'mean_provided')
        assert pm.parse_args(['--model', name, '--dataset', 'synthetic']).model == name
    for cli in (pf, pm):
        with pytest.raises(SystemExit, match='batch norm'):
            cli.parse_args(['--model', 'paper_sampler', '--dataset', 'synthetic'])
        with pytest.raises(SystemExit, match='pix2pix'):
            cli.parse_args(['--model', 'pix2pix', '--dataset', 'synthetic'])


def test_synthetic_dataset_serves_65x65_pairs():
    sess = SimpleNamespace(device=torch.device('cpu'), rank=0, world_size=1)
    for name in NAMES:
        args = pkg('arguments').parse_args(['--model', name, '--dataset', 'synthetic', '--batch_size', '2'], warn=lambda m: None)
        source, n, shape = pkg('plugins').get_dataset('synthetic').get_source(args, sess)
        x, y = source.next_batch()
        assert (n, shape) == (8, (65, 65, 3)) and tuple(x.shape) == (2, 65, 65, 3) and tuple(y.shape) == (2, 65, 65, 1)


# ------------------------------------------------------------------------------------------------ the float64 statements
def test_closed_form_loss_and_gradient_agree_with_autograd_of_the_literal_loss():
    rng = np.random.default_rng(0)
    y = rng.uniform(0.1, 10, (3, 29, 29, 1))
    p = y * rng.uniform(0.5, 1.5, y.shape)
    t = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    loss = R.rmse_literal(torch.tensor(y, dtype=torch.float64), t)
    grad, = torch.autograd.grad(loss, t)
    l, g = R.rmse_closed(y, p)
    np.testing.assert_allclose(l, float(loss.detach()), rtol=1e-12, atol=0)
    np.testing.assert_allclose(g, grad.numpy(), rtol=1e-12, atol=0)
    assert l > 0.01 and np.abs(g).max() > 1e-6


def _variables(version, seed=0):
    rng = np.random.default_rng(seed)
    w = R.ENCODER_WIDTHS[version]
    shapes = {'encoder/vars/e%d' % (k + 1): (5, 5, w[k], co) for k, co in enumerate((64, 128, 256, 512))}
    shapes.update({'decoder/vars/d1': (5, 5, 256, 512), 'decoder/vars/d2': (5, 5, 128, 512), 'decoder/vars/d3': (5, 5, 64, 256),
                   'decoder/vars/d4': (1, 1, R.HEAD_WIDTH[version], 1)})
    P = {}
    for k, s in shapes.items():
        P['generator/%s/weights' % k] = torch.tensor(rng.normal(0, 0.05, s))
        P['generator/%s/bias' % k] = torch.tensor(rng.normal(0, 0.05, s[2] if 'decoder' in k and 'd4' not in k else s[3]))
    return P


def test_generators_reproduce_the_sampler_oracle_where_the_graphs_coincide():
    rng = np.random.default_rng(1)
    x = torch.tensor(rng.uniform(0, 1, (2, 65, 65, 3)))
    ybar = torch.tensor(rng.uniform(1, 9, (2, 1, 1, 1)))
    P = _variables('baseline')
    a = R.oracle_G(P, x, 'baseline', ybar)
    assert tuple(a.shape) == (2, 29, 29, 1)
    assert torch.equal(a, S.oracle_G(P, x, None, False, None)) and torch.equal(a, R.oracle_G(P, x, 'mean_adjusted', ybar))
    P = _variables('mean_provided2')
    assert torch.equal(R.oracle_G(P, x, 'mean_provided2', ybar), S.oracle_G(P, x, 'x', False, torch.ones(2, 65, 65, 1, dtype=torch.float64)))
    # mean_provided: the graph of the sampler's e1 node with the head reading the fed channel too; it depends on y_bar
    P = _variables('mean_provided')
    b = R.oracle_G(P, x, 'mean_provided', ybar)
    assert tuple(b.shape) == (2, 29, 29, 1) and not torch.equal(b, R.oracle_G(P, x, 'mean_provided', ybar + 1.0))
