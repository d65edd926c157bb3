"""improved_sampler without a GPU (hem/models/improved_sampler.py): discovery beside the pinned plugin sets, the flags and the
reference's config files, the recorded graph of every arch pair, every documented refusal, the synthetic source's tuples, and
the float64 oracle of tests/_isamp_ref.py (it differentiates correctly through batch norm and through the RMSE term; its input
assembly and its restated initial variables are what they claim)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _isamp_ref as R

NAME = 'improved_sampler'
GOLDEN = os.path.join(ROOT, 'tests', 'golden', NAME)
PINNED_KNOWN = {'pix2pix', 'paper_cgan', 'paper_sampler', 'paper_noise', 'paper_standalone', 'paper_baseline_standalone',
                'mean_depth_estimator', 'experimental_sampler'}


def plugin():
    return getattr(pkg('models.improved.' + NAME), NAME)


def ns(**kw):
    return SimpleNamespace(batch_size=4, **kw)


# ------------------------------------------------------------------------------------------------ discovery and flags
def test_discovery_leaves_the_pinned_sets_unchanged():
    P = pkg('plugins')
    assert set(P.improved_model_plugins()) == {NAME}
    assert set(P.known_model_plugins()) == PINNED_KNOWN
    assert set(P.every_model_plugin()) == PINNED_KNOWN - {'experimental_sampler'}
    assert set(P.all_model_plugins()) == {'pix2pix', 'paper_cgan', 'paper_sampler', 'paper_noise'}
    assert set(P.accepted_model_plugins()) == PINNED_KNOWN | {NAME}
    assert P.get_model(NAME) is plugin() and pkg('models').get_model(NAME) is plugin() and NAME in pkg('models').model_funcs()
    assert all(P.get_model(n) is c for n, c in P.known_model_plugins().items())
    helps = [a.help for a in pkg('arguments').build_parser()._actions if '--model' in a.option_strings]
    assert NAME in helps[0]


def test_arguments():
    a = plugin().arguments()
    assert set(a) == {'--g_sparsity', '--g_rmse', '--g_arch', '--d_arch', '--examples'}
    assert (a['--g_arch']['default'], a['--d_arch']['default'], a['--examples']['default']) == ('A1', 'A1', 64)
    assert a['--g_sparsity']['default'] is False and a['--g_rmse']['default'] is False


CONFIGS = [('ga1.da1', 'A1', 'A1', [65, 65], False, False), ('ga2.ba1', 'A2', 'A1', [65, 65], False, False),
           ('ga3.da1', 'A3', 'A1', [65, 65], False, False), ('gb2.db2', 'B2', 'B2', [64, 64], False, False),
           ('gd1.dd1', 'D1', 'D1', [64, 64], True, False), ('ge1.de1', 'E1', 'E1', [64, 64], True, True)]


@pytest.mark.parametrize('name,g,d,crop,loc,norm', CONFIGS)
def test_reference_configs_parse_and_build(name, g, d, crop, loc, norm):
    warned = []
    args = pkg('arguments').parse_args(['@' + os.path.join(GOLDEN, name + '.config')], warn=warned.append)
    assert not warned and args.unknown_args == []
    assert (args.model, args.g_arch, args.d_arch, args.g_rmse, args.g_sparsity, args.examples) == (NAME, g, d, False, False, 64)
    assert (args.dataset, args.random_crop, bool(args.include_location), bool(args.normalize)) == ('nyuv2', crop, loc, norm)
    assert (args.epochs, args.batch_size, args.n_gpus, args.optimizer, args.lr, args.beta1) == ('100', 512, 2, 'adam', 1e-5, 0.5)
    assert plugin().check_arch(args) == (g, d)
    # the flags the model's shape error names are the config's own
    S, _, _, P = pkg('models.improved.' + NAME).GEOMETRY[g]
    flags = pkg('models.improved.' + NAME).DATA_FLAGS[P] % (S, S)
    assert ('--include_location' in flags, '--normalize' in flags, '--random_crop %d %d' % tuple(crop) in flags) == (loc, norm, True)


@pytest.mark.parametrize('name,rmse,sparsity', [('ff.rmse', True, True), ('ff.sparsity', False, True)])
def test_ff_configs_parse_then_arch_f_is_refused_by_name(name, rmse, sparsity):
    args = pkg('arguments').parse_args(['@' + os.path.join(GOLDEN, name + '.config')], warn=lambda m: None)
    assert (args.g_arch, args.d_arch, args.g_rmse, args.g_sparsity) == ('F', 'F', rmse, sparsity)
    with pytest.raises(ValueError, match="unknown --g_arch 'F'"):
        plugin().build_graph(args)


# ------------------------------------------------------------------------------------------------ the recorded graphs
@pytest.mark.parametrize('g,d', R.PAIRS)
def test_recorded_graph_has_the_reference_names_and_shapes(g, d):
    nets = plugin().build_graph(ns(g_arch=g, d_arch=d))
    assert set(nets) == {'generator/encoder', 'generator/decoder', 'discriminator/rgb_path', 'discriminator/depth_path',
                         'discriminator/combined_path'}
    got = {net.var_name(l, w): (l.filter_shape if w == 'weights' else (l.out_size,)) for net in nets.values() for l in net.layers
           for w in ('weights', 'bias')}
    assert got == R.shapes(g) and list(got) != []
    E, D = nets['generator/encoder'].layers, nets['generator/decoder'].layers
    K, a = pkg('kernels'), R.ARCHS[g]
    bn = {l.name: net.bn_name(0, i) for net in (nets['generator/encoder'], nets['generator/decoder'])
          for i, l in enumerate(net.layers) if l.use_bn}
    assert bn == R.bn_names(g) and set(bn) == set(a['bn'][0] + a['bn'][1])
    assert E[0].noise == (1, -1.0, 1.0) and E[0].in_size == a['P'] + 1 and E[0].in_shape == (a['S'], a['S'], a['P'] + 1)
    assert not any(l.noise for l in E[1:] + D) and not any(l.fed for l in E + D)
    assert [l.act.code for l in E] == [K.ACT_RELU] * len(E) and [l.act.code for l in D] == [K.ACT_LRELU] * (len(D) - 1) + [K.ACT_TANH]
    rgb, dep, comb = (nets['discriminator/' + p] for p in ('rgb_path', 'depth_path', 'combined_path'))
    assert all(len(n.passes) == 2 for n in (rgb, dep, comb)) and not any(l.use_bn for n in (rgb, dep, comb) for l in n.layers)
    assert rgb.layers[0].in_shape == (a['S'], a['S'], a['P']) and dep.layers[0].in_shape == (a['T'], a['T'], 1)
    assert [l.act.code if l.act else None for l in comb.layers] == [K.ACT_LRELU] * (len(comb.layers) - 1) + [None]
    if a['kind'] == 'A':
        assert [l.out_shape for l in E] == [(31, 31, 64), (14, 14, 128), (5, 5, 256), (1, 1, 512)]
        assert [l.out_shape for l in D] == [(5, 5, 256), (14, 14, 128), (31, 31, 64), (31, 31, 1)]
        assert [(l.k, l.stride, l.padding) for l in E] == [(5, 2, 'VALID')] * 4
        assert [(l.kind, l.k, l.stride, l.padding) for l in D] == [('deconv2d', 5, 2, 'VALID')] * 3 + [('conv2d', 1, 1, 'SAME')]
        assert [l.out_shape for l in rgb.layers] == [(31, 31, 64), (14, 14, 128), (5, 5, 256), (1, 1, 512)]
        assert [l.out_shape for l in dep.layers] == [(14, 14, 128), (5, 5, 256), (1, 1, 512)]
        assert [(l.in_size, l.out_size) for l in comb.layers] == [(1024, 1024), (1024, 512), (512, 1)]
        assert D[3].use_bn == (g == 'A1') and not E[0].use_bn                  # A1's head passes through batch norm; e1 never
    else:
        assert [l.out_shape for l in E] == [(32, 32, 64), (16, 16, 128), (8, 8, 256), (4, 4, 512), (1, 1, 1024)]
        assert [l.out_shape for l in D] == [(4, 4, 512), (8, 8, 256), (16, 16, 128), (32, 32, 64), (32, 32, 1)]
        assert [(l.k, l.stride, l.padding) for l in E] == [(5, 2, 'SAME')] * 4 + [(4, 2, 'VALID')]
        assert [l.out_shape for l in dep.layers] == [(16, 16, 128), (8, 8, 256), (4, 4, 512), (1, 1, 1024)]
        assert [(l.in_size, l.out_size) for l in comb.layers] == [(2048, 1024), (1024, 512), (512, 256), (256, 128), (128, 64), (64, 1)]


def test_e1_has_the_variables_of_experimental_sampler():
    import _xsamp_ref as X
    assert R.shapes('E1') == X.shapes(X.WIDE) and set(R.shapes('E1')) == set(X.G_NAMES + X.D_NAMES)


# ------------------------------------------------------------------------------------------------ refusals
def test_arch_refusals():
    build = plugin().build_graph
    for g, d in (('A1', 'B2'), ('B2', 'A1'), ('D1', 'E1'), ('E1', 'D1'), ('B2', 'D1'), ('A2', 'E1')):
        with pytest.raises(ValueError, match=r'\(A1 \| A2 \| A3, A1\), \(B2, B2\), \(D1, D1\), \(E1, E1\)'):
            build(ns(g_arch=g, d_arch=d))
    for kw in (dict(g_arch='B1', d_arch='B1'), dict(g_arch='C1', d_arch='C1'), dict(g_arch='A1', d_arch='B1'), dict(g_arch='A1', d_arch='C1')):
        with pytest.raises(NotImplementedError, match='36 filter taps.*IG_MAX_TAPS'):
            build(ns(**kw))
    for kw in (dict(g_arch='E2', d_arch='E1'), dict(g_arch='E1', d_arch='E2')):
        with pytest.raises(ValueError, match='--model experimental_sampler'):
            build(ns(**kw))
    for kw in (dict(g_arch='F', d_arch='F'), dict(g_arch='A1', d_arch='F'), dict(g_arch='A2', d_arch='A2'), dict(g_arch='a1', d_arch='A1')):
        with pytest.raises(ValueError, match='unknown --[gd]_arch'):
            build(ns(**kw))
    for g in ('A1', 'A2', 'A3'):
        with pytest.raises(ValueError, match='e5'):
            build(ns(g_arch=g, d_arch='A1', g_sparsity=True))
    for g in ('B2', 'D1', 'E1'):
        build(ns(g_arch=g, d_arch=g, g_sparsity=True, g_rmse=True))


def _shell(g, B=2):
    m = object.__new__(plugin())
    mod = pkg('models.improved.' + NAME)
    m.B, m.g_arch, m.geometry = B, g, mod.GEOMETRY[g]
    S, P = m.geometry[0], m.geometry[3]
    m.n_read = {3: 2, 5: 4, 6: 5}[P]
    m.batch_shapes = [(B, S, S, 3), (B, S, S, 1), (B, S, S, 1), (B, S, S, 1), (B, S, S, 1)][:m.n_read]
    return m


@pytest.mark.parametrize('g,hint', [('A1', '--random_crop 65 65 \\('), ('A3', '--random_crop 65 65 \\('), ('B2', '--random_crop 64 64 \\('),
                                    ('D1', '--random_crop 64 64 --include_location \\('),
                                    ('E1', '--random_crop 64 64 --include_location --normalize \\(')])
def test_batch_shapes_are_checked_with_the_config_flags(g, hint):
    m = _shell(g)
    S = m.geometry[0]
    other = 129 - S
    good = tuple(torch.zeros(s) for s in m.batch_shapes)
    assert len(m._batch(good)) == m.n_read
    longer = good + (torch.zeros(2, 53, 70, 3), torch.zeros(2, 53, 70, 1))
    assert len(m._batch(longer)) == m.n_read                                   # only the leading entries are read
    bad = [good[:-1], good[0], tuple(torch.zeros((2, other, other, s[3])) for s in m.batch_shapes),
           tuple(t[:1] for t in good), good[:1] + (torch.zeros(2, S, S, 3),) + good[2:]]
    for b in bad:
        with pytest.raises(ValueError, match=hint):
            m._batch(b)


@pytest.mark.parametrize('g', list(R.ARCHS))
def test_synthetic_dataset_serves_the_tuple_of_the_arch(g):
    a = R.ARCHS[g]
    args = SimpleNamespace(model=NAME, batch_size=2, g_arch=g)
    sess = SimpleNamespace(device=torch.device('cpu'), rank=0, world_size=1)
    src, count, shape = pkg('plugins').get_dataset('synthetic').get_source(args, sess)
    S = a['S']
    for _ in range(2):
        batch = src.next_batch()
        assert [tuple(t.shape) for t in batch] == [(2, S, S, 3)] + [(2, S, S, 1)] * (R.ENTRIES[a['P']] - 1)
        assert len(_shell(g)._batch(batch)) == R.ENTRIES[a['P']]
        assert float(batch[0].min()) >= 0 and float(batch[1].min()) > 0 and float(batch[1].max()) < 1
        if a['P'] >= 5:
            ramp = np.arange(S) / (S - 1)
            assert np.allclose(batch[2][1, 3, :, 0].numpy(), ramp, atol=1e-7) and np.allclose(batch[3][0, :, 5, 0].numpy(), ramp, atol=1e-7)
        if a['P'] == 6:
            mv = batch[4].numpy()
            assert np.all(mv == mv[:, :1, :1, :]) and np.allclose(mv[:, 0, 0, 0], batch[1].numpy().mean(axis=(1, 2, 3)), atol=1e-6)
    assert shape == (S, S, 3) and count == 8
    # the default arch when the namespace carries none; the other models' sources are untouched
    assert pkg('plugins').get_dataset('synthetic').get_source(SimpleNamespace(model=NAME, batch_size=2), sess)[2] == (65, 65, 3)
    assert len(pkg('plugins').get_dataset('synthetic').get_source(SimpleNamespace(model='experimental_sampler', batch_size=2), sess)[0].next_batch()) == 6


# ------------------------------------------------------------------------------------------------ the oracle
def _narrow_case(g, B=2, seed=3):
    V = R.random_variables(g, R.widths(g, narrow=True), seed, scale=0.5)
    X, y = R.assemble(g, R.Batches(g, B, 1, seed).batch(0))
    S = R.ARCHS[g]['S']
    return V, X, y, np.random.default_rng(seed).uniform(-1, 1, (B, S, S, 1))


@pytest.mark.parametrize('g,rmse,sparsity', [('A1', False, False), ('A1', True, False), ('D1', True, False), ('E1', True, True)])
def test_oracle_differentiates_correctly(g, rmse, sparsity):
    """Central differences in float64 on a narrow copy: along random directions in the critic's and the generator's variables
    (batch-norm betas and A1's head among them) the directional derivative of d_total and of the loss G trains on equals
    <gradient, direction>; both gradient sets come from the SAME forward pass."""
    V, X, y, noise = _narrow_case(g)
    losses, dg, gg, out = R.oracle_grads(g, V, X, y, noise, rmse, sparsity)
    T = R.ARCHS[g]['T']
    assert list(losses) == list(R.loss_keys(rmse, sparsity)) and out.shape == (2, T, T, 1) 
    # tanh is neither flat nor saturated over the batch (a batch-normed head spreads z over several units: only the median is held)
    assert 0.01 < np.median(np.abs(out)) < 0.99 and np.abs(out).max() < 1.0
    assert abs(losses['d_total'] - (losses['d_real'] + losses['d_fake'])) < 1e-15
    assert set(gg) == {k for k in V if k.startswith('generator/')} and set(R.bn_names(g).values()) <= set(gg)
    g_key = 'g_total' if rmse or sparsity else 'g_fake'
    if rmse or sparsity:
        want = losses['g_fake'] - (losses['sparsity_term'] if sparsity else 0.0) + (losses['rmse'] if rmse else 0.0)
        assert abs(losses['g_total'] - want) < 1e-15
    rng = np.random.default_rng(5)
    for grads, key in ((dg, 'd_total'), (gg, g_key)):
        # a conv bias in front of a batch norm has no influence: its gradient is zero up to rounding
        dead = {'generator/%s/vars/%s/bias' % ('encoder' if l[0] == 'e' else 'decoder', l) for l in R.bn_names(g)}
        assert all(np.any(v != 0) for k, v in grads.items() if k not in dead)
        assert all(np.abs(grads[k]).max() < 1e-12 for k in dead if k in grads)
        for _ in range(2):
            direction = {k: rng.standard_normal(v.shape) for k, v in grads.items()}
            analytic = sum(float((grads[k] * direction[k]).sum()) for k in grads)
            eps = 1e-7                           # small against the distance to the nearest (l)relu kink of the 65x65 planes
            vals = []
            for s in (1.0, -1.0):
                Vs = dict(V)
                Vs.update({k: V[k] + s * eps * direction[k] for k in grads})
                vals.append(R.oracle_grads(g, Vs, X, y, noise, rmse, sparsity)[0][key])
            numeric = (vals[0] - vals[1]) / (2 * eps)
            assert abs(numeric - analytic) <= 1e-6 * max(1.0, abs(analytic)), (key, numeric, analytic)


def test_oracle_rmse_gradient_is_the_documented_formula():
    """d rmse / d g = (g - y) / (4 N rmse) on the [-1, 1] tensors, N = B T T: autograd against the closed form."""
    rng = np.random.default_rng(0)
    g = torch.tensor(rng.uniform(-1, 1, (3, 5, 5, 1)), requires_grad=True)
    y = torch.tensor(rng.uniform(-1, 1, (3, 5, 5, 1)))
    rmse = torch.sqrt(torch.mean(torch.square((y + 1) / 2 - (g + 1) / 2)))
    (dg,) = torch.autograd.grad(rmse, [g])
    assert np.allclose(dg.numpy(), ((g - y) / (4 * 75 * rmse)).detach().numpy(), rtol=1e-13, atol=0)


def test_oracle_sparsity_term_counts_exact_zeros_and_has_no_gradient():
    V, X, y, noise = _narrow_case('D1')
    with_s = R.oracle_grads('D1', V, X, y, noise, False, True)
    without = R.oracle_grads('D1', V, X, y, noise, False, False)
    assert all(np.array_equal(with_s[2][k], without[2][k]) for k in without[2]) and 0.0 < with_s[0]['sparsity_term'] < 1.0
    assert with_s[0]['g_total'] == with_s[0]['g_fake'] - with_s[0]['sparsity_term']


@pytest.mark.parametrize('g', ['A1', 'D1', 'E1'])
def test_oracle_input_assembly(g):
    a = R.ARCHS[g]
    b = R.Batches(g, 3, 1, 1).batch(0)
    X, y = R.assemble(g, b, x_rows=[2, 0, 2], y_rows=[0, 0, 0])
    S, T, o, P = a['S'], a['T'], a['off'], a['P']
    assert tuple(X.shape) == (3, S, S, P) and tuple(y.shape) == (3, T, T, 1)
    x32 = b[0].numpy()
    assert np.array_equal(X[0, ..., :3].numpy(), (np.float32(2) * x32[2] - np.float32(1)).astype(np.float64))
    assert np.array_equal(y[1].numpy(), y[0].numpy())
    assert np.array_equal(y[2, ..., 0].numpy(), (np.float32(2) * b[1][0, o:o + T, o:o + T, 0].numpy() - np.float32(1)).astype(np.float64))
    if P >= 5:
        assert np.array_equal(X[1, ..., 3].numpy(), b[2][0, ..., 0].numpy().astype(np.float64))
        assert np.array_equal(X[1, ..., 4].numpy(), b[3][0, ..., 0].numpy().astype(np.float64))
    if P == 6:
        assert np.array_equal(X[..., 5].numpy(), b[4].numpy()[[2, 0, 2], ..., 0].astype(np.float64))
    assert (o, T) == ((17, 31) if S == 65 else (16, 32)) and int((65 - 65 * 0.4769) / 2) == 17      # hem.center_crop(y, 0.4769)


def test_initial_variables_restate_the_engines_draws():
    """tests/_isamp_ref.initial_variables against the engine's own initialiser on a host store, in the model's order."""
    E = pkg('engine')
    for g, d in (('A1', 'A1'), ('D1', 'D1')):
        nets = plugin().build_graph(ns(g_arch=g, d_arch=d))
        store = E.ParamStore(torch.device('cpu'))
        order = [nets[k] for k in ('generator/encoder', 'generator/decoder', 'discriminator/rgb_path', 'discriminator/depth_path',
                                   'discriminator/combined_path')]
        for net in order:
            E.declare_weights(store, net, net.layers)
        store.allocate()
        gen = torch.Generator().manual_seed(0)
        for net in order:
            E.init_weights(store, net, net.layers, gen)
        want, got = store.state_dict(), R.initial_variables(g, 0)
        assert all(np.array_equal(want[k], got[k]) for k in want) and set(got) - set(want) == set(R.bn_names(g).values())
