"""artist without a GPU (hem/models/artist.py): discovery beside the pinned plugin sets, the flag and the reference's config, the
recorded graphs of the three nets, the variable names and how the two stores partition them, the refusals, the new exports of
the C ABI with every argument error of tdg_artist_mse (none launches), the input cast's identity, the jet map, the synthetic
source, and the float64 oracle of tests/_artist_ref.py (it differentiates correctly; its restated initial variables are the
engine's)."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT
import _artist_ref as R

NAME = 'artist'
PINNED_ACCEPTED = {'pix2pix', 'paper_cgan', 'paper_sampler', 'paper_noise', 'paper_standalone', 'paper_baseline_standalone',
                   'mean_depth_estimator', 'experimental_sampler', 'improved_sampler'}


def plugin():
    return getattr(pkg('models.artist.' + NAME), NAME)


def nets():
    return plugin().build_graph(SimpleNamespace(batch_size=4))


# ------------------------------------------------------------------------------------------------ discovery and flags
def test_discovery_leaves_the_pinned_sets_unchanged():
    P = pkg('plugins')
    assert set(P.artist_model_plugins()) == {NAME}
    assert set(P.accepted_model_plugins()) == PINNED_ACCEPTED and set(P.model_plugins()) == {'pix2pix'}
    assert set(P.trainable_model_plugins()) == PINNED_ACCEPTED | {NAME}
    assert P.get_model(NAME) is plugin() and pkg('models').get_model(NAME) is plugin() and NAME in pkg('models').model_funcs()
    assert all(P.get_model(n) is c for n, c in P.accepted_model_plugins().items())
    helps = [a.help for a in pkg('arguments').build_parser()._actions if '--model' in a.option_strings]
    assert NAME in helps[0]


def test_arguments():
    a = plugin().arguments()
    assert set(a) == {'--examples'} and a['--examples']['default'] == 64 and a['--examples']['type'] is int


def test_reference_config_parses():
    warned = []
    args = pkg('arguments').parse_args(['@' + os.path.join(ROOT, 'tests', 'golden', 'artist.config')], warn=warned.append)
    assert not warned and args.unknown_args == []
    assert (args.model, args.examples, args.dataset, args.random_crop) == (NAME, 64, 'nyuv2', [256, 256])
    assert (args.epochs, args.batch_size, args.n_gpus, args.optimizer, args.lr, bool(args.check_numerics)) == ('100', 256, 2, 'rmsprop', 1e-4, True)


# ------------------------------------------------------------------------------------------------ the recorded graphs
def test_recorded_graphs():
    K, N = pkg('kernels'), nets()
    assert list(N) == ['encoder', 'x_decoder', 'y_decoder'] and all(len(n.passes) == 1 for n in N.values())
    E = N['encoder'].layers
    assert [l.name for l in E] == ['e1', 'e2', 'e3', 'e4', 'e5', 'e6']
    assert [(l.kind, l.k, l.stride, l.padding, l.init) for l in E] == [('conv2d', 5, 2, 'VALID', 'xavier')] * 6
    assert [l.in_shape for l in E] == [(256, 256, 3), (126, 126, 6), (61, 61, 12), (29, 29, 24), (13, 13, 48), (5, 5, 192)]
    assert [l.out_shape for l in E] == [(126, 126, 6), (61, 61, 12), (29, 29, 24), (13, 13, 48), (5, 5, 192), (1, 1, 384)]
    assert [l.use_bn for l in E] == [False] + [True] * 5 and not any(l.use_in or l.dropout or l.noise or l.fed for l in E)
    assert [(l.act.code, l.act.leak) for l in E] == [(K.ACT_LRELU, 0.2)] * 6
    for scope, c in R.CHANNELS.items():
        D = N[scope].layers
        assert [l.name for l in D] == ['d1', 'd2', 'd3', 'd4', 'd5', 'd6']
        assert [(l.kind, l.k, l.stride, l.padding, l.init) for l in D] == [('deconv2d', 5, 2, 'VALID', 'xavier')] * 6
        assert [l.in_shape for l in D] == [(1, 1, 384), (5, 5, 192), (13, 13, 48), (29, 29, 24), (61, 61, 12), (126, 126, 6)]
        assert [l.out_shape for l in D] == [(5, 5, 192), (13, 13, 48), (29, 29, 24), (61, 61, 12), (126, 126, 6), (256, 256, c)]
        assert [l.use_bn for l in D] == [True] * 6 and not any(l.use_in or l.dropout or l.noise or l.fed for l in D)
        assert [l.act.code for l in D] == [K.ACT_LRELU] * 5 + [K.ACT_TANH] and all(l.act.leak == 0.2 for l in D[:5])
    # the explicit sides 126 and 256 are one more than the natural ones
    assert (61 - 1) * 2 + 5 == 125 and (126 - 1) * 2 + 5 == 255


def test_variable_names_and_shapes():
    N = nets()
    got = {net.var_name(l, w): (l.filter_shape if w == 'weights' else (l.out_size,)) for net in N.values() for l in net.layers
           for w in ('weights', 'bias')}
    bn = {(net.name, l.name): net.bn_name(0, i) for net in N.values() for i, l in enumerate(net.layers) if l.use_bn}
    assert bn == R.bn_names() and len(bn) == 17
    got.update({name: (N[scope].layers[int(l[1]) - 1].out_size,) for (scope, l), name in bn.items()})
    assert got == R.shapes() and len(got) == 36 + 17
    assert got['encoder/vars/e1/weights'] == (5, 5, 3, 6) and got['x_decoder/vars/d6/bias'] == (3,) and got['y_decoder/vars/d6/weights'] == (5, 5, 1, 6)
    assert bn[('encoder', 'e2')] == 'encoder/BatchNorm/beta' and bn[('y_decoder', 'd6')] == 'y_decoder/BatchNorm_5/beta'


def _bound(B=1):
    m = object.__new__(plugin())
    m.bind(nets(), B, pkg('kernels').F32, torch.device('cpu'), 0)
    return m


def test_the_two_stores_partition_the_variables():
    """:48-49: x_decoder's variables in one store; encoder + y_decoder in the other; nothing shared, nothing left out.  The
    fresh variables are those tests/_artist_ref.initial_variables restates (one generator: encoder, x_decoder, y_decoder)."""
    m = _bound()
    xs, ys = set(m.x_store.index), set(m.y_store.index)
    assert xs == {k for k in R.shapes() if k.startswith(R.X_SET)} and ys == {k for k in R.shapes() if k.startswith(R.Y_SET)}
    assert not xs & ys and xs | ys == set(R.shapes()) and len(xs) == 18 and len(ys) == 35
    assert {k: s for st in (m.x_store, m.y_store) for k, (_, s) in st.index.items()} == R.shapes()
    want = R.initial_variables(0)
    got = dict(m.x_store.state_dict(), **m.y_store.state_dict())
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert all(np.any(got[k] != 0) for k in got if '/vars/' in k) and all(not np.any(got[k]) for k in got if 'BatchNorm' in k)
    # the encoder's output is the y decoder's input, its gradient the y decoder's input gradient; the x decoder has its own
    assert m.E.layers[-1].h is m.Dy.x and m.E.layers[-1].gout is m.Dy.dx and m.Dx.x is not m.Dy.x and m.Dx.dx is None
    assert m.E.dx is None and m.E.store is m.y_store and m.Dy.store is m.y_store and m.Dx.store is m.x_store
    assert [net.layers[-1].h.cs for net in (m.Dx, m.Dy)] == [8, 8] and m.E.x.cs == 8


# ------------------------------------------------------------------------------------------------ refusals
def _shell(B=2):
    m = object.__new__(plugin())
    m.B, m.batch_shapes = B, [(B, 256, 256, 3), (B, 256, 256, 1)]
    return m


def test_batch_shapes_are_checked_with_the_config_flag():
    m = _shell()
    good = tuple(torch.zeros(s) for s in m.batch_shapes)
    assert len(m._batch(good)) == 2 and len(m._batch(good + (torch.zeros(2, 3),))) == 2
    bad = [good[:1], good[0], (torch.zeros(2, 65, 65, 3), torch.zeros(2, 65, 65, 1)), tuple(t[:1] for t in good),
           (good[0], torch.zeros(2, 256, 256, 3)), (good[1], good[0])]
    for b in bad:
        with pytest.raises(ValueError, match=r'--random_crop 256 256 \('):
            m._batch(b)


@pytest.mark.parametrize('n', [0, -1, 0.5])
def test_evaluate_wants_a_batch(n):
    with pytest.raises(ValueError, match='n_batches must be at least 1'):
        _shell().evaluate(None, n)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_signatures_and_library_agree_on_the_new_exports():
    L = pkg('_lib')
    lib = L.load()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'tdg.h')).read(), flags=re.S)
    out = subprocess.check_output(['nm', '-D', '--defined-only', L.LIB_PATH]).decode()
    for name, nargs in (('tdg_artist_mse', 11), ('tdg_artist_mse_workspace_bytes', 0)):
        decl = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
        assert decl, name
        params = [p for p in decl.group(1).split(',') if p.strip() not in ('', 'void')]
        assert len(params) == nargs == len(L.SIGNATURES[name][1]), (name, params)
        assert re.search(r' T %s\b' % name, out), name
    assert L.SIGNATURES['tdg_artist_mse'][0] is C.c_int and L.SIGNATURES['tdg_artist_mse_workspace_bytes'][0] is C.c_size_t
    assert lib.tdg_artist_mse_workspace_bytes() == 8192
    for src in ('build.sh',):
        assert 'tdg_artist' in open(os.path.join(ROOT, '3dgan_amd', 'csrc', src)).read()
    assert 'tdg_artist_mse' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


A = 0x10000                                          # a 16-byte aligned address that no call below may touch
GOOD = dict(dtype=1, target=A, h=A, rows=35, c=3, cs=8, seed=A, scal=A, ws=A, ws_bytes=8192)
EINVAL, EWORKSPACE = -1, -4
BAD = [('null target', dict(target=None), EINVAL), ('null h', dict(h=None), EINVAL), ('null scal', dict(scal=None), EINVAL),
       ('null workspace', dict(ws=None), EINVAL), ('rows 0', dict(rows=0), EINVAL), ('rows -5', dict(rows=-5), EINVAL),
       ('c 0', dict(c=0), EINVAL), ('c 5 of 1..4', dict(c=5), EINVAL), ('c > cs', dict(c=3, cs=0), EINVAL),
       ('cs 12, no multiple of 8', dict(cs=12), EINVAL), ('h misaligned', dict(h=A + 8), EINVAL), ('seed misaligned', dict(seed=A + 2), EINVAL),
       ('target misaligned', dict(target=A + 2), EINVAL), ('workspace misaligned', dict(ws=A + 4), EINVAL), ('dtype 7', dict(dtype=7), EINVAL),
       ('short workspace', dict(ws_bytes=8191), EWORKSPACE), ('no workspace bytes', dict(ws_bytes=0), EWORKSPACE)]


@pytest.mark.parametrize('what,change,code', BAD, ids=[b[0] for b in BAD])
def test_mse_argument_errors_return_their_code_without_a_launch(what, change, code):
    """No GPU here and the pointers lead nowhere: a call that got as far as a launch, or read an argument, would not return
    these codes."""
    lib = pkg('_lib').load()
    a = dict(GOOD, **change)
    rc = lib.tdg_artist_mse(a['dtype'], a['target'], a['h'], a['rows'], a['c'], a['cs'], a['seed'], a['scal'], a['ws'], a['ws_bytes'], None)
    assert rc == code, (what, rc, lib.tdg_last_error())
    msg = lib.tdg_last_error().decode()
    assert 'tdg_artist_mse' in msg or 'dtype' in msg


# ------------------------------------------------------------------------------------------------ small pieces
def test_the_affine_cast_has_the_bits_of_the_rescale():
    """tdg_affine_cast_rows computes scale * (in + shift); at (2, -0.5) that is 2 fl(x - 0.5), and hem.rescale's fl(fl(2 x) - 1)
    is the same float for every float32 x in [0, 1]: 2 x is exact, and doubling commutes with rounding where nothing
    underflows (x - 0.5 is exact within a factor 2 of 0.5, so it never lands in the subnormals).  Checked on every float32 at
    the binade edges, on the ties of the subtraction and on 2**22 random bit patterns of [0, 1]."""
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 0x3f800001, size=1 << 22, dtype=np.uint32)                 # every float32 in [0, 1] is a pattern <= 0x3f800000
    edges = np.concatenate([np.float32(2.0) ** np.arange(-149, 1), np.nextafter(np.float32(2.0) ** np.arange(-126, 1), np.float32(0)),
                            np.nextafter(np.float32(2.0) ** np.arange(-126, 0), np.float32(1)), [0.0, 0.25, 0.5, 0.75, 1.0]]).astype(np.float32)
    near = (np.float32(0.25) + np.arange(-64, 65, dtype=np.float32) * np.float32(2.0 ** -26)).astype(np.float32)      # ties of x - 0.5 below 0.25
    x = np.concatenate([bits.view(np.float32), edges, near, np.float32(0.5) - np.float32(2.0) ** np.arange(-30, -1, dtype=np.float32)])
    assert x.min() >= 0 and x.max() <= 1
    cast = np.float32(2.0) * (x + np.float32(-0.5))
    rescale = np.float32(2.0) * x - np.float32(1.0)
    assert cast.dtype == rescale.dtype == np.float32 and np.array_equal(cast.view(np.uint32), rescale.view(np.uint32))


def test_jet_is_the_fullimage_map():
    import paper_fullimage as pf
    v = np.concatenate([np.linspace(-0.2, 1.2, 57), [0.0, 0.25, 0.5, 0.75, 1.0]]).reshape(2, 31)
    got = pkg('summaries').jet(v)
    assert got.shape == (2, 31, 3) and np.array_equal(got, pf.jet(v)) and got.min() >= 0 and got.max() <= 1
    assert np.array_equal(pkg('summaries').jet(np.array([0.0, 1.0])), [[0, 0, 0.5], [0.5, 0, 0]])


def test_synthetic_dataset_serves_256_pairs():
    sess = SimpleNamespace(device=torch.device('cpu'), rank=0, world_size=1)
    src, count, shape = pkg('plugins').get_dataset('synthetic').get_source(SimpleNamespace(model=NAME, batch_size=1), sess)
    x, y = src.next_batch()
    assert tuple(x.shape) == (1, 256, 256, 3) and tuple(y.shape) == (1, 256, 256, 1) and shape == (256, 256, 3) and count == 4
    assert float(x.min()) >= 0 and float(y.min()) > 0 and float(y.max()) < 1
    assert len(_shell(1)._batch((x, y))) == 2


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_shapes_losses_and_the_round_trip():
    B = 2
    b = R.Batches(B, 1, 3).batch(0)
    V = R.initial_variables(0)
    losses, yg, xg, x01, y01 = R.oracle_grads(V, *b)
    assert list(losses) == list(R.LOSS_KEYS) and x01.shape == (B, 256, 256, 3) and y01.shape == (B, 256, 256, 1)
    assert abs(losses['y_hat_rmse'] - np.sqrt(losses['y_hat_loss'])) < 1e-15 and 0 < x01.min() and x01.max() < 1
    assert set(yg) == {k for k in V if k.startswith(R.Y_SET)} and set(xg) == {k for k in V if k.startswith(R.X_SET)}
    x32 = b[0].numpy()
    assert np.array_equal(R.rescale_in(b[0]).numpy(), (np.float32(2) * x32 - np.float32(1)).astype(np.float64))
    assert np.array_equal(R.target01(b[0]).numpy(), (((np.float32(2) * x32 - np.float32(1)) + np.float32(1)) / np.float32(2)).astype(np.float64))
    assert abs(losses['x_hat_loss'] - np.mean((R.target01(b[0]).numpy() - x01) ** 2)) < 1e-15
    # a conv bias in front of a batch norm has no influence: its gradient is zero up to rounding; every other gradient is live
    dead = R.dead_biases()
    assert len(dead) == 17 and dead <= set(V)
    for grads in (yg, xg):
        assert all(np.any(v != 0) for k, v in grads.items() if k not in dead)
        assert all(np.abs(grads[k]).max() < 1e-12 for k in dead if k in grads)


def test_oracle_differentiates_correctly():
    """Central differences in float64: along a random direction in each variable set the directional derivative of that set's
    loss equals <gradient, direction>; x_hat_loss moves with no encoder variable held in its set, y_hat_loss with no
    x_decoder variable at all."""
    b = R.Batches(2, 1, 4).batch(0)
    rng = np.random.default_rng(5)
    V = {k: v.astype(np.float64) + (rng.uniform(-0.3, 0.3, v.shape) if 'BatchNorm' in k else 0.0) for k, v in R.initial_variables(1).items()}
    losses, yg, xg, _, _ = R.oracle_grads(V, *b)
    for grads, key in ((yg, 'y_hat_loss'), (xg, 'x_hat_loss')):
        direction = {k: rng.standard_normal(v.shape) for k, v in grads.items()}
        analytic = sum(float((grads[k] * direction[k]).sum()) for k in grads)
        eps, vals = 1e-8, []             # small against the distance to the nearest lrelu kink of two million inputs (1e-6 crosses some)
        for s in (1.0, -1.0):
            Vs = dict(V)
            Vs.update({k: V[k] + s * eps * direction[k] for k in grads})
            vals.append(R.oracle_grads(Vs, *b)[0])
        numeric = (vals[0][key] - vals[1][key]) / (2 * eps)
        # 1e-3: of two million lrelu inputs a few lie within the step of their kink and change side between the two evaluations
        # (observed 1e-7 to 1e-4 of the derivative); a wrong factor or a missing term is far outside it
        assert abs(analytic) > 1e-2 and abs(numeric - analytic) <= 1e-3 * abs(analytic), (key, numeric, analytic)
        if key == 'x_hat_loss':
            assert vals[0]['y_hat_loss'] == vals[1]['y_hat_loss'] == losses['y_hat_loss']


def test_oracle_adam_step_is_the_first_tf_step():
    g = np.array([0.5, -2.0, 1e-9])
    v = R.adam_step(np.zeros(3), g, 1e-3, 0.9, 0.999)
    assert np.allclose(v, -1e-3 * g / (np.abs(g) + 1e-8 / np.sqrt(1 - 0.999)), rtol=1e-12, atol=0)
