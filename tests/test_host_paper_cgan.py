"""paper_cgan plugin surface without a GPU (hem/models/paper_cgan.py): discovery, flags, configs, recorded layer shapes,
the unbuildable mean_provided, the loss-key sets and the Eigen-2014 metric formulas."""
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import pkg


def plugin():
    return pkg('models.paper.paper_cgan').paper_cgan


def test_discovered_by_name():
    assert pkg('models').get_model('paper_cgan') is plugin()
    assert pkg('plugins').get_model('paper_cgan') is plugin()
    assert set(pkg('plugins').paper_model_plugins()) == {'paper_cgan'}
    assert 'paper_cgan' in pkg('models').model_funcs()


def test_arguments_defaults_and_choices():
    a = plugin().arguments()
    for k in ('g_lr', 'd_lr'):
        assert a['--' + k]['default'] == 1e-3 and a['--' + k]['type'] is float
    for k in ('g_beta1', 'd_beta1'):
        assert a['--' + k]['default'] == 0.9
    for k in ('g_beta2', 'd_beta2'):
        assert a['--' + k]['default'] == 0.999
    assert a['--model_version']['default'] == 'baseline'
    assert a['--model_version']['choices'] == ['baseline', 'mean_adjusted', 'mean_provided', 'mean_provided2']
    assert a['--training_version']['default'] == 'gan'
    assert a['--training_version']['choices'] == ['gan', 'wgan']


def test_flags_do_not_collide_with_global_flags():
    parser = pkg('arguments').build_parser()
    globals_ = {s for act in parser._actions for s in act.option_strings}
    assert not set(plugin().arguments()) & globals_


def test_reference_style_config_parses(tmp_path):
    cfg = tmp_path / 'cgan.config'
    cfg.write_text('# model\nmodel\t\t   paper_cgan\nmodel_version  mean_provided2\ntraining_version wgan\n\n# data\n'
                   'dataset\t\t   nyuv2\nrandom_crop    65 65\nn_threads      8\nskip_invalid\n\n# training\n'
                   'batch_size \t   512\ng_lr\t\t   0.0002\nd_lr 0.0003\ng_beta1 0.5\nd_beta2 0.99\n')
    args = pkg('arguments').parse_args(['@' + str(cfg)])
    assert args.model == 'paper_cgan' and args.model_version == 'mean_provided2' and args.training_version == 'wgan'
    assert list(args.random_crop) == [65, 65] and args.batch_size == 512 and args.n_threads == 8 and args.skip_invalid
    assert (args.g_lr, args.d_lr, args.g_beta1, args.d_beta1, args.g_beta2, args.d_beta2) == (2e-4, 3e-4, 0.5, 0.9, 0.999, 0.99)


def _nets(version):
    return plugin().build_graph(SimpleNamespace(batch_size=4, model_version=version))


def _spatial(net):
    return [net.layers[0].in_shape[0]] + [l.out_shape[0] for l in net.layers]


@pytest.mark.parametrize('version', ['baseline', 'mean_adjusted', 'mean_provided2'])
def test_builders_record_the_layer_shapes(version):
    nets = _nets(version)
    mp2 = version == 'mean_provided2'
    enc, dec = nets['generator/encoder'], nets['generator/decoder']
    rgb, dep, comb = (nets['discriminator/' + s] for s in ('rgb_path', 'depth_path', 'combined_path'))
    assert _spatial(enc) == [65, 31, 14, 5, 1] and _spatial(rgb) == [65, 31, 14, 5, 1]
    assert _spatial(dep) == [29, 13, 5, 1]                       # ceil(25 / 2) = 13, not the comment's 14
    assert [l.out_shape for l in dec.layers] == [(5, 5, 256), (14, 14, 128), (31, 31, 64), (31, 31, 1)]
    assert [l.in_size for l in dec.layers] == [512, 512, 256, 128]          # the skip concats [d_k | e_{4-k}]
    assert [l.kind for l in dec.layers] == ['deconv2d'] * 3 + ['conv2d']
    assert (dec.layers[3].k, dec.layers[3].padding, dec.layers[3].act) == (1, 'SAME', None)
    assert enc.layers[0].in_size == (4 if mp2 else 3) and rgb.layers[0].in_size == (4 if mp2 else 3)
    assert dep.layers[0].in_size == (2 if mp2 else 1)
    assert [(l.in_size, l.out_size) for l in comb.layers] == [(1024, 1024), (1024, 512), (512, 1)]
    assert [l.padding for l in enc.layers + rgb.layers + dep.layers] == ['VALID'] * 11
    assert all(l.init == 'xavier' for n in nets.values() for l in n.layers)
    assert len(rgb.passes) == 2 and len(dep.passes) == 2 and len(comb.passes) == 2      # D(x, y_hat) and D(x, y)
    names = {n.var_name(l, 'weights') for n in nets.values() for l in n.layers}
    assert {'generator/encoder/vars/e1/weights', 'generator/decoder/vars/d4/weights', 'discriminator/rgb_path/vars/hx1/weights',
            'discriminator/depth_path/vars/hy3/weights', 'discriminator/combined_path/vars/h3/weights'} <= names


def test_mean_provided_raises():
    with pytest.raises(ValueError, match='paper_cgan.py:245'):
        _nets('mean_provided')


class _FakeSess:
    world_size = 1

    def report_scalars(self, scal, mean=False):
        return scal


def _loss_dict(wgan, scal):
    import torch
    m = plugin().__new__(plugin())
    m.wgan, m.args, m.sess, m.scal = wgan, SimpleNamespace(), _FakeSess(), torch.tensor(scal, dtype=torch.float32)
    return m._losses()


def test_loss_keys():
    gan = _loss_dict(False, [0, 0, 0, 0, 0.5, 0.25, 2.0, 0])      # tdg_p2p_xent at scal[4..6]: d_real, d_fake, g_fake
    assert list(gan) == ['g_fake', 'd_fake', 'd_real', 'd_total']
    assert (gan['g_fake'], gan['d_fake'], gan['d_real'], gan['d_total']) == (2.0, 0.25, 0.5, 0.75)
    w = _loss_dict(True, [-0.25, 0.25, 0.75, -0.5, 0, 0, 0, 0])
    assert list(w) == ['g_fake', 'd_fake', 'd_fake_1', 'd_total']       # :403 names the real mean 'd_fake' again
    assert (w['g_fake'], w['d_fake'], w['d_fake_1'], w['d_total']) == (-0.25, 0.25, 0.75, -0.5)


def eigen_metrics(y10, p10, counts):
    """hem/models/paper_cgan.py:447-478 in float64 NumPy; counts = running [hits1, hits2, hits3, n] (updated)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        a, p = y10 / 10.0, p10 / 10.0
        d = np.log(a + 1e-8) - np.log(p + 1e-8)
        n = a.size
        q1, q2 = a / p, p / a
        delta = np.where(q1 < q2, q2, q1)
        out = {'abs_rel_diff': np.mean(np.abs(a - p) / p), 'squared_rel_diff': np.mean((a - p) ** 2 / p),
               'linear_rmse': np.sqrt(np.mean((p - a) ** 2)), 'log_rmse': np.sqrt(np.mean(d ** 2)),
               'scale_invariant_log_rmse': np.mean(d ** 2) - np.sum(d) ** 2 / n ** 2}
        counts[3] += n
        for k in range(3):
            counts[k] += int(np.sum(delta < 1.25 ** (k + 1)))
            out['threshold%d' % (k + 1)] = counts[k] / counts[3]
    return out


def test_metric_formulas_and_streaming_thresholds():
    """The NumPy restatement the GPU metrics test checks tdg_cgan_metrics against, on hand-computed values; its key order is
    the plugin's METRIC_KEYS, the order in which metrics() reads the kernel's eight outputs."""
    assert list(eigen_metrics(np.ones(2), np.ones(2), [0, 0, 0, 0])) == list(pkg('models.paper.paper_cgan').METRIC_KEYS)
    y = np.array([[2.0, 4.0], [5.0, 8.0]])
    p = np.array([[2.0, 5.0], [10.0, 6.0]])
    counts = [0, 0, 0, 0]
    m = eigen_metrics(y, p, counts)
    a, q = y.ravel() / 10, p.ravel() / 10
    assert np.isclose(m['abs_rel_diff'], np.mean([0, 0.1 / 0.5, 0.5 / 1.0, 0.2 / 0.6]))
    assert np.isclose(m['linear_rmse'], np.sqrt(np.mean((a - q) ** 2)))
    # ratios 1, 1.25, 2, 1.333: below 1.25 -> 1, below 1.5625 -> 3, below 1.953 -> 3
    assert (m['threshold1'], m['threshold2'], m['threshold3']) == (0.25, 0.75, 0.75)
    m2 = eigen_metrics(np.array([1.0, 1.0]), np.array([1.0, 1.0]), counts)       # streaming: 6 elements in total
    assert counts == [3, 5, 5, 6]
    assert (m2['threshold1'], m2['threshold2']) == (0.5, 5 / 6)
    z = eigen_metrics(np.array([1.0]), np.array([0.0]), [0, 0, 0, 0])            # a zero prediction: inf, as the reference
    assert np.isinf(z['abs_rel_diff']) and z['threshold1'] == 0.0
