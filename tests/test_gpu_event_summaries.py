"""The event record of a live replica: paper_cgan's summary_items() name every layer of its graph, each activation's,
gradient's and weight's device summary equals the float64 oracle on the host copy of that tensor, write_event round-trips
through read_events, train.py --event_files leaves <dir>/train/events.out.tfevents.* at the cadence's steps (and nothing
without the flag), and a model outside the depth family records weights, gradients and losses only."""
import glob
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT

import _summary_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B = 4


class Batches:
    def __init__(self, n, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.x = [torch.rand(B, 65, 65, 3, generator=g).to(DEV) for _ in range(n)]
        self.y = [(torch.rand(B, 65, 65, 1, generator=g) * 0.98 + 0.01).to(DEV) for _ in range(n)]
        self.i = 0

    def next_batch(self):
        k = self.i % len(self.x)
        self.i += 1
        return self.x[k], self.y[k]


def same(s, ref, what):
    """A TensorSummary, or the dict read_events gives for a histogram, against the oracle."""
    bs, bq = R.sum_bounds(ref)
    if isinstance(s, dict):
        assert (s['min'], s['max'], s['num']) == (ref['min'], ref['max'], float(ref['num'])), what
        assert (s['bucket_limit'], s['bucket']) == R.collapse(ref['buckets']), what
        total, squares = s['sum'], s['sum_squares']
    else:
        assert (s.num, s.zeros, s.nonfinite, s.min, s.max) == (ref['num'], ref['zeros'], ref['nonfinite'], ref['min'], ref['max']), what
        assert np.array_equal(s.buckets, ref['buckets']), what
        total, squares = s.sum, s.sum_squares
    assert abs(total - ref['sum']) <= bs and abs(squares - ref['sum_squares']) <= bq, what


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    K, S = pkg('kernels'), pkg('summaries')
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version='baseline', training_version='gan', seed=0, use_graphs=True,
                           g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)
    sess = pkg('runtime').Session(device=DEV, dtype=K.F32, seed=0, rank=0, world_size=1)
    rep = pkg('models.paper.paper_cgan').paper_cgan(Batches(8), args, sess)
    rep.train()
    losses = rep.train()
    items = rep.summary_items()
    host = {}                                               # tag -> the live elements on the host, the oracle's input
    for tag, t, scale in items:
        host[tag] = t.get() if isinstance(t, K.Act) else t.detach().float().cpu().numpy()
    refs = {tag: R.summary(host[tag], scale) for tag, _, scale in items}
    got = K.TensorSummaries(DEV, items).run()
    d = tmp_path_factory.mktemp('event')
    w = S.EventWriter(str(d))
    rep.write_event(w, 17, losses)
    w.close()
    return dict(rep=rep, items=items, refs=refs, got=got, losses=losses, events=S.read_events([w.path]), host=host)


def test_items_name_every_layer_variable_and_gradient(world):
    rep = world['rep']
    tags = [t for t, _, _ in world['items']]
    assert len(tags) == len(set(tags))
    nets = type(rep).build_graph(rep.args)
    assert set(nets) == {'generator/encoder', 'generator/decoder', 'discriminator/rgb_path', 'discriminator/depth_path',
                         'discriminator/combined_path'}
    layers = {('g' if name.startswith('generator') else 'd') + '_activations/%s/%s' % (name, l.name) for name, net in nets.items()
              for l in net.layers}
    assert len(layers) == 8 + 10
    assert {t for t in tags if '_activations/' in t} == layers
    names = set(rep.variables())
    assert {t for t in tags if t.startswith('weights/')} == {'weights/' + n for n in names}
    assert {t for t in tags if t.endswith('/gradient')} == {n + '/gradient' for n in names}
    assert len(tags) == len(layers) + 2 * len(names)
    scales = {s for t, _, s in world['items']}
    assert scales == {1.0}                                   # one rank: 1 / world size


def test_activation_summaries_equal_the_oracle(world):
    acts = [t for t in world['refs'] if '_activations/' in t]
    for tag in acts:
        same(world['got'][tag], world['refs'][tag], tag)
    # e1 is the right channel window of the last zero-copy concat buffer [d3 | e1]; a relu layer has zeros
    e1 = world['got']['g_activations/generator/encoder/e1']
    assert e1.num == B * 31 * 31 * 64 and 0 < e1.zeros < e1.num and e1.min == 0.0 and e1.buckets[776] == e1.zeros
    assert world['got']['d_activations/discriminator/combined_path/h3'].num == 2 * B


def test_gradient_and_weight_summaries_equal_the_oracle(world):
    rep = world['rep']
    grads, variables = rep.gradients(), rep.variables()
    for name in variables:
        assert np.array_equal(world['host'][name + '/gradient'], grads[name]) and np.array_equal(world['host']['weights/' + name], variables[name])
        same(world['got'][name + '/gradient'], world['refs'][name + '/gradient'], name)        # (the oracle on exactly those arrays)
        same(world['got']['weights/' + name], world['refs']['weights/' + name], name)
    assert any(world['got'][n + '/gradient'].max > 0 for n in variables)


def test_write_event_round_trip(world):
    S = pkg('summaries')
    ev, refs, losses = world['events'], world['refs'], world['losses']
    f32 = lambda v: float(np.float32(v))
    assert set(ev['histo']) == set(refs) | {'loss/' + k for k in losses}
    for tag, ref in refs.items():
        (step, _, h), = S.get_tag_values('histo', tag, ev)
        assert step == 17
        same(h, ref, tag)
        got = world['got'][tag]
        assert h['sum'] == got.sum and h['sum_squares'] == got.sum_squares          # the same launch order: bit-equal again
        scalar = lambda t: S.get_tag_values('scalar', t, ev)[0][2]
        if tag.endswith('/gradient'):
            assert scalar(tag) == f32(got.sum / got.num)
        elif tag.startswith('weights/'):
            assert scalar(tag + '/sparsity') == f32(ref['zeros'] / ref['num']) and tag + '/mean' not in ev['scalar']
        else:
            assert scalar(tag + '/sparsity') == f32(ref['zeros'] / ref['num']) and scalar(tag + '/mean') == f32(got.sum / got.num)
    for k, v in losses.items():
        assert S.get_tag_values('scalar', 'loss/' + k, ev) [0][2] == f32(v)
        same(S.get_tag_values('histo', 'loss/' + k, ev)[0][2], R.summary([v]), k)
    metric_tags = {t for t in ev['scalar'] if t.startswith('metrics_')}
    assert metric_tags == {'metrics_%s/%s' % (s, k) for s in ('y_hat', 'y_0') for k in pkg('models.paper.paper_cgan').METRIC_KEYS}
    assert ev['image'] == {}                                  # paper_cgan's montages are not among the recorded (out of scope)
    expected = len(losses) + len(metric_tags) + sum(1 if t.endswith('/gradient') or t.startswith('weights/') else 2 for t in refs)
    assert sum(len(v) for v in ev['scalar'].values()) == expected


def run_train(ws, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_cgan', '--dataset', 'synthetic', '--batch_size', '4',
                        '--dir', ws] + list(extra), env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])


def test_train_cli_event_files_cadence(tmp_path):
    """Two epochs of three iterations: an event before the first step, one after every iteration (3 // 10 = 0: the divisor
    is kept at 1) and one at each epoch's end; paper_cgan's gan train() is two optimizer steps."""
    S = pkg('summaries')
    ws = str(tmp_path / 'ws')
    run_train(ws, '--event_files', '--epoch_size', '3', '--epochs', '2')
    assert 'train' in os.listdir(ws) and sorted(os.listdir(os.path.join(ws, 'summaries'))) == ['losses.csv']
    files = glob.glob(os.path.join(ws, 'train', 'events.out.tfevents.*'))
    assert len(files) == 1 and os.listdir(os.path.join(ws, 'train')) == [os.path.basename(files[0])]
    ev = S.read_events(files)
    tag = 'weights/generator/encoder/vars/e1/weights'
    assert [e[0] for e in ev['histo'][tag]] == [0, 2, 4, 6, 6, 8, 10, 12, 12]
    assert [e[0] for e in S.get_tag_values('histo', tag, ev)] == [0, 2, 4, 6, 8, 10, 12]
    assert [e[0] for e in S.get_tag_values('scalar', 'loss/g_fake', ev)] == [2, 4, 6, 8, 10, 12]          # no losses before the first step
    assert [e[0] for e in S.get_tag_values('scalar', 'g_activations/generator/decoder/d3/sparsity', ev)] == [0, 2, 4, 6, 8, 10, 12]
    e1 = [e[2] for e in S.get_tag_values('scalar', 'g_activations/generator/encoder/e1/sparsity', ev)]
    assert e1[0] == 1.0 and 0.0 < e1[-1] < 1.0                              # zero-filled buffers before the first step, then a relu layer


def test_train_cli_without_the_flag_leaves_no_train_directory(tmp_path):
    ws = str(tmp_path / 'ws')
    run_train(ws, '--epoch_size', '1', '--epochs', '1')
    assert sorted(os.listdir(ws)) == ['checkpoint-0.npz', 'checkpoint-1.npz', 'options.config', 'summaries']


def test_a_model_outside_the_family_records_weights_gradients_and_losses(tmp_path):
    K, S, cnn, data = pkg('kernels'), pkg('summaries'), pkg('models.cnn'), pkg('data')
    args = SimpleNamespace(model='cnn', batch_size=16, latent_size=32, image_shape=(64, 64, 3), n_gpus=1, optimizer='adam',
                           lr=1e-3, decay=0.9, momentum=0.01, centered=False, beta1=0.9, beta2=0.999)
    sess = pkg('runtime').Session(device=DEV, dtype=K.BF16, seed=1, rank=0, world_size=1)
    rep = cnn.CnnReplica(data.SyntheticSource(16, (64, 64, 3), 16, DEV, seed=3), args, sess)
    rep.train_func()
    losses = rep.train_func()
    names = set(rep.variables())
    tags = [t for t, _, _ in rep.summary_items()]
    assert sorted(tags) == sorted(['weights/' + n for n in names] + [n + '/gradient' for n in names])
    w = S.EventWriter(str(tmp_path))
    rep.write_event(w, 3, losses)
    w.close()
    ev = S.read_events([w.path])
    assert set(ev['histo']) == set(tags) | {'loss/' + k for k in losses}
    assert set(ev['scalar']) == {'weights/' + n + '/sparsity' for n in names} | {n + '/gradient' for n in names} | {'loss/' + k for k in losses}
    grads = rep.gradients()
    for n in names:
        same(S.get_tag_values('histo', n + '/gradient', ev)[0][2], R.summary(grads[n]), n)
    assert set(ev['image']) == {'inputs/image/0', 'fake/image/0'}                 # samples(): the epoch montages, as image summaries
    im = ev['image']['fake/image/0'][0][2]
    assert (im['height'], im['width'], im['colorspace']) == (4 * 64, 4 * 64, 3)
    assert np.array_equal(pkg('png').decode(im['encoded_image_string']).shape, (256, 256, 3))
