"""Held-out passes of paper_cgan: validation_losses and observe change no variable, no optimizer slot and no step counter,
report the losses of the G step's own forward pass and leave the gradients of a D and a G step behind; training with the
passes in between ends where plain training ends; an observed event carries the activation montages and metrics_y_mean; and
train.py --validation writes the validate / test event files, the CSV rows and the mean / variance images (and nothing new
without the flags).  Identically seeded replicas running the step bodies themselves are the oracle: every comparison is
exact."""
import glob
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg, ROOT

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


def make(training_version='gan', model_version='baseline'):
    K = pkg('kernels')
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version=model_version, training_version=training_version, seed=0, use_graphs=True,
                           g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)
    sess = pkg('runtime').Session(device=DEV, dtype=K.F32, seed=0, rank=0, world_size=1)
    return pkg('models.paper.paper_cgan').paper_cgan(Batches(8), args, sess)


def state(rep):
    """Variables, optimizer slots and step counts, packed filters, the global step."""
    d = {'var/' + k: v for k, v in rep.variables().items()}
    for name, opt in rep.optimizers().items():
        d.update({'%s/%s' % (name, k): t.detach().cpu().numpy().copy() for k, t in opt.state_tensors().items()})
        d[name + '/t'] = np.asarray(opt.t)
    convs = [L.conv for net in (rep.Dr, rep.Dd, rep.Dc) for L in net.layers]
    for i, conv in enumerate(convs):
        d['packed/%d/fwd' % i] = conv.w_fwd.detach().cpu().view(torch.uint8).numpy().copy()
        d['packed/%d/bwd' % i] = conv.w_bwd.detach().cpu().view(torch.uint8).numpy().copy()
    d['global_step'] = np.asarray(rep.sess.global_step)
    return d


def same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope='module')
def world():
    held = Batches(3, seed=9)                                   # held-out batches: another seed than the training source's
    return SimpleNamespace(A=make(), held=held, b=held.next_batch())


def test_the_passes_change_nothing_and_report_the_step_bodies_values(world):
    A, b = world.A, world.b
    Bm, Cm = make(), make()
    before = state(A)
    assert any(k.startswith('packed/') for k in before) and any(k.endswith('/m') for k in before)
    lv = A.validation_losses(b)
    same_state(state(A), before)
    lo = A.observe(b)
    same_state(state(A), before)
    assert lv == lo and set(lv) == {'g_fake', 'd_fake', 'd_real', 'd_total'}
    Bm.g_step(b)
    assert Bm._losses() == lv
    Cm.d_step(b)
    ga, gb, gc = A.gradients(), Bm.gradients(), Cm.gradients()
    d_names = [n for n in ga if n.startswith('discriminator/')]
    g_names = [n for n in ga if n.startswith('generator/')]
    assert d_names and g_names and len(d_names) + len(g_names) == len(ga)
    for n in d_names:
        assert np.array_equal(ga[n], gc[n]) and np.any(ga[n] != 0), n
    for n in g_names:
        assert np.array_equal(ga[n], gb[n]) and np.any(ga[n] != 0), n
    # a replayed (captured) validation body reports what the eager one did
    assert A.validation_losses(b) == lv and A.validation_losses(b) == lv
    same_state(state(A), before)


@pytest.mark.parametrize('training_version, model_version', [('wgan', 'baseline'), ('gan', 'mean_adjusted'), ('gan', 'mean_provided2'),
                                                            ('wgan', 'mean_provided2')])
def test_the_other_versions_have_the_passes_too(world, training_version, model_version):
    A, Bm = make(training_version, model_version), make(training_version, model_version)
    before = state(A)
    lv = A.validation_losses(world.b)
    lo = A.observe(world.b)
    same_state(state(A), before)
    Bm.g_step(world.b)
    assert lv == lo == Bm._losses() and all(np.isfinite(v) for v in lv.values())
    assert set(lv) == ({'g_fake', 'd_fake', 'd_fake_1', 'd_total'} if training_version == 'wgan' else {'g_fake', 'd_fake', 'd_real', 'd_total'})
    ga, gb = A.gradients(), Bm.gradients()
    assert all(np.array_equal(ga[n], gb[n]) for n in ga if n.startswith('generator/'))


def test_training_is_undisturbed(world, tmp_path):
    S = pkg('summaries')
    A, P = world.A, make()
    w = S.EventWriter(str(tmp_path))
    A.train()
    A.validation_losses(world.held.next_batch())
    A.train()
    losses = A.observe(world.held.next_batch())
    A.write_event(w, A.sess.global_step, losses, montages=True)
    A.train()
    w.close()
    for _ in range(3):
        P.train()
    same_state(state(A), state(P))
    assert A.sess.global_step == 6


def test_an_observed_event_carries_the_montages_and_the_mean_metrics(world, tmp_path):
    S, png, cgan = pkg('summaries'), pkg('png'), pkg('models.paper.paper_cgan')
    A = world.A
    A.set_mean_image(np.linspace(0.1, 0.9, 29 * 29, dtype=np.float32).reshape(29, 29))
    losses = A.observe(world.b)
    w = S.EventWriter(str(tmp_path / 'with'))
    A.write_event(w, 5, losses, montages=True)
    w.close()
    ev = S.read_events([w.path])
    acts = [t for t, _, _ in A.summary_items() if '_activations/' in t]
    assert len(acts) == 18 and set(ev['image']) == {t + '/montage/image/0' for t in acts}
    kernel = A._montages.run()                                  # the buffers have not changed since the event
    for t in acts:
        (step, _, im), = ev['image'][t + '/montage/image/0']
        img, _, _ = kernel[t + '/montage']
        assert step == 5 and (im['height'], im['width'], im['colorspace']) == (img.shape[0], img.shape[1], 1), t
        assert np.array_equal(np.squeeze(png.decode(im['encoded_image_string'])), np.squeeze(img)), t
    e1 = ev['image']['g_activations/generator/encoder/e1/montage/image/0'][0][2]
    assert (e1['height'], e1['width'], e1['colorspace']) == (248, 248, 1)
    assert np.squeeze(png.decode(e1['encoded_image_string'])).shape == (248, 248)
    for s in ('y_hat', 'y_0', 'y_mean'):
        assert {'metrics_%s/%s' % (s, k) for k in cgan.METRIC_KEYS} <= set(ev['scalar'])
    assert all(S.get_tag_values('scalar', 'loss/' + k, ev)[0][2] == float(np.float32(v)) for k, v in losses.items())
    w = S.EventWriter(str(tmp_path / 'without'))
    A.write_event(w, 6, losses)
    w.close()
    assert S.read_events([w.path])['image'] == {}
    A.set_mean_image(None)


def run_train(ws, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--model', 'paper_cgan', '--dataset', 'synthetic', '--batch_size', '4',
                        '--epoch_size', '3', '--epochs', '2', '--event_files', '--test_epochs', '2', '--dir', ws] + list(extra),
                       env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    return p


def test_train_cli_validation_and_test_passes(tmp_path):
    S, cgan = pkg('summaries'), pkg('models.paper.paper_cgan')
    ws = str(tmp_path / 'ws')
    p = run_train(ws, '--validation', '--event_montages')
    assert 'Validation' in p.stderr and 'Test' in p.stderr     # the tqdm bars
    ev = {}
    for split in ('train', 'validate', 'test'):
        files = glob.glob(os.path.join(ws, split, 'events.out.tfevents.*'))
        assert len(files) == 1 and os.listdir(os.path.join(ws, split)) == [os.path.basename(files[0])], split
        ev[split] = S.read_events(files)
    montage = 'g_activations/generator/encoder/e1/montage/image/0'
    for split, steps in (('validate', [6, 12]), ('test', [12])):
        e = ev[split]
        assert [x[0] for x in e['scalar']['loss/g_fake']] == steps and [x[0] for x in e['image'][montage]] == steps, split
        assert {'loss/g_fake', 'loss/d_fake', 'loss/d_real', 'loss/d_total'} <= set(e['scalar']), split
        for s in ('y_hat', 'y_0', 'y_mean'):
            assert {'metrics_%s/%s' % (s, k) for k in cgan.METRIC_KEYS} <= set(e['scalar']), (split, s)
        assert len(e['image']) == 18 and all(t.endswith('/montage/image/0') for t in e['image']), split
    assert 'metrics_y_mean/linear_rmse' in ev['train']['scalar'] and montage in ev['train']['image']
    rows = open(os.path.join(ws, 'summaries', 'validation.csv')).read().splitlines()
    assert rows[0] == 'epoch,step,d_fake,d_real,d_total,g_fake' and [r.split(',')[:2] for r in rows[1:]] == [['1', '6'], ['2', '12']]
    assert all(np.isfinite(float(v)) for r in rows[1:] for v in r.split(','))
    rows = open(os.path.join(ws, 'summaries', 'test.csv')).read().splitlines()
    assert [r.split(',')[:2] for r in rows[1:]] == [['2', '12']]
    assert sorted(os.listdir(ws)) == sorted(['checkpoint-0.npz', 'checkpoint-1.npz', 'checkpoint-2.npz', 'options.config', 'summaries', 'train',
                                             'validate', 'test', 'mean_training_img.png', 'var_training_img.png',
                                             'mean_validation_img.png', 'var_validation_img.png'])
    shape = np.squeeze(pkg('png').decode(open(os.path.join(ws, 'mean_validation_img.png'), 'rb').read())).shape
    assert shape == (29, 29)


def test_train_cli_without_the_new_flags_leaves_todays_directory(tmp_path):
    S = pkg('summaries')
    ws = str(tmp_path / 'ws')
    run_train(ws)
    assert sorted(os.listdir(ws)) == ['checkpoint-0.npz', 'checkpoint-1.npz', 'checkpoint-2.npz', 'options.config', 'summaries', 'train']
    assert all(f == 'losses.csv' or f.startswith('montage-') for f in os.listdir(os.path.join(ws, 'summaries')))
    ev = S.read_events(glob.glob(os.path.join(ws, 'train', 'events.out.tfevents.*')))
    assert ev['image'] == {} and not any(t.startswith('metrics_y_mean') for t in ev['scalar'])
