"""ms per paper_sampler train() at B = 512, bf16, for the noise nodes x, e2, e4-512 and d4 with and without encoder batch norm,
beside paper_cgan --model_version mean_adjusted IN THE SAME RUN (the yardstick: same box, same minutes), and ms per metrics()
with its split.  Timing as tools/bench_paper_cgan.py: warm-up calls, then wall time of `--steps` graph-replayed calls between
two synchronisations; the models take turns, `--rounds` times over, and each reports the median and the spread of its rounds.
The split of metrics() is one eager call with the library's per-launch events.  One JSON line per model."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HP = dict(g_lr=1e-3, d_lr=1e-3, g_beta1=0.9, d_beta1=0.9, g_beta2=0.999, d_beta2=0.999, seed=0, n_gpus=1)


def time_calls(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def metrics_split(m, K):
    """ms of one eager metrics() by launch: the sampler pass (everything but the two kinds below), cgan_sample_stats, and the
    Eigen launches (cgan_metrics, cgan_eval_batch)."""
    m.use_graphs = False
    m.metrics()
    K.timing_begin()
    m.metrics()
    torch.cuda.synchronize()
    rec = K.timing_end()
    m.use_graphs = True
    out = {'sampler_pass': 0.0, 'cgan_sample_stats': 0.0, 'eigen': 0.0}
    for name, ms, _ in rec:
        key = 'cgan_sample_stats' if name == 'cgan_sample_stats' else 'eigen' if name in ('cgan_metrics', 'cgan_eval_batch') else 'sampler_pass'
        out[key] += ms
    out['launches'] = len(rec)
    out['cgan_sample_stats_per_launch'] = out['cgan_sample_stats'] / max(1, sum(1 for r in rec if r[0] == 'cgan_sample_stats'))
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--nodes', nargs='*', default=['x', 'e2', 'e4-512', 'd4'])
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    data = importlib.import_module('3dgan_amd.data')
    pc = importlib.import_module('3dgan_amd.models.paper.paper_cgan')
    ps = importlib.import_module('3dgan_amd.models.sampler.paper_sampler')
    B = a.batch_size

    def session():
        return rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
    models = {}
    sess = session()
    models['paper_cgan mean_adjusted'] = pc.paper_cgan(data.SyntheticPairSource(2, B, sess.device, 65), SimpleNamespace(
        batch_size=B, model_version='mean_adjusted', training_version='gan', **HP), sess)
    for node in a.nodes:
        for bn in (True, False):
            sess = session()
            models['paper_sampler %s %s' % (node, 'bn' if bn else 'no_bn')] = ps.paper_sampler(
                data.SyntheticPairSource(2, B, sess.device, 65),
                SimpleNamespace(batch_size=B, noise_layer=node, e_bn='false', e_bn_off=not bn, **HP), sess)
    for m in models.values():                                    # eager, capture, first replays
        for _ in range(a.warmup):
            m.train()
            if hasattr(m, 'sample'):
                m.metrics()
    train_ms, metrics_ms = {k: [] for k in models}, {k: [] for k in models}
    for _ in range(a.rounds):                                    # the models take turns: drift hits all of them alike
        for k, m in models.items():
            train_ms[k].append(time_calls(m.train, a.steps))
        for k, m in models.items():
            if hasattr(m, 'sample'):
                metrics_ms[k].append(time_calls(m.metrics, a.steps))
    for k, m in models.items():
        row = {'model': k, 'batch_size': B, 'dtype': 'bf16', 'steps': a.steps, 'rounds': a.rounds,
               'ms_per_train': round(statistics.median(train_ms[k]), 3), 'ms_per_train_min': round(min(train_ms[k]), 3),
               'ms_per_train_max': round(max(train_ms[k]), 3)}
        if metrics_ms[k]:
            row.update(ms_per_metrics=round(statistics.median(metrics_ms[k]), 3), ms_per_metrics_min=round(min(metrics_ms[k]), 3),
                       ms_per_metrics_max=round(max(metrics_ms[k]), 3), metrics_split_ms=metrics_split(m, K))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
