"""ms per paper_standalone train() at B = 512, bf16, for the four --model_version values, beside paper_cgan --model_version
mean_adjusted IN THE SAME RUN (the yardstick: same box, same minutes), and the per-launch time of cgan_rmse_loss.  Timing as
tools/bench_paper_sampler.py: warm-up calls, then wall time of `--steps` graph-replayed calls between two synchronisations; the
models take turns, `--rounds` times over, and each reports the median and the spread of its rounds.  The split is one eager
train() with the library's per-launch events.  One JSON line per model."""
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
VERSIONS = ['baseline', 'mean_adjusted', 'mean_provided', 'mean_provided2']


def time_calls(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def train_split(m, K):
    """ms of one eager train() by launch: cgan_rmse_loss (per launch of the entry point: its two kernels), the other small
    kernels of the plugin (prep, bar_fill, the head), and everything else (GEMMs, bias gradients, casts, Adam)."""
    m.use_graphs = False
    m.train()
    K.timing_begin()
    m.train()
    torch.cuda.synchronize()
    rec = K.timing_end()
    m.use_graphs = True
    out = {'cgan_rmse_loss': 0.0, 'cgan_other': 0.0, 'rest': 0.0}
    for name, ms, _ in rec:
        out['cgan_rmse_loss' if name == 'cgan_rmse_loss' else 'cgan_other' if name.startswith('cgan_') else 'rest'] += ms
    n_loss = sum(1 for r in rec if r[0] == 'cgan_rmse_loss')
    out['cgan_rmse_loss_per_launch'] = out['cgan_rmse_loss'] / max(1, n_loss)
    out = {k: round(v, 4) for k, v in out.items()}
    out['launches'] = len(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--versions', nargs='*', default=VERSIONS, choices=VERSIONS)
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    data = importlib.import_module('3dgan_amd.data')
    pc = importlib.import_module('3dgan_amd.models.paper.paper_cgan')
    st = importlib.import_module('3dgan_amd.models.standalone.paper_standalone')
    B = a.batch_size

    def session():
        return rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
    models = {}
    sess = session()
    yardstick = 'paper_cgan mean_adjusted'
    models[yardstick] = pc.paper_cgan(data.SyntheticPairSource(2, B, sess.device, 65), SimpleNamespace(
        batch_size=B, model_version='mean_adjusted', training_version='gan', **HP), sess)
    for version in a.versions:
        sess = session()
        models['paper_standalone ' + version] = st.paper_standalone(
            data.SyntheticPairSource(2, B, sess.device, 65), SimpleNamespace(batch_size=B, model_version=version, **HP), sess)
    for m in models.values():                                    # eager, capture, first replays
        for _ in range(a.warmup):
            m.train()
    train_ms = {k: [] for k in models}
    for _ in range(a.rounds):                                    # the models take turns: drift hits all of them alike
        for k, m in models.items():
            train_ms[k].append(time_calls(m.train, a.steps))
    base = statistics.median(train_ms[yardstick])
    for k, m in models.items():
        med = statistics.median(train_ms[k])
        row = {'model': k, 'batch_size': B, 'dtype': 'bf16', 'steps': a.steps, 'rounds': a.rounds, 'ms_per_train': round(med, 3),
               'ms_per_train_min': round(min(train_ms[k]), 3), 'ms_per_train_max': round(max(train_ms[k]), 3),
               'vs_paper_cgan': round(med / base, 4)}
        if k != yardstick:
            row['train_split_ms'] = train_split(m, K)
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
