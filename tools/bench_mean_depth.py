"""ms per mean_depth_estimator train() at B = 512, bf16, beside paper_standalone --model_version baseline IN THE SAME RUN (a
yardstick for drift: same box, same minutes), and the time of mde_loss per launch of the entry point.  Timing as
tools/bench_paper_standalone.py: warm-up calls (eager, capture, first replays), then wall time of `--steps` graph-replayed calls
between two synchronisations; the models take turns, `--rounds` times over, and each reports the median and the spread of its
rounds.  The split is one eager train() with the library's per-launch events, by kernel name.  One JSON line per model."""
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


def time_calls(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def train_split(m, K):
    """One eager train() by launch: {kernel: [launches, ms]}, the time of mde_loss per launch of the entry point (its two
    kernels), the total, and every timed launch in order (l1 .. l7 forward, the loss, then the backward pass from l7 down)."""
    m.use_graphs = False
    m.train()
    K.timing_begin()
    m.train()
    torch.cuda.synchronize()
    rec = K.timing_end()
    m.use_graphs = True
    by = {}
    for name, ms, _ in rec:
        e = by.setdefault(name, [0, 0.0])
        e[0] += 1
        e[1] += ms
    loss = by.get('mde_loss', [0, 0.0])
    return {'launches': len(rec), 'timed_ms': round(sum(v[1] for v in by.values()), 4),
            'mde_loss_us_per_launch': round(1e3 * loss[1] / max(1, loss[0]), 2),
            'kernels': {k: [v[0], round(v[1], 4)] for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])},
            'sequence': [[name, round(ms, 4), round(fl / 1e9, 1)] for name, ms, fl in rec]}       # in launch order: kernel, ms, GFLOP


def model_flops(m):
    """Algorithmic FLOPs of one train() (2 x MACs, padding taps counted): three GEMM forms per conv, no input gradient for l1."""
    total = 0.0
    for L in m.M.layers:
        if L.rowdot:
            continue
        total += L.conv.flops(m.B) * (2 if L.idx == 0 else 3)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--optimizer', default='adam')
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    data = importlib.import_module('3dgan_amd.data')
    st = importlib.import_module('3dgan_amd.models.standalone.paper_standalone')
    mde = importlib.import_module('3dgan_amd.models.estimator.mean_depth_estimator')
    B = a.batch_size

    def session():
        return rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
    sess = session()
    yardstick = 'paper_standalone baseline'
    models = {yardstick: st.paper_standalone(data.SyntheticPairSource(2, B, sess.device, 65), SimpleNamespace(
        batch_size=B, model_version='baseline', g_lr=1e-3, g_beta1=0.9, g_beta2=0.999, seed=0, n_gpus=1), sess)}
    sess = session()
    models['mean_depth_estimator E2'] = mde.mean_depth_estimator(data.SyntheticEstimatorSource(2, B, sess.device), SimpleNamespace(
        batch_size=B, m_arch='E2', optimizer=a.optimizer, lr=1e-4, beta1=0.9, beta2=0.999, decay=0.9, momentum=0.01, centered=False,
        seed=0, n_gpus=1), sess)
    for m in models.values():
        for _ in range(a.warmup):
            m.train()
    train_ms = {k: [] for k in models}
    for _ in range(a.rounds):                                    # the models take turns: drift hits both alike
        for k, m in models.items():
            train_ms[k].append(time_calls(m.train, a.steps))
    for k, m in models.items():
        med = statistics.median(train_ms[k])
        row = {'model': k, 'batch_size': B, 'dtype': 'bf16', 'steps': a.steps, 'rounds': a.rounds, 'ms_per_train': round(med, 3),
               'ms_per_train_min': round(min(train_ms[k]), 3), 'ms_per_train_max': round(max(train_ms[k]), 3)}
        if k != yardstick:
            fl = model_flops(m)
            row.update(optimizer=a.optimizer, parameters=m.store.num_params(), gflop_per_train=round(fl / 1e9, 1),
                       tflops_whole_call=round(fl / (med * 1e-3) / 1e12, 1), train_split=train_split(m, K))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
