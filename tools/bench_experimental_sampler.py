"""ms per experimental_sampler train() and per metrics() at B = 512, bf16, beside paper_standalone --model_version baseline IN THE
SAME RUN (a yardstick for drift: same box, same minutes), and the time of the three kernels of csrc/tdg_xsamp.hip and of the
e1 (7-channel) and hx1 (6-channel) convs per launch.  Timing as tools/bench_mean_depth.py: warm-up calls (eager, capture, first
replays), then wall time of `--steps` graph-replayed calls between two synchronisations; the calls take turns, `--rounds` times
over, and each reports the median and the spread of its rounds.  The split is one eager train() with the library's per-launch
events, by kernel name, in launch order.  One JSON line per row."""
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

NEW = ('xsamp_prep', 'xsamp_head_fwd', 'xsamp_head_bwd')


def time_calls(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def train_split(m, K):
    """One eager train() by launch.  The step's launch order is fixed (models/experimental/experimental_sampler.py: _grads), so
    three conv launches are named by position: e1's forward is the first GEMM behind xsamp_prep, hx1's the first behind
    xsamp_head_fwd, e1's filter gradient the last GEMM of the body; every other launch is in `sequence`, in order."""
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
    names = [r[0] for r in rec]
    after = lambda marker: next(([n, round(1e3 * ms, 2)] for n, ms, fl in rec[names.index(marker) + 1:] if fl > 0), None)
    return {'launches': len(rec), 'timed_ms': round(sum(v[1] for v in by.values()), 4),
            'new_kernels_us_per_launch': {k: round(1e3 * by[k][1] / by[k][0], 2) for k in NEW if k in by},
            'e1_forward': after('xsamp_prep'), 'hx1_forward': after('xsamp_head_fwd'),
            'e1_filter_gradient': next(([n, round(1e3 * ms, 2)] for n, ms, fl in reversed(rec) if fl > 0), None),
            'kernels': {k: [v[0], round(v[1], 4)] for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])},
            'sequence': [[name, round(ms, 4), round(fl / 1e9, 1)] for name, ms, fl in rec]}       # in launch order: kernel, ms, GFLOP


def model_flops(m):
    """Algorithmic FLOPs of one train() (2 x MACs, padding taps counted): the estimator's forward pass; three GEMM forms per
    generator conv (no input gradient for e1); the critic's rgb path over B (no input gradient for hx1), its depth and combined
    paths over 2B with one more input-gradient pass over the fake half."""
    B = m.B
    est = sum(L.conv.flops(B) for L in m.estimator.M.layers if not L.rowdot)
    g = sum(c.flops(B) * (2 if k == 1 else 3) for k, c in m.G.e_conv.items()) + sum(c.flops(B) * 3 for c in m.G.d_conv.values())
    rgb = sum(L.conv.flops(B) * (2 if L.idx == 0 else 3) for L in m.Dr.layers)
    depth = sum(L.conv.flops(2 * B) * (2 if L.idx == 0 else 3) + L.conv.flops(B) for L in m.Dd.layers)
    comb = sum(L.conv.flops(2 * B) * 3 + L.conv.flops(B) for L in m.Dc.layers)
    return {'estimator_forward': est, 'generator': g, 'rgb_path': rgb, 'depth_path': depth, 'combined_path': comb}


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
    xs = importlib.import_module('3dgan_amd.models.experimental.experimental_sampler')
    B = a.batch_size

    def session():
        return rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
    sess = session()
    yardstick = 'paper_standalone baseline'
    base = st.paper_standalone(data.SyntheticPairSource(2, B, sess.device, 65), SimpleNamespace(
        batch_size=B, model_version='baseline', g_lr=1e-3, g_beta1=0.9, g_beta2=0.999, seed=0, n_gpus=1), sess)
    sess = session()
    m = xs.experimental_sampler(data.SyntheticEstimatorSource(2, B, sess.device, 64), SimpleNamespace(
        batch_size=B, optimizer=a.optimizer, lr=1e-4, beta1=0.9, beta2=0.999, decay=0.9, momentum=0.01, centered=False, seed=0, n_gpus=1),
        sess)
    calls = {yardstick: base.train, 'experimental_sampler train': m.train, 'experimental_sampler metrics': m.metrics}
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):                                    # the calls take turns: drift hits all alike
        for k, fn in calls.items():
            ms[k].append(time_calls(fn, a.steps))
    fl = model_flops(m)
    for k in calls:
        med = statistics.median(ms[k])
        row = {'call': k, 'batch_size': B, 'dtype': 'bf16', 'steps': a.steps, 'rounds': a.rounds, 'ms_per_call': round(med, 3),
               'ms_per_call_min': round(min(ms[k]), 3), 'ms_per_call_max': round(max(ms[k]), 3)}
        if k == 'experimental_sampler train':
            total = sum(fl.values())
            row.update(optimizer=a.optimizer, parameters={p.name: p.store.num_params() for p in m.parts},
                       gflop_per_train={n: round(v / 1e9, 1) for n, v in fl.items()}, gflop_per_train_total=round(total / 1e9, 1),
                       tflops_whole_call=round(total / (med * 1e-3) / 1e12, 1), train_split=train_split(m, K))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
