"""ms per improved_sampler train() and per metrics() at B = 512, bf16, per arch pair, device-synchronised and warmed, and -- with
`--experimental` -- experimental_sampler's train() IN THE SAME RUN, taking turns with E1's: E1 runs the same GEMMs minus the
estimator's forward pass, so it must not be slower than experimental_sampler by more than the spread of the rounds.  Timing as
tools/bench_experimental_sampler.py: warm-up calls (eager, capture, first replays), then wall time of `--steps` graph-replayed
calls between two synchronisations; the calls of a group take turns, `--rounds` times over, and each reports the median and the
spread of its rounds.  One JSON line per row."""
import argparse
import gc
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


def take_turns(calls, a, extra=None):
    """Warm every call, then `rounds` rounds in which the calls take turns; one JSON row per call."""
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    ms = {k: [] for k in calls}
    for _ in range(a.rounds):                                    # drift hits all alike
        for k, fn in calls.items():
            ms[k].append(time_calls(fn, a.steps))
    for k in calls:
        row = {'call': k, 'batch_size': a.batch_size, 'dtype': 'bf16', 'steps': a.steps, 'rounds': a.rounds,
               'ms_per_call': round(statistics.median(ms[k]), 3), 'ms_per_call_min': round(min(ms[k]), 3),
               'ms_per_call_max': round(max(ms[k]), 3), 'ms_rounds': [round(v, 3) for v in ms[k]]}
        row.update((extra or {}).get(k, {}))
        print(json.dumps(row), flush=True)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--optimizer', default='adam')
    ap.add_argument('--archs', nargs='*', default=None, help='generator archs to time (default: every pair)')
    ap.add_argument('--experimental', action='store_true', help="experimental_sampler's train() beside E1's, taking turns")
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    data = importlib.import_module('3dgan_amd.data')
    im = importlib.import_module('3dgan_amd.models.improved.improved_sampler')
    tuples = importlib.import_module('3dgan_amd.data_plugins.synthetic').IMPROVED          # g_arch -> (crop side, tuple entries)
    d_arch = dict(im.PAIRS)
    B = a.batch_size
    hp = dict(batch_size=B, optimizer=a.optimizer, lr=1e-4, beta1=0.9, beta2=0.999, decay=0.9, momentum=0.01, centered=False, seed=0,
              n_gpus=1)

    def session():
        return rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)

    def improved(g):
        sess = session()
        size, entries = tuples[g]
        return im.improved_sampler(data.SyntheticSamplerSource(2, B, sess.device, size, entries), SimpleNamespace(
            g_arch=g, d_arch=d_arch[g], **hp), sess)

    for g in a.archs or list(d_arch):
        m = improved(g)
        name = 'improved_sampler %s/%s' % (g, d_arch[g])
        calls = {name + ' train': m.train, name + ' metrics': m.metrics}
        extra = {name + ' train': {'optimizer': a.optimizer, 'parameters': {p.name: p.store.num_params() for p in m.parts}}}
        if g == 'E1' and a.experimental:
            xs = importlib.import_module('3dgan_amd.models.experimental.experimental_sampler')
            sess = session()
            x = xs.experimental_sampler(data.SyntheticEstimatorSource(2, B, sess.device, 64), SimpleNamespace(**hp), sess)
            calls = {'experimental_sampler train': x.train, name + ' train': m.train, name + ' metrics': m.metrics}
        ms = take_turns(calls, a, extra)
        if g == 'E1' and a.experimental:
            e1, ex = ms[name + ' train'], ms['experimental_sampler train']
            print(json.dumps({'call': 'E1 train against experimental_sampler train', 'median_ms': [round(statistics.median(e1), 3),
                                                                                                  round(statistics.median(ex), 3)],
                              'spread_ms': {'E1': round(max(e1) - min(e1), 3), 'experimental_sampler': round(max(ex) - min(ex), 3)},
                              'e1_minus_experimental_ms': round(statistics.median(e1) - statistics.median(ex), 3)}), flush=True)
            del x
        del m, calls
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
