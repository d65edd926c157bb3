"""ms per paper_cgan train() and images/s at B = 512, bf16, for the gan and wgan schedules (bench.py's timing method: warm-up
calls, then wall time of `--steps` graph-replayed calls between two synchronisations), and the share of the step taken by the
tdg_cgan.hip kernels (one eager call with the library's per-launch events).  One JSON line per schedule."""
import argparse
import importlib
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def time_calls(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--model_version', default='baseline')
    ap.add_argument('--schedules', nargs='*', default=['gan', 'wgan'])
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    data = importlib.import_module('3dgan_amd.data')
    pc = importlib.import_module('3dgan_amd.models.paper.paper_cgan')
    B = a.batch_size
    for training in a.schedules:
        sess = rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
        args = SimpleNamespace(batch_size=B, n_gpus=1, model_version=a.model_version, training_version=training, g_lr=1e-3,
                               d_lr=1e-3, g_beta1=0.9, d_beta1=0.9, g_beta2=0.999, d_beta2=0.999, seed=0)
        m = pc.paper_cgan(data.SyntheticPairSource(2, B, sess.device, 65), args, sess)
        dt, losses = time_calls(m.train, a.warmup, a.steps)
        m.use_graphs = False                         # one eager call with per-launch events
        m.train()
        K.timing_begin()
        m.train()
        torch.cuda.synchronize()
        rec = K.timing_end()
        m.use_graphs = True
        cgan_ms = {}
        for name, ms, _ in rec:
            if name.startswith('cgan_'):
                cgan_ms[name] = cgan_ms.get(name, 0.0) + ms
        batches = 6 if training == 'wgan' else 2
        print(json.dumps({'model': 'paper_cgan', 'model_version': a.model_version, 'training_version': training, 'batch_size': B,
                          'dtype': 'bf16', 'ms_per_train': round(dt * 1e3, 3), 'images_per_s': round(batches * B / dt, 1),
                          'batches_per_train': batches, 'new_kernels_ms': round(sum(cgan_ms.values()), 4),
                          'new_kernels_share': round(sum(cgan_ms.values()) / (dt * 1e3), 4),
                          'new_kernels': {k: round(v, 4) for k, v in sorted(cgan_ms.items())},
                          'losses': {k: round(v, 5) for k, v in losses.items()}}), flush=True)


if __name__ == '__main__':
    main()
