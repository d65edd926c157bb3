"""ms per batch of paper_cgan.evaluate()'s two sweeps at B = 512, bf16, on synthetic 65x65 pairs (timing as
tools/bench_fullimage.py: warm-up sweeps, then the wall time of `--steps` sweeps of `--n_batches` batches between two
synchronisations, each sweep ending in its finish launch and the host read of its results), the share of a sweep-1 batch taken
by the tdg_cgan_eval.hip kernels (one eager sweep with the library's per-launch events), and for comparison the same sweep
done without them: infer() per batch, tdg_cgan_metrics for y_hat and y_0, one host read per batch.  One JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--n_batches', type=int, default=16, help='Batches per sweep.')
    ap.add_argument('--steps', type=int, default=10, help='Timed sweeps of each kind.')
    ap.add_argument('--warmup', type=int, default=2, help='Warm-up sweeps of each kind.')
    ap.add_argument('--model_version', default='mean_adjusted')
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    _lib = importlib.import_module('3dgan_amd._lib')
    rt = importlib.import_module('3dgan_amd.runtime')
    pc = importlib.import_module('3dgan_amd.models.paper.paper_cgan')
    data = importlib.import_module('3dgan_amd.data')
    B, n = a.batch_size, a.n_batches
    sess = rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version=a.model_version, training_version='gan', seed=0)
    m = pc.paper_cgan(None, args, sess)
    src = data.SyntheticPairSource(4, B, sess.device, 65, 1234)

    def sweep1():
        m.eval_acc.zero_()
        m.eval_counts.zero_()
        m._eval_sweep(src, n, 'eval_model', m._eval_model_body)
        m._eval_finish(True)
        return m.eval_scalars.cpu()

    def sweep2():
        m.eval_acc.zero_()
        m.eval_counts.zero_()
        m._eval_sweep(src, n, 'eval_mean', m._eval_mean_body, both=False)
        m._eval_finish(False)
        return m.eval_scalars.cpu()

    counts = torch.zeros(2, 4, dtype=torch.int64, device=sess.device)
    out = torch.zeros(2, 8, device=sess.device)

    def per_batch_reads():
        """infer() + tdg_cgan_metrics for y_hat and y_0 + one host read, per batch."""
        counts.zero_()
        rows = []
        off = m.inf_ybar if m.version != 0 else None
        for _ in range(n):
            m.infer(src.next_batch())
            for k, (pred, o) in enumerate(((m.inf_yhat, None), (None, off))):
                _lib.call('tdg_cgan_metrics', K.ptr(m.inf_crop), K.ptr(pred), K.ptr(o), B, pc.CROP * pc.CROP, K.ptr(counts[k]),
                          K.ptr(out[k]), K.ptr(m.metric_ws), m.metric_ws.numel(), K.stream())
            rows.append(out.cpu())
        return rows

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (a.steps * n) * 1e3

    # alternate the kinds, so that a drift of the box falls on all of them
    ms = {'sweep1': [], 'sweep2': [], 'per_batch_reads': []}
    for _ in range(3):
        ms['sweep1'].append(timed(sweep1))
        ms['sweep2'].append(timed(sweep2))
        ms['per_batch_reads'].append(timed(per_batch_reads))
    best = {k: min(v) for k, v in ms.items()}
    line = {'model': 'paper_cgan', 'model_version': a.model_version, 'batch_size': B, 'dtype': 'bf16', 'n_batches': n,
            'sweep1_ms_per_batch': round(best['sweep1'], 4), 'sweep2_ms_per_batch': round(best['sweep2'], 4),
            'per_batch_reads_ms_per_batch': round(best['per_batch_reads'], 4),
            'runs_ms_per_batch': {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    m.use_graphs = False                         # one eager sweep of each kind with per-launch events
    for name, fn in (('sweep1', sweep1), ('sweep2', sweep2)):
        K.timing_begin()
        fn()
        torch.cuda.synchronize()
        rec = K.timing_end()
        new_ms, all_ms = {}, 0.0
        for kernel, t, _ in rec:
            all_ms += t
            if kernel.startswith('cgan_eval_'):
                new_ms[kernel] = new_ms.get(kernel, 0.0) + t
        per_batch = sum(new_ms.values()) / n
        line[name + '_new_kernels_ms_per_batch'] = round(per_batch, 5)
        line[name + '_new_kernels_share'] = round(per_batch / best[name], 4)
        line[name + '_timed_launches_ms_per_batch'] = round(all_ms / n, 5)
        line[name + '_new_kernels'] = {k: round(v / n, 5) for k, v in sorted(new_ms.items())}
    m.use_graphs = True
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
