"""ms per SamplerReplica.sample_full frame on 427 x 561 synthetic frames at B = 512, bf16 (timing as tools/bench_fullimage.py:
warm-up frames, then the wall time of `--steps` frames between two synchronisations):
  1. paper_sampler --noise_layer x with encoder batch norm, draws = 512, stride 10;
  2. paper_sampler --e_bn_off, draws = 512 and 64, strides 10 and 4.
Each line also has the share of the frame taken by the sampling kernels of tdg_cgan_full.hip (the repeating gather, the sample store) and their ms per launch (one
eager frame with the library's per-launch events), beside the yardstick of the statistics kernel measured IN THE SAME RUN: ms
per cgan_sample_stats launch of one eager metrics() at the same batch size.  One JSON line per (configuration, draws, stride)."""
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

HP = dict(g_lr=1e-3, d_lr=1e-3, g_beta1=0.9, d_beta1=0.9, g_beta2=0.999, d_beta2=0.999, seed=0, n_gpus=1)
NEW = ('cgan_full_gather_rep', 'cgan_full_sample_store')


def per_launch(rec, names):
    """{name: (ms in all, launches)} of the named launches in a list of (name, ms, flops) records."""
    out = {}
    for name, ms, _ in rec:
        if name in names:
            t, n = out.get(name, (0.0, 0))
            out[name] = (t + ms, n + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=2, help='Timed frames per line.')
    ap.add_argument('--warmup', type=int, default=1, help='Warm-up frames per line.')
    ap.add_argument('--max_passes', type=int, default=2000, help='Lines with more passes per frame time ONE frame.')
    ap.add_argument('--no_eager', action='store_true', help='Skip the eager frame with per-launch events.')
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    data = importlib.import_module('3dgan_amd.data')
    ps = importlib.import_module('3dgan_amd.models.sampler.paper_sampler')
    pf = importlib.import_module('paper_fullimage')
    B = a.batch_size
    frames = [pf.synthetic_frame('validate', i) for i in range(2)]
    configs = [('paper_sampler x bn', True, [(B, 10)]),
               ('paper_sampler x no_bn', False, [(B, 10), (64, 10), (B, 4), (64, 4)])]
    for label, bn, cases in configs:
        sess = rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
        m = ps.paper_sampler(data.SyntheticPairSource(2, B, sess.device, 65),
                             SimpleNamespace(batch_size=B, noise_layer='x', e_bn='false', e_bn_off=not bn, **HP), sess)
        m.train()
        m.use_graphs = False                                     # the yardstick: cgan_sample_stats launches of one eager metrics()
        m.metrics()
        K.timing_begin()
        m.metrics()
        torch.cuda.synchronize()
        stats = per_launch(K.timing_end(), ('cgan_sample_stats',)).get('cgan_sample_stats', (0.0, 0))
        m.use_graphs = True
        for draws, s in cases:
            if B % draws:
                continue
            r = None
            for k in range(a.warmup):
                r = m.sample_full(*frames[k % 2], stride=s, draws=draws)
            passes = -(-r.patches // (B // draws)) if r is not None else 0
            steps = 1 if passes > a.max_passes else a.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(steps):
                r = m.sample_full(*frames[k % 2], stride=s, draws=draws)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            passes = -(-r.patches // (B // draws))
            line = {'model': label, 'frame': [427, 561], 'stride': s, 'batch_size': B, 'draws': draws, 'dtype': 'bf16',
                    'patches': r.patches, 'passes': passes, 'ms_per_frame': round(dt * 1e3, 3), 'ms_per_pass': round(dt * 1e3 / passes, 4),
                    'rmse': round(r.rmse, 6), 'err_mean': round(r.err_mean, 6), 'err_min': round(r.err_min, 6),
                    'cgan_sample_stats_launches': stats[1], 'cgan_sample_stats_us_per_launch': round(1e3 * stats[0] / max(1, stats[1]), 2)}
            if not a.no_eager and passes <= a.max_passes:
                m.use_graphs = False                             # one eager frame with per-launch events
                K.timing_begin()
                m.sample_full(*frames[0], stride=s, draws=draws)
                torch.cuda.synchronize()
                new = per_launch(K.timing_end(), NEW)
                m.use_graphs = True
                total = sum(t for t, _ in new.values())
                line.update({'new_kernels_ms': round(total, 4), 'new_kernels_share': round(total / (dt * 1e3), 4),
                             'new_kernels_us_per_launch': {k: round(1e3 * t / n, 2) for k, (t, n) in sorted(new.items())}})
            print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
