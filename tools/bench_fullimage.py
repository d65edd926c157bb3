"""ms per paper_cgan.infer_full frame on 427 x 561 synthetic frames at B = 512, bf16, for strides 10, 4 and 1 (timing as
tools/bench_paper_cgan.py: warm-up frames, then the wall time of `--steps` frames between two synchronisations), with
patches/s, the whole-call generator rate (padded patch count x generator FLOP per patch over the frame time) and the share
of the frame taken by the tdg_cgan_full.hip kernels (one eager frame with the library's per-launch events).  One JSON line
per stride."""
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


def generator_flops_per_patch(version):
    """2 x multiply-adds of paper_cgan.generator on one 65x65 window: the four 5x5 stride-2 encoder convs, the three 5x5
    stride-2 decoder deconvs (one MAC per input pixel, filter tap and channel pair) and the 1x1 head on the 29x29 crop."""
    cin = 4 if version == 'mean_provided2' else 3
    enc = [(31, cin, 64), (14, 64, 128), (5, 128, 256), (1, 256, 512)]           # (output side, cin, cout)
    dec = [(1, 512, 256), (5, 512, 128), (14, 256, 64)]                          # (input side, cin, cout)
    macs = sum(h * h * ci * co * 25 for h, ci, co in enc) + sum(h * h * ci * co * 25 for h, ci, co in dec) + 29 * 29 * 128
    return 2 * macs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch_size', type=int, default=512)
    ap.add_argument('--steps', type=int, default=5, help='Timed frames per stride.')
    ap.add_argument('--warmup', type=int, default=2, help='Warm-up frames per stride.')
    ap.add_argument('--strides', type=int, nargs='+', default=[10, 4, 1])
    ap.add_argument('--model_version', default='baseline')
    ap.add_argument('--no_eager', action='store_true', help='Skip the eager frame with per-launch events.')
    a = ap.parse_args()
    K = importlib.import_module('3dgan_amd.kernels')
    rt = importlib.import_module('3dgan_amd.runtime')
    pc = importlib.import_module('3dgan_amd.models.paper.paper_cgan')
    pf = importlib.import_module('paper_fullimage')
    B = a.batch_size
    sess = rt.Session(dtype=K.BF16, seed=0, rank=0, world_size=1)
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version=a.model_version, training_version='gan', seed=0)
    m = pc.paper_cgan(None, args, sess)
    frames = [pf.synthetic_frame('validate', i) for i in range(2)]
    fpp = generator_flops_per_patch(a.model_version)
    for s in a.strides:
        for k in range(a.warmup):
            m.infer_full(*frames[k % 2], stride=s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.steps):
            r = m.infer_full(*frames[k % 2], stride=s)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        padded = -(-r.patches // B) * B
        line = {'model': 'paper_cgan', 'model_version': a.model_version, 'frame': [427, 561], 'stride': s, 'batch_size': B,
                'dtype': 'bf16', 'patches': r.patches, 'chunks': padded // B, 'ms_per_frame': round(dt * 1e3, 3),
                'patches_per_s': round(r.patches / dt, 1), 'gen_mflop_per_patch': round(fpp / 1e6, 2),
                'gen_tflops': round(padded * fpp / dt / 1e12, 2), 'rmse': round(r.rmse, 6)}
        if not a.no_eager:
            m.use_graphs = False                     # one eager frame with per-launch events
            K.timing_begin()
            m.infer_full(*frames[0], stride=s)
            torch.cuda.synchronize()
            rec = K.timing_end()
            m.use_graphs = True
            full_ms = {}
            for name, ms, _ in rec:
                if name.startswith('cgan_full_'):
                    full_ms[name] = full_ms.get(name, 0.0) + ms
            line.update({'new_kernels_ms': round(sum(full_ms.values()), 4),
                         'new_kernels_share': round(sum(full_ms.values()) / (dt * 1e3), 4),
                         'new_kernels': {k: round(v, 4) for k, v in sorted(full_ms.items())}})
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
