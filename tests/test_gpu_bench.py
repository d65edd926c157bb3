"""bench.py on the GPU: a plain run prints the headline line and nothing it needs extra runs for, `--dump-outputs` writes
the last timed step's losses and variables (the same ones from run to run), and `--full` adds the instrumented roofline
and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ['--gpus', '1', '--batch_size', '16', '--latent_size', '16']


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + SMALL + list(extra),
                       env=env, timeout=600, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_reports_the_headline_and_dumps_the_last_step(tmp_path):
    runs = []
    for name in ('a', 'b'):
        d = str(tmp_path / name)
        out = _bench('--steps', '3', '--warmup', '1', '--dump-outputs', d)
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in out, k
        assert out['steps'] == 3 and out['unit'] == 'images/sec' and out['higher_is_better'] is True and out['dtype'] == 'bf16'
        assert out['ms_per_step'] > 0 and out['value'] == pytest.approx(16 / (out['ms_per_step'] * 1e-3), rel=1e-9)
        assert not {'roofline', 'cpu_baseline', 'collectives'} & set(out) and 'secondary' not in out['config']
        files = sorted(os.listdir(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64 << 20
        arrays = {f[:-4]: np.load(os.path.join(d, f)) for f in files}
        for k, v in out['config']['final_losses'].items():              # the losses the last timed step returned
            assert arrays[k].dtype == np.float64 and float(arrays[k]) == v, k
        variables = {k: v for k, v in arrays.items() if k not in out['config']['final_losses']}
        assert any(k.startswith('generator.') for k in variables) and any(k.startswith('discriminator.') for k in variables)
        for k, v in variables.items():
            assert v.dtype == np.float32 and np.all(np.isfinite(v)), k
        runs.append(arrays)
    a, b = runs
    assert set(a) == set(b)
    for k in a:                                        # identical inputs and a deterministic step: the same outputs
        assert np.array_equal(a[k], b[k]), k


def test_full_bench_adds_roofline_and_cpu_baseline():
    out = _bench('--steps', '2', '--warmup', '1', '--full', '--no_secondary', '--timer_steps', '1', '--cpu_batch', '8',
                 '--cpu_iters', '1')
    assert out['steps'] == 2 and out['ms_per_step'] > 0
    assert out['roofline']['launches'] > 0 and out['roofline']['achieved'] > 0
    assert out['cpu_baseline']['value'] > 0 and out['cpu_baseline']['unit'] == 'images/sec'
