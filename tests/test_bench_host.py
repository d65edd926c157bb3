"""bench.py's command line and its --dump-outputs writer, without a GPU."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location('bench_under_test', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default_and_full_is_opt_in():
    ap = _bench().make_parser()
    a = ap.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    a = ap.parse_args(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'


def test_dump_outputs_fits_the_budget_and_samples_the_same_positions(tmp_path):
    """Small variables are written whole; one over its share of the budget becomes a fixed sample of its elements, the same
    positions in every run; losses are float64, variables float32, every file name is the variable's with '/' -> '.'."""
    b = _bench()
    variables = {'generator/vars/fc1/weights': np.arange(60000, dtype=np.float32).reshape(300, 200),     # value = position
                 'generator/vars/fc1/bias': np.linspace(-1, 1, 200, dtype=np.float32),
                 'discriminator/vars/c3/weights': -np.arange(80000, dtype=np.float32).reshape(5, 5, 40, 80)}
    losses = {'g_loss': 1.25, 'd_loss': -0.5}
    budget = 3 * 16384 * 4 + 16
    outs = []
    for run in ('a', 'b'):
        d = str(tmp_path / run)
        b.dump_outputs(d, losses, variables, budget=budget)
        files = sorted(os.listdir(d))
        assert files == sorted(['g_loss.npy', 'd_loss.npy', 'generator.vars.fc1.weights.npy', 'generator.vars.fc1.bias.npy',
                                'discriminator.vars.c3.weights.npy'])
        assert sum(os.path.getsize(os.path.join(d, f)) - 128 for f in files) <= budget     # 128 B: the .npy header
        outs.append({f[:-4]: np.load(os.path.join(d, f)) for f in files})
    a, c = outs
    assert a['g_loss'].dtype == np.float64 and float(a['g_loss']) == 1.25 and float(a['d_loss']) == -0.5
    assert np.array_equal(a['generator.vars.fc1.bias'], variables['generator/vars/fc1/bias'])
    for name in ('generator.vars.fc1.weights', 'discriminator.vars.c3.weights'):
        full = variables[name.replace('.', '/')].reshape(-1)
        assert a[name].dtype == np.float32 and a[name].shape == (16384,)
        assert np.array_equal(a[name], c[name])                      # the same positions in both runs
        assert np.isin(a[name], full).all()
        assert len(np.unique(a[name])) == 16384                      # drawn without repeats
        assert np.all(np.diff(np.abs(a[name])) > 0)                  # in the variable's own order
