"""tdg_conv2d_dispatch reproduces tests/golden/conv_dispatch.json: what every recorded (descriptor, n_images, form, epilogue
flags, n_first, switches) dispatched to before the choice was gathered into one pure step.  No GPU: the query enqueues
nothing.  Layout of the table and of the child process: tests/_conv_dispatch.py."""
import json
import os
import subprocess
import sys

import _conv_dispatch as D


def _groups(table):
    """{index of an environment: [row indices]}"""
    out = {}
    for i, row in enumerate(table['rows']):
        out.setdefault(row[5], []).append(i)
    return out


def _mismatches(table, idx, got):
    bad = []
    for i, g in zip(idx, got):
        d, n, form, e, n_first, env, want = table['rows'][i]
        if g != table['results'][want]:
            bad.append('%s n=%d form=%d epi=%s n_first=%d env=%s: got %r, recorded %r' % (
                table['descs'][d], n, form, table['epis'][e], n_first, table['envs'][env], g, table['results'][want]))
    return bad


def test_table_covers_every_family():
    """The table is not empty where it matters: every kernel family, default rows, refused rows, every switch of the table."""
    t = D.load_table()
    names = [r for r in t['results'] if isinstance(r, str)]
    for family in ('igemm_fwd_kernel<', 'igemm_fwd_dma_kernel<', 'igemm_fwd_patch_kernel<', 'igemm_fwd_bp_kernel<', 'thin_fwd_kernel<',
                   'conv_n1_fwd_kernel<', 'bwd_col2im_kernel<', 'bwd_fused_kernel<', 'igemm_wgrad_kernel<', 'igemm_wgrad_dma_kernel<',
                   'igemm_wgrad_patch_kernel<'):
        assert any(n.startswith(family) for n in names), family
    assert any(isinstance(r, int) and r < 0 for r in t['results'])
    assert {} in t['envs']
    assert set().union(*t['envs']) == D.ONCE | D.PER_CALL


def test_per_call_switches(monkeypatch):
    """Rows that set no read-once switch, in this process: the per-call switches are re-read by every query."""
    t = D.load_table()
    for var in [v for v in os.environ if v.startswith('TDG_') and v != 'TDG_LIB_PATH']:
        monkeypatch.delenv(var)
    bad = []
    for e, idx in _groups(t).items():
        env = t['envs'][e]
        if D.ONCE & set(env):
            continue
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            bad += _mismatches(t, idx, [D.ask_row(t, t['rows'][i]) for i in idx])
    assert not bad, '%d rows differ:\n%s' % (len(bad), '\n'.join(bad[:20]))


def test_read_once_switches():
    """Rows that set a read-once switch: one fresh process per setting, all started together."""
    t = D.load_table()
    base = {k: v for k, v in os.environ.items() if not k.startswith('TDG_') or k == 'TDG_LIB_PATH'}
    jobs = []
    for e, idx in _groups(t).items():
        env = t['envs'][e]
        if D.ONCE & set(env):
            p = subprocess.Popen([sys.executable, os.path.join(D.ROOT, 'tests', '_conv_dispatch.py')] + [str(i) for i in idx],
                                 env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            jobs.append((p, idx))
    assert jobs
    bad = []
    for p, idx in jobs:
        out, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
        bad += _mismatches(t, idx, json.loads(out.strip().splitlines()[-1]))
    assert not bad, '%d rows differ:\n%s' % (len(bad), '\n'.join(bad[:20]))
