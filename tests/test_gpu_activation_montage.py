"""tdg_activation_montage against the NumPy oracle (_montage_ref.py), bit-equal in the bytes and in (lo, hi): one job table
with every shape class -- padded channels, a 1x1 layer, a channel window at a misaligned base, one channel, a prime channel
count, all-zero, all-negative, non-finite and relu-like images -- canaries around and between the output regions, a second
launch, every kind of bad job, and the montage items of a live paper_cgan."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg

import _montage_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CANARY = 0xA5


def _values(rng, h, w, c, kind):
    x = rng.standard_normal((h, w, c)).astype(np.float32)
    if kind == 'zero':
        x[:] = 0.0
    elif kind == 'negative':
        x = -np.abs(x) - np.float32(0.125)
    elif kind == 'relu':
        x = np.maximum(x, 0.0)
    elif kind == 'positive':
        x = np.abs(x)
    elif kind == 'nonfinite':
        flat = x.reshape(-1)
        flat[[0, 7, flat.size // 2]] = np.nan
        flat[[3, flat.size - 1]] = np.inf
        flat[[5, 11]] = -np.inf
    return x


def _device_image(x, cs, bf16, c_off=0, misalign=False):
    """The [h, w, c] image as channels [c_off, c_off + c) of an [h, w, cs] device buffer whose other channels are NaN, ending
    right behind the last live element when the window is the right-hand one.  Returns (tensor kept alive, pointer to pixel
    (0,0) channel 0 of the window, the image as the device holds it, f32)."""
    h, w, c = x.shape
    full = np.full((h, w, cs), np.nan, np.float32)
    full[:, :, c_off:c_off + c] = x
    flat = torch.from_numpy(full.reshape(-1))
    flat = flat[:(h * w - 1) * cs + c_off + c]                   # nothing behind the last live element of the last pixel
    dt = torch.bfloat16 if bf16 else torch.float32
    store = torch.empty(flat.numel() + 1, dtype=dt, device=DEV)
    t = store[1:] if misalign else store[:-1]                    # misalign: the base is aligned to one element only
    t.copy_(flat.to(dt))
    held = torch.as_strided(t.float().cpu(), (h, w, c), (w * cs, cs, 1), c_off).numpy().copy()
    return store, t.data_ptr() + c_off * t.element_size(), held


SPECS = [  # h, w, c, cs, bf16, c_off, misalign, kind
    (5, 5, 6, 8, False, 0, False, 'normal'),
    (1, 1, 512, 512, True, 0, False, 'relu'),
    (31, 31, 64, 128, True, 64, True, 'relu'),
    (29, 29, 1, 8, False, 0, False, 'normal'),
    (3, 2, 7, 7, False, 0, True, 'positive'),
    (4, 4, 4, 8, False, 0, False, 'zero'),
    (4, 3, 2, 8, True, 0, False, 'negative'),
    (6, 5, 12, 16, False, 0, False, 'nonfinite'),
    (7, 7, 16, 16, True, 0, False, 'relu'),
]
GAPS = [7, 3, 1, 5, 2, 9, 1, 4, 6, 11]                           # canary bytes before job k; the last one behind them all


@pytest.fixture(scope='module')
def table():
    K, L = pkg('kernels'), pkg('_lib')
    rng = np.random.default_rng(5)
    keep, jobs, refs, regions, off = [], [], [], [], 0
    for k, (h, w, c, cs, bf16, c_off, misalign, kind) in enumerate(SPECS):
        store, p, held = _device_image(_values(rng, h, w, c, kind), cs, bf16, c_off, misalign)
        keep.append(store)
        off += GAPS[k]
        jobs.append(L.MontageJob(p, h, w, c, cs, K.BF16 if bf16 else K.F32, 0, off))
        regions.append((off, h * w * c))
        refs.append(M.montage(held))
        off += h * w * c
    out_bytes = off + GAPS[-1]
    return SimpleNamespace(keep=keep, jobs=jobs, refs=refs, regions=regions, out_bytes=out_bytes)


def launch(jobs, out, res):
    """The raw entry: (status, error text)."""
    K, L = pkg('kernels'), pkg('_lib')
    lib = L.load()
    arr = (L.MontageJob * len(jobs))(*jobs)
    dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    st = lib.tdg_activation_montage(K.ptr(dev), len(jobs), K.ptr(out), out.numel(), K.ptr(res), K.stream())
    torch.cuda.synchronize()
    return st, lib.tdg_last_error().decode()


def fresh(t):
    out = torch.full((t.out_bytes,), CANARY, dtype=torch.uint8, device=DEV)
    res = torch.full((2 * len(t.jobs),), -7.0, dtype=torch.float32, device=DEV)
    return out, res


def test_every_job_equals_the_oracle_and_the_canaries_survive(table):
    out, res = fresh(table)
    st, err = launch(table.jobs, out, res)
    assert st == 0, err
    host, rng = out.cpu().numpy(), res.cpu().numpy().reshape(-1, 2)
    covered = np.zeros(table.out_bytes, bool)
    for k, ((off, n), (ref, lo, hi)) in enumerate(zip(table.regions, table.refs)):
        assert ref.size == n
        assert np.array_equal(host[off:off + n].reshape(ref.shape), ref), SPECS[k]
        assert (float(rng[k, 0]), float(rng[k, 1])) == (lo, hi), SPECS[k]
        covered[off:off + n] = True
    assert (~covered).sum() == sum(GAPS) and np.all(host[~covered] == CANARY)
    kinds = {s[7]: r for s, r in zip(SPECS, table.refs)}
    assert not kinds['zero'][0].any() and kinds['zero'][1:] == (0.0, 0.0)
    assert kinds['negative'][2] < 0 and kinds['negative'][0].max() <= 128 and kinds['negative'][0].min() <= 1
    assert (kinds['nonfinite'][0] == 255).sum() >= 7 and np.isfinite(kinds['nonfinite'][1:]).all()
    relu = table.refs[8][0]
    assert 0.25 < (relu == 0).mean() < 0.75 and relu.max() >= 254
    # a second launch is bit-equal
    out2, res2 = fresh(table)
    assert launch(table.jobs, out2, res2)[0] == 0
    assert torch.equal(out, out2) and torch.equal(res.view(torch.int32), res2.view(torch.int32))


def _edit(job, **kw):
    L = pkg('_lib')
    j = L.MontageJob(job.ptr, job.h, job.w, job.c, job.cs, job.dtype, 0, job.out_offset)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


@pytest.mark.parametrize('what', ['null', 'h', 'w', 'c', 'cs', 'dtype', 'past_the_end', 'offset_past_the_end', 'overlap', 'misaligned', 'no_jobs'])
def test_a_bad_job_is_a_status_and_nothing_is_written(table, what):
    K = pkg('kernels')
    good = table.jobs[0]                                         # 5x5x6 f32, 150 bytes at offset 7
    out, res = fresh(table)
    jobs = [table.jobs[3], None]
    if what == 'null':
        jobs[1] = _edit(good, ptr=None)
    elif what in ('h', 'w', 'c'):
        jobs[1] = _edit(good, **{what: 0 if what == 'h' else -1})
    elif what == 'cs':
        jobs[1] = _edit(good, cs=5)
    elif what == 'dtype':
        jobs[1] = _edit(good, dtype=7)
    elif what == 'past_the_end':
        jobs[1] = _edit(good, out_offset=table.out_bytes - 149)
    elif what == 'offset_past_the_end':
        jobs[1] = _edit(good, out_offset=(1 << 63) + 5)
    elif what == 'overlap':
        jobs[1] = _edit(good, out_offset=table.jobs[3].out_offset + 29 * 29 - 1)
    elif what == 'misaligned':
        jobs[1] = _edit(table.jobs[1], ptr=table.jobs[1].ptr + 1)       # a bf16 image at an odd address
    elif what == 'no_jobs':
        jobs = []
    if jobs:
        st, err = launch(jobs, out, res)
    else:
        lib = pkg('_lib').load()
        st = lib.tdg_activation_montage(K.ptr(out), 0, K.ptr(out), out.numel(), K.ptr(res), K.stream())
        torch.cuda.synchronize()
        err = lib.tdg_last_error().decode()
    assert st != 0 and 'tdg_activation_montage' in err, (what, st, err)
    assert bool((out == CANARY).all()) and bool((res == -7.0).all()), what


def test_the_montage_items_of_a_live_paper_cgan():
    K = pkg('kernels')
    B = 4
    g = torch.Generator().manual_seed(0)
    xs = [(torch.rand(B, 65, 65, 3, generator=g).to(DEV), (torch.rand(B, 65, 65, 1, generator=g) * 0.98 + 0.01).to(DEV)) for _ in range(2)]
    source = SimpleNamespace(i=0)

    def next_batch():
        source.i += 1
        return xs[(source.i - 1) % len(xs)]
    source.next_batch = next_batch
    args = SimpleNamespace(batch_size=B, n_gpus=1, model_version='baseline', training_version='gan', seed=0, use_graphs=True,
                           g_lr=2e-5, d_lr=1e-5, g_beta1=0.5, d_beta1=0.8, g_beta2=0.99, d_beta2=0.995)
    sess = pkg('runtime').Session(device=DEV, dtype=K.BF16, seed=0, rank=0, world_size=1)
    rep = pkg('models.paper.paper_cgan').paper_cgan(source, args, sess)
    rep.train()
    items = rep.montage_items()
    acts = {t for t, _, _ in rep.summary_items() if '_activations/' in t}
    assert len(acts) == 18 and {t for t, _ in items} == {t + '/montage' for t in acts}
    am = K.ActivationMontages(DEV, items)
    got = am.run()
    assert list(got) == [t for t, _ in items]
    for tag, act in items:
        ref, lo, hi = M.montage(act.get()[0])
        img, glo, ghi = got[tag]
        assert img.dtype == np.uint8 and img.shape == ref.shape and np.array_equal(img, ref), tag
        assert (glo, ghi) == (lo, hi), tag
    assert got['g_activations/generator/encoder/e1/montage'][0].shape == (8 * 31, 8 * 31)
    assert got['d_activations/discriminator/combined_path/h1/montage'][0].shape == (32, 32)        # 1x1x1024
    assert got['g_activations/generator/decoder/d4/montage'][0].shape == (29, 29)
    again = am.run()
    assert all(np.array_equal(again[t][0], got[t][0]) and again[t][1:] == got[t][1:] for t in got)
