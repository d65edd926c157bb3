"""tdg_tensor_summary per element against the float64 oracle (tests/_summary_ref.py), in both dtypes: buckets, num, zeros,
nonfinite, min and max exact; sum and sum_squares within n * 2^-53 * sum |term| of math.fsum (the bound of a recursive f64
summation in any order; the f64 square of an f32 is exact).  Every tensor lies inside a larger allocation whose padding
channels and whose elements behind the last live one are poisoned with NaN and 1e30: the result must not see them.
The cases are built, and every launch is run, once per module."""
import numpy as np
import pytest

from conftest import pkg

import _summary_ref as R

pytestmark = pytest.mark.gpu

TAIL = 67                   # poisoned elements behind the last live one
# (rows, c, cs, element offset of the window inside its buffer)
SHAPES = [(1, 1, 8, 0), (7, 3, 8, 0), (7, 3, 8, 5), (961, 64, 136, 64), (961, 1, 137, 136), (961, 1, 137, 135), (25, 512, 512, 0)]
FLAT_F32 = [1, 255, 256, 257, 1051653, 2100227]      # the last: more chunks than the largest grid has blocks


def _poisoned(n, rng):
    return np.where(rng.integers(0, 2, n) == 0, np.float32(np.nan), np.float32(1e30)).astype(np.float32)


def _mixed(n, rng):
    """Spread magnitudes on both sides of zero, with zeros among them."""
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 4, n)
    v[rng.integers(0, 5, n) == 0] = 0.0
    return v.astype(np.float32)


def _value_sets(dtype, rng):
    """name -> f32 values representable in the dtype."""
    fmax = np.array([0x7F7F0000], np.uint32).view(np.float32)[0] if dtype == 'bf16' else np.finfo(np.float32).max
    den = np.float32(2.0 ** -133) if dtype == 'bf16' else np.float32(1e-45)                   # the dtype's smallest denormal
    relu = np.maximum(rng.standard_normal(4096), 0.0).astype(np.float32)
    mix = _mixed(600, rng)
    mix[::7] = np.nan
    mix[3::11] = np.inf
    mix[5::13] = -np.inf
    return {
        'edges': R.edge_values(dtype),
        'specials': np.array([0.0, -0.0, den, -den, den * 3, np.float32(2.0 ** -126), fmax, -fmax, 1.0, -1.0], np.float32),
        'all_zero': np.zeros(3000, np.float32),
        'all_equal': np.full(3000, 0.37109375, np.float32),
        'relu': relu,
        'nonfinite_mix': mix,
        'only_nonfinite': np.array([np.nan, np.inf, -np.inf, np.nan] * 20, np.float32),
    }


class Case:
    def __init__(self, name, dtype, rows, c, cs, off, live, scale, K, dev, rng):
        import torch
        self.name, self.scale = name, scale
        tdt = torch.bfloat16 if dtype == 'bf16' else torch.float32
        live = torch.from_numpy(np.ascontiguousarray(live, np.float32).reshape(rows, c)).to(tdt)        # rounds to the dtype
        self.live = live.float().numpy()                                                          # what the kernel must see
        total = off + (rows - 1) * cs + c + TAIL
        host = torch.from_numpy(_poisoned(total, rng)).to(tdt)
        torch.as_strided(host, (rows, c), (cs, 1), off).copy_(live)
        self.buf = host.to(dev)
        code = K.BF16 if dtype == 'bf16' else K.F32
        if cs == c and rows == 1:
            self.item = self.buf[off:off + c]                                                      # a flat tensor
        else:
            self.item = K.Act(1, rows, 1, c, code, dev, cs, self.buf[off:])
        self.ref = R.summary(self.live, scale)


@pytest.fixture(scope='module')
def world():
    import torch
    K = pkg('kernels')
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(11)
    cases = []
    for dtype in ('f32', 'bf16'):
        for rows, c, cs, off in SHAPES:
            cases.append(Case('%s_%dx%dx%d+%d' % (dtype, rows, c, cs, off), dtype, rows, c, cs, off, _mixed(rows * c, rng), 1.0, K, dev, rng))
        sets = _value_sets(dtype, rng)
        for name, v in sets.items():
            cases.append(Case('%s_%s' % (dtype, name), dtype, 1, v.size, v.size, 0, v, 1.0, K, dev, rng))
        # the edge set again through two windows, so that the strided paths (wide and scalar) meet every bucket too
        e = sets['edges'][:4640]
        cases.append(Case('%s_edges_window' % dtype, dtype, 145, 32, 40, 8, e, 1.0, K, dev, rng))
        cases.append(Case('%s_edges_odd_window' % dtype, dtype, 928, 5, 7, 3, e, 1.0, K, dev, rng))
        for scale in (0.5, 1.0 / 3.0):
            cases.append(Case('%s_scale_%.3f' % (dtype, scale), dtype, 50, 24, 32, 8, rng.standard_normal(1200).astype(np.float32), scale,
                              K, dev, rng))
    for n in FLAT_F32:
        cases.append(Case('f32_flat_%d' % n, 'f32', 1, n, n, 0, _mixed(n, rng), 1.0, K, dev, rng))
    cases.append(Case('f32_flat_257_unaligned', 'f32', 1, 257, 257, 1, _mixed(257, rng), 1.0, K, dev, rng))      # a 4-byte aligned base
    cases.append(Case('bf16_flat_4099_unaligned', 'bf16', 1, 4099, 4099, 1, _mixed(4099, rng), 1.0, K, dev, rng))  # a 2-byte aligned base
    for k in range(40):
        cases.append(Case('f32_small_%d' % k, 'f32', 1, 64, 64, 0, rng.standard_normal(64).astype(np.float32), 1.0, K, dev, rng))
    batch = K.TensorSummaries(dev, [(c.name, c.item, c.scale) for c in cases])
    first = batch.run()
    raw1 = batch.results.cpu().numpy().copy()
    second = batch.run()
    raw2 = batch.results.cpu().numpy().copy()
    singles = {c.name: K.TensorSummaries(dev, [(c.name, c.item, c.scale)]).run()[c.name] for c in cases}
    return {'cases': {c.name: c for c in cases}, 'first': first, 'second': second, 'raw': (raw1, raw2), 'singles': singles, 'K': K,
            'dev': dev, 'batch': batch}


def case_names():
    names = []
    for dtype in ('f32', 'bf16'):
        names += ['%s_%dx%dx%d+%d' % ((dtype,) + s) for s in SHAPES]
        names += ['%s_%s' % (dtype, n) for n in ('edges', 'specials', 'all_zero', 'all_equal', 'relu', 'nonfinite_mix', 'only_nonfinite',
                                                 'edges_window', 'edges_odd_window', 'scale_0.500', 'scale_0.333')]
    names += ['f32_flat_%d' % n for n in FLAT_F32] + ['f32_flat_257_unaligned', 'bf16_flat_4099_unaligned', 'f32_small_0', 'f32_small_39']
    return names


def check(s, ref, name):
    got = (s.num, s.zeros, s.nonfinite, s.min, s.max)
    want = (ref['num'], ref['zeros'], ref['nonfinite'], ref['min'], ref['max'])
    print(name, 'counts/min/max', got, want)
    bad = np.nonzero(s.buckets != ref['buckets'])[0]
    print(name, 'buckets that differ', bad[:10], s.buckets[bad[:10]], ref['buckets'][bad[:10]])
    bs, bq = R.sum_bounds(ref)
    print(name, 'sum error %.3e (bound %.3e), sum_squares error %.3e (bound %.3e)' % (
        abs(s.sum - ref['sum']), bs, abs(s.sum_squares - ref['sum_squares']), bq))
    assert got == want
    assert bad.size == 0
    assert abs(s.sum - ref['sum']) <= bs and abs(s.sum_squares - ref['sum_squares']) <= bq


@pytest.mark.parametrize('name', case_names())
def test_batched_summary_against_the_oracle(world, name):
    assert set(case_names()) <= set(world['cases'])
    check(world['first'][name], world['cases'][name].ref, name)


def test_edge_set_reaches_every_bucket_on_the_device(world):
    for dtype in ('f32', 'bf16'):
        for name in ('%s_edges' % dtype, '%s_edges_window' % dtype, '%s_edges_odd_window' % dtype):
            b = world['first'][name].buckets
            assert b[0] == 0 and np.count_nonzero(b[1:]) >= 1549, name
        assert np.all(world['first']['%s_edges' % dtype].buckets[1:] > 0)
    s = world['first']['f32_only_nonfinite']
    assert (s.num, s.nonfinite, s.zeros, s.min, s.max, s.sum, s.sum_squares, int(s.buckets.sum())) == (80, 80, 0, 0.0, 0.0, 0.0, 0.0, 0)
    z = world['first']['bf16_all_zero']
    assert z.zeros == z.num == z.buckets[776] == 3000 and z.sparsity == 1.0
    assert world['first']['f32_relu'].buckets[776] == world['first']['f32_relu'].zeros > 1500


def test_batch_equals_one_job_at_a_time_and_repeats_bit_equal(world):
    raw1, raw2 = world['raw']
    assert raw1.tobytes() == raw2.tobytes()                               # two launches: every field bit-equal
    for name, c in world['cases'].items():
        a, b = world['first'][name], world['singles'][name]
        for f in ('num', 'zeros', 'nonfinite'):
            assert getattr(a, f) == getattr(b, f), (name, f)
        for f in ('min', 'max', 'sum', 'sum_squares'):
            assert np.float64(getattr(a, f)).tobytes() == np.float64(getattr(b, f)).tobytes(), (name, f)
        assert np.array_equal(a.buckets, b.buckets), name


def test_argument_errors_write_nothing(world):
    import torch
    L, K, dev = pkg('_lib'), world['K'], world['dev']
    lib = L.load()
    x = torch.zeros(64, dtype=torch.float32, device=dev)
    rec = lib.tdg_tensor_summary_result_bytes()
    assert rec == 48 + 8 * 1551 == K.RESULT_DTYPE.itemsize
    results = torch.full((2 * rec,), 0xAB, dtype=torch.uint8, device=dev)
    ws = torch.full((4096,), 0xCD, dtype=torch.uint8, device=dev)
    limits = K.summary_limits(dev)

    def table(*jobs):
        t = (L.SummaryJob * len(jobs))(*jobs)
        return torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev)
    good = L.SummaryJob(x.data_ptr(), 1, 64, 64, K.F32, 1.0)

    def call(jobs, njobs, ws_bytes=4096, lim=limits, out=results):
        rc = lib.tdg_tensor_summary(K.ptr(jobs), njobs, K.ptr(lim), K.ptr(out), K.ptr(ws), ws_bytes, K.stream())
        torch.cuda.synchronize()
        return rc, lib.tdg_last_error().decode()
    assert lib.tdg_tensor_summary_workspace_bytes(2, 128) == 64 and lib.tdg_tensor_summary_workspace_bytes(0, 128) == 0
    assert lib.tdg_tensor_summary_workspace_bytes(1, 1051653) >= 1028 * 32
    cases = [
        (call(None, 1), -1, 'bad argument'),
        (call(table(good), 0), -1, 'bad argument'),
        (call(table(good), 1, lim=None), -1, 'bad argument'),
        (call(table(good), 1, out=None), -1, 'bad argument'),
        (call(table(good, L.SummaryJob(x.data_ptr(), 4, 9, 8, K.F32, 1.0)), 2), -1, 'job 1'),                  # c > cs
        (call(table(good, L.SummaryJob(x.data_ptr(), 1, 64, 64, 7, 1.0)), 2), -1, 'bad dtype 7'),
        (call(table(good, L.SummaryJob(0, 1, 64, 64, K.F32, 1.0)), 2), -1, 'job 1'),                           # null tensor
        (call(table(good, L.SummaryJob(x.data_ptr() + 2, 1, 8, 8, K.F32, 1.0)), 2), -1, 'misaligned'),
        (call(table(good, good), 2, ws_bytes=32), -4, 'workspace'),
    ]
    for (rc, msg), want, text in cases:
        assert rc == want and text in msg, (rc, msg, want, text)
    assert bool((results == 0xAB).all()) and bool((ws == 0xCD).all())
    rc, msg = call(table(good, good), 2, ws_bytes=64)                       # and the same table with enough workspace runs
    assert rc == 0, msg
    got = results.cpu().numpy().view(K.RESULT_DTYPE)
    assert list(got['num']) == [64, 64] and list(got['zeros']) == [64, 64] and got['buckets'][1][776] == 64
