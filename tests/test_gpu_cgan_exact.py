"""tdg_cgan_prep, the four generator-head entries, tdg_cgan_wgan_loss and tdg_cgan_metrics (csrc/tdg_cgan.hip) against the
float64 references of tests/_exact_cgan.py: bit for bit where the tables make exactness provable, per element against
derived bounds elsewhere.  Inputs are NaN wherever a kernel must not read, outputs hold the sentinel wherever it must not
write, every kernel is launched twice into fresh buffers (all outputs bit-equal), a refused call leaves every output
untouched.  The conditions of the exact comparisons are proved on the CPU (tests/test_host_cgan_exact.py).

Each bounded comparison prints its worst ratio (`RATIO <what> <value>`, run with -s); DESIGN.md section 2 records them."""
import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_cgan as G

pytestmark = pytest.mark.gpu

DTYPES = [0, 1]
ES = {0: 4, 1: 2}
DT = {0: 'f32', 1: 'bf16'}
EINVAL, EWORKSPACE = -1, -4
f32, f64 = np.float32, np.float64


def K():
    return pkg('kernels')


def call(name, *args):
    pkg('_lib').call(name, *args)


def status(name, *args):
    return getattr(pkg('_lib').load(), name)(*args)


def dev():
    return torch.device('cuda:0')


def exact(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want), '%s\n%s' % (what, G.describe_mismatch(got, want.astype(got.dtype)))


def within(ratio, what):
    """`ratio`: |error| / bound per element.  Prints the worst one, then asserts it."""
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    print('RATIO %s %.4g' % (what, worst))
    if not worst <= 1.0:
        bad = np.argwhere(~(np.asarray(ratio) <= 1.0))
        raise AssertionError('%s: %d of %d miss the bound, worst ratio %g, first at %s'
                             % (what, len(bad), np.size(ratio), worst, tuple(int(i) for i in bad[0])))


class In:
    """An input on the device: `front` NaNs, the array, G.TAIL NaNs.  The array carries its own NaNs where it is not live."""

    def __init__(self, a, dtype=0, front=0):
        a = np.asarray(a, f32)
        flat = np.concatenate([np.full(front, G.NAN, f32), a.ravel(), np.full(G.TAIL, G.NAN, f32)])
        self.t = torch.from_numpy(flat).to(dev()).to(K().TORCH_DTYPE[dtype])
        self.off = front * ES[dtype]

    def ptr(self):
        return K().ptr(self.t, self.off)


class Out:
    """An output of `shape` on the device between `front` and G.TAIL sentinels, everything prefilled with the sentinel."""

    def __init__(self, shape, dtype=0, front=0):
        self.shape, self.front, self.dtype = tuple(shape), front, dtype
        self.n = int(np.prod(shape))
        self.t = torch.full((front + self.n + G.TAIL,), G.SENTINEL, dtype=K().TORCH_DTYPE[dtype], device=dev())

    def ptr(self, elems=0):
        return K().ptr(self.t, (self.front + elems) * ES[self.dtype])

    def get(self):
        flat = self.t.float().cpu().numpy()
        guard = np.concatenate([flat[:self.front], flat[self.front + self.n:]])
        assert np.all(guard == G.SENTINEL), 'a write landed outside the %s buffer' % (self.shape,)
        return flat[self.front:self.front + self.n].reshape(self.shape)


def same_runs(a, b, what):
    for k in a:
        assert G.same_bits(a[k], b[k]), '%s: %s differs between two launches' % (what, k)


def untouched(*outs):
    for o in outs:
        assert np.all(o.get() == G.SENTINEL), 'a refused call wrote to an output'


# ================================================================================================ tdg_cgan_prep
def prep_buffers(n, strides, dtype):
    dcs, gcs, rcs = strides
    return G.NS(real=Out((n, G.NPIX, dcs), dtype), fake=Out((n, G.NPIX, dcs), dtype), ybar=Out((n,)), crop=Out((n, G.NPIX)),
                g_ones=Out((n, G.NSRC, gcs), dtype), rgb_ybar=Out((n, G.NSRC, rcs), dtype))


def run_prep(y, n, version, strides, dtype, with_g=True):
    o = prep_buffers(n, strides, dtype)
    dcs, gcs, rcs = strides
    call('tdg_cgan_prep', dtype, y.ptr(), n, version, o.real.ptr(), dcs, o.fake.ptr(), o.ybar.ptr(), o.crop.ptr(),
         o.g_ones.ptr(G.PREP_GCH) if with_g else None, gcs, o.rgb_ybar.ptr(G.PREP_GCH) if with_g else None, rcs, K().stream())
    return {k: getattr(o, k).get() for k in ('real', 'fake', 'ybar', 'crop', 'g_ones', 'rgb_ybar')}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', G.PREP_N)
@pytest.mark.parametrize('version', G.PREP_VERSIONS)
def test_prep_exact(version, n, dtype):
    """The symmetric crop: crop, ybar, both halves of depth, g_ones and rgb_ybar bit for bit, every other element of every
    buffer still the sentinel, y NaN outside rows and columns [17, 46)."""
    inp = G.prep_exact_inputs(n)
    v = G.prep_crop_ref(inp.y)
    y = In(inp.y)
    for strides in G.prep_strides(version):
        for with_g in (True, False):
            what = '%s prep v%d n=%d strides=%s g=%s' % (DT[dtype], version, n, strides, with_g)
            want = G.prep_expected(v, inp.centre, version, strides, dtype, with_g)
            a, b = (run_prep(y, n, version, strides, dtype, with_g) for _ in range(2))
            same_runs(a, b, what)
            for k in a:
                exact(a[k].reshape(getattr(want, k).shape), getattr(want, k), '%s: %s' % (what, k))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', G.PREP_N)
@pytest.mark.parametrize('version', G.PREP_VERSIONS)
def test_prep_bounded(version, n, dtype):
    """Uniform y: crop is exact (one rounded product), ybar lies within the reduction tree's bound of the float64 mean, and
    every other output is exact at the device's own ybar."""
    inp = G.prep_bounded_inputs(n)
    v = G.prep_crop_ref(inp.y)
    m, bound = G.prep_ybar_ref(v)
    strides = G.prep_strides(version)[0]
    what = '%s prep v%d n=%d uniform' % (DT[dtype], version, n)
    a, b = (run_prep(In(inp.y), n, version, strides, dtype) for _ in range(2))
    same_runs(a, b, what)
    within(G.bound_ratio(a['ybar'], m, bound), what + ' ybar')
    want = G.prep_expected(v, a['ybar'], version, strides, dtype)
    for k in a:
        exact(a[k].reshape(getattr(want, k).shape), getattr(want, k), '%s: %s' % (what, k))


def test_prep_refusals():
    n, dtype = 1, 0
    y = In(G.prep_exact_inputs(n).y)
    o = prep_buffers(n, (2, 4, 8), dtype)

    def rc(version=2, dcs=2, fake=True, gcs=4, n_=n):
        return status('tdg_cgan_prep', dtype, y.ptr(), n_, version, o.real.ptr(), dcs, o.fake.ptr() if fake else None, o.ybar.ptr(),
                      o.crop.ptr(), o.g_ones.ptr(G.PREP_GCH), gcs, o.rgb_ybar.ptr(G.PREP_GCH), 8, K().stream())

    assert rc(version=3) == EINVAL and rc(version=-1) == EINVAL
    assert rc(dcs=1) == EINVAL
    assert rc(fake=False) == EINVAL
    assert rc(gcs=0) == EINVAL
    assert rc(n_=0) == EINVAL
    assert status('tdg_cgan_prep', 7, y.ptr(), n, 2, o.real.ptr(), 2, o.fake.ptr(), o.ybar.ptr(), o.crop.ptr(), None, 0, None, 0,
                  K().stream()) == EINVAL
    torch.cuda.synchronize()
    untouched(o.real, o.fake, o.ybar, o.crop, o.g_ones, o.rgb_ybar)


# ================================================================================================ the generator head
HEAD_CASES = [(cin, g) for cin in G.HEAD_CINS for g in G.HEAD_GEOMS]
HEAD_IDS = [G.head_id(cin, g) for cin, g in HEAD_CASES]


class HeadDev:
    """One table entry on the device.  The plain forms get w of cin entries followed by NaN (w[cin] is not theirs to read)."""

    def __init__(self, inp, dtype, noise, u=None):
        self.inp, self.dtype, self.noise = inp, dtype, noise
        self.cat = In(inp.cat, dtype)
        self.w = In(inp.w if noise else inp.w[:inp.cin])
        self.b = In(inp.b)
        self.u = In(inp.u if u is None else u) if noise else None
        self.ybar = In(inp.ybar) if inp.ybar is not None else None
        self.dfake = In(inp.dfake, dtype)
        self.cols = inp.cin + (2 if noise else 1)

    def fwd(self, with_g32=True):
        i = self.inp
        npix = i.crop * i.crop
        yhat, g32, fake = Out((i.n, npix)), Out((i.n, npix)), Out((i.n, npix, G.HEAD_FAKE_CS), self.dtype)
        yb = self.ybar.ptr() if self.ybar else None
        if self.noise:
            call('tdg_cgan_head_noise_fwd', self.dtype, self.cat.ptr(), i.n, i.hw, i.cin, i.cs, i.crop, self.w.ptr(), self.b.ptr(),
                 self.u.ptr(), yb, yhat.ptr(), g32.ptr() if with_g32 else None, fake.ptr(), G.HEAD_FAKE_CS, K().stream())
        else:
            call('tdg_cgan_head_fwd', self.dtype, self.cat.ptr(), i.n, i.hw, i.cin, i.cs, i.crop, self.w.ptr(), self.b.ptr(), yb,
                 yhat.ptr(), fake.ptr(), G.HEAD_FAKE_CS, K().stream())
        return dict(yhat=yhat.get(), g32=g32.get(), fake=fake.get())

    def bwd_args(self, mode, dcat, dw, db, ws, ws_bytes, cin=None, cs=None, crop=None):
        i = self.inp
        head = (self.dtype, self.dfake.ptr(), G.HEAD_FAKE_CS, self.cat.ptr(), i.n, i.hw, cin or i.cin, cs or i.cs, crop or i.crop, self.w.ptr())
        tail = (mode, G.HEAD_LEAK, dcat.ptr(), dw.ptr(), db.ptr(), ws.ptr(), ws_bytes, K().stream())
        return head + ((self.u.ptr(),) if self.noise else ()) + tail

    def bwd_outs(self):
        i = self.inp
        return (Out((i.n, i.hw, i.hw, i.cs), self.dtype), Out((self.cols - 1,)), Out((1,)), Out((i.n * self.cols,)))

    def bwd(self, mode):
        dcat, dw, db, ws = self.bwd_outs()
        call('tdg_cgan_head_noise_bwd' if self.noise else 'tdg_cgan_head_bwd', *self.bwd_args(mode, dcat, dw, db, ws, ws.n * 4))
        ws.get()
        return dict(dcat=dcat.get(), dw=dw.get(), db=db.get())


def check_head(h, what):
    """Forward and the three backward modes of one device entry against the float64 references, each launched twice."""
    inp, dtype, noise = h.inp, h.dtype, h.noise
    g, yhat = G.head_fwd_ref(inp, noise)
    a, b = h.fwd(), h.fwd()
    same_runs(a, b, what + ' fwd')
    exact(a['yhat'], yhat, what + ' yhat')
    exact(a['fake'], G.head_fake_expected(inp, g, dtype), what + ' fake')
    if noise:
        exact(a['g32'], g, what + ' g32')
        c = h.fwd(with_g32=False)
        assert np.all(c['g32'] == G.SENTINEL) and G.same_bits(c['yhat'], a['yhat']) and G.same_bits(c['fake'], a['fake']), what + ' g32 NULL'
    else:
        assert np.all(a['g32'] == G.SENTINEL)
    out = {'fwd': a}
    for mode in G.MASKS:
        ref = G.head_bwd_ref(inp, noise, mode)
        a, b = h.bwd(mode), h.bwd(mode)
        w2 = '%s bwd mask=%s' % (what, G.MASK_NAME[mode])
        same_runs(a, b, w2)
        exact(a['dcat'], G.head_dcat_expected(inp, ref.dcat, dtype), w2 + ' dcat')
        assert G.outside_crop_bits_ok(a['dcat'], inp), w2 + ': dcat outside the crop is not +0.0'
        exact(a['dw'], ref.dw, w2 + ' dW')
        exact(a['db'], ref.db, w2 + ' db')
        out[mode] = a
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('noise', [False, True], ids=['plain', 'noise'])
@pytest.mark.parametrize('cin,geom', HEAD_CASES, ids=HEAD_IDS)
def test_head(cin, geom, noise, dtype):
    """Every width (TPP 8 / 16 / 32 / 64), plain and noise, on the four geometries, cs = cin (scale 1, ybar given) and
    cs = cin + 8 (scale 2**-4, ybar NULL): yhat, g32, fake, dcat, dW and db equal the float64 values exactly; NaN in cat's
    padding channels and in cat and u outside the crop reaches nothing; padding channels of dcat, channels 1.. of fake
    and everything around the buffers keep the sentinel.  The noise forms at u == 0 equal the plain forms bit for bit."""
    for cfg in range(len(G.HEAD_CONFIGS)):
        inp = G.head_inputs(cin, geom, cfg)
        what = '%s head %s %s cfg%d' % (DT[dtype], 'noise' if noise else 'plain', G.head_id(cin, geom), cfg)
        got = check_head(HeadDev(inp, dtype, noise), what)
        if noise and cfg == 0:
            u0 = np.where(np.isnan(inp.u), inp.u, f32(0))
            zero, plain = HeadDev(inp, dtype, True, u=u0), HeadDev(inp, dtype, False)
            fz, fp = zero.fwd(), plain.fwd()
            assert G.same_bits(fz['yhat'], fp['yhat']) and G.same_bits(fz['fake'], fp['fake']), what + ': u == 0 against plain, fwd'
            assert not G.same_bits(fz['yhat'], got['fwd']['yhat']) or not np.any(inp.u[:, :inp.crop, :inp.crop])
            bz, bp = zero.bwd(G.MASK_LRELU), plain.bwd(G.MASK_LRELU)
            assert G.same_bits(bz['dcat'], bp['dcat']) and G.same_bits(bz['db'], bp['db']), what + ': u == 0 against plain, bwd'
            assert G.same_bits(bz['dw'][:cin], bp['dw']) and bz['dw'][cin] == 0, what + ': u == 0 against plain, dW'


@pytest.mark.parametrize('noise', [False, True], ids=['plain', 'noise'])
def test_head_refusals(noise):
    """cin 72 and 1024 (and 65, which cin / 8 let through as 64), crop > hw, cs < cin, a bad dtype: TDG_EINVAL; a workspace one
    byte short: TDG_EWORKSPACE.  Nothing is written, and a refused call leaves no record in the timing window."""
    dtype = 0
    inp = G.head_inputs(64, (1, 5, 3), 1)             # cs = 72: cin 72 would be addressable
    h = HeadDev(inp, dtype, noise)
    npix = inp.crop * inp.crop
    yhat, g32, fake = Out((1, npix)), Out((1, npix)), Out((1, npix, G.HEAD_FAKE_CS), dtype)
    fname, bname = ('tdg_cgan_head_noise_fwd', 'tdg_cgan_head_noise_bwd') if noise else ('tdg_cgan_head_fwd', 'tdg_cgan_head_bwd')

    def fwd(cin=inp.cin, cs=inp.cs, crop=inp.crop, dt=dtype):
        a = (dt, h.cat.ptr(), 1, inp.hw, cin, cs, crop, h.w.ptr(), h.b.ptr())
        if noise:
            return status(fname, *a, h.u.ptr(), None, yhat.ptr(), g32.ptr(), fake.ptr(), G.HEAD_FAKE_CS, K().stream())
        return status(fname, *a, None, yhat.ptr(), fake.ptr(), G.HEAD_FAKE_CS, K().stream())

    dcat, dw, db, ws = h.bwd_outs()

    def bwd(ws_bytes=ws.n * 4, **kw):
        return status(bname, *h.bwd_args(G.MASK_LRELU, dcat, dw, db, ws, ws_bytes, **kw))

    K().timing_begin()
    for cin in G.HEAD_REFUSED_CIN + (65,):
        assert fwd(cin=cin, cs=1024) == EINVAL and bwd(cin=cin, cs=1024) == EINVAL, cin
    assert fwd(crop=inp.hw + 1) == EINVAL and bwd(crop=inp.hw + 1) == EINVAL
    assert fwd(cs=56) == EINVAL and bwd(cs=56) == EINVAL
    assert fwd(dt=7) == EINVAL
    assert bwd(ws_bytes=ws.n * 4 - 1) == EWORKSPACE
    records = K().timing_end()
    assert records == [], records
    torch.cuda.synchronize()
    untouched(yhat, g32, fake, dcat, dw, db, ws)
    K().timing_begin()
    assert fwd() == 0 and bwd() == 0
    assert [r[0] for r in K().timing_end()] == [fname[4:], bname[4:]]


# ================================================================================================ tdg_cgan_wgan_loss
WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    return WORST[key]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', G.WGAN_ROWS)
def test_wgan_loss(rows, dtype):
    """Eighth logits in [-6, 6] at cs 1 and 8, modes 0 (seed NULL), 1 and 2: the four scalars and every seed within the bound
    the kernel's own expression gives (sigmoid, p (1 - p) * inv, the sum tree, the multiply by the rounded 1 / rows);
    scal[0] == -scal[1] and the real half's mode-2 zeros bit for bit; channels 1.. of the seed rows keep the sentinel.
    Measured on an MI355X: the scalars use 0.08 of their bound, and the two means lie up to 1.24 f32 ulps from the float64
    mean -- the cost of `* inv` against one division (printed per launch)."""
    inp = G.wgan_inputs(rows)
    for cs in G.WGAN_CS:
        zz = np.full((2 * rows, cs), G.NAN, f32)
        zz[:, 0] = inp.z
        z = In(zz, dtype)
        scals = []
        for mode in G.WGAN_MODES:
            ref = G.wgan_ref(inp, mode, dtype)
            what = '%s wgan rows=%d cs=%d mode=%d' % (DT[dtype], rows, cs, mode)
            runs = []
            for _ in range(2):
                seed, scal = Out((2 * rows, cs), dtype), Out((4,))
                call('tdg_cgan_wgan_loss', dtype, z.ptr(), rows, cs, mode, seed.ptr() if mode else None, scal.ptr(), K().stream())
                runs.append(dict(seed=seed.get(), scal=scal.get()))
            a = runs[0]
            same_runs(a, runs[1], what)
            r = G.bound_ratio(a['scal'], ref.scal, ref.scal_bound)
            within(r, what + ' scalars')
            u = G.ulps(a['scal'][1:3], ref.mean64[1:3])                     # the two means: what `* inv` costs against one division
            print('WGAN rows=%d worst scalar error / bound so far %.3g; the means in ulps of the float64 mean %.3g, so far %.3g'
                  % (rows, note('wgan scal', r.max()), u.max(), note('wgan ulps', u.max())))
            assert a['scal'][0] == -a['scal'][1] and G.same_bits(a['scal'][:1], -a['scal'][1:2])
            scals.append(a['scal'])
            assert np.all(a['seed'][:, 1:] == G.SENTINEL), what + ': a seed channel beyond 0 was written'
            if mode == 0:
                assert np.all(a['seed'] == G.SENTINEL)
                continue
            within(G.bound_ratio(a['seed'][:, 0], ref.seed, ref.seed_bound), what + ' seeds')
            if mode == 2:
                assert not np.any(G.bits(a['seed'][:rows, 0])), what + ': the real half is not +0.0'
        assert G.same_bits(scals[0], scals[1]) and G.same_bits(scals[0], scals[2])


def test_wgan_refusals():
    z, seed, scal = In(np.zeros((4, 1), f32)), Out((4, 1)), Out((4,))
    for rows, cs, mode, sd in ((0, 1, 1, seed), (2, 0, 1, seed), (2, 1, 3, seed), (2, 1, -1, seed), (2, 1, 1, None), (2, 1, 2, None)):
        assert status('tdg_cgan_wgan_loss', 0, z.ptr(), rows, cs, mode, sd.ptr() if sd else None, scal.ptr(), K().stream()) == EINVAL
    assert status('tdg_cgan_wgan_loss', 7, z.ptr(), 2, 1, 1, seed.ptr(), scal.ptr(), K().stream()) == EINVAL
    torch.cuda.synchronize()
    untouched(seed, scal)


# ================================================================================================ tdg_cgan_metrics
METRIC_IDS = ['%dx%d' % s for s in G.METRIC_SIZES]


class Metrics:
    """The streaming state of one evaluation: counts (u64 x 4, guarded), the eight values, the workspace."""

    def __init__(self):
        self.counts = torch.zeros(4 + 4, dtype=torch.int64, device=dev())
        self.counts[4:] = 77
        self.out = Out((8,))
        self.ws = torch.zeros(pkg('_lib').load().tdg_cgan_metrics_workspace_bytes(), dtype=torch.uint8, device=dev())

    def run(self, y, pred, offset, n, hw):
        ins = [In(y)] + [In(a) if a is not None else None for a in (pred, offset)]
        call('tdg_cgan_metrics', ins[0].ptr(), ins[1].ptr() if ins[1] else None, ins[2].ptr() if ins[2] else None, n, hw,
             K().ptr(self.counts), self.out.ptr(), K().ptr(self.ws), self.ws.numel(), K().stream())
        c = self.counts.cpu().tolist()
        assert c[4:] == [77] * 4, 'a write landed behind counts'
        return c[:4], self.out.get().copy()


def check_running(counts, values, what):
    """v[5..7] are the running fractions: one f64 division, one cast."""
    exact(values[5:], (np.array(counts[:3], f64) / counts[3]).astype(f32), what + ' running fractions')


@pytest.mark.parametrize('size', G.METRIC_SIZES, ids=METRIC_IDS)
def test_metrics_counts(size):
    """Every element sits on a threshold (not a hit: `<` is strict) or far from all three: the three counts and the element
    count equal the float64 counts, over two launches that keep running (pred + offset, then pred alone), and a second
    evaluation from zero repeats the first bit for bit."""
    n, hw = size
    inp = G.metric_counts_inputs(n, hw)
    runs = []
    for _ in range(2):
        m = Metrics()
        off = G.metric_offsets(n)
        c1, v1 = m.run(inp.y, inp.p10 - off[:, None], off, n, hw)
        c2, v2 = m.run(inp.y, inp.p10, None, n, hw)
        runs.append(dict(v1=v1, v2=v2, c=np.array(c1 + c2, f32)))
    same_runs(runs[0], runs[1], 'metrics counts %dx%d' % size)
    hits = G.metric_hits64(inp.y, inp.p10)
    on = int((inp.idx < G.METRIC_ON_THRESHOLD).sum())
    assert on >= min(n * hw, G.METRIC_ON_THRESHOLD)
    exact(np.array(c1), np.array(hits + [n * hw]), 'counts after one launch (%d elements on a threshold)' % on)
    exact(np.array(c2), 2 * np.array(hits + [n * hw]), 'counts after two launches')
    check_running(c1, v1, 'first launch')
    check_running(c2, v2, 'second launch')
    assert np.all(np.isfinite(v1)) and np.all(np.isfinite(v2))           # (tests/test_gpu_cgan_exact.py::test_metrics_values bounds the values)


@pytest.mark.parametrize('kind', ['y0', 'p0', 'both', 'neither'])
def test_metrics_nan_rule(kind):
    """y = 0 and / or prediction = 0 (kind 'neither': pred and offset NULL, every prediction 0): the counts equal those of
    delta = q1 < q2 ? q2 : q1 taken literally, and each of the eight values has the reference's class."""
    n, hw = 3, 70
    inp = G.metric_counts_inputs(n, hw) if kind == 'neither' else G.metric_nan_inputs(n, hw, kind)
    pred = None if kind == 'neither' else inp.p10
    p10 = G.prediction(pred, None, (n, hw))
    m = Metrics()
    c, v = m.run(inp.y, pred, None, n, hw)
    want = [0, 0, 0, 0]
    ref = G.metric_values64(inp.y, p10, want)
    exact(np.array(c), np.array(want), 'counts, %s' % kind)
    exact(G.value_class(v), G.value_class(ref), 'classes of the eight values, %s: device %s reference %s' % (kind, v, ref))
    cls = G.value_class(ref)
    assert {'y0': cls[0] == 0, 'p0': cls[0] == 1, 'both': cls[0] == 3, 'neither': cls[0] == 1}[kind], ref
    check_running(c, v, kind)


@pytest.mark.parametrize('form', ['pred+offset', 'offset', 'pred'])
@pytest.mark.parametrize('size', G.METRIC_SIZES, ids=METRIC_IDS)
def test_metrics_values(size, form):
    """y in [0.1, 10] against pred + offset, the offset alone and pred alone: the five means within the bound of their f32
    terms, f64 sums and one cast, the cancellation of v[4] included."""
    n, hw = size
    inp = G.metric_values_inputs(n, hw)
    pred = None if form == 'offset' else (inp.pred if form == 'pred+offset' else (inp.pred + f32(1.25)).astype(f32))
    offset = None if form == 'pred' else inp.offset
    p10 = G.prediction(pred, offset, (n, hw))
    assert p10.min() > 0.05
    runs = []
    for _ in range(2):
        c, v = Metrics().run(inp.y, pred, offset, n, hw)
        runs.append(dict(v=v, c=np.array(c, f32)))
    same_runs(runs[0], runs[1], 'metrics values')
    ref, bound = G.metric_bounded_ref(inp.y, p10)
    r = G.bound_ratio(v[:5], ref, bound)
    within(r, 'metrics %dx%d %s v[0..4]' % (n, hw, form))
    print('METRICS worst so far per value: %s' % ' '.join('%.3g' % note('metrics v%d' % k, r[k]) for k in range(5)))
    assert c[3] == n * hw
    check_running(c, v, form)


def test_metrics_refusals():
    m = Metrics()
    y = In(np.ones(4, f32))
    for n, hw, ws_bytes, want in ((0, 4, m.ws.numel(), EINVAL), (1, 0, m.ws.numel(), EINVAL), (1, 4, m.ws.numel() - 1, EWORKSPACE)):
        assert status('tdg_cgan_metrics', y.ptr(), None, None, n, hw, K().ptr(m.counts), m.out.ptr(), K().ptr(m.ws), ws_bytes,
                      K().stream()) == want
    torch.cuda.synchronize()
    untouched(m.out)
    assert m.counts.cpu().tolist() == [0, 0, 0, 0, 77, 77, 77, 77]
