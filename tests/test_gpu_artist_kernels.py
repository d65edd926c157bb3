"""tdg_artist_mse (csrc/tdg_artist.hip) on the GPU, in both dtypes: the seed bit for bit against a NumPy float32 restatement of
the operation order include/tdg.h documents, the loss and its root against float64 within the bound tests/_exact_pointwise.py's
operation-by-operation rule (Ev) gives for that order, determinism, mode 0, the padding-channel rule (channels [c, cs) of the
seed are NEVER written), guarded surroundings, an unaligned target, a size past the cap on blocks and partials, and every
argument error.  Then the input cast artist uses, tdg_affine_cast_rows at (2, -0.5), bit for bit against fl(fl(2 x) - 1).

Inputs: the target is float32 of arbitrary bits in [0, 1], h is bf16-representable in (-1, 1) so that both dtypes read the same
numbers; h carries NaN in its padding channels and behind its rows (the kernel's 16-byte load brings padding in: none of it may
reach a result), the seed is prefilled with the sentinel.  Each bounded comparison prints its worst ratio (run with -s)."""
import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_pointwise as P
from test_gpu_pointwise_exact import Buf, K, call, dev, exact, fvec, nans, vget, within, DT, _release_inputs, _ALIVE      # noqa: F401
from test_host_artist import BAD, GOOD

pytestmark = pytest.mark.gpu

DTYPES = [0, 1]
TILE, CAP = 1024, 1024                               # include/tdg.h: 1024-pixel tiles, at most 1024 blocks = partials
PAST_CAP = TILE * CAP + 3 * TILE + 5                 # 1028 tiles: a second trip for four blocks, more than one partial per finish thread
SHAPES = [(1, 1, 8), (35, 3, 8), (3721, 3, 8), (3721, 1, 16), (PAST_CAP, 3, 8), (PAST_CAP, 1, 8)]
IDS = ['%dx%d/%d' % s for s in SHAPES]


def inputs(rows, c, seed=0):
    """(target f32 [rows, c] in [0, 1] with 0, 1 and the rescale's ties leading; h f32 [rows, c], bf16-representable in (-1, 1))."""
    rng = np.random.default_rng([31, rows, c, seed])
    t = rng.random((rows, c), dtype=np.float32)
    lead = np.float32([0.0, 1.0, 0.5, 0.25 - 2.0 ** -26, 2.0 ** -30, 1.0 - 2.0 ** -24])
    t.reshape(-1)[:min(t.size, lead.size)] = lead[:min(t.size, lead.size)]
    h = P.bf16_round((rng.random((rows, c), dtype=np.float32) * np.float32(1.98) - np.float32(0.99)))
    return t, h


def restate(t, h, dtype):
    """include/tdg.h's order in NumPy float32, one rounding per operation: (seed as stored, d)."""
    f = np.float32
    rows, c = t.shape
    tm = f(2) * t - f(1)
    t01 = (tm + f(1)) * f(0.5)
    h01 = (h + f(1)) * f(0.5)
    d = h01 - t01
    k = f(1) / f(float(rows * c))
    assert all(a.dtype == np.float32 for a in (tm, t01, h01, d)) and type(k) is np.float32
    return P.store((d * k).astype(np.float64), dtype), d


def loss_ref(t, h):
    """((mean, root), (their bounds)) in float64 on the bytes the kernel reads, by the Ev rule over the documented order; the sum
    of the exact squares is charged gamma(n, 2**-53) for an f64 sum of n terms in ANY order, the two stores half an f32 ulp."""
    n = t.size
    tm = P.sub(P.mul(2.0, P.Ev(t)), 1.0)
    t01 = P.mul(P.add(tm, 1.0), 0.5)
    h01 = P.mul(P.add(P.Ev(h), 1.0), 0.5)
    d = P.sub(h01, t01)
    sq_v, sq_e = d.v * d.v, 2.0 * np.abs(d.v) * d.e + d.e * d.e
    S = P.Ev(sq_v.sum(), sq_e.sum() + P.gamma(n, P.U64) * (sq_v + sq_e).sum())
    mean64 = P.Ev(S.v / n, S.e / n + 2.0 * P.U64 * S.v / n)
    mean = P.Ev(mean64.v, P._rounded(mean64.v, mean64.e))
    root = P.mono(mean64, np.sqrt, 0.5)
    root = P.Ev(root.v, root.e + 2.0 * P.U64 * root.v)
    return np.array([float(mean.v), float(root.v)]), np.array([float(mean.e), float(root.e)])


def workspace(nbytes=8192):
    t = torch.full((nbytes + 64,), 0x5a, dtype=torch.uint8, device=dev())
    _ALIVE.append(t)
    return t


def target_on_device(t, shift=0):
    """The compact target behind `shift` NaN floats (shift 1: a base that is 4- but not 16-byte aligned) and in front of NaN."""
    buf = torch.from_numpy(np.concatenate([nans(shift), t.ravel(), nans(16)])).to(dev())
    _ALIVE.append(buf)
    assert buf.data_ptr() % 16 == 0
    return K().ptr(buf, 4 * shift)


def launch(dtype, t, h, cs, shift=0, with_seed=True, off=0):
    rows, c = t.shape
    lay = P.Layout(rows, c, cs, off=off)
    hb, seed, scal, ws = Buf(lay, dtype, h), Buf(lay, dtype), fvec(nans(2)), workspace()
    call('tdg_artist_mse', dtype, target_on_device(t, shift), hb.ptr(), rows, c, cs, seed.ptr() if with_seed else None, K().ptr(scal),
         K().ptr(ws), 8192, K().stream())
    torch.cuda.synchronize()
    assert bool((ws[8192:] == 0x5a).all()), 'a write landed behind the workspace'
    hb.get()                                                        # h and its guards unchanged
    return seed.get(), vget(scal, 2), seed


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,c,cs', SHAPES, ids=IDS)
def test_seed_bit_for_bit_and_loss_within_its_bound(rows, c, cs, dtype):
    """Seed: np.array_equal with the restatement (bf16: its round-to-nearest-even cast).  seed.get() has already asserted that
    the padding channels, the band of rows behind and nothing else changed: the never-written rule against the sentinel."""
    t, h = inputs(rows, c)
    want_seed, d = restate(t, h, dtype)
    got_seed, scal, _ = launch(dtype, t, h, cs)
    what = '%s artist_mse %dx%d/%d' % (DT[dtype], rows, c, cs)
    exact(got_seed, want_seed, what + ' seed')
    ref, bound = loss_ref(t, h)
    within(P.bound_ratio(scal, ref, bound), what + ' loss, root')
    # the device's own d, summed in float64 in NumPy's order: the f32 results agree to the rounding of the store
    own = (d.astype(np.float64) ** 2).sum() / d.size
    assert np.all(np.abs(scal - np.array([own, np.sqrt(own)])) <= 2.0 ** -23 * np.array([own, np.sqrt(own)]))
    assert np.any(got_seed != 0) and (rows * c < 4 or np.any(got_seed > 0) and np.any(got_seed < 0))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,c,cs', [(35, 3, 8), (3721, 3, 8), (3721, 1, 16), (PAST_CAP, 3, 8)], ids=['35x3', '3721x3', '3721x1', 'past-cap'])
def test_unaligned_target_takes_the_4_byte_path_with_the_same_bits(rows, c, cs, dtype):
    """The target's base one float behind a 16-byte boundary: the same seed and the same two scalars, bit for bit, as from the
    aligned base (the sums meet in the same order either way)."""
    t, h = inputs(rows, c, seed=1)
    a_seed, a_scal, _ = launch(dtype, t, h, cs)
    b_seed, b_scal, _ = launch(dtype, t, h, cs, shift=1)
    exact(b_seed, restate(t, h, dtype)[0], 'unaligned seed')
    assert np.array_equal(a_seed, b_seed) and np.array_equal(a_scal, b_scal)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,c,cs', [(3721, 3, 8), (PAST_CAP, 1, 8)], ids=['3721x3', 'past-cap'])
def test_two_launches_are_bit_equal_and_mode_0_writes_no_seed(rows, c, cs, dtype):
    t, h = inputs(rows, c, seed=2)
    s1, scal1, _ = launch(dtype, t, h, cs)
    s2, scal2, _ = launch(dtype, t, h, cs)
    assert np.array_equal(s1, s2) and np.array_equal(scal1.view(np.uint32), scal2.view(np.uint32))
    s0, scal0, buf = launch(dtype, t, h, cs, with_seed=False)
    assert np.array_equal(scal0.view(np.uint32), scal1.view(np.uint32))
    assert bool((buf.t.float() == P.SENTINEL).all()) and np.all(s0 == P.SENTINEL)          # the sentinel-filled seed, untouched


@pytest.mark.parametrize('dtype', DTYPES)
def test_front_guard_and_every_channel_count(dtype):
    """c = 1..4 at cs = 8 and 16 behind eight guard elements (a 16-byte aligned base that is not the allocation's): each count's
    stores stay inside channels [0, c)."""
    for c in (1, 2, 3, 4):
        for cs in (8, 16):
            t, h = inputs(1500, c, seed=3)
            got, scal, _ = launch(dtype, t, h, cs, off=8)
            exact(got, restate(t, h, dtype)[0], 'c=%d cs=%d seed' % (c, cs))
            ref, bound = loss_ref(t, h)
            within(P.bound_ratio(scal, ref, bound), '%s artist_mse c=%d cs=%d loss, root' % (DT[dtype], c, cs))


@pytest.mark.parametrize('what,change,code', BAD, ids=[b[0] for b in BAD])
def test_argument_errors_launch_nothing(what, change, code):
    """On real buffers: the status, and afterwards the sentinel-filled seed, the scalars and the workspace are as they were."""
    rows, c, cs, dtype = GOOD['rows'], GOOD['c'], GOOD['cs'], GOOD['dtype']
    t, h = inputs(rows, c)
    lay = P.Layout(rows, c, cs, off=8)
    hb, seed, scal, ws = Buf(lay, dtype, h), Buf(lay, dtype), fvec(nans(2)), workspace()
    tbuf = torch.from_numpy(np.concatenate([nans(4), t.ravel(), nans(16)])).to(dev())
    real = dict(target=tbuf.data_ptr() + 16, h=hb.t.data_ptr() + 16, seed=seed.t.data_ptr() + 16, scal=scal.data_ptr(), ws=ws.data_ptr())
    a = dict(GOOD, **real)
    for k, v in change.items():                                     # the host table's offsets from its placeholder address, on the real one
        a[k] = (None if v is None else real[k] + (v - GOOD[k])) if k in real else v
    lib = pkg('_lib').load()
    rc = lib.tdg_artist_mse(a['dtype'], a['target'], a['h'], a['rows'], a['c'], a['cs'], a['seed'], a['scal'], a['ws'], a['ws_bytes'],
                            K().stream())
    torch.cuda.synchronize()
    assert rc == code, (what, rc, lib.tdg_last_error())
    assert bool((seed.t.float() == P.SENTINEL).all()) and bool(torch.isnan(scal[:2]).all()) and bool((ws == 0x5a).all())


# ------------------------------------------------------------------------------------------------ the input cast
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,side', [(2, 7), (2, 256)], ids=['2x7x7', '2x256x256'])
def test_input_cast_is_the_rescale_bit_for_bit(n, side, dtype):
    """tdg_affine_cast_rows at (2, -0.5) into channel stride 8: every stored value is fl(fl(2 x) - 1) (bf16: its nearest-even
    cast) on float32 x of arbitrary bits in [0, 1]; the padding channels and the surroundings keep the sentinel."""
    rows = n * side * side
    rng = np.random.default_rng([32, n, side])
    x = rng.integers(0, 0x3f800001, size=(rows, 3), dtype=np.uint32).view(np.float32)
    x.reshape(-1)[:5] = np.float32([0.0, 1.0, 0.25 - 2.0 ** -26, 2.0 ** -149, 0.5])
    out = Buf(P.Layout(rows, 3, 8, off=8), dtype)
    src = torch.from_numpy(np.concatenate([x.ravel(), nans(16)])).to(dev())
    call('tdg_affine_cast_rows', dtype, K().ptr(src), rows, 3, 8, 2.0, -0.5, out.ptr(), K().stream())
    want = np.float32(2) * x - np.float32(1)
    exact(out.get(), P.store(want.astype(np.float64), dtype), '%s input cast %d x %d x %d' % (DT[dtype], n, side, side))
