"""The three kernels of csrc/tdg_xsamp.hip against restatements: tdg_xsamp_prep bit for bit (bf16 stores against torch's
round-to-nearest-even cast), tdg_xsamp_head_fwd within TANH_ULP ulps of float64 tanh on inputs whose z is exact in f32, and
tdg_xsamp_head_bwd within bounds built from the oracle's own intermediates (the rounding of 1 - g g, of the products, and
gamma_n on the sums: no constant is fitted to a device result) -- and, at g == 0, bit-equal to tdg_cgan_head_bwd."""
import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_cols as X

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 77.0                       # representable in bf16
U32 = 2.0 ** -24
TD = {0: torch.float32, 1: torch.bfloat16}


def K():
    return pkg('kernels')


def L():
    return pkg('_lib')


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def stored(a, dt):
    """float32 values as the device stores them, as float32."""
    t = torch.as_tensor(np.asarray(a, np.float32))
    return (t.bfloat16().float() if dt == 1 else t).numpy()


# ------------------------------------------------------------------------------------------------ prep
def prep_ref(x, xl, yl, m, y, xr, yr, T, off):
    """tdg_xsamp_prep in NumPy float32: (X [n,S,S,6], target [n,T,T])."""
    n = x.shape[0]
    xr = np.arange(n) if xr is None else np.asarray(xr)
    yr = np.arange(n) if yr is None else np.asarray(yr)
    two, one = np.float32(2), np.float32(1)
    X6 = np.concatenate([two * x[xr] - one, xl[xr], yl[xr], np.broadcast_to(m[xr].reshape(n, 1, 1, 1), xl.shape)], axis=-1)
    return X6.astype(np.float32), (two * y[yr] - one)[:, off:off + T, off:off + T, 0].astype(np.float32)


PREP_CASES = [(3, 6, 3, 2, [2, 0, 2], [0, 0, 0]), (2, 64, 32, 16, None, None)]


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('padded', [True, False])
@pytest.mark.parametrize('n,S,T,off,xr,yr', PREP_CASES)
def test_prep(n, S, T, off, xr, yr, padded, dt):
    """Every output against the restatement, channel 6 of the generator's input and every padding channel untouched (a
    sentinel prefill), with the engine's channel strides (8: the vector stores) and with compact ones (7, 6, 1: the scalar
    path); then each output left out in turn."""
    rng = np.random.default_rng([n, S])
    x, xl, yl, y = (rng.uniform(0, 1, (n, S, S, c)).astype(np.float32) for c in (3, 1, 1, 1))
    m = rng.uniform(0, 1, n).astype(np.float32)
    gcs, rcs, dcs = (8, 8, 8) if padded else (7, 6, 1)
    X6, tgt = prep_ref(x, xl, yl, m, y, xr, yr, T, off)
    rows = lambda r: None if r is None else dev(np.asarray(r, np.int32), torch.int32)
    d = [dev(a) for a in (x, xl, yl, m, y)]
    xr_d, yr_d = rows(xr), rows(yr)

    def run(g=True, r=True, dr=True, tg=True, with_y=True):
        gin, rin, dre = (torch.full((n * s * s * cs,), SENTINEL, dtype=TD[dt], device=DEV) for s, cs in ((S, gcs), (S, rcs), (T, dcs)))
        target = torch.full((n, T, T), SENTINEL, device=DEV)
        P = K().ptr
        L().call('tdg_xsamp_prep', dt, P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[4]) if with_y else None, P(xr_d), P(yr_d), n, S, T, off,
                 P(gin) if g else None, gcs, P(rin) if r else None, rcs, P(dre) if dr and with_y else None, dcs,
                 P(target) if tg and with_y else None, K().stream())
        return (gin.float().cpu().numpy().reshape(n, S, S, gcs), rin.float().cpu().numpy().reshape(n, S, S, rcs),
                dre.float().cpu().numpy().reshape(n, T, T, dcs), target.cpu().numpy())

    def check(out, g=True, r=True, dr=True, tg=True):
        gin, rin, dre, target = out
        for buf, on in ((gin, g), (rin, r)):
            assert np.array_equal(buf[..., :6], stored(X6, dt) if on else np.full_like(X6, SENTINEL))
            assert np.all(buf[..., 6:] == SENTINEL)                      # the noise channel and the padding
        assert np.array_equal(dre[..., 0], stored(tgt, dt) if dr else np.full_like(tgt, SENTINEL)) and np.all(dre[..., 1:] == SENTINEL)
        assert np.array_equal(target, tgt if tg else np.full_like(tgt, SENTINEL))

    check(run())
    for off_out in ('g', 'r', 'dr', 'tg'):
        check(run(**{off_out: False}), **{off_out: False})
    check(run(with_y=False), dr=False, tg=False)
    if xr is not None:                                                   # the repeated row and the broadcast are real
        assert np.array_equal(X6[0], X6[2]) and not np.array_equal(X6[0], X6[1]) and np.array_equal(tgt[0], tgt[1])


def test_prep_refuses_bad_geometry():
    t = torch.zeros(64, device=DEV)
    P = K().ptr
    for S, T, off, gcs in ((6, 3, 4, 8), (6, 3, 2, 6)):                  # the crop leaves the window; no room for the noise channel
        with pytest.raises(L().TdgError):
            L().call('tdg_xsamp_prep', 0, P(t), P(t), P(t), P(t), None, None, None, 1, S, T, off, P(t), gcs, None, 0, None, 0, None,
                     K().stream())


# ------------------------------------------------------------------------------------------------ head
def head_inputs(n, hw, cin, dt, scale, seed=0):
    """cat in {-1, 0, 1}; w integers in [-2, 2] and b an integer, both times `scale` (a power of two): every product and every
    partial sum of z = w . cat + b is an integer multiple of `scale` below 2**24 * scale, so z is exact in f32 in any order."""
    rng = np.random.default_rng([seed, n, hw, cin])
    cat = rng.integers(-1, 2, (n, hw, hw, cin)).astype(np.float32)
    w = (rng.integers(-2, 3, cin) * scale).astype(np.float32)
    b = np.array([3 * scale], np.float32)
    return cat, w, b


def head_fwd(cat, w, b, dt):
    n, hw, _, cin = cat.shape
    c = K().Act(n, hw, hw, cin, dt, DEV).set(cat)
    g = torch.full((n, hw, hw), SENTINEL, device=DEV)
    fake = K().Act(n, hw, hw, 1, dt, DEV)
    wd, bd = dev(w), dev(b)
    L().call('tdg_xsamp_head_fwd', dt, c.ptr(), n, hw, cin, c.cs, K().ptr(wd), K().ptr(bd), K().ptr(g), fake.ptr(), fake.cs, K().stream())
    return g.cpu().numpy(), fake


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('scale', [1.0, 2.0 ** -4])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('hw', [3, 32])
@pytest.mark.parametrize('cin', [64, 128])
def test_head_forward(cin, hw, n, scale, dt):
    """g within TANH_ULP f32 ulps of float64 tanh(z), z exact; the dtype store is the f32 g rounded (store_bound on top of the
    tanh bound); the other channels of the fake depth input stay zero.  scale 1: integer w and b (|z| is mostly beyond tanh's
    bend); scale 2**-4: the same integers, z spread over the bend."""
    cat, w, b = head_inputs(n, hw, cin, dt, scale)
    z = cat.astype(np.float64) @ w.astype(np.float64) + float(b[0])
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.abs(z).max() / scale < 2 ** 24
    want = np.tanh(z)
    g, fake = head_fwd(cat, w, b, dt)
    assert np.all(np.isfinite(g)) and float(np.max(X.ulps(g, want))) <= X.TANH_ULP
    if scale < 1 and hw == 32:
        assert 0.05 < np.mean(np.abs(want) < 0.5) and np.abs(want).max() > 0.5            # the bend and the shoulders are both met
    f = fake.buf.float().cpu().numpy().reshape(n, hw, hw, fake.cs)
    assert np.array_equal(f[..., 0], stored(g, dt)) and np.all(f[..., 1:] == 0)
    e = X.TANH_ULP * 2.0 ** -23 * np.abs(want)
    assert np.all(np.abs(f[..., 0].astype(np.float64) - want) <= X.store_bound(e, want, dt))


@pytest.mark.parametrize('dt', [0, 1])
def test_head_forward_of_zero_is_zero(dt):
    cat, w, b = head_inputs(3, 5, 64, dt, 1.0)
    g, fake = head_fwd(cat, 0 * w, 0 * b, dt)
    assert np.all(g == 0) and np.all(fake.buf.float().cpu().numpy() == 0)


def head_bwd(d, g, cat, w, mode, leak, dt, entry='tdg_xsamp_head_bwd'):
    n, hw, _, cin = cat.shape
    c = K().Act(n, hw, hw, cin, dt, DEV).set(cat)
    dfake = K().Act(n, hw, hw, 1, dt, DEV).set(d.reshape(n, hw, hw, 1))
    dcat = K().Act(n, hw, hw, cin, dt, DEV).set(np.full((n, hw, hw, cin), SENTINEL, np.float32))
    dw, db = torch.full((cin,), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)
    ws = torch.zeros(n * (cin + 1), device=DEV)
    wd, gd = dev(w), dev(g) if g is not None else None
    if entry == 'tdg_xsamp_head_bwd':
        L().call(entry, dt, dfake.ptr(), dfake.cs, K().ptr(gd), c.ptr(), n, hw, cin, c.cs, K().ptr(wd), mode, leak, dcat.ptr(),
                 K().ptr(dw), K().ptr(db), K().ptr(ws), ws.numel() * 4, K().stream())
    else:
        L().call(entry, dt, dfake.ptr(), dfake.cs, c.ptr(), n, hw, cin, c.cs, hw, K().ptr(wd), mode, leak, dcat.ptr(),
                 K().ptr(dw), K().ptr(db), K().ptr(ws), ws.numel() * 4, K().stream())
    return dcat.get(), dw.cpu().numpy(), db.cpu().numpy()


def bwd_inputs(n, hw, cin, seed=1):
    """dL/dg multiples of 1/8 in [-1, 1] (exact in bf16), cat in {-1, 0, 1} (zeros sit on the mask's kink, whose convention is
    cat > 0), w integers in [-2, 2], g = f32(tanh) of values over the bend."""
    rng = np.random.default_rng([seed, n, hw, cin])
    d = (rng.integers(-8, 9, (n, hw, hw)) / 8.0).astype(np.float32)
    cat = rng.integers(-1, 2, (n, hw, hw, cin)).astype(np.float32)
    w = rng.integers(-2, 3, cin).astype(np.float32)
    g = np.tanh(rng.uniform(-2.5, 2.5, (n, hw, hw))).astype(np.float32)
    return d, cat, w, g


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('mode', ['lrelu', 'none'])
@pytest.mark.parametrize('n,hw,cin', [(1, 3, 64), (3, 3, 128), (3, 32, 128), (1, 32, 64)])
def test_head_backward_bounds(n, hw, cin, mode, dt):
    """dz = dL/dg * fl(1 - fl(g g)) from the GIVEN f32 g (the kernel reads the stored g: no tanh is evaluated, so the tanh term of
    the bound is zero here and the factor's two roundings remain), dcat = dz w mask with two more roundings and the store,
    dw and db sums of N = n hw hw inexact terms accumulated in f32 in some order: gamma_N of the terms' magnitudes."""
    leak = 0.25
    d, cat, w, g = bwd_inputs(n, hw, cin)
    mm = {'lrelu': K().MASK_LRELU, 'none': K().MASK_NONE}[mode]
    dcat, dw, db = head_bwd(d, g, cat, w, mm, leak, dt)
    again = head_bwd(d, g, cat, w, mm, leak, dt)
    assert all(np.array_equal(a, b) for a, b in zip((dcat, dw, db), again))               # two launches bit-equal
    d64, g64, c64, w64 = (a.astype(np.float64) for a in (d, g, cat, w))
    gg = g64 * g64
    F = 1.0 - gg
    e_f = U32 * gg + U32 * (np.abs(F) + U32 * gg)                                          # fl(g g), then fl(1 - .)
    dz = d64 * F
    e_dz = np.abs(d64) * e_f + U32 * (np.abs(dz) + np.abs(d64) * e_f)
    mask = np.where(c64 > 0, 1.0, leak) if mode == 'lrelu' else np.ones_like(c64)
    want = dz[..., None] * w64 * mask
    e_in = e_dz[..., None] * np.abs(w64) * mask
    e = e_in + X.gamma(2, U32) * (np.abs(want) + e_in)
    assert np.all(np.abs(dcat.astype(np.float64) - want) <= X.store_bound(e, want, dt))
    N = n * hw * hw
    gam = X.gamma(N, U32)
    t = dz[..., None] * c64
    e_t = e_dz[..., None] * np.abs(c64)
    want_w, bound_w = t.sum((0, 1, 2)), e_t.sum((0, 1, 2)) + gam * (np.abs(t) + e_t).sum((0, 1, 2))
    assert np.all(np.abs(dw.astype(np.float64) - want_w) <= bound_w), np.max(np.abs(dw - want_w) / bound_w)
    want_b, bound_b = dz.sum(), e_dz.sum() + gam * (np.abs(dz) + e_dz).sum()
    assert abs(float(db[0]) - want_b) <= bound_b
    assert np.abs(want_w).max() > 10 * bound_w.max() or N < 100                          # the bound is no blanket


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('mode', ['lrelu', 'none'])
@pytest.mark.parametrize('n,hw,cin', [(3, 3, 128), (2, 32, 64)])
def test_head_backward_at_zero_g_is_the_cgan_head(n, hw, cin, mode, dt):
    """g == 0: the factor is exactly 1, and dcat, dw, db are tdg_cgan_head_bwd's at crop == hw bit for bit."""
    rng = np.random.default_rng([2, n, hw, cin])
    d = stored(rng.uniform(-1, 1, (n, hw, hw)).astype(np.float32), dt)
    cat = stored(rng.uniform(-1, 1, (n, hw, hw, cin)).astype(np.float32), dt)
    w = rng.uniform(-1, 1, cin).astype(np.float32)
    mm = {'lrelu': K().MASK_LRELU, 'none': K().MASK_NONE}[mode]
    a = head_bwd(d, np.zeros_like(d), cat, w, mm, 0.2, dt)
    b = head_bwd(d, None, cat, w, mm, 0.2, dt, entry='tdg_cgan_head_bwd')
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.any(a[1] != 0) and not np.any(a[0] == SENTINEL)


def test_head_refuses_bad_arguments():
    t = torch.zeros(4096, device=DEV)
    P = K().ptr
    with pytest.raises(L().TdgError, match='cin'):
        L().call('tdg_xsamp_head_fwd', 0, P(t), 1, 2, 72, 72, P(t), P(t), P(t), P(t), 8, K().stream())
    with pytest.raises(L().TdgError, match='workspace'):
        L().call('tdg_xsamp_head_bwd', 0, P(t), 8, P(t), P(t), 1, 2, 64, 64, P(t), 0, 0.2, P(t), P(t), P(t), P(t), 16, K().stream())
