"""The kernels of csrc/tdg_isamp.hip against restatements.

tdg_isamp_prep and tdg_isamp_zero_fraction: bit for bit (bf16 stores against the round-to-nearest-even cast).
tdg_isamp_rmse_grad: bit for bit against the float32 restatement of the order include/tdg.h documents, and against float64 within
the bound tests/_exact_pointwise.py's operation-by-operation rule (class Ev) gives for that order.

tdg_isamp_head_bn_fwd / _bwd: the rule and the bounds tests/test_gpu_xsamp_kernels.py holds tdg_xsamp_head to -- g within TANH_ULP
f32 ulps of float64 tanh of an argument known exactly; dcat, dW, db within the roundings of their operations and gamma_N on the
sums -- with the terms batch norm adds, all from the oracle's own intermediates (no constant is fitted to a device result):

  forward.  z is exact in f32 in any order (head_inputs: integer data times a power of two), its f64 sums are exact, so
    mean and var are the oracle's up to f64 roundings (gamma_4 in 2**-53, carried).  The kernel stores mean and rstd rounded to
    f32: |mean32 - mean| <= u |mean|, |rstd32 - rstd| <= u rstd, u = 2**-24.  a = fl(z - mean32) is off by u |mean| + u |a|;
    zhat = fl(a rstd32) is off by rstd (u |mean| + u |a|) + |a| u rstd + u |zhat|: the argument of tanh is no longer exact,
    its error is the xsamp head's (zero) plus terms SCALED BY THE ORACLE'S rstd -- where batch norm divides, an absolute error
    of z grows by rstd.  Adding beta rounds once more; tanh moves an argument error e by at most the one-sided differences of
    tanh over [v - e, v + e] and adds TANH_ULP ulps (Ev.mono).  rstd <= 1 / sqrt(0.1 + eps) < 3.2 because every case has an
    oracle variance of z of at least 0.1 (asserted).
  backward.  From the GIVEN f32 g, zhat and rstd (the kernel reads what the forward pass stored): dy = dL/dg fl(1 - fl(g g)) as
    in the xsamp test; m1 = f32(sum dy / N), m2 = f32(sum dy zhat / N) from f64 sums of f32 terms (the terms' errors add,
    gamma_N in 2**-53 on the sums, one f32 rounding each); dz = fl(rstd fl(fl(dy - m1) - fl(zhat m2))): three more roundings,
    and every error that reaches the bracket is multiplied by rstd.  From dz on the bounds are the xsamp head's: two roundings
    and the store for dcat, gamma_N of the terms' magnitudes for dW and db.  dbeta = f32(sum dy).
"""
import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_cols as X
import _exact_pointwise as E
from test_gpu_xsamp_kernels import head_inputs, head_fwd as xsamp_head_fwd

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 77.0                       # representable in bf16
U32, U64 = 2.0 ** -24, 2.0 ** -53
TD = {0: torch.float32, 1: torch.bfloat16}
BN_EPS = 1e-3


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
def prep_ref(x, xl, yl, mv, y, xr, yr, T, off, P):
    """tdg_isamp_prep in NumPy float32: (X [n,S,S,P], target [n,T,T]); row-map entries outside [0, n) clamped into it."""
    n = x.shape[0]
    xr = np.arange(n) if xr is None else np.clip(np.asarray(xr), 0, n - 1)
    yr = np.arange(n) if yr is None else np.clip(np.asarray(yr), 0, n - 1)
    two, one = np.float32(2), np.float32(1)
    planes = [two * x[xr] - one] + ([xl[xr], yl[xr]] if P >= 5 else []) + ([mv[xr]] if P >= 6 else [])
    return np.concatenate(planes, axis=-1).astype(np.float32), (two * y[yr] - one)[:, off:off + T, off:off + T, 0].astype(np.float32)


GEOMS = [(3, 65, 31, 17, 3), (3, 64, 32, 16, 5), (3, 64, 32, 16, 6), (3, 7, 3, 2, 5)]
ROWMAPS = {'none': (None, None), 'zero': ([0, 0, 0], [0, 0, 0]), 'perm': ([2, 0, 1], None), 'outside': ([-1, 3, 1], [7, -5, 2 ** 31 - 1])}


def prep_data(n, S, P):
    rng = np.random.default_rng([n, S, P])
    x, xl, yl, mv, y = (rng.uniform(0, 1, (n, S, S, c)).astype(np.float32) for c in (3, 1, 1, 1, 1))
    return x, xl, yl, mv, y


def run_prep(entry, data, maps, n, S, T, off, P, strides, dt, g=True, r=True, dr=True, tg=True, with_y=True, m=None):
    gcs, rcs, dcs = strides
    gin, rin, dre = (torch.full((n * s * s * cs,), SENTINEL, dtype=TD[dt], device=DEV) for s, cs in ((S, gcs), (S, rcs), (T, dcs)))
    target = torch.full((n, T, T), SENTINEL, device=DEV)
    ptr = K().ptr
    d = [dev(a) for a in data]
    xr, yr = (None if v is None else dev(np.asarray(v, np.int64).astype(np.int32), torch.int32) for v in maps)
    tail = (ptr(gin) if g else None, gcs, ptr(rin) if r else None, rcs, ptr(dre) if dr and with_y else None, dcs,
            ptr(target) if tg and with_y else None, K().stream())
    if entry == 'tdg_isamp_prep':
        L().call(entry, dt, ptr(d[0]), ptr(d[1]) if P >= 5 else None, ptr(d[2]) if P >= 5 else None, ptr(d[3]) if P >= 6 else None,
                 ptr(d[4]) if with_y else None, ptr(xr), ptr(yr), n, S, T, off, P, *tail)
    else:
        L().call(entry, dt, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(dev(m)), ptr(d[4]) if with_y else None, ptr(xr), ptr(yr), n, S, T,
                 off, *tail)
    torch.cuda.synchronize()
    return (gin.float().cpu().numpy().reshape(n, S, S, gcs), rin.float().cpu().numpy().reshape(n, S, S, rcs),
            dre.float().cpu().numpy().reshape(n, T, T, dcs), target.cpu().numpy())


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('padded', [True, False])
@pytest.mark.parametrize('maps', list(ROWMAPS))
@pytest.mark.parametrize('n,S,T,off,P', GEOMS)
def test_prep(n, S, T, off, P, maps, padded, dt):
    """Every output against the restatement; channel P of the generator's input (the noise) and every padding channel untouched
    (a sentinel prefill); the engine's channel strides (8: the vector stores) and compact ones (P + 1, P, 1: single channels);
    then each output left out in turn, and the call without y."""
    data = prep_data(n, S, P)
    xr, yr = ROWMAPS[maps]
    strides = (8, 8, 8) if padded else (P + 1, P, 1)
    XP, tgt = prep_ref(*data, xr, yr, T, off, P)

    def check(out, g=True, r=True, dr=True, tg=True):
        gin, rin, dre, target = out
        for buf, on in ((gin, g), (rin, r)):
            assert np.array_equal(buf[..., :P], stored(XP, dt) if on else np.full_like(XP, SENTINEL))
            assert np.all(buf[..., P:] == SENTINEL)                      # the noise channel and the padding
        assert np.array_equal(dre[..., 0], stored(tgt, dt) if dr else np.full_like(tgt, SENTINEL)) and np.all(dre[..., 1:] == SENTINEL)
        assert np.array_equal(target, tgt if tg else np.full_like(tgt, SENTINEL))

    run = lambda **kw: run_prep('tdg_isamp_prep', data, (xr, yr), n, S, T, off, P, strides, dt, **kw)
    check(run())
    if maps in ('none', 'outside'):
        for off_out in ('g', 'r', 'dr', 'tg'):
            check(run(**{off_out: False}), **{off_out: False})
        check(run(with_y=False), dr=False, tg=False)
    if maps == 'zero':
        assert np.array_equal(XP[0], XP[2]) and np.array_equal(tgt[0], tgt[1])
    if maps == 'perm':
        assert not np.array_equal(XP[0], XP[1]) and np.array_equal(XP[1, ..., :3], np.float32(2) * data[0][0] - np.float32(1))
    if maps == 'outside':                                                # -1 -> row 0, 3 -> row 2; 7, 2**31 - 1 -> row 2, -5 -> row 0
        assert np.array_equal(XP[0], prep_ref(*data, [0, 2, 1], None, T, off, P)[0][0])
        assert np.array_equal(tgt, prep_ref(*data, None, [2, 0, 2], T, off, P)[1])


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('maps', ['none', 'zero', 'perm'])
def test_prep_with_a_constant_mean_plane_is_xsamp_prep(maps, dt):
    """P = 6 and mean_vec[b, :, :] == m[b]: every written bit is tdg_xsamp_prep's."""
    n, S, T, off = 3, 64, 32, 16
    x, xl, yl, _, y = prep_data(n, S, 6)
    m = np.random.default_rng(5).uniform(0, 1, n).astype(np.float32)
    mv = np.broadcast_to(m.reshape(n, 1, 1, 1), (n, S, S, 1)).copy()
    for strides in ((8, 8, 8), (7, 6, 1)):
        a = run_prep('tdg_isamp_prep', (x, xl, yl, mv, y), ROWMAPS[maps], n, S, T, off, 6, strides, dt)
        b = run_prep('tdg_xsamp_prep', (x, xl, yl, mv, y), ROWMAPS[maps], n, S, T, off, 6, strides, dt, m=m)
        assert all(np.array_equal(p, q) for p, q in zip(a, b)) and np.any(a[0][..., 5] != SENTINEL)


def test_prep_refuses_bad_arguments():
    t = torch.zeros(4096, device=DEV)
    P = K().ptr
    cases = [(6, 3, 4, 5, 8, 8), (6, 3, 2, 5, 5, 8), (6, 3, 2, 5, 8, 4), (6, 3, 2, 4, 8, 8), (6, 3, 2, 7, 8, 8)]     # (S, T, off, planes, g_cs, rgb_cs)
    for S, T, off, planes, gcs, rcs in cases:
        with pytest.raises(L().TdgError, match='tdg_isamp_prep'):
            L().call('tdg_isamp_prep', 0, P(t), P(t), P(t), P(t), None, None, None, 1, S, T, off, planes, P(t), gcs, P(t), rcs, None, 0,
                     None, K().stream())
    for missing in (1, 2, 3):                                            # x_loc, y_loc for P >= 5; mean_vec for P = 6
        a = [P(t)] * 4
        a[missing] = None
        with pytest.raises(L().TdgError, match='tdg_isamp_prep'):
            L().call('tdg_isamp_prep', 0, *a, None, None, None, 1, 6, 3, 2, 6, P(t), 8, None, 0, None, 0, None, K().stream())
    with pytest.raises(L().TdgError, match='tdg_isamp_prep'):             # a depth output without y
        L().call('tdg_isamp_prep', 0, P(t), None, None, None, None, None, None, 1, 6, 3, 2, 3, P(t), 8, None, 0, None, 0, P(t), K().stream())


# ------------------------------------------------------------------------------------------------ A1's head
def bn_fwd(cat, w, b, beta, dt, cs=None, eps=BN_EPS):
    n, hw, _, cin = cat.shape
    c = K().Act(n, hw, hw, cin, dt, DEV, cs=cs)
    full = np.full((n, hw, hw, c.cs), SENTINEL, np.float32)              # behind cin: channels the kernel must not read into its sums
    full[..., :cin] = cat
    c.buf.copy_(torch.as_tensor(full.reshape(-1)).to(DEV, TD[dt]))
    g, zhat = torch.full((n, hw, hw), SENTINEL, device=DEV), torch.full((n, hw, hw), SENTINEL, device=DEV)
    stats = torch.full((2,), SENTINEL, device=DEV)
    fake = K().Act(n, hw, hw, 1, dt, DEV)
    ws = torch.zeros(L().load().tdg_isamp_head_bn_workspace_bytes(n, cin), dtype=torch.uint8, device=DEV)
    wd, bd, be = dev(w), dev(b), dev(np.array([beta], np.float32))
    L().call('tdg_isamp_head_bn_fwd', dt, c.ptr(), n, hw, cin, c.cs, K().ptr(wd), K().ptr(bd), K().ptr(be), eps, K().ptr(g), K().ptr(zhat),
             K().ptr(stats), fake.ptr(), fake.cs, K().ptr(ws), ws.numel(), K().stream())
    torch.cuda.synchronize()
    return g.cpu().numpy(), zhat.cpu().numpy(), stats.cpu().numpy(), fake.buf.float().cpu().numpy().reshape(n, hw, hw, fake.cs), c


def bn_fwd_oracle(z, beta, eps=BN_EPS):
    """(mean, var, rstd, zhat as Ev, g as Ev) in float64 from the exact z, following the kernel's operations (docstring above)."""
    z = z.astype(np.float64)
    mean, var = z.mean(), z.var()
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    f64 = 4 * U64                                                         # the f64 roundings of mean, var, sqrt and the division
    mean32 = E.Ev(mean, (U32 + f64) * abs(mean))
    rstd32 = E.Ev(rstd, (U32 + f64 * (1 + (z * z).mean() / max(var, 1e-300))) * rstd)      # var = E[z^2] - mean^2 cancels in f64
    zhat = E.mul(E.sub(E.Ev(z), mean32), rstd32)
    return mean, var, rstd, zhat, E.ev_tanh(E.add(zhat, float(np.float32(beta))))


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('scale,beta', [(1.0, 0.0), (2.0 ** -4, 0.375)])
@pytest.mark.parametrize('hw', [5, 31])
def test_head_bn_forward(hw, scale, beta, wide, dt):
    """n = 3, cin = 128, cs = cin and cs > cin (the channels behind cin hold a sentinel the sums must not see): statistics, zhat
    and g within the derived bounds, the dtype store the f32 g rounded, two launches bit-equal."""
    n, cin = 3, 128
    cat, w, b = head_inputs(n, hw, cin, dt, scale)
    z = cat.astype(np.float64) @ w.astype(np.float64) + float(b[0])
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.abs(z).max() / scale < 2 ** 24
    mean, var, rstd, zhat, g_ev = bn_fwd_oracle(z, beta)
    assert var >= 0.1, 'the oracle variance of z is %g' % var
    cs = cin + 8 if wide else None
    g, zh, stats, fake, _ = bn_fwd(cat, w, b, beta, dt, cs)
    again = bn_fwd(cat, w, b, beta, dt, cs)
    assert all(np.array_equal(a, c) for a, c in zip((g, zh, stats, fake), again[:4]))            # two launches bit-equal
    assert abs(stats[0] - mean) <= 2 * U32 * abs(mean) and abs(stats[1] - rstd) <= 2 * U32 * rstd
    assert np.all(np.abs(zh - zhat.v) <= zhat.e), np.max(np.abs(zh - zhat.v) / zhat.e)
    assert np.all(np.isfinite(g)) and np.all(np.abs(g - g_ev.v) <= g_ev.e), np.max(np.abs(g - g_ev.v) / g_ev.e)
    assert np.max(g_ev.e / np.maximum(np.abs(g_ev.v), 1e-3)) < 1e-4                               # the bound is no blanket
    assert np.array_equal(fake[..., 0], stored(g, dt)) and np.all(fake[..., 1:] == 0)
    assert abs(zh.astype(np.float64).mean()) < 1e-5 and abs(zh.astype(np.float64).var() * (var + 1e-3) / var - 1) < 1e-4


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('hw', [5, 31])
def test_head_bn_forward_on_normalised_z_is_the_xsamp_head(hw, dt):
    """beta = 0 and z already normalised -- z in {0, +a, -a} with one 0 and as many +a as -a, so the mean is exactly 0, and a
    chosen so that var + eps is 1 to f32 rounding: zhat is z up to |z| |rstd - 1| and g matches tdg_xsamp_head_fwd's within the
    two kernels' bounds against float64 tanh plus the oracle's own |tanh(zhat) - tanh(z)|."""
    n, cin = 3, 128
    N = n * hw * hw
    a = np.float32(np.sqrt((1.0 - float(np.float32(BN_EPS))) * N / (N - 1)))
    sign = np.zeros(N, np.float32)
    sign[1:] = np.tile(np.float32([1, -1]), (N - 1) // 2)
    np.random.default_rng(hw).shuffle(sign)
    cat = np.random.default_rng(hw + 1).integers(-1, 2, (n, hw, hw, cin)).astype(np.float32)
    cat[..., 0] = sign.reshape(n, hw, hw)
    w = np.zeros(cin, np.float32)
    w[0] = a
    b = np.zeros(1, np.float32)
    z = sign.reshape(n, hw, hw).astype(np.float64) * float(a)
    mean, var, rstd, zhat, g_ev = bn_fwd_oracle(z, 0.0)
    assert mean == 0.0 and var >= 0.1 and abs(rstd - 1.0) < 2 * U32
    g, zh, stats, _, _ = bn_fwd(cat, w, b, 0.0, dt)
    gx, _ = xsamp_head_fwd(cat, w, b, dt)
    assert stats[0] == 0.0
    shift = np.abs(g_ev.v - np.tanh(z))
    assert shift.max() < 1e-6
    bound = g_ev.e + X.TANH_ULP * 2.0 ** -23 * np.abs(np.tanh(z)) + shift
    assert np.all(np.abs(g.astype(np.float64) - gx) <= bound) and np.all(np.abs(g - g_ev.v) <= g_ev.e)
    assert np.array_equal(g[sign.reshape(n, hw, hw) == 0], np.zeros(1, np.float32))


def bn_bwd(d, g, zhat, stats, cat, w, mode, leak, dt, cs=None):
    n, hw, _, cin = cat.shape
    c = K().Act(n, hw, hw, cin, dt, DEV, cs=cs)
    full = np.zeros((n, hw, hw, c.cs), np.float32)
    full[..., :cin] = cat
    c.buf.copy_(torch.as_tensor(full.reshape(-1)).to(DEV, TD[dt]))
    dfake = K().Act(n, hw, hw, 1, dt, DEV).set(d.reshape(n, hw, hw, 1))
    dcat = K().Act(n, hw, hw, cin, dt, DEV, cs=cs)
    dcat.buf.fill_(SENTINEL)
    dw, db, dbeta = (torch.full((k,), SENTINEL, device=DEV) for k in (cin, 1, 1))
    ws = torch.zeros(L().load().tdg_isamp_head_bn_workspace_bytes(n, cin), dtype=torch.uint8, device=DEV)
    wd, gd, zd, sd = dev(w), dev(g), dev(zhat), dev(stats)
    L().call('tdg_isamp_head_bn_bwd', dt, dfake.ptr(), dfake.cs, K().ptr(gd), K().ptr(zd), K().ptr(sd), c.ptr(), n, hw, cin, c.cs,
             K().ptr(wd), mode, leak, dcat.ptr(), K().ptr(dw), K().ptr(db), K().ptr(dbeta), K().ptr(ws), ws.numel(), K().stream())
    torch.cuda.synchronize()
    full = dcat.buf.float().cpu().numpy().reshape(n, hw, hw, dcat.cs)
    return full[..., :cin], dw.cpu().numpy(), db.cpu().numpy(), dbeta.cpu().numpy(), full[..., cin:]


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('mode', ['lrelu', 'none'])
@pytest.mark.parametrize('hw', [5, 31])
def test_head_bn_backward_bounds(hw, mode, wide, dt):
    """n = 3, cin = 128.  g, zhat and the statistics are the forward kernel's own outputs on head_inputs at scale 2**-4 (variance
    of z >= 0.1 asserted); dL/dg multiples of 1/8 (exact in bf16), cat in {-1, 0, 1} (zeros sit on the mask's kink, whose
    convention is cat > 0).  Bounds: the docstring above."""
    n, cin, leak = 3, 128, 0.25
    cat, w, b = head_inputs(n, hw, cin, dt, 2.0 ** -4)
    z = cat.astype(np.float64) @ w.astype(np.float64) + float(b[0])
    assert z.var() >= 0.1
    g, zhat, stats, _, _ = bn_fwd(cat, w, b, 0.125, dt)
    rng = np.random.default_rng([3, hw])
    d = (rng.integers(-8, 9, (n, hw, hw)) / 8.0).astype(np.float32)
    mm = {'lrelu': K().MASK_LRELU, 'none': K().MASK_NONE}[mode]
    cs = cin + 8 if wide else None
    got = bn_bwd(d, g, zhat, stats, cat, w, mm, leak, dt, cs)
    again = bn_bwd(d, g, zhat, stats, cat, w, mm, leak, dt, cs)
    assert all(np.array_equal(p, q) for p, q in zip(got, again))                          # two launches bit-equal
    dcat, dw, db, dbeta, pad = got
    assert np.all(pad == SENTINEL)                                                       # nothing behind cin is written
    N = n * hw * hw
    rstd = float(stats[1])
    gE, zE = E.Ev(g), E.Ev(zhat)
    dy = E.mul(E.Ev(d), E.sub(1.0, E.mul(gE, gE)))
    gam64 = X.gamma(N + 2, U64)

    def mean32(t):                                                                        # f32(f64 sum / N) of f32 terms known to t.e
        s = t.v.sum()
        e = t.e.sum() + gam64 * (np.abs(t.v) + t.e).sum()
        return s, e, E.Ev(s / N, e / N + U32 * (abs(s) + e) / N)
    s1, e_s1, m1 = mean32(dy)
    _, _, m2 = mean32(E.Ev(dy.v * zE.v, dy.e * np.abs(zE.v)))
    dz = E.mul(rstd, E.sub(E.sub(dy, m1), E.mul(zE, m2)))
    assert abs(float(dbeta[0]) - s1) <= e_s1 + U32 * (abs(s1) + e_s1)
    c64, w64 = cat.astype(np.float64), w.astype(np.float64)
    mask = np.where(c64 > 0, 1.0, leak) if mode == 'lrelu' else np.ones_like(c64)
    want = dz.v[..., None] * w64 * mask
    e_in = dz.e[..., None] * np.abs(w64) * mask
    e = e_in + X.gamma(2, U32) * (np.abs(want) + e_in)
    assert np.all(np.abs(dcat.astype(np.float64) - want) <= X.store_bound(e, want, dt))
    gam = X.gamma(N, U32)
    t, e_t = dz.v[..., None] * c64, dz.e[..., None] * np.abs(c64)
    want_w, bound_w = t.sum((0, 1, 2)), e_t.sum((0, 1, 2)) + gam * (np.abs(t) + e_t).sum((0, 1, 2))
    assert np.all(np.abs(dw.astype(np.float64) - want_w) <= bound_w), np.max(np.abs(dw - want_w) / bound_w)
    want_b, bound_b = dz.v.sum(), dz.e.sum() + gam * (np.abs(dz.v) + dz.e).sum()
    assert abs(float(db[0]) - want_b) <= bound_b
    assert np.abs(want_w).max() > 10 * bound_w.max()                                      # the bound is no blanket
    assert abs(want_b) <= bound_b                       # batch norm's backward pass removes the mean: db vanishes to the bound


def test_head_bn_refuses_bad_arguments():
    t = torch.zeros(8192, device=DEV)
    P = K().ptr
    with pytest.raises(L().TdgError, match='cin'):
        L().call('tdg_isamp_head_bn_fwd', 0, P(t), 1, 2, 72, 72, P(t), P(t), P(t), 1e-3, P(t), P(t), P(t), P(t), 8, P(t), 4096, K().stream())
    with pytest.raises(L().TdgError, match='cs 68'):
        L().call('tdg_isamp_head_bn_fwd', 0, P(t), 1, 2, 64, 68, P(t), P(t), P(t), 1e-3, P(t), P(t), P(t), P(t), 8, P(t), 4096, K().stream())
    with pytest.raises(L().TdgError, match='workspace'):
        L().call('tdg_isamp_head_bn_fwd', 0, P(t), 4, 2, 64, 64, P(t), P(t), P(t), 1e-3, P(t), P(t), P(t), P(t), 8, P(t), 8, K().stream())
    with pytest.raises(L().TdgError, match='workspace'):
        L().call('tdg_isamp_head_bn_bwd', 0, P(t), 8, P(t), P(t), P(t), P(t), 1, 2, 64, 64, P(t), 0, 0.2, P(t), P(t), P(t), P(t), P(t), 16,
                 K().stream())
    assert L().load().tdg_isamp_head_bn_workspace_bytes(3, 128) == 3 * 16 + 3 * 129 * 4


# ------------------------------------------------------------------------------------------------ rmse gradient
@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('rows', [5, 3 * 31 * 31])
def test_rmse_grad(rows, dt):
    """g, y eighths in [-1, 1] and dL/dg multiples of 2**-6 (all bf16-representable: both dtypes read the same numbers); rmse the
    float32 of the tensors' own rmse.  Bit for bit against the float32 restatement of the order include/tdg.h documents
    (IEEE division, no fused multiply-add), and against float64 within the bound that order gives operation by operation."""
    rng = np.random.default_rng([rows, 9])
    cs, dgs = 8, 8
    g = (rng.integers(-8, 9, rows) / 8.0).astype(np.float32)
    y = (rng.integers(-8, 9, rows) / 8.0).astype(np.float32)
    y[0] = g[0]                                                          # a zero difference: no update there
    d0 = (rng.integers(-64, 65, rows) / 64.0).astype(np.float32)
    rmse64 = np.sqrt(np.mean(((g.astype(np.float64) + 1) / 2 - (y.astype(np.float64) + 1) / 2) ** 2))
    rmse = np.float32(rmse64)
    buf = K().Act(2 * rows, 1, 1, 1, dt, DEV, cs=cs)
    full = np.full((2 * rows, cs), SENTINEL, np.float32)
    full[:rows, 0], full[rows:, 0] = y, g
    buf.buf.copy_(torch.as_tensor(full.reshape(-1)).to(DEV, TD[dt]))
    dfake = K().Act(rows, 1, 1, 1, dt, DEV, cs=dgs)
    dfull = np.full((rows, dgs), SENTINEL, np.float32)
    dfull[:, 0] = d0
    dfake.buf.copy_(torch.as_tensor(dfull.reshape(-1)).to(DEV, TD[dt]))
    scal = dev(np.array([SENTINEL, rmse], np.float32))
    L().call('tdg_isamp_rmse_grad', dt, buf.ptr(rows), buf.ptr(0), rows, cs, K().ptr(scal, 4), dfake.ptr(), dgs, K().stream())
    torch.cuda.synchronize()
    out = dfake.buf.float().cpu().numpy().reshape(rows, dgs)
    assert np.all(out[:, 1:] == SENTINEL) and np.array_equal(buf.buf.float().cpu().numpy().reshape(2 * rows, cs), stored(full, dt))
    f32 = np.float32
    k = f32(1) / f32(f32(f32(4) * f32(rows)) * rmse)
    want32 = stored(f32(d0 + f32(f32(g - y) * k)), dt)
    assert np.array_equal(out[:, 0], want32) and out[0, 0] == d0[0]
    kE = E.div(1.0, E.mul(E.mul(4.0, float(rows)), E.Ev(float(rmse))))
    ref, bound = E.stored(E.add(E.Ev(d0), E.mul(E.sub(E.Ev(g), E.Ev(y)), kE)), dt)
    assert np.all(np.abs(out[:, 0].astype(np.float64) - ref) <= bound)
    f32_bound = bound - (X.bf16_half_ulp(np.abs(ref) + bound) if dt == 1 else 0)            # the bound before the bf16 store
    assert np.abs(ref - d0).max() > 100 * f32_bound.max()                                  # the update is far above it: no blanket


def test_rmse_grad_at_zero_rmse_is_not_finite():
    """No guard at rmse == 0, as in TF: k is inf, a zero difference gives NaN and any other inf."""
    rows = 4
    buf = K().Act(2 * rows, 1, 1, 1, 0, DEV).set(np.array([0, 0, 0, 0, 0, 0.5, -0.5, 0], np.float32).reshape(8, 1, 1, 1))
    dfake = K().Act(rows, 1, 1, 1, 0, DEV)
    scal = dev(np.zeros(1, np.float32))
    L().call('tdg_isamp_rmse_grad', 0, buf.ptr(rows), buf.ptr(0), rows, buf.cs, K().ptr(scal), dfake.ptr(), dfake.cs, K().stream())
    out = dfake.get().ravel()
    assert np.isnan(out[0]) and out[1] == np.inf and out[2] == -np.inf and np.isnan(out[3])


# ------------------------------------------------------------------------------------------------ zero fraction
@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('rows,c', [(1, 8), (3, 1024)])
def test_zero_fraction(rows, c, wide, dt):
    """Planted zeros, -0.0 among them, among values that are not zero in either dtype (the smallest 2**-100); with cs > c the
    padding is zero and must not be counted.  Exact: f32(count / (rows c))."""
    rng = np.random.default_rng([rows, c])
    x = rng.choice(np.float32([1.0, -2.5, 2.0 ** -100, -2.0 ** -100, 3.0]), size=(rows, c)).astype(np.float32)
    zeros = rng.random((rows, c)) < 0.3
    zeros.reshape(-1)[:2] = True
    x[zeros] = 0.0
    neg = zeros & (rng.random((rows, c)) < 0.5)
    neg.reshape(-1)[1] = True
    x[neg] = -0.0
    assert np.signbit(x[neg]).all() and neg.sum() >= 1 and (zeros & ~neg).sum() >= 1
    cs = c + 8 if wide else c
    full = np.zeros((rows, cs), np.float32)
    full[:, :c] = x
    xd = torch.as_tensor(full.reshape(-1)).to(DEV, TD[dt])
    assert torch.equal(xd.float().cpu().reshape(rows, cs)[:, :c] == 0, torch.as_tensor(zeros))      # the cast keeps the pattern
    out = torch.full((3,), SENTINEL, device=DEV)
    ws = torch.zeros(L().load().tdg_isamp_zero_fraction_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for _ in range(2):
        L().call('tdg_isamp_zero_fraction', dt, K().ptr(xd), rows, c, cs, K().ptr(out, 4), K().ptr(ws), ws.numel(), K().stream())
        got = out.cpu().numpy()
        assert got[1] == np.float32(int(zeros.sum()) / (rows * c)) and got[0] == SENTINEL == got[2]
    xd.fill_(1.0)
    L().call('tdg_isamp_zero_fraction', dt, K().ptr(xd), rows, c, cs, K().ptr(out, 4), K().ptr(ws), ws.numel(), K().stream())
    assert out.cpu().numpy()[1] == 0.0
    with pytest.raises(L().TdgError, match='tdg_isamp_zero_fraction'):
        L().call('tdg_isamp_zero_fraction', dt, K().ptr(xd), rows, c, c - 1, K().ptr(out), K().ptr(ws), ws.numel(), K().stream())
