"""The new kernels behind paper_sampler on the GPU: tdg_cgan_sample_stats and the head with a noise term against float64
NumPy, and the conv geometries the noise windows add -- through the U-Net executor's own descriptors -- bit for bit against
the integer-valued oracle of tests/_exact_conv.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_conv as X
import _sampler_ref as R
from test_gpu_paper_cgan import close, dev, rnd, TOL, DEV

pytestmark = pytest.mark.gpu


def K():
    return pkg('kernels')


def L():
    return pkg('_lib')


# ------------------------------------------------------------------------------------------------ tdg_cgan_sample_stats
# relative, per value: the f64 sums contribute about n * 2**-53, the final cast 2**-24, x4 for the unit scaling
STATS_BOUND = 2.0 ** -22


def run_stats(y, g, pred, off, image, images=False):
    n, hw = y.shape
    out = torch.full((6,), 7.0, device=DEV)
    mean, var = (torch.full((hw,), 7.0, device=DEV), torch.full((hw,), 7.0, device=DEV)) if images else (None, None)
    ws = torch.zeros(L().load().tdg_cgan_sample_stats_workspace_bytes(n, hw), dtype=torch.uint8, device=DEV)
    p = lambda a: K().ptr(dev(a) if a is not None else None)
    L().call('tdg_cgan_sample_stats', p(y), p(g), p(pred), p(off), p(image), 10.0, n, hw, 10.0, K().ptr(out), K().ptr(mean),
             K().ptr(var), K().ptr(ws), ws.numel(), K().stream())
    return out.cpu().numpy(), (mean.cpu().numpy(), var.cpu().numpy()) if images else None


def stats_case(n, hw, form, seed=0):
    """y, g, the prediction in `form` and y_hat as the kernel rounds it (f32); image n // 2 has the smallest error."""
    rng = np.random.default_rng([seed, n, hw])
    f = np.float32
    pred = rng.uniform(1, 9, (n, hw)).astype(f) if form == 'pred+offset' else None
    off = rng.uniform(0.5, 1.5, n).astype(f) if form in ('pred+offset', 'offset') else None
    image = rng.uniform(0.1, 0.9, hw).astype(f) if form == 'image' else None
    if form == 'image':
        yhat = np.broadcast_to(image * f(10.0), (n, hw)).astype(f)
    else:
        yhat = ((pred if pred is not None else np.zeros((n, hw), f)) + off[:, None]).astype(f)
    amp = (0.05 + 0.3 * np.abs(np.arange(n) - n // 2)).astype(f)
    y = (yhat + amp[:, None] * rng.standard_normal((n, hw)).astype(f)).astype(f)
    g = rng.standard_normal((n, hw)).astype(f)
    return y, g, pred, off, image, yhat


def within(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    assert np.all(err <= STATS_BOUND * np.abs(ref)), '%s: got %r, float64 %r, relative %r' % (what, got, ref, err / np.abs(ref))


@pytest.mark.parametrize('form', ['pred+offset', 'offset', 'image'])
@pytest.mark.parametrize('n,hw', [(5, 841), (13, 841), (13, 70)])
def test_sample_stats_against_float64(n, hw, form):
    y, g, pred, off, image, yhat = stats_case(n, hw, form)
    per_image = np.mean(np.abs(y.astype(np.float64) - yhat), axis=1)
    assert 0 < int(np.argmin(per_image)) < n - 1                 # the minimum sits at an interior image
    got, (mean, var) = run_stats(y, g, pred, off, image, images=True)
    ref = R.sample_stats(y, g, yhat)
    print('sample_stats n %d hw %d %s: got %r float64 %r' % (n, hw, form, got, ref))
    if form == 'image':                                          # every image predicts the same: no variance, exactly
        assert got[5] == 0.0 and np.all(var == 0.0)
        within(np.delete(got, 5), np.delete(ref, 5), 'stats')
    else:
        within(got, ref, 'stats')
        within(var, yhat.astype(np.float64).var(axis=0) / 100.0, 'variance image')
    within(mean, yhat.astype(np.float64).mean(axis=0) / 10.0, 'mean image')
    again, _ = run_stats(y, g, pred, off, image, images=True)
    assert np.array_equal(got, again)                            # fixed-order reductions: two launches are bit-equal
    no_images, _ = run_stats(y, g, pred, off, image)
    assert np.array_equal(got, no_images)


def test_sample_stats_null_g_and_identical_rows_are_exact():
    y, g, pred, off, image, yhat = stats_case(13, 841, 'pred+offset', seed=1)
    got, _ = run_stats(y, None, pred, off, None)
    assert got[2] == 0.0 and got[3] == 0.0                       # g null: exactly 0 moments
    within(got[[0, 1, 4, 5]], R.sample_stats(y, g, yhat)[[0, 1, 4, 5]], 'stats without g')
    g1, p1 = np.repeat(g[3:4], 13, axis=0), np.repeat(pred[3:4], 13, axis=0)
    o1 = np.full(13, off[3], np.float32)
    got, (mean, var) = run_stats(y, g1, p1, o1, None, images=True)
    assert got[3] == 0.0 and got[5] == 0.0 and np.all(var == 0.0)          # n identical rows: a variance of exactly 0
    within(got[[0, 1, 2, 4]], R.sample_stats(y, g1, (p1 + o1[:, None]).astype(np.float32))[[0, 1, 2, 4]], 'identical rows')


def test_sample_stats_rejects_a_small_workspace_and_mixed_forms():
    y = np.ones((4, 70), np.float32)
    out, ws = torch.zeros(6, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV)
    with pytest.raises(L().TdgError, match='workspace'):
        L().call('tdg_cgan_sample_stats', K().ptr(dev(y)), None, K().ptr(dev(y)), None, None, 10.0, 4, 70, 10.0, K().ptr(out), None, None,
                 K().ptr(ws), ws.numel(), K().stream())
    big = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(L().TdgError, match='bad argument'):
        L().call('tdg_cgan_sample_stats', K().ptr(dev(y)), None, K().ptr(dev(y)), None, K().ptr(dev(y[0])), 10.0, 4, 70, 10.0, K().ptr(out),
                 None, None, K().ptr(big), big.numel(), K().stream())


# ------------------------------------------------------------------------------------------------ the head with a noise term
def head_buffers(dt, B, C):
    cat = K().Act(B, 31, 31, C, dt, DEV).set(rnd(dt, B, 31, 31, C, seed=2))
    dfake = K().Act(B, 29, 29, 1, dt, DEV).set(rnd(dt, B, 29, 29, 1, seed=4))
    return cat, dfake


def head_fwd(dt, cat, w, b, u, ybar, noise_entry=True):
    B, C = cat.n, cat.c
    yhat, g32 = torch.zeros(B, 29, 29, device=DEV), torch.zeros(B, 29, 29, device=DEV)
    fake = K().Act(B, 29, 29, 1, dt, DEV)
    if noise_entry:
        L().call('tdg_cgan_head_noise_fwd', dt, cat.ptr(), B, 31, C, cat.cs, 29, K().ptr(dev(w)), K().ptr(dev(b)),
                 K().ptr(dev(u) if u is not None else None), K().ptr(dev(ybar)), K().ptr(yhat), K().ptr(g32), fake.ptr(), fake.cs,
                 K().stream())
    else:
        L().call('tdg_cgan_head_fwd', dt, cat.ptr(), B, 31, C, cat.cs, 29, K().ptr(dev(w)), K().ptr(dev(b)), K().ptr(dev(ybar)),
                 K().ptr(yhat), fake.ptr(), fake.cs, K().stream())
    return yhat.cpu().numpy(), g32.cpu().numpy(), fake.get()[..., 0]


def head_bwd(dt, cat, dfake, w, u, noise_entry=True):
    B, C = cat.n, cat.c
    cols = C + (1 if u is not None else 0)
    dcat = K().Act(B, 31, 31, C, dt, DEV).set(np.full((B, 31, 31, C), 7.0, np.float32))      # must be overwritten everywhere
    dw, db = torch.full((cols,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    ws = torch.zeros(B * (cols + 1), device=DEV)
    if noise_entry:
        L().call('tdg_cgan_head_noise_bwd', dt, dfake.ptr(), dfake.cs, cat.ptr(), B, 31, C, cat.cs, 29, K().ptr(dev(w)),
                 K().ptr(dev(u) if u is not None else None), K().MASK_LRELU, 0.2, dcat.ptr(), K().ptr(dw), K().ptr(db), K().ptr(ws),
                 ws.numel() * 4, K().stream())
    else:
        L().call('tdg_cgan_head_bwd', dt, dfake.ptr(), dfake.cs, cat.ptr(), B, 31, C, cat.cs, 29, K().ptr(dev(w)), K().MASK_LRELU, 0.2,
                 dcat.ptr(), K().ptr(dw), K().ptr(db), K().ptr(ws), ws.numel() * 4, K().stream())
    return dcat.get(), dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize('dt', [0, 1])
def test_head_with_noise_forward_and_backward(dt):
    """The bounds per dtype of test_gpu_paper_cgan.test_head_forward_and_backward."""
    B, C = 3, 128
    cat, dfake = head_buffers(dt, B, C)
    catv = cat.get().astype(np.float64)
    w, b = rnd(0, C + 1, seed=3), np.array([0.3], np.float32)
    u = np.random.default_rng(5).uniform(0, 1, (B, 31, 31)).astype(np.float32)
    ybar = np.array([1.0, 2.0, 3.0], np.float32)
    yhat, g32, fake = head_fwd(dt, cat, w, b, u, ybar)
    g = (catv @ w[:C].astype(np.float64) + w[C].astype(np.float64) * u + b[0])[:, :29, :29]
    close(yhat, g + ybar[:, None, None], 1e-5, 'y_hat')
    close(g32, g, 1e-5, 'g (f32)')
    close(fake, g, TOL[dt], 'fake depth channel')
    assert np.max(np.abs(g - (catv @ w[:C].astype(np.float64) + b[0])[:, :29, :29])) > 0.1      # the noise term matters
    dcat, dw, db = head_bwd(dt, cat, dfake, w, u)
    delta = dfake.get()[..., 0].astype(np.float64)
    full = np.zeros((B, 31, 31))
    full[:, :29, :29] = delta
    ref = full[..., None] * w[None, None, None, :C] * np.where(catv > 0, 1.0, 0.2)
    close(dcat, ref, TOL[dt], 'dcat')
    assert np.all(dcat[:, 29:, :, :] == 0) and np.all(dcat[:, :, 29:, :] == 0)
    close(dw[:C], np.einsum('bhw,bhwc->c', full, catv), TOL[dt] * 10, 'dW')
    close(dw[C:], [np.sum(full * u)], TOL[dt] * 10, 'dW of the noise channel')
    close(db, [full.sum()], TOL[dt] * 10, 'db')


@pytest.mark.parametrize('dt', [0, 1])
def test_head_with_zero_noise_is_the_plain_head_bit_for_bit(dt):
    B, C = 3, 128
    cat, dfake = head_buffers(dt, B, C)
    w, b = rnd(0, C + 1, seed=3), np.array([0.3], np.float32)
    ybar = np.array([1.0, 2.0, 3.0], np.float32)
    zero = np.zeros((B, 31, 31), np.float32)
    yhat0, _, fake0 = head_fwd(dt, cat, w[:C], b, None, ybar, noise_entry=False)
    dcat0, dw0, db0 = head_bwd(dt, cat, dfake, w[:C], None, noise_entry=False)
    for u in (zero, None):                                       # a zero draw, and the new entry points without a draw
        yhat, g32, fake = head_fwd(dt, cat, w if u is not None else w[:C], b, u, ybar)
        assert np.array_equal(yhat, yhat0) and np.array_equal(fake, fake0)
        assert np.array_equal((g32 + ybar[:, None, None]).astype(np.float32), yhat0)
        dcat, dw, db = head_bwd(dt, cat, dfake, w if u is not None else w[:C], u)
        assert np.array_equal(dcat, dcat0) and np.array_equal(dw[:C], dw0) and np.array_equal(db, db0)
        if u is not None:
            assert dw[C] == 0.0


# ------------------------------------------------------------------------------------------------ the new conv geometries
def rows(act):
    """The [rows, c] view of an activation that may be a channel window of a wider buffer."""
    return torch.as_strided(act.buf, (act.n * act.h * act.w, act.c), (act.cs, 1))


def put(act, a):
    rows(act).copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32).reshape(-1, act.c)).to(DEV, K().TORCH_DTYPE[act.dtype]))


def get(act):
    return rows(act).float().cpu().numpy().reshape(act.n, act.h, act.w, act.c)


def exact_forms(conv, dtype, roots):
    """tests/test_gpu_conv_exact.py's three_forms recipe (VALID: forward with bias + relu, backward-data with a bias,
    filter gradient with beta = 1 on a 0.5 pre-fill) on a conv whose sides may be channel windows.  `roots`: the buffers the
    windows lie in; every channel of theirs outside the window a launch writes must keep its pre-fill of 1."""
    big, small = conv.big, conv.small
    n = big.n
    case = (n, big.h, big.w, big.c, small.c, conv.desc.kh, conv.desc.stride)
    assert X.geometry(case, 'VALID')[:2] == (small.h, small.w) and conv.desc.kh == conv.desc.kw
    o = X.oracle(case, 0, 'VALID')
    i = o.inp
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    w = t(i.W)
    conv.pack(w)
    esz = K().ELEM_SIZE[dtype]

    def prefill():
        for r in roots:
            r.buf.zero_()
            rows(r).fill_(1.0)

    def untouched(written, what):
        for r in roots:
            off = (written.buf.data_ptr() - r.buf.data_ptr()) // esz
            full = get(r)
            if 0 <= off < r.cs and written.buf.untyped_storage().data_ptr() == r.buf.untyped_storage().data_ptr():
                full = np.delete(full, np.s_[off:off + written.c], axis=-1)
            assert np.all(full == 1.0), '%s wrote outside its channel window' % what
    bias_small, bias_big = t(i.bias_small), t(i.bias_big)
    # forward
    prefill()
    put(big, i.x)
    conv.fwd(big.ptr(), small.ptr(), n, K().epilogue(bias=bias_small, act=K().ACT_RELU, leak=X.LEAK))
    kern = L().load().tdg_last_kernel().decode()
    want = X.stored(X.epilogue_ref(o.y, i.bias_small, 'relu'), dtype, 'fwd')
    assert np.array_equal(get(small), want), 'fwd %s through %s: %s' % (case, kern, X.describe_mismatch(get(small), want))
    put(big, np.ones(big.n * big.h * big.w * big.c))
    untouched(small, 'fwd')
    # backward data
    prefill()
    put(small, i.dy)
    conv.bwd_data(small.ptr(), big.ptr(), n, K().epilogue(bias=bias_big))
    kern = L().load().tdg_last_kernel().decode()
    want = X.stored(X.epilogue_ref(o.dx, i.bias_big), dtype, 'bwd_data')
    assert np.array_equal(get(big), want), 'bwd_data %s through %s: %s' % (case, kern, X.describe_mismatch(get(big), want))
    put(small, np.ones(small.n * small.h * small.w * small.c))
    untouched(big, 'bwd_data')
    # backward filter
    put(big, i.x)
    put(small, i.dy)
    dw = torch.full(tuple(i.W.shape), 0.5, device=DEV)
    conv.bwd_filter(big.ptr(), small.ptr(), dw, n, beta=1.0)
    kern = L().load().tdg_last_kernel().decode()
    want = X.stored(o.dw + 0.5, 0, 'bwd_filter')
    assert np.array_equal(dw.cpu().numpy(), want), 'bwd_filter %s through %s: %s' % (case, kern, X.describe_mismatch(dw.cpu().numpy(), want))


def unet_for(node, dtype, B=2):
    """The executor of paper_sampler's generator (no batch norm) at batch B, its variables undeclared: descriptors only."""
    plugin = pkg('models.sampler.paper_sampler').paper_sampler
    nets = plugin.build_graph(SimpleNamespace(batch_size=B, noise_layer=node, e_bn='false', e_bn_off=True))
    E = pkg('engine')
    return pkg('unet').UNet(nets['generator/encoder'], nets['generator/decoder'], B, dtype, DEV, E.ParamStore(DEV), K().Workspace(DEV),
                            K().Act(B, 65, 65, 3, dtype, DEV))


# (noise node, 'e' / 'd', layer): the conv of that encoder / decoder layer, and what the geometry is
GEOMETRIES = [('e1', 'e', 2, (65, 128)),      # e2 reads [e1 | u], 65 channels at offset 64 of the 136-stride [d3 | e1 | u]
              ('e2', 'e', 3, (129, 256)),     # e3 reads [e2 | u], 129 channels at offset 128 of a 264-stride buffer
              ('e3', 'e', 4, (257, 512)),     # e4 reads [e3 | u], 257 channels at offset 256 of a 520-stride buffer
              ('e3', 'd', 2, (128, 512)),     # d2 beside it reads the window (0, 512) of the same 520-stride buffer
              ('e4', 'd', 1, (256, 513)),     # d1 reads the 513-channel latent [e4 | u]
              ('d2', 'd', 2, (128, 513)),     # d2 reads all of [d1 | e3 | u]
              ('d3', 'd', 3, (64, 257))]      # d3 reads all of [d2 | e2 | u]


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('node,side,layer,chans', GEOMETRIES)
def test_noise_window_conv_geometries_are_exact(node, side, layer, chans, dtype):
    U = unet_for(node, dtype)
    conv = (U.e_conv if side == 'e' else U.d_conv)[layer]
    assert (conv.big.c, conv.small.c) == chans and conv.big.n == 2
    if (node, side) == ('e1', 'e'):
        assert conv.big.cs == 136 and (conv.big.buf.data_ptr() - U.cat[4].buf.data_ptr()) // K().ELEM_SIZE[dtype] == 64
    roots = list(U.cat.values()) + list(U.gcat.values()) + ([U.lat] if node == 'e4' else [])
    exact_forms(conv, dtype, roots)


@pytest.mark.parametrize('dtype', [0, 1])
def test_513_channel_window_into_a_valid_conv_is_exact(dtype):
    """No layer of the model reads 513 channels through a forward conv (its 513-channel tensors feed deconvs, above); the same
    window arithmetic on a conv: channels [8, 521) of a 528-stride buffer (the window ends where the buffer's channels
    end, as every noise window does) into a VALID k5 s2 conv."""
    root = K().Act(2, 5, 5, 521, dtype, DEV)
    small = K().Act(2, 1, 1, 64, dtype, DEV)
    conv = K().Conv(root.window(8, 513), small, 5, 5, 2, 0, 0)
    assert root.cs == 528
    exact_forms(conv, dtype, [root])
