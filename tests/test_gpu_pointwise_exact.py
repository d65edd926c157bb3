"""The loss, seed and pointwise kernels of csrc/tdg_elementwise.hip (and tdg_cgan_join) against the float64 references of
tests/_exact_pointwise.py, per element: bit for bit where the recipe makes exactness provable, against derived bounds
where it cannot be.  Every input is NaN-guarded (padding channels, a band of rows behind, the elements in front of an
offset base), every output sentinel-guarded; the in-place kernels carry the sentinel in their padding.  The conditions
of the exact comparisons are proved for the whole case table on the CPU (tests/test_host_pointwise_exact.py); nothing
here skips.

Each bounded comparison prints its worst ratio (`RATIO <what> <value>`, run with -s); DESIGN.md section 2 records them."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_pointwise as P

pytestmark = pytest.mark.gpu

DTYPES = [0, 1]
ES = {0: 4, 1: 2}
DT = {0: 'f32', 1: 'bf16'}


def K():
    return pkg('kernels')


def call(name, *args):
    pkg('_lib').call(name, *args)


def rejected(name, *args):
    with pytest.raises(pkg('_lib').TdgError, match=name):
        call(name, *args)


def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def workspace():
    return K().Workspace(dev())


def ws():
    w = workspace().ensure(4096)
    return K().ptr(w), w.numel()


def exact(got, want, what):
    assert np.array_equal(got, want), '%s\n%s' % (what, P.describe_mismatch(np.asarray(got), np.asarray(want)))


def within(ratio, what):
    """`ratio`: |error| / bound per element.  Prints the worst one, then asserts it."""
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    print('RATIO %s %.4g' % (what, worst))
    if not worst <= 1.0:
        bad = np.argwhere(~(np.asarray(ratio) <= 1.0))
        raise AssertionError('%s: %d of %d miss the bound, worst ratio %g, first at %s'
                             % (what, len(bad), np.size(ratio), worst, tuple(int(i) for i in bad[0])))


def compare(got, ref, bound, dtype, what):
    """bound None: the device must equal store(reference); else per element within the bound."""
    if bound is None:
        exact(got, P.store(ref, dtype), what)
    else:
        within(P.bound_ratio(got, ref, bound), what)


class Buf:
    """A guarded [rows][c] tensor (P.Layout) on the device.  data=None: an output, prefilled with the sentinel.  An input is
    NaN outside the tensor, unless `fill` says otherwise (in-place kernels: the sentinel, which must survive)."""

    def __init__(self, lay, dtype, data=None, fill=None):
        self.lay, self.dtype = lay, dtype
        self.fill = fill if fill is not None else (P.NAN if data is not None else P.SENTINEL)
        flat = lay.pack(data, self.fill) if data is not None else np.full(lay.n, P.SENTINEL, dtype=np.float32)
        self.t = torch.from_numpy(flat).to(dev()).to(K().TORCH_DTYPE[dtype])

    def ptr(self, extra_bytes=0):
        return K().ptr(self.t, self.lay.off * ES[self.dtype] + extra_bytes)

    def get(self):
        """The tensor's values, after asserting that nothing outside it has changed."""
        flat = self.t.float().cpu().numpy()
        out = self.lay.outside(flat)
        ok = np.isnan(out) if np.isnan(self.fill) else out == self.fill
        assert np.all(ok), '%d guard elements were overwritten' % int((~ok).sum())
        return self.lay.unpack(flat)


def flat(n, off, dtype, data=None, fill=None):
    return Buf(P.flat_layout(n, off), dtype, None if data is None else np.asarray(data).reshape(n, 1), fill)


def fget(b):
    return b.get().ravel()


def fvec(head, tail=8):
    """An f32 vector on the device followed by `tail` sentinels."""
    return torch.from_numpy(np.concatenate([np.asarray(head, dtype=np.float32).ravel(), np.full(tail, P.SENTINEL, np.float32)])).to(dev())


def vget(t, n):
    a = t.cpu().numpy()
    assert np.all(a[n:] == P.SENTINEL), 'a write landed behind the %d-element vector' % n
    return a[:n]


def nans(n):
    return np.full(n, P.NAN, dtype=np.float32)


_ALIVE = []


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    del _ALIVE[:]


def fin(x):
    """An f32 input vector followed by NaN.  It stays allocated until the test ends: only its pointer goes to the kernel, and
    the block of a tensor that has been dropped is handed to the next one."""
    t = torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.float32).ravel(), nans(16)])).to(dev())
    _ALIVE.append(t)
    return t


# ------------------------------------------------------------------------------------------------ 1. flat pointwise
FLAT_IDS = ['n%d%s' % (n, '-off%d' % o if o else '') for n, o in P.FLAT_CASES]


def run_add_act(n, off, dtype):
    inp = P.add_act_inputs(n)
    a, b = flat(n, off, dtype, inp.a), flat(n, off, dtype, inp.b)
    for act in P.ACTS:
        out = flat(n, off, dtype)
        call('tdg_add_act', dtype, a.ptr(), b.ptr(), n, act, P.LEAK, out.ptr(), K().stream())
        ref, bound = P.add_act_ref(inp, act, dtype)
        compare(fget(out), ref, bound, dtype, '%s add_act n=%d off=%d %s' % (DT[dtype], n, off, P.ACT_NAME[act]))
        if n > 100000:
            break                                                   # the block cap is the same for every activation
    fget(a), fget(b)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,off', P.FLAT_CASES, ids=FLAT_IDS)
def test_add_act(n, off, dtype):
    """Integers: none / relu / lrelu exact, tanh and sigmoid by bound."""
    run_add_act(n, off, dtype)


def run_affine_cast(n, off, dtype):
    x = P.affine_inputs(n)
    src = torch.from_numpy(np.concatenate([nans(off), x, nans(16)])).to(dev())
    out = flat(n, off, dtype)
    call('tdg_affine_cast', dtype, K().ptr(src, 4 * off), n, P.AFFINE_SCALE, P.AFFINE_SHIFT, out.ptr(), K().stream())
    exact(fget(out), P.store(P.affine_ref(x), dtype), '%s affine_cast n=%d off=%d' % (DT[dtype], n, off))


@pytest.mark.parametrize('dtype', DTYPES)
def test_flat_loops_past_the_block_cap(dtype):
    """n = 4096 * 1024 + 257: ew_blocks() caps the grid, the grid-stride loop takes a second, ragged trip."""
    assert P.flat_blocks(P.BIG_N)[1]
    run_add_act(P.BIG_N, 0, dtype)
    run_affine_cast(P.BIG_N, 0, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,off', P.FLAT_CASES, ids=FLAT_IDS)
def test_act_bwd_scale_and_casts(n, off, dtype):
    """act_bwd (all five codes, the mask decided at post == +-0), scale_by_dev, cast_to_f32, cast_from_f32 (with the bf16
    ties), affine_cast: exact."""
    what = '%s n=%d off=%d' % (DT[dtype], n, off)
    inp = P.act_bwd_inputs(n)
    dy, post = flat(n, off, dtype, inp.dy), flat(n, off, dtype, inp.post)
    for act in P.ACTS:
        dx = flat(n, off, dtype)
        call('tdg_act_bwd', dtype, dy.ptr(), post.ptr(), n, act, P.LEAK, dx.ptr(), K().stream())
        exact(fget(dx), P.store(P.act_bwd_ref(inp, act).dx, dtype), 'act_bwd %s %s' % (what, P.ACT_NAME[act]))
    fget(dy), fget(post)
    x = P.scale_inputs(n).x
    src = flat(n, off, dtype, x)
    for k in P.SCALE_COEFS:
        out = flat(n, off, dtype)
        call('tdg_scale_by_dev', dtype, src.ptr(), n, K().ptr(fin([k])), out.ptr(), K().stream())
        exact(fget(out), P.store(k * x.astype(np.float64), dtype), 'scale_by_dev %s k=%g' % (what, k))
    c = P.cast_inputs(n)
    src, out = flat(n, off, dtype, c.x), flat(n, off, 0)
    call('tdg_cast_to_f32', dtype, src.ptr(), n, out.ptr(), K().stream())
    exact(fget(out), c.x, 'cast_to_f32 ' + what)
    src, out = flat(n, off, 0, c.ties), flat(n, off, dtype)
    call('tdg_cast_from_f32', dtype, src.ptr(), n, out.ptr(), K().stream())
    got = fget(out)
    exact(got, P.store(c.ties, dtype), 'cast_from_f32 ' + what)
    if dtype == 1:
        m = min(n, len(P.TIES))
        exact(got[:m], P.TIES_BF16[:m], 'cast_from_f32 ties to even ' + what)
    fget(src)
    run_affine_cast(n, off, dtype)


@pytest.mark.parametrize('n,off', P.FLAT_CASES, ids=FLAT_IDS)
def test_fill_and_clamp(n, off):
    out = flat(n, off, 0)
    call('tdg_fill_f32', out.ptr(), n, P.FILL_VALUE, K().stream())
    exact(fget(out), np.full(n, P.FILL_VALUE, np.float32), 'fill n=%d off=%d' % (n, off))
    for lo, hi in P.CLAMPS:
        x = P.clamp_inputs(n, lo, hi)
        b = flat(n, off, 0, x, fill=P.SENTINEL)
        call('tdg_clamp', b.ptr(), n, lo, hi, K().stream())
        exact(fget(b), np.minimum(np.maximum(x, np.float32(lo)), np.float32(hi)), 'clamp [%g, %g] n=%d off=%d' % (lo, hi, n, off))


# ------------------------------------------------------------------------------------------------ 2. strided pointwise
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,c', P.BIAS_ACT_SHAPES, ids=['%dx%d' % s for s in P.BIAS_ACT_SHAPES])
def test_bias_act(rows, c, dtype):
    inp = P.bias_act_inputs(rows, c)
    bias = fin(inp.bias)
    for cs in P.strides_of(c):
        lay = P.Layout(rows, c, cs)
        x = Buf(lay, dtype, inp.x)
        for with_bias in P.BIAS_GIVEN:
            for act in P.ACTS:
                y = Buf(lay, dtype)
                call('tdg_bias_act', dtype, x.ptr(), rows, c, cs, K().ptr(bias) if with_bias else None, act, P.LEAK, y.ptr(), K().stream())
                ref, bound = P.bias_act_ref(inp, with_bias, act, dtype)
                compare(y.get(), ref, bound, dtype, '%s bias_act %dx%d cs=%d bias=%s %s' % (DT[dtype], rows, c, cs, with_bias, P.ACT_NAME[act]))
        x.get()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', P.CAST_ROWS_ROWS)
def test_affine_cast_rows(rows, dtype):
    """Both sides of the c <= 16 branch, cs > c: the padding columns keep their prefill."""
    for c in P.CAST_ROWS_C:
        for cs in (c + 3, (c + 8) // 8 * 8):
            x = P.affine_inputs((rows, c))
            out = Buf(P.Layout(rows, c, cs), dtype)
            call('tdg_affine_cast_rows', dtype, K().ptr(fin(x)), rows, c, cs, P.AFFINE_SCALE, P.AFFINE_SHIFT, out.ptr(), K().stream())
            exact(out.get(), P.store(P.affine_ref(x), dtype), '%s affine_cast_rows %dx%d cs=%d (%s)' % (DT[dtype], rows, c, cs, P.cast_rows_branch(c)))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', P.CAST_ROWS_ROWS)
def test_affine_cast_pair(rows, dtype):
    for ca, cb in P.PAIR_SPLITS:
        a, b = P.affine_inputs((rows, ca), tag=31), P.affine_inputs((rows, cb), tag=32)
        lay = P.Layout(rows, 4, 4)
        ab, a0 = Buf(lay, dtype), Buf(lay, dtype)
        args = (dtype, K().ptr(fin(a)), ca, K().ptr(fin(b)), cb, rows, P.AFFINE_SCALE, P.AFFINE_SHIFT)
        call('tdg_affine_cast_pair', *args, ab.ptr(), a0.ptr(), K().stream())
        what = '%s affine_cast_pair rows=%d (%d, %d)' % (DT[dtype], rows, ca, cb)
        ra, rb = P.affine_ref(a), P.affine_ref(b)
        exact(ab.get(), P.store(np.concatenate([ra, rb], axis=1), dtype), what + ' out_ab')
        exact(a0.get(), P.store(np.concatenate([ra, np.zeros_like(rb)], axis=1), dtype), what + ' out_a0')
        rejected('tdg_affine_cast_pair', *args, ab.ptr(ES[dtype]), a0.ptr(), K().stream())          # misaligned output
        rejected('tdg_affine_cast_pair', *args, ab.ptr(), a0.ptr(ES[dtype]), K().stream())
    rejected('tdg_affine_cast_pair', dtype, args[1], 3, args[3], 2, rows, 2.0, -0.5, ab.ptr(), a0.ptr(), K().stream())   # ca + cb != 4
    rejected('tdg_affine_cast_pair', dtype, args[1], 1, args[3], 2, rows, 2.0, -0.5, ab.ptr(), a0.ptr(), K().stream())
    ab.get(), a0.get()                                                                              # a rejected call writes nothing


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('keep', P.DROPOUT_KEEPS)
def test_dropout(keep, dtype):
    """In place, ycs > c (the padding's sentinel survives): u == 1 - keep is kept, one grid step below it is dropped; twice
    with the same u gives y / keep**2 where kept and 0 where dropped."""
    for c in P.DROPOUT_C:
        inp = P.dropout_inputs(c, keep)
        u = fin(inp.u)
        y = Buf(P.Layout(P.DROPOUT_ROWS, c, c + 3), dtype, inp.y, fill=P.SENTINEL)
        what = '%s dropout keep=%g c=%d' % (DT[dtype], keep, c)
        once = P.dropout_ref(inp.y, inp.u, keep)
        call('tdg_dropout', dtype, y.ptr(), P.DROPOUT_ROWS, c, c + 3, K().ptr(u), keep, K().stream())
        got = y.get()
        exact(got, P.store(once, dtype), what)
        flags = (got.ravel() != 0)[:len(inp.lead)]
        assert flags.tolist() == [True, keep == 1.0, False][:len(inp.lead)], (what, flags)       # u = 1 - keep, 0, one step below 1 - keep
        call('tdg_dropout', dtype, y.ptr(), P.DROPOUT_ROWS, c, c + 3, K().ptr(u), keep, K().stream())
        twice = np.where(once != 0, inp.y.astype(np.float64) / keep ** 2, 0.0)
        exact(y.get(), P.store(twice, dtype), what + ' twice')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', P.GP_INTERP_ROWS)
def test_gp_interp(rows, dtype):
    for cols in P.GP_INTERP_COLS:
        for off in ((0, 1) if rows == 3 else (0,)):
            inp = P.gp_interp_inputs(rows, cols)
            lay = P.Layout(rows, cols, cols, off)
            x, g, out = Buf(lay, dtype, inp.x), Buf(lay, dtype, inp.g), Buf(lay, dtype)
            call('tdg_gp_interp', dtype, x.ptr(), g.ptr(), K().ptr(fin(inp.alpha)), rows, cols, out.ptr(), K().stream())
            exact(out.get(), P.store(P.gp_interp_ref(inp), dtype), '%s gp_interp %dx%d off=%d' % (DT[dtype], rows, cols, off))
            x.get(), g.get()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', P.JOIN_C)
def test_cgan_join(c, dtype):
    n_rgb = P.JOIN_N_RGB
    ccs, rcs, dcs = P.join_strides(c)
    assert len({ccs, rcs, dcs, c}) == 4
    what = '%s cgan_join c=%d' % (DT[dtype], c)
    (m0, rows, _), (m1, rows1, _), (m1n, rows3, rgb_given) = P.JOIN_RUNS
    assert (m0, m1, m1n, rows1, rgb_given) == (0, 1, 1, rows, False)
    # mode 0: comb[r] = [rgb[r % n_rgb] | depth[r]]
    inp = P.join_inputs(c, rows)
    comb = Buf(P.Layout(rows, 2 * c, ccs), dtype)
    rgb, depth = Buf(P.Layout(n_rgb, c, rcs), dtype, inp.rgb), Buf(P.Layout(rows, c, dcs), dtype, inp.depth)
    call('tdg_cgan_join', dtype, 0, n_rgb, rows, c, comb.ptr(), ccs, rgb.ptr(), rcs, depth.ptr(), dcs, K().stream())
    exact(comb.get(), P.store(P.join_fwd_ref(inp), dtype), what + ' mode 0')
    rgb.get(), depth.get()
    # mode 1 with rgb: depth[r] = comb[r][c:], rgb[r] = comb[r][:c] + comb[r + n_rgb][:c]
    comb = Buf(P.Layout(rows, 2 * c, ccs), dtype, inp.comb)
    rgb, depth = Buf(P.Layout(n_rgb, c, rcs), dtype), Buf(P.Layout(rows, c, dcs), dtype)
    call('tdg_cgan_join', dtype, 1, n_rgb, rows, c, comb.ptr(), ccs, rgb.ptr(), rcs, depth.ptr(), dcs, K().stream())
    want_depth, want_rgb = P.join_bwd_ref(inp)
    exact(depth.get(), P.store(want_depth, dtype), what + ' mode 1 depth')
    exact(rgb.get(), P.store(want_rgb, dtype), what + ' mode 1 rgb')
    comb.get()
    # mode 1, rgb NULL, 3 rows
    inp3 = P.join_inputs(c, rows3)
    comb3 = Buf(P.Layout(rows3, 2 * c, ccs), dtype, inp3.comb)
    rgb3, depth3 = Buf(P.Layout(n_rgb, c, rcs), dtype), Buf(P.Layout(rows3, c, dcs), dtype)
    call('tdg_cgan_join', dtype, 1, n_rgb, rows3, c, comb3.ptr(), ccs, None, 0, depth3.ptr(), dcs, K().stream())
    exact(depth3.get(), P.store(P.join_bwd_ref(inp3)[0], dtype), what + ' mode 1 depth, rgb NULL')
    assert np.all(rgb3.get() == P.SENTINEL)
    comb3.get()
    # the entry point's argument check
    ok = dict(mode=1, n_rgb=n_rgb, rows=rows, c=c, ccs=ccs, rgb=True, rcs=rcs, dcs=dcs)
    for bad in (dict(c=c + 4), dict(ccs=2 * c - 8), dict(ccs=ccs + 4), dict(rcs=rcs + 4), dict(rcs=c - 8), dict(dcs=dcs + 4), dict(dcs=c - 8),
                dict(mode=2), dict(mode=0, rgb=False), dict(rows=2 * n_rgb - 1), dict(n_rgb=0), dict(rows=0)):
        a = dict(ok, **bad)
        rejected('tdg_cgan_join', dtype, a['mode'], a['n_rgb'], a['rows'], a['c'], comb.ptr(), a['ccs'], rgb.ptr() if a['rgb'] else None, a['rcs'],
                 depth.ptr(), a['dcs'], K().stream())
    exact(depth.get(), P.store(want_depth, dtype), what + ': a rejected call writes nothing')


# ------------------------------------------------------------------------------------------------ 3. VAE
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('L', P.VAE_L)
def test_vae_reparam_and_backward(L, dtype):
    """z = m + sd * eps and (dz, dz * eps), exact; hs, es and zs all different and above their minimum."""
    hs, es, zs = P.vae_strides(L)
    for rows in P.VAE_ROWS:
        inp = P.reparam_inputs(rows, L)
        what = '%s %dx%d' % (DT[dtype], rows, L)
        heads = Buf(P.Layout(rows, 2 * L, hs), dtype, np.concatenate([inp.m, inp.sd], axis=1))
        eps, z = Buf(P.Layout(rows, L, es), dtype, inp.eps), Buf(P.Layout(rows, L, zs), dtype)
        call('tdg_vae_reparam', dtype, heads.ptr(), hs, eps.ptr(), es, rows, L, z.ptr(), zs, K().stream())
        exact(z.get(), P.store(P.reparam_ref(inp), dtype), 'vae_reparam ' + what)
        dz, dh = Buf(P.Layout(rows, L, zs), dtype, inp.dz), Buf(P.Layout(rows, 2 * L, hs), dtype)
        call('tdg_vae_reparam_bwd', dtype, dz.ptr(), zs, eps.ptr(), es, rows, L, dh.ptr(), hs, K().stream())
        exact(dh.get(), P.store(P.reparam_bwd_ref(inp), dtype), 'vae_reparam_bwd ' + what)
        heads.get(), eps.get(), dz.get()
    for bad in (dict(hs=2 * L - 1), dict(es=L - 1), dict(zs=L - 1)):
        a = dict(dict(hs=hs, es=es, zs=zs), **bad)
        rejected('tdg_vae_reparam', dtype, heads.ptr(), a['hs'], eps.ptr(), a['es'], rows, L, z.ptr(), a['zs'], K().stream())
        rejected('tdg_vae_reparam_bwd', dtype, dz.ptr(), a['zs'], eps.ptr(), a['es'], rows, L, dh.ptr(), a['hs'], K().stream())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('L', P.VAE_L)
def test_vae_reparam_bwd_kl(L, dtype):
    """By bound; the KL term is exactly 0 at sd == 0; kl weight 0 equals vae_reparam_bwd bit for bit; es < L and zs < L are
    rejected like in its two siblings."""
    hs, es, zs = P.vae_strides(L)
    hs_in = hs + 2
    for rows in P.VAE_ROWS:
        inp = P.kl_inputs(rows, L)
        what = '%s vae_reparam_bwd_kl %dx%d' % (DT[dtype], rows, L)
        heads = Buf(P.Layout(rows, 2 * L, hs_in), dtype, np.concatenate([inp.m, inp.sd], axis=1))
        eps, dz = Buf(P.Layout(rows, L, es), dtype, inp.eps), Buf(P.Layout(rows, L, zs), dtype, inp.dz)
        plain = Buf(P.Layout(rows, 2 * L, hs), dtype)
        call('tdg_vae_reparam_bwd', dtype, dz.ptr(), zs, eps.ptr(), es, rows, L, plain.ptr(), hs, K().stream())
        for klw in (0.0, 1.0):
            dh = Buf(P.Layout(rows, 2 * L, hs), dtype)
            call('tdg_vae_reparam_bwd_kl', dtype, dz.ptr(), zs, eps.ptr(), es, heads.ptr(), hs_in, klw, rows, L, dh.ptr(), hs, K().stream())
            got = dh.get()
            ref, bound = P.reparam_bwd_kl_ref(inp, klw, dtype)
            within(P.bound_ratio(got, ref, bound), what + ' klw=%g' % klw)
            if klw == 0:
                exact(got, plain.get(), what + ': weight 0 against vae_reparam_bwd')
            else:
                z0 = inp.sd == 0
                exact(got[:, L:][z0], P.store(P.reparam_bwd_ref(inp)[:, L:][z0], dtype), what + ': sd == 0, the KL term vanishes')
        heads.get(), eps.get(), dz.get()
    for bad in (dict(es=L - 1), dict(zs=L - 1), dict(hs=2 * L - 1), dict(hs_in=2 * L - 1)):
        a = dict(dict(hs=hs, es=es, zs=zs, hs_in=hs_in), **bad)
        rejected('tdg_vae_reparam_bwd_kl', dtype, dz.ptr(), a['zs'], eps.ptr(), a['es'], heads.ptr(), a['hs_in'], 1.0, rows, L, dh.ptr(), a['hs'],
                 K().stream())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,L', P.VAE_KL_SHAPES, ids=['%dx%d' % s for s in P.VAE_KL_SHAPES])
def test_vae_kl(rows, L, dtype):
    inp = P.kl_inputs(rows, L)
    hs = 2 * L + 3
    heads = Buf(P.Layout(rows, 2 * L, hs), dtype, np.concatenate([inp.m, inp.sd], axis=1))
    scal = fvec(nans(1))
    call('tdg_vae_kl', dtype, heads.ptr(), hs, rows, L, K().ptr(scal), *ws(), K().stream())
    ref, bound = P.vae_kl_ref(inp)
    within(P.bound_ratio(vget(scal, 1), ref, bound), '%s vae_kl %dx%d' % (DT[dtype], rows, L))
    heads.get()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', P.BCE_ROWS)
def test_vae_bce(rows, dtype):
    for c in P.BCE_C:
        inp = P.bce_inputs(rows, c)
        lay = P.Layout(rows, c, P.BCE_CS)
        d, seed, scal = Buf(lay, dtype, inp.d), Buf(lay, dtype), fvec(nans(1))
        call('tdg_vae_bce', dtype, K().ptr(fin(inp.x)), d.ptr(), rows, c, P.BCE_CS, seed.ptr(), K().ptr(scal), *ws(), K().stream())
        ref = P.bce_ref(inp, dtype)
        what = '%s vae_bce %dx%d' % (DT[dtype], rows, c)
        within(P.bound_ratio(vget(scal, 1), ref.loss, ref.loss_bound), what + ' loss')
        within(P.bound_ratio(seed.get(), ref.seed, ref.seed_bound), what + ' seed')
        d.get()


# ------------------------------------------------------------------------------------------------ 4. losses and seeds
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,c', P.L1_CASES, ids=['%dx%d' % s for s in P.L1_CASES])
def test_l1_loss(rows, c, dtype):
    inp = P.l1_inputs(rows, c)
    lay = P.Layout(rows, c, P.L1_CS)
    d, seed, scal = Buf(lay, dtype, inp.d), Buf(lay, dtype), fvec(nans(1))
    call('tdg_l1_loss', dtype, K().ptr(fin(inp.x)), d.ptr(), rows, c, P.L1_CS, P.AFFINE_SCALE, P.AFFINE_SHIFT, seed.ptr(), K().ptr(scal), *ws(),
         K().stream())
    ref = P.l1_ref(inp, dtype)
    what = '%s l1_loss %dx%d' % (DT[dtype], rows, c)
    exact(seed.get(), P.store(ref.seed, dtype), what + ' seed')
    if ref.pow2:
        exact(vget(scal, 1), np.float32([ref.loss]), what + ' loss')
    else:
        within(P.bound_ratio(vget(scal, 1), ref.loss, ref.loss_bound), what + ' loss')
    d.get()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', P.P2P_L1_ROWS)
def test_p2p_l1(rows, dtype):
    """Channel 0 of y and g at stride 8, the update ADDED onto channel 0 of dg at stride 3; dg NULL writes nothing."""
    inp = P.p2p_l1_inputs(rows)
    col = lambda a: a.reshape(rows, 1)                                                      # noqa: E731
    y, g = Buf(P.Layout(rows, 1, P.P2P_CS), dtype, col(inp.y)), Buf(P.Layout(rows, 1, P.P2P_CS), dtype, col(inp.g))
    ref = P.p2p_l1_ref(inp, dtype)
    what = '%s p2p_l1 rows=%d' % (DT[dtype], rows)
    scals = []
    for with_dg in P.DG_GIVEN:
        dg = Buf(P.Layout(rows, 1, P.P2P_DGS), dtype, col(inp.dg), fill=P.SENTINEL)
        scal = fvec(nans(2))
        call('tdg_p2p_l1', dtype, y.ptr(), g.ptr(), rows, P.P2P_CS, P.P2P_WEIGHT, dg.ptr() if with_dg else None, P.P2P_DGS, K().ptr(scal), *ws(),
             K().stream())
        got = dg.get().ravel()
        if not with_dg:
            exact(got, inp.dg, what + ': dg NULL')
        else:
            compare(got, ref.dg, None if ref.pow2 else ref.dg_bound, dtype, what + ' dg')
            exact(got[ref.d == 0], inp.dg[ref.d == 0], what + ': d == 0, no update')
        scals.append(vget(scal, 2))
    exact(scals[1], scals[0], what + ': scal with and without dg')
    if ref.pow2:
        exact(scals[0][:1], np.float32(ref.scal[:1]), what + ' scal[0]')
    within(P.bound_ratio(scals[0], ref.scal, ref.scal_bound), what + ' scal')
    y.get(), g.get()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', P.XENT_ROWS)
def test_p2p_xent(rows, dtype):
    """Logits 0, +-2**-10, +-30, +-88: the three means by bound and finite, the seeds per element; only channel 0 of each
    row is read or written."""
    inp = P.xent_inputs(rows)
    for cs in P.XENT_CS:
        z = Buf(P.Layout(2 * rows, 1, cs), dtype, inp.z.reshape(-1, 1))
        scals = []
        for mode, seed_given in P.XENT_RUNS:
            ref = P.xent_ref(inp, mode, dtype)
            what = '%s p2p_xent rows=%d cs=%d mode=%d%s' % (DT[dtype], rows, cs, mode, '' if seed_given else ' seed NULL')
            seed, scal = Buf(P.Layout(2 * rows, 1, cs), dtype), fvec(nans(3))
            call('tdg_p2p_xent', dtype, z.ptr(), rows, cs, mode, seed.ptr() if seed_given else None, K().ptr(scal), K().stream())
            got = seed.get().ravel()
            within(P.bound_ratio(vget(scal, 3), ref.scal, ref.scal_bound), what + ' scal')
            scals.append(vget(scal, 3))
            exact(scals[-1], scals[0], what + ': the same scalars in every mode')
            if mode == 0:
                assert np.all(got == P.SENTINEL), what + ': mode 0 writes no seed'
            else:
                assert np.all(np.isfinite(got)), what
                within(P.bound_ratio(got, ref.seed, ref.seed_bound), what + ' seed')
                if mode == 2:
                    exact(got[:rows], np.zeros(rows, np.float32), what + ': zeros in the real half')
        rejected('tdg_p2p_xent', dtype, z.ptr(), rows, cs, 1, None, K().ptr(scal), K().stream())
        z.get()


@pytest.mark.parametrize('n', P.LOGLOSS_N)
def test_gan_logloss(n):
    inp = P.logloss_inputs(n)
    seeds, scal = [fvec(nans(n)) for _ in range(3)], fvec(nans(2))
    call('tdg_gan_logloss', K().ptr(fin(inp.dr)), K().ptr(fin(inp.df)), n, *[K().ptr(s) for s in seeds], K().ptr(scal), K().stream())
    ref = P.logloss_ref(inp)
    within(P.bound_ratio(vget(scal, 2), ref.scal, ref.scal_bound), 'gan_logloss n=%d scal' % n)
    for name, s, r in zip(('seed_real', 'seed_fake_d', 'seed_fake_g'), seeds, ref.seeds):
        within(P.bound_ratio(vget(s, n), r.v, r.e), 'gan_logloss n=%d %s' % (n, name))


GP_ROWS_ALL = P.GP_ROWS_EXACT + P.GP_ROWS_BOUNDED


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows,cols', GP_ROWS_ALL, ids=['%dx%d' % s for s in GP_ROWS_ALL])
def test_gp_rows(rows, cols, dtype):
    inp = P.gp_rows_inputs(rows, cols)
    lay = P.Layout(rows, cols, cols)
    v, u, pen = Buf(lay, dtype, inp.v), Buf(lay, dtype), fvec(nans(rows))
    call('tdg_gp_rows', dtype, v.ptr(), rows, cols, P.GP_LAMBDA, K().ptr(pen), u.ptr(), K().stream())
    ref = P.gp_rows_ref(inp, dtype)
    what = '%s gp_rows %dx%d' % (DT[dtype], rows, cols)
    if (rows, cols) in P.GP_ROWS_EXACT:
        exact(vget(pen, rows), np.float32(ref.pen), what + ' pen')
        exact(u.get(), P.store(ref.u, dtype), what + ' u')
        if cols == 1:
            assert np.all(vget(pen, rows) == 0) and np.all(u.get() == 0)
    else:
        within(P.bound_ratio(vget(pen, rows), ref.pen, ref.pen_bound), what + ' pen')
        within(P.bound_ratio(u.get(), ref.u, ref.u_bound), what + ' u')
    v.get()


# ------------------------------------------------------------------------------------------------ 5. Adam and utilities
def adam_bufs(inp):
    return [fvec(a) for a in (inp.p, inp.g, inp.m, inp.v)]


def adam_dev(bufs, n, t_dev):
    call('tdg_adam_step_dev', *[K().ptr(b) for b in bufs], n, P.ADAM.lr, P.ADAM.b1, P.ADAM.b2, P.ADAM.eps, P.ADAM.gs, K().ptr(t_dev), K().stream())


@pytest.mark.parametrize('t0', P.ADAM_T0)
@pytest.mark.parametrize('n', P.ADAM_N)
def test_adam_step_dev(n, t0):
    """One step per element against the float64 rule (lr_t through two powf); t_dev rises by exactly 1 per launch, three
    launches in a row and a sumsq launch in between included; tdg_adam_step with the host's lr_t gives the same m and v
    and a p within the two bounds.  All on torch's current stream (test_ticketed_kernels_keep_to_one_stream)."""
    inp = P.adam_inputs(n)
    what = 'adam_step_dev n=%d (%d blocks, %s tickets) t0=%d' % ((n,) + P.ticket_level(n) + (t0,))
    t_dev = torch.tensor([t0, 77, 77], dtype=torch.int32, device=dev())
    bufs = adam_bufs(inp)
    adam_dev(bufs, n, t_dev)
    assert t_dev.tolist() == [t0 + 1, 77, 77], what
    ref = P.adam_ref(inp, P.adam_lr_t(t0 + 1))
    got = [vget(b, n) for b in bufs]
    exact(got[1], inp.g, what + ': g untouched')
    for name, g, r in (('m', got[2], ref.m), ('v', got[3], ref.v), ('p', got[0], ref.p)):
        within(P.bound_ratio(g, r.v, r.e), what + ' ' + name)
    host = adam_bufs(inp)
    lr_host = P.adam_lr_t(t0 + 1, on_host=True)
    call('tdg_adam_step', *[K().ptr(b) for b in host], n, float(lr_host.v), P.ADAM.b1, P.ADAM.b2, P.ADAM.eps, P.ADAM.gs, K().stream())
    href = P.adam_ref(inp, lr_host)
    hgot = [vget(b, n) for b in host]
    exact(hgot[2], got[2], what + ': m of adam_step')
    exact(hgot[3], got[3], what + ': v of adam_step')
    within(P.bound_ratio(hgot[0], href.p.v, href.p.e), what + ' p of adam_step (host lr_t)')
    within(np.abs(hgot[0].astype(np.float64) - got[0]) / (np.abs(href.p.v - ref.p.v) + href.p.e + ref.p.e), what + ' p, device against host lr_t')
    # three launches back to back, a sumsq launch in between: + 3, no memset, each family its own ticket slot
    x = fin(np.ones(256 * 256 * 4 + 5, np.float32))
    acc = fvec(nans(1))
    adam_dev(bufs, n, t_dev)
    K().sumsq(workspace(), 0, K().ptr(x), 256 * 256 * 4 + 5, acc)
    adam_dev(bufs, n, t_dev)
    adam_dev(bufs, n, t_dev)
    assert t_dev.tolist() == [t0 + 4, 77, 77], what
    exact(vget(acc, 1), np.float32([256 * 256 * 4 + 5]), what + ': sumsq between two Adam launches')
    assert all(np.all(np.isfinite(vget(b, n))) for b in bufs)


def test_adam_rejects_n_not_a_multiple_of_4():
    bufs = adam_bufs(P.adam_inputs(8))
    t_dev = torch.zeros(1, dtype=torch.int32, device=dev())
    for n in (1, 6, 7):
        rejected('tdg_adam_step_dev', *[K().ptr(b) for b in bufs], n, 1e-3, 0.5, 0.9, 1e-8, 1.0, K().ptr(t_dev), K().stream())
        rejected('tdg_adam_step', *[K().ptr(b) for b in bufs], n, 1e-3, 0.5, 0.9, 1e-8, 1.0, K().stream())
    assert t_dev.item() == 0


@pytest.mark.parametrize('n', P.FINITE_N)
def test_check_finite(n):
    """The kernel only ever stores 1: a clean tensor leaves a prefilled flag as it was (0 and 5)."""
    x = np.ones(n, np.float32)
    for prefill in (0, 5):
        flag = torch.tensor([prefill, 77], dtype=torch.int32, device=dev())
        call('tdg_check_finite', K().ptr(fin(x)), n, K().ptr(flag), K().stream())          # (NaN behind the tensor: an over-read shows)
        assert flag.tolist() == [prefill, 77], 'clean n=%d' % n
    for pos in P.finite_positions(n):
        for bad in P.BAD_VALUES:
            y = x.copy()
            y[pos] = bad
            flag = torch.tensor([0, 77], dtype=torch.int32, device=dev())
            call('tdg_check_finite', K().ptr(fin(y)), n, K().ptr(flag), K().stream())
            assert flag.tolist() == [1, 77], 'n=%d %r at %d' % (n, bad, pos)


def test_add_i32():
    x = torch.tensor([10, 77], dtype=torch.int32, device=dev())
    total = 10
    for inc in P.ADD_I32_INCS:
        call('tdg_add_i32', K().ptr(x), inc, K().stream())
        total += inc
        assert x.tolist() == [total, 77]
