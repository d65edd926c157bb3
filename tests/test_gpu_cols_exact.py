"""The column-reduction, batch-norm, scalar- and row-reduction kernels of csrc/tdg_elementwise.hip against the float64
oracles of tests/_exact_cols.py: bit for bit where the recipe makes exactness provable, per element (per column for column
outputs) against derived bounds where it cannot be.  Every input is NaN-guarded (padding columns, a band of rows behind,
the elements in front of an offset base), every output sentinel-guarded.  The caps the exact comparisons rest on are
proved for the whole case table on the CPU (tests/test_host_cols_exact.py); nothing here skips.

Each test prints its worst bound ratio (`RATIO <what> <value>`, run with -s); DESIGN.md section 2 records them."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_cols as X

pytestmark = pytest.mark.gpu

DTYPES = [0, 1]
ES = {0: 4, 1: 2}
DT = {0: 'f32', 1: 'bf16'}
TABLE_IDS = [X.case_id(k) for k in X.TABLE]
ALL_ACTS = (X.ACT_NONE, X.ACT_RELU, X.ACT_LRELU, X.ACT_TANH)
ACT_NAME = {X.ACT_NONE: 'none', X.ACT_RELU: 'relu', X.ACT_LRELU: 'lrelu', X.ACT_TANH: 'tanh'}
# every activation on the small cases, one on the large ones (their geometry is what they are for)
CASE_ACTS = [(k, a) for k in X.TABLE for a in (ALL_ACTS if k in X.SMALL else (X.ACT_LRELU,))]
CASE_ACT_IDS = ['%s-%s' % (X.case_id(k), ACT_NAME[a]) for k, a in CASE_ACTS]
RSTD_CLAMPED = 1.0 / np.sqrt(np.float64(np.float32(X.EPS)))


def K():
    return pkg('kernels')


def call(name, *args):
    pkg('_lib').call(name, *args)


def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def workspace():
    return K().Workspace(dev())


def exact(got, want, what):
    assert np.array_equal(got, want), '%s\n%s' % (what, X.describe_mismatch(np.asarray(got), np.asarray(want)))


def within(ratio, what):
    """`ratio`: |error| / bound per element or column.  Prints the worst one, then asserts it."""
    worst = float(np.max(ratio)) if np.size(ratio) else 0.0
    print('RATIO %s %.4g' % (what, worst))
    if not worst <= 1.0:
        bad = np.argwhere(~(np.asarray(ratio) <= 1.0))
        raise AssertionError('%s: %d of %d miss the bound, worst ratio %g, first at %s'
                             % (what, len(bad), np.size(ratio), worst, tuple(int(i) for i in bad[0])))


class Buf:
    """A guarded [rows][c] tensor (X.Layout) on the device.  data=None: an output, prefilled with the sentinel."""

    def __init__(self, lay, dtype, data=None):
        self.lay, self.dtype = lay, dtype
        self.fill = X.NAN if data is not None else X.SENTINEL
        flat = lay.pack(data) if data is not None else np.full(lay.n, X.SENTINEL, dtype=np.float32)
        self.t = torch.from_numpy(flat).to(dev()).to(K().TORCH_DTYPE[dtype])

    def ptr(self):
        return K().ptr(self.t, self.lay.off * ES[self.dtype])

    def act(self):
        """The tensor as a kernels.Act whose buffer starts at the tensor's first element."""
        lay = self.lay
        return K().Act(lay.rows, 1, 1, lay.c, self.dtype, dev(), lay.cs, buf=self.t[lay.off:])

    def get(self):
        """The tensor's values, after asserting that nothing outside it (padding columns, the band behind, the elements in
        front) has changed."""
        flat = self.t.float().cpu().numpy()
        out = self.lay.outside(flat)
        ok = np.isnan(out) if np.isnan(self.fill) else out == self.fill
        assert np.all(ok), '%d guard elements were overwritten' % int((~ok).sum())
        return self.lay.unpack(flat)


def fvec(head, tail=8):
    """An f32 vector on the device followed by `tail` sentinels."""
    return torch.from_numpy(np.concatenate([np.asarray(head, dtype=np.float32), np.full(tail, X.SENTINEL, np.float32)])).to(dev())


def vget(t, n):
    a = t.cpu().numpy()
    assert np.all(a[n:] == X.SENTINEL), 'a write landed behind the %d-element vector' % n
    return a[:n]


def nans(n):
    return np.full(n, X.NAN, dtype=np.float32)


def layout(k, cs=None, lead_rows=0):
    cs = k.cs if cs is None else cs
    return X.Layout(k.rows, k.c, cs, k.off + lead_rows * cs)


@functools.lru_cache(maxsize=2)
def colsum_inputs(k):
    return X.colsum_inputs(k)


@functools.lru_cache(maxsize=2)
def fwd_inputs(k):
    inp = X.bn_fwd_inputs(k)
    inp.st = X.bn_stats_ref(inp.u)
    return inp


@functools.lru_cache(maxsize=2)
def bwd_inputs(k):
    return X.bn_bwd_inputs(k)


# ------------------------------------------------------------------------------------------------ 1. column sums
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', X.TABLE, ids=TABLE_IDS)
def test_bias_grad_and_colsum_weighted(k, dtype):
    """tdg_bias_grad and tdg_colsum_weighted (integer coefficients and a null coef), beta = 0 onto NaN and beta = 1 onto
    a prefilled vector: exact over the whole geometry table."""
    inp = colsum_inputs(k)
    x = Buf(layout(k), dtype, inp.x)
    coef = torch.from_numpy(np.concatenate([inp.coef, nans(8)])).to(dev())
    for beta, old in ((0.0, None), (1.0, inp.old)):
        head = nans(k.c) if old is None else old
        out = fvec(head)
        K().bias_grad(workspace(), x.act(), k.c, out, beta=beta)
        exact(vget(out, k.c), X.colsum_ref(inp.x, None, old), 'bias_grad beta=%g' % beta)
        for cf, cf_host in ((coef, inp.coef), (None, None)):
            out = fvec(head)
            K().colsum_weighted(workspace(), dtype, x.ptr(), k.rows, k.c, k.cs, cf, out, beta=beta)
            exact(vget(out, k.c), X.colsum_ref(inp.x, cf_host, old), 'colsum_weighted coef=%s beta=%g' % (cf is not None, beta))
    x.get()


# ------------------------------------------------------------------------------------------------ 2. finalize on partials
def device_partials(p, nan_plane1=False):
    a = p.partial.copy()
    if nan_plane1:
        a[:, 1] = X.NAN
    return torch.from_numpy(np.concatenate([a.ravel(), nans(2 * a.shape[2])])).to(dev())       # a block too many reads NaN


@pytest.mark.parametrize('c', X.FIN_C)
@pytest.mark.parametrize('nblk', X.FIN_NBLK)
def test_col_finalize_sum_on_partials(nblk, c):
    p = X.partials_inputs(nblk, c)
    part = device_partials(p, nan_plane1=True)                  # FIN_ACC reads plane 0 only
    want = p.partial[:, 0].astype(np.float64).sum(0)
    for beta, old in ((0.0, None), (1.0, p.old)):
        out = fvec(nans(c) if old is None else old)
        call('tdg_col_finalize_sum', K().ptr(part), nblk, c, K().ptr(out), beta, K().stream())
        exact(vget(out, c), want if old is None else want + old, 'col_finalize_sum nblk=%d beta=%g' % (nblk, beta))


def check_stats(stats, st, dtype, what, const=None, mean_exact=False):
    """mean and rstd of one tensor against the float64 moments `st`; returns (mean, rstd) as read back."""
    c = len(st.mean)
    mean, rstd = stats[:c], stats[c:2 * c]
    if mean_exact:
        exact(mean, st.mean, what + ' mean')
    else:
        within(X.bound_ratio(mean, st.mean, X.mean_bound(st, dtype)), what + ' mean')
    want, lo, hi, amp = X.rstd_interval(st, dtype)
    within(X.interval_ratio(rstd, want, lo, hi), what + ' rstd (amplification up to %.3g)' % amp.max())
    if const is not None:
        assert X.ulps(rstd[const], RSTD_CLAMPED) <= 2, (rstd[const], RSTD_CLAMPED)
    return mean, rstd


def check_apply(u, mean, rstd, beta, act, dtype, pre, h, what):
    ref = X.bn_apply_ref(u, mean, rstd, beta, act, dtype)
    if pre is not None:
        within(X.bound_ratio(pre, ref.pre, ref.pre_bound), what + ' pre')
    within(X.bound_ratio(h, ref.h, ref.h_bound), what + ' h')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', X.FIN_C)
@pytest.mark.parametrize('nblk', X.FIN_NBLK)
def test_bn_fwd_from_partials(nblk, c, dtype):
    """Hand-made integer partials through the finalize and the apply: the mean is exact (64 rows), rstd lies in its
    interval, column 0 (negative variance by construction) is clamped to 1 / sqrt(eps); with the pivot null and given,
    with pre null, separate and == u."""
    p = X.partials_inputs(nblk, c)
    part = device_partials(p)
    s = p.partial.astype(np.float64).sum(0)
    rows, cs = X.FIN_ROWS, (c + 7) // 8 * 8
    lay = X.Layout(rows, c, cs)
    beta = torch.from_numpy(p.beta).to(dev())
    for pivot in (None, p.pivot):
        st = X.stats_from_sums(s[0], s[1], rows, 0.0 if pivot is None else pivot.astype(np.float64))
        pv = None if pivot is None else torch.from_numpy(np.concatenate([pivot, nans(8)])).to(dev())
        seen = {}
        for mode in ('null', 'separate', 'inplace'):
            u, h = Buf(lay, dtype, p.u), Buf(lay, dtype)
            pre = {'null': None, 'separate': Buf(lay, dtype), 'inplace': u}[mode]
            stats = fvec(nans(2 * c))
            call('tdg_bn_fwd_from_partials', dtype, u.ptr(), rows, c, cs, K().ptr(beta), X.EPS, X.ACT_LRELU, X.LEAK,
                 pre.ptr() if pre is not None else None, h.ptr(), cs, K().ptr(stats), K().ptr(part), nblk,
                 K().ptr(pv) if pv is not None else None, K().stream())
            what = '%s from_partials nblk=%d pivot=%s pre=%s' % (DT[dtype], nblk, pivot is not None, mode)
            got = vget(stats, 2 * c)
            mean, rstd = check_stats(got, st, dtype, what, mean_exact=True)
            assert X.ulps(rstd[0], RSTD_CLAMPED) <= 2, 'the clamp: rstd = %r, 1 / sqrt(eps) = %r' % (rstd[0], RSTD_CLAMPED)
            seen[mode] = (got, h.get(), pre.get() if pre is not None else None)
            check_apply(p.u, mean, rstd, p.beta, X.ACT_LRELU, dtype, seen[mode][2], seen[mode][1], what)
            if mode != 'inplace':
                u.get()                                             # (untouched, guards included)
        for mode in ('null', 'inplace'):
            exact(seen[mode][0], seen['separate'][0], 'stats, pre=%s against separate' % mode)
            exact(seen[mode][1], seen['separate'][1], 'h, pre=%s against separate' % mode)
        exact(seen['inplace'][2], seen['separate'][2], 'pre, in place against separate')


# ------------------------------------------------------------------------------------------------ 3. tdg_bn_fwd
def run_bn_fwd(k, dtype, act, mode, h_cs=None):
    """mode 'separate': three buffers; 'inplace': pre == u (engine.py: bn in place); 'aliased': u == pre == h."""
    inp = fwd_inputs(k)
    u = Buf(layout(k), dtype, inp.u)
    pre = Buf(layout(k), dtype) if mode == 'separate' else u
    h = u if mode == 'aliased' else Buf(layout(k, h_cs), dtype)
    stats = fvec(nans(2 * k.c))
    K().bn_fwd(workspace(), u.act(), k.c, torch.from_numpy(inp.beta).to(dev()), act, pre.act(), h.act(), stats, leak=X.LEAK, eps=X.EPS)
    hv = h.get()
    pv = pre.get() if mode != 'aliased' else None
    if mode == 'separate':
        u.get()
    return X.NS(stats=vget(stats, 2 * k.c), pre=pv, h=hv)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,act', CASE_ACTS, ids=CASE_ACT_IDS)
def test_bn_fwd(k, act, dtype):
    """Statistics against float64 moments (columns at 0, +-7 and +-200 around the pivot row, one constant column), the
    apply per element against the float64 formula at the device's own statistics, and the two aliased forms the engine
    runs bit-identical to separate buffers."""
    inp = fwd_inputs(k)
    what = '%s bn_fwd %s %s' % (DT[dtype], X.case_id(k), ACT_NAME[act])
    sep = run_bn_fwd(k, dtype, act, 'separate')
    const = X.const_column(k.c)
    mean, rstd = check_stats(sep.stats, inp.st, dtype, what, const=const)
    if const is not None:
        exact(sep.pre[:, const], np.broadcast_to(inp.beta[const], (k.rows,)), what + ': pre of the constant column == beta')
    if k.rows == 1:
        exact(sep.pre[0], inp.beta, what + ': one row, pre == beta')
    check_apply(inp.u, mean, rstd, inp.beta, act, dtype, sep.pre, sep.h, what)
    inplace = run_bn_fwd(k, dtype, act, 'inplace')
    exact(inplace.stats, sep.stats, what + ': stats, pre == u')
    exact(inplace.pre, sep.pre, what + ': pre, pre == u')
    exact(inplace.h, sep.h, what + ': h, pre == u')
    aliased = run_bn_fwd(k, dtype, act, 'aliased')
    exact(aliased.stats, sep.stats, what + ': stats, u == pre == h')
    exact(aliased.h, sep.h, what + ': h, u == pre == h')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('h_cs', [112, 101])
def test_bn_fwd_h_stride(h_cs, dtype):
    """h_cs != cs: 112 keeps the vector apply, 101 (h_cs % 4 != 0) forces the scalar one; separate and pre == u."""
    k = X.Case(96, 100, 104, 0)
    inp = fwd_inputs(k)
    for act in ALL_ACTS:
        what = '%s bn_fwd h_cs=%d %s' % (DT[dtype], h_cs, ACT_NAME[act])
        sep = run_bn_fwd(k, dtype, act, 'separate', h_cs)
        mean, rstd = check_stats(sep.stats, inp.st, dtype, what, const=X.const_column(k.c))
        check_apply(inp.u, mean, rstd, inp.beta, act, dtype, sep.pre, sep.h, what)
        inplace = run_bn_fwd(k, dtype, act, 'inplace', h_cs)
        exact(inplace.pre, sep.pre, what + ': pre, pre == u')
        exact(inplace.h, sep.h, what + ': h, pre == u')


GROUP_CASES = [(43, 3, 515, 515), (129, 2, 65, 65)]     # (rows per group, groups, c, cs): ragged row blocks, rows * cs odd


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gc', GROUP_CASES, ids=['%dx%d-g%d' % (g[0], g[2], g[1]) for g in GROUP_CASES])
def test_bn_fwd_groups_in_place(gc, dtype):
    rows, groups, c, cs = gc
    g = X.col_geometry(rows, c, cs, ES[dtype])
    assert (rows * cs) % 2 == 1 and 'ragged_last_block' in X.branches(g)
    parts = [X.bn_fwd_inputs(X.Case(rows, c, cs, 0), tag=30 + i) for i in range(groups)]
    beta = parts[0].beta
    lay = X.Layout(rows * groups, c, cs)
    u, h = Buf(lay, dtype, np.concatenate([p.u for p in parts])), Buf(lay, dtype)
    stats = fvec(nans(groups * 2 * c))
    K().bn_fwd_groups(workspace(), u.act(), c, torch.from_numpy(beta).to(dev()), X.ACT_LRELU, u.act(), h.act(), stats, rows, groups,
                      leak=X.LEAK, eps=X.EPS)
    got, pre, hv = vget(stats, groups * 2 * c), u.get(), h.get()
    for i, p in enumerate(parts):
        what = '%s bn_fwd_groups %dx%d group %d' % (DT[dtype], rows, c, i)
        mean, rstd = check_stats(got[i * 2 * c:(i + 1) * 2 * c], X.bn_stats_ref(p.u), dtype, what, const=X.const_column(c))
        sl = slice(i * rows, (i + 1) * rows)
        check_apply(p.u, mean, rstd, beta, X.ACT_LRELU, dtype, pre[sl], hv[sl], what)


# ------------------------------------------------------------------------------------------------ 4. tdg_bn_bwd
def run_bn_bwd(k, dtype, act, beta_acc, dbias_acc=None, dh_cs=None, dh_off=0, lead_rows=0):
    """One tdg_bn_bwd launch on the crafted inputs.  dh_cs / dh_off: dh is a channel slice of a wider tensor;
    lead_rows: the tensors are sub-batch windows that start `lead_rows` rows into their buffers (rows= and *_ptr=)."""
    inp = bwd_inputs(k)
    dh_cs = k.cs if dh_cs is None else dh_cs
    dh = Buf(X.Layout(k.rows, k.c, dh_cs, k.off + dh_off + lead_rows * dh_cs), dtype, inp.dh)
    pre = Buf(layout(k, lead_rows=lead_rows), dtype, inp.pre)
    du = Buf(layout(k, lead_rows=lead_rows), dtype)
    stats = fvec(np.concatenate([nans(k.c), inp.rstd]))                       # the mean half is not the backward's to read
    dbeta = fvec(inp.old_dbeta if beta_acc else nans(k.c))
    dbias = None if dbias_acc is None else fvec(inp.old_dbias if dbias_acc else nans(k.c))
    full = lambda b: K().Act(1, 1, 1, k.c, dtype, dev(), b.lay.cs, buf=b.t)    # noqa: E731  (the whole buffer: the window comes through rows= / *_ptr=)
    K().bn_bwd(workspace(), full(dh), full(pre), k.c, torch.from_numpy(inp.beta).to(dev()), stats, act, full(du), dbeta, rows=k.rows,
               leak=X.LEAK, beta_acc=float(beta_acc), dh_ptr=dh.ptr(), pre_ptr=pre.ptr(), du_ptr=du.ptr(), dbias=dbias,
               dbias_acc=float(dbias_acc or 0))
    dh.get(), pre.get(), vget(stats, 2 * k.c)
    return X.NS(du=du.get(), dbeta=vget(dbeta, k.c), dbias=None if dbias is None else vget(dbias, k.c))


def check_bn_bwd(k, dtype, act, r0, what):
    """du and dbeta (beta_acc = 0) of one launch against the oracle: exact where provable, else the derived bound."""
    inp = bwd_inputs(k)
    ref = X.bn_bwd_ref(inp, act, dtype)
    if act == X.ACT_TANH:
        within(X.bound_ratio(r0.dbeta, ref.s0, ref.dbeta_bound), what + ' dbeta')
    else:
        exact(r0.dbeta, ref.s0, what + ' dbeta')
    if act != X.ACT_TANH and k.rows in X.DU_EXACT_ROWS:
        exact(r0.du, X.store(ref.du, dtype), what + ' du')
    else:
        within(X.bound_ratio(r0.du, ref.du, ref.du_bound), what + ' du')
    return ref


def check_dbias(inp, rb, r0, acc, what):
    exact(rb.du, r0.du, what + ': du with dbias')
    exact(rb.dbeta, r0.dbeta, what + ': dbeta with dbias')
    stored = rb.du.astype(np.float64)
    want = stored.sum(0) + (inp.old_dbias.astype(np.float64) if acc else 0.0)
    within(X.bound_ratio(rb.dbias, want, X.dbias_bound(stored)), what + ' dbias (dbias_acc=%d)' % acc)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,act', CASE_ACTS, ids=CASE_ACT_IDS)
def test_bn_bwd(k, act, dtype):
    """Independent of the forward: crafted dh in {-1, 0, 1}, quarter-integer pre / beta (pre == beta and pre == 0 entries in
    every column), rstd in {0.5, 1, 2}."""
    inp = bwd_inputs(k)
    what = '%s bn_bwd %s %s' % (DT[dtype], X.case_id(k), ACT_NAME[act])
    r0 = run_bn_bwd(k, dtype, act, 0)
    ref = check_bn_bwd(k, dtype, act, r0, what)
    r1 = run_bn_bwd(k, dtype, act, 1)
    exact(r1.du, r0.du, what + ': du, beta_acc = 1')
    want = ref.s0 + inp.old_dbeta.astype(np.float64)
    if act == X.ACT_TANH:
        within(X.bound_ratio(r1.dbeta, want, ref.dbeta_bound + X.U32 * (np.abs(want) + ref.dbeta_bound)), what + ' dbeta, beta_acc = 1')
    else:
        exact(r1.dbeta, want, what + ' dbeta, beta_acc = 1')
    for acc in (0, 1):
        check_dbias(inp, run_bn_bwd(k, dtype, act, 0, dbias_acc=acc), r0, acc, what)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bn_bwd_slice_and_window(dtype):
    """dh as a channel slice of a wider tensor (dh_cs != cs: 232 keeps the vector kernels, 233 forces the scalar ones),
    and all three tensors as sub-batch windows 5 rows into their buffers: nothing in front of a window changes."""
    k = X.Case(96, 100, 104, 0)
    inp = bwd_inputs(k)
    for act in (X.ACT_LRELU, X.ACT_TANH):
        plain = run_bn_bwd(k, dtype, act, 0)
        for name, kw in (('dh_cs=232', dict(dh_cs=232, dh_off=8)), ('dh_cs=233', dict(dh_cs=233, dh_off=8)), ('window', dict(lead_rows=5)),
                         ('window of a slice', dict(dh_cs=232, dh_off=8, lead_rows=5))):
            what = '%s bn_bwd %s %s' % (DT[dtype], name, ACT_NAME[act])
            r = run_bn_bwd(k, dtype, act, 0, **kw)
            check_bn_bwd(k, dtype, act, r, what)
            if name != 'dh_cs=233':                                     # the same kernels on other addresses
                exact(r.du, plain.du, what + ': du against the plain layout')
                exact(r.dbeta, plain.dbeta, what + ': dbeta against the plain layout')
            check_dbias(inp, run_bn_bwd(k, dtype, act, 0, dbias_acc=1, **kw), r, 1, what)


# ------------------------------------------------------------------------------------------------ 5. sumsq
def guarded_flat(x, off, dtype, tail=16):
    t = torch.from_numpy(np.concatenate([nans(off), x, nans(tail)])).to(dev()).to(K().TORCH_DTYPE[dtype])
    return t, K().ptr(t, off * ES[dtype])


def gp_sumsq(dtype, ptr, n, ss, scal, lam=10.0):
    w = workspace().ensure(4096)
    call('tdg_gp_sumsq', dtype, ptr, n, K().ptr(ss), lam, K().ptr(scal), K().ptr(w), w.numel(), K().stream())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('which', range(6))
def test_sumsq_exact(which, off, dtype):
    """Values in {-1, 0, 1}: the 16-byte path with its scalar tail (aligned base) and the scalar path (base one element off)."""
    n = X.sumsq_sizes(dtype)[which]
    x = X.tern(n, 5)
    want = float((x.astype(np.float64) ** 2).sum())
    t, p = guarded_flat(x, off, dtype)
    for beta, old in ((0.0, X.NAN), (1.0, 5.0)):
        acc = fvec([old])
        K().sumsq(workspace(), dtype, p, n, acc, beta=beta)
        exact(vget(acc, 1), np.array([want + (old if beta else 0.0)]), 'sumsq n=%d off=%d beta=%g' % (n, off, beta))
    ss, scal = fvec(nans(1)), fvec(nans(2))
    gp_sumsq(dtype, p, n, ss, scal)
    exact(vget(ss, 1), np.array([want]), 'gp_sumsq n=%d off=%d' % (n, off))
    vget(scal, 2)


@pytest.mark.parametrize('dtype', DTYPES)
def test_sumsq_ticket_cleans_itself_and_order_is_fixed(dtype):
    """Three launches back to back on one stream, different sizes, no synchronisation in between: each exact (a ticket
    that is not reset would make the second launch finish early or never).  Random data twice: identical bits."""
    sizes = X.sumsq_sizes(dtype)
    runs = []
    for i, n in enumerate((sizes[5], sizes[1], sizes[3])):
        x = X.tern(n, 6 + i)
        t, p = guarded_flat(x, 0, dtype)
        runs.append((n, x, t, p, fvec(nans(1)), fvec(nans(2))))
    torch.cuda.synchronize()
    K().sumsq(workspace(), dtype, runs[0][3], runs[0][0], runs[0][4])
    gp_sumsq(dtype, runs[1][3], runs[1][0], runs[1][4], runs[1][5])
    K().sumsq(workspace(), dtype, runs[2][3], runs[2][0], runs[2][4])
    for n, x, t, p, acc, _ in runs:
        exact(vget(acc, 1), np.array([(x.astype(np.float64) ** 2).sum()]), 'back-to-back sumsq n=%d' % n)
    n = sizes[5]
    x = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    t, p = guarded_flat(x, 0, dtype)
    a, b = fvec(nans(1)), fvec(nans(1))
    K().sumsq(workspace(), dtype, p, n, a)
    K().sumsq(workspace(), dtype, p, n, b)
    assert torch.equal(a, b) and np.isfinite(vget(a, 1)).all()
    xs = t.float().cpu().numpy()[:n].astype(np.float64)
    within(np.abs(vget(a, 1) - (xs ** 2).sum()) / (X.gamma(n, X.U32) * (xs ** 2).sum()), '%s sumsq random n=%d' % (DT[dtype], n))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('root', X.GP_ROOTS)
def test_gp_sumsq_scalars(root, dtype):
    """n = root**2 values of +-1: sqrt(sum) is the integer `root`, so scal = ((root - 1)^2, lambda 2 (root - 1) / root) up to the
    roundings of the products and the division: 4 ulp."""
    n = root * root
    x = np.where(X.tern(n, 8) < 0, -1.0, 1.0).astype(np.float32)
    t, p = guarded_flat(x, 0, dtype)
    ss, scal = fvec(nans(1)), fvec(nans(2))
    gp_sumsq(dtype, p, n, ss, scal, lam=10.0)
    exact(vget(ss, 1), np.array([float(n)]), 'gp_sumsq sum')
    u = X.ulps(vget(scal, 2), X.gp_scalars_ref(n, 10.0))
    print('RATIO gp scalars, ulps of 4: %.3g' % (u.max() / 4))
    assert u.max() <= 4, u


# ------------------------------------------------------------------------------------------------ 6. f32 sums and means
@pytest.mark.parametrize('n', X.SEG_LENGTHS)
def test_sum_mean_and_segment_means(n):
    x = X._ints(np.random.default_rng([10, n]), -3, 3, 3 * n)
    t = torch.from_numpy(np.concatenate([x, nans(16)])).to(dev())
    x64 = x.astype(np.float64)
    pow2 = n & (n - 1) == 0
    for beta, old in ((0.0, X.NAN), (1.0, 7.0)):
        out = fvec([old])
        call('tdg_sum_f32', K().ptr(t), n, K().ptr(out), beta, K().stream())
        exact(vget(out, 1), np.array([x64[:n].sum() + (old if beta else 0.0)]), 'sum_f32 n=%d beta=%g' % (n, beta))
    out = fvec(nans(1))
    call('tdg_mean_f32', K().ptr(t), n, K().ptr(out), K().stream())
    seg = fvec(nans(3))
    call('tdg_mean_segments_f32', K().ptr(t), 3, n, K().ptr(seg), K().stream())
    for got, want, what in ((vget(out, 1), np.array([x64[:n].mean()]), 'mean_f32'), (vget(seg, 3), x64.reshape(3, n).mean(1), 'mean_segments_f32')):
        if pow2:
            exact(got, want, '%s n=%d' % (what, n))
        else:
            u = np.where(got == want, 0.0, X.ulps(got, want))
            print('RATIO %s n=%d, ulps of 1: %.3g' % (what, n, u.max()))
            assert u.max() <= 1, (what, got, want)


# ------------------------------------------------------------------------------------------------ 7. row ops
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('shape', X.ROW_SHAPES, ids=['%dx%d' % s for s in X.ROW_SHAPES])
def test_rowdot_and_rowouter(shape, off, dtype):
    """Integers: rowdot with bias and ACT_NONE, rowouter with MASK_NONE and MASK_LRELU at leak 0.25 (mask source with exact
    zeros); aligned and one-element-off bases; nothing lands past rows * cols."""
    rows, cols = shape
    inp = X.row_inputs(rows, cols)
    lay = X.Layout(rows, cols, cols, off)
    w = torch.from_numpy(np.concatenate([inp.w, nans(16)])).to(dev())
    bias = torch.from_numpy(inp.bias).to(dev())
    x = Buf(lay, dtype, inp.x)
    out = fvec(nans(rows))
    call('tdg_rowdot', dtype, x.ptr(), rows, cols, K().ptr(w), K().ptr(bias), X.ACT_NONE, K().ptr(out), K().stream())
    exact(vget(out, rows), X.rowdot_ref(inp), 'rowdot %dx%d off=%d' % (rows, cols, off))
    dout = torch.from_numpy(np.concatenate([inp.dout, nans(8)])).to(dev())
    mask = Buf(lay, dtype, inp.mask)
    for mode, masked in ((K().MASK_NONE, False), (K().MASK_LRELU, True)):
        dx = Buf(lay, dtype)
        call('tdg_rowouter', dtype, K().ptr(dout), K().ptr(w), rows, cols, mode, X.LEAK, mask.ptr() if masked else None, dx.ptr(), K().stream())
        exact(dx.get(), X.store(X.rowouter_ref(inp, masked), dtype), 'rowouter %dx%d off=%d masked=%s' % (rows, cols, off, masked))
    x.get(), mask.get()


# ------------------------------------------------------------------------------------------------ 8. instance norm
IN_CASE_ACTS = [(k, a) for k in X.IN_CASES for a in X.IN_ACTS]
IN_CASE_ACT_IDS = ['%s-%s' % (X.in_id(k), ACT_NAME[a]) for k, a in IN_CASE_ACTS]
RSQRT_ULP = 2                                           # tests/_exact_pointwise.py (OpenCL 1.2 full profile)


@functools.lru_cache(maxsize=2)
def in_inputs(k):
    inp = X.in_inputs(k)
    inp.st = X.in_stats_ref(inp.u)
    return inp


def run_instance_norm(k, dtype, act, beta):
    """tdg_instance_norm_fwd, then tdg_instance_norm_bwd on the statistics it left.  cs, h_cs and dh_cs all differ and lie
    above c: u and dh are NaN in their padding channels, h and du keep the sentinel there; scale, shift, stats and the
    workspace are followed by guards."""
    n, hw, c = k
    inp = in_inputs(k)
    cs, h_cs, dh_cs = X.in_strides(c)
    rows = n * hw
    u, dh = Buf(X.Layout(rows, c, cs), dtype, inp.u.reshape(rows, c)), Buf(X.Layout(rows, c, dh_cs), dtype, inp.dh.reshape(rows, c))
    h, du = Buf(X.Layout(rows, c, h_cs), dtype), Buf(X.Layout(rows, c, cs), dtype)
    scale, shift = (torch.from_numpy(np.concatenate([v, nans(8)])).to(dev()) for v in (inp.scale, inp.shift))
    stats, ws = fvec(nans(n * 2 * c)), fvec(nans(n * 2 * c))
    call('tdg_instance_norm_fwd', dtype, u.ptr(), n, hw, c, cs, K().ptr(scale), K().ptr(shift), X.EPS, act, X.LEAK, h.ptr(), h_cs,
         K().ptr(stats), K().stream())
    dscale, dshift = fvec(inp.old_dscale if beta else nans(c)), fvec(inp.old_dshift if beta else nans(c))
    call('tdg_instance_norm_bwd', dtype, dh.ptr(), dh_cs, u.ptr(), n, hw, c, cs, K().ptr(scale), K().ptr(shift), K().ptr(stats), act,
         X.LEAK, du.ptr(), K().ptr(dscale), K().ptr(dshift), beta, K().ptr(ws), n * 2 * c * 4, K().stream())
    st = vget(stats, n * 2 * c).reshape(n, 2, c)
    vget(ws, n * 2 * c), u.get(), dh.get()
    return dict(mu=st[:, 0].copy(), rstd=st[:, 1].copy(), h=h.get().reshape(n, hw, c), du=du.get().reshape(n, hw, c),
                dscale=vget(dscale, c), dshift=vget(dshift, c))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,act', IN_CASE_ACTS, ids=IN_CASE_ACT_IDS)
def test_instance_norm(k, act, dtype):
    """Statistics against float64 moments (mu exact at power-of-two hw, rstd in its f32-path interval, a constant column at
    1 / sqrt(eps), a column whose pivot is a +-200 outlier), then h, du and dscale per element against the float64 formulas at
    the device's own statistics and dshift exactly (none / relu / lrelu on eighths), with beta 0 and 1; no pre of the table
    lies within its bound of the relu / lrelu kink; two launches are bit-equal."""
    n, hw, c = k
    inp = in_inputs(k)
    what = '%s instance_norm %s %s' % (DT[dtype], X.in_id(k), ACT_NAME[act])
    a, b = run_instance_norm(k, dtype, act, 0.0), run_instance_norm(k, dtype, act, 0.0)
    for name in a:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), '%s: %s differs between two launches' % (what, name)
    mu, rstd = a['mu'], a['rstd']
    if hw & (hw - 1) == 0:
        exact(mu, inp.st.mean, what + ' mu')
    else:
        within(X.bound_ratio(mu, *X.in_mu_ref(inp.st)), what + ' mu')
    want, lo, hi, amp = X.in_rstd_interval(inp.st, X.EPS)
    within(X.interval_ratio(rstd, want, lo, hi), what + ' rstd (amplification up to %.3g)' % amp.max())
    const = X.const_column(c)
    if const is not None:
        assert np.all(inp.st.var[:, const] == 0) and np.all(X.ulps(rstd[:, const], RSTD_CLAMPED) <= RSQRT_ULP), rstd[:, const]
        assert np.all(np.abs(inp.u[:, 0, X.in_outlier_column(c)]) == X.IN_OUTLIER)
    within(X.bound_ratio(a['h'], *X.in_apply_ref(inp, mu, rstd, act, dtype)), what + ' h')
    ref = X.in_bwd_ref(inp, mu, rstd, act, dtype, 0.0)
    if act in (X.ACT_RELU, X.ACT_LRELU):
        assert ref.kink > 0, '%s: an element of pre lies within its bound of 0 (margin %g)' % (what, ref.kink)
    if hw == 1:
        exact(a['du'], np.zeros((n, hw, c)), what + ' du at hw 1')
        if act != X.ACT_TANH:
            exact(a['h'], np.broadcast_to(X.store(X.act_ref(inp.shift.astype(np.float64), act), dtype), (n, hw, c)), what + ' h == act(shift)')
    c1 = run_instance_norm(k, dtype, act, 1.0)
    exact(c1['du'], a['du'], what + ': du, beta = 1')
    ref1 = X.in_bwd_ref(inp, mu, rstd, act, dtype, 1.0)
    for r, got, beta in ((ref, a, 0), (ref1, c1, 1)):
        within(X.bound_ratio(got['du'], r.du, r.du_bound), what + ' du')
        within(X.bound_ratio(got['dscale'], r.dscale, r.dscale_bound), what + ' dscale, beta = %d' % beta)
        if act == X.ACT_TANH:
            within(X.bound_ratio(got['dshift'], r.dshift, r.dshift_bound), what + ' dshift, beta = %d' % beta)
        else:
            exact(got['dshift'], r.dshift, what + ' dshift, beta = %d' % beta)
