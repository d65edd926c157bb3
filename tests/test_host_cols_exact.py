"""The recipe of tests/_exact_cols.py checked on the CPU with oracle arithmetic only: the caps hold for every case
tests/test_gpu_cols_exact.py runs (so that file never skips or weakens one), the case table reaches every geometry branch
of col_geom() for both element sizes, the generators are deterministic, the pivot earns its place, and NumPy
restatements of the reductions are accepted clean and rejected with one deliberate defect each."""
import numpy as np
import pytest

from conftest import pkg
import _exact_cols as X

IDS = [X.case_id(k) for k in X.TABLE]


def test_constants_match_the_library():
    L = pkg('_lib')
    assert (X.ACT_NONE, X.ACT_RELU, X.ACT_LRELU, X.ACT_TANH) == (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH)
    # a bf16 store keeps 8 significant bits: 1 + 2**-8 is stored as 1, an error of 2**-8 |x| = half a bf16 ulp there
    x = np.float32([1 + 2.0 ** -8, 2 - 2.0 ** -8, 3.0, 0.0])
    assert np.array_equal(np.abs(X.bf16_round(x).astype(np.float64) - x), [2.0 ** -8, 2.0 ** -8, 0, 0])
    assert np.array_equal(X.bf16_half_ulp(x), [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0]) and 2.0 ** -8 > 2.0 ** -9 * x[0]
    assert X.LEAK == 0.25 and X.bf16_round(np.float32([1.00390625, 1.01171875, 257.0, -0.3])).tolist() == [1.0, 1.015625, 256.0, -0.30078125]


@pytest.mark.parametrize('elem_size', [4, 2])
def test_table_reaches_every_geometry_branch(elem_size):
    missing = X.missing_branches(X.TABLE, elem_size)
    assert not missing, 'no case of the table takes: %s' % ', '.join(missing)
    # the entries that are in the table for one branch still take it
    want = {(1100, 2048): 'cap32', (65600, 65): 'cap512', (140000, 3): 'cap1024', (131072, 4): 'nblk>=1024', (40, 515): 'ncol>=8',
            (64, 260): 'ncol2-7:one_live_lane', (33, 2052): 'ragged_last_block', (70, 12): 'vw1:cs%4'}
    for k in X.TABLE:
        b = X.branches(X.geometry_of(k, elem_size))
        if (k.rows, k.c) in want and k.off == 0:
            assert want[(k.rows, k.c)] in b, (k, sorted(b))
        if k.off:
            assert 'vw1:pointer' in b
    assert max(k.rows * k.cs for k in X.TABLE) * 4 < 20e6


def test_geometry_restatement_invariants():
    """Every row belongs to exactly one block and every channel to exactly one lane, whatever the shape."""
    rng = np.random.default_rng(0)
    for _ in range(2000):
        rows, c = int(rng.integers(1, 200000)), int(rng.integers(1, 3000))
        cs = c + int(rng.integers(0, 9))
        g = X.col_geometry(rows, c, cs, 4, aligned=bool(rng.integers(0, 2)))
        assert (g.nblk - 1) * g.rows_per_blk < rows <= g.nblk * g.rows_per_blk and 1 <= g.nblk <= 1024
        assert (g.ncol - 1) * g.CL * g.vw < c <= g.ncol * g.CL * g.vw and 1 <= g.live_last_chunk <= g.CL


@pytest.mark.parametrize('k', X.TABLE, ids=IDS)
def test_caps_hold_for_every_case(k):
    X.colsum_caps(X.colsum_inputs(k))
    f = X.bn_fwd_inputs(k)
    X.bn_fwd_caps(f)
    assert np.array_equal(X.bf16_round(f.u), f.u) and np.array_equal(X.bf16_round(f.beta), f.beta)
    b = X.bn_bwd_inputs(k)
    for act in (X.ACT_NONE, X.ACT_RELU, X.ACT_LRELU):
        X.bn_bwd_caps(b, act)
        # dbeta = beta_acc * old + s0 stays on the quarter grid
        r = X.bn_bwd_ref(b, act, 1)
        assert X.fits_f32(r.s0 + b.old_dbeta) and X.fits_f32(r.s0)
        assert X.du_intermediates_fit(b, act) == (k.rows in X.DU_EXACT_ROWS), (k, act)
    assert np.all((b.pre == b.beta[None, :]).any(0)) and (k.rows == 1 or np.all((b.pre == 0).sum(0) >= 1))
    # rows == 1: pre == beta, so du is exactly 0 and dbias == dbias_acc * old needs no rounding
    if k.rows == 1:
        assert np.all(X.bn_bwd_ref(b, X.ACT_LRELU, 0).du == 0)


@pytest.mark.parametrize('nblk', X.FIN_NBLK)
def test_caps_hold_for_the_hand_made_partials(nblk):
    for c in X.FIN_C:
        p = X.partials_inputs(nblk, c)
        X.partials_caps(p)
        s = p.partial.astype(np.float64).sum(0)
        st = X.stats_from_sums(s[0], s[1], X.FIN_ROWS, p.pivot.astype(np.float64))
        assert st.var[0] == -3.0 and np.all(st.var[1:] >= 1.0)
        assert X.fits_f32(st.mean) and X.fits_f32(st.md)          # the mean is exact: rows is a power of two


def test_caps_hold_for_the_scalar_and_row_cases():
    for dtype in (0, 1):
        assert max(X.sumsq_sizes(dtype)) < X.F32_CAP
    assert max(X.GP_ROOTS) ** 2 < X.F32_CAP and max(X.SEG_LENGTHS) * 3 < X.F32_CAP
    for rows, cols in X.ROW_SHAPES:
        X.row_caps(X.row_inputs(rows, cols))
    assert any((X.row_inputs(r, c).mask == 0).any() for r, c in X.ROW_SHAPES)


def test_generators_are_deterministic():
    k = X.TABLE[2]
    for gen in (X.colsum_inputs, X.bn_fwd_inputs, X.bn_bwd_inputs):
        a, b = vars(gen(k)), vars(gen(k))
        assert all(np.array_equal(a[n], b[n]) for n in a)
    a, b = vars(X.partials_inputs(33, 9)), vars(X.partials_inputs(33, 9))
    assert all(np.array_equal(a[n], b[n]) for n in a)
    a, b = vars(X.row_inputs(3, 1028)), vars(X.row_inputs(3, 1028))
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert np.array_equal(X.tern(1000, 5), X.tern(1000, 5))


# ------------------------------------------------------------------------------------------------ the pivot
def _stats_restated(k, acc, defect=None):
    inp = X.bn_fwd_inputs(k)
    lay = X.Layout(k.rows, k.c, k.cs, k.off)
    flat = lay.pack(inp.u)
    g = X.geometry_of(k, 2)
    part = X.restate_col_partial(flat, lay, g, 'stats', acc, defect=defect)
    pivot = np.zeros(k.c, np.float32) if defect == 'no_pivot' else inp.u[0]
    return inp, X.restate_finalize_stats(part, k.rows, pivot, acc)


def _stats_ratios(inp, mean, rstd, dtype):
    st = X.bn_stats_ref(inp.u)
    want, lo, hi, amp = X.rstd_interval(st, dtype)
    return X.bound_ratio(mean, st.mean, X.mean_bound(st, dtype)), X.interval_ratio(rstd, want, lo, hi), amp


@pytest.mark.parametrize('k', [k for k in X.TABLE if k.c >= 5 and k.rows * k.c <= 300000], ids=lambda k: X.case_id(k))
def test_pivotless_float32_statistics_fail_the_bound_on_the_200_columns(k):
    """What the +-200 columns are for.  The float32 restatement of the statistics (the accumulator type of bf16 tensors)
    holds the derived bounds on every column with the pivot; without it the raw second moment of a +-200 column is
    ~4e4 against a variance of ~4, the cancellation costs ~1e4 * 2**-24 relative, and the rstd of most +-200 columns
    leaves the interval by orders of magnitude (a few land inside by the luck of their roundings)."""
    inp, (mean, rstd) = _stats_restated(k, np.float32)
    rm, rr, amp = _stats_ratios(inp, mean, rstd, 1)
    assert rm.max() <= 1 and rr.max() <= 1, (rm.max(), rr.max())
    inp, (mean, rstd) = _stats_restated(k, np.float32, 'no_pivot')
    rm, rr, _ = _stats_ratios(inp, mean, rstd, 1)
    far = np.abs(inp.base) == 200
    const = X.const_column(k.c)
    if const is not None:
        far[const] = False                      # (a constant column has no variance to lose)
    assert far.any() and np.mean(rr[far] > 1) > 0.5 and rr[far].max() > 100, (np.mean(rr[far] > 1), rr[far].max())
    print('%s: pivot-less f32 rstd ratio on the +-200 columns: min %.3g max %.3g' % (X.case_id(k), rr[far].min(), rr[far].max()))


# ------------------------------------------------------------------------------------------------ mutation check
RAGGED = X.Case(33, 2052, 2052, 0)
PADDED = X.Case(130, 7, 8, 0)


@pytest.mark.parametrize('acc', [np.float32, np.float64])
def test_restated_column_sums_clean_and_with_defects(acc):
    for k in (RAGGED, PADDED, X.Case(96, 100, 104, 1)):
        inp = X.colsum_inputs(k)
        lay = X.Layout(k.rows, k.c, k.cs, k.off)
        flat = lay.pack(inp.x)
        g = X.geometry_of(k, 4)
        for coef in (None, inp.coef):
            want = X.colsum_ref(inp.x, coef, inp.old)
            got = X.restate_finalize_sum(X.restate_col_partial(flat, lay, g, 'wsum', acc, coef=coef), acc, inp.old)
            assert np.array_equal(got, want), X.describe_mismatch(got, want)
    inp = X.colsum_inputs(RAGGED)
    lay = X.Layout(*RAGGED)
    g = X.geometry_of(RAGGED, 4)
    assert 'ragged_last_block' in X.branches(g)
    got = X.restate_finalize_sum(X.restate_col_partial(lay.pack(inp.x), lay, g, 'sum', acc, defect='drop_last_row'), acc)
    assert not np.array_equal(got, X.colsum_ref(inp.x))
    inp = X.colsum_inputs(PADDED)
    lay = X.Layout(*PADDED)
    got = X.restate_finalize_sum(X.restate_col_partial(lay.pack(inp.x), lay, X.geometry_of(PADDED, 4), 'sum', acc, defect='pad_read'), acc)
    assert np.isnan(got[-1]) and not np.array_equal(got, X.colsum_ref(inp.x))


def test_restated_statistics_clean_and_with_defects():
    for defect, k in ((None, RAGGED), ('drop_last_row', RAGGED), ('pad_read', PADDED)):
        inp, (mean, rstd) = _stats_restated(k, np.float32, defect)
        rm, rr, _ = _stats_ratios(inp, mean, rstd, 1)
        const = X.const_column(k.c)
        live = np.arange(k.c) != const
        if defect is None:
            assert rm.max() <= 1 and rr.max() <= 1
            assert X.ulps(rstd[const], 1 / np.sqrt(np.float64(np.float32(X.EPS)))) <= 2
        elif defect == 'drop_last_row':
            assert np.mean(np.maximum(rm, rr)[live] > 1) > 0.5  # one row of 33 moves a column's moments unless its d is 0 there
        else:
            assert np.isinf(rm[-1]) and np.isinf(rr[-1])        # the NaN padding poisons the last column


def test_restated_finalize_clamp():
    """The hand-made negative variance: with the clamp rstd is 1 / sqrt(eps) within 2 ulp, without it the test's
    comparison rejects the result (sqrt of a negative number)."""
    p = X.partials_inputs(33, 9)
    want = 1 / np.sqrt(np.float64(np.float32(X.EPS)))
    for acc in (np.float32, np.float64):
        _, rstd = X.restate_finalize_stats(p.partial, X.FIN_ROWS, p.pivot, acc)
        assert X.ulps(rstd[0], want) <= 2
        _, rstd = X.restate_finalize_stats(p.partial, X.FIN_ROWS, p.pivot, acc, defect='no_clamp')
        assert not X.ulps(rstd[0], want) <= 2


@pytest.mark.parametrize('act', [X.ACT_NONE, X.ACT_RELU, X.ACT_LRELU])
def test_restated_bn_bwd_sums_clean_and_with_defects(act):
    for defect, k in ((None, RAGGED), ('drop_last_row', RAGGED), (None, PADDED), ('pad_read', PADDED)):
        inp = X.bn_bwd_inputs(k)
        lay = X.Layout(k.rows, k.c, k.cs, k.off)
        part = X.restate_col_partial(lay.pack(inp.dh), lay, X.geometry_of(k, 2), 'bwd', np.float32, defect=defect,
                                     pre_flat=lay.pack(inp.pre), beta=inp.beta, act=act)
        r = X.bn_bwd_ref(inp, act, 1)
        s0 = part[:, 0].sum(0, dtype=np.float32)
        s1 = part[:, 1].sum(0, dtype=np.float32)
        same = np.array_equal(s0, r.s0) and np.array_equal(s1, r.s1)
        assert same == (defect is None), (defect, k)


def test_restated_scalar_and_row_reductions_with_defects():
    for dtype, vw in ((0, 4), (1, 8)):
        n = 256 * vw - 1
        x = X.tern(n, 5)
        want = (x.astype(np.float64) ** 2).sum()
        assert X.restate_sumsq(x, vw) == want
        assert np.any(x[n // vw * vw:] != 0) and X.restate_sumsq(x, vw, 'drop_tail') != want
    inp = X.row_inputs(3, 1028)
    assert np.array_equal(X.restate_rowdot(inp.x, inp.w, inp.bias), X.rowdot_ref(inp))
    assert not np.array_equal(X.restate_rowdot(inp.x, inp.w, inp.bias, 'drop_last_col'), X.rowdot_ref(inp))


# ------------------------------------------------------------------------------------------------ instance norm
IN_IDS = [X.in_id(k) for k in X.IN_CASES]


def test_instance_norm_constants():
    import _exact_pointwise as P
    # OpenCL 1.2 section 7.4, full profile, single precision: rsqrt <= 2 ulp, beside the limits already taken from that table
    assert (P.RSQRT_ULP, P.SQRT_ULP, P.DIV_ULP) == (2, 3, 2.5)
    r = P.ev_rsqrt(P.Ev(np.array([4.0]), np.array([0.0])))
    assert r.v[0] == 0.5 and 0 < r.e[0] <= 2.0 ** -23


@pytest.mark.parametrize('k', X.IN_CASES, ids=IN_IDS)
def test_instance_norm_table_conditions(k):
    """The sums the bounds take as exact are exact (integers below 2**24), mu is representable at power-of-two hw, the
    constant column has variance 0, the outlier column's pivot is +-200, strides lie above c -- and the kink condition:
    in float64, with everything the statistics' own intervals can move, no pre of any case lies within its bound of 0."""
    n, hw, c = k
    inp = X.in_inputs(k)
    X.in_caps(inp)
    st = X.in_stats_ref(inp.u)
    assert np.array_equal(st.s0, np.rint(st.s0)) and np.array_equal(st.s1, np.rint(st.s1))
    if hw & (hw - 1) == 0:
        assert X.fits_f32(st.mean) and X.fits_f32(st.md) and np.all(X.in_mu_ref(st)[0] == st.mean)
    if X.const_column(c) is not None:
        assert np.all(st.var[:, X.const_column(c)] == 0) and np.all(np.abs(inp.u[:, 0, X.in_outlier_column(c)]) == X.IN_OUTLIER)
        assert np.all(st.var[:, X.in_outlier_column(c)] > 100)
    assert min(X.in_strides(c)) > c and len(set(X.in_strides(c))) == 3
    assert np.all(inp.shift != 0) and np.all(inp.scale != 0)
    margin = X.in_kink_margin(inp, X.EPS)
    assert margin > 0, margin
    if hw == 1:
        assert np.all(st.var == 0) and np.all(st.mean == inp.u[:, 0])
    a, b = vars(X.in_inputs(k)), vars(X.in_inputs(k))
    assert all(np.array_equal(a[name], b[name]) for name in a)


@pytest.mark.parametrize('k', X.IN_CASES, ids=IN_IDS)
def test_instance_norm_restated_clean_and_with_defects(k):
    """The f32 restatement of the statistics holds the mu bound and the rstd interval on every column, the outlier column
    included (there the pivot is the outlier: every deviation is ~200 and the amplification is the table's largest).
    Without the pivot it is the columns that sit at +-200 whose rstd leaves the interval (at hw 5 and 64; at hw 4 and 16 every
    intermediate of the raw moments is still representable); the outlier column alone is not hurt by raw moments, since
    all its other values are small.  dscale and dshift swapped are rejected.  The unclamped
    variance cannot be exposed by a tensor: with exact sums a column's f32 variance is negative only if its true variance
    is below a rounding of its second moment, and deviations from the column's own first value cannot have that shape
    (a constant column gives 0 - 0) -- so that defect is rejected on hand-made sums (md = 2, E[d^2] = 1)."""
    n, hw, c = k
    inp = X.in_inputs(k)
    st = X.in_stats_ref(inp.u)
    want, lo, hi, amp = X.in_rstd_interval(st, X.EPS)
    muv, mue = X.in_mu_ref(st)
    mu, rstd = X.restate_in_stats(inp.u, X.EPS)
    assert X.bound_ratio(mu, muv, mue).max() <= 1 and X.interval_ratio(rstd, want, lo, hi).max() <= 1
    same, _ = X.restate_in_stats(inp.u, X.EPS, 'no_clamp')
    assert np.array_equal(same, mu)
    if c >= 6 and hw > 1:
        assert amp[:, X.in_outlier_column(c)].min() == amp.max() or amp[:, X.in_outlier_column(c)].min() > 0.5 * amp.max()
        _, bad = X.restate_in_stats(inp.u, X.EPS, 'no_pivot')
        r = X.interval_ratio(bad, want, lo, hi)
        far = np.array([abs(X.BASES[j % 5]) == 200 and j not in (X.const_column(c), X.in_outlier_column(c)) for j in range(c)])
        if hw & (hw - 1) or hw >= 64:
            assert far.any() and np.mean(r[:, far] > 1) > 0.5 and r[:, far].max() > 100, (np.mean(r[:, far] > 1), r[:, far].max())
        else:                                           # hw 4 and 16 on integers: s / hw and md * md are exact, raw moments lose nothing
            assert far.any() and r.max() <= 1
    for act in (X.ACT_NONE, X.ACT_RELU, X.ACT_LRELU, X.ACT_TANH):
        ref = X.in_bwd_ref(inp, mu, rstd, act, 1, 0.0)
        accepts = lambda ds, dsh: (X.bound_ratio(ds, ref.dscale, ref.dscale_bound).max() <= 1 and                    # noqa: E731
                                   (X.bound_ratio(dsh, ref.dshift, ref.dshift_bound).max() <= 1 if act == X.ACT_TANH
                                    else np.array_equal(dsh, ref.dshift)))
        assert accepts(*X.restate_in_bwd_sums(inp, mu, rstd, act)), act
        if hw > 1:
            assert not accepts(*X.restate_in_bwd_sums(inp, mu, rstd, act, 'swapped')), act
        hv, hb = X.in_apply_ref(inp, mu, rstd, act, 0)
        assert np.all(np.isfinite(hv)) and np.all(hb >= 0) and (act not in (X.ACT_RELU, X.ACT_LRELU) or ref.kink > 0)


def test_instance_norm_unclamped_variance_is_rejected_on_hand_made_sums():
    hw = 64
    sums = (np.array([[2.0 * hw]]), np.array([[1.0 * hw]]), hw, np.array([[0.0]]))
    want = 1 / np.sqrt(np.float64(np.float32(X.EPS)))
    _, rstd = X.restate_in_stats(None, X.EPS, sums=sums)
    assert X.ulps(rstd[0, 0], want) <= 2
    _, rstd = X.restate_in_stats(None, X.EPS, 'no_clamp', sums=sums)
    assert not X.ulps(rstd[0, 0], want) <= 2
