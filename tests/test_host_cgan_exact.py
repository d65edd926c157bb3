"""The recipe of tests/_exact_cgan.py checked on the CPU with reference arithmetic only: every condition the exact
comparisons of tests/test_gpu_cgan_exact.py rest on holds for the whole tables (so that file never skips or weakens one),
and f32 NumPy restatements of the kernels pass the GPU file's comparisons clean and are rejected, on the tables' own
inputs, with one named defect each."""
import numpy as np
import pytest

from conftest import pkg
import _exact_cgan as G

f32, f64 = np.float32, np.float64
HEAD_CASES = [(cin, g) for cin in G.HEAD_CINS for g in G.HEAD_GEOMS]
HEAD_IDS = [G.head_id(cin, g) for cin, g in HEAD_CASES]


def same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in vars(a))


def test_constants_match_the_library():
    L = pkg('_lib')
    assert (G.MASK_NONE, G.MASK_LRELU, G.MASK_RELU) == (L.MASK_NONE, L.MASK_LRELU, L.MASK_RELU) and (G.F32, G.BF16) == (L.F32, L.BF16)
    assert G.OFF + G.CROP <= G.SRC and G.NPIX == 841 and G.HEAD_LEAK == 0.25
    assert sorted(G.MASK_NAME) == sorted(G.MASKS)


# ================================================================================================ prep
@pytest.mark.parametrize('n', G.PREP_N)
def test_prep_exact_table_conditions(n):
    """The symmetric crop: k / 8 round-trips, 10 y sits on the quarter grid, the 841 values are the centre, and 420 pairs
    that cancel about it; their sum is 841 centres in any order and the f32 division gives the centre back; every stored
    value is bf16-representable; y is NaN everywhere outside [17, 46)^2."""
    inp = G.prep_exact_inputs(n)
    v = G.prep_crop_ref(inp.y)
    live = np.zeros((G.SRC, G.SRC), bool)
    live[G.OFF:G.OFF + G.CROP, G.OFF:G.OFF + G.CROP] = True
    assert np.all(np.isnan(inp.y[:, ~live])) and np.all(np.isfinite(inp.y[:, live]))
    y = inp.y[:, live].astype(f64)
    assert np.array_equal(y * 8, np.rint(y * 8)) and np.array_equal(v, y * 10) and np.array_equal(v * 4, np.rint(v * 4))
    dev = np.sort(v - inp.centre[:, None], axis=1)
    assert np.array_equal(dev, -dev[:, ::-1]) and np.all((dev == 0).sum(1) % 2 == 1) and np.any(dev != 0)
    G.on_grid(np.abs(v).sum(1), 0.25, 'sum |v|')
    assert np.array_equal(v.sum(1), G.NPIX * inp.centre)
    assert np.array_equal((v.sum(1).astype(f32) / f32(G.NPIX)).astype(f64), inp.centre)         # IEEE f32 division
    m, bound = G.prep_ybar_ref(v, exact_sum=True)
    assert np.array_equal(m, inp.centre) and G.fits_f32(m)
    for a in (v, v - inp.centre[:, None], inp.centre):
        assert np.array_equal(G.bf16_round(a.astype(f32)), a) and G.fits_f32(a)
    assert G.PREP_SUM_DEPTH == -(-G.NPIX // 256) + 6 + 3
    again = G.prep_exact_inputs(n)
    assert np.array_equal(again.y, inp.y, equal_nan=True)


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('version', G.PREP_VERSIONS)
def test_prep_restated_clean_and_with_defects(version, dtype):
    for n in G.PREP_N:
        inp = G.prep_exact_inputs(n)
        v = G.prep_crop_ref(inp.y)
        for strides in G.prep_strides(version):
            want = G.prep_expected(v, inp.centre, version, strides, dtype)
            assert same(want, G.restate_prep(inp.y, version, strides, dtype))
            assert not same(want, G.restate_prep(inp.y, version, strides, dtype, 'offset16'))            # (row 16 is NaN)
            assert same(want, G.restate_prep(inp.y, version, strides, dtype, 'v0_minus_m')) == (version != 0)
            assert same(want, G.restate_prep(inp.y, version, strides, dtype, 'ybar_real_only')) == (version != 2)
        # the bounded table: the restated mean lies within the tree's bound, and the outputs are exact at that mean
        inp = G.prep_bounded_inputs(n)
        v = G.prep_crop_ref(inp.y)
        m, bound = G.prep_ybar_ref(v)
        got = G.restate_prep(inp.y, version, G.prep_strides(version)[0], dtype)
        assert G.bound_ratio(got.ybar, m, bound).max() <= 1 and np.all(bound < 2.0 ** -18 * m)
        assert same(G.prep_expected(v, got.ybar, version, G.prep_strides(version)[0], dtype), got)
        assert np.array_equal(got.crop, (inp.y[:, G.OFF:G.OFF + G.CROP, G.OFF:G.OFF + G.CROP].reshape(n, -1) * f32(10)))


# ================================================================================================ head
@pytest.mark.parametrize('cin,geom', HEAD_CASES, ids=HEAD_IDS)
def test_head_table_conditions(cin, geom):
    """Every value the head's exact comparisons rest on: g and yhat round-trip through f32 and stay below 2**24 units of the
    scale, every sum's terms lie on one grid with room to spare, dcat and dfake are bf16-representable, cat holds zeros
    (the kink) inside the crop and NaN in its padding channels and outside the crop."""
    n, hw, crop = geom
    for cfg in range(len(G.HEAD_CONFIGS)):
        inp = G.head_inputs(cin, geom, cfg)
        assert np.all(np.isnan(inp.cat[..., cin:])) and np.all(np.isnan(inp.cat[:, crop:])) and np.all(np.isnan(inp.cat[:, :, crop:]))
        assert np.all(np.isnan(inp.u[:, crop:])) and np.all(np.isnan(inp.u[:, :, crop:])) and np.all(np.isnan(inp.dfake[..., 1:]))
        catc = inp.cat[:, :crop, :crop, :cin]
        assert set(np.unique(catc)) == {-1.0, 0.0, 1.0} and inp.w[cin] != 0 and (inp.cs - cin, inp.cs % 8) == (G.HEAD_CONFIGS[cfg][0], 0)
        d = inp.dfake[..., 0].astype(f64)
        assert np.array_equal(G.bf16_round(inp.dfake[..., 0]), inp.dfake[..., 0]) and np.array_equal(d * 8, np.rint(d * 8))
        assert np.all(d[:, -1, -1] == 1)
        for noise in (False, True):
            g, yhat = G.head_fwd_ref(inp, noise)
            mag = np.abs(catc).astype(f64) @ np.abs(inp.w[:cin]).astype(f64) + abs(float(inp.b[0])) + 2 * abs(float(inp.w[cin])) + 4
            G.on_grid(mag, inp.scale, 'head forward terms')
            assert G.fits_f32(g) and G.fits_f32(yhat) and np.array_equal(g / inp.scale, np.rint(g / inp.scale))
            for mode in G.MASKS:
                r = G.head_bwd_ref(inp, noise, mode)
                G.on_grid(r.mag, 1.0 / 8, 'head backward sums')
                assert G.fits_f32(r.dw) and G.fits_f32(r.db) and len(r.dw) == cin + noise
                assert np.array_equal(G.bf16_round(r.dcat.astype(f32)), r.dcat) and G.fits_f32(r.dcat)
                if mode != G.MASK_NONE:                     # the kink decides: cat == 0 takes the low factor
                    z = (catc == 0) & (d[..., None] != 0) & (inp.w[:cin] != 0)
                    assert z.any() and np.array_equal(r.dcat[z], (d[..., None] * inp.w[:cin] * G.mask_low(mode))[z])


def test_head_table_reaches_every_form():
    """bf16 ties in fake (g beyond 256 units, where bf16 steps by 2: odd g is a tie) and representable values too; cin 256
    and 512 reach the second and third finish block; the geometries' facts the table is built on."""
    ties = plain = 0
    for cin, geom in HEAD_CASES:
        inp = G.head_inputs(cin, geom, 0)
        for noise in (False, True):
            g, _ = G.head_fwd_ref(inp, noise)
            t = G.bf16_ties(g)
            ties += int(t.sum())
            plain += int((G.store(g, 1) == g).sum())
            st = G.store(g, 1).astype(f64)
            assert np.all(np.abs(st - g)[t] == np.abs(g[t] - np.where(st > g, st - 2 * np.abs(st - g), st + 2 * np.abs(st - g))[t]))
            assert np.all((G.bits(G.store(g, 1))[t] >> 16) % 2 == 0)                               # ties went to even
    assert ties > 1000 and plain > 1000
    assert G.head_finish_blocks(256, False) == (2, 1) and G.head_finish_blocks(256, True) == (2, 2)
    assert G.head_finish_blocks(512, False) == (3, 1) and G.head_finish_blocks(512, True) == (3, 2)
    assert G.head_finish_blocks(64, True)[0] == 1 and G.head_finish_blocks(128, False)[0] == 1
    assert 5 * 5 < 256 // 8 and 31 * 31 == 30 * 32 + 1 and all(31 * 31 % (256 // t) for t in (8, 16, 32, 64))
    assert (2, 7, 7) in G.HEAD_GEOMS and (1, 6, 1) in G.HEAD_GEOMS


def head_accepts(inp, noise, mode, dtype, defect_fwd=None, defect_bwd=None):
    """The GPU file's comparisons on the restatement's outputs."""
    g, yhat = G.head_fwd_ref(inp, noise)
    y2, g2, fake = G.restate_head_fwd(inp, noise, dtype, defect_fwd)
    ok = np.array_equal(y2, yhat) and np.array_equal(g2, g) and np.array_equal(fake, G.head_fake_expected(inp, g, dtype))
    r = G.head_bwd_ref(inp, noise, mode)
    dcat, dw, db = G.restate_head_bwd(inp, noise, mode, dtype, defect_bwd)
    return ok and np.array_equal(dcat, G.head_dcat_expected(inp, r.dcat, dtype)) and G.outside_crop_bits_ok(dcat, inp) \
        and np.array_equal(dw, r.dw) and np.array_equal(db, r.db)


@pytest.mark.parametrize('cin', G.HEAD_CINS)
def test_head_restated_clean_and_with_defects(cin):
    for geom in G.HEAD_GEOMS:
        for cfg in range(len(G.HEAD_CONFIGS)):
            inp = G.head_inputs(cin, geom, cfg)
            for noise in (False, True):
                for mode in G.MASKS:
                    assert head_accepts(inp, noise, mode, 1), (geom, cfg, noise, mode)
    ragged, full = G.head_inputs(cin, (3, 31, 29), 0), G.head_inputs(cin, (2, 7, 7), 1)
    for dtype in (0, 1):
        for noise in (False, True):
            assert not head_accepts(ragged, noise, G.MASK_LRELU, dtype, defect_fwd='bottom_right')
            assert not head_accepts(full, noise, G.MASK_LRELU, dtype, defect_bwd='drop_last_group')
            assert not head_accepts(ragged, noise, G.MASK_LRELU, dtype, defect_bwd='db_to_dw')
            assert not head_accepts(ragged, noise, G.MASK_LRELU, dtype, defect_bwd='dcat_unwritten')
            for mode in (G.MASK_RELU, G.MASK_LRELU):
                assert not head_accepts(ragged, noise, mode, dtype, defect_bwd='mask_ge')
        assert not head_accepts(ragged, True, G.MASK_LRELU, dtype, defect_bwd='noise_swapped')
        assert not head_accepts(full, True, G.MASK_NONE, dtype, defect_bwd='noise_swapped')


# ================================================================================================ wgan
@pytest.mark.parametrize('rows', G.WGAN_ROWS)
def test_wgan_restated_clean_and_with_defects(rows):
    inp = G.wgan_inputs(rows)
    assert np.array_equal(G.bf16_round(inp.z), inp.z) and np.abs(inp.z).max() <= 6 and np.array_equal(inp.z * 8, np.rint(inp.z * 8))
    z = inp.z.astype(f32)
    p = (f32(1) / (f32(1) + np.exp(-z))).astype(f32)
    inv = f32(1) / f32(rows)
    mr, mf = p[:rows].sum(dtype=f32) * inv, p[rows:].sum(dtype=f32) * inv
    for dtype in (0, 1):
        for mode in G.WGAN_MODES:
            ref = G.wgan_ref(inp, mode, dtype)
            assert G.bound_ratio(np.array([-mf, mf, mr, mf - mr], f32), ref.scal, ref.scal_bound).max() <= 1
            assert np.all(ref.scal_bound < 2.0 ** -18) and np.all(np.abs(ref.scal - ref.mean64) <= ref.scal_bound)
            if not mode:
                continue
            accepts = lambda s: G.bound_ratio(s, ref.seed, ref.seed_bound).max() <= 1                # noqa: E731
            assert accepts(G.restate_wgan_seeds(inp.z, mode, dtype))
            assert not accepts(G.restate_wgan_seeds(inp.z, mode, dtype, 'halves_swapped'))
            if mode == 2:
                assert np.all(ref.seed[:rows] == 0) and np.all(ref.seed_bound[:rows] == 0) and not np.any(np.signbit(ref.seed[:rows]))
                assert not accepts(G.restate_wgan_seeds(inp.z, mode, dtype, 'mode2_seeds_real'))
    assert G.one_block_depth(rows) == -(-rows // 256) + 9


# ================================================================================================ metrics
def test_metric_pool_is_on_a_threshold_or_far_from_all():
    """In IEEE f32 (NumPy's division is correctly rounded, as the device's is without a fast-math flag): the first six pairs
    give delta equal to a threshold exactly, one pair per threshold and direction, every other pair stays 1 % or more
    away from all three; the float64 formulas agree on which are hits; an element on a threshold is not a hit."""
    pool = np.array(G.METRIC_POOL, f32)
    a, p = pool[:, 0] / f32(10), pool[:, 1] / f32(10)
    q1, q2 = a / p, p / a
    delta = np.where(q1 < q2, q2, q1)
    t = np.array(G.THRESHOLDS, f32)
    assert np.array_equal(t.astype(f64), G.THRESHOLDS) and np.allclose(t, [1.25, 1.25 ** 2, 1.25 ** 3], rtol=0, atol=0)
    on = delta[:, None] == t[None, :]
    assert np.array_equal(on[:G.METRIC_ON_THRESHOLD].sum(1), np.ones(G.METRIC_ON_THRESHOLD)) and not on[G.METRIC_ON_THRESHOLD:].any()
    assert np.array_equal(on[:G.METRIC_ON_THRESHOLD].sum(0), [2, 2, 2])
    far = np.abs(delta[G.METRIC_ON_THRESHOLD:, None].astype(f64) / t[None, :] - 1)
    assert far.min() >= 0.01
    _, d64 = G.metric_terms64(pool[:, 0], pool[:, 1])
    assert np.array_equal(d64[:, None] < t[None, :], delta[:, None] < t[None, :])
    assert np.array_equal(d64[:G.METRIC_ON_THRESHOLD], delta[:G.METRIC_ON_THRESHOLD])
    hits = (delta[:, None] < t[None, :]).sum(0)
    assert 0 < hits[0] < hits[1] < hits[2] < len(pool)
    off = G.metric_offsets(3)
    assert np.array_equal(((pool[:, 1:2] - off[None, :]).astype(f32) + off[None, :]).astype(f32), np.broadcast_to(pool[:, 1:2], (len(pool), 3)))


@pytest.mark.parametrize('size', G.METRIC_SIZES, ids=['%dx%d' % s for s in G.METRIC_SIZES])
def test_metric_counts_restated_clean_and_with_defects(size):
    n, hw = size
    inp = G.metric_counts_inputs(n, hw)
    off = G.metric_offsets(n)
    want = G.metric_hits64(inp.y, inp.p10)
    pred = (inp.p10 - off[:, None]).astype(f32)
    assert np.array_equal(G.prediction(pred, off, (n, hw)), inp.p10)
    for pr, of in ((pred, off), (inp.p10, None)):
        got, _ = G.restate_metric_hits(inp.y, pr, of)
        assert got == want
        assert G.restate_metric_hits(inp.y, pr, of, 'le')[0] != want                   # (the pool's threshold pairs lead every table)
    if n > 1:
        assert G.restate_metric_hits(inp.y, pred, off, 'offset_mod')[0] != want
    v = G.metric_values_inputs(n, hw)
    if n > 1:
        p10 = G.prediction(v.pred, v.offset, (n, hw))
        with np.errstate(all='ignore'):
            bad = G.prediction(v.pred, v.offset[(np.arange(n * hw) % hw) % n].reshape(n, hw)[:, 0] * 0 + v.offset, (n, hw))
        assert np.array_equal(bad, p10)                                                 # (prediction() itself indexes by image)


@pytest.mark.parametrize('kind', ['y0', 'p0', 'both', 'neither'])
def test_metric_nan_rule_classes_and_the_fmaxf_restatement(kind):
    """The classes the NaN-rule table must produce, and the one named defect that no input can expose: a / p is NaN exactly
    when p / a is (both 0, both infinite, or a NaN operand), so `q1 < q2 ? q2 : q1` and fmaxf(q1, q2) -- which differ only
    when ONE operand is NaN -- give the same delta for every (y, prediction).  The restatement with fmaxf is therefore
    accepted on every table (asserted, with the premise), and the two rules are shown to differ on (NaN, 1)."""
    n, hw = 3, 70
    inp = G.metric_counts_inputs(n, hw) if kind == 'neither' else G.metric_nan_inputs(n, hw, kind)
    pred = None if kind == 'neither' else inp.p10
    p10 = G.prediction(pred, None, (n, hw))
    counts = [0, 0, 0, 0]
    cls = G.value_class(G.metric_values64(inp.y, p10, counts))
    want = {'y0': [0, 0, 0, 0, 0], 'p0': [1, 1, 0, 0, 0], 'both': [3, 3, 0, 0, 0], 'neither': [1, 1, 0, 0, 0]}[kind]
    assert cls[:5].tolist() == want and cls[5:].tolist() == [0, 0, 0] and counts[3] == n * hw
    lit, (q1, q2) = G.restate_metric_hits(inp.y, pred, None)
    assert lit == counts[:3] and (kind == 'neither' or lit[2] > 0)
    assert np.array_equal(np.isnan(q1), np.isnan(q2))
    assert G.restate_metric_hits(inp.y, pred, None, 'fmaxf')[0] == lit
    q = np.array([np.nan, 1.0], f32)
    assert np.fmax(q[0], q[1]) == 1 and np.isnan(np.where(q[0] < q[1], q[1], q[0]))


@pytest.mark.parametrize('size', G.METRIC_SIZES[:4], ids=['%dx%d' % s for s in G.METRIC_SIZES[:4]])
def test_metric_values_restated_within_the_bound(size):
    n, hw = size
    v = G.metric_values_inputs(n, hw)
    for pred, offset in ((v.pred, v.offset), (None, v.offset), ((v.pred + f32(1.25)).astype(f32), None)):
        p10 = G.prediction(pred, offset, (n, hw))
        assert p10.min() > 0.05
        a, p = v.y / f32(10), p10 / f32(10)
        e = a - p
        d = np.log(a + f32(1e-8)) - np.log(p + f32(1e-8))
        s = [t.astype(f64).sum() for t in (np.abs(e) / p, e * e / p, e * e, d * d, d)]
        N = float(n * hw)
        got = np.array([s[0] / N, s[1] / N, np.sqrt(s[2] / N), np.sqrt(s[3] / N), s[3] / N - s[4] * s[4] / (N * N)]).astype(f32)
        ref, bound = G.metric_bounded_ref(v.y, p10)
        assert G.bound_ratio(got, ref, bound).max() <= 1 and np.all(bound <= 1e-4 * np.maximum(np.abs(ref), ref[3] ** 2)), (got, ref, bound)
        # a sixteenth of the elements dropped from one sum moves it far outside
        worse = got.copy()
        worse[0] *= f32(15.0 / 16)
        assert G.bound_ratio(worse, ref, bound).max() > 1
