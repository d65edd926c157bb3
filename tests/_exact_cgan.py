"""Case tables, inputs, float64 references and bounds for the kernels of csrc/tdg_cgan.hip that are not tdg_cgan_join:
tdg_cgan_prep, the four head entries, tdg_cgan_wgan_loss and tdg_cgan_metrics (pure NumPy, no GPU here).  The rules are
those of tests/_exact_cols.py and tests/_exact_pointwise.py, whose helpers are imported, not restated:

1. Exact where exactness is provable (np.array_equal with the float64 reference): the symmetric crop of prep, all of the
   head (integers times a power-of-two scale, eighths, leak 0.25), the threshold counts of the metrics.  The conditions
   -- f32 round trip, |v| < 2**24 grid units, |v| <= 256 units where bf16 is stored -- are asserted on reference values
   for the whole tables by tests/test_host_cgan_exact.py.
2. Bounded per element elsewhere: half an f32 ulp per operation of the kernel's own expression (class Ev), the device
   functions' OpenCL 1.2 full-profile limits, gamma(depth) * sum(|term| + error) for a sum whose longest addition chain
   is `depth` (read from the kernel), half a bf16 ulp for a bf16 store.  No constant is fitted to a device result.
3. Inputs are NaN wherever the kernel must not read, outputs hold the sentinel wherever it must not write.

Every reference returns every output array of its kernel.  The f32 NumPy restatements at the end serve the CPU mutation
check alone: clean they pass the comparison the GPU result gets, with one named defect they are rejected."""
from types import SimpleNamespace as NS

import numpy as np

from _exact_conv import LEAK, check_caps, describe_mismatch                                      # noqa: F401
from _exact_cols import store, bf16_round, gamma, bound_ratio, fits_f32, on_grid, ulps, NAN, SENTINEL, U32, U64      # noqa: F401
from _exact_pointwise import (Ev, add, sub, mul, div, neg, ev_log, ev_sigmoid, stored, sum_bound, one_block_depth,  # noqa: F401
                              BLOCK_SUM_DEPTH, f32c, ULP, TINY, GUARD, F32, BF16, _rng, _ints, _pick)

f32, f64 = np.float32, np.float64
SRC, CROP, OFF = 65, 29, 17               # csrc/tdg_cgan_common.h: kSrc, kCrop, kOff
NPIX, NSRC = CROP * CROP, SRC * SRC
MASK_NONE, MASK_LRELU, MASK_RELU = 0, 1, 2      # include/tdg.h (the host test ties them to _lib)
MASKS = (MASK_NONE, MASK_RELU, MASK_LRELU)
MASK_NAME = {0: 'none', 1: 'lrelu', 2: 'relu'}
TAIL = 64                                 # guard elements behind every device buffer


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ================================================================================================ tdg_cgan_prep
PREP_N = (1, 3)
PREP_VERSIONS = (0, 1, 2)
PREP_CENTRES = (4, 3, 5)                  # the images' centre pixels in eighths: y = 0.5, 0.375, 0.625
PREP_SUM_DEPTH = 4 + 6 + 3                # a thread's 3 - 4 pixels (from 0), six shuffle levels, sh[0] + sh[1] + sh[2] + sh[3]
PREP_GCH = 3                              # g_ones / rgb_ybar address channel 3 of a 4- or 8-channel image: the base is 3 elements in


def prep_strides(version):
    """(depth_cs, g_cs, rgb_cs) pairs: the smallest legal stride and a padded one, g and rgb different."""
    return ((2, 4, 8), (8, 8, 4)) if version == 2 else ((1, 4, 8), (8, 8, 4))


def prep_exact_inputs(n):
    """y = k / 8: per image the centre pixel kc and 420 pairs kc +- j, j in [0, 3], shuffled over the 29 x 29 crop; NaN
    everywhere outside rows and columns [17, 46).  v = 10 y = 5 k / 4 sits on the quarter grid, the 841 values add up to
    841 * (5 kc / 4) in any order, and 841 m / 841 is m."""
    rng = _rng(41, n)
    y = np.full((n, SRC, SRC), NAN, f32)
    for b in range(n):
        kc = PREP_CENTRES[b]
        j = rng.integers(0, 4, NPIX // 2)
        k = np.concatenate([[kc], kc + j, kc - j])
        rng.shuffle(k)
        y[b, OFF:OFF + CROP, OFF:OFF + CROP] = (k / 8.0).reshape(CROP, CROP)
    return NS(y=y, centre=np.array([10.0 * PREP_CENTRES[b] / 8.0 for b in range(n)]))


def prep_bounded_inputs(n):
    """Uniform y in [0.01, 0.99], as the model sees it; NaN outside the crop."""
    y = np.full((n, SRC, SRC), NAN, f32)
    y[:, OFF:OFF + CROP, OFF:OFF + CROP] = _rng(43, n).uniform(0.01, 0.99, (n, CROP, CROP)).astype(f32)
    return NS(y=y)


def prep_crop_ref(y):
    """crop = fl(y * 10): the float64 product of an f32 and 10 is exact, so its one rounding to f32 is the kernel's."""
    c = y[:, OFF:OFF + CROP, OFF:OFF + CROP].reshape(len(y), NPIX).astype(f64)
    return (c * 10.0).astype(f32).astype(f64)


def prep_ybar_ref(v, exact_sum=False):
    """(m, bound): m = sum(v) / 841 through the reduction tree and one division (exact_sum: the symmetric table)."""
    s = Ev(v.sum(1)) if exact_sum else Ev(v.sum(1), gamma(PREP_SUM_DEPTH, U32) * np.abs(v).sum(1))
    m = div(s, float(NPIX))
    return m.v, m.e


def prep_expected(v, m, version, strides, dtype, with_g=True):
    """Every output buffer as the device must leave it, bit for bit, given the crop values v (f32 in float64) and the
    mean m the kernel holds (f32: the exact one of the symmetric table, or the device's own, read back).  v - m is one
    f32 subtraction (exact in float64, rounded once), every store rounds once more to the dtype.  Untouched elements hold
    the sentinel: the fake half's channel 0 always, channels >= 1 (>= 2 in version 2) of both halves, and everything but
    channel PREP_GCH of g_ones / rgb_ybar -- whose 65 x 65 pixels are all written."""
    n = len(v)
    dcs, gcs, rcs = strides
    m = np.asarray(m, f64)
    real = np.full((n, NPIX, dcs), SENTINEL, f32)
    fake = np.full((n, NPIX, dcs), SENTINEL, f32)
    ch0 = v if version == 0 else (v - m[:, None]).astype(f32).astype(f64)
    real[:, :, 0] = store(ch0, dtype)
    if version == 2:
        real[:, :, 1] = fake[:, :, 1] = store(m, dtype)[:, None]
    g = np.full((n, NSRC, gcs), SENTINEL, f32)
    r = np.full((n, NSRC, rcs), SENTINEL, f32)
    if with_g:
        g[:, :, PREP_GCH] = 1.0
        r[:, :, PREP_GCH] = store(m, dtype)[:, None]
    return NS(real=real, fake=fake, g_ones=g, rgb_ybar=r, crop=v.astype(f32), ybar=m.astype(f32))


# ================================================================================================ the generator head
HEAD_CINS = (64, 128, 256, 512)            # TPP 8 / 16 / 32 / 64
HEAD_GEOMS = ((1, 5, 3), (3, 31, 29), (2, 7, 7), (1, 6, 1))         # (n, hw, crop)
HEAD_BIAS = {(1, 5, 3): 300, (3, 31, 29): 301, (2, 7, 7): -3, (1, 6, 1): 2}    # in units of the scale; ~300: g beyond bf16's integers
HEAD_CONFIGS = ((0, 1.0, True), (8, 2.0 ** -4, False))              # (cs - cin, scale, ybar given)
HEAD_FAKE_CS = 8
HEAD_LEAK = 0.25
HEAD_REFUSED_CIN = (72, 1024)


def head_id(cin, geom):
    return 'cin%d-n%d-hw%d-crop%d' % ((cin,) + tuple(geom))


def head_inputs(cin, geom, cfg):
    """cat in {-1, 0, 1} (zeros: the mask's kink), w and u integers in [-2, 2] (w times the scale; w[cin], the noise
    weight, never 0), b an integer times the scale, ybar integers or absent, dfake eighths in [-1, 1] with the last crop
    pixel's at 1.  NaN: cat's padding channels, cat and u outside the crop, the other channels of dfake."""
    n, hw, crop = geom
    pad, scale, has_ybar = HEAD_CONFIGS[cfg]
    rng = _rng(42, cin, n, hw, crop, cfg)
    cs = cin + pad
    cat = np.full((n, hw, hw, cs), NAN, f32)
    cat[:, :crop, :crop, :cin] = _ints(rng, -1, 1, (n, crop, crop, cin))
    w = _ints(rng, -2, 2, cin + 1) * f32(scale)
    w[cin] = f32(2 * scale if cin % 128 else -scale)
    u = np.full((n, hw, hw), NAN, f32)
    u[:, :crop, :crop] = _ints(rng, -2, 2, (n, crop, crop))
    dfake = np.full((n, crop, crop, HEAD_FAKE_CS), NAN, f32)
    dfake[..., 0] = _ints(rng, -8, 8, (n, crop, crop)) / f32(8)
    dfake[:, -1, -1, 0] = 1.0
    return NS(n=n, hw=hw, crop=crop, cin=cin, cs=cs, scale=scale, cat=cat, w=w, b=np.array([HEAD_BIAS[tuple(geom)] * scale], f32), u=u,
              ybar=_ints(rng, -4, 4, n) if has_ybar else None, dfake=dfake)


def head_fwd_ref(inp, noise):
    """g = w . cat (+ w[cin] u) + b on the top-left crop, float64: (g, yhat), both [n, crop * crop]."""
    c, cin = inp.crop, inp.cin
    g = inp.cat[:, :c, :c, :cin].astype(f64) @ inp.w[:cin].astype(f64) + float(inp.b[0])
    if noise:
        g = g + float(inp.w[cin]) * inp.u[:, :c, :c].astype(f64)
    g = g.reshape(inp.n, c * c)
    return g, g + (inp.ybar.astype(f64)[:, None] if inp.ybar is not None else 0.0)


def head_fake_expected(inp, g, dtype):
    """fake [n, crop * crop, fake_cs]: channel 0 is g rounded once to the dtype, the rest keeps the sentinel."""
    out = np.full((inp.n, inp.crop * inp.crop, HEAD_FAKE_CS), SENTINEL, f32)
    out[:, :, 0] = store(g, dtype)
    return out


def bf16_ties(g):
    """Elements of g that lie exactly half way between two bf16 values."""
    g32 = np.asarray(g, f64).astype(f32)
    lo = bits(g32) & np.uint32(0xffff)
    return lo == 0x8000


def mask_low(mode):
    return {MASK_NONE: 1.0, MASK_LRELU: HEAD_LEAK, MASK_RELU: 0.0}[mode]


def head_bwd_ref(inp, noise, mode):
    """float64: dcat inside the crop [n, crop, crop, cin], dw [cin (+ 1)], db [1], and the sums of magnitudes the exactness
    conditions are stated on."""
    c, cin = inp.crop, inp.cin
    d = inp.dfake[..., 0].astype(f64)
    catc = inp.cat[:, :c, :c, :cin].astype(f64)
    dcat = d[..., None] * inp.w[:cin].astype(f64) * np.where(catc > 0, 1.0, mask_low(mode))
    dw = np.einsum('bhw,bhwc->c', d, catc)
    mag = np.einsum('bhw,bhwc->c', np.abs(d), np.abs(catc))
    if noise:
        uc = inp.u[:, :c, :c].astype(f64)
        dw = np.concatenate([dw, [(d * uc).sum()]])
        mag = np.concatenate([mag, [np.abs(d * uc).sum()]])
    return NS(dcat=dcat, dw=dw, db=np.array([d.sum()]), mag=np.concatenate([mag, [np.abs(d).sum()]]))


def head_dcat_expected(inp, dcat, dtype):
    """The whole dcat buffer [n, hw, hw, cs]: the values inside the crop, +0.0 in the other pixels' cin channels, the
    sentinel in every padding channel."""
    out = np.full((inp.n, inp.hw, inp.hw, inp.cs), SENTINEL, f32)
    out[..., :inp.cin] = 0.0
    out[:, :inp.crop, :inp.crop, :inp.cin] = store(dcat, dtype)
    return out


def outside_crop_bits_ok(got, inp):
    """dcat outside the crop: +0.0 bit for bit in the cin channels."""
    m = np.ones((inp.hw, inp.hw), bool)
    m[:inp.crop, :inp.crop] = False
    return not np.any(bits(got[:, m][..., :inp.cin]))


def head_finish_blocks(cin, noise):
    """Labelling only: blocks of cgan_head_finish_kernel and the live threads of the last one."""
    cols = cin + (2 if noise else 1)
    return -(-cols // 256), cols - (-(-cols // 256) - 1) * 256


# ================================================================================================ tdg_cgan_wgan_loss
WGAN_ROWS = (1, 5, 255, 256, 257, 600)
WGAN_CS = (1, 8)
WGAN_MODES = (0, 1, 2)


def wgan_inputs(rows):
    """Logits: eighths in [-6, 6], exact in bf16, the two halves drawn apart."""
    z = _pick(_rng(44, rows), np.arange(-48, 49) / 8.0, 2 * rows)
    if rows == 1:
        z[:] = (-1.5, 2.25)
    return NS(z=z)


def wgan_ref(inp, mode, dtype):
    """scal = (-mf, mf, mr, mf - mr), m = fl(sum sigmoid * fl(1 / rows)); seeds [real half | fake half] of channel 0:
    mode 1 (-pr (1 - pr) inv | pf (1 - pf) inv), mode 2 (0 | -pf (1 - pf) inv).  mean64: the float64 means (one
    division), for the record of what `* inv` costs."""
    rows = len(inp.z) // 2
    pr, pf = ev_sigmoid(Ev(inp.z[:rows])), ev_sigmoid(Ev(inp.z[rows:]))
    inv = div(1.0, float(rows))
    depth = one_block_depth(rows)
    mr, mf = mul(sum_bound(pr, depth), inv), mul(sum_bound(pf, depth), inv)
    d = sub(mf, mr)
    out = NS(scal=np.array([-mf.v, mf.v, mr.v, d.v], f64), scal_bound=np.array([mf.e, mf.e, mr.e, d.e], f64),
             mean64=np.array([-pf.v.mean(), pf.v.mean(), pr.v.mean(), pf.v.mean() - pr.v.mean()]))
    if mode:
        if mode == 1:
            real, fake = mul(mul(neg(pr), sub(1.0, pr)), inv), mul(mul(pf, sub(1.0, pf)), inv)
        else:
            real, fake = Ev(np.zeros(rows)), mul(mul(neg(pf), sub(1.0, pf)), inv)
        both = Ev(np.concatenate([real.v, fake.v]), np.concatenate([real.e, fake.e]))
        out.seed, out.seed_bound = stored(both, dtype)
        if mode == 2:
            out.seed_bound[:rows] = 0.0
    return out


# ================================================================================================ tdg_cgan_metrics
METRIC_SIZES = ((1, 1), (3, 70), (3, 841), (1, 1025), (1, 256 * 1024 + 257))       # the last: past the 256-block cap
THRESHOLDS = (1.25, 1.5625, 1.953125)
# (y10, p10): max(a / p, p / a) with a = y10 / 10, p = p10 / 10 in f32 is exactly a threshold (first six: each threshold both
# ways round) or far from all three.  y10 / 10 and p10 / 10 are 1, 1.25, 1.5625 or 1.953125 there -- exact quotients, which a
# correctly rounded f32 division returns as they are (the build has no fast-math flag; tests/test_host_cgan_exact.py
# proves the pool with NumPy's IEEE f32 division under that assumption).
METRIC_POOL = ((12.5, 10.0), (10.0, 12.5), (15.625, 10.0), (10.0, 15.625), (19.53125, 10.0), (10.0, 19.53125),
               (10.0, 10.0), (5.0, 5.0), (10.0, 14.0), (14.0, 10.0), (10.0, 17.0), (17.0, 10.0), (20.0, 10.0), (10.0, 30.0), (3.0, 3.5),
               (11.0, 10.0))
METRIC_ON_THRESHOLD = 6
METRIC_OFFSET = 2.0                       # counts table: pred = p10 - offset[b], offset[b] = 2 + b, an exact sum


def metric_offsets(n):
    return (METRIC_OFFSET + np.arange(n)).astype(f32)


def metric_counts_inputs(n, hw):
    """(y, p10) [n, hw] drawn from the pool, the pool itself leading."""
    idx = _rng(45, n, hw).integers(0, len(METRIC_POOL), n * hw)
    k = min(n * hw, len(METRIC_POOL))
    idx[:k] = np.arange(k)
    pool = np.array(METRIC_POOL, f32)
    return NS(y=pool[idx, 0].reshape(n, hw), p10=pool[idx, 1].reshape(n, hw), idx=idx)


def metric_nan_inputs(n, hw, kind):
    """The counts table with zeros laid over it.  kind 'y0': every third y is 0; 'p0': every fourth prediction is 0; 'both':
    both (every twelfth element has y = prediction = 0)."""
    inp = metric_counts_inputs(n, hw)
    i = np.arange(n * hw).reshape(n, hw)
    if kind in ('y0', 'both'):
        inp.y[i % 3 == 0] = 0.0
    if kind in ('p0', 'both'):
        inp.p10[i % 4 == 0] = 0.0
    return inp


def metric_values_inputs(n, hw):
    """y in [0.1, 10], pred = y * [0.6, 1.6] - 1, offset in [1, 1.5] per image: pred + offset >= 0.06."""
    rng = _rng(46, n, hw)
    y = rng.uniform(0.1, 10, (n, hw)).astype(f32)
    pred = (y * rng.uniform(0.6, 1.6, (n, hw)).astype(f32) - f32(1)).astype(f32)
    return NS(y=y, pred=pred, offset=rng.uniform(1.0, 1.5, n).astype(f32))


def prediction(pred, offset, shape):
    """(pred ? pred[i] : 0) + (offset ? offset[b] : 0): one f32 addition (exact in float64, rounded once)."""
    p = np.zeros(shape, f64) if pred is None else pred.astype(f64)
    o = np.zeros((shape[0], 1), f64) if offset is None else offset.astype(f64)[:, None]
    return (p + o).astype(f32)


def metric_terms64(y10, p10):
    """The per-element formulas of metric_terms literally, in float64: the five terms and delta = q1 < q2 ? q2 : q1."""
    with np.errstate(all='ignore'):
        a, p = y10.astype(f64) / 10.0, p10.astype(f64) / 10.0
        e = a - p
        d = np.log(a + GUARD) - np.log(p + GUARD)
        q1, q2 = a / p, p / a
        delta = np.where(q1 < q2, q2, q1)
        return [np.abs(e) / p, e * e / p, e * e, d * d, d], delta


def metric_hits64(y10, p10):
    _, delta = metric_terms64(y10, p10)
    with np.errstate(invalid='ignore'):
        return [int((delta < t).sum()) for t in THRESHOLDS]


def metric_values64(y10, p10, counts):
    """The eight values in float64 from the literal formulas; `counts` (hits x 3, elements) is advanced in place."""
    t, _ = metric_terms64(y10, p10)
    n = float(y10.size)
    with np.errstate(all='ignore'):
        s = [float(x.sum()) for x in t]
        v = [s[0] / n, s[1] / n, np.sqrt(s[2] / n), np.sqrt(s[3] / n), s[3] / n - s[4] * s[4] / (n * n)]
    for k, h in enumerate(metric_hits64(y10, p10)):
        counts[k] += h
    counts[3] += y10.size
    return np.array(v + [counts[k] / counts[3] for k in range(3)], f64)


def value_class(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    v = np.asarray(v, f64)
    return np.where(np.isnan(v), 3, np.where(np.isposinf(v), 1, np.where(np.isneginf(v), 2, 0)))


def metric_bounded_ref(y10, p10):
    """(v[0..4], bound): every term through Ev in f32 as metric_terms writes it, the sums in f64 (gamma(n) in 2**-53), the
    value arithmetic in f64 (a few roundings in 2**-53, folded into gamma(8)) and one cast to f32.  v[4] = E[d^2] - E[d]^2
    inherits both sums' errors in full: the cancellation is not assumed away."""
    a, p = div(Ev(y10), 10.0), div(Ev(p10), 10.0)
    e = sub(a, p)
    d = sub(ev_log(add(a, GUARD)), ev_log(add(p, GUARD)))
    ee, ab = mul(e, e), Ev(np.abs(e.v), e.e)
    terms = (div(ab, p), div(ee, p), ee, mul(d, d), d)
    n = float(y10.size)
    g = gamma(y10.size, U64)
    s = [t.v.sum() for t in terms]
    es = [t.e.sum() + g * (np.abs(t.v) + t.e).sum() for t in terms]
    v = np.array([s[0] / n, s[1] / n, np.sqrt(s[2] / n), np.sqrt(s[3] / n), s[3] / n - s[4] * s[4] / (n * n)])
    root = lambda x, ex: max(np.sqrt((x + ex) / n) - np.sqrt(x / n), np.sqrt(x / n) - np.sqrt(max(x - ex, 0.0) / n))     # noqa: E731
    ev = np.array([es[0] / n, es[1] / n, root(s[2], es[2]), root(s[3], es[3]),
                   es[3] / n + (2 * abs(s[4]) * es[4] + es[4] ** 2) / (n * n)])
    mag = np.array([abs(v[0]), abs(v[1]), abs(v[2]), abs(v[3]), s[3] / n + s[4] * s[4] / (n * n)])
    return v, ev + gamma(8, U64) * (mag + ev) + U32 * (np.abs(v) + ev)


# ================================================================================================ NumPy restatements
def restate_prep(y, version, strides, dtype, defect=None):
    """cgan_prep_kernel in f32 (sums in a fixed NumPy order).  Defects: 'offset16' (the crop starts at 16), 'v0_minus_m'
    (version 0 subtracts the mean), 'ybar_real_only' (version 2 writes the y_bar channel to the real half alone)."""
    n = len(y)
    off = 16 if defect == 'offset16' else OFF
    v = (y[:, off:off + CROP, off:off + CROP].reshape(n, NPIX) * f32(10)).astype(f32)
    m = (v.sum(1, dtype=f32) / f32(NPIX)).astype(f32)
    out = prep_expected(v.astype(f64), m, 1 if (version == 0 and defect == 'v0_minus_m') else version, strides, dtype)
    if version == 2 and defect == 'ybar_real_only':
        out.fake[:, :, 1] = SENTINEL
    return out


def restate_head_fwd(inp, noise, dtype, defect=None):
    """cgan_head_fwd_kernel in f32: (yhat, g, fake).  Defect 'bottom_right': the crop is read from the bottom-right corner."""
    c, cin, o = inp.crop, inp.cin, (inp.hw - inp.crop if defect == 'bottom_right' else 0)
    with np.errstate(invalid='ignore'):
        g = (inp.cat[:, o:o + c, o:o + c, :cin] @ inp.w[:cin]).astype(f32)
        if noise:
            g = (g + inp.w[cin] * inp.u[:, o:o + c, o:o + c]).astype(f32)
        g = (g + inp.b[0]).astype(f32).reshape(inp.n, c * c)
        yhat = (g + (inp.ybar[:, None] if inp.ybar is not None else f32(0))).astype(f32)
    return yhat, g, head_fake_expected(inp, g.astype(f64), dtype)


def restate_head_bwd(inp, noise, mode, dtype, defect=None):
    """cgan_head_bwd_kernel and cgan_head_finish_kernel in f32: (dcat buffer, dw, db), dw and db prefilled with the sentinel.
    Defects: 'drop_last_group' (dW loses the pixels of the last trip of the group loop), 'db_to_dw' (db lands in
    dw[cols - 1]), 'noise_swapped' (the noise column and db change places), 'mask_ge' (mask cat >= 0), 'dcat_unwritten'
    (nothing is stored outside the crop)."""
    c, cin, hw = inp.crop, inp.cin, inp.hw
    G = 256 // (cin // 8)
    d = inp.dfake[..., 0]
    catc = inp.cat[:, :c, :c, :cin]
    on = catc >= 0 if defect == 'mask_ge' else catc > 0
    dcat = head_dcat_expected(inp, (d[..., None] * inp.w[:cin] * np.where(on, f32(1), f32(mask_low(mode)))).astype(f64), dtype)
    if defect == 'dcat_unwritten':
        keep = np.full_like(dcat, SENTINEL)
        keep[:, :c, :c, :cin] = dcat[:, :c, :c, :cin]
        dcat = keep
    dd = np.zeros((inp.n, hw, hw), f32)
    dd[:, :c, :c] = d
    full = np.zeros((inp.n, hw, hw, cin), f32)
    full[:, :c, :c] = catc
    uu = np.zeros((inp.n, hw, hw), f32)
    uu[:, :c, :c] = inp.u[:, :c, :c]
    dsum = dd.reshape(inp.n, -1).copy()
    if defect == 'drop_last_group':
        dsum[:, (hw * hw - 1) // G * G:] = 0
    cols = [np.einsum('bp,bpc->c', dsum, full.reshape(inp.n, hw * hw, cin)).astype(f32)]
    if noise:
        cols.append(np.array([(dd * uu).sum(dtype=f32)], f32))
    cols.append(np.array([dd.sum(dtype=f32)], f32))
    if defect == 'noise_swapped' and noise:
        cols[1], cols[2] = cols[2], cols[1]
    col = np.concatenate(cols)
    dw, db = np.full(len(col) - 1, SENTINEL, f32), np.full(1, SENTINEL, f32)
    if defect == 'db_to_dw':
        dw[:] = col[:-1]
        dw[-1] = col[-1]
    else:
        dw[:], db[0] = col[:-1], col[-1]
    return dcat, dw, db


def restate_wgan_seeds(z, mode, dtype, defect=None):
    """Defects: 'halves_swapped'; 'mode2_seeds_real' (mode 2 gives the real half mode 1's seeds instead of zeros)."""
    rows = len(z) // 2
    inv = f32(1) / f32(rows)
    p = (f32(1) / (f32(1) + np.exp(-z.astype(f32)))).astype(f32)
    pr, pf = p[:rows], p[rows:]
    real = -pr * (f32(1) - pr) * inv if (mode == 1 or defect == 'mode2_seeds_real') else np.zeros(rows, f32)
    fake = pf * (f32(1) - pf) * inv if mode == 1 else -pf * (f32(1) - pf) * inv
    if defect == 'halves_swapped':
        real, fake = fake, real
    return store(np.concatenate([real, fake]).astype(f32), dtype)


def restate_metric_hits(y, pred, offset, defect=None):
    """The three hit counts in f32.  Defects: 'le' (<= at a threshold), 'fmaxf' (delta = fmaxf(q1, q2)), 'offset_mod'
    (the offset indexed by i % hw)."""
    n, hw = y.shape
    if offset is not None and defect == 'offset_mod':
        o = offset[(np.arange(n * hw) % hw) % n].reshape(n, hw)
    else:
        o = np.zeros((n, 1), f32) if offset is None else offset[:, None]
    p10 = ((np.zeros_like(y) if pred is None else pred) + o).astype(f32)
    with np.errstate(all='ignore'):
        a, p = y / f32(10), p10 / f32(10)
        q1, q2 = a / p, p / a
        delta = np.fmax(q1, q2) if defect == 'fmaxf' else np.where(q1 < q2, q2, q1)
        return [int((delta <= f32(t)).sum() if defect == 'le' else (delta < f32(t)).sum()) for t in THRESHOLDS], (q1, q2)
