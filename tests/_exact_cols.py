"""Inputs, float64 oracles and bounds for the column-reduction / batch-norm / scalar- and row-reduction kernels of
csrc/tdg_elementwise.hip (pure NumPy, no GPU here).

Exact where exactness is provable: inputs are small integers or quarter-integers, coefficients and rstd powers of two,
the lrelu leak 0.25.  Every f32 sum is then exact in any order (all terms lie on one power-of-two grid and the sum of
their magnitudes stays below 2**24 grid steps) and every stored value is representable in its storage type, so the
device must equal the float64 oracle under np.array_equal.  The two caps of tests/_exact_conv.py are the only
conditions; they are asserted on oracle values (tests/test_host_cols_exact.py, for the whole case table).

Derived bounds where exactness is impossible (rstd, the BN apply formulas, tanh, sums of a stored non-integer du): the
oracle is float64 on exactly the bytes the kernel reads, and each bound is built from the oracle's own intermediates as
    (number of f32 roundings on the path) * 2**-24 * (sum of the magnitudes of the terms being rounded)
  + half a bf16 ulp of the value for a bf16 store (2**-9 |value| at the top of a binade, 2**-8 |value| at its bottom)
with gamma(n, u) = n u / (1 - n u) in place of n u (Higham, Accuracy and Stability of Numerical Algorithms, lemma
3.1: it also covers the second-order terms).  f32 tensors are accumulated in double by the kernels (u = 2**-53 on those
roundings), bf16 tensors in float (u = 2**-24).  Device transcendentals get the OpenCL full-profile limits the ROCm
device library is built to (tanh: 5 ulp).  No constant here is fitted to a device result.
"""
from collections import namedtuple
from types import SimpleNamespace as NS

import numpy as np

from _exact_conv import LEAK, BF16_CAP, F32_CAP, check_caps, describe_mismatch  # noqa: F401

U32, U64 = 2.0 ** -24, 2.0 ** -53                     # unit roundoffs: f32, f64
TANH_ULP = 5                                          # OpenCL full profile, in f32 ulps (ulp(x) <= 2**-23 |x|)
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3  # include/tdg.h (tests/test_host_cols_exact.py ties them to _lib)
EPS = 1e-3                                            # the layers' batch-norm epsilon
NAN = float('nan')
SENTINEL = 77.0                                       # output prefill: representable in bf16, never a correct answer's neighbour


def gamma(n, u):
    return n * u / (1.0 - n * u)


def acc_u(dtype):
    """Unit roundoff of the kernels' accumulators: double for f32 tensors (dtype 0), float for bf16 tensors (dtype 1)."""
    return U64 if dtype == 0 else U32


def bf16_round(a):
    """float32 -> nearest-even bf16 -> float32 (finite values)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b >> 16) & 1) + 0x7fff
    return ((b + r) & 0xffff0000).astype(np.uint32).view(np.float32)


def bf16_half_ulp(x):
    """The largest error of a round-to-nearest bf16 store of a value of magnitude |x|: half the bf16 spacing of x's binade,
    2**(floor(log2 |x|) - 8).  bf16 keeps 8 significant bits, so this is 2**-9 |x| only where |x| is just below a power of
    two and 2**-8 |x| just above one (1 + 2**-8 is stored as 1); a bound of 2**-9 |x| throughout would reject correctly
    rounded stores."""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))          # |x| = m 2**e, m in [0.5, 1)
    return np.where(np.asarray(x) != 0, np.ldexp(1.0, e - 9), 0.0)


def store_bound(e, value, dtype):
    """The bound `e` on the f32 value, plus the store: nothing for f32, half a bf16 ulp at the largest magnitude the f32 value
    can have for bf16."""
    return e + (bf16_half_ulp(np.abs(value) + e) if dtype == 1 else 0.0)


def store(v, dtype):
    """The float64 value `v` as the device stores it (dtype 0: f32, 1: bf16), as float32."""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    return bf16_round(f) if dtype == 1 else f


def ulps(got, want):
    """|got - want| in units of the f32 spacing at `want`."""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ geometry and the table
def col_geometry(rows, c, cs, elem_size=4, aligned=True, allow_vec=True):
    """col_geom() of csrc/tdg_elementwise.hip restated.  Used ONLY to label cases, to check that the table reaches every
    branch, and by the NumPy restatements of the mutation check -- never to compute an expected value.
    `aligned`: every base pointer of the launch is a multiple of 4 * elem_size bytes."""
    vw = 4 if (allow_vec and c % 4 == 0 and cs % 4 == 0 and aligned) else 1
    cv = -(-c // vw)
    cl = 1
    while cl < cv and cl < 64:
        cl <<= 1
    ncol = -(-cv // cl)
    wide = ncol >= 8
    want = -(-rows // (32 if wide else 128))
    cap = 32 if wide else (512 if ncol >= 2 else 1024)
    nblk = max(1, min(want, cap))
    rpb = -(-rows // nblk)
    nblk = -(-rows // rpb)
    return NS(rows=rows, c=c, cs=cs, elem_size=elem_size, vw=vw, cv=cv, CL=cl, RL=256 // cl, ncol=ncol, wide=wide, want=want,
              cap=cap, nblk=nblk, rows_per_blk=rpb, last_rows=rows - (nblk - 1) * rpb, live_last_chunk=cv - (ncol - 1) * cl,
              aligned=aligned)


BRANCHES = ('vw4', 'vw1:c%4', 'vw1:cs%4', 'vw1:pointer', 'CL<64:dead_tail_lanes', 'ncol==1', 'ncol2-7:one_live_lane',
            'ncol>=8', 'ragged_last_block', 'block<one_trip', 'cap32', 'cap512', 'cap1024', 'nblk>=1024', 'rows==1')


def branches(g):
    """The labels of BRANCHES a geometry takes."""
    out = set()
    if g.vw == 4:
        out.add('vw4')
    elif g.c % 4:
        out.add('vw1:c%4')
    elif g.cs % 4:
        out.add('vw1:cs%4')
    elif not g.aligned:
        out.add('vw1:pointer')
    if g.CL < 64 and g.cv < g.CL:
        out.add('CL<64:dead_tail_lanes')
    if g.ncol == 1:
        out.add('ncol==1')
    if 2 <= g.ncol <= 7 and g.live_last_chunk == 1:
        out.add('ncol2-7:one_live_lane')
    if g.ncol >= 8:
        out.add('ncol>=8')
    if g.nblk > 1 and g.last_rows != g.rows_per_blk:
        out.add('ragged_last_block')
    if min(g.rows_per_blk, g.last_rows) < 4 * g.RL:
        out.add('block<one_trip')
    if g.want > g.cap:
        out.add('cap%d' % g.cap)
    if g.nblk >= 1024:
        out.add('nblk>=1024')
    if g.rows == 1:
        out.add('rows==1')
    return out


Case = namedtuple('Case', 'rows c cs off')          # off: elements between the (16-byte aligned) allocation and the tensor

TABLE = [
    Case(1, 1, 1, 0),
    Case(130, 7, 8, 0),
    Case(96, 100, 104, 0),
    Case(64, 260, 264, 0),
    Case(33, 2052, 2052, 0),
    Case(1100, 2048, 2048, 0),        # cap 32
    Case(40, 515, 515, 0),            # vw 1, ncol 9
    Case(65600, 65, 65, 0),           # cap 512
    Case(131072, 4, 4, 0),            # nblk 1024: the 2-channel finalize
    Case(140000, 3, 3, 0),            # cap 1024
    Case(512, 200, 200, 0),           # power-of-two rows
    Case(96, 100, 104, 1),            # base pointer offset by one element
    Case(70, 12, 13, 0),              # C % 4 == 0, cs % 4 != 0 (the coverage check asked for it)
]
SMALL = [k for k in TABLE if k.rows * k.c <= 300000]   # every activation / aliasing variant runs on these; the rest get one


def case_id(k):
    return '%dx%d-cs%d%s' % (k.rows, k.c, k.cs, '-off%d' % k.off if k.off else '')


def geometry_of(k, elem_size):
    return col_geometry(k.rows, k.c, k.cs, elem_size, aligned=(k.off * elem_size) % (4 * elem_size) == 0)


def missing_branches(table, elem_size):
    seen = set()
    for k in table:
        seen |= branches(geometry_of(k, elem_size))
    return [b for b in BRANCHES if b not in seen]


# ------------------------------------------------------------------------------------------------ guarded layouts
class Layout:
    """A [rows][c] tensor with row stride cs inside a flat buffer: `off` elements in front, cs - c padding columns and a
    band of `band` extra rows behind.  Inputs carry NaN everywhere outside the tensor (any over-read poisons a sum),
    outputs a sentinel (any stray write shows)."""

    def __init__(self, rows, c, cs, off=0, band=3):
        self.rows, self.c, self.cs, self.off = rows, c, cs, off
        self.n = off + (rows + band) * cs
        self.idx = off + np.arange(rows, dtype=np.int64)[:, None] * cs + np.arange(c, dtype=np.int64)[None, :]

    def pack(self, data, fill=NAN):
        flat = np.full(self.n, fill, dtype=np.float32)
        flat[self.idx] = data
        return flat

    def unpack(self, flat):
        return flat[self.idx]

    def outside(self, flat):
        m = np.ones(self.n, dtype=bool)
        m[self.idx] = False
        return flat[m]


def _rng(k, tag):
    return np.random.default_rng([tag] + [int(v) for v in k])


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def on_grid(sum_abs, q, what=''):
    """The exact-sum condition: terms that are multiples of q with sum |term| < 2**24 q add exactly in f32 in any order."""
    return check_caps(np.asarray(sum_abs, dtype=np.float64) / q, 'f32', what)


def fits_f32(v):
    v = np.asarray(v, dtype=np.float64)
    return bool(np.array_equal(v.astype(np.float32).astype(np.float64), v))


# ------------------------------------------------------------------------------------------------ column sums
def colsum_inputs(k):
    """x, the per-row coefficients and the prefilled vector: integers in [-3, 3]."""
    rng = _rng(k, 1)
    return NS(x=_ints(rng, -3, 3, (k.rows, k.c)), coef=_ints(rng, -3, 3, k.rows), old=_ints(rng, -3, 3, k.c))


def colsum_ref(x, coef=None, old=None):
    x = x.astype(np.float64)
    s = (x if coef is None else x * coef.astype(np.float64)[:, None]).sum(0)
    return s if old is None else s + old.astype(np.float64)


def colsum_caps(inp):
    check_caps(inp.x, 'bf16', 'x')
    check_caps(np.abs(inp.x.astype(np.float64) * inp.coef.astype(np.float64)[:, None]).sum(0) + np.abs(inp.old), 'f32', 'weighted sums')
    check_caps(np.abs(inp.x).astype(np.float64).sum(0) + np.abs(inp.old), 'f32', 'sums')


# ------------------------------------------------------------------------------------------------ finalize on partials
FIN_NBLK = (1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 1537)   # around both layouts' 4-trip strides and the layout switch
FIN_C = (1, 7, 8, 9, 200)
FIN_ROWS = 64                                                        # a power of two: the mean is exact


def partials_inputs(nblk, c):
    """Integer partial planes [nblk][2][c].  For the BN form plane 0 holds row-sum partials of d = u - pivot and plane 1 of
    d*d for a tensor of FIN_ROWS rows; column 0 is built with s1 / rows - md**2 < 0 (md = 2, s1 = rows: 1 - 4), which
    no data can produce and only the clamp turns into rstd = 1 / sqrt(eps)."""
    rng = _rng((nblk, c), 2)
    p = np.zeros((nblk, 2, c), dtype=np.float32)
    p[:, 0] = _ints(rng, -3, 3, (nblk, c))
    p[:, 1] = _ints(rng, 0, 6, (nblk, c))
    # keep var > 0 off column 0: lift plane 1 until s1 * rows > s0**2 with room to spare
    s0 = p[:, 0].astype(np.float64).sum(0)
    s1 = p[:, 1].astype(np.float64).sum(0)
    need = np.ceil(np.maximum(s0 * s0 / FIN_ROWS + FIN_ROWS - s1, 0.0))
    p[0, 1] += need.astype(np.float32)
    p[:, 0, 0] = 0.0
    p[:, 1, 0] = 0.0
    p[nblk - 1, 0, 0] = 2.0 * FIN_ROWS                 # in the LAST block: a finalize that stops early never sees it
    p[nblk - 1, 1, 0] = 1.0 * FIN_ROWS
    u = _ints(rng, -3, 3, (FIN_ROWS, c))
    return NS(partial=p, old=_ints(rng, -3, 3, c), u=u, pivot=_ints(rng, -3, 3, c), beta=_ints(rng, -4, 4, c) / np.float32(4))


def partials_caps(inp):
    check_caps(np.abs(inp.partial).astype(np.float64).sum(0).max() + 3.0, 'f32', 'partial sums')
    check_caps(inp.u, 'bf16', 'u')


def stats_from_sums(s0, s1, rows, pivot):
    """float64 mean / var / the two cancelling terms from exact sums of d and d*d."""
    md = s0 / rows
    e2 = s1 / rows
    return NS(md=md, e2=e2, mean=pivot + md, var=e2 - md * md)


# ------------------------------------------------------------------------------------------------ batch-norm statistics
def mean_bound(st, dtype):
    """mean = fl(pivot + fl(s0 * fl(1 / rows))), s0 exact.  md carries the roundings of 1 / rows and of the product in the
    accumulator type (gamma_2); the sum pivot + md is rounded once in the accumulator type and, for f32 tensors (double
    accumulator), once more by the cast to float."""
    ua = acc_u(dtype)
    e_md = gamma(2, ua) * np.abs(st.md)
    return e_md + (U32 + (U64 if dtype == 0 else 0.0)) * (np.abs(st.mean) + e_md)


def rstd_interval(st, dtype, eps=EPS):
    """rstd = float(1 / sqrt(double(max(var_c, 0)) + double(eps))), var_c = fl(fl(s1 * inv) - fl(md_c * md_c)).
    E[d^2] reaches var_c through 3 roundings (inv, the product, the subtraction), md^2 through 6 (inv and the product,
    twice; the square; the subtraction): |var_c - var| <= gamma_6 (E[d^2] + md^2) =: dv, i.e. a relative error of
    gamma_6 times the amplification (E[d^2] + md^2) / var the cancellation brings.  The clamp moves var_c towards the true
    var >= 0.  rstd is monotone in var, so it lies in [1 / sqrt(var + dv + eps), 1 / sqrt(max(var - dv, 0) + eps)], widened by the
    double add, sqrt and divide (gamma_4 in 2**-53; the OpenCL limits of double sqrt and divide are correctly rounded)
    and the cast to float (2**-24).  Returns (rstd, lo, hi, amplification)."""
    var = np.maximum(st.var, 0.0)
    amp = st.e2 + st.md * st.md
    dv = gamma(6, acc_u(dtype)) * amp
    e = float(np.float32(eps))
    slack = U32 + gamma(4, U64)
    rstd = 1.0 / np.sqrt(var + e)
    lo = (1.0 - slack) / np.sqrt(var + dv + e)
    hi = (1.0 + slack) / np.sqrt(np.maximum(var - dv, 0.0) + e)
    return rstd, lo, hi, amp / np.maximum(var, e)


def interval_ratio(got, want, lo, hi):
    """Per column: the deviation from `want` as a fraction of the room the interval [lo, hi] leaves on that side (NaN -> inf)."""
    got = np.asarray(got, dtype=np.float64)
    room = np.where(got >= want, hi - want, want - lo)
    r = np.abs(got - want) / room
    return np.where(np.isfinite(got), r, np.inf)


def bound_ratio(got, want, bound):
    """Per element |got - want| / bound; 0 where both vanish, inf where a zero bound is missed or got is not finite."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return np.where(np.isfinite(got), r, np.inf)


BASES = (0, 7, -7, 200, -200)     # the +-200 columns are what the pivot is for


def const_column(c):
    return c - 1 if c >= 6 else None


def bn_fwd_inputs(k, tag=3):
    """u[:, j] = BASES[j % 5] + integers in [-3, 3]; the last column constant (c >= 6); beta quarter-integers in [-1, 1]."""
    rng = _rng(k, tag)
    base = np.array([BASES[j % 5] for j in range(k.c)], dtype=np.float32)
    u = base[None, :] + _ints(rng, -3, 3, (k.rows, k.c))
    if const_column(k.c) is not None:
        u[:, const_column(k.c)] = base[const_column(k.c)]
    return NS(u=u, beta=_ints(rng, -4, 4, k.c) / np.float32(4), base=base)


def bn_stats_ref(u):
    """float64 moments of the columns of u, as deviations from row 0 (exact: integers)."""
    u = u.astype(np.float64)
    d = u - u[0]
    return stats_from_sums(d.sum(0), (d * d).sum(0), u.shape[0], u[0])


def bn_fwd_caps(inp):
    check_caps(inp.u, 'bf16', 'u')
    d = inp.u.astype(np.float64) - inp.u[0].astype(np.float64)
    check_caps(np.abs(d).sum(0), 'f32', 'sum |d|')
    check_caps((d * d).sum(0), 'f32', 'sum d^2')


def act_ref(p, act):
    if act == ACT_RELU:
        return np.maximum(p, 0.0)
    if act == ACT_LRELU:
        return np.where(p > 0, p, LEAK * p)
    if act == ACT_TANH:
        return np.tanh(p)
    assert act == ACT_NONE
    return p


def bn_apply_ref(u, mean, rstd, beta, act, dtype):
    """pre = (u - mean) * rstd + beta and h = act(pre) in float64 at the DEVICE's statistics (read back), with bounds.
    The f32 path is fl(fl(fl(u - mean) * rstd) + beta) (or one fma): (u - mean) * rstd passes through 3 roundings, beta
    through 1: |pre_c - pre| <= gamma_3 (|(u - mean) rstd| + |beta|) =: e.  relu / lrelu (leak a power of two) / none
    are 1-Lipschitz and add no rounding, so h inherits e; tanh is 1-Lipschitz too and adds TANH_ULP ulps of its value.
    h is computed from the f32 pre, not from the stored one.  A bf16 store adds half a bf16 ulp (store_bound)."""
    u = u.astype(np.float64)
    xh = (u - mean.astype(np.float64)) * rstd.astype(np.float64)
    b = beta.astype(np.float64)
    pre = xh + b
    e = gamma(3, U32) * (np.abs(xh) + np.abs(b))
    h = act_ref(pre, act)
    eh = e + (TANH_ULP * 2.0 ** -23 * (np.abs(h) + e) if act == ACT_TANH else 0.0)
    return NS(pre=pre, h=h, pre_bound=store_bound(e, pre, dtype), h_bound=store_bound(eh, h, dtype))


# ------------------------------------------------------------------------------------------------ batch-norm backward
DU_EXACT_ROWS = (1, 64, 512, 131072)      # the table's power-of-two rows: every intermediate of du fits f32 (the host test proves it)


def bn_bwd_inputs(k, tag=4):
    """dh in {-1, 0, 1}; beta and pre quarter-integers; rstd in {0.5, 1, 2}.  Row 0 of pre equals beta (xhat = 0), row 1
    (and a tenth of the rest) is exactly 0 with dh = 1 there: the kink, where the kernel's convention is pre > 0.  The
    prefills of dbeta / dbias are quarter-integers.  `mean` is NaN: the backward must not read it."""
    rng = _rng(k, tag)
    dh = _ints(rng, -1, 1, (k.rows, k.c))
    beta = _ints(rng, -4, 4, k.c) / np.float32(4)
    pre = _ints(rng, -8, 8, (k.rows, k.c)) / np.float32(4)
    pre[rng.random((k.rows, k.c)) < 0.1] = 0.0
    if k.rows > 1:
        pre[1] = 0.0
        dh[1] = 1.0
    pre[0] = beta
    rstd = np.float32(2.0) ** _ints(rng, -1, 1, k.c)
    return NS(dh=dh, pre=pre, beta=beta, rstd=rstd, old_dbeta=_ints(rng, -8, 8, k.c) / np.float32(4),
              old_dbias=_ints(rng, -8, 8, k.c) / np.float32(4))


def act_deriv_ref(pre, act):
    if act == ACT_RELU:
        return (pre > 0).astype(np.float64)
    if act == ACT_LRELU:
        return np.where(pre > 0, 1.0, LEAK)
    if act == ACT_TANH:
        return 1.0 - np.tanh(pre) ** 2
    return np.ones_like(pre)


def bn_bwd_ref(inp, act, dtype):
    """float64 dbeta / du of the batch-norm backward from crafted inputs, with every intermediate kept, and the bounds.

    du = rstd * ((dpre - m0) - xhat * m1), dpre = dh * act'(pre), xhat = pre - beta, m0 = mean(dpre), m1 = mean(dpre * xhat).
    none / relu / lrelu: dpre, xhat and both sums are exact (quarter-integer grid, the caps); only the two divisions by
    rows round: m_c = fl(s * fl(1 / rows)) (2 roundings in the accumulator type, + the cast to float for f32 tensors).
    Then fl(dpre - m0_c) and fl(xhat * m1_c) and their difference: m0 and xhat m1 each meet 2 more f32 roundings, dpre 2;
    rstd is a power of two.  tanh: t = tanhf(pre) is off by TANH_ULP ulps, t*t and 1 - t*t round once each; the terms then
    carry that error into sums of `rows` inexact terms, which any summation order keeps within gamma_(rows - 1) of the
    sum of their magnitudes (plus, for f32 tensors, the casts of the partial and of the result to float: 2 * 2**-24)."""
    rows = inp.dh.shape[0]
    dh, pre = inp.dh.astype(np.float64), inp.pre.astype(np.float64)
    beta, rstd = inp.beta.astype(np.float64), inp.rstd.astype(np.float64)
    ua = acc_u(dtype)
    f = act_deriv_ref(pre, act)
    dpre, xh = dh * f, pre - beta
    t1 = dpre * xh
    s0, s1 = dpre.sum(0), t1.sum(0)
    m0, m1 = s0 / rows, s1 / rows
    a_m0, a_xm1 = dpre - m0, xh * m1
    du = rstd * (a_m0 - a_xm1)
    if act == ACT_TANH:
        t = np.tanh(pre)
        tau = TANH_ULP * 2.0 ** -23
        e_tt = t * t * ((1 + tau) ** 2 * (1 + U32) - 1)
        e_f = e_tt + U32 * (np.abs(f) + e_tt)
        e_dpre = np.abs(dh) * e_f
        e_t1 = e_dpre * np.abs(xh) + U32 * (np.abs(t1) + e_dpre * np.abs(xh))
        g = gamma(max(rows - 1, 0), ua) + (2 * U32 if dtype == 0 else 0.0)
        e_s0 = e_dpre.sum(0) + g * (np.abs(dpre) + e_dpre).sum(0)
        e_s1 = e_t1.sum(0) + g * (np.abs(t1) + e_t1).sum(0)
    else:
        e_dpre = np.zeros_like(dpre)
        e_s0 = e_s1 = np.zeros_like(s0)
    gm = gamma(2, ua) + (U32 if dtype == 0 else 0.0)
    e_m0 = e_s0 / rows + gm * (np.abs(m0) + e_s0 / rows)
    e_m1 = e_s1 / rows + gm * (np.abs(m1) + e_s1 / rows)
    g2 = gamma(2, U32)
    e_du = rstd * (e_dpre + e_m0 + np.abs(xh) * e_m1
                   + g2 * (np.abs(dpre) + e_dpre + np.abs(m0) + e_m0) + g2 * np.abs(xh) * (np.abs(m1) + e_m1))
    return NS(dpre=dpre, xh=xh, t1=t1, s0=s0, s1=s1, m0=m0, m1=m1, a_m0=a_m0, a_xm1=a_xm1, du=du, rstd=rstd,
              du_bound=store_bound(e_du, du, dtype), dbeta_bound=e_s0)


def bn_bwd_caps(inp, act):
    """Conditions of the exact sums (none / relu / lrelu): terms of s0 on the 1/4 grid, of s1 on the 1/16 grid."""
    r = bn_bwd_ref(inp, act, 1)
    for v, what in ((inp.dh, 'dh'), (inp.pre, 'pre')):
        check_caps(v, 'bf16', what)
        assert np.array_equal(bf16_round(v), v), what
    on_grid(np.abs(r.dpre).sum(0) + np.abs(inp.old_dbeta), 0.25, 'sum |dpre|')
    on_grid(np.abs(r.t1).sum(0), 1.0 / 16, 'sum |dpre xhat|')
    assert np.array_equal(r.dpre * 4, np.rint(r.dpre * 4)) and np.array_equal(r.t1 * 16, np.rint(r.t1 * 16))


def du_intermediates_fit(inp, act):
    """Every f32 intermediate of du is representable (so fused or not, in any order, the kernel's du is the oracle's)."""
    r = bn_bwd_ref(inp, act, 1)
    rows = inp.dh.shape[0]
    return (rows & (rows - 1)) == 0 and all(fits_f32(v) for v in (r.m0, r.m1, r.a_m0, r.a_xm1, r.a_m0 - r.a_xm1, r.du))


def dbias_bound(du_stored):
    """|dbias - (dbias_acc * old + sum du)| <= (rows - 1) * 2**-24 * sum |du| per column, du the STORED tensor."""
    du = np.asarray(du_stored, dtype=np.float64)
    return (du.shape[0] - 1) * U32 * np.abs(du).sum(0)


# ------------------------------------------------------------------------------------------------ scalar reductions
def sumsq_sizes(dtype):
    vw = 4 if dtype == 0 else 8
    return (1, 3, 255, 256 * vw - 1, 256 * vw, 256 * 256 * vw + 5)


def tern(n, tag):
    return _ints(np.random.default_rng([tag, int(n)]), -1, 1, n)


GP_ROOTS = (3, 64, 724)           # n = root**2 elements of +-1: sqrt(sum x^2) is an integer away from 1


def gp_scalars_ref(ss, lam):
    s = np.sqrt(np.float64(ss))
    return np.array([(s - 1) ** 2, lam * 2 * (s - 1) / s])


SEG_LENGTHS = (1, 255, 256, 257, 1000)

# ------------------------------------------------------------------------------------------------ row ops
ROW_SHAPES = [(r, c) for c in (1, 7, 8, 1028, 2056) for r in (1, 3)] + [(4100, 8)]   # 4100 rows: past the 4096-block grid


def row_inputs(rows, cols):
    rng = np.random.default_rng([7, rows, cols])
    m = _ints(rng, -3, 3, (rows, cols))
    m[rng.random((rows, cols)) < 0.2] = 0.0                     # exact zeros in the mask source: the m > 0 convention
    return NS(x=_ints(rng, -3, 3, (rows, cols)), w=_ints(rng, -3, 3, cols), bias=_ints(rng, -3, 3, 1),
              dout=_ints(rng, -3, 3, rows), mask=m)


def rowdot_ref(inp):
    return inp.x.astype(np.float64) @ inp.w.astype(np.float64) + float(inp.bias[0])


def rowouter_ref(inp, masked):
    v = np.outer(inp.dout.astype(np.float64), inp.w.astype(np.float64))
    return v * np.where(inp.mask > 0, 1.0, LEAK) if masked else v


def row_caps(inp):
    check_caps(inp.x, 'bf16', 'x')
    check_caps(np.abs(inp.x).astype(np.float64) @ np.abs(inp.w).astype(np.float64) + 3.0, 'f32', 'rowdot')
    v = rowouter_ref(inp, True)
    check_caps(v, 'bf16', 'rowouter')
    assert np.array_equal(bf16_round(v.astype(np.float32)), v)


# ------------------------------------------------------------------------------------------------ NumPy restatements
# Of the kernels, block by block on the guarded flat buffer, for the CPU mutation check: each runs clean (and must then
# pass the same comparison the GPU result gets) and with ONE deliberate defect (and must then be rejected).

def restate_col_partial(flat, lay, g, mode, acc, defect=None, coef=None, pre_flat=None, beta=None, act=ACT_NONE):
    """col_partial_kernel: partial[blk][2][c] in float32 from accumulators of type `acc`.  mode: 'stats' | 'bwd' | 'sum' |
    'wsum'.  Defects: 'drop_last_row' (a ragged last block loses its last row), 'pad_read' (the last channel lane reads
    one column further), 'no_pivot' (raw moments instead of deviations from row 0)."""
    cols = np.arange(lay.c, dtype=np.int64)
    if defect == 'pad_read':
        cols[-1] += 1
    partial = np.zeros((g.nblk, 2, lay.c), dtype=np.float32)
    pivot = np.zeros(lay.c, dtype=np.float32) if (mode != 'stats' or defect == 'no_pivot') else flat[lay.off + cols]
    for b in range(g.nblk):
        r0 = b * g.rows_per_blk
        r1 = min(lay.rows, r0 + g.rows_per_blk)
        if defect == 'drop_last_row' and b == g.nblk - 1 and r1 - r0 != g.rows_per_blk:
            r1 -= 1
        idx = lay.off + np.arange(r0, r1, dtype=np.int64)[:, None] * lay.cs + cols[None, :]
        v = flat[idx]
        if mode == 'stats':
            d = (v - pivot).astype(np.float32)
            t0, t1 = d, (d * d).astype(np.float32)
        elif mode == 'bwd':
            p = pre_flat[idx]
            dpre = (v * act_deriv_ref(p.astype(np.float64), act).astype(np.float32)).astype(np.float32)
            t0, t1 = dpre, (dpre * (p - beta).astype(np.float32)).astype(np.float32)
        else:
            t0 = v if (mode == 'sum' or coef is None) else (v * coef[r0:r1, None]).astype(np.float32)
            t1 = np.zeros_like(t0)
        partial[b, 0] = t0.astype(acc).sum(0, dtype=acc)
        partial[b, 1] = t1.astype(acc).sum(0, dtype=acc)
    return partial


def restate_finalize_stats(partial, rows, pivot, acc, eps=EPS, defect=None):
    """col_finalize_kernel<FIN_BN_STATS>: (mean, rstd) in float32.  Defect 'no_clamp': the variance is not clamped at 0."""
    s0 = partial[:, 0].astype(acc).sum(0, dtype=acc)
    s1 = partial[:, 1].astype(acc).sum(0, dtype=acc)
    inv = acc(1) / acc(rows)
    md = s0 * inv
    var = s1 * inv - md * md
    if defect != 'no_clamp':
        var = np.maximum(var, acc(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        rstd = (1.0 / np.sqrt(var.astype(np.float64) + float(np.float32(eps)))).astype(np.float32)
    return (pivot.astype(acc) + md).astype(np.float32), rstd


def restate_finalize_sum(partial, acc, old=None):
    s = partial[:, 0].astype(acc).sum(0, dtype=acc)
    return (s if old is None else old.astype(acc) + s).astype(np.float32)


def restate_sumsq(x, vw, defect=None):
    """sumsq_partial_kernel on an aligned base: n // vw vectors, then the scalar tail.  Defect 'drop_tail': no tail loop."""
    nv = len(x) // vw
    s = (x[:nv * vw].astype(np.float32) ** 2).sum(dtype=np.float32)
    if defect != 'drop_tail':
        s += (x[nv * vw:].astype(np.float32) ** 2).sum(dtype=np.float32)
    return np.float32(s)


def restate_rowdot(x, w, bias, defect=None):
    """rowdot_kernel.  Defect 'drop_last_col': the column loop stops one short."""
    n = x.shape[1] - (1 if defect == 'drop_last_col' else 0)
    return ((x[:, :n] * w[None, :n]).astype(np.float32).sum(1, dtype=np.float32) + bias[0]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ instance norm
# tdg_instance_norm_fwd / _bwd: the one normalisation that reduces in f32 for both dtypes.  Per (image, channel):
#   d = u - u[0],  md = fl(s0 / hw),  var = max(fl(fl(s1 / hw) - fl(md md)), 0),  mu = fl(u[0] + md),  rstd = rsqrtf(fl(var + eps)).
# The tables keep s0 and s1 exact (integers below 2**24, asserted on the CPU); everything behind them goes through the Ev
# algebra of tests/_exact_pointwise.py (imported inside the functions: that module imports this one).
IN_CASES = [(1, 1, 1), (2, 4, 64), (3, 5, 65), (2, 64, 63), (1, 4100, 3), (2, 16, 130)]         # (n, hw, c)
IN_ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH)
IN_OUTLIER = 200.0
IN_SCALES = (0.5, 1.0, 2.0, -1.0, 1.5, -0.5)
IN_SHIFTS = (0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0)          # never 0: a constant column's pre is its shift


def in_id(k):
    return 'n%d-hw%d-c%d' % tuple(k)


def in_strides(c):
    """(cs, h_cs, dh_cs): all above c, all different."""
    return c + 3, c + 1, c + 6


def in_outlier_column(c):
    return c - 2 if c >= 6 else None


def in_sum_depth(hw):
    """A row lane's serial run (every fourth position), then sh[0] + sh[1] + sh[2] + sh[3]."""
    return -(-hw // 4) + 3


def in_inputs(k, tag=50):
    """u[b, :, j] = BASES[j % 5] + integers in [-3, 3]; the last column constant (c >= 6: the variance is 0 and rstd comes from
    eps alone), the one before it integers in [-3, 3] whose FIRST position is +-200 (the pivot is the outlier and does not
    help); scale from IN_SCALES, shift from IN_SHIFTS, dh and the dscale / dshift prefills eighths in [-1, 1]."""
    n, hw, c = k
    rng = _rng(k, tag)
    base = np.array([BASES[j % 5] for j in range(c)], dtype=np.float32)
    u = base[None, None, :] + _ints(rng, -3, 3, (n, hw, c))
    if const_column(c) is not None:
        u[:, :, const_column(c)] = base[const_column(c)]
        oc = in_outlier_column(c)
        u[:, :, oc] = _ints(rng, -3, 3, (n, hw))
        u[:, 0, oc] = IN_OUTLIER * np.where(np.arange(n) % 2 == 0, 1, -1)
    pick = lambda pool: np.asarray(pool, dtype=np.float32)[rng.integers(0, len(pool), c)]          # noqa: E731
    return NS(u=u, scale=pick(IN_SCALES), shift=pick(IN_SHIFTS), dh=_ints(rng, -8, 8, (n, hw, c)) / np.float32(8),
              old_dscale=_ints(rng, -8, 8, c) / np.float32(8), old_dshift=_ints(rng, -8, 8, c) / np.float32(8))


def in_stats_ref(u):
    """float64 moments per (image, channel) as deviations from the image's first position (exact: integers)."""
    u = u.astype(np.float64)
    d = u - u[:, :1]
    hw = u.shape[1]
    s0, s1 = d.sum(1), (d * d).sum(1)
    md = s0 / hw
    return NS(s0=s0, s1=s1, hw=hw, pivot=u[:, 0], md=md, e2=s1 / hw, mean=u[:, 0] + md, var=s1 / hw - md * md,
              abs0=np.abs(d).sum(1))


def in_caps(inp):
    st = in_stats_ref(inp.u)
    check_caps(inp.u, 'bf16', 'u')
    check_caps(st.abs0, 'f32', 'sum |d|')
    check_caps(st.s1, 'f32', 'sum d^2')
    for v in (inp.u, inp.scale, inp.shift, inp.dh, inp.old_dscale, inp.old_dshift):
        assert np.array_equal(bf16_round(v), v)


def in_mu_ref(st):
    """(mu, bound): fl(pivot + fl(s0 / hw)) from the exact s0."""
    from _exact_pointwise import Ev, add, div
    mu = add(Ev(st.pivot), div(Ev(st.s0), float(st.hw)))
    return mu.v, mu.e


def in_rstd_interval(st, eps):
    """rstd_interval restated for the f32 path: var through two divisions, a product and a subtraction (Ev), the clamp (it
    moves the device's variance towards the true one, which is >= 0, and leaves fl(var + eps) >= eps), one addition and
    rsqrtf at RSQRT_ULP.  rsqrt falls with its argument.  Returns (rstd, lo, hi, amplification)."""
    from _exact_pointwise import Ev, add, sub, mul, div, RSQRT_ULP, ULP, f32c
    md, e2 = div(Ev(st.s0), float(st.hw)), div(Ev(st.s1), float(st.hw))
    var = sub(e2, mul(md, md))
    e = f32c(eps)
    arg = add(Ev(np.maximum(var.v, 0.0), var.e), e)
    rstd = 1.0 / np.sqrt(arg.v)
    lo = (1.0 - RSQRT_ULP * ULP) / np.sqrt(arg.v + arg.e)
    hi = (1.0 + RSQRT_ULP * ULP) / np.sqrt(np.maximum(arg.v - arg.e, e))
    return rstd, lo, hi, (st.e2 + st.md * st.md) / np.maximum(st.var, e)


def _in_pre(inp, mu, rstd):
    """xhat = fl(fl(u - mu) rstd) and the backward's pre = fl(fl(scale xhat) + shift) at the given f32 statistics."""
    from _exact_pointwise import Ev, add, sub, mul
    xh = mul(sub(Ev(inp.u), Ev(np.asarray(mu, np.float64)[:, None, :])), Ev(np.asarray(rstd, np.float64)[:, None, :]))
    return xh, add(mul(Ev(inp.scale), xh), Ev(inp.shift))


def in_apply_ref(inp, mu, rstd, act, dtype):
    """h = act(fl(fl(fl(scale fl(u - mu)) rstd) + shift)) in float64 at the DEVICE's statistics (read back), as bn_apply_ref
    does: (reference, bound).  none / relu / lrelu (leak 0.25: an exact product) are 1-Lipschitz and round nothing."""
    from _exact_pointwise import Ev, add, sub, mul, ev_tanh, stored
    x = sub(Ev(inp.u), Ev(np.asarray(mu, np.float64)[:, None, :]))
    pre = add(mul(mul(Ev(inp.scale), x), Ev(np.asarray(rstd, np.float64)[:, None, :])), Ev(inp.shift))
    h = ev_tanh(pre) if act == ACT_TANH else type(pre)(act_ref(pre.v, act), pre.e)
    return stored(h, dtype)


def _ev_sum(t, axis, depth):
    from _exact_pointwise import Ev, TINY
    return Ev(t.v.sum(axis), t.e.sum(axis) + gamma(depth, U32) * (np.abs(t.v) + t.e).sum(axis) + TINY)


def in_bwd_ref(inp, mu, rstd, act, dtype, beta):
    """Every output of tdg_instance_norm_bwd at the given statistics: du [n, hw, c] (reference, bound), dscale and dshift [c]
    (reference, bound; beta * old added), and `kink`: min(|pre| - its bound) over the tensor, which must be positive for
    relu / lrelu -- their derivative is read off the sign of pre.  g = dh act'(pre); s0 = sum g, s1 = sum g xhat per image
    through the kernel's tree (in_sum_depth); du = fl(scale rstd) * ((g - s0 / hw) - xhat * (s1 / hw)); the images' partials
    meet in the finalize kernel: n additions, the prefill's, one cast."""
    from _exact_pointwise import Ev, sub, mul, div, ev_tanh, stored
    n, hw, c = inp.u.shape
    xh, pre = _in_pre(inp, mu, rstd)
    if act == ACT_TANH:
        t = ev_tanh(pre)
        f = sub(1.0, mul(t, t))
    else:
        f = Ev(act_deriv_ref(pre.v, act))
    g = mul(Ev(inp.dh), f)
    t1 = mul(g, xh)
    s0, s1 = _ev_sum(g, 1, in_sum_depth(hw)), _ev_sum(t1, 1, in_sum_depth(hw))
    wide = lambda s: Ev(s.v[:, None, :], s.e[:, None, :])                                            # noqa: E731
    m0, m1 = wide(div(s0, float(hw))), wide(div(s1, float(hw)))
    du = mul(mul(Ev(inp.scale), Ev(np.asarray(rstd, np.float64)[:, None, :])), sub(sub(g, m0), mul(xh, m1)))
    out = NS(kink=float((np.abs(pre.v) - pre.e).min()), g=g.v, s0=s0.v)
    out.du, out.du_bound = stored(du, dtype)
    for name, s, old in (('dscale', s1, inp.old_dscale), ('dshift', s0, inp.old_dshift)):
        o = beta * old.astype(np.float64)
        setattr(out, name, s.v.sum(0) + o)
        setattr(out, name + '_bound', s.e.sum(0) + gamma(n + 2, U32) * ((np.abs(s.v) + s.e).sum(0) + np.abs(o)))
    return out


def in_kink_margin(inp, eps):
    """The kink condition without a device: min over the tensor of |pre| - (its rounding bound + what the intervals of mu and
    rstd can move it by), pre at the float64 statistics."""
    st = in_stats_ref(inp.u)
    mu, e_mu = in_mu_ref(st)
    rstd, lo, hi, _ = in_rstd_interval(st, eps)
    _, pre = _in_pre(inp, mu, rstd)
    d_rstd = np.maximum(hi - rstd, rstd - lo)
    x = np.abs(inp.u.astype(np.float64) - mu[:, None, :])
    moved = np.abs(inp.scale.astype(np.float64)) * (x * d_rstd[:, None, :] + e_mu[:, None, :] * (rstd + d_rstd)[:, None, :])
    return float((np.abs(pre.v) - pre.e - moved * (1 + 2.0 ** -20)).min())


def restate_in_stats(u, eps, defect=None, sums=None):
    """instance_norm_fwd_kernel's statistics in f32: (mu, rstd) [n, c].  Defects: 'no_pivot' (raw moments), 'no_clamp' (the
    variance is not clamped at 0).  sums: (s0, s1, hw, pivot) in place of a tensor."""
    f = np.float32
    if sums is None:
        pivot = np.zeros_like(u[:, 0]) if defect == 'no_pivot' else u[:, 0]
        d = (u - pivot[:, None]).astype(f)
        s0, s1, hw = d.sum(1, dtype=f), (d * d).astype(f).sum(1, dtype=f), u.shape[1]
    else:
        s0, s1, hw, pivot = (np.asarray(sums[0], f), np.asarray(sums[1], f), sums[2], np.asarray(sums[3], f))
    md = (s0 / f(hw)).astype(f)
    var = ((s1 / f(hw)).astype(f) - (md * md).astype(f)).astype(f)
    if defect != 'no_clamp':
        var = np.maximum(var, f(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        rstd = (f(1) / np.sqrt((var + f(eps)).astype(f))).astype(f)
    return (pivot + md).astype(f), rstd


def restate_in_bwd_sums(inp, mu, rstd, act, defect=None):
    """(dscale, dshift) of instance_norm_bwd_kernel in f32 at beta = 0.  Defect 'swapped': each lands in the other's vector."""
    f = np.float32
    xh = ((inp.u - mu[:, None, :]).astype(f) * rstd[:, None, :]).astype(f)
    pre = ((inp.scale * xh).astype(f) + inp.shift).astype(f)
    g = (inp.dh * act_deriv_ref(pre.astype(np.float64), act).astype(f)).astype(f)
    dshift, dscale = g.sum((0, 1), dtype=f), (g * xh).astype(f).sum((0, 1), dtype=f)
    return (dshift, dscale) if defect == 'swapped' else (dscale, dshift)
