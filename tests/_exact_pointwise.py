"""Inputs, float64 references and bounds for the loss, seed and pointwise kernels of csrc/tdg_elementwise.hip and for
tdg_cgan_join (pure NumPy, no GPU here).  The rules are those of tests/_exact_cols.py:

1. Exact where exactness is provable.  Inputs are small integers, eighths or powers of two, the lrelu leak is 0.25, keep
   probabilities, scales and the row counts that are divided by are powers of two.  Every intermediate is then
   representable in f32 (so a fused multiply-add gives the same bits as a multiply and an add) and every stored value is
   either representable in its storage type or the correctly rounded image of an exactly known f32 value: the device must
   equal store(float64 reference, dtype) under np.array_equal.  tests/test_host_pointwise_exact.py asserts the conditions
   on reference values for the whole case table.

2. Derived bounds where it is not (log, exp, log1p, tanh, pow, sqrt of a non-square, 1 / (1e-8 + x), divisors that are no
   power of two, sums of inexact terms).  The reference is float64 on exactly the bytes the kernel reads (every input is
   bf16-representable, so both dtypes read the same numbers; f32 constants such as 1e-8f enter as float64(float32(.))).
   The bound follows the kernel's expression operation by operation (class Ev): each f32 operation adds half an ulp of
   the largest magnitude its result can have -- 2**-24 (|value| + error so far) -- and passes the operands' errors on by
   the operation's own sensitivity; a device function adds its OpenCL full-profile ulp limit instead of the half ulp; a
   sum of n inexact terms adds gamma(depth, 2**-24) * sum(|term| + error), depth = the most additions any term passes
   through in the kernel's reduction tree; a bf16 store adds half a bf16 ulp (store_bound).  A fused multiply-add rounds
   once where the count has two, which only lowers the error.  Results below 2**-126 may be flushed (denormal support is
   optional in the profile): every rounding carries that absolute floor.  No constant here is fitted to a device result.

3. Guards.  Every input is NaN outside its live region (padding channels, a band of rows behind, the elements in front of
   an offset base), every output is prefilled with the sentinel, and nothing outside the live region may change.  The two
   in-place kernels (dropout, the dg of p2p_l1) carry the sentinel in their padding, and it must survive.
"""
from types import SimpleNamespace as NS

import numpy as np

from _exact_conv import LEAK, check_caps, describe_mismatch                                     # noqa: F401
from _exact_cols import (Layout, store, bf16_round, bf16_half_ulp, store_bound, gamma, bound_ratio, fits_f32, on_grid,   # noqa: F401
                         NAN, SENTINEL, U32, U64, TANH_ULP)

# OpenCL 1.2 specification, section 7.4 "Relative error as ULPs", full profile, single precision -- the limits the ROCm
# device library (ocml) is built to, as tests/_exact_cols.py already takes for tanh (TANH_ULP = 5)
LOG_ULP = 3
EXP_ULP = 3
LOG1P_ULP = 2
POW_ULP = 16
SQRT_ULP = 3
DIV_ULP = 2.5
RSQRT_ULP = 2                     # rsqrt in the same table (section 7.4, full profile, single precision): <= 2 ulp
ULP = 2.0 ** -23                  # ulp(x) <= 2**-23 |x|
TINY = 2.0 ** -126                # the smallest normal f32: results below it may be flushed
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4      # include/tdg.h (the host test ties them to _lib)
F32, BF16 = 0, 1
ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID)
EXACT_ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU)
ACT_NAME = {0: 'none', 1: 'relu', 2: 'lrelu', 3: 'tanh', 4: 'sigmoid'}
GUARD = float(np.float32(1e-8))   # the kernels' 1e-8f


def f32c(x):
    """A kernel constant or scalar argument as the float32 the device sees, in float64."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ error propagation
class Ev:
    """A float64 reference value `v` of an f32 quantity with a bound `e` on |device value - v|."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.asarray(e, dtype=np.float64) + np.zeros_like(self.v)


def lift(x):
    return x if isinstance(x, Ev) else Ev(x)


def _rounded(v, e, ulps=0.5):
    """The error after an operation whose exact-arithmetic result is known to `e` and which is `ulps` ulps accurate."""
    return e + ulps * np.maximum(ULP * (np.abs(v) + e), TINY)


def add(a, b):
    a, b = lift(a), lift(b)
    return Ev(a.v + b.v, _rounded(a.v + b.v, a.e + b.e))


def sub(a, b):
    a, b = lift(a), lift(b)
    return Ev(a.v - b.v, _rounded(a.v - b.v, a.e + b.e))


def mul(a, b):
    a, b = lift(a), lift(b)
    return Ev(a.v * b.v, _rounded(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e))


def div(a, b):
    """a / b: |a'/b' - a/b| <= (ea + |a/b| eb) / (|b| - eb), then DIV_ULP ulps."""
    a, b = lift(a), lift(b)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = a.v / b.v
        room = np.abs(b.v) - b.e
        e = np.where(room > 0, (a.e + np.abs(v) * b.e) / room, np.inf)
    return Ev(v, _rounded(v, e, DIV_ULP))


def neg(a):
    a = lift(a)
    return Ev(-a.v, a.e)


def mono(a, f, ulps):
    """A monotone device function: the operand's error moves the result by at most the larger one-sided difference."""
    a = lift(a)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        v = f(a.v)
        e = np.maximum(np.abs(f(a.v + a.e) - v), np.abs(v - f(a.v - a.e)))
        e = np.where(a.e == 0, 0.0, e)
    return Ev(v, _rounded(v, e, ulps))


def ev_log(a):
    return mono(a, np.log, LOG_ULP)


def ev_exp(a):
    return mono(a, np.exp, EXP_ULP)


def ev_log1p(a):
    return mono(a, np.log1p, LOG1P_ULP)


def ev_tanh(a):
    return mono(a, np.tanh, TANH_ULP)


def ev_sqrt(a):
    return mono(a, lambda x: np.sqrt(np.maximum(x, 0.0)), SQRT_ULP)


def ev_rsqrt(a):
    """rsqrtf of a positive argument (monotone decreasing)."""
    return mono(a, lambda x: 1.0 / np.sqrt(np.maximum(x, 0.0)), RSQRT_ULP)


def ev_pow(base, t):
    """powf of exact arguments."""
    v = np.power(np.float64(base), np.float64(t))
    return Ev(v, _rounded(v, 0.0, POW_ULP))


def ev_sigmoid(a):
    """1.f / (1.f + expf(-v)) as apply_act writes it."""
    return div(1.0, add(1.0, ev_exp(neg(a))))


def stored(x, dtype):
    """(reference, bound) of an Ev after the store to `dtype`."""
    return x.v, store_bound(x.e, x.v, dtype) + (TINY if dtype == BF16 else 0.0)


def sum_bound(t, depth):
    """A sum of the terms `t` (Ev) in which no term passes through more than `depth` f32 additions."""
    mag = np.abs(t.v) + t.e
    return Ev(t.v.sum(), t.e.sum() + gamma(depth, U32) * mag.sum() + TINY)


BLOCK_SUM_DEPTH = 9               # block_sum256: 6 wave shuffles, then sh[0] + sh[1] + sh[2] + sh[3]
RED_BLOCKS = 256


def one_block_depth(n):
    """A 256-thread single-block reduction of n terms: the thread's own trips, then block_sum256."""
    return -(-n // 256) + BLOCK_SUM_DEPTH


def two_stage_depth(items, adds_per_item=1):
    """RED_BLOCKS x 256 threads over `items`, then the 256 partials by one block."""
    return -(-items // (RED_BLOCKS * 256)) * adds_per_item + BLOCK_SUM_DEPTH + 1 + BLOCK_SUM_DEPTH


# ------------------------------------------------------------------------------------------------ labelling predicates
# Restated launch geometry, used ONLY to label cases and to check that the tables reach every branch -- never to compute
# an expected value.
def flat_blocks(n, per_block=1024):
    """ew_blocks(): (blocks, capped)."""
    b = max(1, -(-n // per_block))
    return min(b, 4096), b > 4096


def ticket_level(n):
    """adam_step_dev: blocks of 512 float4, one-level tickets up to 64 blocks, two-level above."""
    b, _ = flat_blocks(n // 4, 512)
    return b, ('one-level' if b <= 64 else 'two-level')


def cast_rows_branch(c):
    return 'c<=16' if c <= 16 else 'c>16'


# ------------------------------------------------------------------------------------------------ generators
def _rng(*tag):
    return np.random.default_rng([int(t) for t in tag])


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def _pick(rng, pool, shape):
    """Values of `pool`, drawn at random, with the pool itself laid over the first elements (as many as fit): a one-element
    tensor gets pool[0], anything longer than the pool holds every value of it."""
    pool = np.asarray(pool, dtype=np.float32)
    a = rng.choice(pool, size=shape).astype(np.float32)
    n = min(a.size, pool.size)
    a.reshape(-1)[:n] = pool[:n]
    return a


def act_ref(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_LRELU:
        return np.maximum(LEAK * v, v)
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def act_ev(v, act):
    """apply_act on an exact f32 argument."""
    if act == ACT_TANH:
        return ev_tanh(Ev(v))
    if act == ACT_SIGMOID:
        return ev_sigmoid(Ev(v))
    return Ev(act_ref(np.asarray(v, np.float64), act))


# ================================================================================================ flat pointwise (exact)
FLAT_N = (1, 255, 256, 257, 1025)
BIG_N = 4096 * 1024 + 257                      # past the 4096-block cap of ew_blocks(): the grid-stride loop's second trip
FLAT_CASES = [(n, 0) for n in FLAT_N] + [(257, 1)]                    # (n, elements in front of the base)
TIES = np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -7, 0.0])    # cast_from_f32 to bf16
TIES_BF16 = np.float32([1.0, 1 + 2.0 ** -6, -1.0, 1 + 2.0 ** -7, 0.0])
CLAMPS = ((-1.0, 2.0), (0.5, 0.5))


def flat_layout(n, off=0):
    return Layout(n, 1, 1, off, band=16)


def add_act_inputs(n):
    rng = _rng(11, n)
    return NS(a=_ints(rng, -6, 6, n), b=_ints(rng, -6, 6, n))


def add_act_ref(inp, act, dtype):
    """(reference, bound); bound None: exact."""
    v = inp.a.astype(np.float64) + inp.b.astype(np.float64)
    if act in EXACT_ACTS:
        return act_ref(v, act), None
    return stored(act_ev(v, act), dtype)


def act_bwd_inputs(n):
    """post: eighths in [-1, 1] with +0.0 and -0.0; dy = +-2**j, j in [-2, 2]."""
    rng = _rng(12, n)
    post = _pick(rng, np.concatenate([[0.0, -0.0], np.arange(-8, 9) / 8.0]), n)
    dy = (np.float32(2.0) ** _ints(rng, -2, 2, n)) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)
    return NS(dy=dy, post=post)


def act_bwd_ref(inp, act):
    p, dy = inp.post.astype(np.float64), inp.dy.astype(np.float64)
    f = {ACT_NONE: np.ones_like(p), ACT_RELU: (p > 0).astype(np.float64), ACT_LRELU: np.where(p > 0, 1.0, LEAK),
         ACT_TANH: 1.0 - p * p, ACT_SIGMOID: p * (1.0 - p)}[act]
    return NS(f=f, dx=dy * f)


def scale_inputs(n):
    return NS(x=_ints(_rng(13, n), -8, 8, n))


SCALE_COEFS = (0.5, -4.0)


def cast_inputs(n):
    """Eighths in [-4, 4] (bf16-representable) for cast_to_f32; for cast_from_f32 the ties lead."""
    rng = _rng(14, n)
    x = _ints(rng, -32, 32, n) / np.float32(8)
    t = x.copy()
    t[:min(n, len(TIES))] = TIES[:min(n, len(TIES))]
    return NS(x=x, ties=t)


AFFINE_SCALE, AFFINE_SHIFT = 2.0, -0.5


def affine_inputs(shape, tag=15):
    """k / 256, k in [0, 255]: scale * (x + shift) = (k - 128) / 128 fits 8 significant bits."""
    return _ints(_rng(tag, *np.atleast_1d(shape)), 0, 255, shape) / np.float32(256)


def affine_ref(x):
    return AFFINE_SCALE * (x.astype(np.float64) + AFFINE_SHIFT)


def clamp_inputs(n, lo, hi):
    return _pick(_rng(16, n), [lo, hi, lo - 1, hi + 1, lo - 0.125, hi + 0.125, 0.5 * (lo + hi), 0.0], n)


FILL_VALUE = 0.375

# ================================================================================================ strided pointwise (exact)
BIAS_ACT_SHAPES = [(1, 3), (3, 3), (4100, 3), (3, 1), (3, 8), (3, 257), (3, 300)]       # 4100 rows: past the 4096-block grid


BIAS_GIVEN = (False, True)


def strides_of(c):
    return sorted({c, (c + 7) // 8 * 8, c + 5})


def bias_act_inputs(rows, c):
    rng = _rng(17, rows, c)
    return NS(x=_ints(rng, -6, 6, (rows, c)), bias=_ints(rng, -6, 6, c))


def bias_act_ref(inp, with_bias, act, dtype):
    v = inp.x.astype(np.float64) + (inp.bias.astype(np.float64)[None, :] if with_bias else 0.0)
    if act in EXACT_ACTS:
        return act_ref(v, act), None
    return stored(act_ev(v, act), dtype)


CAST_ROWS_C = (1, 3, 4, 6, 16, 17, 24)
CAST_ROWS_ROWS = (1, 257, 1030)
PAIR_SPLITS = ((3, 1), (1, 3), (2, 2))

DROPOUT_KEEPS = (1.0, 0.5, 0.25)
DROPOUT_C = (1, 7, 200)
DROPOUT_ROWS = 5


def dropout_inputs(c, keep):
    """y integers in [-8, 8] without 0; u on the 1/1024 grid, led by 1 - keep (kept), 1 - keep - 1/1024 (dropped; absent at
    keep = 1, where it would be negative) and 0."""
    rng = _rng(18, c, int(keep * 1024))
    y = _ints(rng, 1, 8, (DROPOUT_ROWS, c)) * np.where(rng.random((DROPOUT_ROWS, c)) < 0.5, -1, 1).astype(np.float32)
    lead = [1 - keep, 0.0] + ([1 - keep - 1 / 1024] if keep < 1 else [])
    u = _ints(rng, 0, 1023, DROPOUT_ROWS * c) / np.float32(1024)
    u[:len(lead)] = lead
    return NS(y=y, u=u, lead=lead)


def dropout_ref(y, u, keep):
    kept = np.floor(keep + u.astype(np.float64)).reshape(y.shape)
    return y.astype(np.float64) * kept / keep


GP_INTERP_ROWS = (1, 3, 4100)
GP_INTERP_COLS = (1, 7, 300)


def gp_interp_inputs(rows, cols):
    rng = _rng(19, rows, cols)
    return NS(x=_ints(rng, -8, 8, (rows, cols)), g=_ints(rng, -8, 8, (rows, cols)),
              alpha=_pick(rng, np.concatenate([[0.0, 1.0], np.arange(9) / 8.0]), rows))


def gp_interp_ref(inp):
    x, g = inp.x.astype(np.float64), inp.g.astype(np.float64)
    return x + inp.alpha.astype(np.float64)[:, None] * (g - x)


JOIN_C = (8, 24)
JOIN_N_RGB = 3
JOIN_RUNS = ((0, 6, True), (1, 6, True), (1, 3, False))         # (mode, rows, rgb given)


def join_strides(c):
    """(comb, rgb, depth): multiples of 8, all different, none equal to c."""
    return 2 * c + 24, c + 8, c + 16


def join_inputs(c, rows):
    rng = _rng(20, c, rows)
    return NS(comb=_ints(rng, -8, 8, (rows, 2 * c)), rgb=_ints(rng, -8, 8, (JOIN_N_RGB, c)), depth=_ints(rng, -8, 8, (rows, c)))


def join_fwd_ref(inp):
    rows = inp.depth.shape[0]
    return np.concatenate([inp.rgb[np.arange(rows) % JOIN_N_RGB], inp.depth], axis=1).astype(np.float64)


def join_bwd_ref(inp):
    """(depth, rgb) of mode 1; rgb None where the tensor has no second half (rows < 2 n_rgb: the rgb == NULL call)."""
    c = inp.depth.shape[1]
    comb = inp.comb.astype(np.float64)
    if comb.shape[0] < 2 * JOIN_N_RGB:
        return comb[:, c:], None
    return comb[:, c:], comb[:JOIN_N_RGB, :c] + comb[JOIN_N_RGB:2 * JOIN_N_RGB, :c]


# ================================================================================================ VAE
VAE_L = (1, 7, 100)
VAE_ROWS = (1, 3, 40)
SD_POOL = (0.0, 2.0 ** -10, -2.0 ** -10, 1.0, 0.5, -0.5, 2.0, 1.5, -1.0)


def vae_strides(L):
    """(hs, es, zs): all different, each above its minimum."""
    return 2 * L + 3, L + 1, L + 2


def reparam_inputs(rows, L):
    """mean integers in [-4, 4], sd in {0, 0.5, 1, 2}, eps and dz integers in [-4, 4]."""
    rng = _rng(21, rows, L)
    return NS(m=_ints(rng, -4, 4, (rows, L)), sd=_pick(rng, [0.0, 0.5, 1.0, 2.0], (rows, L)), eps=_ints(rng, -4, 4, (rows, L)),
              dz=_ints(rng, -4, 4, (rows, L)))


def reparam_ref(inp):
    return inp.m.astype(np.float64) + inp.sd.astype(np.float64) * inp.eps.astype(np.float64)


def reparam_bwd_ref(inp):
    g = inp.dz.astype(np.float64)
    return np.concatenate([g, g * inp.eps.astype(np.float64)], axis=1)


def kl_inputs(rows, L, tag=22):
    """mean eighths in [-2, 2] led by 0, sd from SD_POOL (0: the log(1e-8) term; +-2**-10; 1), eps and dz as above."""
    rng = _rng(tag, rows, L)
    return NS(m=_pick(rng, np.concatenate([[0.0], np.arange(-16, 17) / 8.0]), (rows, L)), sd=_pick(rng, SD_POOL, (rows, L)),
              eps=_ints(rng, -4, 4, (rows, L)), dz=_ints(rng, -4, 4, (rows, L)))


def reparam_bwd_kl_ref(inp, klw, dtype):
    """gm = g + klw * m; gs = g * eps + klw * (sd - sd / (1e-8f + sd * sd)).  (reference, bound) over [gm | gs]."""
    g, m, sd, eps = (Ev(a) for a in (inp.dz, inp.m, inp.sd, inp.eps))
    gm = add(g, mul(klw, m))
    gs = add(mul(g, eps), mul(klw, sub(sd, div(sd, add(GUARD, mul(sd, sd))))))
    both = Ev(np.concatenate([gm.v, gs.v], axis=1), np.concatenate([gm.e, gs.e], axis=1))
    return stored(both, dtype)


VAE_KL_SHAPES = [(1, 1), (257, 1), (700, 100)]            # rows * L = 1, 257, 70000 (past 256 blocks * 256 threads)


def vae_kl_ref(inp):
    """0.5 * sum(m*m + sd*sd - log(1e-8f + sd*sd) - 1): (reference, bound) of the scalar."""
    m, sd = Ev(inp.m), Ev(inp.sd)
    ss = mul(sd, sd)
    t = sub(sub(add(mul(m, m), ss), ev_log(add(GUARD, ss))), 1.0)
    s = mul(0.5, sum_bound(t, two_stage_depth(t.v.size)))
    return float(s.v), float(s.e)


BCE_ROWS = (1, 257, 70000)
BCE_C = (1, 3)
BCE_CS = 8


def bce_inputs(rows, c):
    rng = _rng(23, rows, c)
    return NS(x=_pick(rng, [0.0, 1.0, 0.25], (rows, c)), d=_pick(rng, [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0 ** -7, 0.5, 0.5], (rows, c)))


def bce_ref(inp, dtype, guard=True):
    """loss = -sum(x log(1e-8f + d) + (1 - x) log(1e-8f + (1 - d))), seed = -(x / (1e-8f + d) - (1 - x) / (1e-8f + (1 - d)))."""
    x, d = Ev(inp.x), Ev(inp.d)
    e = GUARD if guard else 0.0
    a, b = add(e, d), add(e, sub(1.0, d))
    omx = sub(1.0, x)
    t = add(mul(x, ev_log(a)), mul(omx, ev_log(b)))
    loss = sum_bound(t, two_stage_depth(inp.x.shape[0], inp.x.shape[1]))
    seed = neg(sub(div(x, a), div(omx, b)))
    sv, sb = stored(seed, dtype)
    return NS(loss=-float(loss.v), loss_bound=float(loss.e), seed=sv, seed_bound=sb)


# ================================================================================================ losses and seeds
L1_CASES = [(1, 1), (1024, 1), (257, 1), (5, 3), (300, 3)]       # (rows, c); rows * c a power of two: (1, 1), (1024, 1)
L1_CS = 8


def l1_inputs(rows, c):
    """x = k / 256, d eighths in [-1, 1]: u = 2 (x - 0.5) - d lies on the 1/128 grid, both signs, with u == 0 wherever x is
    0.5 + d / 2 -- every fourth element is made so."""
    rng = _rng(24, rows, c)
    d = _ints(rng, -7, 7, (rows, c)) / np.float32(8)
    x = affine_inputs((rows, c), tag=25)
    zero = rng.random((rows, c)) < 0.25
    zero.reshape(-1)[0] = rows * c > 1
    x[zero] = (0.5 + d[zero] / 2).astype(np.float32)
    return NS(x=x, d=d)


def l1_ref(inp, dtype):
    rows, c = inp.x.shape
    u = affine_ref(inp.x) - inp.d.astype(np.float64)
    inv_n = float(np.float32(1.0) / (np.float32(rows) * np.float32(c)))       # computed on the host: IEEE
    s = np.abs(u).sum()
    n = rows * c
    pow2 = n & (n - 1) == 0
    return NS(u=u, sum=s, inv_n=inv_n, seed=-np.sign(u) * inv_n, pow2=pow2, loss=s / n,
              loss_bound=None if pow2 else gamma(2, U32) * s / n)


P2P_L1_ROWS = (1, 256, 257, 70000)
P2P_CS, P2P_DGS = 8, 3
P2P_WEIGHT = 100.0
DG_GIVEN = (True, False)                                        # dg == NULL: the loss alone


def p2p_l1_inputs(rows):
    rng = _rng(26, rows)
    y = _ints(rng, -4, 4, rows)
    g = _ints(rng, -4, 4, rows)
    g[::5] = y[::5]                                                  # d == 0: no update
    return NS(y=y, g=g, dg=_ints(rng, -4, 4, rows))


def p2p_l1_ref(inp, dtype):
    rows = len(inp.y)
    d = 0.5 * (inp.g.astype(np.float64) - inp.y.astype(np.float64))
    a, q = np.abs(d).sum(), (d * d).sum()
    pow2 = rows & (rows - 1) == 0
    upd = mul(P2P_WEIGHT * 0.5 * np.sign(d), div(1.0, float(rows)))
    new = add(Ev(inp.dg), upd)
    rms = ev_sqrt(div(q, float(rows)))
    mean = div(a, float(rows))
    dgv, dgb = stored(new, dtype)
    return NS(d=d, a=a, q=q, pow2=pow2, dg=dgv, dg_bound=dgb, scal=np.array([mean.v, rms.v]), scal_bound=np.array([mean.e, rms.e]))


XENT_ROWS = (1, 255, 256, 257, 1000)
XENT_CS = (1, 8)
XENT_RUNS = ((0, True), (0, False), (1, True), (2, True))       # (mode, seed given): mode 0 accepts seed == NULL
LOGIT_POOL = (0.0, 2.0 ** -10, -2.0 ** -10, 30.0, -30.0, 88.0, -88.0, 1.0, -0.5, 3.0, -2.0, 0.125)


def xent_inputs(rows):
    rng = _rng(27, rows)
    z = _pick(rng, LOGIT_POOL, 2 * rows)
    if rows == 1:
        z[:] = (88.0, -0.5)                      # (two saturated logits would make the halves indistinguishable)
    return NS(z=z)


def _softplus_neg_abs(z):
    return ev_log1p(ev_exp(neg(Ev(np.abs(z.v)))))


def xent_ref(inp, mode, dtype):
    """scal = (mean softplus(-zr), mean softplus(zf), mean softplus(-zf)); seeds of channel 0 as [real half | fake half]."""
    rows = len(inp.z) // 2
    zr, zf = Ev(inp.z[:rows]), Ev(inp.z[rows:])
    sr, sf = _softplus_neg_abs(zr), _softplus_neg_abs(zf)
    pos = lambda z: np.maximum(z.v, 0.0)                                                    # noqa: E731
    terms = (add(sub(pos(zr), zr), sr), add(pos(zf), sf), add(sub(pos(zf), zf), sf))
    inv = div(1.0, float(rows))
    scal = [mul(sum_bound(t, one_block_depth(rows)), inv) for t in terms]
    out = NS(scal=np.array([float(s.v) for s in scal]), scal_bound=np.array([float(s.e) for s in scal]))
    if mode:
        pr, pf = ev_sigmoid(zr), ev_sigmoid(zf)
        if mode == 1:
            real, fake = mul(sub(pr, 1.0), inv), mul(pf, inv)
        else:
            real, fake = Ev(np.zeros(rows)), mul(sub(pf, 1.0), inv)
        both = Ev(np.concatenate([real.v, fake.v]), np.concatenate([real.e, fake.e]))
        out.seed, out.seed_bound = stored(both, dtype)
        if mode == 2:
            out.seed_bound[:rows] = 0.0                                                     # exact zeros in the real half
    return out


LOGLOSS_N = (1, 255, 256, 257, 1000)
SCORE_POOL = (0.0, 1.0, 0.5, 2.0 ** -20, 0.125, 0.875, 0.25, 0.75)


def logloss_inputs(n):
    rng = _rng(28, n)
    return NS(dr=_pick(rng, SCORE_POOL, n), df=_pick(rng, SCORE_POOL[::-1] if n > 1 else (1.0,), n))


def logloss_ref(inp):
    n = len(inp.dr)
    r, f = Ev(inp.dr), Ev(inp.df)
    inv = div(1.0, float(n))
    omf = sub(1.0, f)
    ld = sub(neg(ev_log(add(r, GUARD))), ev_log(add(omf, GUARD)))
    lg = neg(ev_log(add(f, GUARD)))
    scal = [mul(sum_bound(t, one_block_depth(n)), inv) for t in (ld, lg)]
    sr = mul(mul(div(neg(inv), add(r, GUARD)), r), sub(1.0, r))
    sfd = mul(mul(div(inv, add(omf, GUARD)), f), omf)
    sfg = mul(mul(div(neg(inv), add(f, GUARD)), f), omf)
    return NS(scal=np.array([float(s.v) for s in scal]), scal_bound=np.array([float(s.e) for s in scal]), seeds=(sr, sfd, sfg))


GP_LAMBDA = 8.0
GP_ROWS_EXACT = [(r, c) for r in (1, 4) for c in (1, 4, 64, 4096)]       # slopes 1, 2, 8, 64
GP_ROWS_BOUNDED = [(3, 7), (4100, 4)]


def gp_rows_inputs(rows, cols):
    return NS(v=np.where(_rng(29, rows, cols).random((rows, cols)) < 0.5, -1, 1).astype(np.float32))


def gp_rows_ref(inp, dtype):
    """pen = (sqrt(ss) - 1)^2, u = lambda 2 (sl - 1) / (sl rows) * v; ss = cols exactly (rows of +-1)."""
    rows, cols = inp.v.shape
    root = int(round(np.sqrt(cols)))
    sl = Ev(float(root)) if root * root == cols else ev_sqrt(Ev(float(cols)))
    d = sub(sl, 1.0)
    pen = mul(d, d)
    coef = div(mul(GP_LAMBDA * 2.0, d), mul(sl, float(rows)))
    u = mul(Ev(np.full((rows, 1), coef.v), np.full((rows, 1), coef.e)), Ev(inp.v))
    uv, ub = stored(u, dtype)
    return NS(pen=np.full(rows, pen.v), pen_bound=np.full(rows, pen.e), u=uv, u_bound=ub)


# ================================================================================================ Adam and utilities
ADAM_N = (4, 2052, 4 * 512 * 64, 4 * 512 * 65)           # 1, 2, 64 and 65 blocks: the last two at and past the one-level tickets
ADAM_T0 = (0, 9)
ADAM = NS(lr=1e-3, b1=0.5, b2=0.9, eps=1e-8, gs=0.5)


def adam_inputs(n):
    rng = _rng(30, n)
    f = lambda a: a.astype(np.float32)                                                      # noqa: E731
    return NS(p=f(rng.standard_normal(n)), g=f(rng.standard_normal(n)), m=f(0.1 * rng.standard_normal(n)),
              v=f(rng.standard_normal(n) ** 2))


def adam_lr_t(t, on_host=False):
    """lr * sqrtf(1 - powf(b2, t)) / (1 - powf(b1, t)) as the kernel computes it; on_host: float64, rounded once to f32."""
    lr, b1, b2 = f32c(ADAM.lr), f32c(ADAM.b1), f32c(ADAM.b2)
    if on_host:
        v = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        return Ev(f32c(v))
    return div(mul(lr, ev_sqrt(sub(1.0, ev_pow(b2, t)))), sub(1.0, ev_pow(b1, t)))


def adam_ref(inp, lr_t):
    """One step of the rule, each of m, v, p as an Ev, from an Ev of lr_t."""
    b1, b2, eps, gs = f32c(ADAM.b1), f32c(ADAM.b2), f32c(ADAM.eps), f32c(ADAM.gs)
    gv = mul(gs, Ev(inp.g))
    m = add(mul(b1, Ev(inp.m)), mul(sub(1.0, b1), gv))
    v = add(mul(b2, Ev(inp.v)), mul(mul(sub(1.0, b2), gv), gv))
    p = sub(Ev(inp.p), div(mul(lr_t, m), add(ev_sqrt(v), eps)))
    return NS(m=m, v=v, p=p)


FINITE_N = (1, 257, 1 << 20)
BAD_VALUES = (float('nan'), float('inf'), -float('inf'))


def finite_positions(n):
    return sorted({0, n - 1, n // 2})


ADD_I32_INCS = (0, 3, -2)


# ================================================================================================ NumPy restatements
# Of the kernels in float32, for the CPU mutation check: each runs clean (and must then pass the comparison the GPU
# result gets) and with ONE named defect (and must then be rejected, on the table's own inputs).
f32 = np.float32


def restate_affine_cast_rows(x, cs, dtype, defect=None):
    """Returns the guarded flat output.  Defect 'cs_for_c': the input row is found with cs where c belongs."""
    rows, c = x.shape
    lay = Layout(rows, c, cs)
    flat_in = np.concatenate([x.ravel(), np.full(rows * cs, NAN, f32)])
    stride = cs if defect == 'cs_for_c' else c
    v = np.stack([flat_in[r * stride:r * stride + c] for r in range(rows)])
    out = np.full(lay.n, SENTINEL, f32)
    out[lay.idx] = store(f32(AFFINE_SCALE) * (v + f32(AFFINE_SHIFT)), dtype)
    return lay, out


def restate_bias_act(x, bias, cs, act, dtype, defect=None):
    """Defect 'pad_written': the channel loop runs to cs."""
    rows, c = x.shape
    lay = Layout(rows, c, cs)
    out = np.full(lay.n, SENTINEL, f32)
    out[lay.idx] = store(act_ref((x + bias[None, :]).astype(np.float64), act), dtype)
    if defect == 'pad_written':
        pad = lay.off + np.arange(rows)[:, None] * cs + np.arange(c, cs)[None, :]
        out[pad] = 0.0
    return lay, out


def restate_add_act(a, b, act, dtype, defect=None):
    """Defect 'drop_last': the flat loop stops one element short."""
    n = len(a)
    lay = flat_layout(n)
    out = np.full(lay.n, SENTINEL, f32)
    m = n - 1 if defect == 'drop_last' else n
    out[:m] = store(act_ref((a[:m] + b[:m]).astype(np.float64), act), dtype)
    return lay, out


def restate_act_bwd(dy, post, act, defect=None):
    """Defect 'ge_at_zero': the relu / lrelu mask is post >= 0."""
    on = post >= 0 if defect == 'ge_at_zero' else post > 0
    f = {ACT_RELU: on.astype(f32), ACT_LRELU: np.where(on, f32(1), f32(LEAK)), ACT_NONE: np.ones_like(post),
         ACT_TANH: f32(1) - post * post, ACT_SIGMOID: post * (f32(1) - post)}[act]
    return (dy * f).astype(f32)


def restate_l1(x, d, dtype, defect=None):
    """(loss, seed).  Defects: 'sign0_is_1' (sign(0) = 1), 'inv_rows' (inv_n = 1 / rows)."""
    rows, c = x.shape
    inv_n = f32(1) / (f32(rows) * (f32(1) if defect == 'inv_rows' else f32(c)))
    u = (f32(AFFINE_SCALE) * (x + f32(AFFINE_SHIFT)) - d).astype(f32)
    sgn = np.where(u > 0, f32(-1), np.where(u < 0, f32(1), f32(-1) if defect == 'sign0_is_1' else f32(0)))
    return f32(np.abs(u).sum(dtype=f32) * inv_n), store(sgn * inv_n, dtype)


def restate_xent_seeds(z, mode, dtype, defect=None):
    """Defect 'halves_swapped': the real rows get the fake rows' seeds and the other way round."""
    rows = len(z) // 2
    inv = f32(1) / f32(rows)
    with np.errstate(over='ignore'):
        p = (f32(1) / (f32(1) + np.exp(-z.astype(f32)))).astype(f32)
    real = (p[:rows] - f32(1)) * inv if mode == 1 else np.zeros(rows, f32)
    fake = p[rows:] * inv if mode == 1 else (p[rows:] - f32(1)) * inv
    if defect == 'halves_swapped':
        real, fake = fake, real
    return store(np.concatenate([real, fake]), dtype)


def restate_p2p_l1_dg(y, g, dg, dtype, defect=None):
    """Defect 'overwrite': dg = update instead of dg += update."""
    rows = len(y)
    d = f32(0.5) * (g - y)
    upd = (f32(P2P_WEIGHT) * f32(0.5) * np.sign(d).astype(f32) * (f32(1) / f32(rows))).astype(f32)
    return store(upd if defect == 'overwrite' else dg + upd, dtype)


def restate_bce_seed(x, d, dtype, defect=None):
    """Defect 'no_guard': the 1e-8 is missing from both denominators."""
    e = f32(0) if defect == 'no_guard' else f32(1e-8)
    with np.errstate(divide='ignore', invalid='ignore'):
        return store(-(x / (e + d) - (f32(1) - x) / (e + (f32(1) - d))), dtype)


def restate_adam(inp, t_dev, defect=None):
    """(p, m, v) after one adam_step_dev launch.  Defect 'count_after_increment': the step is t_dev + 2."""
    lr, b1, b2, eps, gs = (f32(ADAM.lr), f32(ADAM.b1), f32(ADAM.b2), f32(ADAM.eps), f32(ADAM.gs))
    t = f32(t_dev + (2 if defect == 'count_after_increment' else 1))
    lr_t = f32(lr * np.sqrt(f32(1) - np.power(b2, t)) / (f32(1) - np.power(b1, t)))
    gv = gs * inp.g
    m = b1 * inp.m + (f32(1) - b1) * gv
    v = b2 * inp.v + (f32(1) - b2) * gv * gv
    p = inp.p - lr_t * m / (np.sqrt(v) + eps)
    return p.astype(f32), m.astype(f32), v.astype(f32)
