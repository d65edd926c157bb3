"""Inputs, float64 references and bounds for the optimizer steps and the Philox draws of csrc/tdg_elementwise.hip (pure
NumPy, no GPU here).  The recipe, the Ev algebra and the helpers are those of tests/_exact_pointwise.py; its three rules
apply unchanged:

1. Exact where exactness is provable.  With small-integer g, grad_scale 0.5 and decay = rho = momentum = 0.5 (lr a power
   of two for the plain momentum step) every term of an accumulator is representable and so is their sum: rms, mg and the
   acc of Adagrad, Adadelta and FTRL, and all of tdg_sgd_momentum_step, must equal the float64 reference under
   np.array_equal, fused multiply-add or not.  u01(x) = (x >> 8) * 2**-24 is exact in f32, so the uniform draw must equal
   the NumPy Philox4x32-10 of this file bit for bit.  tests/test_host_steps_exact.py asserts the conditions on reference
   values and pins the Philox to its published known answers.

2. Derived bounds elsewhere (p, mom, acc_update, linear, the accumulators at the training defaults, the normal draw): the
   float64 reference follows the kernel's expression operation by operation in class Ev.  Cosine and sine join the device
   functions with the OpenCL 1.2 full-profile limit of 4 ulp; they are not monotone, so the operand's error is passed on
   with Lipschitz constant 1.  No constant here is fitted to a device result.

3. Guards.  g is NaN outside its live region, p and every slot carry the sentinel there, the draws' outputs are
   sentinel-guarded; nothing outside [base, base + n) may change and g must keep its bits.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np

import _exact_pointwise as P
from _exact_pointwise import Ev, add, sub, mul, div, ev_sqrt, ev_log, f32c, f32, flat_blocks   # noqa: F401
from _exact_cols import store, bound_ratio, fits_f32, on_grid, NAN, SENTINEL                    # noqa: F401

SIN_ULP = COS_ULP = 4             # OpenCL 1.2 specification, section 7.4, full profile (as LOG_ULP etc. of _exact_pointwise)
F32, BF16 = P.F32, P.BF16


# ================================================================================================ optimizer steps
GS = 0.5                                                  # grad_scale: a dropped scale shows
TABLE = 4096                                              # every case is a prefix of its kernel's table
STEP_CASES = [(4, 0), (2052, 0), (2052, 4)]               # (n, elements in front of the base): 1 block, 3 blocks, base offset
STEP_BIG_N = 4 * (4096 * 512) + 4 * 300                   # past the 4096-block cap of ew_blocks(n / 4, 512): two more trips, the last ragged
# The big case tiles the first BIG_PERIOD elements of a table.  Each trip starts 4096 * 256 vectors after the one before;
# a period of 4096 elements would divide that, and a trip that read another trip's elements would find the same values.
# 4 * 4096 * 256 = 1025 * 4092 + 4: with this period every trip is one vector out of step with the one before.
BIG_PERIOD = 4092
CFGS = ('exact', 'train')
L1, L2 = 0.25, 0.125

# name -> entry point, its pointer arguments in order, its float arguments in order (grad_scale follows them)
STEPS = {
    'rmsprop': NS(entry='tdg_rmsprop_step', arrays=('p', 'g', 'rms', 'mom'), floats=('lr', 'decay', 'mu', 'eps'), exact=('rms',)),
    'rmsprop_centered': NS(entry='tdg_rmsprop_centered_step', arrays=('p', 'g', 'mg', 'rms', 'mom'), floats=('lr', 'decay', 'mu', 'eps'),
                           exact=('rms', 'mg')),
    'adagrad': NS(entry='tdg_adagrad_step', arrays=('p', 'g', 'acc'), floats=('lr',), exact=('acc',)),
    'adadelta': NS(entry='tdg_adadelta_step', arrays=('p', 'g', 'acc', 'acc_update'), floats=('lr', 'rho', 'eps'), exact=('acc',)),
    'ftrl': NS(entry='tdg_ftrl_step', arrays=('p', 'g', 'acc', 'linear'), floats=('lr', 'l1', 'l2'), exact=('acc',)),
    'ftrl_l1': NS(entry='tdg_ftrl_step', arrays=('p', 'g', 'acc', 'linear'), floats=('lr', 'l1', 'l2'), exact=('acc',)),
    'sgd': NS(entry='tdg_sgd_momentum_step', arrays=('p', 'g', 'acc'), floats=('lr', 'mu'), exact=('p', 'acc')),
}
STEP_NAMES = tuple(STEPS)
BIG_STEPS = ('rmsprop', 'rmsprop_centered', 'adagrad', 'adadelta', 'ftrl_l1', 'sgd')     # one big launch per kernel


def outputs_of(name):
    return tuple(a for a in STEPS[name].arrays if a != 'g')


def hyper(name, cfg):
    """'exact': powers of two.  'train': the defaults of engine.py (decay 0.9, eps 1e-10, momentum 0.3; Adadelta rho 0.95,
    eps 1e-8)."""
    ex = cfg == 'exact'
    h = NS(lr=0.125 if ex else 1e-2, decay=0.5 if ex else 0.9, mu=0.5 if ex else 0.3, eps=1e-10, rho=0.5 if ex else 0.95, l1=0.0, l2=0.0)
    if name == 'adadelta':
        h.eps = 1e-8
    if name.startswith('ftrl'):
        h.lr = 0.125 if ex else 0.1                       # lin = O(1): both sides of |lin| > l1 occur
    if name == 'ftrl_l1':
        h.l1, h.l2 = L1, L2
    return h


def step_floats(name, h):
    return tuple(getattr(h, k) for k in STEPS[name].floats) + (GS,)


TINY_AT = (1, 5)                                          # rmsprop, 'exact': rms = 0 and g = 2**-20, where eps decides the root


def step_inputs(name, cfg):
    """The kernel's 4096-element table as a dict of f32 arrays.  'exact': integers and eighths; rms >= mg**2 + 1 for the
    centered step; FTRL's linear slot on odd eighths (never 0 or +-l1, so g == 0 leaves it clear of the kink).  'train':
    normal p and g, the slots as engine.py creates them (rms 1, accumulators 0.1, the rest 0); ftrl_l1 has g == 0 at every
    seventh element."""
    rng = P._rng(40, STEP_NAMES.index(name), CFGS.index(cfg))
    n = TABLE
    ints = lambda lo, hi: P._ints(rng, lo, hi, n)                                           # noqa: E731
    const = lambda v: np.full(n, v, dtype=np.float32)                                       # noqa: E731
    d = {}
    if cfg == 'exact':
        d['p'] = ints(-8, 8) if name == 'sgd' else ints(-8, 8) / f32(8)
        d['g'] = ints(-6, 6)
        if name == 'rmsprop':
            d['rms'], d['mom'] = ints(0, 4), ints(-4, 4) / f32(8)
            for i in TINY_AT:
                d['rms'][i], d['g'][i] = 0.0, 2.0 ** -20
        elif name == 'rmsprop_centered':
            d['mg'] = ints(-4, 4) / f32(4)
            d['rms'], d['mom'] = d['mg'] * d['mg'] + ints(1, 4), ints(-4, 4) / f32(8)
        elif name == 'adagrad':
            d['acc'] = ints(1, 4)
        elif name == 'adadelta':
            d['acc'], d['acc_update'] = ints(0, 4), ints(0, 8) / f32(8)
        elif name.startswith('ftrl'):
            d['acc'], d['linear'] = ints(1, 4), (f32(2) * ints(-4, 3) + f32(1)) / f32(8)
        else:
            d['acc'] = ints(-4, 4)
    else:
        d['p'], d['g'] = (rng.standard_normal(n).astype(np.float32) for _ in range(2))
        if name.startswith('rmsprop'):
            d['rms'], d['mom'] = const(1.0), const(0.0)
            if name == 'rmsprop_centered':
                d['mg'] = const(0.0)
        elif name == 'adagrad':
            d['acc'] = const(0.1)
        elif name == 'adadelta':
            d['acc'], d['acc_update'] = const(0.0), const(0.0)
        elif name.startswith('ftrl'):
            d['acc'], d['linear'] = const(0.1), const(0.0)
            if name == 'ftrl_l1':
                d['g'][::7] = 0.0
        else:
            d['acc'] = const(0.0)
    return d


def prefix(table, n, period=TABLE):
    """The case of length n: the table's first n elements, or its first `period` elements tiled."""
    return {k: np.resize(v[:period], n) for k, v in table.items()}


def step_ref(name, inp, h):
    """One launch: every output array as an Ev, following the kernel's expression.  Also `kink` (FTRL: elements whose
    reference |lin| lies within its own bound of l1 -- the tables must hold none) and `root` (centered RMSProp: the
    argument of the square root)."""
    x = {k: Ev(v) for k, v in inp.items()}
    gv = mul(f32c(GS), x['g'])
    out = NS(kink=None, root=None)
    if name.startswith('rmsprop'):
        lr, decay, mu, eps = f32c(h.lr), f32c(h.decay), f32c(h.mu), f32c(h.eps)
        omd = sub(1.0, decay)
        rv = add(mul(decay, x['rms']), mul(mul(omd, gv), gv))
        if name == 'rmsprop_centered':
            av = add(mul(decay, x['mg']), mul(omd, gv))
            out.root = add(sub(rv, mul(av, av)), eps)
        else:
            out.root = add(rv, eps)
        mv = add(mul(mu, x['mom']), div(mul(lr, gv), ev_sqrt(out.root)))
        out.out = dict(p=sub(x['p'], mv), rms=rv, mom=mv)
        if name == 'rmsprop_centered':
            out.out['mg'] = av
    elif name == 'adagrad':
        av = add(x['acc'], mul(gv, gv))
        out.out = dict(p=sub(x['p'], div(mul(f32c(h.lr), gv), ev_sqrt(av))), acc=av)
    elif name == 'adadelta':
        lr, rho, eps = f32c(h.lr), f32c(h.rho), f32c(h.eps)
        omr = sub(1.0, rho)
        av = add(mul(rho, x['acc']), mul(mul(omr, gv), gv))
        u = mul(div(ev_sqrt(add(x['acc_update'], eps)), ev_sqrt(add(av, eps))), gv)
        uv = add(mul(rho, x['acc_update']), mul(mul(omr, u), u))
        out.out = dict(p=sub(x['p'], mul(lr, u)), acc=av, acc_update=uv)
    elif name.startswith('ftrl'):
        lr, l1, l2 = f32c(h.lr), f32c(h.l1), f32c(h.l2)
        an = add(x['acc'], mul(gv, gv))
        sn, so = ev_sqrt(an), ev_sqrt(x['acc'])
        lin = add(x['linear'], sub(gv, mul(div(sub(sn, so), lr), x['p'])))
        quad = add(div(sn, lr), mul(2.0, l2))
        taken = div(sub(mul(np.sign(lin.v), l1), lin), quad)
        on = np.abs(lin.v) > l1
        out.kink = np.abs(np.abs(lin.v) - l1) <= lin.e
        out.out = dict(p=Ev(np.where(on, taken.v, 0.0), np.where(on, taken.e, 0.0)), acc=an, linear=lin)
    else:
        a = add(mul(f32c(h.mu), x['acc']), gv)
        out.out = dict(p=sub(x['p'], mul(f32c(h.lr), a)), acc=a)
    return out


def is_exact(name, cfg, arr):
    return cfg == 'exact' and arr in STEPS[name].exact


def tiled_ratio(got, v, e):
    """bound_ratio of a result of any length against a reference it is a tiling of."""
    t = len(v)
    m = len(got) // t * t
    return np.concatenate([bound_ratio(got[:m].reshape(-1, t), v[None, :], e[None, :]).ravel(), bound_ratio(got[m:], v[:len(got) - m], e[:len(got) - m])])


def step_ratios(name, cfg, got, ref):
    """THE comparison, for the device's result and for the restatements alike: per output array the per-element
    |error| / bound; for an exact output 0 where the bits equal store(reference) and inf where they do not.  `got` may be a
    tiling of the reference's period (the big case)."""
    r = {}
    for arr in outputs_of(name):
        x = ref.out[arr]
        if is_exact(name, cfg, arr):
            r[arr] = np.where(got[arr] == np.resize(store(x.v, F32), len(got[arr])), 0.0, np.inf)
        else:
            r[arr] = tiled_ratio(got[arr], x.v, x.e)
    return r


def accepted(ratios):
    return all(bool(np.all(v <= 1.0)) for v in ratios.values())


STEP_DEFECTS = {
    'rmsprop': ('eps_outside_root', 'one_vector_short'),
    'rmsprop_centered': ('mg_not_squared', 'old_mg_in_root'),
    'adagrad': ('acc_without_g2',),
    'adadelta': ('u_from_old_acc',),
    'ftrl': (),
    'ftrl_l1': ('l1_ignored', 'sign_dropped'),
    'sgd': ('gs_dropped',),
}


def restate_step(name, inp, h, defect=None):
    """One launch in float32 NumPy: dict of the output arrays.  Defects: 'eps_outside_root' (sqrtf(rms) + eps),
    'mg_not_squared' (rms - mg + eps), 'old_mg_in_root' (the root sees the mg of before this step), 'acc_without_g2' (acc
    is stored as it was read), 'u_from_old_acc' (acc_update is built from the update the OLD acc would give), 'l1_ignored'
    (p = -lin / quad whatever |lin|), 'sign_dropped' ((l1 - lin) / quad), 'gs_dropped', 'one_vector_short' (the loop ends
    one float4 early: the last four elements keep what they held)."""
    one = f32(1)
    gs = one if defect == 'gs_dropped' else f32(GS)
    gv = gs * inp['g']
    with np.errstate(divide='ignore', invalid='ignore'):
        if name.startswith('rmsprop'):
            lr, decay, mu, eps = f32(h.lr), f32(h.decay), f32(h.mu), f32(h.eps)
            rv = decay * inp['rms'] + (one - decay) * gv * gv
            if name == 'rmsprop_centered':
                av = decay * inp['mg'] + (one - decay) * gv
                used = inp['mg'] if defect == 'old_mg_in_root' else av
                root = np.sqrt(rv - (used if defect == 'mg_not_squared' else used * used) + eps)
            else:
                root = np.sqrt(rv) + eps if defect == 'eps_outside_root' else np.sqrt(rv + eps)
            mv = mu * inp['mom'] + lr * gv / root
            out = dict(p=inp['p'] - mv, rms=rv, mom=mv)
            if name == 'rmsprop_centered':
                out['mg'] = av
        elif name == 'adagrad':
            av = inp['acc'] + gv * gv
            out = dict(p=inp['p'] - f32(h.lr) * gv / np.sqrt(av), acc=inp['acc'] if defect == 'acc_without_g2' else av)
        elif name == 'adadelta':
            lr, rho, eps = f32(h.lr), f32(h.rho), f32(h.eps)
            av = rho * inp['acc'] + (one - rho) * gv * gv
            u = np.sqrt(inp['acc_update'] + eps) / np.sqrt(av + eps) * gv
            u_acc = np.sqrt(inp['acc_update'] + eps) / np.sqrt(inp['acc'] + eps) * gv if defect == 'u_from_old_acc' else u
            out = dict(p=inp['p'] - lr * u, acc=av, acc_update=rho * inp['acc_update'] + (one - rho) * u_acc * u_acc)
        elif name.startswith('ftrl'):
            lr, l1, l2 = f32(h.lr), f32(h.l1), f32(h.l2)
            an = inp['acc'] + gv * gv
            sn, so = np.sqrt(an), np.sqrt(inp['acc'])
            lv = inp['linear'] + (gv - (sn - so) / lr * inp['p'])
            quad = sn / lr + f32(2) * l2
            sgn = one if defect == 'sign_dropped' else np.sign(lv).astype(np.float32)
            if defect == 'l1_ignored':
                p = -lv / quad
            else:
                p = np.where(np.abs(lv) > l1, (sgn * l1 - lv) / quad, f32(0))
            out = dict(p=p, acc=an, linear=lv)
        else:
            a = f32(h.mu) * inp['acc'] + gv
            out = dict(p=inp['p'] - f32(h.lr) * a, acc=a)
    out = {k: v.astype(np.float32) for k, v in out.items()}
    if defect == 'one_vector_short':
        for k in out:
            out[k][-4:] = inp[k][-4:]
    return out


def step_blocks(n):
    """(blocks, capped) of an optimizer launch -- labelling only."""
    return flat_blocks(n // 4, 512)


# ================================================================================================ Philox4x32-10
M32 = np.uint64(0xffffffff)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
PHILOX_DEFECTS = ('nine_rounds', 'key_not_advanced', 'counter_high_dropped', 'words_1_3_swapped')


def philox_words(c, k, defect=None):
    """Philox4x32-10 on counter words c = (c0, c1, c2, c3) and key words k = (k0, k1), each a uint64 array (or scalar)
    holding 32-bit values: the four output words, shape (..., 4), uint32."""
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) & M32 for w in c)
    k0, k1 = (np.asarray(w, dtype=np.uint64) & M32 for w in k)
    for _ in range(9 if defect == 'nine_rounds' else 10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        if defect != 'key_not_advanced':
            k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    if defect == 'words_1_3_swapped':
        c1, c3 = c3, c1
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def philox(seed, stream_id, offset, count, defect=None):
    """The words of counters offset .. offset + count - 1 (mod 2**64) of stream `stream_id` under key `seed`: (count, 4)."""
    ctr = np.uint64(offset) + np.arange(count, dtype=np.uint64)
    hi = np.zeros_like(ctr) if defect == 'counter_high_dropped' else ctr >> np.uint64(32)
    sid, key = np.uint64(stream_id), np.uint64(seed)
    return philox_words((ctr, hi, sid, sid >> np.uint64(32)), (key, key >> np.uint64(32)), defect)


def u01(w, shift=8):
    """(x >> 8) * 2**-24 in float64: exact, and exact in f32."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(shift)).astype(np.float64) * 2.0 ** -24


def uniform_ref(seed, stream_id, offset, n, defect=None):
    w = philox(seed, stream_id, offset, (n + 3) // 4, defect)
    return u01(w.reshape(-1)[:n], 9 if defect == 'shift_9' else 8).astype(np.float32)


TWO_PI = f32c(6.283185307179586)


def box_muller(words, n):
    """Box-Muller per word pair as the kernel writes it, on (count, 4) Philox words: the first n values as one Ev."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1, 2)
    u1, u2 = 1.0 - u01(w[:, 0]), u01(w[:, 1])                       # both exact in f32
    r = ev_sqrt(mul(-2.0, ev_log(Ev(u1))))
    t = mul(TWO_PI, Ev(u2))
    c = Ev(np.cos(t.v), P._rounded(np.cos(t.v), t.e, COS_ULP))       # |cos'| <= 1: the operand's error passes on unchanged
    s = Ev(np.sin(t.v), P._rounded(np.sin(t.v), t.e, SIN_ULP))
    z0, z1 = mul(r, c), mul(r, s)
    both = lambda a, b: np.stack([a, b], axis=1).reshape(-1)[:n]                             # noqa: E731
    return Ev(both(z0.v, z1.v), both(z0.e, z1.e))


@functools.lru_cache(maxsize=2)
def normal_ev(seed, stream_id, offset, n):
    """The draw as one Ev; kept, since the f32 and the bf16 comparison of a case share it (it is never changed)."""
    return box_muller(philox(seed, stream_id, offset, (n + 3) // 4), n)


def normal_ref(seed, stream_id, offset, n, dtype):
    """(reference, bound) of the stored draw."""
    return P.stored(normal_ev(seed, stream_id, offset, n), dtype)


def restate_normal(seed, stream_id, offset, n, dtype, defect=None):
    """random_normal_kernel in float32 NumPy.  Defects: those of the Philox, and 'u1_is_u01' (u1 = u01(w0) without 1 -)."""
    w = philox(seed, stream_id, offset, (n + 3) // 4, defect if defect in PHILOX_DEFECTS else None).reshape(-1, 2)
    a, b = u01(w[:, 0]).astype(np.float32), u01(w[:, 1]).astype(np.float32)
    u1 = a if defect == 'u1_is_u01' else f32(1) - a
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.sqrt(f32(-2) * np.log(u1)).astype(np.float32)
        t = (f32(6.283185307179586) * b).astype(np.float32)
        z = np.stack([r * np.cos(t), r * np.sin(t)], axis=1).astype(np.float32).reshape(-1)[:n]
    return store(z, dtype)


def rng_blocks(n):
    """(blocks, capped, ticket level) of a draw of n values -- labelling only."""
    b, capped = flat_blocks((n + 3) // 4, 256)
    return b, capped, ('one-level' if b <= 64 else 'two-level')


SEED, SEED_HI = 1234, 0x9E3779B97F4A7C15                  # the second: high 32 bits set
SID_NORMAL, SID_UNIFORM = (0 << 8) | 1, (0 << 8) | 2      # runtime.py: (rank << 8) | 1 and | 2
SID_HI = (0x5EED << 40) | (3 << 8) | 1                    # high 32 bits set
RNG_N = (1, 3, 4, 5, 1024 * 64, 1024 * 65 + 2)            # the tail, and 64 / 66 blocks: either side of the ticket levels
RNG_BIG_N = 4 * (4096 * 256) + 6                          # past the block cap, with a tail
RNG_BIG_OFFSET = 1 << 24                                  # draw 0 of the _dev forms: one reference serves both forms
DRAW_WINDOW = 1 << 26                                     # values per draw of the _dev forms


def draw_offset(d):
    return (d + 1) << 24


# (seed, stream_id, offset, n, elements in front of the base)
RNG_CASES = [(SEED, SID_NORMAL, 0, n, 0) for n in RNG_N] + [
    (SEED, SID_UNIFORM, 0, 5, 1),                         # the base one element off
    (SEED_HI, SID_NORMAL, 0, 261, 0),
    (SEED, SID_HI, 0, 261, 0),
    (SEED, SID_UNIFORM, 2 ** 32 - 2, 16, 0),              # the counter carries into its high word in mid-launch
    (SEED, SID_NORMAL, 257 << 24, 16, 0),
]
RNG_IDS = ['n%d' % c[3] for c in RNG_CASES[:len(RNG_N)]] + ['base-off', 'seed-hi', 'stream-hi', 'carry', 'offset-257']
DEV_DRAWS = (0, 254, 255, 256, 2 ** 20)                   # (d + 1) << 24 first needs the high word at d = 255
DEV_ORDERS = (('normal', 'uniform', 'normal_bf16'), ('uniform', 'normal', 'uniform'))
DEV_SIZES = (1024 * 64, 1024 * 65 + 2, 5)                 # per launch of an order: each entry meets both ticket levels
