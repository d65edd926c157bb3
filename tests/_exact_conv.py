"""Integer-valued conv inputs whose answers a correct kernel must reproduce bit for bit (no GPU here).

With inputs in {-1, 0, 1} every bf16 product is exact and every f32 accumulation is exact while the sums stay below
2**24; with the lrelu leak a power of two the activation and the mask stay exact too.  Every value the device stores is
then exactly representable in its storage type, so a kernel must equal the float64 oracle (oracle/tf_ops.py) whatever
its tile shape, K order, split count or slab order: a dropped, doubled or misplaced term moves an integer by >= 1.

The only conditions are the two magnitude caps of `check_caps`, asserted on the ORACLE before anything is compared.
They are not tolerances: a case that breaks one gets a smaller keep probability `q`, the caps stay.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import tf_ops as T

LEAK = 0.25                 # a power of two: lrelu and its mask are exact on quarter-integers
BF16_CAP = 256.0            # |v| <= 256 for everything stored as bf16 (8 significant bits hold every integer up to it)
F32_CAP = float(2 ** 24)    # |v| < 2**24 for everything accumulated or stored as f32
KEEP_TERMS = 600.0          # expected non-zero filter entries per reduction: sums of ~N(0, 600 * 2/3) stay far below the cap


def geometry(case, padding='SAME'):
    """(oh, ow, pad_t, pad_l) of a case (n, h, w, cin, cout, k, stride)."""
    n, h, w, cin, cout, k, s = case
    if padding == 'SAME':
        oh, pt, _ = T.same_pad(h, k, s)
        ow, pl, _ = T.same_pad(w, k, s)
        return oh, ow, pt, pl
    return T.valid_out(h, k, s), T.valid_out(w, k, s), 0, 0


def keep_prob(case):
    """q = min(1, 600 / R), R the longest reduction of the forward (k*k*cin) and backward-data (ceil(k/s)^2 * cout) GEMMs."""
    n, h, w, cin, cout, k, s = case
    R = max(k * k * cin, (-(-k // s)) ** 2 * cout)
    return min(1.0, KEEP_TERMS / R)


def exact_inputs(case, seed=0, padding='SAME', q=None):
    """x, dy, the masks and the prefills uniform in {-1, 0, 1} (zeros exercise the m == 0 side of a mask), biases integers
    in [-3, 3], W in {-1, 0, 1} with each entry kept with probability q (default keep_prob(case)).  float32 arrays;
    `prefill.small` / `prefill.big` are laid out like the small / big side tensors."""
    n, h, w, cin, cout, k, s = case
    oh, ow, _, _ = geometry(case, padding)
    rng = np.random.default_rng([seed] + [int(v) for v in case] + [len(padding)])
    q = keep_prob(case) if q is None else q

    def tern(*shape):
        return rng.integers(-1, 2, size=shape).astype(np.float32)
    big, small = (n, h, w, cin), (n, oh, ow, cout)
    keep = rng.random((k, k, cin, cout)) < q
    return SimpleNamespace(
        x=tern(*big), W=tern(k, k, cin, cout) * keep, dy=tern(*small),
        bias_small=rng.integers(-3, 4, size=cout).astype(np.float32), bias_big=rng.integers(-3, 4, size=cin).astype(np.float32),
        mask_small=tern(*small), mask_big=tern(*big),
        prefill=SimpleNamespace(small=tern(*small), big=tern(*big)), q=q)


def check_caps(v, storage, what=''):
    """The condition: |v| <= 256 for a bf16-stored tensor, |v| < 2**24 for an f32 one.  Asserted on oracle values only."""
    m = float(np.abs(v).max()) if np.size(v) else 0.0
    if storage == 'bf16':
        assert m <= BF16_CAP, '%s: |v| = %g exceeds the bf16 cap of %g (lower this case\'s q)' % (what, m, BF16_CAP)
    else:
        assert m < F32_CAP, '%s: |v| = %g reaches the f32 cap of 2**24 (lower this case\'s q)' % (what, m)
    return m


def stored(ref, dtype, what=''):
    """The oracle's float64 `ref` cast to the storage type (dtype 0: f32, 1: bf16), as float32.  The cap is asserted
    first; under it the cast loses nothing (checked: every expected value is exactly representable)."""
    check_caps(ref, 'bf16' if dtype == 1 else 'f32', what)
    t = torch.tensor(np.asarray(ref, dtype=np.float64))
    out = (t.to(torch.bfloat16) if dtype == 1 else t.to(torch.float32)).to(torch.float64).numpy()
    assert np.array_equal(out, ref), '%s: the oracle holds values its storage type cannot represent' % what
    return out.astype(np.float32)


class Oracle:
    """The three raw float64 answers of one case, each computed on first use and kept (the inputs never change)."""

    def __init__(self, case, seed=0, padding='SAME', q=None):
        self.case, self.padding = tuple(case), padding
        self.s = case[6]
        self.inp = exact_inputs(case, seed, padding, q)
        self._y = self._dx = self._dw = None

    @property
    def y(self):
        if self._y is None:
            self._y = T.conv2d(self.inp.x.astype(np.float64), self.inp.W.astype(np.float64), self.s, self.padding)
            self._y.setflags(write=False)
        return self._y

    @property
    def dx(self):
        if self._dx is None:
            self._dx = T.conv2d_backprop_input(self.inp.x.shape, self.inp.W.astype(np.float64), self.inp.dy.astype(np.float64),
                                               self.s, self.padding)
            self._dx.setflags(write=False)
        return self._dx

    @property
    def dw(self):
        if self._dw is None:
            self._dw = T.conv2d_backprop_filter(self.inp.x.astype(np.float64), self.inp.W.shape, self.inp.dy.astype(np.float64),
                                                self.s, self.padding)
            self._dw.setflags(write=False)
        return self._dw


_CACHE = {}
_CACHE_MAX = 6              # consecutive tests of one case (dtypes, forced variants) share its answers; the largest is ~70 MB


def oracle(case, seed=0, padding='SAME'):
    """Module-level cache: one Oracle per (case, seed, padding), the least recently made dropped past _CACHE_MAX."""
    key = (tuple(case), seed, padding)
    o = _CACHE.pop(key, None)
    if o is None:
        o = Oracle(case, seed, padding)
    _CACHE[key] = o
    while len(_CACHE) > _CACHE_MAX:
        _CACHE.pop(next(iter(_CACHE)))
    return o


def epilogue_ref(acc, bias=None, act='none', mask_mode='none', mask=None, prefill=None):
    """include/tdg.h: out = (act(acc + bias) + out) * mask, in float64 with the oracle's activations at leak 0.25.
    `prefill` is the previous `out` of an accumulating epilogue (None: not accumulating)."""
    v = acc if bias is None else T.bias_add(acc, bias.astype(np.float64))
    if act == 'relu':
        v = T.relu(v)
    elif act == 'lrelu':
        v = T.lrelu(v, LEAK)
    else:
        assert act == 'none'
    if prefill is not None:
        v = v + prefill.astype(np.float64)
    if mask_mode == 'lrelu':
        v = v * T.lrelu_grad_mask(mask.astype(np.float64), LEAK)
    elif mask_mode == 'relu':
        v = v * T.relu_grad_mask(mask.astype(np.float64))
    else:
        assert mask_mode == 'none'
    return v


def describe_mismatch(got, want, limit=6):
    """Count of wrong elements and the first few indices with got / want (readable from a log without another run)."""
    bad = np.argwhere(~(got == want))
    lines = ['%d of %d elements differ' % (len(bad), want.size)]
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        lines.append('  %s: got %r want %r' % (idx, float(got[idx]), float(want[idx])))
    return '\n'.join(lines)
