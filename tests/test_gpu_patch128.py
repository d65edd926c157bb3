"""The 128-row tile of igemm_fwd_patch_kernel in its three forms, BIT FOR BIT, on integer-valued inputs (tests/_exact_conv.py).

The default form keeps 12-piece patch buffers and a 4-stage filter ring whose loaders wait one step behind their issue;
TDG_PATCH128=1 is the 12-piece patch on the 3-stage ring, TDG_PATCH128=0 the 16-piece, 3-stage form both replaced, and a
launch whose chunk table leaves no room for the fourth stage (more than 174 K steps) must fall back to the 3-stage ring.
Every form multiplies the same fragments in the same order, so every comparison here is equality: with the float64
oracle, with the 192-row tile, with the replaced form, and between two launches.  The only conditions are the magnitude
caps of _exact_conv.check_caps, asserted on the oracle.

Shapes: 5x5 stride 2 at 16x16 -> 8x8 (two images per row tile, four parity groups) and 8x8 -> 4x4 (eight images per tile);
40 / 80 / 120 reduction channels = 16 / 32 / 47 K steps forward (the 4-stage ring wraps 4 - 11 times; 47 is no multiple of
four; from 80 channels on the three patch buffers are reused), 200 / 400 columns (one and two column tiles, the last
partly empty), one full row tile, three, and a ragged last one.  The backward-data launches gather with stride 1 in four
classes of 9 / 6 / 6 / 4 taps.
"""
import numpy as np
import pytest
import torch

from conftest import pkg
import _exact_conv as X

pytestmark = pytest.mark.gpu

NEW, MID, OLD, T192 = 'default', '12 pieces, 3 stages', '16 pieces, 3 stages', '192 rows'
ENVS = {
    NEW: {'TDG_PATCH_BM': '128'},
    MID: {'TDG_PATCH_BM': '128', 'TDG_PATCH128': '1'},
    OLD: {'TDG_PATCH_BM': '128', 'TDG_PATCH128': '0'},
    T192: {'TDG_PATCH_BM': '192'},
}
SYMBOL = {
    NEW: 'igemm_fwd_patch_kernel<bf16,128,208>',
    MID: 'igemm_fwd_patch_kernel<bf16,128,208,12,3>',
    OLD: 'igemm_fwd_patch_kernel<bf16,128,208,16,3>',
    T192: 'igemm_fwd_patch_kernel<bf16,192,208>',
}

# (h, images per 128-row tile): image counts = one full tile, three tiles, a last tile partly filled
GEOS = [(16, (2, 6, 5)), (8, (8, 24, 9))]
FWD_CASES = [(n, h, h, cin, cout, 5, 2) for h, ns in GEOS for n in ns for cin in (40, 80) for cout in (200, 400)]
FWD_CASES += [(5, 16, 16, 120, 400, 5, 2), (9, 8, 8, 120, 200, 5, 2)]                     # 47 K steps
# backward data: the GEMM's columns are the conv's input channels, its reduction runs over the output channels (80: 12 / 8 / 8 / 5
# K steps per class, 120: 17 / 12 / 12 / 8; a class needs >= 4 steps)
BWD_CASES = [(n, h, h, cin, cout, 5, 2) for h, ns in GEOS for n in ns for cin in (200, 400) for cout in (80,)]
BWD_CASES += [(5, 16, 16, 400, 120, 5, 2), (9, 8, 8, 200, 120, 5, 2)]
FALLBACK_CASE = (9, 8, 8, 480, 200, 5, 2)                                                # 188 K steps: 152 704 + 64 x 188 > 160 KB


def _kernel():
    return pkg('_lib').load().tdg_last_kernel().decode()


def _dev(a, dev):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _raw(act):
    """Every stored bit of an activation, padding channels included."""
    torch.cuda.synchronize()
    return act.buf.view(torch.int16).cpu().clone()


class Launches:
    """One conv and the launches of one direction under test; `run(form)` returns {what: (Act values, raw bits, extras)}."""

    def __init__(self, case, direction):
        K = self.K = pkg('kernels')
        self.case, self.direction = case, direction
        n, h, w, cin, cout, k, s = case
        dev = self.dev = torch.device('cuda:0')
        oh, ow, pt, pl = X.geometry(case)
        self.o = X.oracle(case)
        i = self.o.inp
        big, small = K.Act(n, h, w, cin, K.BF16, dev), K.Act(n, oh, ow, cout, K.BF16, dev)
        self.conv = K.Conv(big, small, k, k, s, pt, pl)
        self.conv.pack(_dev(i.W, dev))
        if direction == 'fwd':
            big.set(i.x)
            self.src, self.out, self.launch, self.acc = big, small, self.conv.fwd, self.o.y
            self.bias, self.mask, self.ncol = i.bias_small, i.mask_small, cout
        else:
            small.set(i.dy)
            self.src, self.out, self.launch, self.acc = small, big, self.conv.bwd_data, self.o.dx
            self.bias, self.mask, self.ncol = i.bias_big, i.mask_big, cin
        self.bias_d = _dev(self.bias, dev)
        self.msrc = self.out.like().set(self.mask)
        self.ws = K.Workspace(dev)

    def want(self, what):
        if what == 'bias+lrelu':
            return X.epilogue_ref(self.acc, self.bias, 'lrelu')
        return X.epilogue_ref(self.acc, mask_mode='lrelu', mask=self.mask)

    def epilogue(self, what, partials):
        K = self.K
        kw = (dict(bias=self.bias_d, act=K.ACT_LRELU, leak=X.LEAK) if what == 'bias+lrelu' else
              dict(mask_mode=K.MASK_LRELU, mask_src=self.msrc.ptr(), leak=X.LEAK))
        if partials:
            return K.colsum_epilogue(self.ws, self.out.rows, self.ncol, K.COL_SUM, images=0, **kw)
        return K.epilogue(**kw)

    def run(self, form, monkeypatch, symbol=None):
        monkeypatch.setenv('TDG_PATCH', '2')
        monkeypatch.setenv('TDG_KSPLIT', '1')
        monkeypatch.delenv('TDG_PATCH128', raising=False)
        for k, v in ENVS[form].items():
            monkeypatch.setenv(k, v)
        res = {}
        for what in ('bias+lrelu', 'lrelu mask'):
            for partials in (False, True):
                e = self.epilogue(what, partials)
                self.out.buf.fill_(7.0)
                self.launch(self.src.ptr(), self.out.ptr(), self.case[0], e)
                kern = _kernel()
                print('kernel: %s %s %s [%s] %s' % (self.direction, what, 'partials' if partials else 'plain', form, kern))
                assert kern == (symbol or SYMBOL[form]), (kern, form, self.case)
                part = None
                if partials:
                    nb = self.K.nblk(e)
                    print('nblk: %d' % nb)
                    if nb > 0:
                        torch.cuda.synchronize()
                        part = self.ws.buf[:nb * 2 * self.ncol * 4].view(torch.float32).reshape(nb, 2, self.ncol).cpu().numpy().astype(np.float64)
                res[(what, partials)] = (self.out.get(), _raw(self.out), part, kern)
        return res

    def check_oracle(self, res, form):
        for (what, partials), (got, raw, part, kern) in res.items():
            label = '%s %s%s [%s] of %s through %s' % (self.direction, what, ' + column partials' if partials else '', form, self.case, kern)
            ref = self.want(what)
            want = X.stored(ref, 1, label)
            if not np.array_equal(got, want):
                pytest.fail('%s: %s' % (label, X.describe_mismatch(got, want)), pytrace=False)
            full = raw.view(torch.bfloat16).float().reshape(self.out.n, self.out.h, self.out.w, self.out.cs)[..., self.out.c:]
            assert not full.any(), label + ': padding channels'
            if part is not None:                            # granted: the row tiles' column sums add up to the stored tensor's, exactly
                rows = ref.reshape(-1, self.ncol)
                X.check_caps(np.abs(rows).sum(0), 'f32', label + ' column sums')
                assert np.array_equal(part[:, 0].sum(0), rows.sum(0)), label + ': sum of the column partials'


def _same_bits(a, b, fa, fb, lp):
    for key in a:
        assert torch.equal(a[key][1], b[key][1]), '%s %s of %s: %s and %s differ in %d stored values' % (
            lp.direction, key, lp.case, fa, fb, int((a[key][1] != b[key][1]).sum()))
        if a[key][2] is not None and b[key][2] is not None and a[key][2].shape == b[key][2].shape:
            assert np.array_equal(a[key][2], b[key][2]), '%s %s of %s: column partials of %s and %s differ' % (lp.direction, key, lp.case, fa, fb)


def _all_forms(case, direction, monkeypatch):
    lp = Launches(case, direction)
    new = lp.run(NEW, monkeypatch)
    lp.check_oracle(new, NEW)
    again = lp.run(NEW, monkeypatch)
    _same_bits(new, again, NEW, 'its second launch', lp)
    for form in (OLD, MID):
        other = lp.run(form, monkeypatch)
        lp.check_oracle(other, form)
        _same_bits(new, other, NEW, form, lp)
    wide = lp.run(T192, monkeypatch)
    lp.check_oracle(wide, T192)
    for key in new:                                         # (the row tiles differ, so only the stored tensors are compared)
        assert torch.equal(new[key][1], wide[key][1]), '%s %s of %s: 128- and 192-row tiles differ' % (direction, key, case)
    granted = [k for k in new if k[1] and new[k][2] is not None]
    assert granted, 'no launch of %s granted column partials' % (case,)


@pytest.mark.parametrize('case', FWD_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_patch128_forward(case, monkeypatch):
    """Forward launches: bias + lrelu and the tangent pass's lrelu-derivative mask from a second tensor, with and without
    column partials, in every form: equal to the oracle, to each other, to the 192-row tile and to a second launch."""
    _all_forms(case, 'fwd', monkeypatch)


@pytest.mark.parametrize('case', BWD_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_patch128_backward_data(case, monkeypatch):
    """The four parity classes of the backward-data GEMM (9 / 6 / 6 / 4 taps, stride-1 gathers), same assertions."""
    _all_forms(case, 'bwd_data', monkeypatch)


def test_patch128_long_k_takes_three_stage_ring(monkeypatch):
    """188 K steps: the chunk table leaves no room for a fourth ring stage, so the default dispatch must launch the 12-piece,
    3-stage form (its symbol is asserted) -- never over the LDS limit -- and stay exact and equal to the replaced form."""
    lp = Launches(FALLBACK_CASE, 'fwd')
    new = lp.run(NEW, monkeypatch, symbol=SYMBOL[MID])
    lp.check_oracle(new, NEW)
    again = lp.run(NEW, monkeypatch, symbol=SYMBOL[MID])
    _same_bits(new, again, NEW, 'its second launch', lp)
    old = lp.run(OLD, monkeypatch)
    lp.check_oracle(old, OLD)
    _same_bits(new, old, NEW, OLD, lp)
