"""Every conv kernel variant against the float64 oracle, BIT FOR BIT, on integer-valued inputs (tests/_exact_conv.py).

No tolerance is defined here: every comparison is np.array_equal.  The only conditions are the two magnitude caps of
_exact_conv.check_caps (|v| <= 256 for bf16-stored values, |v| < 2**24 for f32 ones), asserted on the oracle.  The case
lists are those of tests/test_gpu_kernels.py, imported, so the two files cannot drift.  Each launch prints the kernel
symbol it dispatched to (`kernel: <form> <symbol>`; run with -s to collect them), and that symbol must be the one
tdg_conv2d_dispatch named when it was asked, just before the launch, with the same arguments.
"""
import itertools

import numpy as np
import pytest
import torch

from conftest import pkg
import _conv_dispatch as D
import _exact_conv as X
import test_gpu_kernels as G

pytestmark = pytest.mark.gpu

DMA_CASES = [(5, 16, 16, 200, 400, 5, 2), (9, 8, 8, 400, 200, 5, 2), (3, 9, 7, 16, 200, 4, 2)]            # test_conv_lds_dma_variant
PATCH_CASES = [(7, 16, 16, 200, 400, 5, 2), (25, 8, 8, 400, 800, 5, 2), (13, 8, 8, 200, 200, 5, 2), (6, 16, 16, 40, 200, 5, 2),
               (5, 8, 8, 200, 400, 3, 1), (4, 16, 16, 400, 200, 4, 2)]                                      # test_conv_patch_resident_kernel
KSPLIT_CASES = [(2, 8, 8, 200, 400, 5, 2), (2, 16, 16, 128, 256, 4, 2), (3, 4, 4, 512, 512, 4, 2)]          # test_conv_split_k_small_m
TWO_SOURCE_CASES = [(6, 16, 16, 200, 400, 5, 2, 4), (5, 8, 8, 40, 104, 5, 2, 2), (4, 32, 32, 3, 200, 5, 2, 3),
                    (6, 16, 16, 64, 256, 4, 2, 2)]                                                         # test_bwd_filter_two_sources
EPILOGUE_CASES = [(3, 16, 16, 8, 24, 5, 2), (3, 32, 32, 3, 200, 5, 2), (2, 16, 16, 200, 400, 5, 2), (2, 16, 16, 128, 256, 4, 2),
                  (3, 7, 9, 1, 24, 5, 2), (5, 15, 17, 24, 1, 3, 1)]                                         # one per kernel family
COL_FORCED_CASE = (5, 16, 16, 200, 400, 5, 2)


def _n(case, n):
    return (n,) + tuple(case[1:])


def all_exact_cases():
    """Every (case, padding) whose oracle this file compares with (tests/test_host_conv_exact.py holds each to the caps)."""
    out = [(tuple(c), 'SAME') for c in G.CONV_CASES] + [(tuple(c), 'VALID') for c in G.VALID_CASES]
    out += [(c, 'SAME') for c in DMA_CASES + PATCH_CASES + KSPLIT_CASES + EPILOGUE_CASES]
    out += [(tuple(c[:7]), 'SAME') for c in G.BLOCK_PATCH_CASES + TWO_SOURCE_CASES] + [(tuple(c), 'SAME') for c in G.WGRAD_PATCH_CASES]
    out += [(_n(c, 6), 'SAME') for c in EPILOGUE_CASES] + [(_n(c, 5), 'SAME') for c in EPILOGUE_CASES]
    seen, uniq = set(), []
    for item in out:
        if item not in seen:
            seen.add(item)
            uniq.append(item)
    return uniq


# ------------------------------------------------------------------------------------------------ helpers
def last_kernel():
    return pkg('_lib').load().tdg_last_kernel().decode()


_ASKED = []                 # what tdg_conv2d_dispatch answered just before the most recent launch of a conv from make()


def asking(conv):
    """Wrap the four launches of `conv`: each first asks the host-only query about the very call it is going to make."""
    fwd, bwd_data, bwd_filter, bwd_filter2 = conv.fwd, conv.bwd_data, conv.bwd_filter, conv.bwd_filter2

    def ask(n_images, form, epi=None, n_first=0):
        _ASKED[:] = [D.ask(conv.desc, n_images, form, epi, n_first)]

    def fwd_(x_ptr, y_ptr, n_images, epi=None):
        epi = conv._with_splitk(epi)
        ask(n_images, 'fwd', epi)
        fwd(x_ptr, y_ptr, n_images, epi)

    def bwd_data_(y_ptr, x_ptr, n_images, epi=None):
        epi = conv._with_splitk(epi)
        ask(n_images, 'bwd_data', epi)
        bwd_data(y_ptr, x_ptr, n_images, epi)

    def bwd_filter_(x_ptr, y_ptr, dw, n_images, beta=0.0):
        ask(n_images, 'bwd_filter')
        bwd_filter(x_ptr, y_ptr, dw, n_images, beta=beta)

    def bwd_filter2_(x_ptr, n_first, x2_ptr, y_ptr, dw, n_images, beta=0.0):
        ask(n_images, 'bwd_filter', n_first=n_first)
        bwd_filter2(x_ptr, n_first, x2_ptr, y_ptr, dw, n_images, beta=beta)
    conv.fwd, conv.bwd_data, conv.bwd_filter, conv.bwd_filter2 = fwd_, bwd_data_, bwd_filter_, bwd_filter2_
    return conv


def note(form, case):
    kern = last_kernel()
    print('kernel: %s %s %s' % (form, kern, case))
    assert _ASKED == [kern], '%s of %s: tdg_conv2d_dispatch named %r, the launch took %r' % (form, case, _ASKED, kern)
    _ASKED.clear()
    return kern


def assert_same(got, want, what, case, kern):
    """np.array_equal, with a message that locates the defect: count, first (image, row, col, channel) indices, kernel."""
    if got.shape == want.shape and np.array_equal(got, want):
        return
    pytest.fail('%s of %s through %s: %s' % (what, case, kern, X.describe_mismatch(got, want)), pytrace=False)


def assert_padding_zero(act, what, case, kern):
    if act.cs == act.c:
        return
    full = act.buf.float().reshape(act.n, act.h, act.w, act.cs)[..., act.c:].cpu().numpy()
    assert_same(full, np.zeros_like(full), what + ' padding channels [c:cs]', case, kern)


def make(K, case, dtype, padding='SAME'):
    n, h, w, cin, cout, k, s = case
    dev = torch.device('cuda:0')
    oh, ow, pt, pl = X.geometry(case, padding)
    big, small = K.Act(n, h, w, cin, dtype, dev), K.Act(n, oh, ow, cout, dtype, dev)
    return big, small, asking(K.Conv(big, small, k, k, s, pt, pl)), dev


def dev_f32(a, dev):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def consts(K):
    return ({'none': K.ACT_NONE, 'relu': K.ACT_RELU, 'lrelu': K.ACT_LRELU},
            {'none': K.MASK_NONE, 'lrelu': K.MASK_LRELU, 'relu': K.MASK_RELU})


def three_forms(case, dtype, padding='SAME', fwd_check=None):
    """fwd (bias + lrelu; VALID: bias + relu), bwd_data (lrelu mask from a tensor with zeros; VALID: bias) and bwd_filter
    (beta = 1 on a gradient pre-filled with 0.5) of one case, each equal to the oracle cast to the storage type, padding
    channels exactly 0 after each launch.  Returns the three dispatched kernel symbols."""
    K = pkg('kernels')
    o = X.oracle(case, 0, padding)
    i = o.inp
    n = case[0]
    big, small, conv, dev = make(K, case, dtype, padding)
    conv.pack(dev_f32(i.W, dev))
    ACT, MASK = consts(K)
    same = padding == 'SAME'
    # ---- forward
    big.set(i.x)
    act = 'lrelu' if same else 'relu'
    bias_small, bias_big = dev_f32(i.bias_small, dev), dev_f32(i.bias_big, dev)
    conv.fwd(big.ptr(), small.ptr(), n, K.epilogue(bias=bias_small, act=ACT[act], leak=X.LEAK))
    kf = note('fwd', case)
    if fwd_check is not None:
        fwd_check(kf)
    want = X.stored(X.epilogue_ref(o.y, i.bias_small, act), dtype, 'fwd')
    assert_same(small.get(), want, 'fwd', case, kf)
    assert_padding_zero(small, 'fwd', case, kf)
    # ---- backward data
    small.set(i.dy)
    out = big.like()
    if same:
        msrc = big.like().set(i.mask_big)
        conv.bwd_data(small.ptr(), out.ptr(), n, K.epilogue(mask_mode=K.MASK_LRELU, mask_src=msrc.ptr(), leak=X.LEAK))
        want = X.epilogue_ref(o.dx, mask_mode='lrelu', mask=i.mask_big)
    else:
        conv.bwd_data(small.ptr(), out.ptr(), n, K.epilogue(bias=bias_big))
        want = X.epilogue_ref(o.dx, i.bias_big)
    kb = note('bwd_data', case)
    assert_same(out.get(), X.stored(want, dtype, 'bwd_data'), 'bwd_data', case, kb)
    assert_padding_zero(out, 'bwd_data', case, kb)
    # ---- backward filter
    k, cin, cout = case[5], case[3], case[4]
    dw = torch.full((k, k, cin, cout), 0.5, device=dev)
    conv.bwd_filter(big.ptr(), small.ptr(), dw, n, beta=1.0)
    kw = note('bwd_filter', case)
    assert_same(dw.cpu().numpy(), X.stored(o.dw + 0.5, 0, 'bwd_filter'), 'bwd_filter', case, kw)
    return kf, kb, kw


def _product(cases, dtypes=(0, 1)):
    return [(tuple(c), d) for c in cases for d in dtypes]          # dtype fastest: both dtypes of a case share its oracle


# ------------------------------------------------------------------------------------------------ default dispatch
@pytest.mark.parametrize('case,dtype', _product(G.CONV_CASES))
def test_exact_same_padding(case, dtype):
    """Default dispatch on every SAME geometry: reaches the thin-input, one-output-channel, fused-class, col2im and
    per-class kernels by geometry."""
    three_forms(case, dtype)


@pytest.mark.parametrize('case,dtype', _product(G.VALID_CASES))
def test_exact_valid_padding(case, dtype):
    three_forms(case, dtype, 'VALID')


# ------------------------------------------------------------------------------------------------ forced variants
@pytest.mark.parametrize('mode,nw', [('4', None), ('3', None), ('0', None), ('3', '8')])
@pytest.mark.parametrize('case', DMA_CASES)
def test_exact_lds_dma_variant(case, mode, nw, monkeypatch):
    """The LDS-DMA tiles forced on small, ragged problems: 256-row tile, 192-row tile (wave-specialised, and with every
    wave loading and computing), and the register-staged kernel.  The forward launch's dispatch is asserted."""
    monkeypatch.setenv('TDG_DMA', mode)
    if nw is not None:
        monkeypatch.setenv('TDG_DMA_NW', nw)

    def check(kern):
        if mode == '0':
            assert 'igemm_fwd_kernel<bf16' in kern, kern
        else:
            assert 'igemm_fwd_dma_kernel<bf16,%s,208' % {'4': '256', '3': '192'}[mode] in kern, kern
            if mode == '3':
                assert kern.endswith(',8,1>') == (nw is None), kern     # the wave-specialised form unless every wave loads
    three_forms(case, 1, fwd_check=check)


@pytest.mark.parametrize('bm', [None, '128'])
@pytest.mark.parametrize('case', PATCH_CASES)
def test_exact_patch_resident_kernel(case, bm, monkeypatch):
    """igemm_fwd_patch_kernel forced onto small problems (ragged last row tile, every parity class of the backward-data
    GEMM, stride 1, 4x4 filters, one and many K slices), in its 192- and 128-row tiles; the dispatch is asserted."""
    monkeypatch.setenv('TDG_PATCH', '2')
    if bm is not None:
        monkeypatch.setenv('TDG_PATCH_BM', bm)

    def check(kern):
        assert 'igemm_fwd_patch_kernel' in kern, kern
    three_forms(case, 1, fwd_check=check)


@pytest.mark.parametrize('case', G.BLOCK_PATCH_CASES)
def test_exact_block_patch_kernel(case, monkeypatch):
    """igemm_fwd_bp_kernel / igemm_fwd_patch_kernel<256, ...> on 16 x 16 blocks or four whole images; the None case must
    fall back to a slab kernel."""
    monkeypatch.setenv('TDG_PATCH', '2')
    monkeypatch.setenv('TDG_BLOCKPATCH', '1')
    want = case[7]

    def check(kern):
        if want is None:
            assert 'igemm_fwd_patch_kernel' not in kern and 'igemm_fwd_bp_kernel' not in kern, kern
        else:
            assert want in kern, kern
    three_forms(tuple(case[:7]), 1, fwd_check=check)


@pytest.mark.parametrize('nw', ['8', '4'])
@pytest.mark.parametrize('case', G.WGRAD_PATCH_CASES)
def test_exact_wgrad_patch_kernel(case, nw, monkeypatch):
    """igemm_wgrad_patch_kernel in both wave layouts, then the slab kernel (TDG_WPATCH=0): each equals the oracle, so the
    two are EQUAL to each other (beta = 1 on a gradient pre-filled with 0.5); both dispatches asserted."""
    K = pkg('kernels')
    monkeypatch.setenv('TDG_WPATCH_NW', nw)
    n, h, w, cin, cout, k, s = case
    o = X.oracle(case)
    big, small, conv, dev = make(K, case, 1)
    big.set(o.inp.x)
    small.set(o.inp.dy)
    want = X.stored(o.dw + 0.5, 0, 'bwd_filter')
    dw = torch.full((k, k, cin, cout), 0.5, device=dev)
    conv.bwd_filter(big.ptr(), small.ptr(), dw, n, beta=1.0)
    kern = note('bwd_filter', case)
    assert 'igemm_wgrad_patch_kernel<bf16,256,208,%s' % nw in kern, kern
    patch = dw.cpu().numpy()
    assert_same(patch, want, 'bwd_filter', case, kern)
    monkeypatch.setenv('TDG_WPATCH', '0')
    dw = torch.full((k, k, cin, cout), 0.5, device=dev)
    conv.bwd_filter(big.ptr(), small.ptr(), dw, n, beta=1.0)
    kern = note('bwd_filter', case)
    assert 'igemm_wgrad_dma_kernel' in kern, kern
    assert_same(dw.cpu().numpy(), patch, 'slab against patch bwd_filter', case, kern)


@pytest.mark.parametrize('ks', [None, '3', '7', '1'])
@pytest.mark.parametrize('case,dtype', _product(KSPLIT_CASES))
def test_exact_split_k_small_m(case, dtype, ks, monkeypatch):
    """Small-M forward-type GEMMs cut along K into f32 partial tiles plus a finishing kernel: default split count, forced
    ragged counts, and never.  The partials are f32, so every split count gives the same integers."""
    if ks is None:
        monkeypatch.delenv('TDG_KSPLIT', raising=False)
    else:
        monkeypatch.setenv('TDG_KSPLIT', ks)
    three_forms(case, dtype)


@pytest.mark.parametrize('case,dtype', _product(TWO_SOURCE_CASES))
def test_exact_bwd_filter_two_sources(case, dtype):
    """tdg_conv2d_bwd_filter2 with beta = 0.5 on an integer dw0 (halves are exact); rows of the first tensor past n_first
    hold 9 and must not be read."""
    K = pkg('kernels')
    n, h, w, cin, cout, k, s, n_first = case
    c7 = tuple(case[:7])
    o = X.oracle(c7)
    x = o.inp.x
    big, small, conv, dev = make(K, c7, dtype)
    dw0 = np.random.default_rng(7).integers(-3, 4, size=(k, k, cin, cout)).astype(np.float32)
    first, second = big.like().set(np.concatenate([x[:n_first], 9.0 * np.ones_like(x[n_first:])])), big.like()
    second.set(np.concatenate([x[n_first:], np.zeros_like(x[:n_first])]))
    small.set(o.inp.dy)
    dw = dev_f32(dw0, dev)
    conv.bwd_filter2(first.ptr(), n_first, second.ptr(), small.ptr(), dw, n, beta=0.5)
    kern = note('bwd_filter2', c7)
    assert_same(dw.cpu().numpy(), X.stored(0.5 * dw0.astype(np.float64) + o.dw, 0, 'bwd_filter2'), 'bwd_filter2', case, kern)


# ------------------------------------------------------------------------------------------------ epilogue matrix
def _form_setup(K, case, dtype, form):
    """(conv, src Act, out Act, launch, raw oracle answer, bias, mask, prefill) of a forward or backward-data launch."""
    o = X.oracle(case)
    i = o.inp
    big, small, conv, dev = make(K, case, dtype)
    conv.pack(dev_f32(i.W, dev))
    if form == 'fwd':
        big.set(i.x)
        return conv, big, small, conv.fwd, o.y, i.bias_small, i.mask_small, i.prefill.small, dev
    small.set(i.dy)
    return conv, small, big, conv.bwd_data, o.dx, i.bias_big, i.mask_big, i.prefill.big, dev


EPI_COMBOS = [(True, a, m, acc) for a, m, acc in itertools.product(('none', 'relu', 'lrelu'), ('none', 'lrelu', 'relu'), (False, True))]
EPI_COMBOS += [(False, 'none', 'none', False), (False, 'none', 'none', True)]


@pytest.mark.parametrize('form', ['fwd', 'bwd_data'])
@pytest.mark.parametrize('case,dtype', _product(EPILOGUE_CASES))
def test_exact_epilogue_matrix(case, dtype, form):
    """bias x {none, relu, lrelu} x {no mask, lrelu mask, relu mask} (the mask source holds zeros) x accumulate 0 / 1 on an
    output pre-filled with `prefill`: out = (act(acc + bias) + out) * mask, as include/tdg.h states it."""
    K = pkg('kernels')
    ACT, MASK = consts(K)
    conv, src, out, launch, acc, bias, mask, prefill, dev = _form_setup(K, case, dtype, form)
    bias_d = dev_f32(bias, dev)
    msrc = out.like().set(mask)
    for with_bias, act, mm, accumulate in EPI_COMBOS:
        out.set(prefill)
        launch(src.ptr(), out.ptr(), case[0],
               K.epilogue(bias=bias_d if with_bias else None, act=ACT[act], leak=X.LEAK, mask_mode=MASK[mm],
                          mask_src=msrc.ptr() if mm != 'none' else None, accumulate=accumulate))
        what = '%s bias=%d act=%s mask=%s accumulate=%d' % (form, with_bias, act, mm, accumulate)
        kern = note(what, case)
        want = X.epilogue_ref(acc, bias if with_bias else None, act, mm, mask, prefill if accumulate else None)
        assert_same(out.get(), X.stored(want, dtype, what), what, case, kern)
        assert_padding_zero(out, what, case, kern)


THIN_ACCUMULATE_CASES = [((3, 32, 32, 3, 200, 5, 2), 'thin_fwd_kernel<bf16>'),          # 208-column tiles
                         ((66, 64, 64, 3, 64, 5, 2), 'thin_fwd_kernel<bf16,64>')]       # 64-column tiles


@pytest.mark.parametrize('case,symbol', THIN_ACCUMULATE_CASES)
def test_exact_thin_forward_accumulates(case, symbol):
    """A thin-input layer's filter exists in thin_fwd_kernel's layout only, so an accumulating forward launch must stay on
    that kernel: it once went to igemm_fwd_dma_kernel, which read the packed filter in the implicit-GEMM layout (found by
    test_exact_epilogue_matrix on (3,32,32,3,200,5,2): 136029 of 153600 elements wrong).  Dispatch asserted."""
    K = pkg('kernels')
    conv, src, out, launch, acc, bias, mask, prefill, dev = _form_setup(K, case, 1, 'fwd')
    bias_d = dev_f32(bias, dev)
    msrc = out.like().set(mask)
    for mm, mode in (('none', K.MASK_NONE), ('lrelu', K.MASK_LRELU)):
        out.set(prefill)
        launch(src.ptr(), out.ptr(), case[0], K.epilogue(bias=bias_d, act=K.ACT_LRELU, leak=X.LEAK, mask_mode=mode,
                                                         mask_src=msrc.ptr() if mm != 'none' else None, accumulate=True))
        what = 'fwd bias=1 act=lrelu mask=%s accumulate=1' % mm
        kern = note(what, case)
        assert kern == symbol, kern
        want = X.epilogue_ref(acc, bias, 'lrelu', mm, mask, prefill)
        assert_same(out.get(), X.stored(want, 1, what), what, case, kern)
        assert_padding_zero(out, what, case, kern)


SENTINEL = 7.0


@pytest.mark.parametrize('form', ['fwd', 'bwd_data'])
@pytest.mark.parametrize('case,dtype', _product(EPILOGUE_CASES))
def test_exact_subbatch_window(case, dtype, form):
    """3 of 6 images through a pointer offset (ptr(2)): the window equals the oracle of those images; the images outside
    hold a non-zero sentinel and must come back unchanged ("untouched", which a zero fill cannot tell from "zeroed")."""
    K = pkg('kernels')
    case = _n(case, 6)
    conv, src, out, launch, acc, bias, mask, prefill, dev = _form_setup(K, case, dtype, form)
    out.set(np.full((out.n, out.h, out.w, out.c), SENTINEL, np.float32))
    bias_d = dev_f32(bias, dev)
    launch(src.ptr(2), out.ptr(2), 3, K.epilogue(bias=bias_d, act=K.ACT_LRELU, leak=X.LEAK))
    kern = note(form + ' sub-batch', case)
    want = X.stored(X.epilogue_ref(acc, bias, 'lrelu'), dtype, form).copy()
    want[:2] = SENTINEL
    want[5:] = SENTINEL
    assert_same(out.get(), want, form + ' sub-batch 2..4 of 6', case, kern)
    assert_padding_zero(out, form + ' sub-batch', case, kern)


# ------------------------------------------------------------------------------------------------ column partials
COL_EPILOGUES = [
    # col_mode, bias, act, mask
    ('sum', True, 'lrelu', 'none'),      # the bias gradient of a layer's output
    ('sum', False, 'none', 'lrelu'),     # ... of a masked tangent / gradient tensor (the sums are of what is stored)
    ('bn', True, 'none', 'none'),        # batch statistics of the stored pre-activation, as deviations from the bias
]
PARTIAL_KERNELS = ('igemm_fwd_dma_kernel<bf16', 'igemm_fwd_patch_kernel', 'igemm_fwd_bp_kernel')


def column_partials(case, col_images, expect_partials):
    """Forward launches of one bf16 case with column partials asked for.  Where the launch grants them (nblk > 0) the sum
    over its row tiles equals the column sums of the stored tensor (the oracle's, images below col_images) exactly, and
    tdg_col_finalize_sum with beta = 1 on a pre-filled vector gives the same integers.  The tile layout is not asserted.
    nblk == 0 is accepted only from a kernel include/tdg.h excuses; `expect_partials`: it must NOT be 0 from the LDS-DMA
    and patch kernels.  Returns [(kernel, nblk)]."""
    K = pkg('kernels')
    ACT, MASK = consts(K)
    n, cout = case[0], case[4]
    conv, src, out, launch, acc, bias, mask, prefill, dev = _form_setup(K, case, 1, 'fwd')
    ws = K.Workspace(dev)
    bias_d = dev_f32(bias, dev)
    msrc = out.like().set(mask)
    seen = []
    for mode, with_bias, act, mm in COL_EPILOGUES:
        e = K.colsum_epilogue(ws, out.rows, cout, K.COL_SUM if mode == 'sum' else K.COL_BN, images=col_images,
                              bias=bias_d if with_bias else None, act=ACT[act], leak=X.LEAK, mask_mode=MASK[mm],
                              mask_src=msrc.ptr() if mm != 'none' else None)
        out.set(np.zeros((out.n, out.h, out.w, out.c), np.float32))
        launch(src.ptr(), out.ptr(), n, e)
        what = 'fwd col=%s images=%d bias=%d act=%s mask=%s' % (mode, col_images, with_bias, act, mm)
        kern = note(what, case)
        nb = K.nblk(e)
        print('nblk: %d %s %s %s' % (nb, kern, what, case))
        seen.append((kern, nb))
        ref = X.epilogue_ref(acc, bias if with_bias else None, act, mm, mask)
        assert_same(out.get(), X.stored(ref, 1, what), what, case, kern)
        assert_padding_zero(out, what, case, kern)
        grants = any(p in kern for p in PARTIAL_KERNELS)
        if nb == 0:
            # include/tdg.h: f32 tiles, accumulating epilogues, thin layers, split-K launches -- never the kernels the models rely on
            assert not (expect_partials and grants), 'no column partials from %s (%s of %s)' % (kern, what, case)
            continue
        rows = ref[:col_images] if col_images else ref
        dev_rows = rows.reshape(-1, cout) - (bias.astype(np.float64) if mode == 'bn' else 0.0)
        want0, want1 = dev_rows.sum(0), (dev_rows ** 2).sum(0)
        X.check_caps(np.abs(dev_rows).sum(0), 'f32', what + ' column sums')
        X.check_caps(want1, 'f32', what + ' second moments')
        torch.cuda.synchronize()
        part = ws.buf[:nb * 2 * cout * 4].view(torch.float32).reshape(nb, 2, cout).cpu().numpy().astype(np.float64)
        assert_same(part[:, 0].sum(0), want0, what + ': sum of the row tiles\' column sums', case, kern)
        if mode == 'bn':
            assert_same(part[:, 1].sum(0), want1, what + ': sum of the row tiles\' second moments', case, kern)
        db = torch.full((cout,), 2.0, device=dev)
        K.bias_grad_from_partials(e, cout, db, beta=1.0)
        assert_same(db.cpu().numpy().astype(np.float64), want0 + 2.0, what + ': tdg_col_finalize_sum, beta = 1 on 2', case, kern)
    return seen


@pytest.mark.parametrize('ksplit', [None, '1'])
@pytest.mark.parametrize('case', EPILOGUE_CASES)
def test_exact_column_partials_default_dispatch(case, ksplit, monkeypatch):
    """The epilogue-matrix geometries: all images at the stated batch, and 3 of 5 images.  Under the default split-K policy
    the small-M launches are cut along K and report nblk == 0 (the partial tiles are not the stored tile); with TDG_KSPLIT=1
    (never split) an LDS-DMA or patch launch must grant the partials."""
    if ksplit is None:
        monkeypatch.delenv('TDG_KSPLIT', raising=False)
    else:
        monkeypatch.setenv('TDG_KSPLIT', ksplit)
    column_partials(case, 0, expect_partials=ksplit == '1')
    column_partials(_n(case, 5), 3, expect_partials=ksplit == '1')


@pytest.mark.parametrize('env', [{'TDG_DMA': '4'}, {'TDG_DMA': '3'}, {'TDG_DMA': '3', 'TDG_DMA_NW': '8'}, {'TDG_DMA': '0'},
                                 {'TDG_PATCH': '2'}, {'TDG_PATCH': '2', 'TDG_PATCH_BM': '128'}],
                         ids=lambda e: '-'.join('%s=%s' % kv for kv in sorted(e.items())))
@pytest.mark.parametrize('col_images', [0, 3])
def test_exact_column_partials_forced_variants(env, col_images, monkeypatch):
    """The forced LDS-DMA tiles and the patch-resident kernel on (5,16,16,200,400,5,2), never split along K: these are the
    launches the models take their bias gradients and batch statistics from, so nblk must not be 0 (TDG_DMA=0, the
    register-staged kernel, provides none)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('TDG_KSPLIT', '1')
    seen = column_partials(COL_FORCED_CASE, col_images, expect_partials=True)
    for kern, nb in seen:
        if env.get('TDG_DMA') == '0':
            assert 'igemm_fwd_kernel<bf16' in kern and nb == 0, (kern, nb)
        elif 'TDG_PATCH' in env:
            assert 'igemm_fwd_patch_kernel' in kern and nb > 0, (kern, nb)
        else:
            assert 'igemm_fwd_dma_kernel<bf16' in kern and nb > 0, (kern, nb)
