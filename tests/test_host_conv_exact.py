"""The integer-valued conv recipe of tests/_exact_conv.py, checked on the CPU with oracle arithmetic only:
the magnitude caps hold for every case tests/test_gpu_conv_exact.py compares, the data is sensitive to the defects the
GPU test is meant to catch, and the gap of the relative-error bound it closes is kept as a record."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tf_ops as T
import _exact_conv as X
import test_gpu_conv_exact as E
import test_gpu_kernels as G


def _torch_answers(case, padding, inp):
    """The three raw answers in float64 through torch's CPU convolutions (numpy's tap loop is slow on the large cases);
    _exact_conv.Oracle -- what the GPU test compares with -- is tf_ops, and test_torch_route_equals_the_oracle ties the two."""
    n, h, w, cin, cout, k, s = case
    oh, ow, pt, pl = X.geometry(case, padding)
    pb, pr = max((oh - 1) * s + k - h - pt, 0), max((ow - 1) * s + k - w - pl, 0)
    x = torch.from_numpy(inp.x.astype(np.float64)).permute(0, 3, 1, 2)
    xp = F.pad(x, (pl, pr, pt, pb)).requires_grad_(True)
    Wt = torch.from_numpy(inp.W.astype(np.float64)).permute(3, 2, 0, 1).contiguous().requires_grad_(True)
    y = F.conv2d(xp, Wt, stride=s)[:, :, :oh, :ow]
    dy = torch.from_numpy(inp.dy.astype(np.float64)).permute(0, 3, 1, 2)
    dxp, dW = torch.autograd.grad(y, (xp, Wt), dy)
    return (y.detach().permute(0, 2, 3, 1).numpy(), dxp[:, :, pt:pt + h, pl:pl + w].permute(0, 2, 3, 1).numpy(),
            dW.permute(2, 3, 1, 0).numpy())


@pytest.mark.parametrize('case,padding', [((3, 7, 9, 3, 24, 5, 2), 'SAME'), ((2, 9, 11, 2, 16, 4, 2), 'SAME'),
                                          ((2, 12, 20, 2, 232, 3, 1), 'SAME'), ((2, 10, 7, 16, 40, 4, 2), 'VALID'),
                                          ((2, 9, 12, 8, 24, 3, 1), 'VALID')])
def test_torch_route_equals_the_oracle(case, padding):
    o = X.Oracle(case, 0, padding)
    y, dx, dw = _torch_answers(case, padding, o.inp)
    assert np.array_equal(y, o.y) and np.array_equal(dx, o.dx) and np.array_equal(dw, o.dw)


@pytest.mark.parametrize('case,padding', E.all_exact_cases())
def test_caps_hold_for_every_gpu_case(case, padding):
    """The condition of the exact comparison, on everything a launch of the GPU file stores: the forward and backward-data
    answers through every epilogue of the matrix (bias in [-3, 3], a prefill in {-1, 0, 1}) stay within 256, the filter
    gradient (+ 0.5, and + half an integer in [-3, 3]) and the column sums / second moments stay below 2**24."""
    inp = X.exact_inputs(case, 0, padding)
    y, dx, dw = _torch_answers(case, padding, inp)
    for acc, bias, what in ((y, inp.bias_small, 'fwd'), (dx, inp.bias_big, 'bwd_data')):
        assert np.array_equal(acc, np.rint(acc))
        X.check_caps(np.abs(acc + bias) + 1.0, 'bf16', what)             # |act(v)| <= |v|, |mask| <= 1, one prefill of magnitude 1
    X.check_caps(np.abs(dw) + 0.5 + 1.5, 'f32', 'bwd_filter')
    dev = y.reshape(-1, y.shape[-1])
    X.check_caps(np.abs(dev + inp.bias_small).sum(0), 'f32', 'column sums')
    X.check_caps((dev ** 2).sum(0), 'f32', 'second moments')
    # every reduction is a sum of products in {-1, 0, 1}: no partial sum, in any order, can pass the number of terms
    n, h, w, cin, cout, k, s = case
    assert max(k * k * cin, k * k * cout, n * y.shape[1] * y.shape[2]) < X.F32_CAP


SMALLEST = [
    ((2, 32, 32, 3, 16, 5, 2), 'SAME'),       # thin input
    ((3, 16, 16, 8, 24, 5, 2), 'SAME'),       # vector gather
    ((2, 16, 16, 4, 64, 4, 2), 'SAME'),       # 4x4 stride 2
    ((2, 12, 20, 2, 232, 3, 1), 'SAME'),      # stride 1
    ((2, 9, 12, 8, 24, 3, 1), 'VALID'),       # VALID
]


def _answers(case, padding, x, W, dy):
    s = case[6]
    x, W, dy = x.astype(np.float64), W.astype(np.float64), dy.astype(np.float64)
    return (T.conv2d(x, W, s, padding), T.conv2d_backprop_input(x.shape, W, dy, s, padding),
            T.conv2d_backprop_filter(x, W.shape, dy, s, padding))


@pytest.mark.parametrize('case,padding', SMALLEST)
def test_recipe_is_sensitive_to_kernel_defects(case, padding):
    """The recipe is not degenerate for what the GPU test must catch.  Zeroing any single filter tap changes the forward
    output, and changes the backward-data output -- in exactly the output-parity class that tap feeds, and over all taps
    every parity class is changed; the filter gradient does not depend on the filter, so there the tap's own gradient
    must be non-zero (a kernel that drops the tap is seen).  Zeroing the first or last row or column of the input
    (of dy, for backward-data) changes all three answers, and so does swapping two images."""
    n, h, w, cin, cout, k, s = case
    _, _, pt, pl = X.geometry(case, padding)
    i = X.exact_inputs(case, 0, padding)
    y, dx, dw = _answers(case, padding, i.x, i.W, i.dy)
    classes = set()
    for a in range(k):
        for b in range(k):
            assert np.any(dw[a, b] != 0), 'the filter gradient of tap (%d, %d) is all zero' % (a, b)
            W2 = i.W.copy()
            W2[a, b] = 0
            y2, dx2, _ = _answers(case, padding, i.x, W2, i.dy)
            assert np.any(y2 != y), 'tap (%d, %d) does not show in the forward output' % (a, b)
            rows, cols = np.nonzero((dx2 != dx).any(axis=(0, 3)))
            assert rows.size, 'tap (%d, %d) does not show in the backward-data output' % (a, b)
            assert np.all((rows + pt) % s == a % s) and np.all((cols + pl) % s == b % s)
            classes.add((int(rows[0] % s), int(cols[0] % s)))
    assert len(classes) == s * s
    # first / last row and column: of x for the forward output and the filter gradient, of dy for backward-data.  A VALID
    # window may never read the last rows / columns of x (the remainder): the last one a window covers is taken instead
    for axis in (1, 2):
        last_read = (i.dy.shape[axis] - 1) * s + k - 1 if padding == 'VALID' else i.x.shape[axis] - 1
        for ix, idy in ((0, 0), (last_read, i.dy.shape[axis] - 1)):
            x2, dy2 = i.x.copy(), i.dy.copy()
            x2[(slice(None),) * axis + (ix,)] = 0
            dy2[(slice(None),) * axis + (idy,)] = 0
            y2, _, dw2 = _answers(case, padding, x2, i.W, i.dy)
            _, dx2, dw3 = _answers(case, padding, i.x, i.W, dy2)
            assert np.any(y2 != y) and np.any(dw2 != dw), (axis, ix)
            assert np.any(dx2 != dx) and np.any(dw3 != dw), (axis, idy)
    swap = np.arange(n)
    swap[[0, 1]] = [1, 0]
    y2, _, dw2 = _answers(case, padding, i.x[swap], i.W, i.dy)
    _, dx2, _ = _answers(case, padding, i.x, i.W, i.dy[swap])
    assert np.any(y2 != y) and np.any(dx2 != dx) and np.any(dw2 != dw)


def test_the_gap_of_the_relative_error_bound():
    """A record of what the exact test closes.  Under the existing recipe (normal inputs rounded to bf16, filter scaled by
    1 / sqrt(k k cin), N(0, 1) bias, lrelu 0.2) on (2,8,8,200,400,5,2), one channel of one filter tap removed at every
    output pixel stays below the bf16 bound of tests/test_gpu_kernels.py in its own metric: that defect passes.  Under the
    integer recipe the same removal is a non-zero difference, which np.array_equal cannot miss."""
    case = (2, 8, 8, 200, 400, 5, 2)
    n, h, w, cin, cout, k, s = case
    rng = np.random.default_rng(1)
    x = G.bf16_round(rng.standard_normal((n, h, w, cin)).astype(np.float32)).astype(np.float64)
    Wt = G.bf16_round((rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)).astype(np.float64)
    b = rng.standard_normal(cout).astype(np.float32)
    ref = T.lrelu(T.conv2d(x, Wt, s) + b)
    broken = Wt.copy()
    broken[2, 2, 0, :] = 0
    err = G.relerr(T.lrelu(T.conv2d(x, broken, s) + b), ref)
    print('existing recipe, one channel of one tap removed: relerr = %.4f (bound %.0e)' % (err, G.TOL[1]))
    assert 0 < err < G.TOL[1]
    i = X.exact_inputs(case)
    broken = i.W.copy()
    broken[2, 2, 0, :] = 0
    assert np.any(broken != i.W)
    want = X.epilogue_ref(T.conv2d(i.x.astype(np.float64), i.W.astype(np.float64), s), i.bias_small, 'lrelu')
    got = X.epilogue_ref(T.conv2d(i.x.astype(np.float64), broken.astype(np.float64), s), i.bias_small, 'lrelu')
    assert np.count_nonzero(got != want) > 0 and not np.array_equal(X.stored(got, 1), X.stored(want, 1))
