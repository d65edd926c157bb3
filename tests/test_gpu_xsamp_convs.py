"""The layer geometries experimental_sampler brings (hem/models/experimental_sampler.py:213-281), each through forward,
backward-data and backward-filter in f32 and bf16, BIT FOR BIT on the integer-valued inputs of tests/_exact_conv.py -- the
comparison, the caps and the epilogues are tests/test_gpu_conv_exact.py's three_forms, imported.  The 6- and 7-channel inputs
are not thin-kernel layers (plan_fwd_thin stops at 4 channels) and run on the implicit-GEMM kernels; the transposed layers are the
backward-data form of the conv between their output (big) and their input (small)."""
import pytest

import test_gpu_conv_exact as E

pytestmark = pytest.mark.gpu

# (n, h, w, cin, cout, k, stride), padding -- n = 3: odd, more than one image
CASES = [
    ((3, 64, 64, 7, 64, 5, 2), 'SAME'),        # e1: [X | noise]
    ((3, 64, 64, 6, 64, 5, 2), 'SAME'),        # hx1: X
    ((3, 32, 32, 1, 128, 5, 2), 'SAME'),       # hy1: the depth plane
    ((3, 4, 4, 512, 1024, 4, 2), 'VALID'),     # e5 / hx5 / hy4 forward, d1 as its backward-data form
    ((3, 8, 8, 256, 1024, 5, 2), 'SAME'),      # d2: 4x4x1024 -> 8x8x256 transposed, as the backward-data form
    ((3, 1, 1, 2048, 1024, 1, 1), 'SAME'),     # h1
    ((3, 1, 1, 128, 64, 1, 1), 'SAME'),        # h5
    ((3, 1, 1, 64, 1, 1, 1), 'SAME'),          # h6
]


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('case,padding', CASES)
def test_exact_experimental_sampler_geometries(case, padding, dtype):
    E.three_forms(case, dtype, padding)
