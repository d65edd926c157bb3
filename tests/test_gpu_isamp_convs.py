"""The layer geometries improved_sampler adds to those the other depth models already run (hem/models/improved_sampler.py:262-540,
:638-808), each through forward, backward-data and backward-filter in f32 and bf16, BIT FOR BIT on the integer-valued inputs of
tests/_exact_conv.py -- the comparison, the caps and the epilogues are tests/test_gpu_conv_exact.py's three_forms, imported."""
import pytest

import test_gpu_conv_exact as E

pytestmark = pytest.mark.gpu

# (n, h, w, cin, cout, k, stride), padding -- n = 3: odd, more than one image
CASES = [
    ((3, 31, 31, 1, 128, 5, 2), 'VALID'),      # critic A1 hy1: the 31x31 depth plane
    ((3, 64, 64, 5, 64, 5, 2), 'SAME'),        # critic D1 hx1: rgb, x_loc, y_loc
    ((3, 64, 64, 4, 64, 5, 2), 'SAME'),        # generator B2 e1: [rgb | noise]
    ((3, 64, 64, 3, 64, 5, 2), 'SAME'),        # critic B2 hx1: rgb
    ((3, 65, 65, 4, 64, 5, 2), 'VALID'),       # generators A1-A3 e1: [rgb | noise] at 65x65
    ((3, 31, 31, 128, 1, 1, 1), 'SAME'),       # the heads' 1x1 geometry at 31x31 as a conv
]


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('case,padding', CASES)
def test_exact_improved_sampler_geometries(case, padding, dtype):
    E.three_forms(case, dtype, padding)
