"""tdg_mde_loss (3dgan_amd/csrc/tdg_mde.hip) against float64 NumPy (tests/_mde_ref.mde_loss_ref) on the same stored inputs.

The bounds follow from the arithmetic.  y lies on the grid k/256, so every f64 sum of an image is exact in any order and
mean_out must be float32(float64 mean) bit for bit.  The loss is a f64 sum of n f64 terms divided once: it agrees with the
oracle's f64 value to some 1e-15 relative, so its f32 rounding is within ONE f32 spacing of the oracle's rounded value.  A seed
is sign(m_i - mean_i) * float32(1/n) rounded to the dtype, exactly, and 0 where m_i == mean_i."""
import numpy as np
import pytest
import torch

from conftest import pkg
from test_gpu_paper_cgan import dev, DEV
import _mde_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 77.0
TDG_EINVAL, TDG_EWORKSPACE = -1, -4
SHAPES = [(1, 1), (3, 7), (5, 64), (2, 257), (4, 3710), (512, 3710)]       # one element, < a wave, a wave, a block + 1, the frame, the batch


def L():
    return pkg('_lib')


def K():
    return pkg('kernels')


def inputs(n, hw, dt, seed=0):
    """y [n,hw] on the grid k/256, m [n] as stored in the dtype; for n >= 2 the last image is constant 0.5 with m = 0.5."""
    rng = np.random.default_rng([seed, n, hw])
    level = rng.integers(20, 236, (n, 1))
    y = ((level + rng.integers(-19, 20, (n, hw))) / 256.0).astype(np.float32)
    m = torch.tensor(rng.uniform(0.05, 0.95, n).astype(np.float32))
    if n >= 2:
        y[-1], m[-1] = 0.5, 0.5
    if dt:
        m = m.bfloat16()
    return y, m


def launch(y, m, dt, cs=1, y_offset=0, ws_bytes=None, n=None, hw=None):
    n0, hw0 = y.shape
    n, hw = n0 if n is None else n, hw0 if hw is None else hw
    lib = L().load()
    need = lib.tdg_mde_loss_workspace_bytes(n0)
    ws = torch.zeros(max(need, 8), dtype=torch.uint8, device=DEV)
    tdt = torch.bfloat16 if dt else torch.float32
    md = torch.full((n0 * cs,), SENTINEL, dtype=tdt, device=DEV)
    md[::cs] = m.to(DEV)
    seed = torch.full((n0 * cs,), SENTINEL, dtype=tdt, device=DEV)
    mean = torch.full((n0 + 1,), SENTINEL, device=DEV)
    scal = torch.full((2,), SENTINEL, device=DEV)
    yd = dev(np.concatenate([np.zeros(y_offset, np.float32), y.ravel()]))
    rc = lib.tdg_mde_loss(dt, K().ptr(yd, 4 * y_offset), n, hw, K().ptr(md), cs, K().ptr(mean), K().ptr(seed), cs, K().ptr(scal),
                          K().ptr(ws), need if ws_bytes is None else ws_bytes, K().stream())
    torch.cuda.synchronize()
    return rc, mean.cpu().numpy(), seed.float().cpu().numpy().reshape(n0, cs), scal.cpu().numpy()


def check(y, m, dt, cs, y_offset=0):
    n, hw = y.shape
    rc, mean, seed, scal = launch(y, m, dt, cs, y_offset)
    assert rc == 0
    want_mean, want_loss, sign = R.mde_loss_ref(y, m.float().numpy())
    assert np.array_equal(mean[:n], want_mean) and mean[n] == SENTINEL
    err = abs(float(scal[0]) - float(want_loss))
    print('n %d hw %d dt %d cs %d: loss %.9g (oracle %.9g, %.2f spacings)' % (n, hw, dt, cs, scal[0], want_loss,
                                                                             err / np.spacing(want_loss) if want_loss else err))
    assert err <= np.spacing(want_loss) and scal[1] == SENTINEL
    step = torch.tensor(np.float32(1.0 / n))
    step = float(step.bfloat16().float() if dt else step)
    assert np.array_equal(seed[:, 0], (sign * step).astype(np.float32))
    if n >= 2:
        assert sign[-1] == 0 and seed[-1, 0] == 0 and np.all(seed[:-1, 0] != 0)
    if cs > 1:
        assert np.all(seed[:, 1:] == SENTINEL)
    return mean, seed, scal


@pytest.mark.parametrize('cs', [1, 8])
@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('n,hw', SHAPES)
def test_mde_loss_against_float64(n, hw, dt, cs):
    check(*inputs(n, hw, dt), dt, cs)


@pytest.mark.parametrize('n,hw,y_offset', [(5, 64, 1), (5, 64, 2), (4, 3710, 1)])
def test_rows_that_do_not_start_on_a_vector_boundary(n, hw, y_offset):
    """hw = 64 from a 16-byte boundary takes four floats per load, 3710 two; one or two floats further on the narrower
    loads must give the same bits."""
    y, m = inputs(n, hw, 0)
    a = check(y, m, 0, 1)
    b = check(y, m, 0, 1, y_offset)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('dt', [0, 1])
def test_two_launches_are_bit_equal(dt):
    rng = np.random.default_rng(5)
    y = rng.uniform(0.01, 0.99, (37, 3710)).astype(np.float32)               # off the grid: the order of the sums matters
    m = torch.tensor(rng.uniform(0.05, 0.95, 37).astype(np.float32))
    m = m.bfloat16() if dt else m
    a, b = launch(y, m, dt, 8), launch(y, m, dt, 8)
    assert a[0] == b[0] == 0 and all(p.tobytes() == q.tobytes() for p, q in zip(a[1:], b[1:]))
    want_mean, want_loss, sign = R.mde_loss_ref(y, m.float().numpy())
    assert np.all(np.abs(a[1][:37] - want_mean) <= np.spacing(want_mean)) and abs(a[3][0] - want_loss) <= np.spacing(want_loss)


def test_bad_arguments_return_the_error_status():
    y, m = inputs(3, 7, 0)
    assert launch(y, m, 0, n=0)[0] == TDG_EINVAL
    assert launch(y, m, 0, hw=0)[0] == TDG_EINVAL
    assert launch(y, m, 7)[0] == TDG_EINVAL
    rc, mean, seed, scal = launch(y, m, 0, ws_bytes=16)
    assert rc == TDG_EWORKSPACE and scal[0] == SENTINEL and np.all(seed == SENTINEL) and np.all(mean == SENTINEL)
    lib, Kk = L().load(), K()
    buf = torch.zeros(64, device=DEV)
    for bad in (dict(y=None), dict(m=None), dict(mean=None), dict(seed=None), dict(scal=None), dict(ws=None), dict(m_cs=0),
                dict(seed_cs=0), dict(m_cs=-1)):
        a = dict(y=buf, m=buf, mean=buf, seed=buf, scal=buf, ws=buf, m_cs=1, seed_cs=1)
        a.update(bad)
        rc = lib.tdg_mde_loss(0, Kk.ptr(a['y']), 3, 7, Kk.ptr(a['m']), a['m_cs'], Kk.ptr(a['mean']), Kk.ptr(a['seed']), a['seed_cs'],
                              Kk.ptr(a['scal']), Kk.ptr(a['ws']), 256, Kk.stream())
        assert rc == TDG_EINVAL, bad
    assert 'tdg_mde_loss' in lib.tdg_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(buf == 0)
