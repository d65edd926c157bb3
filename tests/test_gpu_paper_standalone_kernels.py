"""tdg_cgan_rmse_loss and tdg_cgan_bar_fill (3dgan_amd/csrc/tdg_cgan_standalone.hip) against float64 NumPy on the same f32
inputs.  The bounds follow from the arithmetic: the kernel's differences, squares and sums are f64, so the loss and every
f32 gradient entry are the f32 rounding of a value that agrees with the oracle's to some 1e-15 relative -- within ONE f32
spacing of the oracle's value -- and a bf16 entry is that f32 value rounded again: within one bf16 spacing."""
import numpy as np
import pytest
import torch

from conftest import pkg
from test_gpu_paper_cgan import dev, DEV

pytestmark = pytest.mark.gpu
SENTINEL = 77.0
TDG_EINVAL, TDG_EWORKSPACE = -1, -4


def L():
    return pkg('_lib')


def K():
    return pkg('kernels')


def pair(n, hw, seed):
    rng = np.random.default_rng([seed, n, hw])
    y = rng.uniform(0.1, 10, (n, hw)).astype(np.float32)
    yhat = (y * rng.uniform(0.6, 1.6, (n, hw))).astype(np.float32) - np.float32(0.5)
    return y, yhat


def oracle(y, yhat):
    d = yhat.astype(np.float64) - y.astype(np.float64)
    S, N = np.sum(d * d), d.size
    return np.sqrt(S / N) / 10.0, d / (10.0 * np.sqrt(N * S))


def spacing_bf16(v):
    """The spacing of bf16 at |v| (8 significant bits), for normal values."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


def launch(y, yhat, dt, cs, ws_bytes=None):
    n, hw = y.shape
    lib = L().load()
    need = lib.tdg_cgan_rmse_loss_workspace_bytes(n, hw)
    ws = torch.zeros(max(need if ws_bytes is None else ws_bytes, 8), dtype=torch.uint8, device=DEV)
    dg = torch.full((n * hw * cs,), SENTINEL, dtype=torch.bfloat16 if dt else torch.float32, device=DEV)
    scal = torch.full((2,), SENTINEL, device=DEV)
    yd, pd = dev(y), dev(yhat)
    rc = lib.tdg_cgan_rmse_loss(dt, K().ptr(yd), K().ptr(pd), n, hw, K().ptr(dg), cs, K().ptr(scal), K().ptr(ws),
                                need if ws_bytes is None else ws_bytes, K().stream())
    torch.cuda.synchronize()
    return rc, dg.float().cpu().numpy().reshape(n * hw, cs), scal.cpu().numpy()


@pytest.mark.parametrize('cs', [1, 8])
@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('n,hw', [(1, 841), (3, 841), (8, 841), (3, 70), (512, 841)])
def test_rmse_loss_against_float64(n, hw, dt, cs):
    y, yhat = pair(n, hw, 3)
    rc, dg, scal = launch(y, yhat, dt, cs)
    assert rc == 0
    loss, grad = oracle(y, yhat)
    grad = grad.ravel()
    err_l = abs(float(scal[0]) - loss)
    print('n %d hw %d dt %d cs %d: loss %.9g (oracle %.9g, %.2f spacings), max gradient error %.2f spacings'
          % (n, hw, dt, cs, scal[0], loss, err_l / np.spacing(np.float32(loss)),
             np.max(np.abs(dg[:, 0] - grad) / (spacing_bf16(grad) if dt else np.spacing(np.abs(grad).astype(np.float32))))))
    assert err_l <= np.spacing(np.float32(loss))
    assert scal[1] == SENTINEL
    bound = spacing_bf16(grad) if dt else np.spacing(np.abs(grad).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(dg[:, 0] - grad) <= bound)
    assert np.any(dg[:, 0] != 0)
    if cs > 1:
        assert np.all(dg[:, 1:] == SENTINEL)                   # only channel 0 of a strided buffer is written
    rc2, dg2, scal2 = launch(y, yhat, dt, cs)
    assert rc2 == 0 and np.array_equal(dg, dg2) and scal[0].tobytes() == scal2[0].tobytes()      # two launches: bit-equal


@pytest.mark.parametrize('dt', [0, 1])
def test_rmse_loss_of_a_perfect_prediction_is_zero_with_a_zero_gradient(dt):
    y, _ = pair(3, 841, 5)
    rc, dg, scal = launch(y, y.copy(), dt, 8)
    assert rc == 0 and scal[0] == 0.0
    assert np.all(np.isfinite(dg)) and np.all(dg[:, 0] == 0.0) and np.all(dg[:, 1:] == SENTINEL)


def test_rmse_loss_rejects_bad_arguments_before_any_launch():
    lib, k = L().load(), K()
    y, yhat = pair(3, 841, 7)
    yd, pd = dev(y), dev(yhat)
    dg = torch.full((3 * 841,), SENTINEL, device=DEV)
    scal = torch.full((1,), SENTINEL, device=DEV)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    s = k.stream()
    good = [0, k.ptr(yd), k.ptr(pd), 3, 841, k.ptr(dg), 1, k.ptr(scal), k.ptr(ws), 64, s]
    for i in (1, 2, 5, 7, 8):
        bad = list(good)
        bad[i] = None
        assert lib.tdg_cgan_rmse_loss(*bad) == TDG_EINVAL
    for i, v in ((0, 5), (3, 0), (4, 0), (6, 0)):
        bad = list(good)
        bad[i] = v
        assert lib.tdg_cgan_rmse_loss(*bad) == TDG_EINVAL
    need = lib.tdg_cgan_rmse_loss_workspace_bytes(3, 841)
    assert need == 8 * 3
    short = list(good)
    short[9] = need - 1
    assert lib.tdg_cgan_rmse_loss(*short) == TDG_EWORKSPACE
    torch.cuda.synchronize()
    assert torch.all(dg == SENTINEL) and scal[0] == SENTINEL       # nothing ran
    assert lib.tdg_cgan_bar_fill(0, None, 3, 961, k.ptr(dg), 1, None, s) == TDG_EINVAL
    assert lib.tdg_cgan_bar_fill(0, k.ptr(scal), 3, 961, None, 1, None, s) == TDG_EINVAL
    assert lib.tdg_cgan_bar_fill(0, k.ptr(scal), 0, 961, k.ptr(dg), 1, None, s) == TDG_EINVAL


@pytest.mark.parametrize('dt', [0, 1])
def test_bar_fill_writes_one_channel_and_the_plane(dt):
    B, hw2, cs, ch = 3, 31 * 31, 136, 128
    ybar = np.array([3.14159274, 0.1, 7.77777], np.float32)
    tdt = torch.bfloat16 if dt else torch.float32
    buf = torch.full((B * hw2 * cs,), SENTINEL, dtype=tdt, device=DEV)
    plane = torch.full((B * hw2 + 5,), SENTINEL, device=DEV)
    yb = dev(ybar)
    k = K()
    L().call('tdg_cgan_bar_fill', dt, k.ptr(yb), B, hw2, k.ptr(buf, ch * (2 if dt else 4)), cs, k.ptr(plane), k.stream())
    torch.cuda.synchronize()
    got = buf.float().cpu().numpy().reshape(B, hw2, cs)
    want = torch.tensor(ybar).to(tdt).float().numpy()
    assert np.array_equal(got[:, :, ch], np.repeat(want[:, None], hw2, axis=1))
    got[:, :, ch] = SENTINEL
    assert np.all(got == SENTINEL)                                # everything else untouched
    p = plane.cpu().numpy()
    assert np.array_equal(p[:B * hw2].reshape(B, hw2), np.repeat(ybar[:, None], hw2, axis=1)) and np.all(p[B * hw2:] == SENTINEL)
    # without a plane the window alone is written
    buf.fill_(SENTINEL)
    L().call('tdg_cgan_bar_fill', dt, k.ptr(yb), B, hw2, k.ptr(buf, ch * (2 if dt else 4)), cs, None, k.stream())
    torch.cuda.synchronize()
    assert np.array_equal(buf.float().cpu().numpy().reshape(B, hw2, cs)[:, :, ch], np.repeat(want[:, None], hw2, axis=1))
