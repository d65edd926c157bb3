"""NumPy float32 oracle of tdg_activation_montage (include/tdg.h): hem.montage's layout through summaries.montage /
factorization, and TensorFlow's float-image rule in the same f32 steps -- one divide, one multiply, one add, a minimum with
255, truncation -- so that the comparison with the kernel is exact."""
import numpy as np

from conftest import pkg

F = np.float32


def scale_offset(lo, hi):
    lo, hi = F(lo), F(hi)
    if lo < 0:
        big = max(abs(lo), abs(hi))
        return (F(0) if big < F(1e-6) else F(127.0) / big), F(128.0)
    return (F(0) if hi < F(1e-6) else F(255.0) / hi), F(0)


def montage(image):
    """image: [h, w, c] (any float dtype whose values are f32 values) -> (uint8 [n*h, m*w], lo, hi)."""
    S = pkg('summaries')
    x = np.asarray(image, dtype=F)
    assert x.ndim == 3
    fin = np.isfinite(x)
    lo, hi = (F(x[fin].min()) + F(0), F(x[fin].max()) + F(0)) if fin.any() else (F(0), F(0))      # (+ 0: one zero, never -0)
    scale, offset = scale_offset(lo, hi)
    with np.errstate(all='ignore'):
        t = (np.where(fin, x, F(0)) * scale).astype(F)
        u = np.minimum((t + offset).astype(F), F(255.0))
    px = np.where(fin, u.astype(np.uint8), np.uint8(255))
    planes = np.transpose(px, (2, 0, 1))                     # [c, h, w]: hem.montage on the channel planes
    m, n = S.factorization(x.shape[2])
    out = S.montage(planes, m, n)[:, :, 0]
    assert out.shape == (n * x.shape[0], m * x.shape[1])
    return out, float(lo), float(hi)
