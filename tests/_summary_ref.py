"""Float64 NumPy oracle of the tensor summaries (tdg_tensor_summary, summaries.host_summary, TensorSummary.histo),
independent of the package: TensorFlow's default histogram limits by its own loop, buckets by np.searchsorted(side='right')
(upper_bound), the proto's collapse of empty runs, exact sums by math.fsum."""
import math
import sys

import numpy as np

N_LIMITS, N_POS, ZERO_BUCKET = 1551, 774, 776


def limits():
    pos = []
    v = 1.0e-12
    while v < 1.0e20:
        pos.append(v)
        v *= 1.1
    dbl_max = sys.float_info.max
    return np.array([-dbl_max] + [-p for p in reversed(pos)] + [0.0] + pos + [dbl_max], dtype=np.float64)


LIMITS = limits()


def scaled(x, scale=1.0):
    """The element values: f32(x) * scale in ONE f32 multiply (x: float32 array, any shape)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all='ignore'):
        return (x * np.float32(scale)).astype(np.float32).reshape(-1)


def summary(x, scale=1.0):
    """dict(num, zeros, nonfinite, min, max, sum, sum_squares, buckets, abs_sum, abs_sum_squares, finite) of the live
    elements x.  The last three are for the bound of a recursive f64 summation: finite * 2^-53 * sum |term|."""
    v = scaled(x, scale)
    fin = np.isfinite(v)
    f = v[fin].astype(np.float64)
    b = np.searchsorted(LIMITS, f, side='right')
    squares = math.fsum(f * f)                                             # (the f64 square of an f32 is exact, and >= 0)
    out = {
        'num': int(v.size), 'zeros': int(np.count_nonzero(f == 0.0)), 'nonfinite': int(v.size - f.size), 'finite': int(f.size),
        'min': float(f.min()) if f.size else 0.0, 'max': float(f.max()) if f.size else 0.0,
        'sum': math.fsum(f), 'sum_squares': squares, 'abs_sum': math.fsum(np.abs(f)), 'abs_sum_squares': squares,
        'buckets': np.bincount(b, minlength=N_LIMITS).astype(np.int64),
    }
    assert out['buckets'].size == N_LIMITS
    return out


def sum_bounds(ref):
    """(bound on |sum - fsum|, bound on |sum_squares - fsum|) for any order of f64 additions of the terms."""
    u = 2.0 ** -53
    return ref['finite'] * u * ref['abs_sum'], ref['finite'] * u * ref['abs_sum_squares']


def collapse(buckets):
    """HistogramProto's (bucket_limit, bucket): a run of consecutive empty buckets becomes one entry with the run's last
    limit and count 0 (Histogram::EncodeToProto with preserve_zero_buckets = false)."""
    lim, cnt = [], []
    i, n = 0, len(buckets)
    while i < n:
        end, c = LIMITS[i], float(buckets[i])
        i += 1
        if c <= 0.0:
            while i < n and buckets[i] <= 0:
                end, c = LIMITS[i], float(buckets[i])
                i += 1
        lim.append(float(end))
        cnt.append(c)
    return lim, cnt


def _neighbours(v, dtype):
    """v rounded to the dtype, with the next value below and above in that dtype (f32 values)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over='ignore'):
        f = v.astype(np.float32)
    if dtype == 'f32':
        return np.concatenate([np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))])
    # bf16: round to nearest even on the top 16 bits, neighbours one bf16 ulp away
    bits = f.view(np.uint32).astype(np.uint64)
    h = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.int64)
    key = np.where(h & 0x8000, -(h & 0x7FFF), h)                   # monotone in the value: the neighbours are key -+ 1
    out = []
    for d in (-1, 0, 1):
        k = key + d
        hh = np.where(k < 0, 0x8000 | -k, k).astype(np.uint32)
        out.append((hh << 16).astype(np.uint32).view(np.float32))
    return np.concatenate(out)


def edge_values(dtype):
    """Every interior limit (all but +-DBL_MAX) rounded to the dtype, with its two neighbours in that dtype: 4647 values;
    the finite ones are kept (bf16 and f32 share the exponent range, so only the neighbours of the largest limits can
    leave it)."""
    v = _neighbours(LIMITS[1:-1], dtype)
    assert v.size == 3 * (N_LIMITS - 2)
    return v[np.isfinite(v)].astype(np.float32)
