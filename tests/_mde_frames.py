"""Hand-made nyuv2 frames for the mean_depth_estimator tests: seeded 8-bit RGB and 16-bit depth frames around 100 x 130, free
of the sensor-gap values 0 and 65535, and the TFRecord file the nyuv2 plugin reads them from."""
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import torch

H, W, N = 100, 130, 6
CASES = {'crop': dict(random_crop=(9, 11), resize=None), 'resize_crop': dict(random_crop=(8, 7), resize=(52, 40)),
         'resize': dict(random_crop=None, resize=(13, 10))}        # --resize is W H, --random_crop is H W
GOLDEN_SEED, GOLDEN_B, GOLDEN_BATCHES = 5, 3, 2


def frames(n=N, h=H, w=W, seed=0):
    """(rgb uint8 [n,h,w,3], depth uint16 [n,h,w]): a smooth ramp per frame plus noise, each frame at its own depth level."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    level = rng.uniform(8000, 50000, (n, 1, 1))
    ramp = np.linspace(0, 6000, w)[None, None, :] + np.linspace(0, 3000, h)[None, :, None]
    depth = (level + ramp + rng.uniform(-500, 500, (n, h, w))).round().astype(np.uint16)
    assert depth.min() > 0 and depth.max() < 65535
    return rgb, depth


def source(case, flags=None, seed=GOLDEN_SEED, batch_size=GOLDEN_B, device='cpu'):
    """nyuv2.PairSource on frames() the way NYUv2Dataset.get_source builds it, for CASES[case] plus `flags`."""
    from conftest import pkg
    nyu = pkg('data_plugins.nyuv2')
    rgb, depth = frames()
    c = CASES[case]
    extra = dict(flags or {})
    return nyu.PairSource(rgb, depth, batch_size, torch.device(device), c['random_crop'], c['resize'], seed, 0, 1, **extra)


def png(a):
    """PNG bytes of an [h, w, 3] uint8 or [h, w] uint16 array (filter 0 on every row)."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    depth16 = a.dtype == np.uint16
    rows = a.astype('>u2' if depth16 else np.uint8)
    raw = b''.join(b'\x00' + rows[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 16 if depth16 else 8, 0 if depth16 else 2, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def write_tfrecords(path, rgb, depth):
    """The records of hem/data/nyuv2.py:121-146 as `path`."""
    from conftest import pkg
    tfr = pkg('tfrecord')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tfr.write_records(path, [tfr.make_example({'image': png(a), 'depth': png(d), 'width': a.shape[1], 'height': a.shape[0], 'channels': 3})
                             for a, d in zip(rgb, depth)])
