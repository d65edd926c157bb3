"""Summaries: the per-epoch CSV / PNG record and the TensorBoard event files of a run.

Summaries-lite: what a person looks at to compare a run with the reference -- the loss scalars
and the 8x8 `inputs` / `fake` montages of `models/gan.py:93-107` -- without TensorBoard: one CSV row per epoch
and two PNG files per epoch, written with zlib only.

montage(): the tensor algebra of `ops/summaries.py:97-124` (`montage_summary`): split the batch into n chunks,
stack the chunks vertically, then lay the m images of every chunk out horizontally, i.e. image j*m + r lands at
block row j, block column r.  factorization(): `ops/summaries.py:79-92`.

Event files (`train.py --event_files`): what hem.summarize_layers / summarize_gradients /
summarize_losses / summarize_weights_biases (hem/ops/summaries.py:13-75) record on every run -- per layer, gradient and
weight a histogram, the zero fraction as `/sparsity` and the mean -- in `<dir>/train/events.out.tfevents.*`, the file
`paper_visualize.py` and hem.get_all_events / get_tag_values (hem/ops/summaries.py:204-242) read back.  The statistics of a
device tensor come from tdg_tensor_summary (kernels.TensorSummaries), those of a host value from host_summary; both give
a TensorSummary.  EventWriter encodes the Event / Summary / HistogramProto messages by hand in TFRecord framing;
read_events / get_tag_values restate the reference's readers.  Which tensors a replica records: engine.Replica.summary_items
and write_event.
DEVIATION: TensorFlow uniquifies a tag that is used twice (`linear_rmse_1`, `generator/encoder_1`); tags here are the
    names themselves (`g_activations/generator/encoder/e1`), never suffixed.
Activation montages (`--event_montages`): hem.summarize_layers(..., montage=True) lays the channels of image 0 of every
recorded layer out with hem.montage and hands the result to tf.summary.image; tdg_activation_montage
(kernels.ActivationMontages) computes those bytes on the device, write_event(montages=True) wraps them into grey PNGs under
`<tag>/montage/image/0`.  Validation and test passes (`train.py --validation`, `--test_epochs`): hem.inference's events go to
`<dir>/validate` and `<dir>/test`, of a held-out batch run through Replica.observe.
DEVIATION: the activations recorded in a TRAIN event are those the last train() left in the replica's buffers; the reference
    runs a forward pass of its own, on a fresh batch, for every event.  (A validate / test event is of its own fresh batch.)
DEVIATION: only the depth family of models/paper/paper_cgan.py records activations and their montages; every other model
    records losses, weights and gradients.
DEVIATION: tf.summary.image's value rule is restated from TensorFlow 1.x's NormalizeFloatImage (include/tdg.h); the PNG is
    this package's encoder's (zlib level 6, filter type 0), not libpng's: the decoded samples are the same, the file bytes not.
DEVIATION: the reference's test call has the wrong arity (training.py:168, paper_train.py:106) and never ran; the test pass
    here has the validation call's shape and is fed the validation mean image.
DEVIATION: get_all_events never appends a histogram it finds (hem/ops/summaries.py:215-217 only creates the tag's list);
    read_events appends it.
"""
import os
import socket
import struct
import time
import zlib
from math import sqrt

import numpy as np


def factorization(n):
    """ops/summaries.py:79-92: the largest i <= sqrt(n) dividing n, as (i, n // i)."""
    for i in range(int(sqrt(float(n))), 0, -1):
        if n % i == 0:
            return (i, int(n / i))


def montage(x, m=0, n=0):
    """x: [m*n, H, W, C] (or [m*n, H, W]) -> [n*H, m*W, C]."""
    x = np.asarray(x)
    if n == 0 or m == 0:
        m, n = factorization(x.shape[0])
    if x.shape[0] != m * n:
        raise ValueError('montage: %d images do not fill a %d x %d grid' % (x.shape[0], m, n))
    chunks = np.split(x, n, axis=0)                     # n x [m, H, W, C]
    tall = np.concatenate(chunks, axis=1)               # [m, n*H, W, C]
    out = np.concatenate(list(tall), axis=1)            # [n*H, m*W, C]
    if out.ndim < 3:
        out = out[:, :, None]
    return out


def jet(v):
    """Piecewise-linear jet colours of v in [0, 1] -> [..., 3] in [0, 1] (blue, cyan, yellow, red): paper_fullimage.jet, restated
    for the package (hem.montage's colorize=True)."""
    v = np.clip(np.asarray(v, np.float64), 0.0, 1.0)[..., None]
    return np.clip(1.5 - np.abs(4.0 * v - np.array([3.0, 2.0, 1.0])), 0.0, 1.0)


def png_bytes(img01):
    """8-bit PNG (grey, RGB or RGBA by channel count) of an array [H, W, C] in [0, 1]; filter type 0 on every row."""
    a = np.asarray(img01, dtype=np.float64)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    if c not in (1, 3, 4):
        raise ValueError('png: %d channels' % c)
    return png_bytes_u8(np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8))


def png_bytes_u8(u8):
    """8-bit PNG of a uint8 array [H, W] or [H, W, C] as it stands: the samples are the array's bytes."""
    u8 = np.asarray(u8)
    if u8.dtype != np.uint8:
        raise ValueError('png: %s samples, expected uint8' % u8.dtype)
    if u8.ndim == 2:
        u8 = u8[:, :, None]
    h, w, c = u8.shape
    if c not in (1, 3, 4):
        raise ValueError('png: %d channels' % c)
    raw = b''.join(b'\x00' + u8[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    color = {1: 0, 3: 2, 4: 6}[c]
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, color, 0, 0, 0)) +
            chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def write_png(path, img01):
    with open(path, 'wb') as f:
        f.write(png_bytes(img01))


def sample_montages(real_pm1, fake_pm1, examples=64):
    """[('inputs', img), ('fake', img)]: the two montages of models/gan.py:99-103 of samples in [-1, 1] (NHWC), rescaled to
    [0, 1]; an 8 x 8 grid when there are 64 examples, else the reference's factorization.  A sample set that is None is left out."""
    out = []
    for name, t in (('inputs', real_pm1), ('fake', fake_pm1)):
        if t is None:
            continue
        a = (np.asarray(t, dtype=np.float32)[:examples] + 1.0) / 2.0
        m, n = (8, 8) if a.shape[0] == 64 else factorization(a.shape[0])
        out.append((name, montage(a, m, n)))
    return out


def write_epoch(directory, epoch, status, real_pm1=None, fake_pm1=None, examples=64):
    """One `losses.csv` row and, when samples are given ([-1,1], NHWC), the two montages of models/gan.py:99-103
    (rescaled to [0,1]; an 8 x 8 grid when there are 64 examples, else the reference's factorization)."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, 'losses.csv')
    keys = sorted(status)
    new = not os.path.exists(path)
    with open(path, 'a') as f:
        if new:
            f.write('epoch,' + ','.join(keys) + '\n')
        f.write('%d,' % epoch + ','.join('%.8g' % float(status[k]) for k in keys) + '\n')
    written = [path]
    for name, img in sample_montages(real_pm1, fake_pm1, examples):
        p = os.path.join(directory, 'montage-%s-%04d.png' % (name, epoch))
        write_png(p, img)
        written.append(p)
    return written


# ---------------------------------------------------------------------------------------------- tensor summaries
N_LIMITS, ZERO_BUCKET = 1551, 776
_LIMITS = None


def limits():
    """The 1551 bucket limits of TensorFlow's default histogram, as the library builds them (tdg_tensor_summary_limits, host
    code): bucket b counts the elements with limits[b - 1] <= v < limits[b]."""
    global _LIMITS
    if _LIMITS is None:
        import ctypes as C
        from . import _lib
        buf = (C.c_double * N_LIMITS)()
        _lib.call('tdg_tensor_summary_limits', buf)
        _LIMITS = np.frombuffer(buf, dtype=np.float64).copy()
    return _LIMITS


class TensorSummary:
    """The record of one tensor: num, zeros, nonfinite (counts), min, max, sum, sum_squares (of the finite elements, as
    f64) and buckets (int64 [1551])."""

    def __init__(self, num, zeros, nonfinite, min, max, sum, sum_squares, buckets):
        self.num, self.zeros, self.nonfinite = int(num), int(zeros), int(nonfinite)
        self.min, self.max, self.sum, self.sum_squares = float(min), float(max), float(sum), float(sum_squares)
        self.buckets = np.asarray(buckets, dtype=np.int64)
        if self.buckets.shape != (N_LIMITS,):
            raise ValueError('TensorSummary: %s buckets, expected %d' % (self.buckets.shape, N_LIMITS))

    @property
    def mean(self):
        """tf.reduce_mean."""
        return self.sum / self.num if self.num else 0.0

    @property
    def sparsity(self):
        """tf.nn.zero_fraction."""
        return self.zeros / self.num if self.num else 0.0

    def histo(self):
        """HistogramProto's (bucket_limit, bucket) lists: a run of consecutive empty buckets collapses into one entry that
        carries the last limit of the run and count 0 (Histogram::EncodeToProto)."""
        lim, b = limits(), self.buckets
        empty = b <= 0
        run_end = empty & np.append(~empty[1:], True)          # the last bucket of each run of empty ones
        keep = ~empty | run_end
        return lim[keep].tolist(), np.where(empty, 0, b)[keep].astype(np.float64).tolist()

    def __repr__(self):
        return 'TensorSummary(num=%d, zeros=%d, nonfinite=%d, min=%g, max=%g, mean=%g)' % (
            self.num, self.zeros, self.nonfinite, self.min, self.max, self.mean)


def host_summary(values, scale=1.0):
    """The TensorSummary of a host value (a loss scalar, an array) through NumPy, by tdg_tensor_summary's definition: the
    elements are f32(values) * scale in one f32 multiply; non-finite elements count in `nonfinite` only."""
    x = np.asarray(values, dtype=np.float32).reshape(-1)
    with np.errstate(all='ignore'):
        v = x if scale == 1.0 else (x * np.float32(scale)).astype(np.float32)
    f = v[np.isfinite(v)].astype(np.float64)
    b = np.bincount(np.searchsorted(limits(), f, side='right'), minlength=N_LIMITS)
    return TensorSummary(v.size, np.count_nonzero(f == 0.0), v.size - f.size, f.min() if f.size else 0.0, f.max() if f.size else 0.0,
                         f.sum(), (f * f).sum(), b)


# ---------------------------------------------------------------------------------------------- event files
FILE_VERSION = 'brain.Event:2'


def _key(fn, wt):
    from .tfrecord import _enc_varint
    return _enc_varint((fn << 3) | wt)


def _pb_double(fn, v):
    return _key(fn, 1) + struct.pack('<d', float(v))


def _pb_float(fn, v):
    return _key(fn, 5) + struct.pack('<f', float(v))


def _pb_int(fn, v):
    from .tfrecord import _enc_varint
    return _key(fn, 0) + _enc_varint(int(v) & 0xFFFFFFFFFFFFFFFF)


def _pb_packed_doubles(fn, values):
    from .tfrecord import _ld
    return _ld(fn, np.asarray(values, dtype='<f8').tobytes())


class EventWriter:
    """`<logdir>/events.out.tfevents.<seconds>.<hostname>` in TFRecord framing, protobuf encoded by hand:
        Event{wall_time = 1 (double), step = 2 (int64), file_version = 3, summary = 5}    Summary{value = 1}
        Summary.Value{tag = 1, simple_value = 2 (float), image = 4, histo = 5}
        Summary.Image{height = 1, width = 2, colorspace = 3, encoded_image_string = 4}
        HistogramProto{min = 1, max = 2, num = 3, sum = 4, sum_squares = 5, bucket_limit = 6, bucket = 7 (packed doubles)}
    The first record is Event{wall_time, file_version: "brain.Event:2"}.  Values of one step gather in ONE Event, as one
    run of TensorFlow's merged summary op does; the Event is written when the step changes and on flush() / close()."""

    def __init__(self, logdir, wall_time=None):
        os.makedirs(logdir, exist_ok=True)
        t = time.time() if wall_time is None else wall_time
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(t), socket.gethostname()))
        self._f = open(self.path, 'ab')
        self._step, self._wall, self._values = None, None, []
        from .tfrecord import _ld
        self._record(_pb_double(1, t) + _ld(3, FILE_VERSION.encode()))

    def _record(self, payload):
        from .tfrecord import masked_crc
        head = struct.pack('<Q', len(payload))
        self._f.write(head + struct.pack('<I', masked_crc(head)) + payload + struct.pack('<I', masked_crc(payload)))

    def _add(self, step, value, wall_time):
        from .tfrecord import _ld
        if self._f is None:
            raise ValueError('EventWriter: %s is closed' % self.path)
        if self._values and step != self._step:
            self._emit()
        if not self._values:
            self._step, self._wall = int(step), time.time() if wall_time is None else wall_time
        self._values.append(_ld(1, value))

    def _emit(self):
        from .tfrecord import _ld
        if self._values:
            self._record(_pb_double(1, self._wall) + _pb_int(2, self._step) + _ld(5, b''.join(self._values)))
            self._values = []

    def scalar(self, tag, value, step, wall_time=None):
        from .tfrecord import _ld
        self._add(step, _ld(1, tag.encode()) + _pb_float(2, value), wall_time)

    def histogram(self, tag, summary, step, wall_time=None):
        """tf.summary.histogram of a TensorSummary.  A summary with non-finite elements is refused, as TensorFlow's op
        fails on a NaN or Inf input."""
        from .tfrecord import _ld
        if summary.nonfinite > 0:
            raise ValueError('histogram %s: %d of %d elements are NaN or Inf' % (tag, summary.nonfinite, summary.num))
        lim, cnt = summary.histo()
        h = (_pb_double(1, summary.min) + _pb_double(2, summary.max) + _pb_double(3, summary.num) + _pb_double(4, summary.sum) +
             _pb_double(5, summary.sum_squares) + _pb_packed_doubles(6, lim) + _pb_packed_doubles(7, cnt))
        self._add(step, _ld(1, tag.encode()) + _ld(5, h), wall_time)

    def image(self, tag, png, h, w, channels, step, wall_time=None):
        """tf.summary.image of one encoded image: the tag is `<tag>/image/0`, as TF 1 names the first of max_outputs = 3."""
        from .tfrecord import _ld
        img = _pb_int(1, h) + _pb_int(2, w) + _pb_int(3, channels) + _ld(4, bytes(png))
        self._add(step, _ld(1, (tag + '/image/0').encode()) + _ld(4, img), wall_time)

    def flush(self):
        self._emit()
        self._f.flush()

    def close(self):
        if self._f is not None:
            self.flush()
            self._f.close()
            self._f = None


def _doubles(wt, v):
    return list(np.frombuffer(bytes(v), dtype='<f8')) if wt == 2 else [struct.unpack('<d', bytes(v))[0]]


def read_events(files):
    """hem.get_all_events (hem/ops/summaries.py:204-225): {'scalar', 'image', 'histo'} -> tag -> [(step, wall_time, value)] in
    file order.  A scalar's value is a float, an image's a dict of Summary.Image's fields, a histogram's a dict of
    HistogramProto's (bucket_limit and bucket as lists).  Record checksums are verified."""
    from .tfrecord import read_records, _fields
    events = {'scalar': {}, 'image': {}, 'histo': {}}
    for path in files:
        for payload in read_records(path, verify=True):
            step, wall, summary = 0, 0.0, None
            for fn, wt, v in _fields(payload):
                if fn == 1 and wt == 1:
                    wall = struct.unpack('<d', bytes(v))[0]
                elif fn == 2 and wt == 0:
                    step = v - (1 << 64) if v >= 1 << 63 else v
                elif fn == 5 and wt == 2:
                    summary = v
            if summary is None:
                continue
            for fn, wt, value in _fields(summary):
                if fn != 1 or wt != 2:
                    continue
                tag, simple, image, histo = '', 0.0, None, None
                for f2, w2, v in _fields(value):
                    if f2 == 1:
                        tag = bytes(v).decode()
                    elif f2 == 2 and w2 == 5:
                        simple = struct.unpack('<f', bytes(v))[0]
                    elif f2 == 4:
                        image = {'height': 0, 'width': 0, 'colorspace': 0, 'encoded_image_string': b''}
                        for f3, _, x in _fields(v):
                            if f3 in (1, 2, 3):
                                image[('height', 'width', 'colorspace')[f3 - 1]] = x
                            elif f3 == 4:
                                image['encoded_image_string'] = bytes(x)
                    elif f2 == 5:
                        histo = {'min': 0.0, 'max': 0.0, 'num': 0.0, 'sum': 0.0, 'sum_squares': 0.0, 'bucket_limit': [], 'bucket': []}
                        for f3, w3, x in _fields(v):
                            if 1 <= f3 <= 5:
                                histo[('min', 'max', 'num', 'sum', 'sum_squares')[f3 - 1]] = _doubles(w3, x)[0]
                            elif f3 in (6, 7):
                                histo['bucket_limit' if f3 == 6 else 'bucket'] += _doubles(w3, x)
                if image is not None and image['height'] and image['width']:
                    events['image'].setdefault(tag, []).append((step, wall, image))
                elif histo is not None and histo['bucket']:
                    events['histo'].setdefault(tag, []).append((step, wall, histo))
                else:
                    events['scalar'].setdefault(tag, []).append((step, wall, simple))
    return events


def get_tag_values(kind, tag, events):
    """hem.get_tag_values (hem/ops/summaries.py:228-242): the tag's entries sorted by step; among the entries of one step
    the one with the newest wall time wins."""
    vals = sorted(events[kind][tag], key=lambda e: e[1], reverse=True)
    vals.sort(key=lambda e: e[0])
    out, last = [], None
    for v in vals:
        if v[0] != last:
            out.append(v)
        last = v[0]
    return out


def event_due(epoch, i, iter_per_epoch):
    """The in-epoch cadence of hem/util/training.py:142-150, asked after iteration i of epoch `epoch` (both from 0): ten
    events per epoch in the first three epochs, three per epoch after that.  The divisor is kept from 0 for epochs of fewer
    iterations than that (the reference divides by zero there)."""
    every = max(1, iter_per_epoch // 10) if epoch < 3 else max(1, iter_per_epoch // 3)
    return i % every == 0
