"""Event files on the host: the histogram limits, TensorSummary / host_summary against the float64 oracle, the hand-encoded
protobuf of EventWriter read back by a wire decoder of the test's own (and by google.protobuf where it imports), the
readers of hem/ops/summaries.py:204-242, the --event_files flag and the cadence of hem/util/training.py:142-150."""
import os
import struct
import sys

import numpy as np
import pytest

from conftest import pkg, ROOT

import _summary_ref as R


# ---------------------------------------------------------------------------------------------- limits and buckets
def test_library_limits_equal_the_oracle_bit_for_bit():
    import ctypes as C
    L = pkg('_lib')
    buf = (C.c_double * R.N_LIMITS)()
    assert L.load().tdg_tensor_summary_limits(buf) == 0
    got = np.frombuffer(buf, dtype=np.float64)
    assert got.size == 1551 and got.tobytes() == R.LIMITS.tobytes()
    assert got[776] == 1e-12 and got[775] == 0.0 and got[0] == -sys.float_info.max and got[1550] == sys.float_info.max
    assert np.all(np.diff(got) > 0)
    assert L.load().tdg_tensor_summary_limits(None) == -1 and b'tdg_tensor_summary_limits' in L.load().tdg_last_error()
    assert np.array_equal(pkg('summaries').limits(), R.LIMITS)


def test_host_checked_bucket_examples():
    """The examples of the bucket definition.  The f32 nearest to 1e-12 is 9.99999996e-13, BELOW the limit 1e-12, so by the
    rule (the number of limits <= v) it lies in bucket 776; its upper f32 neighbour is the first value of bucket 777."""
    S = pkg('summaries')
    tiny = np.float32(1e-12)
    assert float(tiny) < 1e-12 < float(np.nextafter(tiny, np.float32(1)))
    fmax = np.finfo(np.float32).max
    for v, want in ((0.0, 776), (-0.0, 776), (np.float32(1e-45), 776), (tiny, 776), (np.nextafter(tiny, np.float32(1)), 777),
                    (1.0, 1066), (-1.0, 485), (fmax, 1550), (-fmax, 1)):
        assert list(np.nonzero(S.host_summary([v]).buckets)[0]) == [want], (v, want)
        assert list(np.nonzero(R.summary([v])['buckets'])[0]) == [want], (v, want)


def test_edge_set_covers_every_reachable_bucket():
    for dt in ('f32', 'bf16'):
        e = R.edge_values(dt)
        assert e.size == 4647 and np.all(np.isfinite(e))
        b = R.summary(e)['buckets']
        assert b[0] == 0 and np.all(b[1:] > 0)                       # buckets 1..1550: all a finite value can reach


def check_against_oracle(s, ref):
    assert (s.num, s.zeros, s.nonfinite) == (ref['num'], ref['zeros'], ref['nonfinite'])
    assert s.min == ref['min'] and s.max == ref['max']
    assert np.array_equal(s.buckets, ref['buckets'])
    bs, bq = R.sum_bounds(ref)
    assert abs(s.sum - ref['sum']) <= bs and abs(s.sum_squares - ref['sum_squares']) <= bq
    assert s.histo() == R.collapse(ref['buckets'])
    if s.num:
        assert s.mean == s.sum / s.num and s.sparsity == s.zeros / s.num


@pytest.mark.parametrize('name', ['empty_runs', 'single', 'zeros', 'both_sides', 'nonfinite', 'scaled'])
def test_host_summary_and_histo_against_the_oracle(name):
    S = pkg('summaries')
    rng = np.random.default_rng(3)
    scale = 1.0
    if name == 'empty_runs':
        x = np.array([1e-3, 1e-3, 5.0, 5.0, 5.0, 7e4], np.float32)           # occupied buckets with empty runs between them
    elif name == 'single':
        x = np.array([0.37], np.float32)
    elif name == 'zeros':
        x = np.zeros(33, np.float32)
    elif name == 'both_sides':
        x = np.concatenate([rng.standard_normal(500), [0.0, -0.0], -np.abs(rng.standard_normal(20)) * 1e-9]).astype(np.float32)
    elif name == 'nonfinite':
        x = np.array([1.0, np.nan, -2.0, np.inf, -np.inf, 0.0], np.float32)
    else:
        x, scale = rng.standard_normal(100).astype(np.float32), 1.0 / 3.0
    s = S.host_summary(x, scale)
    check_against_oracle(s, R.summary(x, scale))
    lim, cnt = s.histo()
    assert len(lim) == len(cnt) and sum(cnt) == s.num - s.nonfinite and lim[-1] == sys.float_info.max
    if name == 'single':
        assert cnt == [0.0, 1.0, 0.0] and lim[0] < 0.37 < lim[1]
    if name == 'zeros':
        assert cnt == [0.0, 33.0, 0.0] and lim[:2] == [0.0, 1e-12]
    if name == 'empty_runs':
        assert cnt == [0.0, 2.0, 0.0, 3.0, 0.0, 1.0, 0.0]
    assert S.host_summary(np.zeros(0, np.float32)).num == 0 and S.host_summary(np.zeros(0, np.float32)).mean == 0.0


# ---------------------------------------------------------------------------------------------- wire format
def decode(buf):
    """[(field number, wire type, value)] of one message: varint (0), 64-bit (1), length-delimited (2), 32-bit (5)."""
    out, i = [], 0
    while i < len(buf):
        key = shift = 0
        while True:
            b = buf[i]
            i += 1
            key |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        fn, wt = key >> 3, key & 7
        if wt == 0:
            v = shift = 0
            while True:
                b = buf[i]
                i += 1
                v |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
        elif wt == 1:
            v, i = buf[i:i + 8], i + 8
        elif wt == 5:
            v, i = buf[i:i + 4], i + 4
        else:
            assert wt == 2, wt
            n = shift = 0
            while True:
                b = buf[i]
                i += 1
                n |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
            v, i = buf[i:i + n], i + n
            assert len(v) == n
        out.append((fn, wt, bytes(v) if wt else v))
    return out


f64 = lambda b: struct.unpack('<d', b)[0]
PNG = pkg('summaries').png_bytes(np.linspace(0, 1, 2 * 3 * 3).reshape(2, 3, 3))


@pytest.fixture(scope='module')
def event_file(tmp_path_factory):
    S = pkg('summaries')
    d = tmp_path_factory.mktemp('events')
    x = np.array([-1.5, 0.0, 0.25, 0.25, 3.0], np.float32)
    w = S.EventWriter(str(d), wall_time=1234567890.5)
    w.scalar('loss/g', 0.75, 7, wall_time=100.25)
    w.histogram('weights/w', S.host_summary(x), 7)
    w.image('montage', PNG, 2, 3, 3, 7)
    w.scalar('loss/g', 1.5, 9, wall_time=200.0)              # a second event
    w.close()
    return w.path, x


def test_event_file_wire_format(event_file):
    path, x = event_file
    import socket
    assert os.path.basename(path) == 'events.out.tfevents.1234567890.' + socket.gethostname()
    recs = list(pkg('tfrecord').read_records(path, verify=True))            # both masked CRCs of every record
    assert len(recs) == 3
    assert decode(recs[0]) == [(1, 1, struct.pack('<d', 1234567890.5)), (3, 2, b'brain.Event:2')]     # the file version first
    ev = decode(recs[1])
    assert [(fn, wt) for fn, wt, _ in ev] == [(1, 1), (2, 0), (5, 2)]
    assert f64(ev[0][2]) == 100.25 and ev[1][2] == 7
    values = decode(ev[2][2])
    assert [(fn, wt) for fn, wt, _ in values] == [(1, 2)] * 3                # Summary.value, three of them in ONE event
    scalar, histo, image = (decode(v) for _, _, v in values)
    assert scalar == [(1, 2, b'loss/g'), (2, 5, struct.pack('<f', 0.75))]
    assert histo[0] == (1, 2, b'weights/w') and [(fn, wt) for fn, wt, _ in histo] == [(1, 2), (5, 2)]
    h = decode(histo[1][2])
    assert [(fn, wt) for fn, wt, _ in h] == [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2), (7, 2)]
    ref = R.summary(x)
    assert [f64(v) for _, _, v in h[:5]] == [-1.5, 3.0, 5.0, ref['sum'], ref['sum_squares']]
    lim, cnt = R.collapse(ref['buckets'])
    assert list(np.frombuffer(h[5][2], '<f8')) == lim and list(np.frombuffer(h[6][2], '<f8')) == cnt
    assert cnt == [0.0, 1.0, 0.0, 1.0, 0.0, 2.0, 0.0, 1.0, 0.0]
    assert image[0] == (1, 2, b'montage/image/0') and [(fn, wt) for fn, wt, _ in image] == [(1, 2), (4, 2)]
    assert decode(image[1][2]) == [(1, 0, 2), (2, 0, 3), (3, 0, 3), (4, 2, PNG)]
    ev2 = decode(recs[2])
    assert f64(ev2[0][2]) == 200.0 and ev2[1][2] == 9 and decode(decode(ev2[2][2])[0][2]) == [(1, 2, b'loss/g'), (2, 5, struct.pack('<f', 1.5))]


def test_event_file_parses_with_google_protobuf(event_file):
    pytest.importorskip('google.protobuf')
    from google.protobuf import descriptor_pb2, descriptor_pool
    from google.protobuf import message_factory
    get_class = getattr(message_factory, 'GetMessageClass', None) or message_factory.MessageFactory().GetPrototype
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name='tdg_event_test.proto', package='tdgtest', syntax='proto3')

    def message(name, fields):
        m = fd.message_type.add(name=name)
        for fname, number, ftype, label, type_name in fields:
            f = m.field.add(name=fname, number=number, type=ftype, label=label)
            if type_name:
                f.type_name = '.tdgtest.' + type_name
    one, many = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    message('HistogramProto', [('min', 1, F.TYPE_DOUBLE, one, None), ('max', 2, F.TYPE_DOUBLE, one, None), ('num', 3, F.TYPE_DOUBLE, one, None),
                               ('sum', 4, F.TYPE_DOUBLE, one, None), ('sum_squares', 5, F.TYPE_DOUBLE, one, None),
                               ('bucket_limit', 6, F.TYPE_DOUBLE, many, None), ('bucket', 7, F.TYPE_DOUBLE, many, None)])
    message('Image', [('height', 1, F.TYPE_INT32, one, None), ('width', 2, F.TYPE_INT32, one, None), ('colorspace', 3, F.TYPE_INT32, one, None),
                      ('encoded_image_string', 4, F.TYPE_BYTES, one, None)])
    message('Value', [('tag', 1, F.TYPE_STRING, one, None), ('simple_value', 2, F.TYPE_FLOAT, one, None),
                      ('image', 4, F.TYPE_MESSAGE, one, 'Image'), ('histo', 5, F.TYPE_MESSAGE, one, 'HistogramProto')])
    message('Summary', [('value', 1, F.TYPE_MESSAGE, many, 'Value')])
    message('Event', [('wall_time', 1, F.TYPE_DOUBLE, one, None), ('step', 2, F.TYPE_INT64, one, None), ('file_version', 3, F.TYPE_STRING, one, None),
                      ('summary', 5, F.TYPE_MESSAGE, one, 'Summary')])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    Event = get_class(pool.FindMessageTypeByName('tdgtest.Event'))
    path, x = event_file
    recs = list(pkg('tfrecord').read_records(path, verify=True))
    first = Event.FromString(recs[0])
    assert first.file_version == 'brain.Event:2' and first.wall_time == 1234567890.5
    e = Event.FromString(recs[1])
    assert e.step == 7 and e.wall_time == 100.25 and len(e.summary.value) == 3
    s, h, im = e.summary.value
    assert s.tag == 'loss/g' and s.simple_value == 0.75
    ref = R.summary(x)
    assert h.tag == 'weights/w' and (h.histo.min, h.histo.max, h.histo.num) == (-1.5, 3.0, 5.0)
    assert h.histo.sum == ref['sum'] and h.histo.sum_squares == ref['sum_squares']
    assert (list(h.histo.bucket_limit), list(h.histo.bucket)) == R.collapse(ref['buckets'])
    assert im.tag == 'montage/image/0' and (im.image.height, im.image.width, im.image.colorspace) == (2, 3, 3)
    assert im.image.encoded_image_string == PNG
    assert Event.FromString(recs[2]).summary.value[0].simple_value == 1.5


def test_read_events_and_get_tag_values(event_file, tmp_path):
    S = pkg('summaries')
    path, x = event_file
    ev = S.read_events([path])
    assert set(ev) == {'scalar', 'image', 'histo'}
    assert S.get_tag_values('scalar', 'loss/g', ev) == [(7, 100.25, 0.75), (9, 200.0, 1.5)]
    (step, wall, h), = S.get_tag_values('histo', 'weights/w', ev)
    ref = R.summary(x)
    assert step == 7 and wall == 100.25 and (h['min'], h['max'], h['num'], h['sum'], h['sum_squares']) == (-1.5, 3.0, 5.0, ref['sum'], ref['sum_squares'])
    assert (h['bucket_limit'], h['bucket']) == R.collapse(ref['buckets'])
    (step, _, im), = S.get_tag_values('image', 'montage/image/0', ev)
    assert step == 7 and im == {'height': 2, 'width': 3, 'colorspace': 3, 'encoded_image_string': PNG}
    # two entries at one step: the later wall time wins, whatever the file order; the result is sorted by step
    w = S.EventWriter(str(tmp_path), wall_time=5.0)
    w.scalar('a', 1.0, 4, wall_time=50.0)
    w.flush()
    w.scalar('a', 2.0, 4, wall_time=60.0)
    w.flush()
    w.scalar('a', 3.0, 4, wall_time=40.0)
    w.scalar('a', 0.5, 2, wall_time=70.0)
    w.scalar('a', -1.0, -3, wall_time=80.0)                                # (int64 steps: a negative one survives the varint)
    w.close()
    ev2 = S.read_events([w.path])
    assert S.get_tag_values('scalar', 'a', ev2) == [(-3, 80.0, -1.0), (2, 70.0, 0.5), (4, 60.0, 2.0)]
    assert len(ev2['scalar']['a']) == 5
    with pytest.raises(ValueError):
        w.scalar('a', 1.0, 5)                                              # closed


def test_histogram_refuses_non_finite_by_tag(tmp_path):
    S = pkg('summaries')
    w = S.EventWriter(str(tmp_path))
    with pytest.raises(ValueError, match='g_activations/dead/e1'):
        w.histogram('g_activations/dead/e1', S.host_summary([1.0, float('nan')]), 1)
    with pytest.raises(ValueError, match='loss/g'):
        w.histogram('loss/g', S.host_summary([float('inf')]), 1)
    w.histogram('fine', S.host_summary([1.0]), 1)
    w.close()
    assert list(S.read_events([w.path])['histo']) == ['fine']


# ---------------------------------------------------------------------------------------------- flag and cadence
def test_event_files_flag_parses_and_defaults_off():
    sys.path.insert(0, ROOT)
    import train
    assert train.parse_args(['--model', 'gan', '--dataset', 'synthetic']).event_files is False
    assert train.parse_args(['--model', 'gan', '--dataset', 'synthetic', '--event_files']).event_files is True


def test_cadence_predicate():
    """hem/util/training.py:142-150: i % (n // 10) == 0 in epochs 0..2, i % (n // 3) == 0 after; divisor kept from 0."""
    due = pkg('summaries').event_due
    want = {
        (1, 0): [0], (1, 2): [0], (1, 3): [0],
        (9, 0): list(range(9)), (9, 2): list(range(9)), (9, 3): [0, 3, 6],
        (10, 0): list(range(10)), (10, 2): list(range(10)), (10, 3): [0, 3, 6, 9],
        (33, 0): list(range(0, 33, 3)), (33, 2): list(range(0, 33, 3)), (33, 3): [0, 11, 22],
    }
    for (n, epoch), steps in want.items():
        assert [i for i in range(n) if due(epoch, i, n)] == steps, (n, epoch)
