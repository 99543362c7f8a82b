"""CPU tier of the column event ingest (hip.event_ingest_columns, MultiStreamSegmenter(event_layout='columns')): EventColumns and its
one-time checks, from_rows against pack_event_records, the four copies of stage_event_columns, the C entry point and the format
enum, and the constructor argument's checker.  The device arithmetic has no restatement of its own: the GPU tier compares its bits
with the restatement of tests/test_host_event_ingest.py on the float64 rows equal to the columns' values."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_host_event_ingest import ROOT, built_lib, packed  # noqa: F401  (built_lib: the fixture)


def _columns(n=6, t=np.float64, xy=np.int16, p=np.uint8):
    g = np.random.default_rng(n)
    pol = g.integers(0, 2, n)
    return (np.sort(g.integers(0, 1000, n)).astype(t), g.integers(0, 40, n).astype(xy), g.integers(0, 24, n).astype(xy),
            (2 * pol - 1).astype(p) if p == np.int8 else pol.astype(p))


# ---------------------------------------------------------------------------------------------- EventColumns
@pytest.mark.parametrize('t', [np.float64, np.int64])
@pytest.mark.parametrize('xy', [np.int16, np.uint16])
@pytest.mark.parametrize('p', [np.uint8, np.int8, np.bool_])
def test_event_columns_accepts_the_delivered_dtypes_and_reports_the_format(t, xy, p):
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    assert (hip.EVCOL_T_I64, hip.EVCOL_XY_U16) == (1, 2)
    cols = _columns(6, t, xy, p)
    c = EventColumns(*cols)
    assert c.format == (hip.EVCOL_T_I64 if t == np.int64 else 0) | (hip.EVCOL_XY_U16 if xy == np.uint16 else 0)
    assert c.n == len(c) == 6
    # held as they are: no copy, no cast
    assert all(got is given for got, given in zip((c.t, c.x, c.y, c.p), cols))
    with pytest.raises(AttributeError):
        c.t = cols[0]
    # CPU torch tensors: viewed as numpy on the same memory
    tt = [torch.from_numpy(a) for a in cols]
    ct = EventColumns(*tt)
    assert ct.format == c.format and ct.t.ctypes.data == tt[0].data_ptr() and ct.p.ctypes.data == tt[3].data_ptr()
    assert EventColumns(*_columns(0, t, xy, p)).n == 0


def test_event_columns_refusals():
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    t, x, y, p = _columns(8)

    def refused(match, **kw):
        args = dict(t=t, x=x, y=y, p=p)
        args.update(kw)
        with pytest.raises(hip.EssHipError, match=match):
            EventColumns(**args)
    refused('1-D', t=t.reshape(2, 4))                       # 2-D columns
    refused('1-D', p=p.reshape(8, 1))
    refused('unequal lengths', x=x[:7].copy())              # unequal lengths
    refused('contiguous', y=np.zeros(16, np.int16)[::2])    # a non-contiguous column
    refused('float64 or int64', t=t.astype(np.float32))     # float32 t
    refused('both', y=y.astype(np.uint16))                  # mixed x / y dtypes
    refused('both', x=x.astype(np.int32), y=y.astype(np.int32))  # int32 x
    refused('int8, uint8 or bool', p=p.astype(np.int32))
    bad = p.copy()
    bad[3] = 2
    refused('polarity', p=bad)                              # uint8 polarity 2
    bad = (2 * p.astype(np.int8) - 1)
    bad[5] = -2
    refused('polarity', p=bad)                              # int8 polarity -2
    bad[5] = 2
    refused('polarity', p=bad)
    refused('1-D', t=list(t))                               # not an array at all
    EventColumns(t, x, y, p)                                # (the same call with nothing wrong)


@pytest.mark.parametrize('as_torch', [False, True])
def test_from_rows_agrees_with_pack_event_records(as_torch):
    """the awkward rows of test_pack_event_records_truncates_clamps_and_maps_polarity, field by field"""
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    ev = np.array([[0.5, -0.5, 3.9, 0], [0.75, -1.2, 40000.0, 1], [1.0, -9.0, 32767.9, -1], [1.25, 32768.0, -1.0, 1], [1.5, 0.99, 23.0, 0]])
    c = EventColumns.from_rows(torch.from_numpy(ev) if as_torch else ev)
    rec = packed(ev)
    assert c.n == 5 and c.format == 0
    assert (c.t.dtype, c.x.dtype, c.y.dtype, c.p.dtype) == (np.float64, np.int16, np.int16, np.int8)
    for k, col in (('t', c.t), ('x', c.x), ('y', c.y), ('p', c.p)):
        assert col.tolist() == rec[k].tolist(), k
    assert c.x.tolist() == [0, -1, -1, 32767, 0] and c.y.tolist() == [3, 32767, 32767, -1, 23] and c.p.tolist() == [-1, 1, -1, 1, -1]
    with pytest.raises(hip.EssHipError, match='polarity'):
        EventColumns.from_rows(np.array([[0.0, 1, 1, 1], [0.1, 1, 1, 0.5]]))
    with pytest.raises(hip.EssHipError, match=r'\[N, 4\]'):
        EventColumns.from_rows(np.zeros((3, 3)))
    assert EventColumns.from_rows(np.zeros((0, 4))).n == 0


# ---------------------------------------------------------------------------------------------- staging
def _views(n, fill=0x5A):
    raw = [np.full(n * size, fill, np.uint8) for size in (8, 2, 2, 1)]
    return raw, (raw[0].view(np.int64), raw[1].view(np.int16), raw[2].view(np.int16), raw[3])


@pytest.mark.parametrize('t', [np.float64, np.int64])
@pytest.mark.parametrize('xy', [np.int16, np.uint16])
@pytest.mark.parametrize('p', [np.uint8, np.int8, np.bool_])
def test_stage_event_columns_writes_the_columns_own_bits_and_nothing_behind_them(t, xy, p):
    from ess_amd.datasets.data_util import EventColumns, stage_event_columns
    cols = _columns(6, t, xy, p)
    if t == np.float64:
        cols[0][:] = [0.1, 0.25, float('nan'), 1e-300, 3.0, 1.6e15]
    else:
        cols[0][:] = [-5, 0, 1, 1_600_000_000_123_457, 1_600_000_000_123_458, (1 << 53) - 1]
    if xy == np.uint16:
        cols[1][:2] = [65535, 32768]
    raw, views = _views(10)
    assert stage_event_columns(EventColumns(*cols), *views) == 6
    for r, c, size in zip(raw, cols, (8, 2, 2, 1)):
        assert r[:6 * size].tobytes() == c.tobytes()        # its own bits: no cast on the way
        assert bool((r[6 * size:] == 0x5A).all())           # nothing behind n
    raw, views = _views(10)
    assert stage_event_columns(EventColumns(*_columns(0, t, xy, p)), *views) == 0
    assert all(bool((r == 0x5A).all()) for r in raw)


def test_stage_event_columns_refuses_an_overflow_before_writing():
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns, stage_event_columns
    c = EventColumns(*_columns(11, np.int64, np.uint16, np.uint8))
    raw, views = _views(10)
    with pytest.raises(hip.EssHipError, match=r'\b11 events\b.*\b10 entries\b'):
        stage_event_columns(c, *views)
    # one view shorter than the others: the shortest decides, still before anything is written
    with pytest.raises(hip.EssHipError, match=r'\b11 events\b.*\b4 entries\b'):
        stage_event_columns(c, views[0], views[1], views[2], np.full(16, 0x5A, np.uint8)[:4])
    assert all(bool((r == 0x5A).all()) for r in raw)
    with pytest.raises(hip.EssHipError, match='8-byte'):
        stage_event_columns(c, np.zeros(16, np.int32), *_views(16)[1][1:])
    with pytest.raises(hip.EssHipError, match='EventColumns'):
        stage_event_columns(np.zeros((3, 4)), *_views(16)[1])


# ---------------------------------------------------------------------------------------------- ABI
def test_the_column_entry_point_is_exported_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, 'ess_event_ingest_columns') and 'ess_event_ingest_columns' in hip.EXPORTS
    assert hip.lib().ess_version() == 110
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    assert 'int ess_event_ingest_columns(' in header
    assert 'ESS_EVCOL_T_I64 = 1' in header and 'ESS_EVCOL_XY_U16 = 2' in header
    assert [hip.event_column_stride(n) for n in (1, 16, 17, 1003, 4096, 100000)] == [16, 16, 32, 1008, 4096, 100000]
    # argument checks come in front of any launch: no device is needed to be refused
    L, P = hip.lib(), ctypes.c_void_p
    a = P(4096)
    assert L.ess_event_ingest_columns(a, a, a, a, a, P(0), 16, 1, 5, 24, 40, a, 5 * 24 * 40 * 8, a, P(0)) == -22 and b'null' in L.ess_last_error()
    for stride in (0, 1003, (1 << 22) + 16):
        assert L.ess_event_ingest_columns(a, a, a, a, a, a, stride, 1, 5, 24, 40, a, 5 * 24 * 40 * 8, a, P(0)) == -22
        assert b'stride' in L.ess_last_error(), stride
    assert L.ess_event_ingest_columns(a, a, P(4098), a, a, a, 16, 1, 5, 24, 40, a, 5 * 24 * 40 * 8, a, P(0)) == -22
    assert b'16-byte aligned' in L.ess_last_error()
    assert L.ess_event_ingest_columns(a, a, a, a, a, a, 16, 1, 5, 24, 40, a, 5 * 24 * 40 * 8 - 8, a, P(0)) == -22 and b'acc has' in L.ess_last_error()


# ---------------------------------------------------------------------------------------------- the constructor argument
def test_segmenter_refuses_a_bad_event_layout():
    from ess_amd import hip
    from ess_amd.run_segmentation import _event_layout
    assert _event_layout('records', None) == 'records' and _event_layout('records', 4096) == 'records'
    assert _event_layout('columns', 4096) == 'columns'
    with pytest.raises(hip.EssHipError, match='event_capacity'):
        _event_layout('columns', None)
    for bad in ('rows', 'Columns', None, 1, b'columns'):
        with pytest.raises(hip.EssHipError, match='event_layout'):
            _event_layout(bad, 4096)


def test_segmenter_refuses_rows_where_columns_are_expected():
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.run_segmentation import check_stream_columns
    c = EventColumns(*_columns(5))
    empty = EventColumns(*_columns(0))
    assert check_stream_columns([c, None, empty], 3) == ([c, None, None], [True, False, False])
    with pytest.raises(hip.EssHipError, match='from_rows'):
        check_stream_columns([c, np.zeros((5, 4)), None], 3)
    with pytest.raises(hip.EssHipError, match='one entry per stream'):
        check_stream_columns([c], 3)
