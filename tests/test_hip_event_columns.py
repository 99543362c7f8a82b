"""GPU tier: the event ingest from raw event columns -- hip.event_ingest_columns (t / x / y / p as a camera delivers them, a format
word per stream read on the device) and MultiStreamSegmenter(event_layout='columns').  What is asserted throughout is BITS: a grid
equals the numpy restatement of tests/test_host_event_ingest.py on the float64 rows EQUAL to the columns' values, i.e. what the
record path gives on the same events; a 'columns' segmenter's labels, colours and confidences equal a 'records' segmenter's."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers, events, result rows, the pins)
from tests import test_hip_stream_compaction as SC  # noqa: E402  (the 64 x 96 models)
from tests import test_host_event_ingest as R  # noqa: E402  (the restatement)

DEV = M.DEV
GUARD, NAN16 = M.GUARD, M.NAN16
NB, H, W, CAP = 5, 24, 40, 4096
XY_DTYPES = (np.int16, np.uint16)  # by format bit 1
T0_US = 1_600_000_000_000_000  # int64 microseconds with a GPS-like offset: below 2^53, far above 2^32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _as_columns(ev, fmt, p_dtype=np.uint8):
    """[n, 4] float64 rows (t in seconds, integral in-int16 coordinates, polarity 0 / 1) -> EventColumns in the dtypes of format
    word fmt; an int64 time is T0_US + microseconds"""
    from ess_amd.datasets.data_util import EventColumns
    t = ev[:, 0].copy() if not fmt & 1 else T0_US + np.round(ev[:, 0] * 1e6).astype(np.int64)
    xy = XY_DTYPES[fmt >> 1 & 1]
    pol = ev[:, 3].astype(np.int64)
    p = (2 * pol - 1).astype(np.int8) if p_dtype == np.int8 else pol.astype(p_dtype)
    return EventColumns(t, ev[:, 1].astype(xy), ev[:, 2].astype(xy), p)


def _rows(c):
    """the float64 rows equal to the columns' values (polarity: 1 where the byte equals 1, else 0)"""
    return np.stack([c.t.astype(np.float64), c.x.astype(np.float64), c.y.astype(np.float64), (c.p.view(np.uint8) == 1).astype(np.float64)], 1)


def _want(c, nb=NB, h=H, w=W):
    return R.restate(R.packed(_rows(c)), nb, h, w)


def _expected(c, nb=NB, h=H, w=W):
    return torch.from_numpy(_want(c, nb, h, w)).to(DEV)


def _device_columns(cols, capacity):
    """cols: per stream an EventColumns (<= capacity events) -> (t int64, x int16, y int16, p uint8) [S, stride] on the device, raw
    words.  The entries behind a stream's own are filled with an event that WOULD land in the grid (a time from the middle of the
    stream's window, pixel (1, 1), positive): a kernel that walked past the count would show."""
    from ess_amd import hip
    from ess_amd.datasets.data_util import stage_event_columns
    S, stride = len(cols), hip.event_column_stride(capacity)
    host = [np.zeros((S, stride), d) for d in (np.int64, np.int16, np.int16, np.uint8)]
    for s, c in enumerate(cols):
        k = (c.n - 1) // 2
        fill = c.t[k:k + 1] if c.n else np.array([0.05])
        host[0][s] = fill.view(np.int64)[0]
        host[1][s], host[2][s], host[3][s] = 1, 1, 1
        assert stage_event_columns(c, *(a[s] for a in host)) == c.n
    return tuple(torch.from_numpy(a).to(DEV) for a in host)


def _words(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _run_guarded(cols, counts, capacity, formats=None, nb=NB, h=H, w=W):
    """-> (out inside its NaN-pre-filled guarded buffer, the buffer, acc)"""
    from ess_amd import hip
    S = len(cols)
    buf, out = M._guarded((S, nb, h, w), torch.float32)
    acc = torch.zeros(S * nb * h * w, dtype=torch.int64, device=DEV)
    fmts = [c.format for c in cols] if formats is None else formats
    got = hip.event_ingest_columns(*_device_columns(cols, capacity), _words(counts), _words(fmts), out, acc=acc)
    assert got is out
    return out, buf, acc


def _guards_intact(buf, out):
    n = out.numel() * 2
    return bool((buf[:GUARD // 2] == NAN16).all()) and bool((buf[GUARD // 2 + n:] == NAN16).all())


# ---------------------------------------------------------------------------------------------- 1. the kernel
def test_four_formats_in_one_call_bit_equal_to_the_record_restatement():
    """S = 4, a different format word per stream (f64 + i16, i64 + i16, f64 + u16, i64 + u16), counts [3000, 1, 0, 4096] at capacity
    4096: bit-equal per stream, the empty stream all zero, guards intact, acc all zero behind the call, a second call the same bits"""
    from ess_amd import hip
    counts = [3000, 1, 0, CAP]
    cols = [_as_columns(R.events(n, H, W, 20 + s), s) for s, n in enumerate(counts)]
    assert [c.format for c in cols] == [0, hip.EVCOL_T_I64, hip.EVCOL_XY_U16, hip.EVCOL_T_I64 | hip.EVCOL_XY_U16]
    assert cols[3].t.dtype == np.int64 and int(cols[3].t.min()) >= T0_US and int(cols[3].t.max()) < 1 << 53
    out, buf, acc = _run_guarded(cols, counts, CAP)
    for s in range(4):
        assert torch.equal(_bits(out[s]), _bits(_expected(cols[s]))), f'stream {s} ({counts[s]} events, format {cols[s].format})'
    assert bool(out[0].any()) and bool(out[1].any()) and bool(out[3].any()) and not bool(_bits(out[2]).any())
    assert _guards_intact(buf, out)
    assert not bool(acc.any())
    first = out.clone()
    buf.fill_(NAN16)
    hip.event_ingest_columns(*_device_columns(cols, CAP), _words(counts), _words([c.format for c in cols]), out, acc=acc)
    assert torch.equal(_bits(out), _bits(first)) and not bool(acc.any()) and _guards_intact(buf, out)
    # acc=None: allocated and zeroed by the call
    got = hip.event_ingest_columns(*_device_columns(cols, CAP), _words(counts), _words([c.format for c in cols]), torch.empty_like(first))
    assert torch.equal(_bits(got), _bits(first))


TAILS = [1, 2, 3, 5, 7, 255, 257, 1025]


@pytest.mark.parametrize('i', range(len(TAILS)), ids=[f'n{n}' for n in TAILS])
def test_tail_counts(i):
    """a lane takes 4 consecutive events, a block 256 lanes: the partial lane, the partial wave and the partial block, each alone,
    the formats taking turns"""
    n = TAILS[i]
    c = _as_columns(R.events(n, H, W, 80 + i), i % 4)
    out, buf, acc = _run_guarded([c], [n], 2048)
    assert torch.equal(_bits(out[0]), _bits(_expected(c))) and bool(out[0].any()), n
    assert _guards_intact(buf, out) and not bool(acc.any())


def test_a_capacity_that_is_no_multiple_of_the_alignment():
    """capacity 1003 -> stride 1008, the count equals the capacity: every row of every column stays 16-byte aligned (stream 1's rows
    start at 1008 entries), and the five landing events between the count and the stride are not summed"""
    from ess_amd import hip
    assert hip.event_column_stride(1003) == 1008
    cols = [_as_columns(R.events(1003, H, W, 90 + s), 3 - s) for s in range(2)]
    dev = _device_columns(cols, 1003)
    assert all(tuple(d.shape) == (2, 1008) for d in dev)
    out, buf, acc = _run_guarded(cols, [1003, 1003], 1003)
    for s in range(2):
        assert torch.equal(_bits(out[s]), _bits(_expected(cols[s]))), s
    assert _guards_intact(buf, out) and not bool(acc.any())


def _edge_columns():
    """the edge rows of tests/test_hip_event_ingest.py, as columns -> name: (EventColumns, capacity)"""
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(9)
    n = 64
    base = R.events(n, H, W, 31)
    same_t = base.copy()
    same_t[:, 0] = 0.125
    nan_t = base.copy()
    nan_t[n // 2, 0] = float('nan')
    nan_first = base.copy()
    nan_first[0, 0] = float('nan')
    at_last = base.copy()
    at_last[-5:, 0] = at_last[-1, 0]
    unsorted = base.copy()
    unsorted[1:-1] = unsorted[1:-1][g.permutation(n - 2)]
    unsorted[3, 0] = -1.0  # (before the first timestamp: ts < 0, dropped)
    unsorted[4, 0] = 9.0   # (behind the last: ts >= nb, dropped)
    # int64 times that start NEGATIVE: first = -500, last = 1000, and events before the first and behind the last
    neg = _as_columns(base, 1)
    neg_t = np.sort(g.integers(-500, 1001, n)).astype(np.int64)
    neg_t[0], neg_t[-1], neg_t[3], neg_t[4], neg_t[5] = -500, 1000, -2000, 5000, -(1 << 40)
    neg = EventColumns(neg_t, neg.x, neg.y, neg.p)

    def coords(vals_x, vals_y, xy):
        k = len(vals_x) + len(vals_y)
        ev = _as_columns(R.events(k, H, W, 32), 0)
        x = np.array(list(vals_x) + [3] * len(vals_y)).astype(xy)
        y = np.array([2] * len(vals_x) + list(vals_y)).astype(xy)
        assert x.tolist() == list(vals_x) + [3] * len(vals_y)  # (every value fits the dtype: none wrapped on the host)
        return EventColumns(ev.t, x, y, ev.p)
    return {'same_timestamp_f64': (_as_columns(same_t, 0), 128), 'same_timestamp_i64': (_as_columns(same_t, 3), 128),
            'one_event_wide': (_as_columns(base[:1], 1), 2048),
            'one_pixel_mixed_polarity': (_as_columns(R.one_pixel_events(2000, 33), 3), 2048),
            'coordinates_i16': (coords([-1, 0, W - 1, W, 32767, -32768], [-1, 0, H - 1, H, 32767], np.int16), 16),
            'coordinates_u16': (coords([0, W - 1, W, 32768, 65535], [0, H - 1, H, 32768, 65535], np.uint16), 16),
            'nan_timestamp': (_as_columns(nan_t, 0), 64), 'nan_first_timestamp': (_as_columns(nan_first, 2), 64),
            'at_last_timestamp_f64': (_as_columns(at_last, 2), 100), 'at_last_timestamp_i64': (_as_columns(at_last, 1), 100),
            'outside_the_time_range_f64': (_as_columns(unsorted, 0), 64), 'outside_the_time_range_i64': (_as_columns(unsorted, 3), 64),
            'negative_i64_times': (neg, 64)}


@pytest.mark.parametrize('name', sorted(_edge_columns()))
def test_edge_columns(name):
    c, capacity = _edge_columns()[name]
    want = _want(c)
    if name.startswith('same_timestamp'):  # dT = 0 -> 1: every event whole in bin 0
        assert want[0].any() and not want[1:].any()
    if name == 'coordinates_i16':  # only the in-range pixels land: x in {0, W - 1} on row 2, y in {0, H - 1} on column 3
        assert 0 < np.count_nonzero(np.abs(want).sum(0)) <= 4
    if name == 'coordinates_u16':  # 32768 and 65535 enter as their unsigned values and lie outside the grid: dropped
        assert 0 < np.count_nonzero(np.abs(want).sum(0)) <= 4
    if name == 'nan_first_timestamp':
        assert not want.any()
    if name.startswith('at_last_timestamp'):
        assert want[NB - 1].any()
    if name == 'one_pixel_mixed_polarity':
        assert np.count_nonzero(want.sum(0)) == 1
    if name == 'negative_i64_times':
        assert int(c.t[0]) == -500 and want.any()
    out, buf, acc = _run_guarded([c], [c.n], capacity)
    assert torch.equal(_bits(out[0]), _bits(torch.from_numpy(want).to(DEV))), name
    assert _guards_intact(buf, out) and not bool(acc.any())


def test_polarity_as_bool_uint8_and_int8_gives_the_same_grid():
    ev = R.events(1500, H, W, 34)
    grids = []
    for p_dtype in (np.bool_, np.uint8, np.int8):
        c = _as_columns(ev, 3, p_dtype)
        assert c.p.dtype == p_dtype
        out, _, _ = _run_guarded([c], [c.n], 2048)
        assert torch.equal(_bits(out[0]), _bits(_expected(c))), p_dtype
        grids.append(out[0].clone())
    assert torch.equal(_bits(grids[0]), _bits(grids[1])) and torch.equal(_bits(grids[1]), _bits(grids[2]))
    assert bool((grids[0] > 0).any()) and bool((grids[0] < 0).any())


def test_a_grid_that_is_no_multiple_of_four():
    """3 x 5 x 7 voxels per stream: the streams' rows of acc / out are not 16-byte aligned, the finish pass takes its scalar form"""
    nb, h, w = 3, 5, 7
    counts = [500, 0, 37]
    cols = [_as_columns(R.events(n, h, w, 40 + s), s + 1) for s, n in enumerate(counts)]
    out, buf, acc = _run_guarded(cols, counts, 512, nb=nb, h=h, w=w)
    for s in range(3):
        assert torch.equal(_bits(out[s]), _bits(_expected(cols[s], nb, h, w))), s
    assert _guards_intact(buf, out) and not bool(acc.any())


def test_the_grid_does_not_depend_on_the_event_order():
    """events 1 .. n - 2 permuted (the first and the last, which set the time scale, in place): bit-identical grids"""
    from ess_amd.datasets.data_util import EventColumns
    ev = R.one_pixel_events(2000, 51)
    ev[700:1400] = R.events(700, H, W, 52)  # (one crowded pixel, where the order of a float sum would matter, and a spread)
    ev[700:1400, 0] = np.linspace(ev[0, 0], ev[-1, 0], 700)
    c = _as_columns(ev, 3)
    g = np.random.default_rng(53)
    out0, _, _ = _run_guarded([c], [c.n], 2048)
    for _ in range(3):
        order = np.concatenate([[0], 1 + g.permutation(c.n - 2), [c.n - 1]])
        perm = EventColumns(*(np.ascontiguousarray(a[order]) for a in (c.t, c.x, c.y, c.p)))
        out1, _, _ = _run_guarded([perm], [c.n], 2048)
        assert torch.equal(_bits(out0), _bits(out1))
    assert torch.equal(_bits(out0[0]), _bits(_expected(c)))


def _head(c, n):
    from ess_amd.datasets.data_util import EventColumns
    return EventColumns(*(a[:n] for a in (c.t, c.x, c.y, c.p)))


def test_ingest_keep_leaves_the_grid_alone():
    from ess_amd import hip
    counts = [3000, hip.INGEST_KEEP, 0, 2000, -7]
    cols = [_as_columns(R.events(3000, H, W, 60 + s), s % 4) for s in range(5)]
    out, buf, acc = _run_guarded(cols, counts, CAP)
    assert _guards_intact(buf, out)
    for s in (1, 4):  # (the NaN pre-fill, every bit of it)
        assert bool((out[s].view(torch.int16) == NAN16).all()), s
    assert torch.equal(_bits(out[0]), _bits(_expected(cols[0]))) and not bool(_bits(out[2]).any())
    assert torch.equal(_bits(out[3]), _bits(_expected(_head(cols[3], 2000))))
    assert not bool(acc.any())


def test_an_unknown_format_bit_gives_an_all_zero_grid():
    """a format word with any bit beyond the two known ones: the stream is treated as count 0 -- its columns, full of events that
    land when read in the stream's true format, are not summed; its neighbours are untouched by it.  With INGEST_KEEP the count still
    decides: the grid stays."""
    from ess_amd import hip
    cols = [_as_columns(R.events(CAP, H, W, 100 + s), s % 4) for s in range(5)]
    counts = [CAP, CAP, 3000, CAP, hip.INGEST_KEEP]
    formats = [cols[0].format, cols[1].format | 4, cols[2].format | (1 << 30), -1, 8]
    out, buf, acc = _run_guarded(cols, counts, CAP, formats=formats)
    assert torch.equal(_bits(out[0]), _bits(_expected(cols[0]))) and bool(out[0].any())
    for s in (1, 2, 3):
        assert not bool(_bits(out[s]).any()), s
    assert bool((out[4].view(torch.int16) == NAN16).all())
    assert _guards_intact(buf, out) and not bool(acc.any())


def test_a_stream_batched_equals_the_stream_alone():
    counts = [3000, 1, 0, CAP]
    cols = [_as_columns(R.events(n, H, W, 70 + s), 3 - s) for s, n in enumerate(counts)]
    out, _, _ = _run_guarded(cols, counts, CAP)
    for s in range(4):
        alone, _, _ = _run_guarded([cols[s]], [counts[s]], CAP)
        assert torch.equal(_bits(out[s]), _bits(alone[0])), s


def test_event_ingest_columns_argument_errors():
    """ESS_EINVAL with a message, in front of any launch; the binding's refusals"""
    import ctypes
    from ess_amd import hip
    EINVAL = -22
    L = hip.lib()
    c = _as_columns(R.events(10, H, W, 1), 3)
    t, x, y, p = _device_columns([c], 16)
    cnt, fmt = _words([10]), _words([c.format])
    out = torch.zeros(1, NB, H, W, device=DEV)
    acc = torch.zeros(NB * H * W, dtype=torch.int64, device=DEV)
    P = ctypes.c_void_p

    def call(stride=16, acc_bytes=None, out_ptr=None, p_ptr=None, fmt_ptr=None):
        return L.ess_event_ingest_columns(P(t.data_ptr()), P(x.data_ptr()), P(y.data_ptr()), P(p.data_ptr() if p_ptr is None else p_ptr),
                                          P(cnt.data_ptr()), P(fmt.data_ptr() if fmt_ptr is None else fmt_ptr), stride, 1, NB, H, W,
                                          P(acc.data_ptr()), acc.numel() * 8 if acc_bytes is None else acc_bytes,
                                          P(out.data_ptr() if out_ptr is None else out_ptr), hip.stream())
    assert call(stride=(1 << 22) + 16) == EINVAL and b'stride' in L.ess_last_error()
    assert call(stride=0) == EINVAL and b'stride' in L.ess_last_error()
    assert call(stride=10) == EINVAL and b'multiple of 16' in L.ess_last_error()  # (a stride that misaligns the rows)
    assert call(acc_bytes=NB * H * W * 8 - 8) == EINVAL and b'acc has' in L.ess_last_error()
    assert call(out_ptr=out.data_ptr() + 4) == EINVAL and b'16-byte aligned' in L.ess_last_error()
    assert call(p_ptr=p.data_ptr() + 1) == EINVAL and b'16-byte aligned' in L.ess_last_error()
    assert call(fmt_ptr=0) == EINVAL and b'null' in L.ess_last_error()
    # ... and through the binding
    ok = dict(t=t, x=x, y=y, p=p, counts=cnt, formats=fmt, out=out, acc=acc)

    def refused(match, **kw):
        with pytest.raises(hip.EssHipError, match=match):
            hip.event_ingest_columns(**{**ok, **kw})
    refused('acc has', acc=acc[:-1])
    refused('t must be', t=t.to(torch.int32))
    refused('x must be', x=x.to(torch.int32))
    refused('y must be', y=y[:, :8].contiguous())
    refused('p must be', p=p.to(torch.int16))
    refused('counts must be int32', counts=_words([1, 2]))
    refused('counts must be int32', counts=cnt.to(torch.int64))
    refused(r'formats must be int32 \[1\]', formats=_words([0, 0]))
    refused(r'formats must be int32 \[1\]', formats=fmt.view(1, 1))
    refused('no CPU path', t=t.cpu())
    refused('no CPU path', formats=fmt.cpu())
    refused('contiguous', x=torch.zeros(1, 32, dtype=torch.int16, device=DEV)[:, ::2])
    refused('multiple of 16', **{k: ok[k][:, :10].contiguous() for k in ('t', 'x', 'y', 'p')})
    assert not bool(out.any()) and not bool(acc.any())
    assert call() == 0  # (the same call with nothing wrong)
    assert torch.equal(_bits(out[0]), _bits(_expected(c)))


# ---------------------------------------------------------------------------------------------- 2. the segmenter
SH_, SW_, SEG_CAP = SC.H, SC.W, 2048
SEG_CASES = [(S, mode, graph) for S in (1, 3) for mode in ('mixed', 'bf16') for graph in (False, True)]
SEG_IDS = [f'S{S}-{mode}-{"graph" if graph else "eager"}' for S, mode, graph in SEG_CASES]


@functools.lru_cache(maxsize=None)
def _window(S, w, exact=None):
    """the events of round w, one EventColumns per stream, built once: the sizes differ per stream (stream `exact`: exactly SEG_CAP
    events), and stream s delivers format (s + w) % 4 -- its t and coordinate dtypes change from round to round"""
    return tuple(_as_columns(M._events(SEG_CAP if s == exact else 700 + 300 * ((s + w) % 3), SH_, SW_, 700 + 10 * w + s), (s + w) % 4)
                 for s in range(S))


def _assert_rows(a, b, active, what):
    assert a.valid == b.valid == tuple(active), what
    for s, on in enumerate(active):
        if on:
            assert M._same(M._row(a, s), M._row(b, s)), f'{what}: stream {s}'


def _feed(col_seg, rec_seg, cols, what):
    """one round of the same events into a 'columns' and a 'records' segmenter -> the active rows agree bit for bit"""
    active = [c is not None and c.n > 0 for c in cols]
    got = col_seg.update_from_events(list(cols))
    want = rec_seg.update_from_events([None if c is None else _rows(c) for c in cols])
    _assert_rows(got, want, active, what)
    return got


@pytest.mark.parametrize('S,mode,graph', SEG_CASES, ids=SEG_IDS)
def test_rounds_from_columns_equal_rounds_from_records(S, mode, graph):
    """4 rounds (a fifth by update(grids)) of the same events into event_layout='columns' and 'records': labels, colours, confidence
    bits of the active rows.  The rounds hold a window of exactly event_capacity events, an idle stream, an empty window, a restart
    through reset([s]); every stream changes its t and coordinate formats from round to round, and ONE capture serves them all."""
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    hip.set_compute(mode)
    try:
        seg = SC._segmenter('convlstm', S, graph=graph, event_capacity=SEG_CAP, event_layout='columns')
        ref = SC._segmenter('convlstm', S, graph=graph, event_capacity=SEG_CAP)
        stride = hip.event_column_stride(SEG_CAP)
        assert seg.event_layout == 'columns' and ref.event_layout == 'records'
        assert seg._records is None and ref._columns is None and ref._formats is None
        assert [(c.dtype, tuple(c.shape)) for c in seg._columns] == [(torch.int64, (S, stride)), (torch.int16, (S, stride)),
                                                                     (torch.int16, (S, stride)), (torch.uint8, (S, stride))]
        assert tuple(seg._counts.shape) == tuple(seg._formats.shape) == (S,) and seg._counts.dtype == seg._formats.dtype == torch.int32
        assert seg._acc.dtype == torch.int64 and tuple(seg._acc.shape) == (S, SC.C, SH_, SW_) and len(seg._stage) == 2
        assert all(t.is_pinned() for st in seg._stage for t in st.cols + (st.words,))
        what = f'{mode} S={S} graph={graph}'
        formats = []

        def feed(w, cols):
            formats.append(tuple(c.format if c is not None and c.n else None for c in cols))
            _feed(seg, ref, cols, f'{what} round {w}')
        feed(0, _window(S, 0, exact=0))                                             # stream 0: exactly event_capacity events
        feed(1, [None if s == S - 1 else c for s, c in enumerate(_window(S, 1))])   # an idle stream
        seg.reset([0])
        ref.reset([0])
        empty = EventColumns(np.zeros(0, np.int64), np.zeros(0, np.uint16), np.zeros(0, np.uint16), np.zeros(0, np.uint8))
        feed(2, [empty] + list(_window(S, 2)[1:]))                                  # an empty window: the restart stays pending
        feed(3, _window(S, 3))                                                      # ... and is served here
        # the formats did change under the one capture: S = 3 staged all four words (stream 0: three of them), S = 1 two
        assert len({f for fs in formats for f in fs if f is not None}) == (4 if S == 3 else 2)
        assert len({fs[0] for fs in formats if fs[0] is not None}) == (3 if S == 3 else 2)
        # update(grids) through the same graph: count words INGEST_KEEP
        grids = torch.from_numpy(np.stack([_want(c, SC.C, SH_, SW_) for c in _window(S, 4)])).to(DEV)
        _assert_rows(seg.update(grids), ref.update(grids), [True] * S, f'{what} update(grids)')
        assert not bool(seg._acc.any())
        assert seg.n_captures == ref.n_captures == (1 if graph else 0) and seg.n_windows == ref.n_windows == 5
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('mode,graph', [(m, g) for m in ('mixed', 'bf16') for g in (False, True)],
                         ids=[f'{m}-{"graph" if g else "eager"}' for m in ('mixed', 'bf16') for g in (False, True)])
def test_compacted_column_rounds_equal_the_uncompacted(mode, graph):
    """S = 3, compact=True with buckets [1, 2]: the rows equal the uncompacted 'columns' segmenter's bit for bit (both
    batch-size-dependent dispatch choices pinned, as in tests/test_hip_stream_compaction.py); the compact input holds the active
    streams' grids in slot order, a padded slot's is all zero; one capture per bucket and one for the ride-along round at the most"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    S = 3
    hip.set_compute(mode)
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        ride = SC._segmenter('convlstm', S, graph=graph, event_capacity=SEG_CAP, event_layout='columns')
        comp = SC._segmenter('convlstm', S, graph=graph, event_capacity=SEG_CAP, event_layout='columns', compact=True, compact_buckets=[1, 2])
        assert comp.buckets == (1, 2)
        # active counts: 3 (the ride-along round), 1, 2 with a restart, 0 (the smallest bucket, its slot padded), 1 in slot 0 from stream 1
        idles = [(), (1, 2), (1,), (0, 1, 2), (0, 2)]
        for w, idle in enumerate(idles):
            cols = [None if s in idle else c for s, c in enumerate(_window(S, w))]
            active = [c is not None for c in cols]
            if w == 2:
                comp.reset([2])
                ride.reset([2])
            got, want = comp.update_from_events(cols), ride.update_from_events(cols)
            _assert_rows(got, want, active, f'{mode} graph={graph} round {w}')
            A = sum(active)
            b = next((b for b in comp.buckets if b >= A), None)
            if b is not None:
                for slot, c in enumerate(c for c in cols if c is not None):
                    assert torch.equal(_bits(comp.compact_input[slot]), _bits(_expected(c, SC.C, SH_, SW_))), (w, slot, 'compact input')
                for slot in range(A, b):
                    assert not bool(_bits(comp.compact_input[slot]).any()), (w, slot, 'a padded slot is not all zero')
        assert comp.n_captures <= (len(comp.buckets) + 1 if graph else 0) and ride.n_captures == (1 if graph else 0)
        assert not bool(comp._acc.any())
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')


def test_column_rounds_refuse_an_oversized_window_and_rows():
    """a window of event_capacity + 1 events: refused before anything is written -- both staging sets, the device columns and words,
    the round counter and the pending restarts are as before, and the next valid round gives the right rows; an [N, 4] array is
    refused with a pointer to EventColumns.from_rows; event_layout needs event_capacity"""
    from ess_amd import hip
    S = 3
    hip.set_compute('bf16')
    try:
        seg = SC._segmenter('convlstm', S, graph=True, event_capacity=SEG_CAP, event_layout='columns')
        ref = SC._segmenter('convlstm', S, graph=True, event_capacity=SEG_CAP)
        _feed(seg, ref, _window(S, 0), 'round 0')
        _feed(seg, ref, _window(S, 1), 'round 1')
        seg.reset([1])
        ref.reset([1])

        def snapshot():
            torch.cuda.synchronize()
            return ([t.clone() for st in seg._stage for t in st.cols + (st.words,)] + [t.clone() for t in seg._columns + (seg._words,)],
                    seg._stage_next, seg.n_windows, list(seg._pending))
        before = snapshot()
        big = list(_window(S, 2))
        big[S - 1] = _as_columns(M._events(SEG_CAP + 1, SH_, SW_, 99), 3)
        with pytest.raises(hip.EssHipError, match=f'{SEG_CAP + 1} events.*event_capacity={SEG_CAP}'):
            seg.update_from_events(big)
        rows = list(_window(S, 2))
        rows[0] = _rows(rows[0])
        with pytest.raises(hip.EssHipError, match='from_rows'):
            seg.update_from_events(rows)
        after = snapshot()
        assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])) and before[1:] == after[1:]
        _feed(seg, ref, _window(S, 2), 'the round after the refusals')
        assert seg.n_captures == 1 and seg.n_windows == 3
        with pytest.raises(hip.EssHipError, match='event_capacity'):
            SC._segmenter('convlstm', S, event_layout='columns')
        with pytest.raises(hip.EssHipError, match='event_layout'):
            SC._segmenter('convlstm', S, event_capacity=SEG_CAP, event_layout='rows')
    finally:
        hip.set_compute('fp32')
