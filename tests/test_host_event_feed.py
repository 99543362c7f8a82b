"""CPU tier of the continuous event feed (hip.event_ingest_ring, MultiStreamSegmenter(event_layout='ring')): the C entry point and the
ABI, the window cutter datasets.event_feed.EventWindows against a brute-force cut of the concatenated stream, the copy of a packet
into a ring that wraps, and the refusals of the binding that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_host_event_ingest import ROOT, built_lib  # noqa: F401  (built_lib: the fixture)

PACKETS = (7, 13, 1, 40, 3)
T0_US = 1_600_000_000_000_000


# ---------------------------------------------------------------------------------------------- ABI
def test_the_ring_entry_point_is_exported_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, 'ess_event_ingest_ring') and 'ess_event_ingest_ring' in hip.EXPORTS
    assert hip.lib().ess_version() == 110
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    assert 'int ess_event_ingest_ring(' in header and 'PURELY ADDITIVE to ABI 110' in header
    # argument checks come in front of any launch: no device is needed to be refused
    L, P = hip.lib(), ctypes.c_void_p
    a = P(4096)
    need = 5 * 24 * 40 * 8

    def call(t=a, p=a, rows=a, starts=a, counts=a, formats=a, ring=16, n_rows=1, n_slots=1, acc=a, acc_bytes=need, out=a):
        return L.ess_event_ingest_ring(t, a, a, p, rows, starts, counts, formats, ring, n_rows, n_slots, 5, 24, 40, acc, acc_bytes, out, P(0))
    for null in ('t', 'p', 'rows', 'starts', 'counts', 'formats', 'acc', 'out'):
        assert call(**{null: P(0)}) == -22 and b'null' in L.ess_last_error(), null
    for ring in (0, -16, 8, 1003, 24, (1 << 22) + 16):
        assert call(ring=ring) == -22 and b'ring=' in L.ess_last_error(), ring
    assert call(ring=24) == -22 and b'multiple of 16' in L.ess_last_error()
    assert call(p=P(4097)) == -22 and b'16-byte aligned' in L.ess_last_error()
    assert call(out=P(4100)) == -22 and b'16-byte aligned' in L.ess_last_error()
    assert call(acc_bytes=need - 8) == -22 and b'acc has' in L.ess_last_error()
    assert call(n_slots=2) == -22 and b'acc has' in L.ess_last_error()  # (acc is sized by the slots, not by the rows)
    assert call(n_slots=0) == -22 and b'n_slots' in L.ess_last_error()
    assert call(n_rows=0) == -22 and b'n_rows' in L.ess_last_error()


# ---------------------------------------------------------------------------------------------- EventWindows, count mode
def _drain(w):
    out = []
    while w.pending:
        out.append(w.pop())
    return out


@pytest.mark.parametrize('M', [16, 8, 1])
def test_count_windows_from_packets_that_straddle_them(M):
    """N = 16, packets of 7, 13, 1, 40, 3 events (64 in all): window k is [k M, k M + 16), pending exactly when its last event is fed"""
    from ess_amd.datasets.event_feed import EventWindows
    N = 16
    w = EventWindows(window_events=N, stride=M)
    t = np.arange(64, dtype=np.float64)
    fed, got = 0, []
    for n in PACKETS:
        before = w.pending
        now = w.push(n, t[fed:fed + n])
        fed += n
        complete = 0 if fed < N else (fed - N) // M + 1
        assert now == w.pending == complete - len(got) and now >= before
        assert w.head == fed
        if n == 13:  # (20 events fed: leave the windows pending over the next packet)
            continue
        got += _drain(w)
        assert w.oldest_needed() == len(got) * M
    assert got == [(k * M, N) for k in range((64 - N) // M + 1)]
    assert len(got) == {16: 4, 8: 7, 1: 49}[M]
    with pytest.raises(Exception, match='no window'):
        w.pop()


def test_count_windows_default_stride_and_arguments():
    from ess_amd import hip
    from ess_amd.datasets.event_feed import EventWindows
    w = EventWindows(window_events=5)
    assert w.stride == 5 and w.push(11, np.zeros(11)) == 2 and _drain(w) == [(0, 5), (5, 5)]
    assert w.push(0, np.zeros(0)) == 0
    for kw in (dict(), dict(window_events=4, window_duration=1.0), dict(window_events=0), dict(window_events=4, stride=0),
               dict(window_events=4.5), dict(window_events=4, stride=1.5), dict(window_duration=-1.0), dict(window_duration=float('nan')),
               dict(window_events=True), dict(window_events=17, event_capacity=16)):
        with pytest.raises(hip.EssHipError):
            EventWindows(**kw)


# ---------------------------------------------------------------------------------------------- EventWindows, duration mode
def _brute(t, D, E):
    """the windows of the WHOLE stream t, straight from the definition: window k holds the events with T0 + k E <= t < T0 + k E + D
    and exists once some event has t >= T0 + k E + D -> [(index of its first event -- of the first event at or behind its lower
    bound, where it is empty --, count)]"""
    t0 = t[0].item()
    out, k = [], 0
    while True:
        lo = t0 + k * E
        hi = lo + D
        if not bool((t >= hi).any()):
            return out
        inside = (t >= lo) & (t < hi)
        out.append((int(np.argmax(t >= lo)), int(inside.sum())))
        k += 1


def _times(dtype):
    """64 times with what the cutter can get wrong: an event EXACTLY on a window bound (belongs to the later window), a pause longer
    than a window (an empty window), and a last packet that spans three windows"""
    gaps = np.array([3, 4, 3] * 7)[:20].tolist()                 # events 0..20: 0, 3, 7, 10, ... (10, 20, 30: exactly on bounds of D = 10)
    t = np.concatenate([[0], np.cumsum(gaps)])                   # 21 events, the last at 67
    t = np.concatenate([t, [100, 100, 101], 101 + np.arange(1, 41)])  # a pause 67 -> 100 (windows 7, 8, 9 of D = E = 10 are empty), then 1 per event
    assert len(t) == 64
    return (T0_US + t).astype(np.int64) if dtype == np.int64 else (0.5 + t / 8).astype(np.float64)


@pytest.mark.parametrize('dtype', [np.int64, np.float64], ids=['int64', 'float64'])
@pytest.mark.parametrize('overlap', [False, True], ids=['stride=window', 'stride=window/4'])
def test_duration_windows_against_a_brute_force_cut(dtype, overlap):
    from ess_amd.datasets.event_feed import EventWindows
    t = _times(dtype)
    D = 10 if dtype == np.int64 else 1.25  # (1.25 = 10 / 8: the float bounds are exact binary fractions, so events DO fall on them)
    E = D / 4 if overlap and dtype != np.int64 else (D if not overlap else 5)
    want = _brute(t, D, E)
    assert any(c == 0 for _, c in want)                                    # an empty window
    lows = t[0] + np.arange(len(want)) * E
    assert len(np.intersect1d(lows[1:], t)) >= 2                           # events exactly on a lower bound
    w = EventWindows(window_duration=D, stride=E)
    fed, got, per_packet = 0, [], []
    for n in PACKETS:
        w.push(n, t[fed:fed + n])
        fed += n
        new = _drain(w)
        per_packet.append(len(new))
        got += new
        # what is still needed: the first event of the next window (or, with none open, whatever comes)
        assert w.oldest_needed() <= fed
    assert got == want
    assert per_packet[3] >= 3                                              # one packet completed three windows and more
    assert all(t[s] >= t[0] + k * E for k, (s, c) in enumerate(got) if c)  # (and the brute force itself reads the definition)
    # the same stream in one packet
    w = EventWindows(window_duration=D, stride=E)
    assert w.push(64, t) == len(want) and _drain(w) == want


def test_duration_windows_keep_the_events_overlapping_windows_still_read():
    from ess_amd.datasets.event_feed import EventWindows
    t = np.arange(0, 100, dtype=np.int64)
    w = EventWindows(window_duration=20, stride=5)
    w.push(30, t[:30])                       # windows 0 ([0, 20)) and 1 ([5, 25)) complete, 2 .. 5 have begun
    assert w.pending == 2 and w.oldest_needed() == 0
    assert w.pop() == (0, 20) and w.oldest_needed() == 5
    assert w.pop() == (5, 20) and w.oldest_needed() == 10
    with pytest.raises(Exception, match='integral'):
        EventWindows(window_duration=2.5).push(3, t[:3])
    with pytest.raises(Exception, match='finite'):
        EventWindows(window_duration=2.5).push(2, np.array([0.0, float('inf')]))


# ---------------------------------------------------------------------------------------------- refusals
def _state(w):
    return (w.head, w.last_t, w.t0, w.window, w.stride, w._next, w._next_start, list(w._starts), list(w._pending), w.oldest_needed())


def test_push_refusals_leave_the_object_unchanged():
    from ess_amd import hip
    from ess_amd.datasets.event_feed import EventWindows
    # an overrun, count mode: N = 16, ring 32; 20 events fed, window 0 pending -> event 0 is needed, 13 more would reach 33
    w = EventWindows(window_events=16, stride=8, event_capacity=16, ring_capacity=32)
    t = np.arange(64, dtype=np.float64)
    w.push(20, t[:20])
    before = _state(w)
    with pytest.raises(hip.EssHipError, match='overrun'):
        w.push(13, t[20:33])
    assert _state(w) == before
    assert w.push(12, t[20:32]) == 3          # (exactly the ring: fine)
    assert w.pop() == (0, 16)
    assert w.push(8, t[32:40]) == 3           # (event 8 is the oldest needed now)
    # a packet larger than the ring, nothing pending
    w = EventWindows(window_events=16, event_capacity=16, ring_capacity=32)
    before = _state(w)
    with pytest.raises(hip.EssHipError, match='overrun'):
        w.push(33, t[:33])
    assert _state(w) == before
    # an oversized window, duration mode: 9 events inside one window of 8 at the most -- also as the very first packet
    for first in (True, False):
        w = EventWindows(window_duration=100, event_capacity=8, ring_capacity=64)
        ts = np.array([0, 10, 20, 30, 40, 50, 60, 70, 80, 100, 101], dtype=np.int64)
        if not first:
            w.push(2, ts[:2])
        before = _state(w)
        with pytest.raises(hip.EssHipError, match='9 events.*event_capacity=8'):
            w.push(len(ts) - (0 if first else 2), ts if first else ts[2:])
        assert _state(w) == before
    # back in time: refused; equal times across packets are fine
    w = EventWindows(window_events=4)
    w.push(3, np.array([1.0, 2.0, 3.0]))
    before = _state(w)
    with pytest.raises(hip.EssHipError, match='non-decreasing'):
        w.push(2, np.array([2.5, 4.0]))
    assert _state(w) == before
    assert w.push(2, np.array([3.0, 4.0])) == 1
    with pytest.raises(hip.EssHipError, match='times'):
        w.push(3, np.zeros(2) + 9)


# ---------------------------------------------------------------------------------------------- the packet's way into a ring
def test_ring_segments_split_at_the_wrap():
    from ess_amd import hip
    from ess_amd.datasets.event_feed import ring_segments
    assert ring_segments(0, 0, 32) == []
    assert ring_segments(0, 32, 32) == [(0, 0, 32)]
    assert ring_segments(30, 2, 32) == [(30, 0, 2)]            # ends exactly at the wrap
    assert ring_segments(30, 5, 32) == [(30, 0, 2), (0, 2, 3)]
    assert ring_segments(64 + 31, 32, 32) == [(31, 0, 1), (0, 1, 31)]
    assert ring_segments(96, 7, 32) == [(0, 0, 7)]
    for bad in ((0, 33, 32), (-1, 1, 32), (0, -1, 32), (0, 0, 0)):
        with pytest.raises(hip.EssHipError):
            ring_segments(*bad)


@pytest.mark.parametrize('t', [np.float64, np.int64])
@pytest.mark.parametrize('xy', [np.int16, np.uint16])
def test_copy_into_ring_writes_the_packets_own_bits_and_nothing_else(t, xy):
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.event_feed import copy_into_ring
    R = 32
    g = np.random.default_rng(3)
    raw = [np.full(R * size, 0x5A, np.uint8) for size in (8, 2, 2, 1)]
    views = (raw[0].view(np.int64), raw[1].view(np.int16), raw[2].view(np.int16), raw[3])
    mirror = [[None] * R for _ in range(4)]  # what each entry must hold, as bytes
    head = 0
    for n in (7, 13, 1, 9, 32, 3):  # 65 events: wraps twice, one packet fills the whole ring
        cols = EventColumns(np.sort(g.integers(0, 1 << 50, n)).astype(t), g.integers(0, 40000, n).astype(xy), g.integers(0, 40000, n).astype(xy),
                            g.integers(0, 2, n).astype(np.uint8))
        segs = copy_into_ring(cols, views, head, R)
        assert sum(m for _, _, m in segs) == n and len(segs) <= 2
        for k in range(n):
            for c, col in enumerate((cols.t, cols.x, cols.y, cols.p)):
                mirror[c][(head + k) % R] = col[k:k + 1].tobytes()
        head += n
        for c, size in enumerate((8, 2, 2, 1)):
            for e in range(R):
                got = raw[c][e * size:(e + 1) * size].tobytes()
                assert got == (mirror[c][e] if mirror[c][e] is not None else b'\x5a' * size), (n, c, e)
    with pytest.raises(hip.EssHipError, match='EventColumns'):
        copy_into_ring(np.zeros((3, 4)), views, 0, R)
    with pytest.raises(hip.EssHipError, match='8-byte'):
        copy_into_ring(cols, (np.zeros(R, np.int32),) + views[1:], 0, R)


# ---------------------------------------------------------------------------------------------- the binding
def test_the_binding_refuses_what_needs_no_device_to_be_refused():
    from ess_amd import hip
    n_rows, ring, n_slots = 2, 32, 3
    ok = dict(t=torch.zeros(n_rows, ring, dtype=torch.int64), x=torch.zeros(n_rows, ring, dtype=torch.int16),
              y=torch.zeros(n_rows, ring, dtype=torch.int16), p=torch.zeros(n_rows, ring, dtype=torch.uint8),
              rows=torch.zeros(n_slots, dtype=torch.int32), starts=torch.zeros(n_slots, dtype=torch.int32),
              counts=torch.zeros(n_slots, dtype=torch.int32), formats=torch.zeros(n_slots, dtype=torch.int32),
              out=torch.zeros(n_slots, 5, 24, 40), acc=torch.zeros(n_slots * 5 * 24 * 40, dtype=torch.int64))

    def refused(match, **kw):
        with pytest.raises(hip.EssHipError, match=match):
            hip.event_ingest_ring(**{**ok, **kw})
    refused('no CPU path')                                                     # CPU tensors, nothing else wrong
    refused('no CPU path', t=np.zeros((n_rows, ring), np.int64))               # not a tensor at all
    refused('t must be', t=ok['t'].to(torch.int32))                            # wrong dtypes
    refused('x must be', x=ok['x'].to(torch.int32))
    refused('p must be', p=ok['p'].to(torch.int16))
    refused('rows must be int32', rows=ok['rows'].to(torch.int64))
    refused('formats must be int32', formats=ok['formats'].to(torch.int16))
    refused('acc must be int64', acc=ok['acc'].to(torch.int32))
    refused('out must be', out=ok['out'].to(torch.float64))
    refused('y must be', y=ok['y'][:, :16].contiguous())                       # wrong shapes
    refused('t must be', t=ok['t'][0])
    refused(r'starts must be int32 \[3\]', starts=torch.zeros(2, dtype=torch.int32))
    refused(r'counts must be int32 \[3\]', counts=torch.zeros(1, 3, dtype=torch.int32))
    refused('out must be', out=ok['out'][0])
    refused('multiple of 16', **{k: ok[k][:, :24].contiguous() for k in 'txyp'})   # a ring that is no multiple of 16
    refused('multiple of 16', **{k: ok[k][:, :8].contiguous() for k in 'txyp'})


def test_segmenter_knows_the_ring_layout():
    from ess_amd import hip
    from ess_amd.run_segmentation import EVENT_LAYOUTS, _event_layout
    assert EVENT_LAYOUTS == ('records', 'columns', 'ring') and _event_layout('ring', 512) == 'ring'
    with pytest.raises(hip.EssHipError, match='event_capacity'):
        _event_layout('ring', None)
