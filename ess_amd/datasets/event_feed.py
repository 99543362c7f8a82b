"""Host side of the continuous event feed (MultiStreamSegmenter(event_layout='ring')): a camera driver or a file reader delivers
PACKETS of arbitrary size that straddle window boundaries; the events go to a per-stream ring in device memory when they arrive,
and a round only names where each window lies.  Here: the per-stream bookkeeping that cuts windows out of the packet sequence
(EventWindows) and the copy of a packet into a ring that wraps (ring_segments, copy_into_ring).  No device work; numpy only."""
import collections

import numpy as np

from .. import hip
from .data_util import EventColumns


def ring_segments(head, n, ring):
    """n entries appended at absolute index head to a ring of `ring` entries -> [(ring position, packet offset, length)]: one
    segment, or two where the packet crosses the wrap.  n <= ring is the caller's to hold."""
    if n < 0 or ring < 1 or head < 0 or n > ring:
        raise hip.EssHipError(f'ring_segments: head={head} n={n} ring={ring}')
    if n == 0:
        return []
    at = head % ring
    first = min(n, ring - at)
    return [(at, 0, first)] + ([(0, first, n - first)] if first < n else [])


def copy_into_ring(cols, views, head, ring):
    """cols (EventColumns) -> four 1-D numpy ring views of `ring` entries each (t 8 raw bytes per entry, x / y 2, p 1) at absolute
    index head: per column at most two copies, each through a view of the column's own dtype -- its own bits, no cast, no temporary.
    -> the segments written (ring_segments)"""
    if not isinstance(cols, EventColumns):
        raise hip.EssHipError(f'copy_into_ring: an EventColumns is needed, got {type(cols).__name__}')
    for name, v, size in zip('txyp', views, (8, 2, 2, 1)):
        if not isinstance(v, np.ndarray) or v.ndim != 1 or v.dtype.itemsize != size or not v.flags.c_contiguous or len(v) != ring:
            raise hip.EssHipError(f'copy_into_ring: the {name} view must be a contiguous 1-D numpy array of {ring} {size}-byte items')
    segs = ring_segments(head, cols.n, ring)
    for c, v in zip((cols.t, cols.x, cols.y, cols.p), views):
        for at, off, m in segs:
            np.copyto(v[at:at + m].view(c.dtype), c[off:off + m])
    return segs


def _positive(name, v, integral):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not v > 0 or v != v or v == float('inf'):
        raise hip.EssHipError(f'EventWindows: {name}={v!r} must be a positive {"int" if integral else "number"}')
    if integral:
        if int(v) != v:
            raise hip.EssHipError(f'EventWindows: {name}={v!r} must be a positive int')
        return int(v)
    return v


MAX_WINDOWS_PER_PACKET = 1 << 16


def _bounds(t0, E, k0, offset, last):
    """the bounds t0 + k E + offset, k = k0 .., that are <= last -> an ascending array (possibly empty), in t0's arithmetic"""
    if last < t0 + k0 * E + offset:
        return np.zeros(0, dtype=np.int64 if isinstance(t0, int) else np.float64)
    m = int((last - t0 - offset) // E) - k0 + 2  # (an estimate from above; the comparison below decides)
    if m > MAX_WINDOWS_PER_PACKET:
        raise hip.EssHipError(f'EventWindows.push: the packet reaches t={last!r}, {m} window strides of {E!r} ahead: more than '
                              f'{MAX_WINDOWS_PER_PACKET} windows from one packet (a time gap, or a stride in another unit than t?)')
    b = t0 + np.arange(k0, k0 + max(m, 1), dtype=np.int64) * E + offset
    return b[:int(np.searchsorted(b, last, side='right'))]


class EventWindows:
    """One stream's window cutter, in ABSOLUTE event indices: index 0 is the first event fed.
    window_events=N, stride=M (default N): window k is [k M, k M + N), complete once k M + N events have been fed.
    window_duration=D, stride=E (default D), in the unit of t, T0 the first event's time: window k holds the events with
    T0 + k E <= t < T0 + k E + D (the two bounds evaluated in t's own arithmetic: float64, or exact integers for an int64 t, whose
    D and E must then be integral), complete once an event with t >= T0 + k E + D has been fed; its bounds are found with
    np.searchsorted on the packet that brings them.
    push(n, t) -> the number of windows now pending; t: the packet's n times, non-decreasing (the caller's contract; only the
    packet's first time is checked, against the previous packet's last).  pop() -> (start, count) of the oldest pending window.
    oldest_needed(): the oldest absolute index a pending or a future window still reads.  push refuses -- before anything
    changes -- a packet that goes back in time, one that would bring the head more than ring_capacity beyond oldest_needed() (a ring
    overrun), and one whose cut makes a window of more than event_capacity events."""

    def __init__(self, window_events=None, window_duration=None, stride=None, event_capacity=None, ring_capacity=None):
        if (window_events is None) == (window_duration is None):
            raise hip.EssHipError('EventWindows: give window_events=N or window_duration=D, one of the two')
        self.by_count = window_events is not None
        self.window = _positive('window_events', window_events, True) if self.by_count else _positive('window_duration', window_duration, False)
        self.stride = self.window if stride is None else _positive('stride', stride, self.by_count)
        self.event_capacity = None if event_capacity is None else _positive('event_capacity', event_capacity, True)
        self.ring_capacity = None if ring_capacity is None else _positive('ring_capacity', ring_capacity, True)
        if self.by_count and self.event_capacity is not None and self.window > self.event_capacity:
            raise hip.EssHipError(f'EventWindows: window_events={self.window} exceeds event_capacity={self.event_capacity}')
        self.head = 0        # events fed
        self.last_t = None   # the last time fed
        self.t0 = None       # duration mode: the first event's time
        self._next = 0       # count mode: the next window to complete; duration mode: the next window whose END is open
        self._next_start = 0  # duration mode: the next window whose START is open
        self._starts = collections.deque()  # duration mode: the starts found of windows _next .. _next_start - 1
        self._pending = collections.deque()  # (start, count), oldest first

    @property
    def pending(self):
        return len(self._pending)

    def oldest_needed(self):
        if self._pending:
            return self._pending[0][0]
        if self.by_count:
            return self._next * self.stride
        return self._starts[0] if self._starts else self.head

    def _cut(self, n, t):
        """the windows a packet completes -> (new pending windows, the state behind the packet); nothing is changed here"""
        head = self.head + n
        if self.by_count:
            N, M, k = self.window, self.stride, self._next
            done = []
            while k * M + N <= head:
                done.append((k * M, N))
                k += 1
            return done, dict(head=head, _next=k)
        t0, D, E = self.t0, self.window, self.stride
        if t0 is None:
            if np.issubdtype(t.dtype, np.integer):
                if int(D) != D or int(E) != E:
                    raise hip.EssHipError(f'EventWindows: integer times need an integral window_duration and stride, got {D!r} and {E!r}')
                t0, D, E = int(t[0]), int(D), int(E)
            else:
                t0 = float(t[0])
                if t0 != t0:
                    raise hip.EssHipError('EventWindows: the first time is NaN')
        last = t[-1].item()
        sb = _bounds(t0, E, self._next_start, 0, last)
        eb = _bounds(t0, E, self._next, D, last)
        starts = list(self._starts) + (self.head + np.searchsorted(t, sb, side='left')).tolist()
        ends = (self.head + np.searchsorted(t, eb, side='left')).tolist()
        done = [(starts[i], e - starts[i]) for i, e in enumerate(ends)]
        return done, dict(head=head, t0=t0, window=D, stride=E, _next=self._next + len(ends), _next_start=self._next_start + len(sb),
                          _starts=collections.deque(starts[len(ends):]))

    def push(self, n, t):
        n = int(n)
        if n == 0:
            return self.pending
        t = np.asarray(t)
        if t.ndim != 1 or len(t) != n:
            raise hip.EssHipError(f'EventWindows.push: t must hold the packet\'s {n} times, got shape {tuple(t.shape)}')
        first = t[0].item()
        if self.last_t is not None and first < self.last_t:
            raise hip.EssHipError(f'EventWindows.push: the packet starts at t={first!r}, before the previous packet\'s last time {self.last_t!r}: '
                                  'packets must be non-decreasing in t')
        if not self.by_count and not np.isfinite(t[-1]):
            raise hip.EssHipError(f'EventWindows.push: the packet ends at t={t[-1]!r}: duration windows need finite times')
        done, state = self._cut(n, t)
        if self.event_capacity is not None:
            for start, count in done:
                if count > self.event_capacity:
                    raise hip.EssHipError(f'EventWindows.push: the packet cuts a window of {count} events (from event {start}), '
                                          f'more than event_capacity={self.event_capacity}')
        if self.ring_capacity is not None:
            oldest = min(self.oldest_needed(), self.head)  # (what the windows still read, and the packet itself, must fit)
            if state['head'] - oldest > self.ring_capacity:
                raise hip.EssHipError(f'EventWindows.push: ring overrun: {n} more events bring the head to {state["head"]}, event {oldest} is '
                                      f'still needed by a window and the ring holds ring_capacity={self.ring_capacity}: pop windows first')
        for k, v in state.items():
            setattr(self, k, v)
        self._pending.extend(done)
        self.last_t = t[-1].item()
        return self.pending

    def pop(self):
        if not self._pending:
            raise hip.EssHipError('EventWindows.pop: no window is pending')
        return self._pending.popleft()


# ------------------------------------------------------------------------------- sequence rounds (run_sequence_segmentation.py)
def sequence_windows(end, available_from, T, n_per_window):
    """The DSEC loader's cut of one validation sample (reference DSEC/dataset/sequence.py:255-279), in absolute event indices: the
    last T * n_per_window events before `end` (the index get_events_fixed_num's t_end maps to), clamped at available_from (the
    loader: the start of the file; a ring: its oldest kept event), split into T equal windows.
        start = max(available_from, end - T * n_per_window);  loaded = end - start;  n = loaded // T
        window i = [start + i n, start + (i + 1) n);  the loaded - T n events at the END are not used (generate_event_tensor)
    -> a list of T pairs (start, count), or None where n == 0: no sequence"""
    end, available_from, T, n_per_window = int(end), int(available_from), int(T), int(n_per_window)
    if T < 1 or n_per_window < 1 or available_from < 0 or end < available_from:
        raise hip.EssHipError(f'sequence_windows: end={end} available_from={available_from} T={T} n_per_window={n_per_window}')
    start = max(available_from, end - T * n_per_window)
    n = (end - start) // T
    if n == 0:
        return None
    return [(start + i * n, n) for i in range(T)]


def ring_end_index(t_ring, head, ring, t_end, need=0):
    """The absolute index of the first fed event with t >= t_end (head where there is none): the index the reference's
    get_time_indices_offsets gives get_events_fixed_num (DSEC/utils/eventslicer.py:116, 223-228: time_array[idx_end] >= time_end_us,
    time_array[idx_end - 1] < time_end_us).  t_ring: the ring's time column on the host, `ring` entries in the stream's own dtype
    (int64 or float64; entry k mod ring holds event k), head: the events fed so far.  The kept events [max(0, head - ring), head)
    are at most two sorted segments of t_ring, each searched with np.searchsorted in t's own arithmetic.
    Refused: a t_end at or before the oldest kept event's time once older events have been overwritten (the index lies, or may lie,
    among them), and -- need: the events the caller's sequence reads before the index -- an index whose `need` predecessors (as far
    as the stream has any) are no longer all in the ring."""
    head, ring, need = int(head), int(ring), int(need)
    if not isinstance(t_ring, np.ndarray) or t_ring.ndim != 1 or len(t_ring) != ring or t_ring.dtype not in (np.int64, np.float64):
        raise hip.EssHipError(f'ring_end_index: t_ring must be the ring\'s {ring} times as a 1-D int64 or float64 array')
    if head < 0 or ring < 1 or need < 0:
        raise hip.EssHipError(f'ring_end_index: head={head} ring={ring} need={need}')
    oldest = max(0, head - ring)
    if isinstance(t_end, (float, np.floating)) and t_end != t_end:
        raise hip.EssHipError('ring_end_index: t_end is NaN')
    if t_ring.dtype == np.int64 and int(t_end) != t_end:
        t_end = int(np.ceil(t_end))  # (integer times: t >= t_end and t >= ceil(t_end) are one condition)
    t_end = t_ring.dtype.type(t_end)
    if oldest > 0 and t_end <= t_ring[oldest % ring]:
        raise hip.EssHipError(f'ring_end_index: t_end={t_end!r} is not after the oldest kept event (index {oldest}, '
                              f't={t_ring[oldest % ring]!r}): the events before it have been overwritten (ring of {ring})')
    end = oldest
    for at, _, m in ring_segments(oldest, head - oldest, ring):
        k = int(np.searchsorted(t_ring[at:at + m], t_end, side='left'))
        end += k
        if k < m:
            break
    if max(0, end - need) < oldest:
        raise hip.EssHipError(f'ring_end_index: the {need} events before index {end} (t_end={t_end!r}) reach back to event '
                              f'{max(0, end - need)}, the ring of {ring} keeps events from {oldest} on: feed a larger ring_capacity')
    return end


def _first_at_or_after(t_ring, oldest, head, ring, bound):
    """the absolute index of the first kept event [oldest, head) with t >= bound (head where there is none); for int64 times the
    bound is raised to the next integer first: t >= b and t >= ceil(b) are one condition"""
    if t_ring.dtype == np.int64 and int(bound) != bound:
        bound = int(np.ceil(bound))
    bound = t_ring.dtype.type(bound)
    at_abs = oldest
    for at, _, m in ring_segments(oldest, head - oldest, ring):
        k = int(np.searchsorted(t_ring[at:at + m], bound, side='left'))
        at_abs += k
        if k < m:
            break
    return at_abs


def sequence_windows_fixed_duration(t_ring, head, ring, t_end, T, window_duration):
    """The DSEC loader's fixed_duration cut of one sample (reference DSEC/dataset/sequence.py:224-231), in absolute event indices:
        ts_start = t_end - T d;  per = (T d) / T (the loader's delta_t_us / nr_events_data: a TRUE division, a float)
        window i = the events with ts_start + i per <= t < ts_start + (i + 1) per
    both bounds of a window found as "the first event with t >= bound" (EventSlicer.get_time_indices_offsets).  t_ring, head, ring: as
    ring_end_index.  -> T pairs (start, count); a count of 0 is a window without events (an all-zero grid).  Refused: a first bound at
    or before the oldest kept event's time once older events have been overwritten (the window's start lies, or may lie, among them)."""
    head, ring, T = int(head), int(ring), int(T)
    if not isinstance(t_ring, np.ndarray) or t_ring.ndim != 1 or len(t_ring) != ring or t_ring.dtype not in (np.int64, np.float64):
        raise hip.EssHipError(f'sequence_windows_fixed_duration: t_ring must be the ring\'s {ring} times as a 1-D int64 or float64 array')
    if head < 0 or ring < 1 or T < 1:
        raise hip.EssHipError(f'sequence_windows_fixed_duration: head={head} ring={ring} T={T}')
    d = window_duration
    if isinstance(d, bool) or not isinstance(d, (int, float, np.integer, np.floating)) or not d > 0 or d == float('inf'):
        raise hip.EssHipError(f'sequence_windows_fixed_duration: window_duration={d!r} must be a positive number')
    if isinstance(t_end, bool) or not isinstance(t_end, (int, float, np.integer, np.floating)) or not np.isfinite(t_end):
        raise hip.EssHipError(f'sequence_windows_fixed_duration: t_end={t_end!r} must be a finite time')
    delta_t = T * d
    ts_start = t_end - delta_t
    per = delta_t / T
    bounds = [ts_start + i * per for i in range(T + 1)]
    oldest = max(0, head - ring)
    if oldest > 0 and bounds[0] <= t_ring[oldest % ring]:
        raise hip.EssHipError(f'sequence_windows_fixed_duration: the sequence starts at t={bounds[0]!r}, not after the oldest kept event '
                              f'(index {oldest}, t={t_ring[oldest % ring]!r}): the events before it have been overwritten (ring of {ring})')
    idx = [_first_at_or_after(t_ring, oldest, head, ring, b) for b in bounds]
    # (window i is [first t >= bound i, first t >= bound i + 1), the two searches the loader makes per window)
    return [(idx[i], idx[i + 1] - idx[i]) for i in range(T)]


def sequence_windows_by_time(t, begin, end, T):
    """The DDD17 loader's cut of one sample by time (reference datasets/ddd17_events_loader.py:134-149) on the events [begin, end)
    of a recording's sorted time column t (entry k: event k's time), in absolute event indices:
        delta = int((t[end - 1] - t[begin]) / T);  id_end_i = searchsorted(t[begin:end], t[begin] + (i + 1) delta), at most end - begin
        window 0 starts at begin, window i at id_end_(i-1)
    -> T pairs (start, count).  The events behind id_end_(T-1) are not used; delta == 0 (a span shorter than T time units) gives T
    empty windows, as the loader's searchsorted does."""
    begin, end, T = int(begin), int(end), int(T)
    if not isinstance(t, np.ndarray) or t.ndim != 1:
        raise hip.EssHipError('sequence_windows_by_time: t must be a 1-D array of times')
    if T < 1 or not 0 <= begin < end <= len(t):
        raise hip.EssHipError(f'sequence_windows_by_time: begin={begin} end={end} T={T} on {len(t)} events (a non-empty range is needed)')
    ts = t[begin:end]
    n = len(ts)
    delta = int((ts[-1] - ts[0]) / T)
    out, id_end = [], 0
    for i in range(T):
        id_start = id_end
        id_end = min(int(np.searchsorted(ts, ts[0] + (i + 1) * delta)), n)
        out.append((begin + id_start, id_end - id_start))
    return out
