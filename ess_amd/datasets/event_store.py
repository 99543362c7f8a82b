"""The device event store: recordings uploaded ONCE, training samples named by a recording, a time (or an index) and a label.

EventBatchBuilder builds a batch from host EventColumns: every sample's events are copied into pinned staging and uploaded again for
every batch, although consecutive samples of a recording overlap almost entirely.  An EventStore keeps the four raw columns of whole
recordings in device memory -- 13 bytes an event: t 8, x 2, y 2, p 1, the bytes the rings store -- laid one behind the other in one
flat set, with a table of (begin, end, format) per recording beside them, also on the device.  A sample is then a StoreSample:
a recording number, the sample's end (a time, as the DSEC loader names it, or an event index, as the DDD17 loader's
img_timestamp_event_idx does), a label index and a map index; hip.event_store_windows turns B of them into the B * T slot words
on the device, and EventBatchBuilder(store=...) runs the rest of the loader behind it inside one captured graph.

File readers stay outside: a recording arrives as EventColumns packets and a uint8 label array.  Numpy and torch only."""
import numpy as np
import torch

from .. import hip
from .data_util import EventColumns, stage_event_columns

STAGING_EVENTS = 1 << 20  # events per pinned staging set of an upload: 13 MiB, whatever the recording's size
_DTYPES = (torch.int64, torch.int16, torch.int16, torch.uint8)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def time_bound(bound, t_i64):
    """a time bound -> the 8-byte word hip.event_store_windows compares a recording's times with, as a Python int: for int64 times
    a fractional bound is raised to the next integer first (t >= b and t >= ceil(b) are one condition:
    datasets.event_feed.ring_end_index), for float64 times the word is the bound's bits"""
    if not _is_number(bound) or bound != bound:
        raise hip.EssHipError(f'time_bound: {bound!r} is no time')
    if t_i64:
        if int(bound) != bound:
            bound = int(np.ceil(bound))
        return int(np.int64(bound))
    return int(np.float64(bound).view(np.int64))


def duration_bounds(t_end, T, window_duration):
    """the T + 1 bounds of the DSEC loader's fixed_duration cut, in the host arithmetic of
    datasets.event_feed.sequence_windows_fixed_duration: ts_start = t_end - T d; per = (T d) / T; bound i = ts_start + i per"""
    delta_t = T * window_duration
    ts_start = t_end - delta_t
    per = delta_t / T
    return [ts_start + i * per for i in range(T + 1)]


class _Staging:
    """one pinned staging set of an upload: the four columns, STAGING_EVENTS entries each"""
    __slots__ = ('cols', 'cols_np', 'done')

    def __init__(self, n):
        self.cols = tuple(torch.zeros(n, dtype=d).pin_memory() for d in _DTYPES)
        self.cols_np = tuple(c.numpy() for c in self.cols)
        self.done = torch.cuda.Event()


class EventStore:
    """EventStore(capacity_events, device=None, label_hw=None, label_capacity=0, max_recordings=1024)

    capacity_events: the events the store can hold, rounded up to a multiple of 16.  Device memory, allocated at the first accepted
    recording: 13 bytes per event of capacity + label_capacity * Hl * Wl bytes of labels + 32 bytes per row of the recording table.
    add_recording(columns_or_packets, t_offset=0, labels=None) -> the recording's number.  columns_or_packets: one EventColumns or
        a list of them (the packets a reader delivers), all of ONE format, times non-decreasing inside every packet and from one to
        the next.  t_offset: what a sample's t_end is lowered by before it is compared with the recording's times (the DSEC files'
        t_offset).  labels: uint8 [n, Hl, Wl] (label_hw), appended to the store's label tensor; label_range(id) -> (first, n), and a
        StoreSample names a label by first + k.
    append(id, EventColumns): more events for the LAST recording (the same format, times going on non-decreasing).
    extent(id) -> (begin, end) in absolute event indices; n_events, n_recordings, bytes().
    Refused with hip.EssHipError, the store left as it was: unsorted times, mixed formats, a full store (events, labels or table
    rows).  Everything is checked before the first byte moves.  An upload goes in chunks of STAGING_EVENTS events through two
    pinned staging sets; the recording's table row is written behind its events, in stream order, so a captured graph that reads
    the table sees a recording only whole."""

    def __init__(self, capacity_events, device=None, label_hw=None, label_capacity=0, max_recordings=1024):
        if not _is_int(capacity_events) or not 1 <= capacity_events <= hip.EVENT_STORE_MAX_CAPACITY:
            raise hip.EssHipError(f'EventStore: capacity_events={capacity_events!r} must be an int in [1, 2^40]')
        if not _is_int(label_capacity) or label_capacity < 0:
            raise hip.EssHipError(f'EventStore: label_capacity={label_capacity!r} must be a non-negative int')
        if not _is_int(max_recordings) or not 1 <= max_recordings <= 1 << 24:
            raise hip.EssHipError(f'EventStore: max_recordings={max_recordings!r} must be an int in [1, 2^24]')
        if (label_hw is None) != (label_capacity == 0):
            raise hip.EssHipError(f'EventStore: label_hw={label_hw!r} and label_capacity={label_capacity!r} are given together or not at all')
        if label_hw is not None and (not isinstance(label_hw, (tuple, list)) or len(label_hw) != 2 or
                                     any(not _is_int(v) or v < 1 for v in label_hw)):
            raise hip.EssHipError(f'EventStore: label_hw={label_hw!r}: a pair of positive ints is needed')
        self.capacity = hip.event_column_stride(capacity_events)
        self.device = device if device is not None else torch.device('cuda:0')
        self.label_hw = None if label_hw is None else (int(label_hw[0]), int(label_hw[1]))
        self.label_capacity, self.max_recordings = int(label_capacity), int(max_recordings)
        self.n_events = self.n_labels = 0
        self._recs = []  # per recording: [begin, end, format, t_offset, last time or None, first label, labels]
        self._dev = None

    # ---- what the store holds
    @property
    def n_recordings(self):
        return len(self._recs)

    def _rec(self, rid, what):
        if not _is_int(rid) or not 0 <= rid < len(self._recs):
            raise hip.EssHipError(f'EventStore.{what}: recording {rid!r} of {len(self._recs)}')
        return self._recs[rid]

    def extent(self, rid):
        r = self._rec(rid, 'extent')
        return r[0], r[1]

    def format_of(self, rid):
        return self._rec(rid, 'format_of')[2]

    def t_offset(self, rid):
        return self._rec(rid, 't_offset')[3]

    def label_range(self, rid):
        r = self._rec(rid, 'label_range')
        return r[5], r[6]

    def bytes(self):
        """the device memory of the store (allocated or not yet)"""
        lab = self.label_capacity * self.label_hw[0] * self.label_hw[1] if self.label_hw else 0
        return 13 * self.capacity + lab + 8 * hip.EVENT_STORE_TABLE_WORDS * self.max_recordings

    # ---- the device side
    @property
    def columns(self):
        """(t, x, y, p): the flat device columns [capacity]; t holds int64 and float64 recordings alike, as their bits"""
        return self._device()['cols']

    @property
    def table(self):
        return self._device()['table']

    @property
    def labels(self):
        return self._device()['labels']

    def _device(self):
        if self._dev is None:
            dev = self.device
            table = torch.zeros(self.max_recordings, hip.EVENT_STORE_TABLE_WORDS, dtype=torch.int64)
            table[:, 2] = -1  # (unused rows)
            self._dev = {
                'cols': tuple(torch.zeros(self.capacity, dtype=d, device=dev) for d in _DTYPES),
                'table': table.to(dev),
                'labels': None if self.label_hw is None else torch.zeros((self.label_capacity,) + self.label_hw, dtype=torch.uint8, device=dev),
                'stage': [_Staging(min(STAGING_EVENTS, self.capacity)) for _ in range(2)],
                'row': torch.zeros(hip.EVENT_STORE_TABLE_WORDS, dtype=torch.int64).pin_memory(),
                'row_done': torch.cuda.Event(),
                'chunks': 0,
            }
        return self._dev

    def _upload(self, packets, at):
        """the packets' events -> the device columns from absolute index `at` on, in chunks through the two pinned sets"""
        d = self._device()
        room = len(d['stage'][0].cols_np[0])
        for c in packets:
            for off in range(0, c.n, room):
                m = min(room, c.n - off)
                stage = d['stage'][d['chunks'] & 1]
                d['chunks'] += 1
                stage.done.synchronize()  # (the set's last upload has completed)
                part = EventColumns(c.t[off:off + m], c.x[off:off + m], c.y[off:off + m], c.p[off:off + m]) if (off or m < c.n) else c
                stage_event_columns(part, *stage.cols_np)
                for dev, host in zip(d['cols'], stage.cols):
                    dev[at:at + m].copy_(host[:m], non_blocking=True)
                stage.done.record()
                at += m

    def _write_row(self, rid):
        d = self._device()
        d['row_done'].synchronize()
        r = self._recs[rid]
        d['row'].copy_(torch.tensor([r[0], r[1], r[2], 0], dtype=torch.int64))
        d['table'][rid].copy_(d['row'], non_blocking=True)
        d['row_done'].record()

    # ---- hot-pixel calibration (datasets.hot_pixels.HotPixelMask.from_store checks the arguments; nothing of the store is written)
    def range_time_span(self, rid, begin, end):
        """float(t of event end - 1) - float(t of event begin) of recording `rid`, indices relative to the recording, in the unit of
        its time column (0.0 for an empty range): one download of two time words"""
        r = self._rec(rid, 'range_time_span')
        if end <= begin:
            return 0.0
        t = self.columns[0]
        words = torch.cat([t[r[0] + begin:r[0] + begin + 1], t[r[0] + end - 1:r[0] + end]]).cpu().numpy()
        times = words if r[2] & hip.EVCOL_T_I64 else words.view(np.float64)
        return float(times[1]) - float(times[0])

    def count_mask_words(self, rid, begin, end, size, threshold):
        """the events begin .. end - 1 of recording `rid` (relative indices) counted per pixel of a size = (h, w) sensor, and the
        pixels with MORE than `threshold` events as mask words, host uint32 [h, ceil(w / 32)]: one zero fill, hip.
        event_store_pixel_counts, hip.event_count_mask, one download.  Plain int64 counts: a pixel may hold any number of events."""
        r = self._rec(rid, 'count_mask_words')
        h, w = size
        x, y = self.columns[1], self.columns[2]
        dev = x.device
        job = torch.tensor([r[0] + begin, r[0] + end, min(int(threshold), 1 << 62)], dtype=torch.int64).to(dev)
        fmt = torch.tensor([r[2]], dtype=torch.int32).to(dev)
        counts = torch.zeros(1, h, w, dtype=torch.int64, device=dev)
        hip.event_store_pixel_counts(x, y, job[0:1], job[1:2], fmt, counts, self.n_events)
        words = torch.empty(1, h, hip.mask_words(w), dtype=torch.int32, device=dev)
        hip.event_count_mask(counts, job[2:3], words, hip.MASK_REPLACE)
        return words[0].cpu().numpy().view(np.uint32)

    # ---- the checks of an upload: nothing is written
    @staticmethod
    def _packets(what, columns_or_packets, fmt, last_t):
        packets = [columns_or_packets] if isinstance(columns_or_packets, EventColumns) else columns_or_packets
        if not isinstance(packets, (list, tuple)) or any(not isinstance(c, EventColumns) for c in packets):
            raise hip.EssHipError(f'EventStore.{what}: an EventColumns or a list of them is needed')
        packets = [c for c in packets if c.n]
        for k, c in enumerate(packets):
            if fmt is None:
                fmt = c.format
            if c.format != fmt:
                raise hip.EssHipError(f'EventStore.{what}: packet {k} has format {c.format}, the recording {fmt}: a recording\'s packets '
                                      'share one format (time and coordinate dtypes)')
            if not bool(np.all(c.t[1:] >= c.t[:-1])) or c.t[0] != c.t[0] or (last_t is not None and not c.t[0] >= last_t):
                raise hip.EssHipError(f'EventStore.{what}: the times of packet {k} are not non-decreasing (inside it, or from the packet '
                                      'before it): the window search needs sorted times')
            last_t = c.t[-1].item()
        return packets, fmt, last_t

    def add_recording(self, columns_or_packets, t_offset=0, labels=None):
        if not _is_number(t_offset) or t_offset != t_offset:
            raise hip.EssHipError(f'EventStore.add_recording: t_offset={t_offset!r} must be a number')
        packets, fmt, last_t = self._packets('add_recording', columns_or_packets, None, None)
        n = sum(c.n for c in packets)
        if len(self._recs) >= self.max_recordings:
            raise hip.EssHipError(f'EventStore.add_recording: the table holds max_recordings={self.max_recordings} recordings')
        if self.n_events + n > self.capacity:
            raise hip.EssHipError(f'EventStore.add_recording: the store is full: {self.n_events} + {n} events, capacity {self.capacity}')
        n_lab = 0
        if labels is not None:
            if torch.is_tensor(labels) and not labels.is_cuda:
                labels = labels.numpy()
            if self.label_hw is None or not isinstance(labels, np.ndarray) or labels.dtype != np.uint8 or labels.ndim != 3 or \
                    tuple(labels.shape[1:]) != self.label_hw:
                got = f'{labels.dtype}{tuple(labels.shape)}' if hasattr(labels, 'dtype') else type(labels).__name__
                raise hip.EssHipError(f'EventStore.add_recording: labels must be a host uint8 [n, Hl, Wl] array with (Hl, Wl) = the '
                                      f'store\'s label_hw={self.label_hw}, got {got}')
            n_lab = labels.shape[0]
            if self.n_labels + n_lab > self.label_capacity:
                raise hip.EssHipError(f'EventStore.add_recording: the label tensor is full: {self.n_labels} + {n_lab} labels, '
                                      f'label_capacity {self.label_capacity}')
        begin = self.n_events
        self._upload(packets, begin)
        if n_lab:
            self._device()['labels'][self.n_labels:self.n_labels + n_lab].copy_(torch.from_numpy(np.ascontiguousarray(labels)))
        self._recs.append([begin, begin + n, 0 if fmt is None else fmt, t_offset, last_t, self.n_labels, n_lab])
        self.n_events += n
        self.n_labels += n_lab
        self._write_row(len(self._recs) - 1)
        return len(self._recs) - 1

    def append(self, rid, cols):
        r = self._rec(rid, 'append')
        if rid != len(self._recs) - 1:
            raise hip.EssHipError(f'EventStore.append: recording {rid} is not the last of {len(self._recs)}: recordings lie one behind '
                                  'the other, only the last can grow')
        if not isinstance(cols, EventColumns):
            raise hip.EssHipError(f'EventStore.append: an EventColumns is needed, got {type(cols).__name__}')
        packets, fmt, last_t = self._packets('append', cols, r[2] if r[1] > r[0] else None, r[4])
        n = sum(c.n for c in packets)
        if self.n_events + n > self.capacity:
            raise hip.EssHipError(f'EventStore.append: the store is full: {self.n_events} + {n} events, capacity {self.capacity}')
        if n == 0:
            return rid
        self._upload(packets, r[1])
        r[1], r[2], r[4] = r[1] + n, fmt, last_t
        self.n_events += n
        self._write_row(rid)
        return rid


class StoreSample:
    """One training sample of an EventStore: recording (its number), its end -- t_end: a time in the unit of the recording's file
    (the recording's t_offset is subtracted before the search), or end: an event index relative to the recording -- exactly one of
    the two; label: the index of its label in the store's label tensor, or None; map: the number of its rectify map, or None;
    frame: the slot of its paired camera frame in a frame store (image_store.ImageStore, EventBatchBuilder(frames=)), or None."""
    __slots__ = ('recording', 't_end', 'end', 'label', 'map', 'frame')

    def __init__(self, recording, t_end=None, end=None, label=None, map=None, frame=None):
        if not _is_int(recording) or recording < 0:
            raise hip.EssHipError(f'StoreSample: recording={recording!r} must be a non-negative int')
        if (t_end is None) == (end is None):
            raise hip.EssHipError('StoreSample: give t_end (a time) or end (an event index of the recording), one of the two')
        if t_end is not None and (not _is_number(t_end) or not np.isfinite(t_end)):
            raise hip.EssHipError(f'StoreSample: t_end={t_end!r} must be a finite time')
        if end is not None and (not _is_int(end) or end < 0):
            raise hip.EssHipError(f'StoreSample: end={end!r} must be a non-negative int')
        for name, v in (('label', label), ('map', map), ('frame', frame)):
            if v is not None and (not _is_int(v) or v < 0):
                raise hip.EssHipError(f'StoreSample: {name}={v!r} must be a non-negative int or None')
        for name, v in zip(self.__slots__, (int(recording), t_end, None if end is None else int(end), label, map, frame)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError('StoreSample is immutable')

    def __repr__(self):
        return f'StoreSample(recording={self.recording}, t_end={self.t_end!r}, end={self.end!r}, label={self.label!r}, map={self.map!r}, frame={self.frame!r})'


class StoreSampler:
    """The batches of an epoch over a list of StoreSamples: an iterable of lists of batch_size samples, with a length, as
    EventBatchLoader's sample_source.  shuffle: a new permutation every iteration (numpy's default_rng(seed + epoch)); drop_last
    False: a short last batch is filled up from the epoch's first samples (a builder takes whole batches only)."""

    def __init__(self, store, batch_size, samples, shuffle=True, seed=0, drop_last=True):
        if not isinstance(store, EventStore):
            raise hip.EssHipError(f'StoreSampler: store must be an EventStore, got {type(store).__name__}')
        if not _is_int(batch_size) or batch_size < 1:
            raise hip.EssHipError(f'StoreSampler: batch_size={batch_size!r} must be a positive int')
        samples = list(samples)
        for k, s in enumerate(samples):
            if not isinstance(s, StoreSample):
                raise hip.EssHipError(f'StoreSampler: samples[{k}] must be a StoreSample, got {type(s).__name__}')
            if s.recording >= store.n_recordings:
                raise hip.EssHipError(f'StoreSampler: samples[{k}] names recording {s.recording}, the store holds {store.n_recordings}')
        if not _is_int(seed):
            raise hip.EssHipError(f'StoreSampler: seed={seed!r} must be an int')
        self.store, self.batch_size, self.samples = store, int(batch_size), samples
        self.shuffle, self.seed, self.drop_last, self.epoch = bool(shuffle), int(seed), bool(drop_last), 0

    def __len__(self):
        n, B = len(self.samples), self.batch_size
        return n // B if self.drop_last else -(-n // B)

    def __iter__(self):
        n, B = len(self.samples), self.batch_size
        order = np.random.default_rng(self.seed + self.epoch).permutation(n) if self.shuffle else np.arange(n)
        self.epoch += 1
        for k in range(len(self)):
            idx = order[k * B:(k + 1) * B]
            if len(idx) < B:
                idx = np.concatenate([idx, np.resize(order, B - len(idx))])
            yield [self.samples[i] for i in idx]
