"""Hot-pixel masks of one sensor, in the bit layout hip.event_ingest_masked reads: uint32 [H, ceil(W / 32)], pixel (x, y) = bit
x & 31 of word x >> 5 of row y, a set bit means hot.  The text form is the reference's hot_pixels_file: one `x,y` line per pixel
(np.loadtxt(..., delimiter=','))."""
import numpy as np

MAX_SIDE = 32768  # (hip.MASK_MAX_SIDE: the sensor's sides the library accepts)


def _side(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIDE:
        raise ValueError(f'HotPixelMask: {name}={v!r} must be an int in [1, {MAX_SIDE}]')
    return int(v)


class HotPixelMask:
    """One sensor's hot pixels.  Built by from_locations / from_file / from_bool / from_words; immutable afterwards (the segmenters
    share one device copy among the streams that name the same object)."""

    def __init__(self, words, height, width):
        self.height, self.width = _side('height', height), _side('width', width)
        n_words = (self.width + 31) // 32
        words = np.asarray(words)
        if words.dtype != np.uint32 or words.shape != (self.height, n_words):
            raise ValueError(f'HotPixelMask: words must be uint32 [{self.height}, {n_words}], got {words.dtype}{words.shape}')
        tail = self.width & 31
        if tail and (words[:, -1] >> np.uint32(tail)).any():
            raise ValueError(f'HotPixelMask: bits at x >= width={self.width} are set in the last word of a row')
        self.words = np.ascontiguousarray(words)
        self.words.setflags(write=False)

    @classmethod
    def from_words(cls, words, height, width):
        return cls(np.array(words, dtype=np.uint32, copy=True), height, width)

    @classmethod
    def from_bool(cls, array):
        a = np.asarray(array)
        if a.dtype != np.bool_ or a.ndim != 2 or a.size == 0:
            raise ValueError(f'HotPixelMask.from_bool: a non-empty bool [H, W] array, got {a.dtype}{a.shape}')
        h, w = a.shape
        n_words = (w + 31) // 32
        padded = np.zeros((h, n_words * 32), dtype=np.bool_)
        padded[:, :w] = a
        weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
        words = (padded.reshape(h, n_words, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32)
        return cls(words, h, w)

    @classmethod
    def from_locations(cls, xy, height, width):
        """xy: [N, 2] integer rows of (x, y), as the reference's hot_pixels_file holds them (N may be 0)"""
        h, w = _side('height', height), _side('width', width)
        a = np.asarray(xy)
        if a.size == 0:
            a = np.zeros((0, 2), dtype=np.int64)
        if a.ndim == 1 and a.shape[0] == 2:
            a = a[None]  # (np.loadtxt gives a one-line file as [2])
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f'HotPixelMask.from_locations: xy must be [N, 2] rows of (x, y), got {a.shape}')
        if not np.issubdtype(a.dtype, np.integer):
            if not np.issubdtype(a.dtype, np.floating) or not np.array_equal(a, np.floor(a)):
                raise ValueError(f'HotPixelMask.from_locations: xy must hold whole numbers, got {a.dtype}')
        a = a.astype(np.int64)
        bad = (a[:, 0] < 0) | (a[:, 0] >= w) | (a[:, 1] < 0) | (a[:, 1] >= h)
        if bad.any():
            x, y = a[np.argmax(bad)]
            raise ValueError(f'HotPixelMask.from_locations: pixel (x={x}, y={y}) lies outside the {h} x {w} sensor '
                             f'({int(bad.sum())} of {len(a)} do)')
        b = np.zeros((h, w), dtype=np.bool_)
        b[a[:, 1], a[:, 0]] = True
        return cls.from_bool(b)

    @classmethod
    def from_file(cls, path, height, width):
        """the reference's hot_pixels_file: np.loadtxt(path, delimiter=',') rows of x,y"""
        with open(path) as f:
            text = f.read()
        if not text.strip():
            return cls.from_locations(np.zeros((0, 2), dtype=np.int64), height, width)
        return cls.from_locations(np.loadtxt(path, delimiter=',', ndmin=2), height, width)

    @classmethod
    def from_store(cls, store, recording, size, max_events_per_pixel=None, max_rate_hz=None, begin=None, end=None):
        """A mask calibrated from a recording of a device EventStore, by MultiStreamSegmenter.calibrate_hot_pixels' rule: a pixel of
        the size = (h, w) sensor is hot when it fired MORE than max_events_per_pixel=k events, or more than
        floor(max_rate_hz * (t_last - t_first)) events, the times of the range's first and last event in the unit of the
        recording's time column -- exactly one of the two limits.  begin, end: event indices relative to the recording (default:
        all of it).  The counts are plain 64-bit integers (hip.event_store_pixel_counts): a whole recording fits, where the
        histogram sums of the ring calibration end at 2^22 events a pixel.  Outside any capture; the store is not modified.
        Refused with ValueError before any device call: an unknown recording, a range outside it, both limits or neither, a size
        outside 1 .. 32768."""
        from .event_store import EventStore
        what = 'HotPixelMask.from_store'
        if not isinstance(store, EventStore):
            raise ValueError(f'{what}: store must be an EventStore, got {type(store).__name__}')
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))  # noqa: E731
        if not is_int(recording) or not 0 <= recording < store.n_recordings:
            raise ValueError(f'{what}: recording {recording!r} of {store.n_recordings}')
        if not isinstance(size, (tuple, list)) or len(size) != 2:
            raise ValueError(f'{what}: size={size!r} must be (h, w), the sensor\'s size')
        h, w = _side('size[0]', size[0]), _side('size[1]', size[1])
        if (max_events_per_pixel is None) == (max_rate_hz is None):
            raise ValueError(f'{what}: give max_events_per_pixel=k or max_rate_hz=r, exactly one of the two')
        by_rate = max_rate_hz is not None
        limit = max_rate_hz if by_rate else max_events_per_pixel
        ok = isinstance(limit, (int, float, np.integer, np.floating)) if by_rate else isinstance(limit, (int, np.integer))
        if isinstance(limit, (bool, np.bool_)) or not ok or not 0 <= limit < float('inf'):
            raise ValueError(f'{what}: the limit {limit!r} must be a non-negative ' + ('number' if by_rate else 'int'))
        first, last = store.extent(int(recording))
        n = last - first
        b, e = 0 if begin is None else begin, n if end is None else end
        if not is_int(b) or not is_int(e) or not 0 <= b <= e <= n:
            raise ValueError(f'{what}: the range begin={begin!r}, end={end!r} lies outside recording {recording} of {n} events '
                             '(0 <= begin <= end <= its events, relative to the recording)')
        import torch
        if torch.cuda.is_current_stream_capturing():
            raise ValueError(f'{what}: a calibration downloads its mask: it runs outside any capture')
        b, e = int(b), int(e)
        threshold = int(np.floor(float(limit) * store.range_time_span(int(recording), b, e))) if by_rate else int(limit)
        return cls.from_words(store.count_mask_words(int(recording), b, e, (h, w), threshold), h, w)

    def to_bool(self):
        bits = (self.words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
        return bits.reshape(self.height, -1)[:, :self.width].astype(np.bool_)

    def to_locations(self):
        """int64 [N, 2] rows of (x, y), sorted by (y, x): np.savetxt(path, m.to_locations(), fmt='%d', delimiter=',') writes a file
        the reference reads"""
        y, x = np.nonzero(self.to_bool())  # (row-major: sorted by y, then x)
        return np.stack([x, y], axis=1).astype(np.int64)

    def count(self):
        return int(self.to_bool().sum())

    def __eq__(self, other):
        return isinstance(other, HotPixelMask) and (self.height, self.width) == (other.height, other.width) and \
            np.array_equal(self.words, other.words)

    __hash__ = object.__hash__

    def __repr__(self):
        return f'HotPixelMask({self.height} x {self.width}, {self.count()} hot)'
