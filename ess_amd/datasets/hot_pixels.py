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
