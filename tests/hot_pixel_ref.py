"""CPU integer restatement of the two hot-pixel kernels' rules (include/ess_hip.h, "HOT-PIXEL MASKS"), written from the header's
words with numpy integers only -- no HotPixelMask, no library:

  masked(cols, words, mask_h, mask_w): which events of a window ess_event_ingest_masked drops -- the event's raw (x, y), decoded as
      its format says, lies inside [0, mask_w) x [0, mask_h) and bit x & 31 of word x >> 5 of row y is set;
  moved_away(cols, hot): the window with every such event's x replaced by a value outside every grid and map (-1 in an int16
      column, 65535 in a uint16 one): the event keeps its place, so the window's time base is the same;
  mask_words_of(sums, thresholds, before, mode): the words ess_event_hot_pixel_mask leaves.
"""
import numpy as np

REPLACE, OR = 0, 1


def n_words(width):
    return (int(width) + 31) // 32


def words_of_locations(xy, mask_h, mask_w):
    """(x, y) pairs -> uint32 [mask_h, n_words(mask_w)], one bit set at a time"""
    w = np.zeros((mask_h, n_words(mask_w)), dtype=np.uint32)
    for x, y in xy:
        assert 0 <= x < mask_w and 0 <= y < mask_h
        w[y, x >> 5] |= np.uint32(1 << (x & 31))
    return w


def masked(cols, words, mask_h, mask_w):
    """cols: an object with x, y (int16 or uint16 arrays); words: uint32 [mask_h, n_words(mask_w)] or None (no mask) -> bool [n]"""
    x, y = cols.x.astype(np.int64), cols.y.astype(np.int64)  # (int16: sign-extended, uint16: the unsigned value)
    if words is None:
        return np.zeros(x.shape, dtype=bool)
    assert words.dtype == np.uint32 and words.shape == (mask_h, n_words(mask_w))
    inside = (x >= 0) & (x < mask_w) & (y >= 0) & (y < mask_h)
    xi, yi = np.where(inside, x, 0), np.where(inside, y, 0)
    bit = (words[yi, xi >> 5].astype(np.int64) >> (xi & 31)) & 1
    return inside & (bit == 1)


def moved_away(cols, hot):
    """-> (t, x', y, p) with x' = x but for the hot events, whose x lies outside everything; dtypes kept"""
    x = cols.x.copy()
    x[hot] = np.array(-1 if x.dtype == np.int16 else 65535).astype(x.dtype)
    return cols.t, x, cols.y, cols.p


def mask_words_of(sums, thresholds, before, mode):
    """sums: int64 [n, 2, H, W] at scale 2^40; thresholds: int64 [n]; before: uint32 [n, H, n_words(W)], the words in front of the
    call -> the words behind it"""
    n, two, H, W = sums.shape
    assert two == 2 and sums.dtype == np.int64 and before.dtype == np.uint32 and before.shape == (n, H, n_words(W))
    out = before.copy()
    for i in range(n):
        if int(thresholds[i]) < 0:
            continue
        for y in range(H):
            new = [0] * n_words(W)
            for x in range(W):
                if ((int(sums[i, 0, y, x]) + int(sums[i, 1, y, x])) >> 40) > int(thresholds[i]):
                    new[x >> 5] |= 1 << (x & 31)
            for k, v in enumerate(new):
                out[i, y, k] = np.uint32(v | int(before[i, y, k])) if mode == OR else np.uint32(v)
    return out
