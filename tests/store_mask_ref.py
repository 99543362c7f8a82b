"""CPU integer restatement of the store's calibration kernels (include/ess_hip.h, "HOT-PIXEL MASKS ON THE STORE SOURCE"), written
from the header's words with numpy integers only -- no HotPixelMask, no library:

  pixel_counts(x_words, y_words, begin, end, fmt, total, H, W): what job (begin, end, fmt) of ess_event_store_pixel_counts adds to its
      plane -- one per event of [begin, end) whose coordinate, decoded under the XY_U16 bit, lies inside H x W; nothing where the
      range lies outside [0, total], begin > end or the format has an unknown bit;
  count_mask_words(counts, thresholds, before, mode): the words ess_event_count_mask leaves -- tests/hot_pixel_ref.mask_words_of's
      rule on plain counts (the CPU tier proves the two equal on sums that are counts at scale 2^40).
"""
import numpy as np

T_I64, XY_U16 = 1, 2
REPLACE, OR = 0, 1


def n_words(width):
    return (int(width) + 31) // 32


def decoded(words, xy_u16):
    """a coordinate column's 16-bit words (any 2-byte dtype) -> int64 values: unsigned under XY_U16, else sign-extended"""
    w = np.ascontiguousarray(words)
    return w.view(np.uint16).astype(np.int64) if xy_u16 else w.view(np.int16).astype(np.int64)


def pixel_counts(x_words, y_words, begin, end, fmt, total, H, W):
    out = np.zeros((H, W), dtype=np.int64)
    if (fmt & ~(T_I64 | XY_U16)) != 0 or begin < 0 or begin > end or end > total:
        return out
    x, y = decoded(x_words[begin:end], bool(fmt & XY_U16)), decoded(y_words[begin:end], bool(fmt & XY_U16))
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    np.add.at(out, (y[inside], x[inside]), 1)
    return out


def count_mask_words(counts, thresholds, before, mode):
    """counts: int64 [n, H, W]; thresholds: int64 [n]; before: uint32 [n, H, n_words(W)], the words in front of the call -> behind it"""
    n, H, W = counts.shape
    assert counts.dtype == np.int64 and before.dtype == np.uint32 and before.shape == (n, H, n_words(W))
    out = before.copy()
    for i in range(n):
        if int(thresholds[i]) < 0:
            continue
        hot = np.zeros((H, n_words(W) * 32), dtype=np.uint64)
        hot[:, :W] = counts[i] > int(thresholds[i])
        new = (hot.reshape(H, n_words(W), 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
        out[i] = (new | before[i]) if mode == OR else new
    return out
