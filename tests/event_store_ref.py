"""A numpy restatement of hip.event_store_windows: the three rules of include/ess_hip.h, one sample at a time, with
np.searchsorted in the column's own type as the search.  The CPU tier (tests/test_host_event_store.py) proves it equal to
datasets.event_feed's host rules -- sequence_windows(ring_end_index(...)) and sequence_windows_fixed_duration(...) --, the GPU tier
(tests/test_hip_event_store.py) holds the kernel to it word for word."""
import numpy as np

T_I64, XY_U16 = 1, 2
RULE_COUNT_TIME, RULE_COUNT_INDEX, RULE_DURATION = 0, 1, 2
FLAG_EMPTY, FLAG_OVERFLOW, FLAG_RANGE = 1, 2, 4


def first_at_or_after(t_words, begin, end, word, t_i64):
    """the first index in [begin, end) with t >= bound, end where there is none; t_words: the store's time column as int64 words"""
    seg = t_words[begin:end]
    if t_i64:
        return begin + int(np.searchsorted(seg, np.int64(word), side='left'))
    return begin + int(np.searchsorted(seg.view(np.float64), np.array([word], dtype=np.int64).view(np.float64)[0], side='left'))


def windows(t_words, total, table, recording, bounds, rule, T, n_per_window, window_capacity):
    """t_words: int64 [capacity]; table: int64 [n_recordings, 4] (begin, end, format, reserved); recording: [B]; bounds: int64 words
    [B, 1] or [B, T + 1] -> (starts int64 [B T], counts int32 [B T], formats int32 [B T], flags int32 [B])"""
    B = len(recording)
    starts, counts = np.zeros(B * T, np.int64), np.zeros(B * T, np.int32)
    formats, flags = np.zeros(B * T, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        s = slice(b * T, (b + 1) * T)
        rec = int(recording[b])
        fine = 0 <= rec < len(table)
        if fine:
            begin, end, fmt = (int(v) for v in table[rec][:3])
            fine = fmt >= 0 and (fmt & ~(T_I64 | XY_U16)) == 0 and 0 <= begin <= end <= total
        if fine and rule == RULE_COUNT_INDEX:
            fine = 0 <= int(bounds[b][0]) <= end - begin
        if not fine:
            flags[b] = FLAG_RANGE
            continue
        t_i64 = bool(fmt & T_I64)
        formats[s] = fmt
        if rule == RULE_DURATION:
            idx = [first_at_or_after(t_words, begin, end, int(w), t_i64) for w in bounds[b][:T + 1]]
            c = np.diff(np.array(idx, dtype=np.int64))
            starts[s] = idx[:T]
            if (c < 0).any():
                flags[b] = FLAG_RANGE
            elif (c > window_capacity).any():
                flags[b] = FLAG_OVERFLOW
            elif not (c > 0).any():
                flags[b] = FLAG_EMPTY
            if not flags[b] & (FLAG_RANGE | FLAG_OVERFLOW):
                counts[s] = c
            continue
        e = begin + int(bounds[b][0]) if rule == RULE_COUNT_INDEX else first_at_or_after(t_words, begin, end, int(bounds[b][0]), t_i64)
        start = max(begin, e - T * n_per_window)
        n = (e - start) // T
        flags[b] = FLAG_EMPTY if n == 0 else (FLAG_OVERFLOW if n > window_capacity else 0)
        starts[s] = start + np.arange(T, dtype=np.int64) * n
        counts[s] = 0 if flags[b] else n
    return starts, counts, formats, flags
