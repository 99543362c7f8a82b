"""CPU tier of the device event store (hip.event_scatter_store, hip.event_store_windows, datasets.event_store, EventBatchBuilder(store=)):
the two C entry points, their enumerators and their refusals -- each before a launch --, the classes' refusals -- each before a device
call, the state left as it was --, and the numpy restatement of the window search (tests/event_store_ref.py) proved equal to the host
rules that tests/test_host_sequence_cut.py pins to the reference's lines."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tests import event_store_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_event_scatter_store', 'ess_event_store_windows')
EINVAL = -22


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_two_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert callable(hip.event_scatter_store) and callable(hip.event_store_windows)


def test_the_enumerators_agree_between_the_header_and_the_bindings_and_the_restatement():
    from ess_amd import hip
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    found = {k: int(v) for k, v in re.findall(r'ESS_(EVENT_STORE_[A-Z_]+) = (-?\d+)', header)}
    assert len(found) == 10, found
    for name, value in found.items():
        assert getattr(hip, name) == value, name
    assert (SR.RULE_COUNT_TIME, SR.RULE_COUNT_INDEX, SR.RULE_DURATION) == \
        (hip.EVENT_STORE_RULE_COUNT_TIME, hip.EVENT_STORE_RULE_COUNT_INDEX, hip.EVENT_STORE_RULE_DURATION)
    assert (SR.FLAG_EMPTY, SR.FLAG_OVERFLOW, SR.FLAG_RANGE) == \
        (hip.EVENT_STORE_FLAG_EMPTY, hip.EVENT_STORE_FLAG_OVERFLOW, hip.EVENT_STORE_FLAG_RANGE)
    assert (hip.EVENT_STORE_SIGNED, hip.EVENT_STORE_SEPARATE, hip.EVENT_STORE_HISTOGRAM) == \
        (hip.EVENT_REP_SIGNED, hip.EVENT_REP_SEPARATE, hip.EVENT_REP_HISTOGRAM)
    assert (SR.T_I64, SR.XY_U16) == (hip.EVCOL_T_I64, hip.EVCOL_XY_U16)


# ---------------------------------------------------------------------------------------------- the library's refusals
def test_the_scatter_refuses_bad_arguments_before_any_launch(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced)

    def call(t=one, x=one, y=one, p=one, starts=one, counts=one, formats=one, cap=64, total=60, wcap=16, n=2, C=3, H=4, W=5, acc=one,
             acc_bytes=1 << 20, flavour=0, maps=P(0), map_of=P(0), n_maps=0):
        return L.ess_event_scatter_store(t, x, y, p, starts, counts, formats, cap, total, wcap, n, C, H, W, acc, acc_bytes, flavour, maps,
                                         map_of, n_maps, 1, 1, P(0))
    cases = [(dict(t=P(0)), 'null'), (dict(starts=P(0)), 'null'), (dict(formats=P(0)), 'null'), (dict(acc=P(0)), 'null'),
             (dict(x=P(8)), '16-byte'), (dict(acc=P(24)), '16-byte'), (dict(starts=P(20)), '8-byte'), (dict(counts=P(18)), '4-byte'),
             (dict(wcap=0), 'window_capacity=0'), (dict(wcap=(1 << 22) + 1), 'the int64 sums hold 2^22 contributions'),
             (dict(cap=72, total=0), 'capacity=72'), (dict(cap=0, total=0), 'capacity=0'), (dict(cap=(1 << 40) + 16), 'capacity='),
             (dict(total=65), 'total=65'), (dict(total=-1), 'total=-1'), (dict(n=0), 'n_slots=0'), (dict(n=65536), 'n_slots=65536'),
             (dict(flavour=4), 'flavour=4'), (dict(flavour=-1), 'flavour=-1'), (dict(flavour=1, C=3), 'must be even'),
             (dict(flavour=2, C=3), 'must be 2'), (dict(H=0), 'height=0'), (dict(acc_bytes=2 * 3 * 4 * 5 * 8 - 1), 'are needed'),
             (dict(flavour=3), 'null map_of'), (dict(flavour=3, map_of=one, n_maps=1), 'maps must be null')]
    for kw, msg in cases:
        assert call(**kw) == EINVAL, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert L.ess_last_error().decode().startswith('event_scatter_store:')


def test_the_window_search_refuses_bad_arguments_before_any_launch(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced)

    def call(t=one, cap=64, total=60, table=one, n_rec=2, recording=one, bounds=one, sample_map=P(0), B=2, T=3, rule=0, npw=8, wcap=16,
             starts=one, counts=one, formats=one, map_of=P(0), flags=one):
        return L.ess_event_store_windows(t, cap, total, table, n_rec, recording, bounds, sample_map, B, T, rule, npw, wcap, starts, counts,
                                         formats, map_of, flags, P(0))
    cases = [(dict(t=P(0)), 'null'), (dict(table=P(0)), 'null'), (dict(bounds=P(0)), 'null'), (dict(flags=P(0)), 'null'),
             (dict(sample_map=one), 'both given'), (dict(map_of=one), 'both given'),
             (dict(t=P(8)), '16-byte'), (dict(table=P(20)), '8-byte'), (dict(flags=P(18)), '4-byte'),
             (dict(wcap=0), 'window_capacity=0'), (dict(wcap=(1 << 22) + 1), 'the int64 sums hold 2^22 contributions'),
             (dict(cap=72), 'capacity=72'), (dict(total=65), 'total=65'), (dict(total=-1), 'total=-1'),
             (dict(B=0), 'n_slots=0'), (dict(B=21846), 'n_slots=65538'), (dict(T=0), 'T=0'), (dict(T=-2), 'T=-2'),
             (dict(rule=3), 'rule=3'), (dict(rule=-1), 'rule=-1'), (dict(npw=0), 'n_per_window=0'), (dict(npw=17), 'n_per_window=17'),
             (dict(n_rec=0), 'n_recordings=0')]
    for kw, msg in cases:
        assert call(**kw) == EINVAL, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert L.ess_last_error().decode().startswith('event_store_windows:')


def test_the_wrappers_refuse_on_the_host():
    import torch
    from ess_amd import hip
    cap = 32
    cols = [torch.zeros(cap, dtype=d) for d in (torch.int64, torch.int16, torch.int16, torch.uint8)]
    starts, words = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    acc = torch.zeros(2, 3, 4, 5, dtype=torch.int64)
    ok = dict(flavour=hip.EVENT_STORE_SIGNED, total=20, window_capacity=8)
    for change, msg in ((dict(flavour=7), 'flavour=7'), (dict(total=33), 'total=33'), (dict(window_capacity=0), 'window_capacity=0'),
                        (dict(flavour=hip.EVENT_STORE_HISTOGRAM), 'fills 2 planes'), (dict(maps=torch.zeros(1, 2, 2, 2)), 'maps / map_of belong')):
        with pytest.raises(hip.EssHipError, match=msg):
            hip.event_scatter_store(*cols, starts, words, words, acc, **{**ok, **change})
    with pytest.raises(hip.EssHipError, match=r'starts must be int64 \[2\]'):
        hip.event_scatter_store(*cols, words, words, words, acc, **ok)
    with pytest.raises(hip.EssHipError, match=r't must be \[capacity\]'):
        hip.event_scatter_store(cols[0][:20], *cols[1:], starts, words, words, acc, **ok)
    with pytest.raises(hip.EssHipError, match='no CPU path'):  # (the last check: everything else about the call is fine)
        hip.event_scatter_store(*cols, starts, words, words, acc, **ok)
    table, rec, flags = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    T = 3
    s6, w6 = torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)
    b1, bT = torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, T + 1, dtype=torch.float64)

    def search(rule=hip.EVENT_STORE_RULE_COUNT_TIME, bounds=b1, n_per_window=4, T=T, table=table, **kw):
        return hip.event_store_windows(cols[0], table, rec, bounds, rule, T, s6, w6, w6, flags, 20, 8, n_per_window=n_per_window, **kw)
    for kw, msg in ((dict(rule=5), 'rule=5'), (dict(T=0), 'sequence_steps=0'), (dict(n_per_window=9), 'n_per_window=9'),
                    (dict(n_per_window=None), 'n_per_window=None'), (dict(bounds=bT), r'bounds must be int64 / float64 \[2, 1\]'),
                    (dict(rule=hip.EVENT_STORE_RULE_DURATION, bounds=bT), 'n_per_window belongs to the count rules'),
                    (dict(rule=hip.EVENT_STORE_RULE_DURATION, n_per_window=None), r'\[2, 4\]'),
                    (dict(table=torch.zeros(2, 3, dtype=torch.int64)), 'table must be int64'), (dict(sample_map=rec), 'given together'),
                    (dict(), 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=msg):
            search(**kw)


# ---------------------------------------------------------------------------------------------- the classes
def _columns(t, fmt_u16=False, seed=0):
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(seed)
    n = len(t)
    xy = np.uint16 if fmt_u16 else np.int16
    return EventColumns(np.ascontiguousarray(t), g.integers(0, 8, n).astype(xy), g.integers(0, 8, n).astype(xy), g.integers(0, 2, n).astype(np.uint8))


def _state(store):
    return (store.n_events, store.n_recordings, store.n_labels, [list(r) for r in store._recs], store._dev)


def test_the_classes_import_and_refuse_without_a_device():
    from ess_amd import hip
    from ess_amd.datasets.event_batches import EventBatchBuilder
    from ess_amd.datasets.event_store import EventStore, StoreSample, StoreSampler
    store = EventStore(1000, label_hw=(4, 6), label_capacity=3)
    assert store.capacity == 1008 and store.n_events == 0 and store.n_recordings == 0
    assert store.bytes() == 13 * 1008 + 3 * 24 + 32 * 1024
    before = _state(store)
    up, down = np.arange(10, dtype=np.int64), np.array([0, 1, 2, 5, 4, 6], dtype=np.int64)
    refusals = [
        (lambda: store.add_recording(_columns(down)), 'not non-decreasing'),
        (lambda: store.add_recording(_columns(np.array([0.0, 1.0, np.nan, 3.0]))), 'not non-decreasing'),
        (lambda: store.add_recording([_columns(up), _columns(up - 1)]), 'not non-decreasing'),  # (sorted packets, the second goes back)
        (lambda: store.add_recording([_columns(up), _columns(up.astype(np.float64) + 20)]), 'share one format'),
        (lambda: store.add_recording([_columns(up), _columns(up + 20, fmt_u16=True)]), 'share one format'),
        (lambda: store.add_recording(_columns(np.arange(1009, dtype=np.int64))), 'the store is full'),
        (lambda: store.add_recording(_columns(up), labels=np.zeros((4, 4, 6), np.uint8)), 'label tensor is full'),
        (lambda: store.add_recording(_columns(up), labels=np.zeros((1, 4, 7), np.uint8)), 'labels must be a host uint8'),
        (lambda: store.add_recording(up), 'an EventColumns or a list'),
        (lambda: store.append(0, _columns(up)), 'recording 0 of 0'),
        (lambda: store.extent(0), 'recording 0 of 0'),
    ]
    for call, msg in refusals:
        with pytest.raises(hip.EssHipError, match=msg):
            call()
        assert _state(store) == before, msg
    for kw, msg in ((dict(), 'one of the two'), (dict(t_end=1.0, end=3), 'one of the two'), (dict(t_end=float('nan')), 'finite time'),
                    (dict(end=-1), 'end=-1'), (dict(end=2, label=-1), 'label=-1'), (dict(end=2.5), 'end=2.5')):
        with pytest.raises(hip.EssHipError, match=msg):
            StoreSample(0, **kw)
    s = StoreSample(1, t_end=5.5, label=2, map=0)
    assert (s.recording, s.t_end, s.end, s.label, s.map) == (1, 5.5, None, 2, 0)
    with pytest.raises(AttributeError):
        s.end = 3
    with pytest.raises(hip.EssHipError, match='names recording 1, the store holds 0'):
        StoreSampler(store, 2, [s])
    geo = dict(grid_hw=(8, 8), height=8, width=8, label_hw=(4, 6))
    for kw, msg in ((dict(window_events=5, window_duration=2.0), 'one of the two'), (dict(), 'one of the two'),
                    (dict(window_duration=2.0), 'needs window_capacity'), (dict(window_events=0), 'window_events=0'),
                    (dict(window_events=5, window_capacity=4), 'window_capacity=4')):
        with pytest.raises(hip.EssHipError, match=msg):
            EventBatchBuilder(2, 3, 2, None, store=store, **geo, **kw)
    for kw in (dict(window_events=5), dict(window_duration=2.0), dict(window_capacity=7)):
        with pytest.raises(hip.EssHipError, match='they need store='):
            EventBatchBuilder(2, 3, 2, 64, **geo, **kw)
    with pytest.raises(hip.EssHipError, match='event_capacity=None'):  # (without a store the capacity is needed as before)
        EventBatchBuilder(2, 3, 2, None, **geo)
    with pytest.raises(hip.EssHipError, match='store must be an EventStore'):
        EventBatchBuilder(2, 3, 2, None, store=object(), window_events=5, **geo)


def test_a_store_batch_is_checked_before_anything_is_written():
    """the builder's checks of a batch against a store whose bookkeeping says it holds two recordings and two labels (no device is
    touched: the checks come first, and nothing is allocated by a refused batch)"""
    from ess_amd import hip
    from ess_amd.datasets.event_batches import EventBatchBuilder
    from ess_amd.datasets.event_store import EventStore, StoreSample, StoreSampler
    store = EventStore(1000, label_hw=(4, 6), label_capacity=3)
    store._recs = [[0, 100, 1, 0, 99, 0, 2], [100, 160, 0, 0.5, 9.0, 2, 0]]  # (the bookkeeping alone)
    store.n_events, store.n_labels = 160, 2
    assert store.extent(1) == (100, 160) and store.label_range(0) == (0, 2) and store.format_of(0) == 1 and store.t_offset(1) == 0.5
    bld = EventBatchBuilder(2, 3, 2, None, store=store, window_events=5, grid_hw=(8, 8), height=8, width=8, label_hw=(4, 6))
    S = StoreSample
    for samples, msg in (([S(0, end=5, label=2), S(1, end=5, label=0)], 'label index 2 of the store\'s 2 labels'),
                         ([S(0, end=5), S(2, end=5)], 'names recording 2, the store holds 2'),
                         ([S(0, end=5), S(1, end=61)], 'end=61 of recording 1\'s 60 events'),
                         ([S(0, end=5), S(1, t_end=5.0)], 'one rule per launch'),
                         ([S(0, end=5, label=0), S(1, end=5)], 'a label for every sample'),
                         ([S(0, end=5, map=0), S(1, end=5)], 'map index 0 of the builder\'s 0 rectify_maps'),
                         ([S(0, end=5)], 'a list of batch_size=2 StoreSamples'), ([(None, None), S(0, end=5)], 'StoreSamples')):
        with pytest.raises(hip.EssHipError, match=msg):
            bld.build(samples)
        assert bld._static is None and bld.n_batches == 0 and store._dev is None
    dur = EventBatchBuilder(2, 3, 2, None, store=store, window_duration=2.0, window_capacity=64, grid_hw=(8, 8), height=8, width=8, label_hw=(4, 6))
    with pytest.raises(hip.EssHipError, match='need t_end, not end'):
        dur.build([S(0, end=5), S(1, end=5)])
    rule, bounds, label_of, map_of, p = dur._check_store_samples([S(0, t_end=10.5, label=1), S(1, t_end=8.0, label=0)], None)
    assert rule == hip.EVENT_STORE_RULE_DURATION and label_of == [1, 0] and map_of == [hip.RECTIFY_NONE] * 2
    assert bounds[0] == [5, 7, 9, 11]  # (int64 times: 4.5, 6.5, 8.5, 10.5 raised to the next integers)
    assert np.array(bounds[1], dtype=np.int64).view(np.float64).tolist() == [1.5, 3.5, 5.5, 7.5]  # (float64 times, t_offset 0.5 taken off)
    sampler = StoreSampler(store, 2, [S(0, end=k) for k in range(5)], seed=3)
    first, second = [b for b in sampler], [b for b in sampler]
    assert len(sampler) == 2 and all(len(b) == 2 for b in first) and first != second
    assert len({s.end for b in first for s in b}) == 4
    tail = StoreSampler(store, 2, [S(0, end=k) for k in range(5)], shuffle=False, drop_last=False)
    assert len(tail) == 3 and [[s.end for s in b] for b in tail] == [[0, 1], [2, 3], [4, 0]]


# ---------------------------------------------------------------------------------------------- the restatement against the host rules
def _recording(n, t_i64, seed):
    """n sorted times with runs of equal timestamps -> a numpy column in the recording's own dtype"""
    g = np.random.default_rng(seed)
    steps = g.integers(0, 4, n) * (g.random(n) < 0.6)  # (many zero steps: runs of equal times)
    t = 1000 + np.cumsum(steps)
    return t.astype(np.int64) if t_i64 else t.astype(np.float64) * 0.25


@pytest.mark.parametrize('T', [1, 3, 20])
@pytest.mark.parametrize('t_i64', [True, False], ids=['int64', 'float64'])
def test_the_restatement_equals_the_host_rules(T, t_i64):
    """three recordings laid back to back in one flat column; for bounds before, at, inside and behind each of them -- fractional ones
    on the int64 times too --: the count rule equals sequence_windows(ring_end_index(...), available_from=0) on the recording alone,
    the duration rule sequence_windows_fixed_duration(...) on the recording alone, both shifted by the recording's begin"""
    from ess_amd.datasets import event_feed as F
    from ess_amd.datasets.event_store import duration_bounds, time_bound
    sizes = [1, 67, 400]
    recs = [_recording(n, t_i64, 10 * T + k) for k, n in enumerate(sizes)]
    total = sum(sizes)
    words = np.zeros(-(-total // 16) * 16, np.int64)
    words[:total] = np.concatenate(recs).view(np.int64)
    begins = np.concatenate([[0], np.cumsum(sizes)])
    fmt = SR.T_I64 if t_i64 else 0
    table = np.array([[begins[k], begins[k + 1], fmt, 0] for k in range(3)], dtype=np.int64)
    n_per, wcap = 7, 64
    checked = empty = clamped = 0
    for k, t in enumerate(recs):
        lo, hi = float(t[0]), float(t[-1])
        ends = sorted({lo - 1, lo, lo + 0.5, hi, hi + 0.25, hi + 3, (lo + hi) / 2, float(t[len(t) // 2]), float(t[len(t) // 3]) + 0.125})
        for t_end in ends:
            # -- the count rule, the end found by time
            b = np.array([[time_bound(t_end, t_i64)]], dtype=np.int64)
            got = SR.windows(words, total, table, [k], b, SR.RULE_COUNT_TIME, T, n_per, wcap)
            end = F.ring_end_index(t, len(t), len(t), t_end)
            want = F.sequence_windows(end, 0, T, n_per)
            if want is None:
                assert got[3][0] == SR.FLAG_EMPTY and not got[1].any()
                empty += 1
            else:
                assert got[3][0] == 0 and list(zip((got[0] - begins[k]).tolist(), got[1].tolist())) == want, (k, t_end)
                clamped += want[0][0] == 0 and end < T * n_per
            # -- the same end given as an index
            by_index = SR.windows(words, total, table, [k], np.array([[end]], dtype=np.int64), SR.RULE_COUNT_INDEX, T, n_per, wcap)
            assert all(np.array_equal(a, c) for a, c in zip(got, by_index))
            # -- the duration rule
            d = 2.5 if not t_i64 else 3
            bd = np.array([[time_bound(v, t_i64) for v in duration_bounds(t_end, T, d)]], dtype=np.int64)
            got = SR.windows(words, total, table, [k], bd, SR.RULE_DURATION, T, None, 1 << 20)
            want = F.sequence_windows_fixed_duration(t, len(t), len(t), t_end, T, d)
            assert list(zip((got[0] - begins[k]).tolist(), got[1].tolist())) == want, (k, t_end)
            assert got[3][0] == (0 if any(c for _, c in want) else SR.FLAG_EMPTY)
            assert (got[2] == fmt).all()
            checked += 1
    assert checked >= 20 and empty >= 3 and clamped >= 1  # (a recording of one event has fewer distinct bounds)


def test_the_restatement_flags_by_hand():
    t = np.zeros(32, np.int64)
    t[:20] = np.arange(20)
    table = np.array([[0, 12, 1, 0], [12, 20, 1, 0], [0, 0, -1, 0]], dtype=np.int64)
    dur = np.array([[0, 5, 12]], dtype=np.int64)
    s, c, f, fl = SR.windows(t, 20, table, [0], dur, SR.RULE_DURATION, 2, None, 7)
    assert s.tolist() == [0, 5] and c.tolist() == [5, 7] and fl.tolist() == [0]
    s, c, f, fl = SR.windows(t, 20, table, [0], dur, SR.RULE_DURATION, 2, None, 6)
    assert s.tolist() == [0, 5] and c.tolist() == [0, 0] and fl.tolist() == [SR.FLAG_OVERFLOW]  # (one window too large: ALL counts 0)
    for rec in (3, -1, 2):  # (one past the table, a negative number, an unused row)
        s, c, f, fl = SR.windows(t, 20, table, [rec], dur, SR.RULE_DURATION, 2, None, 7)
        assert not s.any() and not c.any() and fl.tolist() == [SR.FLAG_RANGE]
    s, c, f, fl = SR.windows(t, 20, table, [1, 1], np.array([[9], [-1]], dtype=np.int64), SR.RULE_COUNT_INDEX, 2, 3, 8)
    assert fl.tolist() == [SR.FLAG_RANGE, SR.FLAG_RANGE]  # (e = 9 of a recording of 8 events; e = -1)
    s, c, f, fl = SR.windows(t, 20, table, [1], np.array([[15]], dtype=np.int64), SR.RULE_COUNT_TIME, 2, 3, 8)
    assert s.tolist() == [12, 13] and c.tolist() == [1, 1] and fl.tolist() == [0]  # (e = 15, clamped at begin = 12: 3 events, n = 1)
    s, c, f, fl = SR.windows(t, 20, table, [1], np.array([[13]], dtype=np.int64), SR.RULE_COUNT_TIME, 2, 3, 8)
    assert c.tolist() == [0, 0] and fl.tolist() == [SR.FLAG_EMPTY]  # (one event before e: n = 0)
