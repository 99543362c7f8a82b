"""GPU tier of the device event store: hip.event_store_windows against its numpy restatement (tests/event_store_ref.py) word for word,
hip.event_scatter_store against the ring scatter on the same events bit for bit, and EventBatchBuilder(store=) against the batch
the column path builds from the host slices that datasets.event_feed's rules cut.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import event_store_ref as SR  # noqa: E402
from tests import test_host_event_trilinear as TL  # noqa: E402  (synthetic maps)

DEV = torch.device('cuda:0')
SIZES = [1, 65, 4097, 64, 63, 300001]  # back to back: begins 0, 1, 66, 4163, 4227, 4290 -- all four residues mod 4
RUN = 130                              # events of a run of equal timestamps (more than two waves' 64 probes)
MH, MW = 16, 22                        # the sensor the events lie on
T0_US = 1_600_000_000_000_000


def _times(n, seed, t_i64):
    """n sorted times from one common base (neighbouring recordings OVERLAP in time) with runs of >= RUN equal timestamps at the
    start, in the middle and at the end (where the recording is long enough to hold them apart)"""
    g = np.random.default_rng(seed)
    steps = g.integers(0, 3, n)
    steps[0] = 0
    for a in (0, n // 2, n - RUN):
        if n >= 3 * RUN:
            steps[max(a, 1):a + RUN] = 0
    us = T0_US + 7 * seed + np.cumsum(steps)
    return us.astype(np.int64) if t_i64 else (us - T0_US).astype(np.float64) * 0.125


def _events(t, seed):
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(1000 + seed)
    n = len(t)
    return EventColumns(np.ascontiguousarray(t), g.integers(0, MW, n).astype(np.int16), g.integers(0, MH, n).astype(np.int16),
                        g.integers(0, 2, n).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _store(t_i64):
    """one store of the six recordings, uploaded through staging chunks smaller than the largest -> (store, the recordings' columns)"""
    from ess_amd.datasets import event_store as ES
    cols = [_events(_times(n, k, t_i64), k) for k, n in enumerate(SIZES)]
    store = ES.EventStore(sum(SIZES) + 5, max_recordings=len(SIZES))
    chunk, ES.STAGING_EVENTS = ES.STAGING_EVENTS, 100000
    try:
        for k, c in enumerate(cols):
            packets = c if k != 5 else [ES.EventColumns(c.t[a:b], c.x[a:b], c.y[a:b], c.p[a:b]) for a, b in ((0, 17), (17, 250000), (250000, c.n))]
            assert store.add_recording(packets) == k
    finally:
        ES.STAGING_EVENTS = chunk
    return store, cols


def _flat(cols, capacity):
    t = np.zeros(capacity, np.int64)
    total = sum(c.n for c in cols)
    t[:total] = np.concatenate([c.t.view(np.int64) for c in cols])
    return t, total


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


# ---------------------------------------------------------------------------------------------- 0. the upload
@pytest.mark.parametrize('t_i64', [True, False], ids=['int64', 'float64'])
def test_the_store_holds_the_recordings_bytes_back_to_back(t_i64):
    store, cols = _store(t_i64)
    total = sum(SIZES)
    assert store.n_events == total and store.n_recordings == 6 and store.capacity % 16 == 0 and total % 4 == 3
    begins = np.concatenate([[0], np.cumsum(SIZES)])
    assert sorted({int(b) % 4 for b in begins[:6]}) == [0, 1, 2, 3]
    assert [store.extent(k) for k in range(6)] == [(int(begins[k]), int(begins[k + 1])) for k in range(6)]
    for col, name in zip(store.columns, 'txyp'):
        want = np.concatenate([getattr(c, name).view(col.cpu().numpy().dtype) for c in cols])
        assert np.array_equal(col[:total].cpu().numpy(), want), name
    fmt = 1 if t_i64 else 0
    assert store.table.cpu().tolist() == [[int(begins[k]), int(begins[k + 1]), fmt, 0] for k in range(6)]
    for k in range(5):  # (neighbours overlap in time: a search that left its extent would find a wrong answer)
        assert cols[k + 1].t[0] < cols[k].t[-1] or SIZES[k] == 1


# ---------------------------------------------------------------------------------------------- 1. the search
def _bounds_of(c, t_i64):
    """before the first event, equal to the first, inside the middle run, equal to the last, after the last"""
    from ess_amd.datasets.event_store import time_bound
    step = 1 if t_i64 else 0.125
    t = c.t
    return [time_bound(v, t_i64) for v in (t[0].item() - step, t[0].item(), t[c.n // 2 + min(RUN, c.n) // 2 - (c.n // 2 > 0)].item(),
                                           t[-1].item(), t[-1].item() + step)]


def _search(store, t_i64, rule, T, recording, bounds, n_per, wcap):
    from ess_amd import hip
    B = len(recording)
    fill = lambda n, d: torch.full((n,), 0x7F, dtype=torch.uint8, device=DEV).view(d)  # noqa: E731
    starts, counts, formats, flags = fill(8 * B * T, torch.int64), fill(4 * B * T, torch.int32), fill(4 * B * T, torch.int32), fill(4 * B, torch.int32)
    got = hip.event_store_windows(store.columns[0], store.table, _dev(recording, torch.int32), _dev(bounds, torch.int64), rule, T, starts, counts,
                                  formats, flags, store.n_events, wcap, n_per_window=n_per)
    assert got is flags
    return [v.cpu().numpy() for v in (starts, counts, formats, flags)]


@pytest.mark.parametrize('T', [1, 5, 20])
@pytest.mark.parametrize('t_i64', [True, False], ids=['int64', 'float64'])
def test_the_three_rules_equal_the_restatement_word_for_word(t_i64, T):
    from ess_amd import hip
    store, cols = _store(t_i64)
    t_words, total = _flat(cols, store.capacity)
    table = store.table.cpu().numpy()
    n_per, wcap = 50, 4096
    # -- count, end by time: five bounds a recording, and two recording numbers outside the table
    recording = [k for k in range(6) for _ in range(5)] + [6, -1]
    bounds = [[w] for k in range(6) for w in _bounds_of(cols[k], t_i64)] + [[0], [0]]
    got = _search(store, t_i64, hip.EVENT_STORE_RULE_COUNT_TIME, T, recording, bounds, n_per, wcap)
    want = SR.windows(t_words, total, table, recording, np.array(bounds, dtype=np.int64), SR.RULE_COUNT_TIME, T, n_per, wcap)
    for name, g, w in zip(('starts', 'counts', 'formats', 'flags'), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, 'count by time')
    flags = want[3].reshape(-1)
    assert flags[-2:].tolist() == [SR.FLAG_RANGE] * 2 and flags[0] == SR.FLAG_EMPTY and flags[25] == SR.FLAG_EMPTY and flags[29] == 0
    assert want[0][29 * T] == total - T * n_per and want[1][29 * T] == n_per          # (the last recording's end: a full sample)
    assert want[0][14 * T] == 66 + 4097 - T * n_per and want[1][14 * T] == n_per      # (after the last of 4097 events)
    if T * n_per > 65:                                                                # (65 events: clamped at begin = 1)
        assert want[0][9 * T] == 1 and want[1][9 * T] == 65 // T and 65 // T < n_per
    # -- count, end by index: 0, 1, the middle, the size, and one past it
    recording = [k for k in range(6) for _ in range(5)]
    bounds = [[e] for n in SIZES for e in (0, 1, n // 2, n, n + 1)]
    got = _search(store, t_i64, hip.EVENT_STORE_RULE_COUNT_INDEX, T, recording, bounds, n_per, wcap)
    want = SR.windows(t_words, total, table, recording, np.array(bounds, dtype=np.int64), SR.RULE_COUNT_INDEX, T, n_per, wcap)
    for name, g, w in zip(('starts', 'counts', 'formats', 'flags'), got, want):
        assert np.array_equal(g, w), (name, 'count by index')
    assert want[3][4::5].tolist() == [SR.FLAG_RANGE] * 6 and want[3][0] == SR.FLAG_EMPTY and want[3][28] == 0
    # -- duration: T + 1 bounds between pairs of the five; one window of window_capacity + 1 events; an empty sample
    recording, bounds = [], []
    for k in range(6):
        b = _bounds_of(cols[k], t_i64)
        as_time = (lambda w: w) if t_i64 else (lambda w: np.array([w], np.int64).view(np.float64)[0])
        to_word = (lambda v: int(np.ceil(v))) if t_i64 else (lambda v: int(np.array([v], np.float64).view(np.int64)[0]))
        for lo, hi in ((0, 4), (1, 2), (2, 3), (1, 3), (4, 4)):
            recording.append(k)
            bounds.append([to_word(v) for v in np.linspace(as_time(b[lo]), as_time(b[hi]), T + 1)])
    b = _bounds_of(cols[2], t_i64)
    recording.append(2)
    bounds.append([b[0]] + [b[4]] * T)  # (all 4097 events in window 0, with window_capacity = 4096)
    got = _search(store, t_i64, hip.EVENT_STORE_RULE_DURATION, T, recording, bounds, None, wcap)
    want = SR.windows(t_words, total, table, recording, np.array(bounds, dtype=np.int64), SR.RULE_DURATION, T, None, wcap)
    for name, g, w in zip(('starts', 'counts', 'formats', 'flags'), got, want):
        assert np.array_equal(g, w), (name, 'duration')
    assert want[3][-1] == SR.FLAG_OVERFLOW and not want[1][-T:].any() and want[0][-T] == 66
    assert want[3][4] == SR.FLAG_EMPTY and want[3][24] == SR.FLAG_EMPTY and want[3][20] == 0 and want[1][20 * T:21 * T].sum() == 63
    assert want[3][25] == SR.FLAG_OVERFLOW  # (300 001 events in at most 20 windows)
    assert (want[3] == 0).sum() >= 12 and want[1].max() > 64


# ---------------------------------------------------------------------------------------------- 2. the scatter
FLAVOURS = {'signed': (3, (MH, MW)), 'separate_pol': (6, (MH, MW)), 'histogram': (2, (MH, MW)), 'trilinear': (3, (13, 18))}


@pytest.mark.parametrize('flavour', list(FLAVOURS))
@pytest.mark.parametrize('t_i64', [True, False], ids=['int64', 'float64'])
def test_the_store_scatter_has_the_bits_of_the_ring_scatter(t_i64, flavour):
    from ess_amd import hip
    store, cols = _store(t_i64)
    total, wcap, ring = store.n_events, 1024, 1024
    C, (H, W) = FLAVOURS[flavour]
    fmt = 1 if t_i64 else 0
    # (start, count, format): every start residue with every size; then the edges
    wins = [(4490 + 8 * j + r, n, fmt) for r in range(4) for j, n in enumerate((1, 3, 4, 5, 1000))]
    assert sorted({s % 4 for s, _, _ in wins}) == [0, 1, 2, 3]
    wins += [(total - 7, 7, fmt), (60, 7, fmt)]                          # ends on the store's last event; crosses three recordings
    n_good = len(wins)
    wins += [(100, 0, fmt), (total - 4, 5, fmt), (-3, 5, fmt), (4300, wcap + 1, fmt), (4400, 9, 4), (1 << 33, 5, fmt)]
    n = len(wins)
    flat = [np.concatenate([getattr(c, name) for c in cols]) for name in 'txyp']
    rows = [np.zeros((n, ring), a.dtype) for a in flat]
    ring_counts = []
    for i, (s, c, f) in enumerate(wins):
        good = i < n_good
        ring_counts.append(c if good else 0)
        for row, a in zip(rows, flat):
            if good:
                row[i, :c] = a[s:s + c]
    g = torch.Generator().manual_seed(5)
    pattern = torch.randint(-1 << 30, 1 << 30, (n, C, H, W), generator=g, dtype=torch.int64).to(DEV)
    acc_store, acc_ring = pattern.clone(), pattern.clone()
    words = lambda v: _dev(v, torch.int32)  # noqa: E731
    ring_cols = [_dev(r.view(np.int64) if r.dtype.itemsize == 8 else r) for r in rows]
    ring_words = (words(list(range(n))), words([0] * n), words(ring_counts), words([f for _, _, f in wins]))
    starts, counts, formats = _dev([s for s, _, _ in wins], torch.int64), words([c for _, c, _ in wins]), words([f for _, _, f in wins])
    if flavour == 'trilinear':
        maps = _dev(np.stack([TL.synthetic_map(MH, MW, H, W, 1), TL.synthetic_map(MH, MW, H, W, 2)]))
        map_of = words([(0, 1, hip.RECTIFY_NONE)[i % 3] for i in range(n)])
        hip.event_scatter_ring_trilinear(*ring_cols, *ring_words, acc_ring, maps, map_of)
        got = hip.event_scatter_store(*store.columns, starts, counts, formats, acc_store, hip.EVENT_STORE_TRILINEAR, total, wcap, maps, map_of)
    else:
        rep = hip.EVENT_REPRESENTATIONS[None if flavour == 'signed' else flavour]
        hip.event_scatter_ring_rep(*ring_cols, *ring_words, acc_ring, rep)
        if flavour == 'signed':
            plain = pattern.clone()
            hip.event_scatter_ring(*ring_cols, *ring_words, plain)
            assert torch.equal(plain, acc_ring)
        got = hip.event_scatter_store(*store.columns, starts, counts, formats, acc_store, rep, total, wcap)
    assert got is acc_store
    assert torch.equal(acc_store, acc_ring)
    assert torch.equal(acc_store[n_good:], pattern[n_good:])  # (refused slots and the empty one: their planes as they were)
    moved = (acc_store[:n_good] != pattern[:n_good]).flatten(1).any(1)
    # (the trilinear flavour gives a window whose last time equals its first an all-zero grid: only its long windows must move)
    assert bool(moved[4:20:5].all()) if flavour == 'trilinear' else bool(moved.all())


# ---------------------------------------------------------------------------------------------- 3. the builder
B, T, BINS, N_WIN = 3, 4, 3, 50
GEO = dict(grid_hw=(12, 20), grid_rows=10, grid_resize=(14, 24), height=12, width=24, crop_hw=(8, 16), crop_band=(2, 10), label_hw=(12, 20))
KINDS = {'signed': dict(), 'separate_pol': dict(representation='separate_pol'), 'histogram': dict(representation='histogram'),
         'trilinear': dict(voxel='trilinear')}


@functools.lru_cache(maxsize=None)
def _small_store():
    """five recordings with labels: int64 / float64 / a short one for the count rules (random times), int64 / float64 with evenly
    spaced times for the duration rule (its windows then hold equal counts, which is all the column path can cut)"""
    from ess_amd.datasets.event_store import EventStore
    g = np.random.default_rng(77)
    times = [T0_US + np.cumsum(g.integers(0, 3, 700)), np.cumsum(g.integers(0, 3, 530)) * 0.25, T0_US + np.cumsum(g.integers(0, 3, 40)),
             5000 + np.repeat(np.arange(200), 3), np.repeat(np.arange(200), 2) * 0.5]
    cols = [_events(np.ascontiguousarray(t), 40 + k) for k, t in enumerate(times)]
    offsets = [1000, 0.5, 0, 0, 2.0]
    store = EventStore(sum(c.n for c in cols) + 50, label_hw=GEO['label_hw'], label_capacity=10)
    values = np.array(list(range(19)) + [255], dtype=np.uint8)
    labels = values[g.integers(0, len(values), (10,) + GEO['label_hw'])]
    for k, c in enumerate(cols):
        assert store.add_recording(c, t_offset=offsets[k], labels=labels[2 * k:2 * k + 2]) == k
        assert store.label_range(k) == (2 * k, 2)
    return store, cols, offsets, labels


def _host_slice(cols, t_off, sample, rule_duration, d=None):
    """the events the reference rule cuts for a sample -> an EventColumns of T n events (or none)"""
    from ess_amd.datasets import event_feed as F
    from ess_amd.datasets.data_util import EventColumns
    c = cols[sample.recording]
    if rule_duration:
        w = F.sequence_windows_fixed_duration(c.t, c.n, c.n, sample.t_end - t_off[sample.recording], T, d)
        assert len({n for _, n in w}) == 1  # (equal counts)
        a, b = w[0][0], w[-1][0] + w[-1][1]
    else:
        end = sample.end if sample.end is not None else F.ring_end_index(c.t, c.n, c.n, sample.t_end - t_off[sample.recording])
        w = F.sequence_windows(end, 0, T, N_WIN)
        a, b = (0, 0) if w is None else (w[0][0], w[-1][0] + w[-1][1])
    return EventColumns(c.t[a:b], c.x[a:b], c.y[a:b], c.p[a:b])


def _batches(rule, cols, off):
    """four batches of StoreSamples: the recordings, times and dtypes change from one to the next; sample 2, 1, 0, 2 is empty"""
    from ess_amd.datasets.event_store import StoreSample as S
    if rule == 'duration':
        u, f = cols[3].t, cols[4].t
        return [[S(3, t_end=int(u[300]), label=6), S(4, t_end=float(f[200]) + 2.0, label=8), S(3, t_end=100, label=7)],
                [S(4, t_end=float(f[390]) + 2.0, label=9), S(4, t_end=-50.0, label=8), S(3, t_end=int(u[90]), label=6)],
                [S(3, t_end=-7, label=7), S(3, t_end=int(u[420]), label=7), S(4, t_end=float(f[64]) + 2.0, label=9)],
                [S(4, t_end=float(f[100]) + 2.0, label=8), S(3, t_end=int(u[150]), label=6), S(4, t_end=0.25, label=9)]]
    a, b, c = cols[0].t, cols[1].t, cols[2].t
    by_time = [[S(0, t_end=int(a[650]) + 1000, label=0), S(1, t_end=float(b[300]) + 0.5 + 0.1, label=2), S(2, t_end=int(c[2]), label=4)],
               [S(1, t_end=float(b[529]) + 9.0, label=3), S(0, t_end=int(a[0]) + 1000 - 5, label=1), S(2, t_end=int(c[39]) + 1, label=5)],
               [S(2, t_end=int(c[0]), label=4), S(0, t_end=int(a[120]) + 1000 + 0.5, label=0), S(1, t_end=float(b[210]) + 0.5, label=3)],
               [S(0, t_end=int(a[400]) + 1000, label=1), S(2, t_end=int(c[30]), label=5), S(1, t_end=-3.0, label=2)]]
    if rule == 'time':
        return by_time
    from ess_amd.datasets import event_feed as F
    ends = [[F.ring_end_index(cols[s.recording].t, cols[s.recording].n, cols[s.recording].n, s.t_end - off[s.recording]) for s in batch]
            for batch in by_time]
    return [[S(s.recording, end=e, label=s.label) for s, e in zip(batch, es)] for batch, es in zip(by_time, ends)]


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('rule', ['time', 'index', 'duration'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_a_store_batch_has_the_bits_of_the_column_path(kind, rule, graph):
    from ess_amd import hip
    from ess_amd.datasets.event_batches import EventBatchBuilder
    store, cols, off, labels = _small_store()
    kw = dict(KINDS[kind])
    if kind == 'trilinear':
        kw['rectify_maps'] = [TL.synthetic_map(MH, MW, *GEO['grid_hw'], 1), TL.synthetic_map(MH, MW, *GEO['grid_hw'], 2)]
    common = dict(grid_normalize='unbiased', **GEO, **kw)
    cut = dict(window_duration=4 if rule == 'duration' else None, window_capacity=64 if rule == 'duration' else None,
               window_events=None if rule == 'duration' else N_WIN)
    bld = EventBatchBuilder(B, T, BINS, None, store=store, graph=graph, seed=3, **common, **cut)
    ref = EventBatchBuilder(B, T, BINS, 512, seed=99, **common)
    empties = (2, 1, 0, 2)
    previous = None
    for k, samples in enumerate(_batches(rule, cols, off)):
        if kind == 'trilinear':
            from ess_amd.datasets.event_store import StoreSample as S
            samples = [S(s.recording, t_end=s.t_end, end=s.end, label=s.label, map=(0, None, 1)[(b + k) % 3]) for b, s in enumerate(samples)]
        ev, lab = bld.build(samples)
        p = bld.last_params
        host = []
        for s in samples:
            d = 4 if s.recording == 3 else 4.0
            entry = (_host_slice(cols, off, s, rule == 'duration', d), labels[s.label])
            host.append(entry + (s.map,) if kind == 'trilinear' else entry)
        wev, wlab = ref.build(host, params=p)
        assert torch.equal(ref.last_params, p)
        what = (kind, rule, graph, k)
        assert ev.dtype == torch.float32 and ev.shape == wev.shape and torch.equal(ev.view(torch.int32), wev.view(torch.int32)), what
        assert lab.dtype == torch.int64 and torch.equal(lab, wlab), what
        flags = bld.last_flags.cpu().tolist()
        assert flags == [hip.EVENT_STORE_FLAG_EMPTY if b == empties[k] else 0 for b in range(B)], what
        # (a few events that all count 1 normalise to zero in the histogram: only the full samples must show)
        shows = [b for b in range(B) if b != empties[k] and (kind != 'histogram' or host[b][0].n >= 100)]
        assert not bool(ev[empties[k]].any()) and all(bool(ev[b].any()) for b in shows) and host[empties[k]][0].n == 0, what
        if previous is not None:  # (the batch before stays valid while this one is built)
            assert torch.equal(previous[0].view(torch.int32), previous[1]) and torch.equal(previous[2], previous[3]), what
        previous = (ev, wev.view(torch.int32).clone(), lab, wlab.clone())
    assert bld.n_batches == 4 and bld.n_captures == (2 if graph else 0) and not bool(bld._static['acc'].any())
    assert 'cols' not in bld._static and bld.event_capacity is None
