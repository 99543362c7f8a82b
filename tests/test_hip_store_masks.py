"""GPU tier of hot-pixel masks on the device event store.  hip.event_ingest_store against the parent's entry points on the same events:
hip.event_scatter_store (unmasked, scatter only: the int64 sums), the ring ingests (with out: the fp32 bits), hip.event_ingest_masked
on the ring source and the unmasked ring ingest on moved-away events (tests/hot_pixel_ref.py says which events a mask drops).
hip.event_store_pixel_counts / hip.event_count_mask against the integer restatement (tests/store_mask_ref.py), and
HotPixelMask.from_store against MultiStreamSegmenter.calibrate_hot_pixels on the same events.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hot_pixel_ref as HR  # noqa: E402
from tests import store_mask_ref as MR  # noqa: E402
from tests import test_host_event_trilinear as TL  # noqa: E402  (synthetic maps)

DEV = torch.device('cuda:0')
SH, SW = 37, 70                     # the sensor the events lie on (and around)
SIZES = [4097, 4098, 4099, 4090]    # back to back: begins 0, 4097, 8195, 12294 -- residues 0, 1, 3, 2; total == capacity == 16384
FORMATS = [1, 0, 3, 2]              # int64 / int16, float64 / int16, int64 / uint16, float64 / uint16
RING, WCAP = 1024, 1024


def _recording(k):
    """recording k's events in the dtypes of FORMATS[k]: coordinates on the sensor and a little around it -- negative int16 words,
    uint16 words up to 65535 -- with repeated timestamps"""
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(40 + k)
    n, fmt = SIZES[k], FORMATS[k]
    us = 1_600_000_000_000_000 + np.cumsum(g.integers(0, 3, n))
    t = us.astype(np.int64) if fmt & 1 else (us - us[0]).astype(np.float64) * 0.125
    x, y = g.integers(-2, SW + 2, n), g.integers(-2, SH + 2, n)
    far = g.random(n) < 0.02
    x[far] = -300
    if fmt & 2:
        return EventColumns(t, x.astype(np.int16).view(np.uint16), y.astype(np.int16).view(np.uint16), g.integers(0, 2, n).astype(np.uint8))
    return EventColumns(t, x.astype(np.int16), y.astype(np.int16), g.integers(0, 2, n).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _store():
    """-> (store, the flat columns as raw words: t int64, x / y int16, p uint8)"""
    from ess_amd.datasets.event_store import EventStore
    cols = [_recording(k) for k in range(4)]
    store = EventStore(sum(SIZES), max_recordings=4)
    for k, c in enumerate(cols):
        assert store.add_recording(c) == k and store.format_of(k) == FORMATS[k]
    assert store.n_events == store.capacity == 16384
    flat = [np.concatenate([getattr(c, name).view(d) for c in cols]) for name, d in zip('txyp', (np.int64, np.int16, np.int16, np.uint8))]
    return store, flat


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _windows():
    """(start, count, format) per slot -> (wins, n_good): every residue of the start with several sizes inside each recording, a
    one-event window, a window that ends on event total - 1 == capacity - 1; behind them the slots the store refuses, and an empty one"""
    begins = np.concatenate([[0], np.cumsum(SIZES)])
    wins = [(int(begins[k]) + 200 + 8 * j + r, n, FORMATS[k]) for k in range(4) for r in range(4)
            for j, n in enumerate((1, 5, 1000 - 7 * r))][::2]
    assert sorted({s % 4 for s, _, _ in wins}) == [0, 1, 2, 3] and any(c == 1 for _, c, _ in wins)
    total = int(begins[-1])
    wins += [(total - 7, 7, FORMATS[3]), (total - 1, 1, FORMATS[3])]
    n_good = len(wins)
    wins += [(100, 0, 1), (total - 4, 5, FORMATS[3]), (-3, 5, 1), (300, WCAP + 1, 1), (400, 9, 4), (1 << 33, 5, 1)]
    return wins, n_good


def _ring_of(flat, wins, n_good, hot=None):
    """the windows' events copied to the head of a ring row each -- hot: {slot: bool [count]}, the events whose x is moved outside
    everything (0xffff: -1 as int16, 65535 as uint16) -> (device columns [n, RING], the four ring words)"""
    n = len(wins)
    rows = [np.zeros((n, RING), a.dtype) for a in flat]
    counts = []
    for i, (s, c, _) in enumerate(wins):
        counts.append(c if i < n_good else 0)
        if i < n_good:
            for row, a in zip(rows, flat):
                row[i, :c] = a[s:s + c]
            if hot is not None and i in hot:
                rows[1][i, :c][hot[i]] = -1
    words = lambda v: _dev(v, torch.int32)  # noqa: E731
    return [_dev(r) for r in rows], (words(list(range(n))), words([0] * n), words(counts), words([f for _, _, f in wins]))


FLAVOURS = {'signed': (3, (SH, SW)), 'separate_pol': (6, (SH, SW)), 'histogram': (2, (SH, SW)), 'trilinear': (3, (20, 40))}


def _flavour(hip, flavour, n):
    """-> (planes, (H, W), the store's flavour word, maps, map_of)"""
    C, (H, W) = FLAVOURS[flavour]
    if flavour == 'trilinear':
        maps = _dev(np.stack([TL.synthetic_map(SH, SW, H, W, 1), TL.synthetic_map(SH, SW, H, W, 2)]))
        return C, (H, W), hip.EVENT_STORE_TRILINEAR, maps, _dev([(0, 1, hip.RECTIFY_NONE)[i % 3] for i in range(n)], torch.int32)
    return C, (H, W), hip.EVENT_REPRESENTATIONS[None if flavour == 'signed' else flavour], None, None


# ---------------------------------------------------------------------------------------------- 1. without masks
@pytest.mark.parametrize('flavour', list(FLAVOURS))
def test_without_masks_the_store_ingest_has_the_sums_of_the_store_scatter_and_the_bits_of_the_ring_ingest(flavour):
    from ess_amd import hip
    store, flat = _store()
    wins, n_good = _windows()
    n, total = len(wins), store.n_events
    C, (H, W), word, maps, map_of = _flavour(hip, flavour, n)
    starts, counts, formats = _dev([s for s, _, _ in wins], torch.int64), _dev([c for _, c, _ in wins], torch.int32), \
        _dev([f for _, _, f in wins], torch.int32)
    # -- scatter only, onto a known non-zero pattern: event_scatter_store's sums
    g = torch.Generator().manual_seed(5)
    pattern = torch.randint(-1 << 30, 1 << 30, (n, C, H, W), generator=g, dtype=torch.int64).to(DEV)
    want, got = pattern.clone(), pattern.clone()
    hip.event_scatter_store(*store.columns, starts, counts, formats, want, word, total, WCAP, maps, map_of)
    back = hip.event_ingest_store(*store.columns, starts, counts, formats, None, word, total, WCAP, maps=maps, map_of=map_of, acc=got)
    assert back is got and torch.equal(got, want)
    assert torch.equal(got[n_good:], pattern[n_good:])  # (refused slots and the empty one: their planes as they were)
    moved = (got[:n_good] != pattern[:n_good]).flatten(1).any(1)
    big = torch.tensor([c >= 5 for _, c, _ in wins[:n_good]], device=DEV)  # (a window of one event may lie outside the grid)
    assert bool(moved[big].all()) if flavour != 'trilinear' else bool(moved[2::3].any())
    # -- with out: the ring ingest's bits on the same events, acc all zero again
    ring_cols, ring_words = _ring_of(flat, wins, n_good)
    out_ring = torch.full((n, C, H, W), 7.0, device=DEV)
    out_store, acc = out_ring.clone(), torch.zeros(n, C, H, W, dtype=torch.int64, device=DEV)
    if flavour == 'trilinear':
        hip.event_ingest_ring_trilinear(*ring_cols, *ring_words, out_ring, maps, map_of)
    elif flavour == 'signed':
        hip.event_ingest_ring(*ring_cols, *ring_words, out_ring)
    else:
        hip.event_ingest_ring_rep(*ring_cols, *ring_words, out_ring, word)
    back = hip.event_ingest_store(*store.columns, starts, counts, formats, out_store, word, total, WCAP, maps=maps, map_of=map_of, acc=acc)
    assert back is out_store and torch.equal(_bits(out_store), _bits(out_ring))
    assert not bool(acc.any()) and not bool(out_store[n_good:].any()) and bool(out_store[:n_good].any())


# ---------------------------------------------------------------------------------------------- 2. with masks
MASK_SIZES = [(SH, 31), (SH, 32), (10, 33), (SH + 3, 64), (SH, 65), (SH + 3, SW + 9)]  # smaller and larger than the grids (20 x 40, 37 x 70)


def _masks(flat, wins, n_good, mh, mw, seed):
    """two masks of mh x mw: a third of the pixels at random, plus the raw pixel of the FIRST and of the LAST event of every window
    (where it lies inside the mask) -- the time base must not move when they are dropped"""
    g = np.random.default_rng(seed)
    words = []
    for k in range(2):
        b = g.random((mh, mw)) < 0.33
        for s, c, f in wins[:n_good]:
            for e in (s, s + c - 1):
                x, y = (int(MR.decoded(flat[j][e:e + 1], bool(f & 2))[0]) for j in (1, 2))
                if 0 <= x < mw and 0 <= y < mh:
                    b[y, x] = True
        ys, xs = np.nonzero(b)
        words.append(HR.words_of_locations(list(zip(xs.tolist(), ys.tolist())), mh, mw))
    return np.stack(words)


class _Window:
    """a window's coordinate words in the dtype its format reads them in (what tests/hot_pixel_ref.masked decodes)"""

    def __init__(self, flat, s, c, f):
        d = np.uint16 if f & 2 else np.int16
        self.t, self.x, self.y, self.p = flat[0][s:s + c], flat[1][s:s + c].view(d), flat[2][s:s + c].view(d), flat[3][s:s + c]


@pytest.mark.parametrize('flavour', list(FLAVOURS))
def test_with_masks_the_store_ingest_has_the_bits_of_the_masked_ring_ingest_and_of_the_restatement(flavour):
    from ess_amd import hip
    store, flat = _store()
    wins, n_good = _windows()
    n, total = len(wins), store.n_events
    C, (H, W), word, maps, map_of = _flavour(hip, flavour, n)
    tri = flavour == 'trilinear'
    starts, counts, formats = _dev([s for s, _, _ in wins], torch.int64), _dev([c for _, c, _ in wins], torch.int32), \
        _dev([f for _, _, f in wins], torch.int32)
    ring_cols, ring_words = _ring_of(flat, wins, n_good)
    # slot i reads: no mask, mask 0, mask 1, and -- every seventh -- the word n_masks, which no mask answers to
    mask_words = [(hip.MASK_NONE, 0, 1)[i % 3] if i % 7 != 6 else 2 for i in range(n)]
    assert {hip.MASK_NONE, 0, 1, 2} == set(mask_words[:n_good])
    mask_of = _dev(mask_words, torch.int32)
    g = torch.Generator().manual_seed(6)
    pattern = torch.randint(-1 << 30, 1 << 30, (n, C, H, W), generator=g, dtype=torch.int64).to(DEV)
    dropped = hot_ends = 0
    for seed, (mh, mw) in enumerate(MASK_SIZES):
        host = _masks(flat, wins, n_good, mh, mw, seed)
        masks = _dev(host.view(np.int32))
        # the restatement: the windows with every dropped event's x moved outside everything, through the UNMASKED ring ingest; a slot
        # whose mask word is unknown counts as empty
        live, hot_of = [], {}
        for i, (s, c, f) in enumerate(wins[:n_good]):
            if mask_words[i] in (0, 1):
                hot = hot_of[i] = HR.masked(_Window(flat, s, c, f), host[mask_words[i]], mh, mw)
                dropped += int(hot.sum())
                hot_ends += int(hot[0]) + int(hot[-1])
            live.append(mask_words[i] != 2)
        moved_cols, _ = _ring_of(flat, wins, n_good, hot_of)
        ref_counts = ring_words[2].clone()
        ref_counts[:n_good][~torch.tensor(live, device=DEV)] = 0
        ref_words = ring_words[:2] + (ref_counts,) + ring_words[3:]
        want = torch.full((n, C, H, W), 7.0, device=DEV)
        if tri:
            hip.event_ingest_ring_trilinear(*moved_cols, *ref_words, want, maps, map_of)
        elif flavour == 'signed':
            hip.event_ingest_ring(*moved_cols, *ref_words, want)
        else:
            hip.event_ingest_ring_rep(*moved_cols, *ref_words, want, word)
        kw = dict(masks=masks, mask_of=mask_of, mask_size=(mh, mw), maps=maps, map_of=map_of)
        # -- the first half alone, onto the pattern: the masked ring scatter's sums; the slots of the unknown word as they were
        acc_ring, acc_store = pattern.clone(), pattern.clone()
        hip.event_ingest_masked(*ring_cols, *ring_words, None, representation=0 if tri else word, trilinear=tri, acc=acc_ring, **kw)
        back = hip.event_ingest_store(*store.columns, starts, counts, formats, None, word, total, WCAP, acc=acc_store, **kw)
        assert back is acc_store and torch.equal(acc_store, acc_ring), (mh, mw)
        for i in range(n):
            if i >= n_good or not live[i]:
                assert torch.equal(acc_store[i], pattern[i]), (mh, mw, i)
        # -- both halves: the masked ring ingest's bits, which are the restatement's
        out_ring, out_store = torch.full_like(want, 7.0), torch.full_like(want, 7.0)
        acc = torch.zeros(n, C, H, W, dtype=torch.int64, device=DEV)
        hip.event_ingest_masked(*ring_cols, *ring_words, out_ring, representation=0 if tri else word, trilinear=tri, **kw)
        hip.event_ingest_store(*store.columns, starts, counts, formats, out_store, word, total, WCAP, acc=acc, **kw)
        assert torch.equal(_bits(out_store), _bits(out_ring)), (mh, mw)
        assert torch.equal(_bits(out_store), _bits(want)), (mh, mw)
        assert not bool(acc.any())
    assert dropped > 2000 and hot_ends > 20  # (over the six mask sizes)
    # no mask tensor at all, every word MASK_NONE: event_scatter_store's sums (and a word that names a mask then names none: empty)
    none = _dev([hip.MASK_NONE] * n, torch.int32)
    a, b = pattern.clone(), pattern.clone()
    hip.event_scatter_store(*store.columns, starts, counts, formats, a, word, total, WCAP, maps, map_of)
    hip.event_ingest_store(*store.columns, starts, counts, formats, None, word, total, WCAP, mask_of=none, maps=maps, map_of=map_of, acc=b)
    assert torch.equal(a, b)
    b = pattern.clone()
    hip.event_ingest_store(*store.columns, starts, counts, formats, None, word, total, WCAP, mask_of=none * 0, maps=maps, map_of=map_of, acc=b)
    assert torch.equal(b, pattern)


# ---------------------------------------------------------------------------------------------- 3. counts and count masks
def _jobs():
    total = sum(SIZES)
    jobs = [(4097 + r, 4097 + r + n, f) for r in range(4) for n, f in ((0, 0), (1, 2), (999, 0), (4001 - r, 2))]
    jobs += [(0, total, 0), (0, total, 2), (8000, 12000, 1), (9000, 13000, 3)]  # the whole store; two overlapping ranges
    n_good = len(jobs)
    jobs += [(-1, 50, 0), (5, total + 1, 0), (60, 59, 0), (10, 500, 4), (1 << 35, (1 << 35) + 9, 0)]
    return jobs, n_good


def test_pixel_counts_and_count_masks_equal_the_restatement():
    from ess_amd import hip
    store, flat = _store()
    jobs, n_good = _jobs()
    n, total = len(jobs), store.n_events
    g = torch.Generator().manual_seed(9)
    before = torch.randint(0, 5, (n, SH, SW), generator=g, dtype=torch.int64)
    counts = before.to(DEV)
    begins, ends, fmts = (_dev([j[k] for j in jobs], d) for k, d in ((0, torch.int64), (1, torch.int64), (2, torch.int32)))
    back = hip.event_store_pixel_counts(store.columns[1], store.columns[2], begins, ends, fmts, counts, total)
    assert back is counts
    want = before.numpy().copy()
    for i, (b, e, f) in enumerate(jobs):
        add = MR.pixel_counts(flat[1], flat[2], b, e, f, total, SH, SW)
        assert not (i >= n_good or e == b) or not add.any(), i
        if i < n_good:  # (np.add.at on the decoded coordinates, said once more without the restatement's refusals)
            x, y = MR.decoded(flat[1][b:e], bool(f & 2)), MR.decoded(flat[2][b:e], bool(f & 2))
            ok = (x >= 0) & (x < SW) & (y >= 0) & (y < SH)
            direct = np.zeros((SH, SW), np.int64)
            np.add.at(direct, (y[ok], x[ok]), 1)
            assert np.array_equal(add, direct) and (e - b == 0 or direct.sum() < e - b or e - b == 1)
        want[i] += add
    assert np.array_equal(counts.cpu().numpy(), want)
    # the masks, in both modes, onto words that are there; a negative threshold leaves its words alone
    plain = torch.from_numpy(want - before.numpy()).to(DEV)
    thresholds = np.array([(-1, 0, 1, 3)[i % 4] for i in range(n)], np.int64)
    thresholds[n_good - 4:n_good] = (40, 41, -3, 2)
    old = np.random.default_rng(2).integers(0, 1 << 32, (n, SH, MR.n_words(SW)), dtype=np.uint64).astype(np.uint32)
    for mode in (hip.MASK_REPLACE, hip.MASK_OR):
        words = _dev(old.view(np.int32))
        assert hip.event_count_mask(plain, _dev(thresholds), words, mode) is words
        got = words.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, MR.count_mask_words(plain.cpu().numpy(), thresholds, old, mode)), mode
        assert np.array_equal(got[thresholds < 0], old[thresholds < 0]) and (got[thresholds >= 0] != old[thresholds >= 0]).any()


def test_one_pixel_holds_more_events_than_the_histogram_sums_can():
    """2^22 + 5 events on pixel (5, 3) of the store (the columns are filled on the device): the plain count is exact, and the mask
    rule tells 2^22 + 4 from 2^22 + 5.  At 2^40 an event the histogram flavour's int64 sum would have left its range."""
    from ess_amd import hip
    n = (1 << 22) + 5
    cap = hip.event_column_stride(n + 3)
    x, y = torch.full((cap,), 5, dtype=torch.int16, device=DEV), torch.full((cap,), 3, dtype=torch.int16, device=DEV)
    begins, ends, fmts = _dev([3, 3], torch.int64), _dev([3 + n, 3 + n - 1], torch.int64), _dev([0, 2], torch.int32)
    counts = torch.zeros(2, SH, SW, dtype=torch.int64, device=DEV)
    hip.event_store_pixel_counts(x, y, begins, ends, fmts, counts, n + 3)
    assert counts[:, 3, 5].tolist() == [n, n - 1] and int(counts.sum()) == 2 * n - 1
    words = torch.zeros(2, SH, MR.n_words(SW), dtype=torch.int32, device=DEV)
    hip.event_count_mask(counts, _dev([n - 1, n - 1], torch.int64), words)
    assert words[:, 3, 0].tolist() == [1 << 5, 0] and int((words != 0).sum()) == 1


# ---------------------------------------------------------------------------------------------- 4. calibration from a stored recording
def test_from_store_equals_the_ring_calibration_on_the_same_events():
    """the packets of tests/test_hip_hot_pixels.py's calibration test, fed to a MultiStreamSegmenter's rings and uploaded as three
    recordings of a store: the same masks under the count rule and under the rate rule, in all three formats"""
    from ess_amd.datasets.event_store import EventStore
    from ess_amd.datasets.hot_pixels import HotPixelMask
    from tests import test_hip_hot_pixels as HPT
    S, k = 3, 3
    with HPT.SQ._Pinned('mixed'):
        seg = HPT.SC._segmenter('convlstm', S, hot_pixel_masks=[None] * S, graph=False, event_capacity=HPT.CAP, event_layout='ring',
                                ring_capacity=HPT.RCAP, window_events=HPT.WIN)
        seg.warm_up()
        packets = [HPT._calibration_packet(s, (3, 0, 1)[s], k) for s in range(S)]
        store = EventStore(3 * HPT.WIN + 40)
        store.add_recording(packets[2][0])  # (the store's order of recordings is its own)
        rec_of = [1, 2, 0]
        for s in (0, 1):
            store.add_recording(packets[s][0])
        for s, (c, _) in enumerate(packets):
            seg.feed(s, c)
        size = (HPT.SH_, HPT.SW_)
        state = (store.n_events, [list(r) for r in store._recs], [c.clone() for c in store.columns])
        ring = seg.calibrate_hot_pixels(max_events_per_pixel=k)
        for s, (c, hot) in enumerate(packets):
            got = HotPixelMask.from_store(store, rec_of[s], size=size, max_events_per_pixel=k)
            assert got == ring[s] and got.to_locations().tolist() == [list(v) for v in sorted(hot, key=lambda v: (v[1], v[0]))], s
            # by rate, in the unit of the recording's t: floor(rate * (t_last - t_first)) == k, and one step below it
            span = float(c.t[-1]) - float(c.t[0])
            for limit in ((k + 0.5) / span, (k - 0.5) / span):
                by_rate = seg.calibrate_hot_pixels(streams=[s], max_rate_hz=limit)[0]
                assert HotPixelMask.from_store(store, rec_of[s], size=size, max_rate_hz=limit) == by_rate, (s, limit)
            assert by_rate.count() > 3  # (k - 1: the hundred pixels with exactly k events are hot too)
            # a part of the recording: the restatement on those events
            b, e = 37, HPT.WIN - 11
            part = HotPixelMask.from_store(store, rec_of[s], size=size, max_events_per_pixel=1, begin=b, end=e)
            raw = [getattr(c, name)[b:e] for name in 'xy']
            plain = MR.pixel_counts(raw[0], raw[1], 0, e - b, c.format, e - b, *size)
            assert np.array_equal(part.to_bool(), plain > 1) and part.count() > 3
        assert HotPixelMask.from_store(store, 0, size=size, max_events_per_pixel=0, begin=5, end=5).count() == 0
        assert (store.n_events, [list(r) for r in store._recs]) == state[:2]
        assert all(torch.equal(a, b) for a, b in zip(store.columns, state[2]))
