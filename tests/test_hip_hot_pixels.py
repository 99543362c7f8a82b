"""GPU tier of the hot-pixel masks: hip.event_ingest_masked against the EXISTING unmasked entry points run on columns in which every
masked event was moved outside every grid and map (tests/hot_pixel_ref.py says which events those are) -- bits, for both sources,
every flavour and both halves --, against the reference's zeroing of the finished grid, hip.event_hot_pixel_mask against the integer
restatement, and the two segmenters with hot_pixel_masks= against segmenters without, fed the moved-away events."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hot_pixel_ref as HP  # noqa: E402
from tests import test_hip_event_columns as C  # noqa: E402  (bits, words, guards, result rows)
from tests import test_hip_event_ring as RG  # noqa: E402  (slices of EventColumns)
from tests import test_hip_event_trilinear as TT  # noqa: E402  (device columns / rings with landing filler, the small rig)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers, models, result rows)
from tests import test_hip_sequence_segmenter as SQ  # noqa: E402  (the pins)
from tests import test_hip_seg_head as SH  # noqa: E402  (palette)
from tests import test_hip_stream_compaction as SC  # noqa: E402  (the 64 x 96 models)
from tests import test_host_event_trilinear as T  # noqa: E402  (synthetic maps, raw events)

DEV = M.DEV
_bits, _words = C._bits, C._words
GH, GW, MH, MW, RING = 5, 70, 7, 70, 2048  # the grid; the sensor: three words a row, 32 + 32 + 6 bits, two rows below the grid
HOT_X = (0, 31, 32, 63, 64, 69)
FLAVOURS = {'signed': (0, 5), 'separate_pol': (1, 4), 'histogram': (2, 2), 'trilinear': (0, 5), 'trilinear_map': (0, 5)}  # word, planes
SOURCES = ('columns', 'ring_residue_3', 'ring_wrapped')
SLOT_MASKS = (0, 1, -1, 2)
SLOT_EVENTS = (1500, 1999, 800, 1203)
STARTS = {'ring_residue_3': (3, 7, 11, 15), 'ring_wrapped': (RING - 50, RING - 49, RING - 700, RING - 3)}


def _locations(k, mh=MH):
    """mask k: the six word-edge columns, each in another row, and -- mh = 7 -- two pixels of row 6, below the grid"""
    loc = [(x, (k + i) % 5) for i, x in enumerate(HOT_X)]
    return loc + ([(HOT_X[k], 6), (HOT_X[k + 3], 6)] if mh > 6 else [])


@functools.lru_cache(maxsize=None)
def _mask_words(mh=MH):
    return np.stack([HP.words_of_locations(_locations(k, mh), mh, MW) for k in range(3)])


def _window(n, fmt, loc, seed, mh=MH, mw=MW, share=0.25, t_span_us=50_000):
    """n raw events in the dtypes of format fmt: about `share` of them -- the FIRST and the LAST among them -- on the pixels loc, the
    others anywhere on the sensor (rows 5 - 6 included); 3 % of those outside it: negative int16 words, uint16 words >= 32768"""
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(seed)
    base = T.raw_events(n, mh, mw, seed, fmt=fmt, t_span_us=t_span_us)
    x, y = base.x.astype(np.int64), base.y.astype(np.int64)
    out = g.random(n) < 0.03
    far = np.array([-3, -32768, -1] if not fmt & 2 else [40000, 65535, 32768])
    x = np.where(out, g.choice(far, n), x)
    y = np.where(g.random(n) < 0.01, g.choice(far, n), y)
    hot = g.random(n) < share - 0.02
    hot[0] = hot[-1] = True
    at = np.array(loc)[g.integers(0, len(loc), n)]
    x, y = np.where(hot, at[:, 0], x), np.where(hot, at[:, 1], y)
    xy = np.uint16 if fmt & 2 else np.int16
    return EventColumns(base.t, x.astype(xy), y.astype(xy), base.p)


@functools.lru_cache(maxsize=None)
def _wins(mh=MH):
    """the four slots' windows (formats 0 .. 3), the hot flags of each by the restatement, and the moved-away windows"""
    from ess_amd.datasets.data_util import EventColumns
    words = _mask_words(mh)
    wins = [_window(n, fmt, _locations(max(k, 0), mh), 40 + fmt) for fmt, (n, k) in enumerate(zip(SLOT_EVENTS, SLOT_MASKS))]
    hot = [HP.masked(c, None if k < 0 else words[k], mh, MW) for c, k in zip(wins, SLOT_MASKS)]
    moved = [EventColumns(*HP.moved_away(c, h)) for c, h in zip(wins, hot)]
    return wins, hot, moved


def test_the_inputs_are_what_the_tests_need():
    wins, hot, moved = _wins()
    assert [c.format for c in wins] == [0, 1, 2, 3]
    for c, h, k in zip(wins, hot, SLOT_MASKS):
        if k < 0:
            assert not h.any()
            continue
        assert 0.20 <= h.mean() <= 0.30, h.mean()  # 20 - 30 % of a masked slot's events are hot ...
        assert h[0] and h[-1]                      # ... the window's first and last among them: the time-base rule
        x, y = c.x.astype(np.int64), c.y.astype(np.int64)
        assert ((y >= 5) & (y < 7) & (x >= 0) & (x < MW)).any() and (h & (y == 6)).any()  # sensor rows below the grid, hot ones too
        assert (x < 0).any() if c.x.dtype == np.int16 else (x >= 32768).any()
        assert {int(v) for v in x[h]} == {xx for xx, _ in _locations(k)}  # every word edge of the mask is hit
    for c, m, h in zip(wins, moved, hot):
        assert np.array_equal(c.t, m.t) and np.array_equal(c.x[~h], m.x[~h]) and (m.x[h].astype(np.int64) & 0xFFFF == 0xFFFF).all()


@functools.lru_cache(maxsize=None)
def _maps():
    return np.stack([T.synthetic_map(MH, MW, GH, GW, 1), T.synthetic_map(MH, MW, GH, GW, 2)])


def _device(source, wins, starts=None, ring=RING):
    if source == 'columns':
        return TT._dev_columns(wins, ring), None, None
    starts = STARTS[source] if starts is None else starts
    return TT._dev_rings(wins, starts, ring), _words(list(range(len(wins)))), _words(list(starts))


def _rectify(flavour):
    """-> (maps on the device or None, map words or None)"""
    if flavour == 'trilinear_map':
        return torch.from_numpy(_maps()).to(DEV), _words([0, 1, T.NONE, 0])
    return None, None


def _masked(source, flavour, wins, mask_of, scatter_only, masks=None, mask_size=(MH, MW), counts=None, starts=None, ring=RING, shape=(GH, GW)):
    """hip.event_ingest_masked -> (out inside its NaN-pre-filled guarded buffer, the buffer, acc); scatter_only: (None, None, acc)"""
    from ess_amd import hip
    rep, planes = FLAVOURS[flavour]
    n = len(wins)
    dev, rows, st = _device(source, wins, starts, ring)
    maps, map_of = _rectify(flavour)
    if map_of is not None:
        map_of = map_of[:n].contiguous()
    masks = torch.from_numpy(_mask_words(mask_size[0]).view(np.int32)).to(DEV) if masks is None else masks
    cnt = _words([c.n for c in wins] if counts is None else counts)
    kw = dict(representation=rep, trilinear=flavour.startswith('trilinear'), maps=maps, map_of=map_of)
    args = (*dev, rows, st, cnt, _words([c.format for c in wins]))
    if scatter_only:
        acc = torch.zeros(n, planes, *shape, dtype=torch.int64, device=DEV)
        assert hip.event_ingest_masked(*args, None, masks, _words(mask_of), mask_size, acc=acc, **kw) is acc
        return None, None, acc
    buf, out = M._guarded((n, planes, *shape), torch.float32)
    acc = torch.zeros(n * planes * shape[0] * shape[1], dtype=torch.int64, device=DEV)
    assert hip.event_ingest_masked(*args, out, masks, _words(mask_of), mask_size, acc=acc, **kw) is out
    return out, buf, acc


def _unmasked(source, flavour, wins, scatter_only, counts=None, starts=None, ring=RING, shape=(GH, GW)):
    """the EXISTING entry point of that source and flavour on the same layout -> out (or, scatter_only, the sums a ring scatter leaves:
    the column source is the ring source with slot s's window at the head of row s)"""
    from ess_amd import hip
    rep, planes = FLAVOURS[flavour]
    n = len(wins)
    dev, rows, st = _device(source, wins, starts, ring)
    maps, map_of = _rectify(flavour)
    if map_of is not None:
        map_of = map_of[:n].contiguous()
    cnt, fmts = _words([c.n for c in wins] if counts is None else counts), _words([c.format for c in wins])
    tri = flavour.startswith('trilinear')
    if scatter_only:
        acc = torch.zeros(n, planes, *shape, dtype=torch.int64, device=DEV)
        if rows is None:
            rows, st = _words(list(range(n))), _words([0] * n)
        if tri:
            return hip.event_scatter_ring_trilinear(*dev, rows, st, cnt, fmts, acc, maps, map_of)
        if rep:
            return hip.event_scatter_ring_rep(*dev, rows, st, cnt, fmts, acc, rep)
        return hip.event_scatter_ring(*dev, rows, st, cnt, fmts, acc)
    out = torch.full((n, planes, *shape), float('nan'), device=DEV)
    if rows is None:
        if tri:
            return hip.event_ingest_columns_trilinear(*dev, cnt, fmts, out, maps, map_of)
        return hip.event_ingest_columns_rep(*dev, cnt, fmts, out, rep) if rep else hip.event_ingest_columns(*dev, cnt, fmts, out)
    if tri:
        return hip.event_ingest_ring_trilinear(*dev, rows, st, cnt, fmts, out, maps, map_of)
    return hip.event_ingest_ring_rep(*dev, rows, st, cnt, fmts, out, rep) if rep else hip.event_ingest_ring(*dev, rows, st, cnt, fmts, out)


# ---------------------------------------------------------------------------------------------- 1. masked equals moved away
@pytest.mark.parametrize('source', SOURCES)
@pytest.mark.parametrize('flavour', list(FLAVOURS))
def test_masked_equals_the_unmasked_entry_point_on_moved_away_events(flavour, source):
    """four slots with masks 0, 1, none, 2 of the 7 x 70 sensor over the 5 x 70 grid: the grids (out, NaN before) and the sums
    (out=None) have the bits the existing entry point gives when every masked event's x is -1 / 65535 -- the event keeps its place, so
    the time base is the one that counts hot events.  A mask applied behind the flavour (trilinear + map), a time base from the
    survivors, an ignored mask_of or a mis-indexed third word all show here."""
    wins, hot, moved = _wins()
    if source != 'columns':
        assert all(s % 4 == 3 for s in STARTS['ring_residue_3']) and all(s + n > RING for s, n in zip(STARTS['ring_wrapped'], SLOT_EVENTS))
    out, buf, acc = _masked(source, flavour, wins, SLOT_MASKS, False)
    want = _unmasked(source, flavour, moved, False)
    plain = _unmasked(source, flavour, wins, False)
    for i, k in enumerate(SLOT_MASKS):
        assert torch.equal(_bits(out[i]), _bits(want[i])), f'{flavour} {source}: slot {i} (mask {k})'
        assert bool(out[i].any()) and not bool(torch.isnan(out[i]).any())
        assert torch.equal(_bits(out[i]), _bits(plain[i])) == (k < 0), f'slot {i}: a mask that does nothing, or one where none is named'
    assert C._guards_intact(buf, out) and not bool(acc.any())  # acc: zero on entry, all zero behind the finish
    _, _, sums = _masked(source, flavour, wins, SLOT_MASKS, True)
    want_sums = _unmasked(source, flavour, moved, True)
    assert torch.equal(sums, want_sums) and bool(sums.any())
    assert not torch.equal(sums, _unmasked(source, flavour, wins, True))


# ---------------------------------------------------------------------------------------------- 2. masked equals the reference's zeroing
@pytest.mark.parametrize('flavour', ['signed', 'separate_pol', 'histogram'])
def test_masked_equals_the_unmasked_grid_with_the_hot_pixels_zeroed(flavour):
    """the mask the size of the grid, integer pixels: what the event preprocessor's loop does to the finished grid,
    grid[:, :, y, x] = 0 over the mask's locations -- voxelise first (the time base counts the hot events), zero afterwards"""
    wins, hot, _ = _wins(GH)
    assert all(h[0] and h[-1] for h, k in zip(hot, SLOT_MASKS) if k >= 0)
    out, buf, acc = _masked('columns', flavour, wins, SLOT_MASKS, False, mask_size=(GH, GW))
    want = _unmasked('columns', flavour, wins, False).clone()
    before = want.clone()
    for i, k in enumerate(SLOT_MASKS):
        if k >= 0:
            for x, y in _locations(k, GH):
                want[i, :, y, x] = 0
    assert torch.equal(_bits(out), _bits(want)) and not torch.equal(_bits(want), _bits(before))
    assert C._guards_intact(buf, out) and not bool(acc.any())


# ---------------------------------------------------------------------------------------------- 3. other ingest cases
def test_an_unknown_mask_word_empties_its_slot_and_ingest_keep_leaves_the_grid():
    from ess_amd import hip
    wins, _, moved = _wins()
    want = _unmasked('ring_wrapped', 'signed', moved, False)
    out, buf, acc = _masked('ring_wrapped', 'signed', wins, [0, 3, -2, 2], False)  # n_masks = 3: the words 3 and -2 name nothing
    for i in (0, 3):
        assert torch.equal(_bits(out[i]), _bits(want[i])) and bool(out[i].any()), i
    for i in (1, 2):
        assert not bool(_bits(out[i]).any()), f'slot {i}: not all zero'
    assert C._guards_intact(buf, out) and not bool(acc.any())
    counts = [wins[0].n, hip.INGEST_KEEP, wins[2].n, -7]
    for source, flavour in (('columns', 'trilinear_map'), ('ring_residue_3', 'separate_pol')):
        out, buf, acc = _masked(source, flavour, wins, SLOT_MASKS, False, counts=counts)
        want = _unmasked(source, flavour, moved, False)
        for i in (0, 2):
            assert torch.equal(_bits(out[i]), _bits(want[i])) and bool(out[i].any()), (source, flavour, i)
        for i in (1, 3):  # (the NaN pre-fill, every bit of it)
            assert bool((out[i].view(torch.int16) == M.NAN16).all()), (source, flavour, i)
        assert C._guards_intact(buf, out) and not bool(acc.any())
    # no masks at all (masks=None, mask_of=None): the unmasked grids
    dev, rows, st = _device('ring_wrapped', wins)
    got = hip.event_ingest_masked(*dev, rows, st, _words([c.n for c in wins]), _words([c.format for c in wins]),
                                  torch.full((4, 5, GH, GW), float('nan'), device=DEV))
    assert torch.equal(_bits(got), _bits(_unmasked('ring_wrapped', 'signed', wins, False)))


@pytest.mark.parametrize('flavour', ['signed', 'trilinear_map'])
def test_a_larger_call_that_spans_several_workgroups(flavour):
    """20 000 events in one slot (twenty workgroups in x), a window that wraps from a start of residue 3, uint16 / int64 columns"""
    from ess_amd.datasets.data_util import EventColumns
    n, ring = 20_000, 20_480
    c = _window(n, 3, _locations(1), 77)
    h = HP.masked(c, _mask_words()[1], MH, MW)
    assert 0.20 <= h.mean() <= 0.30 and h[0] and h[-1]
    moved = EventColumns(*HP.moved_away(c, h))
    start = ring - 4097
    assert start % 4 == 3
    kw = dict(starts=[start], ring=ring)
    out, buf, acc = _masked('ring_wrapped', flavour, [c], [1], False, **kw)
    want, plain = _unmasked('ring_wrapped', flavour, [moved], False, **kw), _unmasked('ring_wrapped', flavour, [c], False, **kw)
    assert torch.equal(_bits(out), _bits(want)) and not torch.equal(_bits(out), _bits(plain)) and bool(out.any())
    assert C._guards_intact(buf, out) and not bool(acc.any())


# ---------------------------------------------------------------------------------------------- 4. counts -> mask
def _counts(W, H=3):
    """per sensor (positive, negative) events a pixel: sensor 0 (threshold 0) totals 0, 1, 2; sensor 1 (threshold 2) totals 1, 2 -- AT
    the threshold, as 1 + 1 --, 3 -- one above, as 2 + 1; sensor 2 (threshold < 0) 5 everywhere"""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    pos = np.stack([(xs + ys) % 2, 1 + (xs + ys) % 2, np.full((H, W), 5)])
    neg = np.stack([((xs + ys) % 4 == 3).astype(np.int64), ((xs + 2 * ys) % 3 != 0).astype(np.int64), np.zeros((H, W), np.int64)])
    return pos, neg


@pytest.mark.parametrize('W', [1, 33, 64, 70])
def test_counts_to_mask(W):
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    H, n, nw = 3, 3, HP.n_words(W)
    pos, neg = _counts(W, H)
    thr = np.array([0, 2, -1], dtype=np.int64)
    total = pos + neg
    assert (total[0] == 0).any() and (total[0] == 1).any()                                       # at the threshold 0, one above
    assert ((total[1] == 2) & (pos[1] == 1) & (neg[1] == 1)).any() and ((total[1] == 3) & (neg[1] == 1)).any()  # at 2 (not hot), 3 (hot)
    wins = []
    for i in range(n):
        ys, xs = np.nonzero(np.ones((H, W), bool))
        x = np.concatenate([np.repeat(xs, pos[i].ravel()), np.repeat(xs, neg[i].ravel())])
        y = np.concatenate([np.repeat(ys, pos[i].ravel()), np.repeat(ys, neg[i].ravel())])
        p = np.concatenate([np.ones(pos[i].sum(), np.uint8), np.zeros(neg[i].sum(), np.uint8)])
        order = np.random.default_rng(W + i).permutation(len(x))
        wins.append(EventColumns(np.arange(len(x), dtype=np.float64), x[order].astype(np.int16), y[order].astype(np.int16), p[order]))
    stride = hip.event_column_stride(max(c.n for c in wins))
    sums = torch.zeros(n, 2, H, W, dtype=torch.int64, device=DEV)
    hip.event_scatter_ring_rep(*TT._dev_columns(wins, stride), _words([0, 1, 2]), _words([0, 0, 0]), _words([c.n for c in wins]),
                               _words([0, 0, 0]), sums, hip.EVENT_REP_HISTOGRAM)
    host = sums.cpu().numpy()
    assert np.array_equal(host[:, 1] >> 40, pos) and np.array_equal(host[:, 0] >> 40, neg) and not (host & ((1 << 40) - 1)).any()
    thr_dev = torch.from_numpy(thr).to(DEV)
    G = 16  # guard words on either side
    for mode, fill in ((hip.MASK_REPLACE, 0xFFFFFFFF), (hip.MASK_OR, 0xA5A5A5A5)):
        buf = torch.full((n * H * nw + 2 * G,), fill - (1 << 32), dtype=torch.int32, device=DEV)
        masks = buf[G:G + n * H * nw].view(n, H, nw)
        before = np.full((n, H, nw), fill, dtype=np.uint32)
        assert hip.event_hot_pixel_mask(sums, thr_dev, masks, mode) is masks
        got = masks.cpu().numpy().view(np.uint32)
        want = HP.mask_words_of(host, thr, before, HP.REPLACE if mode == hip.MASK_REPLACE else HP.OR)
        assert np.array_equal(got, want), (W, mode)
        assert (got[2] == fill).all()  # threshold < 0: neither read nor written
        tail = W & 31
        if tail and mode == hip.MASK_REPLACE:
            assert not (got[:2, :, -1] >> np.uint32(tail)).any()  # the bits at x >= W are written as 0
        if tail and mode == hip.MASK_OR:
            assert ((got[:2, :, -1] >> np.uint32(tail)) == (np.uint32(fill) >> np.uint32(tail))).all()  # ... or left as they were
        if mode == hip.MASK_REPLACE:
            hot = np.stack([total[i] > thr[i] for i in range(2)])
            bits = (got[:2, :, :, None] >> np.arange(32, dtype=np.uint32)) & 1
            assert np.array_equal(bits.reshape(2, H, -1)[:, :, :W].astype(bool), hot)
        edge = buf.cpu().numpy().view(np.uint32)
        assert (edge[:G] == fill).all() and (edge[-G:] == fill).all()
        assert torch.equal(sums.cpu(), torch.from_numpy(host))  # the sums are read only


# ---------------------------------------------------------------------------------------------- 5. the segmenters
SEG_CASES = [c for c in TT.SEG_CASES if c[0] == 'mixed']
SEG_IDS = [f'{m}-{"graph" if g else "eager"}' for m, g in SEG_CASES]
CAP, RCAP, WIN = TT.CAP, TT.RCAP, TT.WIN
SH_, SW_ = SC.H, SC.W


def _seg_locations(k, mh, mw):
    g = np.random.default_rng(500 + k)
    return sorted({(int(x), int(y)) for x, y in zip(g.integers(0, mw, 12), g.integers(0, mh, 12))} | {(0, 0), (mw - 1, mh - 1), (32, 1)})


@functools.lru_cache(maxsize=None)
def _seg_masks(mh, mw):
    from ess_amd.datasets.hot_pixels import HotPixelMask
    return tuple(HotPixelMask.from_locations(np.array(_seg_locations(k, mh, mw)), mh, mw) for k in range(2))


@functools.lru_cache(maxsize=None)
def _seg_source(s, mh, mw, n=2048):
    """stream s's whole sequence on an mh x mw sensor: a quarter of every window's events on the pixels of BOTH masks (so that
    whichever mask the stream reads removes a share), each window's first and last event among them"""
    from ess_amd.datasets.data_util import EventColumns
    loc = _seg_locations(0, mh, mw) + _seg_locations(1, mh, mw)
    parts = [_window(WIN, (3, 0, 1)[s], loc, 900 + 10 * s + k, mh, mw, t_span_us=40_000) for k in range(n // WIN)]
    for c in parts:  # (the two pixels both masks hold: every window's first and last event are hot under either)
        c.x[0], c.y[0], c.x[-1], c.y[-1] = 0, 0, mw - 1, mh - 1
    t = np.concatenate([c.t + k * (40_000 if c.t.dtype == np.int64 else 0.04) for k, c in enumerate(parts)])
    return EventColumns(t, *(np.concatenate([getattr(c, a) for c in parts]) for a in 'xyp'))


def _seg_window(s, k, mask, mh, mw):
    """window k of stream s, as it is and with the events mask removes moved away"""
    from ess_amd.datasets.data_util import EventColumns
    c = RG._slice(_seg_source(s, mh, mw), k * WIN, (k + 1) * WIN)
    if mask is None:
        return c, c
    h = HP.masked(c, mask.words, mh, mw)
    assert 0.05 <= h.mean() <= 0.35 and h[0] and h[-1]
    return c, EventColumns(*HP.moved_away(c, h))


def _seg_round(seg, ref, layout, windows, masks, mh, mw, what):
    """one round of the masked segmenter on the windows as they are and of the unmasked one on the moved-away windows"""
    pairs = [None if k is None else _seg_window(s, k, masks[s], mh, mw) for s, k in enumerate(windows)]
    on = [p is not None for p in pairs]
    if layout == 'ring':
        for s, p in enumerate(pairs):
            if p is not None:
                seg.feed(s, p[0])
                ref.feed(s, p[1])
        got, want = seg.update_from_feed(), ref.update_from_feed()
    else:
        got = seg.update_from_events([None if p is None else p[0] for p in pairs])
        want = ref.update_from_events([None if p is None else p[1] for p in pairs])
    C._assert_rows(got, want, on, what)
    return got


STREAM_CASES = [(layout, compact, 'temporal') for layout in ('ring', 'columns') for compact in (False, True)] + [('ring', True, 'trilinear')]


@pytest.mark.parametrize('layout,compact,voxel', STREAM_CASES, ids=[f'{a}-{"compact" if b else "ride"}-{c}' for a, b, c in STREAM_CASES])
@pytest.mark.parametrize('mode,graph', SEG_CASES, ids=SEG_IDS)
def test_stream_rounds_under_masks_equal_rounds_on_moved_away_events(mode, graph, layout, compact, voxel):
    """S = 3 with hot_pixel_masks=[m0, None, m0]: four rounds -- all streams, stream 2 alone (compacted: slot 0 carries stream 2's
    mask word), two streams, and behind set_hot_pixels(1, m1) all three again -- equal a segmenter without masks that is fed the
    moved-away columns, bit for bit; no capture is added by set_hot_pixels"""
    from ess_amd import hip
    S = 3
    tri = voxel == 'trilinear'
    mh, mw = (TT.SMH, TT.SMW) if tri else (SH_, SW_)
    m0, m1 = _seg_masks(mh, mw)
    with SQ._Pinned(mode):
        kw = dict(graph=graph, event_capacity=CAP, event_layout=layout)
        if layout == 'ring':
            kw.update(ring_capacity=RCAP, window_events=WIN)
        if tri:
            kw.update(voxel='trilinear', rectify_maps=TT._rig())
        if compact:
            kw.update(compact=True, compact_buckets=[1, 2])
        seg = SC._segmenter('convlstm', S, hot_pixel_masks=[m0, None, m0], **kw)
        ref = SC._segmenter('convlstm', S, **kw)
        base = 4 if layout == 'ring' else 2
        assert tuple(seg._words.shape) == (base + 2, S) and seg._hot.mask_of == [0, hip.MASK_NONE, 0] and seg._hot.size == (mh, mw)
        assert tuple(seg._hot.words.shape) == (S, mh, HP.n_words(mw))  # ONE static buffer; m0 is held once
        seg.warm_up()
        ref.warm_up()
        captures = seg.n_captures
        masks = [m0, None, m0]
        rounds = [(0, 0, 0), (None, None, 1), (1, 1, None), (2, 2, 2)]
        for r, windows in enumerate(rounds):
            if r == 3:
                seg.set_hot_pixels(1, m1)
                masks = [m0, m1, m0]
                assert seg._hot.mask_of == [0, 1, 0] and seg.n_captures == captures
            got = _seg_round(seg, ref, layout, windows, masks, mh, mw, f'{mode} graph={graph} {layout} compact={compact} {voxel} round {r}')
            if r == 1:
                torch.cuda.synchronize()
                words = seg._words.cpu()[-1].tolist()
                if compact:
                    assert words[0] == 0 and list(got.valid) == [False, False, True], 'slot 0 holds stream 2 and carries its mask word'
                else:
                    assert words == [hip.MASK_NONE, hip.MASK_NONE, 0]
        assert seg.n_captures == captures == ref.n_captures and not bool(seg._acc.any())
        assert seg.hot_pixels(1) is m1 and seg.hot_pixels(0) is m0


def _calibration_packet(s, fmt, k):
    """512 events of stream s on the 64 x 96 sensor: three pixels fire k + 1, 10 and 50 times, 100 others exactly k times, 148 once"""
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(800 + s)
    pix = g.permutation(SH_ * SW_)[:3 + 100 + 148]
    reps = np.array([k + 1, 10, 50] + [k] * 100 + [1] * 148)
    assert reps.sum() == 64 + 100 * k + 148 == WIN
    flat = np.repeat(pix, reps)[g.permutation(WIN)]
    base = T.raw_events(WIN, SH_, SW_, 810 + s, fmt=fmt, t_span_us=40_000)
    xy = np.uint16 if fmt & 2 else np.int16
    hot = sorted((int(p % SW_), int(p // SW_)) for p in pix[:3])
    return EventColumns(base.t, (flat % SW_).astype(xy), (flat // SW_).astype(xy), base.p), hot


@pytest.mark.parametrize('mode,graph', SEG_CASES, ids=SEG_IDS)
def test_calibration_from_the_rings(mode, graph):
    """three known pixels a stream fire more than k = 3 times, a hundred exactly k times: calibrate_hot_pixels returns exactly the
    three, the next round equals an unmasked segmenter's on the moved-away events, and nothing is captured again"""
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.hot_pixels import HotPixelMask
    S, k = 3, 3
    with SQ._Pinned(mode):
        kw = dict(graph=graph, event_capacity=CAP, event_layout='ring', ring_capacity=RCAP, window_events=WIN)
        seg = SC._segmenter('convlstm', S, hot_pixel_masks=[None] * S, **kw)
        ref = SC._segmenter('convlstm', S, **kw)
        with pytest.raises(hip.EssHipError, match='built without hot_pixel_masks'):
            ref.calibrate_hot_pixels(max_events_per_pixel=k)
        for bad in (dict(), dict(max_events_per_pixel=k, max_rate_hz=1.0), dict(max_events_per_pixel=-1), dict(max_events_per_pixel=k, mode='and')):
            with pytest.raises(hip.EssHipError, match='calibrate_hot_pixels'):
                seg.calibrate_hot_pixels(**bad)
        seg.warm_up()
        captures = seg.n_captures
        packets = [_calibration_packet(s, (3, 0, 1)[s], k) for s in range(S)]
        for s, (c, _) in enumerate(packets):
            seg.feed(s, c)
        pending = [seg.pending(s) for s in range(S)]
        got = seg.calibrate_hot_pixels(max_events_per_pixel=k)
        assert len(got) == S and [seg.pending(s) for s in range(S)] == pending == [1] * S
        for s, (c, hot) in enumerate(packets):
            hand = HotPixelMask.from_locations(np.array(hot), SH_, SW_)
            assert got[s].to_locations().tolist() == [list(v) for v in sorted(hot, key=lambda v: (v[1], v[0]))] and got[s] == hand
            assert seg.hot_pixels(s) is got[s]
            ref.feed(s, EventColumns(*HP.moved_away(c, HP.masked(c, hand.words, SH_, SW_))))
        assert not bool(seg._hot.scratch.any())
        C._assert_rows(seg.update_from_feed(), ref.update_from_feed(), [True] * S, f'{mode} graph={graph}: the round behind the calibration')
        # by rate, on the float64-seconds stream: floor(rate * (t_last - t_first)) == k; 'or' onto the mask it has: the same three
        t = packets[1][0].t
        again = seg.calibrate_hot_pixels(streams=[1], max_rate_hz=(k + 0.5) / float(t[-1] - t[0]), mode='or')
        assert len(again) == 1 and again[0] == got[1] and seg.hot_pixels(1) is again[0]
        assert seg.n_captures == captures and seg.n_windows == 1


HEADS = {'plain': dict(), 'loader_grid': dict(grid_hw=(72, 90), grid_resize=(72, 96), grid_normalize='unbiased')}


@pytest.mark.parametrize('head', list(HEADS))
@pytest.mark.parametrize('mode,graph', SEG_CASES, ids=SEG_IDS)
def test_sequence_rounds_under_masks_equal_rounds_on_moved_away_events(mode, graph, head):
    """SequenceSegmenter(hot_pixel_masks=[m0, None]) with T = 3: labels, colours, confidences and the confusion rows equal the
    unmasked segmenter's on moved-away events, through the plain ring ingest and through the loader grid (scatter half + finish)"""
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    S, T_, NW, K = 2, 3, 256, SC.K
    mh, mw = HEADS[head].get('grid_hw', (SH_, SW_))
    m0, m1 = _seg_masks(mh, mw)
    with SQ._Pinned(mode):
        make = lambda **kw: SequenceSegmenter(*M._models(*SC._weights('convlstm'), K), SH_, SW_, default_options(), S,  # noqa: E731
                                              sequence_steps=T_, window_events=NW, ring_capacity=1024, palette=SH.palette_for(K),
                                              want_confidence=True, graph=graph, **HEADS[head], **kw)
        seg, ref = make(hot_pixel_masks=[m0, None]), make()
        assert tuple(seg._words.shape) == (6, T_ * S) and seg._hot.size == (mh, mw)
        masks = [m0, None]
        src = [_seg_source(s, mh, mw, 1024) for s in range(S)]
        gt = [SQ._gt(0, s) for s in range(S)]
        fed = 0
        for r, (upto, ends) in enumerate(((T_ * NW, [T_ * NW, 700]), (1024, [1000, 1024]))):
            if r == 1:
                seg.set_hot_pixels(1, m1)
                masks = [m0, m1]
            for s in range(S):
                c = RG._slice(src[s], fed, upto)
                seg.feed(s, c)
                whole = src[s]
                h = HP.masked(whole, masks[s].words, mh, mw) if masks[s] is not None else np.zeros(whole.n, bool)
                if r == 1 and s == 1:  # (the ring holds events fed under no mask: the reference's ring is rewritten as m1 sees it)
                    ref.drop_feed([1])
                    ref.feed(1, RG._slice(EventColumns(*HP.moved_away(whole, h)), 0, upto))
                else:
                    ref.feed(s, RG._slice(EventColumns(*HP.moved_away(whole, h)), fed, upto))
            fed = upto
            got, want = seg.segment_at(end=ends, labels=gt), ref.segment_at(end=ends, labels=gt)
            C._assert_rows(got, want, [True] * S, f'{mode} graph={graph} {head} round {r}')
            torch.cuda.synchronize()
            assert torch.equal(seg.confusion, ref.confusion) and bool(seg.confusion.any())
        assert seg.n_captures == ref.n_captures == (1 if graph else 0) and not bool(seg._acc.any())
