"""GPU tier of the event representations: hip.event_scatter_ring_rep / event_ingest_ring_rep / event_ingest_columns_rep (separate
polarity, histogram) and representation= of EventBatchBuilder, SequenceSegmenter and MultiStreamSegmenter.  What is asserted
throughout is BITS against tests/event_rep_ref.py's numpy restatement: a grid equals restate() of the window unrolled into contiguous
columns, the sums a scatter leaves equal restate_sums(); a loader finish equals the finish of the RESTATED sums (and lies inside
tests/loader_grid_ref.py's bound of its float64 reference); a builder's batch equals scatter + finish + torch.flip / slice composed by
hand; a segmenter's labels, colours and confidences from events equal those for the restated grids handed to its grid-taking path.
out buffers are guarded and NaN-pre-filled, acc is all zero behind every call."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import event_batch_ref as EBR  # noqa: E402
from tests import event_rep_ref as E  # noqa: E402
from tests import loader_grid_ref as LG  # noqa: E402
from tests import test_hip_event_columns as C  # noqa: E402  (bits, words, guards, EventColumns from rows)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers, models, result rows)
from tests import test_hip_seg_head as SH  # noqa: E402  (palette)
from tests import test_host_event_ingest as R  # noqa: E402  (events inside a grid)

DEV, NAN16 = M.DEV, M.NAN16
RING = 4096
_bits, _words = C._bits, C._words
REP_WORD = {'signed': 0, 'separate_pol': 1, 'histogram': 2}
#         representation, (H, W), bins
GRIDS = [('separate_pol', (24, 40), 1), ('separate_pol', (24, 40), 5), ('separate_pol', (23, 37), 2), ('separate_pol', (23, 37), 3),
         ('histogram', (24, 40), 1), ('histogram', (23, 37), 1)]
GRID_IDS = [f'{r}-{h}x{w}-b{b}' for r, (h, w), b in GRIDS]
T0_US = C.T0_US


# ---------------------------------------------------------------------------------------------- raw rows and their windows
def _row(fmt, H, W, seed, ring=RING):
    """One FULL row of raw columns in the dtypes of format word fmt (E.Cols): every position holds an event that lands in the grid
    unless an edge is planted on it, so whatever a kernel reads outside its window shows.  Times ascend along the row.  Planted, at
    fixed positions inside the windows the edge table names: polarity bytes 0, 1 and 0xFF throughout; coordinates -1, W, H and 32768
    (raw 0x8000: -32768 as int16, 32768 as uint16); a NaN time (float64 rows); eight events of one time (positions 2048 .. 2055)."""
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0.0, 0.2, ring))
    t[2048:2056] = t[2048]
    xy = (np.int16, np.uint16)[fmt >> 1 & 1]
    x, y = g.integers(0, W, ring).astype(np.int64), g.integers(0, H, ring).astype(np.int64)
    for at, (vx, vy) in ((5, (-1, None)), (9, (W, None)), (13, (None, H)), (17, (None, -1)), (21, (0x8000, None)), (25, (None, 0x8000)),
                         (1030, (-1, -1)), (4090, (W, H))):
        if vx is not None:
            x[at] = vx
        if vy is not None:
            y[at] = vy
    p = g.choice(np.array([0, 1, 0xFF], np.uint8), ring)
    if fmt & 1:
        tc = T0_US + np.round(t * 1e6).astype(np.int64)
    else:
        tc = t.copy()
        tc[[11, 1031, 3000]] = np.nan
    return E.Cols(tc, (x & 0xFFFF).astype(np.uint16).view(xy), (y & 0xFFFF).astype(np.uint16).view(xy), p)


def _upload(rows):
    """rows (E.Cols of equal length) -> (t int64, x int16, y int16, p uint8) [n_rows, ring] on the device: the raw words"""
    host = (np.stack([r.t.view(np.int64) for r in rows]), np.stack([r.x.view(np.int16) for r in rows]),
            np.stack([r.y.view(np.int16) for r in rows]), np.stack([r.p.view(np.uint8) for r in rows]))
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in host)


def _window(row, start, count):
    """the window (start, count) of a full row, unrolled: contiguous E.Cols"""
    ring = len(row.t)
    idx = (start + np.arange(min(max(count, 0), ring))) % ring
    return E.Cols(*(np.ascontiguousarray(a[idx]) for a in row))


def _want(cols, rep, bins, H, W):
    return torch.from_numpy(E.restate(cols, rep, bins, H, W)).to(DEV)


def _call(source, rep, dev, slots, C_, H, W, out=None, acc=None):
    """slots: (row, start, count, format) per slot; source 'columns': slot i reads the head of row i (row and start are not passed)
    -> (out inside its NaN-pre-filled guarded buffer, the buffer or None, acc)"""
    from ess_amd import hip
    n, buf = len(slots), None
    if out is None:
        buf, out = M._guarded((n, C_, H, W), torch.float32)
    if acc is None:
        acc = torch.zeros(n * C_ * H * W, dtype=torch.int64, device=DEV)
    w = [_words([s[k] for s in slots]) for k in range(4)]
    if source == 'ring':
        got = hip.event_ingest_ring_rep(*dev, *w, out, REP_WORD[rep], acc=acc)
    else:
        assert [s[0] for s in slots] == list(range(n)) and all(s[1] == 0 for s in slots) and dev[0].shape[0] == n
        got = hip.event_ingest_columns_rep(*dev, w[2], w[3], out, REP_WORD[rep], acc=acc)
    assert got is out
    return out, buf, acc


# ---------------------------------------------------------------------------------------------- 1. the edge table
def _edge_slots(source, n_rows, KEEP):
    """(row, start, count, format word or None for the row's own, expectation) -- expectation 'grid': the restatement of the window,
    'zero': an all-zero grid, 'keep': the pre-fill stays"""
    if source == 'columns':  # slot i is row i, from entry 0: counts and formats are what there is to vary
        table = [(0, 3000, None, 'grid'), (1, 0, None, 'zero'), (2, 1, None, 'grid'), (3, 2, None, 'grid'), (4, 7, None, 'grid'),
                 (5, KEEP, None, 'keep'), (6, RING, None, 'grid'), (7, 1037, 4, 'zero'), (8, 30, -1, 'zero'), (9, -7, None, 'keep'),
                 (10, RING + 9, None, 'grid'), (11, 2058, None, 'grid')]
        return [(r, 0, n, f, e) for r, n, f, e in table]
    return [(0, 0, 30, None, 'grid'), (1, 1, 30, None, 'grid'), (2, 2, 30, None, 'grid'), (3, 3, 30, None, 'grid'),  # the residues
            (2, 4000, 300, None, 'grid'),            # across the wrap
            (1, 4093, RING, None, 'grid'),           # a full ring from an unaligned start
            (3, 1, RING + 40, None, 'grid'),         # a count above the ring: the ring
            (0, 7, 0, None, 'zero'), (0, 2050, 1, None, 'grid'), (1, 4095, 2, None, 'grid'), (2, 1029, 7, None, 'grid'),
            (3, 9, KEEP, None, 'keep'), (0, 9, -7, None, 'keep'),
            (1, 2048, 8, None, 'grid'),              # eight events of one time: dT == 0
            (0, 2040, 16, None, 'grid'),             # ... and the window that ends on them
            (2, 5, 1000, 4, 'zero'), (2, 5, 1000, -1, 'zero'),  # an unknown format bit
            (-1, 5, 100, None, 'zero'), (n_rows, 5, 100, None, 'zero'), (1 << 30, 5, 100, None, 'zero'),  # a row outside the rings
            (0, -1, 100, None, 'zero'), (0, RING, 100, None, 'zero'), (0, 1 << 30, 100, None, 'zero'),   # a start outside them
            (3, 2999, 1013, None, 'grid')]


@pytest.mark.parametrize('source', ['ring', 'columns'])
@pytest.mark.parametrize('rep,hw,bins', GRIDS, ids=GRID_IDS)
def test_the_edge_table(rep, hw, bins, source):
    """Every row is a FULL ring of events that land, formats 0 .. 3 taking turns (int64 times, uint16 coordinates), so the filler
    behind every count, in front of every start and in a masked head or tail would show.  The slots cover: ring starts at residues
    0 .. 3, a window across the wrap, a full ring from an unaligned start, counts 0, 1, 2, 7 and 1013, INGEST_KEEP, format words that
    differ per slot, polarity bytes 0 / 1 / 0xFF, coordinates -1, W, H and 32768, the window's last event (last bin: no right half),
    dT == 0, NaN times (dropped by separate, counted by the histogram), an unknown format bit, rows and starts outside the rings"""
    from ess_amd import hip
    H, W = hw
    C_ = E.channels(rep, bins)
    assert hip.event_rep_channels(REP_WORD[rep], bins) == C_
    n_rows = 12 if source == 'columns' else 4
    rows = [_row(r % 4, H, W, 40 + r) for r in range(n_rows)]
    table = _edge_slots(source, n_rows, hip.INGEST_KEEP)
    slots = [(r, s, n, (r % 4 if 0 <= r < n_rows else 0) if f is None else f) for r, s, n, f, _ in table]  # (row r has format r % 4)
    out, buf, acc = _call(source, rep, _upload(rows), slots, C_, H, W)
    nan_seen = 0
    for i, ((r, s, n, f, expect), slot) in enumerate(zip(table, slots)):
        what = f'slot {i} {slot} {expect}'
        if expect == 'keep':
            assert bool((out[i].view(torch.int16) == NAN16).all()), what
        elif expect == 'zero':
            assert not bool(_bits(out[i]).any()), what
        else:
            win = _window(rows[r], s, n)
            assert torch.equal(_bits(out[i]), _bits(_want(win, rep, bins, H, W))), what
            assert bool(out[i].any()) and bool((out[i] >= 0).all()), what
            nan_seen += int(win.t.dtype == np.float64 and np.isnan(win.t).any())
    assert nan_seen >= 2
    assert C._guards_intact(buf, out) and not bool(acc.any())
    first = out.clone()
    buf.fill_(NAN16)
    _call(source, rep, _upload(rows), slots, C_, H, W, out=out, acc=acc)  # the run: the same bits again
    assert torch.equal(_bits(out), _bits(first)) and not bool(acc.any()) and C._guards_intact(buf, out)


def test_a_nan_time_is_dropped_by_separate_and_counted_by_the_histogram():
    H, W = 24, 40
    row = _row(0, H, W, 77)
    win = _window(row, 2990, 20)  # (position 3000 holds a NaN time and an in-range pixel)
    k = 10
    assert np.isnan(win.t[k]) and 0 <= win.x[k] < W and 0 <= win.y[k] < H
    slots = [(0, 2990, 20, 0)]
    hist, _, _ = _call('ring', 'histogram', _upload([row]), slots, 2, H, W)
    sep, _, _ = _call('ring', 'separate_pol', _upload([row]), slots, 4, H, W)
    inside = (win.x >= 0) & (win.x < W) & (win.y >= 0) & (win.y < H)
    assert float(hist.sum()) == float(inside.sum())
    assert abs(float(sep.sum()) - float((inside & ~np.isnan(win.t)).sum())) < 1e-3  # (every kept event adds left + right = 1; the last: left)
    assert torch.equal(_bits(hist[0]), _bits(_want(win, 'histogram', 1, H, W))) and torch.equal(_bits(sep[0]), _bits(_want(win, 'separate_pol', 2, H, W)))


# ---------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize('rep,bins', [('separate_pol', 3), ('histogram', 1)])
def test_bits_do_not_depend_on_order_slot_count_or_position(rep, bins):
    """a window's interior events shuffled (its first and last stay: they define the time scale), the slot alone, first, last and
    among eight: one grid, bit for bit -- the restatement's"""
    H, W = 23, 37
    C_ = E.channels(rep, bins)
    base = _row(2, H, W, 90)
    n = 2500
    g = np.random.default_rng(3)
    perm = np.concatenate([[0], 1 + g.permutation(n - 2), [n - 1]])
    shuffled = E.Cols(*(np.concatenate([a[:n][perm], a[n:]]) for a in base))
    other = _row(1, H, W, 91)
    want = _want(_window(base, 0, n), rep, bins, H, W)
    assert torch.equal(_bits(want), _bits(_want(_window(shuffled, 0, n), rep, bins, H, W)))
    dev = _upload([base, shuffled, other])
    me, them = (0, 0, n, 2), (2, 17, 3000, 1)
    for slots, at in (([me], [0]), ([(1, 0, n, 2)], [0]), ([me] + [them] * 7, [0]), ([them] * 7 + [me], [7]),
                      ([them, me, them, (1, 0, n, 2), them, me, them, them], [1, 3, 5])):
        out, buf, acc = _call('ring', rep, dev, slots, C_, H, W)
        for i in at:
            assert torch.equal(_bits(out[i]), _bits(want)), (slots, i)
        assert C._guards_intact(buf, out) and not bool(acc.any())
    out, _, _ = _call('columns', rep, _upload([shuffled, base]), [(0, 0, n, 2), (1, 0, n, 2)], C_, H, W)
    assert torch.equal(_bits(out[0]), _bits(want)) and torch.equal(_bits(out[1]), _bits(want))


# ---------------------------------------------------------------------------------------------- 3. the identity, SIGNED, the golden
@pytest.mark.parametrize('hw,bins', [((24, 40), 5), ((23, 37), 1), ((23, 37), 2)])
def test_positive_minus_negative_sums_are_the_signed_sums_on_the_device(hw, bins):
    """event_scatter_ring_rep(SEPARATE) and event_scatter_ring on the same windows, acc read before any finish: int64, exactly; and
    both equal the restated sums"""
    from ess_amd import hip
    H, W = hw
    rows = [_row(r, H, W, 120 + r) for r in range(4)]
    slots = [(0, 3, 3000, 0), (1, 4000, 500, 1), (2, 4093, RING, 2), (3, 2048, 8, 3), (0, 7, 0, 0), (1, 2, 1, 1)]
    dev, w = _upload(rows), [_words([s[k] for s in slots]) for k in range(4)]
    sep = torch.zeros(len(slots), 2 * bins, H, W, dtype=torch.int64, device=DEV)
    signed = torch.zeros(len(slots), bins, H, W, dtype=torch.int64, device=DEV)
    hist = torch.zeros(len(slots), 2, H, W, dtype=torch.int64, device=DEV)
    assert hip.event_scatter_ring_rep(*dev, *w, sep, hip.EVENT_REP_SEPARATE) is sep
    hip.event_scatter_ring(*dev, *w, signed)
    again = torch.zeros_like(signed)
    hip.event_scatter_ring_rep(*dev, *w, again, hip.EVENT_REP_SIGNED)
    hip.event_scatter_ring_rep(*dev, *w, hist, hip.EVENT_REP_HISTOGRAM)
    assert torch.equal(sep[:, :bins] - sep[:, bins:], signed) and torch.equal(again, signed)
    assert bool((sep >= 0).all()) and bool(sep[0, :bins].any()) and bool(sep[0, bins:].any()) and not bool(sep[4].any())
    for i, (r, s, n, _) in enumerate(slots):
        win = _window(rows[r], s, n)
        assert np.array_equal(sep[i].cpu().numpy(), E.restate_sums(win, 'separate_pol', bins, H, W)), i
        assert np.array_equal(signed[i].cpu().numpy(), E.restate_sums(win, 'signed', bins, H, W)), i
        assert np.array_equal(hist[i].cpu().numpy(), E.restate_sums(win, 'histogram', bins, H, W)), i


def test_the_signed_representation_has_the_bits_of_the_existing_entry_points():
    from ess_amd import hip
    H, W, bins = 24, 40, 5
    rows = [_row(r, H, W, 140 + r) for r in range(4)]
    slots = [(r, s, n, r) for r, s, n in ((0, 0, 3000), (1, 1, 1), (2, 4094, 777), (3, 0, RING))]
    dev, w = _upload(rows), [_words([s[k] for s in slots]) for k in range(4)]
    nan = lambda: torch.full((4, bins, H, W), float('nan'), device=DEV)  # noqa: E731
    a, b = hip.event_ingest_ring_rep(*dev, *w, nan(), hip.EVENT_REP_SIGNED), hip.event_ingest_ring(*dev, *w, nan())
    assert torch.equal(_bits(a), _bits(b)) and bool(a.any())
    a, b = hip.event_ingest_columns_rep(*dev, w[2], w[3], nan(), hip.EVENT_REP_SIGNED), hip.event_ingest_columns(*dev, w[2], w[3], nan())
    assert torch.equal(_bits(a), _bits(b)) and bool(a.any())


def test_the_histogram_golden_through_event_ingest_columns_rep():
    """the reference's generate_event_histogram on the golden's events (tests/golden/event_histogram.pt), bit for bit"""
    from ess_amd import hip
    from tests.test_host_event_representations import _histogram_cols, _histogram_golden
    H, W, cases = _histogram_golden()
    stride = hip.event_column_stride(max(c['n'] for c in cases))
    rows = []
    for c in cases:
        cols = _histogram_cols(c['n'], c['seed'], c['pm'], H, W)
        pad = stride - c['n']  # the filler behind the count: events that would land
        rows.append(E.Cols(np.concatenate([cols.t, np.full(pad, cols.t[0])]), np.concatenate([cols.x, np.ones(pad, np.int16)]),
                           np.concatenate([cols.y, np.ones(pad, np.int16)]), np.concatenate([cols.p.view(np.uint8), np.ones(pad, np.uint8)])))
    slots = [(i, 0, c['n'], 0) for i, c in enumerate(cases)]
    out, buf, acc = _call('columns', 'histogram', _upload(rows), slots, 2, H, W)
    for i, c in enumerate(cases):
        assert torch.equal(_bits(out[i]), _bits(c['histogram'].to(DEV))), c['seed']
    assert C._guards_intact(buf, out) and not bool(acc.any())


# ---------------------------------------------------------------------------------------------- 4. the loader finish on C planes
GEOS = {'ddd17': ((26, 35), dict(resized=(26, 36), rows=20)), 'identity': ((23, 37), dict())}


@pytest.mark.parametrize('window', [False, True], ids=['finish', 'finish_window'])
@pytest.mark.parametrize('mode', ['population', 'unbiased'])
@pytest.mark.parametrize('geo', ['ddd17', 'identity'])
@pytest.mark.parametrize('rep,bins', [('separate_pol', 2), ('histogram', 1)])
def test_the_loader_finish_normalises_over_all_planes(rep, bins, geo, mode, window):
    """scatter_rep, then event_grid_finish / event_grid_finish_window with a 0xFF-filled workspace: the sums equal the restated sums;
    the grid has the bits of the finish of the RESTATED sums, lies inside loader_grid_ref's bound of its float64 reference (the
    statistics over all C planes of a slot, as the DDD17 loader normalises the concatenated representation), and the window is
    torch.flip / slicing of it"""
    from ess_amd import hip
    (Hs, Ws), kw = GEOS[geo]
    g = LG.Geometry((Hs, Ws), **kw)
    C_, norm = E.channels(rep, bins), {'population': LG.NORM_POPULATION, 'unbiased': LG.NORM_UNBIASED}[mode]
    rows = [_row(r, Hs, Ws, 160 + r) for r in range(2)]
    slots = [(0, 5, 3000, 0), (1, 4000, 400, 1), (0, 0, 0, 0), (1, 2050, 1, 1), (0, 9, hip.INGEST_KEEP, 0), (1, 100, 2000, 1)]
    n = len(slots)
    dev, w = _upload(rows), [_words([s[k] for s in slots]) for k in range(4)]
    sums = torch.from_numpy(np.stack([E.restate_sums(_window(rows[r], s, c), rep, bins, Hs, Ws) for r, s, c, _ in slots]))
    acc = torch.zeros(n, C_, Hs, Ws, dtype=torch.int64, device=DEV)
    hip.event_scatter_ring_rep(*dev, *w, acc, REP_WORD[rep])
    assert torch.equal(acc.cpu(), sums)
    counts = torch.tensor([s[2] for s in slots])
    if window:  # (the window is cut out of all Hr rows of the resized grid)
        g = LG.Geometry((Hs, Ws), resized=(g.Hr, g.Wr))
    ref, bound = LG.reference(sums, g, norm, counts)

    def finish(a):
        buf, out = M._guarded((n, C_, g.rows, g.Wr), torch.float32)
        hip.grid_finish_workspace(n, C_, Hs, Ws, DEV).fill_(0xFF)
        hip.event_grid_finish(w[2], a, out, crop_rows=g.crop, resize=(g.Hr, g.Wr), normalize=norm)
        assert C._guards_intact(buf, out) and not bool(a.any())
        return out
    full = finish(sums.to(DEV))
    assert LG.worst_ratio(full, ref, bound) <= 1.0 and bool(torch.isnan(full[4]).all()) and not bool(full[2].any())
    if not window:
        assert torch.equal(_bits(finish(acc)), _bits(full))
        return
    h, wd = g.rows - 6, g.Wr - 12 - (g.Wr % 4)  # (a multiple of 4: the vector store) ...
    for h, wd in ((h, wd), (g.rows, g.Wr - 1)):  # ... and all rows of another width
        words = torch.tensor([[1, 3, 5, 0], [0, 6, 12, 0], [1, 0, 0, 0]], dtype=torch.int32, device=DEV)
        buf, out = M._guarded((n, C_, h, wd), torch.float32)
        hip.grid_finish_workspace(n, C_, Hs, Ws, DEV).fill_(0xFF)
        if not bool(acc.any()):
            hip.event_scatter_ring_rep(*dev, *w, acc, REP_WORD[rep])
        hip.event_grid_finish_window(w[2], acc, out, words, 2, crop_rows=g.crop, resize=(g.Hr, g.Wr), normalize=norm)
        for i in range(n):
            flip, y0, x0 = words[i // 2, :3].tolist()
            y0, x0 = min(y0, g.rows - h), min(x0, g.Wr - wd)
            assert torch.equal(_bits(out[i]), _bits(EBR.window(full[i], flip, y0, x0, h, wd))), (i, h, wd)
        assert C._guards_intact(buf, out) and not bool(acc.any())


# ---------------------------------------------------------------------------------------------- 5. the builder
BB, BT, BBINS, BCAP = 3, 3, 2, 512
BGEO = dict(grid_hw=(26, 34), grid_resize=(26, 36), height=20, width=36, crop_hw=(12, 20), crop_band=(8, 12), label_hw=(20, 34))
BCOUNTS = [300, 200, 2]


@functools.lru_cache(maxsize=None)
def _samples(seed):
    Hs, Ws = BGEO['grid_hw']
    g = np.random.default_rng(2000 + seed)
    return [(C._as_columns(R.events(n, Hs, Ws, 10 * seed + b), (b + seed) % 4), g.integers(0, 19, BGEO['label_hw']).astype(np.uint8))
            for b, n in enumerate(BCOUNTS)]


def _by_hand(rep, samples, params, normalize):
    """scatter_rep + event_grid_finish + torch.flip / slice -> events [B, T C, h, w] on the host"""
    from ess_amd import hip
    Hs, Ws = BGEO['grid_hw']
    C_ = E.channels(rep, BBINS)
    cols = [s[0] for s in samples]
    per = [c.n // BT for c in cols]
    w = [_words(v) for v in ([b for b in range(BB) for _ in range(BT)], [t * per[b] for b in range(BB) for t in range(BT)],
                             [per[b] for b in range(BB) for _ in range(BT)], [cols[b].format for b in range(BB) for _ in range(BT)])]
    acc = torch.zeros(BB * BT, C_, Hs, Ws, dtype=torch.int64, device=DEV)
    hip.event_scatter_ring_rep(*C._device_columns(cols, BCAP), *w, acc, REP_WORD[rep])
    sums = np.stack([E.restate_sums(E.Cols(*(a[t * per[b]:(t + 1) * per[b]] for a in (cols[b].t, cols[b].x, cols[b].y, cols[b].p))),
                                    rep, BBINS, Hs, Ws) for b in range(BB) for t in range(BT)])
    assert np.array_equal(acc.cpu().numpy(), sums)
    full = torch.full((BB * BT, C_, BGEO['height'], BGEO['width']), float('nan'), device=DEV)
    hip.event_grid_finish(w[2], acc, full, resize=BGEO['grid_resize'], normalize=normalize)
    full = full.cpu().view(BB, BT * C_, BGEO['height'], BGEO['width'])
    return torch.stack([EBR.window(full[b], *params[b, :3].tolist(), *BGEO['crop_hw']) for b in range(BB)])


@pytest.mark.parametrize('rep', ['separate_pol', 'histogram'])
def test_the_builder_has_the_bits_of_scatter_finish_flip_and_slice(rep):
    """[B, T C, h, w]; eager and graph=True agree with the composition by hand on four batches in a row, each still intact while
    the next is built: two builds are independent"""
    from ess_amd import hip
    from ess_amd.datasets.event_batches import EventBatchBuilder
    C_ = E.channels(rep, BBINS)
    make = lambda graph: EventBatchBuilder(BB, BT, BBINS, BCAP, **BGEO, grid_normalize='population', representation=rep, graph=graph, seed=5)  # noqa: E731
    eager, graphed = make(False), make(True)
    assert eager.channels == C_ and eager.representation == rep
    previous = None
    for k in range(4):
        samples = _samples(k)
        ev, lab = eager.build(samples)
        ev_g, lab_g = graphed.build(samples)
        assert torch.equal(eager.last_params, graphed.last_params)
        assert ev.dtype == torch.float32 and tuple(ev.shape) == (BB, BT * C_, *BGEO['crop_hw']) and tuple(lab.shape) == (BB, *BGEO['crop_hw'])
        want = _by_hand(rep, samples, eager.last_params, hip.GRID_NORM_POPULATION)
        assert torch.equal(_bits(ev.cpu()), _bits(want)) and torch.equal(_bits(ev_g.cpu()), _bits(want)) and torch.equal(lab, lab_g), k
        # (a window whose counts are all 1 has a population std of 0: NaN at its events, as normalize_voxel_grid gives it)
        assert bool(ev[0].any()) and not bool(ev[2].any()) and bool(ev[1].isfinite().any())
        if previous is not None:
            assert torch.equal(_bits(previous[0].cpu()), _bits(previous[1])), (k, 'the batch before')
        previous = (ev, want)
    assert not bool(eager._static['acc'].any()) and tuple(eager._static['acc'].shape) == (BB * BT, C_, *BGEO['grid_hw'])
    assert graphed.n_captures == 2 and eager.n_captures == 0


# ---------------------------------------------------------------------------------------------- 6. the segmenters
SH_, SW_, K, SCAP = 64, 96, 11, 512
MODELS = {'histogram': 2, 'separate_pol': 4}  # representation -> the encoder's num_bins (separate: 2 bins)


@functools.lru_cache(maxsize=None)
def _weights(num_bins):
    from oracle import ess_oracle as O
    cfg = O.e2vid_config(num_bins=num_bins, recurrent_block_type='convlstm')
    return cfg, O.synth_state_dict(O.e2vid_param_shapes(cfg), 171), O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True)


def _stream_segmenter(num_bins, S, **kw):
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_segmentation import MultiStreamSegmenter
    return MultiStreamSegmenter(*M._models(*_weights(num_bins), K), SH_, SW_, default_options(), S, palette=SH.palette_for(K),
                                want_confidence=True, **kw)


@functools.lru_cache(maxsize=None)
def _source(s, fmt, n=1536):
    return C._as_columns(M._events(n, SH_, SW_, 300 + 10 * s + fmt), fmt)


def _cut(c, a, b):
    from ess_amd.datasets.data_util import EventColumns
    return EventColumns(*(np.ascontiguousarray(v[a:b]) for v in (c.t, c.x, c.y, c.p)))


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('layout', ['columns', 'ring'])
@pytest.mark.parametrize('rep', ['separate_pol', 'histogram'])
def test_stream_rounds_from_events_equal_rounds_from_the_restated_grids(rep, layout, graph):
    """S = 2, three rounds (both streams, stream 1 alone, both): update_from_events / update_from_feed with representation= against
    update(grids) of a twin that is handed the restated grids; eager and graph=True both equal the one eager twin"""
    from ess_amd import hip
    S, nb = 2, MODELS[rep]
    bins = nb // 2 if rep == 'separate_pol' else 1
    hip.set_compute('bf16')
    try:
        kw = dict(window_events=SCAP) if layout == 'ring' else {}
        seg = _stream_segmenter(nb, S, graph=graph, event_capacity=SCAP, event_layout=layout, representation=rep, **kw)
        twin = _stream_segmenter(nb, S)
        assert seg.representation == rep and tuple(seg._acc.shape) == (S, nb, SH_, SW_)
        src = [_source(s, (1, 2)[s]) for s in range(S)]
        for r, active in enumerate([(True, True), (False, True), (True, True)]):
            wins = [_cut(src[s], r * SCAP, (r + 1) * SCAP) if active[s] else None for s in range(S)]
            if layout == 'ring':
                for s in range(S):
                    if wins[s] is not None:
                        seg.feed(s, wins[s])
                got = seg.update_from_feed()
            else:
                got = seg.update_from_events(wins)
            grids = torch.zeros(S, nb, SH_, SW_)
            for s in range(S):
                if wins[s] is not None:
                    grids[s] = torch.from_numpy(E.restate(wins[s], rep, bins, SH_, SW_))
            want = twin.update(grids.to(DEV), active=list(active))
            C._assert_rows(got, want, active, f'{rep} {layout} graph={graph} round {r}')
            assert got.confidence[1].unique().numel() > 1
        torch.cuda.synchronize()
        assert not bool(seg._acc.any()) and seg.n_captures == (1 if graph else 0)
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('rep', ['separate_pol', 'histogram'])
def test_sequence_rounds_from_events_equal_rounds_from_the_restated_grids(rep, graph):
    """S = 2, T = 3 windows of 256 events: segment_at(end=) with representation= against the round behind its grids (_round_from)
    of a twin that is handed the restated grids of the same windows, slot t S + s; two rounds, the second across the ring's wrap;
    through the plain ingest, and through event_scatter_ring_rep + event_grid_finish (grid_normalize='population': the statistics
    over all C planes of a slot)"""
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    S, T, NW, nb = 2, 3, 256, MODELS[rep]
    bins = nb // 2 if rep == 'separate_pol' else 1
    hip.set_compute('bf16')
    try:
        make = lambda **kw: SequenceSegmenter(*M._models(*_weights(nb), K), SH_, SW_, default_options(), S, sequence_steps=T,  # noqa: E731
                                              window_events=NW, ring_capacity=1024, palette=SH.palette_for(K), want_confidence=True, **kw)
        seg, twin = make(representation=rep, graph=graph), make()
        normed = make(representation=rep, graph=graph, grid_normalize='population')
        src = [_source(s, (3, 0)[s]) for s in range(S)]
        fed = 0
        for r, end in enumerate((T * NW, 1400)):
            for s in range(S):
                seg.feed(s, _cut(src[s], fed, end))
                normed.feed(s, _cut(src[s], fed, end))
            fed = end
            got = seg.segment_at(end=[end] * S)
            got_n = normed.segment_at(end=[end] * S)
            start = end - T * NW
            sums = np.stack([E.restate_sums(_cut(src[s], start + t * NW, start + (t + 1) * NW), rep, bins, SH_, SW_)
                             for t in range(T) for s in range(S)])
            ev = torch.from_numpy(E.dequantise(sums)).to(DEV)
            want = twin._round_from(ev)
            for s in range(S):
                assert M._same(M._row(got, s), tuple(o[s] for o in want)), (rep, graph, r, s)
            # the loader grid: the finish of the RESTATED sums (a pure function of them, pinned by tests/test_hip_loader_grid.py)
            ev_n = torch.full((T * S, nb, SH_, SW_), float('nan'), device=DEV)
            hip.event_grid_finish(_words([NW] * (T * S)), torch.from_numpy(sums).to(DEV), ev_n, normalize=hip.GRID_NORM_POPULATION)
            want_n = twin._round_from(ev_n)
            for s in range(S):
                assert M._same(M._row(got_n, s), tuple(o[s] for o in want_n)), (rep, graph, r, s, 'grid_normalize')
            assert got.valid == (True, True) and got.confidence[0].unique().numel() > 1
        torch.cuda.synchronize()
        assert not bool(seg._acc.any()) and tuple(seg._acc.shape) == (T * S, nb, SH_, SW_) and seg.n_captures == (1 if graph else 0)
    finally:
        hip.set_compute('fp32')
