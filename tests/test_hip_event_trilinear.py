"""GPU tier of the rectified trilinear event ingest: hip.event_ingest_columns_trilinear / hip.event_ingest_ring_trilinear (raw event
columns -> rectify-map lookup -> eight-corner fixed-point scatter) and MultiStreamSegmenter(voxel='trilinear', rectify_maps=).  What
is asserted throughout is BITS: a grid equals the numpy restatement of tests/test_host_event_trilinear.py (which that file pins to the
reference's VoxelGrid.convert), the ring kernel equals the column kernel on the same windows, and a trilinear segmenter's labels,
colours and confidences equal those of a twin that is handed the restatement's grids through update(grids)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_event_columns as C  # noqa: E402  (bits, words, guards, result rows)
from tests import test_hip_event_ring as RG  # noqa: E402  (the starts of wrapping windows at every residue)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers, the pins)
from tests import test_hip_stream_compaction as SC  # noqa: E402  (the 64 x 96 models)
from tests import test_host_event_trilinear as T  # noqa: E402  (the restatement, synthetic maps and raw events)

DEV = M.DEV
NAN16 = M.NAN16
NB, H, W, MH, MW = 5, 24, 40, 28, 44  # the sensor (the map) is larger than the grid
NONE = T.NONE
_bits, _words = C._bits, C._words


@functools.lru_cache(maxsize=None)
def _maps(mh=MH, mw=MW, h=H, w=W):
    """two different maps of one sensor -> host [2, mh, mw, 2]"""
    return np.stack([T.synthetic_map(mh, mw, h, w, 1), T.synthetic_map(mh, mw, h, w, 2)])


def _map_for(maps, word):
    return None if word == NONE else maps[word]


def _raw(c):
    """a window's four columns as raw words: t 8 bytes (a float64 time as its bits), x / y 2 bytes, p 1 byte"""
    return (np.ascontiguousarray(c.t).view(np.int64), np.ascontiguousarray(c.x).view(np.int16), np.ascontiguousarray(c.y).view(np.int16),
            np.ascontiguousarray(c.p).view(np.uint8))


def _filler(host, i, c):
    """every entry of row i: an event that WOULD land (a time from the middle of window c, raw pixel (1, 1), positive) -- a kernel
    that read outside its window would show"""
    host[0][i] = _raw(c)[0][(c.n - 1) // 2] if c.n else 0
    host[1][i], host[2][i], host[3][i] = 1, 1, 1


def _dev_columns(wins, stride):
    host = [np.zeros((len(wins), stride), d) for d in (np.int64, np.int16, np.int16, np.uint8)]
    for i, c in enumerate(wins):
        _filler(host, i, c)
        for a, v in zip(host, _raw(c)):
            a[i, :c.n] = v
    return tuple(torch.from_numpy(a).to(DEV) for a in host)


def _dev_rings(wins, starts, ring):
    """row i: window i laid out from starts[i] on, modulo ring, filler everywhere else"""
    host = [np.zeros((len(wins), ring), d) for d in (np.int64, np.int16, np.int16, np.uint8)]
    for i, (c, s) in enumerate(zip(wins, starts)):
        _filler(host, i, c)
        at = (s + np.arange(c.n)) % ring
        for a, v in zip(host, _raw(c)):
            a[i, at] = v
    return tuple(torch.from_numpy(a).to(DEV) for a in host)


def _expected(wins, map_of, maps, nb=NB, h=H, w=W):
    return torch.from_numpy(np.stack([T.restate(c, _map_for(maps, m), nb, h, w) for c, m in zip(wins, map_of)])).to(DEV)


def _by_columns(wins, map_of, maps, stride, counts=None, formats=None, nb=NB, h=H, w=W, n_maps=None):
    """-> (out inside its NaN-pre-filled guarded buffer, the buffer, acc)"""
    from ess_amd import hip
    n = len(wins)
    buf, out = M._guarded((n, nb, h, w), torch.float32)
    acc = torch.zeros(n * nb * h * w, dtype=torch.int64, device=DEV)
    dmaps = None if maps is None else torch.from_numpy(maps[:n_maps]).to(DEV)
    got = hip.event_ingest_columns_trilinear(*_dev_columns(wins, stride), _words([c.n for c in wins] if counts is None else counts),
                                             _words([c.format for c in wins] if formats is None else formats), out, dmaps, _words(map_of), acc)
    assert got is out
    return out, buf, acc


def _by_ring(wins, starts, map_of, maps, ring, counts=None, nb=NB, h=H, w=W):
    from ess_amd import hip
    n = len(wins)
    buf, out = M._guarded((n, nb, h, w), torch.float32)
    acc = torch.zeros(n * nb * h * w, dtype=torch.int64, device=DEV)
    got = hip.event_ingest_ring_trilinear(*_dev_rings(wins, starts, ring), _words(list(range(n))), _words(starts),
                                          _words([c.n for c in wins] if counts is None else counts), _words([c.format for c in wins]), out,
                                          None if maps is None else torch.from_numpy(maps).to(DEV), _words(map_of), acc=acc)
    assert got is out
    return out, buf, acc


# ---------------------------------------------------------------------------------------------- 1. the kernels
COUNTS = [1, 2, 3, 4, 5, 17, 1000]


@pytest.mark.parametrize('count', COUNTS, ids=[f'n{c}' for c in COUNTS])
def test_column_and_ring_kernels_against_the_restatement(count):
    """eight windows of `count` events, all four format words twice, map words 0, 1 and RECTIFY_NONE: the column kernel from entry
    0, the ring kernel from a start at every residue mod 4 -- slots 0 .. 3 without a wrap, slots 4 .. 7 from the last four positions of
    the ring (the window wraps behind its head group wherever it is long enough to) -- each against the restatement, and against each
    other"""
    maps = _maps()
    ring = 32 if count <= 17 else 1024
    wins = [T.raw_events(count, MH, MW, 100 * count + i, fmt=i % 4) for i in range(8)]
    assert [c.format for c in wins] == [0, 1, 2, 3] * 2
    map_of = [0, 1, NONE, 1, 1, NONE, 0, 0]
    starts = [0, 1, 2, 3] + (RG._starts(count, 'late') if ring == RG.RING else [ring - 4 + j for j in range(4)])
    assert [s % 4 for s in starts] == [0, 1, 2, 3] * 2 and all(s + count <= ring for s in starts[:4])
    if count >= 5:
        assert all(s + count > ring for s in starts[4:])
    want = _expected(wins, map_of, maps)
    cols, buf_c, acc_c = _by_columns(wins, map_of, maps, ring)
    rng, buf_r, acc_r = _by_ring(wins, starts, map_of, maps, ring)
    for i in range(8):
        assert torch.equal(_bits(cols[i]), _bits(want[i])), f'columns, window {i} (format {wins[i].format}, map {map_of[i]})'
        assert torch.equal(_bits(rng[i]), _bits(want[i])), f'ring, slot {i} (start {starts[i]}, format {wins[i].format}, map {map_of[i]})'
    assert torch.equal(_bits(cols), _bits(rng))
    if count >= 17:
        assert all(bool(want[i].any()) for i in range(8))
    assert C._guards_intact(buf_c, cols) and C._guards_intact(buf_r, rng) and not bool(acc_c.any()) and not bool(acc_r.any())


EDGE_VALUES = [float('nan'), float('inf'), float('-inf'), -2.0, -1.5, -1.0, -0.25, W - 0.5, float(W), 1e30, -1e30, 0.0, 3.0, W - 1.0,
               H - 0.5, float(H), H - 1.0, 7.25]


def _edge_window():
    """one window and its map: entry [0, i] = (EDGE_VALUES[i], 5.25), entry [1, i] = (7.5, EDGE_VALUES[i]), entry [2, i] = both; two
    events (the four polarity bytes 0, 1, 255, 2 in turn) on each, then raw coordinates outside the map and uint16 coordinates >= 32768"""
    rmap = T.synthetic_map(MH, MW, H, W, 3)
    k = len(EDGE_VALUES)
    assert k <= MW
    for i, v in enumerate(EDGE_VALUES):
        rmap[0, i] = (v, 5.25)
        rmap[1, i] = (7.5, v)
        rmap[2, i] = (v, v)
    x = np.concatenate([np.repeat(np.arange(k), 2)] * 3 + [[MW, MW + 5, 3, 3, 32768, 40000, 65535, 2, 2]]).astype(np.uint16)
    y = np.concatenate([np.repeat(r, 2 * k) for r in (0, 1, 2)] + [[3, 3, MH, MH + 9, 1, 1, 1, 32768, 65535]]).astype(np.uint16)
    n = len(x)
    g = np.random.default_rng(5)
    t = np.sort(g.integers(0, 50_000, n)).astype(np.int64) + 1_600_000_000_000_000
    p = np.tile(np.array([0, 1, 255, 2], np.uint8), n)[:n]
    return T.Cols(t, x, y, p), rmap


def test_edge_words_in_one_call():
    """slot 0: the edge window through its map -- NaN, +-inf, -2, -1.5, -1, -0.25, W - 0.5, W, +-1e30 and exact integers as map
    entries, raw pixels outside the map, uint16 coordinates >= 32768, polarity bytes 0, 1, 255, 2;  1: the same window, RECTIFY_NONE;
    2: every time equal: an all-zero grid;  3 .. 5: a map word out of range: an all-zero grid;  6: ESS_INGEST_KEEP: the grid stays;
    7: an unknown format bit: an all-zero grid.  The same through the ring kernel from unaligned starts; acc all zero behind both."""
    from ess_amd import hip
    edge, rmap = _edge_window()
    maps = np.stack([rmap, _maps()[0]])
    same = T.Cols(np.full(edge.n, 1_600_000_000_000_123, np.int64), edge.x, edge.y, edge.p)
    plain = T.raw_events(200, MH, MW, 9)
    wins = [edge, edge, same, plain, plain, plain, plain, plain]
    map_of = [0, NONE, 0, 2, -2, 1 << 30, 1, 1]
    counts = [edge.n, edge.n, edge.n, 200, 200, 200, hip.INGEST_KEEP, 200]
    formats = [c.format for c in wins[:7]] + [plain.format | 4]
    want = _expected(wins[:2], map_of[:2], maps)
    # what the restatement itself must show of the edges: -1.5 and -1.0 reach column 0, W - 0.5 reaches column W - 1, the rest is dropped
    idx, con = T.contributions(edge, rmap, NB, H, W)
    assert len(idx) and np.isfinite(con).all() and np.abs(con).max() <= 1 and bool(want[0].any()) and bool(want[1].any())
    assert bool((want[0][:, :, 0] < 0).any() | (want[0][:, :, 0] > 0).any()) and bool(want[0][:, :, W - 1].any())
    cols, buf, acc = _by_columns(wins, map_of, maps, 256, counts=counts, formats=formats)
    for i in (0, 1):
        assert torch.equal(_bits(cols[i]), _bits(want[i])), i
    for i in (2, 3, 4, 5, 7):
        assert not bool(_bits(cols[i]).any()), f'slot {i}: map word {map_of[i]}, format {formats[i]}'
    assert bool((cols[6].view(torch.int16) == NAN16).all())
    assert C._guards_intact(buf, cols) and not bool(acc.any())
    starts = [5, 254, 3, 0, 0, 0, 0, 0]
    rng, buf, acc = _by_ring(wins[:7], starts[:7], map_of[:7], maps, 256, counts=counts[:7])
    assert torch.equal(_bits(rng[:6]), _bits(cols[:6])) and bool((rng[6].view(torch.int16) == NAN16).all())
    assert C._guards_intact(buf, rng) and not bool(acc.any())
    # no maps at all: maps=None, map_of=None -- RECTIFY_NONE throughout
    out = torch.full((1, NB, H, W), float('nan'), device=DEV)
    hip.event_ingest_columns_trilinear(*_dev_columns([edge], 256), _words([edge.n]), _words([edge.format]), out)
    assert torch.equal(_bits(out[0]), _bits(want[1]))


def test_the_grid_does_not_depend_on_the_event_order():
    """events 1 .. n - 2 permuted (the first and the last, which set the time scale, in place): bit-identical grids; two consecutive
    runs: bit-identical grids"""
    maps = _maps()
    c = T.raw_events(2000, MH, MW, 51)
    g = np.random.default_rng(53)
    out0, _, _ = _by_columns([c], [1], maps, 2048)
    again, _, _ = _by_columns([c], [1], maps, 2048)
    assert torch.equal(_bits(out0), _bits(again))
    for k in range(3):
        order = np.concatenate([[0], 1 + g.permutation(c.n - 2), [c.n - 1]])
        perm = T.Cols(*(np.ascontiguousarray(a[order]) for a in (c.t, c.x, c.y, c.p)))
        out1, _, _ = (_by_columns([perm], [1], maps, 2048) if k else _by_ring([perm], [1027], [1], maps, 2048))
        assert torch.equal(_bits(out0), _bits(out1)), k
    assert torch.equal(_bits(out0), _bits(_expected([c], [1], maps)))


def test_many_contributions_on_eight_voxels():
    """4096 events on ONE map entry (7.3, 11.6), mixed polarity, two bins: every event but the last adds to the same eight voxels"""
    rmap = T.synthetic_map(MH, MW, H, W, 4)
    rmap[9, 13] = (7.3, 11.6)
    n = 4096
    g = np.random.default_rng(61)
    t = np.sort(g.uniform(1.0, 1.5, n))
    c = T.Cols(t, np.full(n, 13, np.int16), np.full(n, 9, np.int16), g.integers(0, 2, n).astype(np.uint8))
    maps = rmap[None]
    want = _expected([c], [0], maps, nb=2)
    assert int(torch.count_nonzero(want)) == 8 and bool((want[0, :, 11:13, 7:9] != 0).all())
    out, buf, acc = _by_columns([c], [0], maps, 4096, nb=2)
    assert torch.equal(_bits(out), _bits(want)) and C._guards_intact(buf, out) and not bool(acc.any())
    rng, buf, acc = _by_ring([c], [2049], [0], maps, 4096, nb=2)
    assert torch.equal(_bits(rng), _bits(want)) and C._guards_intact(buf, rng) and not bool(acc.any())


def test_a_larger_call_that_spans_several_blocks():
    """40 000 events per stream (40 blocks of 256 lanes x 4 events), 3 streams, two maps and a stream without one, 64 x 96 grid under
    a 72 x 104 sensor"""
    h, w, mh, mw, n = 64, 96, 72, 104, 40_000
    maps = _maps(mh, mw, h, w)
    wins = [T.raw_events(n, mh, mw, 70 + s, fmt=(3, 0, 1)[s]) for s in range(3)]
    map_of = [1, 0, NONE]
    want = _expected(wins, map_of, maps, NB, h, w)
    out, buf, acc = _by_columns(wins, map_of, maps, n, h=h, w=w)
    for s in range(3):
        assert torch.equal(_bits(out[s]), _bits(want[s])) and bool(out[s].any()), s
    assert C._guards_intact(buf, out) and not bool(acc.any())
    rng, buf, acc = _by_ring(wins, [39_999, 2, 20_001], map_of, maps, n, h=h, w=w)
    assert torch.equal(_bits(rng), _bits(out)) and C._guards_intact(buf, rng) and not bool(acc.any())


# ---------------------------------------------------------------------------------------------- 2. the segmenter
SH_, SW_, SMH, SMW = SC.H, SC.W, 72, 104
CAP, RCAP, WIN = 512, 1024, 512
SEG_CASES = [(mode, graph) for mode in ('mixed', 'bf16') for graph in (False, True)]
SEG_IDS = [f'{mode}-{"graph" if graph else "eager"}' for mode, graph in SEG_CASES]


@functools.lru_cache(maxsize=None)
def _rig():
    """two maps of the 72 x 104 sensor over the 64 x 96 grid; stream 2 has none"""
    left, right = _maps(SMH, SMW, SH_, SW_)
    return [np.ascontiguousarray(left), np.ascontiguousarray(right), None]


@functools.lru_cache(maxsize=None)
def _source(s, n=2048):
    """stream s's whole event sequence, built once: stream 0 int64 / uint16, 1 float64 / int16, 2 int64 / int16"""
    return T.raw_events(n, SMH, SMW, 900 + s, fmt=(3, 0, 1)[s], t_span_us=200_000)


def _window(s, k):
    return RG._slice(_source(s), k * WIN, (k + 1) * WIN)


@functools.lru_cache(maxsize=None)
def _grid(s, k):
    """the restatement's grid of window k of stream s, on the device, built once"""
    return torch.from_numpy(T.restate(_window(s, k), _rig()[s], SC.C, SH_, SW_)).to(DEV)


def _segmenter(S, layout, graph, maps, **kw):
    if layout == 'ring':
        kw = dict(ring_capacity=RCAP, window_events=WIN, **kw)
    return SC._segmenter('convlstm', S, graph=graph, event_capacity=CAP, event_layout=layout, voxel='trilinear', rectify_maps=maps, **kw)


def _trilinear_round(seg, layout, windows, sources=(0, 1, 2)):
    """windows: per stream of seg the number of its next window or None; sources: whose events each stream delivers -> the round's
    result, from feed() + update_from_feed() or from update_from_events()"""
    if layout == 'ring':
        for s, k in enumerate(windows):
            if k is not None:
                seg.feed(s, _window(sources[s], k))
        return seg.update_from_feed()
    return seg.update_from_events([None if k is None else _window(sources[s], k) for s, k in enumerate(windows)])


# per round: the window number of every stream, None: idle
ROUNDS = [(0, 0, 0), (1, None, 1), (2, 1, None), (3, 2, 2)]


@pytest.mark.parametrize('layout', ['ring', 'columns'])
@pytest.mark.parametrize('mode,graph', SEG_CASES, ids=SEG_IDS)
def test_trilinear_rounds_equal_update_on_the_restated_grids(mode, graph, layout):
    """S = 3, two different maps and stream 2 without one: every round from feed() / update_from_events() equals update(grids) of a
    twin segmenter fed the restatement's grids -- labels, colours, confidence bits -- with a reset on the way and ONE capture; and
    each stream equals itself alone in an n_streams=1 segmenter (both batch-size-dependent dispatch choices pinned)"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    S = 3
    hip.set_compute(mode)
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        rig = _rig()
        seg = _segmenter(S, layout, graph, rig)
        twin = SC._segmenter('convlstm', S, graph=graph)
        alone = [_segmenter(1, layout, graph, [rig[s]]) for s in range(S)]
        assert seg.voxel == 'trilinear' and tuple(seg._maps.shape) == (2, SMH, SMW, 2) and seg._map_of == [0, 1, NONE]
        assert tuple(seg._words.shape) == ((5, S) if layout == 'ring' else (3, S)) and all(st.words.shape == seg._words.shape for st in seg._stage)
        assert alone[2]._maps is None and tuple(alone[1]._maps.shape) == (1, SMH, SMW, 2)
        for r, windows in enumerate(ROUNDS):
            if r == 2:
                for sg in (seg, twin, alone[0]):
                    sg.reset([0])
            on = [k is not None for k in windows]
            got = _trilinear_round(seg, layout, windows)
            grids = torch.stack([_grid(s, k) if k is not None else torch.zeros_like(_grid(s, 0)) for s, k in enumerate(windows)])
            C._assert_rows(got, twin.update(grids, on), on, f'{mode} graph={graph} {layout} round {r}')
            for s, k in enumerate(windows):
                if k is not None:
                    one = _trilinear_round(alone[s], layout, [k], [s])
                    assert M._same(M._row(got, s), M._row(one, 0)), f'{mode} graph={graph} {layout} round {r}: stream {s} alone'
            torch.cuda.synchronize()
            words = seg._words.cpu()[-1].tolist()
            assert words == [m if a else NONE for m, a in zip(seg._map_of, on)], (r, 'idle slots keep RECTIFY_NONE')
        assert not bool(seg._acc.any())
        assert seg.n_captures == twin.n_captures == (1 if graph else 0) and all(a.n_captures == (1 if graph else 0) for a in alone)
        assert seg.n_windows == len(ROUNDS)
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')


@pytest.mark.parametrize('layout', ['ring', 'columns'])
@pytest.mark.parametrize('mode,graph', SEG_CASES, ids=SEG_IDS)
def test_compacted_trilinear_rounds_equal_the_uncompacted(mode, graph, layout):
    """S = 3, compact=True with buckets [1, 2]: rounds with 3, 1 (stream 1 alone, in slot 0), 2 (streams 0 and 2) and 1 (stream 2)
    active streams equal the uncompacted segmenter's bit for bit -- the map word follows the slot: slot i reads the map of the stream
    in slot i, a padded slot RECTIFY_NONE"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    S = 3
    hip.set_compute(mode)
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        rig = _rig()
        ride = _segmenter(S, layout, graph, rig)
        comp = _segmenter(S, layout, graph, rig, compact=True, compact_buckets=[1, 2])
        assert comp.buckets == (1, 2)
        rounds = [(0, 0, 0), (None, 1, None), (1, None, 1), (None, None, 2), (2, 2, 3)]
        for r, windows in enumerate(rounds):
            if r == 2:
                comp.reset([2])
                ride.reset([2])
            on = [k is not None for k in windows]
            got, want = _trilinear_round(comp, layout, windows), _trilinear_round(ride, layout, windows)
            C._assert_rows(got, want, on, f'{mode} graph={graph} {layout} round {r}')
            streams = [s for s in range(S) if on[s]]
            b = next((b for b in comp.buckets if b >= len(streams)), None)
            if b is not None:
                torch.cuda.synchronize()
                words = comp._words.cpu()[-1].tolist()
                assert words[:b] == [comp._map_of[s] for s in streams] + [NONE] * (b - len(streams)), (r, 'the map word follows the slot')
                for slot, s in enumerate(streams):
                    assert torch.equal(_bits(comp.compact_input[slot]), _bits(_grid(s, windows[s]))), (r, slot, 'compact input')
        assert comp.n_captures <= (len(comp.buckets) + 1 if graph else 0) and ride.n_captures == (1 if graph else 0)
        assert not bool(comp._acc.any()) and not bool(ride._acc.any())
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')


def test_warm_up_covers_every_bucket_of_a_trilinear_segmenter():
    from ess_amd import hip
    hip.set_compute('bf16')
    try:
        comp = _segmenter(3, 'ring', True, _rig(), compact=True, compact_buckets=[1, 2])
        comp.warm_up()
        n = comp.n_captures
        assert n == len(comp.buckets) + 1
        for windows in ((0, 0, 0), (None, 1, None), (1, None, 1)):
            _trilinear_round(comp, 'ring', windows)
        assert comp.n_captures == n
    finally:
        hip.set_compute('fp32')
