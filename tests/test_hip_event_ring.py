"""GPU tier of the continuous event feed: hip.event_ingest_ring (windows named inside per-stream event rings by four device words
per slot) and MultiStreamSegmenter(event_layout='ring').  What is asserted throughout is BITS: a grid equals the numpy restatement of
tests/test_host_event_ingest.py on the window UNROLLED into a contiguous array, and hip.event_ingest_columns on that same array; a
'ring' segmenter's labels, colours and confidences equal a 'columns' segmenter's that is handed the same windows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_event_columns as C  # noqa: E402  (columns from rows, device columns with landing filler, expected grids)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers, events, result rows, the pins)
from tests import test_hip_stream_compaction as SC  # noqa: E402  (the 64 x 96 models)
from tests import test_host_event_ingest as R  # noqa: E402  (the restatement)

DEV = M.DEV
NAN16 = M.NAN16
NB, H, W, RING = 5, 24, 40, 32
_bits, _words = C._bits, C._words


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _columns_of(a, fmt):
    return C._as_columns(a, fmt)


def _full_rows(n_rows, fmts, seed, ring=RING):
    """per row a FULL ring of events that all lie inside the grid, times unsorted over the ring's positions: whatever a kernel reads
    outside its window is an event that may well land -> list of EventColumns (ring events each)"""
    rows = []
    for r in range(n_rows):
        ev = R.events(ring, H, W, seed + r)
        ev[:, 0] = np.random.default_rng(seed + 100 + r).permutation(ev[:, 0])
        rows.append(_columns_of(ev, fmts[r]))
    return rows


def _unrolled(row, start, count, ring=RING):
    """the window (start, count) of a full row as a contiguous EventColumns"""
    from ess_amd.datasets.data_util import EventColumns
    idx = (start + np.arange(min(count, ring))) % ring
    return EventColumns(*(np.ascontiguousarray(a[idx]) for a in (row.t, row.x, row.y, row.p)))


def _ring_call(rows, slots, out=None, acc=None, ring=RING):
    """slots: (row, start, count, format) per slot -> (out inside its NaN-pre-filled guarded buffer, the buffer, acc)"""
    from ess_amd import hip
    n = len(slots)
    buf = None
    if out is None:
        buf, out = M._guarded((n, NB, H, W), torch.float32)
    if acc is None:
        acc = torch.zeros(n * NB * H * W, dtype=torch.int64, device=DEV)
    dev = C._device_columns(rows, ring)
    assert all(tuple(d.shape) == (len(rows), ring) for d in dev)
    got = hip.event_ingest_ring(*dev, *(_words([s[k] for s in slots]) for k in range(4)), out, acc=acc)
    assert got is out
    return out, buf, acc


def _columns_call(wins):
    """hip.event_ingest_columns on the unrolled windows, one stream each -> grids [n, NB, H, W]"""
    from ess_amd import hip
    out = torch.full((len(wins), NB, H, W), float('nan'), device=DEV)
    return hip.event_ingest_columns(*C._device_columns(wins, RING), _words([c.n for c in wins]), _words([c.format for c in wins]), out)


COUNTS = [1, 2, 3, 4, 5, 7, 8, 31, 32]


def _starts(count, wrap):
    """one start per residue 0 .. 3 mod 4.  'late': the last positions of the ring, 28 + j -- the window wraps right behind its head
    group (4 - j events in front of the wrap); 'early': the first start of that residue whose window still wraps, so the wrap falls
    into the window's tail group (where no start of the residue wraps -- count 1 at residues 0 .. 2, say --: the start 28 + j)"""
    out = []
    for j in range(4):
        s = RING - 4 + j
        if wrap == 'early':
            fits = [v for v in range(j, RING, 4) if v + count > RING]
            s = fits[0] if fits else s
        out.append(s)
    return out


@pytest.mark.parametrize('wrap', ['late', 'early'])
@pytest.mark.parametrize('count', COUNTS, ids=[f'n{c}' for c in COUNTS])
def test_windows_that_wrap_at_every_start_residue(count, wrap):
    """ring = 32, 3 rows, 4 slots whose starts cover the residues 0 .. 3 mod 4: the rows permuted (slot 0 reads row 2, slot 1 row 0,
    slot 3 row 1) and row 2 read by two slots.  The counts cover the head mask alone, the tail mask alone, head and tail in ONE group,
    the wrap inside the window and the full ring from an unaligned start; the positions outside every window hold events that land."""
    fmts = [0, 3, 0]
    rows = _full_rows(3, fmts, 200 + count)
    starts = _starts(count, wrap)
    assert [s % 4 for s in starts] == [0, 1, 2, 3]
    if count >= 5:
        assert all(s + count > RING for s in starts)  # every window wraps
    if count == 32 and wrap == 'early':
        assert starts == [4, 1, 2, 3]                 # (the full ring: from an aligned start that is not 0, and from 1, 2, 3)
    slot_rows = [2, 0, 2, 1]
    slots = [(r, s, count, fmts[r]) for r, s in zip(slot_rows, starts)]
    wins = [_unrolled(rows[r], s, count) for r, s in zip(slot_rows, starts)]
    out, buf, acc = _ring_call(rows, slots)
    by_columns = _columns_call(wins)
    for i, c in enumerate(wins):
        assert torch.equal(_bits(out[i]), _bits(C._expected(c))), f'slot {i}: start {starts[i]} count {count}'
        assert torch.equal(_bits(out[i]), _bits(by_columns[i])), f'slot {i} against event_ingest_columns'
        assert bool(out[i].any())
    assert C._guards_intact(buf, out)
    assert not bool(acc.any())
    first = out.clone()
    buf.fill_(NAN16)
    _ring_call(rows, slots, out=out, acc=acc)
    assert torch.equal(_bits(out), _bits(first)) and not bool(acc.any()) and C._guards_intact(buf, out)


def test_a_larger_ring_more_than_one_block():
    """ring = 4096 (four blocks of 256 lanes x 4 events), windows of 3000 and 4096 events that wrap from unaligned starts, and
    acc=None: allocated and zeroed by the call"""
    from ess_amd import hip
    ring = 4096
    fmts = [1, 2]
    rows = [_columns_of(R.events(ring, H, W, 300 + r), fmts[r]) for r in range(2)]
    slots = [(1, 2047, 3000, fmts[1]), (0, 4093, 4096, fmts[0]), (1, 1, 1025, fmts[1])]
    wins = [_unrolled(rows[r], s, n, ring) for r, s, n, _ in slots]
    out, buf, acc = _ring_call(rows, slots, ring=ring)
    for i, c in enumerate(wins):
        assert torch.equal(_bits(out[i]), _bits(C._expected(c))) and bool(out[i].any()), i
    assert C._guards_intact(buf, out) and not bool(acc.any())
    got = hip.event_ingest_ring(*C._device_columns(rows, ring), *(_words([s[k] for s in slots]) for k in range(4)), torch.empty_like(out))
    assert torch.equal(_bits(got), _bits(out))


def test_all_four_formats_in_one_call():
    from ess_amd import hip
    fmts = [0, hip.EVCOL_T_I64, hip.EVCOL_XY_U16, hip.EVCOL_T_I64 | hip.EVCOL_XY_U16]
    rows = _full_rows(4, fmts, 400)
    assert [c.format for c in rows] == fmts
    slots = [(3, 30, 9, fmts[3]), (2, 5, 20, fmts[2]), (1, 17, 32, fmts[1]), (0, 27, 6, fmts[0])]
    wins = [_unrolled(rows[r], s, n) for r, s, n, _ in slots]
    out, buf, acc = _ring_call(rows, slots)
    by_columns = _columns_call(wins)
    for i, c in enumerate(wins):
        assert torch.equal(_bits(out[i]), _bits(C._expected(c))) and torch.equal(_bits(out[i]), _bits(by_columns[i])) and bool(out[i].any()), i
    assert C._guards_intact(buf, out) and not bool(acc.any())


def test_edge_words():
    """count 0: zeros; INGEST_KEEP: the pre-filled grid stays; a row of -1, a row of n_rows, a start of -1, a start of ring and an
    unknown format bit: zeros, nothing read; a count above ring: as ring"""
    from ess_amd import hip
    fmts = [0, 3]
    rows = _full_rows(2, fmts, 500)
    slots = [(0, 7, 0, 0), (1, 7, hip.INGEST_KEEP, 3), (-1, 7, 9, 0), (2, 7, 9, 0), (0, -1, 9, 0), (0, RING, 9, 0), (1, 7, 9, 3 | 4),
             (1, 7, RING + 5, 3), (1, 7, RING, 3), (0, 7, 9, 0), (0, 7, -7, 0), (1 << 30, 0, 9, 0), (0, 1 << 30, 9, 0), (0, 7, 9, -1)]
    out, buf, acc = _ring_call(rows, slots)
    for i in (0, 2, 3, 4, 5, 6, 11, 12, 13):
        assert not bool(_bits(out[i]).any()), f'slot {i} {slots[i]}'
    for i in (1, 10):  # (the NaN pre-fill, every bit of it)
        assert bool((out[i].view(torch.int16) == NAN16).all()), i
    assert torch.equal(_bits(out[7]), _bits(out[8])) and torch.equal(_bits(out[8]), _bits(C._expected(_unrolled(rows[1], 7, RING))))
    assert torch.equal(_bits(out[9]), _bits(C._expected(_unrolled(rows[0], 7, 9)))) and bool(out[9].any()) and bool(out[8].any())
    assert C._guards_intact(buf, out) and not bool(acc.any())


def test_event_ingest_ring_argument_errors():
    """ESS_EINVAL with a message, in front of any launch; the binding's refusals on device tensors; then the same call with nothing
    wrong runs right"""
    from ess_amd import hip
    EINVAL = -22
    L = hip.lib()
    rows = _full_rows(1, [3], 600)
    t, x, y, p = C._device_columns(rows, RING)
    words = [_words([v]) for v in (0, 29, 10, 3)]
    out = torch.zeros(1, NB, H, W, device=DEV)
    acc = torch.zeros(NB * H * W, dtype=torch.int64, device=DEV)
    P = ctypes.c_void_p

    def call(ring=RING, acc_bytes=None, out_ptr=None, p_ptr=None, null=None):
        w = [P(0 if null == k else v.data_ptr()) for k, v in enumerate(words)]
        return L.ess_event_ingest_ring(P(t.data_ptr()), P(x.data_ptr()), P(y.data_ptr()), P(p.data_ptr() if p_ptr is None else p_ptr), *w,
                                       ring, 1, 1, NB, H, W, P(acc.data_ptr()), acc.numel() * 8 if acc_bytes is None else acc_bytes,
                                       P(out.data_ptr() if out_ptr is None else out_ptr), hip.stream())
    assert call(ring=(1 << 22) + 16) == EINVAL and b'ring=' in L.ess_last_error()
    assert call(ring=0) == EINVAL and b'ring=' in L.ess_last_error()
    assert call(ring=24) == EINVAL and b'multiple of 16' in L.ess_last_error()
    assert call(acc_bytes=NB * H * W * 8 - 8) == EINVAL and b'acc has' in L.ess_last_error()
    assert call(out_ptr=out.data_ptr() + 4) == EINVAL and b'16-byte aligned' in L.ess_last_error()
    assert call(p_ptr=p.data_ptr() + 1) == EINVAL and b'16-byte aligned' in L.ess_last_error()
    for k in range(4):
        assert call(null=k) == EINVAL and b'null' in L.ess_last_error()
    ok = dict(t=t, x=x, y=y, p=p, rows=words[0], starts=words[1], counts=words[2], formats=words[3], out=out, acc=acc)

    def refused(match, **kw):
        with pytest.raises(hip.EssHipError, match=match):
            hip.event_ingest_ring(**{**ok, **kw})
    refused('acc has', acc=acc[:-1])
    refused('t must be', t=t.to(torch.int32))
    refused('y must be', y=y[:, :16].contiguous())
    refused('rows must be int32', rows=_words([0, 0]))
    refused('starts must be int32', starts=words[1].to(torch.int64))
    refused('no CPU path', t=t.cpu())
    refused('no CPU path', counts=words[2].cpu())
    refused('contiguous', x=torch.zeros(1, 2 * RING, dtype=torch.int16, device=DEV)[:, ::2])
    refused('multiple of 16', **{k: ok[k][:, :24].contiguous() for k in 'txyp'})
    assert not bool(out.any()) and not bool(acc.any())
    assert call() == 0  # (the same call with nothing wrong)
    assert torch.equal(_bits(out[0]), _bits(C._expected(_unrolled(rows[0], 29, 10)))) and bool(out.any())


# ---------------------------------------------------------------------------------------------- 2. the segmenter
SH_, SW_ = SC.H, SC.W
CAP, RCAP, WIN = 512, 1024, 512
PACKETS = (100, 333, 1, 700, 57, 512, 211)
SEG_CASES = [(S, mode, graph, stride) for S in (1, 3) for mode in ('mixed', 'bf16') for graph in (False, True) for stride in (512, 128)]
SEG_IDS = [f'S{S}-{mode}-{"graph" if graph else "eager"}-stride{stride}' for S, mode, graph, stride in SEG_CASES]


@functools.lru_cache(maxsize=None)
def _source(s, fmt, n=2400, gap_at=None):
    """one stream's whole event sequence as EventColumns (format fmt), built once; gap_at: a pause of 50 ms behind that event"""
    ev = M._events(n, SH_, SW_, 900 + 10 * s + fmt)
    if gap_at is not None:
        ev[gap_at:, 0] += 0.05
    return C._as_columns(ev, fmt)


def _slice(c, a, b):
    from ess_amd.datasets.data_util import EventColumns
    return EventColumns(*(np.ascontiguousarray(v[a:b]) for v in (c.t, c.x, c.y, c.p)))


class _Stream:
    """the test's own view of one stream: its source, how much of it is fed, and the windows it expects -- cut from the WHOLE
    source by the definition, not by the code under test"""

    def __init__(self, s, fmt, cut, **kw):
        self.s, self.fed, self.k, self.n_packets = s, 0, 0, 0
        self.src = _source(s, fmt, **kw)
        self.windows = cut(self.src)

    def packet(self, seg, size):
        """the next packet: `size` events, clipped to what is left of the source and to the room the ring has"""
        f = seg._feeds[self.s].windows
        n = min(size, self.src.n - self.fed, RCAP - (f.head - min(f.oldest_needed(), f.head)))
        c = _slice(self.src, self.fed, self.fed + n)
        self.fed += n
        self.n_packets += 1
        return c

    def next_window(self):
        a, b = self.windows[self.k]
        self.k += 1
        return _slice(self.src, a, b) if b > a else None


def _cut_by_count(stride):
    return lambda src: [(k * stride, k * stride + WIN) for k in range((src.n - WIN) // stride + 1)]


def _cut_by_duration(D, E):
    def cut(src):
        t, out, k = src.t, [], 0
        while bool((t >= t[0] + k * E + D).any()):
            lo = t[0] + k * E
            out.append((int(np.searchsorted(t, lo, 'left')), int(np.searchsorted(t, lo + D, 'left'))))
            k += 1
        return out
    return cut


def _round(seg, ref, streams, what, active=None):
    """one update_from_feed against update_from_events of the 'columns' segmenter on the windows the test expects -> active flags"""
    allowed = [True] * len(streams) if active is None else active
    wins = [st.next_window() if seg.pending(st.s) and a else None for st, a in zip(streams, allowed)]
    on = [w is not None for w in wins]
    got = seg.update_from_feed(active)
    want = ref.update_from_events(wins)
    C._assert_rows(got, want, on, what)
    return on


def _run_feed(S, mode, graph, cut, ring_kw, what, gap=False):
    from ess_amd import hip
    hip.set_compute(mode)
    try:
        seg = SC._segmenter('convlstm', S, graph=graph, event_capacity=CAP, event_layout='ring', ring_capacity=RCAP, **ring_kw)
        ref = SC._segmenter('convlstm', S, graph=graph, event_capacity=CAP, event_layout='columns')
        assert seg.event_layout == 'ring' and seg.ring_capacity == RCAP and seg._records is None and seg._columns is None
        assert [(c.dtype, tuple(c.shape)) for c in seg._ring] == [(torch.int64, (S, RCAP)), (torch.int16, (S, RCAP)),
                                                                  (torch.int16, (S, RCAP)), (torch.uint8, (S, RCAP))]
        assert all(h.is_pinned() and h.shape == d.shape and h.dtype == d.dtype for h, d in zip(seg._ring_host, seg._ring))
        assert tuple(seg._words.shape) == (4, S) and seg._words.dtype == torch.int32 and len(seg._stage) == 2
        assert all(st.words.is_pinned() and tuple(st.words.shape) == (4, S) for st in seg._stage)
        assert seg._acc.dtype == torch.int64 and tuple(seg._acc.shape) == (S, SC.C, SH_, SW_)
        with pytest.raises(hip.EssHipError, match='feed'):
            seg.update_from_events([None] * S)
        fmt0 = 1 if gap else 0  # (a duration cut on int64 microseconds: every stream delivers them)
        streams = [_Stream(s, fmt0 | (2 * (s % 2)), cut, **({'gap_at': 1300} if gap and s == 1 else {})) for s in range(S)]
        actives, tick, rounds = [], 0, 0
        while any(st.fed < st.src.n for st in streams):
            for st in streams:
                size = 700 if tick == 0 else PACKETS[(tick + 2 * st.s) % len(PACKETS)]  # (the first round has every stream)
                c = st.packet(seg, size)
                n_before = seg.pending(st.s)
                assert seg.feed(st.s, c) == seg.pending(st.s) >= n_before
            if tick == 2:
                seg.reset([0])
                ref.reset([0])
            if tick == 3 and S > 1:
                # stream S - 1 starts afresh, in another format: index 0 is its next event, whatever lay pending is forgotten
                seg.drop_feed([S - 1])
                assert seg.pending(S - 1) == 0 and seg._feeds[S - 1].format is None
                streams[S - 1] = _Stream(S - 1, fmt0 | (2 * (S % 2)), cut)
            while any(seg.pending(s) for s in range(S)):
                actives.append(tuple(_round(seg, ref, streams, f'{what} tick {tick} round {rounds}')))
                rounds += 1
            tick += 1
        # every expected complete window was served, and nothing else
        assert all(st.k == len(st.windows) >= 3 for st in streams) and tick > 3
        assert seg._feeds[0].windows.head == streams[0].src.n >= 2 * RCAP  # the ring wrapped at least twice
        if S > 1:
            assert any(0 < sum(a) < S for a in actives) and any(sum(a) == S for a in actives)
        # update(grids) through the same capture: count words INGEST_KEEP
        grids = torch.from_numpy(np.stack([C._want(_slice(st.src, 0, 400), SC.C, SH_, SW_) for st in streams])).to(DEV)
        C._assert_rows(seg.update(grids), ref.update(grids), [True] * S, f'{what} update(grids)')
        torch.cuda.synchronize()
        assert not bool(seg._acc.any())
        assert seg.n_captures == ref.n_captures == (1 if graph else 0) and seg.n_windows == ref.n_windows == rounds + 1
        return actives
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('S,mode,graph,stride', SEG_CASES, ids=SEG_IDS)
def test_rounds_from_the_feed_equal_rounds_from_columns(S, mode, graph, stride):
    """2400 events per stream through a ring of 1024 in packets of 100, 333, 1, 700 ... (clipped to the ring's room), windows of 512
    events every `stride`: each round's active rows equal the 'columns' segmenter's on the same windows; on the way one reset([0])
    and one drop_feed([S - 1]) after which that stream delivers other dtypes; ONE capture serves every round"""
    _run_feed(S, mode, graph, _cut_by_count(stride), dict(window_events=WIN, window_stride=stride), f'{mode} S={S} graph={graph} stride={stride}')


def test_rounds_from_the_feed_cut_by_duration():
    """int64 microsecond times, windows of 30 ms every 10 ms (about 360 events each, each event read by three windows); stream 1
    pauses for 50 ms: its windows inside the pause are empty, consumed, and count as idle"""
    D, E = 30_000, 10_000
    src = _source(1, 3, gap_at=1300)
    cuts = _cut_by_duration(D, E)(src)
    assert any(a == b for a, b in cuts) and max(b - a for a, b in cuts) <= CAP
    actives = _run_feed(3, 'bf16', True, _cut_by_duration(D, E), dict(window_duration=D, window_stride=E), 'duration', gap=True)
    assert any(not a[1] and (a[0] or a[2]) for a in actives)


@pytest.mark.parametrize('mode,graph', [(m, g) for m in ('mixed', 'bf16') for g in (False, True)],
                         ids=[f'{m}-{"graph" if g else "eager"}' for m in ('mixed', 'bf16') for g in (False, True)])
def test_compacted_feed_rounds_equal_the_uncompacted(mode, graph):
    """S = 3, compact=True with buckets [1, 2], both batch-size-dependent dispatch choices pinned: the rows equal the uncompacted
    ring segmenter's bit for bit.  The rounds have 3, 1, 2 (one of them restarting), 0, 1 and -- through the active mask -- 2 and 1
    active streams; a compacted round names its streams in the row words, no event moves"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    S = 3
    hip.set_compute(mode)
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        kw = dict(graph=graph, event_capacity=CAP, event_layout='ring', ring_capacity=RCAP, window_events=WIN)
        ride = SC._segmenter('convlstm', S, **kw)
        comp = SC._segmenter('convlstm', S, compact=True, compact_buckets=[1, 2], **kw)
        assert comp.buckets == (1, 2)
        src = [_source(s, s % 4) for s in range(S)]
        fed = [0] * S
        #           packets per stream      active mask        the streams expected to run
        ticks = [((512, 512, 512), None, (0, 1, 2)), ((512, 100, 0), None, (0,)), ((100, 412, 512), None, (1, 2)),
                 ((300, 50, 20), None, ()), ((0, 462, 0), None, (1,)), ((112, 512, 492), [True, False, True], (0, 2)),
                 ((0, 0, 0), None, (1,))]
        for w, (sizes, mask, expect) in enumerate(ticks):
            for s, n in enumerate(sizes):
                c = _slice(src[s], fed[s], fed[s] + n)
                fed[s] += n
                assert comp.feed(s, c) == ride.feed(s, c)
            if w == 2:
                comp.reset([2])
                ride.reset([2])
            got, want = comp.update_from_feed(mask), ride.update_from_feed(mask)
            on = [s in expect for s in range(S)]
            C._assert_rows(got, want, on, f'{mode} graph={graph} round {w}')
            b = next((b for b in comp.buckets if b >= len(expect)), None)
            if b is not None:
                torch.cuda.synchronize()
                words = comp._words.cpu()
                assert words[0, :len(expect)].tolist() == list(expect), (w, 'the row words name the active streams in slot order')
                assert words[2, :len(expect)].tolist() == [WIN] * len(expect) and words[2, len(expect):b].tolist() == [0] * (b - len(expect))
                for slot in range(len(expect), b):
                    assert not bool(_bits(comp.compact_input[slot]).any()), (w, slot, 'a padded slot is not all zero')
        assert [comp.pending(s) for s in range(S)] == [0, 0, 0]
        assert comp.n_captures <= (len(comp.buckets) + 1 if graph else 0) and ride.n_captures == (1 if graph else 0)
        assert not bool(comp._acc.any()) and not bool(ride._acc.any())
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')


def test_feed_refuses_an_overrun_before_anything_is_written():
    """windows pending and the ring full: the next packet is refused -- device ring, pinned mirror, words, staging sets, pending
    windows, cutter and round counter are as they were -- and so are a packet in other dtypes, one that goes back in time and a plain
    array; the next valid round gives the right rows"""
    from ess_amd import hip
    S = 3
    hip.set_compute('bf16')
    try:
        seg = SC._segmenter('convlstm', S, graph=True, event_capacity=CAP, event_layout='ring', ring_capacity=RCAP, window_events=WIN,
                            window_stride=128)
        ref = SC._segmenter('convlstm', S, graph=True, event_capacity=CAP, event_layout='columns')
        streams = [_Stream(s, s % 4, _cut_by_count(128)) for s in range(S)]
        for st in streams:
            seg.feed(st.s, st.packet(seg, 600))
        _round(seg, ref, streams, 'round 0')
        for st in streams:
            seg.feed(st.s, st.packet(seg, 424))  # 1024 fed, windows from event 128 on pending: the ring is full
        assert [seg.pending(s) for s in range(S)] == [4, 4, 4]

        def snapshot():
            torch.cuda.synchronize()
            f = seg._feeds[1]
            return ([t.clone() for t in seg._ring + seg._ring_host + (seg._words,)] + [st.words.clone() for st in seg._stage],
                    seg._stage_next, seg.n_windows, list(seg._pending), [seg.pending(s) for s in range(S)],
                    (f.windows.head, f.windows.last_t, f.windows.oldest_needed(), f.format, f.dtypes, len(f.uploads)))
        before = snapshot()
        more = _slice(streams[1].src, 1024, 1024 + 129)
        with pytest.raises(hip.EssHipError, match='overrun'):
            seg.feed(1, more)
        with pytest.raises(hip.EssHipError, match='one format'):
            seg.feed(1, _slice(_source(1, 2), 1024, 1034))
        with pytest.raises(hip.EssHipError, match='non-decreasing'):
            seg.feed(1, _slice(streams[1].src, 1000, 1010))
        with pytest.raises(hip.EssHipError, match='EventColumns'):
            seg.feed(1, np.zeros((5, 4)))
        with pytest.raises(hip.EssHipError, match='stream'):
            seg.feed(S, more)
        after = snapshot()
        assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])) and before[1:] == after[1:]
        assert seg.feed(1, _slice(streams[1].src, 1024, 1024 + 128)) == 5  # (up to the oldest needed event: it fits)
        streams[1].fed += 128
        while any(seg.pending(s) for s in range(S)):
            _round(seg, ref, streams, 'the rounds after the refusals')
        assert seg.n_captures == 1 and seg.n_windows == 6
        with pytest.raises(hip.EssHipError, match='ring_capacity'):
            SC._segmenter('convlstm', S, event_capacity=CAP, event_layout='ring', ring_capacity=CAP - 16, window_events=WIN)
        with pytest.raises(hip.EssHipError, match='window_events'):
            SC._segmenter('convlstm', S, event_capacity=CAP, event_layout='ring')
        with pytest.raises(hip.EssHipError, match="event_layout='ring'"):
            SC._segmenter('convlstm', S, event_capacity=CAP, event_layout='columns', window_events=WIN)
        with pytest.raises(hip.EssHipError, match="event_layout='ring'"):
            ref.feed(0, more)
    finally:
        hip.set_compute('fp32')
