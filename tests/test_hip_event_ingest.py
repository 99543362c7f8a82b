"""GPU tier: the event ingest -- hip.event_ingest (packed 16-byte records -> voxel grids, summed in 64-bit fixed point) and
MultiStreamSegmenter(event_capacity=), whose captured round starts with it.  What is asserted throughout is BITS: the grids equal
the numpy restatement of tests/test_host_event_ingest.py (integer sums have no order), they do not depend on the order of the
records, on the batch a stream rides in or on the run, and from events a segmenter's labels, colours and confidences are those it
gives for the same grids."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers, events, result rows, the pins)
from tests import test_hip_stream_compaction as SC  # noqa: E402  (the 64 x 96 models)
from tests import test_host_event_ingest as R  # noqa: E402  (the restatement)

DEV = M.DEV
GUARD, NAN16 = M.GUARD, M.NAN16
NB, H, W, CAP = 5, 24, 40, 4096


def _bits(t):
    return t.contiguous().view(torch.int32)


def _device_records(recs, capacity):
    """recs: per stream a packed record array (<= capacity rows) -> uint8 [S, capacity, 16] on the device.  The rows behind a
    stream's own are filled with an event that WOULD land in the grid: a kernel that walked past the count would show."""
    from ess_amd import hip
    host = np.zeros((len(recs), capacity), dtype=hip.EVENT_RECORD)
    host['t'], host['x'], host['y'], host['p'] = 0.05, 1, 1, 1
    for s, r in enumerate(recs):
        host[s, :len(r)] = r
    return torch.from_numpy(host.view(np.uint8).reshape(len(recs), capacity, 16)).to(DEV)


def _counts(c):
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _expected(rec, nb=NB, h=H, w=W):
    return torch.from_numpy(R.restate(rec, nb, h, w)).to(DEV)


def _run_guarded(recs, counts, capacity, nb=NB, h=H, w=W, prefill=None):
    """-> (out inside its NaN-pre-filled guarded buffer, the buffer, acc)"""
    from ess_amd import hip
    S = len(recs)
    buf, out = M._guarded((S, nb, h, w), torch.float32)
    acc = torch.zeros(S * nb * h * w, dtype=torch.int64, device=DEV)
    got = hip.event_ingest(_device_records(recs, capacity), _counts(counts), out, acc=acc)
    assert got is out
    return out, buf, acc


def _guards_intact(buf, out):
    n = out.numel() * 2
    return bool((buf[:GUARD // 2] == NAN16).all()) and bool((buf[GUARD // 2 + n:] == NAN16).all())


# ---------------------------------------------------------------------------------------------- 1. the kernels
def test_event_ingest_bit_equal_to_the_restatement():
    """S = 4 with counts [3000, 1, 0, 4096] at capacity 4096: bit-equal per stream, the empty stream all zero, the guard bytes
    intact, acc all zero behind the call, a second call on the same buffers the same bits"""
    from ess_amd import hip
    counts = [3000, 1, 0, CAP]
    recs = [R.packed(R.events(n, H, W, 20 + s)) for s, n in enumerate(counts)]
    out, buf, acc = _run_guarded(recs, counts, CAP)
    for s in range(4):
        assert torch.equal(_bits(out[s]), _bits(_expected(recs[s]))), f'stream {s} ({counts[s]} events)'
    assert bool(out[0].any()) and bool(out[1].any()) and not bool(_bits(out[2]).any())
    assert _guards_intact(buf, out)
    assert not bool(acc.any())
    first = out.clone()
    buf.fill_(NAN16)
    hip.event_ingest(_device_records(recs, CAP), _counts(counts), out, acc=acc)
    assert torch.equal(_bits(out), _bits(first)) and not bool(acc.any()) and _guards_intact(buf, out)
    # acc=None: allocated and zeroed by the call
    assert torch.equal(_bits(hip.event_ingest(_device_records(recs, CAP), _counts(counts), torch.empty_like(first))), _bits(first))


def _edge_rows():
    g = np.random.default_rng(9)
    n = 64
    base = R.events(n, H, W, 31)
    same_t = base.copy()
    same_t[:, 0] = 0.125
    coords = R.events(16, H, W, 32)
    coords[:, 1] = [-1, 0, W - 1, W, W + 1, 32767, 40000, -5, -0.5, 3, 3, 3, 3, 3, 3, 3]
    coords[:, 2] = [2, 2, 2, 2, 2, 2, 2, 2, 2, -1, 0, H - 1, H, 32767, 1e9, -1e9]
    nan_t = base.copy()
    nan_t[n // 2, 0] = float('nan')
    nan_first = base.copy()
    nan_first[0, 0] = float('nan')
    at_last = base.copy()
    at_last[-5:, 0] = at_last[-1, 0]
    unsorted = base.copy()
    unsorted[1:-1] = unsorted[1:-1][g.permutation(n - 2)]
    unsorted[3, 0] = -1.0  # (before the first timestamp: ts < 0, dropped)
    unsorted[4, 0] = 9.0   # (behind the last: ts >= nb, dropped)
    return {'same_timestamp': (same_t, 128), 'one_event': (base[:1], 1), 'one_event_wide': (base[:1], 2048),
            'one_pixel_mixed_polarity': (R.one_pixel_events(2000, 33), 2048), 'coordinates': (coords, 16), 'nan_timestamp': (nan_t, 64),
            'nan_first_timestamp': (nan_first, 64), 'at_last_timestamp': (at_last, 100), 'outside_the_time_range': (unsorted, 64)}


@pytest.mark.parametrize('name', sorted(_edge_rows()))
def test_event_ingest_edge_rows(name):
    ev, capacity = _edge_rows()[name]
    rec = R.packed(ev)
    want = R.restate(rec, NB, H, W)
    if name == 'same_timestamp':  # dT = 0 -> 1: every event whole in bin 0
        assert want[0].any() and not want[1:].any()
    if name == 'coordinates':  # only the in-range pixels land: x in {0, W-1, 0 (from -0.5)} on row 2, y in {0, H-1} on column 3
        assert 0 < np.count_nonzero(np.abs(want).sum(0)) <= 4
    if name == 'nan_first_timestamp':
        assert not want.any()
    if name == 'at_last_timestamp':
        assert want[NB - 1].any()
    if name == 'one_pixel_mixed_polarity':
        assert np.count_nonzero(want.sum(0)) == 1
    out, buf, acc = _run_guarded([rec], [len(rec)], capacity)
    assert torch.equal(_bits(out[0]), _bits(torch.from_numpy(want).to(DEV))), name
    assert _guards_intact(buf, out) and not bool(acc.any())


def test_event_ingest_on_a_grid_that_is_no_multiple_of_four():
    """3 x 5 x 7 voxels per stream: the streams' rows are not 16-byte aligned, the finish pass takes its scalar form"""
    nb, h, w = 3, 5, 7
    counts = [500, 0, 37]
    recs = [R.packed(R.events(n, h, w, 40 + s)) for s, n in enumerate(counts)]
    out, buf, acc = _run_guarded(recs, counts, 512, nb, h, w)
    for s in range(3):
        assert torch.equal(_bits(out[s]), _bits(_expected(recs[s], nb, h, w))), s
    assert _guards_intact(buf, out) and not bool(acc.any())


def test_event_ingest_does_not_depend_on_the_record_order():
    """the interior records permuted (the first and the last, which set the time scale, in place): bit-identical grids -- what the
    fp32-atomic kernel cannot promise"""
    rec = R.packed(R.one_pixel_events(2000, 51))
    rec[700:1400] = R.packed(R.events(700, H, W, 52))  # (one crowded pixel, where the order of a float sum would matter, and a spread)
    rec['t'][700:1400] = np.linspace(rec['t'][0], rec['t'][-1], 700)
    g = np.random.default_rng(53)
    out0, _, _ = _run_guarded([rec], [len(rec)], 2048)
    for _ in range(3):
        perm = rec.copy()
        perm[1:-1] = perm[1:-1][g.permutation(len(rec) - 2)]
        out1, _, _ = _run_guarded([perm], [len(rec)], 2048)
        assert torch.equal(_bits(out0), _bits(out1))
    assert torch.equal(_bits(out0[0]), _bits(_expected(rec)))


def test_ingest_keep_leaves_the_grid_alone():
    from ess_amd import hip
    counts = [3000, hip.INGEST_KEEP, 0, 2000, -7]
    recs = [R.packed(R.events(3000, H, W, 60 + s)) for s in range(5)]
    out, buf, acc = _run_guarded(recs, counts, CAP)
    assert _guards_intact(buf, out)
    for s in (1, 4):  # (the NaN pre-fill, every bit of it)
        assert bool((out[s].view(torch.int16) == NAN16).all()), s
    assert torch.equal(_bits(out[0]), _bits(_expected(recs[0]))) and not bool(_bits(out[2]).any())
    assert torch.equal(_bits(out[3]), _bits(_expected(recs[3][:2000])))
    assert not bool(acc.any())


def test_a_stream_batched_equals_the_stream_alone():
    counts = [3000, 1, 0, CAP]
    recs = [R.packed(R.events(n, H, W, 70 + s)) for s, n in enumerate(counts)]
    out, _, _ = _run_guarded(recs, counts, CAP)
    for s in range(4):
        alone, _, _ = _run_guarded([recs[s]], [counts[s]], CAP)
        assert torch.equal(_bits(out[s]), _bits(alone[0])), s


def test_event_ingest_argument_errors():
    """ESS_EINVAL with a message, in front of any launch"""
    import ctypes
    from ess_amd import hip
    EINVAL = -22
    L = hip.lib()
    rec = _device_records([R.packed(R.events(10, H, W, 1))], 16)
    cnt = _counts([10])
    out = torch.zeros(1, NB, H, W, device=DEV)
    acc = torch.zeros(NB * H * W, dtype=torch.int64, device=DEV)
    P = ctypes.c_void_p

    def call(records=rec, capacity=16, acc_t=acc, acc_bytes=None, out_ptr=None):
        return L.ess_event_ingest(P(records.data_ptr()), P(cnt.data_ptr()), capacity, 1, NB, H, W, P(acc_t.data_ptr()),
                                  acc_t.numel() * 8 if acc_bytes is None else acc_bytes, P(out.data_ptr() if out_ptr is None else out_ptr),
                                  hip.stream())
    assert call(capacity=(1 << 22) + 1) == EINVAL and b'capacity' in L.ess_last_error()
    assert call(capacity=0) == EINVAL and b'capacity' in L.ess_last_error()
    assert call(acc_bytes=NB * H * W * 8 - 8) == EINVAL and b'acc has' in L.ess_last_error()
    assert call(out_ptr=out.data_ptr() + 4) == EINVAL and b'16-byte aligned' in L.ess_last_error()
    assert call(out_ptr=0) == EINVAL and b'null' in L.ess_last_error()
    # ... and through the binding
    with pytest.raises(hip.EssHipError, match='acc has'):
        hip.event_ingest(rec, cnt, out, acc=acc[:-1])
    shifted = torch.zeros(NB * H * W + 4, device=DEV)[1:1 + NB * H * W].view(1, NB, H, W)
    with pytest.raises(hip.EssHipError, match='16-byte aligned'):
        hip.event_ingest(rec, cnt, shifted, acc=acc)
    with pytest.raises(hip.EssHipError, match='records must be uint8'):
        hip.event_ingest(rec.view(torch.int8), cnt, out, acc=acc)
    with pytest.raises(hip.EssHipError, match='counts must be int32'):
        hip.event_ingest(rec, _counts([1, 2]), out, acc=acc)
    with pytest.raises(hip.EssHipError, match='no CPU path'):
        hip.event_ingest(rec.cpu(), cnt, out, acc=acc)
    assert not bool(out.any()) and not bool(acc.any())
    assert call() == 0  # (the same call with nothing wrong)
    assert torch.equal(_bits(out[0]), _bits(_expected(R.packed(R.events(10, H, W, 1)))))


# ---------------------------------------------------------------------------------------------- 2. the segmenter
SH_, SW_, SC_CAP = SC.H, SC.W, 4096
SEG_CASES = [(S, mode, graph) for S in (3, 5) for mode in ('bf16', 'mixed') for graph in (False, True)]
SEG_IDS = [f'S{S}-{mode}-{"graph" if graph else "eager"}' for S, mode, graph in SEG_CASES]


@functools.lru_cache(maxsize=None)
def _window(S, w):
    """the events of round w, one [N, 4] array per stream (sizes differ per stream), built once"""
    return tuple(M._events(1500 + 500 * ((s + w) % 4), SH_, SW_, 500 + 10 * w + s) for s in range(S))


def _with_idle(evs, idle):
    return [None if s in idle else e for s, e in enumerate(evs)]


def _standalone_grids(evs):
    """the grids of one round from a standalone hip.event_ingest on the same records (an idle stream: count 0, a zero grid)"""
    from ess_amd import hip
    recs = [R.packed(e) if e is not None else np.zeros(0, dtype=hip.EVENT_RECORD) for e in evs]
    out = torch.empty(len(evs), SC.C, SH_, SW_, device=DEV)
    return hip.event_ingest(_device_records(recs, SC_CAP), _counts([len(r) for r in recs]), out)


def _assert_rows(a, b, active, what):
    assert a.valid == b.valid == tuple(active), what
    for s, on in enumerate(active):
        if on:
            assert M._same(M._row(a, s), M._row(b, s)), f'{what}: stream {s}'


@pytest.mark.parametrize('S,mode,graph', SEG_CASES, ids=SEG_IDS)
def test_rounds_from_events_equal_rounds_from_the_ingested_grids(S, mode, graph):
    """update_from_events(event_capacity=) == update(grids), grids from a standalone hip.event_ingest on the same records: labels,
    colours, confidence bits.  ONE graph serves rounds that alternate update_from_events, update(grids), an idle stream and a reset;
    a window above the capacity raises before anything is written, and the next round is right.  A segmenter built without
    event_capacity has none of the buffers."""
    from ess_amd import hip
    hip.set_compute(mode)
    try:
        seg = SC._segmenter('convlstm', S, graph=graph, event_capacity=SC_CAP)
        ref = SC._segmenter('convlstm', S, graph=graph)
        assert ref.event_capacity is None and ref._records is None and ref._counts is None and ref._acc is None and not hasattr(ref, '_stage')
        assert tuple(seg._records.shape) == (S, SC_CAP, 16) and tuple(seg._counts.shape) == (S,) and len(seg._stage) == 2
        assert seg._acc.dtype == torch.int64 and tuple(seg._acc.shape) == (S, SC.C, SH_, SW_)
        assert all(st.records.is_pinned() and st.counts.is_pinned() for st in seg._stage)

        def both(w, idle=(), from_events=True):
            evs = _with_idle(_window(S, w), idle)
            grids, active = _standalone_grids(evs), [e is not None for e in evs]
            got = seg.update_from_events(evs) if from_events else seg.update(grids, active)
            _assert_rows(got, ref.update(grids, active), active, f'{mode} S={S} graph={graph} round {w}')
        both(0)
        both(1, idle=(1,))
        both(2, from_events=False)           # grids through the same graph: count words INGEST_KEEP
        both(3, idle=(0, S - 1))
        seg.reset([1])
        ref.reset([1])
        both(4)
        both(5, idle=tuple(range(S)))        # nobody has a window
        # a window above the capacity: refused, nothing written -- the state, the pending restarts and the buffers are as before
        seg.reset([2])
        ref.reset([2])
        big = list(_window(S, 6))
        big[S - 1] = M._events(SC_CAP + 1, SH_, SW_, 99)
        n_windows = seg.n_windows
        with pytest.raises(hip.EssHipError, match=f'{SC_CAP + 1} events.*event_capacity={SC_CAP}'):
            seg.update_from_events(big)
        assert seg.n_windows == n_windows
        bad = list(_window(S, 6))
        bad[0] = bad[0].copy()
        bad[0][5, 3] = 0.5
        with pytest.raises(hip.EssHipError, match='polarity'):
            seg.update_from_events(bad)
        both(6)
        both(7, idle=(2,))
        assert not bool(seg._acc.any())
        assert seg.n_captures == ref.n_captures == (1 if graph else 0) and seg.n_windows == ref.n_windows == 8
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('S,mode,graph', SEG_CASES, ids=SEG_IDS)
def test_two_fresh_segmenters_agree_from_events(S, mode, graph):
    """the same three rounds from events into two fresh segmenters: bit for bit the same results -- from events, with the
    fp32-atomic voxeliser, nothing was reproducible"""
    from ess_amd import hip
    hip.set_compute(mode)
    try:
        runs = []
        for _ in range(2):
            seg = SC._segmenter('convlstm', S, graph=graph, event_capacity=SC_CAP)
            runs.append([seg.update_from_events(_with_idle(_window(S, w), (w,) if w == 1 else ())) for w in range(3)])
        for w in range(3):
            _assert_rows(runs[0][w], runs[1][w], [not (w == 1 and s == 1) for s in range(S)], f'{mode} S={S} graph={graph} round {w}')
    finally:
        hip.set_compute('fp32')


@pytest.mark.parametrize('S,mode,graph', SEG_CASES, ids=SEG_IDS)
def test_compacted_ingest_equals_the_uncompacted_ingest(S, mode, graph):
    """compact=True with event_capacity: the labels equal the uncompacted ingest segmenter's bit for bit (the batch size changes
    from round to round: both batch-size-dependent dispatch choices pinned, as in tests/test_hip_stream_compaction.py); a padded
    slot's compact input is all zero; one capture per bucket and one for the ride-along round at the most"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    hip.set_compute(mode)
    prev, prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
    try:
        ride = SC._segmenter('convlstm', S, graph=graph, event_capacity=SC_CAP)
        comp = SC._segmenter('convlstm', S, graph=graph, event_capacity=SC_CAP, compact=True)
        # active counts: S (the ride-along round), 1, 2, then S = 3: 3 / S = 5: 3 (bucket 4, one padded slot) with a restart, S - 1
        # as an update(grids) round, 0 (the smallest bucket, every slot padded)
        idles = [(), tuple(range(1, S)), (0,) if S == 3 else (0, 2, 4), () if S == 3 else (1, 3), (S - 1,), tuple(range(S))]
        for w, idle in enumerate(idles):
            evs = _with_idle(_window(S, w), idle)
            active = [e is not None for e in evs]
            if w == 3:
                comp.reset([0])
                ride.reset([0])
            if w == 4:  # grids through the compacted graph of the same bucket: count words INGEST_KEEP
                grids = _standalone_grids(evs)
                got, want = comp.update(grids, active), ride.update(grids, active)
            else:
                got, want = comp.update_from_events(evs), ride.update_from_events(evs)
            _assert_rows(got, want, active, f'{mode} S={S} graph={graph} round {w}')
            A = sum(active)
            b = next((b for b in comp.buckets if b >= A), None)
            if w != 4 and b is not None:
                if A:  # (the compact input: the active streams' grids in slot order)
                    own = _standalone_grids([evs[s] for s in range(S) if active[s]])
                    assert torch.equal(_bits(comp.compact_input[:A]), _bits(own)), (w, 'compact input')
                for slot in range(A, b):
                    assert not bool(_bits(comp.compact_input[slot]).any()), (w, slot, 'a padded slot is not all zero')
        if S == 5:
            assert comp.buckets == (1, 2, 4)  # (round 2: 2 of 5 in bucket 2; round 3: 3 of 5 in bucket 4, one padded slot)
        assert comp.n_captures <= (len(comp.buckets) + 1 if graph else 0) and ride.n_captures == (1 if graph else 0)
        assert not bool(comp._acc.any())
    finally:
        set_s2d_mode(prev)
        hip.tuning_set('norm_split_wgs', prev_split)
        hip.set_compute('fp32')
