"""GPU tier of SequenceSegmenter(store=...): sequence rounds cut on the device out of an EventStore against the ring-fed
SequenceSegmenter on the same events and ends -- labels, colours and confidences bit for bit per lane and round, the confusion rows
as integers.  The cases, recordings, ends and ground truths are tests/test_hip_sequence_segmenter.py's (T = 5, N_w = 256, three
recordings of 4096 events in three formats, under the two pinned batch-size switches); the duration rule and the loader grid use
tests/test_hip_sequence_loader.py's 'dsec' preset."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_sequence_loader as LD  # noqa: E402  (the 'dsec' preset, times in microseconds)
from tests import test_hip_sequence_segmenter as SQ  # noqa: E402  (models, rigs, sources, pins, ground truths -- imported, not edited)

DEV = SQ.DEV
T, NW, S, H, W, K = SQ.T, SQ.NW, SQ.S, SQ.H, SQ.W, SQ.K
M = SQ.M


@functools.lru_cache(maxsize=None)
def _store():
    """SQ's three recordings, the last one uploaded FIRST (a lane is no sensor, a recording number no stream number): stream s is
    recording REC[s].  Recording REC[0] carries stream 0's four ground truths as the store's labels 0 .. 3."""
    from ess_amd.datasets.event_store import EventStore
    store = EventStore(3 * SQ.N_SRC, label_hw=(H, W), label_capacity=8)
    store.add_recording(SQ._source(2))
    store.add_recording(SQ._source(0), labels=np.stack([SQ._gt(r, 0) for r in range(4)]))
    store.add_recording(SQ._source(1))
    assert store.label_range(1) == (0, 4)
    return store


REC = (1, 2, 0)


def _sample(r, s, by_time=False, label=None):
    from ess_amd.datasets.event_store import StoreSample
    if SQ.ENDS[r][s] is None:
        return None
    if by_time:
        return StoreSample(REC[s], t_end=SQ._t_end(r, s), map=s, label=label)
    return StoreSample(REC[s], end=SQ.ENDS[r][s], map=s, label=label)


def _same_rows(got, s, want, k, what):
    assert M._same(M._row(got, s), M._row(want, k)), what


@pytest.mark.parametrize('rtype,mode,graph', SQ.CASES, ids=SQ.IDS)
def test_store_rounds_equal_the_ring_fed_rounds(rtype, mode, graph):
    """SQ's four rounds (three by index -- fewer than T N_w events, an idle lane that is handed a label, a label missing --, one by
    time), lane 0's ground truth from StoreSample.label and the others' from labels=; then lanes permuted against recordings, two
    lanes on one recording with different ends, and a sample in front of its recording's first event (EMPTY)"""
    from ess_amd import hip
    from ess_amd.datasets.event_store import StoreSample
    SQ._check_the_rounds_cover_what_they_are_meant_to()
    store = _store()
    with SQ._Pinned(mode):
        twin = SQ._segmenter(rtype, S, graph, SQ.TR._rig())
        seg = SQ._segmenter(rtype, S, graph, SQ.TR._rig(), store=store, ring_capacity=None)
        assert seg._ring is None and seg._ring_host is None and seg._feeds is None and seg.ring_capacity is None
        for call in (lambda: seg.feed(0, SQ._source(0)), lambda: seg.fed(0), lambda: seg.drop_feed()):
            with pytest.raises(hip.EssHipError, match='EventStore'):
                call()
        fed, kept = [0] * S, {}
        for r in range(len(SQ.ENDS)):
            want = SQ._round(twin, r, range(S), fed)
            labels = [None] + [SQ._gt(r, s) if SQ.LABELLED[r][s] else None for s in (1, 2)]
            if r == 2:
                labels = [None if g is None else torch.from_numpy(g).to(DEV) for g in labels]
            samples = [_sample(r, s, by_time=r == 3, label=r if s == 0 and SQ.LABELLED[r][0] else None) for s in range(S)]
            got = seg.segment_at(samples=samples, labels=labels)
            assert got.valid == tuple(x is not None for x in samples) == want.valid, r
            for s in range(S):
                if got.valid[s]:
                    _same_rows(got, s, want, s, f'{rtype} {mode} graph={graph}: round {r} lane {s}')
            torch.cuda.synchronize()
            assert torch.equal(seg.confusion, twin.confusion), f'round {r}: confusion'
            assert seg.last_flags.tolist() == [0 if x is not None else hip.EVENT_STORE_FLAG_RANGE for x in samples]
            kept[r] = (got.clone(), want.clone())
        assert bool(seg.confusion.any()) and seg.n_captures == (2 if graph else 0)  # (one capture per rule: by index, by time)
        # -- lanes permuted against recordings: lane i serves stream perm[i], at round 1's ends; every lane is handed a host label
        perm, r = (2, 0, 1), 1
        before = seg.confusion.clone()
        got = seg.segment_at(samples=[_sample(r, s) for s in perm], labels=[SQ._gt(r, s) for s in perm])
        for i, s in enumerate(perm):
            _same_rows(got, i, kept[r][1], s, f'permuted lane {i} = stream {s}')
            assert torch.equal((seg.confusion[i] - before[i]).cpu(), SQ._confusion_of(got.labels[i], SQ._gt(r, s)))
        # -- two lanes on ONE recording with different ends (the third idle): two separate rounds of the twin
        ends = (4000, 3900)
        before = seg.confusion.clone()
        got = seg.segment_at(samples=[StoreSample(REC[0], end=ends[0], map=0), StoreSample(REC[0], end=ends[1], map=0, label=2), None])
        for i, e in enumerate(ends):
            want = twin.segment_at(end=[e, None, None])
            _same_rows(got, i, want, 0, f'two lanes on one recording: lane {i}')
        assert got.valid == (True, True, False)
        assert torch.equal(seg.confusion[0], before[0]) and torch.equal(seg.confusion[2], before[2])
        assert torch.equal((seg.confusion[1] - before[1]).cpu(), SQ._confusion_of(got.labels[1], SQ._gt(2, 0)))
        # -- EMPTY: lane 1's t_end lies in front of its recording's first event; it is handed a label, which must not count
        r = 3
        t0 = SQ._source(1).t[0]
        samples = [_sample(r, 0, by_time=True), StoreSample(REC[1], t_end=float(t0) - 1.0, map=1), _sample(r, 2, by_time=True)]
        before = seg.confusion.clone()
        got = seg.segment_at(samples=samples, labels=[SQ._gt(r, s) for s in range(S)])
        assert seg.last_flags.tolist() == [0, hip.EVENT_STORE_FLAG_EMPTY, 0] and got.valid == (True, True, True)
        assert torch.equal(seg.confusion[1], before[1]) and not torch.equal(seg.confusion[0], before[0])
        for s in (0, 2):
            _same_rows(got, s, kept[r][1], s, f'beside an EMPTY lane: lane {s}')
        assert seg.n_captures == (2 if graph else 0) and not bool(seg._acc.any())


@pytest.mark.parametrize('mode,graph', LD.CASES, ids=LD.IDS)
def test_the_duration_rule_and_the_loader_grid_equal_the_ring_fed_rounds(mode, graph):
    """the 'dsec' preset in miniature (fixed-duration windows, the loader's grid, rectified trilinear events) from a store against the
    ring-fed segmenter with the same keywords; then OVERFLOW: a lane whose window holds more events than window_capacity"""
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.event_store import EventStore, StoreSample
    n = LD.FED[1][0]
    src = [SQ.RG._slice(LD._source(s), 0, n) for s in range(S)]
    dense = EventColumns(src[0].t[0] + np.arange(600, dtype=np.int64) // 4, src[0].x[:600].copy(), src[0].y[:600].copy(), src[0].p[:600].copy())
    store = EventStore(3 * n + 600)
    for c in src + [dense]:
        store.add_recording(c)
    kw = LD.PRESETS['dsec']
    with SQ._Pinned(mode):
        twin = SQ._segmenter('convlstm', S, graph, SQ.TR._rig(), ring_capacity=LD.RING, **kw)
        seg = SQ._segmenter('convlstm', S, graph, SQ.TR._rig(), ring_capacity=None, store=store, window_capacity=512, **kw)
        assert seg._loader_grid and seg.window_duration == LD.D_US and seg.window_capacity == 512
        for s in range(S):
            twin.feed(s, src[s])
        rounds = [(2600, None, n), (2200, 2900, 2500)]
        kept = None
        for r, at in enumerate(rounds):
            t_end = [None if k is None else ((src[s].t[k] if k < n else src[s].t[-1] + 1).item()) for s, k in enumerate(at)]
            labels = [SQ._gt(r, s) for s in range(S)]
            want = twin.segment_at(t_end=t_end, labels=labels)
            got = seg.segment_at(samples=[None if v is None else StoreSample(s, t_end=v, map=s) for s, v in enumerate(t_end)], labels=labels)
            assert got.valid == want.valid == tuple(v is not None for v in t_end)
            for s in range(S):
                if got.valid[s]:
                    _same_rows(got, s, want, s, f'{mode} graph={graph}: duration round {r} lane {s}')
            torch.cuda.synchronize()
            assert torch.equal(seg.confusion, twin.confusion) and bool(seg._st['words'][0].max() > 64)
            kept = (want.clone(), t_end)
        # -- OVERFLOW: lane 0 names the dense recording, whose 600 events lie within 150 us: one window above window_capacity = 512
        want, t_end = kept
        before = seg.confusion.clone()
        samples = [StoreSample(3, t_end=(dense.t[-1] + 1).item())] + [StoreSample(s, t_end=t_end[s], map=s) for s in (1, 2)]
        got = seg.segment_at(samples=samples, labels=[SQ._gt(1, s) for s in range(S)])
        assert seg.last_flags.tolist() == [hip.EVENT_STORE_FLAG_OVERFLOW, 0, 0]
        assert torch.equal(seg.confusion[0], before[0]) and not torch.equal(seg.confusion[1], before[1])
        for s in (1, 2):
            _same_rows(got, s, want, s, f'beside an OVERFLOW lane: lane {s}')
        assert seg.n_captures == (1 if graph else 0) and not bool(seg._acc.any())


@pytest.mark.parametrize('mode,graph', [('mixed', True)], ids=['mixed-graph'])
def test_recording_hot_pixels_equal_the_ring_fed_hot_pixel_masks(mode, graph):
    """recording_hot_pixels against the twin's hot_pixel_masks (the rectify maps' size: masks on RAW pixels), lanes permuted against
    recordings, set_recording_hot_pixels between two replays, slots shared by the same object and refused when they run out"""
    from ess_amd import hip
    from ess_amd.datasets.hot_pixels import HotPixelMask
    store = _store()
    mh, mw = SQ.TR.SMH, SQ.TR.SMW
    g = np.random.default_rng(12)
    m0, m1, m2 = (HotPixelMask.from_bool(g.random((mh, mw)) < 0.3) for _ in range(3))
    with SQ._Pinned(mode):
        twin = SQ._segmenter('convlstm', S, graph, SQ.TR._rig(), hot_pixel_masks=[m0, None, m1])
        seg = SQ._segmenter('convlstm', S, graph, SQ.TR._rig(), store=store, ring_capacity=None, mask_slots=2,
                            recording_hot_pixels={REC[0]: m0, REC[2]: m1})
        assert seg._rec_hot.size == (mh, mw) and tuple(seg._rec_hot.words.shape) == (2, mh, hip.mask_words(mw))
        with pytest.raises(hip.EssHipError, match='set_recording_hot_pixels'):
            seg.set_hot_pixels(0, m0)
        fed = [0] * S
        r = 1
        want = SQ._round(twin, r, range(S), fed)
        perm = (1, 2, 0)
        labels = [SQ._gt(r, s) if SQ.LABELLED[r][s] else None for s in perm]
        got = seg.segment_at(samples=[_sample(r, s) for s in perm], labels=labels)
        for i, s in enumerate(perm):
            _same_rows(got, i, want, s, f'masked lane {i} = stream {s}')
        plain = SQ._segmenter('convlstm', S, False, SQ.TR._rig(), store=store, ring_capacity=None)
        bare = plain.segment_at(samples=[_sample(r, s) for s in perm])
        assert not M._same(M._row(bare, 2), M._row(got, 2)), 'the mask changes nothing: too weak a fixture'
        # -- between two replays: stream 1 gets m1 (the same object: a shared slot), stream 2 loses its mask, stream 0 keeps m0
        with pytest.raises(hip.EssHipError, match='mask_slots=2'):
            seg.set_recording_hot_pixels(REC[1], m2)
        assert seg._rec_hot.slot_of == {REC[0]: 0, REC[2]: 1}  # (refused: nothing changed)
        seg.set_recording_hot_pixels(REC[1], m1)
        seg.set_recording_hot_pixels(REC[2], None)
        assert seg._rec_hot.slot_of == {REC[0]: 0, REC[1]: 1}
        twin.set_hot_pixels(1, m1)
        twin.set_hot_pixels(2, None)
        r = 3  # (every stream runs; by index, so the one capture serves it)
        for s in range(S):
            SQ._feed_to(twin, s, s, SQ.N_SRC, fed)
        want = twin.segment_at(end=list(SQ.ENDS[r]))
        got = seg.segment_at(samples=[_sample(r, s) for s in range(S)])
        for s in range(S):
            _same_rows(got, s, want, s, f'after set_recording_hot_pixels: lane {s}')
        assert seg.n_captures == 1 and twin.n_captures == 1
