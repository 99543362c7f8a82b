"""GPU tier: sequence rounds (ess_amd/run_sequence_segmentation.py: SequenceSegmenter) -- the DSEC validation protocol from a fed
event stream.  What is asserted is BITS and INTEGERS: every round's labels, colours and confidences equal those of a TWIN that runs,
per stream alone, a fresh ImageReconstructor over the numpy restatement's grids of the stream's T windows
(update_reconstruction_sequence(T, need_image=False, final_lean=True), then decoder.predict), the windows cut by the literal
restatement of the DSEC loader (tests/test_host_sequence_cut.py); the per-stream confusion matrix equals numpy's of the returned
labels against the ground truth.  The 64 x 96 models of tests/test_hip_stream_compaction.py; the maps, raw events and restatement
of tests/test_host_event_trilinear.py.  T = 5 > pair_steps() = 3: steps with and without the operand pair both run."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_event_ring as RG  # noqa: E402  (_slice)
from tests import test_hip_event_trilinear as TR  # noqa: E402  (the rig: two maps of a 72 x 104 sensor, stream 2 without one)
from tests import test_hip_multi_stream as M  # noqa: E402  (models, result rows, the pins)
from tests import test_hip_seg_head as SH  # noqa: E402  (palette)
from tests import test_hip_stream_compaction as SC  # noqa: E402  (the 64 x 96 weights)
from tests import test_host_event_trilinear as T_  # noqa: E402  (restate, raw_events)
from tests.test_host_sequence_cut import loader_cut  # noqa: E402

DEV = M.DEV
C, H, W, K = SC.C, SC.H, SC.W, SC.K
T, NW, S, RING = 5, 256, 3, 1536  # a sequence reads up to T * NW = 1280 events; the ring wraps once 1536 have been fed
N_SRC = 4096
IGNORE = 255
CASES = [('convlstm', mode, graph) for mode in ('mixed', 'bf16') for graph in (False, True)] + [('convgru', 'mixed', True)]
IDS = [f'{r}-{m}-{"graph" if g else "eager"}' for r, m, g in CASES]

# Per round: how far each stream has been fed in front of it (packets of 333 events: they straddle windows and wrap the ring), and
# where its sequence ends (an absolute index; None: idle; round 3 asks by TIME).  Round 0: fewer than T * NW events fed (windows of
# 140 / 130 events).  Round 1 overlaps round 0 (from 620 on) and stream 2 has no label.  Round 2: stream 1 is idle -- and is handed a
# label all the same, which must not count -- and the sequences wrap the ring.  Round 3: everything fed; by t_end.
FED = [(700, 700, 700), (2000, 2100, 1800), (2600, 2300, 3000), (N_SRC, N_SRC, N_SRC)]
ENDS = [(700, 650, 700), (1900, 2000, 1777), (2500, None, 2900), (4000, 3900, N_SRC)]
LABELLED = [(True, True, True), (True, True, False), (True, True, True), (True, True, True)]
PACKET = 333


def _check_the_rounds_cover_what_they_are_meant_to():
    assert T > 3 and all(e <= T * NW for e in ENDS[0]) and ENDS[1][0] - T * NW < ENDS[0][0]
    assert ENDS[2][1] is None and not LABELLED[1][2]
    for fed, ends in zip(FED, ENDS):
        for f, e in zip(fed, ends):
            assert e is None or (e <= f and max(0, e - T * NW) >= f - RING)  # in reach of the ring
    assert any(e is not None and (e - T * NW) // RING != (e - 1) // RING for e in ENDS[2])  # a sequence across the ring's wrap
    assert RING % 16 == 0 and RING >= T * NW and PACKET % NW and FED[-1][0] > 2 * RING


@functools.lru_cache(maxsize=None)
def _source(s):
    """stream s's whole recording: stream 0 int64 / uint16, 1 float64 / int16, 2 int64 / int16"""
    return T_.raw_events(N_SRC, TR.SMH, TR.SMW, 700 + s, fmt=(3, 0, 1)[s], t_span_us=400_000)


def _end_of(r, s):
    return ENDS[r][s]


def _t_end(r, s):
    """round 3's request by time: the time of event ENDS[3][s] where it is the first of its time, a time after the last event where
    the sequence ends with the recording -- the index the test expects comes from np.searchsorted on the whole recording"""
    src, e = _source(s), ENDS[r][s]
    if e >= src.n:
        return src.t[-1] + (1 if src.t.dtype == np.int64 else 1e-6)
    return src.t[e]


def _expected_end(r, s):
    e = ENDS[r][s]
    if e is None or r < 3:
        return e
    return int(np.searchsorted(_source(s).t, _t_end(r, s), side='left'))


def _windows(r, s):
    """the index ranges of round r's T windows of stream s by the loader's lines, or None"""
    e = _expected_end(r, s)
    if e is None:
        return None
    chunks, _ = loader_cut(np.arange(N_SRC), e, T, NW)
    return None if chunks[0].size == 0 else [(int(c[0]), int(c[-1]) + 1) for c in chunks]


@functools.lru_cache(maxsize=None)
def _grids(r, s):
    """the restatement's grids of the T windows, [1, T * C, H, W] on the device, built once"""
    rig = TR._rig()
    g = [T_.restate(RG._slice(_source(s), a, b), rig[s], C, H, W) for a, b in _windows(r, s)]
    return torch.from_numpy(np.concatenate(g)[None]).to(DEV)


@functools.lru_cache(maxsize=None)
def _gt(r, s):
    """uint8 [H, W]: classes below K, 10 % values >= K, 10 % the ignore value"""
    g = np.random.default_rng(100 * r + s)
    kind = g.random((H, W))
    gt = g.integers(0, K, (H, W))
    gt = np.where(kind > 0.8, K + g.integers(0, 3, (H, W)), gt)
    return np.where(kind > 0.9, IGNORE, gt).astype(np.uint8)


def _models(rtype):
    return M._models(*SC._weights(rtype), K)


def _segmenter(rtype, n_streams, graph, maps, **kw):
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    kw = dict(dict(sequence_steps=T, window_events=NW, ring_capacity=RING, voxel='trilinear', rectify_maps=maps, graph=graph,
                   palette=SH.palette_for(K), want_confidence=True), **kw)
    return SequenceSegmenter(*_models(rtype), H, W, default_options(), n_streams, **kw)


class _Pinned:
    """the compute configuration and the two batch-size switches, as the existing stream tests pin them"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from ess_amd import hip
        hip.set_compute(self.mode)
        self.prev, self.prev_split = M._pinned_s2d(), M._pinned_norm_split(hip)
        return hip

    def __exit__(self, *exc):
        from ess_amd import hip
        from ess_amd.e2vid.model.submodules import set_s2d_mode
        set_s2d_mode(self.prev)
        hip.tuning_set('norm_split_wgs', self.prev_split)
        hip.set_compute('fp32')


@functools.lru_cache(maxsize=None)
def _twin(rtype, mode):
    """{(round, stream): (labels, colour, confidence) [H, W]...} of every sequence that runs: per stream ALONE, a fresh
    ImageReconstructor, the restated grids, update_reconstruction_sequence and decoder.predict.  Computed once per configuration."""
    from ess_amd.e2vid.image_reconstructor import ImageReconstructor
    from ess_amd.e2vid.options.inference_options import default_options
    out = {}
    with _Pinned(mode):
        enc, dec = _models(rtype)
        pal = SH.palette_for(K).to(DEV)
        for r in range(len(ENDS)):
            for s in range(S):
                if _windows(r, s) is None:
                    continue
                rec = ImageReconstructor(enc, H, W, C, DEV, default_options())
                assert rec.crop.is_identity
                _, _, latent = rec.update_reconstruction_sequence(_grids(r, s), T, need_image=False, final_lean=True)
                lab, col, conf = dec.predict(latent, window=(0, 0, H, W), palette=pal, want_confidence=True)
                out[(r, s)] = (lab[0].clone(), col[0].clone(), conf[0].clone())
        torch.cuda.synchronize()
    return out


def _feed_to(seg, slot, s, upto, fed):
    """stream slot of seg receives source s's events [fed[slot], upto) in packets of PACKET events"""
    while fed[slot] < upto:
        n = min(PACKET, upto - fed[slot])
        assert seg.feed(slot, RG._slice(_source(s), fed[slot], fed[slot] + n)) == fed[slot] + n
        fed[slot] += n


def _round(seg, r, sources, fed):
    """round r of a segmenter whose stream i delivers source sources[i] -> the result"""
    for i, s in enumerate(sources):
        _feed_to(seg, i, s, FED[r][s], fed)
    labels = [_gt(r, s) if LABELLED[r][s] else None for s in sources]
    if r == 2:
        labels = [torch.from_numpy(g).to(DEV) for g in labels]  # (device tensors are taken too)
    if r < 3:
        return seg.segment_at(end=[_end_of(r, s) for s in sources], labels=labels)
    return seg.segment_at(t_end=[_t_end(r, s) for s in sources], labels=labels)


def _confusion_of(labels, gt):
    g, lab = gt.astype(np.int64).ravel(), labels.cpu().numpy().astype(np.int64).ravel()
    m = (g != IGNORE) & (g < K)
    return torch.from_numpy(np.bincount(g[m] * K + lab[m], minlength=K * K).reshape(K, K))


def test_normalize_slices_at_batch_one_equals_normalize_samples():
    """the twin's normalisation (slices, B = 1) and the segmenter's (per sample) are one arithmetic: same bits"""
    from ess_amd import hip
    x = _grids(1, 0)
    a, b = hip.event_normalize_slices(x, T), hip.event_normalize_samples(x.view(T, C, H, W).contiguous())
    assert bool(x.any()) and torch.equal(a.view(T, C, H, W).view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('rtype,mode,graph', CASES, ids=IDS)
def test_rounds_equal_the_twin_and_score_themselves(rtype, mode, graph):
    """four rounds at S = 3: labels, colours, confidence bits of every sequence equal the twin's (eager and replay both equal it, hence
    each other); valid marks exactly the sequences that ran; the confusion rows equal numpy's of the returned labels, an idle or
    unlabelled stream's row does not move; metrics() equals MetricsSemseg on the same matrix; ONE capture; the ingest's sums end zero"""
    from ess_amd.evaluation.metrics import MetricsSemseg
    _check_the_rounds_cover_what_they_are_meant_to()
    twin = _twin(rtype, mode)
    with _Pinned(mode):
        seg = _segmenter(rtype, S, graph, TR._rig())
        assert seg.ring_capacity == RING and tuple(seg._words.shape) == (5, T * S) and tuple(seg.confusion.shape) == (S, K, K)
        fed, want = [0] * S, torch.zeros(S, K, K, dtype=torch.int64)
        for r in range(len(ENDS)):
            res = _round(seg, r, range(S), fed)
            on = tuple(_windows(r, s) is not None for s in range(S))
            assert res.valid == on and any(on), (r, res.valid)
            assert res.labels.dtype == torch.uint8 and tuple(res.labels.shape) == (S, H, W) and tuple(res.colour.shape) == (S, H, W, 3)
            before = want.clone()
            for s in range(S):
                if not on[s]:
                    continue
                assert M._same(M._row(res, s), twin[(r, s)]), f'{rtype} {mode} graph={graph}: round {r} stream {s} differs from the twin'
                if LABELLED[r][s]:
                    want[s] += _confusion_of(res.labels[s], _gt(r, s))
            torch.cuda.synchronize()
            assert torch.equal(seg.confusion.cpu(), want), f'round {r}: confusion'
            for s in range(S):
                if not (on[s] and LABELLED[r][s]):
                    assert torch.equal(want[s], before[s])  # (the row did not move)
                else:
                    assert int((want[s] - before[s]).sum()) == int(((_gt(r, s) != IGNORE) & (_gt(r, s) < K)).sum()) > H * W // 2
                    assert len(res.labels[s].unique()) >= 4, 'too uniform a fixture'
        assert seg.n_captures == (1 if graph else 0) and seg.n_rounds == len(ENDS)
        assert not bool(seg._acc.any())
        ref = MetricsSemseg(K, IGNORE, [str(k) for k in range(K)])
        for streams, cm in ((None, want.sum(0)), ([2], want[2]), ([0, 1], want[0] + want[1])):
            ref.metrics_acc = cm.clone()
            summary, got = ref.get_metrics_summary(), seg.metrics(streams)
            assert torch.equal(got['cm'], cm) and torch.equal(got['mean_iou'], summary['mean_iou']) and torch.equal(got['acc'], summary['acc'])
            assert 0 < float(got['acc']) < 100
        seg.reset_metrics([1])
        want[1] = 0
        assert torch.equal(seg.confusion.cpu(), want) and bool(want[0].any()) and bool(want[2].any())
        seg.reset_metrics()
        assert not bool(seg.confusion.any())


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_each_stream_equals_itself_alone(graph):
    """every stream of the S = 3 segmenter gets what an n_streams = 1 segmenter gives it on the same feed (the twin is the common
    reference: both sides equal it bit for bit); the lone segmenter's confusion row equals the stream's row of the batch"""
    rtype, mode = 'convlstm', 'mixed'
    twin = _twin(rtype, mode)
    with _Pinned(mode):
        rig = TR._rig()
        for s in range(S):
            alone = _segmenter(rtype, 1, graph, [rig[s]])
            fed, want = [0], torch.zeros(K, K, dtype=torch.int64)
            for r in range(len(ENDS)):
                res = _round(alone, r, [s], fed)
                assert res.valid == (_windows(r, s) is not None,)
                if res.valid[0]:
                    assert M._same(M._row(res, 0), twin[(r, s)]), f'graph={graph}: stream {s} alone, round {r}'
                    if LABELLED[r][s]:
                        want += _confusion_of(res.labels[0], _gt(r, s))
            assert torch.equal(alone.confusion[0].cpu(), want) and alone.n_captures == (1 if graph else 0)
            assert not bool(alone._acc.any())


def test_a_round_is_a_pure_function_of_its_events():
    """the same round twice, and the round on a feed whose windows' INNER events are permuted (each window keeps its first and its
    last event: they carry the time normalisation): identical bits -- the ingest sums integers"""
    rtype, mode, r = 'convlstm', 'mixed', 1
    with _Pinned(mode):
        rig = TR._rig()
        seg = _segmenter(rtype, S, True, rig)
        shuffled = _segmenter(rtype, S, True, rig)
        g = np.random.default_rng(5)
        for s in range(S):
            src = _source(s)
            seg.feed(s, RG._slice(src, 0, FED[r][s]))
            order = np.arange(FED[r][s])
            for a, b in _windows(r, s):
                order[a + 1:b - 1] = g.permutation(order[a + 1:b - 1])
            assert (order != np.arange(FED[r][s])).sum() > T * NW // 2
            from ess_amd.datasets.data_util import EventColumns
            shuffled.feed(s, EventColumns(*(np.ascontiguousarray(v[order]) for v in (src.t, src.x, src.y, src.p))))
        ends = [ENDS[r][s] for s in range(S)]
        first = seg.segment_at(end=ends)
        again = seg.segment_at(end=ends)
        other = shuffled.segment_at(end=ends)
        for s in range(S):
            assert M._same(M._row(first, s), M._row(again, s)), f'stream {s}: the same round twice'
            assert M._same(M._row(first, s), M._row(other, s)), f'stream {s}: permuted inner events'
        assert first.labels.data_ptr() != again.labels.data_ptr()  # (copy=True: clones of the replay's buffers)
        assert not bool(seg.confusion.any())  # (no labels given: nothing scored)


def test_refusals():
    from ess_amd import hip
    rtype = 'convlstm'
    with _Pinned('bf16'):
        with pytest.raises(hip.EssHipError, match='ring_capacity=1279'):
            _segmenter(rtype, S, False, TR._rig(), ring_capacity=T * NW - 1)
        seg = _segmenter(rtype, S, False, TR._rig())
        for s in range(S):
            seg.feed(s, RG._slice(_source(s), 0, 2000))
        ok = [1900, 1900, 1900]
        with pytest.raises(hip.EssHipError, match='one of the two'):
            seg.segment_at()
        with pytest.raises(hip.EssHipError, match='one of the two'):
            seg.segment_at(t_end=[None] * S, end=ok)
        with pytest.raises(hip.EssHipError, match='one entry per stream'):
            seg.segment_at(end=ok[:2])
        with pytest.raises(hip.EssHipError, match=r'end\[1\]=2001'):
            seg.segment_at(end=[1900, 2001, 1900])
        # 2000 fed, the ring keeps events from 464 on: a sequence that ends at 1700 would start at 420
        with pytest.raises(hip.EssHipError, match=r'end\[2\]=1700: the sequence reaches back to event 420'):
            seg.segment_at(end=[1900, 1900, 1700])
        with pytest.raises(hip.EssHipError, match='reach back to event'):
            seg.segment_at(t_end=[None, None, _source(2).t[1700]])
        with pytest.raises(hip.EssHipError, match='not after the oldest kept event'):
            seg.segment_at(t_end=[_source(0).t[100], None, None])
        gt = _gt(0, 0)
        for bad, match in (([gt, gt], 'one entry per stream'), ([gt, gt[:-1], gt], r'labels\[1\] must be uint8'),
                           ([gt, gt, gt.astype(np.int64)], r'labels\[2\] must be uint8'), ([gt, 'x', gt], r'labels\[1\] must be a uint8')):
            with pytest.raises(hip.EssHipError, match=match):
                seg.segment_at(end=ok, labels=bad)
        with pytest.raises(hip.EssHipError, match='before the previous packet'):
            seg.feed(0, RG._slice(_source(0), 0, 10))
        with pytest.raises(hip.EssHipError, match='a ring holds one format'):
            seg.feed(0, RG._slice(_source(1), 2000, 2010))
        assert seg.n_rounds == 0 and not bool(seg.confusion.any())  # (everything was refused before anything ran)
        assert seg.segment_at(end=ok).valid == (True, True, True)
        seg.drop_feed([1])
        assert seg.fed(1) == 0 and seg.segment_at(end=[1900, 5, 1900]).valid == (True, False, True)  # (nothing fed: idle)
        hip.set_compute('mixed')
        with pytest.raises(hip.EssHipError, match="built in the 'bf16' configuration"):
            seg.segment_at(end=ok)
