"""GPU tier: sequence rounds on the LOADER's grid (SequenceSegmenter's grid_hw / grid_rows / grid_resize / grid_normalize,
window_duration and segment_at(windows=...)), the two reference presets in miniature on the 64 x 96 models and rigs of
tests/test_hip_sequence_segmenter.py:
    "DDD17": temporal grids voxelised at 72 x 90, normalize_voxel_grid ('population'), resized to 72 x 96, the top 64 rows; the windows
             cut by time with datasets.event_feed.sequence_windows_by_time and handed over through windows=
    "DSEC":  trilinear grids through the rectify maps at 72 x 96, VoxelGrid(normalize=True) ('unbiased') over all 72 rows, the top 60
             rows resized to 64 x 96; the windows cut by window_duration at a t_end
What is asserted is BITS: labels, colours, confidences of every sequence equal a TWIN that runs per stream alone -- its windows by the
restatements of the loaders' lines (tests/loader_grid_ref.py), its grids from one standalone hip.event_scatter_ring* +
hip.event_grid_finish call with n_slots = T on the stream's own events, a fresh ImageReconstructor, decoder.predict -- and the
confusion rows equal numpy's of those labels.  T = 5, S = 3."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loader_grid_ref as LG  # noqa: E402
from tests import test_hip_event_columns as EC  # noqa: E402  (device columns)
from tests import test_hip_sequence_segmenter as SQ  # noqa: E402  (models, rigs, sources, pins, ground truths -- imported, not edited)

DEV = SQ.DEV
C, H, W, K, T, S = SQ.C, SQ.H, SQ.W, SQ.K, SQ.T, SQ.S
RING = 2048
D_US = 20_000  # the DSEC preset's window_duration: T windows of 20 ms, about 200 events each
PRESETS = {
    'ddd17': dict(voxel='temporal', rectify_maps=None, grid_hw=(72, 90), grid_resize=(72, 96), grid_normalize='population'),
    'dsec': dict(voxel='trilinear', grid_hw=(72, 96), grid_rows=60, grid_resize=(64, 96), grid_normalize='unbiased',
                 window_events=None, window_duration=D_US),
}
FINISH = {'ddd17': dict(src=(72, 90), crop_rows=72, resize=(72, 96), normalize=LG.NORM_POPULATION),
          'dsec': dict(src=(72, 96), crop_rows=60, resize=(64, 96), normalize=LG.NORM_UNBIASED)}
FED = [(1500, 1500, 1500), (3000, 3000, 3000)]  # round 1: the rings (2048 events) have wrapped and keep the events from 952 on
SAMPLES = [((200, 1400), (0, 1500), (300, 900)), ((1500, 2900), None, (1800, 3000))]  # ddd17: [begin, end) per stream; None: idle
T_END_AT = [(1400, 1450, 1500), (2600, None, 3000)]  # dsec: t_end = the time of this event (all fed: a time behind the last)
CASES = [('mixed', True), ('bf16', False)]
IDS = ['mixed-graph', 'bf16-eager']


@functools.lru_cache(maxsize=None)
def _source(s):
    """SQ's recordings with every stream's times in MICROSECONDS (one window_duration serves all three): stream 1's float64 seconds
    become float64 microseconds, a quarter off the integers"""
    from ess_amd.datasets.data_util import EventColumns
    src = SQ._source(s)
    if src.t.dtype == np.int64:
        return src
    return EventColumns(np.round(src.t * 1e6) + 0.25, src.x, src.y, src.p)


def _t_end(r, s):
    k = T_END_AT[r][s]
    if k is None:
        return None
    t = _source(s).t
    v = t[k] if k < FED[r][s] else t[FED[r][s] - 1] + 1
    return int(v) if t.dtype == np.int64 else float(v)


@functools.lru_cache(maxsize=None)
def _windows(preset, r, s):
    """round r's T windows of stream s as the LOADER cuts them -> [(first, behind)] in absolute indices, or None (idle)"""
    t = _source(s).t
    if preset == 'ddd17':
        if SAMPLES[r][s] is None:
            return None
        a, b = SAMPLES[r][s]
        return [(a + i, a + j) for i, j in LG.loader_cut_by_time(t[a:b], T)]
    if T_END_AT[r][s] is None:
        return None
    return LG.loader_cut_fixed_duration(t[:FED[r][s]], _t_end(r, s), T, T * D_US)


def _check_the_rounds_cover_what_they_are_meant_to():
    for preset in PRESETS:
        for r in range(2):
            for s in range(S):
                w = _windows(preset, r, s)
                if w is not None:
                    assert all(b - a > 20 for a, b in w), (preset, r, s, w)  # real windows, not the empty case
                    assert w[0][0] >= FED[r][s] - RING and w[-1][1] <= FED[r][s]
    assert any(a // RING != (b - 1) // RING for r in range(2) for s in range(S) for a, b in (_windows('dsec', r, s) or []))  # across the wrap
    assert len({b - a for a, b in _windows('ddd17', 0, 0)}) > 1 and len({b - a for a, b in _windows('dsec', 0, 0)}) > 1  # cut by TIME


@functools.lru_cache(maxsize=None)
def _grids(preset, r, s):
    """the twin's grids: the stream's own events from the first window's start on, laid out from entry 0 of a lone ring; ONE
    hip.event_scatter_ring* + hip.event_grid_finish call over the T windows -> [1, T * C, H, W] on the device"""
    from ess_amd import hip
    f, wins, src = FINISH[preset], _windows(preset, r, s), _source(s)
    base = wins[0][0]
    lone = SQ.RG._slice(src, base, wins[-1][1])
    dev = EC._device_columns([lone], lone.n)
    words = [EC._words(v) for v in ([0] * T, [a - base for a, _ in wins], [b - a for a, b in wins], [lone.format] * T)]
    acc = torch.zeros(T, C, *f['src'], dtype=torch.int64, device=DEV)
    if preset == 'dsec':
        m = SQ.TR._rig()[s]
        maps = None if m is None else torch.from_numpy(m)[None].to(DEV)
        hip.event_scatter_ring_trilinear(*dev, *words, acc, maps, None if m is None else EC._words([0] * T))
    else:
        hip.event_scatter_ring(*dev, *words, acc)
    assert bool(acc.any())
    out = torch.full((T, C, H, W), float('nan'), device=DEV)
    hip.event_grid_finish(words[2], acc, out, crop_rows=f['crop_rows'], resize=f['resize'], normalize=f['normalize'])
    assert not bool(acc.any()) and bool(out.isfinite().all())
    return out.view(1, T * C, H, W)


@functools.lru_cache(maxsize=None)
def _twin(preset, mode):
    """{(round, stream): (labels, colour, confidence)}: per stream alone, a fresh ImageReconstructor over the twin's grids"""
    from ess_amd.e2vid.image_reconstructor import ImageReconstructor
    from ess_amd.e2vid.options.inference_options import default_options
    out = {}
    with SQ._Pinned(mode):
        enc, dec = SQ._models('convlstm')
        pal = SQ.SH.palette_for(K).to(DEV)
        for r in range(2):
            for s in range(S):
                if _windows(preset, r, s) is None:
                    continue
                rec = ImageReconstructor(enc, H, W, C, DEV, default_options())
                _, _, latent = rec.update_reconstruction_sequence(_grids(preset, r, s), T, need_image=False, final_lean=True)
                lab, col, conf = dec.predict(latent, window=(0, 0, H, W), palette=pal, want_confidence=True)
                out[(r, s)] = (lab[0].clone(), col[0].clone(), conf[0].clone())
        torch.cuda.synchronize()
    return out


def _feed_to(seg, s, upto, fed):
    while fed[s] < upto:
        n = min(SQ.PACKET, upto - fed[s])
        assert seg.feed(s, SQ.RG._slice(_source(s), fed[s], fed[s] + n)) == fed[s] + n
        fed[s] += n


def _segment(seg, preset, r):
    from ess_amd.datasets.event_feed import sequence_windows_by_time
    labels = [SQ._gt(r, s) for s in range(S)]
    if preset == 'dsec':
        return seg.segment_at(t_end=[_t_end(r, s) for s in range(S)], labels=labels)
    wins = [None if SAMPLES[r][s] is None else sequence_windows_by_time(_source(s).t, *SAMPLES[r][s], T) for s in range(S)]
    return seg.segment_at(windows=wins, labels=labels)


@pytest.mark.parametrize('preset', list(PRESETS))
@pytest.mark.parametrize('mode,graph', CASES, ids=IDS)
def test_loader_grid_rounds_equal_the_twin(preset, mode, graph):
    """two rounds at S = 3 (the second on wrapped rings, one stream idle): every sequence's labels, colours and confidence bits equal
    the twin's; the confusion rows equal numpy's of the twin's labels; ONE capture; the sums end zero"""
    _check_the_rounds_cover_what_they_are_meant_to()
    twin = _twin(preset, mode)
    with SQ._Pinned(mode):
        seg = SQ._segmenter('convlstm', S, graph, SQ.TR._rig(), ring_capacity=RING, **PRESETS[preset])
        assert tuple(seg._acc.shape) == (T * S, C) + FINISH[preset]['src'] and tuple(seg._in.shape) == (T * S, C, H, W)
        fed, want = [0] * S, torch.zeros(S, K, K, dtype=torch.int64)
        for r in range(2):
            for s in range(S):
                _feed_to(seg, s, FED[r][s], fed)
            res = _segment(seg, preset, r)
            on = tuple(_windows(preset, r, s) is not None for s in range(S))
            assert res.valid == on and any(on) and (r == 0 or not all(on))
            for s in range(S):
                if on[s]:
                    assert SQ.M._same(SQ.M._row(res, s), twin[(r, s)]), f'{preset} {mode} graph={graph}: round {r} stream {s} differs from the twin'
                    want[s] += SQ._confusion_of(twin[(r, s)][0], SQ._gt(r, s))
                    assert len(res.labels[s].unique()) >= 3, 'too uniform a fixture'
            torch.cuda.synchronize()
            assert torch.equal(seg.confusion.cpu(), want), f'round {r}: confusion'
        assert seg.n_captures == (1 if graph else 0) and seg.n_rounds == 2
        assert not bool(seg._acc.any())


def test_explicit_windows_and_durations_are_checked_before_anything_is_written():
    from ess_amd import hip
    with SQ._Pinned('bf16'):
        for kw, match in ((dict(grid_hw=(72, 90)), 'the widths must agree'), (dict(grid_hw=(60, 96)), 'height <= 60'),
                          (dict(grid_hw=(72, 96), grid_rows=73), 'grid_rows=73'), (dict(grid_normalize='biased'), "grid_normalize='biased'"),
                          (dict(grid_resize=(64, 96, 1)), 'grid_resize='), (dict(window_duration=10.0), 'not both'),
                          (dict(window_events=None, window_duration=10.0, ring_capacity=None), 'window_duration needs ring_capacity'),
                          (dict(window_events=None, window_duration=0), 'window_duration=0')):
            with pytest.raises(hip.EssHipError, match=match):
                SQ._segmenter('convlstm', S, False, SQ.TR._rig(), **kw)
        seg = SQ._segmenter('convlstm', S, False, SQ.TR._rig(), ring_capacity=RING, **PRESETS['dsec'])
        for s in range(S):
            seg.feed(s, SQ.RG._slice(_source(s), 0, 3000))
        ok = [(2000 + 100 * i, 100) for i in range(T)]
        for bad, match in (([ok, ok], 'one entry per stream'), ([ok, ok[:4], ok], r'windows\[1\] must hold sequence_steps=5 pairs'),
                           ([ok, ok, ok[:4] + [(2400, 601)]], r'windows\[2\]\[4\]=\(2400, 601\).*3000 events fed'),
                           ([ok[:4] + [(951, 10)], ok, ok], r'windows\[0\]\[4\]=\(951, 10\).*keeps events from 952 on'),
                           ([ok, ok[:4] + [(2400.0, 5)], ok], r'windows\[1\]\[4\]'), ([ok, ok[:4] + [(-1, 5)], ok], r'windows\[1\]\[4\]')):
            with pytest.raises(hip.EssHipError, match=match):
                seg.segment_at(windows=bad)
        with pytest.raises(hip.EssHipError, match='without t_end and end'):
            seg.segment_at(windows=[ok] * 3, t_end=[None] * 3)
        with pytest.raises(hip.EssHipError, match='cuts by time'):
            seg.segment_at(end=[2500] * 3)
        with pytest.raises(hip.EssHipError, match='not after the oldest kept event'):
            seg.segment_at(t_end=[_source(0).t[960], None, None])
        assert seg.n_rounds == 0 and not bool(seg._acc.any())
        # windows without events are allowed: all-zero grids, a sequence all the same; a stream never fed can only name such windows
        seg.drop_feed([1])
        res = seg.segment_at(windows=[ok, [(0, 0)] * T, None])
        assert res.valid == (True, True, False) and not bool(seg._acc.any())


def test_a_segmenter_without_the_new_keywords_still_equals_the_existing_twin():
    """no grid_* keyword, no window_duration, no windows=: the round goes through hip.event_ingest_ring_trilinear as before, and round 0
    of tests/test_hip_sequence_segmenter.py equals that file's twin bit for bit"""
    rtype, mode = 'convlstm', 'mixed'
    twin = SQ._twin(rtype, mode)
    with SQ._Pinned(mode):
        seg = SQ._segmenter(rtype, S, True, SQ.TR._rig())
        assert not seg._loader_grid and seg.window_duration is None and tuple(seg._acc.shape) == (T * S, C, H, W)
        res = SQ._round(seg, 0, range(S), [0] * S)
        assert res.valid == (True,) * S
        for s in range(S):
            assert SQ.M._same(SQ.M._row(res, s), twin[(0, s)]), f'stream {s}'
        assert not bool(seg._acc.any())
