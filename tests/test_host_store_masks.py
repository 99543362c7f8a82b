"""CPU tier of hot-pixel masks on the device event store (hip.event_ingest_store, hip.event_store_pixel_counts, hip.event_count_mask,
HotPixelMask.from_store): the three C entry points and their refusals -- each before a launch --, the bindings' and the class's
refusals -- each before a device call, the store left as it was --, and the numpy restatement of the count rule
(tests/store_mask_ref.py) proved equal to tests/hot_pixel_ref.py where the two overlap."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import hot_pixel_ref as HR
from tests import store_mask_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_event_ingest_store', 'ess_event_store_pixel_counts', 'ess_event_count_mask')
EINVAL = -22


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_three_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert callable(hip.event_ingest_store) and callable(hip.event_store_pixel_counts) and callable(hip.event_count_mask)
    assert (MR.T_I64, MR.XY_U16, MR.REPLACE, MR.OR) == (hip.EVCOL_T_I64, hip.EVCOL_XY_U16, hip.MASK_REPLACE, hip.MASK_OR)


# ---------------------------------------------------------------------------------------------- the library's refusals
def _refused(L, call, cases, prefix):
    for kw, msg in cases:
        assert call(**kw) == EINVAL, kw
        text = L.ess_last_error().decode()
        assert msg in text and text.startswith(prefix), (kw, text)


def test_the_store_ingest_refuses_bad_arguments_before_any_launch(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced)

    def call(t=one, x=one, y=one, p=one, starts=one, counts=one, formats=one, cap=64, total=60, wcap=16, n=2, C=3, H=4, W=5, acc=one,
             acc_bytes=1 << 20, out=one, flavour=0, maps=P(0), map_of=P(0), n_maps=0, masks=P(0), mask_of=one, n_masks=0, mh=1, mw=1):
        return L.ess_event_ingest_store(t, x, y, p, starts, counts, formats, cap, total, wcap, n, C, H, W, acc, acc_bytes, out, flavour,
                                        maps, map_of, n_maps, 1, 1, masks, mask_of, n_masks, mh, mw, P(0))
    cases = [(dict(t=P(0)), 'null'), (dict(starts=P(0)), 'null'), (dict(formats=P(0)), 'null'), (dict(acc=P(0)), 'null'),
             (dict(x=P(8)), '16-byte'), (dict(acc=P(24)), '16-byte'), (dict(out=P(24)), '16-byte'), (dict(starts=P(20)), '8-byte'),
             (dict(counts=P(18)), '4-byte'), (dict(wcap=0), 'window_capacity=0'),
             (dict(wcap=(1 << 22) + 1), 'the int64 sums hold 2^22 contributions'), (dict(cap=72, total=0), 'capacity=72'),
             (dict(cap=(1 << 40) + 16), 'capacity='), (dict(total=65), 'total=65'), (dict(total=-1), 'total=-1'), (dict(n=0), 'n_slots=0'),
             (dict(n=65536), 'n_slots=65536'), (dict(flavour=4), 'flavour=4'), (dict(flavour=-1), 'flavour=-1'),
             (dict(flavour=1, C=3), 'must be even'), (dict(flavour=2, C=3), 'must be 2'), (dict(H=0), 'height=0'),
             (dict(acc_bytes=2 * 3 * 4 * 5 * 8 - 1), 'are needed'),
             (dict(flavour=3), 'null map_of'), (dict(flavour=3, map_of=one, n_maps=1), 'maps must be null'),
             # maps without the trilinear flavour
             (dict(maps=one, map_of=one, n_maps=1), 'belong to flavour=3'), (dict(flavour=2, C=2, map_of=one), 'belong to flavour=3'),
             # the masks
             (dict(masks=one, n_masks=1, mask_of=P(0)), 'null mask_of'), (dict(mask_of=P(0)), 'null mask_of'),
             (dict(masks=one, n_masks=0), 'masks must be null'), (dict(n_masks=2), 'masks must be null'), (dict(n_masks=-1), 'n_masks=-1'),
             (dict(masks=one, n_masks=1, mh=0), 'mask_height=0'), (dict(masks=one, n_masks=1, mw=32769), 'mask_width=32769'),
             (dict(masks=P(24), n_masks=1), 'masks must be 16-byte'), (dict(mask_of=P(18)), 'mask_of must be 4-byte')]
    _refused(L, call, cases, 'event_ingest_store:')
    # out is nullable (scatter only): the next refusal in line is then reached
    assert call(out=P(0), total=65) == EINVAL and 'total=65' in L.ess_last_error().decode()


def test_the_counts_and_the_count_mask_refuse_bad_arguments_before_any_launch(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced)

    def count(x=one, y=one, cap=64, total=60, begins=one, ends=one, formats=one, n=2, H=4, W=5, counts=one):
        return L.ess_event_store_pixel_counts(x, y, cap, total, begins, ends, formats, n, H, W, counts, P(0))
    cases = [(dict(x=P(0)), 'null'), (dict(begins=P(0)), 'null'), (dict(ends=P(0)), 'null'), (dict(formats=P(0)), 'null'),
             (dict(counts=P(0)), 'null'), (dict(y=P(8)), '16-byte'), (dict(begins=P(20)), '8-byte'), (dict(counts=P(12)), '8-byte'),
             (dict(formats=P(18)), '4-byte'), (dict(H=0), 'height=0'), (dict(W=0), 'width=0'), (dict(W=32769), 'width=32769'),
             (dict(n=0), 'n=0'), (dict(n=65536), 'n=65536'), (dict(cap=72), 'capacity=72'), (dict(cap=0, total=0), 'capacity=0'),
             (dict(cap=(1 << 40) + 16), 'capacity='), (dict(total=65), 'total=65'), (dict(total=-1), 'total=-1')]
    _refused(L, count, cases, 'event_store_pixel_counts:')

    def mask(counts=one, n=2, H=4, W=5, thresholds=one, masks=one, mode=0):
        return L.ess_event_count_mask(counts, n, H, W, thresholds, masks, mode, P(0))
    cases = [(dict(counts=P(0)), 'null counts'), (dict(thresholds=P(0)), 'null'), (dict(masks=P(0)), 'null'), (dict(counts=P(8)), '16-byte'),
             (dict(masks=P(8)), '16-byte'), (dict(thresholds=P(20)), '8-byte'), (dict(n=0), 'n=0'), (dict(H=0), 'height=0'),
             (dict(W=32769), 'width=32769'), (dict(mode=2), 'mode=2'), (dict(mode=-1), 'mode=-1')]
    _refused(L, mask, cases, 'event_count_mask:')
    # the entry point it shares its kernel with still speaks under its own name
    assert L.ess_event_hot_pixel_mask(P(0), 2, 4, 5, one, one, 0, P(0)) == EINVAL
    assert L.ess_last_error().decode() == 'event_hot_pixel_mask: null sums, thresholds or masks'


def test_the_wrappers_refuse_on_the_host():
    import torch
    from ess_amd import hip
    cap = 32
    cols = [torch.zeros(cap, dtype=d) for d in (torch.int64, torch.int16, torch.int16, torch.uint8)]
    starts, words = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    out, acc = torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5, dtype=torch.int64)
    masks = torch.zeros(1, 4, 1, dtype=torch.int32)
    ok = dict(flavour=hip.EVENT_STORE_SIGNED, total=20, window_capacity=8)
    for change, msg in ((dict(flavour=7), 'flavour=7'), (dict(total=33), 'total=33'), (dict(window_capacity=0), 'window_capacity=0'),
                        (dict(flavour=hip.EVENT_STORE_HISTOGRAM), 'fills 2 planes'), (dict(maps=torch.zeros(1, 2, 2, 2)), 'maps / map_of belong'),
                        (dict(mask_size=(4, 5)), 'without masks'), (dict(masks=masks, mask_size=(4, 33)), r'\[n_masks, 4, 2\]'),
                        (dict(masks=masks, mask_size=(0, 5)), 'mask_size='), (dict(masks=masks, mask_size=(4, 5), mask_of=starts), 'mask_of must be int32'),
                        (dict(acc=torch.zeros(2, 3, 4, 5)), 'acc must be int64')):
        with pytest.raises(hip.EssHipError, match=msg):
            hip.event_ingest_store(*cols, starts, words, words, out, **{**ok, **change})
    with pytest.raises(hip.EssHipError, match='needs acc'):
        hip.event_ingest_store(*cols, starts, words, words, None, **ok)
    with pytest.raises(hip.EssHipError, match='out must be a non-empty fp32'):
        hip.event_ingest_store(*cols, starts, words, words, acc, **ok)
    with pytest.raises(hip.EssHipError, match=r'starts must be int64 \[2\]'):
        hip.event_ingest_store(*cols, words, words, words, out, **ok)
    for o, a in ((out, None), (None, acc)):
        with pytest.raises(hip.EssHipError, match='no CPU path'):  # (the last check: everything else about the call is fine)
            hip.event_ingest_store(*cols, starts, words, words, o, masks=masks, mask_size=(4, 5), mask_of=words, acc=a, **ok)
    counts, thr = torch.zeros(2, 4, 5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)

    def count(x=cols[1], y=cols[2], begins=starts, ends=starts, formats=words, counts=counts, total=20):
        return hip.event_store_pixel_counts(x, y, begins, ends, formats, counts, total)
    for kw, msg in ((dict(x=cols[1][:20]), r'x must be \[capacity\]'), (dict(y=cols[3]), 'y must be'), (dict(total=33), 'total=33'),
                    (dict(counts=counts.int()), 'counts must be a non-empty int64'), (dict(counts=counts[0]), 'counts must be a non-empty int64'),
                    (dict(begins=words), r'begins must be int64 \[2\]'), (dict(formats=starts), r'formats must be int32 \[2\]'),
                    (dict(x=None), 'x must be a CUDA'), (dict(), 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=msg):
            count(**kw)
    m2 = torch.zeros(2, 4, 1, dtype=torch.int32)
    for args, msg in (((counts.int(), thr, m2), 'counts must be a non-empty int64'), ((counts, thr[:1], m2), r'thresholds must be int64 \[2\]'),
                      ((counts, thr, masks), 'must hold 2 masks'), ((counts, thr, torch.zeros(2, 4, 2, dtype=torch.int32)), r'\[2, 4, 1\]'),
                      ((counts, thr, m2, 2), 'mode=2'), ((counts, thr, m2), 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=msg):
            hip.event_count_mask(*args)


# ---------------------------------------------------------------------------------------------- the class
def test_from_store_refuses_before_any_device_call_and_leaves_the_store_as_it_was():
    from ess_amd.datasets.event_store import EventStore
    from ess_amd.datasets.hot_pixels import HotPixelMask
    store = EventStore(1000)
    store._recs = [[0, 100, 1, 0, 99, 0, 0], [100, 160, 0, 0.5, 9.0, 0, 0]]  # (the bookkeeping alone)
    store.n_events = 160
    before = (store.n_events, [list(r) for r in store._recs])
    ok = dict(size=(8, 9), max_events_per_pixel=3)
    for args, kw, msg in (((object(), 0), ok, 'store must be an EventStore'), ((store, 2), ok, 'recording 2 of 2'),
                          ((store, -1), ok, 'recording -1 of 2'), ((store, True), ok, 'recording True'),
                          ((store, 0), dict(size=(8, 9)), 'exactly one of the two'),
                          ((store, 0), dict(size=(8, 9), max_events_per_pixel=3, max_rate_hz=2.0), 'exactly one of the two'),
                          ((store, 0), dict(size=(0, 9), max_events_per_pixel=3), r'size\[0\]=0'),
                          ((store, 0), dict(size=(8, 32769), max_events_per_pixel=3), r'size\[1\]=32769'),
                          ((store, 0), dict(size=8, max_events_per_pixel=3), r'must be \(h, w\)'),
                          ((store, 0), dict(size=(8, 9), max_events_per_pixel=-1), 'non-negative int'),
                          ((store, 0), dict(size=(8, 9), max_events_per_pixel=2.5), 'non-negative int'),
                          ((store, 0), dict(size=(8, 9), max_rate_hz=float('inf')), 'non-negative number'),
                          ((store, 1), dict(end=61, **ok), 'outside recording 1 of 60 events'),
                          ((store, 1), dict(begin=-1, **ok), 'outside recording 1'), ((store, 1), dict(begin=5, end=4, **ok), 'outside recording 1'),
                          ((store, 1), dict(begin=2.0, **ok), 'outside recording 1')):
        with pytest.raises(ValueError, match=msg):
            HotPixelMask.from_store(*args, **kw)
        assert store._dev is None and (store.n_events, [list(r) for r in store._recs]) == before, msg


# ---------------------------------------------------------------------------------------------- the restatement
def test_the_restated_count_rule_agrees_with_the_hot_pixel_restatement_where_they_overlap():
    g = np.random.default_rng(3)
    H, W, n = 7, 70, 5000
    x16, y16 = g.integers(-3, W + 3, n).astype(np.int16), g.integers(-3, H + 3, n).astype(np.int16)
    x16[:40], y16[:40] = 69, 6  # (one busy pixel in the last word's tail column)
    for xy_u16 in (False, True):
        xw, yw = (x16.view(np.uint16), y16.view(np.uint16)) if xy_u16 else (x16, y16)
        fmt = MR.XY_U16 if xy_u16 else 0
        got = MR.pixel_counts(xw, yw, 3, n - 2, fmt, n, H, W)
        # the same events by a direct loop over the decoded values (a negative int16 is 65533.. as uint16: outside either way)
        want = np.zeros((H, W), np.int64)
        for xv, yv in zip(x16[3:n - 2].astype(np.int64), y16[3:n - 2].astype(np.int64)):
            if 0 <= xv < W and 0 <= yv < H:
                want[yv, xv] += 1
        assert np.array_equal(got, want) and got.sum() < n - 5
        for bad in (dict(begin=-1), dict(end=n + 1), dict(begin=9, end=8), dict(fmt=4)):
            args = {**dict(begin=3, end=n - 2, fmt=fmt), **bad}
            assert not MR.pixel_counts(xw, yw, args['begin'], args['end'], args['fmt'], n, H, W).any(), bad
        assert not MR.pixel_counts(xw, yw, 8, 8, fmt, n, H, W).any()
        # the masks: plain counts against the histogram rule on the same counts at scale 2^40, split over the two planes
        counts = np.stack([got, got // 2])
        sums = np.stack([np.stack([c // 3, c - c // 3]) for c in counts]) << 40
        before = g.integers(0, 1 << 32, (2, H, MR.n_words(W)), dtype=np.uint64).astype(np.uint32)
        for thr in ([0, 1], [2, -1], [39, 40], [-5, 0]):
            for mode in (MR.REPLACE, MR.OR):
                a = MR.count_mask_words(counts, np.array(thr, np.int64), before, mode)
                b = HR.mask_words_of(sums, np.array(thr, np.int64), before, mode)
                assert np.array_equal(a, b), (thr, mode)
        assert (MR.count_mask_words(counts, np.array([39, 40], np.int64), before * 0, MR.REPLACE)[0] != 0).sum() == 1


# ---------------------------------------------------------------------------------------------- SequenceSegmenter(store=)
def test_the_store_fed_segmenter_refuses_before_the_models_reach_the_device():
    from types import SimpleNamespace
    import torch
    from ess_amd import hip
    from ess_amd.datasets.event_store import EventStore
    from ess_amd.datasets.hot_pixels import HotPixelMask
    from ess_amd.run_sequence_segmentation import SequenceSegmenter, _RecordingMasks
    encoder = SimpleNamespace(num_bins=5, to=lambda *a, **k: (_ for _ in ()).throw(AssertionError('the device was reached')))
    store = EventStore(1000, label_hw=(64, 96), label_capacity=2)
    m, other = HotPixelMask.from_locations([[1, 2]], 64, 96), HotPixelMask.from_locations([[1, 2]], 72, 104)
    ok = dict(n_streams=3, sequence_steps=5, window_events=256, store=store)
    for change, msg in ((dict(store=object()), 'store must be an EventStore'), (dict(device=torch.device('cuda:1')), 'where the store lies'),
                        (dict(ring_capacity=2048), 'has no rings'), (dict(hot_pixel_masks=[None] * 3), 'recording_hot_pixels='),
                        (dict(window_events=None), 'window_events is needed'), (dict(window_duration=5.0), 'not both'),
                        (dict(window_events=None, window_duration=5.0), 'needs window_capacity'),
                        (dict(window_capacity=255), 'window_capacity=255'), (dict(window_capacity=(1 << 22) + 1), 'window_capacity='),
                        (dict(window_events=None, window_duration=5.0, window_capacity=0), 'window_capacity=0'),
                        (dict(out_hw=(32, 48)), 'the store keeps labels of'), (dict(mask_slots=0), 'mask_slots=0'),
                        (dict(recording_hot_pixels=[m]), 'must be a dict'), (dict(recording_hot_pixels={0: other}), '72 x 104'),
                        (dict(recording_hot_pixels={-1: m}), 'recording -1'), (dict(recording_hot_pixels={0: object()}), 'HotPixelMask or None'),
                        (dict(recording_hot_pixels={0: m, 1: HotPixelMask.from_locations([[3, 4]], 64, 96)}, mask_slots=1), '2 distinct masks'),
                        (dict(rectify_maps=[None]), "voxel='trilinear'")):
        with pytest.raises(hip.EssHipError, match=msg):
            SequenceSegmenter(encoder, None, 64, 96, None, **{**ok, **change})
        assert store._dev is None, msg
    for kw in (dict(window_capacity=512), dict(recording_hot_pixels={0: m})):
        with pytest.raises(hip.EssHipError, match='they need store='):
            SequenceSegmenter(encoder, None, 64, 96, None, n_streams=3, sequence_steps=5, window_events=256, **kw)
    # the books of the mask slots, without a device: sharing by identity, and a refusal that changes nothing
    books = _RecordingMasks.__new__(_RecordingMasks)
    books.n_slots, books.size, books.held, books.slot_of = 2, (64, 96), [m, None], {4: 0}
    books.assign(7, m)
    assert books.slot_of == {4: 0, 7: 0} and books.word(7) == 0 and books.word(5) == hip.MASK_NONE
    books.held[1], books.slot_of[9] = other, 1
    with pytest.raises(hip.EssHipError, match='mask_slots=2'):
        books.assign(5, HotPixelMask.from_locations([[3, 4]], 64, 96))
    assert books.slot_of == {4: 0, 7: 0, 9: 1} and books.held == [m, other]
    books.assign(9, None)
    assert books.slot_of == {4: 0, 7: 0}


def test_the_lane_to_slot_transposition_restated():
    """event_store_windows writes slot b T + i (sample-major), the encoder reads slot i S + s (step-major): the round transposes the
    words, and a lane's mask word is repeated over its T windows -- on tests/event_store_ref.py's words for three lanes"""
    from tests import event_store_ref as SR
    S, T = 3, 4
    t = np.arange(64, dtype=np.int64)
    table = np.array([[0, 30, 1, 0], [30, 64, 1, 0]], dtype=np.int64)
    starts, counts, formats, flags = SR.windows(t, 64, table, [1, 0, -1], np.array([[20], [30], [0]]), SR.RULE_COUNT_INDEX, T, 3, 8)
    assert flags.tolist() == [0, 0, SR.FLAG_RANGE] and counts.tolist() == [3] * 8 + [0] * 4
    step_major = lambda w: np.asarray(w).reshape(S, T).T.reshape(-1)  # noqa: E731
    st, ct = step_major(starts), step_major(counts)
    for i in range(T):
        for s in range(S):
            assert st[i * S + s] == starts[s * T + i] and ct[i * S + s] == counts[s * T + i]
    assert st[:S].tolist() == [30 + 20 - 12, 30 - 12, 0] and st[S:2 * S].tolist() == [41, 21, 0]
    assert np.repeat(np.array([5, -1, 7])[None], T, axis=0).reshape(-1).tolist() == [5, -1, 7] * T
