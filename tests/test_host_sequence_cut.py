"""CPU tier of the sequence rounds (ess_amd/run_sequence_segmentation.py): the two host functions that cut a sequence out of a fed
stream -- datasets.event_feed.sequence_windows against a literal restatement of the DSEC loader's lines on index arrays, and
datasets.event_feed.ring_end_index against np.searchsorted on the unrolled event sequence -- and the host side of the scoring class
head's binding (ess_seg_head_eval: declared, exported, bound; what it refuses before a device is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_host_seg import ROOT, _dev, built_lib  # noqa: F401  (built_lib: the fixture)


# ---------------------------------------------------------------------------------------------- sequence_windows
def loader_cut(events, end, T, n_per_window):
    """DSEC/dataset/sequence.py:258-279 and :202-205 of the reference on an array of event indices, line for line:
    get_events_fixed_num(ts_end, nr_events) -> events[max(0, end - nr_events):end]; start_index 0 or -nr_events; nr_events_temp =
    loaded // nr_events_data; chunk i = events[i * temp:(i + 1) * temp]"""
    nr_events = T * n_per_window
    start_idx = end - nr_events
    if start_idx < 0:
        start_idx = 0
    data = events[start_idx:end]
    start_index = 0 if nr_events >= data.size else -nr_events
    t = data[start_index:]
    nr_events_temp = t.size // T
    return [t[i * nr_events_temp:(i + 1) * nr_events_temp] for i in range(T)], t


@pytest.mark.parametrize('T', [1, 5])
@pytest.mark.parametrize('N', [1, 4, 9])
def test_sequence_windows_against_the_loader(T, N):
    from ess_amd.datasets.event_feed import sequence_windows
    for loaded in sorted({0, T - 1, T, T + 1, T * N - 1, T * N, T * N + 7}):
        for base in (0, 13):  # (a recording that begins at index 0, and a ring whose oldest kept event is 13)
            end = base + loaded
            events_from_zero = np.arange(0, end + 50)
            chunks, t = loader_cut(events_from_zero[base:], end - base, T, N)
            got = sequence_windows(end, base, T, N)
            n = min(loaded, T * N) // T
            if n == 0:
                assert got is None, (T, N, loaded, base)
                assert all(c.size == 0 for c in chunks)
                continue
            assert got is not None and len(got) == T
            for (start, count), c in zip(got, chunks):
                assert count == n == c.size and np.array_equal(np.arange(start, start + count), c), (T, N, loaded, base)
            for (s0, c0), (s1, _) in zip(got, got[1:]):
                assert s0 + c0 == s1  # contiguous
            # the remainder that is dropped is the TAIL: the first window starts where the loaded span starts
            assert got[0][0] == max(base, end - T * N) == t[0]
            assert end - (got[-1][0] + got[-1][1]) == min(loaded, T * N) - T * n


def test_sequence_windows_refuses_nonsense():
    from ess_amd import hip
    from ess_amd.datasets.event_feed import sequence_windows
    for args in ((5, 6, 5, 4), (5, 0, 0, 4), (5, 0, 5, 0), (5, -1, 5, 4)):
        with pytest.raises(hip.EssHipError, match='sequence_windows'):
            sequence_windows(*args)


# ---------------------------------------------------------------------------------------------- ring_end_index
def _ring_of(seq, ring):
    t = np.zeros(ring, seq.dtype)
    for k, v in enumerate(seq):
        t[k % ring] = v
    return t


@pytest.mark.parametrize('dtype', [np.int64, np.float64])
@pytest.mark.parametrize('head', [11, 16, 32, 37], ids=['first_lap', 'exactly_full', 'at_a_wrap', 'past_a_wrap'])
def test_ring_end_index_against_searchsorted(dtype, head):
    from ess_amd import hip
    from ess_amd.datasets.event_feed import ring_end_index
    ring = 16
    g = np.random.default_rng(head)
    seq = np.sort(g.integers(100, 100 + head // 2, head)).astype(np.int64)  # (fewer values than events: ties, by counting)
    assert len(np.unique(seq)) < head
    seq = seq if dtype == np.int64 else seq.astype(np.float64) * 0.5
    t = _ring_of(seq, ring)
    oldest = max(0, head - ring)
    asked = 0
    for v in sorted(set(seq[oldest:].tolist())) + [seq[-1] + 1, seq[-1] + 1000]:
        for t_end in (v, v + (0.25 if dtype == np.float64 else 0)):
            want = int(np.searchsorted(seq, dtype(t_end), side='left'))
            if oldest > 0 and t_end <= seq[oldest]:
                with pytest.raises(hip.EssHipError, match='not after the oldest kept event'):
                    ring_end_index(t, head, ring, t_end)
                continue
            got = ring_end_index(t, head, ring, t_end)
            assert got == want, (dtype, head, t_end)
            assert got == head or seq[got] >= t_end
            assert got == 0 or seq[got - 1] < t_end  # (ties: the FIRST event of that time, as get_time_indices_offsets)
            asked += 1
    assert asked >= 4
    before = seq[oldest] - 1
    if oldest > 0:
        with pytest.raises(hip.EssHipError, match='not after the oldest kept event'):
            ring_end_index(t, head, ring, before)
    else:
        assert ring_end_index(t, head, ring, before) == 0  # (nothing was overwritten: the recording begins here)
    assert ring_end_index(t, head, ring, seq[-1] + 1) == head


def test_ring_end_index_refuses_a_sequence_that_reaches_behind_the_ring():
    from ess_amd import hip
    from ess_amd.datasets.event_feed import ring_end_index
    ring, head = 16, 40
    seq = np.arange(1000, 1000 + head, dtype=np.int64)
    t = _ring_of(seq, ring)
    assert ring_end_index(t, head, ring, 1000 + 36, need=12) == 36  # events 24..35: all kept
    with pytest.raises(hip.EssHipError, match='reach back to event 23'):
        ring_end_index(t, head, ring, 1000 + 36, need=13)
    assert ring_end_index(_ring_of(seq[:10], ring), 10, ring, 1005, need=12) == 5  # (the stream has no more: the loader's clamp at 0)
    assert ring_end_index(t, head, ring, 1035.5) == 36  # a fractional time against integer times
    for bad in (t[:8], t.astype(np.float32), t.reshape(4, 4)):
        with pytest.raises(hip.EssHipError, match='t_ring must be'):
            ring_end_index(bad, head, ring, 1030)
    with pytest.raises(hip.EssHipError, match='NaN'):
        ring_end_index(t.astype(np.float64), head, ring, float('nan'))


# ---------------------------------------------------------------------------------------------- the scoring head's binding
def test_seg_head_eval_symbol_is_declared_exported_and_bound(built_lib):
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    assert re.search(r'\bint\s+ess_seg_head_eval\s*\(', header)
    assert hasattr(ctypes.CDLL(built_lib), 'ess_seg_head_eval')
    from ess_amd import hip
    assert 'ess_seg_head_eval' in hip.EXPORTS
    assert len(hip.lib().ess_seg_head_eval.argtypes) == 23 and len(hip.lib().ess_seg_head.argtypes) == 20
    assert hip.lib().ess_version() == 110  # (purely additive)


def test_seg_head_eval_library_refuses_bad_arguments(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced)

    def call(gt=one, conf=one, ign=255, N=1, C=32, K=11, lab=one):
        return L.ess_seg_head_eval(one, 0, one, one, P(0), lab, P(0), P(0), gt, conf, ign, N, C, K, 4, 6, 0, 0, 4, 6, 4, 6, P(0))
    for kw, msg in ((dict(gt=P(0)), 'confusion needs gt'), (dict(conf=P(0)), 'gt needs confusion'), (dict(K=65), 'K=65'),
                    (dict(lab=P(0)), 'labels'), (dict(N=65536), 'N=65536'),
                    # K = 64 (KM = 64), C = 184: 64 * 184 * 4 + 64 * 4 + 192 = 47 552 bytes of weights fit, + 64 * 64 * 4 = 16 384 of counts
                    # = 63 936 still fit; C = 192: 49 600 + 16 384 = 65 984 > 65 536 do not, while ess_seg_head takes them
                    (dict(K=64, C=192), 'K x K counts')):
        assert call(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
    assert L.ess_seg_head(one, 0, one, one, P(0), P(0), P(0), P(0), 1, 192, 64, 4, 6, 0, 0, 4, 6, 4, 6, P(0)) == -22
    assert 'labels' in L.ess_last_error().decode()  # (the plain head stops at its labels, not at LDS: K = 64 x C = 192 fit there)


def test_seg_head_eval_refuses_on_the_host(built_lib):
    from ess_amd import hip
    C, K = 32, 11
    xd = _dev(torch.zeros(2, C, 4, 6))
    w, b = torch.zeros(K, C), torch.zeros(K)
    gt, cm = _dev(torch.zeros(2, 4, 6, dtype=torch.uint8)), _dev(torch.zeros(2, K, K, dtype=torch.int64))
    with pytest.raises(hip.EssHipError, match=r'seg_head_eval: x .*no CPU path'):
        hip.seg_head_eval(torch.zeros(2, C, 4, 6), C, w, b, gt, cm)
    with pytest.raises(hip.EssHipError, match='gt and confusion come together'):
        hip.seg_head_eval(xd, C, w, b, gt, None)
    with pytest.raises(hip.EssHipError, match='gt and confusion come together'):
        hip.seg_head_eval(xd, C, w, b, None, cm)
    for bad in (gt.long(), _dev(torch.zeros(2, 4, 7, dtype=torch.uint8)), _dev(torch.zeros(1, 4, 6, dtype=torch.uint8)),
                torch.zeros(2, 4, 6, dtype=torch.uint8), _dev(torch.zeros(2, 6, 4, dtype=torch.uint8)).transpose(1, 2)):
        with pytest.raises(hip.EssHipError, match=r'seg_head_eval: gt must be a contiguous torch.uint8 \[2, 4, 6\]'):
            hip.seg_head_eval(xd, C, w, b, bad, cm)
    for bad in (cm.int(), _dev(torch.zeros(K, K, dtype=torch.int64)), _dev(torch.zeros(2, K, K + 1, dtype=torch.int64)),
                torch.zeros(2, K, K, dtype=torch.int64)):
        with pytest.raises(hip.EssHipError, match=r'seg_head_eval: confusion must be a contiguous torch.int64 \[2, 11, 11\]'):
            hip.seg_head_eval(xd, C, w, b, gt, bad)
    with pytest.raises(hip.EssHipError, match=r'seg_head_eval: gt must be .* \[2, 3, 5\]'):  # (the OUTPUT size, not the source's)
        hip.seg_head_eval(xd, C, w, b, gt, cm, out_hw=(3, 5))
    with pytest.raises(hip.EssHipError, match=r'seg_head_eval: weight must be \[K, C=32\]'):  # (seg_head's checks, under its own name)
        hip.seg_head_eval(xd, C, torch.zeros(K, C + 8), b, gt, cm)
    from ess_amd.models.style_networks import SemSegE2VID
    with pytest.raises(hip.EssHipError, match='gt and confusion come together'):
        SemSegE2VID.predict(None, {}, gt=gt)


def test_sequence_module_imports_without_a_gpu_and_refuses_bad_arguments():
    from ess_amd import hip
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    assert callable(SequenceSegmenter.segment_at) and callable(SequenceSegmenter.from_checkpoints)
    doc = SequenceSegmenter.__doc__
    assert '0.9 GB + 1.8 GB' in doc and 'fixed_duration' in doc
    for kw, match in ((dict(n_streams=0, sequence_steps=5, window_events=256), 'n_streams=0'),
                      (dict(n_streams=3, sequence_steps=0, window_events=256), 'sequence_steps=0'),
                      (dict(n_streams=3, sequence_steps=5), 'window_events is needed'),
                      (dict(n_streams=3, sequence_steps=5, window_events=256, voxel='bilinear'), "voxel='bilinear'"),
                      (dict(n_streams=3, sequence_steps=5, window_events=256, ring_capacity=5 * 256 - 1), 'ring_capacity=1279'),
                      (dict(n_streams=3, sequence_steps=5, window_events=256, ring_capacity=(1 << 22) + 1), 'ring_capacity='),
                      (dict(n_streams=3, sequence_steps=5, window_events=256, ignore_index=256), 'ignore_index=256')):
        with pytest.raises(hip.EssHipError, match=match):
            SequenceSegmenter(None, None, 64, 96, None, **kw)
