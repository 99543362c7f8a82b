"""CPU tier of the hot-pixel masks (hip.event_ingest_masked, hip.event_hot_pixel_mask, datasets.hot_pixels.HotPixelMask,
hot_pixel_masks= of the segmenters): the two C entry points and their refusals, the wrappers' and the classes' refusals -- each raised
before a device call --, the mask's bit layout against np.packbits, and the integer restatement (tests/hot_pixel_ref.py) that the GPU
tier compares against, checked here on hand-made cases."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import hot_pixel_ref as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_event_ingest_masked', 'ess_event_hot_pixel_mask')
EINVAL = -22
WIDTHS = [1, 31, 32, 33, 64, 70]


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_two_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert 'ESS_MASK_NONE = -1' in header and 'ESS_MASK_REPLACE = 0, ESS_MASK_OR = 1' in header
    assert (hip.MASK_NONE, hip.MASK_REPLACE, hip.MASK_OR) == (-1, 0, 1)
    assert callable(hip.event_ingest_masked) and callable(hip.event_hot_pixel_mask)


# ---------------------------------------------------------------------------------------------- HotPixelMask
@pytest.mark.parametrize('width', WIDTHS)
def test_the_packing_is_numpy_packbits_little(width):
    from ess_amd.datasets.hot_pixels import HotPixelMask
    H = 5
    b = np.random.default_rng(width).random((H, width)) < 0.4
    b[0, 0] = b[H - 1, width - 1] = True
    m = HotPixelMask.from_bool(b)
    padded = np.zeros((H, HP.n_words(width) * 32), dtype=bool)
    padded[:, :width] = b
    want = np.packbits(padded, axis=1, bitorder='little').view(np.uint32)
    assert m.words.dtype == np.uint32 and m.words.shape == (H, HP.n_words(width)) and np.array_equal(m.words, want)
    assert np.array_equal(m.to_bool(), b) and m.count() == int(b.sum()) and (m.height, m.width) == (H, width)
    ys, xs = np.nonzero(b)
    assert np.array_equal(m.words, HP.words_of_locations(zip(xs.tolist(), ys.tolist()), H, width))
    assert not m.words.flags.writeable


def test_locations_text_file_round_trip(tmp_path):
    from ess_amd.datasets.hot_pixels import HotPixelMask
    H, W = 7, 70
    xy = np.array([[69, 6], [0, 0], [31, 2], [32, 2], [63, 5], [64, 5], [0, 0]])  # (unsorted, one pixel twice)
    m = HotPixelMask.from_locations(xy, H, W)
    loc = m.to_locations()
    assert loc.tolist() == [[0, 0], [31, 2], [32, 2], [63, 5], [64, 5], [69, 6]] and m.count() == 6  # sorted by (y, x)
    path = tmp_path / 'hot_pixels.txt'
    np.savetxt(path, loc, fmt='%d', delimiter=',')
    assert open(path).read().splitlines()[0] == '0,0'
    assert np.loadtxt(path, delimiter=',').shape == (6, 2)  # (what the reference's EventPreprocessor reads)
    back = HotPixelMask.from_file(path, H, W)
    assert back == m and np.array_equal(back.words, m.words)
    one = tmp_path / 'one.txt'
    np.savetxt(one, loc[:1], fmt='%d', delimiter=',')
    assert HotPixelMask.from_file(one, H, W).to_locations().tolist() == [[0, 0]]
    empty = tmp_path / 'empty.txt'
    empty.write_text('')
    assert HotPixelMask.from_file(empty, H, W).count() == 0 and HotPixelMask.from_locations(np.zeros((0, 2), int), H, W).count() == 0


def test_the_mask_refuses_what_lies_outside_the_sensor_and_wrong_shapes():
    from ess_amd.datasets.hot_pixels import HotPixelMask
    for xy in ([[70, 0]], [[0, 7]], [[-1, 0]], [[0, -1]], [[3, 3], [69, 7]]):
        with pytest.raises(ValueError, match='outside the 7 x 70 sensor'):
            HotPixelMask.from_locations(np.array(xy), 7, 70)
    with pytest.raises(ValueError, match=r'\[N, 2\]'):
        HotPixelMask.from_locations(np.zeros((3, 3), int), 7, 70)
    with pytest.raises(ValueError, match='whole numbers'):
        HotPixelMask.from_locations(np.array([[0.5, 1.0]]), 7, 70)
    with pytest.raises(ValueError, match=r'bool \[H, W\]'):
        HotPixelMask.from_bool(np.zeros((7, 70), np.uint8))
    with pytest.raises(ValueError, match=r'bool \[H, W\]'):
        HotPixelMask.from_bool(np.zeros((7,), bool))
    with pytest.raises(ValueError, match='height='):
        HotPixelMask.from_locations(np.zeros((0, 2), int), 0, 70)
    with pytest.raises(ValueError, match='width='):
        HotPixelMask.from_locations(np.zeros((0, 2), int), 7, 40000)
    with pytest.raises(ValueError, match=r'uint32 \[7, 3\]'):
        HotPixelMask.from_words(np.zeros((7, 2), np.uint32), 7, 70)
    bad = np.zeros((7, 3), np.uint32)
    bad[2, 2] = 1 << 6  # x = 70
    with pytest.raises(ValueError, match='x >= width=70'):
        HotPixelMask.from_words(bad, 7, 70)


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_the_restatement_of_the_masking_rule_by_hand():
    words = HP.words_of_locations([(0, 0), (31, 1), (32, 1), (69, 6)], 7, 70)
    assert words[1].tolist() == [1 << 31, 1, 0] and words[6].tolist() == [0, 0, 1 << 5]
    x = np.array([0, 31, 32, 69, 69, 33, -1, 0, 70, 0], dtype=np.int16)
    y = np.array([0, 1, 1, 6, 5, 1, 0, -1, 6, 7], dtype=np.int16)
    cols = SimpleNamespace(t=np.arange(10.0), x=x, y=y, p=np.ones(10, np.uint8))
    hot = HP.masked(cols, words, 7, 70)
    assert hot.tolist() == [True, True, True, True, False, False, False, False, False, False]
    assert not HP.masked(cols, None, 7, 70).any()
    _, moved, _, _ = HP.moved_away(cols, hot)
    assert moved.dtype == np.int16 and moved.tolist() == [-1, -1, -1, -1, 69, 33, -1, 0, 70, 0] and x[0] == 0
    u = SimpleNamespace(t=cols.t, x=x.view(np.uint16), y=y.view(np.uint16), p=cols.p)
    hot_u = HP.masked(u, words, 7, 70)  # (65535 is no pixel of the mask)
    assert hot_u.tolist() == hot.tolist()
    assert HP.moved_away(u, hot_u)[1].tolist()[:4] == [65535] * 4


def test_the_restatement_of_the_threshold_rule_by_hand():
    one = 1 << 40
    sums = np.zeros((3, 2, 1, 33), dtype=np.int64)
    sums[0, 0, 0, 0] = one                      # 1 event > 0: hot
    sums[1, 0, 0, 1], sums[1, 1, 0, 1] = one, one          # 2 events, threshold 2: AT it, not hot
    sums[1, 0, 0, 32], sums[1, 1, 0, 32] = one, 2 * one    # 3 events: hot (both polarities count together)
    sums[2, 0, 0, 5] = 9 * one
    before = np.full((3, 1, 2), 0xFFFFFFFF, dtype=np.uint32)
    got = HP.mask_words_of(sums, np.array([0, 2, -1]), before, HP.REPLACE)
    assert got[0, 0].tolist() == [1, 0] and got[1, 0].tolist() == [0, 1] and got[2, 0].tolist() == [0xFFFFFFFF] * 2
    pattern = np.full((3, 1, 2), 0x80000002, dtype=np.uint32)
    got = HP.mask_words_of(sums, np.array([0, 2, -1]), pattern, HP.OR)
    assert got[0, 0].tolist() == [0x80000003, 0x80000002] and got[1, 0].tolist() == [0x80000002, 0x80000003]
    assert got[2, 0].tolist() == [0x80000002] * 2


# ---------------------------------------------------------------------------------------------- the library
def test_the_library_refuses_in_front_of_any_launch(built_lib):
    """ESS_EINVAL with a message that names the argument; the pointers are never followed (no GPU is needed): any aligned address does"""
    from ess_amd import hip
    L = hip.lib()
    P, A = ctypes.c_void_p, 0x10000

    def ingest(rows=A, starts=A, ring=64, channels=4, rep=1, trilinear=0, out=A, acc=A, acc_bytes=None, maps=0, map_of=A, n_maps=0, map_hw=(1, 1),
               masks=A, mask_of=A, n_masks=2, mask_hw=(7, 70)):
        nbytes = 2 * max(channels, 1) * 6 * 8 * 8 if acc_bytes is None else acc_bytes
        return L.ess_event_ingest_masked(P(A), P(A), P(A), P(A), P(rows), P(starts), P(A), P(A), ring, 1, 2, channels, 6, 8, P(acc), nbytes,
                                         P(out), rep, trilinear, P(maps), P(map_of), n_maps, *map_hw, P(masks), P(mask_of), n_masks, *mask_hw,
                                         None)
    err = L.ess_last_error
    assert ingest(masks=0, n_masks=2) == EINVAL and b'masks must be null with n_masks=0 and only then' in err()
    assert ingest(masks=A, n_masks=0) == EINVAL and b'masks must be null with n_masks=0 and only then' in err()
    assert ingest(n_masks=-1) == EINVAL and b'n_masks=-1' in err()
    assert ingest(mask_of=0) == EINVAL and b'null mask_of' in err()
    assert ingest(masks=A + 4) == EINVAL and b'masks must be 16-byte aligned' in err()
    for hw in ((0, 70), (7, 0), (32769, 70), (7, 32769), (-1, 70)):
        assert ingest(mask_hw=hw) == EINVAL and b'mask_height=' in err() and b'1..32768' in err()
    for rep in (1, 2):
        assert ingest(trilinear=1, rep=rep, channels=2) == EINVAL and b'trilinear=1' in err() and b'representation=' in err()
    assert ingest(trilinear=2, rep=0) == EINVAL and b'trilinear=2' in err()
    assert ingest(rows=0) == EINVAL and b'rows null, starts given' in err()
    assert ingest(starts=0) == EINVAL and b'rows given, starts null' in err()
    assert ingest(rep=3) == EINVAL and b'representation=3' in err()
    assert ingest(channels=5) == EINVAL and b'must be even' in err()
    assert ingest(rep=2) == EINVAL and b'channels=4 must be 2' in err()
    # the source's own checks hold as they stand, for the ring and for the column source (rows == starts == NULL)
    for src in (dict(), dict(rows=0, starts=0)):
        assert ingest(ring=24, **src) == EINVAL and b'multiple of 16' in err()
        assert ingest(ring=(1 << 22) + 16, **src) == EINVAL and (b'ring=' in err() or b'stride=' in err())
        assert ingest(acc_bytes=2 * 4 * 6 * 8 * 8 - 8, **src) == EINVAL and b'acc has' in err()
        assert ingest(acc=0, **src) == EINVAL and b'null' in err()
        assert ingest(out=A + 4, **src) == EINVAL and b'16-byte aligned' in err()
    # trilinear = 1 reads the rectify arguments, trilinear = 0 does not
    assert ingest(trilinear=1, rep=0, map_of=0) == EINVAL and b'null map_of' in err()
    assert ingest(trilinear=1, rep=0, maps=A, n_maps=0) == EINVAL and b'maps must be null' in err()
    assert ingest(trilinear=1, rep=0, map_hw=(0, 1)) == EINVAL and b'map_height=' in err()

    def mask(sums=A, n=3, hw=(3, 70), thr=A, masks=A, mode=0):
        return L.ess_event_hot_pixel_mask(P(sums), n, *hw, P(thr), P(masks), mode, None)
    for mode in (2, -1, 1 << 20):
        assert mask(mode=mode) == EINVAL and f'mode={mode}'.encode() in err()
    for kw in (dict(sums=0), dict(thr=0), dict(masks=0)):
        assert mask(**kw) == EINVAL and b'null' in err()
    for hw in ((0, 70), (3, 0), (32769, 70), (3, 32769)):
        assert mask(hw=hw) == EINVAL and b'height=' in err() and b'1..32768' in err()
    for n in (0, -1, 65536):
        assert mask(n=n) == EINVAL and f'n={n}'.encode() in err()
    assert mask(masks=A + 4) == EINVAL and b'aligned' in err()
    assert mask(sums=A + 8) == EINVAL and b'aligned' in err()
    assert mask(thr=A + 4) == EINVAL and b'aligned' in err()


# ---------------------------------------------------------------------------------------------- the wrappers
def _host_call(S=2, C=4, H=6, W=8, ring=32, mh=7, mw=70):
    z = lambda *s, d=torch.int32: torch.zeros(*s, dtype=d)  # noqa: E731
    return dict(t=z(S, ring, d=torch.int64), x=z(S, ring, d=torch.int16), y=z(S, ring, d=torch.int16), p=z(S, ring, d=torch.uint8),
                rows=z(S), starts=z(S), counts=z(S), formats=z(S), out=z(S, C, H, W, d=torch.float32), acc=z(S, C, H, W, d=torch.int64),
                masks=z(2, mh, HP.n_words(mw)), mask_of=z(S), mask_size=(mh, mw))


INGEST_REFUSALS = [
    (dict(representation=3), 'representation=3'),
    (dict(representation=True), 'representation=True'),
    (dict(representation=2), 'EVENT_REP_HISTOGRAM fills 2 planes'),
    (dict(trilinear=True), 'trilinear=True builds the signed grid alone'),
    (dict(trilinear=2, representation=0), 'trilinear=2'),
    (dict(representation=0, maps=torch.zeros(1, 7, 70, 2)), 'trilinear flavour alone'),
    (dict(rows=None), 'rows and starts are both'),
    (dict(starts=None), 'rows and starts are both'),
    (dict(out=None, acc=None), 'out=None .* needs acc'),
    (dict(out=None, acc=torch.zeros(2 * 4 * 6 * 8, dtype=torch.int64)), 'acc must be a non-empty int64'),
    (dict(masks=torch.zeros(2, 7, 2, dtype=torch.int32)), r'masks must be a non-empty int32 / uint32 \[n_masks, 7, 3\]'),
    (dict(masks=torch.zeros(2, 6, 3, dtype=torch.int32)), 'masks must be'),
    (dict(masks=torch.zeros(2, 7, 3, dtype=torch.int64)), 'masks must be'),
    (dict(masks=np.zeros((2, 7, 3), np.uint32)), 'masks must be'),
    (dict(mask_size=None), 'mask_size=None'),
    (dict(mask_size=(7, 40000)), 'mask_size='),
    (dict(mask_size=(0, 70)), 'mask_size='),
    (dict(masks=None), 'mask_size=.*without masks'),
    (dict(mask_of=torch.zeros(3, dtype=torch.int32)), r'mask_of must be int32 \[2\]'),
    (dict(mask_of=torch.zeros(2, dtype=torch.int64)), 'mask_of must be int32'),
    (dict(t=torch.zeros(2, 32, dtype=torch.int32)), 't must be'),
    (dict(counts=torch.zeros(3, dtype=torch.int32)), 'counts must be int32'),
    (dict(rows=torch.zeros(2, dtype=torch.int64)), 'rows must be int32'),
    (dict(out=torch.zeros(2, 4, 6, 8, dtype=torch.float64)), 'out must be a non-empty fp32'),
    (dict(t=np.zeros((2, 32))), 'must be a CUDA'),
]


def test_wrapper_refusals_come_before_a_pointer_is_taken(monkeypatch):
    """CPU tensors reach every check of form; the last check is the device's, so the library is never loaded"""
    from ess_amd import hip
    monkeypatch.setattr(hip, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was reached')))

    def call(representation=1, trilinear=False, maps=None, map_of=None, **kw):
        a = {**_host_call(), **kw}
        return hip.event_ingest_masked(a['t'], a['x'], a['y'], a['p'], a['rows'], a['starts'], a['counts'], a['formats'], a['out'], a['masks'],
                                       a['mask_of'], a['mask_size'], representation=representation, trilinear=trilinear, maps=maps,
                                       map_of=map_of, acc=a['acc'])
    for kw, match in INGEST_REFUSALS:
        with pytest.raises(hip.EssHipError, match=match):
            call(**kw)
    with pytest.raises(hip.EssHipError, match='multiple of 16'):
        call(**{k: torch.zeros(2, 24, dtype=d) for k, d in zip('txyp', (torch.int64, torch.int16, torch.int16, torch.uint8))})
    for kw in (dict(), dict(rows=None, starts=None), dict(out=None), dict(masks=None, mask_size=None, mask_of=None)):
        with pytest.raises(hip.EssHipError, match='no CPU path'):  # nothing wrong with the form: the device check is what is left
            call(**kw)

    def mask(mode=hip.MASK_REPLACE, **kw):
        a = {**dict(sums=torch.zeros(3, 2, 3, 70, dtype=torch.int64), thresholds=torch.zeros(3, dtype=torch.int64),
                    masks=torch.zeros(3, 3, 3, dtype=torch.int32)), **kw}
        return hip.event_hot_pixel_mask(a['sums'], a['thresholds'], a['masks'], mode)
    for kw, match in ((dict(mode=2), 'mode=2'), (dict(mode=True), 'mode=True'), (dict(mode='or'), "mode='or'"),
                      (dict(sums=torch.zeros(3, 3, 3, 70, dtype=torch.int64)), r'sums must be a non-empty int64 \[n, 2, H, W\]'),
                      (dict(sums=torch.zeros(3, 2, 3, 70, dtype=torch.float32)), 'sums must be'),
                      (dict(thresholds=torch.zeros(3, dtype=torch.int32)), r'thresholds must be int64 \[3\]'),
                      (dict(thresholds=torch.zeros(2, dtype=torch.int64)), 'thresholds must be int64'),
                      (dict(masks=torch.zeros(3, 3, 2, dtype=torch.int32)), r'masks must be .*\[3, 3, 3\]'),
                      (dict(masks=torch.zeros(2, 3, 3, dtype=torch.int32)), 'masks must hold 3 masks'),
                      (dict(sums=np.zeros((3, 2, 3, 70), np.int64)), 'must be a CUDA')):
        with pytest.raises(hip.EssHipError, match=match):
            mask(**kw)
    with pytest.raises(hip.EssHipError, match='no CPU path'):
        mask()


# ---------------------------------------------------------------------------------------------- the segmenters
def _encoder(num_bins=5):
    return SimpleNamespace(num_bins=num_bins, to=lambda *a, **k: (_ for _ in ()).throw(AssertionError('the device was reached')))


def test_the_segmenters_refuse_before_the_models_reach_the_device():
    from ess_amd import hip
    from ess_amd.datasets.hot_pixels import HotPixelMask
    from ess_amd.run_segmentation import MultiStreamSegmenter
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    m = HotPixelMask.from_locations([[1, 2]], 64, 96)
    other = HotPixelMask.from_locations([[1, 2]], 72, 104)
    multi = lambda masks, **kw: MultiStreamSegmenter(_encoder(), None, 64, 96, None, 3, hot_pixel_masks=masks, **kw)  # noqa: E731
    seq = lambda masks: SequenceSegmenter(_encoder(), None, 64, 96, None, n_streams=3, sequence_steps=2, window_events=256,  # noqa: E731
                                          hot_pixel_masks=masks)
    for layout in ('columns', 'ring'):
        kw = dict(event_capacity=256, event_layout=layout)
        for bad in ([m, None], [m] * 4, m, (m for _ in range(3))):
            with pytest.raises(hip.EssHipError, match='one entry per stream'):
                multi(bad, **kw)
        with pytest.raises(hip.EssHipError, match=r'hot_pixel_masks\[1\] must be a datasets.hot_pixels.HotPixelMask'):
            multi([None, np.zeros((64, 96), bool), None], **kw)
        with pytest.raises(hip.EssHipError, match='one call reads masks of one sensor size'):
            multi([m, None, other], **kw)
    for bad in ([m, None], [m] * 4, m):
        with pytest.raises(hip.EssHipError, match='one entry per stream'):
            seq(bad)
    with pytest.raises(hip.EssHipError, match='one sensor size'):
        seq([other, m, None])
    # the record layout, and no event source at all: refused with the reason
    for kw in (dict(), dict(event_capacity=256), dict(event_capacity=256, event_layout='records'), dict(event_layout='columns')):
        with pytest.raises(hip.EssHipError, match="raw events.*event_capacity=N and event_layout='columns' or 'ring'"):
            multi([m, None, m], **kw)


def test_the_mask_slots_refuse_a_mask_of_another_size_and_share_equal_objects(monkeypatch):
    """_HotPixelSlots on the CPU (the buffer is a plain tensor there): the books set_hot_pixels keeps"""
    from ess_amd import hip
    from ess_amd.datasets.hot_pixels import HotPixelMask
    from ess_amd.run_segmentation import MultiStreamSegmenter, _HotPixelSlots
    m0, m1 = HotPixelMask.from_locations([[0, 0], [69, 6]], 7, 70), HotPixelMask.from_locations([[32, 1]], 7, 70)
    hot = _HotPixelSlots([m0, None, m0], 3, (5, 70), torch.device('cpu'))
    assert hot.size == (7, 70) and hot.mask_of == [0, hip.MASK_NONE, 0] and tuple(hot.words.shape) == (3, 7, 3)
    assert np.array_equal(hot.words[0].numpy().view(np.uint32), m0.words) and not bool(hot.words[1:].any())
    seg = SimpleNamespace(_hot=hot, n_streams=3, _hot_slots=lambda what: hot)
    with pytest.raises(hip.EssHipError, match='is 5 x 70, the masks of this segmenter 7 x 70'):
        MultiStreamSegmenter.set_hot_pixels(seg, 1, HotPixelMask.from_locations([[0, 0]], 5, 70))
    with pytest.raises(hip.EssHipError, match='must be a datasets.hot_pixels.HotPixelMask'):
        MultiStreamSegmenter.set_hot_pixels(seg, 1, np.zeros((7, 70), bool))
    with pytest.raises(hip.EssHipError, match='stream 3 of n_streams=3'):
        MultiStreamSegmenter.set_hot_pixels(seg, 3, m1)
    assert hot.mask_of == [0, hip.MASK_NONE, 0]
    MultiStreamSegmenter.set_hot_pixels(seg, 1, m1)
    assert hot.mask_of == [0, 1, 0] and np.array_equal(hot.words[1].numpy().view(np.uint32), m1.words)
    MultiStreamSegmenter.set_hot_pixels(seg, 0, None)
    MultiStreamSegmenter.set_hot_pixels(seg, 2, m1)
    assert hot.mask_of == [hip.MASK_NONE, 1, 1]
    k = hot.own_slot(2, keep=True)  # (a calibration in 'or' mode: stream 2 gets a slot of its own, with m1's bits)
    assert k != 1 and hot.mask_of == [hip.MASK_NONE, 1, k] and torch.equal(hot.words[k], hot.words[1])
    assert _HotPixelSlots([None] * 3, 3, (5, 70), torch.device('cpu')).size == (5, 70)
    built_without = SimpleNamespace(_hot=None)
    with pytest.raises(hip.EssHipError, match='built without hot_pixel_masks'):
        MultiStreamSegmenter._hot_slots(built_without, 'set_hot_pixels')
