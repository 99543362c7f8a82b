"""CPU tier of the training batches from events (ess_amd/datasets/event_batches.py, hip.event_grid_finish_window, hip.label_window):
the host draw of the window rows, and every refusal of the builder and of the two wrappers -- each raised before any device call: the
builder allocates nothing before its first accepted batch and the wrappers check before they take a pointer, so CPU tensors reach the
checks and neither a GPU nor the built library is needed; and the library's own refusals of a bad window (ESS_EINVAL with a message, in
front of any launch), which need the built library and no GPU."""
import numpy as np
import pytest
import torch

from ess_amd import hip
from ess_amd.datasets import event_batches as EB
from ess_amd.datasets.data_util import EventColumns


# ------------------------------------------------------------------------------------------------------------------ the draw
def test_draw_ranges_flips_and_both_ends_of_x0():
    p = EB.draw_window_params(4096, (200, 352), (120, 216), band=(60, 130), generator=torch.Generator().manual_seed(1))
    assert p.dtype == torch.int32 and tuple(p.shape) == (4096, 4) and not p.is_cuda
    assert set(p[:, 0].tolist()) == {0, 1} and not bool(p[:, 3].any())
    assert int(p[:, 1].min()) == 60 and int(p[:, 1].max()) == 70  # the band: rows [60, 190), a window of 120
    assert int(p[:, 2].min()) == 0 and int(p[:, 2].max()) == 352 - 216
    assert 0.45 < float(p[:, 0].float().mean()) < 0.55


def test_draw_respects_the_ddd17_band_and_the_seed():
    g = lambda: torch.Generator().manual_seed(7)  # noqa: E731
    p = EB.draw_window_params(256, (200, 352), (120, 216), band=(80, 120), generator=g())
    assert bool((p[:, 1] == 80).all()) and len(set(p[:, 2].tolist())) > 50
    assert torch.equal(p, EB.draw_window_params(256, (200, 352), (120, 216), band=(80, 120), generator=g()))
    assert not torch.equal(p, EB.draw_window_params(256, (200, 352), (120, 216), band=(80, 120), generator=torch.Generator().manual_seed(8)))
    flips = EB.draw_window_params(256, (448, 640), (448, 640), generator=g())  # DSEC: the flip alone
    assert set(flips[:, 0].tolist()) == {0, 1} and not bool(flips[:, 1:].any())


def test_draw_without_augmentation_is_all_zero():
    p = EB.draw_window_params(5, (24, 32), (24, 32), augment=False)
    assert tuple(p.shape) == (5, 4) and not bool(p.any())
    with pytest.raises(hip.EssHipError, match='must equal grid_hw'):
        EB.draw_window_params(5, (24, 32), (12, 32), augment=False)


@pytest.mark.parametrize('kw,message', [
    (dict(win_hw=(25, 32)), 'does not fit'),
    (dict(win_hw=(12, 33)), 'does not fit'),
    (dict(win_hw=(12, 20), band=(8, 11)), 'no window fits the band'),
    (dict(win_hw=(12, 20), band=(14, 12)), 'band='),
    (dict(win_hw=(12, 20), band=(-1, 12)), 'band='),
    (dict(win_hw=(0, 20)), 'positive ints'),
])
def test_draw_refuses(kw, message):
    with pytest.raises(hip.EssHipError, match=message):
        EB.draw_window_params(4, (24, 32), **kw)


# ------------------------------------------------------------------------------------------------------------------ the builder
GEO = dict(batch_size=2, sequence_steps=3, bins=3, event_capacity=64, grid_hw=(26, 34), grid_resize=(26, 36), height=20, width=36,
           label_hw=(20, 34), crop_hw=(12, 20), crop_band=(8, 12))


def _cols(n, seed=0, t_dtype=np.float64):
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0, 1, n)) if t_dtype == np.float64 else np.sort(g.integers(0, 10 ** 6, n)).astype(np.int64)
    return EventColumns(t, g.integers(0, 34, n).astype(np.int16), g.integers(0, 26, n).astype(np.int16), g.integers(0, 2, n).astype(np.uint8))


def _label(hw=(20, 34), dtype=np.uint8):
    return np.zeros(hw, dtype)


@pytest.fixture()
def no_device(monkeypatch):
    """any allocation or launch of the builder fails the test"""
    def boom(*a, **k):
        raise AssertionError('a device call was reached')
    monkeypatch.setattr(EB.EventBatchBuilder, '_allocate', boom)
    monkeypatch.setattr(EB.EventBatchBuilder, '_launch', boom)


BAD_BATCHES = [
    ('one sample short', lambda: [(_cols(10), _label())], None, 'batch_size=2'),
    ('not a list', lambda: 5, None, 'batch_size=2'),
    ('rows in place of columns', lambda: [(np.zeros((4, 4)), _label()), (_cols(10), _label())], None, r'samples\[0\] must be'),
    ('label dtype', lambda: [(_cols(10), _label(dtype=np.int64)), (_cols(10), _label())], None, r'samples\[0\]: the label'),
    ('label shape', lambda: [(_cols(10), _label()), (_cols(10), _label((20, 36)))], None, r'samples\[1\]: the label'),
    ('labels for some', lambda: [(_cols(10), _label()), (_cols(10), None)], None, 'for none'),
    ('too many events', lambda: [(_cols(10), _label()), (_cols(65), _label())], None, 'event_capacity=64'),
    ('a map index without maps', lambda: [(_cols(10), _label(), 0), (_cols(10), _label())], None, 'map index'),
    ('params shape', lambda: [(_cols(10), _label())] * 2, torch.zeros(3, 4, dtype=torch.int32), 'params must be'),
    ('params dtype', lambda: [(_cols(10), _label())] * 2, torch.zeros(2, 4), 'params must be'),
    ('params flip', lambda: [(_cols(10), _label())] * 2, torch.tensor([[2, 8, 0, 0], [0, 8, 0, 0]], dtype=torch.int32), 'out of range'),
    ('params above the band', lambda: [(_cols(10), _label())] * 2, torch.tensor([[0, 7, 0, 0], [0, 8, 0, 0]], dtype=torch.int32),
     'out of range'),
    ('params x0', lambda: [(_cols(10), _label())] * 2, torch.tensor([[0, 8, 0, 0], [0, 8, 17, 0]], dtype=torch.int32), 'out of range'),
]


@pytest.mark.parametrize('case', BAD_BATCHES, ids=[c[0] for c in BAD_BATCHES])
def test_a_refused_batch_reaches_no_device_call_and_leaves_the_builder_as_it_was(case, no_device):
    _, samples, params, message = case
    b = EB.EventBatchBuilder(**GEO, seed=3)
    state = b.generator.get_state()
    with pytest.raises(hip.EssHipError, match=message):
        b.build(samples(), params=params)
    assert b.n_batches == 0 and b.last_params is None and b._static is None and torch.equal(b.generator.get_state(), state)


def test_a_well_formed_batch_gets_past_the_checks(no_device):
    """the same builder with a good batch reaches the allocation: the refusals above are not refusals of everything"""
    b = EB.EventBatchBuilder(**GEO)
    with pytest.raises(AssertionError, match='a device call was reached'):
        b.build([(_cols(10), _label()), (_cols(7, t_dtype=np.int64), _label())],
                params=torch.tensor([[1, 8, 16, 0], [0, 8, 0, 0]], dtype=torch.int32))


BAD_BUILDERS = [
    ('crop larger than the grid', dict(crop_hw=(21, 20), crop_band=None), 'does not fit'),
    ('crop without a fitting band', dict(crop_band=(8, 11)), 'no window fits the band'),
    ('band outside the grid', dict(crop_band=(10, 12)), 'band='),
    ('band without crop', dict(crop_hw=None), 'without crop_hw'),
    ('crop without augmentation', dict(augmentation=False), 'part of the augmentation'),
    ('capacity not a multiple of 16', dict(event_capacity=60), 'event_capacity'),
    ('width differs from the resize', dict(width=34), 'widths must agree'),
    ('height above the resize', dict(height=27), 'widths must agree'),
    ('normalisation', dict(grid_normalize='biased'), 'grid_normalize'),
    ('voxel', dict(voxel='histogram'), 'voxel='),
    ('maps with the temporal grid', dict(rectify_maps=[np.zeros((26, 34, 2), np.float32)]), "voxel='trilinear'"),
    ('batch size', dict(batch_size=0), 'batch_size'),
]


@pytest.mark.parametrize('case', BAD_BUILDERS, ids=[c[0] for c in BAD_BUILDERS])
def test_the_builder_refuses_its_keywords(case):
    with pytest.raises(hip.EssHipError, match=case[2]):
        EB.EventBatchBuilder(**{**GEO, **case[1]})


def test_the_presets_are_the_sequence_segmenters():
    d = EB.EventBatchBuilder.dsec(8)
    assert (d.grid_hw, d.grid_rows, d.grid_resize, d.height, d.width, d.crop_hw, d.crop_band, d.label_hw) == \
        ((480, 640), 440, (448, 640), 448, 640, (448, 640), (0, 448), (440, 640))
    k = EB.EventBatchBuilder.ddd17(8, grid_normalize='population')
    assert (k.grid_hw, k.grid_rows, k.grid_resize, k.height, k.width, k.crop_hw, k.crop_band, k.label_hw) == \
        ((260, 346), 260, (260, 352), 200, 352, (120, 216), (80, 120), (200, 346))
    assert d._static is None and k._static is None and k.grid_normalize == hip.GRID_NORM_POPULATION


def test_the_loader_has_the_trainers_loader_interface(no_device):
    b = EB.EventBatchBuilder(**GEO)
    batches = [[(_cols(10), _label())] * 2] * 5
    assert len(EB.EventBatchLoader(batches, b)) == 5 and len(EB.EventBatchLoader(lambda: iter(batches), b, steps=3)) == 3
    with pytest.raises(hip.EssHipError, match='steps is needed'):
        EB.EventBatchLoader(lambda: iter(batches), b)
    with pytest.raises(hip.EssHipError, match='EventBatchBuilder'):
        EB.EventBatchLoader(batches, object())
    seen = []
    b.build = lambda samples: (seen.append(samples) or ('ev', 'lab'))
    loader = EB.EventBatchLoader(lambda: iter(batches), b, steps=3)
    loader.createIterators()
    assert list(loader) == [['ev', 'lab']] * 3 and len(seen) == 3
    assert len(list(loader)) == 3  # (a second epoch: the callable is asked again)


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_the_label_rule_gives_the_double_rules_index_at_the_presets():
    """min(d * src // dst, src - 1) equals floor(d * (1 / (dst / src))) in doubles (cv2's INTER_NEAREST expression; cv2 itself is not
    here: parity with it stays unpinned) for every d at the loaders' label sizes"""
    for src, dst in ((440, 448), (640, 640), (346, 352), (480, 448)):
        d = np.arange(dst)
        assert (np.minimum(d * src // dst, src - 1) == np.minimum(np.floor(d * (1.0 / (dst / src))).astype(np.int64), src - 1)).all()


@pytest.mark.parametrize('src,rows,resize,height,win', [((13, 18), 10, (13, 20), 12, (6, 12)), ((24, 32), 22, (23, 32), 23, (23, 32)),
                                                        ((26, 34), 26, (26, 36), 20, (12, 20))], ids=['small', 'dsec', 'ddd17'])
def test_the_loaders_fp32_lines_pass_the_reference_bound(src, rows, resize, height, win):
    """tests/event_batch_ref.loader_lines -- F.interpolate(bilinear, align_corners=True), the row cuts, torch.flip, the crop -- on
    the fp32 normalised grids stays within loader_grid_ref's bound of its float64 reference pushed through the same flip and crop:
    the yardstick tests/test_hip_event_batches.py holds the builder to is one the loader itself meets"""
    from tests import event_batch_ref as EBR
    from tests import loader_grid_ref as LG
    h, w = win
    for mode in (LG.NORM_NONE, LG.NORM_UNBIASED, LG.NORM_POPULATION):
        acc = LG.seeded_acc(3, 3, *src, seed=mode + src[0], mean=0.3)
        ref, bound = LG.reference(acc, LG.Geometry(src, resize, crop=rows, rows=height), mode)
        grids = LG.restate(acc, LG.Geometry(src), mode)
        for b, (flip, y0, x0) in enumerate([(0, height - h, 0), (1, 0, resize[1] - w), (1, (height - h) // 2, (resize[1] - w) // 2)]):
            got = EBR.loader_lines(grids[b], rows, resize, height, flip, y0, x0, win)
            assert tuple(got.shape) == (3, h, w)
            assert LG.worst_ratio(got, EBR.window(ref[b], flip, y0, x0, h, w), EBR.window(bound[b], flip, y0, x0, h, w)) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ the wrappers
def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


I32, I64, U8 = torch.int32, torch.int64, torch.uint8
GOOD = dict(counts=z(6, dtype=I32), acc=z(6, 3, 13, 18, dtype=I64), out=z(6, 3, 6, 12), words=z(2, 4, dtype=I32), slots_per_group=3,
            crop_rows=10, resize=(13, 20))
BAD_FINISH = [
    ('window taller than the grid', dict(out=z(6, 3, 14, 12)), 'out must be fp32'),
    ('window wider than the grid', dict(out=z(6, 3, 6, 21)), 'out must be fp32'),
    ('out dtype', dict(out=z(6, 3, 6, 12, dtype=torch.float64)), 'out must be fp32'),
    ('out slots', dict(out=z(5, 3, 6, 12)), 'out must be fp32'),
    ('acc dtype', dict(acc=z(6, 3, 13, 18)), 'acc must be'),
    ('counts shape', dict(counts=z(5, dtype=I32)), 'counts must be int32'),
    ('words rows', dict(words=z(3, 4, dtype=I32)), r'words must be int32 \[2, 4\]'),
    ('words dtype', dict(words=z(2, 4, dtype=I64)), 'words must be int32'),
    ('words columns', dict(words=z(2, 3, dtype=I32)), 'words must be int32'),
    ('slots per group', dict(slots_per_group=0), 'slots_per_group'),
    ('crop rows', dict(crop_rows=14), 'crop_rows'),
    ('resize', dict(resize=(13,)), 'resize='),
    ('normalize', dict(normalize=3), 'normalize='),
    ('not a tensor', dict(words=[[0, 0, 0, 0]] * 2), 'words must be a CUDA'),
]


@pytest.mark.parametrize('case', BAD_FINISH, ids=[c[0] for c in BAD_FINISH])
def test_event_grid_finish_window_refuses_before_taking_a_pointer(case):
    with pytest.raises(hip.EssHipError, match=case[2]) as e:
        hip.event_grid_finish_window(**{**GOOD, **case[1]})
    assert 'CPU tensor' not in str(e.value) and 'no CPU path' not in str(e.value) or case[0] == 'not a tensor'


GOOD_LABEL = dict(src=z(2, 7, 5, dtype=U8), out=z(2, 4, 6, dtype=I64), words=z(2, 4, dtype=I32), resize=(5, 9))
BAD_LABEL = [
    ('src dtype', dict(src=z(2, 7, 5, dtype=I64)), 'src must be'),
    ('src rank', dict(src=z(7, 5, dtype=U8)), 'src must be'),
    ('out dtype', dict(out=z(2, 4, 6, dtype=I32)), 'out must be int64'),
    ('window taller than the label', dict(out=z(2, 6, 6, dtype=I64)), 'out must be int64'),
    ('window wider than the label', dict(out=z(2, 4, 10, dtype=I64)), 'out must be int64'),
    ('out samples', dict(out=z(3, 4, 6, dtype=I64)), 'out must be int64'),
    ('words rows', dict(words=z(1, 4, dtype=I32)), 'words must be int32'),
    ('resize', dict(resize=(0, 9)), 'resize='),
]


@pytest.mark.parametrize('case', BAD_LABEL, ids=[c[0] for c in BAD_LABEL])
def test_label_window_refuses_before_taking_a_pointer(case):
    with pytest.raises(hip.EssHipError, match=case[2]) as e:
        hip.label_window(**{**GOOD_LABEL, **case[1]})
    assert 'no CPU path' not in str(e.value)


@pytest.fixture(scope='module')
def built_lib():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


def test_the_library_refuses_bad_windows_before_any_launch(built_lib):
    """ess_event_grid_finish_window / ess_label_window: ESS_EINVAL with a message; every refusal needs no device, the pointers are
    never followed; ess_version() is still 110"""
    import ctypes
    L, P = hip.lib(), ctypes.c_void_p
    assert L.ess_version() == 110
    a = P(4096)
    bins, Hs, Ws = 5, 72, 96
    need, ws_need = bins * Hs * Ws * 8, L.ess_event_grid_finish_workspace(1, bins, Hs, Ws)

    def call(counts=a, n_slots=1, bins=bins, src_height=Hs, src_width=Ws, acc=a, acc_bytes=need, crop_rows=60, resize_height=64,
             resize_width=96, out_rows=60, normalize=1, words=a, slots_per_group=1, win_height=32, win_width=48, out=a, workspace=a,
             workspace_bytes=ws_need):
        return L.ess_event_grid_finish_window(counts, n_slots, bins, src_height, src_width, acc, acc_bytes, crop_rows, resize_height,
                                              resize_width, out_rows, normalize, words, slots_per_group, win_height, win_width, out,
                                              workspace, workspace_bytes, P(0))
    for null in ('counts', 'acc', 'out', 'workspace', 'words'):
        assert call(**{null: P(0)}) == -22 and b'event_grid_finish_window: null' in L.ess_last_error(), null
    for h in (0, -1, 61):
        assert call(win_height=h) == -22 and f'win_height={h} (1..out_rows=60)'.encode() in L.ess_last_error(), h
    for w in (0, 97):
        assert call(win_width=w) == -22 and f'win_width={w} (1..resize_width=96)'.encode() in L.ess_last_error(), w
    assert call(slots_per_group=0) == -22 and b'slots_per_group=0' in L.ess_last_error()
    assert call(words=P(4098)) == -22 and b'words must be 4-byte aligned' in L.ess_last_error()
    assert call(out=P(4104)) == -22 and b'16-byte aligned' in L.ess_last_error()
    assert call(crop_rows=73) == -22 and b'crop_rows=73' in L.ess_last_error()
    assert call(out_rows=65) == -22 and b'out_rows=65' in L.ess_last_error()
    assert call(normalize=3) == -22 and b'normalize=3' in L.ess_last_error()
    assert call(acc_bytes=need - 8) == -22 and b'acc has' in L.ess_last_error()
    assert call(workspace_bytes=ws_need - 1) == -22 and b'workspace has' in L.ess_last_error()

    def label(src=a, n=2, src_height=7, src_width=5, resize_height=5, resize_width=9, words=a, win_height=4, win_width=6, out=a):
        return L.ess_label_window(src, n, src_height, src_width, resize_height, resize_width, words, win_height, win_width, out, P(0))
    for null in ('src', 'words', 'out'):
        assert label(**{null: P(0)}) == -22 and b'label_window: null' in L.ess_last_error(), null
    assert label(n=0) == -22 and b'n=0' in L.ess_last_error()
    assert label(n=65536) == -22 and b'n=65536' in L.ess_last_error()
    assert label(src_height=0) == -22 and b'must be positive' in L.ess_last_error()
    assert label(win_height=6) == -22 and b'win_height=6 (1..resize_height=5)' in L.ess_last_error()
    assert label(win_width=10) == -22 and b'win_width=10 (1..resize_width=9)' in L.ess_last_error()
    assert label(out=P(4100)) == -22 and b'8-byte aligned' in L.ess_last_error()


def test_well_formed_wrapper_calls_get_past_the_shape_checks():
    """what stops them on CPU tensors is the device check: the refusals above are not refusals of everything"""
    for call in (lambda: hip.event_grid_finish_window(**GOOD), lambda: hip.label_window(**GOOD_LABEL)):
        with pytest.raises(hip.EssHipError, match='no CPU path'):
            call()
