"""CPU tier of the paired camera frames (hip.image_ingest_frame, hip.image_gather_unit, ImageStore's resample / gray / keep_rows,
EventBatchBuilder(frames=, original_labels=)): the numpy restatement (tests/frame_store_ref.py) against PIL ITSELF -- live where PIL is
installed, called as the event loaders call it (Image.resize without a filter, then convert('L')), and against PIL's recorded outputs
(tests/golden/frame_store.npz) everywhere -- bit for bit; the package's host tables against the restatement's; the mutants the bit
tests must catch; every refusal of the wrappers and classes, each before a device call; the ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import frame_store_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_image_ingest_frame', 'ess_image_gather_unit')
EINVAL = -22
CASES = [((37, 300, 3), (29, 277)), ((23, 41), (31, 59)), ((30, 64, 3), (28, 64)), ((30, 64, 3), (30, 50)), ((26, 35), (26, 36)),
         ((37, 53, 3), (29, 41)), ((37, 53), (61, 90)), ((64, 80, 3), (9, 11))]
PRESETS = [((480, 640, 3), (448, 640)), ((260, 346), (260, 352)), ((260, 346, 3), (260, 352))]


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'frame_store.npz'))
    return {k: z[k] for k in z.files}


def _pil(img, out_hw):
    """the event loaders' calls: Image.resize with NO filter argument, transforms.Grayscale() behind it"""
    from PIL import Image
    r = Image.fromarray(img).resize((out_hw[1], out_hw[0]))
    return np.array(r.convert('L') if img.ndim == 3 else r)


# ---------------------------------------------------------------------------------------------- the restatement against PIL
def test_the_golden_holds_the_cases_of_this_file(gold):
    got = [(tuple(int(v) for v in row[:3] if v), (int(row[3]), int(row[4]))) for row in gold['cases']]
    assert got == CASES
    assert R.resize_table(300, 277)[1] == 7 and R.resize_table(41, 59)[1] == 5 and R.resize_table(80, 11)[1] == 31  # (the window sizes)


def test_the_restatement_equals_pil_recorded_bit_for_bit(gold):
    seed = int(gold['seed'])
    for i, (shape, out_hw) in enumerate(CASES):
        got = R.frame(R.make_image(shape, seed + i), out_hw)
        assert got.dtype == np.uint8 and np.array_equal(got, gold[f'out_{i}']), (shape, out_hw)


def test_the_restatement_equals_pil_live_bit_for_bit():
    Image = pytest.importorskip('PIL.Image')
    bicubic = getattr(Image, 'Resampling', Image).BICUBIC
    for i, (shape, out_hw) in enumerate(CASES + PRESETS):
        img = R.make_image(shape, 77 + i)
        want = _pil(img, out_hw)
        assert np.array_equal(R.frame(img, out_hw), want), (shape, out_hw)
        named = Image.fromarray(img).resize(out_hw[::-1], bicubic)  # (the default filter IS bicubic on this PIL)
        assert np.array_equal(np.array(named.convert('L') if img.ndim == 3 else named), want), (shape, out_hw)
    # the DDD17 cut and the no-resize form
    img = R.make_image((260, 346, 3), 5)
    assert np.array_equal(R.frame(img, (260, 352), keep_rows=200), _pil(img, (260, 352))[:200])
    assert np.array_equal(R.frame(img), np.array(Image.fromarray(img).convert('L')))
    # bilinear through the same code is PIL's bilinear
    bilinear = getattr(Image, 'Resampling', Image).BILINEAR
    g = R.make_image((37, 53), 6)
    assert np.array_equal(R.frame(g, (16, 24), resample='bilinear'), np.array(Image.fromarray(g).resize((24, 16), bilinear)))


def test_the_bit_tests_catch_the_plausible_misreadings(gold):
    """each mutant changes at least one pixel of a recorded case: the comparisons above are not vacuous"""
    seed = int(gold['seed'])
    shape, out_hw = CASES[0]  # (RGB, both sides shrink)
    img, want = R.make_image(shape, seed), gold['out_0']

    def differing(**mutant):
        return int((R.frame(img, out_hw, **mutant) != want).sum())
    assert differing() == 0
    assert differing(gray_last=False) >= 1    # gray first instead of gray last
    assert differing(round_away=False) >= 1   # trunc(0.5 + w 2^22) for the negative coefficients
    assert differing(clip_low=False) >= 1     # no clip at 0: a negative value wraps
    assert differing(clip_high=False) >= 1    # no clip at 255
    assert differing(float_mid=True) >= 1     # an unrounded intermediate between the passes
    # the gray cases see the clip and the intermediate too (both sides grow)
    shape, out_hw = CASES[1]
    img, want = R.make_image(shape, seed + 1), gold['out_1']
    for mutant in (dict(clip_low=False), dict(clip_high=False), dict(float_mid=True)):
        assert int((R.frame(img, out_hw, **mutant) != want).sum()) >= 1, mutant


def test_the_unit_gather_is_totensors_expression():
    import torch
    g = np.random.default_rng(3)
    slots = g.integers(0, 256, (7, 20, 36), dtype=np.uint8)
    slots[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    got = R.gather_unit(slots, [3, 0, 3, -1, 7])
    want = torch.from_numpy(slots).float().div(255)
    assert got.dtype == np.float32 and got.shape == (5, 1, 20, 36)
    for b, i in enumerate((3, 0, 3)):
        assert np.array_equal(got[b, 0].view(np.uint32), want[i].numpy().view(np.uint32))
    assert not got[3].any() and not got[4].any()
    recip = slots[0].astype(np.float32) * np.float32(1.0 / 255.0)  # (the mutant: a reciprocal multiply)
    assert (recip.view(np.uint32) != got[1, 0].view(np.uint32)).any()


# ---------------------------------------------------------------------------------------------- the package's host tables
RATIOS = ((53, 24), (37, 16), (30, 47), (20, 33), (64, 63), (64, 65), (9, 1), (7, 1), (128, 32), (64, 16), (256, 44), (128, 25), (2048, 512),
          (2048, 352), (1024, 200), (40, 40), (32, 2))  # (those of tests/test_host_image_store.py)


def test_the_bilinear_case_is_the_existing_builder_exactly():
    from ess_amd.datasets.image_store import pil_bilinear_tables, pil_resize_tables
    for n_in, n_out in RATIOS:
        a, b = pil_resize_tables(n_in, n_out, 'bilinear'), pil_bilinear_tables(n_in, n_out)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (n_in, n_out)
        assert np.array_equal(pil_resize_tables(n_in, n_out), b)  # (the default)


def test_the_bicubic_tables_equal_the_restatements_tables():
    from ess_amd.datasets.image_store import pil_resize_tables
    negative = 0
    for n_in, n_out in RATIOS + ((480, 448), (346, 352), (300, 277), (41, 59), (64, 8), (80, 11)):
        if 2 * int(np.ceil(2 * max(n_in / n_out, 1.0))) + 1 > 33:
            continue
        got = pil_resize_tables(n_in, n_out, 'bicubic')
        want = R.as_array(*R.resize_table(n_in, n_out, 'bicubic'))
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (n_in, n_out)
        assert (got[0] >= 0).all() and (got[0] + got[1] <= n_in).all() and (got[1] >= 1).all() and (np.diff(got[0]) >= 0).all()
        assert (np.diff(got[0] + got[1]) >= 0).all()  # (the windows' ends never decrease: the kept rows' last window ends what is read)
        assert int(np.abs(got[2:].astype(np.int64)).sum(axis=0).max()) * 255 + (1 << 21) < 1 << 31  # (the kernels' int32 sums)
        negative += int((got[2:] < 0).sum())
        trunc = R.as_array(*R.resize_table(n_in, n_out, 'bicubic', round_away=False))
        assert n_in == n_out or n_out == 1 or not (got[2:] < 0).any() or (trunc != got).any(), (n_in, n_out)  # (the rounding rule shows)
    assert negative > 0


def test_the_table_builder_refuses():
    from ess_amd import hip
    from ess_amd.datasets.image_store import pil_resize_tables
    assert pil_resize_tables(8 * 7, 7, 'bicubic').shape[0] == 2 + hip.IMAGE_MAX_TAPS  # (the largest shrink the kernels hold)
    for call, msg in ((lambda: pil_resize_tables(8 * 7 + 1, 7, 'bicubic'), 'shrinks by at most 8'), (lambda: pil_resize_tables(0, 4, 'bicubic'), 'n_in=0'),
                      (lambda: pil_resize_tables(4, 2.0, 'bicubic'), 'n_out=2.0'), (lambda: pil_resize_tables(4, 2, 'lanczos'), "resample='lanczos'"),
                      (lambda: pil_resize_tables(16 * 7 + 1, 7, 'bilinear'), 'shrinks by at most 16')):
        with pytest.raises(hip.EssHipError, match=msg):
            call()


# ---------------------------------------------------------------------------------------------- ABI and the library's refusals
def test_the_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert callable(hip.image_ingest_frame) and callable(hip.image_gather_unit)


def test_the_library_refuses_bad_arguments_before_any_launch(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    a, b, c, tab = P(16), P(4096), P(8192), P(64)  # (never dereferenced)

    def ingest(frame=a, ch=3, H=8, W=12, ht=tab, htaps=5, vt=tab, vtaps=5, scratch=b, out=c, Hr=4, Wr=6, rows=4, last=1):
        return L.ess_image_ingest_frame(frame, ch, H, W, ht, htaps, vt, vtaps, scratch, out, Hr, Wr, rows, last, P(0))
    cases = [(dict(frame=P(0)), 'null frame'), (dict(out=P(0)), 'null frame or out'), (dict(ch=2), 'channels=2'), (dict(last=2), 'gray_last=2'),
             (dict(H=0), 'every side'), (dict(Wr=32769), 'every side'), (dict(rows=0), 'out_rows=0'), (dict(rows=5), 'out_rows=5'),
             (dict(ht=P(0)), 'h_table is given exactly where the width changes'), (dict(W=6), 'h_table is given exactly where the width changes'),
             (dict(vt=P(0)), 'v_table is given exactly where the height changes'), (dict(htaps=34), 'h_taps=34'), (dict(vtaps=0), 'v_taps=0'),
             (dict(scratch=P(0)), 'null scratch'), (dict(scratch=c), 'distinct'), (dict(vt=P(18)), '4-byte aligned'),
             (dict(ch=3, last=0, W=6, ht=P(0), scratch=P(0)), 'null scratch')]  # (gray first needs the scratch without a horizontal table)
    for kw, msg in cases:
        assert ingest(**kw) == EINVAL, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert L.ess_last_error().decode().startswith('image_ingest_frame:')

    def gather(images=a, capacity=3, Hs=8, Ws=12, index=tab, i64=0, B=2, out=b):
        return L.ess_image_gather_unit(images, capacity, Hs, Ws, index, i64, B, out, P(0))
    cases = [(dict(images=P(0)), 'null images'), (dict(index=P(0)), 'null images, index'), (dict(out=P(0)), 'null images, index or out'),
             (dict(capacity=0), 'capacity=0'), (dict(Hs=0), 'a positive count'), (dict(B=0), 'B=0'), (dict(B=65536), 'B=65536'),
             (dict(i64=2), 'index_i64=2'), (dict(index=P(68), i64=1), 'aligned'), (dict(index=P(66)), 'aligned')]
    for kw, msg in cases:
        assert gather(**kw) == EINVAL, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert L.ess_last_error().decode().startswith('image_gather_unit:')


# ---------------------------------------------------------------------------------------------- the wrappers' refusals
def test_the_wrappers_refuse_on_the_host():
    import torch
    from ess_amd import hip
    from ess_amd.datasets.image_store import pil_resize_tables
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    frame, out = u8(8, 12, 3), u8(4, 6)
    ht, vt = torch.from_numpy(pil_resize_tables(12, 6, 'bicubic')), torch.from_numpy(pil_resize_tables(8, 4, 'bicubic'))
    ok = dict(frame=frame, out=out, h_table=ht, v_table=vt)
    for change, msg in ((dict(frame=frame.float()), r'frame must be a non-empty contiguous uint8'), (dict(frame=u8(8, 12, 4)), 'frame must be'),
                        (dict(frame=np.zeros((8, 12), np.uint8)), 'got ndarray'), (dict(out=u8(4, 6, 1)), 'out must be'),
                        (dict(out=i32(4, 6)), 'out must be'), (dict(h_table=None), 'h_table must be'), (dict(h_table=ht.long()), 'h_table must be'),
                        (dict(v_table=torch.zeros(36, 4, dtype=torch.int32)), 'taps <= 33'),
                        (dict(frame=u8(8, 6, 3)), 'h_table belongs to a pass that changes the size'),
                        (dict(resized_rows=3), 'resized_rows=3'), (dict(resized_rows=4.0), 'resized_rows=4.0'),
                        (dict(resized_rows=5), r'v_table must be .*\[2 \+ taps, 5\]'), (dict(gray_last=2), 'gray_last=2'),
                        (dict(scratch=u8(8, 6)), r'scratch must be .*\[8, 6, 3\]'), (dict(scratch=u8(8, 6, 3), gray_last=False), r'scratch must be .*\[8, 6\]'),
                        (dict(frame=u8(8, 12), scratch=u8(8, 6, 3)), r'scratch must be .*\[8, 6\]'),
                        (dict(), 'no CPU path'), (dict(out=u8(3, 6), resized_rows=4), 'no CPU path')):  # (the last check)
        with pytest.raises(hip.EssHipError, match=msg):
            hip.image_ingest_frame(**{**ok, **change})
    images, index = u8(3, 8, 12), i32(2)
    ok = dict(images=images, index=index)
    for change, msg in ((dict(images=images.float()), 'images must be'), (dict(images=u8(8, 12)), 'images must be'),
                        (dict(index=index.float()), 'index must be'), (dict(index=i32(2, 1)), 'index must be'), (dict(index=i32(0)), 'index must be'),
                        (dict(index=[0, 1]), 'got list'), (dict(out=torch.zeros(2, 8, 12)), r'out must be .*\[2, 1, 8, 12\]'),
                        (dict(out=torch.zeros(2, 1, 8, 12, dtype=torch.float64)), 'out must be'), (dict(), 'no CPU path'),
                        (dict(index=index.long()), 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=msg):
            hip.image_gather_unit(**{**ok, **change})


# ---------------------------------------------------------------------------------------------- the classes
def test_the_frame_store_keywords_and_presets_refuse_before_a_byte_moves():
    from ess_amd import hip
    from ess_amd.datasets.image_store import ImageBatchBuilder, ImageStore
    base = dict(capacity_images=3, resize_hw=(4, 6), source_hw=(8, 12))
    for kw, msg in ((dict(resample='lanczos'), "resample='lanczos'"), (dict(resample=2), 'resample=2'), (dict(gray='middle'), "gray='middle'"),
                    (dict(keep_rows=0), 'keep_rows=0'), (dict(keep_rows=5), 'keep_rows=5'), (dict(keep_rows=2.0), 'keep_rows=2.0'),
                    (dict(gray='last', standardization=True), 'standardization belongs'), (dict(keep_rows=2, standardization=True), 'standardization belongs'),
                    (dict(resample='bicubic', standardization=True), 'standardization belongs'),
                    (dict(resample='bicubic', source_hw=(8, 6 * 9)), 'shrinks by at most 8')):
        with pytest.raises(hip.EssHipError, match=msg):
            ImageStore(**{**base, **kw})
    plain = ImageStore(**base)
    assert (plain.resample, plain.gray, plain.keep_rows, plain.frame_store, plain.slot_hw) == ('bilinear', 'first', None, False, (4, 6))
    assert plain.bytes() == 3 * (2 * 24 + 8)  # (today's figure)
    same = ImageStore(3, resize_hw=None, source_hw=(8, 12), gray='last')
    assert same.resize_hw == (8, 12) and same._tables['h'] is None and same._tables['v'] is None and same.frame_store
    dsec, raw, ddd = ImageStore.dsec_frames(4), ImageStore.dsec_frames(4, resize=False), ImageStore.ddd17_frames(5)
    assert (dsec.source_hw, dsec.resize_hw, dsec.slot_hw, dsec.resample, dsec.gray, dsec.keep_rows) == ((480, 640), (448, 640), (448, 640), 'bicubic', 'last', None)
    assert (raw.source_hw, raw.resize_hw, raw.slot_hw) == ((480, 640), (480, 640), (480, 640)) and raw._tables['v'] is None
    assert (ddd.source_hw, ddd.resize_hw, ddd.slot_hw, ddd.resample, ddd.gray, ddd.keep_rows) == ((260, 346), (260, 352), (200, 352), 'bicubic', 'last', 200)
    assert dsec._tables['h'] is None and dsec._tables['v'].shape == (2 + 7, 448) and ddd._tables['v'] is None and ddd._tables['h'].shape == (2 + 5, 352)
    assert (dsec._tables['v'][2:] < 0).any()
    assert ddd.bytes() == 5 * (200 * 352 + 8) and ddd.capacity == 5
    rgb, lab = np.zeros((260, 346, 3), np.uint8), np.zeros((260, 346), np.uint8)
    for store in (ddd, ImageStore(3, resize_hw=(260, 352), source_hw=(260, 346), keep_rows=200), ImageStore(3, resize_hw=None, source_hw=(260, 346), gray='last')):
        before = (store.n_images, store.has_labels, store._dev)
        for call, msg in ((lambda: store.add_images([rgb], labels=[lab]), 'keeps no labels'), (lambda: store.add_images([rgb[:200]]), r'frames\[0\] must be'),
                          (lambda: store.add_images([rgb] * 6), 'the store is full'), (lambda: store.images, 'the store is empty')):
            with pytest.raises(hip.EssHipError, match=msg):
                call()
            assert (store.n_images, store.has_labels, store._dev) == before, msg
    assert ImageBatchBuilder(ddd, 120, 352).rows == 120 and ImageBatchBuilder(ddd, 260, 352).rows == 200  # (a slot's rows, not the resize's)


def test_the_batch_builder_refuses_frames_before_anything_is_staged():
    from ess_amd import hip
    from ess_amd.datasets.event_batches import EventBatchBuilder, EventBatchLoader
    from ess_amd.datasets.event_store import EventStore, StoreSample
    from ess_amd.datasets.image_store import ImageStore
    for kw, msg in ((dict(frame=-1), 'frame=-1'), (dict(frame=1.0), 'frame=1.0'), (dict(frame=True), 'frame=True')):
        with pytest.raises(hip.EssHipError, match=msg):
            StoreSample(0, end=5, **kw)
    s = StoreSample(0, end=5, frame=2)
    assert s.frame == 2 and StoreSample(0, end=5).frame is None and 'frame=2' in repr(s)
    with pytest.raises(AttributeError):
        s.frame = 3
    store = EventStore(1000, label_hw=(4, 6), label_capacity=3)
    store._recs = [[0, 100, 1, 0, 99, 0, 2], [100, 160, 0, 0.5, 9.0, 2, 0]]  # (the bookkeeping alone)
    store.n_events, store.n_labels = 160, 2
    frames = ImageStore(4, resize_hw=None, source_hw=(8, 8), gray='last')
    frames.n_images, frames.has_labels = 2, False
    geo = dict(grid_hw=(8, 8), height=8, width=8, label_hw=(4, 6))
    for kw, msg in ((dict(frames=frames, store=None, window_events=None, event_capacity=64), 'it needs store='),
                    (dict(frames=object()), 'frames must be an ImageStore'),
                    (dict(frames=ImageStore(4, resize_hw=None, source_hw=(8, 8), gray='last', device='cuda:1')), 'a batch is built on one device'),
                    (dict(original_labels=1), 'original_labels=1'), (dict(original_labels=True), 'with augmentation=True'),
                    (dict(original_labels=True, augmentation=False, store=None, window_events=None, event_capacity=64), 'it needs store=')):
        args = {**dict(store=store, window_events=5, event_capacity=None), **geo, **kw}
        with pytest.raises(hip.EssHipError, match=msg):
            EventBatchBuilder(2, 3, 2, args.pop('event_capacity'), **args)
    bld = EventBatchBuilder(2, 3, 2, None, store=store, window_events=5, frames=frames, original_labels=True, augmentation=False, **geo)
    assert bld.frames is frames and bld.original_labels is True
    layout, nbytes = bld._store_layout()
    assert 'frame_of' in layout and layout['frame_of'][0] % 16 == 0 and nbytes == layout['frame_of'][0] + 16
    plain = EventBatchBuilder(2, 3, 2, None, store=store, window_events=5, **geo)
    assert 'frame_of' not in plain._store_layout()[0] and plain._store_layout()[1] == layout['frame_of'][0]  # (today's table is unchanged)
    S = StoreSample
    state = bld.generator.get_state()
    for samples, msg in (([S(0, end=5, label=0, frame=0), S(1, end=5, label=1)], r'samples\[1\] has no frame'),
                         ([S(0, end=5, label=0, frame=2), S(1, end=5, label=1, frame=0)], r'samples\[0\]: frame slot 2, the frame store holds 2'),
                         ([S(0, end=5, frame=0), S(1, end=5, frame=1)], 'original_labels=True: every sample')):
        with pytest.raises(hip.EssHipError, match=msg):
            bld.build(samples)
        assert bld._static is None and bld.n_batches == 0 and store._dev is None and frames._dev is None
    assert (bld.generator.get_state() == state).all()
    # the loader passes the longer tuples through unchanged
    bld.build = lambda samples: ('ev', 'img', 'lab', 'orig')
    assert list(EventBatchLoader([[0], [1]], bld)) == [['ev', 'img', 'lab', 'orig']] * 2
    plain.build = lambda samples: ('ev', 'lab')
    assert list(EventBatchLoader([[0]], plain)) == [['ev', 'lab']]
