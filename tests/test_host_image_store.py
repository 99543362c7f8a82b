"""CPU tier of the device image store (hip.image_ingest, hip.augment_image_label_store, ess_amd/datasets/image_store.py): the numpy
restatement (tests/image_store_ref.py) against PIL ITSELF -- live where PIL is installed, and against PIL's recorded outputs
(tests/golden/image_store.npz) everywhere -- bit for bit; the package's host table builders against the restatement's tables; the
mutants the bit test must catch; every refusal of the wrappers and classes, each before a device call; the host logic of the sampler
and of the paired loader; the ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import image_store_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_image_ingest', 'ess_augment_image_label_store')
EINVAL = -22


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'image_store.npz'))
    return {k: z[k] for k in z.files}


def pairs(gold):
    return [((int(h), int(w)), (int(hr), int(wr))) for h, w, hr, wr in gold['pairs']]


# ---------------------------------------------------------------------------------------------- the restatement against PIL
def test_the_golden_holds_the_size_pairs_the_rules_can_go_wrong_at(gold):
    assert pairs(gold) == [((37, 53), (16, 24)), ((37, 53), (37, 24)), ((20, 30), (33, 47)), ((64, 64), (63, 65)), ((9, 7), (1, 1)),
                           ((64, 128), (16, 32)), ((128, 256), (25, 44))]
    assert R.bilinear_table(128, 32)[1] == 9 and R.bilinear_table(30, 47)[1] == 3  # (the production ratio's 9 taps; upsampling: support 1)


def test_the_restatement_equals_pil_recorded_bit_for_bit(gold):
    for i, (_, out_hw) in enumerate(pairs(gold)):
        assert np.array_equal(R.gray(gold[f'rgb_{i}']), gold[f'gray_{i}']), i
        assert np.array_equal(R.resize_bilinear(gold[f'gray_{i}'], out_hw), gold[f'bil_{i}']), i
        assert np.array_equal(R.ingest(gold[f'rgb_{i}'], out_hw)[0], gold[f'bil_{i}']), i
        assert np.array_equal(R.resize_nearest(gold[f'lab_{i}'], out_hw), gold[f'near_{i}']), i
    out_hw = pairs(gold)[0][1]
    for k, name in enumerate(('all 0', 'all 255', 'checkerboard')):
        assert np.array_equal(R.resize_bilinear(gold['special_in'][k], out_hw), gold['special_out'][k]), name
    assert (gold['special_out'][1] == 255).all() and (gold['special_out'][0] == 0).all()
    assert np.array_equal(R.nearest_table(2048, 352), gold['nearest_2048_352'])


def test_the_restatement_equals_pil_live_bit_for_bit(gold):
    Image = pytest.importorskip('PIL.Image')
    g = np.random.default_rng(5)
    H, W = 37, 53
    yy, xx = np.mgrid[:H, :W]
    for i, (in_hw, out_hw) in enumerate(pairs(gold)):
        Hr, Wr = out_hw
        for rgb in (gold[f'rgb_{i}'], g.integers(0, 256, in_hw + (3,), dtype=np.uint8)):
            L = np.array(Image.fromarray(rgb).convert('L'))
            assert np.array_equal(R.gray(rgb), L), i
            assert np.array_equal(R.resize_bilinear(L, out_hw), np.array(Image.fromarray(L).resize((Wr, Hr), Image.BILINEAR))), i
        lab = g.integers(0, 256, in_hw, dtype=np.uint8)
        assert np.array_equal(R.resize_nearest(lab, out_hw), np.array(Image.fromarray(lab).resize((Wr, Hr), Image.NEAREST))), i
    for frame in (np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8)):
        for out_hw in ((16, 24), (37, 24), (50, 60)):
            want = np.array(Image.fromarray(frame).resize(out_hw[::-1], Image.BILINEAR))
            assert np.array_equal(R.resize_bilinear(frame, out_hw), want), out_hw


def test_the_stretch_is_the_loaders_expression():
    g = np.random.default_rng(9)
    img = g.integers(17, 204, (12, 20), dtype=np.uint8)
    img[0, 0], img[3, 4] = 17, 203
    Imin, Imax = np.min(img), np.max(img)
    want = (255.0 * (img - Imin) / (Imax - Imin)).astype('uint8')  # (cityscapes_loader.py:93-96, on the uint8 array as the loader holds it)
    assert np.array_equal(R.stretch(img), want) and want.min() == 0 and want.max() == 255
    assert not R.stretch(np.full((4, 5), 77, np.uint8)).any()  # (the deviation: a constant frame becomes all 0)


# ---------------------------------------------------------------------------------------------- the package's host tables
def test_the_table_builders_equal_the_restatements_tables():
    from ess_amd.datasets.image_store import pil_bilinear_tables, pil_nearest_table
    for n_in, n_out in ((53, 24), (37, 16), (30, 47), (20, 33), (64, 63), (64, 65), (9, 1), (7, 1), (128, 32), (64, 16), (256, 44), (128, 25),
                        (2048, 512), (2048, 352), (1024, 200), (40, 40), (32, 2)):
        got = pil_bilinear_tables(n_in, n_out)
        want = R.as_array(*R.bilinear_table(n_in, n_out))
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (n_in, n_out)
        assert (got[0] >= 0).all() and (got[0] + got[1] <= n_in).all() and (got[1] >= 1).all() and (np.diff(got[0]) >= 0).all()
        near = pil_nearest_table(n_in, n_out)
        assert near.dtype == np.int32 and np.array_equal(near, R.nearest_table(n_in, n_out)), (n_in, n_out)
        assert near.min() >= 0 and near.max() < n_in


def test_the_table_builders_refuse():
    from ess_amd import hip
    from ess_amd.datasets.image_store import pil_bilinear_tables, pil_nearest_table
    assert pil_bilinear_tables(16 * 7, 7).shape[0] == 2 + hip.IMAGE_MAX_TAPS  # (the largest shrink the kernels hold)
    for call, msg in ((lambda: pil_bilinear_tables(16 * 7 + 1, 7), 'shrinks by at most 16'), (lambda: pil_bilinear_tables(0, 4), 'n_in=0'),
                      (lambda: pil_bilinear_tables(4, 2.0), 'n_out=2.0'), (lambda: pil_nearest_table(4, 0), 'n_out=0'),
                      (lambda: pil_nearest_table(True, 4), 'n_in=True')):
        with pytest.raises(hip.EssHipError, match=msg):
            call()


# ---------------------------------------------------------------------------------------------- mutants
def test_the_bit_test_catches_the_plausible_misreadings(gold):
    """each mutant gives at least one differing pixel on the golden inputs: the comparison above is not vacuous"""
    ps = pairs(gold)

    def differing(**mutant):
        return sum(int((R.resize_bilinear(gold[f'gray_{i}'], out_hw, **mutant) != gold[f'bil_{i}']).sum()) for i, (_, out_hw) in enumerate(ps))
    assert differing() == 0
    assert differing(rounding=False) >= 1            # the 2^21 rounding term dropped
    assert differing(horizontal_first=False) >= 1    # vertical before horizontal: another 8-bit intermediate
    assert differing(half_pixel=False) >= 1          # center without the + 0.5
    assert sum(int((R.gray(gold[f'rgb_{i}'], rounding=False) != gold[f'gray_{i}']).sum()) for i in range(len(ps))) >= 1  # gray without 0x8000
    product = R.nearest_table(2048, 352, running_sum=False)
    assert (product != gold['nearest_2048_352']).sum() >= 1  # nearest by product instead of the running sum
    assert np.array_equal(R.nearest_table(2048, 512, running_sum=False), R.nearest_table(2048, 512))  # (a representable ratio: one rule)


# ---------------------------------------------------------------------------------------------- ABI and the library's refusals
def test_the_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert f'#define ESS_IMAGE_MAX_TAPS {hip.IMAGE_MAX_TAPS} ' in header and f'#define ESS_IMAGE_MAX_SIDE {hip.IMAGE_MAX_SIDE}\n' in header
    assert callable(hip.image_ingest) and callable(hip.augment_image_label_store)


def test_the_library_refuses_bad_arguments_before_any_launch(built_lib):
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    a, b, c, tab = P(16), P(4096), P(8192), P(64)  # (never dereferenced)

    def ingest(frame=a, ch=3, H=8, W=12, ht=tab, htaps=5, vt=tab, vtaps=5, scratch=b, out=c, Hr=4, Wr=6, std=0, mm=P(0), lab=P(0), rows=P(0),
               cols=P(0), out_lab=P(0)):
        return L.ess_image_ingest(frame, ch, H, W, ht, htaps, vt, vtaps, scratch, out, Hr, Wr, std, mm, lab, rows, cols, out_lab, P(0))
    cases = [(dict(frame=P(0)), 'null frame'), (dict(out=P(0)), 'null frame or out'), (dict(ch=2), 'channels=2'), (dict(H=0), 'every side'),
             (dict(Wr=32769), 'every side'), (dict(ht=P(0)), 'h_table is given exactly where the width changes'),
             (dict(W=6), 'h_table is given exactly where the width changes'), (dict(vt=P(0)), 'v_table is given exactly where the height changes'),
             (dict(htaps=34), 'h_taps=34'), (dict(vtaps=0), 'v_taps=0'), (dict(scratch=P(0)), 'null scratch'), (dict(scratch=c), 'distinct'),
             (dict(std=1), 'standardize needs minmax'), (dict(mm=P(18)), '4-byte aligned'), (dict(lab=a), 'come together'),
             (dict(lab=P(32), out_lab=P(48)), 'needs label_rows')]
    for kw, msg in cases:
        assert ingest(**kw) == EINVAL, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert L.ess_last_error().decode().startswith('image_ingest:')

    def aug(images=a, labels=P(0), index=tab, n_slots=3, Hs=8, Ws=12, rows=6, params=b, lut=P(0), out=c, out_l=P(0), N=2, H=5, W=7):
        return L.ess_augment_image_label_store(images, labels, index, n_slots, Hs, Ws, rows, params, lut, out, out_l, N, H, W, P(0))
    cases = [(dict(images=P(0)), 'null images'), (dict(index=P(0)), 'null images, index'), (dict(N=0), 'all must be positive'),
             (dict(n_slots=0), 'all must be positive'), (dict(rows=0), 'rows=0'), (dict(rows=9), 'rows=9'), (dict(labels=a), 'come together'),
             (dict(out_l=c), 'come together'), (dict(index=P(18)), 'aligned'), (dict(lut=P(20)), 'aligned')]
    for kw, msg in cases:
        assert aug(**kw) == EINVAL, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert L.ess_last_error().decode().startswith('augment_image_label_store:')


# ---------------------------------------------------------------------------------------------- the wrappers' refusals
def test_the_wrappers_refuse_on_the_host():
    import torch
    from ess_amd import hip
    from ess_amd.datasets.image_store import pil_bilinear_tables
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    frame, out = u8(8, 12, 3), u8(4, 6)
    ht, vt = torch.from_numpy(pil_bilinear_tables(12, 6)), torch.from_numpy(pil_bilinear_tables(8, 4))
    ok = dict(frame=frame, out=out, h_table=ht, v_table=vt)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    lab = dict(label=u8(8, 12), label_rows=i32(4), label_cols=i32(6), out_label=u8(4, 6))
    for change, msg in ((dict(frame=frame.float()), r'frame must be a non-empty contiguous uint8'), (dict(frame=u8(8, 12, 4)), 'frame must be'),
                        (dict(frame=frame[:, ::2]), 'frame must be'), (dict(frame=np.zeros((8, 12), np.uint8)), 'got ndarray'),
                        (dict(out=u8(4, 6, 1)), 'out must be'), (dict(out=i32(4, 6)), 'out must be'), (dict(h_table=None), r'h_table must be'),
                        (dict(h_table=ht.long()), 'h_table must be'), (dict(h_table=ht[:, :5]), r'\[2 \+ taps, 6\]'),
                        (dict(v_table=torch.zeros(36, 4, dtype=torch.int32)), 'taps <= 33'),
                        (dict(frame=u8(8, 6, 3)), 'h_table belongs to a pass that changes the size'),
                        (dict(out=u8(8, 6), v_table=vt), 'v_table belongs to a pass'), (dict(scratch=u8(8, 12)), r'scratch must be .*\[8, 6\]'),
                        (dict(standardize=True), 'standardize needs minmax'), (dict(minmax=i32(3)), 'minmax must be'),
                        (dict(label=u8(8, 12)), 'given together'), ({**lab, 'label': u8(4, 6)}, r'label must be .*\[8, 12\]'),
                        ({**lab, 'label_rows': i32(6)}, r'label_rows must be .*\[4\]'), ({**lab, 'out_label': u8(8, 12)}, 'out_label must be'),
                        (dict(), 'no CPU path'), (lab, 'no CPU path')):  # (the last check: everything else about the call is fine)
        with pytest.raises(hip.EssHipError, match=msg):
            hip.image_ingest(**{**ok, **change})
    images, labels, index, params = u8(3, 8, 12), u8(3, 8, 12), i32(2), torch.zeros(2, 12)
    lut = torch.arange(256)
    ok = dict(images=images, labels=labels, index=index, rows=6, params=params, height=5, width=7, id_lut=lut)
    for change, msg in ((dict(images=images.float()), 'images must be'), (dict(images=u8(8, 12)), 'images must be'),
                        (dict(labels=u8(3, 8, 11)), 'labels must be'), (dict(index=index.long()), 'index must be'), (dict(index=i32(2, 1)), 'index must be'),
                        (dict(rows=0), 'rows=0'), (dict(rows=9), 'rows=9'), (dict(rows=True), 'rows=True'), (dict(height=0), 'height=0'),
                        (dict(width=2.5), 'width=2.5'), (dict(params=torch.zeros(2, 11)), r'params must be .*\[2, 12\]'),
                        (dict(params=torch.zeros(3, 12)), 'params must be'), (dict(id_lut=torch.arange(255)), '256 entries'),
                        (dict(id_lut=lut.int()), '256 entries'), (dict(out=(torch.zeros(2, 1, 5, 7), None)), 'exactly where labels are given'),
                        (dict(out=(torch.zeros(2, 5, 7), torch.zeros(2, 5, 7, dtype=torch.int64))), r'out\[0\] must be'),
                        (dict(out=(torch.zeros(2, 1, 5, 7), torch.zeros(2, 5, 7))), r'out\[1\] must be'), (dict(), 'no CPU path'),
                        (dict(labels=None, id_lut=None), 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=msg):
            hip.augment_image_label_store(**{**ok, **change})


# ---------------------------------------------------------------------------------------------- the classes
def _state(store):
    return (store.n_images, store.has_labels, store._dev)


def test_the_store_refuses_before_a_byte_moves():
    import torch
    from ess_amd import hip
    from ess_amd.datasets.image_store import ImageBatchBuilder, ImageSampler, ImageStore
    for kw, msg in ((dict(capacity_images=0), 'capacity_images=0'), (dict(capacity_images=2.0), 'capacity_images=2.0'),
                    (dict(capacity_images=3, staging_images=1), 'staging_images=1'), (dict(capacity_images=3, resize_hw=(0, 4)), 'resize_hw'),
                    (dict(capacity_images=3, source_hw=[8]), 'source_hw'),
                    (dict(capacity_images=3, resize_hw=(4, 6), source_hw=(8, 6 * 17)), 'shrinks by at most 16')):
        with pytest.raises(hip.EssHipError, match=msg):
            ImageStore(**kw)
    store = ImageStore(3, resize_hw=(4, 6), source_hw=(8, 12))
    assert store.capacity == 3 and store.n_images == 0 and store.bytes() == 3 * (2 * 24 + 8)
    full = ImageStore(2975)
    assert round(full.bytes() / 1e9, 2) == 0.78  # (the docstring's figure: Cityscapes train with labels)
    rgb, gray, lab = np.zeros((8, 12, 3), np.uint8), np.zeros((8, 12), np.uint8), np.zeros((8, 12), np.uint8)
    before = _state(store)
    refusals = [
        (lambda: store.add_images([rgb.astype(np.float32)]), r'frames\[0\] must be a host uint8'),
        (lambda: store.add_images([rgb, np.zeros((8, 12, 4), np.uint8)]), r'frames\[1\] must be'),
        (lambda: store.add_images([np.zeros((12, 8), np.uint8)]), r'frames\[0\] must be'),
        (lambda: store.add_images([]), 'non-empty list'), (lambda: store.add_images(rgb), 'non-empty list'),
        (lambda: store.add_images(torch.zeros(1, 8, 12, dtype=torch.uint8)), 'non-empty list'),
        (lambda: store.add_images([rgb, gray], labels=[lab, None]), 'a label for every frame of the call, or for none'),
        (lambda: store.add_images([rgb, gray], labels=[lab]), 'one label map per frame'),
        (lambda: store.add_images([rgb], labels=[lab.astype(np.int64)]), r'labels\[0\] must be a host uint8'),
        (lambda: store.add_images([rgb], labels=[np.zeros((4, 6), np.uint8)]), r'labels\[0\] must be'),
        (lambda: store.add_images([rgb] * 4), 'the store is full: 0 \\+ 4 frames, capacity_images 3'),
        (lambda: store.images, 'the store is empty'),
    ]
    for call, msg in refusals:
        with pytest.raises(hip.EssHipError, match=msg):
            call()
        assert _state(store) == before, msg
    store.has_labels, store.n_images = True, 2  # (the bookkeeping alone: no device is touched by a refusal)
    for call, msg in ((lambda: store.add_images([rgb]), 'this store keeps labels'), (lambda: store.add_images([rgb] * 2, labels=[lab] * 2), 'the store is full')):
        with pytest.raises(hip.EssHipError, match=msg):
            call()
    store.has_labels = False
    with pytest.raises(hip.EssHipError, match='this store keeps no labels'):
        store.add_images([rgb], labels=[lab])
    assert store._dev is None
    # -- the builder and the sampler over that bookkeeping
    for kw, msg in ((dict(store=object()), 'store must be an ImageStore'), (dict(device='cuda:1'), 'built where the store lies'),
                    (dict(height=0), 'height, width'), (dict(semseg_num_classes=19), '6 or 11 classes'), (dict(seed=1.5), 'seed=1.5')):
        with pytest.raises(hip.EssHipError, match=msg):
            ImageBatchBuilder(**{**dict(store=store, height=4, width=6), **kw})
    bld = ImageBatchBuilder(store, 3, 5)
    assert (bld.rows, bld.shift_limit) == (3, 0.0)  # (random_crop: the img[:height] cut, shift_limit 0)
    assert (ImageBatchBuilder(store, 6, 5).rows, ImageBatchBuilder(store, 3, 5, random_crop=False).rows) == (4, 4)
    assert ImageBatchBuilder(store, 3, 5, random_crop=False).shift_limit == 0.1
    for indices, msg in (([0, 2], r'indices\[1\]=2, the store holds 2'), ([-1], r'indices\[0\]=-1'), ([], 'non-empty list'), ([0.5], 'non-empty list'),
                         (3, 'non-empty list')):
        with pytest.raises(hip.EssHipError, match=msg):
            bld.build(indices)
        assert bld._static is None and bld.n_batches == 0 and store._dev is None
    bld.batch_size = 2
    with pytest.raises(hip.EssHipError, match='static buffers hold batch_size=2'):
        bld.build([0, 1, 0])
    for kw, msg in ((dict(store=None), 'store must be an ImageStore'), (dict(batch_size=0), 'batch_size=0'), (dict(indices=[0, 2]), r'indices\[1\]=2'),
                    (dict(seed='a'), "seed='a'")):
        with pytest.raises(hip.EssHipError, match=msg):
            ImageSampler(**{**dict(store=store, batch_size=2), **kw})


def test_the_id_table_is_the_references_rule():
    from ess_amd.datasets.image_store import cityscapes_id_lut
    six, eleven = cityscapes_id_lut(6), cityscapes_id_lut(11)
    assert six.dtype.is_floating_point is False and six.shape == (256,) and eleven.shape == (256,)
    assert [int(six[i]) for i in (0, 7, 8, 11, 13, 17, 20, 21, 23, 24, 26, 29, 31, 33)] == [255, 0, 0, 1, 1, 2, 2, 3, 1, 4, 5, 255, 5, 5]
    assert [int(eleven[i]) for i in (7, 8, 11, 12, 13, 17, 19, 21, 23, 25, 28, 30, 33)] == [5, 6, 1, 9, 2, 4, 10, 7, 0, 3, 8, 255, 8]
    assert set(six[:34].tolist()) == set(range(6)) | {255} and set(eleven[:34].tolist()) == set(range(11)) | {255}
    assert six[34:].tolist() == list(range(34, 256))  # (ids the table does not name stay as they are)


def test_the_samplers_permutation_and_fill_up_rule():
    from ess_amd.datasets.image_store import ImageSampler, ImageStore
    store = ImageStore(8, resize_hw=(4, 6), source_hw=(8, 12))
    store.n_images = 5
    s = ImageSampler(store, 2, seed=3)
    first, second = [b.tolist() for b in s], [b.tolist() for b in s]
    assert len(s) == 2 and all(len(b) == 2 for b in first) and first != second and len({i for b in first for i in b}) == 4
    want = np.random.default_rng(3).permutation(5)
    assert first == [want[:2].tolist(), want[2:4].tolist()]
    tail = ImageSampler(store, 2, shuffle=False, drop_last=False)
    assert len(tail) == 3 and [b.tolist() for b in tail] == [[0, 1], [2, 3], [4, 0]]
    sub = ImageSampler(store, 3, indices=[4, 1, 3, 2], shuffle=False, drop_last=False)
    assert [b.tolist() for b in sub] == [[4, 1, 3], [2, 4, 1]]


class _Stub:
    """a loader of `n` batches [name k, label k]; counts its restarts"""

    def __init__(self, name, n):
        self.name, self.n, self.starts = name, n, 0

    def __len__(self):
        return self.n

    def createIterators(self):
        self.starts += 1

    def __iter__(self):
        return iter([[f'{self.name}{k}', f'l{self.name}{k}'] for k in range(self.n)])


def test_the_paired_loader_follows_the_wrappers_rule():
    from ess_amd import hip
    from ess_amd.datasets.image_store import PairedBatchLoader
    a, b = _Stub('a', 2), _Stub('b', 5)
    p = PairedBatchLoader(a, b)
    assert len(p) == 5  # (the longer side sets the epoch)
    got = list(p)
    assert [x[0][0] for x in got] == ['a0', 'a1', 'a0', 'a1', 'a0'] and [x[1][0] for x in got] == ['b0', 'b1', 'b2', 'b3', 'b4']
    assert got[0] == [['a0', 'la0'], ['b0', 'lb0']]  # (the UDA layout: [[img, label_a], [events, label_b]])
    assert (a.starts, b.starts) == (3, 1)  # (the shorter side restarted twice)
    assert len(list(p)) == 5  # (a new epoch without createIterators)
    first = PairedBatchLoader(a, b, dataset_len_to_use='first')
    assert len(first) == 2 and [x[1][0] for x in first] == ['b0', 'b1']
    second = PairedBatchLoader(_Stub('a', 4), _Stub('b', 3), dataset_len_to_use='second')
    assert len(second) == 3 and [x[0][0] for x in second] == ['a0', 'a1', 'a2']
    longer_a = PairedBatchLoader(_Stub('a', 3), _Stub('b', 2))
    assert len(longer_a) == 3 and [(x[0][0], x[1][0]) for x in longer_a] == [('a0', 'b0'), ('a1', 'b1'), ('a2', 'b0')]
    equal = PairedBatchLoader(_Stub('a', 2), _Stub('b', 2))  # (equal lengths: the second side sets the epoch, as len(a) > len(b) is False)
    assert not equal.a_sets_epoch and len(list(equal)) == 2
    # -- the shorter side is advanced FIRST: it has restarted before the longer side ends the epoch
    order = []

    class Spy(_Stub):
        def __iter__(self):
            for k in range(self.n):
                order.append(f'{self.name}{k}')
                yield [f'{self.name}{k}', None]
    list(PairedBatchLoader(Spy('a', 1), Spy('b', 2)))
    assert order == ['a0', 'b0', 'a0', 'b1']
    for kw, msg in ((dict(loader_a=object()), 'loader_a must be a loader'), (dict(dataset_len_to_use='third'), "dataset_len_to_use='third'")):
        with pytest.raises(hip.EssHipError, match=msg):
            PairedBatchLoader(**{**dict(loader_a=a, loader_b=b), **kw})
    with pytest.raises(hip.EssHipError, match='yields no batch'):
        list(PairedBatchLoader(_Stub('a', 0), _Stub('b', 2)))


def test_the_batch_loader_refuses_and_iterates_with_a_stub_builder():
    from ess_amd import hip
    from ess_amd.datasets.image_store import ImageBatchBuilder, ImageBatchLoader, ImageSampler, ImageStore
    store = ImageStore(8, resize_hw=(4, 6), source_hw=(8, 12))
    store.n_images = 5
    bld = ImageBatchBuilder(store, 3, 5)
    sampler = ImageSampler(store, 2, shuffle=False)
    for kw, msg in ((dict(builder=object()), 'builder must be an ImageBatchBuilder'), (dict(sampler=iter([])), 'steps is needed'),
                    (dict(steps=-1), 'steps=-1'), (dict(sampler=3, steps=1), 'sampler must be an iterable')):
        with pytest.raises(hip.EssHipError, match=msg):
            ImageBatchLoader(**{**dict(sampler=sampler, builder=bld), **kw})
    seen = []
    bld.build = lambda indices: (seen.append(indices.tolist()) or 'img', 'lab')  # (the loop alone: no device)
    loader = ImageBatchLoader(sampler, bld)
    assert len(loader) == 2 and list(loader) == [['img', 'lab']] * 2 and seen == [[0, 1], [2, 3]]
    assert len(list(ImageBatchLoader(lambda: iter(sampler), bld, steps=1))) == 1
