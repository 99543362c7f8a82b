"""GPU tier of the device image store: hip.image_ingest against the numpy restatement (tests/image_store_ref.py, proved equal to PIL on
the CPU tier) and against PIL's recorded outputs (tests/golden/image_store.npz), BIT FOR BIT; the ImageStore's upload through its
staging sets; hip.augment_image_label_store against the float entry point on gathered slots, bit for bit; ImageBatchBuilder eager
against its captured graph and against the composition it replaces; and one UDA train step from an ImageStore and an EventStore
through a PairedBatchLoader.  Small shapes: every rule that can go wrong does so at them (odd sizes, a skipped pass, upsampling,
the 9-tap production ratio, ratios float64 does not represent, more than one workgroup a row at 2 x 300 -> 1 x 290)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import image_store_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')
FILL = 0xA5  # what every output and scratch buffer holds before a launch: an unwritten pixel cannot pass


@functools.lru_cache(maxsize=None)
def _gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'image_store.npz'))
    return {k: z[k] for k in z.files}


def _pairs():
    return [((int(h), int(w)), (int(hr), int(wr))) for h, w, hr, wr in _gold()['pairs']]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ingest(frame, out_hw, standardize=False, label=None):
    """one frame through hip.image_ingest with 0xA5 in every buffer it writes -> (slot, (min, max), label slot or None) on the host"""
    from ess_amd import hip
    from ess_amd.datasets.image_store import pil_bilinear_tables, pil_nearest_table
    (H, W), (Hr, Wr) = frame.shape[:2], out_hw
    out = torch.full((Hr, Wr), FILL, dtype=torch.uint8, device=DEV)
    scratch = torch.full((H, Wr), FILL, dtype=torch.uint8, device=DEV)
    minmax = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    kw = {}
    if label is not None:
        kw = dict(label=_dev(label), label_rows=_dev(pil_nearest_table(H, Hr)), label_cols=_dev(pil_nearest_table(W, Wr)),
                  out_label=torch.full((Hr, Wr), FILL, dtype=torch.uint8, device=DEV))
    got = hip.image_ingest(_dev(frame), out, None if W == Wr else _dev(pil_bilinear_tables(W, Wr)),
                           None if H == Hr else _dev(pil_bilinear_tables(H, Hr)), scratch, standardize, minmax, **kw)
    assert got is out
    return out.cpu().numpy(), tuple(minmax.cpu().tolist()), (kw['out_label'].cpu().numpy() if kw else None)


# ---------------------------------------------------------------------------------------------- 1. ingest bits
@pytest.mark.parametrize('pair', range(7))
def test_ingest_has_pils_bits(pair):
    g = _gold()
    _, out_hw = _pairs()[pair]
    rgb, gray, lab = g[f'rgb_{pair}'], g[f'gray_{pair}'], g[f'lab_{pair}']
    for frame in (rgb, gray):
        got, mm, got_lab = _ingest(frame, out_hw, label=lab)
        want, want_mm = R.ingest(frame, out_hw)
        assert np.array_equal(want, g[f'bil_{pair}'])  # (the restatement and PIL's record agree: one reference)
        assert np.array_equal(got, want) and mm == want_mm, (pair, frame.shape, int((got != want).sum()))
        assert np.array_equal(got_lab, g[f'near_{pair}']) and np.array_equal(got_lab, R.resize_nearest(lab, out_hw))
        got, mm, _ = _ingest(frame, out_hw, standardize=True)
        want, want_mm = R.ingest(frame, out_hw, standardization=True)
        assert np.array_equal(got, want) and mm == want_mm, (pair, 'standardization')


def test_ingest_clips_and_covers_every_pixel_of_special_frames():
    g = _gold()
    out_hw = _pairs()[0][1]
    for k in range(3):  # all 0, all 255 (the clip), a checkerboard
        got, mm, _ = _ingest(g['special_in'][k], out_hw)
        assert np.array_equal(got, g['special_out'][k]) and mm == (int(got.min()), int(got.max())), k
    # more than one workgroup along a row, the last one partial; one output row
    rng = np.random.default_rng(4)
    wide = rng.integers(0, 256, (2, 300, 3), dtype=np.uint8)
    got, mm, _ = _ingest(wide, (1, 290))
    assert np.array_equal(got, R.ingest(wide, (1, 290))[0])
    # a gray frame whose size stays: both passes skipped, the slot is the frame
    same = rng.integers(0, 256, (9, 7), dtype=np.uint8)
    got, mm, _ = _ingest(same, (9, 7))
    assert np.array_equal(got, same) and mm == (int(same.min()), int(same.max()))


def test_the_stretch_of_a_17_to_203_frame_and_of_a_constant_frame():
    (H, W), out_hw = _pairs()[5]  # (64, 128) -> (16, 32)
    frame = np.random.default_rng(8).integers(17, 204, (H, W), dtype=np.uint8)
    frame[:16, :16], frame[-16:, -16:] = 17, 203  # (flat blocks larger than a window: the resized frame keeps both extremes)
    plain, mm = R.ingest(frame, out_hw)
    assert mm == (17, 203)
    got, got_mm, _ = _ingest(frame, out_hw, standardize=True)
    want = (255.0 * (plain - np.min(plain)) / (np.max(plain) - np.min(plain))).astype('uint8')  # (the loader's own expression)
    assert np.array_equal(got, want) and got_mm == (17, 203) and got.min() == 0 and got.max() == 255
    for frame in (np.full((H, W), 77, np.uint8), np.full((H, W, 3), 255, np.uint8)):
        got, got_mm, _ = _ingest(frame, out_hw, standardize=True)
        assert not got.any() and got_mm[0] == got_mm[1] == int(frame.flat[0])  # (the deviation: a constant frame becomes all 0)


# ---------------------------------------------------------------------------------------------- 2. the store
def test_five_frames_through_two_staging_sets_and_the_sixth_refused():
    from ess_amd import hip
    from ess_amd.datasets.image_store import ImageStore
    (H, W), out_hw = (37, 53), (16, 24)
    rng = np.random.default_rng(21)
    frames = [rng.integers(10 * k, 120 + 20 * k, (H, W, 3), dtype=np.uint8) if k != 2 else rng.integers(0, 256, (H, W), dtype=np.uint8)
              for k in range(5)]  # (RGB frames of different ranges and one gray frame)
    labels = [rng.integers(0, 34, (H, W), dtype=np.uint8) for _ in range(5)]
    for standardization in (False, True):
        store = ImageStore(5, resize_hw=out_hw, source_hw=(H, W), standardization=standardization, staging_images=2)
        assert store.add_images(frames[:1], labels[:1]) == [0]
        assert store.add_images(frames[1:], labels[1:]) == [1, 2, 3, 4] and store.n_images == 5
        images, labs, mms = store.images.cpu().numpy(), store.labels.cpu().numpy(), store.minmax.cpu().numpy()
        for k in range(5):
            want, mm = R.ingest(frames[k], out_hw, standardization)
            assert np.array_equal(images[k], want) and tuple(mms[k]) == mm, (k, standardization)
            assert np.array_equal(labs[k], R.resize_nearest(labels[k], out_hw)), k
        assert len({tuple(m) for m in mms}) == 5  # (each slot with its own min / max)
        with pytest.raises(hip.EssHipError, match='the store is full: 5 \\+ 1 frames'):
            store.add_images(frames[:1], labels[:1])
        assert store.n_images == 5 and np.array_equal(store.images.cpu().numpy(), images) and np.array_equal(store.labels.cpu().numpy(), labs)


# ---------------------------------------------------------------------------------------------- 3. the fused source
N_SLOTS, HR, WR, ROWS = 5, 12, 20, 9
INDEX = [4, 4, 0, 2, 1, 4, 3, 0]  # (repeated indices and the last slot)


@functools.lru_cache(maxsize=None)
def _slots():
    rng = np.random.default_rng(31)
    return _dev(rng.integers(0, 256, (N_SLOTS, HR, WR), dtype=np.uint8)), _dev(rng.integers(0, 34, (N_SLOTS, HR, WR), dtype=np.uint8))


@pytest.mark.parametrize('out_hw', [(11, 16), (7, 24)], ids=['pad rows, crop columns', 'crop rows, pad columns'])
@pytest.mark.parametrize('augment', [True, False], ids=['drawn', 'centre crop'])
@pytest.mark.parametrize('labelled', [True, False], ids=['labels', 'no labels'])
def test_the_fused_source_has_the_bits_of_the_float_entry_point_on_gathered_slots(labelled, augment, out_hw):
    from ess_amd import hip
    from ess_amd.datasets.augment import draw_params
    from ess_amd.datasets.image_store import cityscapes_id_lut
    images, labels = _slots()
    H, W = out_hw
    B = len(INDEX)
    p = draw_params(B, (ROWS, WR), out_hw, 0.1, torch.Generator().manual_seed(0), augment)
    if augment:
        assert p[:, 0].any() and not p[:, 0].all() and (p[:, 1] > 1).any() and (p[:, 10] > 0).any()  # (flips, scales and noise fire)
    params = p.to(DEV)
    index = torch.tensor(INDEX, dtype=torch.int32, device=DEV)
    lut = cityscapes_id_lut(6).to(DEV)
    gathered = images[index.long()][:, :ROWS].float().contiguous()
    gathered_l = labels[index.long()][:, :ROWS].long().contiguous() if labelled else None
    for table in (lut, None):
        want, want_l = hip.augment_image_label(gathered, gathered_l, params, H, W, table)
        out = (torch.full((B, 1, H, W), -3.0, device=DEV), torch.full((B, H, W), -3, dtype=torch.int64, device=DEV) if labelled else None)
        got, got_l = hip.augment_image_label_store(images, labels if labelled else None, index, ROWS, params, H, W, table, out=out)
        assert got is out[0] and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert (got_l is None and want_l is None) if not labelled else torch.equal(got_l, want_l)
        fresh, fresh_l = hip.augment_image_label_store(images, labels if labelled else None, index, ROWS, params, H, W, table)
        assert torch.equal(fresh, got) and (not labelled or torch.equal(fresh_l, got_l))
    assert bool(want.any())
    # a word outside the slots: an all-zero sample, its neighbours untouched
    bad = index.clone()
    bad[1], bad[6] = N_SLOTS, -1
    got, got_l = hip.augment_image_label_store(images, labels if labelled else None, bad, ROWS, params, H, W, None)
    keep = [b for b in range(B) if b not in (1, 6)]
    assert torch.equal(got[keep], want[keep])
    if not augment:
        assert not got[[1, 6]].any() and (not labelled or not got_l[[1, 6]].any())


# ---------------------------------------------------------------------------------------------- 4. the builder
@functools.lru_cache(maxsize=None)
def _small_store():
    from ess_amd.datasets.image_store import ImageStore
    rng = np.random.default_rng(41)
    store = ImageStore(6, resize_hw=(12, 20), source_hw=(24, 40))
    store.add_images([rng.integers(0, 256, (24, 40, 3), dtype=np.uint8) for _ in range(6)],
                     [rng.integers(0, 34, (24, 40), dtype=np.uint8) for _ in range(6)])
    return store


BATCHES = ([5, 0, 3], [1, 1, 5], [2, 4, 0])


@pytest.mark.parametrize('augmentation', [True, False], ids=['augmented', 'centre crop'])
def test_the_builder_eager_equals_its_graph_and_the_composition_it_replaces(augmentation):
    from ess_amd import hip
    from ess_amd.datasets.image_store import ImageBatchBuilder, cityscapes_id_lut
    store = _small_store()
    H, W = 8, 16
    eager = ImageBatchBuilder(store, H, W, augmentation=augmentation, seed=5)
    graph = ImageBatchBuilder(store, H, W, augmentation=augmentation, seed=5, graph=True)
    lut = cityscapes_id_lut(6)
    allowed = set(lut[:34].tolist())
    kept = []
    for indices in BATCHES:
        img, lab = eager.build(indices)
        img_g, lab_g = graph.build(np.array(indices))
        assert tuple(img.shape) == (3, 1, H, W) and img.dtype == torch.float32 and tuple(lab.shape) == (3, H, W) and lab.dtype == torch.int64
        assert torch.equal(img.view(torch.int32), img_g.view(torch.int32)) and torch.equal(lab, lab_g), indices
        assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0 and bool(img.any())
        assert set(lab.unique().tolist()) <= allowed  # (the trainId table's range: 0 .. 5 and 255)
        # -- the composition: index_select + .float() + the two-stage entry points, with the rows the builder drew
        p1, p2 = eager.last_params
        assert all(torch.equal(a, b) for a, b in zip(eager.last_params, graph.last_params) if a is not None)
        idx = torch.tensor(indices, device=DEV)
        src, src_l = store.images[idx][:, :eager.rows].float().contiguous(), store.labels[idx][:, :eager.rows].long().contiguous()
        if augmentation:
            mid, mid_l = hip.augment_image_label(src, src_l, p1.to(DEV), H, W, None)
            want, want_l = hip.augment_perspective_filter(mid, mid_l, p2.to(DEV), lut.to(DEV))
        else:
            want, want_l = hip.augment_image_label(src, src_l, p1.to(DEV), H, W, lut.to(DEV))
        assert torch.equal(img.view(torch.int32), want.view(torch.int32)) and torch.equal(lab, want_l), indices
        kept.append((img, lab, want.clone(), want_l.clone()))
    assert graph.n_captures == 2 and graph.n_batches == 3  # (one capture per output set: new indices and parameters need none)
    # a batch stays valid until the one after the next is built: the second and third are still what they were
    for img, lab, want, want_l in kept[1:]:
        assert torch.equal(img, want) and torch.equal(lab, want_l)
    assert eager.rows == 8 and eager.shift_limit == 0.0


# ---------------------------------------------------------------------------------------------- 5. the paired loader and one UDA step
def test_a_paired_loader_over_both_stores_serves_one_uda_train_step():
    from ess_amd.config.settings import synthetic_settings
    from ess_amd.datasets.event_batches import EventBatchBuilder, EventBatchLoader
    from ess_amd.datasets.event_store import EventStore, StoreSample, StoreSampler
    from ess_amd.datasets.image_store import ImageBatchBuilder, ImageBatchLoader, ImageSampler, ImageStore, PairedBatchLoader
    from ess_amd.training.ess_trainer import ESSModel
    from tests import test_hip_event_columns as C
    from tests import test_host_event_ingest as EV
    B, T, Cb, H, W, K = 1, 2, 2, 32, 48, 6  # (the size of the repository's smoke run)
    rng = np.random.default_rng(3)
    images = ImageStore(3, resize_hw=(40, 48), source_hw=(80, 96))
    images.add_images([rng.integers(0, 256, (80, 96, 3), dtype=np.uint8) for _ in range(3)],
                      [rng.integers(0, 34, (80, 96), dtype=np.uint8) for _ in range(3)])
    loader_a = ImageBatchLoader(ImageSampler(images, B, shuffle=False), ImageBatchBuilder(images, H, W, semseg_num_classes=K, seed=2, graph=True))
    label = rng.integers(0, K, (H, W)).astype(np.uint8)
    label[:2] = 255
    events = EventStore(4096, label_hw=(H, W), label_capacity=1)
    events.add_recording(C._as_columns(EV.events(4000, H, W, 5), 1), labels=label[None])
    builder_b = EventBatchBuilder(B, T, Cb, None, store=events, window_events=2000, grid_hw=(H, W), height=H, width=W, label_hw=(H, W),
                                  grid_normalize='unbiased', seed=9)
    loader_b = EventBatchLoader(StoreSampler(events, B, [StoreSample(0, end=4000, label=0)], shuffle=False), builder_b)
    paired = PairedBatchLoader(loader_a, loader_b)
    assert len(paired) == 3  # (the image side is the longer one; the event side restarts)
    tr = ESSModel(synthetic_settings('ess', 'DSEC_events', (H, W), K, B, T, Cb))
    tr.train_loader = paired
    tr.train_loader.createIterators()
    n = 0
    for batch in tr.train_loader:
        (img, lab_a), (ev, lab_b) = batch
        assert all(t.device == DEV for t in (img, lab_a, ev, lab_b))
        assert tuple(img.shape) == (B, 1, H, W) and tuple(lab_a.shape) == (B, H, W) and lab_a.dtype == torch.int64
        assert tuple(ev.shape) == (B, T * Cb, H, W) and tuple(lab_b.shape) == (B, H, W) and bool(ev.any()) and bool(img.any())
        assert set(lab_a.unique().tolist()) <= set(range(K)) | {255}
        if n == 0:
            _, _, final = tr.train_step(batch)
            assert bool(torch.isfinite(final.detach()))
        n += 1
    assert n == 3
