"""GPU tier of the paired camera frames: hip.image_ingest_frame and hip.image_gather_unit against the numpy restatement
(tests/frame_store_ref.py, which tests/test_host_frame_store.py pins to PIL), the two frame-store presets at full size against PIL
itself where it is installed, EventBatchBuilder(frames=, original_labels=) against the same builder without frames, and one validation
step of the supervised trainer whose panel shows the frame.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import frame_store_ref as R  # noqa: E402

DEV = torch.device('cuda:0')
POISON = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(shape, out_hw, resample='bicubic'):
    from ess_amd.datasets.image_store import pil_resize_tables
    (H, W), (Hr, Wr) = shape[:2], out_hw
    return (None if W == Wr else _dev(pil_resize_tables(W, Wr, resample)), None if H == Hr else _dev(pil_resize_tables(H, Hr, resample)))


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.uint8, device=DEV)


# ---------------------------------------------------------------------------------------------- 1. the ingest of one frame
INGEST = {  # name: (source shape, (Hr, Wr), out_rows or None)
    'both shrink, two workgroups a row': ((37, 300, 3), (29, 277), None),
    'gray, both grow': ((23, 41), (31, 59), None),
    'width unchanged': ((30, 64, 3), (28, 64), None),
    'height unchanged': ((30, 64, 3), (30, 50), None),
    'the DDD17 form': ((26, 35), (26, 36), 20),
    'gray conversion only': ((30, 64, 3), (30, 64), None),
    'rgb, rows cut behind a vertical pass': ((37, 53, 3), (29, 41), 11),
}


@pytest.mark.parametrize('name', list(INGEST))
def test_a_frame_has_the_restatements_bits(name):
    from ess_amd import hip
    shape, (Hr, Wr), rows = INGEST[name]
    rows = Hr if rows is None else rows
    img = R.make_image(shape, 11 + len(name))
    ht, vt = _tables(shape, (Hr, Wr))
    big = _poison(rows + 3, Wr)  # (a larger allocation: the rows behind out_rows must stay as they are)
    rgb = len(shape) == 3
    scratch = _poison(shape[0], Wr, 3) if rgb else _poison(shape[0], Wr)
    out = hip.image_ingest_frame(_dev(img), big[:rows], ht, vt, scratch if ht is not None else None, resized_rows=Hr)
    want = R.frame(img, (Hr, Wr), keep_rows=rows)
    assert out.data_ptr() == big.data_ptr() and np.array_equal(big[:rows].cpu().numpy(), want), name
    assert bool((big[rows:] == POISON).all()), name
    if ht is not None:  # (the horizontal pass ran on the source rows the kept rows read, and on no other)
        read = shape[0] if vt is None else int(vt[0, rows - 1] + vt[1, rows - 1])
        read = rows if vt is None else read
        mid = R.resize(img, (shape[0], Wr))
        assert np.array_equal(scratch[:read].cpu().numpy(), mid[:read]) and bool((scratch[read:] == POISON).all()), (name, read)
    assert (want == 0).any() and (want == 255).any()  # (the clip was reached on both sides)


def test_gray_first_equals_image_ingest_on_the_same_tables():
    from ess_amd import hip
    shape, (Hr, Wr) = (37, 53, 3), (29, 41)
    img = _dev(R.make_image(shape, 4))
    ht, vt = _tables(shape, (Hr, Wr))
    a = hip.image_ingest_frame(img, _poison(Hr, Wr), ht, vt, _poison(shape[0], Wr), gray_last=False)
    b = hip.image_ingest(img, _poison(Hr, Wr), ht, vt, _poison(shape[0], Wr))
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), R.frame(img.cpu().numpy(), (Hr, Wr), gray_last=False))
    assert not torch.equal(a, hip.image_ingest_frame(img, _poison(Hr, Wr), ht, vt))  # (the order shows)


# ---------------------------------------------------------------------------------------------- 2. the unit gather
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64], ids=['int32', 'int64'])
def test_the_unit_gather_has_the_bits_of_totensor(dtype):
    from ess_amd import hip
    g = np.random.default_rng(8)
    slots = g.integers(0, 256, (7, 20, 36), dtype=np.uint8)
    slots[2].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)  # (every byte value)
    index = [2, 6, 2, -1, 7]  # (a repeated slot, and two outside the store: zero frames)
    out = torch.full((5, 1, 20, 36), float('nan'), device=DEV)
    got = hip.image_gather_unit(_dev(slots), torch.tensor(index, dtype=dtype, device=DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    cpu = torch.from_numpy(slots).float().div(255)  # (transforms.ToTensor() on the host)
    want = torch.stack([cpu[i] if 0 <= i < 7 else torch.zeros(20, 36) for i in index]).unsqueeze(1)
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), R.gather_unit(slots, index).view(np.uint32))
    odd = g.integers(0, 256, (2, 5, 7), dtype=np.uint8)  # (a slot size that is no multiple of anything)
    got = hip.image_gather_unit(_dev(odd), torch.tensor([1], dtype=dtype, device=DEV))
    assert torch.equal(got.cpu(), torch.from_numpy(odd[1:2]).float().div(255).unsqueeze(1))


# ---------------------------------------------------------------------------------------------- 3. the presets at full size
def _expected(img, out_hw, keep_rows=None):
    """PIL itself where it is installed (the loaders' calls), the restatement otherwise"""
    try:
        from PIL import Image
    except ImportError:
        return R.frame(img, out_hw, keep_rows=keep_rows)
    r = Image.fromarray(img)
    if out_hw is not None:
        r = r.resize((out_hw[1], out_hw[0]))
    r = np.array(r.convert('L') if img.ndim == 3 else r)
    return r if keep_rows is None else r[:keep_rows]


def test_the_presets_at_full_size():
    from ess_amd import hip
    from ess_amd.datasets.image_store import ImageStore
    ddd = ImageStore.ddd17_frames(3)
    frames = [R.make_image((260, 346), 21), R.make_image((260, 346, 3), 22)]  # (a gray and an RGB frame in one call)
    assert ddd.add_images(frames) == [0, 1] and ddd.has_labels is False and ddd.labels is None
    assert tuple(ddd.images.shape) == (3, 200, 352)
    for k, f in enumerate(frames):
        assert np.array_equal(ddd.images[k].cpu().numpy(), _expected(f, (260, 352), 200)), k
    assert not bool(ddd.images[2].any())
    with pytest.raises(hip.EssHipError, match='keeps no labels'):
        ddd.add_images([frames[0]], labels=[np.zeros((260, 346), np.uint8)])
    assert ddd.n_images == 2
    dsec = ImageStore.dsec_frames(2)
    frames = [R.make_image((480, 640, 3), 23), R.make_image((480, 640, 3), 24)]
    assert dsec.add_images(frames) == [0, 1] and tuple(dsec.images.shape) == (2, 448, 640)
    for k, f in enumerate(frames):
        assert np.array_equal(dsec.images[k].cpu().numpy(), _expected(f, (448, 640))), k
    raw = ImageStore.dsec_frames(1, resize=False)
    assert raw.add_images(frames[:1]) == [0] and np.array_equal(raw.images[0].cpu().numpy(), _expected(frames[0], None))


# ---------------------------------------------------------------------------------------------- 4. batches
T, N_WIN = 2, 700
SENSOR = {'ddd17': dict(hw=(260, 346), label_hw=(200, 346), slot=(200, 352)), 'dsec': dict(hw=(480, 640), label_hw=(440, 640), slot=(448, 640))}


@functools.lru_cache(maxsize=None)
def _stores(kind):
    """an event store of two recordings (a few thousand events, four labels) and a frame store of four frames"""
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.event_store import EventStore
    from ess_amd.datasets.image_store import ImageStore
    geo = SENSOR[kind]
    H, W = geo['hw']
    g = np.random.default_rng(31)
    store = EventStore(6000, label_hw=geo['label_hw'], label_capacity=4)
    labels = g.integers(0, 6, (4,) + geo['label_hw'], dtype=np.uint8)
    for k, n in enumerate((3000, 2500)):
        t = np.cumsum(g.integers(0, 3, n)).astype(np.int64)
        c = EventColumns(t, g.integers(0, W, n).astype(np.int16), g.integers(0, H, n).astype(np.int16), g.integers(0, 2, n).astype(np.uint8))
        assert store.add_recording(c, labels=labels[2 * k:2 * k + 2]) == k
    frames = ImageStore.ddd17_frames(4) if kind == 'ddd17' else ImageStore.dsec_frames(4)
    frames.add_images([R.make_image((H, W, 3), 40 + k) for k in range(4)])
    return store, frames, labels


def _samples(k, with_frames):
    from ess_amd.datasets.event_store import StoreSample as S
    rows = [[(0, 2900, 0, 3), (1, 2400, 2, 1)], [(1, 1500, 3, 2), (0, 1400, 1, 2)], [(0, 2000, 1, 0), (0, 2999, 0, 3)]][k]
    return [S(r, end=e, label=lab, frame=f if with_frames else None) for r, e, lab, f in rows]


@pytest.mark.parametrize('kind', ['ddd17', 'dsec'])
def test_a_batch_with_frames(kind):
    from ess_amd.datasets.event_batches import EventBatchBuilder
    store, frames, labels = _stores(kind)
    make = getattr(EventBatchBuilder, kind)
    extra = dict(original_labels=True, augmentation=False) if kind == 'ddd17' else {}
    common = dict(sequence_steps=T, store=store, window_events=N_WIN, seed=5)
    plain = make(2, augmentation=kind != 'ddd17', **common)
    eager, graph = make(2, frames=frames, **common, **extra), make(2, frames=frames, graph=True, **common, **extra)
    slots = frames.images.cpu()
    for k in range(3):  # (three builds: both output sets, and the first set again)
        params = None
        if kind == 'dsec':
            params = torch.tensor([[1, 0, 0, 0], [k & 1, 0, 0, 0]], dtype=torch.int32)  # (flip = 1 forced)
        want_ev, want_lab = plain.build(_samples(k, False), params=params)
        got, rep = eager.build(_samples(k, True), params=params), graph.build(_samples(k, True), params=params)
        assert len(got) == len(rep) == (4 if kind == 'ddd17' else 3)
        for batch in (got, rep):
            ev, img, lab = batch[:3]
            assert torch.equal(ev.view(torch.int32), want_ev.view(torch.int32)) and torch.equal(lab, want_lab), (kind, k)
            assert img.dtype == torch.float32 and tuple(img.shape) == (2, 1) + SENSOR[kind]['slot']
            index = [s.frame for s in _samples(k, True)]
            want = slots[index].float().div(255).unsqueeze(1)  # (neither flipped nor cropped)
            assert torch.equal(img.cpu().view(torch.int32), want.view(torch.int32)), (kind, k)
            if kind == 'ddd17':
                orig = batch[3]
                assert orig.dtype == torch.int64 and torch.equal(orig.cpu(), torch.from_numpy(labels[[s.label for s in _samples(k, True)]]).long())
        if kind == 'dsec':  # (the flip reached the events and the label, and the frame is not symmetric)
            unflipped = plain.build(_samples(k, False), params=torch.zeros(2, 4, dtype=torch.int32))[1]
            assert torch.equal(want_lab[0], unflipped[0].flip(-1)) and not torch.equal(got[1][0], got[1][0].flip(-1))
    assert graph.n_captures == 2 and eager.n_captures == 0 and eager.n_batches == 3


# ---------------------------------------------------------------------------------------------- 5. the trainer's panel
def test_a_validation_panel_shows_the_paired_frame():
    from ess_amd import hip
    from ess_amd.config.settings import synthetic_settings
    from ess_amd.datasets.image_store import ImageStore
    from ess_amd.training.ess_supervised_trainer import ESSSupervisedModel
    H, W, K, B = 32, 48, 6, 2
    st = synthetic_settings('ess_supervised', 'DSEC_events', (H, W), K, B, 2, 4, train_on_event_labels=True, val_steps=2)
    tr = ESSSupervisedModel(st)
    tr.vis_panels = True
    ev, lab = next(iter(tr.val_loader_sensor_b))[:2]
    ev, lab = ev.to(DEV), lab.to(DEV)
    tr.val_step([ev, lab], 'sensor_b', vis_reconstr_idx=0)
    tag = 'val_events/reconst_input_events_0'
    without = tr.last_val_panels[tag].clone()
    frames = ImageStore(B, resize_hw=None, source_hw=(H, W), gray='last')
    frames.add_images([R.make_image((H, W, 3), 60 + k) for k in range(B)])
    paired = hip.image_gather_unit(frames.images, torch.tensor([1, 0], dtype=torch.int32, device=DEV))
    tr.settings.require_paired_data_val_b = True
    try:
        tr.val_step([ev, paired, lab], 'sensor_b', vis_reconstr_idx=0)
    finally:
        tr.settings.require_paired_data_val_b = False
    panel = tr.last_val_panels[tag]
    # four rows of B tiles without the frame, five with it: two more tiles, a grid row more at four tiles a row
    assert tuple(without.shape) == (3, 2 * (H + 2) + 2, 4 * (W + 2) + 2) and tuple(panel.shape) == (3, 3 * (H + 2) + 2, 4 * (W + 2) + 2)
    assert torch.equal(panel[:, :without.shape[1] - 2], without[:, :without.shape[1] - 2])  # (the other columns are unchanged)
    for j in range(B):
        k = 4 * B + j
        y, x = 2 + (k // 4) * (H + 2), 2 + (k % 4) * (W + 2)
        tile = panel[:, y:y + H, x:x + W]
        assert torch.equal(tile, paired[j].expand(3, H, W)), j
