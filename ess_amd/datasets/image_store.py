"""The device image store: source frames uploaded ONCE and resized as PIL resizes them, training batches cut on the device.

The image counterpart of datasets/event_store.py.  The reference's Cityscapes loader (datasets/cityscapes_loader.py) hands the
albumentations pipeline a gray uint8 image that went through transforms.Grayscale(), transforms.Resize([256, 512]) -- on a PIL image:
PIL's antialiased bilinear resize --, the label through label.resize(..., Image.NEAREST), optionally the `standardization` stretch,
and under random_crop the img[:height] cut.  DeviceAugmentation (datasets/augment.py) begins behind all that, with a float image of
the resize size on the device.  An ImageStore is the front: hip.image_ingest takes a decoded frame to a uint8 [Hr, Wr] slot (and its
label to a uint8 label-id slot) in PIL's own integer arithmetic, and ImageBatchBuilder cuts a batch out of the slots: stage 1 of the
augmentation reads them through a device index (hip.augment_image_label_store, no float copy of the source), stage 2 is
hip.augment_perspective_filter as before.

PINNED to PIL itself, bit for bit (tests/test_host_image_store.py compares with the installed PIL and with PIL's recorded outputs):
convert('L'), Image.resize(BILINEAR) on mode L, Image.resize(NEAREST).  The coefficient tables of the bilinear resize and the index
tables of the nearest one are built HERE, on the host, in float64 (pil_bilinear_tables, pil_nearest_table); the kernels multiply and
add int32.  NOT pinned, as before: the albumentations half (datasets/augment.py says what is restated there).

Deviation: the reference's stretch divides by zero on a constant frame (numpy: NaN -> an undefined uint8); here such a frame becomes
all 0.  A.Normalize is constructed by the reference and never applied: it has no counterpart.

The PAIRED CAMERA FRAMES of the event loaders (DSEC/dataset/sequence.py:166-176, datasets/ddd17_events_loader.py:187-213) go through
the same store with other settings -- Image.resize's default filter (bicubic) on the RGB image, the gray conversion behind it, the
top rows kept: pil_resize_tables, hip.image_ingest_frame, ImageStore(resample=, gray=, keep_rows=), pinned to PIL in the same way
(tests/test_host_frame_store.py) -- and reach a batch through EventBatchBuilder(frames=) (datasets/event_batches.py).

File readers (png) stay outside: a frame arrives as a uint8 array.  Numpy and torch only."""
import math

import numpy as np
import torch

from .. import hip
from .augment import draw_params, draw_params2

PRECISION_BITS = 22  # PIL's 8-bit resize: 32 - 8 - 2


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _pair(what, v):
    if not isinstance(v, (tuple, list)) or len(v) != 2 or any(not _is_int(a) or a < 1 for a in v):
        raise hip.EssHipError(f'{what}={v!r}: a pair of positive ints is needed')
    return int(v[0]), int(v[1])


# ---------------------------------------------------------------------------------------------- PIL's tables, on the host
def pil_bilinear_tables(n_in, n_out):
    """The windows and fixed-point coefficients of PIL's Image.resize(BILINEAR) on an 8-bit image along one axis n_in -> n_out ->
    int32 [2 + ksize, n_out]: row 0 the first input index of an output index's window, row 1 its length (<= ksize), rows 2.. the
    coefficients k_i = int(0.5 + w_i 2^22), 0 behind the window; ksize = 2 ceil(max(n_in / n_out, 1)) + 1.  Per output index xx, in
    float64 and in PIL's order of operations: scale = n_in / n_out, fs = max(scale, 1), center = (xx + 0.5) scale,
    xmin = max(int(center - fs + 0.5), 0), xmax = min(int(center + fs + 0.5), n_in), w_i = max(0, 1 - |(i + xmin - center + 0.5) / fs|)
    normalised by their sum accumulated in order.  The pixel is clip8((2^21 + sum k_i p_i) >> 22).  Refused: a ksize above
    hip.IMAGE_MAX_TAPS (a side shrinking by more than 16)."""
    for name, v in (('n_in', n_in), ('n_out', n_out)):
        if not _is_int(v) or not 1 <= v <= hip.IMAGE_MAX_SIDE:
            raise hip.EssHipError(f'pil_bilinear_tables: {name}={v!r} must be an int in [1, {hip.IMAGE_MAX_SIDE}]')
    n_in, n_out = int(n_in), int(n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    if ksize > hip.IMAGE_MAX_TAPS:
        raise hip.EssHipError(f'pil_bilinear_tables: {n_in} -> {n_out} needs windows of {ksize} coefficients, the kernels hold '
                              f'{hip.IMAGE_MAX_TAPS}: a side shrinks by at most {hip.IMAGE_MAX_TAPS // 2}')
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    count = xmax - xmin
    w = np.zeros((ksize, n_out), dtype=np.float64)
    ww = np.zeros(n_out, dtype=np.float64)
    for i in range(ksize):
        live = i < count
        wi = np.maximum(0.0, 1.0 - np.abs(((i + xmin).astype(np.float64) - center + 0.5) / fs))
        w[i] = np.where(live, wi, 0.0)
        ww = np.where(live, ww + w[i], ww)  # (accumulated in order, as PIL accumulates it)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)
    return np.ascontiguousarray(np.concatenate([xmin[None], count[None], k]).astype(np.int32))


RESAMPLE = ('bilinear', 'bicubic')


def _bicubic(x):
    """PIL's bicubic filter (Keys' kernel, a = -0.5, support 2) on a float64 array, in PIL's order of operations"""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def pil_resize_tables(n_in, n_out, resample='bilinear'):
    """pil_bilinear_tables for either filter of PIL's 8-bit Image.resize: resample='bilinear' is that function itself, 'bicubic' (the
    default of Image.resize on an 'RGB' or 'L' image where the reference's event loaders call it without a filter) has the same
    int32 [2 + ksize, n_out] layout and window rule with the support doubled -- support = 2 max(n_in / n_out, 1),
    ksize = 2 ceil(support) + 1 --, the weight ((a + 2)|x| - (a + 3)) x^2 + 1 below 1, (((|x| - 5)|x| + 8)|x| - 4) a below 2, a = -0.5,
    at x = (i + xmin - center + 0.5) (1 / max(n_in / n_out, 1)), normalised by the sum accumulated in order.  A coefficient is rounded
    AWAY from zero, as PIL rounds it: int(0.5 + w 2^22) for w >= 0, int(-0.5 + w 2^22) for w < 0.  Refused: a ksize above
    hip.IMAGE_MAX_TAPS (bicubic: a side shrinking by more than 8)."""
    if not isinstance(resample, str) or resample not in RESAMPLE:
        raise hip.EssHipError(f'pil_resize_tables: resample={resample!r}: one of {RESAMPLE}')
    if resample == 'bilinear':
        return pil_bilinear_tables(n_in, n_out)
    for name, v in (('n_in', n_in), ('n_out', n_out)):
        if not _is_int(v) or not 1 <= v <= hip.IMAGE_MAX_SIDE:
            raise hip.EssHipError(f'pil_resize_tables: {name}={v!r} must be an int in [1, {hip.IMAGE_MAX_SIDE}]')
    n_in, n_out = int(n_in), int(n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    if ksize > hip.IMAGE_MAX_TAPS:
        raise hip.EssHipError(f'pil_resize_tables: {n_in} -> {n_out} needs bicubic windows of {ksize} coefficients, the kernels hold '
                              f'{hip.IMAGE_MAX_TAPS}: a side shrinks by at most {hip.IMAGE_MAX_TAPS // 4}')
    ss = 1.0 / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in)
    count = xmax - xmin
    w = np.zeros((ksize, n_out), dtype=np.float64)
    ww = np.zeros(n_out, dtype=np.float64)
    for i in range(ksize):
        live = i < count
        w[i] = np.where(live, _bicubic(((i + xmin).astype(np.float64) - center + 0.5) * ss), 0.0)
        ww = np.where(live, ww + w[i], ww)  # (accumulated in order, as PIL accumulates it)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.trunc(np.where(w < 0.0, -0.5, 0.5) + w * float(1 << PRECISION_BITS)).astype(np.int64)
    # (the kernels add in int32: 2^21 + sum |k| 255 stays below 2^31 while sum |w| < 2, and bicubic's is at most about 1.3)
    if int(np.abs(k).sum(axis=0).max()) * 255 + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise hip.EssHipError(f'pil_resize_tables: {n_in} -> {n_out}: a window\'s coefficients overflow the kernels\' int32 sums')
    return np.ascontiguousarray(np.concatenate([xmin[None], count[None], k]).astype(np.int32))


def pil_nearest_table(n_in, n_out):
    """The source index of every output index of PIL's Image.resize(NEAREST) along one axis -> int32 [n_out]: min(int(xo), n_in - 1)
    with xo starting at 0.5 n_in / n_out and advanced by repeated float64 ADDITION of n_in / n_out -- a running sum, which differs
    from the product (xx + 0.5) n_in / n_out at ratios float64 does not represent (2048 / 352)."""
    for name, v in (('n_in', n_in), ('n_out', n_out)):
        if not _is_int(v) or not 1 <= v <= hip.IMAGE_MAX_SIDE:
            raise hip.EssHipError(f'pil_nearest_table: {name}={v!r} must be an int in [1, {hip.IMAGE_MAX_SIDE}]')
    step = float(n_in) / float(n_out)
    xo = 0.5 * step
    out = np.empty(int(n_out), dtype=np.int32)
    for x in range(int(n_out)):
        out[x] = min(int(xo), int(n_in) - 1)
        xo += step
    return out


_TRAIN_IDS = {  # trainId of the Cityscapes ids 0 .. 33 in the reference's 6- and 11-class tables (utils/labels.py); other ids stay
    6: [255] * 7 + [0, 0, 255, 255, 1, 1, 1, 255, 255, 255, 2, 255, 2, 2, 3, 3, 1, 4, 4, 5, 5, 5, 255, 255, 5, 5, 5],
    11: [255] * 7 + [5, 6, 255, 255, 1, 9, 2, 255, 255, 255, 4, 255, 10, 10, 7, 7, 0, 3, 3, 8, 8, 8, 255, 255, 8, 8, 8],
}


def cityscapes_id_lut(semseg_num_classes):
    """the id -> trainId table of fromIdToTrainId (utils/labels.py:123-127) as int64 [256]: ids 0 .. 33 by the 6- or 11-class table,
    every other id unchanged (the reference rewrites only the ids its table names)"""
    if semseg_num_classes not in _TRAIN_IDS:
        raise hip.EssHipError(f'semseg_num_classes={semseg_num_classes!r}: the Cityscapes tables have 6 or 11 classes')
    lut = torch.arange(256, dtype=torch.int64)
    lut[:34] = torch.tensor(_TRAIN_IDS[semseg_num_classes], dtype=torch.int64)
    return lut


# ---------------------------------------------------------------------------------------------- the store
class _FrameStage:
    """one staging set of an upload: a pinned frame and label, their device copies, the events behind the copy and behind the kernels"""
    __slots__ = ('host', 'host_np', 'dev', 'lab_host', 'lab_np', 'lab_dev', 'copied', 'consumed')

    def __init__(self, frame_shape, label_shape, device):
        self.host = torch.zeros(frame_shape, dtype=torch.uint8).pin_memory()
        self.host_np = self.host.numpy()
        self.dev = torch.zeros(frame_shape, dtype=torch.uint8, device=device)
        self.lab_host = torch.zeros(label_shape, dtype=torch.uint8).pin_memory()
        self.lab_np = self.lab_host.numpy()
        self.lab_dev = torch.zeros(label_shape, dtype=torch.uint8, device=device)
        self.copied, self.consumed = torch.cuda.Event(), torch.cuda.Event()


class ImageStore:
    """ImageStore(capacity_images, resize_hw=(256, 512), source_hw=(1024, 2048), standardization=False, staging_images=2, device=None,
               resample='bilinear', gray='first', keep_rows=None)

    add_images(frames, labels=None) -> the slot numbers.  frames: a list (or one array [n, ...]) of host uint8 frames, each
    [H, W, 3] RGB or [H, W] gray with (H, W) = source_hw; labels: None, or one host uint8 [H, W] label-id map per frame.  Every frame is
    uploaded ONCE and ends as a uint8 [Hr, Wr] slot (resize_hw) -- convert('L'), Image.resize(BILINEAR) and, with standardization, the
    loader's stretch, in PIL's integer arithmetic (hip.image_ingest) -- plus a uint8 label-id slot (Image.resize(NEAREST)).  Labels
    stay raw ids: the id -> trainId table is applied after the augmentation, as in the reference.  The first accepted call decides
    whether the store keeps labels; later calls follow it.  minmax[slot]: the resized frame's min and max before the stretch.

    An upload goes through staging_images (>= 2) staging sets, pinned and on the device: frame k + 1 is copied on a stream of its own
    while frame k's kernels run.  Refused with hip.EssHipError before a byte moves, the store left as it was: a wrong dtype or shape,
    a full store, labels for some frames but not others, labels where the store keeps none (or none where it keeps them).

    Device memory, allocated at the first accepted frame: Hr Wr bytes a slot, as much again with labels, 8 bytes a slot of min / max,
    the tables, the staging sets and an [H, Wr] scratch.  Cityscapes train, 2975 frames at 256 x 512 with labels: 0.78 GB.

    The PAIRED FRAMES of the event loaders (img_left of DSEC, img of DDD17's validation split) are resized otherwise, and three
    keywords say how; their defaults are the Cityscapes loader's.  resample='bilinear' | 'bicubic': the filter of Image.resize --
    called without one, as those loaders call it, PIL takes BICUBIC (pil_resize_tables).  gray='first' | 'last': convert('L') in front
    of the resize, or behind the resize of the RGB image (transforms.Grayscale() follows Image.resize there; the bits differ).
    keep_rows=n: a slot holds the top n rows of the resized frame, uint8 [n, Wr] (slot_hw).  resize_hw=None: no resize, the gray
    conversion alone.  A store with gray='last' or keep_rows is a FRAME store: its frames go through hip.image_ingest_frame, it keeps
    no labels (add_images(labels=...) is refused) and no min / max, and EventBatchBuilder(frames=) gathers its slots beside the events.
    standardization is refused with any of the three.  ImageStore.dsec_frames(capacity, resize=True) and
    ImageStore.ddd17_frames(capacity) are the two loaders' settings."""

    def __init__(self, capacity_images, resize_hw=(256, 512), source_hw=(1024, 2048), standardization=False, staging_images=2, device=None,
                 resample='bilinear', gray='first', keep_rows=None):
        if not _is_int(capacity_images) or not 1 <= capacity_images <= 1 << 24:
            raise hip.EssHipError(f'ImageStore: capacity_images={capacity_images!r} must be an int in [1, 2^24]')
        if not _is_int(staging_images) or not 2 <= staging_images <= 16:
            raise hip.EssHipError(f'ImageStore: staging_images={staging_images!r} must be an int in [2, 16]: one set copies while another is read')
        self.source_hw = _pair('ImageStore: source_hw', source_hw)
        self.resize_hw = self.source_hw if resize_hw is None else _pair('ImageStore: resize_hw', resize_hw)  # (None: no resize)
        (Hr, Wr), (H, W) = self.resize_hw, self.source_hw
        if not isinstance(resample, str) or resample not in RESAMPLE:
            raise hip.EssHipError(f'ImageStore: resample={resample!r}: one of {RESAMPLE}')
        if not isinstance(gray, str) or gray not in ('first', 'last'):
            raise hip.EssHipError(f"ImageStore: gray={gray!r}: 'first' (convert, then resize: the Cityscapes loader) or 'last' (resize the RGB "
                                  'image, then convert: the event loaders\' paired frame)')
        if keep_rows is not None and (not _is_int(keep_rows) or not 1 <= keep_rows <= Hr):
            raise hip.EssHipError(f'ImageStore: keep_rows={keep_rows!r}: the top rows of the {Hr} resized rows a slot holds, an int in [1, {Hr}]')
        # (a FRAME store -- the paired frames of an event loader -- goes through hip.image_ingest_frame and keeps no labels)
        self.resample, self.gray, self.keep_rows = resample, gray, None if keep_rows is None else int(keep_rows)
        self.frame_store = gray == 'last' or keep_rows is not None
        if standardization and (self.frame_store or resample != 'bilinear'):
            raise hip.EssHipError('ImageStore: standardization belongs to the Cityscapes loader: it is not applied with resample=, gray= or '
                                  'keep_rows= (the event loaders do not stretch their paired frames)')
        self.slot_hw = (Hr if keep_rows is None else int(keep_rows), Wr)
        # (the host tables of both passes and of the label: a size beyond the kernels' windows is refused here)
        self._tables = {
            'h': None if W == Wr else pil_resize_tables(W, Wr, resample), 'v': None if H == Hr else pil_resize_tables(H, Hr, resample),
            'rows': pil_nearest_table(H, Hr), 'cols': pil_nearest_table(W, Wr),
        }
        self.capacity, self.staging_images, self.standardization = int(capacity_images), int(staging_images), bool(standardization)
        self.device = torch.device(device) if device is not None else torch.device('cuda:0')
        self.n_images = 0
        self.has_labels = None  # (decided by the first accepted call)
        self._dev = None

    @classmethod
    def dsec_frames(cls, capacity_images, resize=True, **kw):
        """the DSEC loader's paired img_left (sequence.py:166-176): 480 x 640 RGB, with resize all 480 rows -> 448 x 640 by
        Image.resize's default filter (bicubic) -- the bottom 40 rows are NOT cut first, although the events' are --, then Grayscale"""
        return cls(capacity_images, resize_hw=(448, 640) if resize else None, source_hw=(480, 640), resample='bicubic', gray='last', **kw)

    @classmethod
    def ddd17_frames(cls, capacity_images, **kw):
        """the DDD17 loader's paired frame (ddd17_events_loader.py:187-213): 260 x 346 -> 260 x 352 by Image.resize's default filter
        (bicubic), Grayscale, and the top 200 rows (img_tensor[:, :-60, :])"""
        return cls(capacity_images, resize_hw=(260, 352), source_hw=(260, 346), resample='bicubic', gray='last', keep_rows=200, **kw)

    def bytes(self):
        """the device memory of the slots (allocated or not yet), labels included unless the store is known to keep none"""
        Hs, Ws = self.slot_hw
        return self.capacity * (Hs * Ws * (1 if self.has_labels is False or self.frame_store else 2) + 8)

    @property
    def images(self):
        """uint8 [capacity, Hr, Wr] ([capacity, keep_rows, Wr] with keep_rows)"""
        return self._device()['images']

    @property
    def labels(self):
        """uint8 [capacity, Hr, Wr] of raw label ids, or None"""
        return self._device()['labels']

    @property
    def minmax(self):
        """int32 [capacity, 2]: a slot's min and max before the stretch"""
        return self._device()['minmax']

    def _device(self):
        if self._dev is None:
            if self.has_labels is None:
                raise hip.EssHipError('ImageStore: the store is empty: its device tensors exist from the first accepted frame on')
            dev, (Hr, Wr), (H, W), (Hs, Ws) = self.device, self.resize_hw, self.source_hw, self.slot_hw
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
            self._dev = {
                'images': torch.zeros(self.capacity, Hs, Ws, dtype=torch.uint8, device=dev),
                'labels': torch.zeros(self.capacity, Hr, Wr, dtype=torch.uint8, device=dev) if self.has_labels else None,
                'minmax': torch.zeros(self.capacity, 2, dtype=torch.int32, device=dev),
                # (gray last: the horizontal pass leaves three channels)
                'scratch': torch.zeros((H, Wr, 3) if self.gray == 'last' else (H, Wr), dtype=torch.uint8, device=dev),
                'tables': {k: up(v) for k, v in self._tables.items()},
                'stage': {}, 'copy_stream': torch.cuda.Stream(device=dev), 'frames': 0,
            }
        return self._dev

    def _check_frames(self, frames, labels):
        H, W = self.source_hw
        if isinstance(frames, np.ndarray) and frames.ndim in (3, 4) and frames.shape[1:3] == (H, W):
            frames = list(frames)
        if torch.is_tensor(frames) or not isinstance(frames, (list, tuple)) or not frames:
            raise hip.EssHipError('ImageStore.add_images: frames must be a non-empty list of host uint8 arrays (or one array [n, H, W(, 3)])')
        out = []
        for k, f in enumerate(frames):
            if torch.is_tensor(f) and not f.is_cuda:
                f = f.numpy()
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.shape not in ((H, W), (H, W, 3)):
                got = f'{f.dtype}{tuple(f.shape)}' if hasattr(f, 'dtype') else type(f).__name__
                raise hip.EssHipError(f'ImageStore.add_images: frames[{k}] must be a host uint8 [{H}, {W}, 3] (RGB) or [{H}, {W}] (gray) array '
                                      f'(source_hw), got {got}')
            out.append(f)
        labs = None
        if labels is not None and self.frame_store:
            raise hip.EssHipError("ImageStore.add_images: a frame store (gray='last' or keep_rows) keeps no labels: the paired frame's label "
                                  'is the event sample\'s')
        if labels is not None:
            if isinstance(labels, np.ndarray) and labels.ndim == 3:
                labels = list(labels)
            if not isinstance(labels, (list, tuple)) or len(labels) != len(out):
                raise hip.EssHipError(f'ImageStore.add_images: labels must be None or a list of one label map per frame ({len(out)})')
            if any(g is None for g in labels):
                if all(g is None for g in labels):
                    labels = None
                else:
                    raise hip.EssHipError('ImageStore.add_images: a label for every frame of the call, or for none')
        if labels is not None:
            labs = []
            for k, g in enumerate(labels):
                if torch.is_tensor(g) and not g.is_cuda:
                    g = g.numpy()
                if not isinstance(g, np.ndarray) or g.dtype != np.uint8 or g.shape != (H, W):
                    got = f'{g.dtype}{tuple(g.shape)}' if hasattr(g, 'dtype') else type(g).__name__
                    raise hip.EssHipError(f'ImageStore.add_images: labels[{k}] must be a host uint8 [{H}, {W}] array of label ids, got {got}')
                labs.append(g)
        if self.has_labels is not None and self.has_labels != (labs is not None):
            raise hip.EssHipError('ImageStore.add_images: this store keeps ' + ('labels: every frame needs one' if self.has_labels else
                                                                                 'no labels: its first frames came without'))
        if self.n_images + len(out) > self.capacity:
            raise hip.EssHipError(f'ImageStore.add_images: the store is full: {self.n_images} + {len(out)} frames, capacity_images {self.capacity}')
        return out, labs

    def add_images(self, frames, labels=None):
        frames, labs = self._check_frames(frames, labels)
        if self.has_labels is None:
            self.has_labels = labs is not None
        d = self._device()
        (H, W), tabs = self.source_hw, d['tables']
        compute = torch.cuda.current_stream(self.device)
        slots = []
        for k, f in enumerate(frames):
            key = (d['frames'] % self.staging_images, f.ndim)  # (a set per frame kind: RGB and gray frames differ in size)
            d['frames'] += 1
            if key not in d['stage']:
                d['stage'][key] = _FrameStage(f.shape, (H, W), self.device)
                d['copy_stream'].wait_stream(compute)  # (the new buffers' zero fill runs on the compute stream)
            st = d['stage'][key]
            st.copied.synchronize()  # (the set's last upload has left the pinned buffers)
            np.copyto(st.host_np, f)
            if labs is not None:
                np.copyto(st.lab_np, labs[k])
            with torch.cuda.stream(d['copy_stream']):
                d['copy_stream'].wait_event(st.consumed)  # (the kernels that read the set's device copy have run)
                st.dev.copy_(st.host, non_blocking=True)
                if labs is not None:
                    st.lab_dev.copy_(st.lab_host, non_blocking=True)
                st.copied.record()
            compute.wait_event(st.copied)
            slot = self.n_images
            with torch.cuda.device(self.device):
                if self.frame_store:
                    rgb_last = f.ndim == 3 and self.gray == 'last'
                    scratch = d['scratch'] if rgb_last or self.gray == 'first' else d['scratch'].view(-1)[:H * self.resize_hw[1]].view(H, -1)
                    hip.image_ingest_frame(st.dev, d['images'][slot], tabs['h'], tabs['v'], scratch, resized_rows=self.resize_hw[0],
                                           gray_last=self.gray == 'last')
                else:
                    hip.image_ingest(st.dev, d['images'][slot], tabs['h'], tabs['v'], d['scratch'], self.standardization, d['minmax'][slot],
                                     **({} if labs is None else dict(label=st.lab_dev, label_rows=tabs['rows'], label_cols=tabs['cols'],
                                                                     out_label=d['labels'][slot])))
            st.consumed.record(compute)
            self.n_images += 1
            slots.append(slot)
        return slots


# ---------------------------------------------------------------------------------------------- batches
class ImageBatchBuilder:
    """build(indices) -> (img fp32 [B, 1, height, width] in [0, 1], label int64 [B, height, width] of trainIds, or None for a store
    without labels): the [data, label] batch of the image sensor (the layout SyntheticPairedLoader(images_only=True) yields), from B
    slot numbers of an ImageStore -- the reference loader behind its resize: the img[:height] cut under random_crop, the
    albumentations pipeline of datasets/augment.py (augmentation=False: the centred pad / crop only), the id -> trainId table of
    semseg_num_classes (6 | 11; None: raw ids), ToTensor.  shift_limit follows the reference: 0 under random_crop, 0.1 otherwise.

    A batch uploads ONE pinned table -- the B indices and the two parameter blocks, drawn by draw_params / draw_params2 as
    DeviceAugmentation draws them (seed: the generator) -- and runs hip.augment_image_label_store (stage 1 reading the uint8 slots
    through the index: no float copy of the source) and hip.augment_perspective_filter.  Every buffer is static, allocated at the
    first batch, whose size B every later batch must have; graph=True replays the captured launches (one capture per output set):
    other indices and parameters need no new capture.  Two output sets alternate: a batch stays valid until the one after the next
    is built.  last_params: the host rows (stage 1, stage 2 or None) of the batch just built."""

    def __init__(self, store, height, width, augmentation=True, random_crop=True, semseg_num_classes=6, seed=0, graph=False, device=None):
        if not isinstance(store, ImageStore):
            raise hip.EssHipError(f'ImageBatchBuilder: store must be an ImageStore, got {type(store).__name__}')
        if device is not None and torch.device(device) != store.device:
            raise hip.EssHipError(f'ImageBatchBuilder: device={device!r}: the batch is built where the store lies ({store.device})')
        self.height, self.width = _pair('ImageBatchBuilder: (height, width)', (height, width))
        if not _is_int(seed):
            raise hip.EssHipError(f'ImageBatchBuilder: seed={seed!r} must be an int')
        self.id_lut = None if semseg_num_classes is None else cityscapes_id_lut(semseg_num_classes)
        self.store, self.device = store, store.device
        self.augmentation, self.random_crop, self.use_graph = bool(augmentation), bool(random_crop), bool(graph)
        self.rows = min(self.height, store.slot_hw[0]) if self.random_crop else store.slot_hw[0]
        self.shift_limit = 0.0 if self.random_crop else 0.1
        self.generator = torch.Generator().manual_seed(int(seed))
        self.batch_size = None
        self.n_batches = self.n_captures = 0
        self.last_params = None
        self._static = None

    def _check(self, indices):
        if torch.is_tensor(indices) and not indices.is_cuda:
            indices = indices.numpy()
        idx = np.asarray(indices) if isinstance(indices, (list, tuple, np.ndarray)) else None
        if idx is None or idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in 'iu':
            raise hip.EssHipError('ImageBatchBuilder.build: indices must be a non-empty list of slot numbers')
        if self.batch_size is not None and idx.size != self.batch_size:
            raise hip.EssHipError(f'ImageBatchBuilder.build: {idx.size} indices, the builder\'s static buffers hold batch_size={self.batch_size}')
        bad = (idx < 0) | (idx >= self.store.n_images)
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            raise hip.EssHipError(f'ImageBatchBuilder.build: indices[{b}]={int(idx[b])}, the store holds {self.store.n_images} images')
        return idx.astype(np.int32)

    def _allocate(self, B):
        dev, H, W = self.device, self.height, self.width
        labelled = self.store.has_labels
        n_words = B * (1 + 12 + 24)
        table = torch.zeros(n_words, dtype=torch.int32, device=dev)
        stage = []
        for _ in range(2):
            host = torch.zeros(n_words, dtype=torch.int32).pin_memory()
            stage.append({'buf': host, 'index': host[:B].numpy(), 'p1': host[B:13 * B].view(torch.float32).view(B, 12).numpy(),
                          'p2': host[13 * B:].view(torch.float32).view(B, 24).numpy(), 'done': torch.cuda.Event()})
        pair = lambda: (torch.zeros(B, 1, H, W, dtype=torch.float32, device=dev),  # noqa: E731
                        torch.zeros(B, H, W, dtype=torch.int64, device=dev) if labelled else None)
        self._static = {
            'table': table, 'index': table[:B], 'p1': table[B:13 * B].view(torch.float32).view(B, 12),
            'p2': table[13 * B:].view(torch.float32).view(B, 24), 'stage': stage,
            'mid': pair() if self.augmentation else None, 'scratch': torch.zeros(B, H, W, dtype=torch.float32, device=dev) if self.augmentation else None,
            'out': [pair(), pair()], 'lut': None if self.id_lut is None else self.id_lut.to(dev), 'graphs': [None, None],
        }
        self.batch_size = B

    def _launch(self, k):
        st, store = self._static, self.store
        if not self.augmentation:
            hip.augment_image_label_store(store.images, store.labels, st['index'], self.rows, st['p1'], self.height, self.width, st['lut'],
                                          out=st['out'][k])
            return
        # two stages, as DeviceAugmentation runs them: the brightness / contrast values and the id table belong to the second
        hip.augment_image_label_store(store.images, store.labels, st['index'], self.rows, st['p1'], self.height, self.width, None, out=st['mid'])
        hip.augment_perspective_filter(st['mid'][0], st['mid'][1], st['p2'], st['lut'], out=st['out'][k], scratch=st['scratch'])

    def _replay(self, k):
        graphs = self._static['graphs']
        if graphs[k] is None:
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                self._launch(k)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch(k)
            graphs[k] = g
            self.n_captures += 1
        graphs[k].replay()

    def build(self, indices):
        idx = self._check(indices)
        B = idx.size
        if self.store.n_images == 0:
            raise hip.EssHipError('ImageBatchBuilder.build: the store holds no image')
        Hs, Ws = self.rows, self.store.slot_hw[1]
        p1 = draw_params(B, (Hs, Ws), (self.height, self.width), self.shift_limit, self.generator, self.augmentation)
        p2 = None
        if self.augmentation:
            p2 = draw_params2(B, (self.height, self.width), self.generator, alpha_beta=p1[:, 8:10].clone())
            p1[:, 8], p1[:, 9] = 1.0, 0.0
        with torch.cuda.device(self.device):
            if self._static is None:
                self._allocate(B)
            st = self._static
            k = self.n_batches & 1
            stage = st['stage'][k]
            stage['done'].synchronize()  # (the set's last upload has completed: it is free to be rewritten)
            stage['index'][:] = idx
            stage['p1'][:] = p1.numpy()
            if p2 is not None:
                stage['p2'][:] = p2.numpy()
            st['table'].copy_(stage['buf'], non_blocking=True)
            stage['done'].record()
            if self.use_graph:
                self._replay(k)
            else:
                self._launch(k)
        self.n_batches += 1
        self.last_params = (p1, p2)
        return st['out'][k]


class ImageSampler:
    """The batches of an epoch over the slots of an ImageStore: an iterable of int arrays of batch_size slot numbers, with a length --
    StoreSampler's rules.  indices: the slots of the epoch (default: all the store holds now).  shuffle: a new permutation every
    iteration (numpy's default_rng(seed + epoch)); drop_last False: a short last batch is filled up from the epoch's first slots."""

    def __init__(self, store, batch_size, indices=None, shuffle=True, seed=0, drop_last=True):
        if not isinstance(store, ImageStore):
            raise hip.EssHipError(f'ImageSampler: store must be an ImageStore, got {type(store).__name__}')
        if not _is_int(batch_size) or batch_size < 1:
            raise hip.EssHipError(f'ImageSampler: batch_size={batch_size!r} must be a positive int')
        if not _is_int(seed):
            raise hip.EssHipError(f'ImageSampler: seed={seed!r} must be an int')
        idx = list(range(store.n_images)) if indices is None else list(indices)
        for k, i in enumerate(idx):
            if not _is_int(i) or not 0 <= i < store.n_images:
                raise hip.EssHipError(f'ImageSampler: indices[{k}]={i!r}, the store holds {store.n_images} images')
        self.store, self.batch_size, self.indices = store, int(batch_size), np.array(idx, dtype=np.int64)
        self.shuffle, self.seed, self.drop_last, self.epoch = bool(shuffle), int(seed), bool(drop_last), 0

    def __len__(self):
        n, B = len(self.indices), self.batch_size
        return n // B if self.drop_last else -(-n // B)

    def __iter__(self):
        n, B = len(self.indices), self.batch_size
        order = np.random.default_rng(self.seed + self.epoch).permutation(n) if self.shuffle else np.arange(n)
        self.epoch += 1
        for k in range(len(self)):
            idx = order[k * B:(k + 1) * B]
            if len(idx) < B:
                idx = np.concatenate([idx, np.resize(order, B - len(idx))])
            yield self.indices[idx]


class ImageBatchLoader:
    """A loader of an ESS trainer (createIterators(), __len__, __iter__) over an ImageBatchBuilder: the image side of train_loader, or
    val_loader_sensor_a.  sampler: an iterable of batches of slot numbers (an ImageSampler), or a callable that returns one (called anew
    by createIterators).  steps: the batches of an epoch (default: len(sampler)).  Yields [img, label] (builder.build)."""

    def __init__(self, sampler, builder, steps=None):
        if not isinstance(builder, ImageBatchBuilder):
            raise hip.EssHipError(f'ImageBatchLoader: builder must be an ImageBatchBuilder, got {type(builder).__name__}')
        if steps is None:
            if not hasattr(sampler, '__len__'):
                raise hip.EssHipError('ImageBatchLoader: steps is needed where the sampler has no length')
            steps = len(sampler)
        if not _is_int(steps) or steps < 0:
            raise hip.EssHipError(f'ImageBatchLoader: steps={steps!r} must be a non-negative int')
        if not callable(sampler) and not hasattr(sampler, '__iter__'):
            raise hip.EssHipError('ImageBatchLoader: sampler must be an iterable of batches or a callable that returns one')
        self.sampler, self.builder, self.steps = sampler, builder, int(steps)
        self._it = None

    def __len__(self):
        return self.steps

    def createIterators(self):
        src = self.sampler() if callable(self.sampler) else self.sampler
        self._it = iter(src)

    def __iter__(self):
        if self._it is None:
            self.createIterators()
        it, self._it = self._it, None
        for _, indices in zip(range(self.steps), it):
            img, lab = self.builder.build(indices)
            yield [img, lab]


class PairedBatchLoader:
    """The UDA trainer's train_loader over two device loaders (an ImageBatchLoader and an EventBatchLoader): WrapperDataset's rule
    (datasets/wrapper_dataloader.py) without a host tensor in the loop.  The LONGER loader sets the epoch -- dataset_len_to_use =
    'first' | 'second' names it instead --; the shorter one restarts whenever it runs out and is advanced first.  Yields
    [[img, label_a], [events, label_b]].  createIterators() starts an epoch; iterating without it starts one too."""

    def __init__(self, loader_a, loader_b, dataset_len_to_use=None):
        for name, ld in (('loader_a', loader_a), ('loader_b', loader_b)):
            if not hasattr(ld, '__len__') or not hasattr(ld, '__iter__'):
                raise hip.EssHipError(f'PairedBatchLoader: {name} must be a loader with a length, got {type(ld).__name__}')
        if dataset_len_to_use not in (None, 'first', 'second'):
            raise hip.EssHipError(f"PairedBatchLoader: dataset_len_to_use={dataset_len_to_use!r}: None, 'first' or 'second'")
        self.loader_a, self.loader_b = loader_a, loader_b
        self.a_sets_epoch = len(loader_a) > len(loader_b)
        if dataset_len_to_use is not None:
            self.a_sets_epoch = dataset_len_to_use == 'first'
        self._iters = None

    def __len__(self):
        return len(self.loader_a if self.a_sets_epoch else self.loader_b)

    @staticmethod
    def _start(loader):
        if hasattr(loader, 'createIterators'):
            loader.createIterators()
        return iter(loader)

    def createIterators(self):
        self._iters = [self._start(self.loader_a), self._start(self.loader_b)]

    def __iter__(self):
        if self._iters is None:
            self.createIterators()
        its, self._iters = self._iters, None
        long, short = (0, 1) if self.a_sets_epoch else (1, 0)
        loaders = (self.loader_a, self.loader_b)
        for _ in range(len(self)):
            try:
                s = next(its[short])
            except StopIteration:
                its[short] = self._start(loaders[short])
                try:
                    s = next(its[short])
                except StopIteration:
                    raise hip.EssHipError('PairedBatchLoader: the shorter loader yields no batch') from None
            try:
                batch = next(its[long])
            except StopIteration:
                return
            pair = [None, None]
            pair[long], pair[short] = list(batch), list(s)
            yield pair
