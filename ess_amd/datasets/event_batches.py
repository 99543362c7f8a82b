"""Training batches from raw events: the reference loaders' grid AND their training augmentation, built on the device.

The reference loaders hand a train step [B, T * bins, h, w] event grids and [B, h, w] labels that went through the same geometric
augmentation:
    DSEC  (DSEC/dataset/sequence.py:281-295):              the loader's grid (rows cut, bilinear resize), then a horizontal flip, p = 0.5
    DDD17 (datasets/ddd17_events_loader.py:87-96, 162-183): the loader's grid, then HorizontalFlip(p=0.5) and RandomCrop(120, 216)
                                                            inside the bottom 120 of its 200 rows
EventBatchBuilder does that from the columns a camera or a file delivers: one hip.event_scatter_ring* over the B * T windows, one
hip.event_grid_finish_window (the loader's grid with flip and crop applied where it is written) and one hip.label_window (the label's
nearest resize with the same flip and crop).  The augmentation parameters are drawn on the host (draw_window_params), one row
(flip, y0, x0, reserved) per sample, and read on the device by both kernels.

NOT pinned: the random STREAM of albumentations / the reference's `random` calls (which draw is used for what), as datasets/augment.py
says of the image branch: a draw here is u < 0.5 for the flip and floor(u * (range + 1)) for an offset, its RandomCrop convention.  The
label's nearest resize follows the exact integer rule of hip.label_window; parity with cv2.resize(INTER_NEAREST) is unpinned (cv2 is
not a dependency).  File readers (h5, png) stay outside: a sample source delivers EventColumns and uint8 label arrays."""
import numpy as np
import torch

from .. import hip
from .data_util import EventColumns, stage_event_columns
from .event_store import EventStore, StoreSample, duration_bounds, time_bound
from .image_store import ImageStore

VOXEL_FLAVOURS = ('temporal', 'trilinear')
_NORMS = {None: hip.GRID_NORM_NONE, 'unbiased': hip.GRID_NORM_UNBIASED, 'population': hip.GRID_NORM_POPULATION}


def _pair(name, v):
    if not isinstance(v, (tuple, list)) or len(v) != 2 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a < 1 for a in v):
        raise hip.EssHipError(f'{name}={v!r}: a pair of positive ints is needed')
    return int(v[0]), int(v[1])


def _window_geometry(grid_hw, win_hw, band):
    """-> (H, W, h, w, first_row, n_rows), the window checked against the grid and the band against both"""
    H, W = _pair('grid_hw', grid_hw)
    h, w = _pair('win_hw', win_hw)
    if h > H or w > W:
        raise hip.EssHipError(f'win_hw={(h, w)} does not fit grid_hw={(H, W)}: the window is cut out of the grid')
    if band is None:
        band = (0, H)
    if not isinstance(band, (tuple, list)) or len(band) != 2 or \
            any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in band) or band[0] < 0 or band[1] < 1 or \
            band[0] + band[1] > H:
        raise hip.EssHipError(f'band={band!r}: (first_row, n_rows) of the {H} grid rows the window is drawn inside')
    if band[1] < h:
        raise hip.EssHipError(f'band={tuple(band)!r} has {band[1]} rows, the window needs {h}: no window fits the band')
    return H, W, h, w, int(band[0]), int(band[1])


def draw_window_params(n, grid_hw, win_hw, band=None, generator=None, augment=True):
    """The rows hip.event_grid_finish_window and hip.label_window read, drawn on the host -> int32 [n, 4] = (flip, y0, x0, 0).
    grid_hw=(H, W): the finished grid; win_hw=(h, w): the window cut out of it; band=(first_row, n_rows): the rows the window lies
    inside (default: all of them; DDD17: (80, 120)).  Per sample, in this order, one uniform draw u each (torch.rand, `generator`):
        flip = u < 0.5;   y0 = first_row + min(floor(u * (n_rows - h + 1)), n_rows - h);   x0 = min(floor(u * (W - w + 1)), W - w)
    (datasets/augment.py's RandomCrop convention).  augment=False: all zero -- and win_hw must then equal grid_hw."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise hip.EssHipError(f'draw_window_params: n={n!r} must be a positive int')
    H, W, h, w, first, rows = _window_geometry(grid_hw, win_hw, band)
    p = torch.zeros(int(n), 4, dtype=torch.int32)
    if not augment:
        if (h, w) != (H, W):
            raise hip.EssHipError(f'draw_window_params: augment=False leaves the grid as it is, win_hw={(h, w)} must equal grid_hw={(H, W)}')
        return p
    u = torch.rand(3, int(n), generator=generator, dtype=torch.float64)
    p[:, 0] = (u[0] < 0.5).to(torch.int32)
    p[:, 1] = first + torch.floor(u[1] * (rows - h + 1)).clamp(max=rows - h).to(torch.int32)
    p[:, 2] = torch.floor(u[2] * (W - w + 1)).clamp(max=W - w).to(torch.int32)
    return p


def check_window_params(params, n, grid_hw, win_hw, band=None):
    """params as build(params=) takes them -> int32 [n, 4] on the host, every row inside its range (flip 0 / 1, the window inside
    the band), else refused"""
    H, W, h, w, first, rows = _window_geometry(grid_hw, win_hw, band)
    p = torch.as_tensor(params)
    if p.is_cuda or p.dtype not in (torch.int32, torch.int64) or tuple(p.shape) != (n, 4):
        raise hip.EssHipError(f'params must be a host int32 [{n}, 4] table of (flip, y0, x0, reserved), got {p.dtype}{tuple(p.shape)}')
    p = p.to(torch.int32)
    ok = ((p[:, 0] == 0) | (p[:, 0] == 1)) & (p[:, 1] >= first) & (p[:, 1] <= first + rows - h) & (p[:, 2] >= 0) & (p[:, 2] <= W - w)
    if not bool(ok.all()):
        b = int((~ok).nonzero()[0])
        raise hip.EssHipError(f'params[{b}]={p[b].tolist()} is out of range: flip 0 / 1, y0 in [{first}, {first + rows - h}], '
                              f'x0 in [0, {W - w}] (a {h} x {w} window of the {H} x {W} grid)')
    return p.contiguous()


class _BatchStage:
    """one pinned staging set: the columns [B, capacity], the slot words [n_words, B T], the window rows [B, 4], the labels
    [B, Hl, Wl], and the event recorded behind the set's last upload"""
    __slots__ = ('cols', 'cols_np', 'words', 'words_np', 'params', 'labels', 'labels_np', 'done')

    def __init__(self, B, T, capacity, n_words, label_hw):
        dtypes = (torch.int64, torch.int16, torch.int16, torch.uint8)
        self.cols = tuple(torch.zeros(B, capacity, dtype=d).pin_memory() for d in dtypes)
        self.cols_np = tuple(c.numpy() for c in self.cols)
        self.words = torch.zeros(n_words, B * T, dtype=torch.int32).pin_memory()
        self.words_np = self.words.numpy()
        self.params = torch.zeros(B, 4, dtype=torch.int32).pin_memory()
        self.labels = torch.zeros((B,) + label_hw, dtype=torch.uint8).pin_memory()
        self.labels_np = self.labels.numpy()
        self.done = torch.cuda.Event()


class EventBatchBuilder:
    """build(samples) -> (events fp32 [B, T * C, h, w], labels int64 [B, h, w] or None): the [data, label] batch a train step of
    ESSSupervisedModel takes (the layout SyntheticPairedLoader(events_only=True) yields), from B samples of raw events.

    samples: B entries (EventColumns, label[, map index]) -- label: a uint8 [label_hw] array / CPU tensor, or None for EVERY sample of
    the batch (then no labels are returned); map index (voxel='trilinear' with rectify_maps): the number of the sample's map in
    rectify_maps, or None.  A sample's n events are cut as the loader cuts them (datasets.event_feed.sequence_windows from event 0):
    n // T events per window, window i = [i (n // T), (i + 1) (n // T)), the remainder at the end unused; n < T: an all-zero sample.

    Geometry (SequenceSegmenter's keywords): the events are voxelised at grid_hw=(Hs, Ws) with `bins` bins (voxel='temporal' |
    'trilinear') into C = `channels` planes a window -- representation=None: the signed grid, C = bins; 'separate_pol': C = 2 bins,
    [positive bins; negative bins]; 'histogram': C = 2, [negative counts, positive counts], bins unused (hip.event_scatter_ring_rep;
    both need voxel='temporal' and no rectify_maps) --, normalised over the non-zero voxels of all C planes, as the DDD17 loader
    normalises the concatenated representation (grid_normalize=None | 'unbiased' | 'population'), the top grid_rows are
    resized bilinearly to grid_resize=(Hr, Wr), and the top `height` rows of `width` = Wr columns are the loader's grid.  The
    augmentation cuts a crop_hw=(h, w) window (default: the whole height x width) out of its horizontally flipped (p = 0.5) self, at a
    random place inside the rows crop_band=(first_row, n_rows) (default: all).  The label, label_hw=(Hl, Wl), is resized (nearest)
    to height x width and gets the same flip and window.  augmentation=False: no flip, and crop_hw must be None.  The presets:
        EventBatchBuilder.dsec(batch_size, ...):  grid_hw=(480, 640), grid_rows=440, grid_resize=(448, 640), height=448, width=640,
                                                  label_hw=(440, 640); flip only
        EventBatchBuilder.ddd17(batch_size, ...): grid_hw=(260, 346), grid_resize=(260, 352), height=200, width=352,
                                                  crop_hw=(120, 216), crop_band=(80, 120), label_hw=(200, 346)
    params=: an int32 [B, 4] table of (flip, y0, x0, reserved) in place of the draw (seed: the draw's generator); the rows used are
    kept as last_params.  Everything is checked before anything is staged; a refused batch leaves the builder as it was.

    The columns are copied as they are (stage_event_columns) into one of two pinned staging sets, and from there into static device
    columns [B, event_capacity] (a multiple of 16); then one event_scatter_ring*, one event_grid_finish_window, one label_window.
    graph=True: those launches are captured once per output set and replayed.  The returned tensors stay valid until the build after
    the next one: two output sets alternate.

    Static device memory (allocated at the first batch): B T int64 sum grids [C, Hs, Ws] + two fp32 output sets [B T, C, h, w]
    + 13 bytes per event of capacity -- DSEC, B = 8, T = 20, C = bins = 5: 1.97 GB + 2 x 0.92 GB; DDD17, B = 8, T = 20, C = bins = 5:
    0.58 GB + 2 x 0.08 GB; 'separate_pol' doubles both terms (C = 10), 'histogram' takes 2 / 5 of them -- and the staging sets in
    pinned host memory: 2 x 13 bytes x B x event_capacity.

    store=EventStore (datasets/event_store.py): the samples are StoreSamples of recordings that lie in device memory already, and
    event_capacity is not read (pass None): neither the static columns nor the pinned column staging exist.  window_events=N: a sample
    is the last T N events before its end -- t_end: the first event of the recording with t >= t_end - t_offset, as
    EventSlicer.get_events_fixed_num finds it, or end: an event index of the recording --, clamped at the recording's first event and
    split into T equal windows (datasets.event_feed.sequence_windows); window_duration=D: T windows of D time units that end at t_end
    (sequence_windows_fixed_duration), with window_capacity= the most events one may hold.  One of the two; one rule per batch.  A
    batch uploads ONE pinned table of 8 (T + 1 | 1) + 32 bytes a sample; then hip.event_store_windows, hip.event_scatter_store,
    hip.event_grid_finish_window, a torch.index_select of the store's labels and hip.label_window, all inside the captured graph with
    graph=True (one capture per output set, kind of batch and rule).  last_flags: the device int32 [B] flag words of the batch just
    built (hip.EVENT_STORE_FLAG_*; a flagged sample is all zero, as a sample with n < T is); reading them is the caller's
    synchronisation.

    frames=ImageStore (store path only; ImageStore.dsec_frames / ddd17_frames): the loaders' PAIRED camera frame.  Every StoreSample
    then names its frame's slot (frame=), and build() returns (events, frames fp32 [B, 1, Hf, Wf] in [0, 1], labels) -- the tuple the
    reference loaders return with require_paired_data_*_b.  The slot numbers travel in the batch's one table; hip.image_gather_unit
    (slot / 255, ToTensor's bits) runs behind label_window, inside the capture.  The frame is NOT flipped or cropped by the window
    parameters: the reference flips events and label only (sequence.py:291-295), and DDD17 pairs frames in its validation split.
    original_labels=True (store path, augmentation=False): the sample's stored label, int64 [B, label_hw] as it is, is appended --
    DDD17's (events, img, label, label_original)."""

    def __init__(self, batch_size, sequence_steps, bins, event_capacity, grid_hw, height, width, label_hw, grid_rows=None,
                 grid_resize=None, grid_normalize=None, crop_hw=None, crop_band=None, voxel='temporal', rectify_maps=None,
                 augmentation=True, seed=0, device=None, graph=False, representation=None, store=None, window_events=None,
                 window_duration=None, window_capacity=None, frames=None, original_labels=False):
        for name, v in (('batch_size', batch_size), ('sequence_steps', sequence_steps), ('bins', bins)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise hip.EssHipError(f'{name}={v!r}: a positive int is needed')
        if batch_size * sequence_steps > 65535:
            raise hip.EssHipError(f'batch_size * sequence_steps = {batch_size * sequence_steps}: one launch serves at most 65535 windows')
        Hs, Ws = _pair('grid_hw', grid_hw)
        self._check_store(store, window_events, window_duration, window_capacity, device)
        self._check_frames(frames, original_labels, augmentation)
        if store is not None:
            event_capacity = None  # (no static columns: the windows are read where the store keeps them)
        elif isinstance(event_capacity, bool) or not isinstance(event_capacity, int) or event_capacity < 1 or \
                event_capacity % hip.EVCOL_STRIDE_ALIGN or event_capacity > hip.INGEST_MAX_CAPACITY:
            raise hip.EssHipError(f'event_capacity={event_capacity!r}: events per sample, a multiple of {hip.EVCOL_STRIDE_ALIGN} in '
                                  f'[{hip.EVCOL_STRIDE_ALIGN}, {hip.INGEST_MAX_CAPACITY}] (hip.event_column_stride rounds up)')
        if Hs > 32767 or Ws > 32767:
            raise hip.EssHipError(f'grid_hw={(Hs, Ws)}: the columns carry 16-bit coordinates')
        rows = Hs if grid_rows is None else grid_rows
        if isinstance(rows, bool) or not isinstance(rows, int) or not 1 <= rows <= Hs:
            raise hip.EssHipError(f'grid_rows={rows!r}: the top rows of the {Hs} x {Ws} grid that are kept, an int in [1, {Hs}]')
        Hr, Wr = (rows, Ws) if grid_resize is None else _pair('grid_resize', grid_resize)
        height, width = _pair('(height, width)', (height, width))
        if Wr != width or height > Hr:
            raise hip.EssHipError(f'the loader grid ends as {Hr} x {Wr} (grid_resize, or grid_rows x the grid\'s width), the batch holds its '
                                  f'top {height} rows of {width} columns: the widths must agree and height <= {Hr}')
        if not isinstance(grid_normalize, (str, type(None))) or grid_normalize not in _NORMS:
            raise hip.EssHipError(f"grid_normalize={grid_normalize!r}: None, 'unbiased' (VoxelGrid(normalize=True)) or 'population' "
                                  '(normalize_voxel_grid)')
        if voxel not in VOXEL_FLAVOURS:
            raise hip.EssHipError(f'voxel={voxel!r}: one of {VOXEL_FLAVOURS}')
        self._rep = hip.event_representation(representation, voxel, rectify_maps)
        self.representation, self.channels = representation, hip.event_rep_channels(self._rep, bins)
        self.augmentation = bool(augmentation)
        if crop_hw is None:
            if crop_band is not None:
                raise hip.EssHipError(f'crop_band={crop_band!r} without crop_hw: a band places a crop')
            crop_hw = (height, width)
        elif not self.augmentation:
            raise hip.EssHipError(f'crop_hw={crop_hw!r} with augmentation=False: the crop is part of the augmentation')
        _, _, h, w, first, n_rows = _window_geometry((height, width), crop_hw, crop_band)
        self.label_hw = _pair('label_hw', label_hw)
        self.maps = self._check_maps(rectify_maps, voxel)
        self.batch_size, self.sequence_steps, self.bins, self.event_capacity = batch_size, sequence_steps, bins, event_capacity
        self.grid_hw, self.grid_rows, self.grid_resize, self.grid_normalize = (Hs, Ws), rows, (Hr, Wr), _NORMS[grid_normalize]
        self.height, self.width, self.crop_hw, self.crop_band, self.voxel = height, width, (h, w), (first, n_rows), voxel
        self.device = device if device is not None else (store.device if store is not None else torch.device('cuda:0'))
        self.use_graph = bool(graph)
        self.last_flags = None
        self.generator = torch.Generator().manual_seed(int(seed))
        self.last_params = None
        self.n_batches = self.n_captures = 0
        self._static = None  # (the device and pinned buffers: allocated at the first accepted batch)

    @classmethod
    def dsec(cls, batch_size, sequence_steps=20, bins=5, event_capacity=2000000, **kw):
        """the DSEC loader with resize=True (sequence.py:281-295): 480 x 640 -> the top 440 rows -> 448 x 640, flip only"""
        geo = dict(grid_hw=(480, 640), grid_rows=440, grid_resize=(448, 640), height=448, width=640, label_hw=(440, 640))
        return cls(batch_size, sequence_steps, bins, event_capacity, **{**geo, **kw})

    @classmethod
    def ddd17(cls, batch_size, sequence_steps=20, bins=5, event_capacity=2000000, **kw):
        """the DDD17 loader (ddd17_events_loader.py:162-183): 260 x 346 -> 260 x 352 -> the top 200 rows, flip, a 120 x 216 crop
        inside the bottom 120 rows; augmentation=False (its validation split, :187-213): neither flip nor crop, the 200 x 352 grid"""
        geo = dict(grid_hw=(260, 346), grid_resize=(260, 352), height=200, width=352, label_hw=(200, 346))
        if kw.get('augmentation', True):
            geo.update(crop_hw=(120, 216), crop_band=(80, 120))
        return cls(batch_size, sequence_steps, bins, event_capacity, **{**geo, **kw})

    def _check_store(self, store, window_events, window_duration, window_capacity, device):
        """store=, window_events=, window_duration=, window_capacity= -> self.store, self.store_rule_by_count, self.window,
        self.window_capacity (the events a window may hold: it shapes the scatter's launch)"""
        self.store = store
        if store is None:
            if window_events is not None or window_duration is not None or window_capacity is not None:
                raise hip.EssHipError('window_events / window_duration / window_capacity cut samples out of an EventStore: they need store=')
            return
        if not isinstance(store, EventStore):
            raise hip.EssHipError(f'store must be an EventStore, got {type(store).__name__}')
        if device is not None and torch.device(device) != torch.device(store.device):
            raise hip.EssHipError(f'device={device!r}: the batch is built where the store lies ({store.device})')
        if (window_events is None) == (window_duration is None):
            raise hip.EssHipError('give window_events=N (the events of a window) or window_duration=D (its time span), one of the two')
        self.store_by_count = window_events is not None
        if self.store_by_count:
            if isinstance(window_events, bool) or not isinstance(window_events, int) or not 1 <= window_events <= hip.INGEST_MAX_CAPACITY:
                raise hip.EssHipError(f'window_events={window_events!r}: an int in [1, {hip.INGEST_MAX_CAPACITY}]')
            self.window = window_events
            window_capacity = window_events if window_capacity is None else window_capacity
        else:
            d = window_duration
            if isinstance(d, bool) or not isinstance(d, (int, float)) or not d > 0 or d == float('inf'):
                raise hip.EssHipError(f'window_duration={d!r} must be a positive number')
            if window_capacity is None:
                raise hip.EssHipError('window_duration needs window_capacity=: the most events a window may hold (a larger one flags its sample)')
            self.window = d
        if isinstance(window_capacity, bool) or not isinstance(window_capacity, int) or \
                not (self.window if self.store_by_count else 1) <= window_capacity <= hip.INGEST_MAX_CAPACITY:
            raise hip.EssHipError(f'window_capacity={window_capacity!r}: an int in [window_events or 1, {hip.INGEST_MAX_CAPACITY}]')
        self.window_capacity = window_capacity

    def _check_frames(self, frames, original_labels, augmentation):
        """frames=, original_labels= -> self.frames, self.original_labels: both belong to the store path"""
        if frames is not None:
            if self.store is None:
                raise hip.EssHipError('frames= pairs camera frames with the samples of an EventStore: it needs store=')
            if not isinstance(frames, ImageStore):
                raise hip.EssHipError(f'frames must be an ImageStore (ImageStore.dsec_frames / ddd17_frames), got {type(frames).__name__}')
            if torch.device(frames.device) != torch.device(self.store.device):
                raise hip.EssHipError(f'frames lies on {frames.device}, the event store on {self.store.device}: a batch is built on one device')
        if not isinstance(original_labels, bool):
            raise hip.EssHipError(f'original_labels={original_labels!r} must be True or False')
        if original_labels and self.store is None:
            raise hip.EssHipError('original_labels=True returns the labels an EventStore keeps: it needs store=')
        if original_labels and augmentation:
            raise hip.EssHipError('original_labels=True with augmentation=True: the stored label is returned as it is, beside a label that '
                                  'was flipped and cropped (the DDD17 loader returns it in its validation split only)')
        self.frames, self.original_labels = frames, original_labels

    def _check_store_samples(self, samples, params):
        """the checks of one store batch: nothing is written -> (rule, bound words [B][n_bounds], label indices or None, map words, params)"""
        B, T, store = self.batch_size, self.sequence_steps, self.store
        if not isinstance(samples, (list, tuple)) or len(samples) != B or any(not isinstance(s, StoreSample) for s in samples):
            raise hip.EssHipError(f'samples must be a list of batch_size={B} StoreSamples')
        by_time = samples[0].t_end is not None
        if any((s.t_end is not None) != by_time for s in samples):
            raise hip.EssHipError('samples: t_end for every sample of the batch, or end for every one (one rule per launch)')
        if not by_time and not self.store_by_count:
            raise hip.EssHipError('window_duration cuts by time: its samples need t_end, not end')
        rule = hip.EVENT_STORE_RULE_DURATION if not self.store_by_count else \
            (hip.EVENT_STORE_RULE_COUNT_TIME if by_time else hip.EVENT_STORE_RULE_COUNT_INDEX)
        bounds = []
        n_maps =0 if self.maps is None else self.maps.shape[0]
        for b, s in enumerate(samples):
            if s.recording >= store.n_recordings:
                raise hip.EssHipError(f'samples[{b}] names recording {s.recording}, the store holds {store.n_recordings}')
            if s.label is not None and s.label >= store.n_labels:
                raise hip.EssHipError(f'samples[{b}]: label index {s.label} of the store\'s {store.n_labels} labels')
            if s.map is not None and s.map >= n_maps:
                raise hip.EssHipError(f'samples[{b}]: map index {s.map!r} of the builder\'s {n_maps} rectify_maps')
            begin, end = store.extent(s.recording)
            if not by_time:
                if s.end > end - begin:
                    raise hip.EssHipError(f'samples[{b}]: end={s.end} of recording {s.recording}\'s {end - begin} events')
                bounds.append([s.end])
                continue
            t_i64 = bool(store.format_of(s.recording) & hip.EVCOL_T_I64)
            t_end = s.t_end - store.t_offset(s.recording)
            times = [t_end] if self.store_by_count else duration_bounds(t_end, T, self.window)
            bounds.append([time_bound(v, t_i64) for v in times])
        map_of =[hip.RECTIFY_NONE if s.map is None else s.map for s in samples]
        labelled = [s.label is not None for s in samples]
        if any(labelled) and not all(labelled):
            raise hip.EssHipError('samples: a label for every sample of the batch, or for none')
        if all(labelled) and (store.label_hw != self.label_hw):
            raise hip.EssHipError(f'the store keeps labels of {store.label_hw}, the builder takes label_hw={self.label_hw}')
        if self.original_labels and not all(labelled):
            raise hip.EssHipError('original_labels=True: every sample of the batch needs a label')
        if self.frames is not None:
            for b, s in enumerate(samples):
                if s.frame is None:
                    raise hip.EssHipError(f'samples[{b}] has no frame: with frames= every sample names its paired frame\'s slot')
                if s.frame >= self.frames.n_images:
                    raise hip.EssHipError(f'samples[{b}]: frame slot {s.frame}, the frame store holds {self.frames.n_images} images')
        grid, win = (self.height, self.width), self.crop_hw
        if params is None:
            p = draw_window_params(B, grid, win, self.crop_band, self.generator, self.augmentation)  # (the last check: it cannot fail)
        else:
            p = check_window_params(params, B, grid, win, self.crop_band)
        return rule, bounds, ([s.label for s in samples] if all(labelled) else None), map_of, p

    @staticmethod
    def _check_maps(rectify_maps, voxel):
        """rectify_maps: None or a list of fp32 [map_h, map_w, 2] maps of one sensor size -> host fp32 [n_maps, map_h, map_w, 2] / None"""
        if rectify_maps is None:
            return None
        if voxel != 'trilinear':
            raise hip.EssHipError(f"rectify_maps belongs to voxel='trilinear' (this builder: voxel={voxel!r})")
        if not isinstance(rectify_maps, (list, tuple)) or not rectify_maps:
            raise hip.EssHipError('rectify_maps must be a non-empty list of fp32 [map_h, map_w, 2] maps; a sample names one by its number')
        maps = []
        for i, m in enumerate(rectify_maps):
            v = torch.as_tensor(m) if torch.is_tensor(m) or isinstance(m, np.ndarray) else None
            if v is None or v.dtype != torch.float32 or v.dim() != 3 or v.shape[2] != 2 or v.numel() == 0 or \
                    max(v.shape[:2]) > hip.RECTIFY_MAX_SIDE or (maps and v.shape != maps[0].shape):
                raise hip.EssHipError(f'rectify_maps[{i}] must be a float32 [map_h, map_w, 2] array or tensor of the first map\'s size')
            maps.append(v.detach().cpu())
        return torch.stack(maps).contiguous()

    # ---- the checks of one batch: nothing is written
    def _check(self, samples, params):
        B = self.batch_size
        if not isinstance(samples, (list, tuple)) or len(samples) != B:
            n = len(samples) if isinstance(samples, (list, tuple)) else type(samples).__name__
            raise hip.EssHipError(f'samples must be a list of batch_size={B} entries (EventColumns, label[, map index]): got {n}')
        cols, labels, map_of = [], [], []
        for b, s in enumerate(samples):
            if not isinstance(s, (list, tuple)) or len(s) not in (2, 3) or not isinstance(s[0], EventColumns):
                raise hip.EssHipError(f'samples[{b}] must be (EventColumns, label[, map index])')
            if s[0].n > self.event_capacity:
                raise hip.EssHipError(f'samples[{b}] has {s[0].n} events, event_capacity={self.event_capacity}')
            g = s[1]
            if g is not None:
                if torch.is_tensor(g) and not g.is_cuda:
                    g = g.numpy()
                if not isinstance(g, np.ndarray) or g.dtype != np.uint8 or tuple(g.shape) != self.label_hw:
                    got = f'{g.dtype}{tuple(g.shape)}' if hasattr(g, 'dtype') else type(g).__name__
                    raise hip.EssHipError(f'samples[{b}]: the label must be a host uint8 {list(self.label_hw)} array or None, got {got}')
            m = s[2] if len(s) == 3 else None
            if m is not None:
                n_maps = 0 if self.maps is None else self.maps.shape[0]
                if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= m < n_maps:
                    raise hip.EssHipError(f'samples[{b}]: map index {m!r} of the builder\'s {n_maps} rectify_maps')
            cols.append(s[0])
            labels.append(g)
            map_of.append(hip.RECTIFY_NONE if m is None else int(m))
        if any(g is None for g in labels) and not all(g is None for g in labels):
            raise hip.EssHipError('samples: a label for every sample of the batch, or for none')
        grid, win = (self.height, self.width), self.crop_hw
        if params is None:
            p = draw_window_params(B, grid, win, self.crop_band, self.generator, self.augmentation)  # (the last check: it cannot fail)
        else:
            p = check_window_params(params, B, grid, win, self.crop_band)
        return cols, (None if labels[0] is None else labels), map_of, p

    # ---- the device side
    def _allocate(self):
        B, T, cap, dev = self.batch_size, self.sequence_steps, self.event_capacity, self.device
        n_words = 5 if self.voxel == 'trilinear' else 4  # (rows, starts, counts, formats; the map words behind them)
        h, w = self.crop_hw
        dtypes = (torch.int64, torch.int16, torch.int16, torch.uint8)
        st = {
            'cols': tuple(torch.zeros(B, cap, dtype=d, device=dev) for d in dtypes),
            'words': torch.zeros(n_words, B * T, dtype=torch.int32, device=dev),
            'params': torch.zeros(B, 4, dtype=torch.int32, device=dev),
            'labels': torch.zeros((B,) + self.label_hw, dtype=torch.uint8, device=dev),
            'acc': torch.zeros(B * T, self.channels, *self.grid_hw, dtype=torch.int64, device=dev),
            'out': [(torch.zeros(B * T, self.channels, h, w, dtype=torch.float32, device=dev),
                     torch.zeros(B, h, w, dtype=torch.int64, device=dev)) for _ in range(2)],
            'maps': None if self.maps is None else self.maps.to(dev),
            'stage': [_BatchStage(B, T, cap, n_words, self.label_hw) for _ in range(2)],
            'graphs': [None, None],
        }
        st['words'][4:].fill_(hip.RECTIFY_NONE)
        self._static = st

    def _launch(self, k, with_labels):
        """the three launches of one batch into output set k"""
        st = self._static
        ev, lab = st['out'][k]
        words = st['words']
        tri = self.voxel == 'trilinear'
        hip.event_voxels('ring', st['cols'], words[:4], None, st['acc'], representation=self._rep, trilinear=tri, maps=st['maps'],
                         map_of=words[4] if tri else None)
        hip.event_grid_finish_window(words[2], st['acc'], ev, st['params'], self.sequence_steps, crop_rows=self.grid_rows,
                                     resize=self.grid_resize, normalize=self.grid_normalize)
        if with_labels:
            hip.label_window(st['labels'], lab, st['params'], resize=(self.height, self.width))

    def _replay(self, k, with_labels, rule=None):
        """rule: the store's window rule of the batch (a captured launch holds it), None for host columns"""
        st = self._static
        launch = (lambda: self._launch(k, with_labels)) if rule is None else (lambda: self._launch_store(k, with_labels, rule))
        kind = with_labels if rule is None else (with_labels, rule)
        graphs = st['graphs'][k] = st['graphs'][k] or {}
        if kind not in graphs:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch()
            graphs[kind] = g
            self.n_captures += 1
        graphs[kind].replay()

    # ---- the store source: no static columns, no column staging; one small table a batch
    def _store_layout(self):
        """the per-batch table, in bytes: name -> (offset, dtype, shape); every section starts 16-byte aligned"""
        B, T = self.batch_size, self.sequence_steps
        n_bounds = T + 1 if not self.store_by_count else 1
        at, out = 0, {}
        sections = [('bounds', torch.int64, (B, n_bounds)), ('label_of', torch.int64, (B,)), ('recording', torch.int32, (B,)),
                    ('sample_map', torch.int32, (B,)), ('params', torch.int32, (B, 4))]
        if self.frames is not None:
            sections.append(('frame_of', torch.int32, (B,)))  # (the paired frames' slots travel in the same table: one upload a batch)
        for name, dtype, shape in sections:
            out[name] = (at, dtype, shape)
            at += -(-int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 16) * 16
        return out, at

    def _allocate_store(self):
        B, T, dev = self.batch_size, self.sequence_steps, self.device
        h, w = self.crop_hw
        layout, nbytes = self._store_layout()
        views = lambda buf: {name: buf[at:at + int(np.prod(shape)) * torch.empty(0, dtype=d).element_size()].view(d).view(shape)  # noqa: E731
                             for name, (at, d, shape) in layout.items()}
        table = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        stage = []
        for _ in range(2):
            host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            stage.append({'buf': host, 'np': {n: v.numpy() for n, v in views(host).items()}, 'done': torch.cuda.Event()})
        self._static = {
            'table': table, 'in': views(table), 'stage': stage,
            'starts': torch.zeros(B * T, dtype=torch.int64, device=dev),
            'words': torch.zeros(3, B * T, dtype=torch.int32, device=dev),  # counts, formats, map words
            'flags': [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)],
            'labels': torch.zeros((B,) + self.label_hw, dtype=torch.uint8, device=dev),
            'acc': torch.zeros(B * T, self.channels, *self.grid_hw, dtype=torch.int64, device=dev),
            'out': [(torch.zeros(B * T, self.channels, h, w, dtype=torch.float32, device=dev),
                     torch.zeros(B, h, w, dtype=torch.int64, device=dev)) for _ in range(2)],
            'maps': None if self.maps is None else self.maps.to(dev),
            'graphs': [None, None],
            'frames': None if self.frames is None else
            [torch.zeros((B, 1) + self.frames.slot_hw, dtype=torch.float32, device=dev) for _ in range(2)],
            'original': [torch.zeros((B,) + self.label_hw, dtype=torch.int64, device=dev) for _ in range(2)] if self.original_labels else None,
        }

    def _launch_store(self, k, with_labels, rule):
        """the launches of one store batch into output set k: the window search, the scatter, the finish, the labels' gather and window"""
        st, store, T = self._static, self.store, self.sequence_steps
        ev, lab = st['out'][k]
        tin, (counts, formats, map_of) = st['in'], st['words']
        t = store.columns[0]
        # (total = the capacity: the search keeps every window inside its recording's table row, and a replayed graph serves
        # recordings that were added after its capture)
        hip.event_store_windows(t, store.table, tin['recording'], tin['bounds'], rule, T, st['starts'], counts, formats, st['flags'][k],
                                store.capacity, self.window_capacity, n_per_window=self.window if self.store_by_count else None,
                                sample_map=tin['sample_map'], map_of=map_of)
        hip.event_voxels('store', store.columns, (st['starts'], counts, formats), None, st['acc'], representation=self._rep,
                         trilinear=self.voxel == 'trilinear', maps=st['maps'], map_of=map_of, total=store.capacity,
                         window_capacity=self.window_capacity)
        hip.event_grid_finish_window(counts, st['acc'], ev, tin['params'], T, crop_rows=self.grid_rows, resize=self.grid_resize,
                                     normalize=self.grid_normalize)
        if with_labels:
            torch.index_select(store.labels, 0, tin['label_of'], out=st['labels'])
            hip.label_window(st['labels'], lab, tin['params'], resize=(self.height, self.width))
            if self.original_labels:
                st['original'][k].copy_(st['labels'])  # (the stored label as it is: not resized, flipped or cropped)
        if self.frames is not None:  # (the frame is neither flipped nor cropped: the loaders flip the events and the label only)
            hip.image_gather_unit(self.frames.images, tin['frame_of'], out=st['frames'][k])

    def _build_store(self, samples, params):
        rule, bounds, label_of, map_of, p = self._check_store_samples(samples, params)
        if self.store.n_recordings == 0:
            raise hip.EssHipError('the store holds no recording')
        if self._static is None:
            self._allocate_store()
        st, B, T = self._static, self.batch_size, self.sequence_steps
        k = self.n_batches & 1
        stage = st['stage'][k]
        stage['done'].synchronize()  # (the set's last upload has completed: it is free to be rewritten)
        w = stage['np']
        w['bounds'][:] = 0
        for b, row in enumerate(bounds):
            w['bounds'][b, :len(row)] = row
        w['label_of'][:] = 0 if label_of is None else label_of
        w['recording'][:] = [s.recording for s in samples]
        w['sample_map'][:] = map_of
        w['params'][:] = p.numpy()
        if self.frames is not None:
            w['frame_of'][:] = [s.frame for s in samples]
        st['table'].copy_(stage['buf'], non_blocking=True)
        stage['done'].record()
        if self.use_graph:
            self._replay(k, label_of is not None, rule)
        else:
            self._launch_store(k, label_of is not None, rule)
        self.n_batches += 1
        self.last_params, self.last_flags = p, st['flags'][k]
        ev, lab = st['out'][k]
        h, wd = self.crop_hw
        batch = [ev.view(B, T * self.channels, h, wd), (lab if label_of is not None else None)]
        if self.frames is not None:  # (the loaders' tuple: events, paired frame, label)
            batch.insert(1, st['frames'][k])
        if self.original_labels:
            batch.append(st['original'][k])
        return tuple(batch)

    def build(self, samples, params=None):
        """-> (events fp32 [B, T * bins, h, w], labels int64 [B, h, w] or None) on the device, valid until the build after the next"""
        if self.store is not None:
            return self._build_store(samples, params)
        cols, labels, map_of, p = self._check(samples, params)
        if self._static is None:
            self._allocate()
        st, B, T = self._static, self.batch_size, self.sequence_steps
        k = self.n_batches & 1
        stage = st['stage'][k]
        stage.done.synchronize()  # (the set's last upload has completed: it is free to be rewritten)
        w = stage.words_np
        for b, c in enumerate(cols):
            stage_event_columns(c, *(a[b] for a in stage.cols_np))
            n = c.n // T
            s = slice(b * T, (b + 1) * T)
            w[0, s], w[1, s], w[2, s], w[3, s] = b, np.arange(T, dtype=np.int32) * n, n, c.format
            if w.shape[0] > 4:
                w[4, s] = map_of[b]
            if labels is not None:
                np.copyto(stage.labels_np[b], labels[b])
        stage.params.copy_(p)
        for b, c in enumerate(cols):
            if c.n:
                for dev, host in zip(st['cols'], stage.cols):
                    dev[b, :c.n].copy_(host[b, :c.n], non_blocking=True)
        st['words'].copy_(stage.words, non_blocking=True)
        st['params'].copy_(stage.params, non_blocking=True)
        if labels is not None:
            st['labels'].copy_(stage.labels, non_blocking=True)
        stage.done.record()
        if self.use_graph:
            self._replay(k, labels is not None)
        else:
            self._launch(k, labels is not None)
        self.n_batches += 1
        self.last_params = p
        ev, lab = st['out'][k]
        h, wd = self.crop_hw
        return ev.view(B, T * self.channels, h, wd), (lab if labels is not None else None)


class EventBatchLoader:
    """A train / validation loader of an ESS trainer (createIterators(), __len__, __iter__) over an EventBatchBuilder: assign it as
    train_loader / val_loader_sensor_b of ESSSupervisedModel.  sample_source: an iterable of batches -- each a list of batch_size
    samples (EventColumns, label[, map index]) -- or a callable that returns one (called anew by createIterators: one epoch each).
    steps: the batches of an epoch (default: len(sample_source)); the iteration also ends where the source does.  Yields
    [events, labels] (builder.build; with frames= / original_labels= the longer tuples, as a list): a batch stays valid until the one
    after the next is built."""

    def __init__(self, sample_source, builder, steps=None):
        if not isinstance(builder, EventBatchBuilder):
            raise hip.EssHipError(f'EventBatchLoader: builder must be an EventBatchBuilder, got {type(builder).__name__}')
        if steps is None:
            if not hasattr(sample_source, '__len__'):
                raise hip.EssHipError('EventBatchLoader: steps is needed where the sample source has no length')
            steps = len(sample_source)
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
            raise hip.EssHipError(f'EventBatchLoader: steps={steps!r} must be a non-negative int')
        if not callable(sample_source) and not hasattr(sample_source, '__iter__'):
            raise hip.EssHipError('EventBatchLoader: sample_source must be an iterable of batches or a callable that returns one')
        self.sample_source, self.builder, self.steps = sample_source, builder, steps
        self._it = None

    def __len__(self):
        return self.steps

    def createIterators(self):
        src = self.sample_source() if callable(self.sample_source) else self.sample_source
        self._it = iter(src)

    def __iter__(self):
        if self._it is None:
            self.createIterators()
        it, self._it = self._it, None
        for _, samples in zip(range(self.steps), it):
            yield list(self.builder.build(samples))
