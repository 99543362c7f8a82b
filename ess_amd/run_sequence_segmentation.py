"""
Sequence rounds: the validation protocol of the DSEC trainers, served from a continuous event feed and scored on the device.

The reference never carries recurrent state across labels.  Its DSEC loader (DSEC/dataset/sequence.py:255-279) takes, for a label
at time t, the last nr_events_data x nr_events_window events before t (20 x 100 000 in settings_DSEC.yaml), splits them into
nr_events_data equal chunks and voxelises each; the trainer's validation (training/ess_trainer.py:424-493) resets the encoder's
state, runs the T chunks from zero, resizes the logits, takes the argmax and adds to a confusion matrix.  MultiStreamSegmenter
(run_segmentation.py) carries one state for the life of a stream instead, so its labels are not those validation would give on
the same events, and nothing in it can score itself.

SequenceSegmenter does the protocol: at a label time each stream's last T x N_w fed events are cut as the loader cuts them
(datasets.event_feed.sequence_windows), voxelised inside the round from the stream's device ring (T x S slots, slot t S + s naming
row s), normalised per sample, run through T encoder steps from a ZERO state (ImageReconstructor.update_reconstruction_sequence:
lean steps, the last one final-lean, in 'mixed' the [hi | lo] operand pair only where steps_left says so) and decoded by
SemSegE2VID.predict with the class head that scores itself (hip.seg_head_eval): labels, colours, confidences and a per-stream
confusion matrix against the ground truth, all on the device, in one captured graph.
"""
import collections

import numpy as np
import torch

from . import hip
from .e2vid.image_reconstructor import ImageReconstructor
from .evaluation.metrics import semseg_accum_confusion_to_acc, semseg_accum_confusion_to_iou
from .run_segmentation import (VOXEL_FLAVOURS, MultiSegmentationResult, _check_hot_pixel_masks, _event_capacity,
                               _event_representation, _HotPixelSlots, _models_from_checkpoints, _rectify_maps, _RingStage)


class _SequenceStage(_RingStage):
    """one pinned staging set of a sequence round: _RingStage's words, [4 or 5, T S], and the ground-truth rows [S, H_out, W_out]"""
    __slots__ = ('gt', 'gt_np')

    def __init__(self, words, gt, done):
        super().__init__(words, done)
        self.gt, self.gt_np = gt, gt.numpy()


class _RecordingMasks:
    """The hot-pixel masks of a store-fed segmenter, keyed by RECORDING (a mask belongs to a sensor, and a lane of a round may name any
    recording): ONE static device buffer words int32 [n_slots, mask_h, ceil(mask_w / 32)] under the capture, and the host's books --
    which HotPixelMask each slot holds (entries that are the same object share a slot) and slot_of, recording -> slot."""

    def __init__(self, n_slots, size, device):
        self.n_slots, self.size = n_slots, (int(size[0]), int(size[1]))
        self.words = torch.zeros(n_slots, self.size[0], hip.mask_words(self.size[1]), dtype=torch.int32, device=device)
        self.held = [None] * n_slots
        self.slot_of = {}

    @staticmethod
    def check(what, recording, mask, size):
        from .datasets.hot_pixels import HotPixelMask
        if isinstance(recording, bool) or not isinstance(recording, (int, np.integer)) or recording < 0:
            raise hip.EssHipError(f'{what}: recording {recording!r} must be a non-negative int (a recording of the store)')
        if mask is not None and not isinstance(mask, HotPixelMask):
            raise hip.EssHipError(f'{what}: recording {recording} needs a datasets.hot_pixels.HotPixelMask or None, got {type(mask).__name__}')
        if mask is not None and (mask.height, mask.width) != tuple(size):
            raise hip.EssHipError(f'{what}: the mask of recording {recording} is {mask.height} x {mask.width}, the masks of this segmenter '
                                  f'{size[0]} x {size[1]} (the rectify maps\' size, else the size the events are voxelised at)')

    def assign(self, recording, mask):
        """recording reads `mask` (None: none) from the next round on; refused, nothing changed, when no slot is free"""
        recording = int(recording)
        if mask is None:
            self.slot_of.pop(recording, None)
            return
        for k, o in enumerate(self.held):
            if o is mask:
                self.slot_of[recording] = k
                return
        named = {k for r, k in self.slot_of.items() if r != recording}
        free = [k for k in range(self.n_slots) if k not in named]
        if not free:
            raise hip.EssHipError(f'set_recording_hot_pixels: all mask_slots={self.n_slots} hold masks that recordings read: build the '
                                  'segmenter with more mask_slots, or take a mask from a recording first (None)')
        k = free[0]
        self.words[k].copy_(torch.from_numpy(mask.words.view(np.int32).copy()))  # (outside any capture)
        self.held[k] = mask
        self.slot_of[recording] = k

    def word(self, recording):
        return self.slot_of.get(int(recording), hip.MASK_NONE)


class _SequenceFeed:
    """one stream's side of the feed: the events fed so far (absolute index of the next one; position in the ring = index mod R),
    the last time fed, the dtypes of its first packet with the format word they give, and the uploads out of the pinned mirror
    still to be waited for -- (the absolute index the packet began at, the event recorded behind its copies), oldest first"""
    __slots__ = ('head', 'last_t', 'dtypes', 'format', 'uploads')

    def __init__(self):
        self.head, self.last_t, self.dtypes, self.format, self.uploads = 0, None, None, None, collections.deque()


class SequenceSegmenter:
    """n_streams event streams, one SEQUENCE ROUND at a time: segment_at(t_end=[...]) or segment_at(end=[...]) cuts, per stream, the
    last sequence_steps x window_events events before the given time (or absolute event index) into sequence_steps equal windows
    -- the DSEC loader's rule, remainder dropped at the end, fewer events than that: what there is, none: no sequence -- and runs
    them from a zero recurrent state -> MultiSegmentationResult (valid[s]: a sequence ran; the rows of the other streams are
    unspecified).  labels=[...]: per stream None or a uint8 [H_out, W_out] ground truth (array or tensor); the round adds
    confusion[s, gt, label] over the pixels whose gt is neither ignore_index nor >= K.  A stream that is idle or has no label this
    round has its ground-truth row filled with ignore_index in front of the round, so its row of `confusion` does not move.

    feed(stream, EventColumns): packets of any size as they arrive, through a pinned mirror into the stream's ring of ring_capacity
    events in device memory (default 2 T N_w, in [T N_w, 2^22], rounded up to a multiple of 16).  No window is pending here and
    nothing is refused for room: old events are overwritten, and segment_at refuses a sequence that reaches behind the ring.
    voxel / rectify_maps / representation: as MultiStreamSegmenter(event_layout='ring').  graph=True: the round's device work -- ring ingest over
    the T S slots, normalisation, T encoder steps, decoder, scoring head -- is captured once (n_captures stays 1); a round is then
    one upload of the slot words, the ground-truth rows that were given, and one replay.  copy, palette, want_confidence, out_hw:
    as StreamingSegmenter.  Each stream's results are those it gets alone (n_streams=1) under the two process-wide batch-size
    switches MultiStreamSegmenter's docstring names.

    confusion: int64 [S, K, K] on the device, accumulated over the rounds; metrics(streams=None) -> {'mean_iou', 'acc', 'cm'} of the
    summed rows (evaluation.metrics' formulas); reset_metrics(streams=None) zeroes rows; drop_feed(streams=None) forgets rings.

    Memory: the T S grids of a round are static buffers -- fp32 [T S, num_bins, H, W] plus the ingest's int64 sums of the same
    shape: at T = 20, S = 8, 5 x 440 x 640 about 0.9 GB + 1.8 GB (num_bins = 10, 'separate_pol' of 5 bins: twice that) -- and the rings take 13 bytes per event on the device and again in
    pinned host memory (T = 20, N_w = 100 000, S = 8: 0.42 GB each).

    The LOADER's grid (all opt-in; with none of these keywords a round goes through hip.event_ingest_ring* as before).  The reference
    loaders do not voxelise at the network's size: they voxelise at the sensor's, normalise the grid over its non-zero voxels, cut
    rows and resize bilinearly.  grid_hw=(Hs, Ws): the size the events are voxelised at (a rectify map stays the sensor's size
    whatever it is); grid_normalize=None | 'unbiased' (VoxelGrid(normalize=True)) | 'population' (normalize_voxel_grid): over all Hs
    rows, in front of the event preprocessor's own normalisation; grid_rows: the top rows kept (default Hs); grid_resize=(Hr, Wr):
    their bilinear resize, align_corners=True (default: none); the top `height` rows of that are the network's input, so Wr == width
    and height <= Hr.  The round then starts with hip.event_scatter_ring* and hip.event_grid_finish: the grids stay a pure function
    of the events.  The two presets:
        DDD17 (ddd17_events_loader.py:162-173): grid_hw=(260, 346), grid_resize=(260, 352), height=200, width=352, voxel='temporal'
        DSEC resize=True (sequence.py:281-287): grid_hw=(480, 640), grid_rows=440, grid_resize=(448, 640), height=448, width=640
    window_duration=d in place of window_events (ring_capacity must then be given): segment_at(t_end=[...]) cuts the DSEC loader's
    fixed_duration windows (datasets.event_feed.sequence_windows_fixed_duration): T windows of d time units ending at t_end.
    segment_at(windows=[...]): per stream None or T explicit (start, count) pairs in absolute event indices -- any other rule, such as
    the DDD17 loader's datasets.event_feed.sequence_windows_by_time.

    hot_pixel_masks=[...]: as MultiStreamSegmenter's -- per stream None or a HotPixelMask of the sensor's size (with every entry
    None: the rectify maps' size, else the size the events are voxelised at), applied to the raw events by hip.event_ingest_masked
    on both ingest heads (with a loader grid: its scatter half, out=None, in front of hip.event_grid_finish); every one of a
    stream's T windows reads that stream's mask.  set_hot_pixels(stream, mask | None) changes it between rounds.

    store=EventStore (datasets/event_store.py), with window_events=N or window_duration=d and window_capacity= as
    EventBatchBuilder(store=) takes them: the rounds are cut on the device out of recordings that lie in device memory already.  No
    rings and no pinned mirrors exist (ring_capacity is refused; feed, fed and drop_feed refuse), and a round is
    segment_at(samples=[StoreSample | None per lane], labels=None).  A LANE is a batch position, not a sensor: any lane may name any
    recording, two lanes may name the same one; n_streams is the number of lanes.  The samples select the window rule -- t_end with
    window_events: the count rule by time, end: by index, t_end with window_duration: the fixed-duration rule -- and all samples of
    a round share it; one capture per rule serves every round.  Inside the capture: hip.event_store_windows over the S lanes (slot
    b T + i), the slot words transposed on the device to the order the encoder reads the grids in (slot i S + s; the grids are not
    moved), hip.event_ingest_store (with a loader grid: its scatter half in front of hip.event_grid_finish), then the round as
    above.  rectify_maps=[...] is then a list of maps and StoreSample.map names an entry.  Ground truth: StoreSample.label, a row of
    the store's labels (store.label_hw must be out_hw; gathered on the device), or labels=[...] from the host, one of the two per
    lane.  last_flags: device int32 [S], hip.EVENT_STORE_FLAG_* as event_store_windows sets them (a lane given None: RANGE); a
    flagged sample or an idle lane does not score -- its ground-truth row is the ignore value, decided on the device from the flag
    word -- and valid[s] says a sample was given.  A round uploads one pinned table of 40 bytes a lane (8 T + 40 under the duration
    rule) and the host labels that were given.  Hot pixels belong to sensors, so here they are keyed by recording:
    recording_hot_pixels={recording: HotPixelMask}, mask_slots=M static slots under the capture (entries that are the same object
    share one), set_recording_hot_pixels(recording, mask | None) between rounds without re-capture; hot_pixel_masks= and
    set_hot_pixels are refused.  Everything is refused before the first device allocation: a store on another device, neither or
    both of window_events / window_duration, window_capacity outside [window_events or 1, 2^22], labels of another size."""

    def __init__(self, encoder, decoder, height, width, options, n_streams, sequence_steps=None, window_events=None, ring_capacity=None,
                 voxel='temporal', rectify_maps=None, graph=False, copy=True, palette=None, want_confidence=False, out_hw=None,
                 ignore_index=255, device=None, window_duration=None, grid_hw=None, grid_rows=None, grid_resize=None,
                 grid_normalize=None, representation=None, hot_pixel_masks=None, store=None, window_capacity=None,
                 recording_hot_pixels=None, mask_slots=16):
        if not isinstance(n_streams, int) or isinstance(n_streams, bool) or n_streams < 1:
            raise hip.EssHipError(f'n_streams={n_streams!r}: a positive number of streams is needed')
        T = sequence_steps
        if not isinstance(T, int) or isinstance(T, bool) or T < 1:
            raise hip.EssHipError(f'sequence_steps={T!r}: the number of windows of a sequence, a positive int (DSEC: nr_events_data = 20)')
        if window_events is not None and window_duration is not None:
            raise hip.EssHipError('give window_events=N or window_duration=d, not both: a sequence is cut by count or by time')
        if window_events is None and window_duration is None:
            raise hip.EssHipError('window_events is needed: the events per window (DSEC: nr_events_window = 100000)')
        self.store = store
        if store is None and (window_capacity is not None or recording_hot_pixels is not None):
            raise hip.EssHipError('window_capacity / recording_hot_pixels belong to a store-fed segmenter: they need store=')
        if store is not None:
            self._check_store(store, device, ring_capacity, hot_pixel_masks, window_events, window_duration, window_capacity, mask_slots,
                              out_hw if out_hw is not None else (height, width))
        self._loader_grid = any(v is not None for v in (grid_hw, grid_rows, grid_resize, grid_normalize))
        Hs, Ws, self._grid = height, width, None
        if self._loader_grid:
            Hs, Ws = self._grid_geometry(height, width, grid_hw, grid_rows, grid_resize, grid_normalize)
        if window_duration is not None:
            d = window_duration
            if isinstance(d, bool) or not isinstance(d, (int, float, np.integer, np.floating)) or not d > 0 or d == float('inf'):
                raise hip.EssHipError(f'window_duration={d!r}: the duration of one window in the unit of t, a positive number')
            if ring_capacity is None and store is None:
                raise hip.EssHipError('window_duration needs ring_capacity: no event count follows from a duration')
            N_w = 0
            _event_capacity(1, Hs, Ws)  # (the coordinates must fit the columns)
        else:
            N_w = _event_capacity(window_events, Hs, Ws)
        self.window_duration = window_duration
        if voxel not in VOXEL_FLAVOURS:
            raise hip.EssHipError(f'voxel={voxel!r}: one of {VOXEL_FLAVOURS}')
        if not isinstance(ignore_index, int) or isinstance(ignore_index, bool) or not 0 <= ignore_index <= 255:
            raise hip.EssHipError(f'ignore_index={ignore_index!r}: a value of the uint8 ground truth is needed')
        R = 2 * T * N_w if ring_capacity is None else ring_capacity
        # (with a store no ring exists: the windows are read where the store keeps them)
        if store is None and (not isinstance(R, int) or isinstance(R, bool) or R < max(1, T * N_w) or
                              hip.event_column_stride(R) > hip.INGEST_MAX_CAPACITY):
            raise hip.EssHipError(f'ring_capacity={R!r}: events per stream the ring holds, an int in [sequence_steps * window_events = '
                                  f'{T * N_w}, {hip.INGEST_MAX_CAPACITY}] (default: twice the lower bound)')
        self.n_streams, self.sequence_steps, self.window_events = n_streams, T, (N_w if window_duration is None else None)
        self.ring_capacity = R = None if store is not None else hip.event_column_stride(R)
        self.voxel, self.ignore_index = voxel, ignore_index
        self.representation = representation
        self._rep = _event_representation(representation, voxel, rectify_maps, encoder.num_bins)
        if hot_pixel_masks is not None:
            _check_hot_pixel_masks(hot_pixel_masks, n_streams, None)  # (the last refusal before the device)
        if store is not None:  # (the store's own last refusals before the device: the maps' list, the masks' sizes)
            maps_host, self._map_entry = _rectify_maps(rectify_maps, voxel, len(rectify_maps) if isinstance(rectify_maps, (list, tuple)) else 0)
            mask_size = tuple(maps_host.shape[1:3]) if maps_host is not None else (Hs, Ws)
            hot_given = self._check_recording_masks(recording_hot_pixels, mask_size, mask_slots)
        self.copy_outputs = bool(copy)
        self.device = device if device is not None else torch.device('cuda:0')
        self.model = encoder.to(self.device).eval()
        self.decoder = decoder.to(self.device).eval()
        self.rec = ImageReconstructor(self.model, height, width, encoder.num_bins, self.device, options)
        if self.rec.no_recurrent:
            raise hip.EssHipError('SequenceSegmenter: options.no_recurrent leaves no sequence to run')
        if self.rec.event_preprocessor.no_normalize:
            raise hip.EssHipError('SequenceSegmenter: options.no_normalize is not supported')
        self.height, self.width, self.num_bins = height, width, encoder.num_bins
        crop = self.rec.crop
        self.window = (crop.iy0, crop.ix0, crop.iy1 - crop.iy0, crop.ix1 - crop.ix0)
        self.out_hw = (height, width) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        self.palette = None if palette is None else torch.as_tensor(palette).to(self.device).contiguous()
        self.want_confidence = bool(want_confidence)
        self.use_graph = graph
        self.n_rounds = 0
        self.n_captures = 0
        self.compute = hip.compute_name()
        self.num_classes = K = int(self.decoder.decoder_scale_5[0].weight.shape[0])
        S, dev = n_streams, self.device
        self._hot = None
        self._g = self._outputs = None
        self._in = torch.zeros(T * S, self.num_bins, height, width, dtype=torch.float32, device=dev)
        self._acc = torch.zeros(T * S, self.num_bins, Hs, Ws, dtype=torch.int64, device=dev)  # (the size the events are voxelised at)
        self._gt = torch.full((S,) + self.out_hw, ignore_index, dtype=torch.uint8, device=dev)
        self.confusion = torch.zeros(S, K, K, dtype=torch.int64, device=dev)
        if store is not None:  # no rings, no mirrors, no ring words: one small table a round
            self._maps = None if maps_host is None else maps_host.to(dev)
            self._feeds = self._ring = self._ring_host = self._ring_np = self._words = None
            self._stage, self._gt_live = [], [False] * S
            self._rec_hot = _RecordingMasks(mask_slots, mask_size, dev)
            for r, m in hot_given:
                self._rec_hot.assign(r, m)
            self._allocate_store()
            return
        maps, self._map_of = _rectify_maps(rectify_maps, voxel, n_streams)
        self._maps = None if maps is None else maps.to(self.device)  # (uploaded once, here)
        dtypes = (torch.int64, torch.int16, torch.int16, torch.uint8)
        self._feeds = [_SequenceFeed() for _ in range(S)]
        self._ring = tuple(torch.zeros(S, R, dtype=d, device=dev) for d in dtypes)
        self._ring_host = tuple(torch.zeros(S, R, dtype=d).pin_memory() for d in dtypes)
        self._ring_np = tuple(c.numpy() for c in self._ring_host)
        n_words = 5 if voxel == 'trilinear' else 4  # (rows, starts, counts, formats; the map words behind them)
        if hot_pixel_masks is not None:  # (the mask words behind the map words, which are then always there: -1 is NONE for both)
            n_words = 6
            self._hot = _HotPixelSlots(hot_pixel_masks, n_streams, tuple(maps.shape[1:3]) if maps is not None else (Hs, Ws), dev)
        self._words = torch.zeros(n_words, T * S, dtype=torch.int32, device=dev)
        self._words[4:].fill_(hip.RECTIFY_NONE)
        self._gt_live = [False] * S  # (host: the stream's row of _gt holds a ground truth, not the ignore fill)
        self._stage = []
        for _ in range(2):
            words = torch.zeros(n_words, T * S, dtype=torch.int32).pin_memory()
            words[4:].fill_(hip.RECTIFY_NONE)
            self._stage.append(_SequenceStage(words, torch.zeros((S,) + self.out_hw, dtype=torch.uint8).pin_memory(), torch.cuda.Event()))
        self._stage_next = 0

    # ---- the store source (store=EventStore): no rings, no mirrors; one small table a round
    def _check_store(self, store, device, ring_capacity, hot_pixel_masks, window_events, window_duration, window_capacity, mask_slots, out_hw):
        """the store keywords, checked on the host -> self.window_capacity"""
        from .datasets.event_store import EventStore
        if not isinstance(store, EventStore):
            raise hip.EssHipError(f'store must be an EventStore, got {type(store).__name__}')
        if device is not None and torch.device(device) != torch.device(store.device):
            raise hip.EssHipError(f'device={device!r}: a store-fed segmenter runs where the store lies ({store.device})')
        if ring_capacity is not None:
            raise hip.EssHipError(f'ring_capacity={ring_capacity!r} together with store=: a store-fed segmenter has no rings, its windows are '
                                  'read where the store keeps them')
        if hot_pixel_masks is not None:
            raise hip.EssHipError('hot_pixel_masks= is keyed by stream; with store= a lane may name any recording: give '
                                  'recording_hot_pixels={recording: HotPixelMask}')
        low = 1
        if window_events is not None:
            if isinstance(window_events, bool) or not isinstance(window_events, int) or not 1 <= window_events <= hip.INGEST_MAX_CAPACITY:
                raise hip.EssHipError(f'window_events={window_events!r}: an int in [1, {hip.INGEST_MAX_CAPACITY}]')
            low = window_events
            window_capacity = window_events if window_capacity is None else window_capacity
        elif window_capacity is None:
            raise hip.EssHipError('window_duration needs window_capacity=: the most events a window may hold (a larger one flags its sample)')
        if isinstance(window_capacity, bool) or not isinstance(window_capacity, int) or not low <= window_capacity <= hip.INGEST_MAX_CAPACITY:
            raise hip.EssHipError(f'window_capacity={window_capacity!r}: an int in [window_events or 1 = {low}, {hip.INGEST_MAX_CAPACITY}]')
        if isinstance(mask_slots, bool) or not isinstance(mask_slots, int) or not 1 <= mask_slots <= 65535:
            raise hip.EssHipError(f'mask_slots={mask_slots!r}: the static hot-pixel mask slots under the capture, an int in [1, 65535]')
        if store.label_hw is not None and tuple(store.label_hw) != (int(out_hw[0]), int(out_hw[1])):
            raise hip.EssHipError(f'the store keeps labels of {store.label_hw}, this segmenter scores at out_hw={tuple(out_hw)}: a '
                                  'StoreSample.label is compared as it lies in the store')
        self.window_capacity = window_capacity

    @staticmethod
    def _check_recording_masks(given, size, mask_slots):
        """recording_hot_pixels={recording: HotPixelMask | None}, checked on the host -> [(recording, mask)]"""
        if given is None:
            return []
        if not isinstance(given, dict):
            raise hip.EssHipError(f'recording_hot_pixels must be a dict recording -> HotPixelMask, got {type(given).__name__}')
        for r, m in given.items():
            _RecordingMasks.check('recording_hot_pixels', r, m, size)
        distinct = {id(m) for m in given.values() if m is not None}
        if len(distinct) > mask_slots:
            raise hip.EssHipError(f'recording_hot_pixels names {len(distinct)} distinct masks, mask_slots={mask_slots} slots hold them')
        return [(int(r), m) for r, m in given.items() if m is not None]

    def _store_layout(self):
        """the per-round table, in bytes: name -> (offset, dtype, shape); 40 bytes a lane (8 T + 40 under the duration rule)"""
        S, T = self.n_streams, self.sequence_steps
        n_bounds = T + 1 if self.window_duration is not None else 1
        at, out = 0, {}
        for name, dtype, shape in (('bounds', torch.int64, (S, n_bounds)), ('label_of', torch.int64, (S,)), ('recording', torch.int32, (S,)),
                                   ('sample_map', torch.int32, (S,)), ('mask_of', torch.int32, (S,)), ('gt_mode', torch.int32, (S,)),
                                   ('reserved', torch.int64, (S,))):
            out[name] = (at, dtype, shape)
            at += -(-int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size() // 16) * 16
        return out, at

    def _allocate_store(self):
        S, T, dev = self.n_streams, self.sequence_steps, self.device
        layout, nbytes = self._store_layout()
        views = lambda buf: {name: buf[at:at + int(np.prod(shape)) * torch.empty(0, dtype=d).element_size()].view(d).view(shape)  # noqa: E731
                             for name, (at, d, shape) in layout.items()}
        table = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        stage = []
        for _ in range(2):
            host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            gt = torch.zeros((S,) + self.out_hw, dtype=torch.uint8).pin_memory()
            stage.append({'buf': host, 'np': {n: v.numpy() for n, v in views(host).items()}, 'gt': gt, 'gt_np': gt.numpy(),
                          'done': torch.cuda.Event()})
        self._st = {
            'table': table, 'in': views(table), 'stage': stage,
            'starts_bt': torch.zeros(S * T, dtype=torch.int64, device=dev),           # as event_store_windows writes them: slot b T + i
            'words_bt': torch.zeros(3, S * T, dtype=torch.int32, device=dev),        # counts, formats, map words
            'starts': torch.zeros(T * S, dtype=torch.int64, device=dev),              # as the encoder reads the grids: slot i S + s
            'words': torch.zeros(4, T * S, dtype=torch.int32, device=dev),           # counts, formats, map words, mask words
            'flags': torch.zeros(S, dtype=torch.int32, device=dev),
            'gt_host': torch.full((S,) + self.out_hw, self.ignore_index, dtype=torch.uint8, device=dev),
            'gt_store': None if self.store.label_hw is None else torch.zeros((S,) + self.out_hw, dtype=torch.uint8, device=dev),
        }
        self._stage_next = 0
        self._store_graphs = {}
        self.last_flags = self._st['flags']

    def _round_store(self, rule):
        """the device work of one store round, all of it capturable: the window search over the S lanes, the slot words transposed from
        sample-major to step-major, the (masked) store ingest, the ground truth picked per lane from its flag word, the round"""
        st, store, T, S = self._st, self.store, self.sequence_steps, self.n_streams
        tin, ev = st['in'], self._in
        counts_bt, formats_bt, maps_bt = st['words_bt']
        with torch.no_grad():
            # (total = the capacity: the search keeps every window inside its recording's table row, so a replayed graph serves
            # recordings that were added after its capture)
            hip.event_store_windows(store.columns[0], store.table, tin['recording'], tin['bounds'], rule, T, st['starts_bt'], counts_bt,
                                    formats_bt, st['flags'], store.capacity, self.window_capacity,
                                    n_per_window=self.window_events if self.window_duration is None else None,
                                    sample_map=tin['sample_map'], map_of=maps_bt)
            w = st['words']
            st['starts'].view(T, S).copy_(st['starts_bt'].view(S, T).t())
            w[:3].view(3, T, S).copy_(st['words_bt'].view(3, S, T).transpose(1, 2))
            w[3].view(T, S).copy_(tin['mask_of'].view(1, S).expand(T, S))  # (a lane's T windows read the mask of its sample's recording)
            tri = self.voxel == 'trilinear'
            hip.event_ingest_store(*store.columns, st['starts'], w[0], w[1], None if self._loader_grid else ev,
                                   hip.EVENT_STORE_TRILINEAR if tri else self._rep, store.capacity, self.window_capacity,
                                   masks=self._rec_hot.words, mask_of=w[3], mask_size=self._rec_hot.size,
                                   maps=self._maps if tri else None, map_of=w[2] if tri else None, acc=self._acc)
            if self._loader_grid:
                crop_rows, resize, normalize = self._grid
                hip.event_grid_finish(w[0], self._acc, ev, crop_rows=crop_rows, resize=resize, normalize=normalize)
            # the ground truth: gt_mode 0 none, 1 the store's label, 2 the host's; a flagged lane must not score, whatever it was handed
            mode, gt = tin['gt_mode'].view(S, 1, 1), st['gt_host']
            if st['gt_store'] is not None:
                torch.index_select(store.labels, 0, tin['label_of'], out=st['gt_store'])
                gt = torch.where(mode == 1, st['gt_store'], gt)
            live = (st['flags'].view(S, 1, 1) == 0) & (mode != 0)
            self._gt.copy_(torch.where(live, gt, torch.full_like(gt, self.ignore_index)))
            return self._round_from(ev)

    def _capture_store(self, rule):
        """one eager run on a side stream, then the recording.  Neither may score: every lane is idle (recording -1) in the table"""
        st = self._st
        st['table'].zero_()
        st['in']['recording'].fill_(-1)
        st['in']['mask_of'].fill_(hip.MASK_NONE)
        st['in']['sample_map'].fill_(hip.RECTIFY_NONE)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._round_store(rule)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = self._round_store(rule)
        self._store_graphs[rule] = (g, out)
        self.n_captures += 1

    def _check_samples(self, samples):
        """segment_at's samples=[...] of a store-fed segmenter, checked; nothing is written -> (rule, bound words per lane or None)"""
        from .datasets.event_store import StoreSample, duration_bounds, time_bound
        S, T, store = self.n_streams, self.sequence_steps, self.store
        if not isinstance(samples, (list, tuple)) or len(samples) != S or any(s is not None and not isinstance(s, StoreSample) for s in samples):
            n = len(samples) if isinstance(samples, (list, tuple)) else type(samples).__name__
            raise hip.EssHipError(f'samples must be a list with one entry per lane (a StoreSample, or None: idle): got {n}, n_streams={S}')
        given = [s for s in samples if s is not None]
        by_time = given[0].t_end is not None if given else True
        if any((s.t_end is not None) != by_time for s in given):
            raise hip.EssHipError('samples: t_end for every sample of the round, or end for every one (one rule per launch)')
        by_count = self.window_duration is None
        if not by_time and not by_count:
            raise hip.EssHipError('window_duration cuts by time: its samples need t_end, not end')
        rule = hip.EVENT_STORE_RULE_DURATION if not by_count else \
            (hip.EVENT_STORE_RULE_COUNT_TIME if by_time else hip.EVENT_STORE_RULE_COUNT_INDEX)
        bounds = []
        for b, s in enumerate(samples):
            if s is None:
                bounds.append(None)
                continue
            if s.recording >= store.n_recordings:
                raise hip.EssHipError(f'samples[{b}] names recording {s.recording}, the store holds {store.n_recordings}')
            if s.label is not None and (store.label_hw is None or s.label >= store.n_labels):
                raise hip.EssHipError(f'samples[{b}]: label index {s.label} of the store\'s {store.n_labels} labels')
            if s.map is not None and s.map >= len(self._map_entry):
                raise hip.EssHipError(f'samples[{b}]: map index {s.map!r} of the segmenter\'s {len(self._map_entry)} rectify_maps')
            begin, end = store.extent(s.recording)
            if not by_time:
                if s.end > end - begin:
                    raise hip.EssHipError(f'samples[{b}]: end={s.end} of recording {s.recording}\'s {end - begin} events')
                bounds.append([s.end])
                continue
            t_i64 = bool(store.format_of(s.recording) & hip.EVCOL_T_I64)
            t_end = s.t_end - store.t_offset(s.recording)
            bounds.append([time_bound(v, t_i64) for v in ([t_end] if by_count else duration_bounds(t_end, T, self.window_duration))])
        return rule, bounds

    def _segment_store(self, samples, labels):
        rule, bounds = self._check_samples(samples)
        gts = self._check_labels(labels)
        S = self.n_streams
        for s, (smp, g) in enumerate(zip(samples, gts)):
            if smp is not None and smp.label is not None and g is not None:
                raise hip.EssHipError(f'lane {s} is handed a label by its StoreSample (label={smp.label}) and by labels=[...]: one of the two')
        if self.store.n_recordings == 0:
            raise hip.EssHipError('the store holds no recording')
        if self.use_graph and rule not in self._store_graphs:
            self._capture_store(rule)
        st = self._st
        stage = st['stage'][self._stage_next]
        self._stage_next ^= 1
        stage['done'].synchronize()  # (the set's last upload has completed: it is free to be rewritten)
        w = stage['np']
        w['bounds'][:] = 0
        w['label_of'][:] = 0
        w['reserved'][:] = 0
        for s, (smp, g) in enumerate(zip(samples, gts)):
            if smp is None:  # (recording -1: the search flags the lane, its windows are empty, its ground truth is the ignore fill)
                w['recording'][s], w['sample_map'][s], w['mask_of'][s], w['gt_mode'][s] = -1, hip.RECTIFY_NONE, hip.MASK_NONE, 0
                continue
            w['bounds'][s, :len(bounds[s])] = bounds[s]
            w['recording'][s] = smp.recording
            w['sample_map'][s] = hip.RECTIFY_NONE if smp.map is None else self._map_entry[smp.map]
            w['mask_of'][s] = self._rec_hot.word(smp.recording)
            w['gt_mode'][s] = 1 if smp.label is not None else (2 if g is not None else 0)
            if smp.label is not None:
                w['label_of'][s] = smp.label
            if g is not None:
                if torch.is_tensor(g):
                    st['gt_host'][s].copy_(g, non_blocking=True)
                else:
                    np.copyto(stage['gt_np'][s], g)
                    st['gt_host'][s].copy_(stage['gt'][s], non_blocking=True)
        st['table'].copy_(stage['buf'], non_blocking=True)
        stage['done'].record()
        if self.use_graph:
            g, out = self._store_graphs[rule]
            g.replay()
        else:
            out = self._round_store(rule)
        self.n_rounds += 1
        res = MultiSegmentationResult(*out, valid=[smp is not None for smp in samples])
        return res.clone() if (self.use_graph and self.copy_outputs) else res

    def set_recording_hot_pixels(self, recording, mask):
        """a store-fed segmenter: the lanes that name `recording` read `mask` (a HotPixelMask of the segmenter's sensor size, or None)
        in every one of their T windows from the next round on.  The words go into a slot of the static mask buffer here, outside the
        capture; no re-capture.  Entries that are the same object share a slot; with every slot taken the call is refused and
        nothing changes."""
        if self.store is None:
            raise hip.EssHipError('set_recording_hot_pixels belongs to a store-fed segmenter (store=); this one reads rings: set_hot_pixels')
        _RecordingMasks.check('set_recording_hot_pixels', recording, mask, self._rec_hot.size)
        self._rec_hot.assign(recording, mask)

    def _no_feed(self, what):
        if self.store is not None:
            raise hip.EssHipError(f'{what}: this segmenter reads an EventStore (store=), it has no rings to feed: add recordings to the '
                                  'store and name them in segment_at(samples=[StoreSample, ...])')

    def _grid_geometry(self, height, width, grid_hw, grid_rows, grid_resize, grid_normalize):
        """the loader-grid keywords, checked -> (Hs, Ws); self._grid = (crop_rows, (Hr, Wr), hip.GRID_NORM_*)"""
        def pair(name, v):
            if not isinstance(v, (tuple, list)) or len(v) != 2 or any(isinstance(a, bool) or not isinstance(a, int) or a < 1 for a in v):
                raise hip.EssHipError(f'{name}={v!r}: a pair of positive ints (rows, columns) is needed')
            return int(v[0]), int(v[1])
        Hs, Ws = (height, width) if grid_hw is None else pair('grid_hw', grid_hw)
        rows = Hs if grid_rows is None else grid_rows
        if isinstance(rows, bool) or not isinstance(rows, int) or not 1 <= rows <= Hs:
            raise hip.EssHipError(f'grid_rows={rows!r}: the top rows of the {Hs} x {Ws} grid that are kept, an int in [1, {Hs}]')
        Hr, Wr = (rows, Ws) if grid_resize is None else pair('grid_resize', grid_resize)
        if Wr != width or height > Hr:
            raise hip.EssHipError(f'the loader grid ends as {Hr} x {Wr} (grid_resize, or grid_rows x the grid\'s width), the network reads its '
                                  f'top {height} rows of {width} columns: the widths must agree and height <= {Hr}')
        norms = {None: hip.GRID_NORM_NONE, 'unbiased': hip.GRID_NORM_UNBIASED, 'population': hip.GRID_NORM_POPULATION}
        if not isinstance(grid_normalize, (str, type(None))) or grid_normalize not in norms:
            raise hip.EssHipError(f"grid_normalize={grid_normalize!r}: None, 'unbiased' (VoxelGrid(normalize=True)) or 'population' "
                                  '(normalize_voxel_grid)')
        self._grid = (rows, (Hr, Wr), norms[grid_normalize])
        return Hs, Ws

    @classmethod
    def from_checkpoints(cls, e2vid_path, ess_checkpoint_path, settings_or_kwargs, n_streams, **kw):
        """as StreamingSegmenter.from_checkpoints, plus the number of streams; sequence_steps, window_events and the rest: keywords"""
        encoder, decoder, height, width, options, palette = _models_from_checkpoints(e2vid_path, ess_checkpoint_path, settings_or_kwargs)
        kw.setdefault('palette', palette)
        return cls(encoder, decoder, height, width, options, n_streams, **kw)

    # ---- the feed
    def _stream(self, stream, what):
        if not isinstance(stream, (int, np.integer)) or isinstance(stream, bool) or not 0 <= stream < self.n_streams:
            raise hip.EssHipError(f'{what}: stream {stream!r} of n_streams={self.n_streams}')
        return int(stream)

    def feed(self, stream, cols):
        """A packet of a stream's events as it arrives (datasets.data_util.EventColumns; the times non-decreasing, also from packet to
        packet) -> the number of events the stream has been fed.  The packet is copied as it is into the pinned mirror at head mod R --
        at most two segments per column -- and those segments go to the device ring on the current stream, non-blocking; of a packet
        larger than the ring only its last R events are kept.  Refused before anything is written: another object than an
        EventColumns, other dtypes than the stream's first packet had (drop_feed forgets them), a packet that goes back in time."""
        from .datasets.data_util import EventColumns
        from .datasets.event_feed import copy_into_ring
        self._no_feed('feed')
        s = self._stream(stream, 'feed')
        f = self._feeds[s]
        if not isinstance(cols, EventColumns):
            raise hip.EssHipError(f'feed: an EventColumns is needed, got {type(cols).__name__}: hand the columns over as they arrive, '
                                  'EventColumns(t, x, y, p)')
        if cols.n == 0:
            return f.head
        dtypes = (cols.t.dtype, cols.x.dtype)
        if f.dtypes is not None and dtypes != f.dtypes:
            raise hip.EssHipError(f'feed: stream {s} delivers t {f.dtypes[0]} and x / y {f.dtypes[1]} since its first packet, this packet has '
                                  f'{dtypes[0]} and {dtypes[1]}: a ring holds one format (drop_feed([{s}]) starts afresh)')
        first = cols.t[0].item()
        if f.last_t is not None and first < f.last_t:
            raise hip.EssHipError(f'feed: the packet starts at t={first!r}, before the previous packet\'s last time {f.last_t!r}: packets must '
                                  'be non-decreasing in t')
        R, head, last = self.ring_capacity, f.head, cols.t[-1].item()
        if cols.n > R:  # (the ring keeps the last R events anyway)
            head += cols.n - R
            cols = EventColumns(cols.t[-R:], cols.x[-R:], cols.y[-R:], cols.p[-R:])
        f.dtypes, f.format = dtypes, cols.format
        # the pinned entries about to be rewritten held the events [head - R, head + n - R): the uploads that read them must be over
        while f.uploads and (f.uploads[0][0] < head + cols.n - R or f.uploads[0][1].query()):
            f.uploads.popleft()[1].synchronize()
        for at, _, m in copy_into_ring(cols, tuple(c[s] for c in self._ring_np), head, R):
            for dev, host in zip(self._ring, self._ring_host):
                dev[s, at:at + m].copy_(host[s, at:at + m], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        f.uploads.append((head, done))
        f.head, f.last_t = head + cols.n, last
        return f.head

    def fed(self, stream):
        """the number of events the stream has been fed (the absolute index of its next event)"""
        self._no_feed('fed')
        return self._feeds[self._stream(stream, 'fed')].head

    def drop_feed(self, streams=None):
        """these streams (default: all) forget their ring contents and their dtypes: the next packet is event 0 of a new recording.
        The confusion rows are reset_metrics' business, not this call's."""
        self._no_feed('drop_feed')
        for s in (range(self.n_streams) if streams is None else streams):
            s = self._stream(s, 'drop_feed')
            for _, done in self._feeds[s].uploads:  # (the new recording writes the mirror from entry 0 on)
                done.synchronize()
            self._feeds[s] = _SequenceFeed()

    # ---- hot-pixel masks
    def set_hot_pixels(self, stream, mask):
        """stream reads `mask` (a datasets.hot_pixels.HotPixelMask of the segmenter's sensor size, or None) in every one of its T
        windows from the next round on: the words go into the static mask buffer here, outside the capture; no re-capture"""
        if self.store is not None:
            raise hip.EssHipError('set_hot_pixels is keyed by stream; this segmenter reads an EventStore (store=), whose masks are keyed by '
                                  'recording: set_recording_hot_pixels(recording, mask)')
        if self._hot is None:
            raise hip.EssHipError('set_hot_pixels: this segmenter was built without hot_pixel_masks, so no mask buffer exists under its '
                                  'capture: pass hot_pixel_masks=[...] (a list of None will do)')
        self._hot.assign(self._stream(stream, 'set_hot_pixels'), mask)

    # ---- metrics
    def _rows(self, streams, what):
        return list(range(self.n_streams)) if streams is None else [self._stream(s, what) for s in streams]

    def metrics(self, streams=None):
        """-> {'mean_iou', 'acc', 'iou_per_class', 'cm'} of these streams' (default: all) summed confusion rows: one host read, the
        formulas of evaluation.metrics (MetricsSemseg.get_metrics_summary's)"""
        rows = self._rows(streams, 'metrics')
        cm = self.confusion[rows].sum(dim=0).cpu()
        mean_iou, per_class = semseg_accum_confusion_to_iou(cm)
        return {'mean_iou': mean_iou, 'acc': semseg_accum_confusion_to_acc(cm), 'iou_per_class': per_class, 'cm': cm}

    def reset_metrics(self, streams=None):
        """these streams' (default: all) rows of `confusion` start again from zero"""
        if streams is None:
            self.confusion.zero_()
        else:
            for s in self._rows(streams, 'reset_metrics'):
                self.confusion[s].zero_()

    # ---- one round
    def _round(self):
        """the device work of one sequence round on the static rings, words and ground truth -> (labels, colour, confidence)"""
        with torch.no_grad():
            ev = self._in
            tri, w = self.voxel == 'trilinear', self._words  # (rows, starts, counts, formats; the map words; the mask words)
            # the loader's grid: scatter only -- the sums at the size the loader voxelises at -- then its normalise / cut / resize
            hip.event_voxels('ring', self._ring, w[:4], None if self._loader_grid else ev, self._acc, representation=self._rep, trilinear=tri,
                             maps=self._maps, map_of=w[4] if tri else None,
                             masks=None if self._hot is None else (self._hot.words, w[5], self._hot.size))
            if self._loader_grid:
                crop_rows, resize, normalize = self._grid
                hip.event_grid_finish(w[2], self._acc, ev, crop_rows=crop_rows, resize=resize, normalize=normalize)
            return self._round_from(ev)

    def _round_from(self, ev):
        """the round behind its grids: ev fp32 [T S, num_bins, height, width] (the round's own buffer, or -- tools/bench_seg_stream.py --
        grids put together another way) -> (labels, colour, confidence)"""
        rec, pre = self.rec, self.rec.event_preprocessor
        T, S = self.sequence_steps, self.n_streams
        with torch.no_grad():
            for x, y in pre.hot_pixel_locations:
                ev[:, :, y, x] = 0
            if pre.flip:
                ev = torch.flip(ev, dims=[2, 3]).contiguous()
            ev = rec.crop.pad(hip.event_normalize_samples(ev))  # (per slot: a window's statistics are its own; an idle slot: zeros)
            if not ev.is_contiguous():
                ev = ev.contiguous()
            rec.last_states_for_each_channel = {'grayscale': None}  # every sequence runs from a zero state
            try:
                _, _, latent = rec.update_reconstruction_sequence(None, T, need_image=False, final_lean=True,
                                                                  slices=ev.view(T, S, *ev.shape[1:]))
            finally:
                rec.last_states_for_each_channel = {'grayscale': None}
            return self.decoder.predict(latent, out_hw=self.out_hw, window=self.window, palette=self.palette,
                                        want_confidence=self.want_confidence, gt=self._gt, confusion=self.confusion,
                                        ignore_index=self.ignore_index)

    def _capture(self):
        """one eager run on a side stream, then the recording on the current stream.  The warm-up run must not score: every slot is
        empty and every ground-truth row holds the ignore fill during it."""
        self._words[2].zero_()
        self._gt.fill_(self.ignore_index)
        self._gt_live = [False] * self.n_streams
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._round()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g):
            self._outputs = self._round()
        self.n_captures += 1

    def _next_stage(self):
        """the staging set of this round, free to be rewritten: its last upload has completed"""
        st = self._stage[self._stage_next]
        self._stage_next ^= 1
        st.done.synchronize()
        return st

    def _check_labels(self, labels):
        """labels: None or S entries, each None or a uint8 [H_out, W_out] array / tensor -> list of S (None | numpy | device tensor)"""
        S = self.n_streams
        if labels is None:
            return [None] * S
        if not isinstance(labels, (list, tuple)) or len(labels) != S:
            n = len(labels) if isinstance(labels, (list, tuple)) else type(labels).__name__
            raise hip.EssHipError(f'labels must be a list with one entry per stream (a ground truth or None): got {n}, n_streams={S}')
        out = []
        for s, g in enumerate(labels):
            if g is not None:
                if not (torch.is_tensor(g) or isinstance(g, np.ndarray)):
                    raise hip.EssHipError(f'labels[{s}] must be a uint8 {list(self.out_hw)} array or tensor or None, got {type(g).__name__}')
                if g.dtype != (torch.uint8 if torch.is_tensor(g) else np.uint8) or tuple(g.shape) != self.out_hw:
                    raise hip.EssHipError(f'labels[{s}] must be uint8 {list(self.out_hw)} (the output size), got {g.dtype}{tuple(g.shape)}')
                if torch.is_tensor(g) and not g.is_cuda:
                    g = g.numpy()
            out.append(g)
        return out

    def _ends(self, t_end, end):
        """the round's request -> per stream None (idle) or the absolute index its sequence ends in front of"""
        from .datasets.event_feed import ring_end_index
        S, R, need = self.n_streams, self.ring_capacity, self.sequence_steps * self.window_events
        if (t_end is None) == (end is None):
            raise hip.EssHipError('segment_at: give t_end=[...] (times) or end=[...] (absolute event indices), one of the two')
        req, what = (t_end, 't_end') if end is None else (end, 'end')
        if not isinstance(req, (list, tuple)) or len(req) != S:
            n = len(req) if isinstance(req, (list, tuple)) else type(req).__name__
            raise hip.EssHipError(f'{what} must be a list with one entry per stream (None: idle): got {n}, n_streams={S}')
        out = []
        for s, (v, f) in enumerate(zip(req, self._feeds)):
            if v is None or f.head == 0:
                out.append(None)
            elif end is None:
                out.append(ring_end_index(self._ring_np[0][s].view(f.dtypes[0]), f.head, R, v, need=need))
            else:
                if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= v <= f.head:
                    raise hip.EssHipError(f'end[{s}]={v!r}: an absolute event index in [0, {f.head}] (the events fed) is needed')
                if max(0, int(v) - need) < f.head - R:
                    raise hip.EssHipError(f'end[{s}]={v}: the sequence reaches back to event {max(0, int(v) - need)}, the ring of {R} keeps '
                                          f'events from {f.head - R} on')
                out.append(int(v))
        return out

    def _check_compute(self):
        if hip.compute_name() != self.compute:
            raise hip.EssHipError(f"SequenceSegmenter: built in the '{self.compute}' configuration, called in '{hip.compute_name()}'")

    def _explicit_windows(self, windows):
        """segment_at's windows=[...] -> per stream None or T pairs (start, count), every one checked against the events the ring keeps"""
        T, S, R = self.sequence_steps, self.n_streams, self.ring_capacity
        if not isinstance(windows, (list, tuple)) or len(windows) != S:
            n = len(windows) if isinstance(windows, (list, tuple)) else type(windows).__name__
            raise hip.EssHipError(f'windows must be a list with one entry per stream (None: idle): got {n}, n_streams={S}')
        out = []
        for s, (w, f) in enumerate(zip(windows, self._feeds)):
            if w is None:
                out.append(None)
                continue
            if not isinstance(w, (list, tuple)) or len(w) != T:
                n = len(w) if isinstance(w, (list, tuple)) else type(w).__name__
                raise hip.EssHipError(f'windows[{s}] must hold sequence_steps={T} pairs (start, count): got {n}')
            pairs = []
            for i, v in enumerate(w):
                if not isinstance(v, (list, tuple)) or len(v) != 2 or \
                        any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in v):
                    raise hip.EssHipError(f'windows[{s}][{i}]={v!r}: a pair of ints (start, count) in absolute event indices is needed')
                start, count = int(v[0]), int(v[1])
                if start < 0 or count < 0 or start + count > f.head:
                    raise hip.EssHipError(f'windows[{s}][{i}]=({start}, {count}): the events [{start}, {start + count}) are not all among the '
                                          f'{f.head} events fed')
                if count > 0 and start < f.head - R:
                    raise hip.EssHipError(f'windows[{s}][{i}]=({start}, {count}): the window reaches back to event {start}, the ring of {R} '
                                          f'keeps events from {f.head - R} on')
                pairs.append((start, count))
            out.append(pairs)
        return out

    def _duration_windows(self, t_end):
        """segment_at's t_end=[...] of a window_duration segmenter -> per stream None (idle) or the loader's fixed_duration windows"""
        from .datasets.event_feed import sequence_windows_fixed_duration
        S, R = self.n_streams, self.ring_capacity
        if not isinstance(t_end, (list, tuple)) or len(t_end) != S:
            n = len(t_end) if isinstance(t_end, (list, tuple)) else type(t_end).__name__
            raise hip.EssHipError(f't_end must be a list with one entry per stream (None: idle): got {n}, n_streams={S}')
        return [None if v is None or f.head == 0 else
                sequence_windows_fixed_duration(self._ring_np[0][s].view(f.dtypes[0]), f.head, R, v, self.sequence_steps, self.window_duration)
                for s, (v, f) in enumerate(zip(t_end, self._feeds))]

    def segment_at(self, t_end=None, end=None, labels=None, windows=None, samples=None):
        """One sequence round.  t_end / end: S entries -- a time (the sequence ends in front of the first event with t >= t_end, as
        the reference's get_events_fixed_num; with window_duration: the T windows of that duration in front of t_end) / an absolute
        event index, or None for an idle stream; windows: S entries, each None or sequence_steps pairs (start, count) in absolute
        event indices, a count of 0 being a window without events; exactly one of the three lists.
        labels: None or S entries, each None or the stream's uint8 [H_out, W_out] ground truth.  Everything is checked before
        anything is written.  -> MultiSegmentationResult"""
        from .datasets.event_feed import sequence_windows
        self._check_compute()
        if self.store is not None:
            if samples is None or t_end is not None or end is not None or windows is not None:
                raise hip.EssHipError('segment_at: a store-fed segmenter (store=) takes samples=[StoreSample | None per lane] alone: the '
                                      'samples name their recordings and their ends')
            return self._segment_store(samples, labels)
        if samples is not None:
            raise hip.EssHipError('segment_at: samples=[...] name recordings of an EventStore: build the segmenter with store=')
        T, S, R = self.sequence_steps, self.n_streams, self.ring_capacity
        if windows is not None:
            if t_end is not None or end is not None:
                raise hip.EssHipError('segment_at: windows=[...] names the windows themselves: give it without t_end and end')
            wins = self._explicit_windows(windows)
        elif self.window_duration is not None:
            if end is not None or t_end is None:
                raise hip.EssHipError('segment_at: a window_duration segmenter cuts by time: give t_end=[...] (or windows=[...])')
            wins = self._duration_windows(t_end)
        else:
            wins = [None if e is None else sequence_windows(e, 0, T, self.window_events) for e in self._ends(t_end, end)]
        gts = self._check_labels(labels)
        on = [w is not None for w in wins]
        if self.use_graph and self._g is None:
            self._capture()
        st = self._next_stage()
        st.rows_np[:] = np.tile(np.arange(S, dtype=np.int32), T)
        st.starts_np[:] = 0
        st.counts_np[:] = 0
        st.formats_np[:] = 0
        if st.maps_np is not None:
            st.maps_np[:] = hip.RECTIFY_NONE
        if st.masks_np is not None:
            st.masks_np[:] = hip.MASK_NONE
        for s, w in enumerate(wins):
            if w is not None:
                for i, (start, count) in enumerate(w):
                    k = i * S + s
                    # (a stream that was never fed can only name empty windows: its format word is not read)
                    st.starts_np[k], st.counts_np[k], st.formats_np[k] = start % R, count, self._feeds[s].format or 0
                    if st.maps_np is not None:
                        st.maps_np[k] = self._map_of[s]
                    if st.masks_np is not None:  # (every one of a stream's T windows reads that stream's mask)
                        st.masks_np[k] = self._hot.mask_of[s]
        self._words.copy_(st.words, non_blocking=True)
        for s, g in enumerate(gts):
            if g is not None and on[s]:
                if torch.is_tensor(g):
                    self._gt[s].copy_(g, non_blocking=True)
                else:
                    np.copyto(st.gt_np[s], g)
                    self._gt[s].copy_(st.gt[s], non_blocking=True)
                self._gt_live[s] = True
            elif self._gt_live[s]:  # (idle, or no label this round: the row must not score)
                self._gt[s].fill_(self.ignore_index)
                self._gt_live[s] = False
        st.done.record()
        if self.use_graph:
            self._g.replay()
            out = self._outputs
        else:
            out = self._round()
        self.n_rounds += 1
        res = MultiSegmentationResult(*out, valid=on)
        return res.clone() if (self.use_graph and self.copy_outputs) else res
