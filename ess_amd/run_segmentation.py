"""
Streaming event segmentation: event windows -> semantic label maps, one window at a time, the recurrent state of the frozen E2VID
encoder kept between windows.

The reference has no such driver: its only way from events to labels is the trainers' validation step (training/ess_trainer.py:
424-493 -- a reset state per batch, logits resized with F.interpolate(nearest) to img_size_b, argmax, confusion matrix).  Those
lines define the semantics here; the loop is that of e2vid/run_reconstruction.py:84-112 (StreamingReconstructor).  Per window:

  voxel grid -> EventPreprocessor normalisation -> reflection padding where the size needs it (CropParameters)
  -> ONE ENCODER-ONLY recurrent step (head, three stride-2 convolutions + ConvLSTM / ConvGRU; no residual blocks, no E2VID
     decoders, no prediction layer, no image: 42 % of a full step's MACs are not run)
  -> SemSegE2VID.predict: the decoder up to decoder_scale_4, then the fused class head (hip.seg_head: 1x1 convolution + nearest
     resize + argmax in one pass; uint8 labels, optionally palette colours and the winner's softmax probability; no logits).

State forms: in the 'bf16' configuration the step runs the lean form ImageReconstructor.update_reconstruction_sequence uses for
the last step of a training sequence (hidden states as BF16_C8 copies + channel-blocked fp32 cells; latents bit-identical to the
full step's).  In 'fp32' / 'bf16x3' that form does not exist and the step writes fp32 states, as there.  In 'mixed' the lean last
step leaves the deepest hidden state as a [hi | lo] half pair that is meant for the decoder, not for the next time step (ConvGRU
refuses it, ConvLSTM would read 22 instead of 11 bits of it and drift from the window-by-window results of
ImageReconstructor.update_reconstruction), so a carried state keeps the plain encoder-only form there.

graph=True records one window (normalise, step, state carry into static buffers, predict) in a hipGraph on the current stream and
replays it; the first window of a sequence runs eagerly (no previous state: different launches).  Results are bit-identical to the
eager path.  The compute configuration (hip.set_compute) is read when a window runs; a captured graph keeps the one it was
recorded under.  File readers, image writers and displays are out of scope, as for the reconstruction driver.

MultiStreamSegmenter serves S independent event streams (a stereo pair, a vehicle rig, a replay farm) as ONE batch per round.  What
makes a stream's results independent of the batch it rides in: per-sample normalisation statistics (hip.event_normalize_samples,
bit-identical per sample to the single-stream kernel), and a recurrent state that lives in static [S, ...] buffers from
construction and is steered per stream by mode words in device memory (hip.state_carry_masked: HOLD / TAKE / ZERO).  A restart is a
ZEROED state, not an absent one -- the reference's ConvLSTM / ConvGRU create a zero state when prev_state is None
(e2vid/model/submodules.py:196-207, 255-262) -- so every window, the first included, runs the ordinary with-state launches and one
captured graph serves them all.  An idle stream rides along on a zero grid and its new state is discarded: it costs its share of
the batch's compute.  With compact=True a round runs only its A active streams, as a batch of the smallest prepared size (bucket)
>= A: an indexed gather (hip.state_carry_indexed) brings their states from the home [S, ...] buffers into work buffers, restarts and
padded slots arriving as zeros, the step runs at the bucket's batch size, and an indexed scatter takes the new states home.  The
plan of such a round is a function on host lists (compact_plan); a round with more active streams than the largest bucket rides
along as before.

MultiStreamSegmenter(reconstruct=True, postprocess=True, overlay=alpha) is the display of a rig: beside the labels a round returns,
per stream, the E2VID image (the FULL recurrent step in place of the encoder-only one, on the same encoder pass), the displayable
uint8 frame (PostProcessor.process_u8: unsharp mask, auto-HDR rescale) and the label overlay (hip.viz_overlay), inside the one
captured graph.  Every stream has its own auto-HDR history in device memory, and the round steers them by words in device memory as
it steers the state (display_words; hip.recon_post_bounds(mode=, rows=) / hip.recon_post_frame(mode=)): the history of an idle
stream does not move -- a zero grid's blank frame never enters its bounds --, the history of a stream whose restart is carried out in
this round is emptied first, and a compacted round names each slot's history by an index table.  Captures and warm_up() run with
every history on HOLD.  Out of scope: SequenceSegmenter (its rounds score labels, nobody looks at them), image writers and
displays, and the bilateral filter (ImageFilter refuses it, as for the single-stream driver).
"""
import collections

import numpy as np
import torch

from . import hip
from .e2vid.image_reconstructor import ImageReconstructor, PostProcessor
from .e2vid.run_reconstruction import _PARTS, GraphedWindowState, events_to_voxel_grid_device


class SegmentationResult:
    """labels uint8 [1, H, W]; colour uint8 [1, H, W, 3] or None (no palette); confidence fp32 [1, H, W] or None; with
    StreamingSegmenter(reconstruct=True): image fp32 [1, 1, Hs, Ws], the E2VID reconstruction as StreamingReconstructor returns it;
    (postprocess=True): frame uint8 [1, H, W], the displayable frame; (overlay=alpha): overlay uint8 [1, H, W, 3], the label colours
    over the frame -- each None where it was not asked for."""
    __slots__ = ('labels', 'colour', 'confidence', 'image', 'frame', 'overlay')

    def __init__(self, labels, colour=None, confidence=None, image=None, frame=None, overlay=None):
        self.labels, self.colour, self.confidence = labels, colour, confidence
        self.image, self.frame, self.overlay = image, frame, overlay

    def clone(self):
        return SegmentationResult(*(None if t is None else t.clone() for t in (self.labels, self.colour, self.confidence, self.image,
                                                                                self.frame, self.overlay)))


def _models_from_checkpoints(e2vid_path, ess_checkpoint_path, settings_or_kwargs):
    """-> (encoder, decoder, height, width, options, palette): see StreamingSegmenter.from_checkpoints"""
    from .e2vid.options.inference_options import default_options
    from .e2vid.utils.loading_utils import load_model
    from .models.style_networks import SemSegE2VID
    s = settings_or_kwargs
    if isinstance(s, dict):
        K, height, width = s['num_classes'], s['height'], s['width']
        skip, skip_type = s.get('skip_connect', True), s.get('skip_type', 'concat')
        options, palette = s.get('options'), s.get('palette')
    else:
        K, (height, width) = s.semseg_num_classes, s.img_size_b
        skip, skip_type = s.skip_connect_task, s.skip_connect_task_type
        options, palette = getattr(s, 'e2vid_options', None), getattr(s, 'semseg_color_map', None)
    encoder, _ = load_model(e2vid_path)
    decoder = SemSegE2VID(input_c=256, output_c=K, skip_connect=skip, skip_type=skip_type)
    ckpt = torch.load(ess_checkpoint_path, map_location='cpu', weights_only=False)  # (utils/saver.py: one entry per model name)
    if 'back_end' not in ckpt:
        raise hip.EssHipError(f"{ess_checkpoint_path} has no 'back_end' entry (CheckpointSaver layout)")
    decoder.load_state_dict(ckpt['back_end'])
    return encoder, decoder, height, width, options if options is not None else default_options(), palette


class StreamingSegmenter(GraphedWindowState):
    """One sequence, one window at a time.  update(voxel grid [1, num_bins, H, W] or [num_bins, H, W]) / update_from_events([N, 4]
    rows (t, x, y, polarity)) -> SegmentationResult at the sensor size height x width (or out_hw); reset() starts a new sequence.

    encoder: an E2VIDRecurrent; decoder: a SemSegE2VID.  palette: uint8 [K, 3] (Settings.semseg_color_map; numpy or torch) -> the
    result carries colours.  out_hw: resize from the sensor-size region by the nearest rule (validation's img_size_b semantics).
    copy (graph mode): update() returns clones of the replay's static output buffers, so results held across windows stay intact;
    copy=False hands out the buffers themselves (valid until the next update()).

    update_from_events builds the grid with hip.voxel_grid_temporal in front of the window (fp32 atomics: the last bits follow
    arrival order).  The order-independent event ingest inside the captured round (event_capacity=) is MultiStreamSegmenter's: this
    driver's first window runs eagerly outside the capture; MultiStreamSegmenter(n_streams=1, event_capacity=N) is the
    single-stream form, at +0.02 ms per window.

    The display (all off by default; the results then are what they were without these keywords):
    reconstruct=True   the window's recurrent step is the FULL one (need_image=True: residual blocks, E2VID decoders, prediction layer) in
                       place of the encoder-only one, on the same encoder pass; the result carries `image`.  Labels, colours and
                       confidence stay bit-identical to the plain segmenter's: the latents of the two steps are.
    postprocess=True   (needs reconstruct) `frame`: PostProcessor.process_u8 of the image, cropped to the sensor -- StreamingReconstructor(
                       postprocess=True)'s frame, bit for bit; part of the captured window; one auto-HDR history in device memory shared
                       by the eager first window and the replays, untouched by the capture's warm-up run, emptied by reset().
    overlay=alpha      (needs postprocess and a palette; labels at the frame's size) `overlay`: hip.viz_overlay(labels, frame, palette,
                       alpha), uint8 [1, H, W, 3]."""

    def __init__(self, encoder, decoder, height, width, options, device=None, graph=False, copy=True, palette=None,
                 want_confidence=False, out_hw=None, reconstruct=False, postprocess=False, overlay=None):
        if postprocess and not reconstruct:
            raise hip.EssHipError('StreamingSegmenter: postprocess=True needs reconstruct=True (the frame is made from the image)')
        if overlay is not None:
            if not postprocess or palette is None:
                raise hip.EssHipError('StreamingSegmenter: overlay= needs postprocess=True (the frame) and a palette (the colours)')
            if not 0.0 <= float(overlay) <= 1.0:
                raise hip.EssHipError(f'StreamingSegmenter: overlay={overlay} outside [0, 1]')
            if out_hw is not None and (int(out_hw[0]), int(out_hw[1])) != (height, width):
                raise hip.EssHipError(f'StreamingSegmenter: overlay= needs labels at the frame\'s size {(height, width)}, out_hw is '
                                      f'{tuple(out_hw)}')
        self.copy_outputs = bool(copy)
        self.device = device if device is not None else torch.device('cuda:0')
        self.model = encoder.to(self.device).eval()
        self.decoder = decoder.to(self.device).eval()
        self.rec = ImageReconstructor(self.model, height, width, encoder.num_bins, self.device, options)
        self.height, self.width, self.num_bins = height, width, encoder.num_bins
        crop = self.rec.crop
        # the region ImageReconstructor crops its image to: the sensor inside the padded plane
        self.window = (crop.iy0, crop.ix0, crop.iy1 - crop.iy0, crop.ix1 - crop.ix0)
        self.out_hw = None if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        self.palette = None if palette is None else torch.as_tensor(palette).to(self.device).contiguous()
        self.want_confidence = bool(want_confidence)
        self.use_graph = graph
        self.n_windows = 0
        self.last_latent = None  # (eager windows: the latents handed to decoder.predict, for inspection)
        self.reconstruct = bool(reconstruct)
        self.post = PostProcessor(self.device, options, n=1, crop=crop) if postprocess else None
        self.overlay_alpha = None if overlay is None else float(overlay)

    @classmethod
    def from_checkpoints(cls, e2vid_path, ess_checkpoint_path, settings_or_kwargs, **kw):
        """Build both models from files: the E2VID checkpoint through loading_utils.load_model, the decoder from the 'back_end'
        entry of a CheckpointSaver file (Epoch_<n>.pt of this package's trainers or the reference's).  settings_or_kwargs: a
        Settings object (semseg_num_classes, skip_connect_task, skip_connect_task_type, img_size_b, semseg_color_map, optionally
        e2vid options) or a dict with num_classes, height, width and optionally skip_connect (True), skip_type ('concat'),
        options, palette; further keyword arguments go to the constructor."""
        encoder, decoder, height, width, options, palette = _models_from_checkpoints(e2vid_path, ess_checkpoint_path, settings_or_kwargs)
        kw.setdefault('palette', palette)
        return cls(encoder, decoder, height, width, options, **kw)

    def reset(self):
        self.rec.last_states_for_each_channel = {'grayscale': None}
        if self.post is not None:
            self.post.reset()
        self.n_windows = 0  # (the captured graph stays valid: it reads the static state buffers, which the next first step rewrites)

    def update_from_events(self, events):
        return self.update(events_to_voxel_grid_device(events, self.num_bins, self.width, self.height, self.device))

    def _capture(self, example):
        """the warm-up window in front of the recording must not leave an entry in the auto-HDR history either"""
        saved = [t.clone() for t in self.post.state_tensors()] if self.post is not None else []
        super()._capture(example)
        for t, sv in zip(self.post.state_tensors() if saved else [], saved):
            t.copy_(sv)

    def _window(self, ev):
        """one window's device work -> ((labels, colour, confidence, image, frame, overlay), new states)"""
        rec = self.rec
        with torch.no_grad():
            ev = rec.crop.pad(rec.event_preprocessor(ev))
            if not ev.is_contiguous():
                ev = ev.contiguous()
            # encoder-only step whose latents ARE consumed; final_lean: the lean state form where the configuration has one
            # (reconstruct: the full step on the same encoder pass -- its image is the reconstruction, its latents are the same bits)
            img, states, latent = rec._step(ev, self.reconstruct, False, final_lean=not hip.mixed())
            self.last_latent = latent
            out = self.decoder.predict(latent, out_hw=self.out_hw, window=self.window, palette=self.palette,
                                       want_confidence=self.want_confidence)
            if self.reconstruct:
                frame = None if self.post is None else self.post.process_u8(img)
                over = None if self.overlay_alpha is None else hip.viz_overlay(out[0], frame, self.palette, self.overlay_alpha)
                out = tuple(out) + (img, frame, over)
        return out, states

    def update(self, event_tensor):
        ev = event_tensor.to(self.device)
        if ev.dim() == 3:
            ev = ev.unsqueeze(0)
        if ev.shape != (1, self.num_bins, self.height, self.width):
            raise hip.EssHipError(f'expected a [1, {self.num_bins}, {self.height}, {self.width}] voxel grid, got {tuple(ev.shape)}')
        first = self.rec.last_states_for_each_channel['grayscale'] is None
        if not self.use_graph or first:
            out, states = self._window(ev)
            if self.use_graph:
                self._adopt_state(states)
            self.n_windows += 1
            return SegmentationResult(*out)
        if self._g is None:
            self._capture(ev)
        self._in.copy_(ev, non_blocking=True)
        self._g.replay()
        self.n_windows += 1
        res = SegmentationResult(*self._outputs)
        return res.clone() if self.copy_outputs else res


# ---------------------------------------------------------------------------------------------- S streams in one batch
class MultiSegmentationResult:
    """labels uint8 [S, H, W]; colour uint8 [S, H, W, 3] or None (no palette); confidence fp32 [S, H, W] or None; valid: a host
    tuple of S bools -- stream s had a window this round.  With MultiStreamSegmenter(reconstruct=True): image fp32 [S, 1, Hs, Ws], each
    stream's E2VID reconstruction; (postprocess=True): frame uint8 [S, H, W], the displayable frames; (overlay=alpha): overlay uint8
    [S, H, W, 3], the label colours over the frames -- each None where it was not asked for.  The rows of the other (idle) streams
    are UNSPECIFIED, in every tensor."""
    __slots__ = ('labels', 'colour', 'confidence', 'valid', 'image', 'frame', 'overlay')

    def __init__(self, labels, colour=None, confidence=None, valid=(), image=None, frame=None, overlay=None):
        self.labels, self.colour, self.confidence, self.valid = labels, colour, confidence, tuple(bool(v) for v in valid)
        self.image, self.frame, self.overlay = image, frame, overlay

    def clone(self):
        c = [None if t is None else t.clone() for t in (self.labels, self.colour, self.confidence, self.image, self.frame, self.overlay)]
        return MultiSegmentationResult(*c[:3], valid=self.valid, image=c[3], frame=c[4], overlay=c[5])


def stream_modes(pending, active):
    """The per-stream mode words of one round, from host lists of bools -> (mode_pre, mode_post, pending after the round).
    mode_pre steers the state carry in FRONT of the step: CARRY_ZERO for a stream that restarts now (a pending restart meets an
    active window), CARRY_HOLD otherwise; mode_post steers the normalisation and the carry BEHIND it: CARRY_TAKE for an active stream
    (its new state is kept), CARRY_HOLD for an idle one (zero grid, new state discarded).  A pending restart of an idle stream stays
    pending."""
    if len(pending) != len(active):
        raise hip.EssHipError(f'stream_modes: {len(pending)} pending flags for {len(active)} streams')
    pre = [hip.CARRY_ZERO if (p and a) else hip.CARRY_HOLD for p, a in zip(pending, active)]
    post = [hip.CARRY_TAKE if a else hip.CARRY_HOLD for a in active]
    return pre, post, [bool(p and not a) for p, a in zip(pending, active)]


def compact_buckets(n_streams, buckets=None):
    """The batch sizes a compacting segmenter of n_streams prepares -> a tuple, ascending.  Default: the powers of two BELOW
    n_streams (8 -> (1, 2, 4); 5 -> (1, 2, 4); 3 -> (1, 2); 2 -> (1,); 1 -> ()); a round with more active streams than the largest
    bucket rides along at n_streams.  An explicit list must be ints, strictly increasing, each in [1, n_streams)."""
    if buckets is None:
        out, b = [], 1
        while b < n_streams:
            out.append(b)
            b *= 2
        return tuple(out)
    if isinstance(buckets, (str, bytes)) or not hasattr(buckets, '__iter__'):
        raise hip.EssHipError(f'compact_buckets={buckets!r}: a list of batch sizes is needed')
    out = list(buckets)
    for i, b in enumerate(out):
        if not isinstance(b, int) or isinstance(b, bool) or not 1 <= b < n_streams:
            raise hip.EssHipError(f'compact_buckets={out!r}: entry {b!r} is not an int in [1, n_streams={n_streams})')
        if i and b <= out[i - 1]:
            raise hip.EssHipError(f'compact_buckets={out!r}: the sizes must be strictly increasing')
    return tuple(out)


_compact_buckets = compact_buckets  # (MultiStreamSegmenter's argument of that name shadows the function)
CompactPlan = collections.namedtuple('CompactPlan', 'bucket rows gather_dst gather_src norm_mode scatter_dst scatter_src pending_after')
SCATTER_SKIP = -2  # a dst_index outside every destination: hip.state_carry_indexed skips the move (a padded slot)


def compact_plan(pending, active, buckets):
    """One compacted round, from host lists -> None or a CompactPlan.  A = the number of active streams, bucket = the smallest of
    `buckets` >= A; none: None (the round rides along on all streams).  rows: the active stream numbers, ascending; they take slots
    0..A-1 of the compact batch, the slots A..bucket-1 are padding.  gather_dst / gather_src steer the indexed carry home -> work in
    front of the step: slot <- its stream's state, CARRY_SRC_ZERO for a stream that restarts now (pending and active) and for a
    padded slot.  norm_mode: 1 for a slot with a window, 0 for a padded one (a zero grid).  scatter_dst / scatter_src steer the carry
    new state -> home behind it: stream <- its slot, SCATTER_SKIP for a padded slot.  pending_after: as stream_modes gives it."""
    if len(pending) != len(active):
        raise hip.EssHipError(f'compact_plan: {len(pending)} pending flags for {len(active)} streams')
    rows = [s for s, a in enumerate(active) if a]
    A = len(rows)
    b = next((b for b in buckets if b >= A), None)
    if b is None:
        return None
    pad = b - A
    return CompactPlan(bucket=b, rows=rows, gather_dst=list(range(b)),
                       gather_src=[hip.CARRY_SRC_ZERO if pending[s] else s for s in rows] + [hip.CARRY_SRC_ZERO] * pad,
                       norm_mode=[1] * A + [0] * pad, scatter_dst=rows + [SCATTER_SKIP] * pad, scatter_src=list(range(b)),
                       pending_after=[bool(p and not a) for p, a in zip(pending, active)])


def display_words(pending, active, plan=None):
    """The display words of one round, from host lists -> (words, rows): what steers the auto-HDR histories of the round's frames
    (PostProcessor.process_u8(mode=words, rows=rows)).  pending: the restart flags IN FRONT of the round.  A slot's word is CARRY_ZERO
    where its stream restarts now (pending and active: the history empties and takes this frame), CARRY_TAKE where it is active,
    CARRY_HOLD otherwise -- a pending restart of an idle stream stays pending, and its history stays as it is until then.
    plan None (a ride-along round): one word per stream, rows None (slot s holds stream s).  plan: a CompactPlan of the same
    lists: one word and one history row per SLOT -- the row is the stream's number; a padded slot gets CARRY_HOLD and the row
    SCATTER_SKIP, which lies outside every history."""
    if len(pending) != len(active):
        raise hip.EssHipError(f'display_words: {len(pending)} pending flags for {len(active)} streams')
    word = [hip.CARRY_HOLD if not a else (hip.CARRY_ZERO if p else hip.CARRY_TAKE) for p, a in zip(pending, active)]
    if plan is None:
        return word, None
    if plan.rows != [s for s, a in enumerate(active) if a]:
        raise hip.EssHipError(f'display_words: the plan serves streams {plan.rows}, active says {[s for s, a in enumerate(active) if a]}')
    pad = plan.bucket - len(plan.rows)
    return [word[s] for s in plan.rows] + [hip.CARRY_HOLD] * pad, list(plan.rows) + [SCATTER_SKIP] * pad


def check_active(active, n_streams):
    """active: None (every stream) or S truth values on the host -> list of S bools"""
    if active is None:
        return [True] * n_streams
    if torch.is_tensor(active):
        active = active.tolist()
    active = list(active)
    if len(active) != n_streams:
        raise hip.EssHipError(f'active has {len(active)} entries, the segmenter serves n_streams={n_streams}')
    return [bool(a) for a in active]


def check_stream_grids(shape, n_streams, num_bins, height, width):
    if tuple(shape) != (n_streams, num_bins, height, width):
        raise hip.EssHipError(f'expected [{n_streams}, {num_bins}, {height}, {width}] voxel grids (one per stream), got {tuple(shape)}')


def check_stream_events(events, n_streams):
    """events: S entries, each [N, 4] rows (t, x, y, polarity) or None / empty (idle) -> (list of [N, 4] tensors or None, active)"""
    if not isinstance(events, (list, tuple)) or len(events) != n_streams:
        n = len(events) if isinstance(events, (list, tuple)) else type(events).__name__
        raise hip.EssHipError(f'events must be a list with one entry per stream: got {n}, the segmenter serves n_streams={n_streams}')
    out = []
    for s, e in enumerate(events):
        if e is not None:
            e = torch.as_tensor(e)
            if e.dim() != 2 or e.shape[1] != 4:
                raise hip.EssHipError(f'events[{s}] must be [N, 4] rows (t, x, y, polarity) or None, got {tuple(e.shape)}')
            if e.shape[0] == 0:
                e = None
        out.append(e)
    return out, [e is not None for e in out]


def _event_capacity(n, height, width):
    """MultiStreamSegmenter's event_capacity argument, checked -> int"""
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= hip.INGEST_MAX_CAPACITY:
        raise hip.EssHipError(f'event_capacity={n!r}: events per stream and round, an int in [1, {hip.INGEST_MAX_CAPACITY}]')
    if height > 32767 or width > 32767:
        raise hip.EssHipError(f'event_capacity: the event records carry int16 coordinates, {height} x {width} does not fit (<= 32767)')
    return n


EVENT_LAYOUTS = ('records', 'columns', 'ring')


def _event_layout(layout, event_capacity):
    """MultiStreamSegmenter's event_layout argument, checked against event_capacity (the argument as given) -> the layout"""
    if layout not in EVENT_LAYOUTS:
        raise hip.EssHipError(f'event_layout={layout!r}: one of {EVENT_LAYOUTS}')
    if event_capacity is None and layout != 'records':
        raise hip.EssHipError(f'event_layout={layout!r} needs event_capacity: without it no ingest buffers exist')
    return layout


VOXEL_FLAVOURS = ('temporal', 'trilinear')


def _voxel_flavour(voxel, layout, event_capacity):
    """MultiStreamSegmenter's voxel argument, checked against event_layout and event_capacity (the arguments as given) -> the flavour"""
    if voxel not in VOXEL_FLAVOURS:
        raise hip.EssHipError(f'voxel={voxel!r}: one of {VOXEL_FLAVOURS}')
    if voxel == 'trilinear' and (event_capacity is None or layout == 'records'):
        raise hip.EssHipError(f"voxel='trilinear' is built from raw event columns inside the round: pass event_capacity=N and "
                              f"event_layout='columns' or 'ring' (got event_layout={layout!r}, event_capacity={event_capacity!r})")
    return voxel


def _event_representation(representation, voxel, rectify_maps, num_bins):
    """The segmenters' representation argument, checked against voxel, rectify_maps (hip.event_representation) and the planes
    C = encoder.num_bins the network reads -> the hip.EVENT_REP_* word"""
    rep = hip.event_representation(representation, voxel, rectify_maps)
    if rep == hip.EVENT_REP_SEPARATE and num_bins % 2:
        raise hip.EssHipError(f"representation='separate_pol' fills 2 * bins planes [positive bins; negative bins]: the encoder's "
                              f'num_bins={num_bins} must be even')
    if rep == hip.EVENT_REP_HISTOGRAM and num_bins != 2:
        raise hip.EssHipError(f"representation='histogram' fills 2 planes [negative counts, positive counts]: the encoder's "
                              f'num_bins={num_bins} must be 2')
    return rep


def _rectify_maps(rectify_maps, voxel, n_streams):
    """MultiStreamSegmenter's rectify_maps argument, checked -> (the distinct maps stacked, host fp32 [n_maps, map_h, map_w, 2], or
    None where no stream has one; per stream its map's number or hip.RECTIFY_NONE).  Entries that are the same object share a map."""
    none = [hip.RECTIFY_NONE] * n_streams
    if rectify_maps is None:
        return None, none
    if voxel != 'trilinear':
        raise hip.EssHipError(f"rectify_maps belongs to voxel='trilinear' (this segmenter: voxel={voxel!r}): the temporal grid takes the "
                              'integer pixels as they are')
    if not isinstance(rectify_maps, (list, tuple)) or len(rectify_maps) != n_streams:
        n = len(rectify_maps) if isinstance(rectify_maps, (list, tuple)) else type(rectify_maps).__name__
        raise hip.EssHipError(f'rectify_maps must be a list with one entry per stream (a map or None): got {n}, the segmenter serves '
                              f'n_streams={n_streams}')
    seen, maps, map_of = {}, [], []
    for s, m in enumerate(rectify_maps):
        if m is None:
            map_of.append(hip.RECTIFY_NONE)
            continue
        if id(m) not in seen:
            if not (torch.is_tensor(m) or isinstance(m, np.ndarray)):
                raise hip.EssHipError(f'rectify_maps[{s}] must be a float32 array or tensor [map_h, map_w, 2] or None, got {type(m).__name__}')
            v = torch.as_tensor(m)
            if v.dtype != torch.float32:
                raise hip.EssHipError(f'rectify_maps[{s}] must be float32 (the rectify map as the file holds it), got {v.dtype}')
            if v.dim() != 3 or v.shape[2] != 2 or v.numel() == 0 or max(v.shape[:2]) > hip.RECTIFY_MAX_SIDE:
                raise hip.EssHipError(f'rectify_maps[{s}] must be [map_h, map_w, 2] with sides in 1..{hip.RECTIFY_MAX_SIDE}: entry [y, x] = '
                                      f'the rectified (x, y); got {tuple(v.shape)}')
            if maps and v.shape != maps[0].shape:
                raise hip.EssHipError(f'rectify_maps[{s}] is {tuple(v.shape)}, the maps before it {tuple(maps[0].shape)}: one call reads '
                                      'maps of one sensor size')
            seen[id(m)] = len(maps)
            maps.append(v.detach().cpu())
        map_of.append(seen[id(m)])
    return (torch.stack(maps).contiguous() if maps else None), map_of


def _check_hot_pixel_masks(masks, n_streams, size):
    """The segmenters' hot_pixel_masks argument: n_streams entries, each None or a datasets.hot_pixels.HotPixelMask, all of one sensor
    size (size: (h, w) they must have, or None) -> that size, None where every entry is None"""
    from .datasets.hot_pixels import HotPixelMask
    if not isinstance(masks, (list, tuple)) or len(masks) != n_streams:
        n = len(masks) if isinstance(masks, (list, tuple)) else type(masks).__name__
        raise hip.EssHipError(f'hot_pixel_masks must be a list with one entry per stream (a HotPixelMask or None): got {n}, the segmenter '
                              f'serves n_streams={n_streams}')
    for s, m in enumerate(masks):
        if m is None:
            continue
        if not isinstance(m, HotPixelMask):
            raise hip.EssHipError(f'hot_pixel_masks[{s}] must be a datasets.hot_pixels.HotPixelMask or None, got {type(m).__name__}')
        if size is not None and (m.height, m.width) != tuple(size):
            raise hip.EssHipError(f'hot_pixel_masks[{s}] is {m.height} x {m.width}, the masks of this segmenter {size[0]} x {size[1]}: one '
                                  'call reads masks of one sensor size')
        size = (m.height, m.width)
    return size


class _HotPixelSlots:
    """The hot-pixel masks of a segmenter: ONE static device buffer words int32 [S, mask_h, ceil(mask_w / 32)] -- a slot per stream,
    so that set_hot_pixels and calibrate_hot_pixels never run out of room under a capture that has the buffer's address and size --
    and the host's books: which HotPixelMask each slot holds (entries that are the same object share a slot) and mask_of, per STREAM
    its slot or hip.MASK_NONE, which the staging writes into the round's words."""

    def __init__(self, masks, n_streams, default_size, device):
        self.size = _check_hot_pixel_masks(masks, n_streams, None) or (int(default_size[0]), int(default_size[1]))
        mh, mw = self.size
        self.n_streams, self.device = n_streams, device
        self.words = torch.zeros(n_streams, mh, hip.mask_words(mw), dtype=torch.int32, device=device)
        self.held = [None] * n_streams
        self.mask_of = [hip.MASK_NONE] * n_streams
        self.scratch = None  # (calibration: the histogram sums, made when first needed)
        for s, m in enumerate(masks):
            self.assign(s, m)

    def free_slot(self):
        """a slot no stream names (there is always one for a stream that has just let go of its own)"""
        return next(k for k in range(self.n_streams) if k not in self.mask_of)

    def assign(self, s, m):
        """stream s reads mask m (None: none) from its next round on; a mask no slot holds is uploaded, outside any capture"""
        self.mask_of[s] = hip.MASK_NONE
        if m is None:
            return
        _check_hot_pixel_masks([m], 1, self.size)
        for k, o in enumerate(self.held):
            if o is m:
                self.mask_of[s] = k
                return
        k = self.free_slot()
        self.words[k].copy_(torch.from_numpy(m.words.view(np.int32).copy()))
        self.held[k] = m
        self.mask_of[s] = k

    def own_slot(self, s, keep):
        """a slot that stream s alone names, for a calibration to write; keep: with the bits of the stream's mask so far"""
        k = self.mask_of[s]
        if k != hip.MASK_NONE and self.mask_of.count(k) == 1:
            self.held[k] = None
            return k
        self.mask_of[s] = hip.MASK_NONE
        j = self.free_slot()
        if keep and k != hip.MASK_NONE:
            self.words[j].copy_(self.words[k])
        elif keep:
            self.words[j].zero_()
        self.held[j] = None
        self.mask_of[s] = j
        return j


def check_stream_columns(events, n_streams):
    """events: S entries, each a datasets.data_util.EventColumns or None / empty (idle) -> (list of EventColumns or None, active)"""
    from .datasets.data_util import EventColumns
    if not isinstance(events, (list, tuple)) or len(events) != n_streams:
        n = len(events) if isinstance(events, (list, tuple)) else type(events).__name__
        raise hip.EssHipError(f'events must be a list with one entry per stream: got {n}, the segmenter serves n_streams={n_streams}')
    out = []
    for s, e in enumerate(events):
        if e is not None and not isinstance(e, EventColumns):
            raise hip.EssHipError(f"events[{s}] must be an EventColumns or None with event_layout='columns', got {type(e).__name__}: hand the "
                                  'columns over as they arrive, EventColumns(t, x, y, p); EventColumns.from_rows converts [N, 4] rows (the slow way)')
        out.append(e if e is not None and e.n else None)
    return out, [e is not None for e in out]


class _ColumnStage:
    """one pinned staging set of the column ingest: the four columns [S, stride] and the words [2, S] (counts, formats; voxel=
    'trilinear': [3, S], the map words behind them) as torch (pinned) and as numpy views, the event recorded behind the set's last
    upload, and the (slot, events) pairs staged for the next"""
    __slots__ = ('cols', 'words', 'cols_np', 'counts_np', 'formats_np', 'maps_np', 'masks_np', 'done', 'used')

    def __init__(self, cols, words, done):
        self.cols, self.words, self.done, self.used = cols, words, done, ()
        self.cols_np = tuple(c.numpy() for c in cols)
        self.counts_np, self.formats_np = words.numpy()[0], words.numpy()[1]
        self.maps_np = words.numpy()[2] if words.shape[0] > 2 else None
        self.masks_np = words.numpy()[3] if words.shape[0] > 3 else None  # (hot_pixel_masks: [4, S], the map words always there)


class _RingStage:
    """one pinned staging set of the ring ingest: the words [4, S] (rows, starts, counts, formats; voxel='trilinear': [5, S], the map
    words behind them) as torch (pinned) and as numpy views, and the event recorded behind the set's last upload.  No event is
    staged: they went to the device ring when they arrived"""
    __slots__ = ('words', 'rows_np', 'starts_np', 'counts_np', 'formats_np', 'maps_np', 'masks_np', 'done', 'used')

    def __init__(self, words, done):
        self.words, self.done, self.used = words, done, ()
        self.rows_np, self.starts_np, self.counts_np, self.formats_np = words.numpy()[:4]
        self.maps_np = words.numpy()[4] if words.shape[0] > 4 else None
        self.masks_np = words.numpy()[5] if words.shape[0] > 5 else None  # (hot_pixel_masks: [6, S], the map words always there)


class _Feed:
    """one stream's side of the continuous feed: its window cutter (absolute event indices; position in the ring = index mod R), the
    format word its dtypes give (None until the first packet), and the uploads out of the pinned mirror still to be waited for --
    (the absolute index the packet began at, the event recorded behind its copies), oldest first"""
    __slots__ = ('windows', 'format', 'dtypes', 'uploads')

    def __init__(self, windows):
        self.windows, self.format, self.dtypes, self.uploads = windows, None, None, collections.deque()


class _IngestStage:
    """one pinned staging set of the event ingest: records / counts (torch, pinned), their numpy views, the event recorded behind
    the set's last upload, and the (slot, rows) pairs staged for the next one"""
    __slots__ = ('records', 'counts', 'records_np', 'counts_np', 'done', 'used')

    def __init__(self, records, counts, records_np, counts_np, done):
        self.records, self.counts, self.records_np, self.counts_np, self.done, self.used = records, counts, records_np, counts_np, done, ()


class MultiStreamSegmenter(GraphedWindowState):
    """n_streams independent sequences, one ROUND (one window of every active stream) at a time, as one batch.
    update(grids [S, num_bins, H, W], active=None) / update_from_events(list of S [N, 4] arrays -- event_layout='columns': EventColumns -- or None) -> MultiSegmentationResult;
    reset(streams=None): these streams (default: all) start from a zero state at their next active window.

    Each stream's labels, colours and confidences are those it would get alone in a MultiStreamSegmenter(n_streams=1): normalisation
    statistics are per stream and the layers' arithmetic per sample.  Bit for bit that holds where no kernel choice follows the batch
    size.  Two do at large sizes (measured at 480 x 640, B = 8 against B = 1: some tens of labels of 307 200, confidences to 5e-4): the
    form of the encoder's 5x5 / stride-2 convolutions (pin it with submodules.set_s2d_mode('2')) and the slice count of the decoder's
    split InstanceNorm statistics (pin it with hip.tuning_set('norm_split_wgs', hip.NORM_SPLIT_BY_PLANE)).  Both switches are
    process-wide, so the driver leaves them to the deployment; with both pinned the S = 8 and S = 1 results are equal.  Idle streams (active[s] false, or None in update_from_events) ride along on a zero grid; their
    state is left as it was and their result rows are unspecified.  The state's form depends on the compute configuration, which
    is therefore fixed at construction: update() refuses another one.  graph=True: the round's device work is captured ONCE (n_captures
    stays 1) and every later round -- whatever its mix of advancing, idle and restarting streams -- is two small input copies and one
    replay.  Other arguments: see StreamingSegmenter.

    compact=True: a round with A active streams runs as a batch of the smallest bucket >= A (compact_buckets: a list of batch
    sizes, default the powers of two below n_streams) instead of n_streams; each stream still gets, bit for bit, what it gets
    without (the two switches above pinned: the batch size now changes from round to round).  The state stays at home in the
    [S, ...] buffers between rounds; a round gathers the active streams' states into work buffers [largest bucket, ...] (bucket b
    steps on their first b records), steps there and scatters the new states home: two carry launches, as before.  A round with more
    active streams than the largest bucket -- every round with all streams active -- is the ride-along round above, unchanged.
    graph=True: one capture per bucket and one for the ride-along round, each made when first needed or all at once by warm_up();
    n_captures <= len(buckets) + 1.  The index tables and the compact input are static device buffers the host writes in front of
    the round; results keep the shape [S, ...], the active rows copied to their streams' rows behind it.

    event_capacity=N (events per stream and round, <= 2^22; None: nothing below exists and every path is as without): the round
    itself starts with hip.event_ingest, inside the capture (n_captures is as before).  update_from_events packs each active
    stream's rows into pinned 16-byte records on the host (datasets.data_util.pack_event_records), copies their used prefixes and
    the per-stream count words to static device buffers and replays; a window of more than N events is refused before anything
    is written.  The ingest sums in 64-bit fixed point, so the grids -- and with them labels, colours and confidences -- are a pure
    function of the events: run to run, batched or alone, compacted or not.  update(grids) writes the count word INGEST_KEEP for
    every stream and copies the grids in as without.  Allocated once: device records [S, N, 16], counts [S], the int64 sums
    [S, num_bins, H, W], and two pinned staging sets used alternately (the host waits for a set's last upload before rewriting
    it); a compacted round stages its records in slot order into the first `bucket` records, padded slots with count 0.

    event_layout='columns' (with event_capacity; 'records', the default, is the path above): update_from_events takes, per stream,
    a datasets.data_util.EventColumns -- t float64 or int64, x / y int16 or uint16, p one byte, as a camera or a DSEC file delivers
    them -- or None, and the round starts with hip.event_ingest_columns.  The host does no arithmetic: staging is four copies per
    stream into pinned columns (13 bytes per event), then their used prefixes, the counts and the per-stream format words go to
    static device columns [S, stride].  The format is a device word like the count, so streams may change their dtypes from round
    to round under the one capture.  Labels, colours and confidences equal the record path's on the same events bit for bit.

    event_layout='ring' (with event_capacity=N; ring_capacity=R, default 2 N, rounded up to a multiple of 16; window_events=N_w or
    window_duration=D, window_stride= default the window): the continuous feed.  feed(stream, EventColumns) takes packets of any size
    as they arrive and appends them to the stream's ring of R events in device memory, through a pinned mirror, at once; the host
    cuts windows by event count or by duration, with an optional overlap, from the indices and times it holds
    (datasets.event_feed.EventWindows).  update_from_feed(active=None) runs one round on the oldest pending window of every stream
    that has one: its upload is the four words per slot -- row, start, count, format -- that hip.event_ingest_ring reads inside
    the capture; an event crosses to the device once however many overlapping windows read it.  pending(stream), drop_feed(streams);
    update_from_events raises.  Labels, colours and confidences equal the column path's on the same windows bit for bit.

    voxel='trilinear' (with event_layout='columns' or 'ring'; 'temporal', the default, is everything above, unchanged): the round
    starts with hip.event_ingest_columns_trilinear / hip.event_ingest_ring_trilinear and builds the grid a DSEC-trained decoder
    expects from the same raw columns -- each (x, y) through the stream's rectify map on the device, time normalised in fp32 as the
    DSEC loader does, eight trilinear corners per event (VoxelGrid.convert), summed in 64-bit fixed point like the temporal grid.
    rectify_maps: n_streams entries, None or a float32 [map_h, map_w, 2] array / tensor (entry [y, x] = the rectified (x, y); the
    sensor's size, which may exceed the grid's: a 480-row map over height=440 cuts DSEC's 40 bottom rows), all of one shape,
    uploaded once here; entries that are the SAME object share one device copy (a stereo rig: two maps; a farm replaying one
    camera: one).  A stream without a map takes its integer pixels as coordinates.  The stream's map number is a device word that
    travels with its count and format (the words grow by one row: [3, S] / [5, S]; still one upload a round), and a compacted round
    writes it per slot.  Not reproduced from the DSEC loader: VoxelGrid(normalize=True)'s own per-grid normalisation in front of the
    event preprocessor's -- the grid enters the round as the raw sums.

    representation='separate_pol' | 'histogram' (with event_layout='columns' or 'ring', voxel='temporal' and no rectify_maps; None,
    the default, is the signed grid of everything above): the round starts with hip.event_ingest_columns_rep /
    hip.event_ingest_ring_rep and fills the C = encoder.num_bins planes the network reads with the reference loaders' other two
    event representations -- 'separate_pol': C even, [C / 2 positive bins; C / 2 negative bins], both non-negative; 'histogram':
    C == 2, [negative counts, positive counts], the time column not read -- summed in 64-bit fixed point like the signed grid.  The
    static grids and int64 sums are sized by C as before: 5 bins kept apart are C = 10, twice the signed grid's memory.

    hot_pixel_masks=[...] (with event_layout='columns' or 'ring', any voxel / representation; None, the default, is everything
    above, unchanged): n_streams entries, None or a datasets.hot_pixels.HotPixelMask of the SENSOR's size (all of one size; with
    every entry None: the rectify maps' size, else height x width), and the round starts with hip.event_ingest_masked: a hot
    pixel's events are dropped as RAW events, before a rectify map moves them, where the event preprocessor's hot_pixels_file loop
    (kept as it is) zeroes grid pixels afterwards.  Hot pixels belong to a sensor: each stream has its own mask; entries that are
    the same object share one device copy.  The masks live in one static buffer of n_streams slots; a stream's mask word travels
    with its count and format (the words grow to [4, S] / [6, S], the map words always among them), and a compacted round writes
    it per slot.  set_hot_pixels(stream, mask | None) and calibrate_hot_pixels(...) change masks between rounds without a
    re-capture.  The window's time base still counts the hot events, as the reference's does.

    The display (all off by default: a round is then launch for launch what it was, and the mode words and bucket tables keep their
    shapes; orthogonal to everything above -- the keywords only add to the tail of the round), with StreamingSegmenter's rules and
    refusals:
    reconstruct=True   the round's recurrent step is the FULL one; the result carries `image` fp32 [S, 1, Hs, Ws].  Labels, colours
                       and confidences stay bit-identical to the plain driver's.
    postprocess=True   (needs reconstruct) `frame` uint8 [S, H, W]: PostProcessor.process_u8 of each stream's image, cropped to the
                       sensor, with ONE auto-HDR history per stream (a PostProcessor(n=S) of the driver's).  A history takes a frame only
                       in a round its stream is active in; reset(streams) stays a pending flag, and a stream's history empties in
                       the round its restart is carried out, not before.  A third row of mode words carries that (display_words); in
                       a compacted round the bucket table gains the display word and the history row of every slot.  Captures and
                       warm_up() move no history: every stream is on HOLD during them, nothing is saved or restored.
    overlay=alpha      (needs postprocess and a palette; labels at the frames' size) `overlay` uint8 [S, H, W, 3]: hip.viz_overlay.
    Rows of idle streams are unspecified in all three, as in the labels."""

    def __init__(self, encoder, decoder, height, width, options, n_streams, device=None, graph=False, copy=True, palette=None,
                 want_confidence=False, out_hw=None, compact=False, compact_buckets=None, event_capacity=None, event_layout='records',
                 ring_capacity=None, window_events=None, window_duration=None, window_stride=None, voxel='temporal', rectify_maps=None,
                 representation=None, hot_pixel_masks=None, reconstruct=False, postprocess=False, overlay=None):
        if not isinstance(n_streams, int) or isinstance(n_streams, bool) or n_streams < 1:
            raise hip.EssHipError(f'n_streams={n_streams!r}: a positive number of streams is needed')
        if postprocess and not reconstruct:  # (the display's refusals are StreamingSegmenter's, made before the models reach the device)
            raise hip.EssHipError('MultiStreamSegmenter: postprocess=True needs reconstruct=True (the frames are made from the images)')
        if overlay is not None:
            if not postprocess or palette is None:
                raise hip.EssHipError('MultiStreamSegmenter: overlay= needs postprocess=True (the frames) and a palette (the colours)')
            if not 0.0 <= float(overlay) <= 1.0:
                raise hip.EssHipError(f'MultiStreamSegmenter: overlay={overlay} outside [0, 1]')
            if out_hw is not None and (int(out_hw[0]), int(out_hw[1])) != (height, width):
                raise hip.EssHipError(f'MultiStreamSegmenter: overlay= needs labels at the frames\' size {(height, width)}, out_hw is '
                                      f'{tuple(out_hw)}')
        if hot_pixel_masks is not None:  # (refused before the models reach the device)
            if event_capacity is None or event_layout not in ('columns', 'ring'):
                raise hip.EssHipError(f"hot_pixel_masks are applied to raw events, where (x, y) is still the sensor's pixel: that needs the "
                                      f"raw event columns inside the round, event_capacity=N and event_layout='columns' or 'ring' (got "
                                      f'event_layout={event_layout!r}, event_capacity={event_capacity!r}; the record layout and grids handed '
                                      'to update() keep the hot_pixels_file loop of the event preprocessor)')
            _check_hot_pixel_masks(hot_pixel_masks, n_streams, None)
        self.representation = representation
        if representation is not None:  # (refused before the models reach the device)
            self._rep = _event_representation(representation, voxel, rectify_maps, encoder.num_bins)
            if event_capacity is None or event_layout not in ('columns', 'ring'):
                raise hip.EssHipError(f"representation={representation!r} is built from raw event columns inside the round: pass "
                                      f"event_capacity=N and event_layout='columns' or 'ring' (got event_layout={event_layout!r}, "
                                      f'event_capacity={event_capacity!r})')
        self.compact = bool(compact)
        self.buckets = _compact_buckets(n_streams, compact_buckets) if self.compact else ()
        self.n_streams = n_streams
        self.copy_outputs = bool(copy)
        self.device = device if device is not None else torch.device('cuda:0')
        self.model = encoder.to(self.device).eval()
        self.decoder = decoder.to(self.device).eval()
        self.rec = ImageReconstructor(self.model, height, width, encoder.num_bins, self.device, options)
        if self.rec.no_recurrent:
            raise hip.EssHipError('MultiStreamSegmenter: options.no_recurrent leaves no state to carry; use StreamingSegmenter')
        if self.rec.event_preprocessor.no_normalize:
            raise hip.EssHipError('MultiStreamSegmenter: options.no_normalize is not supported (the normalisation launch is what zero-fills idle streams)')
        self.height, self.width, self.num_bins = height, width, encoder.num_bins
        crop = self.rec.crop
        self.window = (crop.iy0, crop.ix0, crop.iy1 - crop.iy0, crop.ix1 - crop.ix0)
        self.out_hw = None if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        self.palette = None if palette is None else torch.as_tensor(palette).to(self.device).contiguous()
        self.want_confidence = bool(want_confidence)
        self.use_graph = graph
        self.n_windows = 0   # rounds
        self.n_captures = 0  # hipGraph captures (graph mode: 1 from the first round on)
        self.last_latent = None  # (eager rounds: the latents handed to decoder.predict, for inspection)
        self.compute = hip.compute_name()
        S = n_streams
        self._in = torch.zeros(S, self.num_bins, height, width, dtype=torch.float32, device=self.device)
        self.reconstruct = bool(reconstruct)
        self.post = PostProcessor(self.device, options, n=S, crop=crop) if postprocess else None  # (one history per STREAM)
        self.overlay_alpha = None if overlay is None else float(overlay)
        # [0]: in front of the step, [1]: behind it; postprocess: [2]: the display word of each stream's auto-HDR history
        self._modes = torch.zeros(3 if postprocess else 2, S, dtype=torch.int32, device=self.device)
        self._pending = [True] * S
        self.event_layout = _event_layout(event_layout, event_capacity)
        self.event_capacity = None if event_capacity is None else _event_capacity(event_capacity, height, width)
        self.voxel = _voxel_flavour(voxel, self.event_layout, event_capacity)
        maps, self._map_of = _rectify_maps(rectify_maps, self.voxel, n_streams)
        self._maps = None if maps is None else maps.to(self.device)  # (uploaded once, here)
        if hot_pixel_masks is not None:
            default = tuple(maps.shape[1:3]) if maps is not None else (height, width)
            self._hot = _HotPixelSlots(hot_pixel_masks, n_streams, default, self.device)
        if self.event_layout == 'ring':
            self._build_ingest_ring(ring_capacity, window_events, window_duration, window_stride)
        elif not (ring_capacity is None and window_events is None and window_duration is None and window_stride is None):
            raise hip.EssHipError("ring_capacity, window_events, window_duration and window_stride belong to event_layout='ring'")
        elif self.event_capacity is not None:
            self._build_ingest() if self.event_layout == 'records' else self._build_ingest_columns()
        self._build_state()
        if self.buckets:
            self._build_compact()

    # ---- event ingest (event_capacity=N): static record / count buffers the captured round reads, pinned staging in front of them
    event_capacity = ring_capacity = _records = _columns = _counts = _formats = _acc = _ring = _maps = _hot = None
    voxel = 'temporal'
    representation, _rep = None, hip.EVENT_REP_SIGNED

    def _build_ingest(self):
        """Device records [S, N, 16], counts [S] and the int64 sums of hip.event_ingest (zeroed here, once), and two pinned staging
        sets used alternately, each with the event that marks the end of its last upload.  A compacted round reads the first
        `bucket` records / counts of the same buffers (slot order) and the leading part of the sums."""
        S, N = self.n_streams, self.event_capacity
        self._records = torch.zeros(S, N, hip.EVENT_RECORD.itemsize, dtype=torch.uint8, device=self.device)
        self._counts = torch.full((S,), hip.INGEST_KEEP, dtype=torch.int32, device=self.device)
        self._acc = torch.zeros(S, self.num_bins, self.height, self.width, dtype=torch.int64, device=self.device)
        self._stage = []
        for _ in range(2):
            rec = torch.zeros(S, N, hip.EVENT_RECORD.itemsize, dtype=torch.uint8).pin_memory()
            cnt = torch.full((S,), hip.INGEST_KEEP, dtype=torch.int32).pin_memory()
            self._stage.append(_IngestStage(rec, cnt, rec.numpy().view(hip.EVENT_RECORD).reshape(S, N), cnt.numpy(), torch.cuda.Event()))
        self._stage_next = 0

    def _build_ingest_columns(self):
        """event_layout='columns': the four device columns [S, stride] (t as raw 8-byte words, x / y as raw 2-byte words, p as
        bytes; stride = the capacity rounded up so that every row starts 16-byte aligned), the words [2, S] -- counts and formats,
        one upload -- and the int64 sums of hip.event_ingest_columns, and two pinned staging sets of the same, used alternately
        under _next_stage's rule.  A compacted round reads the first `bucket` rows."""
        S, stride = self.n_streams, hip.event_column_stride(self.event_capacity)
        dtypes = (torch.int64, torch.int16, torch.int16, torch.uint8)
        self._columns = tuple(torch.zeros(S, stride, dtype=d, device=self.device) for d in dtypes)
        n_words = 3 if self.voxel == 'trilinear' else 2  # (the map words ride behind the counts and formats: still one upload)
        if self._hot is not None:
            n_words = 4  # (... and the mask words behind the map words, which are then always there: -1 is NONE for both)
        self._words = torch.zeros(n_words, S, dtype=torch.int32, device=self.device)
        self._counts, self._formats = self._words[0], self._words[1]
        self._counts.fill_(hip.INGEST_KEEP)
        self._words[2:].fill_(hip.RECTIFY_NONE)
        self._acc = torch.zeros(S, self.num_bins, self.height, self.width, dtype=torch.int64, device=self.device)
        self._stage = []
        for _ in range(2):
            words = torch.zeros(n_words, S, dtype=torch.int32).pin_memory()
            words[0].fill_(hip.INGEST_KEEP)
            words[2:].fill_(hip.RECTIFY_NONE)
            self._stage.append(_ColumnStage(tuple(torch.zeros(S, stride, dtype=d).pin_memory() for d in dtypes), words, torch.cuda.Event()))
        self._stage_next = 0

    def _build_ingest_ring(self, ring_capacity, window_events, window_duration, window_stride):
        """event_layout='ring': per stream a ring of R events in device memory -- the four raw columns [S, R] -- that feed() appends
        packets to, a pinned mirror of the same shape the packets pass through, the device words [4, S] (rows, starts, counts,
        formats: one upload a round) with two pinned staging sets under _next_stage's rule, the int64 sums of hip.event_ingest_ring,
        and per stream the window cutter.  R: ring_capacity (default 2 N), at least N, rounded up to a multiple of 16."""
        from .datasets.event_feed import EventWindows
        S, N = self.n_streams, self.event_capacity
        R = 2 * N if ring_capacity is None else ring_capacity
        if not isinstance(R, int) or isinstance(R, bool) or R < N or hip.event_column_stride(R) > hip.INGEST_MAX_CAPACITY:
            raise hip.EssHipError(f'ring_capacity={ring_capacity!r}: events per stream the ring holds, an int in [event_capacity={N}, '
                                  f'{hip.INGEST_MAX_CAPACITY}] (default: 2 * event_capacity)')
        self.ring_capacity = R = hip.event_column_stride(R)
        self._window_args = dict(window_events=window_events, window_duration=window_duration, stride=window_stride, event_capacity=N,
                                 ring_capacity=R)
        self._feeds = [_Feed(EventWindows(**self._window_args)) for _ in range(S)]  # (refuses a bad window argument here)
        dtypes = (torch.int64, torch.int16, torch.int16, torch.uint8)
        self._ring = tuple(torch.zeros(S, R, dtype=d, device=self.device) for d in dtypes)
        self._ring_host = tuple(torch.zeros(S, R, dtype=d).pin_memory() for d in dtypes)
        self._ring_np = tuple(c.numpy() for c in self._ring_host)
        n_words = 5 if self.voxel == 'trilinear' else 4  # (the map words ride behind the four: still one upload)
        if self._hot is not None:
            n_words = 6  # (... and the mask words behind the map words, which are then always there: -1 is NONE for both)
        self._words = torch.zeros(n_words, S, dtype=torch.int32, device=self.device)
        self._counts, self._formats = self._words[2], self._words[3]
        self._counts.fill_(hip.INGEST_KEEP)
        self._words[4:].fill_(hip.RECTIFY_NONE)
        self._acc = torch.zeros(S, self.num_bins, self.height, self.width, dtype=torch.int64, device=self.device)
        self._stage = []
        for _ in range(2):
            words = torch.zeros(n_words, S, dtype=torch.int32).pin_memory()
            words[2].fill_(hip.INGEST_KEEP)
            words[4:].fill_(hip.RECTIFY_NONE)
            self._stage.append(_RingStage(words, torch.cuda.Event()))
        self._stage_next = 0

    def _feed_of(self, stream, what):
        if self._ring is None:
            raise hip.EssHipError(f"{what} belongs to event_layout='ring' (this segmenter: {self.event_layout!r})")
        if not isinstance(stream, (int, np.integer)) or isinstance(stream, bool) or not 0 <= stream < self.n_streams:
            raise hip.EssHipError(f'{what}: stream {stream!r} of n_streams={self.n_streams}')
        return self._feeds[int(stream)]

    def feed(self, stream, cols):
        """A packet of a stream's events as it arrives (datasets.data_util.EventColumns, any size up to the ring's room; the times
        non-decreasing, also from packet to packet) -> the number of windows of that stream now pending.  The packet is copied as it
        is into the pinned mirror at head mod R -- at most two segments per column where it wraps -- and those segments go to the
        device ring on the current stream, non-blocking: each event crosses to the device once, when it arrives, however many
        overlapping windows read it.  Refused before anything is written: another object than an EventColumns, other dtypes than the
        stream's first packet had (drop_feed forgets them), a packet that goes back in time, a ring overrun (windows must be consumed
        by update_from_feed first) and a cut window of more than event_capacity events."""
        from .datasets.data_util import EventColumns
        from .datasets.event_feed import copy_into_ring
        f = self._feed_of(stream, 'feed')
        s = int(stream)
        if not isinstance(cols, EventColumns):
            raise hip.EssHipError(f'feed: an EventColumns is needed, got {type(cols).__name__}: hand the columns over as they arrive, '
                                  'EventColumns(t, x, y, p)')
        if cols.n == 0:
            return f.windows.pending
        dtypes = (cols.t.dtype, cols.x.dtype)
        if f.dtypes is not None and dtypes != f.dtypes:
            raise hip.EssHipError(f'feed: stream {s} delivers t {f.dtypes[0]} and x / y {f.dtypes[1]} since its first packet, this packet has '
                                  f'{dtypes[0]} and {dtypes[1]}: a ring holds one format (drop_feed([{s}]) starts afresh)')
        head, R = f.windows.head, self.ring_capacity
        f.windows.push(cols.n, cols.t)  # (refuses before anything changes)
        f.dtypes, f.format = dtypes, cols.format
        # the pinned entries about to be rewritten held the events [head - R, head + n - R): the uploads that read them must be over
        # (a whole ring lies between two uses of an entry, so in practice this never waits; finished uploads are forgotten on the way)
        while f.uploads and (f.uploads[0][0] < head + cols.n - R or f.uploads[0][1].query()):
            f.uploads.popleft()[1].synchronize()
        for at, _, m in copy_into_ring(cols, tuple(c[s] for c in self._ring_np), head, R):
            for dev, host in zip(self._ring, self._ring_host):
                dev[s, at:at + m].copy_(host[s, at:at + m], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        f.uploads.append((head, done))
        return f.windows.pending

    def pending(self, stream):
        """the number of complete windows of the stream that update_from_feed has not consumed yet"""
        return self._feed_of(stream, 'pending').windows.pending

    def drop_feed(self, streams=None):
        """these streams (default: all) forget their ring contents, their pending windows, the origin of their windows and their
        dtypes: the next packet is event 0 of a new sequence.  The recurrent state is reset()'s business, not this call's."""
        from .datasets.event_feed import EventWindows
        for s in (range(self.n_streams) if streams is None else streams):
            f = self._feed_of(s, 'drop_feed')
            for _, done in f.uploads:  # (the new sequence writes the mirror from entry 0 on)
                done.synchronize()
            self._feeds[int(s)] = _Feed(EventWindows(**self._window_args))

    def _stage_ring(self, slots):
        """slots: per slot (stream, or slot of a compact batch) None or (row, start, count, format) -> the staging set with the four
        words written; a slot without a window and the slots behind the list: count 0.  voxel='trilinear': the map word of the
        stream whose row the slot names, RECTIFY_NONE in every other slot"""
        st = self._next_stage()
        st.rows_np[:] = np.arange(self.n_streams)
        st.starts_np[:] = 0
        st.counts_np[:] = 0
        st.formats_np[:] = 0
        if st.maps_np is not None:
            st.maps_np[:] = hip.RECTIFY_NONE
        if st.masks_np is not None:
            st.masks_np[:] = hip.MASK_NONE
        for i, w in enumerate(slots):
            if w is not None:
                st.rows_np[i], st.starts_np[i], st.counts_np[i], st.formats_np[i] = w
                if st.maps_np is not None:
                    st.maps_np[i] = self._map_of[w[0]]
                if st.masks_np is not None:  # (a compacted round's slot carries the mask of the stream it holds)
                    st.masks_np[i] = self._hot.mask_of[w[0]]
        return st

    def update_from_feed(self, active=None):
        """One round from the fed events: every stream with a pending window -- and active[s] true, where active is given --
        consumes its OLDEST window; the others ride along idle.  A window without events (a duration window in a pause) is consumed
        and counts as idle: a pending restart stays pending, as with an empty window in update_from_events.  The round is one upload
        of the words [4, S] and the replay: a ride-along round names rows 0 .. S - 1, a compacted round writes the active streams'
        numbers into the rows in slot order and count 0 into a padded slot; no event moves."""
        if self._ring is None:
            raise hip.EssHipError(f"update_from_feed belongs to event_layout='ring' (this segmenter: {self.event_layout!r})")
        allowed = check_active(active, self.n_streams)
        self._check_compute()
        R = self.ring_capacity
        wins = []
        for f, a in zip(self._feeds, allowed):
            start, count = f.windows.pop() if a and f.windows.pending else (0, 0)
            wins.append((start % R, count, f.format) if count else None)
        on = [w is not None for w in wins]
        plan = compact_plan(self._pending, on, self.buckets) if self.buckets else None
        if plan is None:
            return self._ride_along(None, on, self._stage_ring([None if w is None else (s,) + w for s, w in enumerate(wins)]))
        return self._update_compact(plan, None, on, True, self._stage_ring([(s,) + wins[s] for s in plan.rows]))

    def _ingest(self, ev, b=None):
        """the round's first launches: the static event buffers (b: their first b slots) -> the grids ev, inside the capture"""
        cut = (lambda v: v) if b is None else (lambda v: v[:b])
        if self._ring is None and self._columns is None:
            hip.event_ingest(cut(self._records), cut(self._counts), ev, self._acc)
            return
        # the words: the source's own (rows, starts, counts, formats / counts, formats), the map words where there are any, the mask
        # words behind them.  Every row of the rings stays in reach (a slot names its row); the columns are cut like the words.
        kind, cols, k = ('ring', self._ring, 4) if self._ring is not None else ('columns', tuple(cut(c) for c in self._columns), 2)
        w = [cut(v) for v in self._words]
        tri = self.voxel == 'trilinear'
        hip.event_voxels(kind, cols, w[:k], ev, self._acc, representation=self._rep, trilinear=tri, maps=self._maps,
                         map_of=w[k] if tri else None, masks=None if self._hot is None else (self._hot.words, w[k + 1], self._hot.size))

    # ---- hot-pixel masks (hot_pixel_masks=[...]): per-sensor bit masks the ingest applies to the raw events
    def _hot_slots(self, what):
        if self._hot is None:
            raise hip.EssHipError(f'{what}: this segmenter was built without hot_pixel_masks, so no mask buffer exists under its captures: '
                                  'pass hot_pixel_masks=[...] (a list of None will do)')
        return self._hot

    def set_hot_pixels(self, stream, mask):
        """stream reads `mask` (a HotPixelMask of the segmenter's sensor size, or None: no mask) from its next round on.  The words
        go into the static mask buffer here, outside any capture; the stream's mask word travels with its next round's words: no
        re-capture, n_captures does not move."""
        hot = self._hot_slots('set_hot_pixels')
        if not isinstance(stream, (int, np.integer)) or isinstance(stream, bool) or not 0 <= stream < self.n_streams:
            raise hip.EssHipError(f'set_hot_pixels: stream {stream!r} of n_streams={self.n_streams}')
        hot.assign(int(stream), mask)

    def hot_pixels(self, stream):
        """the HotPixelMask the stream reads, or None"""
        hot = self._hot_slots('hot_pixels')
        k = hot.mask_of[int(stream)]
        return None if k == hip.MASK_NONE else hot.held[k]

    def calibrate_hot_pixels(self, streams=None, max_events_per_pixel=None, max_rate_hz=None, mode='replace'):
        """event_layout='ring': per named stream (default: all) a mask from the events its ring holds NOW -> the list of their
        HotPixelMask objects, in the order of `streams` (one download), which the streams read from their next round on.  A pixel
        is hot when it fired MORE than the limit: max_events_per_pixel=k events, or max_rate_hz=r: floor(r * (t_last - t_first))
        events, from the first and last time the ring holds, t taken in seconds -- exactly one of the two.  mode='replace': the
        stream's mask becomes the calibrated one; 'or': its bits are added to the mask the stream has.  On the device: the UNMASKED
        histogram scatter (hip.event_scatter_ring_rep) of the rings into scratch sums of the sensor's size, then
        hip.event_hot_pixel_mask into the stream's slot of the static buffer, then the scratch is zeroed.  Outside the captured
        round: recurrent state, pending windows and rings are not touched, nothing is captured again."""
        from .datasets.hot_pixels import HotPixelMask
        what = 'calibrate_hot_pixels'
        if self._ring is None:
            raise hip.EssHipError(f"{what} reads the streams' device rings: event_layout='ring' (this segmenter: {self.event_layout!r})")
        hot = self._hot_slots(what)
        if (max_events_per_pixel is None) == (max_rate_hz is None):
            raise hip.EssHipError(f'{what}: give max_events_per_pixel=k or max_rate_hz=r, exactly one of the two')
        limit = max_events_per_pixel if max_rate_hz is None else max_rate_hz
        ok = isinstance(limit, (int, np.integer)) if max_rate_hz is None else isinstance(limit, (int, float, np.integer, np.floating))
        if isinstance(limit, bool) or not ok or not 0 <= limit < float('inf'):
            raise hip.EssHipError(f'{what}: the limit {limit!r} must be a non-negative ' + ('int' if max_rate_hz is None else 'number'))
        if mode not in ('replace', 'or'):
            raise hip.EssHipError(f"{what}: mode={mode!r}: 'replace' or 'or'")
        streams = list(range(self.n_streams)) if streams is None else list(streams)
        for s in streams:
            self._feed_of(s, what)
        if len(set(int(s) for s in streams)) != len(streams):
            raise hip.EssHipError(f'{what}: streams={streams!r} names a stream twice')
        S, R = self.n_streams, self.ring_capacity
        mh, mw = hot.size
        words = np.zeros((4, S), dtype=np.int32)
        words[0] = np.arange(S)
        thresholds = np.full(S, -1, dtype=np.int64)
        slots = []
        for s in (int(s) for s in streams):
            f = self._feeds[s]
            head = f.windows.head
            n = min(head, R)
            k = hot.own_slot(s, keep=mode == 'or')
            slots.append(k)
            words[:, k] = (s, (head - n) % R, n, f.format or 0)
            if max_rate_hz is None:
                thresholds[k] = int(limit)
            else:
                t = self._ring_np[0][s].view(f.dtypes[0]) if n else np.zeros(1)
                span = float(t[(head - 1) % R]) - float(t[(head - n) % R]) if n else 0.0
                thresholds[k] = int(np.floor(float(limit) * span))
        if hot.scratch is None:
            hot.scratch = torch.zeros(S, 2, mh, mw, dtype=torch.int64, device=self.device)
        w = torch.from_numpy(words).to(self.device)
        hip.event_scatter_ring_rep(*self._ring, w[0], w[1], w[2], w[3], hot.scratch, hip.EVENT_REP_HISTOGRAM)
        hip.event_hot_pixel_mask(hot.scratch, torch.from_numpy(thresholds).to(self.device), hot.words,
                                 hip.MASK_OR if mode == 'or' else hip.MASK_REPLACE)
        hot.scratch.zero_()
        host = hot.words.cpu().numpy().view(np.uint32)
        out = []
        for k in slots:
            hot.held[k] = HotPixelMask.from_words(host[k], mh, mw)
            out.append(hot.held[k])
        return out

    def _next_stage(self):
        """the staging set of this round, free to be rewritten: its last upload has completed (in practice long ago -- a whole
        round lies between two uses of a set)"""
        st = self._stage[self._stage_next]
        self._stage_next ^= 1
        st.done.synchronize()
        return st

    def _stage_keep(self):
        """a round whose grids the caller provides: every count word INGEST_KEEP (None without event_capacity)"""
        if self.event_capacity is None:
            return None
        st = self._next_stage()
        st.counts_np[:] = hip.INGEST_KEEP
        st.used = ()
        return st

    def _stage_events(self, slots):
        """slots: per record slot (stream, or slot of a compact batch) an [N, 4] array or None -> the staging set with the rows
        packed and the counts written; slots behind the list: count 0.  Raises before anything is written when a window does not
        fit; nothing reaches the device here."""
        from .datasets.data_util import pack_event_records
        for i, e in enumerate(slots):
            if e is not None and e.shape[0] > self.event_capacity:
                raise hip.EssHipError(f'update_from_events: a window of {e.shape[0]} events (slot {i}) exceeds event_capacity={self.event_capacity}')
        st = self._next_stage()
        st.counts_np[:] = 0
        st.used = ()  # (a refused polarity below leaves a set without uploads)
        used = []
        for i, e in enumerate(slots):
            if e is not None:
                n = pack_event_records(e, st.records_np[i])
                st.counts_np[i] = n
                used.append((i, n))
        st.used = tuple(used)
        return st

    def _stage_columns(self, slots, streams=None):
        """_stage_events for event_layout='columns': slots hold EventColumns or None; per staged slot four copies into the pinned
        columns (datasets.data_util.stage_event_columns), its count and its format word -- voxel='trilinear': and the map word of the
        stream in the slot (streams[i]; None: stream i), RECTIFY_NONE in every other slot"""
        from .datasets.data_util import stage_event_columns
        for i, e in enumerate(slots):
            if e is not None and e.n > self.event_capacity:
                raise hip.EssHipError(f'update_from_events: a window of {e.n} events (slot {i}) exceeds event_capacity={self.event_capacity}')
        st = self._next_stage()
        st.counts_np[:] = 0
        st.formats_np[:] = 0
        if st.maps_np is not None:
            st.maps_np[:] = hip.RECTIFY_NONE
        if st.masks_np is not None:
            st.masks_np[:] = hip.MASK_NONE
        used = []
        for i, e in enumerate(slots):
            if e is not None:
                st.counts_np[i] = stage_event_columns(e, *(c[i] for c in st.cols_np))
                st.formats_np[i] = e.format
                if st.maps_np is not None:
                    st.maps_np[i] = self._map_of[i if streams is None else streams[i]]
                if st.masks_np is not None:
                    st.masks_np[i] = self._hot.mask_of[i if streams is None else streams[i]]
                used.append((i, e.n))
        st.used = tuple(used)
        return st

    def _upload(self, st):
        """the staged counts (and formats) and the used prefix of every staged slot -> the static device buffers, on the current
        stream"""
        if self._ring is not None:
            self._words.copy_(st.words, non_blocking=True)
        elif self._columns is not None:
            for i, n in st.used:
                for dev, host in zip(self._columns, st.cols):
                    dev[i, :n].copy_(host[i, :n], non_blocking=True)
            self._words.copy_(st.words, non_blocking=True)
        else:
            for i, n in st.used:
                self._records[i, :n].copy_(st.records[i, :n], non_blocking=True)
            self._counts.copy_(st.counts, non_blocking=True)
        st.done.record()

    @classmethod
    def from_checkpoints(cls, e2vid_path, ess_checkpoint_path, settings_or_kwargs, n_streams, **kw):
        """as StreamingSegmenter.from_checkpoints, plus the number of streams (compact, compact_buckets, reconstruct, postprocess,
        overlay, ...: keyword arguments, handed to the constructor)"""
        encoder, decoder, height, width, options, palette = _models_from_checkpoints(e2vid_path, ess_checkpoint_path, settings_or_kwargs)
        kw.setdefault('palette', palette)
        return cls(encoder, decoder, height, width, options, n_streams, **kw)

    # ---- state: static [S, ...] buffers from construction, never None
    def _step(self, ev, carried=None):
        """one encoder-only step of the whole batch from the carried state (carried: a compact batch's work state instead) --
        reconstruct: the FULL step on the same encoder pass, as StreamingSegmenter._window runs it -> (states, latent, image or
        None); the carried state stays the static buffers"""
        rec = self.rec
        if carried is not None:
            rec.last_states_for_each_channel['grayscale'] = carried
        img, states, latent = rec._step(ev, self.reconstruct, False, final_lean=not hip.mixed())
        rec.last_states_for_each_channel['grayscale'] = self._carried
        return states, latent, img

    def _display(self, out, img, mode, rows=None):
        """the tail of a round behind predict: (labels, colour, confidence) -> + (image, frame, overlay) where the display is on.
        mode / rows steer the auto-HDR histories: only the streams that advance in this round push their frame."""
        if not self.reconstruct:
            return out
        frame = None if self.post is None else self.post.process_u8(img, mode=mode, rows=rows)
        over = None if self.overlay_alpha is None else hip.viz_overlay(out[0], frame, self.palette, self.overlay_alpha)
        return tuple(out) + (img, frame, over)

    def _result(self, out, active):
        return MultiSegmentationResult(*out[:3], valid=active, **dict(zip(('image', 'frame', 'overlay'), out[3:])))

    def _build_state(self):
        """Learn the state's forms from the zero-input step (run once without and once WITH a state: the form must be a fixed point of
        the with-state step, which is the only one a round runs), make the static buffers the carried state, then ZERO everything."""
        rec = self.rec
        rec.last_states_for_each_channel = {'grayscale': None}
        self._carried = None
        with torch.no_grad():
            ev = rec.crop.pad(self._in)
            if not ev.is_contiguous():
                ev = ev.contiguous()
            states = self._step(ev)[0]
            self._adopt_state(states)  # (allocates the static buffers in the forms this step left)
            self._carried = rec.last_states_for_each_channel['grayscale']
            states = self._step(ev)[0]
            self._src_parts(states)  # (raises when the with-state step leaves another form)
        self._dst = [st[0][k] for st in self._static for k in _PARTS if st[0][k] is not None]
        self._pre = hip.StateCarryTable(self._dst)  # (no source: ZERO / HOLD)
        self._modes[0].fill_(hip.CARRY_ZERO)
        self._pre.run(self._modes[0])
        self._modes.zero_()

    def _src_parts(self, states, static=None):
        """the tensors of a step's output state, in the order of the static buffers (self._dst; static: a bucket's work state
        instead) -- refused when the forms differ"""
        src = []
        for st, (parts, hilo, shape) in zip(self._static if static is None else static, self._state_tensors(states)):
            sp, s_hilo, s_shape, _ = st
            if [t is None for t in sp.values()] != [t is None for t in parts.values()] or s_hilo != hilo or s_shape != shape:
                raise hip.EssHipError('streaming: a step left its recurrent state in another form than the static buffers were made for')
            src += [parts[k] for k in _PARTS if sp[k] is not None]
        return src

    # ---- compaction: work buffers [largest bucket, ...] of the home state's per-stream forms; bucket b steps on their first b records
    def _build_compact(self):
        """The work buffers, and per bucket: the carried state as leading-slice views of them (a leading slice of a stream-major
        tensor is contiguous; copies.attach ties the copies to the view, and a lean state's placeholder is made per bucket, so ONE
        set of buffers serves every bucket), the gather table, the index tables and the slice of the compact input.  Each
        bucket's forms are checked as _build_state checks the home state's: the with-state step at batch b must leave them."""
        from . import copies
        bmax, S = self.buckets[-1], self.n_streams
        work = [{k: None if t is None else torch.zeros((bmax,) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
                 for k, t in st[0].items()} for st in self._static]
        self.compact_input = torch.zeros(bmax, self.num_bins, self.height, self.width, dtype=torch.float32, device=self.device)
        self._bucket = {}
        self._cg = {}  # bucket -> (graph, outputs)
        for b in self.buckets:
            static = []
            for wp, (sp, hilo, shape, _) in zip(work, self._static):
                parts = {k: None if t is None else t[:b] for k, t in wp.items()}
                shape_b = (b,) + tuple(shape[1:])
                sh = parts['h'] if parts['h'] is not None else copies.placeholder(shape_b, self.device)
                st = (parts, hilo, shape_b, sh)
                self._attach(st)
                static.append(st)
            carried = [st[3] if st[0]['c'] is None else (st[3], st[0]['c']) for st in static]
            wdst = [st[0][k] for st in static for k in _PARTS if st[0][k] is not None]
            # rows: gather_dst, gather_src, norm_mode, scatter_dst, scatter_src; postprocess: + the display word and history row
            tab = torch.zeros(5 if self.post is None else 7, b, dtype=torch.int32, device=self.device)
            self._bucket[b] = (static, carried, hip.StateMoveTable(wdst, self._dst), tab)
            self._idle_tables(b)
            with torch.no_grad():
                ev = self.rec.crop.pad(self.compact_input[:b])
                if not ev.is_contiguous():
                    ev = ev.contiguous()
                states = self._step(ev, carried)[0]
                self._src_parts(states, static)  # (raises when the step at batch b leaves another form)

    def _idle_tables(self, b):
        """bucket b's tables for a round that touches nothing at home: every slot padded"""
        idle = [False] * self.n_streams
        plan = compact_plan(idle, idle, (b,))
        self._write_tables(plan, display_words(idle, idle, plan))  # (no history moves either: every slot on HOLD)

    def _write_tables(self, plan, display):
        rows = [plan.gather_dst, plan.gather_src, plan.norm_mode, plan.scatter_dst, plan.scatter_src]
        if self.post is not None:
            rows += list(display)
        self._bucket[plan.bucket][3].copy_(torch.tensor(rows, dtype=torch.int32), non_blocking=True)

    def _round_compact(self, b):
        """the device work of one compacted round at batch b on the static compact input and bucket b's index tables
        -> (labels, colour, confidence) of the b slots (+ image, frame, overlay: _display)"""
        rec, pre = self.rec, self.rec.event_preprocessor
        static, carried, gather, tab = self._bucket[b]
        with torch.no_grad():
            gather.run(tab[0], tab[1])  # slot <- its stream's state; restarting streams and padded slots: 0
            ev = self.compact_input[:b]
            if self.event_capacity is not None:  # (count words INGEST_KEEP: the grids the caller copied in stay)
                self._ingest(ev, b)
            for x, y in pre.hot_pixel_locations:
                ev[:, :, y, x] = 0
            if pre.flip:
                ev = torch.flip(ev, dims=[2, 3]).contiguous()
            ev = rec.crop.pad(hip.event_normalize_samples(ev, tab[2]))  # (padded slots: a zero grid)
            if not ev.is_contiguous():
                ev = ev.contiguous()
            states, latent, img = self._step(ev, carried)
            src = self._src_parts(states, static)
            self.last_latent = latent
            out = self.decoder.predict(latent, out_hw=self.out_hw, window=self.window, palette=self.palette,
                                       want_confidence=self.want_confidence)
            out = self._display(out, img, *((tab[5], tab[6]) if self.post is not None else (None,)))
            hip.StateMoveTable(self._dst, src).run(tab[3], tab[4])  # stream <- its slot's new state; padded slots skipped
        return out

    def _capture_compact(self, b):
        """as _capture: the warm-up run leaves the home state untouched because every slot is padded during it"""
        self._idle_tables(b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._round_compact(b)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outputs = self._round_compact(b)
        self._cg[b] = (g, outputs)
        self.last_latent = None
        self.n_captures += 1

    def warm_up(self):
        """Capture every graph now (the ride-along round's and one per bucket), so that no round in service pays a capture; eager
        mode: run each bucket once.  The home state and the pending restarts are as they were: the runs have every stream on HOLD
        / every slot padded."""
        self._check_compute()
        if self.use_graph and self._g is None:
            self._capture()
        for b in self.buckets:
            if not self.use_graph:
                self._idle_tables(b)
                self._round_compact(b)
            elif b not in self._cg:
                self._capture_compact(b)
        self.last_latent = None

    def _update_compact(self, plan, grids, active, compacted, stage=None):
        """one compacted round; grids: [S, ...] (compacted false: the active rows are placed into the compact input here), the
        compact grids [bucket, ...] themselves, or None: the round's ingest builds them from the staged records.  stage: the
        ingest's staging set of this round (event_capacity)"""
        b, A = plan.bucket, len(plan.rows)
        display = display_words(self._pending, active, plan)  # (from the restart flags in FRONT of the round)
        self._pending = plan.pending_after
        if self.use_graph and b not in self._cg:
            self._capture_compact(b)
        self._write_tables(plan, display)
        if stage is not None:
            self._upload(stage)
        if grids is None:
            pass  # (the ingest in front of the round builds compact_input[:b])
        elif compacted:
            self.compact_input[:b].copy_(grids, non_blocking=True)
        elif A:
            self.compact_input[:A].copy_(grids[plan.rows], non_blocking=True)
        if self.use_graph:
            self._cg[b][0].replay()
            out = self._cg[b][1]
        else:
            out = self._round_compact(b)
        self.n_windows += 1
        # the A result rows to their streams' rows of an [S, ...] result; the idle rows stay unspecified
        fresh = self.copy_outputs or not self.use_graph
        if fresh or self._cres is None:
            res = tuple(None if t is None else torch.empty((self.n_streams,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in out)
            if not fresh:
                self._cres = res
        else:
            res = self._cres
        if A:
            rows = torch.tensor(plan.rows, dtype=torch.int64).to(self.device, non_blocking=True)
            for r, t in zip(res, out):
                if t is not None:
                    r.index_copy_(0, rows, t[:A])
        return self._result(res, active)

    _cres = None

    def reset(self, streams=None):
        for s in (range(self.n_streams) if streams is None else streams):
            if not 0 <= int(s) < self.n_streams:
                raise hip.EssHipError(f'reset: stream {s} of n_streams={self.n_streams}')
            self._pending[int(s)] = True

    # ---- one round
    def _round(self):
        """the device work of one round on the static input and mode buffers -> (labels, colour, confidence) (+ image, frame,
        overlay: _display)"""
        rec, pre = self.rec, self.rec.event_preprocessor
        with torch.no_grad():
            self._pre.run(self._modes[0])  # restarting streams: state = 0
            ev = self._in
            if self.event_capacity is not None:  # (count words INGEST_KEEP: the grids the caller copied in stay)
                self._ingest(ev)
            for x, y in pre.hot_pixel_locations:
                ev[:, :, y, x] = 0
            if pre.flip:
                ev = torch.flip(ev, dims=[2, 3]).contiguous()
            ev = rec.crop.pad(hip.event_normalize_samples(ev, self._modes[1]))  # (idle streams: a zero grid)
            if not ev.is_contiguous():
                ev = ev.contiguous()
            states, latent, img = self._step(ev)
            src = self._src_parts(states)  # (taken in front of predict, which may attach further copies to the latents)
            self.last_latent = latent
            out = self.decoder.predict(latent, out_hw=self.out_hw, window=self.window, palette=self.palette,
                                       want_confidence=self.want_confidence)
            out = self._display(out, img, self._modes[2] if self.post is not None else None)
            hip.StateCarryTable(self._dst, src).run(self._modes[1])  # active streams: state = new state
        return out

    def _capture(self):
        """GraphedWindowState's recipe -- one eager run on a side stream, then the recording on the current stream -- with the
        warm-up run's effect on the state avoided instead of undone: every stream is on HOLD during it (the display word too: no
        auto-HDR history moves)."""
        self._modes.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._round()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g):
            self._outputs = self._round()
        self.last_latent = None
        self.n_captures += 1

    def _check_compute(self):
        if hip.compute_name() != self.compute:
            raise hip.EssHipError(f"MultiStreamSegmenter: built in the '{self.compute}' configuration (its state buffers have that form), "
                                  f"called in '{hip.compute_name()}'")

    def update(self, grids, active=None):
        if not torch.is_tensor(grids):
            raise hip.EssHipError(f'grids must be a tensor [{self.n_streams}, {self.num_bins}, {self.height}, {self.width}], got {type(grids).__name__}')
        check_stream_grids(grids.shape, self.n_streams, self.num_bins, self.height, self.width)
        active = check_active(active, self.n_streams)
        self._check_compute()
        plan = compact_plan(self._pending, active, self.buckets) if self.buckets else None
        if plan is not None:
            return self._update_compact(plan, grids, active, False, self._stage_keep())
        return self._ride_along(grids, active, self._stage_keep())

    def _ride_along(self, grids, active, stage=None):
        """one round at the full batch; grids None: the round's ingest builds them from the staged records.  stage: the ingest's
        staging set of this round (event_capacity)"""
        words = [display_words(self._pending, active)[0]] if self.post is not None else []
        pre, post, self._pending = stream_modes(self._pending, active)
        if self.use_graph and self._g is None:
            self._capture()
        self._modes.copy_(torch.tensor([pre, post] + words, dtype=torch.int32), non_blocking=True)
        if stage is not None:
            self._upload(stage)
        if grids is not None:
            self._in.copy_(grids, non_blocking=True)
        if self.use_graph:
            self._g.replay()
            out = self._outputs
        else:
            out = self._round()
        self.n_windows += 1
        res = self._result(out, active)
        return res.clone() if (self.use_graph and self.copy_outputs) else res

    def update_from_events(self, events):
        """events: S entries, [N, 4] rows (t, x, y, polarity) of the stream's window or None (idle).  All grids are built by ONE
        hip.voxel_grid_temporal call over the concatenated events; an idle stream is an empty slice (an all-zero grid).  A compacted
        round builds only its bucket's grids: the active streams' in slot order, a padded slot an empty slice."""
        if self._ring is not None:
            raise hip.EssHipError("update_from_events: event_layout='ring' cuts its windows itself: hand the packets to feed(stream, cols) "
                                  'as they arrive and run the rounds with update_from_feed()')
        if self.event_capacity is not None:
            return self._update_from_events_ingest(events)
        evs, active = check_stream_events(events, self.n_streams)
        if not any(active):
            return self.update(self._in, active)  # (nothing is read of an idle stream's grid)
        plan = compact_plan(self._pending, active, self.buckets) if self.buckets else None
        if plan is not None:
            self._check_compute()
        slots = evs if plan is None else [evs[s] for s in plan.rows] + [None] * (plan.bucket - len(plan.rows))
        offsets = [0]
        for e in slots:
            offsets.append(offsets[-1] + (0 if e is None else e.shape[0]))
        ev = torch.cat([e.to(torch.float64) for e in evs if e is not None]).to(self.device)
        t = ev[:, 0].contiguous()
        x = ev[:, 1].to(torch.int32).contiguous()
        y = ev[:, 2].to(torch.int32).contiguous()
        p = ev[:, 3].to(torch.float32).contiguous()
        grids = hip.voxel_grid_temporal(x, y, t, p, offsets, self.num_bins, self.height, self.width, separate_pol=False)
        if plan is None:
            return self.update(grids, active)
        return self._update_compact(plan, grids, active, True)

    def _update_from_events_ingest(self, events):
        """event_capacity=N: each active stream's rows are packed on the host into pinned 16-byte records (event_layout='columns':
        its EventColumns are copied into pinned columns as they are; a compacted round: in slot order), their used prefixes and the
        count (and format) words are copied to the static device buffers, and the round's own first launches (hip.event_ingest or
        hip.event_ingest_columns, inside the capture) build the grids: idle streams and padded slots have count 0, an all-zero grid.  The
        labels are a pure function of the events: the ingest's sums do not depend on arrival order."""
        if self._columns is not None:
            evs, active = check_stream_columns(events, self.n_streams)
        else:
            evs, active = check_stream_events(events, self.n_streams)
            evs = [None if e is None else e.detach().cpu().numpy() for e in evs]
        self._check_compute()
        plan = compact_plan(self._pending, active, self.buckets) if self.buckets else None
        rows = None if plan is None else plan.rows  # (the stream in every slot; None: slot s holds stream s)
        slots = evs if plan is None else [evs[s] for s in rows]
        stage = self._stage_columns(slots, rows) if self._columns is not None else self._stage_events(slots)
        if plan is None:
            return self._ride_along(None, active, stage)
        return self._update_compact(plan, None, active, True, stage)
