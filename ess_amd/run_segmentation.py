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
"""
import torch

from . import hip
from .e2vid.image_reconstructor import ImageReconstructor
from .e2vid.run_reconstruction import GraphedWindowState, events_to_voxel_grid_device


class SegmentationResult:
    """labels uint8 [1, H, W]; colour uint8 [1, H, W, 3] or None (no palette); confidence fp32 [1, H, W] or None."""
    __slots__ = ('labels', 'colour', 'confidence')

    def __init__(self, labels, colour=None, confidence=None):
        self.labels, self.colour, self.confidence = labels, colour, confidence

    def clone(self):
        return SegmentationResult(*(None if t is None else t.clone() for t in (self.labels, self.colour, self.confidence)))


class StreamingSegmenter(GraphedWindowState):
    """One sequence, one window at a time.  update(voxel grid [1, num_bins, H, W] or [num_bins, H, W]) / update_from_events([N, 4]
    rows (t, x, y, polarity)) -> SegmentationResult at the sensor size height x width (or out_hw); reset() starts a new sequence.

    encoder: an E2VIDRecurrent; decoder: a SemSegE2VID.  palette: uint8 [K, 3] (Settings.semseg_color_map; numpy or torch) -> the
    result carries colours.  out_hw: resize from the sensor-size region by the nearest rule (validation's img_size_b semantics).
    copy (graph mode): update() returns clones of the replay's static output buffers, so results held across windows stay intact;
    copy=False hands out the buffers themselves (valid until the next update())."""

    def __init__(self, encoder, decoder, height, width, options, device=None, graph=False, copy=True, palette=None,
                 want_confidence=False, out_hw=None):
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

    @classmethod
    def from_checkpoints(cls, e2vid_path, ess_checkpoint_path, settings_or_kwargs, **kw):
        """Build both models from files: the E2VID checkpoint through loading_utils.load_model, the decoder from the 'back_end'
        entry of a CheckpointSaver file (Epoch_<n>.pt of this package's trainers or the reference's).  settings_or_kwargs: a
        Settings object (semseg_num_classes, skip_connect_task, skip_connect_task_type, img_size_b, semseg_color_map, optionally
        e2vid options) or a dict with num_classes, height, width and optionally skip_connect (True), skip_type ('concat'),
        options, palette; further keyword arguments go to the constructor."""
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
        kw.setdefault('palette', palette)
        return cls(encoder, decoder, height, width, options if options is not None else default_options(), **kw)

    def reset(self):
        self.rec.last_states_for_each_channel = {'grayscale': None}
        self.n_windows = 0  # (the captured graph stays valid: it reads the static state buffers, which the next first step rewrites)

    def update_from_events(self, events):
        return self.update(events_to_voxel_grid_device(events, self.num_bins, self.width, self.height, self.device))

    def _window(self, ev):
        """one window's device work -> ((labels, colour, confidence), new states)"""
        rec = self.rec
        with torch.no_grad():
            ev = rec.crop.pad(rec.event_preprocessor(ev))
            if not ev.is_contiguous():
                ev = ev.contiguous()
            # encoder-only step whose latents ARE consumed; final_lean: the lean state form where the configuration has one
            _, states, latent = rec._step(ev, False, False, final_lean=not hip.mixed())
            self.last_latent = latent
            out = self.decoder.predict(latent, out_hw=self.out_hw, window=self.window, palette=self.palette,
                                       want_confidence=self.want_confidence)
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
