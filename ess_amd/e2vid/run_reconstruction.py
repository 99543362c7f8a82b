"""
Streaming single-sequence E2VID inference with persistent recurrent state (reference: e2vid/run_reconstruction.py,
e2vid/utils/inference_utils.py:432-546 `events_to_voxel_grid[_pytorch]`).

The reference script reads event windows from a text file with pandas, builds one voxel grid per window (np.add.at on the host or
index_add_ on the device) and calls `ImageReconstructor.update_reconstruction` once per window, the recurrent state living in the
reconstructor between calls.  Here:

* `events_to_voxel_grid_device` builds the window's grid with the library's temporal voting kernel (integer pixels, linear
  weights over the two neighbouring time bins, signed polarities: `ess_voxel_grid_temporal`, separate_pol = False);
* `StreamingReconstructor` is the per-window driver.  Its `graph=True` mode records ONE window's work -- voxel-grid normalisation,
  the full recurrent UNet step, the carry of the new state into the static state buffers -- in a hipGraph and replays it per
  window (host time per window: one input copy + one graph launch).  Measured (tools/bench_stream.py, B = 1, 5 x 480 x 640,
  107 520 events per window, bf16): 0.66 ms per window eager, 0.69 ms replayed -- the ~45 launches of a B = 1 step are long enough
  (60 x 80 planes: 20 workgroups per image and layer on 256 CUs) that eager issue already keeps up, and the replay pays ~35 us for
  carrying 70 MB of state into its static buffers; the mode exists for hosts that are busy with event I/O.  Results are
  bit-identical to the eager path.

File readers (FixedSizeEventReader / FixedDurationEventReader: pandas) and the image writer / display of the reference script are
data handling, outside the hot path: `iter_windows_fixed_size` covers the in-memory case.
"""
import torch

from .. import copies, hip
from .image_reconstructor import ImageReconstructor, PostProcessor


def events_to_voxel_grid_device(events, num_bins, width, height, device):
    """events: [N, 4] rows (timestamp, x, y, polarity) as in the reference (numpy or torch, any float / int dtype) -> fp32
    [num_bins, height, width] on `device`.  Reference: inference_utils.py:432-546 (polarity 0 counts as -1, timestamps scaled to
    [0, num_bins - 1], weights (1 - dt) / dt on bins floor(t) / floor(t) + 1, out-of-range bins dropped)."""
    ev = torch.as_tensor(events)
    if ev.dim() != 2 or ev.shape[1] != 4 or ev.shape[0] == 0:
        raise hip.EssHipError('events must be a non-empty [N, 4] array of (t, x, y, polarity) rows')
    ev = ev.to(device)
    t = ev[:, 0].to(torch.float64).contiguous()
    x = ev[:, 1].to(torch.int32).contiguous()
    y = ev[:, 2].to(torch.int32).contiguous()
    p = ev[:, 3].to(torch.float32).contiguous()
    return hip.voxel_grid_temporal(x, y, t, p, [0, ev.shape[0]], num_bins, height, width, separate_pol=False)[0]


def iter_windows_fixed_size(events, num_events):
    """Non-overlapping windows of `num_events` rows of an in-memory [N, 4] event array (FixedSizeEventReader's packaging)."""
    n = events.shape[0]
    for i in range(0, n - num_events + 1, num_events):
        yield events[i:i + num_events]


_PARTS = ('h', 'c8', 'h16', 'f32c8', 'c')


class GraphedWindowState:
    """What the streaming drivers share (StreamingReconstructor here, StreamingSegmenter in ess_amd/run_segmentation.py): the
    recurrent state of `self.rec` (an ImageReconstructor) carried in STATIC buffers, and the capture of one window's work -- a
    warm-up run on a side stream whose effect on the carried state is undone, then the recording -- as a hipGraph on the current
    stream.  A subclass provides `_window(ev) -> (outputs, states)`: one window's device work on the static input `ev`."""

    _static = None
    _g = None

    def _state_tensors(self, states):
        """the device tensors of a state list that the next step reads, per level: h (the fp32 hidden state, None where a lean step
        left an unwritten placeholder), its BF16_C8 copy, its half copy ('mixed'), its channel-blocked fp32 form (lean ConvGRU),
        the cell c -- each None where absent; + (hilo of the half copy, the hidden state's shape)"""
        out = []
        for s in states:
            h, c = (s[0], s[1]) if isinstance(s, (tuple, list)) else (s, None)
            r = copies.of(h)
            h16, hilo = r.h16 or (None, False)
            out.append(({'h': None if r.unwritten else h, 'c8': r.c8, 'h16': h16, 'f32c8': r.f32c8, 'c': c}, hilo, tuple(h.shape)))
        return out

    @staticmethod
    def _attach(st):
        """(re-)tie a static level's copies to its hidden-state tensor: the record follows the tensor's version"""
        parts, hilo, _, sh = st
        found = {'c8': parts['c8'], 'h16': None if parts['h16'] is None else (parts['h16'], hilo), 'f32c8': parts['f32c8']}
        copies.attach(sh, **{k: v for k, v in found.items() if v is not None})

    def _adopt_state(self, states):
        """Copy a step's output state into the static buffers (allocated on first use) and make THEM the carried state."""
        new = self._state_tensors(states)
        if self._static is None:
            self._static = []
            for parts, hilo, shape in new:
                sp = {k: None if t is None else torch.empty_like(t) for k, t in parts.items()}
                sh = sp['h']
                if sh is None:  # (a lean state: the fp32 hidden tensor is a placeholder without memory, the copies are the state)
                    sh = copies.placeholder(shape, self.device)
                self._static.append((sp, hilo, shape, sh))
        carried = []
        for st, (parts, hilo, shape) in zip(self._static, new):
            sp, s_hilo, s_shape, sh = st
            if [t is None for t in sp.values()] != [t is None for t in parts.values()] or s_hilo != hilo or s_shape != shape:
                raise hip.EssHipError('streaming: a step left its recurrent state in another form than the static buffers were made for')
            for k in _PARTS:
                if sp[k] is not None:
                    sp[k].copy_(parts[k])
            self._attach(st)  # (after the copies: the attachments are tied to the tensor's version)
            carried.append(sh if sp['c'] is None else (sh, sp['c']))
        self.rec.last_states_for_each_channel['grayscale'] = carried

    def _capture(self, example):
        self._in = example.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        saved = [{k: None if t is None else t.clone() for k, t in st[0].items()} for st in self._static]
        with torch.cuda.stream(side):  # (one eager run of the generic step on a side stream before the capture, torch's recipe)
            _, st = self._window(self._in)
            self._adopt_state(st)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for st, sv in zip(self._static, saved):  # undo the warm-up step's effect on the carried state
            for k in _PARTS:
                if st[0][k] is not None:
                    st[0][k].copy_(sv[k])
            self._attach(st)  # (the restore bumped the tensors' versions)
        self._g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g):
            outputs, st = self._window(self._in)
            self._adopt_state(st)
        self._outputs = outputs


class StreamingReconstructor(GraphedWindowState):
    """One sequence, one window at a time; the recurrent state persists between calls (reference run_reconstruction.py:84-112).

    update(event_tensor [1, num_bins, H, W] or [num_bins, H, W]) -> (image [1, 1, H, W], latent dict) ; reset() drops the state.
    postprocess=True: update() -> (image, latent, frame uint8 [H, W]) -- the displayable frame of image_reconstructor.PostProcessor
    (unsharp mask, fixed or auto-HDR rescale, 8 bit; cropped to the sensor's size where the model runs on a padded one).  Its launches
    are part of the captured window in graph mode; the eager first window and the replays share the one auto-HDR history in device
    memory, which reset() empties."""

    def __init__(self, model, height, width, options, device=None, graph=False, copy=True, postprocess=False):
        """copy (graph mode): update() returns CLONES of the captured graph's static output buffers, like the eager path's fresh
        tensors -- a caller that keeps frames across windows (the reference script's writer / display queue) must not see them
        overwritten by the next replay.  copy=False hands out the static buffers themselves (70 KB - 1 MB less traffic per
        window; valid until the next update()).  It governs the post-processed frame as it governs the image."""
        self.copy_outputs = bool(copy)
        self.device = device if device is not None else torch.device('cuda:0')
        self.model = model.to(self.device).eval()
        self.rec = ImageReconstructor(self.model, height, width, model.num_bins, self.device, options)
        self.height, self.width, self.num_bins = height, width, model.num_bins
        self.use_graph = graph
        self._g = None
        self.n_windows = 0
        self.post = PostProcessor(self.device, options, n=1, crop=self.rec.crop) if postprocess else None

    def reset(self):
        self.rec.last_states_for_each_channel = {'grayscale': None}
        if self.post is not None:
            self.post.reset()
        self.n_windows = 0  # (the captured graph stays valid: it reads the static state buffers, which the next first step rewrites)

    def update_from_events(self, events):
        grid = events_to_voxel_grid_device(events, self.num_bins, self.width, self.height, self.device)
        return self.update(grid)

    def update(self, event_tensor):
        ev = event_tensor.to(self.device)
        if ev.dim() == 3:
            ev = ev.unsqueeze(0)
        if ev.shape != (1, self.num_bins, self.height, self.width):
            raise hip.EssHipError(f'expected a [1, {self.num_bins}, {self.height}, {self.width}] voxel grid, got {tuple(ev.shape)}')
        first = self.rec.last_states_for_each_channel['grayscale'] is None
        if not self.use_graph or first:
            # the first window of a sequence runs eagerly: no previous state (x-only gate convolutions), different launches
            outputs, states = self._window(ev)
            if self.use_graph:
                self._adopt_state(states)
            self.n_windows += 1
            return outputs
        if self._g is None:
            self._capture(ev)
        self._in.copy_(ev, non_blocking=True)
        self._g.replay()
        self.n_windows += 1
        if not self.copy_outputs:
            return self._outputs
        lat = self._out_latent
        if isinstance(lat, dict):
            lat = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in lat.items()}
        elif torch.is_tensor(lat):
            lat = lat.clone()
        return (self._out_img.clone(), lat) + tuple(t.clone() for t in self._outputs[2:])

    # ---- hipGraph mode: static input, static state buffers; one recorded window = step + state carry (GraphedWindowState)
    def _window(self, ev):
        img, states, latent = self.rec.update_reconstruction(ev)
        if self.post is None:
            return (img, latent), states
        return (img, latent, self.post.process_u8(img)[0]), states

    def _capture(self, example):
        """the warm-up window in front of the recording must not leave an entry in the auto-HDR history either"""
        saved = [t.clone() for t in self.post.state_tensors()] if self.post is not None else []
        super()._capture(example)
        for t, sv in zip(self.post.state_tensors() if saved else [], saved):
            t.copy_(sv)

    @property
    def _out_img(self):
        return self._outputs[0]

    @property
    def _out_latent(self):
        return self._outputs[1]
