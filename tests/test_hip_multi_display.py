"""GPU tier of the multi-stream display: the steered auto-HDR and frame kernels (hip.recon_post_bounds(mode=, rows=),
hip.recon_post_frame(mode=)) against the host restatements (tests/multi_display_ref.py, tests/recon_post_ref.py), and
MultiStreamSegmenter(reconstruct=True, postprocess=True, overlay=alpha): per stream and active window the labels of the plain driver,
the frame a per-stream PostProcessor(n=1) makes of the round's own image, the overlay of tests/viz_ref.py -- eager, replayed,
compacted, from event columns; a stream against its batch and against the single-stream driver.  Every comparison is on BITS."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402
from tests import multi_display_ref as D  # noqa: E402
from tests import recon_post_ref as R  # noqa: E402
from tests import test_hip_multi_stream as M  # noqa: E402  (builders: _models, _events, the pins)
from tests import test_hip_seg_head as SH  # noqa: E402  (palette)
from tests import viz_ref as V  # noqa: E402

DEV = torch.device('cuda:0')
ALPHA = 0.6
W5 = R.gkern(5, 1.0)
WL = W5.reshape(-1).tolist()


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------- 1. the steered bounds kernel
class _Buffers:
    def __init__(self, n_slots, n_rows, size):
        from ess_amd import hip
        self.ring = torch.zeros(n_rows, size + 1, 2, dtype=torch.float64, device=DEV)
        self.state = torch.zeros(n_rows, 2, dtype=torch.int32, device=DEV)
        self.ws = torch.empty(n_slots, hip.RECON_POST_PARTIALS, 2, device=DEV)
        self.bounds = torch.empty(n_slots, 2, device=DEV)
        self.size = size

    def poison(self):
        self.ws.view(torch.uint8).fill_(0xFF)
        self.bounds.view(torch.uint8).fill_(0xFF)

    def call(self, img, amount, mode=None, rows=None):
        from ess_amd import hip
        kw = {} if mode is None else dict(mode=_i32(mode), rows=rows)
        hip.recon_post_bounds(torch.from_numpy(img).to(DEV), WL, amount, self.ws, self.ring, self.state, self.size, self.bounds, **kw)


def _check_call(buf, ref, img, amount, mode, rows, what):
    """one steered call into poisoned bounds / workspace against the restatement: taken slots' bounds bits, untouched 0xFF bytes of
    every other slot, a fully rewritten workspace of the taken slots, the history counts per ROW"""
    buf.poison()
    buf.call(img, amount, mode, rows)
    want, taken = ref.update(img, W5, amount, mode, None if rows is None else [int(r) for r in rows])
    got, ws = buf.bounds.cpu().numpy(), buf.ws.cpu().numpy()
    for n in range(len(mode)):
        if taken[n]:
            assert (_bits(got[n]) == _bits(want[n])).all(), (what, n, got[n], want[n])
            assert not np.isnan(ws[n]).any(), (what, n, 'workspace of a taken slot not fully rewritten')
        else:
            assert (got[n].view(np.uint8) == 0xFF).all() and (ws[n].view(np.uint8) == 0xFF).all(), (what, n, 'a skipped slot was written')
    assert buf.state[:, 1].tolist() == ref.counts(), (what, buf.state.tolist(), ref.counts())


@pytest.mark.parametrize('size', R.HDR_FILTER_SIZES)
@pytest.mark.parametrize('name', ['ride_along', 'compact'])
def test_steered_bounds_equal_the_restatement_after_every_call(name, size):
    """the two schedules of the CPU tier (which proves they separate a HOLD that pushes, a ZERO that only takes and the slot used as
    the row) on the 33 x 70 images; rows as a device tensor and, at size 3, as a host list"""
    schedule = D.RIDE_ALONG if name == 'ride_along' else D.COMPACT
    buf, ref = _Buffers(len(schedule[0][1]), D.N_ROWS, size), D.Steered(D.N_ROWS, size)
    for t, (rows, mode) in enumerate(schedule):
        r = rows if (rows is None or size == 3) else _i32(rows)
        _check_call(buf, ref, D.slot_images(t, rows, len(mode)), 0.3, mode, r, (name, size, t))


def test_steered_bounds_large_and_single_pixel():
    """(2, 480, 640) with amount 0.3 -- more four-pixel groups than a sample's 256 workgroups have lanes --, one slot held per call, a
    restart; (1, 1, 1) with amount 0; and words that are none of the three skip the slot"""
    img = [R.image(2, 480, 640, 40 + t, lo=0.05 * t, hi=1.0 - 0.04 * t) for t in range(3)]
    buf, ref = _Buffers(2, 2, 2), D.Steered(2, 2)
    for t, mode in enumerate(([D.T, D.H], [D.T, D.T], [D.H, D.Z])):
        _check_call(buf, ref, img[t], 0.3, mode, None, ('480x640', t))
    buf, ref = _Buffers(1, 1, 3), D.Steered(1, 3)
    for t, mode in enumerate(([D.T], [D.H], [D.T], [D.Z], [7], [-1])):
        _check_call(buf, ref, np.full((1, 1, 1, 1), 0.2 + 0.1 * t, dtype=R.F32), 0.0, mode, None, ('1x1', t))


@pytest.mark.parametrize('size', R.HDR_FILTER_SIZES)
def test_steered_all_take_equals_the_unsteered_call(size):
    """rows=None and every slot on TAKE: bounds, ring and state equal hip.recon_post_bounds on twin buffers, bit for bit"""
    a, b = _Buffers(3, 3, size), _Buffers(3, 3, size)
    for img in R.hdr_images():
        a.call(img, 0.3, [D.T] * 3)
        b.call(img, 0.3)
        assert torch.equal(a.bounds.view(torch.int32), b.bounds.view(torch.int32))
        assert torch.equal(a.ring.view(torch.int64), b.ring.view(torch.int64)) and torch.equal(a.state, b.state)
        assert torch.equal(a.ws.view(torch.int32), b.ws.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 2. the steered frame kernel
@pytest.mark.parametrize('size', [(5, 7), (17, 68), (16, 64), (24, 40)])
def test_steered_frame_kernel(size):
    """N = 3, slot 1 on HOLD (slot 2 on ZERO: taken like TAKE): taken rows equal the restatement, the held row keeps its sentinel in
    the uint8 and the fp32 output; an all-TAKE run equals the unsteered call"""
    from ess_amd import hip
    hs, ws = size
    cases = R.frame_cases()
    for amount in (0.0, 0.3):
        c = cases[f'{hs}x{ws}-n3-a{amount}-s1.0-b0']
        w = R.gkern(5, c['sigma'])
        u8_ref, f32_ref = R.frame(c['img'], w, c['amount'], c['bounds'], c['window'])
        img, bounds = torch.from_numpy(c['img']).to(DEV), torch.from_numpy(c['bounds']).to(DEV)
        u8 = torch.full(u8_ref.shape, 0xA5, dtype=torch.uint8, device=DEV)
        f32 = torch.full(f32_ref.shape, -7.0, dtype=torch.float32, device=DEV)
        hip.recon_post_frame(img, w, c['amount'], bounds, window=c['window'], out_u8=u8, out_f32=f32, mode=_i32([D.T, D.H, D.Z]))
        for n in (0, 2):
            assert np.array_equal(u8[n].cpu().numpy(), u8_ref[n]), (size, amount, n)
            assert (_bits(f32[n].cpu().numpy()) == _bits(f32_ref[n])).all(), (size, amount, n)
        assert bool((u8[1] == 0xA5).all()) and bool((f32[1] == -7.0).all()), (size, amount, 'the held row was written')
        a8, a32 = hip.recon_post_frame(img, w, c['amount'], bounds, window=c['window'], want_f32=True, mode=_i32([D.T] * 3))
        b8, b32 = hip.recon_post_frame(img, w, c['amount'], bounds, window=c['window'], want_f32=True)
        assert torch.equal(a8, b8) and torch.equal(a32.view(torch.int32), b32.view(torch.int32))
        assert np.array_equal(a8.cpu().numpy(), u8_ref)


# ---------------------------------------------------------------------------------------------- 3. the driver
N_WIN = 10
#   (the schedule of tests/test_hip_multi_stream.py) stream 0 runs throughout; stream 1 joins at window 3 and is restarted at window 7;
#   stream 2 is idle on windows 2 and 5.  compact=True: buckets 2, 2, 1, ride-along, ride-along, 2, ride-along ...
ACTIVE = [[True, w >= 3, w not in (2, 5)] for w in range(N_WIN)]
RESTART = {7: [1]}
FIELDS = ('labels', 'colour', 'confidence', 'image', 'frame', 'overlay')


def _options(**kw):
    from ess_amd.e2vid.options.inference_options import default_options
    o = default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else a.view(torch.int32),
                                                                       b.view(torch.uint8) if b.dtype == torch.uint8 else b.view(torch.int32))


@pytest.fixture(scope='module')
def weights():
    out = {}

    def get(rtype, C=5, K=11):
        if rtype not in out:
            cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
            out[rtype] = (cfg, O.synth_state_dict(O.e2vid_param_shapes(cfg), 171),
                          O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True))
        return out[rtype]
    return get


_GRIDS = {}


def _grids(H, W, C=5):
    """one set of host-built grids per size, shared by every test that reads it and left unchanged"""
    if (H, W) not in _GRIDS:
        g = torch.Generator().manual_seed(H * 1000 + W)
        _GRIDS[H, W] = (torch.randn(N_WIN, 3, C, H, W, generator=g) * (torch.rand(N_WIN, 3, C, H, W, generator=g) < 0.3)).to(DEV)
    return _GRIDS[H, W]


def _segmenter(wts, H, W, opts, S, display, K=11, **kw):
    from ess_amd.run_segmentation import MultiStreamSegmenter
    cfg, sd_e, sd_d = wts
    if display:
        kw = dict(kw, reconstruct=True, postprocess=True, overlay=ALPHA)
    return MultiStreamSegmenter(*M._models(cfg, sd_e, sd_d, K), H, W, opts, S, palette=SH.palette_for(K), want_confidence=True, **kw)


def _run_schedule(seg, grids, streams=(0, 1, 2)):
    """the schedule's rounds for `streams` of the three (seg serves len(streams)); an idle stream's grid is NaN: it is not read"""
    out = []
    for w in range(N_WIN):
        if w in RESTART:
            hit = [i for i, s in enumerate(streams) if s in RESTART[w]]
            if hit:
                seg.reset(hit)
        g = grids[w, list(streams)].clone()
        active = [ACTIVE[w][s] for s in streams]
        for i, a in enumerate(active):
            if not a:
                g[i] = float('nan')
        out.append(seg.update(g, active))
    return out


def _check_display(seg, res, plain, opts, what, active=ACTIVE, restart=RESTART):
    """per stream and active window: labels / colour / confidence of the plain driver; frame == a per-stream PostProcessor(n=1) fed the
    round's own image[s] on exactly the stream's active windows, reset() where its restart is carried out; overlay == viz_ref"""
    from ess_amd.e2vid.image_reconstructor import PostProcessor
    S = len(active[0])
    pal = SH.palette_for(11).numpy()
    posts = [PostProcessor(DEV, opts, n=1, crop=seg.rec.crop) for _ in range(S)]
    pending = [True] * S
    H, W = seg.height, seg.width
    for w, r in enumerate(res):
        for s in restart.get(w, ()):
            pending[s] = True
        assert r.valid == tuple(active[w])
        assert r.frame.dtype == torch.uint8 and tuple(r.frame.shape) == (S, H, W) and tuple(r.overlay.shape) == (S, H, W, 3), what
        assert r.image.dtype == torch.float32 and r.image.dim() == 4 and r.image.shape[:2] == (S, 1), what
        for s in range(S):
            if not active[w][s]:
                continue
            if plain is not None:
                for f in FIELDS[:3]:
                    assert _same(getattr(r, f)[s], getattr(plain[w], f)[s]), (what, w, s, f, 'differs from the plain driver')
            if pending[s]:
                posts[s].reset()
                pending[s] = False
            want = posts[s].process_u8(r.image[s:s + 1].clone())
            assert _same(r.frame[s:s + 1], want), (what, w, s, 'frame')
            ov = V.overlay(r.labels[s:s + 1].cpu().numpy(), r.frame[s:s + 1].cpu().numpy(), pal, ALPHA)
            assert np.array_equal(r.overlay[s:s + 1].cpu().numpy(), ov), (what, w, s, 'overlay')
    assert len(np.unique(res[-1].frame[0].cpu().numpy())) > 1  # (a frame, not a constant)


def _check_replay(re_, rg, what, active=ACTIVE):
    for w in range(len(re_)):
        for s in range(len(active[0])):
            if active[w][s]:
                for f in FIELDS:
                    assert _same(getattr(re_[w], f)[s], getattr(rg[w], f)[s]), (what, w, s, f, 'replay differs from eager')


DRIVER_CASES = [('convlstm', 'fp32', 64, 96, True), ('convlstm', 'bf16', 40, 52, True), ('convlstm', 'bf16', 64, 96, False),
                ('convlstm', 'mixed', 40, 52, False), ('convlstm', 'mixed', 64, 96, True), ('convgru', 'mixed', 40, 52, True)]


@pytest.mark.parametrize('compact', [False, True], ids=['ride', 'compact'])
@pytest.mark.parametrize('rtype,mode,H,W,auto_hdr', DRIVER_CASES)
def test_display_rounds_on_the_schedule(weights, rtype, mode, H, W, auto_hdr, compact):
    """S = 3, ten windows, eager and graph=True (warm_up() in front of the first round: it must move no history), against the
    plain driver built the same way.  40 x 52 runs reflection-padded to 40 x 56 inside.  compact=True drives buckets 1 and 2 and
    ride-along rounds; one capture per bucket and one for the ride-along round."""
    from ess_amd import hip
    opts = _options(auto_hdr=auto_hdr, auto_hdr_median_filter_size=3)
    grids = _grids(H, W)
    what = f'{rtype} {mode} {H}x{W} auto_hdr={auto_hdr} compact={compact}'
    hip.set_compute(mode)
    try:
        plain = _run_schedule(_segmenter(weights(rtype), H, W, opts, 3, False, compact=compact), grids)
        assert plain[0].image is None and plain[0].frame is None and plain[0].overlay is None
        eager = _segmenter(weights(rtype), H, W, opts, 3, True, compact=compact)
        graph = _segmenter(weights(rtype), H, W, opts, 3, True, compact=compact, graph=True)
        graph.warm_up()
        assert graph.n_captures == (3 if compact else 1)
        re_, rg = _run_schedule(eager, grids), _run_schedule(graph, grids)
        _check_display(eager, re_, plain, opts, what + ' eager')
        _check_display(graph, rg, plain, opts, what + ' graph')
        _check_replay(re_, rg, what)
        assert graph.n_captures == (3 if compact else 1) and eager.n_captures == 0 and graph.n_windows == eager.n_windows == N_WIN
        assert tuple(eager._modes.shape) == (3, 3)
    finally:
        hip.set_compute('fp32')


def test_without_the_keywords_nothing_moves(weights):
    """all three off: the mode words and bucket tables have the shapes they had, no post-processor exists"""
    seg = _segmenter(weights('convlstm'), 64, 96, _options(), 3, False, compact=True)
    assert tuple(seg._modes.shape) == (2, 3) and seg.post is None and not seg.reconstruct and seg.overlay_alpha is None
    assert all(tuple(seg._bucket[b][3].shape) == (5, b) for b in seg.buckets)
    img_only = _segmenter(weights('convlstm'), 64, 96, _options(), 3, False, reconstruct=True)
    r = img_only.update(_grids(64, 96)[0])
    assert r.image is not None and r.frame is None and r.overlay is None and tuple(img_only._modes.shape) == (2, 3)


def test_display_rounds_from_event_columns(weights):
    """event_layout='columns', compact=True, graph=True, rounds from EventColumns: the display tail composes with the in-graph ingest
    (labels of the plain columns driver, frames of the per-stream post-processors, overlays of the restatement)"""
    from ess_amd import hip
    from tests.test_hip_event_columns import _as_columns
    H, W, cap = 64, 96, 4096
    opts = _options(auto_hdr=True, auto_hdr_median_filter_size=3)
    active = [[True, False, True], [True, True, True], [False, True, False], [True, True, False], [True, False, True]]
    restart = {3: [0]}
    hip.set_compute('mixed')
    try:
        kw = dict(compact=True, graph=True, event_capacity=cap, event_layout='columns')
        plain, disp = _segmenter(weights('convlstm'), H, W, opts, 3, False, **kw), _segmenter(weights('convlstm'), H, W, opts, 3, True, **kw)
        rp, rd = [], []
        for w, act in enumerate(active):
            cols = [_as_columns(M._events(3000, H, W, 500 + 10 * w + s), (w + s) % 4) if a else None for s, a in enumerate(act)]
            for seg, out in ((plain, rp), (disp, rd)):
                if w in restart:
                    seg.reset(restart[w])
                out.append(seg.update_from_events(cols))
        _check_display(disp, rd, rp, opts, 'columns', active, restart)
        assert disp.n_captures == plain.n_captures <= 3
    finally:
        hip.set_compute('fp32')


# ---------------------------------------------------------------------------------------------- 4. a stream and its batch
@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'mixed'])
def test_display_of_a_stream_does_not_depend_on_its_batch(weights, mode):
    """the S = 3 run against MultiStreamSegmenter(n_streams=1, same keywords) fed each stream alone, the space-to-depth form pinned
    on both sides: image, frame and overlay rows (and labels) are equal bits"""
    from ess_amd import hip
    from ess_amd.e2vid.model.submodules import set_s2d_mode
    H, W = 64, 96
    opts = _options(auto_hdr=True, auto_hdr_median_filter_size=3)
    grids = _grids(H, W)
    hip.set_compute(mode)
    prev = M._pinned_s2d()
    try:
        res = _run_schedule(_segmenter(weights('convlstm'), H, W, opts, 3, True), grids)
        for s in range(3):
            solo = _run_schedule(_segmenter(weights('convlstm'), H, W, opts, 1, True), grids, streams=(s,))
            for w in range(N_WIN):
                if ACTIVE[w][s]:
                    for f in FIELDS:
                        assert _same(getattr(res[w], f)[s], getattr(solo[w], f)[0]), f'{mode}: stream {s} window {w}: {f} depends on the batch'
    finally:
        set_s2d_mode(prev)
        hip.set_compute('fp32')


# ---------------------------------------------------------------------------------------------- 5. against the single-stream driver
@pytest.mark.parametrize('H,W,mode', [(64, 96, 'bf16'), (40, 52, 'mixed')])
def test_one_stream_against_the_single_stream_display(weights, H, W, mode):
    """MultiStreamSegmenter(1, display) and StreamingSegmenter(display) over four windows, reset(), the four again: image, frame and
    overlay (and labels) are equal bits -- a zeroed state on the with-state launches against no state on the x-only launches"""
    from ess_amd import hip
    from ess_amd.run_segmentation import StreamingSegmenter
    from tests.conftest import record_parity
    opts = _options(auto_hdr=True, auto_hdr_median_filter_size=3)
    cfg, sd_e, sd_d = weights('convlstm')
    grids = _grids(H, W)
    hip.set_compute(mode)
    try:
        multi = _segmenter(weights('convlstm'), H, W, opts, 1, True)
        single = StreamingSegmenter(*M._models(cfg, sd_e, sd_d, 11), H, W, opts, palette=SH.palette_for(11), want_confidence=True,
                                    reconstruct=True, postprocess=True, overlay=ALPHA)
        equal = {f: True for f in FIELDS}
        for rep in range(2):
            for i in range(4):
                rm, rs = multi.update(grids[i, :1]), single.update(grids[i, 0])
                for f in FIELDS:
                    equal[f] = equal[f] and _same(getattr(rm, f), getattr(rs, f))
            multi.reset()
            single.reset()
        record_parity(f'MultiStreamSegmenter(1, display) vs StreamingSegmenter(display) convlstm 5x{H}x{W} K=11, 8 windows', mode,
                      **{f'{f}_bit_equal': v for f, v in equal.items()})
        assert all(equal.values()), (mode, equal)
    finally:
        hip.set_compute('fp32')
