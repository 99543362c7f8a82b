"""GPU tier of the reconstruction post-processing: ess_recon_post_frame, ess_recon_post_bounds and ess_event_preview against the numpy
float32 restatement (tests/recon_post_ref.py; checked against the reference's formulas by the CPU tier) BIT for bit, and
StreamingReconstructor(postprocess=True) eagerly and as a hipGraph replay.  No library convolution runs on the device here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ess_oracle as O  # noqa: E402
from tests import recon_post_ref as R  # noqa: E402

CASES = R.frame_cases()
SIZES = sorted({tuple(c['img'].shape[2:]) for c in CASES.values()})


def _guarded(n, h, w, lead):
    """a uint8 [n, h, w] view inside a 0xFF buffer with `lead` bytes in front of it and a guard row and column (w + 1 bytes) and more
    behind it -> (buffer, view); lead % 4 decides whether the 4-byte store path may be taken"""
    buf = torch.full((lead + n * h * w + w + 1 + 8,), 0xFF, dtype=torch.uint8, device='cuda')
    return buf, buf[lead:lead + n * h * w].view(n, h, w)


@pytest.mark.parametrize('size', SIZES, ids=[f'{h}x{w}' for h, w in SIZES])
def test_frame_kernel_equals_the_restatement_bit_for_bit(size):
    """Every case of this source size (N 1 / 3 with different bounds per sample, amount 0 / 0.3, sigma 1 / 0.5, both bounds; the 24 x 40
    source through its window): frame_u8 and frame_f32 equal the restatement; outputs start as 0xFF / NaN; the bytes in front of and
    behind the uint8 output stay 0xFF, with the output 4-byte aligned (the vector store where W % 4 == 0) and misaligned by one."""
    from ess_amd import hip
    names = [k for k, c in CASES.items() if tuple(c['img'].shape[2:]) == size]
    assert len(names) == 12
    for name in names:
        c = CASES[name]
        w = R.gkern(5, c['sigma'])
        want8, want32 = R.frame(c['img'], w, c['amount'], c['bounds'], c['window'])
        n, H, W = want8.shape
        img, bounds = torch.from_numpy(c['img']).cuda(), torch.from_numpy(c['bounds']).cuda()
        for lead in (4 * ((W + 4) // 4), W + 1 if (W + 1) % 4 else W + 2):
            buf, out8 = _guarded(n, H, W, lead)
            out32 = torch.full((n, 1, H, W), float('nan'), device='cuda')
            got8, got32 = hip.recon_post_frame(img, w, c['amount'], bounds, window=c['window'], out_u8=out8, out_f32=out32)
            assert got8 is out8 and got32 is out32
            assert np.array_equal(out8.cpu().numpy(), want8), (name, lead)
            assert np.array_equal(out32.cpu().numpy(), want32), (name, lead)
            host = buf.cpu().numpy()
            assert (host[:lead] == 0xFF).all() and (host[lead + n * H * W:] == 0xFF).all(), (name, lead)
        only8, none32 = hip.recon_post_frame(img, w, c['amount'], bounds, window=c['window'])
        assert none32 is None and np.array_equal(only8.cpu().numpy(), want8), name
        none8, only32 = hip.recon_post_frame(img, w, c['amount'], bounds, window=c['window'], want_u8=False, want_f32=True)
        assert none8 is None and np.array_equal(only32.cpu().numpy(), want32), name


def test_frame_kernel_more_than_one_workgroup_and_the_grid_stride():
    """200 x 346 (DDD17's width, the byte path; 17 400 four-pixel groups = 68 workgroups) and 8 x 480 x 640 (the vector path;
    614 400 groups on the capped grid of 2048 workgroups: every lane strides once)"""
    from ess_amd import hip
    w = R.gkern()
    for n, hs, ws, window in ((1, 200, 346, None), (8, 480, 640, None), (1, 264, 352, (2, 3, 260, 346))):
        img = R.image(n, hs, ws, 900 + n)
        bounds = R.bounds_rows([(0.05 * i, 0.9 + 0.01 * i) for i in range(n)])
        want8, _ = R.frame(img, w, 0.3, bounds, window)
        got8, _ = hip.recon_post_frame(torch.from_numpy(img).cuda(), w, 0.3, torch.from_numpy(bounds).cuda(), window=window)
        assert np.array_equal(got8.cpu().numpy(), want8), (n, hs, ws)


def test_a_nan_pixel_gives_zero():
    from ess_amd import hip
    img = R.image(1, 5, 7, 3)
    img[0, 0, 2, 3] = np.nan
    b = R.bounds_rows([(0.0, 1.0)])
    for amount in (0.0, 0.3):
        want8, _ = R.frame(img, R.gkern(), amount, b)
        got8, _ = hip.recon_post_frame(torch.from_numpy(img).cuda(), R.gkern(), amount, torch.from_numpy(b).cuda())
        assert np.array_equal(got8.cpu().numpy(), want8) and got8[0, 2, 3].item() == 0


# ---------------------------------------------------------------------------------------------- auto-HDR
def _options(**kw):
    from ess_amd.e2vid.options.inference_options import default_options
    o = default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize('size', R.HDR_FILTER_SIZES)
def test_bounds_kernel_equals_the_restatement_after_every_call(size):
    """Seven consecutive frames of three samples (every clip limit binds, the sharpened minimum is negative: the CPU tier checks the
    inputs) through IntensityRescaler's device history: bounds equal the restatement's bits after every call; the workspace is 0xFF
    before every call and fully rewritten by it; then reset(samples=[1]) empties that one history."""
    from ess_amd.e2vid.utils.inference_utils import IntensityRescaler
    w = R.gkern()
    dev = torch.device('cuda:0')
    r = IntensityRescaler(_options(auto_hdr=True, auto_hdr_median_filter_size=size), n=3, device=dev)
    hist = R.History(3, size)
    imgs = R.hdr_images()
    for t, img in enumerate(imgs):
        r.workspace.view(torch.uint8).fill_(0xFF)
        u8, _ = r.rescale(torch.from_numpy(img).cuda(), w.reshape(-1).tolist(), 0.3)
        want = hist.update(img, w, 0.3)
        assert np.array_equal(r.bounds.cpu().numpy(), want), (size, t, r.bounds.cpu().numpy(), want)
        assert np.array_equal(u8.cpu().numpy(), R.frame(img, w, 0.3, want)[0]), (size, t)
        ws = r.workspace.cpu().numpy()
        assert not np.isnan(ws).any(), (size, t)  # (0xFFFFFFFF is a NaN: no slot was left)
        s = R.sharpen(img, w, 0.3)
        assert np.array_equal(ws[:, :, 0].min(1), s.min((1, 2))) and np.array_equal(ws[:, :, 1].max(1), s.max((1, 2)))
        assert r.ring_state.cpu()[:, 1].tolist() == [min(t + 1, size + 1)] * 3
    r.reset(samples=[1])
    hist.reset(samples=[1])
    full = min(R.HDR_CALLS, size + 1)
    assert r.ring_state.cpu()[:, 1].tolist() == [full, 0, full]
    for img in imgs[:2]:
        r.rescale(torch.from_numpy(img).cuda(), w.reshape(-1).tolist(), 0.3)
        assert np.array_equal(r.bounds.cpu().numpy(), hist.update(img, w, 0.3)), size
    r.reset()
    assert r.ring_state.cpu().tolist() == [[0, 0]] * 3


def test_bounds_kernel_on_the_unsharpened_image_and_one_pixel():
    """amount = 0 (no stencil), a 1 x 1 and a 480 x 640 source (more four-pixel groups than the 256 workgroups of a sample have lanes),
    and a NaN pixel, which the min / max skip"""
    from ess_amd import hip
    w = R.gkern()
    for n, hs, ws, amount in ((1, 1, 1, 0.0), (2, 5, 7, 0.0), (2, 480, 640, 0.3), (1, 5, 7, 0.3)):
        img = R.image(n, hs, ws, 40 + hs, lo=0.1, hi=0.9)
        if (hs, amount) == (5, 0.0):
            img[1, 0, 4, 6] = np.nan
        hist = R.History(n, 2)
        ring = torch.zeros(n, 3, 2, dtype=torch.float64, device='cuda')
        state = torch.zeros(n, 2, dtype=torch.int32, device='cuda')
        wsp = torch.empty(n, hip.RECON_POST_PARTIALS, 2, device='cuda')
        bounds = torch.zeros(n, 2, device='cuda')
        for rep in range(4):
            x = (img * np.float32(1 - 0.1 * rep)).astype(np.float32)
            hip.recon_post_bounds(torch.from_numpy(x).cuda(), w, amount, wsp, ring, state, 2, bounds)
            assert np.array_equal(bounds.cpu().numpy(), hist.update(x, w, amount)), (hs, ws, amount, rep)


# ---------------------------------------------------------------------------------------------- the preview
@pytest.mark.parametrize('n,h,w', R.PREVIEW_SIZES)
def test_event_preview_equals_the_restatement(n, h, w):
    from ess_amd.e2vid.utils.inference_utils import make_event_preview
    g = R.preview_grids(n, h, w)
    x = torch.from_numpy(g).cuda()
    for nb in (-1, 2, 0, 5, 9):
        for mode in ('red-blue', 'grayscale'):
            got = make_event_preview(x, mode=mode, num_bins_to_show=nb)
            want = R.event_preview(g, mode, nb)
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (mode, nb)
    assert not np.array_equal(R.event_preview(g, 'red-blue', -1), R.event_preview(g, 'red-blue', 2))


# ---------------------------------------------------------------------------------------------- the driver
def _events(n, H, W, seed):
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0.0, 0.2, n))
    return np.stack([t, g.integers(0, W, n).astype(np.float64), g.integers(0, H, n).astype(np.float64),
                     g.integers(0, 2, n).astype(np.float64)], 1)


@pytest.mark.parametrize('H,W,rtype,mode', [(64, 96, 'convlstm', 'bf16'), (60, 90, 'convlstm', 'bf16'), (64, 96, 'convgru', 'mixed')])
def test_streaming_reconstructor_postprocess_eager_and_graph(H, W, rtype, mode):
    """Six windows, auto-HDR with filter size 3, twice with a reset() between: the replayed frames equal the eager frames bit for bit
    (the eager first window and the replays share one device history), the eager frame equals PostProcessor.process_u8 of the
    returned image (and the restatement of it), frames are [H, W] uint8 -- cropped where 60 x 90 runs padded to 64 x 96 --, and
    frames held from earlier windows stay intact under copy=True."""
    from ess_amd import hip
    from ess_amd.e2vid.image_reconstructor import PostProcessor
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.e2vid.run_reconstruction import StreamingReconstructor, events_to_voxel_grid_device, iter_windows_fixed_size
    C, n_win, per = 5, 6, 4000
    cfg = O.e2vid_config(num_bins=C, recurrent_block_type=rtype)
    sd = O.synth_state_dict(O.e2vid_param_shapes(cfg), 171)
    ev = _events(n_win * per, H, W, 5)
    opts = _options(auto_hdr=True, auto_hdr_median_filter_size=3)
    dev = torch.device('cuda:0')
    hip.set_compute(mode)
    try:
        def model():
            m = E2VIDRecurrent(dict(cfg))
            m.load_state_dict(sd)
            return m.cuda().eval()
        eager = StreamingReconstructor(model(), H, W, opts, graph=False, postprocess=True)
        graph = StreamingReconstructor(model(), H, W, opts, graph=True, postprocess=True)
        plain = StreamingReconstructor(model(), H, W, opts, graph=False)
        post = PostProcessor(dev, opts, n=1, crop=eager.rec.crop)
        hist = R.History(1, 3)
        w = R.gkern()
        held = []
        for rep in range(2):
            for i, win in enumerate(iter_windows_fixed_size(ev, per)):
                grid = events_to_voxel_grid_device(win, C, W, H, dev)
                img_e, lat_e, f_e = eager.update(grid)
                img_g, lat_g, f_g = graph.update(grid)
                assert f_e.dtype == torch.uint8 and tuple(f_e.shape) == tuple(f_g.shape) == (H, W)
                assert torch.equal(img_e, img_g) and torch.equal(f_e, f_g), (rep, i)
                assert torch.equal(post.process_u8(img_e)[0], f_e), (rep, i)
                x = img_e.cpu().numpy()
                want = R.frame(x, w, 0.3, hist.update(x, w, 0.3), post.window)[0][0]
                assert np.array_equal(f_e.cpu().numpy(), want), (rep, i)
                assert len(np.unique(want)) > 1  # (a frame, not a constant)
                held.append((f_e.clone(), f_g))
                if rep == 0:
                    out = plain.update(grid)
                    assert len(out) == 2 and torch.equal(out[0], img_e)  # (postprocess=False: the two outputs, the same image)
            assert all(torch.equal(a, b) for a, b in held)  # frames of earlier windows are intact
            assert len({b.data_ptr() for _, b in held}) == len(held)
            eager.reset()
            graph.reset()
            post.reset()
            hist.reset()
        f32 = PostProcessor(dev, opts, n=1, crop=eager.rec.crop).process(img_e)
        assert tuple(f32.shape) == (1, 1, H, W) and f32.dtype == torch.float32
        assert torch.equal((f32 * 255).round().to(torch.uint8)[0, 0], PostProcessor(dev, opts, n=1, crop=eager.rec.crop).process_u8(img_e)[0])
    finally:
        hip.set_compute('fp32')
