"""CPU tier of the reconstruction post-processing (hip.recon_post_frame, hip.recon_post_bounds, hip.event_preview; the display
helpers of e2vid/utils/inference_utils.py; image_reconstructor.PostProcessor): the three C entry points and their refusals, the
wrappers' and the classes' refusals -- each raised before a device call --, gkern, and the numpy restatement (tests/recon_post_ref.py)
that the GPU tier compares bits against: checked here against the reference's formulas evaluated by torch on the CPU on exactly the
GPU tier's inputs, and shown to be sensitive to six mutations."""
import ctypes
import os
import sys
from collections import deque

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import recon_post_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_recon_post_frame', 'ess_recon_post_bounds', 'ess_event_preview')
EINVAL = -22
CASES = R.frame_cases()


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


def _options(**kw):
    from ess_amd.e2vid.options.inference_options import default_options
    o = default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---------------------------------------------------------------------------------------------- ABI
def test_the_three_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert '#define ESS_RECON_POST_PARTIALS 256' in header and '#define ESS_RECON_POST_MAX_FILTER 63' in header
    assert 'ESS_PREVIEW_RED_BLUE = 0, ESS_PREVIEW_GRAYSCALE = 1' in header
    assert (hip.RECON_POST_PARTIALS, hip.RECON_POST_MAX_FILTER) == (R.PARTIALS, R.MAX_FILTER) == (256, 63)
    assert hip.PREVIEW_MODES == {'red-blue': 0, 'grayscale': 1}
    assert callable(hip.recon_post_frame) and callable(hip.recon_post_bounds) and callable(hip.event_preview)


# ---------------------------------------------------------------------------------------------- gkern
GKERN_SIGMA_1 = [
    0.030338143929839134, 0.03699158877134323, 0.039519015699625015, 0.03699158877134323, 0.030338143929839134,
    0.03699158877134323, 0.04510420188307762, 0.048185914754867554, 0.04510420188307762, 0.03699158877134323,
    0.039519015699625015, 0.048185914754867554, 0.05147818103432655, 0.048185914754867554, 0.039519015699625015,
    0.03699158877134323, 0.04510420188307762, 0.048185914754867554, 0.04510420188307762, 0.03699158877134323,
    0.030338143929839134, 0.03699158877134323, 0.039519015699625015, 0.03699158877134323, 0.030338143929839134]


def test_gkern_equals_the_written_values_and_the_restatement():
    from ess_amd.e2vid.utils.inference_utils import gkern
    k = gkern(5, 1.0)
    assert k.dtype == torch.float32 and tuple(k.shape) == (5, 5)
    assert k.reshape(-1).tolist() == [float(np.float32(v)) for v in GKERN_SIGMA_1]
    assert torch.equal(gkern(), k)
    for sigma in (0.5, 1.0, 2.0):
        assert np.array_equal(gkern(5, sigma).numpy(), R.gkern(5, sigma)), sigma
        assert abs(float(gkern(5, sigma).double().sum()) - 1.0) < 1e-6


@pytest.mark.parametrize('sigma', [0.5, 1.0, 2.0])
def test_gkern_equals_the_scipy_form_bit_for_bit(sigma):
    st = pytest.importorskip('scipy.stats')
    from ess_amd.e2vid.utils.inference_utils import gkern
    interval = (2 * sigma + 1.) / 5
    x = np.linspace(-sigma - interval / 2., sigma + interval / 2., 6)
    k1 = np.diff(st.norm.cdf(x))
    raw = np.sqrt(np.outer(k1, k1))
    assert np.array_equal(gkern(5, sigma).numpy(), (raw / raw.sum()).astype(np.float32))


# ---------------------------------------------------------------------------------------------- the library
def test_the_library_refuses_in_front_of_any_launch(built_lib):
    """ESS_EINVAL with a message that names the argument; no device pointer is followed (no GPU is needed): any aligned address does.
    The weights are HOST memory and are read only after every check has passed, so they are a real array here."""
    from ess_amd import hip
    L = hip.lib()
    P, A = ctypes.c_void_p, 0x10000
    W25 = (ctypes.c_float * 25)(*([0.04] * 25))
    err = L.ess_last_error

    def frame(img=A, w=W25, c1=1.3, amount=0.3, bounds=A, u8=A, f32=A, N=1, hs=24, ws=40, win=(0, 0, 24, 40)):
        return L.ess_recon_post_frame(P(img), w, c1, amount, P(bounds), P(u8), P(f32), N, hs, ws, *win, None)
    assert frame(img=0) == EINVAL and b'null img' in err()
    assert frame(bounds=0) == EINVAL and b'null bounds' in err()
    assert frame(u8=0, f32=0) == EINVAL and b'both null' in err()
    assert frame(w=None) == EINVAL and b'needs the 25 weights' in err()
    assert frame(img=A + 2) == EINVAL and b'aligned' in err()
    assert frame(f32=A + 2) == EINVAL and b'aligned' in err()
    assert frame(amount=float('nan')) == EINVAL and b'NaN' in err()
    for kw in (dict(N=0), dict(hs=0), dict(ws=-1)):
        assert frame(**kw) == EINVAL and b'bad extents' in err()
    for win in ((0, 0, 25, 40), (0, 0, 24, 41), (1, 0, 24, 40), (0, 7, 24, 34), (-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 5, 0),
                (2 ** 31 - 1, 0, 2, 2)):
        assert frame(win=win) == EINVAL and b'leaves the 24 x 40 source' in err(), win

    def bounds(img=A, w=W25, amount=0.3, N=3, hs=33, ws=70, ws_ptr=A, ws_bytes=None, ring=A, state=A, size=3, out=A):
        nbytes = N * 256 * 2 * 4 if ws_bytes is None else ws_bytes
        return L.ess_recon_post_bounds(P(img), w, 1.3, amount, N, hs, ws, P(ws_ptr), nbytes, P(ring), P(state), size, P(out), None)
    for size in (64, -1, 1 << 20):
        assert bounds(size=size) == EINVAL and f'filter_size={size} outside 0..63'.encode() in err()
    for kw in (dict(ws_ptr=0), dict(ring=0), dict(state=0), dict(out=0)):
        assert bounds(**kw) == EINVAL and b'null' in err()
    assert bounds(img=0) == EINVAL and b'null img' in err()
    assert bounds(ws_bytes=3 * 256 * 8 - 4) == EINVAL and b'workspace has' in err()
    assert bounds(ring=A + 4) == EINVAL and b'aligned' in err()
    assert bounds(N=65536, ws_bytes=1 << 40) == EINVAL and b'65535' in err()
    assert bounds(w=None) == EINVAL and b'needs the 25 weights' in err()

    def preview(x=A, out=A, N=1, C=5, H=5, W=7, nb=-1, mode=0):
        return L.ess_event_preview(P(x), P(out), N, C, H, W, nb, mode, None)
    assert preview(x=0) == EINVAL and b'null' in err()
    assert preview(out=0) == EINVAL and b'null' in err()
    for mode in (2, -1):
        assert preview(mode=mode) == EINVAL and f'mode={mode}'.encode() in err()
    for kw in (dict(N=0), dict(C=0), dict(H=0), dict(W=-3)):
        assert preview(**kw) == EINVAL and b'bad extents' in err()
    assert preview(x=A + 2) == EINVAL and b'aligned' in err()


# ---------------------------------------------------------------------------------------------- the wrappers
def _frame_call():
    return dict(img=torch.zeros(2, 1, 24, 40), weights=R.gkern(), amount=0.3, bounds=torch.zeros(2, 2))


FRAME_REFUSALS = [
    (dict(img=torch.zeros(2, 24, 40)), r'img must be a non-empty contiguous fp32 \[N, 1, Hs, Ws\]'),
    (dict(img=torch.zeros(2, 2, 24, 40)), 'img must be'),
    (dict(img=torch.zeros(2, 1, 24, 40, dtype=torch.float64)), 'img must be'),
    (dict(img=torch.zeros(2, 1, 24, 80)[..., ::2]), 'img must be'),
    (dict(img=torch.zeros(0, 1, 24, 40)), 'img must be'),
    (dict(img=np.zeros((2, 1, 24, 40), np.float32)), 'img must be'),
    (dict(weights=None), 'needs the 5 x 5 weights'),
    (dict(weights=np.zeros(24, np.float32)), 'weights must be 25 finite values'),
    (dict(weights=np.full((5, 5), np.nan, np.float32)), 'weights must be 25 finite values'),
    (dict(amount=float('nan')), 'amount is NaN'),
    (dict(bounds=torch.zeros(2)), r'bounds must be a contiguous torch.float32 \[2, 2\]'),
    (dict(bounds=torch.zeros(3, 2)), 'bounds must be'),
    (dict(bounds=torch.zeros(2, 2, dtype=torch.float64)), 'bounds must be'),
    (dict(bounds=[[0.0, 1.0]] * 2), 'bounds must be'),
    (dict(window=(0, 0, 25, 40)), 'window .* leaves the 24 x 40 source'),
    (dict(window=(2, 3, 19, 38)), 'window .* leaves'),
    (dict(window=(-1, 0, 4, 4)), 'window .* leaves'),
    (dict(window=(0, 0, 0, 4)), 'window .* leaves'),
    (dict(want_u8=False), 'neither frame_u8 nor frame_f32'),
    (dict(out_u8=torch.zeros(2, 24, 40)), 'out_u8 must be'),
    (dict(out_u8=torch.zeros(2, 1, 24, 40, dtype=torch.uint8)), 'out_u8 must be'),
    (dict(out_f32=torch.zeros(2, 24, 40)), 'out_f32 must be'),
    (dict(), 'no CPU path'),
]


@pytest.mark.parametrize('change,message', FRAME_REFUSALS, ids=[m[:28] + str(i) for i, (_, m) in enumerate(FRAME_REFUSALS)])
def test_recon_post_frame_refuses_before_any_device_call(change, message):
    from ess_amd import hip
    kw = _frame_call()
    kw.update(change)
    with pytest.raises(hip.EssHipError, match=message):
        hip.recon_post_frame(**kw)


def _bounds_call():
    return dict(img=torch.zeros(3, 1, 33, 70), weights=R.gkern(), amount=0.3, workspace=torch.zeros(3, 256, 2),
                ring=torch.zeros(3, 4, 2, dtype=torch.float64), ring_state=torch.zeros(3, 2, dtype=torch.int32), filter_size=3,
                bounds=torch.zeros(3, 2))


BOUNDS_REFUSALS = [
    (dict(filter_size=64), 'filter_size=64 outside 0..63'),
    (dict(filter_size=-1), 'filter_size=-1 outside'),
    (dict(filter_size=2.5), 'filter_size=2.5 outside'),
    (dict(filter_size=True), 'filter_size=True outside'),
    (dict(filter_size=10), r'ring must be a contiguous torch.float64 \[3, 11, 2\]'),
    (dict(ring=torch.zeros(3, 4, 2)), 'ring must be'),
    (dict(ring_state=torch.zeros(3, 2, dtype=torch.int64)), 'ring_state must be'),
    (dict(ring_state=torch.zeros(3, dtype=torch.int32)), 'ring_state must be'),
    (dict(workspace=torch.zeros(3, 255, 2)), r'workspace must be a contiguous torch.float32 \[3, 256, 2\]'),
    (dict(workspace=torch.zeros(2, 256, 2)), 'workspace must be'),
    (dict(bounds=torch.zeros(3, 3)), 'bounds must be'),
    (dict(img=torch.zeros(3, 33, 70)), 'img must be'),
    (dict(weights=None), 'needs the 5 x 5 weights'),
    (dict(), 'no CPU path'),
]


@pytest.mark.parametrize('change,message', BOUNDS_REFUSALS, ids=[m[:28] + str(i) for i, (_, m) in enumerate(BOUNDS_REFUSALS)])
def test_recon_post_bounds_refuses_before_any_device_call(change, message):
    from ess_amd import hip
    kw = _bounds_call()
    kw.update(change)
    with pytest.raises(hip.EssHipError, match=message):
        hip.recon_post_bounds(**kw)


def test_event_preview_refuses_before_any_device_call():
    from ess_amd import hip
    from ess_amd.e2vid.utils.inference_utils import make_event_preview
    g = torch.zeros(1, 5, 5, 7)
    for kw, message in ((dict(mode='colour'), "mode must be 'red-blue' or 'grayscale'"), (dict(grids=torch.zeros(5, 5, 7)), 'grids must be'),
                        (dict(grids=g.double()), 'grids must be'), (dict(grids=g[..., ::2]), 'grids must be'),
                        (dict(num_bins_to_show=1.5), 'no whole number'), (dict(out=torch.zeros(1, 5, 7, dtype=torch.uint8)), 'out must be'),
                        (dict(mode='grayscale', out=torch.zeros(1, 5, 7, 3, dtype=torch.uint8)), 'out must be'), (dict(), 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=message):
            hip.event_preview(**{'grids': g, **kw})
    with pytest.raises(ValueError, match='mode must be'):
        make_event_preview(g, mode='colour')
    with pytest.raises(hip.EssHipError, match='no CPU path'):
        make_event_preview(g)


# ---------------------------------------------------------------------------------------------- the classes
def test_the_classes_refuse_what_the_kernels_cannot_do():
    from ess_amd import hip
    from ess_amd.e2vid.image_reconstructor import PostProcessor
    from ess_amd.e2vid.utils.inference_utils import ImageFilter, IntensityRescaler, UnsharpMaskFilter
    cpu = torch.device('cpu')
    for lo, hi in ((0.5, 0.5), (0.6, 0.4)):
        with pytest.raises(hip.EssHipError, match='Imax=.* <= Imin='):
            IntensityRescaler(_options(Imin=lo, Imax=hi), device=cpu)
    for size in (64, -1, 2.5):
        with pytest.raises(hip.EssHipError, match='auto_hdr_median_filter_size=.* outside 0..63'):
            IntensityRescaler(_options(auto_hdr=True, auto_hdr_median_filter_size=size), device=cpu)
    IntensityRescaler(_options(auto_hdr=False, auto_hdr_median_filter_size=64), device=cpu)  # (unused without auto_hdr, as in the reference)
    with pytest.raises(NotImplementedError, match='cv2.bilateralFilter'):
        ImageFilter(_options(bilateral_filter_sigma=1.0))
    with pytest.raises(NotImplementedError, match='cv2.bilateralFilter'):
        PostProcessor(cpu, _options(bilateral_filter_sigma=0.5))
    assert ImageFilter(_options())('anything') == 'anything'
    with pytest.raises(ValueError, match='unsharp_mask_sigma'):
        UnsharpMaskFilter(_options(unsharp_mask_sigma=0.0), cpu)
    u = UnsharpMaskFilter(_options(), cpu)
    assert tuple(u.gaussian_kernel.shape) == (1, 1, 5, 5) and u.weights == u.gaussian_kernel.reshape(-1).tolist() and len(u.weights) == 25
    with pytest.raises(NotImplementedError, match='fused into the rescale'):
        u(torch.zeros(1, 1, 4, 4))
    z = torch.zeros(1, 1, 4, 4)
    assert UnsharpMaskFilter(_options(unsharp_mask_amount=0.0), cpu)(z) is z
    r = IntensityRescaler(_options(Imin=0.12, Imax=0.83), n=3, device=cpu)
    assert np.array_equal(r.bounds.numpy(), R.bounds_rows([(0.12, 0.83)] * 3)) and r.ring is None
    r.reset()
    h = IntensityRescaler(_options(auto_hdr=True, auto_hdr_median_filter_size=3), n=2, device=cpu)
    assert tuple(h.ring.shape) == (2, 4, 2) and h.ring.dtype == torch.float64 and tuple(h.workspace.shape) == (2, 256, 2)
    h.ring_state.fill_(3)
    h.reset(samples=[1])
    assert h.ring_state.tolist() == [[3, 3], [0, 0]]
    with pytest.raises(hip.EssHipError, match='sample 2 outside'):
        h.reset(samples=[2])
    with pytest.raises(hip.EssHipError, match='made for 2 samples'):
        h.rescale(torch.zeros(1, 1, 4, 4))
    from ess_amd.e2vid.utils.inference_utils import CropParameters
    assert PostProcessor(cpu, _options(), crop=CropParameters(90, 60, 3)).window == (2, 3, 60, 90)
    assert PostProcessor(cpu, _options(), crop=CropParameters(96, 64, 3)).window is None


def test_the_streaming_driver_takes_the_keyword_and_leaves_the_default_alone():
    import inspect
    from ess_amd.e2vid.run_reconstruction import StreamingReconstructor
    p = inspect.signature(StreamingReconstructor.__init__).parameters
    assert p['postprocess'].default is False and list(p)[-1] == 'postprocess'


# ---------------------------------------------------------------------------------------------- the restatement against torch
def _torch_frame(img, w, amount, imin, imax):
    """The reference's lines (UnsharpMaskFilter.__call__, IntensityRescaler.__call__ without auto-HDR) on one sample, torch on the CPU;
    imin / imax are Python floats as the options are -> uint8 [Hs, Ws] of the whole frame"""
    x = torch.from_numpy(img)[None]
    if amount > 0:
        blurred = F.conv2d(x, torch.from_numpy(w)[None, None], padding=2)
        x = (1 + amount) * x - amount * blurred
    x = 255.0 * (x - imin) / (imax - imin)
    x.clamp_(0.0, 255.0)
    return x.byte()[0, 0].numpy(), x


PAIRS = {0: lambda n: [R.BOUNDS[0]] if n == 1 else [R.BOUNDS[0], R.BOUNDS[1], (0.3, 0.4)],
         1: lambda n: [R.BOUNDS[1]] if n == 1 else [R.BOUNDS[1], R.BOUNDS[0], (0.3, 0.4)]}


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_restatement_against_the_reference_lines_in_torch(name):
    """On every frame case of the GPU tier: at most one grey level apart, and only where the float64 value in front of the truncation
    lies within delta (R.delta: 27 float32 roundings scaled by 255 / range) of a whole number; such pixels are at most 5 % of a case
    (a condition on the inputs).  The float32 form of the frame is float(u8) / 255."""
    c = CASES[name]
    w = R.gkern(5, c['sigma'])
    n = c['img'].shape[0]
    got, got32 = R.frame(c['img'], w, c['amount'], c['bounds'], c['window'])
    pre = R.pre_truncation_f64(c['img'], w, c['amount'], c['bounds'], c['window'])
    d = R.delta(c['img'], w, c['amount'], c['bounds'])
    pairs = PAIRS[int(name[-1])](n)
    assert np.array_equal(c['bounds'], R.bounds_rows(pairs))
    y0, x0, H, W = c['window'] or (0, 0) + c['img'].shape[2:]
    near_all = 0
    for i in range(n):
        want = _torch_frame(c['img'][i], w, c['amount'], *pairs[i])[0][y0:y0 + H, x0:x0 + W]
        near = np.abs(pre[i] - np.rint(pre[i])) <= d[i]
        diff = got[i].astype(int) - want.astype(int)
        assert np.abs(diff).max() <= 1, (name, i)
        assert not (diff != 0)[~near].any(), (name, i, int((diff != 0).sum()))
        near_all += int((near & (pre[i] > -1) & (pre[i] < 256)).sum())
        assert d[i] < 0.02
    assert near_all <= 0.05 * got.size + 1, (name, near_all, got.size)  # (+ 1: the 1 x 1 and 2 x 3 sources have under 20 pixels)
    assert got32.dtype == np.float32 and got32.shape == (n, 1, H, W)
    assert np.array_equal(got32[:, 0], torch.from_numpy(got).float().div(255).numpy())


def test_the_cases_cover_what_the_kernel_branches_on():
    sizes = {tuple(c['img'].shape[2:]) for c in CASES.values()}
    assert sizes == set(R.FRAME_SIZES) | {(24, 40)} and len(CASES) == 7 * 2 * 3 * 2
    assert {c['window'] for c in CASES.values()} == {None, (2, 3, 19, 34)}
    assert any(s[1] % 4 == 0 for s in sizes) and any(s[1] % 4 == 2 for s in sizes) and any(s[1] % 4 == 3 for s in sizes)
    for c in CASES.values():  # the images overshoot [0, 1]: every case of some size has pixels that clamp at either end
        assert c['img'].min() < 0.0 < 1.0 < c['img'].max() or c['img'].size < 200


def test_nan_pixels_become_zero_and_are_skipped_by_the_bounds():
    img = R.image(1, 5, 7, 3)
    img[0, 0, 2, 3] = np.nan
    u8, _ = R.frame(img, R.gkern(), 0.0, R.bounds_rows([(0.0, 1.0)]))
    assert u8[0, 2, 3] == 0 and (u8 > 0).sum() > 20
    u8s, _ = R.frame(img, R.gkern(), 0.3, R.bounds_rows([(0.0, 1.0)]))
    assert (u8s[0, 0:5, 1:6] == 0).all()  # (the NaN reaches every pixel whose stencil holds it)
    b = R.History(1, 0).update(img, R.gkern(), 0.0)
    assert np.isfinite(b).all() and b[0, 0] == np.float32(np.clip(np.nanmin(img), 0, 0.45))


# ---------------------------------------------------------------------------------------------- auto-HDR
def test_the_auto_hdr_inputs_bind_every_clip_limit():
    w = R.gkern()
    lo_bind = {0: False, 0.45: False}
    hi_bind = {0.55: False, 1.0: False}
    free = negative = False
    for img in R.hdr_images():
        s = R.sharpen(img, w, 0.3)
        for i in range(3):
            mn, mx = float(s[i].min()), float(s[i].max())
            lo_bind[0] |= mn < 0
            lo_bind[0.45] |= mn > 0.45
            hi_bind[0.55] |= mx < 0.55
            hi_bind[1.0] |= mx > 1.0
            free |= 0 < mn < 0.45 and 0.55 < mx < 1.0
            negative |= mn < 0
    assert all(lo_bind.values()) and all(hi_bind.values()) and free and negative


@pytest.mark.parametrize('size', R.HDR_FILTER_SIZES)
def test_the_history_restatement_against_the_reference_lines(size):
    """The reference's auto-HDR lines (min / max .item(), np.clip, the deque that pops when LONGER than the filter size, np.median) per
    sample on torch's sharpened image: the bounds agree to the error of s (R.sharpen_error, 27 roundings) -- exactly where a clip
    limit binds --, through seven calls."""
    w = R.gkern()
    hist = R.History(3, size)
    dq = [deque() for _ in range(3)]
    for t, img in enumerate(R.hdr_images()):
        got = hist.update(img, w, 0.3)
        e = R.sharpen_error(img, w, 0.3)
        for i in range(3):
            x = torch.from_numpy(img[i])[None]
            x = (1 + 0.3) * x - 0.3 * F.conv2d(x, torch.from_numpy(w)[None, None], padding=2)
            imin, imax = np.clip(torch.min(x).item(), 0.0, 0.45), np.clip(torch.max(x).item(), 0.55, 1.0)
            if len(dq[i]) > size:
                dq[i].popleft()
            dq[i].append((imin, imax))
            lo, hi = np.median([a for a, _ in dq[i]]), np.median([b for _, b in dq[i]])
            assert len(hist.held[i]) == len(dq[i]) == min(t + 1, size + 1)
            assert abs(float(got[i, 0]) - lo) <= e + 2 ** -24 and abs(float(got[i, 1]) - (hi - lo)) <= 2 * e + 2 ** -24, (size, t, i)
            if i == 1:
                assert got[i].tolist() == [np.float32(0.45), np.float32(0.55 - 0.45)]


def test_reset_of_one_sample_in_the_restatement():
    w = R.gkern()
    a, b = R.History(3, 3), R.History(3, 3)
    imgs = R.hdr_images()
    for img in imgs[:3]:
        a.update(img, w, 0.3)
    a.reset(samples=[1])
    assert [len(h) for h in a.held] == [3, 0, 3]
    got = a.update(imgs[3], w, 0.3)
    for img in imgs[:3]:
        b.update(img, w, 0.3)
    full = b.update(imgs[3], w, 0.3)
    assert np.array_equal(got[[0, 2]], full[[0, 2]]) and np.array_equal(got[1], R.History(3, 3).update(imgs[3], w, 0.3)[1])


# ---------------------------------------------------------------------------------------------- sensitivity
def test_each_mutant_of_the_restatement_changes_an_output():
    """What the GPU tier's bit comparison can see: one dropped tap, edge clamp for zero padding, rounding for truncation (frame case
    33x70-n1-a0.3-s1.0-b1); a ring of `size` entries, the mean for the median, bounds from the unsharpened image (the auto-HDR
    frames, filter size 3)."""
    c = CASES['33x70-n1-a0.3-s1.0-b1']
    w = R.gkern(5, c['sigma'])
    base = R.frame(c['img'], w, c['amount'], c['bounds'])[0]
    for mutant in (dict(drop_tap=(0, 0)), dict(drop_tap=(2, 2)), dict(drop_tap=(4, 3)), dict(edge='clamp'), dict(rounding='round')):
        other = R.frame(c['img'], w, c['amount'], c['bounds'], **mutant)[0]
        assert (other != base).any(), mutant
    edge = R.frame(c['img'], w, c['amount'], c['bounds'], edge='clamp')[0]
    assert np.array_equal(edge[:, 2:-2, 2:-2], base[:, 2:-2, 2:-2])  # (the padding rule shows in the two border rows and columns only)
    imgs = R.hdr_images()
    for mutant in (dict(ring_extra=0), dict(stat='mean'), dict(bounds_from='raw')):
        ref, mut = R.History(3, 3), R.History(3, 3, **mutant)
        differs = False
        for img in imgs:
            differs |= not np.array_equal(ref.update(img, w, 0.3), mut.update(img, w, 0.3))
        assert differs, mutant


# ---------------------------------------------------------------------------------------------- the preview
@pytest.mark.parametrize('n,h,w', R.PREVIEW_SIZES)
@pytest.mark.parametrize('nb', [-1, 2])
def test_the_preview_restatement_against_the_reference_lines(n, h, w, nb):
    """make_event_preview's lines per sample (torch.sum over the shown bins, the two masks, the grey ramp): equal where the grey value
    lies inside [0, 255]; outside, the reference's cast-then-clip wraps and the restatement saturates (the stated deviation)."""
    g = R.preview_grids(n, h, w)
    rb, grey = R.event_preview(g, 'red-blue', nb), R.event_preview(g, 'grayscale', nb)
    assert rb.shape == (n, h, w, 3) and grey.shape == (n, h, w) and rb.dtype == grey.dtype == np.uint8
    saturated = 0
    for i in range(n):
        t = torch.from_numpy(g[i])
        s = (torch.sum(t, dim=0) if nb < 0 else torch.sum(t[-nb:], dim=0)).numpy()
        want = np.zeros((h, w, 3), dtype=np.uint8)
        want[:, :, 0][s > 0] = 255
        want[:, :, 2][s < 0] = 255
        assert np.array_equal(rb[i], want)
        q = 255.0 * (s - (-10.0)) / (10.0 - (-10.0))
        inside = (q >= 0) & (q < 256)
        assert np.array_equal(grey[i][inside], q[inside].astype(np.uint8))
        assert (grey[i][q >= 256] == 255).all() and (grey[i][q < 0] == 0).all()
        saturated += int((~inside).sum())
        assert (s > 0).any() and (s < 0).any() and (s == 0).any()
    assert saturated > 0
    assert R.first_bin(5, -1) == R.first_bin(5, 0) == R.first_bin(5, 5) == R.first_bin(5, 9) == 0 and R.first_bin(5, 2) == 3
