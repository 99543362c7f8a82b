"""Event pre-processing, crop geometry and the display helpers (reference: e2vid/utils/inference_utils.py:18-53,60-153,261-338)."""
from math import ceil, erf, erfc, floor, sqrt

import numpy as np
import torch
from torch.nn import ReflectionPad2d

from ... import hip


class EventPreprocessor:
    """Normalises a voxel-grid step tensor so that its NON-ZERO entries have mean 0 / std 1 over the whole
    tensor (reference :96-107) -- one reduction + one map kernel, no host synchronisation (the reference's
    `if num_nonzeros > 0` is evaluated on the device).  Hot-pixel removal and flipping keep their semantics."""

    def __init__(self, options):
        self.no_normalize = options.no_normalize
        self.hot_pixel_locations = []
        if getattr(options, 'hot_pixels_file', None):
            try:
                self.hot_pixel_locations = np.loadtxt(options.hot_pixels_file, delimiter=',').astype(int)
            except IOError:
                print('WARNING: could not load hot pixels file: {}'.format(options.hot_pixels_file))
        self.flip = options.flip

    def __call__(self, events):
        for x, y in self.hot_pixel_locations:
            events[:, :, y, x] = 0
        if self.flip:
            events = torch.flip(events, dims=[2, 3])
        if not self.no_normalize:
            events = hip.event_normalize(events.contiguous())
        return events


def optimal_crop_size(max_size, max_subsample_factor):
    m = 2 ** max_subsample_factor
    return int(m * ceil(max_size / m))


class CropParameters:
    """Reflection padding up to a multiple of 2^num_encoders (reference :302-338).  The ESS trainers always
    pass extents that already are multiples of 8, where this is the identity; otherwise torch's ReflectionPad2d
    does the (cold-path) copy."""

    def __init__(self, width, height, num_encoders):
        self.height, self.width, self.num_encoders = height, width, num_encoders
        self.width_crop_size = optimal_crop_size(width, num_encoders)
        self.height_crop_size = optimal_crop_size(height, num_encoders)
        self.padding_top = ceil(0.5 * (self.height_crop_size - height))
        self.padding_bottom = floor(0.5 * (self.height_crop_size - height))
        self.padding_left = ceil(0.5 * (self.width_crop_size - width))
        self.padding_right = floor(0.5 * (self.width_crop_size - width))
        self.is_identity = not (self.padding_top or self.padding_bottom or self.padding_left or self.padding_right)
        self._pad = ReflectionPad2d((self.padding_left, self.padding_right, self.padding_top, self.padding_bottom))
        self.cx, self.cy = floor(self.width_crop_size / 2), floor(self.height_crop_size / 2)
        self.ix0, self.ix1 = self.cx - floor(width / 2), self.cx + ceil(width / 2)
        self.iy0, self.iy1 = self.cy - floor(height / 2), self.cy + ceil(height / 2)

    def pad(self, x):
        return x if self.is_identity else self._pad(x).contiguous()


def _norm_cdf(x):
    """The standard normal CDF as scipy's ndtr evaluates it (erf in the middle, erfc in the tails), on math.erf / math.erfc in
    float64: scipy is not assumed where this runs."""
    t = x * sqrt(0.5)
    z = abs(t)
    if z < sqrt(0.5):
        return 0.5 + 0.5 * erf(t)
    y = 0.5 * erfc(z)
    return 1.0 - y if t > 0 else y


def gkern(kernlen=5, nsig=1.0):
    """The reference's 2-D Gaussian kernel (:45-53) -> fp32 [kernlen, kernlen], computed in float64."""
    interval = (2 * nsig + 1.) / kernlen
    x = np.linspace(-nsig - interval / 2., nsig + interval / 2., kernlen + 1)
    kern1d = np.diff(np.array([_norm_cdf(float(v)) for v in x], dtype=np.float64))
    kernel_raw = np.sqrt(np.outer(kern1d, kern1d))
    kernel = kernel_raw / kernel_raw.sum()
    return torch.from_numpy(kernel).float()


def make_event_preview(events, mode='red-blue', num_bins_to_show=-1):
    """The reference's event preview (:18-42) for EVERY sample, on the device: events fp32 [N, C, H, W] -> uint8 [N, H, W, 3] (BGR;
    'red-blue') or uint8 [N, H, W] ('grayscale'), a device tensor (the reference returns sample 0 as a numpy array).  Deviation: the
    grey value is clamped to [0, 255] before the cast; the reference casts first and lets out-of-range values wrap."""
    if mode not in ('red-blue', 'grayscale'):
        raise ValueError(f"make_event_preview: mode must be 'red-blue' or 'grayscale', got {mode!r}")
    return hip.event_preview(events, mode, num_bins_to_show)


class UnsharpMaskFilter:
    """The unsharp mask's parameters (reference :261-279): `weights`, the 5 x 5 Gaussian of unsharp_mask_sigma, `amount`, and the
    reference's `gaussian_kernel` tensor.  The filter itself runs inside the frame and bounds kernels (hip.recon_post_frame /
    hip.recon_post_bounds), which recompute the sharpened value per pixel and never write it: PostProcessor is its caller."""

    def __init__(self, options, device):
        self.unsharp_mask_amount = float(options.unsharp_mask_amount)
        self.unsharp_mask_sigma = float(options.unsharp_mask_sigma)
        if not self.unsharp_mask_sigma > 0:
            raise ValueError(f'unsharp_mask_sigma={self.unsharp_mask_sigma} must be positive')
        self.gaussian_kernel_size = 5
        k = gkern(self.gaussian_kernel_size, self.unsharp_mask_sigma)
        self.weights = k.reshape(-1).tolist()  # (host values: the kernels take them by value)
        self.gaussian_kernel = k.unsqueeze(0).unsqueeze(0).to(device)

    def __call__(self, img):
        if self.unsharp_mask_amount > 0:
            raise NotImplementedError('the sharpened image is not materialised here: the unsharp mask is fused into the rescale '
                                      '(PostProcessor.process / process_u8, hip.recon_post_frame)')
        return img


class IntensityRescaler:
    """Rescales intensities to 8 bit with fixed (Imin, Imax) or auto-HDR bounds (reference :112-153), for `n` samples with one history
    each (n = 1: the reference).  All state is static device memory -- `bounds` fp32 [n, 2] = (Imin, Imax - Imin), the histories `ring`
    fp64 [n, size + 1, 2] with `ring_state` int32 [n, 2], the min / max `workspace` -- and a call makes no synchronisation, so it can be
    captured in a hipGraph; the reference fetches min and max with .item() and keeps a deque on the host.
    Deviation: NaN pixels are skipped by the auto-HDR min / max."""

    def __init__(self, options, n=1, device=None):
        self.device = device if device is not None else torch.device('cuda:0')
        self.n = int(n)
        if self.n < 1:
            raise ValueError(f'IntensityRescaler: n={n} samples')
        self.auto_hdr = bool(options.auto_hdr)
        self.auto_hdr_median_filter_size = options.auto_hdr_median_filter_size
        size = self.auto_hdr_median_filter_size
        if self.auto_hdr and (isinstance(size, bool) or int(size) != size or not 0 <= size <= hip.RECON_POST_MAX_FILTER):
            raise hip.EssHipError(f'auto_hdr_median_filter_size={size} outside 0..{hip.RECON_POST_MAX_FILTER}')
        self.Imin, self.Imax = float(options.Imin), float(options.Imax)
        if not self.Imax > self.Imin:
            raise hip.EssHipError(f'Imax={self.Imax} <= Imin={self.Imin}: an empty intensity range')
        # (Imax - Imin in double, rounded once: what `255.0 * (img - Imin) / (Imax - Imin)` divides an fp32 tensor by)
        self.bounds = torch.tensor([[self.Imin, self.Imax - self.Imin]] * self.n, dtype=torch.float64).to(torch.float32).to(self.device)
        self.ring = self.ring_state = self.workspace = None
        if self.auto_hdr:
            self.ring = torch.zeros(self.n, int(size) + 1, 2, dtype=torch.float64, device=self.device)
            self.ring_state = torch.zeros(self.n, 2, dtype=torch.int32, device=self.device)
            self.workspace = torch.empty(self.n, hip.RECON_POST_PARTIALS, 2, dtype=torch.float32, device=self.device)

    def reset(self, samples=None):
        """Empty the histories of `samples` (default: all): device fills only.  The bounds are rewritten by the next call."""
        if self.ring_state is None:
            return
        if samples is None:
            self.ring_state.zero_()
            return
        for s in samples:
            if not 0 <= int(s) < self.n:
                raise hip.EssHipError(f'IntensityRescaler.reset: sample {s} outside 0..{self.n - 1}')
            self.ring_state[int(s)].zero_()

    def state_tensors(self):
        """the device tensors a call changes (a driver that runs a warm-up window saves and restores them)"""
        return [t for t in (self.bounds, self.ring, self.ring_state) if t is not None]

    def rescale(self, img, weights=None, amount=0.0, window=None, want_u8=True, want_f32=False, mode=None, rows=None):
        """(unsharp mask with `weights`, `amount` +) rescale of img fp32 [n, 1, Hs, Ws] -> (uint8 [n, H, W] or None, fp32 [n, 1, H, W] or
        None); with auto_hdr the bounds are first updated from this frame.
        mode / rows (default None: the call above, launch for launch): the steered call of a multi-stream round.  `n` is then the number
        of history ROWS and img holds N SLOTS (N <= n with rows, N == n without); mode int32 [N] on the device: CARRY_TAKE -- the slot's
        history row takes this frame --, CARRY_ZERO -- the row is emptied first (the restart) --, anything else: the slot is skipped, no
        history moves and its output rows are unspecified; rows int32 [N] on the device (or a host list): the history row of each slot,
        default the slot's number.  bounds and workspace are indexed by slot: their first N entries are used.  With fixed bounds only
        the steered frame launch runs."""
        if mode is None:
            if rows is not None:
                raise hip.EssHipError('IntensityRescaler: rows= belongs to the steered call: pass mode= with it')
            if torch.is_tensor(img) and img.dim() == 4 and img.shape[0] != self.n:
                raise hip.EssHipError(f'IntensityRescaler: made for {self.n} samples, got {img.shape[0]}')
            if self.auto_hdr:
                hip.recon_post_bounds(img, weights, amount, self.workspace, self.ring, self.ring_state, int(self.auto_hdr_median_filter_size),
                                      self.bounds)
            return hip.recon_post_frame(img, weights, amount, self.bounds, window=window, want_u8=want_u8, want_f32=want_f32)
        N = img.shape[0] if torch.is_tensor(img) and img.dim() == 4 else self.n
        if N > self.n or (rows is None and N != self.n):
            raise hip.EssHipError(f'IntensityRescaler: made for {self.n} history rows, got {N} slots' + (' without rows=' if N < self.n else ''))
        if self.auto_hdr:
            hip.recon_post_bounds(img, weights, amount, self.workspace[:N], self.ring, self.ring_state, int(self.auto_hdr_median_filter_size),
                                  self.bounds[:N], mode=mode, rows=rows)
        elif rows is not None and not torch.is_tensor(rows) and len(rows) != N:
            raise hip.EssHipError(f'IntensityRescaler: rows has {len(rows)} entries for {N} slots')
        return hip.recon_post_frame(img, weights, amount, self.bounds[:N], window=window, want_u8=want_u8, want_f32=want_f32, mode=mode)

    def __call__(self, img):
        """the reference's call: fp32 [n, 1, H, W] in [0, 1] -> float(uint8) / 255"""
        return self.rescale(img, want_u8=False, want_f32=True)[1]


class ImageFilter:
    """The reference's optional bilateral filter (:282-299).  Only bilateral_filter_sigma = 0, the default (the identity), is provided:
    the reference calls cv2.bilateralFilter on a 4-D float array after a round trip through the host, and without cv2 there is
    nothing to pin a restatement of it against."""

    def __init__(self, options):
        self.bilateral_filter_sigma = options.bilateral_filter_sigma
        if self.bilateral_filter_sigma:
            raise NotImplementedError('bilateral_filter_sigma > 0 is not provided: the reference hands a 4-D float array to '
                                      'cv2.bilateralFilter on the host, and there is no cv2 to pin a restatement against; '
                                      'bilateral_filter_sigma = 0 (the default) is the identity')

    def __call__(self, img):
        return img
