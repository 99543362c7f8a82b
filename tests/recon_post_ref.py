"""The reconstruction post-processing kernels (ess_amd/csrc/recon_post.hip) restated in numpy, operation for operation in float32, so
that the GPU tier can compare BITS: the 5 x 5 unsharp mask in row-major tap order from 0.f, s = c1 v - a blur, q = (255 (s - Imin)) /
range clamped and truncated; the auto-HDR history of filter_size + 1 entries with np.median in float64; the event preview.  Every
numpy operation on float32 arrays rounds once, which is what the kernels' uncontracted arithmetic does.

Also here: the same formulas in float64 (`pre_truncation_f64`, what both float32 evaluations approximate), the bound `delta` on how far
a float32 evaluation can be from it in grey levels, the mutants the CPU tier uses to show that the comparison can fail, and the cases
both tiers run (the CPU tier checks the restatement on them against torch, the GPU tier checks the kernels against the restatement)."""
from math import erf, erfc, sqrt

import numpy as np

F32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32
PARTIALS = 256
MAX_FILTER = 63


# ---------------------------------------------------------------------------------------------- the Gaussian
def norm_cdf(x):
    t = x * sqrt(0.5)
    z = abs(t)
    if z < sqrt(0.5):
        return 0.5 + 0.5 * erf(t)
    y = 0.5 * erfc(z)
    return 1.0 - y if t > 0 else y


def gkern(kernlen=5, nsig=1.0):
    """float32 [kernlen, kernlen]: sqrt of the outer product of the differences of the normal CDF on kernlen + 1 points, normalised"""
    interval = (2 * nsig + 1.) / kernlen
    x = np.linspace(-nsig - interval / 2., nsig + interval / 2., kernlen + 1)
    k1 = np.diff(np.array([norm_cdf(float(v)) for v in x]))
    raw = np.sqrt(np.outer(k1, k1))
    return (raw / raw.sum()).astype(F32)


# ---------------------------------------------------------------------------------------------- the frame
def scalars(amount):
    """(c1, a) as the wrapper hands them to the kernel: (1 + amount) and amount, each rounded from double once"""
    return F32(1 + float(amount)), F32(float(amount))


def sharpen(img, w, amount, drop_tap=None, edge='zero'):
    """img float32 [N, 1, Hs, Ws] -> s float32 [N, Hs, Ws].  Mutants: drop_tap=(ky, kx) leaves one tap out; edge='clamp' repeats the
    border pixel where the kernel pads with zeros."""
    v = np.ascontiguousarray(img[:, 0], dtype=F32)
    if not amount > 0:
        return v.copy()
    c1, a = scalars(amount)
    N, Hs, Ws = v.shape
    pad = np.pad(v, ((0, 0), (2, 2), (2, 2)), mode='constant' if edge == 'zero' else 'edge')
    blur = np.zeros_like(v)
    for ky in range(5):
        for kx in range(5):
            if drop_tap == (ky, kx):
                continue
            blur = blur + F32(w[ky, kx]) * pad[:, ky:ky + Hs, kx:kx + Ws]
    return c1 * v - a * blur


def quantise(s, bounds, rounding='trunc'):
    """s float32 [N, H, W], bounds float32 [N, 2] = (Imin, range) -> uint8.  Mutant: rounding='round'."""
    b = np.asarray(bounds, dtype=F32)
    q = (F32(255) * (s - b[:, 0, None, None])) / b[:, 1, None, None]
    q = np.fmin(np.fmax(q, F32(0)), F32(255))  # (a NaN becomes 0, as fmaxf does it)
    if rounding == 'round':
        q = np.rint(q)
    return q.astype(np.uint8)


def frame(img, w, amount, bounds, window=None, **mutant):
    """-> (uint8 [N, H, W], float32 [N, 1, H, W] = float(u8) / 255): the stencil over the whole source, the window cut afterwards"""
    s = sharpen(img, w, amount, **{k: v for k, v in mutant.items() if k in ('drop_tap', 'edge')})
    y0, x0, H, W = (0, 0, s.shape[1], s.shape[2]) if window is None else window
    u8 = quantise(s[:, y0:y0 + H, x0:x0 + W], bounds, **{k: v for k, v in mutant.items() if k == 'rounding'})
    return u8, (u8.astype(F32) / F32(255))[:, None]


def pre_truncation_f64(img, w, amount, bounds, window=None):
    """The value in front of clamp and truncation in float64, from the SAME float32 inputs (image, weights, c1, a, Imin, range): what
    any float32 evaluation of the formulas approximates."""
    v = img[:, 0].astype(np.float64)
    s = v
    if amount > 0:
        c1, a = scalars(amount)
        N, Hs, Ws = v.shape
        pad = np.pad(v, ((0, 0), (2, 2), (2, 2)))
        blur = sum(float(w[ky, kx]) * pad[:, ky:ky + Hs, kx:kx + Ws] for ky in range(5) for kx in range(5))
        s = float(c1) * v - float(a) * blur
    b = np.asarray(bounds, dtype=F32).astype(np.float64)
    q = 255.0 * (s - b[:, 0, None, None]) / b[:, 1, None, None]
    y0, x0, H, W = (0, 0, q.shape[1], q.shape[2]) if window is None else window
    return q[:, y0:y0 + H, x0:x0 + W]


def sharpen_error(img, w, amount):
    """Bound on |s_float32 - s_exact| for ANY order of the 25 products and sums, fused or not: the longest chain behind s has 27
    roundings (one product, 24 sums -- the first addend meets an exact 0 --, the product with a, the final difference; c1 v runs
    beside it), each relative to a partial result no larger than M = c1 max|v| + a sum|w| max|v|:  27 U M  (first order in U)."""
    if not amount > 0:
        return 0.0
    c1, a = scalars(amount)
    m = float(np.abs(img).max())
    return 27 * U * (float(c1) * m + float(a) * float(np.abs(w).astype(np.float64).sum()) * m)


def delta(img, w, amount, bounds):
    """Per sample: how many grey levels a float32 evaluation of q can lie from pre_truncation_f64 where it matters (0 <= q <= 255):
    the error of s scaled by 255 / range, plus the three roundings of (s - Imin), 255 *, / range, each relative to |q| <= 256.  Two
    evaluations can therefore truncate differently only where the float64 value lies within delta of a whole number, and then by
    one level.  (At the auto-HDR floor range = 0.1, amount 0.3 and |v| <= 1: 27 U 1.6 2550 = 6.6e-3 levels.)"""
    b = np.asarray(bounds, dtype=F32).astype(np.float64)
    return 255.0 / b[:, 1] * sharpen_error(img, w, amount) + 3 * U * 256.0


# ---------------------------------------------------------------------------------------------- auto-HDR
class History:
    """The bounds kernel's state for N samples: per sample the held (Imin, Imax) pairs, oldest first.  Mutants: ring_extra=0 holds
    filter_size entries instead of filter_size + 1; stat='mean'; bounds_from='raw' takes min / max of the unsharpened image."""

    def __init__(self, n, filter_size, ring_extra=1, stat='median', bounds_from='sharp'):
        self.n, self.size, self.extra, self.stat, self.bounds_from = n, filter_size, ring_extra, stat, bounds_from
        self.held = [[] for _ in range(n)]

    def reset(self, samples=None):
        for i in (range(self.n) if samples is None else samples):
            self.held[i] = []

    def update(self, img, w, amount):
        """-> bounds float32 [N, 2] after pushing this frame's clipped min / max"""
        s = sharpen(img, w, amount if self.bounds_from == 'sharp' else 0.0)
        out = np.zeros((self.n, 2), dtype=F32)
        for i in range(self.n):
            flat = s[i].ravel()
            mn = np.fmin.reduce(flat, initial=F32(np.inf))  # (NaN pixels are skipped)
            mx = np.fmax.reduce(flat, initial=F32(-np.inf))
            lo = float(np.clip(np.float64(mn), 0.0, 0.45))
            hi = float(np.clip(np.float64(mx), 0.55, 1.0))
            h = self.held[i]
            if len(h) > self.size - (1 - self.extra):  # the reference pops only when the history is LONGER than the filter size
                h.pop(0)
            h.append((lo, hi))
            f = np.median if self.stat == 'median' else np.mean
            imin = float(f(np.array([p[0] for p in h], dtype=np.float64)))
            imax = float(f(np.array([p[1] for p in h], dtype=np.float64)))
            out[i] = (F32(imin), F32(imax - imin))
        return out


# ---------------------------------------------------------------------------------------------- the event preview
def first_bin(C, num_bins_to_show):
    return 0 if num_bins_to_show <= 0 or num_bins_to_show >= C else C - num_bins_to_show


def event_preview(grids, mode, num_bins_to_show=-1):
    """grids float32 [N, C, H, W] -> uint8 [N, H, W, 3] (BGR) or [N, H, W]; the planes are summed in plane order, in float32"""
    g = np.asarray(grids, dtype=F32)
    N, C, H, W = g.shape
    s = np.zeros((N, H, W), dtype=F32)
    for c in range(first_bin(C, num_bins_to_show), C):
        s = s + g[:, c]
    if mode == 'red-blue':
        out = np.zeros((N, H, W, 3), dtype=np.uint8)
        out[..., 0][s > 0] = 255
        out[..., 2][s < 0] = 255
        return out
    q = (F32(255) * (s + F32(10))) / F32(20)
    return np.fmin(np.fmax(q, F32(0)), F32(255)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the cases of both tiers
FRAME_SIZES = [(1, 1), (2, 3), (5, 7), (16, 64), (17, 68), (33, 70)]
BOUNDS = [(0.0, 1.0), (0.12, 0.83)]


def bounds_rows(pairs):
    """(Imin, Imax) pairs -> float32 [N, 2] = (Imin, Imax - Imin), the difference in double"""
    return np.array([[F32(lo), F32(hi - lo)] for lo, hi in pairs], dtype=F32)


def image(n, hs, ws, seed, lo=-0.05, hi=1.05):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 1, hs, ws)).astype(F32)


def frame_cases():
    """name -> dict(img, sigma, amount, bounds [N, 2], window): every source size x N in (1, 3) x amount in (0, 0.3) x sigma in
    (1.0, 0.5) x the two bounds (N = 3: a different pair per sample), plus the windowed 24 x 40 source"""
    cases = {}
    for (hs, ws) in FRAME_SIZES + [(24, 40)]:
        window = (2, 3, 19, 34) if (hs, ws) == (24, 40) else None
        for n in (1, 3):
            for amount in (0.0, 0.3):
                for sigma in ((1.0, 0.5) if amount > 0 else (1.0,)):
                    for bi, b in enumerate(BOUNDS):
                        pairs = [b] if n == 1 else [BOUNDS[bi], BOUNDS[1 - bi], (0.3, 0.4)]
                        name = f'{hs}x{ws}-n{n}-a{amount}-s{sigma}-b{bi}'
                        cases[name] = dict(img=image(n, hs, ws, len(cases) + 1), sigma=sigma, amount=amount, bounds=bounds_rows(pairs),
                                           window=window)
    return cases


HDR_SHAPE = (3, 33, 70)
HDR_CALLS = 7
HDR_FILTER_SIZES = (0, 3, 10)


def hdr_images():
    """Seven frames of three samples: sample 0 stays inside every clip limit with a range that moves from call to call; sample 1 is
    nearly flat just above 0.45 (its minimum clips to 0.45; its maximum, the zero-padded border that
    the mask brightens by up to 19 %, stays under 0.55 and clips to it); sample 2 overshoots [0, 1] on both sides (0 and 1 bind,
    the sharpened minimum is negative) except in calls 2 and 5."""
    n, hs, ws = HDR_SHAPE
    g = np.random.default_rng(77)
    out = []
    for t in range(HDR_CALLS):
        img = np.empty((n, 1, hs, ws), dtype=F32)
        img[0, 0] = g.uniform(0.10 + 0.04 * ((t * 3) % 7), 0.95 - 0.05 * ((t * 5) % 7), (hs, ws))
        img[1, 0] = g.uniform(0.455, 0.46, (hs, ws))
        img[2, 0] = g.uniform(0.2, 0.8, (hs, ws)) if t in (2, 5) else g.uniform(-0.2 - 0.01 * t, 1.3, (hs, ws))
        out.append(img)
    return out


PREVIEW_SIZES = [(1, 5, 7), (1, 33, 70), (2, 16, 64)]  # (N, H, W); the last one takes the 4-pixels-per-lane path


def preview_grids(n, h, w, C=5):
    """eighths in [-3, 3] with many zeros (sums are exact in any order), every seventh pixel scaled by 12 (the grey ramp saturates)"""
    g = np.random.default_rng(h * 100 + w)
    x = g.integers(-24, 25, (n, C, h, w)).astype(F32) / F32(8)
    x[g.random((n, C, h, w)) < 0.4] = 0
    flat = x.reshape(n, C, -1)
    flat[:, :, ::7] *= F32(12)
    return x
