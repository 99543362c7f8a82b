"""The numpy float32 restatement of the segmentation display (ess_amd/csrc/viz.hip, ess_amd/utils/viz_utils.py): the three kernels, make_grid
and panel, plus the case tables of the CPU and the GPU tier.  Every function here DEFINES the bits the device must produce: fp32
operations, each rounded once, sums in ascending channel order from 0.  `mutate` names a deliberate mistake; the CPU tier uses it to show
that the cases would notice it."""
import numpy as np

F = np.float32
IGNORE = 255


def colour_table(color_map):
    """prepare_semseg's table: fp32 [K, 3], divided by 255 in fp32 if its maximum exceeds 128"""
    c = np.asarray(color_map, dtype=F)
    return c / F(255) if c.max() > 128 else c


def checkerboard(H, W, mutate=None):
    """create_checkerboard's plane [H, W]: cell = max(min(H, W) // 32, 1); 0.75 where (y // cell + x // cell) is even, else 0.25"""
    cell = max((max if mutate == 'cell_from_max' else min)(H, W) // 32, 1)
    y, x = np.arange(H)[:, None] // cell, np.arange(W)[None, :] // cell
    even = ((y + x) % 2 == 0) != (mutate == 'parity')
    return np.where(even, F(0.75), F(0.25)).astype(F)


def semseg(labels, colours, ignore=IGNORE, mutate=None):
    """labels integer [N, H, W], colours fp32 [K, 3] (0..1) -> fp32 [N, 3, H, W]; the ignore label and every label outside [0, K) show
    the checkerboard"""
    lab = np.asarray(labels).astype(np.int64)
    N, H, W = lab.shape
    K = colours.shape[0]
    board = (lab == ignore) | (lab < 0) | (lab >= K)
    out = colours[np.where(board, 0, lab)].transpose(0, 3, 1, 2).astype(F)
    cb = np.broadcast_to(checkerboard(H, W, mutate), (N, 3, H, W))
    return np.ascontiguousarray(np.where(board[:, None], cb, out), dtype=F)


def _clamp01(v):
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)


def polarity_sums(x, mutate=None):
    """-> (pos, neg) fp32 [N, H, W] before the clamp: sum over c < half of x[c] * ((c + 1) / half), ascending c from 0"""
    N, C, H, W = x.shape
    half = C // 2
    pos, neg = np.zeros((N, H, W), F), np.zeros((N, H, W), F)
    for c in range(half):
        t = F(c if mutate == 'scale_from_c' else c + 1) / F(half)
        pos = (pos + (x[:, c] * t).astype(F)).astype(F)
        neg = (neg + (x[:, half + c] * t).astype(F)).astype(F)
    return pos, neg


def events(x, mode, unit=False, mutate=None):
    """x fp32 [N, C, H, W] -> fp32 [N, 3, H, W]: 'histogram' | 'separate_pol' | 'signed'"""
    x = np.asarray(x, dtype=F)
    N, C, H, W = x.shape
    out = np.zeros((N, 3, H, W), F)
    if mode == 'histogram':
        assert C == 2
        out[:, 0], out[:, 1] = _clamp01(x[:, 0]), _clamp01(x[:, 1])
    elif mode == 'separate_pol':
        assert C >= 4 and C % 2 == 0
        pos, neg = polarity_sums(x, mutate)
        if mutate == 'swap_polarity':
            pos, neg = neg, pos
        out[:, 0], out[:, 1] = _clamp01(neg), _clamp01(pos)
    else:
        assert mode == 'signed' and C > 3
        s = np.zeros((N, H, W), F)
        for c in range(C):
            s = (s + x[:, c]).astype(F)
        hi = F(1 if unit else 255)
        out[:, 0] = np.where(s >= 0 if mutate == 'ge_zero' else s > 0, hi, F(0))
        out[:, 2] = np.where(s < 0, hi, F(0))
    return out


def overlay(labels, gray, palette, alpha, mutate=None):
    """labels, gray uint8 [N, H, W]; palette uint8 [K, 3] -> uint8 [N, H, W, 3]: v = (1 - alpha) g + alpha colour in fp32 (two products,
    one sum), (uint8) min(v + 0.5, 255); a label >= K shows g"""
    labels, gray, palette = np.asarray(labels), np.asarray(gray), np.asarray(palette)
    K = palette.shape[0]
    a = F(alpha)
    b = F(1) - a
    g = gray.astype(F)[..., None]
    col = palette[np.where(labels >= K, 0, labels)].astype(F)
    v = ((b * g).astype(F) + (a * col).astype(F)).astype(F)
    if mutate != 'truncate':
        v = (v + F(0.5)).astype(F)
    q = np.minimum(v, F(255)).astype(np.uint8)
    return np.where((labels >= K)[..., None], np.broadcast_to(gray[..., None], q.shape), q).astype(np.uint8)


def grid_slot(k, xmaps, H, W, padding=2):
    """tile k's top-left corner in a make_grid panel"""
    return (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding


def make_grid(t, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid's documented layout for a [n, 3, H, W] array (a single image is returned unpadded)"""
    t = np.asarray(t, dtype=F)
    n, C, H, W = t.shape
    if n == 1:
        return t[0].copy()
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    out = np.full((C, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), pad_value, F)
    for k in range(n):
        y, x = grid_slot(k, xmaps, H, W, padding)
        out[:, y:y + H, x:x + W] = t[k]
    return out


def tiles(kind, a, colours=None, ignore=IGNORE):
    """one panel row's tiles [n, 3, H, W] (createRGBImage's dispatch on the channel count)"""
    a = np.asarray(a)
    if kind == 'semseg':
        return semseg(a, colours, ignore)
    a = a.astype(F)
    C = a.shape[1]
    if kind == 'histogram' or (kind in ('events', 'events_signed') and C == 2):
        return events(a, 'histogram')
    if kind == 'gray' or (kind != 'rgb' and C == 1):
        assert C == 1
        return np.broadcast_to(a, (a.shape[0], 3) + a.shape[2:]).copy()
    if kind == 'rgb' or C == 3:
        assert C == 3
        return a
    if kind == 'events':
        return events(a, 'separate_pol')
    assert kind == 'events_signed'
    return events(a, 'signed', unit=True)


def panel(rows, nrow=4, colours=None, ignore=IGNORE):
    """the trainers' torch.cat([tiles of each row's first nrow samples]) -> make_grid(nrow=nrow)"""
    return make_grid(np.concatenate([tiles(kind, np.asarray(a)[:nrow], colours, ignore) for kind, a in rows], 0), nrow=nrow)


# ---------------------------------------------------------------------------------------------- case tables
def palette_u8(K, seed=0):
    g = np.random.default_rng(100 + K + seed)
    return g.integers(0, 256, (K, 3)).astype(np.uint8)


def labels_case(N, H, W, K, seed, dtype=np.uint8):
    """labels in [0, K) with the ignore label, K (out of range) and K - 1 present"""
    g = np.random.default_rng(seed)
    lab = g.integers(0, K, (N, H, W)).astype(dtype)
    lab[g.random((N, H, W)) < 0.2] = IGNORE
    flat = lab.reshape(-1)
    flat[0], flat[1], flat[-1] = IGNORE, K, K - 1
    flat[flat.size // 2] = K
    return lab


def gray_case(N, H, W, seed):
    g = np.random.default_rng(seed)
    f = g.integers(0, 256, (N, H, W)).astype(np.uint8)
    f.reshape(-1)[:4] = (0, 255, 254, 1)
    return f


def event_case(N, C, H, W, seed, integer=False):
    """a sparse signed grid; integer: whole values (every sum of the separate_pol / signed tiles is exact for half a power of two)"""
    g = np.random.default_rng(seed)
    if integer:
        x = g.integers(-3, 4, (N, C, H, W)).astype(F)
    else:
        x = (g.standard_normal((N, C, H, W)) * 0.8).astype(F)
    x[g.random((N, C, H, W)) < 0.4] = 0
    return x


def signed_case(N, C, H, W, seed):
    """event_case plus pixels whose channels cancel to exactly 0, pixels that are all -0.0 and one of each sign"""
    x = event_case(N, C, H, W, seed)
    x[:, :, 0, 0] = 0
    x[:, 0, 0, 0], x[:, 1, 0, 0] = 1.5, -1.5  # cancels to +0.0
    x[:, :, 0, 1] = -0.0
    x[:, :, 0, 2] = 0
    x[:, 2, 0, 2] = 0.25
    x[:, :, 0, 3] = 0
    x[:, 3, 0, 3] = -0.25
    return x


def histogram_case(N, H, W, seed):
    g = np.random.default_rng(seed)
    x = (g.integers(0, 5, (N, 2, H, W)) * g.choice([0.25, 0.5, 1.0], (N, 2, H, W))).astype(F)
    x.reshape(-1)[:3] = (-0.5, 1.0, 0.75)
    return x


SIZES = ((5, 7), (33, 70), (64, 96), (97, 65))   # cell 1, 1, 2, 2 (ragged last cell, odd width, one past a 4-pixel group)
NK = ((1, 6), (3, 11), (5, 19))
ALPHAS = (0.0, 0.5, 0.6, 1.0)
POL_CHANNELS = (4, 6, 10)


def trainer_layouts(B, H=16, W=24, K=6, C=4, seed=7):
    """the four validation layouts of the two trainers -> {name: rows}; sensor a: an image; sensor b: events"""
    g = np.random.default_rng(seed + B)
    img = g.random((B, 1, H, W)).astype(F)
    fake = g.random((B, 1, H, W)).astype(F)
    ev = event_case(B, C, H, W, seed + 1)
    pred, cyc, gt = (labels_case(B, H, W, K, seed + 2 + i, np.int64) for i in range(3))
    return {
        'ess_sensor_a': [('gray', img), ('semseg', pred), ('semseg', gt)],
        'ess_sensor_b': [('events', ev), ('gray', fake), ('semseg', pred), ('semseg', cyc), ('semseg', gt)],
        'ess_sensor_b_signed_no_gt': [('events_signed', ev), ('gray', fake), ('semseg', pred), ('semseg', cyc)],
        'sup_sensor_b': [('events', ev), ('semseg', pred), ('semseg', gt), ('gray', fake)],
    }
