"""Numpy restatement of the paired-frame path (hip.image_ingest_frame, hip.image_gather_unit, ImageStore's resample / gray /
keep_rows keywords): PIL's two-pass 8-bit Image.resize with the bilinear or the BICUBIC filter on an 'L' or an 'RGB' image, the gray
conversion before or after it, the top-rows cut and ToTensor's / 255, written from PIL's documented algorithm one output index at a
time (plain Python floats are IEEE float64) and independently of the package's vectorised table builder.
tests/test_host_frame_store.py proves it equal to PIL itself, bit for bit; the GPU tier compares the kernels with it.  The keyword
switches are the MUTANTS those tests must catch: each one is a plausible misreading of the algorithm."""
import math

import numpy as np

PRECISION_BITS = 22
SUPPORT = {'bilinear': 1.0, 'bicubic': 2.0}


def bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def bicubic_filter(x):
    """PIL's bicubic: Keys' kernel with a = -0.5, support 2"""
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTER = {'bilinear': bilinear_filter, 'bicubic': bicubic_filter}


def fixed(w, round_away=True):
    """a normalised weight -> its 22-bit coefficient: rounded AWAY from zero (the mutant: trunc(0.5 + ...), wrong below zero)"""
    if w < 0 and round_away:
        return int(-0.5 + w * (1 << PRECISION_BITS))
    return int(0.5 + w * (1 << PRECISION_BITS))


def resize_table(n_in, n_out, resample='bicubic', round_away=True):
    """-> [(xmin, [k_0 .. k_{count - 1}])] per output index, and ksize"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[resample] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    rows = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w, ww = [], 0.0
        for i in range(xmax - xmin):
            v = FILTER[resample]((i + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((xmin, [fixed(v, round_away) for v in w]))
    return rows, ksize


def as_array(rows, ksize):
    """the rows of resize_table in the layout of pil_resize_tables: int32 [2 + ksize, n_out]"""
    out = np.zeros((2 + ksize, len(rows)), dtype=np.int32)
    for xx, (xmin, k) in enumerate(rows):
        out[0, xx], out[1, xx] = xmin, len(k)
        out[2:2 + len(k), xx] = k
    return out


def gray(rgb):
    """uint8 [H, W, 3] -> uint8 [H, W]: L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16"""
    v = rgb.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def _pass(img, n_out, axis, resample, round_away=True, clip_low=True, clip_high=True, float_out=False):
    """one pass along `axis` (every channel with the same coefficients); a pass that changes nothing is skipped, as PIL skips it.
    The sum's shift is arithmetic (numpy's >> on int64 floors, as C's does on the int PIL holds).  float_out: the mutant without
    the 8-bit intermediate -- the unrounded, unclipped value"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    rows, _ = resize_table(n_in, n_out, resample, round_away)
    src = np.moveaxis(img, axis, 0)
    src = src.astype(np.float64) if src.dtype.kind == 'f' else src.astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.float64 if float_out else np.uint8)
    for xx, (xmin, k) in enumerate(rows):
        ss = np.zeros(src.shape[1:], dtype=src.dtype)
        for i, ki in enumerate(k):
            ss = ss + ki * src[xmin + i]
        if float_out:
            out[xx] = ss / float(1 << PRECISION_BITS)
            continue
        v = np.floor((ss + (1 << (PRECISION_BITS - 1))) / float(1 << PRECISION_BITS)).astype(np.int64) if ss.dtype.kind == 'f' else \
            (ss + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS
        if clip_low:
            v = np.maximum(v, 0)
        if clip_high:
            v = np.minimum(v, 255)
        out[xx] = v.astype(np.uint8)  # (an unclipped value wraps, as a C cast to UINT8 does)
    return np.moveaxis(out, 0, axis)


def resize(img, out_hw, resample='bicubic', float_mid=False, **mutant):
    """uint8 [H, W] or [H, W, 3] -> the same kind at [Hr, Wr]: horizontal pass, 8-bit intermediate, vertical pass"""
    Hr, Wr = out_hw
    mid = _pass(img, Wr, 1, resample, float_out=float_mid and img.shape[0] != Hr, **mutant)
    return np.ascontiguousarray(_pass(mid, Hr, 0, resample, **mutant))


def frame(img, out_hw=None, resample='bicubic', gray_last=True, keep_rows=None, **mutant):
    """a camera frame uint8 [H, W, 3] or [H, W] -> the slot uint8 [keep_rows or Hr, Wr] of a frame store: Image.resize((Wr, Hr))
    then convert('L') (gray_last; the loaders' order), or convert('L') first (hip.image_ingest's order); out_hw=None: no resize"""
    out_hw = img.shape[:2] if out_hw is None else out_hw
    if img.ndim == 3 and not gray_last:
        img = gray(img)
    out = resize(img, out_hw, resample, **mutant)
    if out.ndim == 3:
        out = gray(out)
    return np.ascontiguousarray(out if keep_rows is None else out[:keep_rows])


def gather_unit(slots, index):
    """uint8 [capacity, Hs, Ws], B slot numbers -> fp32 [B, 1, Hs, Ws] = ToTensor()'s value / 255 in fp32 (one IEEE division); a
    number outside [0, capacity) gives an all-zero frame"""
    out = np.zeros((len(index), 1) + slots.shape[1:], dtype=np.float32)
    for b, i in enumerate(index):
        if 0 <= int(i) < slots.shape[0]:
            out[b, 0] = slots[int(i)].astype(np.float32) / np.float32(255.0)
    return out


def make_image(shape, seed):
    """random bytes with a saturated 0 / 255 checkerboard patch and solid 0 and 255 blocks with sharp edges: the bicubic filter
    overshoots on both sides there, so the clip and the rounding of negative coefficients show"""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, shape, dtype=np.uint8)
    H, W = shape[:2]
    yy, xx = np.mgrid[:H, :W]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    blocks = ((((yy // 3) + (xx // 4)) & 1) * 255).astype(np.uint8)
    if img.ndim == 3:
        board, blocks = board[..., None], blocks[..., None]
    h3, w2 = max(H // 3, 1), max(W // 2, 1)
    img[:h3, :w2] = board[:h3, :w2]
    img[h3:2 * h3, w2:] = blocks[h3:2 * h3, w2:]
    return img
