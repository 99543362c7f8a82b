"""Numpy restatement of the image ingest (hip.image_ingest, ess_amd/datasets/image_store.py): PIL's convert('L'), its two-pass
Image.resize(BILINEAR) on an 8-bit image, Image.resize(NEAREST) and the Cityscapes loader's standardization stretch, written from
PIL's documented algorithm one output index at a time (plain Python floats are IEEE float64) and independently of the package's
vectorised table builders.  tests/test_host_image_store.py proves it equal to PIL itself, bit for bit; the GPU tier compares the
kernels with it.  The keyword switches are the MUTANTS that tier must catch: each one is a plausible misreading of the algorithm."""
import math

import numpy as np

PRECISION_BITS = 22


def gray(rgb, rounding=True):
    """uint8 [H, W, 3] -> uint8 [H, W]: L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16"""
    v = rgb.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + (0x8000 if rounding else 0)) >> 16).astype(np.uint8)


def bilinear_table(n_in, n_out, half_pixel=True):
    """-> [(xmin, [k_0 .. k_{count - 1}])] per output index, and ksize"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    rows = []
    for xx in range(n_out):
        center = (xx + (0.5 if half_pixel else 0.0)) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w, ww = [], 0.0
        for i in range(xmax - xmin):
            v = max(0.0, 1.0 - abs((i + xmin - center + 0.5) / fs))
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((xmin, [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return rows, ksize


def as_array(rows, ksize):
    """the rows of bilinear_table in the layout of pil_bilinear_tables: int32 [2 + ksize, n_out]"""
    out = np.zeros((2 + ksize, len(rows)), dtype=np.int32)
    for xx, (xmin, k) in enumerate(rows):
        out[0, xx], out[1, xx] = xmin, len(k)
        out[2:2 + len(k), xx] = k
    return out


def _pass(img, n_out, axis, rounding=True, half_pixel=True):
    """one pass along `axis` with an 8-bit result; a pass that changes nothing is skipped, as PIL skips it"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    rows, _ = bilinear_table(n_in, n_out, half_pixel)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for xx, (xmin, k) in enumerate(rows):
        ss = np.full(src.shape[1:], (1 << (PRECISION_BITS - 1)) if rounding else 0, dtype=np.int64)
        for i, ki in enumerate(k):
            ss += ki * src[xmin + i]
        out[xx] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(img, out_hw, rounding=True, horizontal_first=True, half_pixel=True):
    """uint8 [H, W] -> uint8 [Hr, Wr]: horizontal pass, 8-bit intermediate, vertical pass"""
    Hr, Wr = out_hw
    order = ((1, Wr), (0, Hr)) if horizontal_first else ((0, Hr), (1, Wr))
    for axis, n in order:
        img = _pass(img, n, axis, rounding, half_pixel)
    return np.ascontiguousarray(img)


def nearest_table(n_in, n_out, running_sum=True):
    step = n_in / n_out
    out, xo = [], 0.5 * step
    for x in range(n_out):
        v = xo if running_sum else (x + 0.5) * step
        out.append(min(int(v), n_in - 1))
        xo += step
    return np.array(out, dtype=np.int32)


def resize_nearest(lab, out_hw):
    Hr, Wr = out_hw
    return np.ascontiguousarray(lab[nearest_table(lab.shape[0], Hr)][:, nearest_table(lab.shape[1], Wr)])


def stretch(img):
    """cityscapes_loader.py:92-96 on a uint8 frame; a constant frame (the reference divides by zero) -> all 0"""
    mn, mx = int(img.min()), int(img.max())
    if mx == mn:
        return np.zeros_like(img)
    return (255.0 * (img.astype(np.int64) - mn).astype(np.float64) / float(mx - mn)).astype(np.uint8)


def ingest(frame, out_hw, standardization=False, **mutant):
    """frame uint8 [H, W, 3] or [H, W] -> (slot uint8 [Hr, Wr], (min, max) before the stretch)"""
    g = gray(frame, mutant.pop('gray_rounding', True)) if frame.ndim == 3 else frame
    r = resize_bilinear(g, out_hw, **mutant)
    mm = (int(r.min()), int(r.max()))
    return (stretch(r) if standardization else r), mm
