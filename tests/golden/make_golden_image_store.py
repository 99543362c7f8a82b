"""Writes tests/golden/image_store.npz: seeded uint8 inputs and what PIL ITSELF makes of them -- convert('L'), Image.resize(BILINEAR)
on mode L, Image.resize(NEAREST) -- at the size pairs of tests/test_host_image_store.py, so that a machine without PIL can still
compare with PIL's bits.  Imports PIL and numpy only.  Run from the repository root: python tests/golden/make_golden_image_store.py"""
import os

import numpy as np
from PIL import Image

import PIL

PAIRS = [((37, 53), (16, 24)), ((37, 53), (37, 24)), ((20, 30), (33, 47)), ((64, 64), (63, 65)), ((9, 7), (1, 1)), ((64, 128), (16, 32)),
         ((128, 256), (25, 44))]
BILINEAR = getattr(Image, 'Resampling', Image).BILINEAR
NEAREST = getattr(Image, 'Resampling', Image).NEAREST


def main():
    g = np.random.default_rng(20240611)
    out = {'pairs': np.array([[h, w, hr, wr] for (h, w), (hr, wr) in PAIRS], dtype=np.int32), 'pil_version': np.array(PIL.__version__)}
    for i, ((H, W), (Hr, Wr)) in enumerate(PAIRS):
        rgb = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rgb[: H // 3, : W // 3] = 255  # (a saturated corner: the clip at 255 is exercised by real data too)
        lab = g.integers(0, 34, (H, W), dtype=np.uint8)
        L = Image.fromarray(rgb).convert('L')
        out[f'rgb_{i}'], out[f'gray_{i}'] = rgb, np.array(L)
        out[f'bil_{i}'] = np.array(L.resize((Wr, Hr), BILINEAR))
        out[f'lab_{i}'] = lab
        out[f'near_{i}'] = np.array(Image.fromarray(lab).resize((Wr, Hr), NEAREST))
    # all-0, all-255 and a checkerboard at the first pair (the sum of a window's coefficients is not exactly 2^22: the clip matters)
    (H, W), (Hr, Wr) = PAIRS[0]
    yy, xx = np.mgrid[:H, :W]
    special = np.stack([np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8)])
    out['special_in'] = special
    out['special_out'] = np.stack([np.array(Image.fromarray(s).resize((Wr, Hr), BILINEAR)) for s in special])
    # the nearest rule's indices at a ratio float64 does not represent: a one-row int32 image of its own column numbers
    cols = Image.fromarray(np.arange(2048, dtype=np.int32)[None, :])
    out['nearest_2048_352'] = np.array(cols.resize((352, 1), NEAREST))[0].astype(np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'image_store.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
