"""
Generate tests/golden/viz.npz by IMPORTING THE REFERENCE (read-only) on CPU, as make_golden_representations.py does: the outputs of
utils/viz_utils.py's visualizeHistogram, visualizeVoxelGrid (both branches), create_checkerboard and prepare_semseg on the CPU-tier
cases of tests/viz_ref.py, with their inputs.  Data only.  Run:   python tests/golden/make_golden_viz.py <path of the reference>

The reference module imports cv2, matplotlib and torchvision at its top without using them in these five functions: they are stubbed.
For the separate-polarity tile the sums BEFORE the clamp are recorded as well (the same torch.sum over the scaled halves the reference
calls), for the bounded comparison where torch's summation order is not the sequential one.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import viz_ref as V  # noqa: E402


def _reference(path):
    for name in ('cv2', 'torchvision', 'torchvision.utils', 'matplotlib', 'matplotlib.pyplot'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['torchvision'].utils = sys.modules['torchvision.utils']
    plt = sys.modules['matplotlib.pyplot']
    if not hasattr(plt, 'cm'):
        plt.cm = types.SimpleNamespace(Blues=None)
    sys.modules['matplotlib'].pyplot = plt
    spec = importlib.util.spec_from_file_location('ref_viz_utils', os.path.join(path, 'utils/viz_utils.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


SEMSEG = [  # (N, H, W, K, seed, colour map on the 0..255 scale?)
    (1, 5, 7, 6, 11, True), (1, 33, 70, 11, 12, True), (1, 64, 96, 19, 13, True), (2, 5, 7, 11, 14, False)]
BOARDS = [(1, 3, 5, 7), (2, 1, 33, 70), (1, 3, 64, 96), (1, 3, 97, 65)]
HISTOGRAMS = [(2, 5, 7, 21), (1, 33, 70, 22)]
VOXEL_EXACT = [(2, 4, 5, 7, 31), (1, 8, 16, 24, 32), (1, 16, 9, 13, 33)]   # integer grids, half a power of two
VOXEL_ROUNDED = [(2, 6, 8, 12, 41), (1, 10, 8, 12, 42)]                     # half = 3, 5: random values
SIGNED = [(2, 5, 5, 7, 51), (1, 8, 16, 24, 52)]                             # integer grids


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    R = _reference(sys.argv[1])
    out = {}
    for i, (N, H, W, K, seed, scale255) in enumerate(SEMSEG):
        lab = V.labels_case(N, H, W, K, seed, np.int64)
        lab[lab == K] = V.IGNORE  # (the reference asserts on a label outside [0, K))
        cmap = V.palette_u8(K).astype(np.float32) if scale255 else (V.palette_u8(K).astype(np.float32) / np.float32(512))
        got = R.prepare_semseg(torch.from_numpy(lab), cmap.tolist(), V.IGNORE)
        out[f'semseg{i}_labels'], out[f'semseg{i}_cmap'], out[f'semseg{i}_out'] = lab, cmap, got.numpy()
    for i, (N, C, H, W) in enumerate(BOARDS):
        out[f'board{i}_shape'], out[f'board{i}_out'] = np.array([N, C, H, W]), R.create_checkerboard(N, C, H, W).numpy()
    for i, (N, H, W, seed) in enumerate(HISTOGRAMS):
        x = V.histogram_case(N, H, W, seed)
        out[f'hist{i}_in'], out[f'hist{i}_out'] = x, R.visualizeHistogram(torch.from_numpy(x)).numpy()
    for tag, table, integer in (('exact', VOXEL_EXACT, True), ('rounded', VOXEL_ROUNDED, False)):
        for i, (N, C, H, W, seed) in enumerate(table):
            x = V.event_case(N, C, H, W, seed, integer=integer)
            t = torch.from_numpy(x)
            half = C // 2
            scale = torch.arange(1, half + 1, dtype=t.dtype)[None, :, None, None] / half
            out[f'pol_{tag}{i}_in'] = x
            out[f'pol_{tag}{i}_out'] = R.visualizeVoxelGrid(t, True).numpy()
            out[f'pol_{tag}{i}_pos'] = torch.sum(t[:, :half] * scale, dim=1).numpy()
            out[f'pol_{tag}{i}_neg'] = torch.sum(t[:, half:] * scale, dim=1).numpy()
    for i, (N, C, H, W, seed) in enumerate(SIGNED):
        x = V.event_case(N, C, H, W, seed, integer=True)
        out[f'signed{i}_in'], out[f'signed{i}_out'] = x, R.visualizeVoxelGrid(torch.from_numpy(x), False).numpy()
    path = os.path.join(HERE, 'viz.npz')
    np.savez_compressed(path, **out)
    print(f'viz: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB')


if __name__ == '__main__':
    main()
