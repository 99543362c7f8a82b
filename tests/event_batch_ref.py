"""Shared by tests/test_hip_event_batches.py (GPU tier) and tests/test_host_event_batches.py (CPU tier): the reference loaders' lines
between a sample's voxel grids and the tensors a train step gets, restated in torch on the CPU.  A plain helper module: no fixtures,
no collection hooks.

    DSEC  (DSEC/dataset/sequence.py:281-295):  resize=True: the grid's top rows are kept, F.interpolate(size=(448, 640), mode=
          'bilinear', align_corners=True); the label is resized (nearest) to the same size; with p = 0.5 both are flipped along x.
    DDD17 (datasets/ddd17_events_loader.py:162-183): F.interpolate(size=(260, 352), mode='bilinear', align_corners=True), the top 200
          rows; the label resized (nearest) to 200 x 352; HorizontalFlip(p=0.5), then RandomCrop(120, 216) of the bottom 120 rows,
          the same for both.

The voxel grids and their normalisation are NOT restated here: they come from tests/loader_grid_ref.py (reference / restate), whose
bound the comparison holds.  The random draws are arguments: (flip, y0, x0) as ess_amd.datasets.event_batches.draw_window_params
gives them, y0 counted from the grid's top row."""
import torch
import torch.nn.functional as F


def window(t, flip, y0, x0, h, w):
    """t [..., H, W] -> the flip along x, then rows [y0, y0 + h) and columns [x0, x0 + w): index operations, exact in every dtype"""
    if flip:
        t = torch.flip(t, dims=[-1])
    return t[..., y0:y0 + h, x0:x0 + w]


def loader_lines(grid, rows, resize, height, flip, y0, x0, crop_hw):
    """one sample's voxel grids [C, Hs, Ws] (the T windows' bins stacked, normalised as the loader normalises them) -> what the
    loader hands the network [C, h, w], in grid's dtype: the top `rows` rows, the bilinear resize to `resize` (None: none), the top
    `height` rows, the flip, the crop"""
    g = grid[:, :rows]
    if resize is not None and tuple(resize) != tuple(g.shape[-2:]):
        g = F.interpolate(g[None], size=tuple(resize), mode='bilinear', align_corners=True)[0]
    return window(g[:, :height], flip, y0, x0, *crop_hw)


def label_lines(label, height, width, flip, y0, x0, crop_hw):
    """one sample's uint8 label [Hl, Wl] -> int64 [h, w]: nearest resize to height x width by the integer rule of hip.label_window
    (parity with cv2.resize(INTER_NEAREST) itself is unpinned), the same flip and crop; 255 stays 255"""
    Hl, Wl = label.shape
    sy = (torch.arange(height) * Hl // height).clamp(max=Hl - 1)
    sx = (torch.arange(width) * Wl // width).clamp(max=Wl - 1)
    return window(torch.as_tensor(label)[sy][:, sx].to(torch.int64), flip, y0, x0, *crop_hw)
