"""
The reference's utils/viz_utils.py on the device: the tiles of the trainers' validation panels (createRGBImage, visualizeHistogram,
visualizeVoxelGrid, prepare_semseg, create_checkerboard), torchvision's make_grid, and `panel`, which writes every tile straight into
its slot of the grid.  Same signatures, result shapes and values as the reference; what differs:

* every result is a DEVICE tensor, produced without a synchronisation: the reference's prepare_semseg goes through .cpu(),
  torch.unique and boolean-mask writes and returns a CPU tensor, and its separate_pol=False branch builds its tile on the CPU;
* prepare_semseg shows a label outside [0, K) that is not the ignore label as the checkerboard; the reference asserts on the host;
* make_grid is restated from torchvision's documented layout (torchvision is not a dependency; unpinned against it);
* plot_confusion_matrix and visualizeConfusionMatrix (matplotlib) are not provided.

The tiles come from three kernels (ess_amd/csrc/viz.hip) whose fp32 arithmetic is fixed; tests/viz_ref.py restates it in numpy.
"""
import torch

from .. import hip

PANEL_KINDS = ('gray', 'rgb', 'events', 'events_signed', 'histogram', 'semseg')


def _f32c(t):
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def visualizeHistogram(histogram):
    """[B, 2, H, W] -> [B, 3, H, W]: (clamp(h0, 0, 1), clamp(h1, 0, 1), 0)"""
    return hip.viz_events(_f32c(histogram), 'histogram')


def visualizeVoxelGrid(voxel_grid, separate_pol=True):
    """[B, C, H, W] -> [B, 3, H, W].  separate_pol: the two polarity halves, each weighted by (c + 1) / half and summed, as (neg, pos, 0)
    clamped to [0, 1]; otherwise 255 in plane 0 where the channel sum is positive and in plane 2 where it is negative."""
    return hip.viz_events(_f32c(voxel_grid), 'separate_pol' if separate_pol else 'signed')


def createRGBImage(tensor, separate_pol=True):
    """an rgb image of a batch: rgb as it is, grayscale expanded, an event histogram (2 channels) or a voxel grid (> 3 channels)"""
    if tensor.shape[1] == 3:
        return tensor
    elif tensor.shape[1] == 1:
        return tensor.expand(-1, 3, -1, -1)
    elif tensor.shape[1] == 2:
        return visualizeHistogram(tensor)
    elif tensor.shape[1] > 3:
        return visualizeVoxelGrid(tensor, separate_pol)


def visualizeTensors(tensor):
    return createRGBImage(tensor)


def create_checkerboard(N, C, H, W, device=None):
    """[N, C, H, W]: 0.75 / 0.25 cells of max(min(H, W) // 32, 1) pixels -- the tile of an all-ignore label map (device: cuda:0)"""
    dev = torch.device('cuda:0') if device is None else device
    lab = torch.full((1, H, W), 255, dtype=torch.uint8, device=dev)
    board = hip.viz_semseg(lab, torch.zeros(1, 3, device=dev), 255)
    return board[:, :1].repeat(N, C, 1, 1)


def _labels(img):
    if not torch.is_tensor(img) or not (img.dim() == 3 or img.dim() == 4 and img.shape[1] == 1) or \
            img.dtype not in (torch.uint8, torch.int32, torch.int64):
        raise hip.EssHipError(f'prepare_semseg: expecting an integer [N, H, W] or [N, 1, H, W] tensor of classes, got '
                              f'{tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}')
    if img.dim() == 4:
        img = img.squeeze(1)
    if img.dtype == torch.int32:
        img = img.long()
    return img if img.is_contiguous() else img.contiguous()


def prepare_semseg(img, semseg_color_map, semseg_ignore_label):
    """labels [N, H, W] or [N, 1, H, W] (uint8 / int / long, on the device) -> fp32 [N, 3, H, W] colours on the 0..1 scale, the ignore
    label as the checkerboard"""
    img = _labels(img)
    return hip.viz_semseg(img, hip.viz_colour_table(semseg_color_map, img.device), semseg_ignore_label)


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid's layout for a [n, C, H, W] batch (a list of images is stacked; 1-channel images are expanded to 3):
    xmaps = min(nrow, n) tiles per grid row, tile k at rows (k // xmaps) (H + padding) + padding and columns (k % xmaps) (W + padding)
    + padding of a [C, ymaps (H + padding) + padding, xmaps (W + padding) + padding] tensor filled with pad_value.  A single image is
    returned as it is, unpadded."""
    if isinstance(tensor, (list, tuple)):
        tensor = torch.stack(list(tensor), 0)
    if tensor.dim() == 2:
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 3:
        if tensor.shape[0] == 1:
            tensor = tensor.expand(3, -1, -1)
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 4 and tensor.shape[1] == 1:
        tensor = tensor.expand(-1, 3, -1, -1)
    n, C, H, W = tensor.shape
    if n == 1:
        return tensor.squeeze(0)
    xmaps, ymaps, Hg, Wg = hip.grid_geometry(n, H, W, nrow, padding)
    grid = tensor.new_full((C, Hg, Wg), pad_value)
    for y in range(ymaps):  # one strided copy per grid row
        k0, k1 = y * xmaps, min((y + 1) * xmaps, n)
        y0 = y * (H + padding) + padding
        dst = grid[:, y0:y0 + H, padding:].unfold(2, W, W + padding)  # [C, H, slots, W]
        dst[:, :, :k1 - k0].copy_(tensor[k0:k1].permute(1, 2, 0, 3))
    return grid


def createRGBGrid(tensor_list, nrow):
    return make_grid(torch.cat([visualizeTensors(t) for t in tensor_list], dim=0), nrow=nrow)


def _copy_tiles(grid, tiles, tile0, xmaps, padding):
    """`tiles` [n, 1 or 3, H, W] into slots tile0 .. of the grid: one strided copy_ per grid row the tiles touch"""
    n, _, H, W = tiles.shape
    k = 0
    while k < n:
        t = tile0 + k
        y, x = divmod(t, xmaps)
        m = min(xmaps - x, n - k)
        y0 = y * (H + padding) + padding
        dst = grid[:, y0:y0 + H, padding:].unfold(2, W, W + padding)[:, :, x:x + m]  # [3, H, m, W]
        dst.copy_(tiles[k:k + m].permute(1, 2, 0, 3).expand(3, -1, -1, -1))
        k += m


def panel(rows, nrow=4, color_map=None, ignore_label=255, padding=hip.GRID_PADDING):
    """A validation panel: rows = [(kind, tensor), ...] with kind one of PANEL_KINDS; each row contributes its first `nrow` samples;
    the result is what the trainers' torch.cat([createRGBImage(row[:nrow]) ...]) -> make_grid(nrow=nrow) builds -- fp32 [3, Hg, Wg] --
    without the tile tensors and the cat: one zero fill, then each row's tiles written by ONE launch into their grid slots ('gray' and
    'rgb' rows: strided copy_).  'events' is createRGBImage(separate_pol=True), 'events_signed' is createRGBImage(separate_pol=False)
    .clamp(0, 1) (2-channel tensors are histograms in both, as there); 'semseg' takes integer labels [n, H, W] and needs color_map."""
    if not rows:
        raise hip.EssHipError('panel: no rows')
    prepared = []
    for kind, t in rows:
        if kind not in PANEL_KINDS:
            raise hip.EssHipError(f'panel: kind must be one of {PANEL_KINDS}, got {kind!r}')
        if kind == 'semseg':
            if color_map is None:
                raise hip.EssHipError("panel: a 'semseg' row needs color_map")
            t = _labels(t)[:nrow]
            shape = (t.shape[1], t.shape[2])
        else:
            if not torch.is_tensor(t) or t.dim() != 4:
                raise hip.EssHipError(f'panel: a {kind!r} row must be a [n, C, H, W] tensor')
            t = t[:nrow]
            C = t.shape[1]
            if kind == 'histogram' or (kind in ('events', 'events_signed') and C == 2):
                kind = 'histogram'
            elif C == 1 or C == 3:
                kind = 'copy'
            elif kind in ('gray', 'rgb') or C < 4:
                raise hip.EssHipError(f'panel: a {kind!r} row with {C} channels')
            shape = (t.shape[2], t.shape[3])
        if t.shape[0] == 0:
            raise hip.EssHipError('panel: an empty row')
        prepared.append((kind, t, shape))
    H, W = prepared[0][2]
    if any(s != (H, W) for _, _, s in prepared):
        raise hip.EssHipError(f'panel: the rows differ in size: {[s for _, _, s in prepared]}')
    dev = prepared[0][1].device
    n = sum(t.shape[0] for _, t, _ in prepared)
    if n == 1:  # (make_grid hands a single image back unpadded)
        xmaps, Hg, Wg, padding = 1, H, W, 0
    else:
        xmaps, _, Hg, Wg = hip.grid_geometry(n, H, W, nrow, padding)
    grid = torch.zeros(3, Hg, Wg, dtype=torch.float32, device=dev)
    tile0 = 0
    for kind, t, _ in prepared:
        dst = (grid, tile0, xmaps, padding)
        if kind == 'semseg':
            hip.viz_semseg(t if t.is_contiguous() else t.contiguous(), hip.viz_colour_table(color_map, dev), ignore_label, dst=dst)
        elif kind == 'copy':
            _copy_tiles(grid, t.detach(), tile0, xmaps, padding)
        else:
            mode = {'histogram': 'histogram', 'events': 'separate_pol', 'events_signed': 'signed'}[kind]
            hip.viz_events(_f32c(t), mode, unit=True, dst=dst)
        tile0 += t.shape[0]
    return grid
