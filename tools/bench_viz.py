#!/usr/bin/env python
"""Cost of the segmentation display: (a) the three kernels of csrc/viz.hip at N x 480 x 640, N = 1 and 8, against the reference's own
lines composed from torch operations on the same device; (b) a StreamingSegmenter window with reconstruct + postprocess + overlay
('mixed' and 'bf16', eager and replayed) against the way to the same outputs without it -- a StreamingSegmenter window plus a
StreamingReconstructor(postprocess=True) window on the same grid plus a torch blend -- and against the plain segmenter window; (c) one
validation panel of five rows at the DSEC size through viz_utils.panel against the reference's composition (tiles, cat, grid copy).
Every variant is timed twice, the variants alternating (run 1 of all, then run 2 of all); both figures are printed.  Host clock around
work that ends in a device synchronise.
usage: python tools/bench_viz.py [--height 480 --width 640 --iters 2000 --windows 100]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / iters * 1e6, 2)  # microseconds per call


# ---- the reference's lines on the device (utils/viz_utils.py), kept as they are but for the .cpu() round trips it cannot avoid
def torch_checkerboard(N, C, H, W, dev):
    cell = max(min(H, W) // 32, 1)
    mH, mW = (H + cell - 1) // cell, (W + cell - 1) // cell
    cb = torch.full((mH, mW), 0.25, dtype=torch.float32, device=dev)
    cb[0::2, 0::2] = 0.75
    cb[1::2, 1::2] = 0.75
    cb = torch.nn.functional.interpolate(cb.view(1, 1, mH, mW), scale_factor=cell, mode='nearest')
    return cb[:, :, :H, :W].repeat(N, C, 1, 1)


def torch_prepare_semseg(img, colors, ignore):
    img = img.clone()
    N, H, W = img.shape
    ids = torch.unique(img)  # (a synchronisation, as in the reference)
    has = bool((ids == ignore).any())
    if has:
        board = torch_checkerboard(N, 3, H, W, img.device)
        mask = img == ignore
        img[mask] = 0
    out = colors[img].permute(0, 3, 1, 2)
    if has:
        mask = mask.unsqueeze(1).repeat(1, 3, 1, 1)
        out[mask] = board[mask]
    return out


def torch_voxel(x):
    half = x.shape[1] // 2
    t = torch.arange(1, half + 1, dtype=x.dtype, device=x.device)[None, :, None, None] / half
    pos, neg = torch.sum(x[:, :half] * t, 1, keepdim=True), torch.sum(x[:, half:] * t, 1, keepdim=True)
    return torch.cat([neg.clamp(0, 1), pos.clamp(0, 1), torch.zeros_like(pos)], 1)


def torch_overlay(labels, gray, palette, alpha):
    """the blend a caller would write; a label outside the palette (the ignore label) must not index it: it shows the gray value"""
    inside = (labels < palette.shape[0]).unsqueeze(-1)
    g = gray.float().unsqueeze(-1)
    col = palette[torch.where(inside[..., 0], labels, torch.zeros_like(labels)).long()].float()
    v = torch.where(inside, (1 - alpha) * g + alpha * col, g.expand(-1, -1, -1, 3))
    return (v + 0.5).clamp_(max=255).to(torch.uint8)


def torch_make_grid(t, nrow, padding=2):
    n, C, H, W = t.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = t.new_zeros((C, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding))
    for k in range(n):  # (torchvision's loop: one narrow().copy_() per tile)
        y, x = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        grid[:, y:y + H, x:x + W].copy_(t[k])
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--windows', type=int, default=100)
    ap.add_argument('--skip-stream', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_viz needs the GPU: there is nothing to time without one')
    from ess_amd import hip
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.run_reconstruction import StreamingReconstructor
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.run_segmentation import StreamingSegmenter
    from ess_amd.utils import viz_utils
    dev = torch.device('cuda:0')
    H, W, K = a.height, a.width, 11
    out = {'shape': f'{H}x{W}', 'iters': a.iters, 'unit': 'us per call (all N samples)', 'runs': 2}
    g = torch.Generator().manual_seed(0)
    pal = torch.randint(0, 256, (K, 3), generator=g, dtype=torch.uint8).to(dev)
    cmap = pal.cpu().numpy()
    colours = hip.viz_colour_table(cmap, dev)
    variants = {}
    slow = max(a.iters // 10, 50)
    # ---- (a) the kernels
    for n in (1, 8):
        lab = torch.randint(0, K, (n, H, W), generator=g)
        lab[:, :H // 16] = 255
        lab64, lab8 = lab.to(dev), lab.to(torch.uint8).to(dev)
        ev = (torch.randn(n, 10, H, W, generator=g) * (torch.rand(n, 10, H, W, generator=g) < 0.1)).to(dev)
        gray = torch.randint(0, 256, (n, H, W), generator=g, dtype=torch.uint8).to(dev)
        out_f, out_o = torch.empty(n, 3, H, W, device=dev), torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        variants[f'N{n}_semseg_ours'] = (lambda l=lab64, o=out_f: hip.viz_semseg(l, colours, 255, out=o), a.iters)
        variants[f'N{n}_semseg_torch'] = (lambda l=lab64: torch_prepare_semseg(l, colours, 255), slow)
        variants[f'N{n}_events_ours'] = (lambda x=ev, o=out_f: hip.viz_events(x, 'separate_pol', out=o), a.iters)
        variants[f'N{n}_events_torch'] = (lambda x=ev: torch_voxel(x), slow)
        variants[f'N{n}_overlay_ours'] = (lambda l=lab8, f=gray, o=out_o: hip.viz_overlay(l, f, pal, 0.6, out=o), a.iters)
        variants[f'N{n}_overlay_torch'] = (lambda l=lab8, f=gray: torch_overlay(l, f, pal, 0.6), slow)
    # ---- (c) a validation panel of five rows, B = 4
    B = 4
    ev = (torch.randn(B, 10, H, W, generator=g) * (torch.rand(B, 10, H, W, generator=g) < 0.1)).to(dev)
    fake = torch.rand(B, 1, H, W, generator=g).to(dev)
    labs = []
    for _ in range(3):
        lab = torch.randint(0, K, (B, H, W), generator=g)
        lab[:, :H // 16] = 255
        labs.append(lab.to(dev))
    rows = [('events', ev), ('gray', fake)] + [('semseg', lab) for lab in labs]

    def panel_torch():
        tiles = [torch_voxel(ev).clamp(0, 1), fake.expand(-1, 3, -1, -1)] + [torch_prepare_semseg(lab, colours, 255) for lab in labs]
        return torch_make_grid(torch.cat(tiles, 0), 4)
    # (torch's channel sum is not the sequential order: the event row may differ in the last bit; the label rows may not)
    diff = (viz_utils.panel(rows, 4, color_map=cmap) - panel_torch()).abs()
    out['panel_ours_vs_torch_composition_max_abs_diff'] = float(diff.max().item())
    out['panel_ours_vs_torch_composition_elements_differing'] = int((diff != 0).sum().item())
    variants['panel5_ours'] = (lambda: viz_utils.panel(rows, 4, color_map=cmap), a.iters)
    variants['panel5_torch'] = (panel_torch, slow)
    for run in range(2):
        for name, (fn, iters) in variants.items():
            out.setdefault(name, []).append(timed(fn, iters))
    # ---- (b) the streaming window
    if not a.skip_stream:
        cfg = dict(num_bins=5, skip_type='sum', num_encoders=3, base_num_channels=32, num_residual_blocks=2, norm='BN',
                   use_upsample_conv=True, recurrent_block_type='convlstm')
        opts = default_options()
        opts.auto_hdr = True
        grids = [(torch.randn(1, 5, H, W, generator=g) * (torch.rand(1, 5, H, W, generator=g) < 0.1)).to(dev) for _ in range(4)]

        class Pair:
            """the way to the same outputs without the feature: two drivers on the same grid + a torch blend"""

            def __init__(self, use_graph):
                self.seg = StreamingSegmenter(E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, K, skip_connect=True, skip_type='concat'), H, W, opts,
                                              graph=use_graph, palette=pal)
                self.rec = StreamingReconstructor(E2VIDRecurrent(dict(cfg)), H, W, opts, graph=use_graph, postprocess=True)

            def update(self, grid):
                r = self.seg.update(grid)
                _, _, frame = self.rec.update(grid)
                return r, frame, torch_overlay(r.labels, frame.unsqueeze(0), pal, 0.6)

        for mode in ('mixed', 'bf16'):
            hip.set_compute(mode)
            torch.manual_seed(6)
            drivers = {}
            for how in ('eager', 'graph'):
                ug = how == 'graph'
                new = lambda **kw: StreamingSegmenter(E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, K, skip_connect=True, skip_type='concat'),  # noqa: E731
                                                      H, W, opts, graph=ug, palette=pal, **kw)
                drivers[f'stream_{mode}_{how}_display_ms_per_window'] = new(reconstruct=True, postprocess=True, overlay=0.6)
                drivers[f'stream_{mode}_{how}_two_drivers_and_torch_blend_ms_per_window'] = Pair(ug)
                drivers[f'stream_{mode}_{how}_plain_segmenter_ms_per_window'] = new()
            for s in drivers.values():
                for i in range(5):
                    s.update(grids[i % 4])
            for run in range(2):
                for name, s in drivers.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(a.windows):
                        s.update(grids[i % 4])
                    torch.cuda.synchronize()
                    out.setdefault(name, []).append(round((time.perf_counter() - t0) / a.windows * 1e3, 4))
        hip.set_compute('fp32')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
