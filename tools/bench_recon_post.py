#!/usr/bin/env python
"""Cost of the reconstruction post-processing (image_reconstructor.PostProcessor: unsharp mask, auto-HDR bounds, 8-bit frame) at
N x 480 x 640, N = 1 and 8, against the reference's own lines composed from torch operations on the same device, and of a
StreamingReconstructor window with and without postprocess=True, eager and replayed.  Every variant is timed twice, the variants
alternating (run 1 of all, then run 2 of all); both figures are printed.  Host clock around work that ends in a device synchronise.
usage: python tools/bench_recon_post.py [--height 480 --width 640 --iters 3000 --windows 100]"""
import argparse
import json
import os
import sys
import time
from collections import deque

import numpy as np
import torch
import torch.nn.functional as F

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


class TorchReference:
    """The reference's lines for ONE frame [1, 1, H, W] (UnsharpMaskFilter.__call__, IntensityRescaler.__call__ with auto_hdr): a library
    convolution, min / max fetched with .item() (two synchronisations), the history in a deque, the medians in numpy, the rescale as
    five element-wise torch operations."""

    def __init__(self, kernel, amount, size):
        self.k, self.amount, self.size, self.hist = kernel, amount, size, deque()

    def __call__(self, img):
        x = (1 + self.amount) * img - self.amount * F.conv2d(img, self.k, padding=2)
        lo, hi = np.clip(torch.min(x).item(), 0.0, 0.45), np.clip(torch.max(x).item(), 0.55, 1.0)
        if len(self.hist) > self.size:
            self.hist.popleft()
        self.hist.append((lo, hi))
        imin, imax = np.median([a for a, _ in self.hist]), np.median([b for _, b in self.hist])
        x = 255.0 * (x - imin) / (imax - imin)
        x.clamp_(0.0, 255.0)
        return x.byte()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--iters', type=int, default=3000)
    ap.add_argument('--windows', type=int, default=100)
    ap.add_argument('--events', type=int, default=107520)
    ap.add_argument('--skip-stream', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_recon_post needs the GPU: there is nothing to time without one')
    from ess_amd import hip
    from ess_amd.e2vid.image_reconstructor import PostProcessor
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.run_reconstruction import StreamingReconstructor
    dev = torch.device('cuda:0')
    H, W = a.height, a.width
    out = {'shape': f'{H}x{W}', 'iters': a.iters, 'unit': 'us per call (frames of all N samples)', 'runs': 2}
    hdr, fixed = default_options(), default_options()
    hdr.auto_hdr = True
    variants = {}
    for n in (1, 8):
        img = torch.rand(n, 1, H, W, device=dev)
        pp_hdr, pp_fixed = PostProcessor(dev, hdr, n=n), PostProcessor(dev, fixed, n=n)
        variants[f'N{n}_ours_bounds_and_frame'] = (lambda p=pp_hdr, x=img: p.process_u8(x), a.iters)
        variants[f'N{n}_ours_frame_fixed_bounds'] = (lambda p=pp_fixed, x=img: p.process_u8(x), a.iters)
        pp_g = PostProcessor(dev, hdr, n=n)
        pp_g.process_u8(img)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pp_g.process_u8(img)
        variants[f'N{n}_ours_bounds_and_frame_replayed'] = (g.replay, a.iters)
        refs = [TorchReference(pp_hdr.unsharp_mask_filter.gaussian_kernel, 0.3, hdr.auto_hdr_median_filter_size) for _ in range(n)]
        frames = [img[i:i + 1] for i in range(n)]
        try:
            got = refs[0](frames[0])
            ours = PostProcessor(dev, hdr, n=n).process_u8(img)[0]
            diff = (got[0, 0].int() - ours.int()).abs()
            out[f'N{n}_torch_vs_ours_pixels_differing'] = int((diff != 0).sum().item())
            out[f'N{n}_torch_vs_ours_max_levels'] = int(diff.max().item())
            refs[0].hist.clear()
            # (N = 8: the reference has one history and takes one frame, so eight streams are eight calls)
            variants[f'N{n}_torch_composition'] = (lambda r=refs, f=frames: [ri(fi) for ri, fi in zip(r, f)], max(a.iters // 10, 50))
        except RuntimeError as e:
            out[f'N{n}_torch_composition'] = 'could not run: ' + str(e).splitlines()[0][:160]
    for run in range(2):
        for name, (fn, iters) in variants.items():
            out.setdefault(name, []).append(timed(fn, iters))
    if not a.skip_stream:
        torch.manual_seed(6)
        cfg = dict(num_bins=5, skip_type='sum', num_encoders=3, base_num_channels=32, num_residual_blocks=2, norm='BN',
                   use_upsample_conv=True, recurrent_block_type='convlstm')
        hip.set_compute('bf16')
        g = np.random.default_rng(0)
        wins = []
        for w in range(4):
            t = np.sort(g.uniform(0, 0.03, a.events)) + 0.03 * w
            wins.append(torch.from_numpy(np.stack([t, g.integers(0, W, a.events).astype(np.float64),
                                                   g.integers(0, H, a.events).astype(np.float64),
                                                   g.integers(0, 2, a.events).astype(np.float64)], 1)).cuda())
        drivers = {}
        for mode in ('eager', 'graph'):
            for post in (False, True):
                s = StreamingReconstructor(E2VIDRecurrent(dict(cfg)), H, W, hdr, graph=mode == 'graph', postprocess=post)
                for i in range(5):
                    s.update_from_events(wins[i % 4])
                drivers[f'stream_{mode}_{"post" if post else "plain"}_ms_per_window'] = s
        for run in range(2):
            for name, s in drivers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.windows):
                    s.update_from_events(wins[i % 4])
                torch.cuda.synchronize()
                out.setdefault(name, []).append(round((time.perf_counter() - t0) / a.windows * 1e3, 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
