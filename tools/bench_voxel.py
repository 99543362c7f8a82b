#!/usr/bin/env python
"""Measurement for SURVEY.md 8(f)1 (events -> voxel grids): one DSEC-shape batch = B=8 sequences x T=5 slices of
100 000 events -> [8, 5*2, 480, 640], converted by ONE call.  Prints one JSON line: events/s on the GPU (inputs
resident in HBM), the algorithmic traffic (16 B per event + 4 B per voxel) against the HBM peak, and the oracle (a restatement of the reference's put_(accumulate) loop) timed on
the host cores for a bounded sample.  usage: python tools/bench_voxel.py [--slices 40] [--events 100000]

--ingest measures the temporal flavour INSTEAD, two ways on the same events (device resident), alternating: hip.voxel_grid_temporal
(memset + fp32 atomics, separate_pol=False) and hip.event_ingest (the scatter + finish pair: 64-bit integer atomics into int64 sums,
then the conversion pass that also zeroes the sums again); an ingest with every count 0 gives the finish pass alone, the difference
the scatter, and from it the chip-wide rate of 64-bit integer atomics with one lane per row that the pair implies.  Next to the
record row, hip.event_ingest_columns (scatter + finish as well) on the same events held as DSEC's columns -- x / y uint16, p uint8, t
once as float64 (the records' own times: the grids are compared as bits) and once as int64 microseconds (compared as bits with the
record kernel on those times); reported with the record row's max - min over the repetitions as the run-to-run spread.  And
hip.event_ingest_ring on the int64 columns laid into rings of twice the stride, the window named by device words: from position 0
(every group of four aligned and whole, as in the column kernel), from position 3 (head and tail masked) and from a position that
puts the wrap into the middle of the window; each compared as bits with the column kernel, reported as its difference to it.
Beside them the TRILINEAR flavour on the same int64 columns, hip.event_ingest_columns_trilinear and hip.event_ingest_ring_trilinear
(ring: from position 3), through an identity map and through a smooth synthetic distortion map of the sensor -- the ring's bits
compared with the columns', the identity map's with no map at all -- and hip.voxel_grid_trilinear (binned) on the same events
rectified and converted to floats on the host beforehand, compared within the fp32 sums' rounding.
Behind them the LOADER FINISH at the two reference presets (their own sensor sizes, whatever --height / --width say): per preset
the ring ingest as it is (hip.event_ingest_ring*: the grid at the sensor's size), the loader's grid from the same sums
(hip.event_scatter_ring* + hip.event_grid_finish: normalised over its non-zero voxels, rows cut, resized, rows cut) and the
composition the older pieces allow (the ring ingest, hip.voxel_normalize_, torch's F.interpolate on the device, a slice made
contiguous), alternating.  --loader-finish-only skips everything in front of these rows.

And the event REPRESENTATIONS (representations()): the signed ring ingest against hip.event_ingest_ring_rep's separate-polarity and
histogram flavours on the same rings, at 480 x 640 and 260 x 346.

And the HOT-PIXEL MASKS (masked(), --masked: these rows alone): the ring source, signed temporal and trilinear through the distortion
map, three ways in ONE run -- the unmasked kernel, hip.event_ingest_masked under an all-zero mask, and under a mask of 100 hot pixels
that carry 5 % of the events -- and hip.event_hot_pixel_mask on one histogram a stream.

And the DEVICE EVENT STORE (store(), --store: these rows alone): hip.event_scatter_store against hip.event_scatter_ring on the same
events from start residues 0 and 3, and hip.event_store_windows alone on a time column of --store-events events.

And HOT-PIXEL MASKS ON THE STORE (store_masked(), --store-masked: these rows alone): the scatter half of hip.event_ingest_store -- no
mask tensor, an all-zero mask, 100 hot pixels that carry 5 % of the events -- beside hip.event_scatter_store on the same windows;
hip.event_store_pixel_counts + hip.event_count_mask on 10 M and 100 M events; and, with --parent-lib, ess_event_scatter_store of a
library built from the parent commit beside this build's, in the same run.

usage: python tools/bench_voxel.py --ingest --slices 8 --events 100000 --bins 5
       python tools/bench_voxel.py --ingest --masked --slices 8 --events 100000 --bins 5
       python tools/bench_voxel.py --ingest --representations-only --slices 8 --events 100000 --bins 5
       python tools/bench_voxel.py --ingest --loader-finish-only --slices 160 --events 100000 --bins 5 --reps 20
       python tools/bench_voxel.py --ingest --store --slices 8 --events 100000 --bins 5
       python tools/bench_voxel.py --ingest --store-masked --slices 8 --events 100000 --bins 5 [--parent-lib PATH]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slices', type=int, default=40)
    ap.add_argument('--events', type=int, default=100_000)
    ap.add_argument('--bins', type=int, default=2)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--normalize', action='store_true')
    ap.add_argument('--ingest', action='store_true', help='hip.event_ingest against hip.voxel_grid_temporal (see above)')
    ap.add_argument('--loader-finish-only', action='store_true', help='(with --ingest) only the loader-finish rows')
    ap.add_argument('--representations-only', action='store_true', help='(with --ingest) only the event-representation rows')
    ap.add_argument('--masked', action='store_true', help='(with --ingest) only the hot-pixel mask rows')
    ap.add_argument('--store', action='store_true', help='(with --ingest) only the device event store rows')
    ap.add_argument('--store-masked', action='store_true', help='(with --ingest) only the rows of hot-pixel masks on the store source')
    ap.add_argument('--parent-lib', default=None, help="(with --store-masked) a libess_hip.so built from the parent commit: its "
                    'ess_event_scatter_store is timed beside this build\'s in the same run')
    ap.add_argument('--store-events', type=int, default=100_000_000, help='(with --store) events of the column the window search runs on')
    a = ap.parse_args()
    if a.ingest:
        return ingest(a)
    from ess_amd import hip
    from oracle import ess_oracle as O
    hip.lib()
    S, n, C, H, W = a.slices, a.events, a.bins, a.height, a.width
    xs, ys, ps, ts = [], [], [], []
    for s in range(S):
        x, y, pol, t = O.synth_events(n, H, W, 100 + s)
        tf = (t - t[0]).float()
        xs.append(x); ys.append(y); ps.append(pol); ts.append(tf / tf[-1])
    offs = [i * n for i in range(S + 1)]
    d = [torch.cat(v).cuda() for v in (xs, ys, ps, ts)]
    for _ in range(50):  # warm-up: clocks (DVFS ramps over tens of ms), allocator
        out = hip.voxel_grid_trilinear(*d, offs, C, H, W, normalize=a.normalize)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out = hip.voxel_grid_trilinear(*d, offs, C, H, W, normalize=a.normalize)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    # parity spot check against the oracle on slice 0 (the checker, not the thing measured)
    ref = O.voxel_grid_trilinear(xs[0], ys[0], ps[0], ts[0], C, H, W, a.normalize)
    err = (out[0].cpu() - ref).abs().max().item()
    assert err <= 1e-4 * max(1.0, ref.abs().max().item()), err
    # CPU baseline: the oracle on a bounded sample of the same slices
    # (index_put_(accumulate) is a serial scatter: more threads do not help, 8 is what a DataLoader worker gets)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    k, m = 1, min(n, 20_000)
    t0 = time.perf_counter()
    O.voxel_grid_trilinear(xs[0][:m], ys[0][:m], ps[0][:m], ts[0][:m], C, H, W, a.normalize)
    cpu_s = time.perf_counter() - t0
    ev = S * n
    grid_bytes = S * C * H * W * 4
    alg = ev * 16 + grid_bytes  # every event read once (x, y, pol, t) + every voxel written once
    print(json.dumps({
        'metric': 'events -> voxel grids (trilinear), events/s', 'value': ev / (ms * 1e-3), 'unit': 'events/s',
        'ms_per_batch': ms, 'config': {'workload': f'{S} slices x {n} events -> [{S},{C},{H},{W}] fp32', 'normalize': a.normalize},
        'dtype': 'f32', 'data': 'synthetic',
        'roofline': {'bound': 'hbm', 'achieved': alg / (ms * 1e-3) / 1e9, 'peak': 8000.0, 'unit': 'GB/s',
                     'frac': alg / (ms * 1e-3) / 8e12, 'traffic': None,
                     'note': 'algorithmic bytes = 16 B/event + 4 B/voxel; the tile-binned path moves ~56 B/event + 2x the grid in its four passes'},
        'cpu_baseline': {'value': k * m / cpu_s, 'unit': 'events/s', 'cores': torch.get_num_threads(), 'kind': 'port',
                         'sample': f'{k} slice x {m} events through oracle.voxel_grid_trilinear'},
        'max_abs_err_vs_oracle_slice0': err,
    }))


# the reference loaders' grids: DDD17 (datasets/ddd17_events_loader.py: 260 x 346 -> 260 x 352, the top 200 rows; temporal) and DSEC
# with resize=True (DSEC/dataset/sequence.py: 480 rows -> the top 440 -> 448 x 640; trilinear, VoxelGrid(normalize=True))
LOADER_PRESETS = {'ddd17': dict(flavour='temporal', src=(260, 346), crop_rows=260, resize=(260, 352), out_rows=200, normalize='population'),
                  'dsec': dict(flavour='trilinear', src=(480, 640), crop_rows=440, resize=(448, 640), out_rows=448, normalize='unbiased')}


def loader_finish(a):
    """-> {preset: row}: ms per batch of the three ways above, alternating, 3 x --reps launches each"""
    import numpy as np
    import torch.nn.functional as F
    from ess_amd import hip
    S, n, C = a.slices, a.events, a.bins
    dev = torch.device('cuda:0')
    rows_out = {}
    for name, ps in LOADER_PRESETS.items():
        (Hs, Ws), (Hr, Wr), crop, rows = ps['src'], ps['resize'], ps['crop_rows'], ps['out_rows']
        g = np.random.default_rng(1)
        ring = hip.event_column_stride(n)
        t = np.sort(g.integers(0, 30_000, (S, ring)), axis=1).astype(np.int64) + 1_600_000_000_000_000
        cols = (t, g.integers(0, Ws, (S, ring)).astype(np.int16), g.integers(0, Hs, (S, ring)).astype(np.int16),
                g.integers(0, 2, (S, ring)).astype(np.uint8))
        dcols = tuple(torch.from_numpy(c).to(dev) for c in cols)
        words = (torch.arange(S, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev),
                 torch.full((S,), n, dtype=torch.int32, device=dev), torch.full((S,), hip.EVCOL_T_I64, dtype=torch.int32, device=dev))
        acc = torch.zeros(S, C, Hs, Ws, dtype=torch.int64, device=dev)
        big, net = torch.empty(S, C, Hs, Ws, device=dev), torch.empty(S, C, rows, Wr, device=dev)
        tri = ps['flavour'] == 'trilinear'
        ingest_fn, scatter_fn = (hip.event_ingest_ring_trilinear, hip.event_scatter_ring_trilinear) if tri else \
            (hip.event_ingest_ring, hip.event_scatter_ring)
        norm = hip.GRID_NORM_UNBIASED if ps['normalize'] == 'unbiased' else hip.GRID_NORM_POPULATION

        def plain():
            return ingest_fn(*dcols, *words, big, acc=acc)

        def finish():
            scatter_fn(*dcols, *words, acc)
            return hip.event_grid_finish(words[2], acc, net, crop_rows=crop, resize=(Hr, Wr), normalize=norm)

        def composed():
            plain()
            hip.voxel_normalize_(big, 0 if norm == hip.GRID_NORM_UNBIASED else 1)
            return F.interpolate(big[:, :, :crop], size=(Hr, Wr), mode='bilinear', align_corners=True)[:, :, :rows].contiguous()
        ways = {'ingest_ring_at_sensor_size': plain, 'scatter_plus_grid_finish': finish, 'ingest_normalize_interpolate_slice': composed}
        for fn in ways.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        diff = (finish() - composed()).abs().max().item()
        assert diff <= 1e-3 and not bool(acc.any()) and bool(net.any()), (name, diff)
        ms = {k: [] for k in ways}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            for k, fn in ways.items():
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.reps)
        med = {k: sorted(v)[1] for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        rows_out[name] = {
            'workload': f'{S} slots x {n} events, {ps["flavour"]}, [{S},{C},{Hs},{Ws}] sums -> [{S},{C},{rows},{Wr}] fp32, {ps["normalize"]}',
            'ms_per_batch': {k: {'median': round(med[k], 5), 'min': round(min(v), 5), 'max': round(max(v), 5)} for k, v in ms.items()},
            'finish_minus_plain_ingest_ms': round(med['scatter_plus_grid_finish'] - med['ingest_ring_at_sensor_size'], 5),
            'finish_SLOWER_than_plain_ingest': bool(med['scatter_plus_grid_finish'] - med['ingest_ring_at_sensor_size'] > spread),
            'composed_over_finish': round(med['ingest_normalize_interpolate_slice'] / med['scatter_plus_grid_finish'], 3),
            'finish_SLOWER_than_composed': bool(med['scatter_plus_grid_finish'] - med['ingest_normalize_interpolate_slice'] > spread),
            'spread_ms': round(spread, 5), 'max_abs_diff_finish_vs_composed': diff}
        del acc, big, net, dcols
        torch.cuda.empty_cache()
    return rows_out


def representations(a):
    """The event representations beside the signed grid: hip.event_ingest_ring (scatter + finish, `bins` planes) against
    hip.event_ingest_ring_rep in the separate-polarity (2 * bins planes) and the histogram (2 planes, no time loads) flavour, on
    the same int64 / uint16 rings read from an unaligned start, at the DSEC and the DDD17 sensor size; three alternating rounds of
    a.reps calls each.  A library without the _rep entry points (an older build) gets the signed row alone.  -> rows for the JSON"""
    import numpy as np
    from ess_amd import hip
    S, n, bins = a.slices, a.events, a.bins
    dev = torch.device('cuda:0')
    have = hasattr(hip, 'event_ingest_ring_rep')
    stride = hip.event_column_stride(n)
    ring, start = 2 * stride, 3
    rows = {}
    for H, W in ((480, 640), (260, 346)):
        g = np.random.default_rng(1)
        at = (start + np.arange(n)) % ring
        cols = [np.zeros((S, ring), d) for d in (np.int64, np.uint16, np.uint16, np.uint8)]
        cols[0][:, at] = np.sort(g.integers(0, 30_000, (S, n)), axis=1)
        cols[1][:, at], cols[2][:, at], cols[3][:, at] = g.integers(0, W, (S, n)), g.integers(0, H, (S, n)), g.integers(0, 2, (S, n))
        dcols = tuple(torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).to(dev) for c in cols)
        words = (torch.arange(S, dtype=torch.int32, device=dev), torch.full((S,), start, dtype=torch.int32, device=dev),
                 torch.full((S,), n, dtype=torch.int32, device=dev),
                 torch.full((S,), hip.EVCOL_XY_U16 | hip.EVCOL_T_I64, dtype=torch.int32, device=dev))
        buffers = lambda C: (torch.empty(S, C, H, W, device=dev), torch.zeros(S, C, H, W, dtype=torch.int64, device=dev))  # noqa: E731
        out_s, acc_s = buffers(bins)
        ways = {'signed_event_ingest_ring': lambda: hip.event_ingest_ring(*dcols, *words, out_s, acc=acc_s)}
        if have:
            out_p, acc_p = buffers(2 * bins)
            out_h, acc_h = buffers(2)
            ways['signed_event_ingest_ring_rep'] = lambda: hip.event_ingest_ring_rep(*dcols, *words, out_s, hip.EVENT_REP_SIGNED, acc=acc_s)
            ways['separate_pol'] = lambda: hip.event_ingest_ring_rep(*dcols, *words, out_p, hip.EVENT_REP_SEPARATE, acc=acc_p)
            ways['histogram'] = lambda: hip.event_ingest_ring_rep(*dcols, *words, out_h, hip.EVENT_REP_HISTOGRAM, acc=acc_h)
        for fn in ways.values():  # warm-up: clocks, allocator
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in ways}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            for k, fn in ways.items():
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.reps)
        med = {k: sorted(v)[1] for k, v in ms.items()}
        spread = max(ms['signed_event_ingest_ring']) - min(ms['signed_event_ingest_ring'])
        row = {'ms_per_batch': {k: {'median': round(med[k], 5), 'min': round(min(v), 5), 'max': round(max(v), 5)} for k, v in ms.items()},
               'signed_spread_ms': round(spread, 5)}
        if have:
            # what is timed is what the representations are: positive - negative = the signed grid, the counts add up to the events
            signed = ways['signed_event_ingest_ring']().clone()
            sep, hist = ways['separate_pol'](), ways['histogram']()
            assert float((sep[:, :bins] - sep[:, bins:] - signed).abs().max()) <= 1e-5 * max(1.0, float(signed.abs().max()))
            assert float(hist.sum()) == S * n and bool((sep >= 0).all()) and not bool(acc_p.any()) and not bool(acc_h.any())
            for k in ('separate_pol', 'histogram', 'signed_event_ingest_ring_rep'):
                row[f'{k}_over_signed'] = round(med[k] / med['signed_event_ingest_ring'], 3)
                row[f'{k}_SLOWER_than_signed'] = bool(med[k] - med['signed_event_ingest_ring'] > spread)
        rows[f'{H}x{W}'] = row
    return {'workload': f'{S} streams x {n} events, bins={bins}, ring of {ring} from start {start}', 'reps': a.reps, 'rows': rows}


def masked(a):
    """The hot-pixel masks beside the kernels they wrap, on int64 / uint16 rings read from start 3 (S streams x n events, 5 % of them
    on 100 pixels of the sensor): per flavour -- signed temporal, trilinear through the synthetic distortion map -- the unmasked
    entry point, hip.event_ingest_masked with an all-zero mask (the added load and test, no event dropped) and with the 100 pixels
    masked (5 % fewer events reach the flavour); three alternating rounds of a.reps calls each.  And hip.event_hot_pixel_mask on
    [S, 2, H, W] histogram sums.  -> rows for the JSON"""
    import numpy as np
    from ess_amd import hip
    from ess_amd.datasets.hot_pixels import HotPixelMask
    S, n, C, H, W = a.slices, a.events, a.bins, a.height, a.width
    dev = torch.device('cuda:0')
    g = np.random.default_rng(2)
    stride = hip.event_column_stride(n)
    ring, start = 2 * stride, 3
    at = (start + np.arange(n)) % ring
    hot = g.permutation(H * W)[:100]
    x, y = g.integers(0, W, (S, n)), g.integers(0, H, (S, n))
    on_hot = g.random((S, n)) < 0.05
    pick = hot[g.integers(0, len(hot), (S, n))]
    x, y = np.where(on_hot, pick % W, x), np.where(on_hot, pick // W, y)
    cols = [np.zeros((S, ring), d) for d in (np.int64, np.uint16, np.uint16, np.uint8)]
    cols[0][:, at] = np.sort(g.integers(0, 30_000, (S, n)), axis=1)
    cols[1][:, at], cols[2][:, at], cols[3][:, at] = x, y, g.integers(0, 2, (S, n))
    dcols = tuple(torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).to(dev) for c in cols)
    words = (torch.arange(S, dtype=torch.int32, device=dev), torch.full((S,), start, dtype=torch.int32, device=dev),
             torch.full((S,), n, dtype=torch.int32, device=dev), torch.full((S,), hip.EVCOL_XY_U16 | hip.EVCOL_T_I64, dtype=torch.int32, device=dev))
    mask = HotPixelMask.from_locations(np.stack([hot % W, hot // W], 1), H, W)
    dmasks = torch.from_numpy(np.stack([np.zeros_like(mask.words), mask.words]).view(np.int32)).to(dev)  # mask 0: empty, mask 1: the 100
    of = {'all_zero_mask': torch.zeros(S, dtype=torch.int32, device=dev), 'hot_100_pixels': torch.ones(S, dtype=torch.int32, device=dev)}
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    dmap = torch.from_numpy(np.stack([xx + 3.0 * np.sin(yy / 40.0), yy + 3.0 * np.cos(xx / 50.0)], -1).astype(np.float32)[None]).to(dev)
    map0 = torch.zeros(S, dtype=torch.int32, device=dev)
    out, acc = torch.empty(S, C, H, W, device=dev), torch.zeros(S, C, H, W, dtype=torch.int64, device=dev)
    ways = {'temporal_unmasked': lambda: hip.event_ingest_ring(*dcols, *words, out, acc=acc),
            'trilinear_unmasked': lambda: hip.event_ingest_ring_trilinear(*dcols, *words, out, dmap, map0, acc=acc)}
    for k, w in of.items():
        ways[f'temporal_{k}'] = lambda w=w: hip.event_ingest_masked(*dcols, *words, out, dmasks, w, (H, W), acc=acc)
        ways[f'trilinear_{k}'] = lambda w=w: hip.event_ingest_masked(*dcols, *words, out, dmasks, w, (H, W), trilinear=True, maps=dmap,
                                                                     map_of=map0, acc=acc)
    sums = hip.event_scatter_ring_rep(*dcols, *words, torch.zeros(S, 2, H, W, dtype=torch.int64, device=dev), hip.EVENT_REP_HISTOGRAM)
    thresholds = torch.full((S,), 20, dtype=torch.int64, device=dev)
    found = torch.zeros(S, H, hip.mask_words(W), dtype=torch.int32, device=dev)
    ways['event_hot_pixel_mask'] = lambda: hip.event_hot_pixel_mask(sums, thresholds, found)
    for fn in ways.values():  # warm-up: clocks, allocator
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # alternating: drift of the box hits every way alike
        for k, fn in ways.items():
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)
    # what is timed is what it says: an all-zero mask gives the unmasked bits, the 100 pixels remove their events and only those,
    # and the calibration finds exactly the 100 (5 % of n over 100 pixels: ~ n / 2000 events each, against ~ n / (H W) elsewhere)
    for f in ('temporal', 'trilinear'):
        plain = ways[f'{f}_unmasked']().clone()
        assert torch.equal(ways[f'{f}_all_zero_mask']().view(torch.int32), plain.view(torch.int32)), f
        assert not torch.equal(ways[f'{f}_hot_100_pixels']().view(torch.int32), plain.view(torch.int32)), f
    cut = ways['temporal_hot_100_pixels']()
    assert not bool(cut[:, :, torch.from_numpy(hot // W).to(dev), torch.from_numpy(hot % W).to(dev)].any()) and not bool(acc.any())
    ways['event_hot_pixel_mask']()
    host = found.cpu().numpy().view(np.uint32)
    expect = n * 0.05 / 100 > 2 * 20
    if expect:
        assert all(np.array_equal(host[s], mask.words) for s in range(S)), 'the calibration does not return the 100 pixels'
    med = {k: sorted(v)[1] for k, v in ms.items()}
    row = {'ms_per_batch': {k: {'median': round(med[k], 5), 'min': round(min(v), 5), 'max': round(max(v), 5)} for k, v in ms.items()}}
    for f in ('temporal', 'trilinear'):
        spread = max(ms[f'{f}_unmasked']) - min(ms[f'{f}_unmasked'])
        row[f'{f}_unmasked_spread_ms'] = round(spread, 5)
        for k in of:
            d = med[f'{f}_{k}'] - med[f'{f}_unmasked']
            row[f'{f}_{k}_minus_unmasked_ms'] = round(d, 5)
            row[f'{f}_{k}_over_unmasked'] = round(med[f'{f}_{k}'] / med[f'{f}_unmasked'], 3)
            row[f'{f}_{k}_SLOWER_than_unmasked'] = bool(d > spread)
    return {'workload': f'{S} streams x {n} events, bins={C}, {H} x {W}, ring of {ring} from start {start}; 100 hot pixels carry 5 % of '
                        f'the events; event_hot_pixel_mask at {S} x {H} x {W}', 'reps': a.reps, 'mask_bytes': int(mask.words.nbytes), 'rows': row}


def store(a):
    """The device event store beside the ring: hip.event_scatter_store against hip.event_scatter_ring on the SAME events (S windows
    of n int64 / uint16 events), from start residues 0 and 3, alternating in one run -- every way scatters into one all-zero acc that
    an untimed torch zero_() clears outside the events (a scatter alone never clears its sums); and hip.event_store_windows alone on a
    time column of --store-events events made on the device, B = 8 samples x T = 20, by the count rule (one search a sample) and by
    the duration rule (21 searches a sample).  -> rows for the JSON"""
    import numpy as np
    from ess_amd import hip
    S, n, C, H, W = a.slices, a.events, a.bins, a.height, a.width
    dev = torch.device('cuda:0')
    stride = hip.event_column_stride(n)
    ring = 2 * stride
    g = np.random.default_rng(1)
    ev = [np.sort(g.integers(0, 30_000, (S, n)), axis=1).astype(np.int64), g.integers(0, W, (S, n)).astype(np.uint16),
          g.integers(0, H, (S, n)).astype(np.uint16), g.integers(0, 2, (S, n)).astype(np.uint8)]
    i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    fmt = i32([hip.EVCOL_XY_U16 | hip.EVCOL_T_I64] * S)
    counts = i32([n] * S)
    acc = torch.zeros(S, C, H, W, dtype=torch.int64, device=dev)
    ways, sums = {}, {}
    for start in (0, 3):
        rcols = [np.zeros((S, ring), c.dtype) for c in ev]
        flat = [np.zeros(S * ring, c.dtype) for c in ev]  # (window s lies at s * ring + start of the flat store: the ring's own bytes)
        for r, f, c in zip(rcols, flat, ev):
            r[:, start:start + n] = c
            f[:] = r.reshape(-1)
        dr = tuple(torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).to(dev) for c in rcols)
        df = tuple(torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).to(dev) for c in flat)
        rwords = (i32(list(range(S))), i32([start] * S), counts, fmt)
        starts = torch.as_tensor([s * ring + start for s in range(S)], dtype=torch.int64, device=dev)
        ways[f'scatter_ring_start{start}'] = lambda dr=dr, rwords=rwords: hip.event_scatter_ring(*dr, *rwords, acc)
        ways[f'scatter_store_start{start}'] = lambda df=df, starts=starts: hip.event_scatter_store(*df, starts, counts, fmt, acc, hip.EVENT_STORE_SIGNED,
                                                                                                  S * ring, stride)
    for k, fn in ways.items():  # (what is timed gives the same sums) + warm-up
        acc.zero_()
        fn()
        sums[k] = acc.clone()
        for _ in range(20):
            fn()
    same = all(torch.equal(sums[f'scatter_ring_start{s}'], sums[f'scatter_store_start{s}']) for s in (0, 3))
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        for k, fn in ways.items():
            total = 0.0
            for _ in range(a.reps):
                acc.zero_()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1)
            ms[k].append(total / a.reps)
    med = {k: sorted(v)[1] for k, v in ms.items()}
    spread = max(max(v) - min(v) for k, v in ms.items() if 'ring' in k)
    rows = {'ms_per_batch': {k: {'median': round(med[k], 5), 'min': round(min(v), 5), 'max': round(max(v), 5)} for k, v in ms.items()},
            'same_sums': bool(same), 'ring_spread_ms': round(spread, 5)}
    for s in (0, 3):
        d = med[f'scatter_store_start{s}'] - med[f'scatter_ring_start{s}']
        rows[f'store_minus_ring_start{s}_ms'] = round(d, 5)
        rows[f'store_SLOWER_than_ring_start{s}'] = bool(d > spread)
    # -- the window search alone
    N = hip.event_column_stride(a.store_events)
    t = torch.cumsum(torch.randint(0, 3, (N,), device=dev, dtype=torch.int64), 0)
    B, T = 8, 20
    table = torch.tensor([[0, N, hip.EVCOL_T_I64, 0]], dtype=torch.int64, device=dev)
    rec = torch.zeros(B, dtype=torch.int32, device=dev)
    last = int(t[-1])
    ends = torch.linspace(0.1, 0.95, B, dtype=torch.float64) * last
    b_count = ends.to(torch.int64).view(B, 1).to(dev)
    d = 50_000
    b_dur = (ends.to(torch.int64).view(B, 1) - T * d + d * torch.arange(T + 1, dtype=torch.int64).view(1, T + 1)).to(dev)
    out = (torch.zeros(B * T, dtype=torch.int64, device=dev), torch.zeros(B * T, dtype=torch.int32, device=dev),
           torch.zeros(B * T, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    search = {'count_rule': lambda: hip.event_store_windows(t, table, rec, b_count, hip.EVENT_STORE_RULE_COUNT_TIME, T, *out, N, 1 << 22,
                                                            n_per_window=n),
              'duration_rule': lambda: hip.event_store_windows(t, table, rec, b_dur, hip.EVENT_STORE_RULE_DURATION, T, *out, N, 1 << 22)}
    sms = {k: [] for k in search}
    for fn in search.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(3):
        for k, fn in search.items():
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            sms[k].append(e0.elapsed_time(e1) / a.reps)
    flags_ok = not bool(out[3].any())
    rows['event_store_windows'] = {'events': N, 'samples': B, 'T': T, 'flags_all_zero': flags_ok,
                                   'us_per_launch': {k: {'median': round(sorted(v)[1] * 1e3, 2), 'min': round(min(v) * 1e3, 2),
                                                         'max': round(max(v) * 1e3, 2)} for k, v in sms.items()},
                                   'clock': f'device events around {a.reps} back-to-back launches (launch overhead included)'}
    return {'workload': f'{S} windows x {n} events, bins={C}, {H} x {W}; ring of {ring} / a flat store of {S * ring}', 'reps': a.reps, 'rows': rows}


def store_masked(a):
    """Hot-pixel masks on the store source, three things in one run.  (1) hip.event_ingest_store, scatter half, against
    hip.event_scatter_store on the SAME windows (S windows of n int64 / uint16 events from start residue 3): no mask tensor, an
    all-zero mask, and 100 hot pixels that carry 5 % of the events.  (2) hip.event_store_pixel_counts + hip.event_count_mask on 10 M
    and 100 M events made on the device, 5 % of them on 100 pixels (a pixel takes 50 000 / 500 000 atomics).  (3) --parent-lib:
    ess_event_scatter_store of a library built from the parent commit, called on the same pointers, alternating with this build's.
    -> rows for the JSON"""
    import ctypes
    import numpy as np
    from ess_amd import hip
    S, n, C, H, W = a.slices, a.events, a.bins, a.height, a.width
    dev = torch.device('cuda:0')
    stride = hip.event_column_stride(n)
    ring, start = 2 * stride, 3
    g = np.random.default_rng(1)
    hot = g.permutation(H * W)[:100]
    pix = g.integers(0, H * W, (S, n))
    on_hot = g.random((S, n)) < 0.05
    pix[on_hot] = hot[g.integers(0, 100, int(on_hot.sum()))]
    ev = [np.sort(g.integers(0, 30_000, (S, n)), axis=1).astype(np.int64), (pix % W).astype(np.uint16), (pix // W).astype(np.uint16),
          g.integers(0, 2, (S, n)).astype(np.uint8)]
    flat = []
    for c in ev:
        r = np.zeros((S, ring), c.dtype)
        r[:, start:start + n] = c
        flat.append(torch.from_numpy(r.reshape(-1).view(np.int16) if c.dtype == np.uint16 else r.reshape(-1)).to(dev))
    i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    fmt, counts = i32([hip.EVCOL_XY_U16 | hip.EVCOL_T_I64] * S), i32([n] * S)
    starts = torch.as_tensor([s * ring + start for s in range(S)], dtype=torch.int64, device=dev)
    acc = torch.zeros(S, C, H, W, dtype=torch.int64, device=dev)
    bits = np.zeros((H, W), dtype=bool)
    bits[hot // W, hot % W] = True
    from ess_amd.datasets.hot_pixels import HotPixelMask
    mask = HotPixelMask.from_bool(bits)
    dmasks = torch.from_numpy(np.stack([np.zeros_like(mask.words), mask.words]).view(np.int32)).to(dev)
    total = S * ring
    ways = {'scatter_store': lambda: hip.event_scatter_store(*flat, starts, counts, fmt, acc, hip.EVENT_STORE_SIGNED, total, stride),
            'ingest_store_no_masks': lambda: hip.event_ingest_store(*flat, starts, counts, fmt, None, hip.EVENT_STORE_SIGNED, total, stride, acc=acc),
            'ingest_store_all_zero_mask': lambda: hip.event_ingest_store(*flat, starts, counts, fmt, None, hip.EVENT_STORE_SIGNED, total, stride,
                                                                         masks=dmasks, mask_of=i32([0] * S), mask_size=(H, W), acc=acc),
            'ingest_store_hot_100_pixels': lambda: hip.event_ingest_store(*flat, starts, counts, fmt, None, hip.EVENT_STORE_SIGNED, total, stride,
                                                                          masks=dmasks, mask_of=i32([1] * S), mask_size=(H, W), acc=acc)}
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.ess_event_scatter_store.argtypes = hip.lib().ess_event_scatter_store.argtypes
        P = ctypes.c_void_p
        args = [P(c.data_ptr()) for c in flat] + [P(starts.data_ptr()), P(counts.data_ptr()), P(fmt.data_ptr()), total, total, stride, S, C, H, W,
                                                  P(acc.data_ptr()), acc.numel() * 8, hip.EVENT_STORE_SIGNED, P(0), P(0), 0, 1, 1]

        def by_parent():
            assert parent.ess_event_scatter_store(*args, hip.stream()) == 0
        ways['scatter_store_parent_commit'] = by_parent
    sums = {}
    for k, fn in ways.items():  # (what is timed gives the sums it should) + warm-up
        acc.zero_()
        fn()
        sums[k] = acc.clone()
        for _ in range(20):
            fn()
    same = {k: bool(torch.equal(v, sums['scatter_store'])) for k, v in sums.items()}
    assert all(v for k, v in same.items() if k != 'ingest_store_hot_100_pixels') and not same['ingest_store_hot_100_pixels'], same
    assert not bool(sums['ingest_store_hot_100_pixels'][:, :, torch.from_numpy(hot // W).to(dev), torch.from_numpy(hot % W).to(dev)].any())
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # alternating: drift of the box hits every way alike
        for k, fn in ways.items():
            spent = 0.0
            for _ in range(a.reps):
                acc.zero_()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                spent += e0.elapsed_time(e1)
            ms[k].append(spent / a.reps)
    med = {k: sorted(v)[1] for k, v in ms.items()}
    spread = max(ms['scatter_store']) - min(ms['scatter_store'])
    rows = {'ms_per_batch': {k: {'median': round(med[k], 5), 'min': round(min(v), 5), 'max': round(max(v), 5)} for k, v in ms.items()},
            'scatter_store_spread_ms': round(spread, 5)}
    for k in ways:
        if k != 'scatter_store':
            d = med[k] - med['scatter_store']
            rows[f'{k}_minus_scatter_store_ms'] = round(d, 5)
            rows[f'{k}_SLOWER_than_scatter_store'] = bool(d > spread)
    if a.parent_lib:
        d = med['scatter_store'] - med['scatter_store_parent_commit']
        both = max(spread, max(ms['scatter_store_parent_commit']) - min(ms['scatter_store_parent_commit']))
        rows['scatter_store_minus_parent_commit_ms'] = round(d, 5)
        rows['scatter_store_MOVED_against_parent_commit'] = bool(abs(d) > both)
    # -- the calibration pair on whole recordings
    rows['count_and_mask'] = {}
    for N in (10_000_000, 100_000_000):
        cap = hip.event_column_stride(N)
        p = torch.randint(0, H * W, (cap,), device=dev)
        sel = torch.rand(cap, device=dev) < 0.05
        p[sel] = torch.from_numpy(hot).to(dev)[torch.randint(0, 100, (int(sel.sum()),), device=dev)]
        x, y = (p % W).to(torch.int16), (p // W).to(torch.int16)
        del p, sel
        job = torch.tensor([0, N, N // 20000], dtype=torch.int64, device=dev)  # (threshold: a tenth of a hot pixel's share of N / 2000)
        cnt = torch.zeros(1, H, W, dtype=torch.int64, device=dev)
        found = torch.zeros(1, H, hip.mask_words(W), dtype=torch.int32, device=dev)
        f0 = i32([0])
        pair = {'event_store_pixel_counts': lambda: hip.event_store_pixel_counts(x, y, job[0:1], job[1:2], f0, cnt, N),
                'event_count_mask': lambda: hip.event_count_mask(cnt, job[2:3], found)}
        cms = {k: [] for k in pair}
        reps = max(3, min(a.reps, 20))
        for _ in range(3):
            for k, fn in pair.items():
                spent = 0.0
                for _ in range(reps):
                    if k == 'event_store_pixel_counts':
                        cnt.zero_()
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    spent += e0.elapsed_time(e1)
                cms[k].append(spent / reps)
        assert int(cnt.sum()) == N and np.array_equal(found.cpu().numpy().view(np.uint32)[0], mask.words), 'the calibration does not find the 100'
        rows['count_and_mask'][str(N)] = {k: {'median_ms': round(sorted(v)[1], 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}
                                          for k, v in cms.items()}
        rows['count_and_mask'][str(N)]['GB_per_s_of_x_and_y'] = round(4 * N / (sorted(cms['event_store_pixel_counts'])[1] * 1e-3) / 1e9, 1)
        del x, y
    return {'workload': f'{S} windows x {n} events from start residue {start}, bins={C}, {H} x {W}, a flat store of {total}; 100 hot pixels '
                        f'carry 5 % of the events', 'reps': a.reps, 'rows': rows, 'UNMEASURED': 'index ranges above 2^31 events'}


def ingest(a):
    import numpy as np
    from ess_amd import hip
    from ess_amd.datasets.data_util import pack_event_records
    hip.lib()
    if a.store_masked:
        print(json.dumps({'metric': 'hot-pixel masks on the store source: masked ingest beside the scatter; counts + mask; the scatter '
                                    'beside the parent commit', 'unit': 'ms', 'store_masked': store_masked(a), 'data': 'synthetic'}))
        return
    if a.store:
        print(json.dumps({'metric': 'store events -> sums beside the ring scatter; the window search alone', 'unit': 'ms', 'store': store(a),
                          'data': 'synthetic'}))
        return
    if a.masked:
        print(json.dumps({'metric': 'ring events -> grids under hot-pixel masks, ms per batch', 'unit': 'ms', 'masked': masked(a),
                          'data': 'synthetic'}))
        return
    if a.representations_only:
        print(json.dumps({'metric': 'ring events -> grids in the three event representations, ms per batch', 'unit': 'ms',
                          'representations': representations(a), 'data': 'synthetic'}))
        return
    if a.loader_finish_only:
        print(json.dumps({'metric': 'ring events -> the loader\'s grids, ms per batch', 'unit': 'ms', 'reps': a.reps,
                          'loader_finish': loader_finish(a), 'data': 'synthetic'}))
        return
    S, n, C, H, W = a.slices, a.events, a.bins, a.height, a.width
    g = np.random.default_rng(0)
    host = np.zeros((S, n), dtype=hip.EVENT_RECORD)
    atomics = 0
    for s in range(S):
        t = np.sort(g.uniform(0, 0.03, n))
        ev = np.stack([t, g.integers(0, W, n).astype(np.float64), g.integers(0, H, n).astype(np.float64), g.integers(0, 2, n).astype(np.float64)], 1)
        pack_event_records(ev, host[s])
        ts = (C - 1) * (t - t[0]) / (t[-1] - t[0])
        dts = ts - np.floor(ts)
        # (the left half always, unless it rounds to zero; the right half where its bin exists and it is not zero)
        atomics += int(np.count_nonzero((1.0 - dts).astype(np.float32))) + int(np.count_nonzero((dts.astype(np.float32) != 0) & (np.floor(ts) + 1 < C)))
    dev = torch.device('cuda:0')
    records = torch.from_numpy(host.view(np.uint8).reshape(S, n, 16)).to(dev)
    counts, zero = torch.full((S,), n, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    acc = torch.zeros(S, C, H, W, dtype=torch.int64, device=dev)
    out = torch.empty(S, C, H, W, device=dev)
    x = torch.from_numpy(host['x'].astype(np.int32).ravel()).to(dev)
    y = torch.from_numpy(host['y'].astype(np.int32).ravel()).to(dev)
    t = torch.from_numpy(host['t'].ravel().copy()).to(dev)
    p = torch.from_numpy(host['p'].astype(np.float32).ravel()).to(dev)
    offs = torch.tensor([i * n for i in range(S + 1)])
    # the same events as DSEC delivers them: 13 bytes per event in four columns, rows at the aligned stride
    stride = hip.event_column_stride(n)
    hcols = [np.zeros((S, stride), d) for d in (np.float64, np.int64, np.uint16, np.uint16, np.uint8)]
    hcols[0][:, :n], hcols[2][:, :n], hcols[3][:, :n], hcols[4][:, :n] = host['t'], host['x'], host['y'], host['p'] == 1
    hcols[1][:, :n] = np.round(host['t'] * 1e6)  # (int64 microseconds)
    t_f64, t_i64, cx, cy, cp = (torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).to(dev) for c in hcols)
    fmt_f64 = torch.full((S,), hip.EVCOL_XY_U16, dtype=torch.int32, device=dev)
    fmt_i64 = torch.full((S,), hip.EVCOL_XY_U16 | hip.EVCOL_T_I64, dtype=torch.int32, device=dev)
    # the int64 columns as rings of 2 * stride events: the window (n events from `start` on, modulo the ring) holds the same events
    ring = 2 * stride
    rows_w = torch.arange(S, dtype=torch.int32, device=dev)
    ring_starts = {'start0': 0, 'start3': 3, 'wrapped': ring - (n // 2) // 4 * 4}
    rings = {}
    for k, start in ring_starts.items():
        at = (start + np.arange(n)) % ring
        hr = [np.zeros((S, ring), c.dtype) for c in (hcols[1], hcols[2], hcols[3], hcols[4])]
        for dst, src in zip(hr, (hcols[1], hcols[2], hcols[3], hcols[4])):
            dst[:, at] = src[:, :n]
        rings[k] = tuple(torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).to(dev) for c in hr) + \
            (torch.full((S,), start, dtype=torch.int32, device=dev),)

    def ring_way(k):
        rt, rx, ry, rp, starts_w = rings[k]
        return lambda: hip.event_ingest_ring(rt, rx, ry, rp, rows_w, starts_w, counts, fmt_i64, out, acc=acc)
    ways = {'voxel_grid_temporal': lambda: hip.voxel_grid_temporal(x, y, t, p, offs, C, H, W, separate_pol=False),
            'event_ingest': lambda: hip.event_ingest(records, counts, out, acc=acc),
            'event_ingest_columns_t_i64': lambda: hip.event_ingest_columns(t_i64, cx, cy, cp, counts, fmt_i64, out, acc=acc),
            'event_ingest_columns_t_f64': lambda: hip.event_ingest_columns(t_f64, cx, cy, cp, counts, fmt_f64, out, acc=acc),
            'event_ingest_finish_only': lambda: hip.event_ingest(records, zero, out, acc=acc)}
    ways.update({f'event_ingest_ring_{k}': ring_way(k) for k in rings})
    # the trilinear flavour: an identity map and a smooth distortion (a few pixels, some events pushed over the border) of the sensor
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    hmaps = {'identity': np.stack([xx, yy], -1).astype(np.float32),
             'distorted': np.stack([xx + 3.0 * np.sin(yy / 40.0), yy + 3.0 * np.cos(xx / 50.0)], -1).astype(np.float32)}
    map0 = torch.zeros(S, dtype=torch.int32, device=dev)
    rt, rx, ry, rp, starts3 = rings['start3']
    tri_out = {}
    for k, m in hmaps.items():
        dm = torch.from_numpy(m[None]).to(dev)
        ways[f'event_ingest_columns_trilinear_{k}'] = lambda dm=dm: hip.event_ingest_columns_trilinear(t_i64, cx, cy, cp, counts, fmt_i64, out, dm, map0, acc=acc)
        ways[f'event_ingest_ring_trilinear_{k}'] = lambda dm=dm: hip.event_ingest_ring_trilinear(rt, rx, ry, rp, rows_w, starts3, counts, fmt_i64, out, dm,
                                                                                                  map0, acc=acc)
        # the host alternative's input: the map looked up and the time normalised as the DSEC loader does, floats on the device
        xy = m[hcols[3][:, :n].astype(np.int64), hcols[2][:, :n].astype(np.int64)]
        d = (hcols[1][:, :n] - hcols[1][:, :1]).astype(np.float32)
        fl = [torch.from_numpy(np.ascontiguousarray(v).ravel()).to(dev) for v in (xy[..., 0], xy[..., 1], hcols[4][:, :n].astype(np.float32), d / d[:, -1:])]
        ways[f'voxel_grid_trilinear_binned_{k}'] = lambda fl=fl: hip.voxel_grid_trilinear(*fl, offs, C, H, W)
    for fn in ways.values():  # warm-up: clocks, allocator
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # alternating: drift of the box hits every way alike
        for k, fn in ways.items():
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.reps)
    ref = hip.voxel_grid_temporal(x, y, t, p, offs, C, H, W, separate_pol=False)
    got = hip.event_ingest(records, counts, out, acc=acc)
    err = (got - ref).abs().max().item()
    assert err <= 1e-5 * max(1.0, ref.abs().max().item()) and not bool(acc.any()), err
    # the column source gives the record kernel's bits: float64 times against the records above, int64 microseconds against
    # records that carry those times
    got = got.clone()
    assert torch.equal(hip.event_ingest_columns(t_f64, cx, cy, cp, counts, fmt_f64, out, acc=acc).view(torch.int32), got.view(torch.int32))
    host['t'] = hcols[1][:, :n]
    got = hip.event_ingest(torch.from_numpy(host.view(np.uint8).reshape(S, n, 16)).to(dev), counts, torch.empty_like(out), acc=acc)
    assert torch.equal(hip.event_ingest_columns(t_i64, cx, cy, cp, counts, fmt_i64, out, acc=acc).view(torch.int32), got.view(torch.int32))
    by_columns = out.clone()
    for k in rings:  # the ring source gives the column kernel's bits, wherever the window starts
        assert torch.equal(ways[f'event_ingest_ring_{k}']().view(torch.int32), by_columns.view(torch.int32)), k
    # the trilinear flavour: the ring kernel gives the column kernel's bits, the identity map those of no map at all, and both the
    # grid hip.voxel_grid_trilinear sums in fp32 from the same rectified events
    for k in hmaps:
        tri_out[k] = ways[f'event_ingest_columns_trilinear_{k}']().clone()
        assert torch.equal(ways[f'event_ingest_ring_trilinear_{k}']().view(torch.int32), tri_out[k].view(torch.int32)), k
        ref = ways[f'voxel_grid_trilinear_binned_{k}']()
        tri_err = (tri_out[k] - ref).abs().max().item()
        assert tri_err <= 1e-5 * max(1.0, ref.abs().max().item()) and bool(ref.any()), (k, tri_err)
    no_map = hip.event_ingest_columns_trilinear(t_i64, cx, cy, cp, counts, fmt_i64, torch.empty_like(out), acc=acc)
    assert torch.equal(no_map.view(torch.int32), tri_out['identity'].view(torch.int32))
    assert not bool(acc.any())
    med = {k: sorted(v)[1] for k, v in ms.items()}
    spread = max(ms['event_ingest']) - min(ms['event_ingest'])
    scatter_ms = med['event_ingest'] - med['event_ingest_finish_only']
    print(json.dumps({
        'metric': 'events -> voxel grids (temporal, one signed grid per stream), ms per batch', 'unit': 'ms',
        'config': {'workload': f'{S} streams x {n} events -> [{S},{C},{H},{W}] fp32', 'reps': a.reps},
        'ms_per_batch': {k: {'median': round(med[k], 5), 'min': round(min(v), 5), 'max': round(max(v), 5)} for k, v in ms.items()},
        'record_spread_ms': round(spread, 5),
        'columns_minus_records_ms': {k[-5:]: round(med[k] - med['event_ingest'], 5) for k in med if 'columns_t_' in k},
        'columns_slower_than_records_by_more_than_the_spread': {k[-5:]: bool(med[k] - med['event_ingest'] > spread) for k in med if 'columns_t_' in k},
        'ring': {'events_per_row': ring, 'starts': ring_starts,
                 'ring_minus_columns_t_i64_ms': {k: round(med[f'event_ingest_ring_{k}'] - med['event_ingest_columns_t_i64'], 5) for k in rings},
                 'slower_than_columns_by_more_than_the_spread': {k: bool(med[f'event_ingest_ring_{k}'] - med['event_ingest_columns_t_i64'] > spread)
                                                                 for k in rings}},
        'trilinear': {k: {'columns_over_temporal_columns': round(med[f'event_ingest_columns_trilinear_{k}'] / med['event_ingest_columns_t_i64'], 3),
                          'ring_over_temporal_ring': round(med[f'event_ingest_ring_trilinear_{k}'] / med['event_ingest_ring_start3'], 3),
                          'ring_over_voxel_grid_trilinear_binned': round(med[f'event_ingest_ring_trilinear_{k}'] / med[f'voxel_grid_trilinear_binned_{k}'], 3),
                          'slower_than_temporal_ring': bool(med[f'event_ingest_ring_trilinear_{k}'] - med['event_ingest_ring_start3'] > spread),
                          'slower_than_voxel_grid_trilinear_binned':
                              bool(med[f'event_ingest_ring_trilinear_{k}'] - med[f'voxel_grid_trilinear_binned_{k}'] > spread)} for k in hmaps},
        'bytes_per_event': {'records': 16, 'columns': 13},
        'scatter_ms': round(scatter_ms, 5), 'atomics_per_batch': atomics,
        'int64_atomics_per_s': atomics / (scatter_ms * 1e-3) if scatter_ms > 0 else None,
        'fp32_atomics_per_s_of_voxel_grid_temporal_incl_memset': atomics / (med['voxel_grid_temporal'] * 1e-3),
        'finish_GBps': S * C * H * W * 12 / (med['event_ingest_finish_only'] * 1e-3) / 1e9,
        'max_abs_diff_ingest_vs_temporal': err, 'loader_finish': loader_finish(a), 'representations': representations(a),
        'data': 'synthetic'}))


if __name__ == '__main__':
    main()
