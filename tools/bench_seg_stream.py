#!/usr/bin/env python
"""Latency of streaming event segmentation (B = 1, 5 x 480 x 640, K = 11, skip_connect=True): per event window voxel grid +
normalisation + recurrent step + semantic decoder + labels.  Two ways, in ONE process, alternating:

  segmenter    ess_amd.run_segmentation.StreamingSegmenter (encoder-only step, fused class head), eager issue and hipGraph replay;
  composed     what the package's older public pieces give: StreamingReconstructor.update (full UNet step, eager / replayed)
               -> SemSegE2VID.forward -> hip.argmax_confusion(want_pred=True).

Per (configuration, mode, way): `--reps` repetitions of `--windows` windows after `--warmup` windows, each repetition timed with the
host clock between device synchronisations; median and range over the repetitions, ms per window.  One JSON line.

--streams S[,S...] measures multi-stream serving INSTEAD: per stream count, one ROUND = one window of each of S streams, two ways,
alternating in the same process with the same repetition scheme:

  multi        ess_amd.run_segmentation.MultiStreamSegmenter(n_streams=S).update_from_events, eager issue and hipGraph replay;
  round_robin  S independent replayed StreamingSegmenters (graph=True) served one after the other -- what the package offered before.

Reported: ms per round and aggregate windows / s.

--streams S[,S...] --active k[,k...] measures rounds in which only k of the S streams have a window (round i: the streams
(i + j) % S, j < k -- which ones rotates) INSTEAD, two ways, both replayed, warm_up() in front of the timed region, alternating in the
same process with the same repetition scheme:

  ride_along   MultiStreamSegmenter(compact=False): the round runs all S streams, the idle ones on a zero grid;
  compact      MultiStreamSegmenter(compact=True[, compact_buckets=--buckets]): the round runs the smallest bucket >= k.

--streams S[,S...] --display measures DISPLAY ROUNDS INSTEAD -- MultiStreamSegmenter(reconstruct=True, postprocess=True, overlay=0.6), auto_hdr on:
labels plus each stream's image, displayable frame and label overlay --, every round timed from the call to the synchronised
result, all replayed, alternating in the same process:

  plain        MultiStreamSegmenter(graph=True): labels only (what the display costs is read against this);
  image        ... (reconstruct=True): the full recurrent step, no frame;
  display      ... (reconstruct=True, postprocess=True, overlay=0.6);
  round_robin  S StreamingSegmenter(graph=True, reconstruct=True, postprocess=True, overlay=0.6) served one after the other.

With --active k[,k...]: display rounds with k of the S streams active, compact=True against ride-along (both with the display).
Beside them the steered launches alone at N = S, 480 x 640 (device time over 200 launches): hip.recon_post_bounds + hip.recon_post_frame
unsteered, steered with every slot taken, and steered with 1 slot of S taken.  SLOWER is reported wherever that is the result.

--streams S[,S...] --ingest measures rounds FROM HOST EVENT ARRAYS INSTEAD: per round the wall time from S numpy [N, 4] arrays in host
memory to synchronised labels (a device synchronisation behind every round), three ways, all replayed, alternating in the same
process with the same repetition scheme:

  parent       MultiStreamSegmenter(event_capacity=None).update_from_events: concatenate, pageable upload, column split,
               hip.voxel_grid_temporal in front of the graph, copy of the S grids into the static input, replay;
  ingest       MultiStreamSegmenter(event_capacity=N).update_from_events: host packing into pinned 16-byte records, S small
               copies, replay (the voxeliser runs inside the graph);
  columns      MultiStreamSegmenter(event_capacity=N, event_layout='columns').update_from_events on the SAME events held as
               EventColumns in DSEC's dtypes (x / y uint16, p uint8, t int64 microseconds): four host copies per stream into pinned
               columns, 4 S small copies, replay.

Reported: ms per round (median, min, max over the repetitions), the parent's spread, the host packing and the host column staging
alone, whether the ingest way wins by more than that spread, and the column way's claim: it is below the record way by at least the
packing time minus the staging time, both as measured in this run.

--streams S[,S...] --feed measures rounds FROM A CONTINUOUS PACKET FEED INSTEAD: every stream delivers packets of a tenth of a window;
per round the wall time from the hand-over of the packet that completes the window to synchronised labels, two ways, both replayed,
alternating in the same process, once with windows back to back (stride = window) and once overlapping (stride = window / 4):

  columns      MultiStreamSegmenter(event_capacity=N, event_layout='columns').update_from_events on the window the deployment's own
               cutter has buffered and assembled (its assembly is NOT timed: the window is handed over as one contiguous EventColumns);
  ring         MultiStreamSegmenter(event_capacity=N, event_layout='ring').feed of that last packet + update_from_feed(): the earlier
               packets went to the device ring when they arrived, outside the timed region.

--feed --voxel trilinear builds both with voxel='trilinear' and two synthetic rectify maps shared by the streams in turn (a stereo
rig's), and times two more ways beside them, alternating in the same process:

  ring_temporal  the 'ring' way with voxel='temporal' on the same packets: what the flavour costs a round;
  host           what the flavour replaces: per stream a numpy lookup of the window's pixels in its map and the loader's fp32 time
                 normalisation, four float uploads, hip.voxel_grid_trilinear (binned), update(grids).

--streams S[,S...] --sequence T measures SEQUENCE ROUNDS INSTEAD (the DSEC validation protocol: at a label time the last T windows of
--events events run from a zero state and are scored against a ground truth): every stream has been fed its T x --events events
before the clock starts; per round the wall time from the request to synchronised labels and confusion rows, two ways, both
replayed, alternating in the same process:

  sequence     ess_amd.run_sequence_segmentation.SequenceSegmenter.segment_at(end=, labels=): one upload, one replay;
  composed     what the older public pieces give: MultiStreamSegmenter(event_layout='ring').reset() + T x update_from_feed(), then
               hip.label_confusion of every stream's last labels against its ground truth.

and, beside them, the class head alone (device time over 50 launches): hip.seg_head_eval against hip.seg_head followed by S
hip.label_confusion calls on int64 copies of the labels.  SLOWER is reported wherever that is the result.

--sequence T --loader-grid ddd17|dsec measures the sequence round on the LOADER's grid instead (the preset sets the sensor's size, the
network's size and the classes: DDD17 260 x 346 -> 200 x 352, K = 6, temporal, normalize_voxel_grid; DSEC 480 x 640 -> 448 x 640,
K = 11, trilinear, VoxelGrid(normalize=True)), two ways on ONE segmenter's rings, slot words and models, both replayed, alternating:

  loader_grid  SequenceSegmenter(grid_hw=, grid_rows=, grid_resize=, grid_normalize=).segment_at(end=, labels=);
  composed     the same round with its grids put together from the older pieces: hip.event_ingest_ring* at the sensor's size,
               hip.voxel_normalize_, torch's F.interpolate on the device, a slice made contiguous, then the round behind its grids
               (one captured graph as well; it reads the slot words the other way uploaded, so it pays no upload of its own).

--sequence T --store measures the sequence round cut on the device out of an EventStore, SequenceSegmenter(store=).segment_at(samples=),
against the ring-fed path on the same events and 50 %-overlapping consecutive labels -- feed() of the label's events and
segment_at(end=), inside the clock: only the half a lane has not been fed yet (ring_feed_new_half), or the whole sample after
drop_feed() (ring_refeed_sample) --, the three ways alternating inside every round, to synchronised labels.

usage: python tools/bench_seg_stream.py [--compute mixed,bf16 --windows 40 --warmup 8 --reps 3 --recurrent convlstm --streams 1,2,4,8
                                         [--active 1,2,4,6,8 [--buckets 1,2,4]] | --streams 8 --events 100000 --ingest | --streams 8 --events 100000 --feed [--voxel trilinear]
                                         | --streams 8 --events 100000 --sequence 20 --height 440 --windows 6 --warmup 2
                                         | --streams 8 --events 100000 --sequence 20 --loader-grid dsec --windows 6 --warmup 2
                                         | --streams 8 --events 100000 --sequence 20 --store --height 440 --windows 6 --warmup 2]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--bins', type=int, default=5)
    ap.add_argument('--classes', type=int, default=11)
    ap.add_argument('--events', type=int, default=107520, help='events per window (as tools/bench_stream.py)')
    ap.add_argument('--windows', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--recurrent', default='convlstm')
    ap.add_argument('--compute', default='mixed,bf16')
    ap.add_argument('--streams', default=None, help='comma-separated stream counts: measure MultiStreamSegmenter against round-robin serving')
    ap.add_argument('--active', default=None, help='(with --streams) comma-separated counts of active streams per round: measure compacted '
                                                   'against ride-along rounds')
    ap.add_argument('--buckets', default=None, help="(with --active) the compacting segmenter's compact_buckets, comma-separated (default: its own)")
    ap.add_argument('--display', action='store_true', help='(with --streams) display rounds: image, frame and overlay per stream, against '
                                                           'round-robin single-stream display segmenters; with --active: compacted against ride-along')
    ap.add_argument('--ingest', action='store_true', help='(with --streams) rounds from host event arrays: event_capacity=--events against '
                                                          'event_capacity=None')
    ap.add_argument('--feed', action='store_true', help="(with --streams) rounds from a continuous packet feed: event_layout='ring' against "
                                                        "'columns'")
    ap.add_argument('--voxel', default='temporal', choices=('temporal', 'trilinear'),
                    help="(with --feed) the grid the fed rounds build; 'trilinear': through rectify maps, timed against the temporal feed "
                         'and against the host alternative as well')
    ap.add_argument('--sequence', type=int, default=None, help='(with --streams) sequence rounds of this many windows: SequenceSegmenter '
                                                               'against reset() + T x update_from_feed() + label_confusion')
    ap.add_argument('--loader-grid', default=None, choices=tuple(LOADER_PRESETS),
                    help="(with --sequence) the round on a reference loader's grid against the composition of the older pieces; sets "
                         '--height, --width (the sensor) and --classes')
    ap.add_argument('--store', action='store_true', help='(with --sequence) rounds cut on the device out of an EventStore, '
                    'segment_at(samples=), against the ring-fed path on the same events: feed() of each label\'s events, then segment_at(end=)')
    a = ap.parse_args()
    if a.loader_grid and a.sequence is None:
        ap.error('--loader-grid belongs to --sequence')
    if a.loader_grid:
        (a.height, a.width), a.classes = LOADER_PRESETS[a.loader_grid]['sensor'], LOADER_PRESETS[a.loader_grid]['classes']
    if a.sequence is not None and (not a.streams or a.active or a.ingest or a.feed or a.sequence < 1):
        ap.error('--sequence T (T >= 1) needs --streams and excludes --active, --ingest and --feed')
    if a.feed and (not a.streams or a.active or a.ingest):
        ap.error('--feed needs --streams and excludes --active and --ingest')
    if a.voxel != 'temporal' and not a.feed:
        ap.error('--voxel belongs to --feed')
    if a.active and not a.streams:
        ap.error('--active needs --streams')
    if a.ingest and (not a.streams or a.active):
        ap.error('--ingest needs --streams and excludes --active')
    if a.display and (not a.streams or a.ingest or a.feed or a.sequence is not None):
        ap.error('--display needs --streams and excludes --ingest, --feed and --sequence')
    from ess_amd import hip
    from ess_amd.e2vid.model.model import E2VIDRecurrent
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.run_reconstruction import StreamingReconstructor, events_to_voxel_grid_device
    from ess_amd.models.style_networks import SemSegE2VID
    from ess_amd.run_segmentation import MultiStreamSegmenter, StreamingSegmenter
    cfg = dict(num_bins=a.bins, skip_type='sum', num_encoders=3, base_num_channels=32, num_residual_blocks=2, norm='BN',
               use_upsample_conv=True, recurrent_block_type=a.recurrent)
    g = np.random.default_rng(0)
    n = a.events
    wins = []
    for w in range(4):
        t = np.sort(g.uniform(0, 0.03, n)) + 0.03 * w
        wins.append(torch.from_numpy(np.stack([t, g.integers(0, a.width, n).astype(np.float64), g.integers(0, a.height, n).astype(np.float64),
                                               g.integers(0, 2, n).astype(np.float64)], 1)).cuda())
    dev = torch.device('cuda:0')
    out = {'shape': f'B=1 {a.bins}x{a.height}x{a.width} K={a.classes}', 'events_per_window': n, 'recurrent': a.recurrent,
           'windows': a.windows, 'warmup': a.warmup, 'reps': a.reps, 'ms_per_window': {}}

    def timed(step):
        for i in range(a.warmup):
            step(wins[i % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.windows):
            step(wins[i % 4])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.windows * 1e3

    if a.sequence is not None and a.loader_grid:
        sequence_loader_grid(a, hip, cfg, [w.cpu().numpy() for w in wins], out, E2VIDRecurrent, SemSegE2VID, default_options)
        print(json.dumps(out))
        return
    if a.sequence is not None and a.store:
        sequence_store(a, hip, cfg, [w.cpu().numpy() for w in wins], out, E2VIDRecurrent, SemSegE2VID, default_options)
        print(json.dumps(out))
        return
    if a.sequence is not None:
        sequence_rounds(a, hip, cfg, [w.cpu().numpy() for w in wins], out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, default_options)
        print(json.dumps(out))
        return
    if a.feed:
        from_packet_feed(a, hip, cfg, [w.cpu().numpy() for w in wins], out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, default_options)
        print(json.dumps(out))
        return
    if a.display:
        display_rounds(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, StreamingSegmenter, default_options)
        print(json.dumps(out))
        return
    if a.ingest:
        from_host_events(a, hip, cfg, [w.cpu().numpy() for w in wins], out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, default_options)
        print(json.dumps(out))
        return
    if a.streams:
        (partly_active if a.active else multi_stream)(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, StreamingSegmenter, default_options)
        print(json.dumps(out))
        return

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for mode in ('eager', 'graph'):
                torch.manual_seed(6)
                enc = E2VIDRecurrent(dict(cfg))
                dec = SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat')
                seg = StreamingSegmenter(enc, dec, a.height, a.width, default_options(), graph=mode == 'graph')
                torch.manual_seed(6)
                rec = StreamingReconstructor(E2VIDRecurrent(dict(cfg)), a.height, a.width, default_options(), graph=mode == 'graph')
                dec2 = SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat').cuda().eval()

                def composed(events):
                    grid = events_to_voxel_grid_device(events, a.bins, a.width, a.height, dev)
                    _, latent = rec.update(grid)
                    with torch.no_grad():
                        return hip.argmax_confusion(dec2(latent)[1], want_pred=True)

                ways = {'segmenter': seg.update_from_events, 'composed': composed}
                ms = {k: [] for k in ways}
                for _ in range(a.reps):  # alternating: drift of the box hits both ways alike
                    for k, fn in ways.items():
                        ms[k].append(timed(fn))
                for k, v in ms.items():
                    out['ms_per_window'][f'{compute}/{mode}/{k}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4),
                                                                     'max': round(max(v), 4)}
                del seg, rec
        finally:
            hip.set_compute('fp32')
    print(json.dumps(out))


def multi_stream(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, StreamingSegmenter, default_options):
    out['shape'] = f'S streams of {a.bins}x{a.height}x{a.width} K={a.classes}'
    del out['ms_per_window']
    out['ms_per_round'], out['windows_per_s'] = {}, {}

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat')

    def timed(step):  # a round: stream s gets window (i + s) % 4
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.windows):
            step(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.windows * 1e3

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                solos = [StreamingSegmenter(*models(), a.height, a.width, default_options(), graph=True) for _ in range(S)]
                multis = {mode: MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=mode == 'graph')
                          for mode in ('eager', 'graph')}

                def round_robin(i):
                    for s, seg in enumerate(solos):
                        seg.update_from_events(wins[(i + s) % 4])

                ways = {'round_robin/graph': round_robin}
                for mode, seg in multis.items():
                    ways[f'multi/{mode}'] = (lambda seg: lambda i: seg.update_from_events([wins[(i + s) % 4] for s in range(S)]))(seg)
                ms = {k: [] for k in ways}
                for _ in range(a.reps):  # alternating: drift of the box hits every way alike
                    for k, fn in ways.items():
                        ms[k].append(timed(fn))
                for k, v in ms.items():
                    med = statistics.median(v)
                    out['ms_per_round'][f'{compute}/S={S}/{k}'] = {'median': round(med, 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                    out['windows_per_s'][f'{compute}/S={S}/{k}'] = round(S / med * 1e3, 1)
                assert all(seg.n_captures == (1 if mode == 'graph' else 0) for mode, seg in multis.items())
                del solos, multis, ways
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


def partly_active(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, StreamingSegmenter, default_options):
    out['shape'] = f'k active of S streams of {a.bins}x{a.height}x{a.width} K={a.classes}'
    del out['ms_per_window']
    out['ms_per_round'], out['buckets'] = {}, {}
    buckets = None if a.buckets is None else [int(v) for v in a.buckets.split(',') if v]

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat')

    def timed(step):
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.windows):
            step(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.windows * 1e3

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                segs = {'ride_along': MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True),
                        'compact': MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, compact=True,
                                                        compact_buckets=None if buckets is None else [b for b in buckets if b < S])}
                for seg in segs.values():
                    seg.warm_up()
                out['buckets'][f'{compute}/S={S}'] = list(segs['compact'].buckets)
                captures = {k: seg.n_captures for k, seg in segs.items()}
                for k_active in (int(v) for v in a.active.split(',')):
                    if not 0 <= k_active <= S:
                        raise SystemExit(f'--active {k_active} of --streams {S}')

                    def events(i):  # stream s gets window (i + s) % 4, as in the all-active table
                        on = {(i + j) % S for j in range(k_active)}
                        return [wins[(i + s) % 4] if s in on else None for s in range(S)]
                    ways = {k: (lambda seg: lambda i: seg.update_from_events(events(i)))(seg) for k, seg in segs.items()}
                    ms = {k: [] for k in ways}
                    for _ in range(a.reps):  # alternating: drift of the box hits both ways alike
                        for k, fn in ways.items():
                            ms[k].append(timed(fn))
                    for k, v in ms.items():
                        out['ms_per_round'][f'{compute}/S={S}/active={k_active}/{k}'] = {
                            'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                assert captures == {k: seg.n_captures for k, seg in segs.items()}  # (no round in the timed regions paid a capture)
                del segs, ways
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


def display_rounds(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, StreamingSegmenter, default_options):
    from ess_amd.e2vid.image_reconstructor import PostProcessor
    out['shape'] = f'S streams of {a.bins}x{a.height}x{a.width} K={a.classes}, display rounds, graph replay, synchronised per round'
    del out['ms_per_window']
    out['ms_per_round'], out['recon_post_pair_us'], out['SLOWER'] = {}, {}, []
    alpha = 0.6
    palette = torch.from_numpy(np.random.default_rng(1).integers(0, 255, (a.classes, 3)).astype(np.uint8))
    shown = dict(reconstruct=True, postprocess=True, overlay=alpha, palette=palette)

    def options():  # auto-HDR on (filter size 10, the default): the frame costs its bounds step too
        o = default_options()
        o.auto_hdr = True
        return o

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat')

    def timed(step):  # every round from the call to the synchronised result
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.windows):
            step(i)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.windows * 1e3

    def measure(ways, key):
        ms = {k: [] for k in ways}
        for _ in range(a.reps):  # alternating: drift of the box hits every way alike
            for k, fn in ways.items():
                ms[k].append(timed(fn))
        for k, v in ms.items():
            out['ms_per_round'][f'{key}/{k}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
        return {k: statistics.median(v) for k, v in ms.items()}

    def pair_us(S, options):
        """the bounds + frame launches alone, device time per pair over 200 launches"""
        post = {k: PostProcessor(torch.device('cuda:0'), options, n=S) for k in ('unsteered', 'steered_all', 'steered_1')}
        img = torch.rand(S, 1, a.height, a.width, device='cuda')
        mode = {'unsteered': None, 'steered_all': torch.full((S,), hip.CARRY_TAKE, dtype=torch.int32, device='cuda'),
                'steered_1': torch.tensor([hip.CARRY_TAKE] + [hip.CARRY_HOLD] * (S - 1), dtype=torch.int32, device='cuda')}
        us = {k: [] for k in post}
        for _ in range(a.reps):
            for k, p in post.items():
                for _ in range(20):
                    p.process_u8(img, mode=mode[k])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    p.process_u8(img, mode=mode[k])
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / 200)
        return {k: {'median': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)} for k, v in us.items()}

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                key = f'{compute}/S={S}'
                if not a.active:
                    multis = {'plain': MultiStreamSegmenter(*models(), a.height, a.width, options(), S, graph=True),
                              'image': MultiStreamSegmenter(*models(), a.height, a.width, options(), S, graph=True, reconstruct=True),
                              'display': MultiStreamSegmenter(*models(), a.height, a.width, options(), S, graph=True, **shown)}
                    solos = [StreamingSegmenter(*models(), a.height, a.width, options(), graph=True, **shown) for _ in range(S)]

                    def round_robin(i):
                        for s, seg in enumerate(solos):
                            seg.update_from_events(wins[(i + s) % 4])
                    ways = {k: (lambda seg: lambda i: seg.update_from_events([wins[(i + s) % 4] for s in range(S)]))(seg)
                            for k, seg in multis.items()}
                    ways['round_robin'] = round_robin
                    med = measure(ways, key)
                    if med['display'] > med['round_robin']:
                        out['SLOWER'].append(f'{key}: display round {med["display"]:.3f} ms against round-robin {med["round_robin"]:.3f} ms')
                    assert all(seg.n_captures == 1 for seg in multis.values())
                    del solos, multis, ways
                else:
                    segs = {'ride_along': MultiStreamSegmenter(*models(), a.height, a.width, options(), S, graph=True, **shown),
                            'compact': MultiStreamSegmenter(*models(), a.height, a.width, options(), S, graph=True, compact=True, **shown)}
                    for seg in segs.values():
                        seg.warm_up()
                    captures = {k: seg.n_captures for k, seg in segs.items()}
                    for k_active in (int(v) for v in a.active.split(',')):
                        if not 0 <= k_active <= S:
                            raise SystemExit(f'--active {k_active} of --streams {S}')

                        def events(i):
                            on = {(i + j) % S for j in range(k_active)}
                            return [wins[(i + s) % 4] if s in on else None for s in range(S)]
                        ways = {k: (lambda seg: lambda i: seg.update_from_events(events(i)))(seg) for k, seg in segs.items()}
                        med = measure(ways, f'{key}/active={k_active}')
                        if med['compact'] > med['ride_along']:
                            out['SLOWER'].append(f'{key}/active={k_active}: compact {med["compact"]:.3f} ms against ride-along {med["ride_along"]:.3f} ms')
                    assert captures == {k: seg.n_captures for k, seg in segs.items()}  # (no round in the timed regions paid a capture)
                    del segs, ways
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')
    for S in (int(v) for v in a.streams.split(',')):
        us = pair_us(S, options())
        out['recon_post_pair_us'][f'N={S}'] = us
        for k in ('steered_all', 'steered_1'):
            if us[k]['median'] > us['unsteered']['median']:
                out['SLOWER'].append(f'N={S}: {k} pair {us[k]["median"]} us against unsteered {us["unsteered"]["median"]} us')


def from_host_events(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, default_options):
    from ess_amd.datasets.data_util import EventColumns, pack_event_records, stage_event_columns
    out['shape'] = f'S streams of {a.bins}x{a.height}x{a.width} K={a.classes}, rounds from host event arrays, graph replay'
    del out['ms_per_window']
    out['ms_per_round'], out['parent_spread_ms'], out['ingest_wins_by_more_than_parent_spread'] = {}, {}, {}
    out['columns'] = {}
    # the same events as a DSEC file delivers them: t int64 microseconds, x / y uint16, p uint8.  The rows' times become those
    # microseconds (as float64) too, so that all three ways are fed the same events.
    cols = []
    for w in wins:
        us = np.round(w[:, 0] * 1e6).astype(np.int64)
        w[:, 0] = us
        cols.append(EventColumns(us, w[:, 1].astype(np.uint16), w[:, 2].astype(np.uint16), w[:, 3].astype(np.uint8)))

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat')

    def timed(step):  # a round: stream s gets window (i + s) % 4; every round synchronised -> the median round of the repetition
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        ms = []
        for i in range(a.windows):
            t0 = time.perf_counter()
            step(i)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                segs = {'parent': MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True),
                        'ingest': MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, event_capacity=a.events),
                        'columns': MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, event_capacity=a.events,
                                                        event_layout='columns')}
                ways = {k: (lambda seg, src: lambda i: seg.update_from_events([src[(i + s) % 4] for s in range(S)]))(seg, cols if k == 'columns' else wins)
                        for k, seg in segs.items()}
                same = [ways[k](0).labels.clone() for k in ('ingest', 'columns')]  # (both from a zero state: the same events, the same labels)
                assert torch.equal(*same)
                for seg in segs.values():
                    seg.reset()
                staging = np.zeros((S, a.events), dtype=hip.EVENT_RECORD)

                def pack_only(i):
                    for s in range(S):
                        pack_event_records(wins[(i + s) % 4], staging[s])
                ways['host_packing_alone'] = pack_only
                stride = hip.event_column_stride(a.events)
                col_staging = [np.zeros((S, stride), d) for d in (np.int64, np.int16, np.int16, np.uint8)]

                def stage_only(i):
                    for s in range(S):
                        stage_event_columns(cols[(i + s) % 4], *(c[s] for c in col_staging))
                ways['host_column_staging_alone'] = stage_only
                ms = {k: [] for k in ways}
                for _ in range(a.reps):  # alternating: drift of the box hits both ways alike
                    for k, fn in ways.items():
                        ms[k].append(timed(fn))
                key = f'{compute}/S={S}'
                for k, v in ms.items():
                    out['ms_per_round'][f'{key}/{k}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                spread = max(ms['parent']) - min(ms['parent'])
                out['parent_spread_ms'][key] = round(spread, 4)
                out['ingest_wins_by_more_than_parent_spread'][key] = bool(statistics.median(ms['parent']) - statistics.median(ms['ingest']) > spread)
                m = {k: statistics.median(v) for k, v in ms.items()}
                saved, owed = m['ingest'] - m['columns'], m['host_packing_alone'] - m['host_column_staging_alone']
                out['columns'][key] = {'records_minus_columns_ms': round(saved, 4), 'packing_minus_staging_ms': round(owed, 4),
                                       'below_records_by_at_least_packing_minus_staging': bool(saved >= owed),
                                       'parent_minus_columns_ms': round(m['parent'] - m['columns'], 4),
                                       'columns_wins_over_parent_by_more_than_parent_spread': bool(m['parent'] - m['columns'] > spread)}
                assert all(seg.n_captures == 1 for seg in segs.values())
                del segs, ways
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


def from_packet_feed(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, default_options):
    from ess_amd.datasets.data_util import EventColumns
    out['shape'] = f'S streams of {a.bins}x{a.height}x{a.width} K={a.classes}, rounds from a packet feed, graph replay'
    del out['ms_per_window']
    out['ms_per_round'], out['columns_minus_ring_ms'], out['ring_wins_by_more_than_columns_spread'] = {}, {}, {}
    N = a.events
    packet = max(N // 10, 1)
    out['packet_events'] = packet
    rounds = a.warmup + a.windows
    tri = a.voxel == 'trilinear'
    out['voxel'] = a.voxel
    if tri:  # two smooth distortions of the sensor by a few pixels (some events pushed over the border), as float32 [H, W, 2]
        out['trilinear_ring_minus_temporal_ring_ms'], out['trilinear_ring_SLOWER_than_temporal_ring'] = {}, {}
        out['host_minus_trilinear_ring_ms'], out['trilinear_ring_SLOWER_than_host'] = {}, {}
        yy, xx = np.meshgrid(np.arange(a.height, dtype=np.float64), np.arange(a.width, dtype=np.float64), indexing='ij')
        rectify = [np.stack([xx + amp * np.sin(yy / 40.0), yy + amp * np.cos(xx / 50.0)], -1).astype(np.float32) for amp in (3.0, -2.0)]

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, a.classes, skip_connect=True, skip_type='concat')

    def source(total):
        """one long sequence in DSEC's dtypes (t int64 microseconds, x / y uint16, p uint8): the four windows over and over, the times
        running on"""
        reps = -(-total // (4 * N))
        base = np.concatenate(wins)
        us = np.round(base[:, 0] * 1e6).astype(np.int64)
        period = int(us[-1] - us[0]) + 1
        t = np.concatenate([us + r * period for r in range(reps)])[:total]
        x, y, p = (np.tile(base[:, k].astype(d), reps)[:total] for k, d in ((1, np.uint16), (2, np.uint16), (3, np.uint8)))
        return t, x, y, p

    def piece(src, lo, hi):
        return EventColumns(*(np.ascontiguousarray(c[lo:hi]) for c in src))

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                for M in (N, max(N // 4, 1)):
                    shift = 1237  # (stream s reads the sequence from event s * shift on: the streams' windows differ)
                    src = source(N + M * rounds + packet + S * shift)
                    rig = [rectify[s % 2] for s in range(S)] if tri else None
                    flavour = dict(voxel='trilinear', rectify_maps=rig) if tri else {}
                    ring = MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, event_capacity=N,
                                                event_layout='ring', window_events=N, window_stride=M, **flavour)
                    cols = MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, event_capacity=N,
                                                event_layout='columns', **flavour)
                    ms = {'ring': [], 'columns': []}
                    if tri:
                        ring_t = MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, event_capacity=N,
                                                      event_layout='ring', window_events=N, window_stride=M)
                        host_seg = MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True)
                        offs = [i * N for i in range(S + 1)]
                        ms.update(ring_temporal=[], host=[])
                    fed, k = 0, 0
                    while k < rounds:
                        last = fed + packet >= k * M + N  # this packet completes window k of every stream
                        pk = [piece(src, s * shift + fed, s * shift + fed + packet) for s in range(S)]
                        if not last:
                            for s in range(S):
                                ring.feed(s, pk[s])
                                if tri:
                                    ring_t.feed(s, pk[s])
                            fed += packet
                            torch.cuda.synchronize()  # (the packet arrived long before the next one: its upload is over)
                            continue
                        window = [piece(src, s * shift + k * M, s * shift + k * M + N) for s in range(S)]
                        def by_ring():
                            for s in range(S):
                                ring.feed(s, pk[s])
                            return ring.update_from_feed()

                        def by_columns():
                            return cols.update_from_events(window)

                        def by_ring_temporal():
                            for s in range(S):
                                ring_t.feed(s, pk[s])
                            return ring_t.update_from_feed()

                        def by_host():
                            cols4 = [[], [], [], []]
                            for s, w in enumerate(window):
                                xy = rig[s][w.y, w.x]
                                d = (w.t - w.t[0]).astype(np.float32)
                                for c, v in zip(cols4, (xy[:, 0], xy[:, 1], w.p.astype(np.float32), d / d[-1])):
                                    c.append(v)
                            dev4 = [torch.from_numpy(np.concatenate(c)).cuda(non_blocking=True) for c in cols4]
                            return host_seg.update(hip.voxel_grid_trilinear(*dev4, offs, a.bins, a.height, a.width))
                        res, took = {}, {}
                        order = [('ring', by_ring), ('columns', by_columns)] + ([('ring_temporal', by_ring_temporal), ('host', by_host)] if tri else [])
                        order = order[::1 if k % 2 == 0 else -1]  # (who goes first alternates)
                        for way, fn in order:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            res[way] = fn()
                            torch.cuda.synchronize()
                            took[way] = (time.perf_counter() - t0) * 1e3
                        got, want = res['ring'], res['columns']
                        fed += packet
                        assert got.valid == want.valid == (True,) * S and ring.pending(0) == 0
                        if k == 0:  # (both from a zero state: the same windows, the same labels)
                            assert torch.equal(got.labels, want.labels)
                        if k >= a.warmup:
                            for way in ms:
                                ms[way].append(took[way])
                        k += 1
                    key = f'{compute}/S={S}/stride={"window" if M == N else "window/4"}'
                    for way, v in ms.items():
                        out['ms_per_round'][f'{key}/{way}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4),
                                                               'max': round(max(v), 4), 'p90': round(sorted(v)[int(0.9 * (len(v) - 1))], 4)}
                    diff = statistics.median(ms['columns']) - statistics.median(ms['ring'])
                    q = sorted(ms['columns'])
                    spread = q[int(0.75 * (len(q) - 1))] - q[int(0.25 * (len(q) - 1))]
                    out['columns_minus_ring_ms'][key] = round(diff, 4)
                    out['ring_wins_by_more_than_columns_spread'][key] = bool(diff > spread)
                    if tri:
                        spread_r = sorted(ms['ring'])
                        spread_r = spread_r[int(0.75 * (len(spread_r) - 1))] - spread_r[int(0.25 * (len(spread_r) - 1))]
                        d_t = statistics.median(ms['ring']) - statistics.median(ms['ring_temporal'])
                        d_h = statistics.median(ms['host']) - statistics.median(ms['ring'])
                        out['trilinear_ring_minus_temporal_ring_ms'][key] = round(d_t, 4)
                        out['trilinear_ring_SLOWER_than_temporal_ring'][key] = bool(d_t > spread_r)
                        out['host_minus_trilinear_ring_ms'][key] = round(d_h, 4)
                        out['trilinear_ring_SLOWER_than_host'][key] = bool(-d_h > spread_r)
                        assert ring_t.n_captures == host_seg.n_captures == 1
                        del ring_t, host_seg
                    assert ring.n_captures == cols.n_captures == 1
                    del ring, cols, src
                    torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


# the reference loaders' grids (SequenceSegmenter's docstring): the sensor's size, the network's, the classes, the keywords
LOADER_PRESETS = {
    'ddd17': dict(sensor=(260, 346), net=(200, 352), classes=6,
                  kw=dict(voxel='temporal', grid_hw=(260, 346), grid_resize=(260, 352), grid_normalize='population')),
    'dsec': dict(sensor=(480, 640), net=(448, 640), classes=11,
                 kw=dict(voxel='trilinear', grid_hw=(480, 640), grid_rows=440, grid_resize=(448, 640), grid_normalize='unbiased')),
}


def sequence_loader_grid(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, default_options):
    import torch.nn.functional as F
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    preset = LOADER_PRESETS[a.loader_grid]
    (Hs, Ws), (Hn, Wn), T, N, K = preset['sensor'], preset['net'], a.sequence, a.events, a.classes
    out['shape'] = f'S streams, events voxelised at {a.bins}x{Hs}x{Ws} -> the loader grid {a.bins}x{Hn}x{Wn} ({a.loader_grid}) K={K}, ' \
                   f'sequence rounds of T={T} windows, graph replay'
    del out['ms_per_window']
    out['ms_per_round'], out['composed_minus_loader_grid_ms'], out['loader_grid_SLOWER_than_composed'] = {}, {}, {}
    out['labels_equal_fraction'] = {}
    rounds = a.warmup + a.windows
    dev = torch.device('cuda:0')
    base = np.concatenate(wins)
    us = np.round(base[:, 0] * 1e6).astype(np.int64)
    period = int(us[-1] - us[0]) + 1

    def piece(lo, hi):
        idx = np.arange(lo, hi)
        r, k = idx // len(us), idx % len(us)
        return EventColumns(us[k] + r * period, base[k, 1].astype(np.uint16), base[k, 2].astype(np.uint16), base[k, 3].astype(np.uint8))

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                torch.manual_seed(6)
                seq = SequenceSegmenter(E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, K, skip_connect=True, skip_type='concat'), Hn, Wn,
                                        default_options(), S, sequence_steps=T, window_events=N, graph=True, **preset['kw'])
                crop_rows, (Hr, Wr), norm = seq._grid
                big = torch.empty(T * S, a.bins, Hs, Ws, device=dev)
                acc_big = torch.zeros(T * S, a.bins, Hs, Ws, dtype=torch.int64, device=dev)

                def composed_round():
                    tri = seq.voxel == 'trilinear'
                    hip.event_voxels('ring', seq._ring, seq._words[:4], big, acc_big, trilinear=tri, maps=seq._maps,
                                     map_of=seq._words[4] if tri else None)
                    hip.voxel_normalize_(big, 0 if norm == hip.GRID_NORM_UNBIASED else 1)
                    ev = F.interpolate(big[:, :, :crop_rows], size=(Hr, Wr), mode='bilinear', align_corners=True)[:, :, :Hn].contiguous()
                    return seq._round_from(ev)
                g = torch.Generator().manual_seed(1)
                gt = torch.randint(0, K, (S, Hn, Wn), generator=g, dtype=torch.uint8).to(dev)
                shift, ms, fed, same = 1237, {'loader_grid': [], 'composed': []}, 0, []
                graph = None
                for k in range(rounds):
                    for s in range(S):  # the T windows of this round arrive: outside the clock
                        for lo in range(fed, fed + T * N, N):
                            seq.feed(s, piece(s * shift + lo, s * shift + lo + N))
                    fed += T * N
                    torch.cuda.synchronize()
                    if graph is None:  # a priming round captures the segmenter's graph and leaves slot words for the composed capture
                        seq.segment_at(end=[fed] * S, labels=list(gt))
                        side = torch.cuda.Stream()
                        side.wait_stream(torch.cuda.current_stream())
                        with torch.cuda.stream(side):
                            composed_round()
                        torch.cuda.current_stream().wait_stream(side)
                        torch.cuda.synchronize()
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph):
                            composed_out = composed_round()

                    def by_loader_grid():
                        return seq.segment_at(end=[fed] * S, labels=list(gt)).labels

                    def by_composed():
                        graph.replay()
                        return composed_out[0].clone()
                    took, res = {}, {}
                    for way, fn in [('loader_grid', by_loader_grid), ('composed', by_composed)][::1 if k % 2 == 0 else -1]:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res[way] = fn()
                        torch.cuda.synchronize()
                        took[way] = (time.perf_counter() - t0) * 1e3
                    if k >= a.warmup:
                        for way in ms:
                            ms[way].append(took[way])
                        if k % 2 == 0:  # (the composed way read this round's slot words)
                            same.append(float((res['loader_grid'] == res['composed']).float().mean()))
                key = f'{compute}/S={S}/T={T}'
                for way, v in ms.items():
                    out['ms_per_round'][f'{key}/{way}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                spread = max(max(v) - min(v) for v in ms.values())
                diff = statistics.median(ms['composed']) - statistics.median(ms['loader_grid'])
                out['composed_minus_loader_grid_ms'][key] = round(diff, 4)
                out['loader_grid_SLOWER_than_composed'][key] = bool(diff < 0)
                out.setdefault('spread_ms', {})[key] = round(spread, 4)
                out['labels_equal_fraction'][key] = round(min(same), 6) if same else None
                assert seq.n_captures == 1 and not bool(seq._acc.any()) and not bool(acc_big.any())
                del seq, big, acc_big, graph
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


def sequence_store(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, default_options):
    """--sequence T --store: consecutive labels of S recordings, each label's sequence overlapping the one before by 50 %.  The store
    way: the recordings lie in an EventStore (uploaded once, outside the clock), a round is segment_at(samples=[StoreSample(s, end=e)])
    to synchronised labels.  The ring-fed ways, the parent's path on the same events, inside the clock: 'ring_feed_new_half' -- feed()
    of the T N / 2 events a lane has not been fed yet, then segment_at(end=) -- and 'ring_refeed_sample' -- drop_feed(), feed() of the
    label's whole T N events, segment_at(end=), what scoring labels in any order costs.  The ways alternate inside every round."""
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.event_store import EventStore, StoreSample
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    T, N, K = a.sequence, a.events, a.classes
    out['shape'] = f'S lanes of {a.bins}x{a.height}x{a.width} K={K}, sequence rounds of T={T} windows of {N} events, graph replay, labels overlap 50 %'
    del out['ms_per_window']
    out['ms_per_round'], out['ring_minus_store_ms'], out['store_SLOWER_than_ring'] = {}, {}, {}
    rounds = a.warmup + a.windows
    dev = torch.device('cuda:0')
    half = T * N // 2
    length = T * N + rounds * half

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, K, skip_connect=True, skip_type='concat')

    base = np.concatenate(wins)
    us = np.round(base[:, 0] * 1e6).astype(np.int64)
    period = int(us[-1] - us[0]) + 1

    def piece(lo, hi):
        idx = np.arange(lo, hi)
        r, k = idx // len(us), idx % len(us)
        return EventColumns(us[k] + r * period, base[k, 1].astype(np.uint16), base[k, 2].astype(np.uint16), base[k, 3].astype(np.uint8))

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                recs = [piece(s * 1237, s * 1237 + length) for s in range(S)]
                store = EventStore(S * length)
                for c in recs:
                    store.add_recording(c)
                by_store = SequenceSegmenter(*models(), a.height, a.width, default_options(), S, sequence_steps=T, window_events=N, graph=True,
                                             store=store)
                rings = {w: SequenceSegmenter(*models(), a.height, a.width, default_options(), S, sequence_steps=T, window_events=N, graph=True)
                         for w in ('ring_feed_new_half', 'ring_refeed_sample')}
                g = torch.Generator().manual_seed(1)
                gt = list(torch.randint(0, K, (S, a.height, a.width), generator=g, dtype=torch.uint8).to(dev))
                cut = lambda c, lo, hi: EventColumns(c.t[lo:hi], c.x[lo:hi], c.y[lo:hi], c.p[lo:hi])  # noqa: E731
                for s in range(S):  # the first label's older half is there already
                    rings['ring_feed_new_half'].feed(s, cut(recs[s], 0, T * N - half))
                ms = {'store': [], 'ring_feed_new_half': [], 'ring_refeed_sample': []}
                same = True
                for k in range(rounds):
                    end = T * N + k * half

                    def store_round():
                        return by_store.segment_at(samples=[StoreSample(s, end=end) for s in range(S)], labels=gt).labels

                    def new_half_round():
                        seg = rings['ring_feed_new_half']
                        for s in range(S):
                            seg.feed(s, cut(recs[s], end - half, end))
                        return seg.segment_at(end=[end] * S, labels=gt).labels

                    def refeed_round():
                        seg = rings['ring_refeed_sample']
                        seg.drop_feed()
                        for s in range(S):
                            seg.feed(s, cut(recs[s], end - T * N, end))
                        return seg.segment_at(end=[T * N] * S, labels=gt).labels
                    ways = [('store', store_round), ('ring_feed_new_half', new_half_round), ('ring_refeed_sample', refeed_round)]
                    took, res = {}, {}
                    for way, fn in ways[k % 3:] + ways[:k % 3]:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res[way] = fn()
                        torch.cuda.synchronize()
                        took[way] = (time.perf_counter() - t0) * 1e3
                    same = same and all(torch.equal(res['store'], res[w]) for w in rings)
                    if k >= a.warmup:
                        for way in ms:
                            ms[way].append(took[way])
                key = f'{compute}/S={S}/T={T}'
                for way, v in ms.items():
                    out['ms_per_round'][f'{key}/{way}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                out.setdefault('same_labels', {})[key] = bool(same)
                out.setdefault('same_confusion', {})[key] = bool(all(torch.equal(by_store.confusion, r.confusion) for r in rings.values()))
                for way in rings:
                    diff = statistics.median(ms[way]) - statistics.median(ms['store'])
                    out['ring_minus_store_ms'][f'{key}/{way}'] = round(diff, 4)
                    out['store_SLOWER_than_ring'][f'{key}/{way}'] = bool(diff < 0)
                    out.setdefault('ring_spread_ms', {})[f'{key}/{way}'] = round(max(ms[way]) - min(ms[way]), 4)
                out.setdefault('store_bytes', {})[key] = store.bytes()
                assert by_store.n_captures == 1 and all(r.n_captures == 1 for r in rings.values())
                del by_store, rings, store
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


def sequence_rounds(a, hip, cfg, wins, out, E2VIDRecurrent, SemSegE2VID, MultiStreamSegmenter, default_options):
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    T, N, K = a.sequence, a.events, a.classes
    out['shape'] = f'S streams of {a.bins}x{a.height}x{a.width} K={K}, sequence rounds of T={T} windows, graph replay'
    del out['ms_per_window']
    out['ms_per_round'], out['composed_minus_sequence_ms'], out['sequence_SLOWER_than_composed'] = {}, {}, {}
    out['head_ms'], out['head_eval_SLOWER_than_head_plus_label_confusion'] = {}, {}
    rounds = a.warmup + a.windows
    dev = torch.device('cuda:0')

    def models():
        torch.manual_seed(6)
        return E2VIDRecurrent(dict(cfg)), SemSegE2VID(256, K, skip_connect=True, skip_type='concat')

    base = np.concatenate(wins)
    us = np.round(base[:, 0] * 1e6).astype(np.int64)
    period = int(us[-1] - us[0]) + 1

    def piece(lo, hi):
        """events [lo, hi) of the endless sequence made of the four windows over and over, in DSEC's dtypes"""
        idx = np.arange(lo, hi)
        r, k = idx // len(us), idx % len(us)
        return EventColumns(us[k] + r * period, base[k, 1].astype(np.uint16), base[k, 2].astype(np.uint16), base[k, 3].astype(np.uint8))

    for compute in a.compute.split(','):
        hip.set_compute(compute)
        try:
            for S in (int(v) for v in a.streams.split(',')):
                seq = SequenceSegmenter(*models(), a.height, a.width, default_options(), S, sequence_steps=T, window_events=N, graph=True)
                R = seq.ring_capacity
                multi = MultiStreamSegmenter(*models(), a.height, a.width, default_options(), S, graph=True, event_capacity=N,
                                             event_layout='ring', window_events=N, ring_capacity=R)
                g = torch.Generator().manual_seed(1)
                gt = torch.randint(0, K, (S, a.height, a.width), generator=g, dtype=torch.uint8).to(dev)
                gt64 = gt.long()
                conf = torch.zeros(S, K, K, dtype=torch.int64, device=dev)
                shift, ms, fed = 1237, {'sequence': [], 'composed': []}, 0
                for k in range(rounds):
                    for s in range(S):  # the T windows of this round arrive: outside the clock, as in a replay farm
                        for lo in range(fed, fed + T * N, N):
                            pk = piece(s * shift + lo, s * shift + lo + N)
                            seq.feed(s, pk)
                            multi.feed(s, pk)
                    fed += T * N
                    torch.cuda.synchronize()

                    def by_sequence():
                        return seq.segment_at(end=[fed] * S, labels=list(gt)).labels

                    def by_composed():
                        multi.reset()
                        for _ in range(T):
                            res = multi.update_from_feed()
                        lab = res.labels.long()
                        for s in range(S):
                            hip.label_confusion(lab[s], gt64[s], conf[s])
                        return res.labels
                    took, res = {}, {}
                    for way, fn in [('sequence', by_sequence), ('composed', by_composed)][::1 if k % 2 == 0 else -1]:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        res[way] = fn()
                        torch.cuda.synchronize()
                        took[way] = (time.perf_counter() - t0) * 1e3
                    assert multi.pending(0) == 0
                    if k >= a.warmup:
                        for way in ms:
                            ms[way].append(took[way])
                key = f'{compute}/S={S}/T={T}'
                for way, v in ms.items():
                    out['ms_per_round'][f'{key}/{way}'] = {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}
                q = sorted(ms['composed'])
                spread = q[-1] - q[0]
                diff = statistics.median(ms['composed']) - statistics.median(ms['sequence'])
                out['composed_minus_sequence_ms'][key] = round(diff, 4)
                out['sequence_SLOWER_than_composed'][key] = bool(diff < 0)
                out.setdefault('composed_spread_ms', {})[key] = round(spread, 4)
                assert seq.n_captures == multi.n_captures == 1
                # the class head alone, on an activation of the decoder's last width in the configuration's operand format
                C = seq.decoder.decoder_scale_5[0].weight.shape[1]
                c5 = seq.decoder.decoder_scale_5[0]
                x = torch.randn(S, C, a.height, a.width, device=dev).relu()
                x = hip.to_f16_c8(x) if compute == 'mixed' else hip.to_bf16_c8(x) if compute == 'bf16' else x
                cm = torch.zeros(S, K, K, dtype=torch.int64, device=dev)

                def head_eval():
                    hip.seg_head_eval(x, C, c5.weight, c5.bias, gt, cm)

                def head_then_confusion():
                    lab = hip.seg_head(x, C, c5.weight, c5.bias)[0].long()
                    for s in range(S):
                        hip.label_confusion(lab[s], gt64[s], conf[s])
                hm = {}
                for way, fn in (('seg_head_eval', head_eval), ('seg_head+label_confusion', head_then_confusion)) * 2:
                    for _ in range(5):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(50):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    hm.setdefault(way, []).append(e0.elapsed_time(e1) / 50)
                out['head_ms'][f'{compute}/S={S}'] = {way: [round(v, 4) for v in vs] for way, vs in hm.items()}
                out['head_eval_SLOWER_than_head_plus_label_confusion'][f'{compute}/S={S}'] = bool(min(hm['seg_head_eval']) > min(hm['seg_head+label_confusion']))
                del seq, multi
                torch.cuda.empty_cache()
        finally:
            hip.set_compute('fp32')


if __name__ == '__main__':
    main()
