"""Times the device image store at the Cityscapes size (1024 x 2048 RGB -> 256 x 512), --rounds runs of each figure:

    ingest_launches      hip.image_ingest on a frame that is on the device already (gray + horizontal pass, vertical pass + min / max,
                         the label's gather; with --standardization the stretch too): device events around --reps calls
    ingest_with_upload   ImageStore.add_images, one frame and label a call: pinned staging, the upload, the launches; host clock to a
                         device synchronise, per frame
    build_eager / build_graph   ImageBatchBuilder.build at --batch to synchronised tensors
    composed             the composition it replaces on the same device: index_select of the slots + .float() / .long() + the two-stage
                         entry points through DeviceAugmentation (which draws and uploads its own parameter rows)
    pil_host             where PIL imports: convert('L'), the two resizes, the float upload, per frame; else a line saying PIL is absent

The ways alternate.  Every figure is ms, median (min - max) over the rounds; one JSON line per figure.  Before anything is timed a
slot of the store is compared with PIL itself, where it imports (slot_equals_pil in the first line).

    python tools/bench_image_batch.py [--batch 8] [--height 200 --width 352] [--rounds 2] [--batches 64] [--standardization]

--frames (without a number) times the PAIRED CAMERA FRAMES of the event loaders instead, at both their sizes -- DSEC 480 x 640 RGB ->
448 x 640, DDD17 260 x 346 -> 260 x 352 (the top 200 rows kept):

    frame_ingest_launches      hip.image_ingest_frame on a frame that is on the device already (bicubic, gray last)
    frame_ingest_with_upload   ImageStore.add_images on a frame store, one frame a call
    pil_host                   Image.fromarray(f).resize((Wr, Hr)).convert('L'), / 255 and the float upload, per frame
    batch_with_frames / batch_without_frames   EventBatchBuilder(graph=True, augmentation=False) at --batch over a synthetic event store
                               (5 windows of 20000 events a sample) with frames= and without it

    python tools/bench_image_batch.py --frames [--batch 8] [--rounds 2] [--batches 64]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ess_amd import hip  # noqa: E402
from ess_amd.datasets.augment import DeviceAugmentation  # noqa: E402
from ess_amd.datasets.image_store import ImageBatchBuilder, ImageStore, cityscapes_id_lut  # noqa: E402


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def paired_frames(a):
    """--frames without a number: the paired camera frames of the two event loaders (module docstring)"""
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.event_batches import EventBatchBuilder
    from ess_amd.datasets.event_store import EventStore, StoreSample
    dev = torch.device('cuda:0')
    try:
        from PIL import Image
    except ImportError:
        Image = None
    B, T, n_win = a.batch, 5, 20000
    rng = np.random.default_rng(0)
    for name, shape, (Hr, Wr), keep, label_hw in (('dsec', (480, 640, 3), (448, 640), None, (440, 640)), ('ddd17', (260, 346), (260, 352), 200, (200, 346))):
        H, W = shape[:2]
        frames = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(4)]
        timed = a.rounds * a.upload_frames
        make = ImageStore.dsec_frames if name == 'dsec' else ImageStore.ddd17_frames
        store = make(B + timed)
        store.add_images([frames[k % 4] for k in range(B)])
        head = dict(frames=name, source=list(shape), resize=[Hr, Wr], keep_rows=keep, batch=B, sequence_steps=T, window_events=n_win,
                    store_bytes=store.bytes(), pil=None if Image is None else Image.__version__)

        def pil_frame(f):
            r = Image.fromarray(f).resize((Wr, Hr))
            return np.array(r.convert('L') if f.ndim == 3 else r)[:keep]
        if Image is not None:
            head['slot_equals_pil'] = bool(np.array_equal(store.images[1].cpu().numpy(), pil_frame(frames[1])))
        print(json.dumps(head), flush=True)
        d = store._device()
        tabs = d['tables']
        frame_dev, slot = torch.from_numpy(frames[0]).to(dev), torch.zeros_like(store.images[0])
        n_added = [0]
        scratch = d['scratch'] if len(shape) == 3 else d['scratch'].view(-1)[:H * Wr].view(H, Wr)  # (a gray frame's pass leaves one channel)

        def launches():
            hip.image_ingest_frame(frame_dev, slot, tabs['h'], tabs['v'], scratch, resized_rows=Hr)

        def with_upload():
            n_added[0] += 1
            store.add_images([frames[n_added[0] % 4]])

        def pil_host():
            return torch.from_numpy(pil_frame(frames[0])).float().div(255).to(dev)
        n = B * T * n_win + 1000
        events = EventStore(n, label_hw=label_hw, label_capacity=B)
        cols = EventColumns(np.cumsum(rng.integers(0, 3, n)).astype(np.int64), rng.integers(0, W, n).astype(np.int16),
                            rng.integers(0, H, n).astype(np.int16), rng.integers(0, 2, n).astype(np.uint8))
        events.add_recording(cols, labels=rng.integers(0, 6, (B,) + label_hw, dtype=np.uint8))
        samples = [StoreSample(0, end=(b + 1) * T * n_win, label=b, frame=b) for b in range(B)]
        common = dict(sequence_steps=T, store=events, window_events=n_win, graph=True, augmentation=False)
        preset = getattr(EventBatchBuilder, name)
        with_frames, without = preset(B, frames=store, **common), preset(B, **common)
        ways = {
            'frame_ingest_launches': lambda: device_ms(launches, a.reps),
            'frame_ingest_with_upload': lambda: statistics.mean(host_ms(with_upload) for _ in range(a.upload_frames)),
            'batch_with_frames': lambda: statistics.mean(host_ms(lambda: with_frames.build(samples)) for _ in range(a.batches)),
            'batch_without_frames': lambda: statistics.mean(host_ms(lambda: without.build(samples)) for _ in range(a.batches)),
        }
        if Image is not None:
            ways['pil_host'] = lambda: statistics.mean(host_ms(pil_host) for _ in range(16))
        else:
            print(json.dumps(dict(frames=name, way='pil_host', note='PIL is absent on this machine: the host path is not measured')), flush=True)
        for _ in range(3):  # (the warm-up of every shape that is timed, and the captures)
            launches(), with_frames.build(samples), without.build(samples)
            if Image is not None:
                pil_host()
        torch.cuda.synchronize()
        times = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                times[k].append(fn())
        unit = {'frame_ingest_launches': f'ms per frame, device events, {a.reps} calls'}
        for k, v in times.items():
            per = f'ms per batch of {B}' if k.startswith('batch') else 'ms per frame'
            print(json.dumps(dict(frames=name, way=k, ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                                  clock=unit.get(k, f'{per}, host clock to a device synchronise'))), flush=True)
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = max(times['batch_without_frames']) - min(times['batch_without_frames'])
        verdict = dict(frames=name, batch_spread_ms=round(spread, 3), frames_cost_ms=round(med['batch_with_frames'] - med['batch_without_frames'], 3))
        verdict['batch_with_frames_SLOWER'] = bool(med['batch_with_frames'] - med['batch_without_frames'] > spread)
        if Image is not None:
            verdict['frame_ingest_with_upload_SLOWER_than_pil_host'] = bool(med['frame_ingest_with_upload'] > med['pil_host'])
        print(json.dumps(verdict), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--source', type=int, nargs=2, default=(1024, 2048))
    ap.add_argument('--resize', type=int, nargs=2, default=(256, 512))
    ap.add_argument('--height', type=int, default=200)
    ap.add_argument('--width', type=int, default=352)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, nargs='?', const=-1, default=16,
                    help='with a number: frames the store holds for the batches; without one: time the paired camera frames instead')
    ap.add_argument('--batches', type=int, default=64, help='timed batches per way and round')
    ap.add_argument('--upload-frames', type=int, default=64, help='timed add_images calls per round')
    ap.add_argument('--reps', type=int, default=200, help='calls between the device events')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--standardization', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_batch needs an MI355X: there is no CPU path and no figure without one')
    if a.frames == -1:
        return paired_frames(a)
    dev = torch.device('cuda:0')
    (H, W), (Hr, Wr) = a.source, a.resize
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    labels = [rng.integers(0, 34, (H, W), dtype=np.uint8) for _ in range(4)]
    timed_frames = a.rounds * a.upload_frames
    store = ImageStore(a.frames + timed_frames, resize_hw=(Hr, Wr), source_hw=(H, W), standardization=a.standardization)
    store.add_images([frames[k % 4] for k in range(a.frames)], [labels[k % 4] for k in range(a.frames)])
    try:
        from PIL import Image
    except ImportError:
        Image = None
    head = dict(source=[H, W], resize=[Hr, Wr], crop=[a.height, a.width], batch=a.batch, standardization=a.standardization,
                store_bytes=store.bytes(), pil=None if Image is None else Image.__version__)
    if Image is not None and not a.standardization:
        L = Image.fromarray(frames[1]).convert('L').resize((Wr, Hr), Image.BILINEAR)
        near = Image.fromarray(labels[1]).resize((Wr, Hr), Image.NEAREST)
        head['slot_equals_pil'] = bool(np.array_equal(store.images[1].cpu().numpy(), np.array(L)) and
                                       np.array_equal(store.labels[1].cpu().numpy(), np.array(near)))
    print(json.dumps(head), flush=True)

    # ---- the ways
    d = store._device()
    tabs = d['tables']
    frame_dev, label_dev = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(labels[0]).to(dev)
    slot, slot_l, mm = torch.zeros_like(store.images[0]), torch.zeros_like(store.images[0]), torch.zeros(2, dtype=torch.int32, device=dev)

    def launches():
        hip.image_ingest(frame_dev, slot, tabs['h'], tabs['v'], d['scratch'], a.standardization, mm, label=label_dev, label_rows=tabs['rows'],
                         label_cols=tabs['cols'], out_label=slot_l)
    n_added = [0]

    def with_upload():
        k = n_added[0]
        n_added[0] += 1
        store.add_images([frames[k % 4]], [labels[k % 4]])
    eager = ImageBatchBuilder(store, a.height, a.width, seed=1)
    graph = ImageBatchBuilder(store, a.height, a.width, seed=1, graph=True)
    aug = DeviceAugmentation(a.height, a.width, shift_limit=eager.shift_limit, id_lut=cityscapes_id_lut(6).to(dev), seed=1)
    order = np.random.default_rng(1)
    batches = [order.integers(0, a.frames, a.batch) for _ in range(a.batches)]
    batches_dev = [torch.from_numpy(b).to(dev) for b in batches]

    def composed(k):
        idx = batches_dev[k]
        img = store.images.index_select(0, idx)[:, :eager.rows]
        lab = store.labels.index_select(0, idx)[:, :eager.rows]
        return aug(img, lab)

    def pil_host():
        L = Image.fromarray(frames[0]).convert('L').resize((Wr, Hr), Image.BILINEAR)
        near = Image.fromarray(labels[0]).resize((Wr, Hr), Image.NEAREST)
        return torch.from_numpy(np.array(L)).float().to(dev), torch.from_numpy(np.array(near)).long().to(dev)
    ways = {
        'ingest_launches': lambda: device_ms(launches, a.reps),
        'ingest_with_upload': lambda: statistics.mean(host_ms(with_upload) for _ in range(a.upload_frames)),
        'build_eager': lambda: statistics.mean(host_ms(lambda k=k: eager.build(batches[k])) for k in range(a.batches)),
        'build_graph': lambda: statistics.mean(host_ms(lambda k=k: graph.build(batches[k])) for k in range(a.batches)),
        'composed': lambda: statistics.mean(host_ms(lambda k=k: composed(k)) for k in range(a.batches)),
    }
    if Image is not None:
        ways['pil_host'] = lambda: statistics.mean(host_ms(pil_host) for _ in range(16))
    else:
        print(json.dumps(dict(way='pil_host', note='PIL is absent on this machine: the host path is not measured')), flush=True)
    for k in range(2):  # (the warm-up of every shape that is timed, and the captures)
        launches(), eager.build(batches[k]), graph.build(batches[k]), composed(k)
        if Image is not None:
            pil_host()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            times[k].append(fn())
    unit = {'ingest_launches': f'ms per frame, device events, {a.reps} calls', 'ingest_with_upload': 'ms per frame, host clock to a device synchronise',
            'pil_host': 'ms per frame, host clock to a device synchronise'}
    for k, v in times.items():
        print(json.dumps(dict(way=k, ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                              clock=unit.get(k, f'ms per batch of {a.batch}, host clock to a device synchronise'))), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(times['composed']) - min(times['composed'])
    verdict = dict(composed_spread_ms=round(spread, 3))
    for k in ('build_eager', 'build_graph'):
        verdict[f'{k}_minus_composed_ms'] = round(med[k] - med['composed'], 3)
        verdict[f'{k}_SLOWER_than_composed'] = bool(med[k] - med['composed'] > spread)
    if Image is not None:
        verdict['ingest_with_upload_SLOWER_than_pil_host'] = bool(med['ingest_with_upload'] > med['pil_host'])
    print(json.dumps(verdict), flush=True)


if __name__ == '__main__':
    main()
