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

    python tools/bench_image_batch.py [--batch 8] [--height 200 --width 352] [--rounds 2] [--batches 64] [--standardization]"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--source', type=int, nargs=2, default=(1024, 2048))
    ap.add_argument('--resize', type=int, nargs=2, default=(256, 512))
    ap.add_argument('--height', type=int, default=200)
    ap.add_argument('--width', type=int, default=352)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--frames', type=int, default=16, help='frames the store holds for the batches')
    ap.add_argument('--batches', type=int, default=64, help='timed batches per way and round')
    ap.add_argument('--upload-frames', type=int, default=64, help='timed add_images calls per round')
    ap.add_argument('--reps', type=int, default=200, help='calls between the device events')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--standardization', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_batch needs an MI355X: there is no CPU path and no figure without one')
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
