"""Times one training batch from raw events at a loader preset, from host columns to synchronised tensors:

    builder   EventBatchBuilder.build: stage, upload, hip.event_scatter_ring, hip.event_grid_finish_window, hip.label_window
    composed  the same staging and upload, then what the library offered before: hip.event_scatter_ring + hip.event_grid_finish
              into a full-size buffer, per-sample torch.flip / slicing into the batch, the label through torch indexing

and the device launches alone (device events around --reps launches): the scatter, scatter + finish_window, scatter + finish,
scatter + finish + flip / slice (the scatter refills the sums every finish clears, so it is in every pair and is timed alone too).
The ways alternate, --rounds times; every figure is ms per batch, median (min - max) over the rounds.  The two ways' batches are
compared bit for bit at the timed size before anything is timed.  One JSON line per figure.

    python tools/bench_train_batch.py --preset dsec|ddd17 --batch 8 --steps 20 --events 100000 [--graph]
    python tools/bench_train_batch.py --store --preset dsec|ddd17 --batch 8 --steps 20 --events 100000 [--graph]
        (a batch cut out of a device EventStore against the same batch from host columns: main_store)"""
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
from ess_amd.datasets.data_util import EventColumns  # noqa: E402
from ess_amd.datasets.event_batches import EventBatchBuilder  # noqa: E402

PRESETS = {'dsec': (EventBatchBuilder.dsec, dict(grid_normalize='unbiased', voxel='trilinear'), 11),
           'ddd17': (EventBatchBuilder.ddd17, dict(grid_normalize='population', voxel='temporal'), 6)}


class ComposedBuilder(EventBatchBuilder):
    """the builder's staging and upload in front of the launches the library offered before it"""

    def _launch(self, k, with_labels):
        st = self._static
        ev, lab = st['out'][k]
        words, B, T = st['words'], self.batch_size, self.sequence_steps
        if 'full' not in st:
            st['full'] = torch.zeros(B * T, self.bins, self.height, self.width, dtype=torch.float32, device=self.device)
        full = st['full']
        tri = self.voxel == 'trilinear'
        hip.event_voxels('ring', st['cols'], words[:4], None, st['acc'], trilinear=tri, maps=st['maps'], map_of=words[4] if tri else None)
        hip.event_grid_finish(words[2], st['acc'], full, crop_rows=self.grid_rows, resize=self.grid_resize, normalize=self.grid_normalize)
        flip_slice(full, ev, self.last_words, T)
        if with_labels:
            Hl, Wl = self.label_hw
            sy = (torch.arange(self.height, device=self.device) * Hl // self.height).clamp(max=Hl - 1)
            sx = (torch.arange(self.width, device=self.device) * Wl // self.width).clamp(max=Wl - 1)
            h, w = self.crop_hw
            for b, (flip, y0, x0, _) in enumerate(self.last_words):
                g = st['labels'][b][sy][:, sx]
                lab[b].copy_((torch.flip(g, dims=[-1]) if flip else g)[y0:y0 + h, x0:x0 + w])

    def build(self, samples, params=None):
        self.last_words = params.tolist()  # (the composition flips and slices on the host's knowledge of the words)
        return super().build(samples, params=params)


def flip_slice(full, out, words, T):
    """per sample: torch.flip and the slice of its T windows' grids, copied into the batch"""
    h, w = out.shape[-2:]
    for b, (flip, y0, x0, _) in enumerate(words):
        g = full[b * T:(b + 1) * T]
        out[b * T:(b + 1) * T].copy_((torch.flip(g, dims=[-1]) if flip else g)[..., y0:y0 + h, x0:x0 + w])


def make_samples(bld, n_events, classes, seed):
    g = np.random.default_rng(seed)
    Hs, Ws = bld.grid_hw
    out = []
    for b in range(bld.batch_size):
        n = n_events * bld.sequence_steps
        t = np.sort(g.integers(0, 50_000 * bld.sequence_steps, n)).astype(np.int64) + 1_600_000_000_000_000
        cols = EventColumns(t, g.integers(0, Ws, n).astype(np.uint16), g.integers(0, Hs, n).astype(np.uint16), g.integers(0, 2, n).astype(np.uint8))
        out.append((cols, g.integers(0, classes, bld.label_hw).astype(np.uint8)))
    return out


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


def main_store(a):
    """--store: a batch from a device EventStore against the same batch from host columns, build() to synchronised tensors.
    A synthetic store of --recordings recordings of 3 samples' worth of events each; a sample is the T * events events before an end
    index, the ends half a sample apart (consecutive samples overlap by 50 %); the host-column way gets the same events as slices of
    the recordings' host arrays.  Both ways get the same window rows, their batches are compared bit for bit before anything is
    timed; they alternate, --rounds times.  Also: the one-off upload, ms per million events."""
    from ess_amd.datasets.event_store import EventStore, StoreSample
    make, kw, classes = PRESETS[a.preset]
    B, T, n = a.batch, a.steps, a.events
    per = T * n
    probe = make(B, T, a.bins, hip.event_column_stride(per), **kw)
    Hs, Ws = probe.grid_hw
    g = np.random.default_rng(0)
    store = EventStore(a.recordings * 3 * per, label_hw=probe.label_hw, label_capacity=a.recordings * 5)
    recs, upload = [], []
    for r in range(a.recordings):
        m = 3 * per
        t = np.sort(g.integers(0, 50_000 * 3 * T, m)).astype(np.int64) + 1_600_000_000_000_000
        cols = EventColumns(t, g.integers(0, Ws, m).astype(np.uint16), g.integers(0, Hs, m).astype(np.uint16), g.integers(0, 2, m).astype(np.uint8))
        labels = g.integers(0, classes, (5,) + probe.label_hw).astype(np.uint8)
        upload.append(host_ms(lambda: store.add_recording(cols, labels=labels)) / (m / 1e6))
        recs.append((cols, labels))
    pool = [(r, per + k * per // 2, 5 * r + k) for r in range(a.recordings) for k in range(5)]  # (recording, end index, label)
    order = np.random.default_rng(1).permutation(len(pool))
    batches = [[pool[i] for i in order[(j * B + np.arange(B)) % len(pool)]] for j in range(2)]
    new = make(B, T, a.bins, None, store=store, window_events=n, graph=a.graph, **kw)
    old = make(B, T, a.bins, hip.event_column_stride(per), graph=a.graph, **kw)
    s_store = [[StoreSample(r, end=e, label=lab) for r, e, lab in batch] for batch in batches]
    s_cols = [[(EventColumns(*(c[e - per:e] for c in (recs[r][0].t, recs[r][0].x, recs[r][0].y, recs[r][0].p))), recs[r][1][lab - 5 * r])
               for r, e, lab in batch] for batch in batches]
    from ess_amd.datasets.event_batches import draw_window_params
    gen = torch.Generator().manual_seed(1)
    params = [draw_window_params(B, (new.height, new.width), new.crop_hw, new.crop_band, gen) for _ in range(2)]
    same = True
    for k in range(2):  # (also the warm-up, and the captures)
        for _ in range(2):
            ev, lab = new.build(s_store[k], params=params[k])
            wev, wlab = old.build(s_cols[k], params=params[k])
            same = same and torch.equal(ev.view(torch.int32), wev.view(torch.int32)) and torch.equal(lab, wlab)
    same = same and not bool(new.last_flags.any())
    print(json.dumps(dict(preset=a.preset, batch=B, steps=T, events=n, bins=a.bins, graph=a.graph, store_events=store.n_events,
                          store_bytes=store.bytes(), same_bits=bool(same),
                          upload_ms_per_million_events=dict(median=round(statistics.median(upload), 3), min=round(min(upload), 3),
                                                            max=round(max(upload), 3)))), flush=True)
    if not same:
        raise SystemExit('the two ways do not give the same batch: nothing is timed')
    ways = {'store': lambda: statistics.mean(host_ms(lambda k=k: new.build(s_store[k & 1], params=params[k & 1])) for k in range(a.batches)),
            'host_columns': lambda: statistics.mean(host_ms(lambda k=k: old.build(s_cols[k & 1], params=params[k & 1])) for k in range(a.batches)),
            'store_launches_alone': lambda: device_ms(lambda: new._launch_store(0, True, hip.EVENT_STORE_RULE_COUNT_INDEX), a.reps)}
    times = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            times[k].append(fn())
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(json.dumps(dict(way=k, ms_median=round(med[k], 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                              clock=f'device events, {a.reps} launches' if 'alone' in k else 'host, to a device synchronise')), flush=True)
    spread = max(times['host_columns']) - min(times['host_columns'])
    print(json.dumps(dict(store_minus_host_columns_ms=round(med['store'] - med['host_columns'], 3), host_columns_spread_ms=round(spread, 3),
                          store_SLOWER_than_host_columns=bool(med['store'] - med['host_columns'] > spread))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--store', action='store_true', help='a device EventStore against host columns (see main_store)')
    ap.add_argument('--recordings', type=int, default=3, help='(with --store) recordings of 3 samples\' worth of events each')
    ap.add_argument('--preset', choices=sorted(PRESETS), default='ddd17')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20, help='windows per sample (T)')
    ap.add_argument('--events', type=int, default=100000, help='events per window')
    ap.add_argument('--bins', type=int, default=5)
    ap.add_argument('--graph', action='store_true', help='both ways replay captured launches')
    ap.add_argument('--batches', type=int, default=4, help='timed batches per way and round (after 2 untimed)')
    ap.add_argument('--reps', type=int, default=10, help='launches between the device events')
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_train_batch needs an MI355X: there is no CPU path and no figure without one')
    if a.store:
        return main_store(a)
    make, kw, classes = PRESETS[a.preset]
    cap = hip.event_column_stride(a.steps * a.events)
    new = make(a.batch, a.steps, a.bins, cap, graph=a.graph, **kw)
    # (graph: the composition's launches depend on the words through the host, so it cannot replay; it runs eager either way)
    old = ComposedBuilder(a.batch, a.steps, a.bins, cap, grid_hw=new.grid_hw, grid_rows=new.grid_rows, grid_resize=new.grid_resize,
                          height=new.height, width=new.width, label_hw=new.label_hw,
                          crop_hw=new.crop_hw if new.crop_hw != (new.height, new.width) else None,
                          crop_band=new.crop_band if new.crop_hw != (new.height, new.width) else None, **kw)
    samples = [make_samples(new, a.events, classes, s) for s in range(2)]
    from ess_amd.datasets.event_batches import draw_window_params
    g = torch.Generator().manual_seed(1)
    params = [draw_window_params(a.batch, (new.height, new.width), new.crop_hw, new.crop_band, g) for _ in range(2)]
    same = True
    for s, p in zip(samples, params):  # (also the warm-up of every shape that is timed)
        for _ in range(2):
            ev, lab = new.build(s, params=p)
            wev, wlab = old.build(s, params=p)
            same = same and torch.equal(ev.view(torch.int32), wev.view(torch.int32)) and torch.equal(lab, wlab)
    head = dict(preset=a.preset, batch=a.batch, steps=a.steps, events=a.events, bins=a.bins, graph=a.graph, same_bits=bool(same))
    print(json.dumps(head), flush=True)
    if not same:
        raise SystemExit('the two ways do not give the same batch: nothing is timed')

    st = new._static
    words, T = st['words'], a.steps
    full = old._static['full']
    host_words = params[1].tolist()

    def scatter():
        tri = new.voxel == 'trilinear'
        hip.event_voxels('ring', st['cols'], words[:4], None, st['acc'], trilinear=tri, maps=st['maps'], map_of=words[4] if tri else None)

    def finish():
        hip.event_grid_finish(words[2], st['acc'], full, crop_rows=new.grid_rows, resize=new.grid_resize, normalize=new.grid_normalize)

    def window():
        hip.event_grid_finish_window(words[2], st['acc'], st['out'][0][0], st['params'], T, crop_rows=new.grid_rows,
                                     resize=new.grid_resize, normalize=new.grid_normalize)
    ways = {
        'builder': lambda: statistics.mean(host_ms(lambda k=k: new.build(samples[k & 1], params=params[k & 1])) for k in range(a.batches)),
        'composed': lambda: statistics.mean(host_ms(lambda k=k: old.build(samples[k & 1], params=params[k & 1])) for k in range(a.batches)),
        'scatter': lambda: device_ms(scatter, a.reps),
        'scatter+finish_window': lambda: device_ms(lambda: (scatter(), window()), a.reps),
        'scatter+finish': lambda: device_ms(lambda: (scatter(), finish()), a.reps),
        'scatter+finish+flip_slice': lambda: device_ms(lambda: (scatter(), finish(), flip_slice(full, st['out'][0][0], host_words, T)), a.reps),
    }
    new.build(samples[1], params=params[1])  # (the words and columns the launches-alone figures read)
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            times[k].append(fn())
    assert not bool(st['acc'].any())
    for k, v in times.items():
        print(json.dumps(dict(way=k, ms_median=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3),
                              clock='host, to a device synchronise' if k in ('builder', 'composed') else f'device events, {a.reps} launches')),
              flush=True)


if __name__ == '__main__':
    main()
