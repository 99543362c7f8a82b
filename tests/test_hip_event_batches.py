"""GPU tier of the training batches from events (ess_amd/datasets/event_batches.py: EventBatchBuilder, EventBatchLoader) on small
geometries: the builder against the composition the library offered before it (hip.event_scatter_ring* + hip.event_grid_finish +
torch.flip / slicing on the host + a numpy label), BIT FOR BIT; grids and labels moving together; the builder against the loaders'
own lines (tests/event_batch_ref.py) within tests/loader_grid_ref.py's bound; the two presets' aspect ratios in miniature; and one
supervised train step on a built batch."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import event_batch_ref as EBR  # noqa: E402
from tests import loader_grid_ref as LG  # noqa: E402
from tests import test_hip_event_columns as C  # noqa: E402  (device columns, words, bits)
from tests import test_hip_label_window as LW  # noqa: E402  (the numpy restatement of the label rule)
from tests import test_host_event_ingest as R  # noqa: E402  (events inside a grid)
from tests import test_host_event_trilinear as TL  # noqa: E402  (synthetic maps, raw sensor events)

DEV = C.DEV
_bits = C._bits
B, T, BINS, CAP = 3, 3, 3, 512
COUNTS = [300, 200, 2]  # (200: a remainder of 2 events is dropped; 2 < T: an all-zero sample)
MH, MW = 16, 22  # the sensor of the trilinear rigs: another size than any grid
GEOMETRIES = {
    'small': dict(grid_hw=(13, 18), grid_rows=10, grid_resize=(13, 20), height=12, width=20, crop_hw=(6, 12), crop_band=(4, 8),
                  label_hw=(12, 18)),
    'dsec': dict(grid_hw=(24, 32), grid_rows=22, grid_resize=(23, 32), height=23, width=32, label_hw=(22, 32)),  # flip only
    'ddd17': dict(grid_hw=(26, 34), grid_resize=(26, 36), height=20, width=36, crop_hw=(12, 20), crop_band=(8, 12), label_hw=(20, 34)),
}
NORMS = {None: LG.NORM_NONE, 'unbiased': LG.NORM_UNBIASED, 'population': LG.NORM_POPULATION}


def _builder(geo, voxel='temporal', normalize='unbiased', **kw):
    from ess_amd.datasets.event_batches import EventBatchBuilder
    maps = [_maps(geo)[0], _maps(geo)[1]] if voxel == 'trilinear' else None
    return EventBatchBuilder(B, T, BINS, CAP, **GEOMETRIES[geo], grid_normalize=normalize, voxel=voxel, rectify_maps=maps, **kw)


@functools.lru_cache(maxsize=None)
def _maps(geo):
    """two different maps of one sensor onto the geometry's grid -> host [2, MH, MW, 2]"""
    Hs, Ws = GEOMETRIES[geo]['grid_hw']
    return np.stack([TL.synthetic_map(MH, MW, Hs, Ws, 1), TL.synthetic_map(MH, MW, Hs, Ws, 2)])


@functools.lru_cache(maxsize=None)
def _samples(geo, voxel, seed, labelled=True):
    """B samples (EventColumns, uint8 label[, map index]): int64 and float64 times mixed within the batch; unchanged by its users"""
    Hs, Ws = GEOMETRIES[geo]['grid_hw']
    g = np.random.default_rng(1000 + seed)
    values = np.array(list(range(19)) + [255], dtype=np.uint8)
    out = []
    for b, n in enumerate(COUNTS):
        fmt = (b + seed) % 2  # (EVCOL_T_I64 or not)
        cols = TL.raw_events(n, MH, MW, 10 * seed + b, fmt) if voxel == 'trilinear' else C._as_columns(R.events(n, Hs, Ws, 10 * seed + b), fmt)
        label = values[g.integers(0, len(values), GEOMETRIES[geo]['label_hw'])] if labelled else None
        out.append((cols, label, [0, None, 1][(b + seed) % 3]) if voxel == 'trilinear' else (cols, label))
    assert {s[0].t.dtype for s in out} == {np.dtype(np.int64), np.dtype(np.float64)}
    return out


def _sums(geo, voxel, samples):
    """the samples' B T windows scattered by the library's own kernel -> (acc int64 [B T, bins, Hs, Ws] on the device, counts words)"""
    from ess_amd import hip
    Hs, Ws = GEOMETRIES[geo]['grid_hw']
    cols = [s[0] for s in samples]
    per = [c.n // T for c in cols]
    words = [C._words(v) for v in ([b for b in range(B) for _ in range(T)], [t * per[b] for b in range(B) for t in range(T)],
                                  [per[b] for b in range(B) for _ in range(T)], [cols[b].format for b in range(B) for _ in range(T)])]
    acc = torch.zeros(B * T, BINS, Hs, Ws, dtype=torch.int64, device=DEV)
    dev = C._device_columns(cols, CAP)
    if voxel == 'trilinear':
        map_of = C._words([hip.RECTIFY_NONE if s[2] is None else s[2] for s in samples for _ in range(T)])
        hip.event_scatter_ring_trilinear(*dev, *words, acc, torch.from_numpy(_maps(geo)).to(DEV), map_of)
    else:
        hip.event_scatter_ring(*dev, *words, acc)
    return acc, words[2]


def _composition(geo, voxel, normalize, samples, params):
    """what the library offered before the builder: scatter, hip.event_grid_finish, then flip / slice on the host and a numpy label
    -> (events [B, T bins, h, w] on the host, labels int64 numpy [B, h, w] or None)"""
    from ess_amd import hip
    G = GEOMETRIES[geo]
    rows, resize = G.get('grid_rows', G['grid_hw'][0]), G.get('grid_resize')
    h, w = G.get('crop_hw', (G['height'], G['width']))
    acc, counts = _sums(geo, voxel, samples)
    full = torch.full((B * T, BINS, G['height'], G['width']), float('nan'), device=DEV)
    hip.event_grid_finish(counts, acc, full, crop_rows=rows, resize=resize, normalize=NORMS[normalize])
    assert not bool(acc.any())
    full = full.cpu().view(B, T * BINS, G['height'], G['width'])
    ev = torch.stack([EBR.window(full[b], *params[b, :3].tolist(), h, w) for b in range(B)])
    if samples[0][1] is None:
        return ev, None
    return ev, LW.restate(np.stack([s[1] for s in samples]), (G['height'], G['width']), params.tolist(), h, w)


def _assert_batch(got, want, what):
    (ev, lab), (wev, wlab) = got, want
    assert ev.dtype == torch.float32 and tuple(ev.shape) == tuple(wev.shape) and ev.is_contiguous(), what
    assert torch.equal(_bits(ev.cpu()), _bits(wev)), what
    if wlab is None:
        assert lab is None, what
    else:
        assert lab.dtype == torch.int64 and (lab.cpu().numpy() == wlab).all(), what


# ---------------------------------------------------------------------------------------------- 1. against the composition
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('voxel', ['temporal', 'trilinear'])
def test_the_builder_has_the_bits_of_the_composition(voxel, graph):
    """three different batches through one builder (drawn words, given words, no labels): scatter + finish + flip / slice + numpy
    label, bit for bit; int64 and float64 times mixed, a sample with a remainder, a sample with n < T (zeros); a batch stays valid
    while the next one is built; graph=True: one capture per output set and kind of batch, then replays"""
    bld = _builder('small', voxel, graph=graph, seed=11)
    given = torch.tensor([[1, 4, 3, 0], [0, 6, 8, 0], [1, 5, 0, 0]], dtype=torch.int32)
    previous = None
    for k, (params, labelled) in enumerate([(None, True), (given, True), (None, True), (None, False), (given, True)]):
        samples = _samples('small', voxel, k, labelled)
        got = bld.build(samples, params=params)
        p = bld.last_params
        assert p.dtype == torch.int32 and tuple(p.shape) == (B, 4) and (params is None or torch.equal(p, params))
        want = _composition('small', voxel, 'unbiased', samples, p)
        _assert_batch(got, want, (voxel, graph, k))
        assert not bool(got[0][2].any()) and bool(got[0][0].any()) and bool(got[0].isfinite().all())  # (n < T: an all-zero sample)
        if previous is not None:
            _assert_batch(*previous, (voxel, graph, k, 'the batch before'))
        previous = (got, want)
    assert bld.n_batches == 5 and not bool(bld._static['acc'].any())
    assert bld.n_captures == (3 if graph else 0)  # (set 0 and set 1 with labels, set 1 without)
    assert len({tuple(r) for r in p.tolist()}) > 1


# ---------------------------------------------------------------------------------------------- 2. grids and labels move together
def test_grids_and_labels_move_together():
    """one event per marked pixel, the label 1 on the same pixels, identity resize, random words: the non-zero pixels of the summed
    |bins| are exactly label == 1, for every sample"""
    from ess_amd.datasets.data_util import EventColumns
    from ess_amd.datasets.event_batches import EventBatchBuilder
    H, W, h, w = 13, 18, 6, 12
    bld = EventBatchBuilder(B, T, BINS, CAP, grid_hw=(H, W), height=H, width=W, label_hw=(H, W), crop_hw=(h, w), seed=4)
    seen = set()
    for k in range(4):
        g = np.random.default_rng(50 + k)
        samples = []
        for b in range(B):
            at = g.permutation(H * W)[:30 * T]  # (a multiple of T: no event is dropped)
            label = np.zeros((H, W), np.uint8)
            label.reshape(-1)[at] = 1
            cols = EventColumns(np.sort(g.uniform(0, 1, at.size)), (at % W).astype(np.int16), (at // W).astype(np.int16),
                                g.integers(0, 2, at.size).astype(np.uint8))
            samples.append((cols, label))
        ev, lab = bld.build(samples)
        marked = ev.abs().sum(dim=1) != 0
        assert torch.equal(marked, lab == 1) and bool(marked.any()) and tuple(lab.shape) == (B, h, w)
        seen |= {tuple(r) for r in bld.last_params.tolist()}
    assert len(seen) > 6 and {r[0] for r in seen} == {0, 1}


# ---------------------------------------------------------------------------------------------- 3, 4. against the loaders' lines
@pytest.mark.parametrize('geo,normalize', [('small', 'unbiased'), ('dsec', 'unbiased'), ('ddd17', 'population'), ('ddd17', None)])
def test_the_builder_against_the_loaders_lines(geo, normalize):
    """the builder's grids within loader_grid_ref's bound of its float64 reference pushed through the loaders' flip and crop
    (worst error / bound <= 1, the bound test_hip_loader_grid.py holds the finish to: no new tolerance), and the loaders' own fp32
    lines -- F.interpolate(bilinear, align_corners=True), the row cuts, torch.flip, the crop -- within the same bound of the same
    reference; the labels equal the loaders' lines exactly; and the bits of the composition at this geometry"""
    G = GEOMETRIES[geo]
    rows, resize = G.get('grid_rows', G['grid_hw'][0]), G.get('grid_resize')
    h, w = G.get('crop_hw', (G['height'], G['width']))
    bld = _builder(geo, normalize=normalize, seed=21)
    samples = _samples(geo, 'temporal', 7)
    ev, lab = bld.build(samples)
    p = bld.last_params
    _assert_batch((ev, lab), _composition(geo, 'temporal', normalize, samples, p), geo)
    sums = _sums(geo, 'temporal', samples)[0].cpu()
    lg = LG.Geometry(G['grid_hw'], resize, crop=rows, rows=G['height'])
    ref, bound = (t.view(B, T * BINS, G['height'], G['width']) for t in LG.reference(sums, lg, NORMS[normalize]))
    grids = LG.restate(sums, LG.Geometry(G['grid_hw']), NORMS[normalize]).view(B, T * BINS, *G['grid_hw'])  # (the loader's fp32 grids)
    for b in range(B):
        flip, y0, x0 = p[b, :3].tolist()
        r, bd = EBR.window(ref[b], flip, y0, x0, h, w), EBR.window(bound[b], flip, y0, x0, h, w)
        ratio = LG.worst_ratio(ev[b], r, bd)
        lines = LG.worst_ratio(EBR.loader_lines(grids[b], rows, resize, G['height'], flip, y0, x0, (h, w)), r, bd)
        print(f'{geo} {normalize} sample {b}: builder worst error / bound = {ratio:.3f}, the loader\'s fp32 lines = {lines:.3f}')
        assert ratio <= 1.0 and lines <= 1.0, (geo, b, ratio, lines)
        assert torch.equal(lab[b].cpu(), EBR.label_lines(samples[b][1], G['height'], G['width'], flip, y0, x0, (h, w)))
    assert bool(ev[0].any()) and not bool(ev[2].any())
    if 'crop_band' in G:
        assert bool((p[:, 1] >= G['crop_band'][0]).all())


# ---------------------------------------------------------------------------------------------- 5. one supervised step
def test_one_supervised_step_on_a_built_batch_and_the_same_bits_twice():
    """ESSSupervisedModel.train_step takes a built batch through an EventBatchLoader and gives a finite loss; the same samples and
    seed give the same batch bits twice"""
    from oracle import ess_oracle as O
    from ess_amd.config.settings import synthetic_settings
    from ess_amd.datasets.event_batches import EventBatchBuilder, EventBatchLoader
    from ess_amd.training.ess_supervised_trainer import ESSSupervisedModel
    Bs, Ts, Cs, H, W, K = 1, 2, 2, 32, 48, 6  # (the size of the repository's smoke run)
    g = np.random.default_rng(3)
    label = g.integers(0, K, (H, W)).astype(np.uint8)
    label[:2] = 255
    samples = [(C._as_columns(R.events(4000, H, W, 5), 1), label)]
    make = lambda: EventBatchBuilder(Bs, Ts, Cs, 4096, grid_hw=(H, W), height=H, width=W, label_hw=(H, W), grid_normalize='unbiased', seed=9)  # noqa: E731
    first, second = make(), make()
    ev, lab = first.build(samples)
    ev2, lab2 = second.build(samples)
    assert torch.equal(first.last_params, second.last_params) and torch.equal(_bits(ev), _bits(ev2)) and torch.equal(lab, lab2)
    assert tuple(ev.shape) == (Bs, Ts * Cs, H, W) and tuple(lab.shape) == (Bs, H, W) and bool(ev.any())
    st = synthetic_settings('ess_supervised', 'DDD17_events', (H, W), K, Bs, Ts, Cs, train_on_event_labels=True)
    tr = ESSSupervisedModel(st)
    tr.front_end_sensor_b.load_state_dict(O.synth_state_dict(O.e2vid_param_shapes(O.e2vid_config(num_bins=Cs)), 11))
    tr.task_backend.load_state_dict(O.synth_state_dict(O.semseg_param_shapes(256, K), 12, decoder_style=True))
    tr.train_loader = EventBatchLoader([samples], first)
    tr.train_loader.createIterators()
    batches = list(tr.train_loader)
    assert len(batches) == 1 and len(tr.train_loader) == 1
    _, _, final = tr.train_step(batches[0])
    assert bool(torch.isfinite(final.detach())) and float(final.detach()) > 0
