"""GPU tier of the loader finish (csrc/voxel_ingest.hip: ess_event_scatter_ring*, ess_event_grid_finish): every row of the table of
tests/test_host_loader_grid.py -- geometries 1 x 1, 3 x 2 -> 5 x 1 (a scale of 0), 2 x 7 -> 2 x 9, the two loader presets in
miniature, two identities (one whose slot size is no multiple of 4); 1 and 5 bins; 1 and 7 slots, among the seven an INGEST_KEEP
slot, an empty one, one with a single non-zero voxel and one whose non-zero voxels are all equal; the three normalisations -- against
tests/loader_grid_ref.py's float64 reference and bounds.  Poison: out starts NaN inside a guarded buffer, the workspace as 0xFF bytes;
acc is all zero behind every call.  Bits: a second run, a slot alone, shuffled events, and the identity against hip.event_ingest_ring."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loader_grid_ref as LG  # noqa: E402
from tests import test_hip_event_columns as C  # noqa: E402  (device columns, guards)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers)
from tests import test_host_event_ingest as R  # noqa: E402  (events inside a grid)
from tests import test_host_loader_grid as TH  # noqa: E402  (the table: geometries, rows, cases with their references)

DEV = M.DEV
_bits, _words = C._bits, C._words
KEEP = LG.KEEP


def _finish(acc_host, counts_host, geo, mode):
    """one call on a fresh upload of the sums, out NaN in a guarded buffer, the workspace 0xFF -> (out, buffer, acc on the device)"""
    from ess_amd import hip
    n, bins = acc_host.shape[:2]
    acc = acc_host.to(DEV)
    counts = _words([1] * n if counts_host is None else counts_host.tolist())
    buf, out = M._guarded((n, bins, geo.rows, geo.Wr), torch.float32)
    hip.grid_finish_workspace(n, bins, geo.Hs, geo.Ws, DEV).fill_(0xFF)
    got = hip.event_grid_finish(counts, acc, out, crop_rows=geo.crop, resize=(geo.Hr, geo.Wr), normalize=mode)
    assert got is out
    return out, buf, acc


@pytest.mark.parametrize('geo,bins,n_slots,mode', TH.ROWS, ids=['-'.join(map(str, r)) for r in TH.ROWS])
def test_the_table_against_fp64(geo, bins, n_slots, mode):
    """every output voxel within its bound of the float64 reference, NaN exactly where the reference has it (the KEEP slot's poison; a
    population std of 0); nothing written outside out; acc all zero; the same bits from a second run; each slot alone gives the bits it
    gets among seven"""
    acc, counts, ref, bound = TH._case(geo, bins, n_slots, mode)
    g, m = TH.GEOMETRIES[geo], TH.MODES[mode]
    out, buf, dev_acc = _finish(acc, counts, g, m)
    torch.cuda.synchronize()
    ratio = LG.worst_ratio(out, ref, bound)
    print(f'{geo} bins={bins} n={n_slots} {mode}: worst error / bound = {ratio:.3f}')
    assert ratio <= 1.0, (geo, bins, n_slots, mode, ratio)
    assert C._guards_intact(buf, out) and not bool(dev_acc.any())
    if counts is not None:
        assert bool(torch.isnan(out[1]).all()) and not bool(out[2].any())
    again, _, acc2 = _finish(acc, counts, g, m)
    assert torch.equal(_bits(again), _bits(out)) and not bool(acc2.any())
    if n_slots > 1:
        for i in range(n_slots):
            if counts is not None and counts[i] < 0:
                continue
            alone, _, acc1 = _finish(acc[i:i + 1], None if counts is None else counts[i:i + 1], g, m)
            assert torch.equal(_bits(alone[0]), _bits(out[i])), f'slot {i} alone'
            assert not bool(acc1.any())


def test_a_kept_slot_with_every_other_count_word():
    """counts: any negative word keeps, 0 and any positive word finish (the finish reads the sums, not the events)"""
    acc, _, _, _ = TH._case('dsec', 5, 7, 'unbiased')
    g = TH.GEOMETRIES['dsec']
    counts = torch.tensor([5, KEEP, 0, -7, 1 << 30, 1, -(1 << 31)], dtype=torch.int32)
    acc = acc.clone()
    acc[counts < 0] = 0
    ref, bound = LG.reference(acc, g, LG.NORM_UNBIASED, counts)
    out, buf, dev_acc = _finish(acc, counts, g, LG.NORM_UNBIASED)
    assert LG.worst_ratio(out, ref, bound) <= 1.0 and C._guards_intact(buf, out) and not bool(dev_acc.any())
    assert all(bool(torch.isnan(out[i]).all()) == bool(counts[i] < 0) for i in range(7))


# ---------------------------------------------------------------------------------------------- from events: scatter, then finish
RING = 32


def _rows(n_rows, nb, H, W, seed, fmts):
    """per row a full ring of events inside the H x W grid, times sorted (a window's first and last event carry its normalisation)"""
    return [C._as_columns(R.events(RING, H, W, seed + r), fmts[r]) for r in range(n_rows)]


def _slot_words(slots):
    return tuple(_words([s[k] for s in slots]) for k in range(4))


@pytest.mark.parametrize('nb,H,W', [(5, 24, 40), (3, 5, 7)], ids=['vec', 'odd'])
@pytest.mark.parametrize('flavour', ['temporal', 'trilinear'])
def test_scatter_then_identity_finish_has_the_bits_of_the_ring_ingest(nb, H, W, flavour):
    """seven slots over three rows -- windows that wrap, a KEEP slot, an empty one --: hip.event_scatter_ring* followed by
    hip.event_grid_finish without crop, resize or normalisation equals hip.event_ingest_ring* bit for bit; acc holds sums in between
    and zeros behind"""
    from ess_amd import hip
    rows = _rows(3, nb, H, W, 40, (1, 0, 3))
    slots = [(0, 0, 32, 1), (1, 30, 9, 0), (2, 5, KEEP, 3), (2, 17, 0, 3), (0, 3, 1, 1), (1, 31, 32, 0), (2, 8, 20, 3)]
    dev = C._device_columns(rows, RING)
    words = _slot_words(slots)
    acc = torch.zeros(7, nb, H, W, dtype=torch.int64, device=DEV)
    (_, want), (buf, out) = (M._guarded((7, nb, H, W), torch.float32) for _ in range(2))  # (the same NaN poison in both)
    if flavour == 'temporal':
        hip.event_ingest_ring(*dev, *words, want)
        assert hip.event_scatter_ring(*dev, *words, acc) is acc
    else:
        hip.event_ingest_ring_trilinear(*dev, *words, want)
        assert hip.event_scatter_ring_trilinear(*dev, *words, acc) is acc
    assert bool(acc[0].any()) and not bool(acc[2].any()) and not bool(acc[3].any())
    hip.grid_finish_workspace(7, nb, H, W, DEV).fill_(0xFF)
    hip.event_grid_finish(words[2], acc, out)
    assert torch.equal(_bits(out), _bits(want)) and bool(torch.isnan(out[2]).all()) and not bool(out[3].any()) and bool(out[0].any())
    assert C._guards_intact(buf, out) and not bool(acc.any())


@pytest.mark.parametrize('mode', ['unbiased', 'population'])
def test_shuffled_events_give_the_same_bits(mode):
    """a window's inner events in another order (its first and last stay: they carry the time normalisation): the sums are integers,
    the statistics are taken in an order fixed by the launch -- the resized, normalised grids are identical"""
    from ess_amd import hip
    from ess_amd.datasets.data_util import EventColumns
    nb, H, W = 5, 24, 40
    geo = LG.Geometry((H, W), (26, 48), crop=20, rows=25)
    rows = _rows(2, nb, H, W, 60, (1, 2))
    g = np.random.default_rng(9)
    order = np.concatenate([[0], 1 + g.permutation(RING - 2), [RING - 1]])
    other = [EventColumns(*(np.ascontiguousarray(v[order]) for v in (c.t, c.x, c.y, c.p))) for c in rows]
    slots = [(0, 0, 32, 1), (1, 0, 32, 2)]
    outs = []
    for cols in (rows, other):
        acc = torch.zeros(2, nb, H, W, dtype=torch.int64, device=DEV)
        hip.event_scatter_ring(*C._device_columns(cols, RING), *_slot_words(slots), acc)
        out = torch.full((2, nb, geo.rows, geo.Wr), float('nan'), device=DEV)
        hip.grid_finish_workspace(2, nb, H, W, DEV).fill_(0xFF)
        sums = acc.cpu()
        hip.event_grid_finish(_words([32, 32]), acc, out, crop_rows=geo.crop, resize=(geo.Hr, geo.Wr), normalize=TH.MODES[mode])
        outs.append((out, sums))
        assert not bool(acc.any())
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
    ref, bound = LG.reference(outs[0][1], geo, TH.MODES[mode])
    assert LG.worst_ratio(outs[0][0], ref, bound) <= 1.0 and bool(outs[0][0].isfinite().all()) and len(outs[0][0].unique()) > 20


def test_the_finish_is_captured_once_and_replayed():
    """no memset, no synchronisation: scatter + finish (the map and the clear in two kernels) in a graph, replayed on new counts"""
    from ess_amd import hip
    nb, H, W = 5, 24, 40
    geo = LG.Geometry((H, W), (24, 44), rows=20)
    rows = _rows(2, nb, H, W, 80, (1, 0))
    dev = C._device_columns(rows, RING)
    words = [w.clone() for w in _slot_words([(0, 0, 32, 1), (1, 4, 20, 0)])]
    acc = torch.zeros(2, nb, H, W, dtype=torch.int64, device=DEV)
    out = torch.full((2, nb, geo.rows, geo.Wr), float('nan'), device=DEV)

    def run():
        hip.event_scatter_ring(*dev, *words, acc)
        hip.event_grid_finish(words[2], acc, out, resize=(geo.Hr, geo.Wr), normalize=hip.GRID_NORM_UNBIASED)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    out.fill_(float('nan'))
    graph.replay()
    assert torch.equal(_bits(out), _bits(eager)) and not bool(acc.any())
    words[2].copy_(_words([KEEP, 7]))
    first = out[0].clone()
    graph.replay()
    acc7 = torch.zeros(1, nb, H, W, dtype=torch.int64, device=DEV)
    lone = torch.full((1, nb, geo.rows, geo.Wr), float('nan'), device=DEV)
    hip.event_scatter_ring(*dev, *_slot_words([(1, 4, 7, 0)]), acc7)
    hip.event_grid_finish(_words([7]), acc7, lone, resize=(geo.Hr, geo.Wr), normalize=hip.GRID_NORM_UNBIASED)
    assert torch.equal(_bits(out[0]), _bits(first)) and torch.equal(_bits(out[1]), _bits(lone[0])) and not bool(acc.any())
