"""GPU tier of the training window (csrc/voxel_ingest.hip: ess_event_grid_finish_window): the loader finish with the loaders' flip and
crop fused into its map pass.  The yardstick is hip.event_grid_finish itself, BIT FOR BIT: flip and crop are index permutations of
the grid it stores, so hip.event_grid_finish_window(acc, words) must have exactly the bits of hip.event_grid_finish(a copy of acc)
followed by torch.flip and slicing on the host -- no tolerance exists to choose.  One table of geometries and windows, seeded sums
(tests/loader_grid_ref.seeded_acc) with the special slots (KEEP, empty, one voxel, equal voxels), the three normalisations,
slots_per_group 1 and 3 with flips and offsets that differ between the groups.  Poison: out starts NaN inside a guarded buffer, the
workspace as 0xFF bytes; acc is all zero behind every call."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import loader_grid_ref as LG  # noqa: E402
from tests import test_hip_event_columns as C  # noqa: E402  (guards, words)
from tests import test_hip_multi_stream as M  # noqa: E402  (guarded buffers)

DEV = M.DEV
_bits = C._bits
N_SLOTS = 7
MODES = {'none': LG.NORM_NONE, 'unbiased': LG.NORM_UNBIASED, 'population': LG.NORM_POPULATION}
RESIZED = dict(src=(13, 18), resized=(13, 20), crop=10)
# name -> (bins, geometry, window (h, w), the (y0, x0) offsets the groups cycle through; None: spread over the whole range)
ROWS = {
    'identity-odd': (3, LG.Geometry((5, 7)), (3, 5), None),                     # scalar stores, odd everything
    'identity-vec': (5, LG.Geometry((24, 40)), (8, 16), None),                  # vector stores, sums that nobody reads
    'resized': (3, LG.Geometry(**RESIZED), (6, 12), [(4, 3), (4, 8), (4, 5)]),  # row cut + resize, x0 odd and x0 = 8
    'resized-scalar': (3, LG.Geometry(**RESIZED), (6, 5), None),                # a scalar window of a vector-width grid
    'whole-identity': (5, LG.Geometry((24, 40)), (24, 40), None),               # window = whole grid
    'whole-resized': (3, LG.Geometry(**RESIZED), (13, 20), None),
}


def _group_words(name, n_groups, flips=True):
    """per group (flip, y0, x0, 0): flips alternate from group to group, offsets differ between the groups (host int32 [n_groups, 4])"""
    _, geo, (h, w), offsets = ROWS[name]
    rows = []
    for k in range(n_groups):
        if offsets is not None:
            y0, x0 = offsets[k % len(offsets)]
        else:
            y0, x0 = (k * 3) % (geo.rows - h + 1), (k * 5 + 1) % (geo.Wr - w + 1)
        rows.append([int(flips and k % 2 == 0), y0, x0, 0])
    return torch.tensor(rows, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _sums(name):
    """the row's seeded sums with the special slots -> (acc int64 [7, bins, Hs, Ws] on the host, counts); unchanged by its users"""
    bins, geo, _, _ = ROWS[name]
    return LG.special_slots(LG.seeded_acc(N_SLOTS, bins, geo.Hs, geo.Ws, seed=len(name) + 7 * bins, mean=0.4))


def _full(acc_host, counts_host, geo, mode):
    """the yardstick's first half: hip.event_grid_finish on a fresh upload of the sums -> the grid it stores (a KEEP slot: the NaN
    poison), on the host"""
    from ess_amd import hip
    n, bins = acc_host.shape[:2]
    acc = acc_host.to(DEV)
    _, out = M._guarded((n, bins, geo.rows, geo.Wr), torch.float32)
    hip.grid_finish_workspace(n, bins, geo.Hs, geo.Ws, DEV).fill_(0xFF)
    hip.event_grid_finish(C._words(counts_host.tolist()), acc, out, crop_rows=geo.crop, resize=(geo.Hr, geo.Wr), normalize=mode)
    assert not bool(acc.any())
    return out.cpu()


def _expected(full, words, spg, h, w):
    """the yardstick's second half, on the host: torch.flip, then the slice, per slot with its group's row of `words`"""
    out = []
    for i in range(full.shape[0]):
        flip, y0, x0, _ = words[i // spg].tolist()
        g = torch.flip(full[i], dims=[-1]) if flip else full[i]
        out.append(g[:, y0:y0 + h, x0:x0 + w])
    return torch.stack(out)


def _window(acc_host, counts_host, geo, mode, words, spg, h, w):
    """one call under test on a fresh upload of the sums -> (out, its guarded buffer, acc on the device)"""
    from ess_amd import hip
    n, bins = acc_host.shape[:2]
    acc = acc_host.to(DEV)
    buf, out = M._guarded((n, bins, h, w), torch.float32)
    hip.grid_finish_workspace(n, bins, geo.Hs, geo.Ws, DEV).fill_(0xFF)
    assert geo.rows == geo.Hr  # (the window lies inside the whole resized grid)
    got = hip.event_grid_finish_window(C._words(counts_host.tolist()), acc, out, words.to(DEV), spg, crop_rows=geo.crop,
                                       resize=(geo.Hr, geo.Wr), normalize=mode)
    assert got is out
    return out, buf, acc


CASES = [(name, mode, spg) for name in ROWS for mode in MODES for spg in (1, 3)]


@pytest.mark.parametrize('name,mode,spg', CASES, ids=['-'.join(map(str, c)) for c in CASES])
def test_the_table_has_the_bits_of_finish_flip_slice(name, mode, spg):
    """every row x normalisation x slots_per_group, seven slots among them the special ones: the bits of event_grid_finish + flip +
    slice; the KEEP slot's out untouched (the NaN poison), the empty slot zeros; nothing written outside out; acc all zero"""
    _, geo, (h, w), _ = ROWS[name]
    acc, counts = _sums(name)
    words = _group_words(name, -(-N_SLOTS // spg))
    assert len({tuple(r) for r in words[:, :3].tolist()}) > 1 or (h, w) == (geo.rows, geo.Wr)
    want = _expected(_full(acc, counts, geo, MODES[mode]), words, spg, h, w)
    out, buf, dev_acc = _window(acc, counts, geo, MODES[mode], words, spg, h, w)
    assert torch.equal(_bits(out.cpu()), _bits(want)), (name, mode, spg)
    assert C._guards_intact(buf, out) and not bool(dev_acc.any())
    assert bool(torch.isnan(out[1]).all()) and not bool(out[2].any()) and bool(out[0].isfinite().all()) and bool(out[0].any())


@pytest.mark.parametrize('name', ['whole-identity', 'whole-resized'])
@pytest.mark.parametrize('mode', list(MODES))
def test_the_whole_grid_unflipped_is_event_grid_finish(name, mode):
    """window = whole grid with flip = 0 equals hip.event_grid_finish directly"""
    _, geo, (h, w), _ = ROWS[name]
    acc, counts = _sums(name)
    words = torch.zeros(N_SLOTS, 4, dtype=torch.int32)
    out, buf, dev_acc = _window(acc, counts, geo, MODES[mode], words, 1, h, w)
    assert torch.equal(_bits(out.cpu()), _bits(_full(acc, counts, geo, MODES[mode])))
    assert C._guards_intact(buf, out) and not bool(dev_acc.any())


@pytest.mark.parametrize('name', ['identity-vec', 'resized', 'resized-scalar'])
def test_words_out_of_range_give_the_bits_of_their_clamped_values(name):
    """y0 = -3, x0 = 10^6, flip = 7 -> y0 = 0, x0 = Wr - w, flip = 1; and the other ends"""
    _, geo, (h, w), _ = ROWS[name]
    acc, counts = _sums(name)
    wild = torch.tensor([[7, -3, 10 ** 6, 0], [-1, 10 ** 6, -(1 << 31), 5], [1 << 31 - 1, (1 << 31) - 1, -1, -1]], dtype=torch.int32)
    tame = torch.tensor([[1, 0, geo.Wr - w, 0], [1, geo.rows - h, 0, 0], [1, geo.rows - h, 0, 0]], dtype=torch.int32)
    a, buf, acc_a = _window(acc, counts, geo, LG.NORM_UNBIASED, wild, 3, h, w)
    b, _, _ = _window(acc, counts, geo, LG.NORM_UNBIASED, tame, 3, h, w)
    assert torch.equal(_bits(a), _bits(b)) and C._guards_intact(buf, a) and not bool(acc_a.any())
    want = _expected(_full(acc, counts, geo, LG.NORM_UNBIASED), tame, 3, h, w)
    assert torch.equal(_bits(a.cpu()), _bits(want))


@pytest.mark.parametrize('name', ['identity-vec', 'resized'])
def test_a_slot_alone_gives_the_bits_it_gives_in_the_batch(name):
    _, geo, (h, w), _ = ROWS[name]
    acc, counts = _sums(name)
    words = _group_words(name, 3)
    for mode in MODES.values():
        out, _, _ = _window(acc, counts, geo, mode, words, 3, h, w)
        for i in range(N_SLOTS):
            if counts[i] < 0:
                continue
            alone, _, acc1 = _window(acc[i:i + 1], counts[i:i + 1], geo, mode, words[i // 3:i // 3 + 1], 3, h, w)
            assert torch.equal(_bits(alone[0]), _bits(out[i])), f'slot {i} alone'
            assert not bool(acc1.any())


def test_one_capture_replayed_with_other_words_and_other_sums_equals_eager():
    """no memset, no synchronisation, words and counts read on the device: the launches are captured once; a replay on new sums, new
    words and a KEEP word equals the eager call on the same"""
    from ess_amd import hip
    name = 'resized'
    bins, geo, (h, w), _ = ROWS[name]
    sums = [_sums(name)[0], LG.seeded_acc(N_SLOTS, bins, geo.Hs, geo.Ws, seed=99, mean=-0.2)]
    words_host = [_group_words(name, 3), torch.tensor([[0, 7, 1, 0], [1, 0, 8, 0], [1, 2, 2, 0]], dtype=torch.int32)]
    counts_host = [_sums(name)[1], torch.tensor([3, 1, LG.KEEP, 1, 1, 1, 1], dtype=torch.int32)]
    sums[1][2] = 0
    acc = torch.zeros(N_SLOTS, bins, geo.Hs, geo.Ws, dtype=torch.int64, device=DEV)
    words, counts = words_host[0].to(DEV), counts_host[0].to(DEV)
    buf, out = M._guarded((N_SLOTS, bins, h, w), torch.float32)  # (the poison of _window's: a KEEP slot keeps its bits)

    def run():
        hip.event_grid_finish_window(counts, acc, out, words, 3, crop_rows=geo.crop, resize=(geo.Hr, geo.Wr), normalize=hip.GRID_NORM_POPULATION)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for k in (0, 1, 0):
        acc.copy_(sums[k])
        words.copy_(words_host[k])
        counts.copy_(counts_host[k])
        buf.fill_(M.NAN16)
        graph.replay()
        eager, _, _ = _window(sums[k], counts_host[k], geo, LG.NORM_POPULATION, words_host[k], 3, h, w)
        assert torch.equal(_bits(out), _bits(eager)) and not bool(acc.any()) and C._guards_intact(buf, out), k
