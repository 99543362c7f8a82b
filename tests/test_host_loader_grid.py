"""CPU tier of the loader finish (csrc/voxel_ingest.hip: ess_event_scatter_ring*, ess_event_grid_finish) and of the two cuts by time
(ess_amd/datasets/event_feed.py): the ABI, the refusals of the library and of the bindings in front of any device, the cuts against
restatements of the loaders' lines, and the CHECK ITSELF -- tests/loader_grid_ref.py's fp32 restatement of the kernels' arithmetic
passes every bound, each seeded defect misses one by four times or more on a row named for it (the factor of
tests/test_host_norm_check.py), and torch's F.interpolate and the oracle's VoxelGrid(normalize=True) pass the same bounds."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loader_grid_ref as LG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = LG.Geometry


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)

# the geometries of the GPU table (tests/test_hip_loader_grid.py), by name
GEOMETRIES = {
    'one': G((1, 1), (1, 1)),
    'scale0': G((3, 2), (5, 1)),
    'wide': G((2, 7), (2, 9)),
    'ddd17': G((72, 90), (72, 96), rows=64),
    'dsec': G((72, 96), (64, 96), crop=60),
    'identity': G((6, 10)),
    'identity_odd': G((3, 5)),
}
MODES = {'none': LG.NORM_NONE, 'unbiased': LG.NORM_UNBIASED, 'population': LG.NORM_POPULATION}


@functools.lru_cache(maxsize=None)
def _case(geo_name, bins, n_slots, mode, mean=0.5):
    """(acc, counts, ref, bound) of a table row, built once: seeded sums whose bottom rows (those a crop drops) are three times the
    others', the special slots where there are seven"""
    geo = GEOMETRIES[geo_name]
    acc = LG.seeded_acc(n_slots, bins, geo.Hs, geo.Ws, seed=len(geo_name) * 100 + bins * 10 + n_slots, mean=mean)
    acc[:, :, geo.crop:] *= 3
    counts = None
    if n_slots >= 7:
        acc, counts = LG.special_slots(acc)
    ref, bound = LG.reference(acc, geo, MODES[mode], counts)
    return acc, counts, ref, bound


# ---------------------------------------------------------------------------------------------- ABI and the C argument checks
NEW = ('ess_event_scatter_ring', 'ess_event_scatter_ring_trilinear', 'ess_event_grid_finish_workspace', 'ess_event_grid_finish')


def test_the_entry_points_are_declared_exported_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NEW:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'{name}(' in header, name
    assert 'The LOADER\'s grid from the ring ingest -- PURELY ADDITIVE to ABI 110' in header
    assert 'ESS_GRID_NORM_NONE = 0, ESS_GRID_NORM_UNBIASED = 1, ESS_GRID_NORM_POPULATION = 2' in header
    assert (hip.GRID_NORM_NONE, hip.GRID_NORM_UNBIASED, hip.GRID_NORM_POPULATION) == (0, 1, 2)
    assert hip.lib().ess_version() == 110
    for fn in ('event_scatter_ring', 'event_scatter_ring_trilinear', 'event_grid_finish'):
        assert callable(getattr(hip, fn))


def test_the_workspace_follows_from_the_slot_size_alone(built_lib):
    """16 bytes of statistics a slot and 24 a workgroup; the workgroups a slot from bins x rows x columns, 4096 voxels each, at most 64"""
    from ess_amd import hip
    L = hip.lib()
    per_slot = {n: L.ess_event_grid_finish_workspace(n, 5, 72, 96) // n for n in (1, 7, 160)}
    assert len(set(per_slot.values())) == 1 and per_slot[1] == 16 + 24 * 9  # 34 560 voxels: 9 workgroups
    assert L.ess_event_grid_finish_workspace(1, 1, 1, 1) == 16 + 24
    assert L.ess_event_grid_finish_workspace(1, 5, 480, 640) == 16 + 24 * 64
    for bad in ((0, 5, 72, 96), (1, 0, 72, 96), (1, 5, -1, 96), (1, 5, 72, 0)):
        assert L.ess_event_grid_finish_workspace(*bad) == 0


def test_scatter_argument_errors_come_before_any_launch(built_lib):
    """every refusal needs no device: the pointers are never followed"""
    from ess_amd import hip
    L, P = hip.lib(), ctypes.c_void_p
    a = P(4096)
    need = 5 * 24 * 40 * 8

    def temporal(t=a, p=a, rows=a, starts=a, counts=a, formats=a, ring=16, n_rows=1, n_slots=1, acc=a, acc_bytes=need):
        return L.ess_event_scatter_ring(t, a, a, p, rows, starts, counts, formats, ring, n_rows, n_slots, 5, 24, 40, acc, acc_bytes, P(0))

    def trilinear(t=a, p=a, rows=a, starts=a, counts=a, formats=a, ring=16, n_rows=1, n_slots=1, acc=a, acc_bytes=need, maps=a, map_of=a,
                  n_maps=1, map_height=28, map_width=44):
        return L.ess_event_scatter_ring_trilinear(t, a, a, p, rows, starts, counts, formats, ring, n_rows, n_slots, 5, 24, 40, acc, acc_bytes,
                                                  maps, map_of, n_maps, map_height, map_width, P(0))
    for call, name in ((temporal, b'event_scatter_ring: '), (trilinear, b'event_scatter_ring_trilinear: ')):
        for null in ('t', 'p', 'rows', 'starts', 'counts', 'formats', 'acc'):
            assert call(**{null: P(0)}) == -22 and name + b'null' in L.ess_last_error(), null
        assert b'or acc' in L.ess_last_error() and b'out' not in L.ess_last_error()
        for ring in (0, -16, 8, 24, (1 << 22) + 16):
            assert call(ring=ring) == -22 and f'ring={ring}'.encode() in L.ess_last_error(), ring
        assert call(acc=P(4104)) == -22 and b't, x, y, p, acc must be 16-byte aligned' in L.ess_last_error()
        assert call(n_slots=2) == -22 and b'acc has' in L.ess_last_error()
        assert call(n_slots=0) == -22 and b'n_slots=0' in L.ess_last_error()
        assert call(n_rows=0) == -22 and b'n_rows=0' in L.ess_last_error()
    assert trilinear(map_of=P(0)) == -22 and b'null map_of' in L.ess_last_error()
    assert trilinear(maps=P(4104)) == -22 and b'maps must be 16-byte aligned' in L.ess_last_error()
    assert trilinear(map_height=0) == -22 and b'map_height=0' in L.ess_last_error()


def test_grid_finish_argument_errors_come_before_any_launch(built_lib):
    from ess_amd import hip
    L, P = hip.lib(), ctypes.c_void_p
    a = P(4096)
    bins, Hs, Ws = 5, 72, 96
    need, ws_need = bins * Hs * Ws * 8, L.ess_event_grid_finish_workspace(1, bins, Hs, Ws)

    def call(counts=a, n_slots=1, bins=bins, src_height=Hs, src_width=Ws, acc=a, acc_bytes=need, crop_rows=60, resize_height=64,
             resize_width=96, out_rows=64, normalize=1, out=a, workspace=a, workspace_bytes=ws_need):
        return L.ess_event_grid_finish(counts, n_slots, bins, src_height, src_width, acc, acc_bytes, crop_rows, resize_height, resize_width,
                                       out_rows, normalize, out, workspace, workspace_bytes, P(0))
    for null in ('counts', 'acc', 'out', 'workspace'):
        assert call(**{null: P(0)}) == -22 and b'event_grid_finish: null' in L.ess_last_error(), null
    for name in ('acc', 'out', 'workspace'):
        assert call(**{name: P(4104)}) == -22 and b'16-byte aligned' in L.ess_last_error(), name
    for n in (0, -1, 65536):
        assert call(n_slots=n) == -22 and f'n_slots={n}'.encode() in L.ess_last_error()
    for kw in (dict(bins=0), dict(src_height=0), dict(src_width=-3)):
        assert call(**kw) == -22 and b'must be positive' in L.ess_last_error(), kw
    for kw in (dict(resize_height=0), dict(resize_width=0)):
        assert call(**kw) == -22 and b'resize_height=' in L.ess_last_error(), kw
    for crop in (0, -1, Hs + 1):
        assert call(crop_rows=crop) == -22 and f'crop_rows={crop} (1..src_height={Hs})'.encode() in L.ess_last_error(), crop
    for rows in (0, 65):
        assert call(out_rows=rows) == -22 and f'out_rows={rows} (1..resize_height=64)'.encode() in L.ess_last_error(), rows
    for mode in (-1, 3):
        assert call(normalize=mode) == -22 and f'normalize={mode}'.encode() in L.ess_last_error(), mode
    assert call(acc_bytes=need - 8) == -22 and b'acc has' in L.ess_last_error()
    assert call(workspace_bytes=ws_need - 1) == -22 and b'workspace has' in L.ess_last_error()
    assert call(n_slots=2) == -22 and b'acc has' in L.ess_last_error()


def test_the_bindings_refuse_in_front_of_the_library():
    """shape and dtype before the device: everything below is said about host tensors"""
    from ess_amd import hip
    i32 = functools.partial(torch.zeros, dtype=torch.int32)
    acc, out, counts = torch.zeros(3, 2, 8, 12, dtype=torch.int64), torch.zeros(3, 2, 6, 16), i32(3)
    for kw, match in ((dict(acc=acc.int()), 'acc must be a non-empty int64'), (dict(acc=acc[0]), 'acc must be a non-empty int64'),
                      (dict(crop_rows=9), r'crop_rows=9 must be an int in \[1, 8\]'), (dict(crop_rows=True), 'crop_rows=True'),
                      (dict(resize=(7,)), 'resize=.* must be a pair'), (dict(resize=(0, 16)), 'must be a pair of positive ints'),
                      (dict(resize=(5, 16)), r'out must be fp32 \[3, 2, rows <= 5, 16\]'),
                      (dict(resize=(7, 12)), r'out must be fp32 \[3, 2, rows <= 7, 12\]'),
                      (dict(resize=(7, 16), out=out.double()), 'out must be fp32'),
                      (dict(resize=(7, 16), out=out[:2]), r'out must be fp32 \[3, 2'),
                      (dict(resize=(7, 16), normalize=3), 'normalize=3 must be'),
                      (dict(resize=(7, 16), counts=i32(2)), r'counts must be int32 \[3\]'),
                      (dict(resize=(7, 16), counts=counts.long()), r'counts must be int32 \[3\]'),
                      (dict(resize=(7, 16)), 'no CPU path'), (dict(counts=None), 'counts must be a CUDA')):
        args = dict(dict(counts=counts, acc=acc, out=out), **kw)
        with pytest.raises(hip.EssHipError, match='event_grid_finish: .*' + match):
            hip.event_grid_finish(args.pop('counts'), args.pop('acc'), args.pop('out'), **args)
    t = torch.zeros(2, 32, dtype=torch.int64)
    x, p, w = torch.zeros(2, 32, dtype=torch.int16), torch.zeros(2, 32, dtype=torch.uint8), i32(3)
    for fn, tail in ((hip.event_scatter_ring, ()), (hip.event_scatter_ring_trilinear, (None, None))):
        name = fn.__name__
        for args, match in (((t, x, x, p, w, w, w, w, acc.float()), 'acc must be a non-empty int64'),
                            ((t, x, x, p, w, w, w, w, acc.view(-1)), 'acc must be a non-empty int64'),
                            ((t[0], x, x, p, w, w, w, w, acc), r't must be \[n_rows, ring\]'),
                            ((t, x.int(), x, p, w, w, w, w, acc), 'x must be torch.int16'),
                            ((t, x, x, p[:, :16], w, w, w, w, acc), 'p must be'),
                            ((t, x, x, p, w, i32(2), w, w, acc), r'starts must be int32 \[3\]'),
                            ((t[:, :24], x[:, :24], x[:, :24], p[:, :24], w, w, w, w, acc), 'ring=24 must be a multiple of 16'),
                            ((t, x, x, p, w, w, w, w, acc), 'no CPU path'), ((t, x, x, p, w, w, w, None, acc), 'formats must be a CUDA')):
            with pytest.raises(hip.EssHipError, match=name + ': .*' + match):
                fn(*args, *tail)


# ---------------------------------------------------------------------------------------------- the cuts by time
def _times(kind, n, seed, step=40):
    """n sorted times: 'i64' microseconds with runs of duplicates, 'f64' the same as float seconds-like values"""
    g = np.random.default_rng(seed)
    t = np.cumsum(g.integers(0, step, n) * (g.random(n) < 0.7)).astype(np.int64) + 1_000_000
    return t if kind == 'i64' else t.astype(np.float64) + 0.25 * (g.random(n) < 0.5)


def _ring_of(t, head, ring):
    """the ring's time column after events [0, head) have been fed"""
    r = np.zeros(ring, dtype=t.dtype)
    for k in range(max(0, head - ring), head):
        r[k % ring] = t[k]
    return r


@pytest.mark.parametrize('kind', ['i64', 'f64'])
@pytest.mark.parametrize('T', [1, 5])
def test_fixed_duration_windows_against_the_loader(kind, T):
    """absolute (start, count) equal the loader's two searches per window: on a boundary that is a run of duplicate times, with an
    empty window (a gap), with a duration that does not divide (a true division), before the first and after the last event"""
    from ess_amd.datasets.event_feed import sequence_windows_fixed_duration
    t = _times(kind, 600, 3)
    t[300:] += 5000  # a gap: windows without events
    dup = int(np.flatnonzero(np.diff(t) == 0)[5])
    assert t[dup] == t[dup + 1]
    n_checked = n_empty = 0
    for head in (600, 400):
        ring = _ring_of(t, head, 1024)
        for d in (700, 333, 2500 / 3, 1):
            if kind == 'i64' and d != int(d) and T == 1:
                continue
            for t_end in (t[dup], t[dup] + T * d, t[head - 1] + 1, t[0] + 1, t[350], t[0] - 10, float(t[200]) + 0.5):
                if kind == 'i64':
                    t_end = int(t_end) if float(t_end) == int(t_end) else t_end
                want = LG.loader_cut_fixed_duration(t[:head], t_end, T, T * d)
                got = sequence_windows_fixed_duration(ring, head, 1024, t_end, T, d)
                assert got == [(a, b - a) for a, b in want], (kind, T, head, d, t_end)
                n_checked += 1
                n_empty += sum(c == 0 for _, c in got)
    assert n_checked >= 40 and n_empty > 0


def test_fixed_duration_windows_on_a_wrapped_ring():
    """a ring of 256 after 600 events keeps [344, 600): windows inside it equal the loader's on the whole recording; a sequence whose
    first bound is at or before the oldest kept event is refused"""
    from ess_amd import hip
    from ess_amd.datasets.event_feed import sequence_windows_fixed_duration
    for kind in ('i64', 'f64'):
        t = _times(kind, 600, 4)
        ring = _ring_of(t, 600, 256)
        T = 4
        span = float(t[599] - t[400])
        d = int(span / T)
        t_end = t[599] + 1
        got = sequence_windows_fixed_duration(ring, 600, 256, t_end, T, d)
        want = LG.loader_cut_fixed_duration(t, t_end, T, T * d)
        assert got == [(a, b - a) for a, b in want] and got[0][0] > 344 and any(a % 256 > (a + c) % 256 for a, c in got if c)
        with pytest.raises(hip.EssHipError, match='not after the oldest kept event'):
            sequence_windows_fixed_duration(ring, 600, 256, t[344] + T * d, T, d)
        with pytest.raises(hip.EssHipError, match='not after the oldest kept event'):
            sequence_windows_fixed_duration(ring, 600, 256, t[100] + T * d, T, d)
    for bad in (dict(window_duration=0), dict(window_duration=-1.0), dict(window_duration=True), dict(T=0), dict(t_end=float('nan'))):
        kw = dict(dict(t_ring=ring, head=600, ring=256, t_end=t_end, T=4, window_duration=10), **bad)
        with pytest.raises(hip.EssHipError, match='sequence_windows_fixed_duration'):
            sequence_windows_fixed_duration(**kw)
    with pytest.raises(hip.EssHipError, match='1-D int64 or float64'):
        sequence_windows_fixed_duration(ring.astype(np.float32), 600, 256, t_end, 4, 10)


@pytest.mark.parametrize('kind', ['i64', 'f64'])
@pytest.mark.parametrize('T', [1, 5])
def test_windows_by_time_against_the_loader(kind, T):
    """the DDD17 rule on [begin, end): duplicates on a boundary, an empty window (a gap), a delta of 0 (a span below T units)"""
    from ess_amd.datasets.event_feed import sequence_windows_by_time
    t = _times(kind, 500, 7)
    t[250:] += 9000
    n_empty = 0
    for begin, end in ((0, 500), (13, 400), (100, 101), (240, 260), (7, 8 + T)):
        want = LG.loader_cut_by_time(t[begin:end], T)
        got = sequence_windows_by_time(t, begin, end, T)
        assert got == [(begin + a, b - a) for a, b in want], (kind, T, begin, end)
        assert got[0][0] == begin and all(got[i][0] + got[i][1] == got[i + 1][0] for i in range(T - 1)) and got[-1][0] + got[-1][1] <= end
        n_empty += sum(c == 0 for _, c in got)
    # a boundary that falls on a run of duplicates: the run goes to the LATER window (searchsorted's left side)
    d = np.array([0, 10, 10, 10, 20, 20, 30, 40], dtype=np.int64 if kind == 'i64' else np.float64)
    assert sequence_windows_by_time(d, 0, 8, 4) == [(0, 1), (1, 3), (4, 2), (6, 1)] == \
        [(a, b - a) for a, b in LG.loader_cut_by_time(d, 4)]
    # delta == 0: every bound is t[0], every window empty
    z = np.array([5, 5, 6, 7], dtype=d.dtype)
    assert sequence_windows_by_time(z, 0, 4, 5) == [(0, 0)] * 5 == [(a, b - a) for a, b in LG.loader_cut_by_time(z, 5)]
    assert n_empty > 0 or T == 1


def test_windows_by_time_refusals():
    from ess_amd import hip
    from ess_amd.datasets.event_feed import sequence_windows_by_time
    t = _times('i64', 50, 1)
    for args in ((t, 10, 10, 3), (t, -1, 10, 3), (t, 0, 51, 3), (t, 0, 50, 0), (list(t), 0, 50, 3), (t.reshape(5, 10), 0, 5, 3)):
        with pytest.raises(hip.EssHipError, match='sequence_windows_by_time'):
            sequence_windows_by_time(*args)


# ---------------------------------------------------------------------------------------------- the check itself
ROWS = [(g, b, n, m) for g in ('ddd17', 'dsec') for b in (1, 5) for n in (1, 7) for m in MODES if (b, n) in ((1, 7), (5, 1))] + \
       [(g, 5, 7, m) for g in ('one', 'scale0', 'wide', 'identity', 'identity_odd') for m in MODES]


@pytest.mark.parametrize('geo,bins,n_slots,mode', ROWS, ids=['-'.join(map(str, r)) for r in ROWS])
def test_the_fp32_restatement_passes_every_bound(geo, bins, n_slots, mode):
    acc, counts, ref, bound = _case(geo, bins, n_slots, mode)
    got = LG.restate(acc, GEOMETRIES[geo], MODES[mode], counts)
    r = LG.worst_ratio(got, ref, bound)
    assert r <= 1.0, (geo, bins, n_slots, mode, r)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n_slots, bins, GEOMETRIES[geo].rows, GEOMETRIES[geo].Wr)
    if counts is not None:  # the special slots do what the derivation says of them
        assert bool(torch.isnan(got[1]).all()) and not bool(got[2].any())
        if mode == 'unbiased':
            assert not bool(got[3].any()) and not bool(got[4].any())  # (one voxel, equal voxels: v - mean = 0)
        if mode == 'population':
            assert bool(torch.isnan(got[4]).any()) and not bool(torch.isnan(got[5]).any())
    if mode == 'none' and GEOMETRIES[geo].identity:
        assert torch.equal(got.view(torch.int32), LG.dequantise(acc).view(torch.int32)[:, :, :GEOMETRIES[geo].rows] if counts is None
                           else torch.where(torch.isnan(got), got, LG.dequantise(acc)).view(torch.int32))


# defect -> (geometry, mode): a row on which it must show
DEFECT_ROWS = {'stats_cropped': ('dsec', 'unbiased'), 'biased': ('ddd17', 'unbiased'), 'zeros_too': ('ddd17', 'population'),
               'half_pixel': ('ddd17', 'none'), 'resize_first': ('dsec', 'none'), 'bottom_rows': ('ddd17', 'none')}


@pytest.mark.parametrize('defect', LG.DEFECTS)
def test_a_seeded_defect_misses_a_bound_four_times_over(defect):
    geo, mode = DEFECT_ROWS[defect]
    acc, counts, ref, bound = _case(geo, 5, 1, mode)
    clean = LG.worst_ratio(LG.restate(acc, GEOMETRIES[geo], MODES[mode], counts), ref, bound)
    bad = LG.worst_ratio(LG.restate(acc, GEOMETRIES[geo], MODES[mode], counts, defect=defect), ref, bound)
    assert clean <= 1.0 and bad >= 4.0, (defect, clean, bad)


def test_every_defect_has_a_row():
    assert set(DEFECT_ROWS) == set(LG.DEFECTS)


RESIZES = [((72, 90), (72, 96)), ((60, 96), (64, 96)), ((260, 346), (260, 352)), ((440, 640), (448, 640)), ((1, 7), (1, 9)), ((3, 2), (5, 1))]


@pytest.mark.parametrize('src,dst', RESIZES, ids=[f'{a[0]}x{a[1]}-{b[0]}x{b[1]}' for a, b in RESIZES])
def test_torch_interpolate_passes_the_resize_bound(src, dst):
    """F.interpolate(mode='bilinear', align_corners=True), what the loaders call, stays inside 4 u sum |w| |v| of the fp64 blend with
    its own fp32 weights; and the crop of top rows commutes bitwise with a resize that keeps the height"""
    g = torch.Generator().manual_seed(src[0] * 7 + src[1])
    v = torch.randn(2, *src, generator=g) * (torch.rand(2, *src, generator=g) < 0.4)
    geo = G(src, dst)
    ref, mag = LG.resize_ref(v.double(), geo)
    got = F.interpolate(v[None], size=dst, mode='bilinear', align_corners=True)[0]
    assert LG.worst_ratio(got, ref, 4 * LG.U24 * mag) <= 1.0
    if src[0] == dst[0] and src[0] > 8:
        keep = src[0] - 8
        top = F.interpolate(v[None, :, :keep], size=(keep, dst[1]), mode='bilinear', align_corners=True)[0]
        assert torch.equal(top.view(torch.int32), got[:, :keep].view(torch.int32))


def test_the_oracle_voxel_grid_normalisation_passes_the_bound():
    """oracle.voxel_grid_trilinear(normalize=True) -- VoxelGrid.convert's own normalisation, fp32 mean and std by torch -- against the
    fp64 reference of the unnormalised grid, inside the bound derived for the kernel."""
    from oracle import ess_oracle as O
    g = torch.Generator().manual_seed(11)
    n, C, H, W = 4000, 5, 24, 40
    x, y = torch.rand(n, generator=g) * (W + 1) - 1, torch.rand(n, generator=g) * (H + 1) - 1
    pol = (torch.rand(n, generator=g) < 0.6).float()
    t = torch.sort(torch.rand(n, generator=g))[0] * 1e5
    plain = O.voxel_grid_trilinear(x, y, pol, t, C, H, W, normalize=False)
    got = O.voxel_grid_trilinear(x, y, pol, t, C, H, W, normalize=True)
    ref, bound = LG.normalise_ref(plain, LG.NORM_UNBIASED)
    assert LG.worst_ratio(got, ref, bound) <= 1.0
    assert float((got.double() - plain.double()).abs().max()) > 0.1  # (it did normalise)
