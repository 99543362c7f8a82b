"""CPU tier of the rectified trilinear event ingest (hip.event_ingest_columns_trilinear / hip.event_ingest_ring_trilinear,
MultiStreamSegmenter(voxel='trilinear', rectify_maps=)): the numpy RESTATEMENT of the device arithmetic that the GPU tier compares
bits against -- pinned here to the reference's VoxelGrid.convert through the oracle, with a bound derived from the two sums'
roundings --, the two C entry points and their argument checks, and what the segmenter's constructor refuses."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_host_event_ingest import ROOT, SCALE_BITS, built_lib  # noqa: F401  (built_lib: the fixture)

NONE = -1  # hip.RECTIFY_NONE


# ---------------------------------------------------------------------------------------------- the restatement
def _since_first(t):
    """d = t - t_first in the column's own type (int64: modulo 2^64, float64: fp64), rounded ONCE to fp32"""
    with np.errstate(over='ignore', invalid='ignore'):
        return (t - t[0]).astype(np.float32)


def rectified(cols, rmap):
    """raw pixels -> (xe fp32, ye fp32, kept bool): rmap None: the integer pixel itself; else rmap[y, x] ([map_h, map_w, 2]) where the
    raw pixel lies inside the map, dropped where it does not.  A uint16 coordinate enters as its unsigned value."""
    x, y = cols.x.astype(np.int64), cols.y.astype(np.int64)
    if rmap is None:
        return x.astype(np.float32), y.astype(np.float32), np.ones(len(x), bool)
    mh, mw = rmap.shape[:2]
    inside = (x >= 0) & (x < mw) & (y >= 0) & (y < mh)
    v = rmap[np.where(inside, y, 0), np.where(inside, x, 0)]
    return np.ascontiguousarray(v[:, 0]), np.ascontiguousarray(v[:, 1]), inside


def contributions(cols, rmap, nb, H, W):
    """One window (t / x / y / p columns: an EventColumns, or any object with these four arrays) -> (flat voxel index int64 [m], fp32
    contribution [m]): per event u = d / d_last, tn = ((nb - 1) * (u - u_first)) / (u_last - u_first) in fp32, the test
    xe > -2 && xe < W && ye > -2 && ye < H && tn > -2 && tn < nb in front of the truncations, value from the polarity byte, and for the
    corners inside the grid wx = value * (1 - |xl - xe|), wxy = wx * (1 - |yl - ye|), c = wxy * (1 - |tb - tn|), all fp32."""
    n = len(cols.t)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    f32 = np.float32
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        d = _since_first(cols.t)
        u = d / d[n - 1]
        u_first, u_last = u[0], u[n - 1]
        tn = (f32(nb - 1) * (u - u_first)) / (u_last - u_first)
        xe, ye, kept = rectified(cols, rmap)
        kept &= (xe > f32(-2)) & (xe < f32(W)) & (ye > f32(-2)) & (ye < f32(H)) & (tn > f32(-2)) & (tn < f32(nb))
    assert d.dtype == u.dtype == tn.dtype == xe.dtype == ye.dtype == f32
    xe, ye, tn = xe[kept], ye[kept], tn[kept]
    value = np.where(np.asarray(cols.p).view(np.uint8)[kept] == 1, f32(1), f32(-1))
    x0, y0, t0 = xe.astype(np.int64), ye.astype(np.int64), tn.astype(np.int64)  # (truncation toward zero, of values inside int)
    idx, con = [], []
    for dx in (0, 1):
        xl = x0 + dx
        wx = value * (f32(1) - np.abs(xl.astype(f32) - xe))
        for dy in (0, 1):
            yl = y0 + dy
            wxy = wx * (f32(1) - np.abs(yl.astype(f32) - ye))
            for dt in (0, 1):
                tb = t0 + dt
                c = wxy * (f32(1) - np.abs(tb.astype(f32) - tn))
                assert c.dtype == f32
                m = (xl >= 0) & (xl < W) & (yl >= 0) & (yl < H) & (tb >= 0) & (tb < nb)
                idx.append((tb * H * W + yl * W + xl)[m])
                con.append(c[m])
    return np.concatenate(idx), np.concatenate(con)


def restate(cols, rmap, nb, H, W):
    """-> the grid the trilinear ingest must give, bit for bit: q = rint(c * 2^40) summed in int64 (no order: integer addition), then
    ONE conversion to fp32 and the exact scaling by 2^-40"""
    idx, c = contributions(cols, rmap, nb, H, W)
    q = np.rint(c.astype(np.float64) * 2.0 ** SCALE_BITS).astype(np.int64)
    acc = np.zeros(nb * H * W, np.int64)
    np.add.at(acc, idx, q)
    return (acc.astype(np.float32) * np.float32(2.0 ** -SCALE_BITS)).reshape(nb, H, W)


class Cols:
    """four raw columns that need not pass EventColumns' checks (polarity bytes 2 and 255, say)"""
    __slots__ = ('t', 'x', 'y', 'p', 'n', 'format')

    def __init__(self, t, x, y, p):
        self.t, self.x, self.y, self.p, self.n = t, x, y, p, len(t)
        self.format = (1 if t.dtype == np.int64 else 0) | (2 if x.dtype == np.uint16 else 0)


def synthetic_map(mh, mw, H, W, seed=0):
    """a smooth distortion [mh, mw, 2] of a sensor mh x mw onto a grid H x W that overshoots it on every side: coordinates from below
    -2 to above W + 1 (H + 1), so some events land in (-2, 0) and some in [W - 1, W + 1)"""
    g = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(mh, dtype=np.float64), np.arange(mw, dtype=np.float64), indexing='ij')
    a, b = g.uniform(0.2, 0.3, 2)
    xe = -2.1 + xs * (W + 3.3) / (mw - 1) + a * np.sin(0.4 * ys + seed)
    ye = -2.1 + ys * (H + 3.3) / (mh - 1) + b * np.cos(0.3 * xs + seed)
    return np.stack([xe, ye], -1).astype(np.float32)


def raw_events(n, mh, mw, seed, fmt=3, t_span_us=50_000):
    """n raw sensor events over a sensor mh x mw in the dtypes of format word fmt: sorted int64 microseconds with an offset (or
    float64 seconds), pixels inside the sensor, polarity bytes 0 / 1 -> EventColumns"""
    from ess_amd.datasets.data_util import EventColumns
    g = np.random.default_rng(seed)
    us = np.sort(g.integers(0, t_span_us, n)).astype(np.int64) + 1_600_000_000_000_000
    t = us if fmt & 1 else us.astype(np.float64) * 1e-6
    xy = np.uint16 if fmt & 2 else np.int16
    return EventColumns(t, g.integers(0, mw, n).astype(xy), g.integers(0, mh, n).astype(xy), g.integers(0, 2, n).astype(np.uint8))


# ---------------------------------------------------------------------------------------------- the restatement against the oracle
@pytest.mark.parametrize('fmt', [3, 0], ids=['t_i64', 't_f64'])
@pytest.mark.parametrize('nb', [2, 5])
def test_restatement_against_the_oracle_within_the_derived_bound(nb, fmt):
    """The oracle (VoxelGrid.convert restated, pinned to tests/golden/voxel.pt) is handed what the DSEC loader hands VoxelGrid.convert:
    the map's coordinates of every event and u = fp32(t - t_first) / last.  Its contributions are the restatement's fp32 values; the
    sums differ.  Per voxel with k contributions c_i the oracle adds them one after the other in fp32: k - 1 roundings (the first
    addition, to zero, is exact), an error of at most gamma_(k-1) * sum |c_i| with gamma_m = m u / (1 - m u), u = 2^-24 (Higham,
    Accuracy and Stability, Lemma 3.1), and gamma_(k-1) <= k u while k (k - 1) u <= 1.  The restatement adds exact integers and
    rounds once: u * |sum| <= u * sum |c_i|; each c_i was quantised to a multiple of 2^-40 before: at most 2^-41 each (none at all
    for |c_i| >= 2^-16).  Together |oracle - restatement| <= (k + 1) * 2^-24 * sum |c_i| + k * 2^-41."""
    from oracle import ess_oracle as O
    H, W, mh, mw = 24, 40, 28, 44
    rmap = synthetic_map(mh, mw, H, W)
    cols = raw_events(3000, mh, mw, 7 + nb, fmt)
    xe, ye, inside = rectified(cols, rmap)
    assert inside.all()
    assert np.any((xe > -2) & (xe < 0)) and np.any((xe >= W - 1) & (xe < W + 1)) and np.any((ye > -2) & (ye < 0)) and np.any(ye >= H - 1)
    d = _since_first(cols.t)
    u = d / d[-1]
    pol = (cols.p == 1).astype(np.float32)
    oracle = O.voxel_grid_trilinear(torch.from_numpy(xe), torch.from_numpy(ye), torch.from_numpy(pol), torch.from_numpy(u), nb, H, W)
    oracle = oracle.numpy().astype(np.float64).ravel()
    fixed = restate(cols, rmap, nb, H, W).astype(np.float64).ravel()
    idx, c = contributions(cols, rmap, nb, H, W)
    k = np.bincount(idx, minlength=nb * H * W).astype(np.float64)
    mag = np.bincount(idx, weights=np.abs(c.astype(np.float64)), minlength=nb * H * W)
    assert k.max() * (k.max() - 1) * 2.0 ** -24 <= 1
    bound = (k + 1) * 2.0 ** -24 * mag + k * 2.0 ** -41
    err = np.abs(fixed - oracle)
    print(f'nb {nb} fmt {fmt}: {len(idx)} contributions, max k {int(k.max())}, max |fixed - oracle| {err.max():.3e}, '
          f'min slack {np.min(bound - err):.3e}, max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}')
    assert int(k.max()) >= 4 and np.count_nonzero(fixed) > 1000
    assert np.all(err <= bound)
    assert np.all(fixed[k == 0] == 0) and np.all(oracle[k == 0] == 0)


def test_restatement_without_a_map_is_the_grid_of_integer_pixels():
    """RECTIFY_NONE: xe = (float)x -- at most two non-zero contributions per event, both on the event's own pixel"""
    H, W, nb = 24, 40, 5
    cols = raw_events(500, H, W, 3)
    idx, c = contributions(cols, None, nb, H, W)
    nz = c != 0
    pix = (idx % (H * W))[nz]
    assert set(pix.tolist()) <= set((cols.y.astype(np.int64) * W + cols.x.astype(np.int64)).tolist())
    assert cols.n < np.count_nonzero(nz) <= 2 * cols.n
    grid = restate(cols, None, nb, H, W)
    assert grid.any() and grid.shape == (nb, H, W)
    # a window whose last time equals its first: NaN throughout, an all-zero grid (no dT = 1 rescue)
    same = Cols(np.full(8, 5, np.int64), cols.x[:8], cols.y[:8], cols.p[:8])
    assert not restate(same, None, nb, H, W).any()


# ---------------------------------------------------------------------------------------------- ABI and the C argument checks
def test_the_trilinear_entry_points_are_exported_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in ('ess_event_ingest_columns_trilinear', 'ess_event_ingest_ring_trilinear'):
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header
    assert hip.lib().ess_version() == 110
    assert 'ESS_RECTIFY_NONE = -1' in header and hip.RECTIFY_NONE == NONE
    assert callable(hip.event_ingest_columns_trilinear) and callable(hip.event_ingest_ring_trilinear)


def _refusals(L, call):
    """the rectify arguments' checks, the same for both entry points"""
    P = ctypes.c_void_p
    assert call(map_of=P(0)) == -22 and b'null map_of' in L.ess_last_error()
    assert call(n_maps=-1) == -22 and b'n_maps=-1' in L.ess_last_error()
    assert call(maps=P(0), n_maps=2) == -22 and b'n_maps=2' in L.ess_last_error() and b'maps' in L.ess_last_error()
    assert call(n_maps=0) == -22 and b'n_maps=0' in L.ess_last_error()  # (maps given, none counted)
    assert call(maps=P(4104)) == -22 and b'maps must be 16-byte aligned' in L.ess_last_error()
    for mh, mw in ((0, 44), (28, 0), (-1, 44), (32769, 44), (28, 32769)):
        assert call(map_height=mh, map_width=mw) == -22, (mh, mw)
        msg = L.ess_last_error()
        assert f'map_height={mh} map_width={mw}'.encode() in msg and b'1..32768' in msg, msg


def test_columns_trilinear_argument_errors_come_before_any_launch(built_lib):
    """every refusal needs no device: the pointers are never followed"""
    from ess_amd import hip
    L, P = hip.lib(), ctypes.c_void_p
    a = P(4096)
    need = 5 * 24 * 40 * 8

    def call(t=a, p=a, counts=a, formats=a, stride=16, n_streams=1, acc=a, acc_bytes=need, out=a, maps=a, map_of=a, n_maps=1,
             map_height=28, map_width=44):
        return L.ess_event_ingest_columns_trilinear(t, a, a, p, counts, formats, stride, n_streams, 5, 24, 40, acc, acc_bytes, out, maps,
                                                    map_of, n_maps, map_height, map_width, P(0))
    for null in ('t', 'p', 'counts', 'formats', 'acc', 'out'):
        assert call(**{null: P(0)}) == -22 and b'event_ingest_columns_trilinear: null' in L.ess_last_error(), null
    for stride in (0, -16, 24, (1 << 22) + 16):
        assert call(stride=stride) == -22 and f'stride={stride}'.encode() in L.ess_last_error(), stride
    assert call(stride=24) == -22 and b'multiple of 16' in L.ess_last_error()
    assert call(p=P(4097)) == -22 and b'16-byte aligned' in L.ess_last_error()
    assert call(acc_bytes=need - 8) == -22 and b'acc has' in L.ess_last_error()
    assert call(n_streams=0) == -22 and b'n_streams=0' in L.ess_last_error()
    _refusals(L, call)


def test_ring_trilinear_argument_errors_come_before_any_launch(built_lib):
    from ess_amd import hip
    L, P = hip.lib(), ctypes.c_void_p
    a = P(4096)
    need = 5 * 24 * 40 * 8

    def call(t=a, p=a, rows=a, starts=a, counts=a, formats=a, ring=16, n_rows=1, n_slots=1, acc=a, acc_bytes=need, out=a, maps=a, map_of=a,
             n_maps=1, map_height=28, map_width=44):
        return L.ess_event_ingest_ring_trilinear(t, a, a, p, rows, starts, counts, formats, ring, n_rows, n_slots, 5, 24, 40, acc, acc_bytes,
                                                 out, maps, map_of, n_maps, map_height, map_width, P(0))
    for null in ('t', 'p', 'rows', 'starts', 'counts', 'formats', 'acc', 'out'):
        assert call(**{null: P(0)}) == -22 and b'event_ingest_ring_trilinear: null' in L.ess_last_error(), null
    for ring in (0, -16, 8, 24, (1 << 22) + 16):
        assert call(ring=ring) == -22 and f'ring={ring}'.encode() in L.ess_last_error(), ring
    assert call(out=P(4100)) == -22 and b'16-byte aligned' in L.ess_last_error()
    assert call(n_slots=2) == -22 and b'acc has' in L.ess_last_error()
    assert call(n_slots=0) == -22 and b'n_slots=0' in L.ess_last_error()
    assert call(n_rows=0) == -22 and b'n_rows=0' in L.ess_last_error()
    _refusals(L, call)


def test_the_binding_refuses_host_tensors_and_bad_maps():
    """what hip.event_ingest_*_trilinear refuse about maps / map_of, in front of the library"""
    from ess_amd import hip
    ok = (torch.zeros(3, dtype=torch.int32),)
    for maps, map_of, match in ((torch.zeros(1, 28, 44, 2, dtype=torch.float64), None, 'maps must be a non-empty fp32'),
                                (torch.zeros(28, 44, 2), None, 'maps must be a non-empty fp32'),
                                (torch.zeros(1, 28, 44, 3), None, 'maps must be a non-empty fp32'),
                                (np.zeros((1, 28, 44, 2), np.float32), None, 'maps must be a non-empty fp32'),
                                (None, torch.zeros(2, dtype=torch.int32), r'map_of must be int32 \[3\]'),
                                (None, torch.zeros(3, dtype=torch.int64), r'map_of must be int32 \[3\]'),
                                (torch.zeros(1, 28, 44, 2), ok[0], 'no CPU path'), (None, ok[0], 'no CPU path')):
        with pytest.raises(hip.EssHipError, match=match):
            hip._rectify_args('event_ingest_columns_trilinear', maps, map_of, 3, torch.device('cpu'))


# ---------------------------------------------------------------------------------------------- the segmenter's constructor
def test_the_constructor_refuses_trilinear_without_columns():
    from ess_amd import hip
    from ess_amd.run_segmentation import VOXEL_FLAVOURS, _voxel_flavour
    assert VOXEL_FLAVOURS == ('temporal', 'trilinear')
    for layout, cap in (('records', None), ('records', 512), ('columns', 512), ('ring', 512)):
        assert _voxel_flavour('temporal', layout, cap) == 'temporal'
    assert _voxel_flavour('trilinear', 'columns', 512) == _voxel_flavour('trilinear', 'ring', 512) == 'trilinear'
    with pytest.raises(hip.EssHipError, match=r"event_layout='columns' or 'ring'.*'records'"):
        _voxel_flavour('trilinear', 'records', 512)
    with pytest.raises(hip.EssHipError, match='event_capacity=N'):
        _voxel_flavour('trilinear', 'records', None)
    with pytest.raises(hip.EssHipError, match="voxel='bilinear'"):
        _voxel_flavour('bilinear', 'columns', 512)


def test_the_constructor_refuses_bad_rectify_maps():
    from ess_amd import hip
    from ess_amd.run_segmentation import _rectify_maps
    m = synthetic_map(28, 44, 24, 40)
    assert _rectify_maps(None, 'temporal', 3) == (None, [NONE] * 3) and _rectify_maps(None, 'trilinear', 2) == (None, [NONE] * 2)
    with pytest.raises(hip.EssHipError, match="rectify_maps belongs to voxel='trilinear'"):
        _rectify_maps([m, m, None], 'temporal', 3)
    with pytest.raises(hip.EssHipError, match='got 2, .* n_streams=3'):
        _rectify_maps([m, m], 'trilinear', 3)
    with pytest.raises(hip.EssHipError, match='got ndarray'):
        _rectify_maps(m, 'trilinear', 3)
    with pytest.raises(hip.EssHipError, match=r'rectify_maps\[1\] must be float32.*float64'):
        _rectify_maps([None, m.astype(np.float64), None], 'trilinear', 3)
    for bad in (m[..., 0], np.zeros((28, 44, 3), np.float32), np.zeros((0, 44, 2), np.float32), np.zeros((2, 28, 44, 2), np.float32)):
        with pytest.raises(hip.EssHipError, match=r'rectify_maps\[0\] must be \[map_h, map_w, 2\]'):
            _rectify_maps([bad, None, None], 'trilinear', 3)
    with pytest.raises(hip.EssHipError, match=r'rectify_maps\[2\] is \(30, 44, 2\), the maps before it \(28, 44, 2\)'):
        _rectify_maps([m, None, synthetic_map(30, 44, 24, 40)], 'trilinear', 3)
    with pytest.raises(hip.EssHipError, match=r'rectify_maps\[1\] must be a float32 array or tensor'):
        _rectify_maps([m, [[1.0, 2.0]], None], 'trilinear', 3)


def test_entries_that_are_the_same_object_share_one_map():
    from ess_amd.run_segmentation import _rectify_maps
    left, right = synthetic_map(28, 44, 24, 40, 1), synthetic_map(28, 44, 24, 40, 2)
    maps, map_of = _rectify_maps([left, right, left, None, right, left], 'trilinear', 6)
    assert tuple(maps.shape) == (2, 28, 44, 2) and maps.dtype == torch.float32 and maps.is_contiguous()
    assert map_of == [0, 1, 0, NONE, 1, 0]
    assert np.array_equal(maps[0].numpy(), left) and np.array_equal(maps[1].numpy(), right)
    # a replay farm of one camera: one map; tensors and arrays alike; an equal COPY is another object, hence another map
    one = torch.from_numpy(left)
    maps, map_of = _rectify_maps([one] * 4, 'trilinear', 4)
    assert tuple(maps.shape) == (1, 28, 44, 2) and map_of == [0] * 4
    maps, map_of = _rectify_maps([left, left.copy()], 'trilinear', 2)
    assert tuple(maps.shape) == (2, 28, 44, 2) and map_of == [0, 1]
    maps, map_of = _rectify_maps([None, None], 'trilinear', 2)
    assert maps is None and map_of == [NONE, NONE]
