"""CPU tier of the event ingest (hip.event_ingest, MultiStreamSegmenter(event_capacity=)): the 16-byte record and its host packing,
the two C entry points, and the numpy RESTATEMENT of the device arithmetic that the GPU tier compares bits against -- checked here
against the oracle's sequential fp32 sum with a bound derived from the two sums' roundings, not from what either gives."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_BITS = 40


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


# ---------------------------------------------------------------------------------------------- the restatement
def contributions(rec, nb, H, W):
    """One stream's records (hip.EVENT_RECORD) -> (flat voxel index int64 [m], fp32 contribution [m]): per event the double
    expressions of voxel_temporal_kernel -- ts = ((nb - 1) * (t - first)) / dT, ti = int(ts), dts = ts - ti, left = fp32(1 - dts),
    right = fp32(dts), the sign from the polarity, the same validity test; first / last = the times of record 0 / record n - 1,
    dT == 0 -> 1.  The right half of an event in the last bin is dropped."""
    n = len(rec)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    t = rec['t'].astype(np.float64)
    x, y, p = rec['x'].astype(np.int64), rec['y'].astype(np.int64), rec['p']
    first = t[0]
    dT = t[n - 1] - first
    if dT == 0:
        dT = 1.0
    with np.errstate(invalid='ignore'):
        ts = (float(nb - 1) * (t - first)) / dT
        valid = (x < W) & (x >= 0) & (y < H) & (y >= 0) & (ts >= 0) & (ts < nb)
    ts, x, y, p = ts[valid], x[valid], y[valid], p[valid]
    ti = ts.astype(np.int64)
    dts = ts - ti
    sign = np.where(p == 1, np.float32(1), np.float32(-1))
    left, right = sign * (1.0 - dts).astype(np.float32), sign * dts.astype(np.float32)
    assert left.dtype == right.dtype == np.float32
    base = x + y * W
    has_right = ti + 1 < nb
    return (np.concatenate([base + ti * W * H, (base + (ti + 1) * W * H)[has_right]]), np.concatenate([left, right[has_right]]))


def restate(rec, nb, H, W):
    """-> the grid hip.event_ingest must give, bit for bit: q = rint(c * 2^40) summed in int64 (no order: integer addition),
    then ONE conversion to fp32 and the exact scaling by 2^-40"""
    idx, c = contributions(rec, nb, H, W)
    q = np.rint(c.astype(np.float64) * 2.0 ** SCALE_BITS).astype(np.int64)
    acc = np.zeros(nb * H * W, np.int64)
    np.add.at(acc, idx, q)
    return (acc.astype(np.float32) * np.float32(2.0 ** -SCALE_BITS)).reshape(nb, H, W)


def events(n, H, W, seed):
    """[n, 4] rows (t, x, y, polarity in {0, 1}), times sorted, pixels inside H x W"""
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(0.0, 0.2, n))
    return np.stack([t, g.integers(0, W, n).astype(np.float64), g.integers(0, H, n).astype(np.float64),
                     g.integers(0, 2, n).astype(np.float64)], 1)


def one_pixel_events(n, seed, x=7, y=11):
    g = np.random.default_rng(seed)
    t = np.sort(g.uniform(1.0, 1.5, n))
    return np.stack([t, np.full(n, float(x)), np.full(n, float(y)), g.integers(0, 2, n).astype(np.float64)], 1)


def packed(ev, capacity=None):
    from ess_amd import hip
    from ess_amd.datasets.data_util import pack_event_records
    out = np.zeros(len(ev) if capacity is None else capacity, dtype=hip.EVENT_RECORD)
    assert pack_event_records(ev, out) == len(ev)
    return out


# ---------------------------------------------------------------------------------------------- record and packing
def test_event_record_layout():
    from ess_amd import hip
    r = hip.EVENT_RECORD
    assert r.itemsize == 16
    assert {k: (r.fields[k][0].str, r.fields[k][1]) for k in r.names} == {'t': ('<f8', 0), 'x': ('<i2', 8), 'y': ('<i2', 10), 'p': ('<i4', 12)}
    assert hip.INGEST_KEEP == -1


@pytest.mark.parametrize('as_torch', [False, True])
def test_pack_event_records_truncates_clamps_and_maps_polarity(as_torch):
    from ess_amd import hip
    from ess_amd.datasets.data_util import pack_event_records
    ev = np.array([[0.5, -0.5, 3.9, 0], [0.75, -1.2, 40000.0, 1], [1.0, -9.0, 32767.9, -1], [1.25, 32768.0, -1.0, 1], [1.5, 0.99, 23.0, 0]])
    out = np.zeros(8, dtype=hip.EVENT_RECORD)
    out['p'] = 77
    assert pack_event_records(torch.from_numpy(ev) if as_torch else ev, out) == 5
    assert out['t'][:5].tolist() == [0.5, 0.75, 1.0, 1.25, 1.5]
    assert out['x'][:5].tolist() == [0, -1, -1, 32767, 0]       # -0.5 -> 0, -1.2 -> -1, -9 -> clamp -1, 32768 -> clamp 32767
    assert out['y'][:5].tolist() == [3, 32767, 32767, -1, 23]   # 3.9 -> 3, 40000 -> clamp
    assert out['p'][:5].tolist() == [-1, 1, -1, 1, -1]          # polarity 0 -> -1
    assert out['p'][5:].tolist() == [77, 77, 77]                # nothing behind out[:N] is written
    # integer and float32 rows pack alike
    iev = np.array([[3, 5, 7, 1], [4, -3, 2, 0]], dtype=np.int64)
    a, b = np.zeros(2, dtype=hip.EVENT_RECORD), np.zeros(2, dtype=hip.EVENT_RECORD)
    pack_event_records(iev, a)
    pack_event_records(iev.astype(np.float32), b)
    assert a.tobytes() == b.tobytes() and a['x'].tolist() == [5, -1] and a['p'].tolist() == [1, -1]
    assert pack_event_records(np.zeros((0, 4)), out) == 0


def test_pack_event_records_refuses_bad_polarity_and_overflow():
    from ess_amd import hip
    from ess_amd.datasets.data_util import pack_event_records
    out = np.zeros(4, dtype=hip.EVENT_RECORD)
    for bad in (0.5, 2.0, -3.0, float('nan')):
        with pytest.raises(hip.EssHipError, match='polarity'):
            pack_event_records(np.array([[0.0, 1, 1, 1], [0.1, 1, 1, bad]]), out)
    with pytest.raises(hip.EssHipError, match=r'\b5 events\b.*\b4 records\b'):
        pack_event_records(events(5, 8, 8, 0), out)
    with pytest.raises(hip.EssHipError, match=r'\[N, 4\]'):
        pack_event_records(np.zeros((3, 3)), out)
    with pytest.raises(hip.EssHipError, match='EVENT_RECORD'):
        pack_event_records(events(2, 8, 8, 0), np.zeros((4, 16), np.uint8))


def test_segmenter_refuses_a_bad_event_capacity():
    from ess_amd import hip
    from ess_amd.run_segmentation import _event_capacity
    assert _event_capacity(1, 480, 640) == 1 and _event_capacity(1 << 22, 32767, 32767) == 1 << 22
    for bad in (0, -1, (1 << 22) + 1, 4096.0, True, '4096'):
        with pytest.raises(hip.EssHipError, match='event_capacity'):
            _event_capacity(bad, 480, 640)
    with pytest.raises(hip.EssHipError, match='int16'):
        _event_capacity(4096, 480, 32768)
    with pytest.raises(hip.EssHipError, match='int16'):
        _event_capacity(4096, 32768, 640)


# ---------------------------------------------------------------------------------------------- ABI
def test_ingest_entry_points_are_exported_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    for name in ('ess_event_ingest_workspace', 'ess_event_ingest'):
        assert hasattr(lib, name) and name in hip.EXPORTS
    assert hip.lib().ess_version() == 110
    L = hip.lib()
    assert L.ess_event_ingest_workspace(8, 5, 480, 640) == 8 * 5 * 480 * 640 * 8
    assert L.ess_event_ingest_workspace(0, 5, 480, 640) == 0
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    assert 'ESS_INGEST_KEEP = -1' in header


# ---------------------------------------------------------------------------------------------- the restatement against the oracle
@pytest.mark.parametrize('case', ['spread', 'one_pixel'])
def test_restatement_against_the_oracle_within_the_derived_bound(case):
    """Per voxel with n contributions c_i: the oracle adds them one after the other in fp32 (n - 1 roundings, relative error u =
    2^-24 each), the restatement adds exact integers and rounds once -- together at most n roundings of partial sums bounded by
    sum |c_i|: gamma_n * sum |c_i| with gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, Lemma 3.1) -- and each c_i was
    quantised to a multiple of 2^-40: at most 2^-41 each.  In-range events only (the oracle does not guard coordinates)."""
    from oracle import ess_oracle as O
    nb, H, W = 5, 24, 40
    ev = events(3000, H, W, 5) if case == 'spread' else one_pixel_events(2000, 6)
    rec = packed(ev)
    fixed = restate(rec, nb, H, W).astype(np.float64).ravel()
    oracle = O.events_to_voxel_grid(ev, nb, W, H).numpy().astype(np.float64).ravel()
    idx, c = contributions(rec, nb, H, W)
    n = np.bincount(idx, minlength=nb * H * W).astype(np.float64)
    mag = np.bincount(idx, weights=np.abs(c.astype(np.float64)), minlength=nb * H * W)
    u = 2.0 ** -24
    bound = (n * u / (1 - n * u)) * mag + n * 2.0 ** -41
    err = np.abs(fixed - oracle)
    print(f'{case}: max n {int(n.max())}, max |fixed - oracle| {err.max():.3e}, min slack {np.min(bound - err):.3e}, '
          f'max err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}')
    assert int(n.max()) >= (1000 if case == 'one_pixel' else 2)
    assert np.all(err <= bound)
    assert np.all(fixed[n == 0] == 0) and np.all(oracle[n == 0] == 0)
