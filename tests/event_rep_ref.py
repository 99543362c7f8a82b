"""The numpy RESTATEMENT of the event ingest's two further representations (hip.event_ingest_columns_rep / _ring_rep), mirroring
tests/test_host_event_ingest.py's contributions / restate for the signed grid: what the device must give, bit for bit.

    'separate_pol': 2 * bins planes [positive bins; negative bins], both halves non-negative (generate_voxel_grid(separate_pol=True));
    'histogram':    2 planes [negative counts, positive counts] (generate_event_histogram), the time column not read;
    'signed':       the existing grid (test_host_event_ingest.contributions on the same events), for the identity between the two.

cols: anything with the four raw columns .t (float64 or int64), .x / .y (int16 or uint16), .p (one byte per event) -- an
EventColumns, or a Cols of arrays an EventColumns would refuse (a 0xFF polarity byte, say).  A polarity is positive where its BYTE
equals 1."""
import collections

import numpy as np

SCALE_BITS = 40
REPRESENTATIONS = ('signed', 'separate_pol', 'histogram')
Cols = collections.namedtuple('Cols', 't x y p')


def channels(representation, bins):
    return {'signed': bins, 'separate_pol': 2 * bins, 'histogram': 2}[representation]


def _words(cols):
    """-> (t float64, x int64, y int64, positive bool) as the loader reads the raw words"""
    t = np.asarray(cols.t)
    pos = np.ascontiguousarray(np.asarray(cols.p)).view(np.uint8) == 1
    return t.astype(np.float64), np.asarray(cols.x).astype(np.int64), np.asarray(cols.y).astype(np.int64), pos


def contributions(cols, representation, bins, H, W, sign_halves=False, swap_halves=False, pos_first=False):
    """-> (flat voxel index int64 [m] into [C, H, W], fp32 contribution [m]).  The three keywords are the deliberate MUTATIONS the
    host test proves the goldens can tell apart: the sign applied in the halves, the halves swapped, [pos, neg] histogram order."""
    t, x, y, pos = _words(cols)
    n, plane = len(t), H * W
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    inside = (x < W) & (x >= 0) & (y < H) & (y >= 0)
    if representation == 'histogram':
        ch = np.where(pos, 0, 1) if pos_first else np.where(pos, 1, 0)
        return (x + y * W + ch * plane)[inside], np.ones(int(inside.sum()), np.float32)
    first = t[0]
    dT = t[n - 1] - first
    if dT == 0:
        dT = 1.0
    with np.errstate(invalid='ignore'):
        ts = (float(bins - 1) * (t - first)) / dT
        valid = inside & (ts >= 0) & (ts < bins)
    ts, x, y, pos = ts[valid], x[valid], y[valid], pos[valid]
    ti = ts.astype(np.int64)
    dts = ts - ti
    left, right = (1.0 - dts).astype(np.float32), dts.astype(np.float32)
    if representation == 'signed' or sign_halves:
        sign = np.where(pos, np.float32(1), np.float32(-1))
        left, right = sign * left, sign * right
    half = np.zeros(len(ts), np.int64)
    if representation == 'separate_pol':
        half = np.where(pos, bins, 0) if swap_halves else np.where(pos, 0, bins)
    base = x + y * W + (half + ti) * plane
    has_right = ti + 1 < bins
    return np.concatenate([base, (base + plane)[has_right]]), np.concatenate([left, right[has_right]])


def restate_sums(cols, representation, bins, H, W, **mutation):
    """-> int64 [C, H, W]: the sums the scatter leaves in acc, q = rint(c * 2^40) added as integers (no order)"""
    C = channels(representation, bins)
    idx, c = contributions(cols, representation, bins, H, W, **mutation)
    q = np.rint(c.astype(np.float64) * 2.0 ** SCALE_BITS).astype(np.int64)
    acc = np.zeros(C * H * W, np.int64)
    np.add.at(acc, idx, q)
    return acc.reshape(C, H, W)


def dequantise(sums):
    """ONE conversion to fp32 and the exact scaling by 2^-40"""
    return sums.astype(np.float32) * np.float32(2.0 ** -SCALE_BITS)


def restate(cols, representation, bins, H, W, **mutation):
    """-> fp32 [C, H, W]: the grid the plain ingest must give, bit for bit"""
    return dequantise(restate_sums(cols, representation, bins, H, W, **mutation))


def columns_of_rows(ev):
    """[n, 4] float64 rows (t, x, y, polarity 0 / 1) as R.events / R.one_pixel_events give them -> Cols(float64, int16, int16, uint8)"""
    return Cols(np.ascontiguousarray(ev[:, 0]), ev[:, 1].astype(np.int16), ev[:, 2].astype(np.int16), ev[:, 3].astype(np.uint8))
