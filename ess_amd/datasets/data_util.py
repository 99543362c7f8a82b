"""
Device-side counterparts of datasets/data_util.py (reference): voxel grids with bilinear interpolation in time
(`generate_voxel_grid`, :54-126) and the non-zero normalisation (`normalize_voxel_grid`, :38-51).

Inputs are CUDA tensors; there is no host path (the reference's numpy code is restated in oracle/ for the tests).  The host
functions lay events out for the device and do nothing more: pack_event_records writes [N, 4] rows as the 16-byte records
hip.event_ingest reads; EventColumns / stage_event_columns hand the columns a camera delivers to hip.event_ingest_columns as they are.
"""
import numpy as np
import torch

from .. import hip


def normalize_voxel_grid(events):
    """Non-zero mean/std normalisation of ONE voxel grid tensor (any shape), data_util.py:38-51."""
    return hip.voxel_normalize_(events.clone().view(1, -1), mode=1).view(events.shape)


def generate_voxel_grid(events, shape, nr_temporal_bins, separate_pol=True):
    """events: [N, 4] float64 CUDA tensor, columns (x, y, t, polarity) as the reference indexes them
    (data_util.py:78-85) -> [2*bins or bins, H, W] float32."""
    return generate_voxel_grid_batch(events, [0, events.shape[0]], shape, nr_temporal_bins, separate_pol)[0]


def generate_voxel_grid_batch(events, slice_offsets, shape, nr_temporal_bins, separate_pol=True, normalize=False):
    """All slices of a batch in one launch -> [n_slices, 2*bins or bins, H, W]."""
    height, width = shape
    assert events.dim() == 2 and events.shape[1] == 4
    assert nr_temporal_bins > 0 and width > 0 and height > 0
    ev = events.to(torch.float64)
    x = ev[:, 0].to(torch.int32).contiguous()  # astype(int): truncation
    y = ev[:, 1].to(torch.int32).contiguous()
    t = ev[:, 2].contiguous()
    pol = ev[:, 3].to(torch.float32).contiguous()
    with torch.no_grad():
        return hip.voxel_grid_temporal(x, y, t, pol, slice_offsets, nr_temporal_bins, height, width, separate_pol, normalize)


def generate_input_representation(events, event_representation, shape, nr_temporal_bins=5, separate_pol=True):
    """data_util.py:6-14 (the histogram representation is not on the ESS path)."""
    if event_representation == 'voxel_grid':
        return generate_voxel_grid(events, shape, nr_temporal_bins, separate_pol)
    raise NotImplementedError(f'event representation {event_representation!r} is not part of the ESS hot path')


_COORD_MIN, _COORD_MAX = -1, 32767  # the record's int16 coordinates; the kernel drops both ends (W, H <= 32767)


def pack_event_records(events, out):
    """events: [N, 4] rows (t, x, y, polarity) of any numeric dtype, numpy or torch (host) -> out[:N], `out` a 1-D numpy array of
    hip.EVENT_RECORD (a view of pinned staging memory, say).  Vectorised numpy on the host, no torch launch.  Coordinates are
    truncated toward zero as astype(int) does and clamped to [-1, 32767] (NaN: -1) -- both ends lie outside every grid; polarity 0
    becomes -1, as generate_voxel_grid has it; any polarity outside {-1, 0, 1} is refused, and so are more rows than `out` holds.
    -> N"""
    ev = events.detach().cpu().numpy() if torch.is_tensor(events) else np.asarray(events)
    if ev.ndim != 2 or ev.shape[1] != 4 or ev.dtype.kind not in 'fiub':
        raise hip.EssHipError(f'pack_event_records: events must be numeric [N, 4] rows (t, x, y, polarity), got {ev.dtype}{tuple(ev.shape)}')
    if not isinstance(out, np.ndarray) or out.dtype != hip.EVENT_RECORD or out.ndim != 1:
        raise hip.EssHipError('pack_event_records: out must be a 1-D numpy array of hip.EVENT_RECORD')
    n = ev.shape[0]
    if n > len(out):
        raise hip.EssHipError(f'pack_event_records: {n} events do not fit the {len(out)} records of out')
    # every column is first copied out of the row-major rows (the strided read is the expensive part), then worked on in place
    p = np.array(ev[:, 3], dtype=np.float64)
    with np.errstate(invalid='ignore'):
        pi = p.astype(np.int8)
    if n and not (bool((pi == p).all()) and pi.min() >= -1 and pi.max() <= 1):
        raise hip.EssHipError('pack_event_records: a polarity outside {-1, 0, 1}')
    rec = out[:n]
    rec['t'] = ev[:, 0]
    rec['x'] = _record_coordinate(ev[:, 1])
    rec['y'] = _record_coordinate(ev[:, 2])
    rec['p'] = pi | -(pi == 0).view(np.int8)  # 0 -> -1
    return n


def _record_coordinate(col):
    """fmax / fmin: a NaN coordinate becomes -1; the cast truncates toward zero, and truncation commutes with a clamp to integer
    bounds"""
    c = np.array(col, dtype=np.float64)
    np.fmax(c, _COORD_MIN, out=c)
    np.fmin(c, _COORD_MAX, out=c)
    return c.astype(np.int16)


class EventColumns:
    """One window of events as the four columns an event camera or a DSEC / DDD17 file delivers: t float64 or int64 (any unit; an
    int64 time must stay below 2^53 in magnitude), x and y both int16 or both uint16, p int8, uint8 or bool (1: positive, anything
    else: negative).  Four 1-D, equal-length, C-contiguous host arrays -- numpy, or CPU torch tensors viewed as numpy without a copy
    -- held as they are and checked ONCE, here: the polarity check is one min / max over the byte column.  Immutable; .format is the
    device word hip.event_ingest_columns reads for a stream that delivers these dtypes, .n the number of events."""
    __slots__ = ('t', 'x', 'y', 'p', 'n', 'format')

    def __init__(self, t, x, y, p):
        cols = [c.numpy() if torch.is_tensor(c) and not c.is_cuda else c for c in (t, x, y, p)]
        for name, c in zip('txyp', cols):
            if not isinstance(c, np.ndarray) or c.ndim != 1:
                raise hip.EssHipError(f'EventColumns: {name} must be a 1-D host array (numpy or a CPU tensor), got '
                                      f'{type(c).__name__}{tuple(getattr(c, "shape", ()))}')
            if not c.flags.c_contiguous:
                raise hip.EssHipError(f'EventColumns: {name} must be contiguous')
        t, x, y, p = cols
        if not len(t) == len(x) == len(y) == len(p):
            raise hip.EssHipError(f'EventColumns: the columns have unequal lengths {[len(c) for c in cols]}')
        if t.dtype not in (np.float64, np.int64):
            raise hip.EssHipError(f'EventColumns: t must be float64 or int64, got {t.dtype}')
        if x.dtype != y.dtype or x.dtype not in (np.int16, np.uint16):
            raise hip.EssHipError(f'EventColumns: x and y must both be int16 or both uint16, got {x.dtype} and {y.dtype}')
        if p.dtype not in (np.int8, np.uint8, np.bool_):
            raise hip.EssHipError(f'EventColumns: polarity p must be int8, uint8 or bool, got {p.dtype}')
        if len(p) and p.dtype != np.bool_:
            lo, hi = int(p.min()), int(p.max())
            if hi > 1 or lo < -1:
                raise hip.EssHipError(f'EventColumns: a polarity outside {"{-1, 0, 1}" if p.dtype == np.int8 else "{0, 1}"} ({p.dtype} column, min {lo}, max {hi})')
        fmt = (hip.EVCOL_T_I64 if t.dtype == np.int64 else 0) | (hip.EVCOL_XY_U16 if x.dtype == np.uint16 else 0)
        for name, v in zip(self.__slots__, (t, x, y, p, len(t), fmt)):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError('EventColumns is immutable')

    def __len__(self):
        return self.n

    @classmethod
    def from_rows(cls, events):
        """[N, 4] rows (t, x, y, polarity) of any numeric dtype -> EventColumns(float64, int16, int16, int8).  The SLOW way, for
        convenience and for tests: the rows go through pack_event_records (its truncation, its clamp to [-1, 32767], its polarity
        0 -> -1 and its refusals) and the columns are copied out of the records."""
        n = events.shape[0] if hasattr(events, 'shape') and len(events.shape) == 2 else 0
        rec = np.empty(n, dtype=hip.EVENT_RECORD)
        pack_event_records(events, rec)
        return cls(np.ascontiguousarray(rec['t']), np.ascontiguousarray(rec['x']), np.ascontiguousarray(rec['y']), rec['p'].astype(np.int8))


def stage_event_columns(cols, t_view, x_view, y_view, p_view):
    """cols (EventColumns) -> the first cols.n entries of four 1-D numpy views (of pinned staging memory, say): t_view 8 raw bytes
    per event, x_view / y_view 2, p_view 1; each is written through a view of the column's own dtype, so an int64 time and a float64
    time both arrive as their own bits.  Four copies, nothing else: no cast, no clamp, no temporary; nothing behind cols.n is
    written, and more events than the views hold are refused before anything is.  -> cols.n"""
    if not isinstance(cols, EventColumns):
        raise hip.EssHipError(f'stage_event_columns: an EventColumns is needed, got {type(cols).__name__}')
    views = (t_view, x_view, y_view, p_view)
    for name, v, size in zip('txyp', views, (8, 2, 2, 1)):
        if not isinstance(v, np.ndarray) or v.ndim != 1 or v.dtype.itemsize != size or not v.flags.c_contiguous:
            raise hip.EssHipError(f'stage_event_columns: the {name} view must be a contiguous 1-D numpy array of {size}-byte items')
    n = cols.n
    room = min(len(v) for v in views)
    if n > room:
        raise hip.EssHipError(f'stage_event_columns: {n} events do not fit the {room} entries of the views')
    for c, v in zip((cols.t, cols.x, cols.y, cols.p), views):
        np.copyto(v[:n].view(c.dtype), c)
    return n
