"""
Device-side counterparts of datasets/data_util.py (reference): voxel grids with bilinear interpolation in time
(`generate_voxel_grid`, :54-126) and the non-zero normalisation (`normalize_voxel_grid`, :38-51).

Inputs are CUDA tensors; there is no host path (the reference's numpy code is restated in oracle/ for the tests).  The one host
function is pack_event_records: it lays event rows out as the 16-byte records hip.event_ingest reads, nothing more.
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
