"""Shared by tests/test_host_loader_grid.py (CPU tier), tests/test_hip_loader_grid.py and tests/test_hip_sequence_loader.py (GPU
tier): the loader finish of csrc/voxel_ingest.hip (ess_event_grid_finish) restated -- a float64 reference with the bound of every
output voxel, a CPU fp32 restatement of the kernels' arithmetic with injectable defects, seeded int64 sums, and the literal
restatements of the two loaders' cuts by time.  A plain helper module: no fixtures, no collection hooks.

What is compared.  The kernel reads int64 sums q; v = fl32(q) 2^-40 is bit-defined (one round-to-nearest conversion, an exact
scaling), so the reference starts from the SAME fp32 v, in float64.  u = 2^-24: one fp32 rounding, relative to what it rounds.

Normalisation (over the non-zero voxels of ALL source rows).  Reference: n, m = sum v / n, and s = sqrt(sum (v - m)^2 / (n - 1))
('unbiased', VoxelGrid(normalize=True)) or s = sqrt(sum v^2 / n - m^2) ('population', normalize_voxel_grid), all in float64;
y* = (v - m) / s where s > 0, else v - m ('unbiased': also where n == 1, torch's NaN std failing "std > 0"); 'population' divides
unguarded, so s == 0 gives NaN at every non-zero voxel.  Zeros stay zero (voxel_apply_kernel's case analysis; the loader's
mask * (v - m) / s differs from it only where s is 0 or NaN).
The kernel: count and sum are exact integers, so its fp64 mean carries one fp64 division (and one int64 -> fp64 conversion): 2^-52
relative; fm = fl32(mean): |fm - m| <= (u + 2^-52) |m|.
  'unbiased':   var' = (sq - n mean^2) / (n - 1) in fp64, sq a sum of n exact squares in a fixed order: |sq - sum v^2| <= n 2^-53 sum v^2,
                n mean^2 two roundings; the difference cancels against var (n - 1):  relative error of var' <= 1.5 n 2^-53 (var + m^2) / var
                =: 2 e_s (norm_ref's rstd term);  fs = fl32(sqrt(var')): |fs - s| / s <= u + e_s + 2^-52.
  'population': fs = sqrtf(fl32(sq / n) - fm fm) in fp32, unfused: E = sq / n rounded (u E), fm^2 with fm's rounding (2 u m^2) and
                its own (u m^2), the difference rounded (u var): relative error of fs^2 <= u (E + 3 m^2 + var) / var = u (2 + 4 m^2 / var),
                the root halves it and rounds once:  |fs - s| / s <= u (2 + 2 m^2 / var) + e_s.
  the map:      d = fl32(v - fm) (u |v - fm|), y = fl32(d / fs) (u |y|).  With rel_s the bound on |fs - s| / s above,
                |y - y*| <= (2 u + rel_s) |y*| + (u + 2^-52) |m| / s,   times (1 + 2^-10) for the second-order terms
                (where nothing is divided: s = 1, rel_s = 0).
Where var == 0 (one non-zero voxel, or all of them equal) the conditioning is infinite and the comparison is of NaN positions and
exact zeros: E[v^2] and mean^2 are then the same fp32 number (v^2 rounded once, the kernel does not fuse the two), so the kernel's
population std is exactly 0 like the reference's, and its unbiased variance exactly 0 while n v^2 is exact in fp64 (n <= 32).

Resize (align_corners=True).  Source index and weights are torch's fp32 expressions, bit-defined: scale = fl32((in - 1) / (out - 1))
(0 where out == 1), src = fl32(scale dst), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = fl32(src - i0), l0 = fl32(1 - l1).  The
reference blends the four taps with THESE weights in float64; the kernel's l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11) has four
roundings on its deepest path (product, inner sum, outer product, outer sum), each relative to a partial magnitude <= sum |w| |v|:
    |out - ref| <= 4 u sum_taps |w| |v|    (+ the taps' own normalisation bounds, blended with the same weights)
A tap with weight 0 still multiplies: a NaN tap makes a NaN output in the kernel, in torch and in this reference alike.
The crop of top rows commutes bitwise with a resize that keeps the height (scale 1: src = dst exactly, l1 = 0)."""
import numpy as np
import torch

U24 = 2.0 ** -24
U53 = 2.0 ** -53
SCALE = 2.0 ** 40
NORM_NONE, NORM_UNBIASED, NORM_POPULATION = 0, 1, 2
KEEP = -1


# ------------------------------------------------------------------------------------------------------------------ geometry
class Geometry:
    """src (Hs, Ws) -> rows [0, crop) -> resize (Hr, Wr) -> rows [0, rows)"""

    def __init__(self, src, resized=None, crop=None, rows=None):
        self.Hs, self.Ws = src
        self.crop = self.Hs if crop is None else crop
        self.Hr, self.Wr = (self.crop, self.Ws) if resized is None else resized
        self.rows = self.Hr if rows is None else rows
        assert 1 <= self.crop <= self.Hs and 1 <= self.rows <= self.Hr

    @property
    def identity(self):
        return self.crop == self.Hs == self.Hr == self.rows and self.Wr == self.Ws

    def __repr__(self):
        return f'{self.Hs}x{self.Ws}[:{self.crop}]->{self.Hr}x{self.Wr}[:{self.rows}]'


def source_index(n_in, n_out, align_corners=True):
    """torch's fp32 source index and weights of every output index -> (i0, i1 int64, l0, l1 float32), numpy float32 arithmetic:
    one rounding per operation, no fused multiply-add.  align_corners=False (a seeded defect only): the half-pixel rule."""
    f = np.float32
    dst = np.arange(n_out, dtype=np.float32)
    if align_corners:
        scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
        src = scale * dst
    else:
        scale = f(n_in) / f(n_out)
        src = np.maximum(scale * (dst + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l0), torch.from_numpy(l1)


def _blend(y, n_out_h, n_out_w, dtype, align_corners=True):
    """y [..., h, w] -> [..., n_out_h, n_out_w]: the four-tap blend in `dtype` with the fp32 weights (fp32: one rounding per
    operation, as the kernel with contraction off)"""
    y0, y1, ly0, ly1 = source_index(y.shape[-2], n_out_h, align_corners)
    x0, x1, lx0, lx1 = source_index(y.shape[-1], n_out_w, align_corners)
    ly0, ly1 = ly0.to(dtype)[:, None], ly1.to(dtype)[:, None]
    lx0, lx1 = lx0.to(dtype), lx1.to(dtype)
    r0, r1 = y[..., y0, :], y[..., y1, :]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    return ly0 * top + ly1 * bot


def resize_ref(y, geo):
    """fp64 y [..., crop, Ws] -> (ref, sum |w| |v|) [..., Hr, Wr]"""
    return _blend(y, geo.Hr, geo.Wr, torch.float64), _blend(y.abs(), geo.Hr, geo.Wr, torch.float64)


# ------------------------------------------------------------------------------------------------------------------ reference
def dequantise(acc):
    """int64 sums -> the fp32 values the finish starts from (bit-defined)"""
    return acc.to(torch.float32) * np.float32(2.0 ** -40)


def normalise_ref(v32, mode):
    """one slot's fp32 grid v [bins, Hs, Ws] -> (y* fp64, its bound fp64) by the derivation in the module docstring"""
    v = v32.double()
    nz = v != 0
    n = int(nz.sum())
    if mode == NORM_NONE or n == 0:
        return v, torch.zeros_like(v)
    vals = v[nz]
    m = vals.sum() / n
    var_p = ((vals - m) ** 2).sum() / n  # (the centred form: no cancellation in the reference)
    m2 = float(m * m)
    if mode == NORM_UNBIASED:
        var = float(((vals - m) ** 2).sum() / (n - 1)) if n > 1 else float('nan')
        s = var ** 0.5 if var > 0 else 1.0  # (NaN or 0: subtract only)
        divides = var > 0
        rel_s = (U24 + 0.75 * n * U53 * (var + m2) / var + 2 * U53) if divides else 0.0
    else:
        var = float(var_p)
        s = var ** 0.5  # (0: 0 / 0 and x / 0 below, as the kernel)
        divides = True
        rel_s = (U24 * (2 + 2 * m2 / var) + 0.75 * n * U53 * (var + m2) / var) if var > 0 else 0.0
    y = torch.where(nz, (v - m) / s if divides else v - m, v)
    s_b = s if s > 0 else 1.0
    bound = torch.where(nz, (2 * U24 + rel_s) * y.abs() + (U24 + 2 * U53) * float(m.abs()) / s_b, torch.zeros_like(v)) * (1 + 2.0 ** -10)
    return y, bound


def reference(acc, geo, mode, counts=None):
    """acc int64 [n, bins, Hs, Ws] -> (ref, bound) fp64 [n, bins, rows, Wr]; a KEEP slot's rows are NaN in ref (the poison)"""
    out, bnd = [], []
    for i in range(acc.shape[0]):
        if counts is not None and counts[i] < 0:
            z = torch.full((acc.shape[1], geo.rows, geo.Wr), float('nan'), dtype=torch.float64)
            out.append(z)
            bnd.append(torch.zeros_like(z))
            continue
        y, b = normalise_ref(dequantise(acc[i]), mode)
        y, b = y[:, :geo.crop], b[:, :geo.crop]
        if geo.crop == geo.Hr and geo.Ws == geo.Wr:
            r, mag, bb = y, torch.zeros_like(y), b  # (no resize: scale 1 in both axes, the blend returns the tap)
        else:
            r, mag = resize_ref(y, geo)
            bb = _blend(b, geo.Hr, geo.Wr, torch.float64)
        out.append(r[:, :geo.rows])
        bnd.append((bb + 4 * U24 * torch.nan_to_num(mag, nan=0.0, posinf=0.0))[:, :geo.rows])
    return torch.stack(out), torch.stack(bnd)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite reference voxels (0 / 0 counts as 0); NaN positions must agree -> the ratio, inf where
    they do not"""
    got = got.double().cpu()
    if got.shape != ref.shape or not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return float('inf')
    ok = ~torch.isnan(ref)
    err = (got - ref).abs()[ok]
    b = bound[ok]
    if not bool(((err == 0) | (b > 0)).all()):
        return float('inf')
    r = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------ the fp32 restatement
DEFECTS = ('stats_cropped', 'biased', 'zeros_too', 'half_pixel', 'resize_first', 'bottom_rows')


def _stat(q, mode, defect=None):
    """one slot's int64 sums -> (fm, fs, divide, active) as grid_stats_finalize_kernel gives them: exact integer count and sum, fp64
    sum of exact squares, voxel_apply_kernel's expressions (the fp32 ones unfused)"""
    f = q.to(torch.float32)
    nz = f != 0
    n = int(nz.sum())
    if n == 0:
        return np.float32(0), np.float32(1), False, False
    total = float(int(f[nz].to(torch.int64).sum())) * 2.0 ** -40
    sq = float(((f[nz] * np.float32(2.0 ** -40)).double() ** 2).sum())
    mean = total / n
    fm = np.float32(mean)
    if mode == NORM_UNBIASED:
        den = n if defect == 'biased' else n - 1
        var = (sq - n * mean * mean) / den if (n > 1 or defect == 'biased') else -1.0
        sd = var ** 0.5 if var > 0 else 0.0
        return fm, np.float32(sd), sd > 0, True
    with np.errstate(invalid='ignore'):
        fs = np.sqrt(np.float32(sq / n) - fm * fm, dtype=np.float32)
    return fm, np.float32(fs), True, True


def restate(acc, geo, mode, counts=None, defect=None):
    """the kernels' arithmetic in fp32 on the CPU -> fp32 [n, bins, rows, Wr] (a KEEP slot: NaN, the poison).  defect: one of DEFECTS"""
    assert defect is None or defect in DEFECTS
    out = []
    for i in range(acc.shape[0]):
        if counts is not None and counts[i] < 0:
            out.append(torch.full((acc.shape[1], geo.rows, geo.Wr), float('nan'), dtype=torch.float32))
            continue
        v = dequantise(acc[i])
        if mode != NORM_NONE:
            fm, fs, divide, active = _stat(acc[i, :, :geo.crop] if defect == 'stats_cropped' else acc[i], mode, defect)
            if active:
                with np.errstate(invalid='ignore', divide='ignore'):
                    y = (v - fm) / fs if divide else v - fm
                v = y if defect == 'zeros_too' else torch.where(v != 0, y, v)
        if defect == 'resize_first':  # all source rows are resized, and the crop's share of them is kept behind it
            v = _blend(v, geo.Hr, geo.Wr, torch.float32)
        else:
            v = v[:, :geo.crop]
            if not (geo.crop == geo.Hr and geo.Ws == geo.Wr):
                v = _blend(v, geo.Hr, geo.Wr, torch.float32, align_corners=defect != 'half_pixel')
            elif defect == 'half_pixel':
                v = _blend(v, geo.Hr, geo.Wr, torch.float32, align_corners=False)
        out.append(v[:, geo.Hr - geo.rows:] if defect == 'bottom_rows' else v[:, :geo.rows])
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------------------------ inputs
def seeded_acc(n_slots, bins, Hs, Ws, seed, density=0.3, mean=0.0):
    """int64 sums as a few events per voxel leave them: `density` of the voxels non-zero, values of magnitude up to ~4 at scale 2^40
    with all 40 fraction bits in use, centred on `mean`; every slot has its own scale (a slot normalised with another's statistics
    is off by far more than a bound)"""
    g = torch.Generator().manual_seed(seed)
    shape = (n_slots, bins, Hs, Ws)
    val = (torch.randn(shape, generator=g, dtype=torch.float64) + mean) * (1 + 0.5 * torch.arange(n_slots, dtype=torch.float64)).view(-1, 1, 1, 1)
    q = torch.round(val * SCALE).to(torch.int64)
    on = torch.rand(shape, generator=g) < density
    return torch.where(on, q, torch.zeros_like(q))


def special_slots(acc):
    """acc [n >= 7, ...] -> (acc, counts): slot 1 INGEST_KEEP (its sums zero, as the contract has it), slot 2 empty, slot 3 one
    non-zero voxel (1.0), slot 4 twelve equal non-zero voxels (0.5): statistics that are exact in every arithmetic"""
    acc = acc.clone()
    n = acc.shape[0]
    assert n >= 7
    counts = torch.full((n,), 1000, dtype=torch.int32)
    acc[1:5] = 0
    counts[1], counts[2] = KEEP, 0
    flat3, flat4 = acc[3].view(-1), acc[4].view(-1)
    flat3[flat3.numel() // 2] = 1 << 40
    idx = torch.arange(12) * max(1, flat4.numel() // 12 - 1) % flat4.numel()
    flat4[idx.unique()] = 1 << 39
    return acc, counts


# ------------------------------------------------------------------------------------------------------------------ the loaders' cuts
def loader_cut_fixed_duration(t, ts_end, T, delta_t_us):
    """The DSEC loader's fixed_duration branch (reference DSEC/dataset/sequence.py:224-231) restated on the whole time column t, the
    two searches of a window done the slow way, by looking at every event: the span delta_t_us before ts_end in T parts of
    delta_t_us / T (a true division), window i from the first event at or after its lower bound to the first event at or after its
    upper bound (EventSlicer.get_time_indices_offsets: both indices are t.size where no event is that late)
    -> [(first, behind)] * T"""
    ts_start = ts_end - delta_t_us
    part = delta_t_us / T
    out = []
    for i in range(T):
        lower = ts_start + i * part
        upper = ts_start + (i + 1) * part
        first = next((k for k in range(t.size) if t[k] >= lower), t.size)
        behind = next((k for k in range(t.size) if t[k] >= upper), t.size)
        out.append((first, behind))
    return out


def loader_cut_by_time(t_ns, T):
    """The DDD17 loader's cut by time (reference datasets/ddd17_events_loader.py:134-149) restated on one sample's times: the span
    between the first and the last event in T parts of int(span / T) time units, window i ends in front of the first event at or
    after t_ns[0] + (i + 1) parts (never behind the sample), and starts where window i - 1 ended -> [(first, behind)] * T"""
    part = int((t_ns[-1] - t_ns[0]) / T)
    loaded = t_ns.shape[0]
    out, behind = [], 0
    for i in range(T):
        first = behind
        behind = min(int(np.searchsorted(t_ns, t_ns[0] + (i + 1) * part)), loaded)
        out.append((first, behind))
    return out
