"""Shared by tests/test_hip_norm_edges.py (GPU tier), tests/test_host_norm_check.py (CPU tier) and the norm tests of
tests/test_hip_mixed_edges.py: seeded inputs, float64 references of the InstanceNorm / train-mode BatchNorm kernels of csrc/norm_c8.hip and
csrc/norm.hip, the bound of every output as a ratio (error / bound, <= 1 passes), the launch plans restated from the tuning values, and
a CPU fp32 restatement of the kernels' arithmetic with injectable defects.  A plain helper module: no fixtures, no collection hooks.

References are float64 restatements ON THE VALUES THE KERNEL READS (the stored bf16 / half / hi + lo values, the stored bf16 dy, the
stored y where the mask comes from y).  Everything downstream of the statistics is computed from the kernel's OWN saved (mean, rstd) /
(a, b) after those were checked against float64: the fp32 subtraction x - mean keeps the sign of the exact difference, so the
InstanceNorm mask (x - mean) rstd <= 0 is exact and no element is excluded; so is the mask read from the stored y.

Bounds.  u = 2^-24 (one fp32 rounding, relative to the magnitude it rounds); the fp64 partial sums count as exact.
  mean (C8)      2^-20 mean|x| + 1e-7 (the project's: ~16 fp32 steps on a running magnitude <= sum|x|);  rstd (C8): 1e-5 relative
  mean (fp32)    u |mean| + n 2^-53 mean|x|: n fp64 additions, one cast
  rstd (fp32)    2u + 1.5 n 2^-53 (var + mean^2) / (var + eps): E[x^2] - mean^2 in fp64 cancels against var + eps, then one cast
                 (and the fp32 cast of 1 / sqrt)
  y (IN)         t = (x - mean) rstd, y = relu?(t) + res:  out |ref| + 2^-22 (|t| + |res|)   [3 roundings: the difference, the product, the
                 residual add, each <= u (|t| + |res|)];  out = 2^-8 for a bf16 y (the project's), 2^-11 (+ 2^-25 absolute, the half
                 subnormal spacing) for a half y16, 0 for the fp32 kernels
  saved map      a = fl(rstd gamma): 2u |a|;  b = fl(beta - mean a), fused or not: 2u (|mean a| + |beta|)
  y (BN, C8)     y = relu?(x a + b + res) from the saved (a, b):  2^-8 |ref| + 2^-22 (|x a| + |b| + |res|)   [<= 3 roundings]
  y (BN, fp32)   ((x - mean) rstd gamma + beta) + res: 5 roundings <= 2^-21 (|t gamma| + |beta| + |res|)
  running_mean   (1 - mom) rm + mom mean from the kernel's mean: 4 roundings <= 2^-22 (|(1 - mom) rm| + |mom mean|)
  running_var    the same plus mom unb times twice the relative rstd bound (var + eps = rstd^-2), unb = var cnt / (cnt - 1), or var at cnt = 1
  dx (C8)        2^-8 |ref| + 2^-12 g rstd max|dy| (the project's, _bwd_check)
  dx (fp32)      g rstd (gr - m1 - xhat m2): 2 roundings in xhat, 1 in the product, 2 differences, 1 scale, the casts of m1 and m2:
                 <= 2^-21 g rstd (|gr| + |m1| + |xhat m2|), plus g rstd |xhat| 2u mean|gr xhat|: m2 = mean(gr xhat) is summed from terms
                 whose fp32 xhat carries 2 roundings, and where the mean cancels (|m2| << mean|gr xhat|) they do not cancel with it
  dbeta          C8: fp32 partials of 4 (3 additions, each <= u of the partial's sum |gr|), one cast, one accumulate add:
                 3u sum|gr| + 2u (|sum| + |prior| + |ref|);  fp32 kernels: fp64 sums of exact terms, the 2u term only
  dgamma         C8: xhat carries 2 roundings, the fma chain of 4 another 4: 6u sum|gr xhat| + 2u (...);  fp32 kernels: 2u sum|gr xhat| + 2u (...)
  dres           a masked copy of the stored dy: bit for bit
The affine-map mask x a + b <= 0 (BatchNorm backward with beta) is evaluated in fp32, possibly contracted to an fma: elements with
|x a + b| <= 2^-21 (|x a| + |b|) from the saved fp32 (a, b) form the ambiguous set A; they are left out of the per-element checks, the
bounds of the sums widen by sum_A |dy| (1, |xhat|), and A may hold at most AMBIGUOUS_CAP of the N hw elements of any channel of a row (a condition on the seeded
inputs that tests/test_host_norm_check.py proves for every row, not a measurement)."""
import functools

import torch
import torch.nn.functional as F

NAN = float('nan')
EPS = 1e-5
U24 = 2.0 ** -24
AMBIGUOUS_CAP = 1e-5
NORM_SPLIT_BY_PLANE = 1 << 30
MOM = 0.1


# ------------------------------------------------------------------------------------------------------------------ inputs
def _channels(N, C, Hh, W, g, sd=0.7):
    """x with channel means of 0, 6, 17 and 30 standard deviations (cycling), a near-constant channel (sigma^2 << eps) and an exactly
    constant one (the last two channels).  Every sample has its own means: sample n sits 1.25 n standard deviations nearer to zero
    than sample 0 (away from it on the zero-mean channels), so statistics read from the wrong sample are off by more than one sigma."""
    ratios = torch.tensor([0.0, 6.0, 17.0, 30.0]).repeat((C + 3) // 4)[:C]
    sign = torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    x = torch.randn(N, C, Hh, W, generator=g) * sd + (ratios * sd * sign).view(1, C, 1, 1)
    x = x - (1.25 * sd * torch.arange(N, dtype=torch.float32)).view(N, 1, 1, 1) * sign.view(1, C, 1, 1)
    x[:, C - 2] = 3.0 + 1e-4 * torch.randn(N, Hh, W, generator=g)
    x[:, C - 1] = 5.0
    return x


def _stat_ratios(stats, xv, dims, eps, exact_sums=False):
    """(max |dmean| / bound, max relative rstd error / bound) of the kernel's [rows, 2] stats against float64 over the stored values"""
    m = xv.mean(dims).reshape(-1)
    var = ((xv - xv.mean(dims, keepdim=True)) ** 2).mean(dims).reshape(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    am = xv.abs().mean(dims).reshape(-1)
    gm, gr = stats[:, 0].cpu().double(), stats[:, 1].cpu().double()
    n = xv.numel() // m.numel()
    if exact_sums:
        mb = U24 * m.abs() + n * 2.0 ** -53 * am + 1e-300
        rb = 2 * U24 + 1.5 * n * 2.0 ** -53 * (var + m * m) / (var + eps)
    else:
        mb = 2 ** -20 * am + 1e-7
        rb = torch.full_like(m, 1e-5)
    return ((gm - m).abs() / mb).max().item(), (((gr - rstd) / rstd).abs() / rb).max().item(), rb


def _check_stats(stats, xv, dims, eps, what):
    """mean and rstd of the kernel against fp64 over the stored values.  rstd: 1e-5 relative at every mean ratio (the bound
    test_instance_norm_c8 applies to benign data).  mean: the fp32 value of a sum taken in fp32 partials, |dm| <= 2^-20 mean|x| + 1e-7
    (at most ~16 rounding steps of 2^-24 on a running magnitude <= the sum of |x|)."""
    m = xv.mean(dims).reshape(-1)
    var = ((xv - xv.mean(dims, keepdim=True)) ** 2).mean(dims).reshape(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    am = xv.abs().mean(dims).reshape(-1)
    gm, gr = stats[:, 0].cpu().double(), stats[:, 1].cpu().double()
    dm = (gm - m).abs()
    assert (dm <= 2 ** -20 * am + 1e-7).all(), (what, 'mean', dm.max().item(), int((dm > 2 ** -20 * am + 1e-7).sum()))
    rel = ((gr - rstd) / rstd).abs()
    assert rel.max().item() < 1e-5, (what, 'rstd', rel.max().item(), int(rel.argmax()))
    return rel.max().item()


def _bwd_ratio(got, xr, dyq, stats, dims, gamma=None, off=None, skip=None, fp32_kernel=False):
    """max (|dx - ref| / bound) with dx = g rstd (gr - mean(gr) - xhat mean(gr xhat)) in fp64 from the kernel's (mean, rstd) over the
    stored x and dy, gr = dy outside the mask `off`; `skip`: elements left out of the comparison (the ambiguous set of an affine mask)"""
    N, C = xr.shape[0], xr.shape[1]
    shp = (N, C, 1, 1) if dims == (2, 3) else (1, C, 1, 1)
    m = stats[:, 0].cpu().double().view(shp)
    r = stats[:, 1].cpu().double().view(shp)
    xh = (xr - m) * r
    grd = dyq if off is None else torch.where(off, torch.zeros_like(dyq), dyq)
    s1 = grd.mean(dims, keepdim=True)
    s2 = (grd * xh).mean(dims, keepdim=True)
    gr = r * (gamma.double().view(1, -1, 1, 1) if gamma is not None else 1.0)
    ref = gr * (grd - s1 - xh * s2)
    if fp32_kernel:
        sa = (grd * xh).abs().mean(dims, keepdim=True)  # (m2 sums terms gr xhat whose xhat carries 2 roundings: it cancels, they do not)
        tol = gr.abs() * (2 ** -21 * (grd.abs() + s1.abs() + (xh * s2).abs()) + 2 * U24 * xh.abs() * sa) + 1e-300
    else:
        tol = 2 ** -8 * ref.abs() + 2 ** -12 * gr.abs() * dyq.abs().amax(dims, keepdim=True)
    err = (got - ref).abs()
    if skip is not None:
        err = torch.where(skip, torch.zeros_like(err), err)
    return err, tol


def _bwd_check(got, xr, dyq, stats, dims, what, gamma=None):
    """dx = g rstd (dy - mean(dy) - xhat mean(dy xhat)) in fp64 from the kernel's (mean, rstd) over the stored x and dy; bound: the bf16
    rounding of dx (2^-8 |dx|) plus 2^-12 rstd |dy|max per element for the fp32 xhat the kernel forms"""
    err, tol = _bwd_ratio(got, xr, dyq, stats, dims, gamma)
    assert not torch.isnan(got).any()
    assert (err - tol).max().item() <= 0, (what, err.max().item())


def bfr(x):
    return x.float().bfloat16().double()


def hfr(x):
    return x.float().half().double()


class Row:
    """One row of NORM_EDGE_CASES (tests/test_hip_norm_edges.py): id, family, N, C, hw, tuning values, label.
    family: 'in8' (ess_instnorm_forward_c8 / backward_c8), 'mix' (ess_instnorm_forward_c8_mixed, backward with x_f16 = 2 for a pair),
    'bn8' (ess_batchnorm_train_*_c8), 'in32' / 'bn32' (csrc/norm.hip);  label: 'forward route/backward route' as plan() restates them."""

    def __init__(self, row):
        self.id, self.family, self.N, self.C, self.hw, self.tune, self.label = row
        self.tune = dict(self.tune)
        self.CB = (self.C + 7) // 8
        self.misaligned = 'misaligned' in self.id
        self.partial = self.family in ('in8', 'mix', 'bn8') and self.C % 8 != 0

    @property
    def seed(self):
        return sum(map(ord, self.id))


def split_for8(groups, hw, target=1024, minv=1024):
    """split_for8() of csrc/norm_c8.hip: slices per group of the split statistics pass"""
    s = -(-target // groups)
    s = min(s, -(-hw // minv), 64)
    return max(s, 1)


def split_for(groups, hw):
    """split_for() of csrc/norm.hip"""
    return max(min(-(-2048 // groups), -(-hw // 2048)), 1)


def plan(r):
    """'forward route/backward route' of a row: which kernels the dispatch of csrc/norm_c8.hip / csrc/norm.hip takes and, on the split
    path, into how many slices, from the tuning values the row sets (in_small_threads default 512, norm_split_wgs default 1024)"""
    target = r.tune.get('norm_split_wgs', 1024)
    if target == 'groups':
        target = r.N * r.CB
    if r.family == 'bn8':
        s = split_for8(r.CB, r.hw, target)
        return f'split{s}/split{s}'
    if r.family in ('in8', 'mix'):
        groups = r.N * r.CB
        s = f'split{split_for8(groups, r.hw, target)}'
        if r.hw <= 5120:
            th = r.tune.get('in_small_threads', 512)
            return f'fused512/fused{th}' if r.family == 'mix' else f'fused{th}/fused{th}'
        if r.family == 'in8' and r.hw <= 1024 * 19 and groups >= 256:
            return f'fused1024x19/{s}'
        return f'{s}/{s}'
    if r.family == 'bn32':
        s = split_for(r.C, r.hw)
        return f'split{s}/split{s}'
    planes = r.N * r.C
    if planes >= 1024 or r.hw < 16384:
        aligned = r.hw % 4 == 0 and not r.misaligned
        f = 'registers' if aligned and r.hw <= 6144 else 'strided16' if aligned else 'scalar'
        return f'fused_{f}/fused_{"registers" if f == "registers" else "scalar"}'
    s = split_for(planes, r.hw)
    v = '16' if r.hw % 4 == 0 and not r.misaligned else 'scalar'
    return f'split{s}_{v}/split{s}_{v}'


def nslices(route):
    return int(route.split('_')[0][5:]) if route.startswith('split') else 0


@functools.lru_cache(maxsize=1)
def row_inputs(row_key):
    """Seeded fp32 CPU inputs of a row, shared by its tests: do not write into them.  x [N, C, hw] (see _channels), dy, res ~ N(0, 1),
    gamma in [0.5, 1.5), beta ~ N(0, 1), non-trivial running statistics and prior dgamma / dbeta."""
    r = Row(row_key)
    g = torch.Generator().manual_seed(r.seed)
    d = {'x': _channels(r.N, r.C, r.hw, 1, g).view(r.N, r.C, r.hw),
         'dy': torch.randn(r.N, r.C, r.hw, generator=g),
         'res': torch.randn(r.N, r.C, r.hw, generator=g),
         'gamma': torch.rand(r.C, generator=g) + 0.5,
         'beta': torch.randn(r.C, generator=g),
         'rm0': torch.randn(r.C, generator=g),
         'rv0': torch.rand(r.C, generator=g) + 0.5,
         'dgamma0': torch.randn(r.C, generator=g) * 3 + 7,
         'dbeta0': torch.randn(r.C, generator=g) * 3 - 5}
    return d


def stored(x, fmt):
    """float64 values a kernel reads of fp32 `x` stored as fmt 0 bf16, 1 half, 2 a [hi | lo] half pair, 32 fp32"""
    if fmt == 32:
        return x.double()
    if fmt == 0:
        return bfr(x)
    hi = x.float().half()
    if fmt == 1:
        return hi.double()
    lo = (x.float() - hi.float()).half()
    return hi.double() + lo.double()


# ------------------------------------------------------------------------------------------------------------------ ratios
def _mx(t):
    return t.max().item() if t.numel() else 0.0


def in_forward_ratios(xv, res, relu, stats, ys, fp32_kernel=False, eps=EPS):
    """InstanceNorm forward.  xv, res: float64 [N, C, hw] stored values; stats: the kernel's [N, C, 2]; ys: {'y': bf16 values, 'y16': half
    values, 'y32': fp32 values} as float64 [N, C, hw].  relu: 0, 1 (before the residual) or 2 (after it, fp32 kernels).  -> {name: ratio}"""
    N, C, hw = xv.shape
    x4 = xv.view(N, C, hw, 1)
    rm, rr, _ = _stat_ratios(stats.reshape(N * C, 2), x4, (2, 3), eps, fp32_kernel)
    m = stats[..., 0].double().view(N, C, 1)
    r = stats[..., 1].double().view(N, C, 1)
    t = (xv - m) * r
    if relu == 1:
        t = t.clamp_min(0)
    ref = t if res is None else t + res
    if relu == 2:
        ref = ref.clamp_min(0)
    slack = 2 ** -22 * (t.abs() + (res.abs() if res is not None else 0)) + 1e-300
    out = {'mean': rm, 'rstd': rr}
    for k, got in ys.items():
        tol = {'y': 2 ** -8, 'y16': 2 ** -11, 'y32': 0.0}[k] * ref.abs() + slack + (2 ** -25 if k == 'y16' else 0)
        out[k] = _mx((got - ref).abs() / tol)
    return out


def in_backward_ratios(xr, dy, relu, stats, dx, fp32_kernel=False):
    """InstanceNorm backward from the kernel's statistics.  xr: what the backward reads of x (the hi parts of a pair)."""
    N, C, hw = xr.shape
    m = stats[..., 0].double().view(N, C, 1)
    off = (xr - m) <= 0 if relu else None
    v4 = lambda t: None if t is None else t.view(N, C, hw, 1)
    err, tol = _bwd_ratio(v4(dx), v4(xr), v4(dy), stats.reshape(N * C, 2), (2, 3), off=v4(off), fp32_kernel=fp32_kernel)
    return {'dx': _mx(err / tol)}


def bn_forward_ratios(xv, res, relu, gamma, beta, st, y, rm0, rv0, rm, rv, fp32_kernel=False, eps=EPS, mom=MOM):
    """BatchNorm(train) forward.  st: the kernel's [2, C, 2] ((mean, rstd) pairs, then the saved map; [C, 2] for the fp32 kernels);
    y float64 [N, C, hw]; rm0 / rv0 the running statistics before the call, rm / rv after it (None: not passed)."""
    N, C, hw = xv.shape
    x4 = xv.view(N, C, hw, 1)
    stats = (st if fp32_kernel else st[0]).double()
    rmn, rrs, rb = _stat_ratios(stats, x4, (0, 2, 3), eps, fp32_kernel)
    out = {'mean': rmn, 'rstd': rrs}
    m, r = stats[:, 0].view(1, C, 1), stats[:, 1].view(1, C, 1)
    ga, be = gamma.double().view(1, C, 1), beta.double().view(1, C, 1)
    rs = res.abs() if res is not None else 0
    if fp32_kernel:
        t = (xv - m) * r * ga
        pre = t + be + (res if res is not None else 0)
        tol = 2 ** -21 * (t.abs() + be.abs() + rs) + 1e-300
        key = 'y32'
    else:
        a, b = st[1, :, 0].double().view(1, C, 1), st[1, :, 1].double().view(1, C, 1)
        out['map_a'] = _mx((a - r * ga).abs() / (2 * U24 * (r * ga).abs()))
        out['map_b'] = _mx((b - (be - m * a)).abs() / (2 * U24 * ((m * a).abs() + be.abs()) + 1e-300))
        pre = xv * a + b + (res if res is not None else 0)
        tol = 2 ** -22 * ((xv * a).abs() + b.abs() + rs) + 1e-300
        key = 'y'
    ref = pre.clamp_min(0) if relu else pre
    if not fp32_kernel:
        tol = tol + 2 ** -8 * ref.abs()
    out[key] = _mx((y - ref).abs() / tol)
    if rm is not None:
        mom32 = float(torch.tensor(mom, dtype=torch.float32))
        keep = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(mom, dtype=torch.float32))
        cnt = N * hw
        var = ((x4 - x4.mean((0, 2, 3), keepdim=True)) ** 2).mean((0, 2, 3))
        unb = var * cnt / (cnt - 1) if cnt > 1 else var
        rm_ref = keep * rm0.double() + mom32 * stats[:, 0]
        out['running_mean'] = _mx((rm.double() - rm_ref).abs() / (2 ** -22 * ((keep * rm0.double()).abs() + (mom32 * stats[:, 0]).abs()) + 1e-300))
        rv_ref = keep * rv0.double() + mom32 * unb
        f = cnt / (cnt - 1) if cnt > 1 else 1.0
        tolv = mom32 * 2.1 * rb * (var + eps) * f + 2 ** -22 * ((keep * rv0.double()).abs() + mom32 * unb)
        out['running_var'] = _mx((rv.double() - rv_ref).abs() / tolv)
    return out


def affine_mask(xv, st):
    """(off, A) of the affine-map mask from the kernel's saved fp32 (a, b): off = x a + b <= 0, A the ambiguous set"""
    C = xv.shape[1]
    a, b = st[1, :, 0].double().view(1, C, 1), st[1, :, 1].double().view(1, C, 1)
    v = xv * a + b
    return v <= 0, v.abs() <= 2 ** -21 * ((xv * a).abs() + b.abs())


def bn_backward_ratios(xv, dy, st, gamma, off, amb, dx, dgamma, dbeta, dgamma0, dbeta0, accumulate, fp32_kernel=False):
    """BatchNorm(train) backward.  off: the mask (None: no ReLU), already exact (stored y <= 0) or the affine one with its ambiguous set
    `amb`; dgamma0 / dbeta0: what dgamma / dbeta held before the call (counted when `accumulate`).  dx may be None (need_dx=False)."""
    N, C, hw = xv.shape
    stats = (st if fp32_kernel else st[0]).double()
    m, r = stats[:, 0].view(1, C, 1), stats[:, 1].view(1, C, 1)
    xh = (xv - m) * r
    gr = dy if off is None else torch.where(off, torch.zeros_like(dy), dy)
    za = torch.zeros(C, dtype=torch.float64)
    wa0 = (dy.abs() * amb).sum((0, 2)) if amb is not None else za
    wa1 = (dy.abs() * xh.abs() * amb).sum((0, 2)) if amb is not None else za
    t0, t1 = gr.sum((0, 2)), (gr * xh).sum((0, 2))
    p0 = dbeta0.double() if accumulate else za
    p1 = dgamma0.double() if accumulate else za
    kb, kg = (0, 2) if fp32_kernel else (3, 6)
    tb = kb * U24 * gr.abs().sum((0, 2)) + 2 * U24 * (t0.abs() + p0.abs() + (t0 + p0).abs()) + wa0 + 1e-300
    tg = kg * U24 * (gr * xh).abs().sum((0, 2)) + 2 * U24 * (t1.abs() + p1.abs() + (t1 + p1).abs()) + wa1 + 1e-300
    out = {'dbeta': _mx((dbeta.double() - (t0 + p0)).abs() / tb), 'dgamma': _mx((dgamma.double() - (t1 + p1)).abs() / tg)}
    if dx is not None:
        v4 = lambda t: None if t is None else t.view(N, C, hw, 1)
        # the scale of dx is the saved a = fl(gamma rstd) (C8) or gamma rstd (fp32): one rounding apart, inside either bound
        err, tol = _bwd_ratio(v4(dx), v4(xv), v4(dy), stats, (0, 2, 3), gamma=gamma, off=v4(off), skip=v4(amb), fp32_kernel=fp32_kernel)
        if amb is not None:  # the sums inside dx move with the ambiguous elements as well
            cnt = N * hw
            g4 = (r * gamma.double().view(1, C, 1)).abs().view(1, C, 1, 1)
            tol = tol + g4 * (wa0.view(1, C, 1, 1) + v4(xh).abs() * wa1.view(1, C, 1, 1)) / cnt
        out['dx'] = _mx(err / tol)
    return out


def assert_ratios(ratios, what):
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f'{what}: error / bound = {bad} (all: {ratios})'


def worst(ratios):
    return max(ratios.values())


# ------------------------------------------------------------------------------------------------------------------ restatement
# A CPU fp32 restatement of the kernels' arithmetic: fp32 partials of 4 vectors (256 lanes apart), fp64 running sums, slices in order;
# the fused kernels' two-pass fp32 mean / centred variance.  `defect` injects ONE named mistake:
#   'drop_last'  the last pixel of slice 0 left out of the sums     'drop_max'   the pixel of largest |x| of channel 0 left out
#   'slice_twice' the last slice's partial counted twice            'stats_sample0' sample 0's statistics used for sample 1 (backward)
#   'mask_lt'    < 0 instead of <= 0 in the backward mask           'res_before_relu' the InstanceNorm residual added before the ReLU
#   'no_accumulate' accumulate ignored                              'no_unbiased' running_var from the biased variance
DEFECTS = ('drop_last', 'drop_max', 'slice_twice', 'stats_sample0', 'mask_lt', 'res_before_relu', 'no_accumulate', 'no_unbiased')


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _slice_sums(v, a, b, nsl, exact=False, defect=None, quantum=1):
    """(sum v, sum a b) over the last axis as the split kernels take them -> fp64 [...].  nsl = 0: one fused workgroup (exact: fp64
    per element; else plain fp32 sums)."""
    hw = v.shape[-1]
    if defect in ('drop_last', 'drop_max'):
        ln = hw if nsl <= 1 else ((-(-hw // nsl) + quantum - 1) // quantum) * quantum
        p = min(ln, hw) - 1
        if defect == 'drop_max':
            flat = v.reshape(-1, hw)[0]
            p = int(flat.abs().argmax())
        keep = torch.ones(v.shape[0], 1, hw, dtype=v.dtype)  # (one pixel vector of sample 0: every channel of it)
        keep[0, 0, p] = 0
        v, a = v * keep, a * keep
    if nsl == 0 and not exact:
        return v.sum(-1, dtype=torch.float32).double(), (a * b).sum(-1, dtype=torch.float32).double()
    if exact:
        nsl = max(nsl, 1)
    ln = ((-(-hw // nsl) + quantum - 1) // quantum) * quantum
    t0 = torch.zeros(v.shape[:-1], dtype=torch.float64)
    t1 = torch.zeros(v.shape[:-1], dtype=torch.float64)
    for sl in range(nsl):
        i0, i1 = sl * ln, min(hw, sl * ln + ln)
        if i1 <= i0:
            continue
        if exact:
            p0 = v[..., i0:i1].double().sum(-1)
            p1 = (a[..., i0:i1].double() * b[..., i0:i1].double()).sum(-1)
        else:
            pad = -(i1 - i0) % 1024
            cut = lambda t: F.pad(t[..., i0:i1], (0, pad)).reshape(*t.shape[:-1], -1, 4, 256)
            vv, aa, bb = cut(v), cut(a), cut(b)
            q0 = torch.zeros_like(vv[..., 0, :])
            q1 = torch.zeros_like(q0)
            for u in range(4):
                q0 = q0 + vv[..., u, :]
                q1 = _fma(aa[..., u, :], bb[..., u, :], q1)
            p0, p1 = q0.double().sum((-1, -2)), q1.double().sum((-1, -2))
        w = 2 if (defect == 'slice_twice' and sl == nsl - 1) else 1
        t0, t1 = t0 + w * p0, t1 + w * p1
    return t0, t1


def _stats_of(x, nsl, over_n, exact, hilo, eps, defect, quantum=1):
    """(mean, rstd, var fp64) fp32 as the forward computes them; x fp32 [N, C, hw]; over_n: BatchNorm"""
    N, C, hw = x.shape
    cnt = N * hw if over_n else hw
    if nsl == 0 and not exact:  # fused C8: two-pass fp32
        s, _ = _slice_sums(x, x, x, 0, defect=defect)
        mean = (s.float() / hw)
        d = x - mean.unsqueeze(-1)
        q, _ = _slice_sums(d * d, d, d, 0, defect=None)
        rstd = 1.0 / torch.sqrt(q.float() / hw + torch.tensor(eps, dtype=torch.float32))
        return mean, rstd, None
    t0, t1 = _slice_sums(x, x, x, nsl, exact=exact or hilo, defect=defect, quantum=quantum)
    if over_n:
        t0, t1 = t0.sum(0), t1.sum(0)
    m = t0 / cnt
    var = (t1 / cnt - m * m).clamp_min(0)
    return m.float(), (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))).float(), var


def restate_in_forward(x, res, relu, routes, out_fmt='y', fp32_kernel=False, hilo=False, eps=EPS, defect=None):
    """-> (stats [N, C, 2] fp32, y float64 of the stored output).  x: fp32 (hi + lo of a pair), res fp32 or None."""
    nsl = nslices(routes)
    mean, rstd, _ = _stats_of(x, nsl, False, fp32_kernel, hilo, eps, defect, quantum=4 if fp32_kernel else 1)
    t = (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    if defect == 'res_before_relu' and res is not None:
        t = t + res
        if relu:
            t = t.clamp_min(0)
    else:
        if relu == 1:
            t = t.clamp_min(0)
        if res is not None:
            t = t + res
        if relu == 2:
            t = t.clamp_min(0)
    y = {'y': bfr, 'y16': hfr, 'y32': lambda z: z.double()}[out_fmt](t)
    return torch.stack([mean, rstd], -1), y


def _bwd_sums(x, dy, mean, rstd, off, nsl, exact, defect, quantum=1):
    xh = (x - mean) * rstd
    gr = torch.where(off, torch.zeros_like(dy), dy) if off is not None else dy
    t0, t1 = _slice_sums(gr, gr, xh, nsl, exact=exact, defect=defect, quantum=quantum)
    return xh, gr, t0, t1


def restate_in_backward(x, dy, stats, relu, routes, fp32_kernel=False, defect=None):
    """-> dx float64 of the stored output.  x: fp32 values the backward reads; dy fp32 (bf16 values for the C8 kernels)"""
    N, C, hw = x.shape
    st = stats.clone()
    if defect == 'stats_sample0':
        st[1:] = st[:1]
    mean, rstd = st[..., 0:1], st[..., 1:2]
    xh = (x - mean) * rstd
    off = None
    if relu:
        off = xh < 0 if defect == 'mask_lt' else xh <= 0
    nsl = nslices(routes)
    xh, gr, t0, t1 = _bwd_sums(x, dy, mean, rstd, off, nsl, fp32_kernel, defect, quantum=4 if fp32_kernel else 1)
    if nsl == 0 and not fp32_kernel:
        m1, m2 = (t0.float() / hw).unsqueeze(-1), (t1.float() / hw).unsqueeze(-1)
    else:
        m1, m2 = (t0 / hw).float().unsqueeze(-1), (t1 / hw).float().unsqueeze(-1)
    dx = rstd * (gr - m1 - xh * m2)
    return dx.double() if fp32_kernel else bfr(dx)


def restate_bn_forward(x, res, relu, gamma, beta, rm0, rv0, routes, fp32_kernel=False, eps=EPS, mom=MOM, defect=None):
    """-> (st [2, C, 2] ([C, 2] for the fp32 kernels), y float64 stored, running_mean, running_var)"""
    N, C, hw = x.shape
    cnt = N * hw
    mean, rstd, var = _stats_of(x, nslices(routes), True, fp32_kernel, False, eps, defect, quantum=4 if fp32_kernel else 1)
    m_, r_ = mean.view(1, C, 1), rstd.view(1, C, 1)
    if fp32_kernel:
        t = (x - m_) * r_ * gamma.view(1, C, 1) + beta.view(1, C, 1)
        st = torch.stack([mean, rstd], -1)
    else:
        a = rstd * gamma
        b = beta - mean * a
        t = x * a.view(1, C, 1) + b.view(1, C, 1)
        st = torch.stack([torch.stack([mean, rstd], -1), torch.stack([a, b], -1)])
    if res is not None:
        t = t + res
    if relu:
        t = t.clamp_min(0)
    momf = torch.tensor(mom, dtype=torch.float32)
    unb = var * cnt / (cnt - 1) if (cnt > 1 and defect != 'no_unbiased') else var
    rm = (1 - momf) * rm0 + momf * mean
    rv = (1 - momf) * rv0 + momf * unb.float()
    return st, (t.double() if fp32_kernel else bfr(t)), rm, rv


def restate_bn_backward(x, ystored, dy, st, gamma, form, routes, dgamma0, dbeta0, accumulate, need_dx=True, fp32_kernel=False, defect=None):
    """form: 'none', 'y' (mask from the stored y) or 'map' (from the saved affine map).  -> (dx float64 or None, dres float64, dgamma, dbeta)"""
    N, C, hw = x.shape
    cnt = N * hw
    stats = st if fp32_kernel else st[0]
    mean, rstd = stats[:, 0].view(1, C, 1), stats[:, 1].view(1, C, 1)
    lt = defect == 'mask_lt'
    off = None
    if form == 'y':
        off = ystored.float() < 0 if lt else ystored.float() <= 0
    elif form == 'map':
        v = x * st[1, :, 0].view(1, C, 1) + st[1, :, 1].view(1, C, 1)
        off = v < 0 if lt else v <= 0
    xh, gr, t0, t1 = _bwd_sums(x, dy, mean, rstd, off, nslices(routes), fp32_kernel, defect, quantum=4 if fp32_kernel else 1)
    t0, t1 = t0.sum(0), t1.sum(0)
    acc = accumulate and defect != 'no_accumulate'
    dbeta = dbeta0 + t0.float() if acc else t0.float()
    dgamma = dgamma0 + t1.float() if acc else t1.float()
    dx = None
    if need_dx:
        m1, m2 = (t0 / cnt).float().view(1, C, 1), (t1 / cnt).float().view(1, C, 1)
        scale = (gamma * stats[:, 1]) if fp32_kernel else st[1, :, 0]
        dx = scale.view(1, C, 1) * (gr - m1 - xh * m2)
        dx = dx.double() if fp32_kernel else bfr(dx)
    return dx, gr.double(), dgamma, dbeta
