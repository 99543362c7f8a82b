"""GPU tier: every route of the norm kernels (csrc/norm_c8.hip: fused 256 / 512 / 1024-thread InstanceNorm, the 1024 x 19 fused forward, the
split reduce / apply pairs of InstanceNorm and train-mode BatchNorm, the mixed configuration's forward; csrc/norm.hip: the fp32 fused
and split kernels) against float64 torch-CPU restatements of the same operation on the stored values (tests/norm_ref.py), with ReLU
masks, residuals, dres, accumulate and need_dx=False, on inputs whose channel means differ between the samples of a batch, at the
smallest shapes at which each plan edge exists.

Every launch under test gets a workspace the test owns, filled with 0xFF bytes, and outputs it does not accumulate onto filled with
NaN: the library is called through hip.lib() with the test's tensors, so nothing can read back an earlier result.  No NaN may remain in
a real channel.  y, y16 and dx are written under `cb*8 + j < C ? ... : 0`: their padding lanes must be zero.  Rows with a partial
channel block run a second time with finite garbage in the padding lanes of x, dy and the residual: every real channel and every
statistic must stay bit for bit.  bn_bwd_apply_c8_kernel writes dres WITHOUT that select: what it guarantees, and what is asserted, is
that a padding lane of dres is the padding lane of dy where the mask lets it through and zero where the mask applies (with a y the
forward wrote, whose padding lanes are zero, that is zero under ReLU).
tests/test_host_norm_check.py proves on the CPU that each bound notices the defects it is there for, and checks the row labels."""
import ctypes

import pytest
import torch

import norm_ref as R
from norm_ref import NAN, NORM_SPLIT_BY_PLANE as BY_PLANE, Row, row_inputs

pytestmark = pytest.mark.gpu

T256, T512, T1024 = ((('in_small_threads', t),) for t in (256, 512, 1024))
# id, family, N, C, hw, tuning values, 'forward route/backward route' (norm_ref.plan restates the dispatch; splitN: N slices per group)
NORM_EDGE_CASES = [
    # ---- ess_instnorm_forward_c8 / ess_instnorm_backward_c8: fused single-plane kernels at every in_small_threads value
    ('in8_t256_hw1', 'in8', 2, 12, 1, T256, 'fused256/fused256'),
    ('in8_t256_hw63', 'in8', 2, 16, 63, T256, 'fused256/fused256'),
    ('in8_t256_hw5120', 'in8', 2, 12, 5120, T256, 'fused256/fused256'),
    ('in8_t512_hw1', 'in8', 2, 16, 1, T512, 'fused512/fused512'),
    ('in8_t512_hw63', 'in8', 2, 12, 63, T512, 'fused512/fused512'),
    ('in8_t512_hw5120', 'in8', 2, 16, 5120, T512, 'fused512/fused512'),
    ('in8_t1024_hw1', 'in8', 2, 12, 1, T1024, 'fused1024/fused1024'),
    ('in8_t1024_hw63', 'in8', 2, 16, 63, T1024, 'fused1024/fused1024'),
    ('in8_t1024_hw5120', 'in8', 2, 12, 5120, T1024, 'fused1024/fused1024'),
    # ---- split path: default target; one slice (several iterations of the unrolled loop and a ragged tail); 18 uneven slices (more than
    # the 16 lane groups of group_total8); the 64-slice cap
    ('in8_split_default', 'in8', 2, 16, 5121, (), 'split6/split6'),
    ('in8_split_one_slice', 'in8', 2, 12, 5121, (('norm_split_wgs', 'groups'),), 'split1/split1'),
    ('in8_split_18_slices', 'in8', 2, 16, 17 * 1024 + 5, (('norm_split_wgs', BY_PLANE),), 'split18/split18'),
    ('in8_split_cap_64', 'in8', 2, 12, 240 * 320, (('norm_split_wgs', BY_PLANE),), 'split64/split64'),
    # ---- the fused 1024 x 19 forward (groups >= 256): a short plane, the last plane it takes, the first it hands to the split path
    ('in8_f1024_groups256', 'in8', 2, 1020, 5121, (), 'fused1024x19/split4'),
    ('in8_f1024_last_plane', 'in8', 2, 1024, 19456, (), 'fused1024x19/split4'),
    ('in8_f1024_one_past', 'in8', 2, 1020, 19457, (), 'split4/split4'),
    # ---- ess_instnorm_forward_c8_mixed (backward: ess_instnorm_backward_c8 with x_f16 = x_fmt)
    ('mix_hw5120', 'mix', 2, 12, 5120, (), 'fused512/fused512'),
    ('mix_hw5121_split', 'mix', 2, 16, 5121, (), 'split6/split6'),
    ('mix_hw63_below_threads', 'mix', 2, 12, 63, (), 'fused512/fused512'),
    # ---- ess_batchnorm_train_forward_c8 / backward_c8 (always the split pair; groups = channel blocks)
    ('bn8_hw1', 'bn8', 2, 12, 1, (), 'split1/split1'),
    ('bn8_hw15', 'bn8', 2, 16, 15, (), 'split1/split1'),
    ('bn8_hw1200', 'bn8', 2, 12, 1200, (), 'split2/split2'),
    ('bn8_hw5121', 'bn8', 2, 20, 5121, (), 'split6/split6'),
    ('bn8_n1_hw1_cnt1', 'bn8', 1, 12, 1, (), 'split1/split1'),
    # ---- csrc/norm.hip, fp32 NCHW
    ('in32_hw4', 'in32', 2, 3, 4, (), 'fused_registers/fused_registers'),
    ('in32_hw6144_last_in_registers', 'in32', 2, 3, 6144, (), 'fused_registers/fused_registers'),
    ('in32_hw6148_strided16', 'in32', 2, 3, 6148, (), 'fused_strided16/fused_scalar'),
    ('in32_hw6145_scalar', 'in32', 2, 3, 6145, (), 'fused_scalar/fused_scalar'),
    ('in32_hw6144_misaligned', 'in32', 2, 3, 6144, (), 'fused_scalar/fused_scalar'),
    ('in32_hw16384_3planes', 'in32', 1, 3, 16384, (), 'split8_16/split8_16'),
    ('in32_hw16385_short_last_slice', 'in32', 1, 3, 16385, (), 'split9_scalar/split9_scalar'),
    ('in32_planes1024_hw16384', 'in32', 2, 512, 16384, (), 'fused_strided16/fused_scalar'),
    ('bn32_hw15', 'bn32', 2, 4, 15, (), 'split1/split1'),
    ('bn32_hw16384', 'bn32', 2, 4, 16384, (), 'split8/split8'),
    ('bn32_hw4096_misaligned', 'bn32', 2, 4, 4096, (), 'split2/split2'),
]
ROWS = {fam: [c for c in NORM_EDGE_CASES if c[1] == fam] for fam in ('in8', 'mix', 'bn8', 'in32', 'bn32')}
ids = lambda rows: [c[0] for c in rows]
WORST = {}  # family -> largest error / bound seen (printed by each test: run with -s to collect MEASUREMENTS.md's table)


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


class Tuned:
    """the row's tuning values for the duration of a with block"""

    def __init__(self, H, r):
        self.H, self.r = H, r

    def __enter__(self):
        self.prev = {k: self.H.tuning_get(k) for k in self.r.tune}
        for k, v in self.r.tune.items():
            self.H.tuning_set(k, self.r.N * self.r.CB if v == 'groups' else v)

    def __exit__(self, *a):
        try:
            torch.cuda.synchronize()
        finally:
            for k, v in self.prev.items():
                self.H.tuning_set(k, v)


def P(t):
    assert t is None or (t.is_cuda and t.is_contiguous())
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def call(H, name, *args):
    rc = getattr(H.lib(), name)(*args, H.stream())
    assert rc == 0, (name, rc, H.lib().ess_last_error().decode())


def poisoned_ws(H, groups, c8=True):
    """a workspace the test owns, every byte 0xFF (every double in it a NaN) -> its (pointer, size) arguments"""
    n = H.lib().ess_norm_workspace_c8(groups) if c8 else H.lib().ess_norm_workspace(groups)
    ws = torch.full((max(int(n), 16),), 0xFF, dtype=torch.uint8, device='cuda')
    return ws, (P(ws), ctypes.c_size_t(ws.numel()))


def block(t, CB):
    """16-bit [N, C, hw] -> the C8 layout [N][CB][hw][8], padding lanes zero"""
    N, C, hw = t.shape
    p = torch.zeros(N, CB * 8, hw, dtype=t.dtype, device=t.device)
    p[:, :C] = t
    return p.view(N, CB, 8, hw).permute(0, 1, 3, 2).contiguous()


def unblock(b, c0, c1):
    """float64 CPU [N, c1 - c0, hw] of channels [c0, c1) (c0 % 8 == 0) of a [N][CB][hw][8] tensor"""
    N, _, hw, _ = b.shape
    s = b[:, c0 // 8:(c1 + 7) // 8]
    return s.permute(0, 1, 3, 2).reshape(N, -1, hw)[:, :c1 - c0].double().cpu()


def padding(b, C):
    return b[:, -1, :, C % 8:] if C % 8 else b[:, :0]


def garbage(b, C, seed):
    """the same tensor with finite garbage in its padding lanes"""
    b = b.clone()
    if C % 8:
        g = torch.Generator().manual_seed(seed)
        pad = b[:, -1, :, C % 8:]
        pad.copy_((torch.randn(pad.shape, generator=g) * 7 + 3).to(b.dtype))
    return b


def store(x, fmt, CB):
    """device C8 tensor of fp32 CPU x [N, C, hw] in format 0 bf16, 1 half, 2 [hi | lo] half pair ([N][2 CB][hw][8])"""
    x = x.cuda()
    if fmt == 0:
        return block(x.bfloat16(), CB)
    hi = x.half()
    if fmt == 1:
        return block(hi, CB)
    return torch.cat([block(hi, CB), block((x - hi.float()).half(), CB)], 1)


def chunks(r):
    step = max(8, (1 << 22) // (r.N * r.hw) // 8 * 8)
    return [(c0, min(r.C, c0 + step)) for c0 in range(0, r.C, step)]


def merge(total, part):
    for k, v in part.items():
        total[k] = max(total.get(k, 0.0), v) if v == v else v
    return total


def report(r, what, ratios):
    R.assert_ratios(ratios, (r.id, r.label) + tuple(what))
    w = R.worst(ratios)
    WORST[r.family] = max(WORST.get(r.family, 0.0), w)
    print(f'{r.id} [{r.label}] {what}: worst error / bound {w:.3f} {({k: round(v, 3) for k, v in ratios.items()})}; family so far {WORST[r.family]:.3f}')


def no_nan_real(t, C, what):
    N, CB, hw, _ = t.shape
    real = t.permute(0, 1, 3, 2).reshape(N, CB * 8, hw)[:, :C]
    assert not torch.isnan(real.float()).any(), (what, 'NaN in a real channel')


def clean(t, C, what):
    no_nan_real(t, C, what)
    if C % 8:
        assert (padding(t, C).float() == 0).all(), (what, 'padding lanes not zero')


def same_real(a, b, C, what):
    N, CB, hw, _ = a.shape
    ra = a.permute(0, 1, 3, 2).reshape(N, CB * 8, hw)[:, :C]
    rb = b.permute(0, 1, 3, 2).reshape(N, CB * 8, hw)[:, :C]
    assert torch.equal(ra.view(torch.int16), rb.view(torch.int16)), (what, 'moved with the garbage in the padding lanes')


def new16(shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


# ---------------------------------------------------------------------------------------------------------------- InstanceNorm, C8
def _in8_run(H, r, xs, rs, dys, relu, x_f16):
    N, C, hw, CB = r.N, r.C, r.hw, r.CB
    y, dx = new16((N, CB, hw, 8)), new16((N, CB, hw, 8))
    stats = torch.full((N, C, 2), NAN, device='cuda')
    with Tuned(H, r):
        ws, wa = poisoned_ws(H, N * CB)
        call(H, 'ess_instnorm_forward_c8', P(xs), P(rs), P(y), P(stats), N, C, hw, ctypes.c_float(R.EPS), relu, x_f16, *wa)
        ws2, wa2 = poisoned_ws(H, N * CB)
        call(H, 'ess_instnorm_backward_c8', P(xs), P(dys), P(stats), P(dx), N, C, hw, relu, x_f16, *wa2)
    return y, stats, dx


@pytest.mark.parametrize('res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('relu', [0, 1], ids=['lin', 'relu'])
@pytest.mark.parametrize('x_f16', [0, 1], ids=['xbf16', 'xf16'])
@pytest.mark.parametrize('row', ROWS['in8'], ids=ids(ROWS['in8']))
def test_instance_norm_c8_edges(H, row, x_f16, relu, res):
    """ess_instnorm_forward_c8 and ess_instnorm_backward_c8 (with the forward's statistics) on a BF16_C8 / F16_C8 x, with and without
    ReLU and a BF16_C8 residual: statistics against float64, y and dx within the bounds of tests/norm_ref.py from the kernel's own
    statistics (the exactly constant channel has xhat == 0: its gradient is masked under <= 0, not under < 0)."""
    r, d = Row(row), row_inputs(row)
    assert R.plan(r) == r.label
    xs, dys = store(d['x'], x_f16, r.CB), store(d['dy'], 0, r.CB)
    rs = store(d['res'], 0, r.CB) if res else None
    y, stats, dx = _in8_run(H, r, xs, rs, dys, relu, x_f16)
    clean(y, r.C, 'y'), clean(dx, r.C, 'dx')
    assert not torch.isnan(stats).any()
    st = stats.cpu()
    ratios = {}
    for c0, c1 in chunks(r):
        xv = R.stored(d['x'][:, c0:c1], x_f16)
        rv = R.bfr(d['res'][:, c0:c1]) if res else None
        merge(ratios, R.in_forward_ratios(xv, rv, relu, st[:, c0:c1], {'y': unblock(y, c0, c1)}))
        merge(ratios, R.in_backward_ratios(xv, R.bfr(d['dy'][:, c0:c1]), relu, st[:, c0:c1], unblock(dx, c0, c1)))
    report(r, ('x_f16', x_f16, 'relu', relu, 'res', res), ratios)
    if r.partial:
        y2, stats2, dx2 = _in8_run(H, r, garbage(xs, r.C, 1), garbage(rs, r.C, 2) if res else None, garbage(dys, r.C, 3), relu, x_f16)
        clean(y2, r.C, 'y (garbage)'), clean(dx2, r.C, 'dx (garbage)')
        same_real(y, y2, r.C, 'y'), same_real(dx, dx2, r.C, 'dx')
        assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32)), 'stats moved with the garbage in the padding lanes'


# ---------------------------------------------------------------------------------------------------------------- InstanceNorm, mixed
RES_KINDS = ['nores', 'res_bf16', 'res_f16', 'res_pair']


def _mix_run(H, r, xs, rs, res_f16, dys, relu, x_fmt, want_bf16):
    N, C, hw, CB = r.N, r.C, r.hw, r.CB
    y = new16((N, CB, hw, 8)) if want_bf16 else None
    y16, dx = new16((N, CB, hw, 8), torch.float16), new16((N, CB, hw, 8))
    stats = torch.full((N, C, 2), NAN, device='cuda')
    with Tuned(H, r):
        ws, wa = poisoned_ws(H, N * CB)
        call(H, 'ess_instnorm_forward_c8_mixed', P(xs), P(rs), P(y), P(y16), P(stats), N, C, hw, ctypes.c_float(R.EPS), relu, x_fmt,
             res_f16, *wa)
        ws2, wa2 = poisoned_ws(H, N * CB)
        call(H, 'ess_instnorm_backward_c8', P(xs), P(dys), P(stats), P(dx), N, C, hw, relu, x_fmt, *wa2)
    return y, y16, stats, dx


@pytest.mark.parametrize('kind', RES_KINDS)
@pytest.mark.parametrize('relu', [0, 1], ids=['lin', 'relu'])
@pytest.mark.parametrize('x_fmt', [1, 2], ids=['xf16', 'xpair'])
@pytest.mark.parametrize('row', ROWS['mix'], ids=ids(ROWS['mix']))
def test_instance_norm_mixed_edges(H, row, x_fmt, relu, kind):
    """ess_instnorm_forward_c8_mixed on an F16_C8 / [hi | lo] x with a BF16_C8, an F16_C8 or a [hi | lo] residual (its hi parts are
    added), with y and without it (want_bf16=False: y NULL, y16 and the statistics must not change), and the backward with x_f16 = x_fmt
    (a pair: its hi parts are read)."""
    r, d = Row(row), row_inputs(row)
    assert R.plan(r) == r.label
    xs, dys = store(d['x'], x_fmt, r.CB), store(d['dy'], 0, r.CB)
    rfmt = RES_KINDS.index(kind) - 1
    rs = store(d['res'], rfmt, r.CB) if rfmt >= 0 else None
    y, y16, stats, dx = _mix_run(H, r, xs, rs, max(rfmt, 0), dys, relu, x_fmt, True)
    clean(y, r.C, 'y'), clean(y16, r.C, 'y16'), clean(dx, r.C, 'dx')
    assert not torch.isnan(stats).any()
    xv = R.stored(d['x'], x_fmt)
    rv = None if rfmt < 0 else R.bfr(d['res']) if rfmt == 0 else R.hfr(d['res'])
    st = stats.cpu()
    ratios = R.in_forward_ratios(xv, rv, relu, st, {'y': unblock(y, 0, r.C), 'y16': unblock(y16, 0, r.C)})
    xr = R.stored(d['x'], 1) if x_fmt == 2 else xv
    merge(ratios, R.in_backward_ratios(xr, R.bfr(d['dy']), relu, st, unblock(dx, 0, r.C)))
    report(r, ('x_fmt', x_fmt, 'relu', relu, kind), ratios)
    _, h2, s2, _ = _mix_run(H, r, xs, rs, max(rfmt, 0), dys, relu, x_fmt, False)
    assert torch.equal(h2.view(torch.int16), y16.view(torch.int16)) and torch.equal(s2.view(torch.int32), stats.view(torch.int32)), 'y NULL changed y16 / stats'
    if r.partial:
        gx = torch.cat([garbage(xs[:, :r.CB], r.C, 1), garbage(xs[:, r.CB:], r.C, 4)], 1) if x_fmt == 2 else garbage(xs, r.C, 1)
        gr_ = None if rs is None else (torch.cat([garbage(rs[:, :r.CB], r.C, 2), rs[:, r.CB:]], 1) if rfmt == 2 else garbage(rs, r.C, 2))
        y3, h3, s3, dx3 = _mix_run(H, r, gx, gr_, max(rfmt, 0), garbage(dys, r.C, 3), relu, x_fmt, True)
        clean(y3, r.C, 'y (garbage)'), clean(h3, r.C, 'y16 (garbage)'), clean(dx3, r.C, 'dx (garbage)')
        same_real(y, y3, r.C, 'y'), same_real(y16, h3, r.C, 'y16'), same_real(dx, dx3, r.C, 'dx')
        assert torch.equal(stats.view(torch.int32), s3.view(torch.int32)), 'stats moved with the garbage in the padding lanes'


# ---------------------------------------------------------------------------------------------------------------- BatchNorm, C8
BN_FORMS = ['none', 'none_res', 'y', 'y_res_dres', 'map']  # backward mask form (and what the forward was)


def _bn8_run(H, r, d, xs, rs, dys, form, x_f16):
    """forward, then the backward of `form` -> everything the calls wrote"""
    N, C, hw, CB = r.N, r.C, r.hw, r.CB
    relu = int(form in ('y', 'y_res_dres', 'map'))
    gam, bet = d['gamma'].cuda(), d['beta'].cuda()
    y = new16((N, CB, hw, 8))
    st = torch.full((2, C, 2), NAN, device='cuda')
    rm, rv = d['rm0'].cuda(), d['rv0'].cuda()
    ws, wa = poisoned_ws(H, CB)
    call(H, 'ess_batchnorm_train_forward_c8', P(xs), P(rs), P(gam), P(bet), P(rm), P(rv), ctypes.c_float(R.MOM), ctypes.c_float(R.EPS),
         P(y), P(st), N, C, hw, relu, x_f16, *wa)
    acc = form in ('y', 'map')  # accumulate onto known non-zero values; otherwise onto NaN, which must be overwritten
    dg = d['dgamma0'].cuda() if acc else torch.full((C,), NAN, device='cuda')
    db = d['dbeta0'].cuda() if acc else torch.full((C,), NAN, device='cuda')
    dx = new16((N, CB, hw, 8))
    dres = new16((N, CB, hw, 8)) if form in ('none', 'y_res_dres') else None
    ws2, wa2 = poisoned_ws(H, CB)
    call(H, 'ess_batchnorm_train_backward_c8', P(xs), P(None if form == 'map' else y), P(dys), P(gam), P(bet if form == 'map' else None),
         P(st), P(dx), P(dres), P(dg), P(db), int(acc), N, C, hw, relu, x_f16, *wa2)
    # need_dx=False: the sums alone, onto NaN
    dg2, db2 = torch.full((C,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
    ws3, wa3 = poisoned_ws(H, CB)
    call(H, 'ess_batchnorm_train_backward_c8', P(xs), P(None if form == 'map' else y), P(dys), P(gam), P(bet if form == 'map' else None),
         P(st), P(None), P(None), P(dg2), P(db2), 0, N, C, hw, relu, x_f16, *wa3)
    torch.cuda.synchronize()
    return dict(y=y, st=st, rm=rm, rv=rv, dx=dx, dres=dres, dg=dg, db=db, dg2=dg2, db2=db2, relu=relu, acc=acc)


@pytest.mark.parametrize('form', BN_FORMS)
@pytest.mark.parametrize('x_f16', [0, 1], ids=['xbf16', 'xf16'])
@pytest.mark.parametrize('row', ROWS['bn8'], ids=ids(ROWS['bn8']))
def test_batch_norm_c8_edges(H, row, x_f16, form):
    """ess_batchnorm_train_forward_c8 (statistics, saved map, y, running statistics with the unbiased factor -- cnt = 1 keeps var) and
    ess_batchnorm_train_backward_c8 in its three mask forms, accumulate=True onto known dgamma / dbeta and accumulate=False onto NaN,
    dres bit for bit, and need_dx=False."""
    r, d = Row(row), row_inputs(row)
    assert R.plan(r) == r.label
    N, C, hw = r.N, r.C, r.hw
    res = form in ('none_res', 'y_res_dres')
    xs, dys = store(d['x'], x_f16, r.CB), store(d['dy'], 0, r.CB)
    rs = store(d['res'], 0, r.CB) if res else None
    o = _bn8_run(H, r, d, xs, rs, dys, form, x_f16)
    clean(o['y'], C, 'y'), clean(o['dx'], C, 'dx')
    for k in ('st', 'rm', 'rv', 'dg', 'db', 'dg2', 'db2'):
        assert not torch.isnan(o[k]).any(), (k, 'NaN')
    xv, dyv = R.stored(d['x'], x_f16), R.bfr(d['dy'])
    st = o['st'].cpu()
    yv = unblock(o['y'], 0, C)
    ratios = R.bn_forward_ratios(xv, R.bfr(d['res']) if res else None, o['relu'], d['gamma'], d['beta'], st, yv, d['rm0'], d['rv0'],
                                 o['rm'].cpu(), o['rv'].cpu())
    off = amb = None
    if form in ('y', 'y_res_dres'):
        off = yv <= 0
    elif form == 'map':
        off, amb = R.affine_mask(xv, st)
        assert amb.sum((0, 2)).max().item() <= R.AMBIGUOUS_CAP * N * hw, 'the ambiguous set of the affine mask is over its cap'
    b1 = R.bn_backward_ratios(xv, dyv, st, d['gamma'], off, amb, unblock(o['dx'], 0, C), o['dg'].cpu(), o['db'].cpu(), d['dgamma0'], d['dbeta0'], o['acc'])
    b2 = R.bn_backward_ratios(xv, dyv, st, d['gamma'], off, amb, None, o['dg2'].cpu(), o['db2'].cpu(), d['dgamma0'], d['dbeta0'], False)
    merge(ratios, b1), merge(ratios, {k + '(need_dx=False)': v for k, v in b2.items()})
    report(r, ('x_f16', x_f16, form), ratios)
    if o['dres'] is not None:
        want = torch.where(off, torch.zeros_like(dyv), dyv) if off is not None else dyv
        got = unblock(o['dres'], 0, C)
        assert torch.equal(got, want), 'dres is not the masked copy of dy'
        # padding lanes: dy's own where the mask lets them through, zero where y's (zero) padding lane masks them
        assert torch.equal(padding(o['dres'], C), torch.zeros_like(padding(dys, C)) if o['relu'] else padding(dys, C))
    if r.partial:
        gy = garbage(dys, C, 3)
        o2 = _bn8_run(H, r, d, garbage(xs, C, 1), garbage(rs, C, 2) if res else None, gy, form, x_f16)
        clean(o2['y'], C, 'y (garbage)'), clean(o2['dx'], C, 'dx (garbage)')
        same_real(o['y'], o2['y'], C, 'y'), same_real(o['dx'], o2['dx'], C, 'dx')
        for k in ('st', 'rm', 'rv', 'dg', 'db', 'dg2', 'db2'):
            assert torch.equal(o[k].view(torch.int32), o2[k].view(torch.int32)), (k, 'moved with the garbage in the padding lanes')
        if o['dres'] is not None:
            same_real(o['dres'], o2['dres'], C, 'dres')
            assert torch.equal(padding(o2['dres'], C), torch.zeros_like(padding(gy, C)) if o['relu'] else padding(gy, C))


# ---------------------------------------------------------------------------------------------------------------- fp32 (csrc/norm.hip)
def dev32(t, misaligned):
    """fp32 device tensor; misaligned: the same values one float into a larger buffer (4-byte aligned, not 16)"""
    if t is None:
        return None
    if not misaligned:
        return t.cuda().contiguous()
    buf = torch.empty(t.numel() + 1, device='cuda')
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def nan32(shape, misaligned):
    return dev32(torch.full(shape, NAN), misaligned)


@pytest.mark.parametrize('res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('relu', [0, 1, 2], ids=['lin', 'relu', 'relu_after_res'])
@pytest.mark.parametrize('row', ROWS['in32'], ids=ids(ROWS['in32']))
def test_instance_norm_fp32_edges(H, row, relu, res):
    """ess_instnorm_forward (relu 0, 1 and 2 = after the residual) and ess_instnorm_backward (relu 0 and 1) of csrc/norm.hip: planes held
    in registers, the strided 16-byte loop, the scalar loop (odd plane, misaligned tensors), the split pair with 16-byte and scalar loads."""
    r, d = Row(row), row_inputs(row)
    assert R.plan(r) == r.label
    N, C, hw, mis = r.N, r.C, r.hw, r.misaligned
    x, dy, rs = dev32(d['x'], mis), dev32(d['dy'], mis), dev32(d['res'], mis) if res else None
    y, dx = nan32((N, C, hw), mis), nan32((N, C, hw), mis)
    stats = torch.full((N, C, 2), NAN, device='cuda')
    ws, wa = poisoned_ws(H, N * C, c8=False)
    call(H, 'ess_instnorm_forward', P(x), P(rs), P(y), P(stats), N * C, hw, ctypes.c_float(R.EPS), relu, *wa)
    if relu < 2:
        ws2, wa2 = poisoned_ws(H, N * C, c8=False)
        call(H, 'ess_instnorm_backward', P(x), P(dy), P(stats), P(dx), N * C, hw, relu, *wa2)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(stats).any()
    st, ratios = stats.cpu(), {}
    for c0, c1 in chunks(r):
        xv = d['x'][:, c0:c1].double()
        rv = d['res'][:, c0:c1].double() if res else None
        merge(ratios, R.in_forward_ratios(xv, rv, relu, st[:, c0:c1], {'y32': y[:, c0:c1].double().cpu()}, fp32_kernel=True))
        if relu < 2:
            merge(ratios, R.in_backward_ratios(xv, d['dy'][:, c0:c1].double(), relu, st[:, c0:c1], dx[:, c0:c1].double().cpu(), fp32_kernel=True))
    assert relu == 2 or not torch.isnan(dx).any()
    report(r, ('relu', relu, 'res', res), ratios)


def test_instance_norm_fp32_backward_refuses_relu_after_residual(H):
    """relu = 2 (ReLU after the residual) is forward only: the backward refuses it and writes nothing"""
    x = torch.randn(2, 3, 16, device='cuda')
    stats = torch.zeros(6, 2, device='cuda')
    dx = torch.full_like(x, NAN)
    ws, wa = poisoned_ws(H, 6, c8=False)
    rc = H.lib().ess_instnorm_backward(P(x), P(x), P(stats), P(dx), 6, 16, 2, *wa, H.stream())
    torch.cuda.synchronize()
    assert rc != 0 and b'forward only' in H.lib().ess_last_error()
    assert torch.isnan(dx).all()


@pytest.mark.parametrize('form', BN_FORMS[:-1])
@pytest.mark.parametrize('row', ROWS['bn32'], ids=ids(ROWS['bn32']))
def test_batch_norm_fp32_edges(H, row, form):
    """ess_batchnorm_train_forward / backward of csrc/norm.hip (the mask always comes from the stored y), with dres, accumulate and
    need_dx=False as for the C8 kernels."""
    r, d = Row(row), row_inputs(row)
    assert R.plan(r) == r.label
    N, C, hw, mis = r.N, r.C, r.hw, r.misaligned
    res, relu = form in ('none_res', 'y_res_dres'), int(form in ('y', 'y_res_dres'))
    x, dy, rs = dev32(d['x'], mis), dev32(d['dy'], mis), dev32(d['res'], mis) if res else None
    gam, bet = d['gamma'].cuda(), d['beta'].cuda()
    y, dx = nan32((N, C, hw), mis), nan32((N, C, hw), mis)
    dres = nan32((N, C, hw), mis) if form in ('none', 'y_res_dres') else None
    st = torch.full((C, 2), NAN, device='cuda')
    rm, rv = d['rm0'].cuda(), d['rv0'].cuda()
    ws, wa = poisoned_ws(H, C, c8=False)
    call(H, 'ess_batchnorm_train_forward', P(x), P(rs), P(gam), P(bet), P(rm), P(rv), ctypes.c_float(R.MOM), ctypes.c_float(R.EPS), P(y),
         P(st), N, C, hw, relu, *wa)
    acc = form == 'y'
    dg = d['dgamma0'].cuda() if acc else torch.full((C,), NAN, device='cuda')
    db = d['dbeta0'].cuda() if acc else torch.full((C,), NAN, device='cuda')
    ws2, wa2 = poisoned_ws(H, C, c8=False)
    call(H, 'ess_batchnorm_train_backward', P(x), P(y), P(dy), P(gam), P(st), P(dx), P(dres), P(dg), P(db), int(acc), N, C, hw, relu, *wa2)
    dg2, db2 = torch.full((C,), NAN, device='cuda'), torch.full((C,), NAN, device='cuda')
    ws3, wa3 = poisoned_ws(H, C, c8=False)
    call(H, 'ess_batchnorm_train_backward', P(x), P(y), P(dy), P(gam), P(st), P(None), P(None), P(dg2), P(db2), 0, N, C, hw, relu, *wa3)
    torch.cuda.synchronize()
    for t in (y, dx, st, rm, rv, dg, db, dg2, db2):
        assert not torch.isnan(t).any()
    xv, dyv, yv, stc = d['x'].double(), d['dy'].double(), y.double().cpu(), st.cpu()
    ratios = R.bn_forward_ratios(xv, d['res'].double() if res else None, relu, d['gamma'], d['beta'], stc, yv, d['rm0'], d['rv0'], rm.cpu(),
                                 rv.cpu(), fp32_kernel=True)
    off = yv <= 0 if relu else None
    b1 = R.bn_backward_ratios(xv, dyv, stc, d['gamma'], off, None, dx.double().cpu(), dg.cpu(), db.cpu(), d['dgamma0'], d['dbeta0'], acc, fp32_kernel=True)
    b2 = R.bn_backward_ratios(xv, dyv, stc, d['gamma'], off, None, None, dg2.cpu(), db2.cpu(), d['dgamma0'], d['dbeta0'], False, fp32_kernel=True)
    merge(ratios, b1), merge(ratios, {k + '(need_dx=False)': v for k, v in b2.items()})
    report(r, (form,), ratios)
    if dres is not None:
        want = torch.where(off, torch.zeros_like(dyv), dyv) if off is not None else dyv
        assert torch.equal(dres.double().cpu(), want), 'dres is not the masked copy of dy'
