"""GPU tier: the mixed configuration's kernels (ESS_COMPUTE_F16 convolutions, their recurrent epilogues, the norm statistics they feed)
against fp64 torch-CPU restatements of the same operation on the same rounded operands (half-rounded inputs and weights, hi + lo for a
[hi | lo] pair), at the shapes where tiles are partial, channel tiles are padded and the dispatcher changes kernels.  Every output tensor
is filled with NaN before its launch: a tile, a lo block or a channel block the kernel leaves unwritten fails the comparison.
Reference layers: e2vid/model/submodules.py:24-31, 190-230, 283-380 and models/style_networks.py:158-193."""
import math

import pytest
import torch
import torch.nn.functional as F

from norm_ref import _bwd_check, _channels, _check_stats

pytestmark = pytest.mark.gpu

NAN = float('nan')


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


def hfr(x):
    return x.to(torch.float16).float()


def unblock(t, C):
    """fp32 NCHW values of a 16-bit [N][CB][H][W][8] tensor"""
    N, nb, Hh, W, _ = t.shape
    return t.float().permute(0, 1, 4, 2, 3).reshape(N, nb * 8, Hh, W)[:, :C].cpu()


def unblock_hilo(t, C):
    nb = t.shape[1] // 2
    return unblock(t[:, :nb], C).double() + unblock(t[:, nb:], C).double()


def f32_blocked(t):
    """fp32 [N][C/8][H][W][8] of an fp32 NCHW tensor (C % 8 == 0)"""
    N, C, Hh, W = t.shape
    return t.view(N, C // 8, 8, Hh, W).permute(0, 1, 3, 4, 2).contiguous().cuda()


def unblock32(t, C):
    N, nb, Hh, W, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(N, nb * 8, Hh, W)[:, :C].cpu().double()


class Wide:
    """tuning switch conv_wide for the duration of a block: 0 = the wave-specialised kernels only, 2 = the wide-tile kernel wherever one of
    its forms applies"""

    def __init__(self, H, mode):
        self.H, self.mode = H, mode

    def __enter__(self):
        self.prev = self.H.tuning_get('conv_wide')
        self.H.tuning_set('conv_wide', self.mode)

    def __exit__(self, *a):
        self.H.tuning_set('conv_wide', self.prev)


def wide_form(H, Cout, cout_tile, Ho, Wo, N):
    """<MBW, CW> the dispatcher's wide-tile pick (conv_bf16.hip wide_pick: the cheapest candidate by rounds x tile, in candidate order)
    takes for a LINEAR launch when the wide kernel is forced; None when no candidate applies.  A restatement of the dispatcher's rule, not
    an observation of it: which kernel a launch took is not visible from here, so this only keeps each case's label true to the rule (the
    recurrent cases with conv_wide = 2 likewise take the wide kernel only where wide_pick_recurrent's conditions hold -- e.g. not for a
    GRU_OUT launch whose packed rows are not a multiple of 128 -- and the ws kernel otherwise)"""
    cus = H.tuning_get('device_cus')
    mb, best, pick = cout_tile // 32, None, None
    for mbw, cw in ((2, 2), (2, 1), (1, 2), (1, 1)):
        cot = mbw * cw * 32
        if (mb == 2) != (cot >= 64) or mb > 2 or Cout % cot:
            continue
        th, tw = (4 // cw) * 5 * 2, 16
        tiles = math.ceil(Wo / tw) * math.ceil(Ho / th) * (Cout // cot) * N
        cost = math.ceil(tiles / cus) * cot * th * tw
        if best is None or cost < best:
            best, pick = cost, (mbw, cw)
    return pick


# ---------------------------------------------------------------------------------------------------------------- convolutions
CONV_EDGE_CASES = [
    # id, N, (C0, pair0), (C1, pair1), Cout, Hv, Wv, k, s, p, mode0, relu, affine, out, wide, expected kernel / instantiation
    ('ws2_h16_c96_odd', 2, (64, False), (0, False), 96, 13, 21, 3, 1, 1, 0, False, False, 'h16', 0, 'ws<2,O8,H>'),
    ('ws1_f32_c11_odd', 2, (32, False), (0, False), 11, 9, 23, 3, 1, 1, 0, False, True, 'f32', 0, 'ws<1,f32,H>'),
    ('ws1_h16_c32_odd', 2, (32, False), (0, False), 32, 11, 19, 3, 1, 1, 0, True, True, 'h16', 0, 'ws<1,O8,H>'),
    ('ws2_f32_c96_pair1', 2, (64, False), (32, True), 96, 9, 21, 3, 1, 1, 0, False, True, 'f32', 0, 'ws<2,f32,H>'),
    ('ws2_hilo_c192_pair1', 2, (64, False), (64, True), 192, 11, 19, 3, 1, 1, 0, True, True, 'hilo', 0, 'ws<2,O8,H>'),
    ('ws2_hilo_c320_pair0', 1, (128, True), (0, False), 320, 12, 17, 3, 1, 1, 0, False, False, 'hilo', 0, 'ws<2,O8,H>'),
    ('ws2_h16_pair_both_384', 2, (128, True), (64, True), 128, 10, 18, 3, 1, 1, 0, True, False, 'h16', 0, 'ws<2,O8,H>'),
    ('ws4_h16_c320_pair0_512', 1, (256, True), (0, False), 320, 11, 19, 3, 1, 1, 0, False, False, 'h16', 0, 'ws<4,O8,H>'),
    ('ws4_hilo_c256_pair0_512', 1, (256, True), (0, False), 256, 9, 18, 3, 1, 1, 0, True, True, 'hilo', 0, 'ws<4,O8,H>'),
    ('ws4_f32_c320_512', 1, (256, False), (256, False), 320, 7, 13, 3, 1, 1, 0, False, False, 'f32', 0, 'ws<4,f32,H>'),
    ('wide12_hilo_c192', 2, (64, True), (0, False), 192, 13, 21, 3, 1, 1, 0, False, True, 'hilo', 2, 'wide<1,2>'),
    ('wide21_h16_c192', 4, (64, False), (0, False), 192, 100, 80, 3, 1, 1, 0, True, False, 'h16', 2, 'wide<2,1>'),
    ('wide22_hilo_c256', 8, (128, True), (0, False), 256, 60, 80, 3, 1, 1, 0, True, False, 'hilo', 2, 'wide<2,2>'),
    ('wide11_h16_c32_odd', 2, (48, False), (16, True), 32, 15, 27, 3, 1, 1, 0, True, True, 'h16', 2, 'wide<1,1>'),
    ('poly_h16_c96_odd', 2, (64, False), (0, False), 96, 18, 22, 3, 1, 1, 1, False, True, 'h16', 0, 'poly<H>'),
    ('poly_h16_c64_pair0', 1, (32, True), (0, False), 64, 14, 26, 3, 1, 1, 1, True, False, 'h16', 0, 'poly<H>'),
    ('ws_up_concat_pair1', 2, (64, False), (32, True), 64, 14, 26, 3, 1, 1, 1, False, False, 'h16', 0, 'ws<2,O8,H>'),
    ('pair_s2_h16_c96_odd', 2, (16, False), (0, False), 96, 23, 37, 5, 2, 2, 0, True, True, 'h16', 0, 'pair<S2,MB1,O8,H>'),
    ('pair_s2_f32_c11', 2, (32, True), (0, False), 11, 22, 30, 5, 2, 2, 0, False, False, 'f32', 0, 'pair<S2,MB1,f32,H>'),
    ('pair_s1_h16_c64_odd', 2, (16, False), (0, False), 64, 13, 21, 5, 1, 2, 0, True, False, 'h16', 0, 'pair<S1,MB2,O8,H>'),
    ('pair_s1_f32_c32_pair0', 1, (16, True), (0, False), 32, 12, 19, 5, 1, 2, 0, False, True, 'f32', 0, 'pair<S1,MB1,f32,H>'),
    ('pair_s1_f32_c64_odd', 2, (16, False), (0, False), 64, 11, 23, 5, 1, 2, 0, False, False, 'f32', 0, 'pair<S1,MB2,f32,H>'),
    ('pair_s1_h16_c32_pair0', 1, (16, True), (0, False), 32, 13, 19, 5, 1, 2, 0, True, True, 'h16', 0, 'pair<S1,MB1,O8,H>'),
    ('s2d21_hilo_c64', 8, (32, False), (0, False), 64, 192, 320, 5, 2, 2, 0, True, True, 'hilo', 0, 's2d<2,1>'),
    ('s2d22_h16_c128_pair0', 4, (32, True), (0, False), 128, 192, 320, 5, 2, 2, 0, False, False, 'h16', 0, 's2d<2,2>'),
    ('gen_1x1_c11_f32', 2, (32, False), (0, False), 11, 13, 21, 1, 1, 0, 0, False, False, 'f32', 0, 'generic<1,1,MB1,CB8=4,H>'),
    ('gen_1x1_c96_h16_cin16', 2, (16, False), (0, False), 96, 13, 21, 1, 1, 0, 0, True, True, 'h16', 0, 'generic<1,1,MB2,CB8=2,H>'),
    ('gen_1x1_c64_hilo_pair0', 2, (64, True), (0, False), 64, 9, 22, 1, 1, 0, 0, False, False, 'hilo', 0, 'generic<1,1,MB2,CB8=4,H>'),
    ('gen_3x3s2_c96_h16_odd', 2, (32, False), (0, False), 96, 23, 33, 3, 2, 1, 0, True, True, 'h16', 0, 'generic<3,2,MB2,H>'),
    ('gen_1x1s2_c32_f32', 2, (32, False), (0, False), 32, 18, 26, 1, 2, 0, 0, False, False, 'f32', 0, 'generic<1,2,MB1,H>'),
    ('gen_1x1_c32_h16_cin16', 2, (16, False), (0, False), 32, 13, 21, 1, 1, 0, 0, False, True, 'h16', 0, 'generic<1,1,MB1,CB8=2,H>'),
    ('gen_1x1s2_c96_h16_pair0', 2, (32, True), (0, False), 96, 18, 27, 1, 2, 0, 0, True, False, 'h16', 0, 'generic<1,2,MB2,H>'),
    ('gen_3x3s2_c11_f32_odd', 2, (32, False), (0, False), 11, 21, 31, 3, 2, 1, 0, False, True, 'f32', 0, 'generic<3,2,MB1,H>'),
]
# Not reached by these cases, because default dispatch cannot reach them: generic<3,1,*,H> (a 3x3 / stride-1 launch reaches the generic
# kernel only with the ws kernel switched off by environment, read once per process), pair<S2,MB2,*,H> (stride-2 5x5 launches take 32-row
# tiles unless an environment switch says otherwise).  The ws kernel's recurrent instantiations are reached by the recurrent tests below.


def _operand(H, x, pair):
    """device F16_C8 tensor of x (a [hi | lo] pair if `pair`) and the (hi, lo) values it holds (lo None without a pair)"""
    C = x.shape[1]
    t = H.to_f16_c8(x.cuda(), hilo=pair)
    if pair:
        nb = t.shape[1] // 2
        return t, unblock(t[:, :nb], C).double(), unblock(t[:, nb:], C).double()
    return t, unblock(t, C).double(), None


@pytest.mark.parametrize('case', CONV_EDGE_CASES, ids=[c[0] for c in CONV_EDGE_CASES])
def test_conv_f16_edges(H, case):
    """One half-operand convolution per dispatch path and edge: the result against the fp64 convolution of the operands the kernel reads
    (a pair contributes w * hi + w * lo through repeated weight columns).  Bounds, relative to max(1, |ref|): fp32 output 2e-5 (fp32
    accumulation of exact half x half products), half output one rounding 2^-11, a [hi | lo] output 2^-20 (hi + lo keeps ~22 bits);
    the polyphase kernel's effective weights carry one more half rounding (x4)."""
    from ess_amd.functional import packed_weight
    (cid, N, (C0, d0), (C1, d1), Cout, Hv, Wv, k, s, p, m0, relu, affine, outk, wide, kern) = case
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    sh = 2 if m0 == 1 else 1
    x0 = torch.randn(N, C0, Hv // sh, Wv // sh, generator=g) * 1.3 + 1.5
    x1 = torch.randn(N, C1, Hv, Wv, generator=g) * 2 - 0.5 if C1 else None
    w = torch.randn(Cout, C0 + C1, k, k, generator=g) * (1.0 / (k * (C0 + C1) ** 0.5))
    bias = torch.randn(Cout, generator=g) * 0.1
    scale = torch.rand(Cout, generator=g) + 0.5 if affine else None
    h0, x0h, x0l = _operand(H, x0, d0)
    h1, x1h, x1l = _operand(H, x1, d1) if C1 else (None, None, None)
    wq = hfr(w).double()
    up = (lambda t: F.interpolate(t, scale_factor=2, mode='nearest')) if m0 == 1 else (lambda t: t)
    ref = F.conv2d(up(x0h), wq[:, :C0], None, s, p)
    if d0:
        ref = ref + F.conv2d(up(x0l), wq[:, :C0], None, s, p)
    if C1:
        ref = ref + F.conv2d(x1h, wq[:, C0:], None, s, p)
        if d1:
            ref = ref + F.conv2d(x1l, wq[:, C0:], None, s, p)
    ref = ref * (scale.double().view(1, -1, 1, 1) if affine else 1.0) + bias.double().view(1, -1, 1, 1)
    if relu:
        ref = ref.clamp(min=0)
    act = H.ACT_RELU if relu else H.ACT_NONE
    cols = [w[:, :C0]] * (2 if d0 else 1) + ([w[:, C0:]] * (2 if d1 else 1) if C1 else [])
    wd = torch.cat(cols, 1).contiguous()
    C0e, C1e = C0 * (2 if d0 else 1), C1 * (2 if d1 else 1)
    spec = H.conv_spec(N, Hv, Wv, C0e, C1e, Cout, k, s, p, mode0=m0, act=act, compute=H.COMPUTE_F16)
    kind = H.W_CONV
    if k == 5 and s == 2 and (4 * C0e) % 128 == 0 and C1 == 0 and Cout % 64 == 0:  # (the forms ESS_SRC_S2D exists for)
        s2 = H.conv_spec(N, Hv // 2, Wv // 2, 4 * C0e, 0, Cout, 3, 1, 1, mode0=H.SRC_S2D, act=act, compute=H.COMPUTE_F16)
        assert H.s2d_preferred(s2) == kern.startswith('s2d'), (cid, 'space-to-depth choice')
        if kern.startswith('s2d'):
            spec, kind = s2, H.W_CONV5_S2D
            assert spec.plan.cout_tile == 64
    # the plan's channel tile (the instantiation's MB) and, where the wide kernel is forced, the <MBW, CW> form it takes
    mb = {'ws<4': 4, 'ws<2': 2, 'ws<1': 1, 'pair<S2,MB1': 1, 'pair<S1,MB2': 2, 'pair<S1,MB1': 1, 'generic<1,1,MB1': 1,
          'generic<1,1,MB2': 2, 'generic<3,2,MB2': 2, 'generic<3,2,MB1': 1, 'generic<1,2,MB1': 1, 'generic<1,2,MB2': 2}
    for key, v in mb.items():
        if kern.startswith(key):
            assert spec.plan.cout_tile == 32 * v, (cid, spec.plan.cout_tile)
    if kern.startswith('generic<1,1'):
        assert spec.plan.ck == (32 if 'CB8=4' in kern else 16)
    if kern.startswith('wide'):
        assert spec.plan.cout_tile == (32 if kern == 'wide<1,1>' else 64)
        assert wide_form(H, Cout, spec.plan.cout_tile, spec.H_out, spec.W_out, N) == (int(kern[5]), int(kern[7])), cid
    pw = packed_weight(spec, wd.cuda(), kind=kind)
    sc = H.pack_rows(spec, scale.cuda(), fill=1.0) if affine else None
    shf = H.pack_rows(spec, bias.cuda())
    Ho, Wo = ref.shape[2], ref.shape[3]
    with Wide(H, wide):
        if outk == 'f32':
            out = torch.full((N, Cout, Ho, Wo), NAN, device='cuda')
            H.conv_forward_h16(spec, h0, h1, pw, sc, shf, out=out)
            torch.cuda.synchronize()
            got = out.cpu().double()
            tol = 2e-5
        else:
            out = H.f16_blocks_empty(N, Cout, Ho, Wo, 'cuda', hilo=outk == 'hilo').fill_(NAN)
            H.conv_forward_h16(spec, h0, h1, pw, sc, shf, out=out, out_fmt=H.FMT_F16_C8_HILO if outk == 'hilo' else H.FMT_F16_C8)
            torch.cuda.synchronize()
            got = unblock_hilo(out, Cout) if outk == 'hilo' else unblock(out, Cout).double()
            tol = 2 ** -20 if outk == 'hilo' else 2 ** -11
    assert not torch.isnan(got).any(), (cid, 'unwritten output elements', int(torch.isnan(got).sum()))
    if outk == 'hilo':  # every lo block written (a NaN lo would already fail above; this names the block)
        nb = out.shape[1] // 2
        lo = unblock(out[:, nb:], Cout)
        assert not torch.isnan(lo).any(), (cid, 'lo blocks', sorted(set(torch.isnan(lo).nonzero()[:, 1].div(8, rounding_mode='floor').tolist())))
    err = ((got - ref).abs() / ref.abs().clamp(min=1.0)).max().item()
    if kern.startswith('poly'):
        tol *= 4  # (four half weights summed in fp32 and rounded to half once more: a second 2^-12 rounding of the effective weights)
    assert err <= tol * 1.5 + 3e-6, (cid, err)


def test_conv2dfn_hilo_request_on_partial_channel_tiles(H):
    """Conv2dFn in the mixed configuration asked for a [hi | lo] pre-norm output (INSResBlock's first convolution) where the plan cannot
    give one: C_out = 320 behind a doubled 256-channel source takes 128-channel tiles (512 input channels), and the plan refuses a pair
    output on a half-filled tile.  The function writes one half copy instead -- within its rounding of the fp64 convolution of hi + lo --
    and still writes the pair where the tiles are whole (C_out = 256)."""
    from ess_amd import copies, functional as Fn
    N, C, Hh, W = 1, 256, 9, 19
    g = torch.Generator().manual_seed(320)
    x = torch.randn(N, C, Hh, W, generator=g) + 1.5
    H.set_compute('mixed')
    try:
        for Cout in (320, 256):
            w = torch.randn(Cout, C, 3, 3, generator=g) / (3 * C ** 0.5)
            b = torch.randn(Cout, generator=g) * 0.1
            x8 = H.to_bf16_c8(x.cuda())
            pair = H.to_f16_c8(x.cuda(), hilo=True)
            H.attach_h16(x8, pair, hilo=True)
            out = Fn.conv2d(x8, w.cuda(), b.cuda(), 1, 1, out_c8=Fn.PRE_NORM_HILO, half=True)
            torch.cuda.synchronize()
            ref = F.conv2d(unblock_hilo(pair, C), hfr(w).double(), b.double(), 1, 1)
            if Cout == 320:
                assert H.is_f16_c8(out) and copies.of(out).pair is None
                got = H.f16_c8_to_float(out, Cout).cpu().double()
                tol = 2 ** -11
            else:
                got = unblock_hilo(copies.of(out).pair, Cout)
                tol = 2 ** -20
            err = ((got - ref).abs() / ref.abs().clamp(min=1.0)).max().item()
            assert err <= tol * 1.5 + 3e-6, (Cout, err)
    finally:
        H.set_compute('fp32')


def test_head_f16_edges(H):
    """the 5x5 head kernel on half operands (fp32 NCHW image rounded to half in the kernel): 2 and 3-5 input channels (the two
    instantiations of its channel count), with and without a scale, odd extents, 11 and 32 output channels"""
    from ess_amd.functional import packed_weight
    for C, Cout, Hh, W, affine in ((2, 32, 37, 51, True), (3, 11, 23, 45, False), (5, 32, 17, 29, True), (2, 11, 21, 35, False)):
        g = torch.Generator().manual_seed(C * 100 + Cout)
        x = torch.randn(1, C, Hh, W, generator=g) * (torch.rand(1, C, Hh, W, generator=g) < 0.3) * 3
        w = torch.randn(Cout, C, 5, 5, generator=g) * 0.1
        b = torch.randn(Cout, generator=g) * 0.1
        sc = torch.rand(Cout, generator=g) + 0.5
        ref = F.conv2d(hfr(x).double(), hfr(w).double(), None, 1, 2)
        ref = (ref * sc.double().view(1, -1, 1, 1) if affine else ref) + b.double().view(1, -1, 1, 1)
        ref = ref.clamp(min=0)
        spec = H.conv_spec(1, Hh, W, C, 0, Cout, 5, 1, 2, act=H.ACT_RELU, compute=H.COMPUTE_F16)
        assert spec.plan.cout_tile == 32 and spec.plan.n_chunks == 1
        out = torch.full((1, Cout, Hh, W), NAN, device='cuda')
        h16 = H.f16_blocks_empty(1, Cout, Hh, W, 'cuda').fill_(NAN)
        H.conv_forward_h16(spec, x.cuda(), None, packed_weight(spec, w.cuda()), H.pack_rows(spec, sc.cuda(), fill=1.0) if affine else None,
                           H.pack_rows(spec, b.cuda()), out=out, out_h16=h16, src_fp32=True)
        torch.cuda.synchronize()
        got = out.cpu().double()
        assert not torch.isnan(got).any()
        assert (got - ref).abs().max().item() < 2e-5, (C, Cout)  # (fp32 accumulation of exact half x half products, |ref| < 4)
        assert torch.equal(unblock(h16, Cout), hfr(out.cpu()))


# ---------------------------------------------------------------------------------------------------------------- recurrent epilogues
def _sig(t):
    return torch.sigmoid(t)


REC_CASES = [
    # hid, N, Hh, W, first step, wide mode, saturate, x channels (a [hi | lo] pair: twice as many stored)
    (8, 2, 9, 13, False, 0, False, 32),        # 32-row tiles (LSTM: 4 x 8 gate rows)
    (256, 1, 12, 20, False, 0, False, 256),    # 512 + 256 input channels: 128-row tiles (the deepest level's form)
    (16, 2, 13, 21, False, 0, False),
    (64, 2, 24, 40, True, 0, False),
    (64, 1, 30, 44, False, 2, False),
    (128, 1, 17, 23, False, 0, False),
    (128, 2, 30, 40, True, 2, False),
    (256, 1, 12, 20, False, 0, False),
    (256, 1, 15, 20, False, 2, False),
    (64, 1, 11, 19, False, 0, True),
]
REC_CASES = [c if len(c) == 8 else c + (32,) for c in REC_CASES]


@pytest.mark.parametrize('case', REC_CASES)
def test_conv_lstm_f16_edges(H, case):
    """One ConvLSTM step on half operands (x a [hi | lo] pair, h a half copy, channel-blocked fp32 cell): the plain form (h' as one half
    copy) and LSTM_H_HILO (h' as a [hi | lo] pair) against fp64 gates on the same operands.  First step: no h source, no cell (c = 0).
    Bounds: cell 3e-5 (fp32 accumulation; |gates| ~ 1, fast sigma / tanh within a few fp32 ulp), h' pair 2e-5, h' half copy its
    rounding 2^-11 |h'| + 2e-5.  saturate: pre-activations of |z| ~ 20-40 (sigma / tanh of the fast exp / rcp forms at their limits)."""
    from ess_amd.functional import packed_weight
    hid, N, Hh, W, first, wide, sat, C = case
    g = torch.Generator().manual_seed(hid + Hh + 7 * sat)
    x = torch.randn(N, C, Hh, W, generator=g).clamp(min=0) * 2 + 3
    h = torch.tanh(torch.randn(N, hid, Hh, W, generator=g))
    c = torch.randn(N, hid, Hh, W, generator=g)
    C1 = 0 if first else hid
    wg = torch.randn(4 * hid, C + C1, 3, 3, generator=g) * (1.0 / (3 * (C + C1) ** 0.5))
    bg = torch.randn(4 * hid, generator=g) * 0.1
    if sat:  # (gate pre-activations of 20-40 in magnitude, both signs)
        wg = wg * 0.0
        bg = (torch.rand(4 * hid, generator=g) * 20 + 20) * torch.where(torch.rand(4 * hid, generator=g) < 0.5, -1.0, 1.0)
    xh = H.to_f16_c8(x.cuda(), hilo=True)
    hh = None if first else H.to_f16_c8(h.cuda())
    xin = unblock_hilo(xh, C) if first else torch.cat([unblock_hilo(xh, C), hfr(h).double()], 1)
    gates = F.conv2d(xin, hfr(wg).double(), bg.double(), padding=1)
    i, f, o, gg = gates.chunk(4, 1)
    c_prev = torch.zeros_like(c).double() if first else c.double()
    cn = _sig(f) * c_prev + _sig(i) * torch.tanh(gg)
    hn = _sig(o) * torch.tanh(cn)
    wd = torch.cat([wg[:, :C], wg[:, :C], wg[:, C:]], 1).contiguous()
    c8 = None if first else f32_blocked(c)
    for act in (H.LSTM_H_HILO, 0):
        spec = H.conv_spec(N, Hh, W, 2 * C, C1, 4 * hid, 3, 1, 1, epi=H.EPI_LSTM, hidden=hid, compute=H.COMPUTE_F16)
        if act and (hid % (8 * (spec.plan.cout_tile // 32)) or spec.plan.cout_tile < 64):
            continue  # (no pair copy of h' on such tiles: the product writes one half copy there, submodules.ConvLSTM.forward)
        spec = H.conv_spec(N, Hh, W, 2 * C, C1, 4 * hid, 3, 1, 1, epi=H.EPI_LSTM, hidden=hid, act=act, compute=H.COMPUTE_F16)
        cell = H.f32_c8_empty(N, hid, Hh, W, 'cuda').fill_(NAN)
        new16 = H.f16_blocks_empty(N, hid, Hh, W, 'cuda', hilo=act == H.LSTM_H_HILO).fill_(NAN)
        with Wide(H, wide):
            H.conv_forward_h16(spec, xh, hh, packed_weight(spec, wd.cuda()), None, H.pack_rows(spec, bg.cuda()), aux0=c8, out=None,
                               out2=cell, out_h16=new16, out_fmt=H.FMT_F32_C8, aux_fmt=H.FMT_F32_C8)
            torch.cuda.synchronize()
        gc = unblock32(cell, hid)
        assert not torch.isnan(gc).any() and (gc - cn).abs().max().item() < 3e-5, (act, (gc - cn).abs().max().item())
        if act:
            gh = unblock_hilo(new16, hid)
            assert not torch.isnan(gh).any() and (gh - hn).abs().max().item() < 2e-5, (gh - hn).abs().max().item()
        else:
            gh = unblock(new16, hid).double()
            assert not torch.isnan(gh).any()
            assert ((gh - hn).abs() - 2 ** -11 * hn.abs()).max().item() < 2e-5


@pytest.mark.parametrize('case', REC_CASES)
def test_conv_gru_f16_edges(H, case):
    """One ConvGRU step on half operands, as the mixed configuration runs it (submodules.ConvGRU.forward, half kind): GRU_UR writes the update
    gate u (IEEE half with GRU_U_F16 where whole gate tiles allow, else fp32) and the half copy of r * h; GRU_OUT reads them and writes
    h' = h (1 - u) + u tanh(o) (fp32 channel-blocked + half copy, or a [hi | lo] copy with GRU_H_HILO).  Each launch against fp64 on the
    operands it reads: u within its storage rounding of sigma (2^-11 u / fp32) + 2e-6, r * h within 2^-11 |r h| + 2e-6, h' within 3e-5
    (fp32 accumulation, fast tanh), its pair 3e-5 and its half copy 2^-11 |h'| + 3e-5.  First step: no h source, h = 0."""
    from ess_amd.functional import packed_weight
    hid, N, Hh, W, first, wide, sat, C = case
    g = torch.Generator().manual_seed(3 * hid + W + 11 * sat)
    x = torch.randn(N, C, Hh, W, generator=g).clamp(min=0) * 2 + 3
    h = torch.randn(N, hid, Hh, W, generator=g)
    C1 = 0 if first else hid
    wu, wr, wo = [torch.randn(hid, C + C1, 3, 3, generator=g) * (1.0 / (3 * (C + C1) ** 0.5)) for _ in range(3)]
    bu, br, bo = [torch.randn(hid, generator=g) * 0.1 for _ in range(3)]
    if sat:
        wu, wr, wo = wu * 0, wr * 0, wo * 0
        bu, br, bo = [(torch.rand(hid, generator=g) * 20 + 20) * torch.where(torch.rand(hid, generator=g) < 0.5, -1.0, 1.0) for _ in range(3)]
    xh = H.to_f16_c8(x.cuda(), hilo=True)
    x_eff = unblock_hilo(xh, C)
    hs = None if first else H.to_f16_c8(h.cuda())
    hq = hfr(h).double()
    h32 = None if first else f32_blocked(h)
    dup = lambda w_: torch.cat([w_[:, :C], w_[:, :C], w_[:, C:]], 1).contiguous()  # noqa: E731
    xin = x_eff if first else torch.cat([x_eff, hq], 1)
    zu = F.conv2d(xin, hfr(wu).double(), bu.double(), padding=1)
    zr = F.conv2d(xin, hfr(wr).double(), br.double(), padding=1)
    u_ref = _sig(zu)
    rh_ref = None if first else _sig(zr) * h.double()
    for uact in (H.GRU_U_F16, H.GRU_U_F32):
        s1 = H.conv_spec(N, Hh, W, 2 * C, C1, 2 * hid, 3, 1, 1, epi=H.EPI_GRU_UR, act=uact, hidden=hid, compute=H.COMPUTE_F16)
        if uact == H.GRU_U_F16 and hid % (s1.plan.cout_tile // 2):
            continue  # (refused there: the product uses GRU_U_F32 at such a hidden size)
        u = (H.f16_c8_raw_empty if uact == H.GRU_U_F16 else H.f32_c8_empty)(N, hid, Hh, W, 'cuda').fill_(NAN)
        rh16 = None if first else H.f16_blocks_empty(N, hid, Hh, W, 'cuda').fill_(NAN)
        with Wide(H, wide):
            H.conv_forward_h16(s1, xh, hs, packed_weight(s1, dup(wu).cuda(), dup(wr).cuda()), None, H.pack_rows(s1, bu.cuda(), br.cuda()),
                               aux0=h32, out=u, out2=None, out_h16=rh16, out_fmt=H.FMT_F32_C8, aux_fmt=H.FMT_F32_C8)
            torch.cuda.synchronize()
        ug = unblock32(u.float(), hid)
        assert not torch.isnan(ug).any()
        utol = 2 ** -11 * u_ref if uact == H.GRU_U_F16 else 2 ** -22 * u_ref
        assert ((ug - u_ref).abs() - utol).max().item() < 2e-6, (uact, (ug - u_ref).abs().max().item())
        if sat and uact == H.GRU_U_F32:
            # z is the bias itself here (zero weights): relative to fp64 sigma, v_exp_f32 and v_rcp_f32 give ~1 ulp each and the
            # scaling of z by log2(e) before the exponential one rounding of |z| 2^-24 in the exponent -- |z| ulp at |z| ~ 20-40, finite
            # and nonzero down to sigma(-40) ~ 4e-18
            zb = bu.double().abs().view(1, -1, 1, 1)
            rel = (ug - u_ref).abs() / u_ref
            assert (ug > 0).all() and (rel <= (4 + zb) * 2 ** -23).all(), rel.max().item()
        if not first:
            rg = unblock(rh16, hid).double()
            assert not torch.isnan(rg).any()
            assert ((rg - rh_ref).abs() - 2 ** -11 * rh_ref.abs()).max().item() < 2e-6
        # GRU_OUT on the operands it reads: the kernel's own u and r * h
        rq = None if first else unblock(rh16, hid).double()
        zo = F.conv2d(xin if first else torch.cat([x_eff, rq], 1), hfr(wo).double(), bo.double(), padding=1)
        hp = 0.0 if first else h.double()
        hn_ref = hp * (1 - ug) + ug * torch.tanh(zo)
        for hilo in (False, True):
            s2 = H.conv_spec(N, Hh, W, 2 * C, C1, hid, 3, 1, 1, epi=H.EPI_GRU_OUT, act=uact | (H.GRU_H_HILO if hilo else 0), hidden=hid,
                             compute=H.COMPUTE_F16)
            if hilo and hid % s2.plan.cout_tile:
                continue  # (the product falls back to one half copy there)
            nb = H.f32_c8_empty(N, hid, Hh, W, 'cuda').fill_(NAN)
            new16 = H.f16_blocks_empty(N, hid, Hh, W, 'cuda', hilo=hilo).fill_(NAN)
            with Wide(H, wide):
                H.conv_forward_h16(s2, xh, rh16, packed_weight(s2, dup(wo).cuda()), None, H.pack_rows(s2, bo.cuda()), aux0=h32, aux1=u,
                                   out=nb, out_h16=new16, out_fmt=H.FMT_F32_C8, aux_fmt=H.FMT_F32_C8)
                torch.cuda.synchronize()
            hg = unblock32(nb, hid)
            assert not torch.isnan(hg).any() and (hg - hn_ref).abs().max().item() < 3e-5, (uact, hilo, (hg - hn_ref).abs().max().item())
            if hilo:
                gp = unblock_hilo(new16, hid)
                assert not torch.isnan(gp).any() and (gp - hn_ref).abs().max().item() < 3e-5
            else:
                gq = unblock(new16, hid).double()
                assert not torch.isnan(gq).any() and ((gq - hn_ref).abs() - 2 ** -11 * hn_ref.abs()).max().item() < 3e-5


# ---------------------------------------------------------------------------------------------------------------- norm statistics
# (_channels, _check_stats and _bwd_check live in tests/norm_ref.py, shared with tests/test_hip_norm_edges.py)
NORM_SHAPES = [
    # N, C, H, W
    (2, 20, 60, 80),      # fused single-plane kernels (4800 pixels), C % 8 != 0
    (1, 12, 64, 80),      # 5120 pixels: the last plane the fused kernels take
    (1, 16, 240, 320),    # split reduce / apply
    (1, 12, 480, 640),    # split, the full-resolution plane, C % 8 != 0
]


@pytest.mark.parametrize('x_fmt', [1, 2])
@pytest.mark.parametrize('shape', NORM_SHAPES)
def test_instance_norm_mixed_statistics(H, shape, x_fmt):
    """ess_instnorm_forward_c8_mixed on an F16_C8 (x_fmt 1) and a [hi | lo] (x_fmt 2) pre-norm tensor with the decoder's channel means
    (0 - 30 sigma): mean and rstd against fp64 over the stored values (hi + lo for a pair); y16 within its half rounding of the fp64
    map plus what the fp32 statistics carry (a mean off by dm moves every output by dm rstd); the backward (reading the hi parts of a
    pair) within the bf16 rounding of dx computed in fp64 from the forward's own statistics."""
    N, C, Hh, W = shape
    g = torch.Generator().manual_seed(N * C + Hh + x_fmt)
    x = _channels(N, C, Hh, W, g)
    xs = H.to_f16_c8(x.cuda(), hilo=x_fmt == 2)
    xv = unblock_hilo(xs, C) if x_fmt == 2 else unblock(xs, C).double()
    y, y16, stats = H.instnorm_forward_c8_mixed(xs, C, None, False, 1e-5, x_fmt)
    torch.cuda.synchronize()
    _check_stats(stats, xv, (2, 3), 1e-5, ('IN mixed', shape, x_fmt))
    mr = xv.mean((2, 3), keepdim=True)
    rs = 1.0 / torch.sqrt(((xv - mr) ** 2).mean((2, 3), keepdim=True) + 1e-5)
    ref = (xv - mr) * rs
    slack = (2 ** -20 * xv.abs().mean((2, 3), keepdim=True) + 1e-7) * rs + 1e-5 * ref.abs() + 1e-6
    g16 = unblock(y16, C).double()
    assert ((g16 - ref).abs() - 2 ** -11 * ref.abs() - slack).max().item() <= 0, (g16 - ref).abs().max().item()
    g8 = H.from_bf16_c8(y, C).cpu().double()
    assert ((g8 - ref).abs() - 2 ** -8 * ref.abs() - slack).max().item() <= 0
    # backward on the values it reads, with the forward's statistics
    dy = torch.randn(N, C, Hh, W, generator=g)
    dy8 = H.to_bf16_c8(dy.cuda())
    dx = H.instnorm_backward_c8(xs, C, dy8, stats, False, x_f16=x_fmt)
    torch.cuda.synchronize()
    xr = unblock(xs[:, :xs.shape[1] // 2], C).double() if x_fmt == 2 else xv
    _bwd_check(H.from_bf16_c8(dx, C).cpu().double(), xr, dy.to(torch.bfloat16).double(), stats, (2, 3), ('IN mixed bwd', shape, x_fmt))


IN_STAT_CASES = [((2, 20, 60, 80), 256), ((2, 20, 60, 80), 512), ((2, 20, 60, 80), 1024),  # fused, each in_small_threads value
                 ((4, 256, 72, 72), 512),    # the 1024-thread fused kernel (256 groups of 5184 pixels)
                 ((1, 12, 480, 640), 512)]   # split reduce / apply


@pytest.mark.parametrize('x_f16', [False, True])
@pytest.mark.parametrize('shape,threads', IN_STAT_CASES)
def test_instance_norm_c8_statistics(H, shape, threads, x_f16):
    """ess_instnorm_forward_c8 / backward on a BF16_C8 or an F16_C8 x at the decoder's channel means: every fused thread count
    (in_small_threads; planes <= 5120 pixels), the 1024-thread fused kernel (256 groups of 5184 pixels) and the split path.  Statistics
    as above; y within its bf16 rounding."""
    N, C, Hh, W = shape
    g = torch.Generator().manual_seed(C + Hh + int(x_f16))
    x = _channels(N, C, Hh, W, g)
    if x_f16:
        xs = H.to_f16_c8(x.cuda()).view(torch.bfloat16)
        xv = unblock(xs.view(torch.float16), C).double()
    else:
        xs = H.to_bf16_c8(x.cuda())
        xv = H.from_bf16_c8(xs, C).cpu().double()
    prev = H.tuning_get('in_small_threads')
    try:
        H.tuning_set('in_small_threads', threads)
        y, stats = H.instnorm_forward_c8(xs, C, None, False, x_f16=x_f16)
        dy = torch.randn(N, C, Hh, W, generator=g)
        dx = H.instnorm_backward_c8(xs, C, H.to_bf16_c8(dy.cuda()), stats, False, x_f16=x_f16)
        torch.cuda.synchronize()
    finally:
        H.tuning_set('in_small_threads', prev)
    _check_stats(stats, xv, (2, 3), 1e-5, ('IN', shape, x_f16, threads))
    mr = xv.mean((2, 3), keepdim=True)
    rs = 1.0 / torch.sqrt(((xv - mr) ** 2).mean((2, 3), keepdim=True) + 1e-5)
    ref = (xv - mr) * rs
    slack = (2 ** -20 * xv.abs().mean((2, 3), keepdim=True) + 1e-7) * rs + 1e-5 * ref.abs() + 1e-6
    g8 = H.from_bf16_c8(y, C).cpu().double()
    assert ((g8 - ref).abs() - 2 ** -8 * ref.abs() - slack).max().item() <= 0
    _bwd_check(H.from_bf16_c8(dx, C).cpu().double(), xv, dy.to(torch.bfloat16).double(), stats, (2, 3), ('IN bwd', shape, x_f16))


@pytest.mark.parametrize('x_f16', [False, True])
@pytest.mark.parametrize('shape', [(4, 20, 60, 80), (4, 12, 480, 640)])
def test_batch_norm_c8_statistics(H, shape, x_f16):
    """train-mode BatchNorm (split path, reduction over N x H x W: 1.2 M pixels per channel at 4 x 480 x 640) on a BF16_C8 or F16_C8 x
    at 0 - 30 sigma channel means: mean / rstd against fp64 (stats[0]), the saved affine map, y within bf16 rounding, and the backward"""
    N, C, Hh, W = shape
    g = torch.Generator().manual_seed(N + C + int(x_f16))
    x = _channels(N, C, Hh, W, g)
    if x_f16:
        xs = H.to_f16_c8(x.cuda()).view(torch.bfloat16)
        xv = unblock(xs.view(torch.float16), C).double()
    else:
        xs = H.to_bf16_c8(x.cuda())
        xv = H.from_bf16_c8(xs, C).cpu().double()
    gam = torch.rand(C, generator=g) + 0.5
    bet = torch.randn(C, generator=g)
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    y, st = H.batchnorm_train_forward_c8(xs, C, None, gam.cuda(), bet.cuda(), rm, rv, 0.1, 1e-5, False, x_f16=x_f16)
    dy = torch.randn(N, C, Hh, W, generator=g)
    dg, db = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
    dx, _ = H.batchnorm_train_backward_c8(xs, C, y, H.to_bf16_c8(dy.cuda()), gam.cuda(), st, False, True, False, dg, db, x_f16=x_f16)
    torch.cuda.synchronize()
    stats = st[0]
    _check_stats(stats, xv, (0, 2, 3), 1e-5, ('BN', shape, x_f16))
    mr = xv.mean((0, 2, 3), keepdim=True)
    var = ((xv - mr) ** 2).mean((0, 2, 3))
    rs = (1.0 / torch.sqrt(var + 1e-5)).view(1, C, 1, 1)
    ref = (xv - mr) * rs * gam.double().view(1, C, 1, 1) + bet.double().view(1, C, 1, 1)
    slack = ((2 ** -20 * xv.abs().mean((0, 2, 3), keepdim=True) + 1e-7) * rs + 1e-5 * (xv - mr).abs() * rs) * gam.double().view(1, C, 1, 1) + 1e-6
    g8 = H.from_bf16_c8(y, C).cpu().double()
    assert ((g8 - ref).abs() - 2 ** -8 * ref.abs() - slack).max().item() <= 0, (g8 - ref).abs().max().item()
    n = N * Hh * W
    assert (rv.cpu().double() - (0.9 + 0.1 * var * n / (n - 1))).abs().max().item() < 1e-5 * (1 + var.max().item())
    _bwd_check(H.from_bf16_c8(dx, C).cpu().double(), xv, dy.to(torch.bfloat16).double(), stats, (0, 2, 3), ('BN bwd', shape, x_f16), gamma=gam)
