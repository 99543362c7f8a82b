"""Shared by tests/test_hip_dgrad_edges.py (GPU tier) and tests/test_host_dgrad_check.py (CPU tier): a row of the data gradient's
form-by-edge table, its seeded inputs, the float64 reference of one data-gradient launch, the elementwise bound every comparison uses,
the restated dispatcher (which kernel, tile and epilogue a launch takes) and the BF16_C8 unblock helpers.  A plain helper module: no
fixtures, no collection hooks."""
import functools
import math

import torch
import torch.nn.functional as F

NAN = float('nan')

F32, BF16, F16 = 0, 1, 3     # ESS_COMPUTE_FP32 / BF16 / F16
NCHW, C8 = 0, 1              # ESS_FMT_F32_NCHW / ESS_FMT_BF16_C8
DIRECT, NEAREST_UP2, ZERO_UP2 = 0, 1, 2
ACT_NONE, ACT_SUMPOOL2 = 0, 4
W_TRANSPOSED = 1

# |d| per element, relative to max|ref| of the output tensor: fp32 accumulation of bf16-exact products in another order
# (wgrad_ref.TOL['bf16'], test_conv_f16_edges) / unrounded fp32 operands on the exact-fp32 kernels (wgrad_ref.TOL['fp32'])
ACC_TOL = {'c8': 2e-5, 'nchw_bf16': 2e-5, 'nchw_f32': 5e-5}


class Case:
    """One row of DGRAD_EDGE_CASES (tests/test_hip_dgrad_edges.py) by name.  The row is written as the FORWARD convolution it is the
    gradient of ((C0 [+ C1]) -> Cout over Hv x Wv, k / s / p, first source nearest-upsampled if m0); the data-gradient launch follows
    from it exactly as in Conv2dFn.backward."""

    def __init__(self, row):
        (self.id, self.compute, self.dyfmt, self.outfmt, self.N, self.C0, self.C1, self.Cout, self.Hv, self.Wv, self.k, self.s, self.p,
         self.m0, self.skip, self.wide, self.label) = row
        self.row = row
        self.Cin = self.C0 + self.C1
        self.Ho = (self.Hv + 2 * self.p - self.k) // self.s + 1
        self.Wo = (self.Wv + 2 * self.p - self.k) // self.s + 1
        self.pool = self.s == 1 and self.m0 == NEAREST_UP2
        self.split = self.C0 if self.C1 else 0
        # the data-gradient launch: a stride-1 convolution of dy (zero-inserted for s == 2) with the flipped, transposed weights
        self.d_Hin, self.d_Win = (self.Ho, self.Wo) if self.s == 1 else (2 * self.Ho, 2 * self.Wo)
        self.d_mode0 = DIRECT if self.s == 1 else ZERO_UP2
        self.d_pad = self.k - 1 - self.p
        self.d_act = ACT_SUMPOOL2 if self.pool else ACT_NONE
        self.kind = 'c8' if self.outfmt == C8 else ('nchw_f32' if self.compute == F32 else 'nchw_bf16')
        self.c_first = self.split or self.Cin
        self.shape0 = (self.N, self.c_first, self.Hv // 2 if self.pool else self.Hv, self.Wv // 2 if self.pool else self.Wv)
        self.shape1 = (self.N, self.C1, self.Hv, self.Wv) if self.C1 else None

    def spec_args(self):
        """positional and keyword arguments of hip.conv_spec for the data-gradient launch (Conv2dFn.backward)"""
        return ((self.N, self.d_Hin, self.d_Win, self.Cout, 0, self.Cin, self.k, 1, self.d_pad),
                dict(mode0=self.d_mode0, out_split=self.split, act=self.d_act, compute=self.compute))

    def cropped(self, Hv, Wv):
        """the same row (same id, hence same seed) on a smaller extent: the CPU tier's teeth for a row that is large in pixels"""
        r = list(self.row)
        r[8], r[9] = Hv, Wv
        return Case(tuple(r))


def bfr(x):
    """round to bf16 (nearest even, as cvt8 and ess_to_bf16_c8 do) and back"""
    return x.bfloat16().float()


def zero_up(x):
    z = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
    z[:, :, ::2, ::2] = x
    return z


def case_inputs(case):
    """The case's seeded (dy, w, r) as they are handed to the library: fp32 CPU tensors, already bf16 values where the tensor is stored
    as BF16_C8.  w is the forward convolution's weight [Cout][C0 + C1][k][k]; r (the skip gradient, None without `skip`) has the first
    output's shape and format."""
    c = case
    g = torch.Generator().manual_seed(sum(map(ord, c.id)))
    dy = torch.randn(c.N, c.Cout, c.Ho, c.Wo, generator=g)
    w = torch.randn(c.Cout, c.Cin, c.k, c.k, generator=g) / (c.k * math.sqrt(c.Cin))
    r = torch.randn(c.shape0, generator=g) if c.skip else None
    if c.dyfmt == C8:
        dy = bfr(dy)
    if r is not None and c.outfmt == C8:
        r = bfr(r)
    return dy, w, r


def kernel_operands(case, dy, w):
    """The values the kernel contracts: the bf16 kernels read bf16 weights (the pack rounds them) and round an fp32 NCHW dy while they
    stage it (a BF16_C8 dy holds bf16 values already); ESS_COMPUTE_FP32 sees every bit of both."""
    if case.compute == F32:
        return dy, w
    return bfr(dy), bfr(w)


def _outputs(case, g, r):
    """(first, second) outputs of the launch from the gradient g over the virtual input: split, 2x2 sum and skip as the row says"""
    c = case
    first = g[:, :c.C0] if c.C1 else g
    if c.pool:
        first = 4 * F.avg_pool2d(first, 2)
    if r is not None:
        first = first + r.to(g.dtype)
    return first, (g[:, c.C0:] if c.C1 else None)


def dgrad_reference(case, dy_op, w_op, r):
    """(first, second) in float64 on the CPU: autograd of F.conv2d over the virtual input, at the operands the kernel reads"""
    c = case
    xv = torch.zeros(c.N, c.Cin, c.Hv, c.Wv, dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(F.conv2d(xv, w_op.double(), None, c.s, c.p), xv, dy_op.double())
    return _outputs(c, g, r)


def dgrad_fp32_standin(case, src, w_op, r):
    """What a correct kernel is allowed to be (the CPU tier's stand-in for one), computed the way the kernel computes it: an fp32
    stride-1 convolution of the launch's virtual source `src` (dy, or dy zero-inserted) with the flipped, transposed weights; pooled,
    split and skip-added in fp32; rounded to bf16 where the output is 16-bit."""
    c = case
    g = F.conv2d(src.float(), w_op.float().transpose(0, 1).flip(2, 3).contiguous(), None, 1, c.d_pad)
    first, second = _outputs(c, g, r)
    if c.outfmt == C8:
        first, second = bfr(first), None if second is None else bfr(second)
    return first, second


def virtual_source(case, dy_op):
    return dy_op if case.s == 1 else zero_up(dy_op)


@functools.lru_cache(maxsize=None)
def case_reference(row):
    """(case, (dy, w, r), (first, second) float64) of a table row, computed once per process and shared by the tests that need it: do
    not write into what it returns."""
    case = Case(row)
    dy, w, r = case_inputs(case)
    return case, (dy, w, r), dgrad_reference(case, *kernel_operands(case, dy, w), r)


def bound(ref, kind):
    """elementwise bound on |got - ref|.  16-bit output: a stored value is rn_bf16(ref + d), so |got - ref| <= 2^-8 |ref| +
    (1 + 2^-8) |d|; fp32 output: |d|.  |d| <= ACC_TOL[kind] * max|ref of that tensor|."""
    ref = ref.double()
    d = ACC_TOL[kind] * ref.abs().max()
    if kind == 'c8':
        return 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * d
    return torch.full_like(ref, d.item())


def excess(got, ref, kind):
    """the largest elementwise |got - ref| / bound"""
    got, ref = got.detach().double().cpu(), ref.double()
    return ((got - ref).abs() / bound(ref, kind)).max().item()


def check(got, ref, kind, what=''):
    """No element is NaN (an element a kernel left unwritten in a poisoned output), then every element within the bound."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f'{what}: {nan} of {got.numel()} elements are NaN'
    e = excess(got, ref, kind)
    assert e <= 1.0, f'{what}: |got - ref| reaches {e:.3g} x the elementwise bound ({kind})'
    return e


# ------------------------------------------------------------------------------------------------ BF16_C8 helpers
def un8(H, y, C):
    """fp32 NCHW values (on the CPU) of the first C channels of a BF16_C8 tensor (tests/test_hip_c8.py)"""
    return H.from_bf16_c8(y, C).cpu()


def tail8(y, C):
    """the channels past C inside the last 8-channel block of a BF16_C8 tensor [N][CB][H][W][8] (empty when C % 8 == 0): the BF16_C8
    contract wants zeros there"""
    return y[:, -1, :, :, C % 8:].float().cpu() if C % 8 else y[:, -1, :, :, :0].float().cpu()


# ------------------------------------------------------------------------------------------------ the dispatcher, restated
def choose_geom(Hout, Wout, k, pooled):
    """choose_geom() of csrc/conv_common.h for a stride-1 launch: (bwl, wxl, TW, TH, tiles_x, tiles_y) of the cheapest pixel tile"""
    kpc = {1: 1, 3: 2, 5: 2, 7: 3}[k]
    best, best_cost = None, 1e300
    for bwl in (5, 4, 3):
        for wxl in (0, 1, 2):
            BW, RB = 1 << bwl, 32 >> bwl
            TW, TH = BW << wxl, (4 >> wxl) * 2 * RB
            tx, ty = -(-Wout // TW), -(-Hout // TH)
            IH, IW = TH - 1 + k, TW - 1 + k
            if IH * IW > kpc * 256:
                continue
            if pooled and Wout >= 32 and bwl != 5:
                continue
            cost = tx * ty * TW * TH * (1.0 + 0.02 * (IH * IW) / (TH * TW) + 0.04 * 64.0 / TW) + 1e-3 * (5 - bwl)
            if cost < best_cost:
                best_cost, best = cost, (bwl, wxl, TW, TH, tx, ty)
    return best


def wide_pick(case, cout_tile, cus):
    """<MBW, CW> of wide_pick() in csrc/conv_bf16.hip for a LINEAR BF16_C8 data-gradient launch with the wide kernel forced (conv_wide =
    2): the cheapest candidate by rounds x tile, in candidate order; None when no form of the wide-tile kernel applies"""
    c = case
    if c.compute != BF16 or c.dyfmt != C8 or c.outfmt != C8 or c.k != 3 or c.pool:
        return None
    if c.split and (c.skip or c.split & 15):
        return None
    mb, best, pick = cout_tile // 32, None, None
    for mbw, cw in ((2, 2), (2, 1), (1, 2), (1, 1)):
        cot = mbw * cw * 32
        if (mb == 2) != (cot >= 64) or mb > 2 or c.Cin % cot or (c.split and c.split % (mbw * 32)):
            continue
        th, tw = (4 // cw) * 5 * 2, 16
        tiles = -(-c.Wv // tw) * -(-c.Hv // th) * (c.Cin // cot) * c.N
        cost = -(-tiles // cus) * cot * th * tw
        if best is None or cost < best:
            best, pick = cost, (mbw, cw)
    return pick


def restated(case, cus=256):
    """What the library does with the row's launch, restated from the dispatcher (which kernel a launch took is not observable):
    dict(kernel, cout_tile, ck, n_cout_tiles, geom, tiles, epilogue, persistent) and the label 'kernel/epilogue[/persistent]'.
      plan: pick_mb / pick_ck / make_plan (conv_common.h); kernel: conv_bf16_launch, wide_pick (conv_bf16.hip), conv_fwd.hip for fp32;
      epilogue: conv_epilogue / conv_epilogue_c8_sel / conv_epilogue_c8_wide_sel (conv_common.h)."""
    c = case
    rows, K = c.Cin, c.Cout          # the launch's output channels (packed rows) and contraction channels
    bf = c.compute == BF16
    mb = 4 if (bf and c.k == 3 and rows >= 256 and K >= 512) else (2 if rows > 32 else 1)
    cot = 32 * mb
    ck = ((32 if (c.k == 1 and K >= 32) else 16) if bf else {1: 8, 3: 8, 5: 4, 7: 2}[c.k])
    nct = -(-rows // cot)
    geom = choose_geom(c.Hv, c.Wv, c.k, c.pool)
    bwl, _, _, _, tx, ty = geom
    tiles = tx * ty * nct * c.N
    wp = wide_pick(c, cot, cus) if c.wide == 2 else None
    persistent = False
    if not bf:
        kernel = f'f32<{mb}>'
    elif c.k == 3 and wp:
        kernel = f'wide<{wp[0]},{wp[1]}>'
    elif c.k == 3:
        kernel = f'ws<{mb}>'
        persistent = tiles > cus * (1 if mb == 4 else 2)  # (two stages of LDS allow at least two workgroups per CU at ck = 16, mb <= 2)
    else:
        kernel = f'generic<{c.k},1,{mb},ck{ck}>'
    whole = rows % cot == 0
    if c.outfmt == NCHW:
        epi = ('pool<rows1>' if bwl == 5 else 'pool<lanes>') if c.pool else ('rows<split>' if c.split else ('rows<res>' if c.skip else 'plain'))
        epi = 'nchw_' + epi
    elif kernel.startswith('wide'):
        epi = 'dgrad<split>' if c.split else ('plain<res>' if c.skip else 'plain')
    elif (c.pool or c.split) and not c.skip and not (c.split & 15) and whole and (not c.pool or bwl == 5):
        epi = 'dgrad<pool>' if c.pool else 'dgrad<split>'
    elif not c.split and not c.pool and whole:
        epi = 'plain<res>' if c.skip else 'plain'
    else:
        epi = 'general' + ('<rows1>' if c.pool and bwl == 5 else '<lanes>' if c.pool else '')
    label = f'{kernel}/{epi}' + ('/persistent' if persistent else '')
    return dict(kernel=kernel, cout_tile=cot, ck=ck, n_cout_tiles=nct, geom=geom, tiles=tiles, epilogue=epi, persistent=persistent, label=label)
