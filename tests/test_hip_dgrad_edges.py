"""GPU tier: every form in which Conv2dFn.backward runs the forward convolution kernels as a DATA gradient -- flipped, transposed weight
packs (ESS_W_TRANSPOSED), zero-inserted sources (ESS_SRC_ZERO_UP2: the gradient of a stride-2 convolution), two outputs (out_split:
a concat convolution), the pooled epilogue (ESS_ACT_SUMPOOL2: a nearest-upsampled first source) in its three implementations, the
fused skip gradient (`residual`) and the head's fp32 NCHW logit gradient written to a BF16_C8 tensor -- elementwise against a float64
torch-CPU autograd gradient of the operands the kernel reads (tests/dgrad_ref.py), at the smallest shapes at which each edge exists:
partial tiles, odd stored extents, ragged channel blocks, splits that are no multiple of 16, pooled launches narrower than 32 columns.
Every output starts as NaN (bf16 0x7fc0 / fp32 NaN): an element a kernel leaves unwritten fails the comparison.
tests/test_host_dgrad_check.py proves on the CPU that the bound notices one dropped pixel (and one hole read as data) in every row and
checks every row's label against the planner."""
import pytest
import torch

from dgrad_ref import (BF16, C8, F16, F32, NAN, NCHW, NEAREST_UP2, W_TRANSPOSED, Case, bound, case_inputs, case_reference, check,
                       dgrad_reference, kernel_operands, restated, tail8, un8)

pytestmark = pytest.mark.gpu

# id, compute, dy fmt, out fmt, N, C0, C1, Cout, Hv, Wv, k, s, p, m0, skip, wide, label
# A row is named by the FORWARD convolution it is the gradient of: (C0 [+ C1]) -> Cout channels over Hv x Wv (m0 = 1: the first source
# nearest-upsampled); the launch contracts Cout channels of dy into C0 + C1 output rows.  `label` restates the dispatcher for that launch
# (dgrad_ref.restated: kernel<channel blocks of the tile>/epilogue[/persistent]); which kernel a launch took is not observable, so the
# CPU tier keeps every label true to the planner and every case asserts the plan fields its label states.
#   epilogues of a BF16_C8 output (conv_epilogue_c8_sel): plain / plain<res> = conv_epilogue_c8_plain, dgrad<split> / dgrad<pool> =
#   conv_epilogue_c8_dgrad<MB, POOL>, general = conv_epilogue_c8_impl (<rows1>: pooled with 32-wide pixel blocks, the vertical partner in
#   the wave's other pixel block; <lanes>: narrower blocks, the partner in lane ^ BW); of an fp32 NCHW output: nchw_*.
DGRAD_EDGE_CASES = [
    # direct, wave-specialised kernel
    ('k3_rows20_k40_odd', BF16, C8, C8, 1, 20, 0, 40, 17, 30, 3, 1, 1, 0, False, 0, 'ws<1>/general'),
    ('k3_skip_plain_odd', BF16, C8, C8, 2, 64, 0, 64, 13, 21, 3, 1, 1, 0, True, 0, 'ws<2>/plain<res>'),
    ('k3_skip_ragged', BF16, C8, C8, 1, 72, 0, 40, 9, 19, 3, 1, 1, 0, True, 0, 'ws<2>/general'),
    ('k3_mb4_skip', BF16, C8, C8, 1, 256, 0, 512, 7, 13, 3, 1, 1, 0, True, 0, 'ws<4>/plain<res>'),
    ('k3_mb4_ragged', BF16, C8, C8, 1, 320, 0, 512, 7, 13, 3, 1, 1, 0, False, 0, 'ws<4>/general'),
    # concat: two outputs
    ('split_straight', BF16, C8, C8, 2, 64, 64, 32, 11, 19, 3, 1, 1, 0, False, 0, 'ws<2>/dgrad<split>'),
    ('split_rows96', BF16, C8, C8, 2, 64, 32, 64, 13, 21, 3, 1, 1, 0, False, 0, 'ws<2>/general'),
    ('split_24', BF16, C8, C8, 1, 24, 40, 32, 9, 17, 3, 1, 1, 0, False, 0, 'ws<2>/general'),
    ('wide_split', BF16, C8, C8, 2, 64, 64, 64, 13, 21, 3, 1, 1, 0, False, 2, 'wide<1,2>/dgrad<split>'),
    ('wide_skip', BF16, C8, C8, 2, 64, 0, 64, 13, 21, 3, 1, 1, 0, True, 2, 'wide<1,2>/plain<res>'),
    # pooled (the first source nearest-upsampled; Hv, Wv even)
    ('pool_w30', BF16, C8, C8, 1, 64, 0, 32, 18, 30, 3, 1, 1, 1, False, 0, 'ws<2>/dgrad<pool>'),
    ('pool_w14_lanes', BF16, C8, C8, 1, 64, 0, 32, 18, 14, 3, 1, 1, 1, False, 0, 'ws<2>/general<lanes>'),
    ('pool_w32_straight', BF16, C8, C8, 2, 64, 0, 32, 10, 32, 3, 1, 1, 1, False, 0, 'ws<2>/dgrad<pool>'),
    ('pool_w34_partial', BF16, C8, C8, 1, 64, 0, 32, 14, 34, 3, 1, 1, 1, False, 0, 'ws<2>/dgrad<pool>'),
    ('pool_w34_rows24', BF16, C8, C8, 1, 24, 0, 40, 14, 34, 3, 1, 1, 1, False, 0, 'ws<1>/general<rows1>'),
    ('pool_split_straight', BF16, C8, C8, 1, 64, 64, 32, 12, 36, 3, 1, 1, 1, False, 0, 'ws<2>/dgrad<pool>'),
    ('pool_split_24', BF16, C8, C8, 1, 24, 40, 32, 12, 36, 3, 1, 1, 1, False, 0, 'ws<2>/general<rows1>'),
    ('pool_persistent', BF16, C8, C8, 1, 16, 0, 16, 386, 386, 3, 1, 1, 1, False, 0, 'ws<1>/general<rows1>/persistent'),
    # stride 2: zero-inserted dy
    ('k3s2_dy_9x17', BF16, C8, C8, 2, 64, 0, 128, 18, 34, 3, 2, 1, 0, False, 0, 'ws<2>/plain'),
    ('k3s2_ragged', BF16, C8, C8, 1, 24, 0, 40, 10, 12, 3, 2, 1, 0, False, 0, 'ws<1>/general'),
    ('k1s2_ck32', BF16, C8, C8, 2, 64, 0, 128, 18, 26, 1, 2, 0, 0, False, 0, 'generic<1,1,2,ck32>/plain'),
    ('k1s2_ck16_ragged', BF16, C8, C8, 1, 40, 0, 24, 10, 14, 1, 2, 0, 0, False, 0, 'generic<1,1,2,ck16>/general'),
    # head: dy as fp32 NCHW logits' gradient, rounded while staged
    ('head11_odd', BF16, NCHW, C8, 2, 32, 0, 11, 9, 15, 1, 1, 0, 0, False, 0, 'generic<1,1,1,ck16>/plain'),
    ('head6_35px', BF16, NCHW, C8, 1, 20, 0, 6, 5, 7, 1, 1, 0, 0, False, 0, 'generic<1,1,1,ck16>/general'),
    # fp32 NCHW in and out (the form test_conv_c8_forms trusts as its reference), on the bf16 kernels and on the exact-fp32 kernel
    ('nchw_pool_w30_bf16', BF16, NCHW, NCHW, 1, 32, 0, 32, 18, 30, 3, 1, 1, 1, False, 0, 'ws<1>/nchw_pool<rows1>'),
    ('nchw_pool_w30_f32', F32, NCHW, NCHW, 1, 32, 0, 32, 18, 30, 3, 1, 1, 1, False, 0, 'f32<1>/nchw_pool<rows1>'),
    ('nchw_pool_w14_bf16', BF16, NCHW, NCHW, 1, 32, 0, 32, 18, 14, 3, 1, 1, 1, False, 0, 'ws<1>/nchw_pool<lanes>'),
    ('nchw_pool_w14_f32', F32, NCHW, NCHW, 1, 32, 0, 32, 18, 14, 3, 1, 1, 1, False, 0, 'f32<1>/nchw_pool<lanes>'),
    ('nchw_pool_split_w34_bf16', BF16, NCHW, NCHW, 1, 32, 24, 32, 14, 34, 3, 1, 1, 1, False, 0, 'ws<2>/nchw_pool<rows1>'),
    ('nchw_pool_split_w34_f32', F32, NCHW, NCHW, 1, 32, 24, 32, 14, 34, 3, 1, 1, 1, False, 0, 'f32<2>/nchw_pool<rows1>'),
    ('nchw_k3s2_odd_bf16', BF16, NCHW, NCHW, 1, 24, 0, 40, 18, 34, 3, 2, 1, 0, False, 0, 'ws<1>/nchw_plain'),
    ('nchw_k3s2_odd_f32', F32, NCHW, NCHW, 1, 24, 0, 40, 18, 34, 3, 2, 1, 0, False, 0, 'f32<1>/nchw_plain'),
    # ... and the fp32 configuration's remaining forms: an unpooled split anywhere (24 is no multiple of 16), the fused skip, 1x1 / s2
    ('nchw_split_odd_bf16', BF16, NCHW, NCHW, 1, 24, 20, 32, 13, 21, 3, 1, 1, 0, False, 0, 'ws<2>/nchw_rows<split>'),
    ('nchw_split_odd_f32', F32, NCHW, NCHW, 1, 24, 20, 32, 13, 21, 3, 1, 1, 0, False, 0, 'f32<2>/nchw_rows<split>'),
    ('nchw_skip_odd_bf16', BF16, NCHW, NCHW, 1, 40, 0, 24, 9, 19, 3, 1, 1, 0, True, 0, 'ws<2>/nchw_rows<res>'),
    ('nchw_skip_odd_f32', F32, NCHW, NCHW, 1, 40, 0, 24, 9, 19, 3, 1, 1, 0, True, 0, 'f32<2>/nchw_rows<res>'),
    ('nchw_k1s2_bf16', BF16, NCHW, NCHW, 1, 40, 0, 24, 10, 14, 1, 2, 0, 0, False, 0, 'generic<1,1,2,ck16>/nchw_plain'),
    ('nchw_k1s2_f32', F32, NCHW, NCHW, 1, 40, 0, 24, 10, 14, 1, 2, 0, 0, False, 0, 'f32<2>/nchw_plain'),
]
CASE_IDS = [c[0] for c in DGRAD_EDGE_CASES]
# pool_w30 / nchw_pool_w30: choose_geom keeps 32-wide pixel blocks for every output 26 - 32 columns wide (a 16- or 8-wide block pads the
# same 32 columns and loses the coalescing term), so a pooled launch meets the lane ^ BW pairing only from 16 columns down: the *_w14
# rows reach it (16-wide blocks, 14 real columns) and the *_w30 rows stay as the partial 32-wide block they are.
# pool_w34_*: from 32 columns on a pooled launch takes 32-wide blocks; at 14 x 34 the cheapest tile is 64 x 4 (two 32-wide blocks side
# by side), so the 2 real pixels -- one pooled column -- sit in the tile's second 32-wide block column (the CPU tier prints every row's tile).
# Not reached by these cases:
#   * the generic tile kernel's 3x3 / stride-1 form (conv_bf16_generic.hip:85 for a zero-inserted source): a 3x3 / stride-1 launch
#     reaches it only with ESS_CONV_WS=0, an environment switch read once per process;
#   * the 5x5 tap-paired data gradient: no trainable 5x5 convolution exists (the 5x5 layers belong to the frozen encoder), and the fp32
#     form of a transposed 5x5 pack has tests/test_hip_kernels.py::test_conv_backward;
#   * every data-gradient form under ESS_COMPUTE_F16: validate() refuses them (tests/test_host_dgrad_check.py::test_refusals).


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


class Wide:
    """tuning switch conv_wide for the duration of a block (tests/test_hip_mixed_edges.py): 0 = the wave-specialised kernels only, 2 =
    the wide-tile kernel wherever one of its forms applies"""

    def __init__(self, H, mode):
        self.H, self.mode = H, mode

    def __enter__(self):
        self.prev = self.H.tuning_get('conv_wide')
        self.H.tuning_set('conv_wide', self.mode)

    def __exit__(self, *a):
        self.H.tuning_set('conv_wide', self.prev)


def _put(H, t, fmt):
    if t is None:
        return None
    return H.to_bf16_c8(t.cuda()) if fmt == C8 else t.cuda()


def _poisoned(H, shape, fmt):
    if shape is None:
        return None
    N, C, Hh, W = shape
    if fmt == C8:
        t = H.bf16_c8_empty(N, C, Hh, W, 'cuda').fill_(NAN)
        assert int(t.view(torch.int16)[0, 0, 0, 0, 0]) == 0x7fc0
        return t
    return torch.full(shape, NAN, device='cuda')


@pytest.mark.parametrize('row', DGRAD_EDGE_CASES, ids=CASE_IDS)
def test_dgrad_form_edges(H, row):
    """One row: the launch Conv2dFn.backward issues for it (ESS_W_TRANSPOSED pack of the forward weight, dy as the only source, the
    skip gradient as `residual`) onto NaN outputs, both outputs elementwise within dgrad_ref.bound of the float64 gradient, zeros in the
    channels past C of a partial last BF16_C8 block, and the plan fields the label states."""
    c, (dy, w, r), (ref0, ref1) = case_reference(row)
    assert (H.COMPUTE_FP32, H.COMPUTE_BF16, H.COMPUTE_F16) == (F32, BF16, F16) and (H.FMT_F32_NCHW, H.FMT_BF16_C8) == (NCHW, C8)
    assert (H.SRC_NEAREST_UP2, H.W_TRANSPOSED) == (NEAREST_UP2, W_TRANSPOSED)
    args, kw = c.spec_args()
    spec = H.conv_spec(*args, **kw)
    assert (spec.H_out, spec.W_out) == (c.Hv, c.Wv)
    # the label: these plan fields, this epilogue selection
    want = restated(c, H.tuning_get('device_cus'))
    assert want['label'] == c.label, (c.id, want['label'])
    assert (spec.plan.cout_tile, spec.plan.ck, spec.plan.n_cout_tiles) == (want['cout_tile'], want['ck'], want['n_cout_tiles']), c.id
    if c.id == 'pool_persistent':
        assert want['tiles'] > 2 * H.tuning_get('device_cus'), want['tiles']  # (several tiles per resident workgroup)
    pw = H.pack_weights(spec, w.cuda(), kind=H.W_TRANSPOSED)
    out, out2 = _poisoned(H, c.shape0, c.outfmt), _poisoned(H, c.shape1, c.outfmt)
    with Wide(H, c.wide):
        H.conv_forward(spec, _put(H, dy, c.dyfmt), None, pw, residual=_put(H, r, c.outfmt), out=out, out2=out2,
                       src_fmt=H.FMT_BF16_C8 if c.dyfmt == C8 else H.FMT_F32_NCHW, out_fmt=H.FMT_BF16_C8 if c.outfmt == C8 else H.FMT_F32_NCHW)
        torch.cuda.synchronize()
    for name, t, ref, C in (('first', out, ref0, c.c_first), ('second', out2, ref1, c.C1)):
        if t is None:
            continue
        got = un8(H, t, C) if c.outfmt == C8 else t.cpu()
        e = check(got, ref, c.kind, f'{c.id} {name} output')
        print(f'{c.id} {name}: at {e:.3f} of the bound')
        if c.outfmt == C8:
            tail = tail8(t, C)
            assert (tail == 0).all(), (c.id, name, 'channels past C in the last block', int((tail != 0).sum()) + int(torch.isnan(tail).sum()))
    if c.compute == BF16:  # the re-pack after an optimiser step goes through the multi-tensor kernel: the same bytes
        pm = torch.full_like(pw, 0xFF)
        H.pack_weights_multi([(spec, H.W_TRANSPOSED, w.cuda(), pm)])
        torch.cuda.synchronize()
        assert torch.equal(pm, pw), (c.id, 'pack_weights_multi != pack_weights (ESS_W_TRANSPOSED)')


# ------------------------------------------------------------------------------------------------ Conv2dFn.backward at the same edges
def _leaf(H, t):
    return H.to_bf16_c8(t.cuda()).requires_grad_(True)


def _fn_case(cid, N, C0, C1, Cout, Hv, Wv, k, s, p, m0, skip):
    """an ad-hoc row for the function-level cases: (case, (dy, w, r), float64 reference)"""
    c = Case((cid, BF16, C8, C8, N, C0, C1, Cout, Hv, Wv, k, s, p, m0, skip, 0, ''))
    dy, w, r = case_inputs(c)
    return c, (dy, w, r), dgrad_reference(c, *kernel_operands(c, dy, w), r)


def test_conv2dfn_backward_dgrad_edges(H):
    """Conv2dFn.backward on BF16_C8 leaves in the bf16 configuration, d0 / d1 against the float64 reference with the rows' bound: the
    pooled + split launch (both sources requiring grad), the first source's filters alone (columns(weight, [(0, C0)])) when the skip is
    detached, the fused skip gradient of conv2d_passthrough, and the sum of a 3x3 / s2 and a 1x1 / s2 data gradient behind fork()."""
    from ess_amd import functional as Fn
    g = torch.Generator().manual_seed(4)
    H.set_compute('bf16')
    try:
        # nearest-upsampled first source + direct skip, 12 x 36 (the row pool_split_straight), then the same with x1 detached
        c, (dy, w, _), (ref0, ref1) = _fn_case('fn_pool_split', 1, 64, 64, 32, 12, 36, 3, 1, 1, 1, False)
        for need1 in (True, False):
            x0 = _leaf(H, torch.randn(c.N, c.C0, c.Hv // 2, c.Wv // 2, generator=g))
            x1 = _leaf(H, torch.randn(c.N, c.C1, c.Hv, c.Wv, generator=g))
            y = Fn.conv2d(x0, w.cuda(), None, 1, 1, x1=x1 if need1 else x1.detach(), mode0=H.SRC_NEAREST_UP2)
            y.backward(H.to_bf16_c8(dy.cuda()))
            torch.cuda.synchronize()
            check(un8(H, x0.grad, c.C0), ref0, 'c8', f'd0 (pooled, x1 {"requires grad" if need1 else "detached"})')
            if need1:
                check(un8(H, x1.grad, c.C1), ref1, 'c8', 'd1 (full resolution)')
            else:
                assert x1.grad is None
        # conv2d_passthrough, 13 x 21: the skip branch's gradient rides in the data-gradient epilogue
        c, (dy, w, r), (ref0, _) = _fn_case('fn_passthrough', 2, 64, 0, 64, 13, 21, 3, 1, 1, 0, True)
        x = _leaf(H, torch.randn(c.N, c.C0, c.Hv, c.Wv, generator=g))
        y, xp = Fn.conv2d_passthrough(x, w.cuda(), None, 1, 1)
        torch.autograd.backward([y, xp], [H.to_bf16_c8(dy.cuda()), H.to_bf16_c8(r.cuda())])
        torch.cuda.synchronize()
        check(un8(H, x.grad, c.C0), ref0, 'c8', 'd0 (fused skip)')
        # 3x3 / s2 and 1x1 / s2 behind fork(), 18 x 34: each data gradient is stored as bf16 (one rounding each, within the rows' bound
        # b3 / b1 of its own reference), ess_add_bf16 sums the two in fp32 and rounds once more:
        #   |got - (ref3 + ref1)| <= 2^-8 |ref3 + ref1| + (1 + 2^-8) (b3 + b1)
        c3, (dy3, w3, _), (ref3, _) = _fn_case('fn_fork_k3s2', 2, 64, 0, 128, 18, 34, 3, 2, 1, 0, False)
        c1, (dy1, w1, _), (ref1, _) = _fn_case('fn_fork_k1s2', 2, 64, 0, 128, 18, 34, 1, 2, 0, 0, False)
        x = _leaf(H, torch.randn(c3.N, c3.C0, c3.Hv, c3.Wv, generator=g))
        a, b = Fn.fork(x, 2)
        y3, y1 = Fn.conv2d(a, w3.cuda(), None, 2, 1), Fn.conv2d(b, w1.cuda(), None, 2, 0)
        torch.autograd.backward([y3, y1], [H.to_bf16_c8(dy3.cuda()), H.to_bf16_c8(dy1.cuda())])
        torch.cuda.synchronize()
        got, ref = un8(H, x.grad, c3.C0).double(), ref3 + ref1
        assert not torch.isnan(got).any()
        lim = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * (bound(ref3, 'c8') + bound(ref1, 'c8'))
        e = ((got - ref).abs() / lim).max().item()
        assert e <= 1.0, f'fork(3x3 / s2, 1x1 / s2): {e:.3g} x the bound'
    finally:
        H.set_compute('fp32')


def test_conv2dfn_backward_dgrad_refusals(H):
    """refused by Conv2dFn.backward on BF16_C8 tensors: the data gradient of a stride-2 convolution at an odd input extent, and a
    nearest-upsampled SECOND source that wants a gradient (only the first source's gradient is pooled in the epilogue)"""
    from ess_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    H.set_compute('bf16')
    try:
        x = _leaf(H, torch.randn(1, 24, 17, 30, generator=g))
        w = (torch.randn(40, 24, 3, 3, generator=g) / 15).cuda()
        y = Fn.conv2d(x, w, None, 2, 1)
        with pytest.raises(H.EssHipError, match=r'even input extents'):
            y.backward(torch.ones_like(y))
        x0 = _leaf(H, torch.randn(1, 16, 12, 20, generator=g))
        x1 = _leaf(H, torch.randn(1, 16, 6, 10, generator=g))
        w = (torch.randn(32, 32, 3, 3, generator=g) / 17).cuda()
        y = Fn.conv2d(x0, w, None, 1, 1, x1=x1, mode1=H.SRC_NEAREST_UP2)
        with pytest.raises(H.EssHipError, match=r'only the first source may be nearest-upsampled'):
            y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        assert x0.grad is None and x1.grad is None
    finally:
        H.set_compute('fp32')
    # half operands: the planner refuses the pooled and zero-inserted forms (tests/test_host_dgrad_check.py); two half outputs are
    # refused at the launch, before anything runs
    spec = H.conv_spec(1, 9, 17, 32, 0, 64, 3, 1, 1, out_split=32, compute=H.COMPUTE_F16)
    src = H.to_f16_c8(torch.randn(1, 32, 9, 17, generator=g).cuda())
    pw = H.pack_weights(spec, (torch.randn(32, 64, 3, 3, generator=g) / 17).cuda(), kind=H.W_TRANSPOSED)
    o1, o2 = (H.f16_blocks_empty(1, 32, 9, 17, 'cuda').fill_(NAN) for _ in range(2))
    with pytest.raises(H.EssHipError, match=r'forward forms only'):
        H.conv_forward_h16(spec, src, None, pw, out=o1, out2=o2, out_fmt=H.FMT_F16_C8)
    torch.cuda.synchronize()
    assert torch.isnan(o1).all() and torch.isnan(o2).all()  # nothing was launched
