"""GPU tier: every weight-gradient route (wroute() of csrc/conv_wgrad.hip: ten kernels) and what the plan and launch code add around
them -- split-K slabs, the four parity-phase launches of a stride-2 3x3, one-launch multi-set passes with a per-pass bias mask, split
operands through BF16_C8 copies, the scalar 1x1 head on MFMA-planned slabs for tensors that are not 16-byte aligned -- against a
float64 torch-CPU weight gradient of the operands the kernel reads (tests/wgrad_ref.py), at the smallest shapes at which each edge
exists.  Before EVERY launch the cached slab workspace is filled with 0xFF bytes, and dw / db start as NaN where they are not
accumulated onto: a slab or output element the kernels leave unwritten fails the comparison instead of reading back an earlier value.
tests/test_host_wgrad_check.py proves on the CPU that the bound notices one dropped product in every row."""
import ctypes

import pytest
import torch

from wgrad_ref import BF16, C8, F32, NAN, NCHW, X3, case_reference, check, poison_workspace

pytestmark = pytest.mark.gpu

# id, compute, X fmt, dY fmt, N, C0, C1, Cout, Hv, Wv, k, s, p, m0, m1, route, nsplit
# `route` and `nsplit` restate wroute() / wplan() of csrc/conv_wgrad.hip (which kernel a launch took is not observable): every case
# asserts ess_conv2d_wgrad_workspace == nsplit * (k*k*Cout*Cin + Cout) * 4, so a label stops holding when the plan changes.
# A route suffix: '/tw16', '/tw32' the pixel-tile width of the 1x1 BF16_C8 kernel; '/phases' four parity-phase launches; '/sets3' three
# sets (where the others take two); '/misaligned' tensors one float into their buffers; '/stem' no bias gradient.
WGRAD_EDGE_CASES = [
    ('c8k3_ragged_blocks_odd', BF16, C8, C8, 1, 24, 0, 40, 17, 30, 3, 1, 1, 0, 0, 'W_C8_K3', 6),
    ('c8k3_last_tile_1x1', BF16, C8, C8, 1, 16, 0, 16, 9, 17, 3, 1, 1, 0, 0, 'W_C8_K3', 4),
    ('c8k3_below_one_tile', BF16, C8, C8, 1, 32, 0, 32, 5, 7, 3, 1, 1, 0, 0, 'W_C8_K3', 1),
    ('c8k3_concat_ragged_second', BF16, C8, C8, 2, 64, 20, 72, 13, 21, 3, 1, 1, 0, 0, 'W_C8_K3', 8),
    ('c8k3_nearest_up_concat', BF16, C8, C8, 1, 40, 24, 40, 18, 26, 3, 1, 1, 1, 0, 'W_C8_K3', 6),
    ('c8k3_nearest_up_both', BF16, C8, C8, 2, 32, 16, 32, 16, 24, 3, 1, 1, 1, 1, 'W_C8_K3', 8),
    ('c8k3_zero_up', BF16, C8, C8, 2, 32, 0, 32, 16, 24, 3, 1, 1, 2, 0, 'W_C8_K3', 8),
    ('c8k3_partial_blocks', BF16, C8, C8, 1, 12, 0, 20, 9, 17, 3, 1, 1, 0, 0, 'W_C8_K3', 4),
    ('c8k3_one_launch_3sets', BF16, C8, C8, 2, 256, 0, 256, 24, 40, 3, 1, 1, 0, 0, 'W_C8_K3/sets3', 16),
    ('c8k3s2_ragged_blocks', BF16, C8, C8, 2, 24, 0, 40, 10, 12, 3, 2, 1, 0, 0, 'W_C8_K3/phases', 2),
    ('c8k3s2_out_9x17', BF16, C8, C8, 1, 64, 0, 72, 18, 34, 3, 2, 1, 0, 0, 'W_C8_K3/phases', 4),
    ('c8k3s2_partial_blocks', BF16, C8, C8, 1, 12, 0, 20, 10, 12, 3, 2, 1, 0, 0, 'W_C8_K3/phases', 1),
    ('c8k1_s1_tw32', BF16, C8, C8, 1, 24, 0, 40, 17, 30, 1, 1, 0, 0, 0, 'W_C8_K1/tw32', 5),
    ('c8k1_s1_tw16', BF16, C8, C8, 2, 72, 0, 24, 9, 16, 1, 1, 0, 0, 0, 'W_C8_K1/tw16', 4),
    ('c8k1_s2_odd_tw16', BF16, C8, C8, 2, 24, 0, 40, 17, 29, 1, 2, 0, 0, 0, 'W_C8_K1/tw16', 4),
    ('c8k1_s2_odd_tw32', BF16, C8, C8, 1, 64, 0, 128, 25, 43, 1, 2, 0, 0, 0, 'W_C8_K1/tw32', 4),
    ('c8k1_partial_blocks', BF16, C8, C8, 1, 12, 0, 20, 9, 16, 1, 1, 0, 0, 0, 'W_C8_K1/tw16', 2),
    ('head_c8x_35px', BF16, C8, NCHW, 1, 20, 0, 6, 5, 7, 1, 1, 0, 0, 0, 'W_SMALL1X1_C8X', 1),
    ('head_c8x_partial_chunk', BF16, C8, NCHW, 2, 32, 0, 11, 9, 15, 1, 1, 0, 0, 0, 'W_SMALL1X1_C8X', 4),
    ('stem7_odd_f32', F32, NCHW, NCHW, 2, 1, 0, 64, 23, 37, 7, 2, 3, 0, 0, 'W_TAPS7/stem', 12),
    ('stem7_odd_c8_dy', BF16, NCHW, C8, 2, 1, 0, 64, 23, 37, 7, 2, 3, 0, 0, 'W_TAPS7/stem', 12),
    ('f32_tile_k3s1', F32, NCHW, NCHW, 1, 12, 0, 17, 17, 29, 3, 1, 1, 0, 0, 'W_F32_TILE', 9),
    ('f32_tile_k3s2', F32, NCHW, NCHW, 1, 12, 0, 17, 17, 29, 3, 2, 1, 0, 0, 'W_F32_TILE', 3),
    ('f32_tile_k1s1', F32, NCHW, NCHW, 1, 12, 0, 17, 17, 29, 1, 1, 0, 0, 0, 'W_F32_TILE', 9),
    ('f32_tile_k1s2', F32, NCHW, NCHW, 1, 12, 0, 17, 17, 29, 1, 2, 0, 0, 0, 'W_F32_TILE', 3),
    ('f32_tile_nearest_up_concat', F32, NCHW, NCHW, 2, 16, 12, 20, 14, 18, 3, 1, 1, 1, 0, 'W_F32_TILE', 12),
    ('bf16k3_concat_odd', BF16, NCHW, NCHW, 1, 12, 8, 40, 17, 30, 3, 1, 1, 0, 0, 'W_BF16_K3', 5),
    ('bf16k3_zero_up', BF16, NCHW, NCHW, 2, 32, 0, 32, 16, 24, 3, 1, 1, 2, 0, 'W_BF16_K3', 8),
    ('bf16k3_fast_concat', BF16, NCHW, NCHW, 2, 20, 16, 64, 16, 24, 3, 1, 1, 0, 0, 'W_BF16_K3_FAST', 8),
    ('bf16k1_rows8', BF16, NCHW, NCHW, 1, 72, 0, 40, 16, 24, 1, 1, 0, 0, 0, 'W_BF16_K1', 4),
    ('small1x1_1024_pairs', F32, NCHW, NCHW, 1, 64, 0, 16, 5, 7, 1, 1, 0, 0, 0, 'W_SMALL1X1', 1),
    ('small1x1_cin33', F32, NCHW, NCHW, 2, 33, 0, 11, 8, 16, 1, 1, 0, 0, 0, 'W_SMALL1X1', 2),
    ('small1x1_mfma', F32, NCHW, NCHW, 2, 20, 0, 6, 8, 16, 1, 1, 0, 0, 0, 'W_SMALL1X1_MFMA', 1),
    ('small1x1_mfma_slabs_scalar_kernel', F32, NCHW, NCHW, 2, 20, 0, 6, 8, 16, 1, 1, 0, 0, 0, 'W_SMALL1X1_MFMA/misaligned', 1),
    ('x3_c8_copies', X3, NCHW, NCHW, 1, 12, 0, 40, 17, 30, 3, 1, 1, 0, 0, 'X3_VIA_C8/sets3', 6),
    ('x3_c8_copies_mask_flips_mid_loop', X3, NCHW, NCHW, 2, 8, 0, 8, 136, 128, 3, 1, 1, 0, 0, 'X3_VIA_C8', 256),
]
CASE_IDS = [c[0] for c in WGRAD_EDGE_CASES]
# Not reached: the ESS_X3_WGRAD_C8=0 / ESS_X3_WGRAD_FUSED=0 forms of split operands (environment switches read once per process).


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


def _one_float_in(t):
    """the same fp32 values as a contiguous view one float into a larger buffer: 4-byte aligned, not 16"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _device_set(H, c, q):
    """device tensors of one (x0, x1, dy) set in the row's storage formats"""
    def put(t, fmt):
        if t is None:
            return None
        if fmt == C8:
            return H.to_bf16_c8(t.cuda())  # (channels past C in a partial block are zeros)
        return _one_float_in(t.cuda()) if c.misaligned else t.cuda()
    return put(q[0], c.xfmt), put(q[1], c.xfmt), put(q[2], c.dyfmt)


def _spec(H, c):
    return H.conv_spec(c.N, c.Hv, c.Wv, c.C0, c.C1, c.Cout, c.k, c.s, c.p, c.m0, c.m1, compute=c.compute)


def _plain(H, spec, dset, dw, db, accumulate=False):
    poison_workspace(H, spec, dset[0], dset[2])
    H.conv_wgrad(spec, dset[0], dset[1], dset[2], dw, db, accumulate=accumulate)


def _sets(H, spec, dsets, dw, db, accumulate=False):
    poison_workspace(H, spec, dsets[0][0], dsets[0][2])
    H.conv_wgrad_sets(spec, dsets, dw, db, accumulate=accumulate)


def _tiles_of_c8_k3(c):
    """(ntiles, C_out x C_in tile pairs) of the LDS-DMA kernel's plan: 16 x 8 pixel tiles, 64 x 64 channel tiles"""
    return c.N * -(-c.Wo // 16) * -(-c.Ho // 8), -(-c.Cout // 64) * -(-c.Cin // 64)


@pytest.mark.parametrize('row', WGRAD_EDGE_CASES, ids=CASE_IDS)
def test_wgrad_route_edges(H, row):
    """One row: (1) a plain call onto NaN outputs; (2) accumulate=True onto known values WITH db (what functional._weight_gradient does
    on every layer of every step); (3) ess_conv2d_wgrad_sets with 2 (3) independent sets and a bias, plain and accumulating, against
    the float64 sum over the sets; (4) one set through the sets entry == the plain call, bit for bit.  Bounds: wgrad_ref.TOL times the
    number of accumulated contributions, relative to max|ref|."""
    c, sets, refs = case_reference(row)
    spec = _spec(H, c)
    sfmt = H.FMT_BF16_C8 if c.xfmt == C8 else H.FMT_F32_NCHW
    dfmt = H.FMT_BF16_C8 if c.dyfmt == C8 else H.FMT_F32_NCHW
    assert (H.COMPUTE_FP32, H.COMPUTE_BF16, H.COMPUTE_BF16X3) == (F32, BF16, X3) and (H.FMT_F32_NCHW, H.FMT_BF16_C8) == (NCHW, C8)
    # the label: this route with this many slabs is what the library plans
    assert H.lib().ess_conv2d_wgrad_workspace(ctypes.byref(spec.desc_fmt(sfmt, dfmt))) == c.workspace_bytes(), (c.id, H.lib().ess_last_error())
    if c.id in ('c8k3_one_launch_3sets', 'x3_c8_copies_mask_flips_mid_loop'):
        # a workgroup's tile list crosses the pass boundaries at other positions than its neighbour's (with split operands the
        # per-tile bias switch then flips mid-loop: bias mask 0b101)
        ntiles, npairs = _tiles_of_c8_k3(c)
        assert c.nsplit == min(-(-256 // npairs), ntiles) and ntiles % c.nsplit != 0 and c.nsplit < ntiles, (ntiles, npairs)
    dsets = [_device_set(H, c, q) for q in sets]
    g = torch.Generator().manual_seed(len(c.id))
    wshape = (c.Cout, c.Cin, c.k, c.k)

    def outputs(ref_w, ref_b, known):
        """dw, db (None on a route without a bias gradient) and the values they start from: NaN, or random ones of the gradient's size"""
        if known:
            A = (torch.randn(wshape, generator=g) * ref_w.std().item()).cuda()
            a = (torch.randn(c.Cout, generator=g) * ref_b.std().item()).cuda()
        else:
            A, a = torch.full(wshape, NAN, device='cuda'), torch.full((c.Cout,), NAN, device='cuda')
        return A.clone(), (a.clone() if c.bias else None), A, a

    def compare(dw, db, A, a, ref_w, ref_b, passes, what):
        torch.cuda.synchronize()
        ew = check(dw.cpu().double() - (0 if A is None else A.cpu().double()), ref_w, passes, c.kind, f'{c.id} {what} dw')
        eb = check(db.cpu().double() - (0 if a is None else a.cpu().double()), ref_b, passes, c.kind, f'{c.id} {what} db') if c.bias else 0.0
        print(f'{c.id} {what}: dw at {ew:.3f}, db at {eb:.3f} of the bound')

    # 1. plain call
    rw, rb = refs[0]
    dw, db, _, _ = outputs(rw, rb, False)
    _plain(H, spec, dsets[0], dw, db)
    compare(dw, db, None, None, rw, rb, 1, 'plain')
    # 2. accumulate onto known values, db included
    dw2, db2, A, a = outputs(rw, rb, True)
    _plain(H, spec, dsets[0], dw2, db2, accumulate=True)
    compare(dw2, db2, A, a, rw, rb, 2, 'accumulate')
    # 3. several sets
    sw, sb = sum(r[0] for r in refs), sum(r[1] for r in refs)
    dw3, db3, _, _ = outputs(sw, sb, False)
    _sets(H, spec, dsets, dw3, db3)
    compare(dw3, db3, None, None, sw, sb, c.nsets, f'{c.nsets} sets')
    dw4, db4, A, a = outputs(sw, sb, True)
    _sets(H, spec, dsets, dw4, db4, accumulate=True)
    compare(dw4, db4, A, a, sw, sb, c.nsets + 1, f'{c.nsets} sets accumulate')
    # 4. one set through the sets entry == the plain call
    dw5, db5, _, _ = outputs(rw, rb, False)
    _sets(H, spec, dsets[:1], dw5, db5)
    torch.cuda.synchronize()
    assert torch.equal(dw5, dw) and (not c.bias or torch.equal(db5, db)), (c.id, 'one set through ess_conv2d_wgrad_sets != ess_conv2d_wgrad')


PARTIAL_BLOCK_ROWS = [r for r in WGRAD_EDGE_CASES if (r[2] == C8 and (r[5] % 8 or r[6] % 8)) or (r[3] == C8 and r[7] % 8)]


@pytest.mark.parametrize('row', PARTIAL_BLOCK_ROWS, ids=[r[0] for r in PARTIAL_BLOCK_ROWS])
def test_wgrad_c8_padding_lanes_are_masked(H, row):
    """BF16_C8 tensors with a partial last channel block: the lanes past C hold FINITE GARBAGE (1e4) instead of to_bf16_c8's zeros.  The
    kernels mask by channel index (ci < Cin, co < Cout on the slab store; whole blocks on the loads), so the gradient over the real
    channels must not move by a bit -- plain call and sets call."""
    c, sets, _ = case_reference(row)
    assert len(PARTIAL_BLOCK_ROWS) >= 5
    spec = _spec(H, c)
    clean = [_device_set(H, c, q) for q in sets]

    def garbage(t, C):
        if t is None or not H.is_c8(t) or C % 8 == 0:
            return t
        t = t.clone()
        t[:, -1, :, :, C % 8:] = 1e4
        return t
    dirty = [(garbage(q[0], c.C0), garbage(q[1], c.C1), garbage(q[2], c.Cout)) for q in clean]
    assert any(d is not k for qd, qk in zip(dirty, clean) for d, k in zip(qd, qk))
    outs = []
    for dsets in (clean, dirty):
        dw, db = torch.full((c.Cout, c.Cin, c.k, c.k), NAN, device='cuda'), torch.full((c.Cout,), NAN, device='cuda')
        dws, dbs = torch.full_like(dw, NAN), torch.full_like(db, NAN)
        _plain(H, spec, dsets[0], dw, db)
        _sets(H, spec, dsets, dws, dbs)
        torch.cuda.synchronize()
        outs.append((dw, db, dws, dbs))
    for got, want, what in zip(outs[1], outs[0], ('dw', 'db', 'dw of the sets call', 'db of the sets call')):
        assert not torch.isnan(want).any(), (c.id, what)
        assert torch.equal(got, want), (c.id, what, (got - want).abs().max().item())


def test_wgrad_refusals(H):
    """Two refusals of the library as hip.conv_wgrad raises them: a BF16_C8 3x3 / stride 2 at odd input extents (refused by design, as
    Conv2dFn.backward's "needs even input extents"), and BF16_C8 tensors that are not 16-byte aligned."""
    N, C, Co, Hv, Wv = 1, 24, 40, 17, 30
    x, dw = torch.randn(N, C, Hv, Wv).cuda(), torch.full((Co, C, 3, 3), NAN, device='cuda')
    spec = H.conv_spec(N, Hv, Wv, C, 0, Co, 3, 2, 1, compute=H.COMPUTE_BF16)
    dy = torch.randn(N, Co, spec.H_out, spec.W_out).cuda()
    with pytest.raises(H.EssHipError, match=r'3x3 / stride 2 / pad 1 on even extents'):
        H.conv_wgrad(spec, H.to_bf16_c8(x), None, H.to_bf16_c8(dy), dw)
    spec = H.conv_spec(N, Hv, Wv, C, 0, Co, 3, 1, 1, compute=H.COMPUTE_BF16)
    dy8 = H.to_bf16_c8(torch.randn(N, Co, Hv, Wv).cuda())
    x8 = H.to_bf16_c8(x)
    buf = torch.empty(x8.numel() + 1, dtype=torch.bfloat16, device='cuda')
    off = buf[1:].view(x8.shape)
    off.copy_(x8)
    assert H.is_c8(off) and off.is_contiguous() and off.data_ptr() % 16 == 2
    with pytest.raises(H.EssHipError, match=r'BF16_C8 tensors must be 16-byte aligned'):
        H.conv_wgrad(spec, off, None, dy8, dw)
    torch.cuda.synchronize()
    assert torch.isnan(dw).all()  # nothing was launched
