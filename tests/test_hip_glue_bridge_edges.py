"""GPU tier: the glue kernels (bilinear x2 (+ skip sum) in its four forms, 2x2 sum pool, add, add_bf16, sum_scalars) and the format
bridges (fp32 <-> BF16_C8, fp32 / BF16_C8 -> F16_C8 and its [hi | lo] pair, F16_C8 -> BF16_C8) of csrc/pointwise.hip, element by element
against fp64 / IEEE torch-CPU restatements at the shapes where these kernels change paths: odd widths (scalar kernels), one-vector rows,
H = 1, channel counts that leave tail lanes, unaligned pointers, and sizes past the grid cap (4096 x 256 threads) where the grid-stride
loops take a second trip.  Plus the two writers of [hi | lo] pairs (the bridge and the convolution epilogue) above half's range, and
what the mixed InstanceNorm makes of such a pair.  Every test prints its largest error / bound ratio (`RATIO ...`).
Reference layers: e2vid/model/submodules.py:83-93 (UpsampleConvLayer), models/submodules.py:7-24."""
import pytest
import torch
import torch.nn.functional as F

from test_hip_mixed_edges import _check_stats

pytestmark = pytest.mark.gpu

NAN = float('nan')
INF = float('inf')
U24 = 2.0 ** -24


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


def bfr(x):
    return x.to(torch.bfloat16).float()


def block8(x, dtype):
    """`dtype` [N][ceil(C/8)][H][W][8] tensor of an fp32 NCHW one, tail lanes zero (built on the CPU: independent of the bridges)"""
    N, C, Hh, W = x.shape
    CB = (C + 7) // 8
    p = torch.zeros(N, CB * 8, Hh, W, dtype=x.dtype)
    p[:, :C] = x
    return p.view(N, CB, 8, Hh, W).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


def lanes(t):
    """[N][8 nb][H][W] CPU tensor (same dtype) of a channel-blocked [N][nb][H][W][8] one: every lane, the tail lanes included"""
    N, nb, Hh, W, _ = t.shape
    return t.cpu().permute(0, 1, 4, 2, 3).reshape(N, nb * 8, Hh, W).contiguous()


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same(got, want, what):
    """bit-identical wherever `want` is a number (the sign of a zero included), NaN exactly where `want` is NaN (payloads are free)"""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, 'NaN placement', int(gn.sum()), int(wn.sum()))
    bad = (bits(got) != bits(want)) & ~wn
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError((what, int(bad.sum()), 'of', bad.numel(), 'first at', i, got[i].item(), want[i].item()))


def within(got, ref, bound, what):
    """|got - ref| <= bound for EVERY element of the tensor, none of them NaN / inf; -> the largest error / bound ratio"""
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), (what, 'non-finite outputs', int((~torch.isfinite(got)).sum()))
    err = (got.double() - ref).abs()
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError((what, int(bad.sum()), 'of', bad.numel(), 'first at', i, got[i].item(), ref[i].item(), bound[i].item()))
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f'RATIO {what}: {ratio:.3f}')
    return ratio


# ---------------------------------------------------------------------------------------------------------------- bilinear x2 (+ skip sum)
def _up(t):
    return F.interpolate(t, scale_factor=2, mode='bilinear', align_corners=False)


def _bilinear_ref(a, b):
    """(ref, B): the fp64 interpolation of a + b and of |a| + |b|.  An fp32 evaluation of hy (hx v00 + lx v01) + ly (hx v10 + lx v11)
    with v = a + b rounds at most 7 times (1 for a + b, 3 per horizontal blend -- shared --, 3 for the vertical one; the weights 0.25 /
    0.75 / 1 are exact) on partial magnitudes <= B: |got - ref| <= 8 2^-24 B."""
    s = a.double() + (b.double() if b is not None else 0.0)
    m = a.double().abs() + (b.double().abs() if b is not None else 0.0)
    return _up(s), _up(m)


def _sources(shape, seed):
    """a, b with per-plane magnitudes of 1e-3 .. 1e3 and, in every third plane, b ~ -a (the sum cancels: the bound stays |a| + |b|)"""
    g = torch.Generator().manual_seed(seed)
    N, C, Hh, W = shape
    mag = 10.0 ** (torch.rand(N, C, 1, 1, generator=g) * 6 - 3)
    a = torch.randn(shape, generator=g) * mag
    b = torch.randn(shape, generator=g) * mag
    cancel = (torch.arange(N * C).view(N, C, 1, 1) % 3 == 2)
    b = torch.where(cancel, -a * (1 + 1e-3 * torch.randn(shape, generator=g)), b)
    return a, b


BILINEAR_F32 = [
    ('scalar_1x1_all_clamped', (2, 3, 1, 1)),
    ('scalar_odd_w', (1, 5, 7, 9)),
    ('x4_h1', (2, 9, 1, 6)),
    ('x4_w2_one_vector_row', (1, 13, 5, 2)),
    ('x4_33x46', (2, 4, 33, 46)),
    ('scalar_odd_w_blocks', (2, 4, 33, 47)),
    ('x4_second_grid_trip', (4, 16, 128, 136)),   # planes H W = 1 114 112 threads > 4096 x 256
]


@pytest.mark.parametrize('with_b', [True, False], ids=['a+b', 'a'])
@pytest.mark.parametrize('case', BILINEAR_F32, ids=[c[0] for c in BILINEAR_F32])
def test_bilinear_f32(H, case, with_b):
    """fp32 -> fp32: the scalar kernel (odd W) and the x4 kernel (even W), every element against fp64 -- border rows / columns
    (clamped taps) included: `within` compares the whole [N, C, 2H, 2W] tensor"""
    cid, shape = case
    N, C, Hh, W = shape
    a, b = _sources(shape, sum(map(ord, cid)))
    if not with_b:
        b = None
    if cid == 'x4_second_grid_trip':
        assert N * C * Hh * W > 4096 * 256
    got = H.upsample_bilinear2x_add(a.cuda(), None if b is None else b.cuda())
    torch.cuda.synchronize()
    ref, B = _bilinear_ref(a, b)
    assert tuple(got.shape) == (N, C, 2 * Hh, 2 * W)
    within(got.cpu(), ref, 8 * U24 * B, f'bilinear f32 {cid} b={with_b}')


C8_CHANNELS = [5, 8, 13, 24]
C8_PLANES = [(2, 5, 6), (1, 1, 2), (1, 1, 6), (2, 5, 2), (3, 11, 16)]   # N, H, W: H = 1, W = 2 (one vector per row), several workgroups


@pytest.mark.parametrize('C', C8_CHANNELS)
def test_bilinear_f32_to_c8(H, C):
    """fp32 -> BF16_C8: the real channels within the output's bf16 rounding (2^-8 |ref|: half an ulp is 2^-9 of the value) of fp64 plus
    the fp32 evaluation's 8 2^-24 B; the lanes past C inside the last block exactly +0"""
    for N, Hh, W in C8_PLANES:
        a, b = _sources((N, C, Hh, W), 100 * C + Hh + W)
        for second in (b, None):
            y = H.upsample_bilinear2x_add_c8(a.cuda(), None if second is None else second.cuda())
            torch.cuda.synchronize()
            assert tuple(y.shape) == (N, (C + 7) // 8, 2 * Hh, 2 * W, 8) and y.dtype == torch.bfloat16
            full = lanes(y)
            ref, B = _bilinear_ref(a, second)
            within(full[:, :C].float(), ref, 2.0 ** -8 * ref.abs() + 8 * U24 * B, f'bilinear c8 C={C} {N}x{Hh}x{W} b={second is not None}')
            assert (bits(full)[:, C:] == 0).all(), (C, 'tail lanes')


def test_bilinear_c8_refuses_odd_width(H):
    a = torch.randn(1, 8, 3, 5).cuda()
    with pytest.raises(H.EssHipError, match='even source width'):
        H.upsample_bilinear2x_add_c8(a)
    a8 = block8(torch.randn(1, 8, 3, 5), torch.bfloat16).cuda()
    with pytest.raises(H.EssHipError, match='even source width'):
        H.upsample_bilinear2x_add_c8_from_c8(a8)


@pytest.mark.parametrize('C', C8_CHANNELS)
def test_bilinear_c8_to_c8(H, C):
    """BF16_C8 -> BF16_C8 (C channels stored as ceil(C/8) blocks, zero tail lanes): bit-identical to the fp32-source kernel fed the
    same bf16 values, within the bounds above of fp64 over those values, and the zero tail lanes stay +0"""
    for N, Hh, W in C8_PLANES:
        a, b = _sources((N, C, Hh, W), 200 * C + Hh + W)
        a8, b8 = block8(bfr(a), torch.bfloat16), block8(bfr(b), torch.bfloat16)
        av, bv = lanes(a8).float(), lanes(b8).float()   # [N, 8 CB, H, W]: what the kernel reads
        for second in (b8, None):
            y = H.upsample_bilinear2x_add_c8_from_c8(a8.cuda(), None if second is None else second.cuda())
            want = H.upsample_bilinear2x_add_c8(av.cuda(), None if second is None else bv.cuda())
            torch.cuda.synchronize()
            assert tuple(y.shape) == (N, (C + 7) // 8, 2 * Hh, 2 * W, 8)
            same(y, want, f'bilinear c8c8 vs fp32-source kernel C={C} {N}x{Hh}x{W}')
            full = lanes(y)
            ref, B = _bilinear_ref(av, None if second is None else bv)
            within(full.float(), ref, 2.0 ** -8 * ref.abs() + 8 * U24 * B, f'bilinear c8c8 C={C} {N}x{Hh}x{W} b={second is not None}')
            assert (bits(full)[:, C:] == 0).all(), (C, 'tail lanes')


# ---------------------------------------------------------------------------------------------------------------- 2x2 sum pool
SUMPOOL = [
    ('scalar_wo5', (2, 3, 6, 10)),
    ('x2_wo6', (2, 3, 6, 12)),
    ('scalar_ho1', (2, 3, 2, 10)),
    ('x2_ho1', (2, 3, 2, 12)),
    ('x2_second_grid_trip', (4, 16, 256, 520)),   # 64 x 128 x 260 / 2 = 1 064 960 threads > 4096 x 256
]


@pytest.mark.parametrize('accumulate', [False, True], ids=['store', 'accumulate'])
@pytest.mark.parametrize('case', SUMPOOL, ids=[c[0] for c in SUMPOOL])
def test_sumpool2x2(H, case, accumulate):
    """the scalar kernel (odd W_out) and the x2 kernel: bit-identical to the fp32 expression (p00 + p01) + (p10 + p11) (accumulate: one
    more fp32 addition onto the destination's previous value), and within 3 2^-24 sum |p| of the fp64 sum (three roundings on partial
    magnitudes <= sum |p|); also through a caller's `out` (prefilled with NaN where it is to be overwritten)"""
    cid, shape = case
    N, C, Hh, W = shape
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    x = torch.randn(shape, generator=g) * 10.0 ** (torch.rand(N, C, 1, 1, generator=g) * 4 - 2)
    if cid == 'x2_second_grid_trip':
        assert N * C * (Hh // 2) * (W // 2) // 2 > 4096 * 256
    p00, p01, p10, p11 = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
    s32 = (p00 + p01) + (p10 + p11)
    if accumulate:
        before = torch.randn(s32.shape, generator=g) * 3
        out = before.clone().cuda()
        got = H.sumpool2x2(x.cuda(), out=out, accumulate=True)
        assert got is out
        torch.cuda.synchronize()
        same(got, before + s32, f'sumpool accumulate {cid}')
        return
    got = H.sumpool2x2(x.cuda())
    out = torch.full(s32.shape, NAN).cuda()
    H.sumpool2x2(x.cuda(), out=out)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (N, C, Hh // 2, W // 2)
    same(got, s32, f'sumpool {cid}')
    same(out, s32, f'sumpool out= {cid}')
    ref = (p00.double() + p01.double()) + (p10.double() + p11.double())
    mag = p00.double().abs() + p01.double().abs() + p10.double().abs() + p11.double().abs()
    within(got.cpu(), ref, 3 * U24 * mag, f'sumpool {cid}')


# ---------------------------------------------------------------------------------------------------------------- add
def test_add_vector_and_scalar_paths(H):
    """a + b is one fp32 addition per element on every path: 16-byte vectors (n % 4 == 0, aligned pointers; n past the grid cap: the
    second trip of the loop), scalars (n % 4 != 0, or any of a / b / out 4 bytes off a 16-byte boundary), and out aliasing a"""
    g = torch.Generator().manual_seed(5)
    for n in (1000, 1003, 1, 4 * (4096 * 256 + 300)):
        a, b = torch.randn(n, generator=g) * 100, torch.randn(n, generator=g)
        got = H.add(a.cuda(), b.cuda())
        torch.cuda.synchronize()
        same(got, a + b, f'add n={n}')
    n = 1000
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
    want = a + b
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        fa, fb, fo = [torch.full((n + 1,), NAN).cuda() for _ in range(3)]
        va, vb, vo = fa[off[0]:off[0] + n], fb[off[1]:off[1] + n], fo[off[2]:off[2] + n]
        assert [t.data_ptr() % 16 for t in (va, vb, vo)] == [4 * o for o in off] and vo.is_contiguous()
        va.copy_(a)
        vb.copy_(b)
        got = H.add(va, vb, out=vo)
        torch.cuda.synchronize()
        assert got is vo
        same(vo, want, f'add at 4-byte offsets {off}')
        rest = torch.cat([fo[:off[2]], fo[off[2] + n:]])
        assert torch.isnan(rest).all(), ('add wrote outside its view', off)
    for n in (1000, 1003):
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        want = a + b
        ad = a.cuda()
        got = H.add(ad, b.cuda(), out=ad)
        torch.cuda.synchronize()
        assert got is ad
        same(ad, want, f'add in place n={n}')


# ---------------------------------------------------------------------------------------------------------------- add_bf16
def _bf16_operands(n, g, k):
    ts = [torch.randn(n, generator=g).to(torch.bfloat16) for _ in range(k)]
    for t, v in zip(ts, (1.0, 2.0 ** -8, 2.0 ** -9)):   # rounded once 1.0078125, rounded after each addition 1.0
        t[3] = v
    return ts


@pytest.mark.parametrize('n_vec', [5, 300, 4096 * 256 + 333], ids=['5v', '300v', 'second_grid_trip'])
def test_add_bf16_rounds_once(H, n_vec):
    """bf16(fp32(a) + fp32(b) (+ fp32(c))), ONE rounding, bit-identical to the same expression on the CPU; the restatement that rounds
    a + b to bf16 before adding c differs from the kernel in more than 5 % of the elements (it does in about a fifth of N(0, 1)
    triples), so this comparison tells the two apart"""
    g = torch.Generator().manual_seed(n_vec)
    n = 8 * n_vec
    a, b, c = _bf16_operands(n, g, 3)
    got2 = H.add_bf16(a.cuda(), b.cuda())
    got3 = H.add_bf16(a.cuda(), b.cuda(), c.cuda())
    out = torch.full((n,), NAN).to(torch.bfloat16).cuda()
    assert H.add_bf16(a.cuda(), b.cuda(), c.cuda(), out=out) is out
    torch.cuda.synchronize()
    same(got2, (a.float() + b.float()).to(torch.bfloat16), 'add_bf16 a + b')
    once = (a.float() + b.float() + c.float()).to(torch.bfloat16)
    same(got3, once, 'add_bf16 a + b + c')
    same(out, once, 'add_bf16 a + b + c, out=')
    assert got3[3].item() == 1.0078125
    twice = ((a.float() + b.float()).to(torch.bfloat16).float() + c.float()).to(torch.bfloat16)
    assert twice[3].item() == 1.0
    differ = (bits(twice) != bits(got3.cpu())).float().mean().item()
    assert differ > 0.05, differ


def test_add_bf16_shapes_and_refusals(H):
    g = torch.Generator().manual_seed(9)
    a, b, c = [t.view(2, 3, 2, 4, 8) for t in _bf16_operands(2 * 3 * 2 * 4 * 8, g, 3)]   # a BF16_C8 gradient's shape
    got = H.add_bf16(a.cuda(), b.cuda(), c.cuda())
    assert got.shape == a.shape
    same(got, (a.float() + b.float() + c.float()).to(torch.bfloat16), 'add_bf16 5-d')
    bf = torch.bfloat16
    z = lambda *s: torch.zeros(*s, dtype=bf).cuda()  # noqa: E731
    with pytest.raises(H.EssHipError, match='8-element'):
        H.add_bf16(z(12), z(12))
    with pytest.raises(H.EssHipError, match='shape mismatch'):
        H.add_bf16(z(16), z(24))
    with pytest.raises(H.EssHipError, match='shape mismatch'):
        H.add_bf16(z(16), z(16), z(2, 8)[:1])
    flat = z(32)
    off = flat[4:4 + 16]   # 8 bytes past a 16-byte boundary, a whole number of vectors
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    for args, kw in (((off, z(16)), {}), ((z(16), off), {}), ((z(16), z(16), off), {}), ((z(16), z(16)), {'out': off})):
        with pytest.raises(H.EssHipError, match='16-byte aligned'):
            H.add_bf16(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------- sum_scalars
def test_sum_scalars_in_listed_order(H):
    """1, 5 and 16 device scalars of mixed magnitude: the fp32 sum taken in the listed order (s = 0; s += t), bit for bit -- the
    values are such that another order gives another fp32 sum; 17 terms are refused"""
    vals = [1e8, 1.0, -1e8, 3e-5, 7.25, -2.5e-3, 6e4, 1.0 / 3, -6e4, 1e-7, 123.456, -0.1, 2e7, 5.0, -2e7, 0.7]
    for n in (1, 5, 16):
        terms = [torch.tensor(v, dtype=torch.float32) for v in vals[:n]]
        s = torch.tensor(0.0)
        for t in terms:
            s = s + t
        got = H.sum_scalars([t.cuda() for t in terms])
        torch.cuda.synchronize()
        assert got.shape == () and got.dtype == torch.float32
        same(got, s, f'sum_scalars of {n}')
        if n > 1:
            r = torch.tensor(0.0)
            for t in reversed(terms):
                r = r + t
            assert r.item() != s.item()
    with pytest.raises(H.EssHipError, match='1..16 terms'):
        H.sum_scalars([torch.tensor(1.0).cuda() for _ in range(17)])


# ---------------------------------------------------------------------------------------------------------------- format bridges
BIG = [65504.0, 65519.996, 65520.0, 1e5, 131008.0, 131023.99, 131024.0, 2e5]
SMALL = [2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 6e-8, 6.1e-5]   # half subnormals, the flush boundary (a tie to even: 0), the smallest normals
TIES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,      # bf16 ties: neighbours (1, 1 + 2^-7) -> 1 (even), (1 + 2^-7, 1 + 2^-6) -> 1 + 2^-6 (up to even)
        1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,    # half ties: -> 1 (even), -> 1 + 2^-9 (up to even)
        1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -11 - 2.0 ** -20]   # just past / just short of a tie
SPECIALS = [0.0, -0.0, INF, -INF, NAN] + [s * v for v in SMALL + TIES + BIG for s in (1.0, -1.0)]
BRIDGE_CHANNELS = [1, 7, 8, 9, 13, 24]


def _bridge_input(C):
    """[2, C, 5, 7] (70 elements per channel over the two samples): N(0, 1) x 10^(-3 .. 3), with every SPECIALS value planted in every
    channel (at positions that move with the channel, so every lane of a vector sees them at different pixels).  No fp32 subnormals."""
    g = torch.Generator().manual_seed(1000 + C)
    N, Hh, W = 2, 5, 7
    x = torch.randn(N, C, Hh, W, generator=g) * 10.0 ** (torch.rand(N, C, Hh, W, generator=g) * 6 - 3)
    per = N * Hh * W
    assert len(SPECIALS) <= per
    xc = x.permute(1, 0, 2, 3).reshape(C, per).clone()
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    for ch in range(C):
        pos = (torch.arange(len(SPECIALS)) * 3 + 7 * ch) % per   # (3 and 70 are coprime: distinct positions)
        xc[ch, pos] = sp
    x = xc.view(C, N, Hh, W).permute(1, 0, 2, 3).contiguous()
    assert not ((x != 0) & (x.abs() < 2.0 ** -126)).any()
    for v in SPECIALS:
        hit = torch.isnan(x) if v != v else (bits(x) == bits(torch.tensor(v)))
        assert (hit.view(N, C, -1).sum((0, 2)) >= 1).all(), v
    return x


def _sat(v):
    """clamp to half's finite range; NaN stays NaN (torch.clamp propagates it)"""
    return v.clamp(-65504.0, 65504.0)


def _pair_model(v):
    """(hi, lo) halves of fp32 v: hi = half(clamp(v)), lo = half(clamp(v - hi)), IEEE round to nearest even (torch CPU conversions)"""
    hi = _sat(v).to(torch.float16)
    lo = _sat(v - hi.float()).to(torch.float16)
    return hi, lo


@pytest.mark.parametrize('C', BRIDGE_CHANNELS)
def test_bf16_c8_round_trip(H, C):
    """to_bf16_c8: round to nearest even into [N][ceil(C/8)][H][W][8], +-inf / NaN kept, tail lanes +0; from_bf16_c8 back: exactly the
    bf16 values in NCHW (with C % 8 != 0 and N = 2, sample 1's channel 0 sits right behind sample 0's tail lanes)"""
    x = _bridge_input(C)
    y = H.to_bf16_c8(x.cuda())
    back = H.from_bf16_c8(y, C)
    torch.cuda.synchronize()
    same(y, block8(x, torch.bfloat16), f'to_bf16_c8 C={C}')
    assert (bits(lanes(y))[:, C:] == 0).all()
    same(back, bfr(x), f'from_bf16_c8 C={C}')
    assert torch.isinf(back.cpu()).sum().item() == 2 * C and torch.isnan(back.cpu()).sum().item() == C
    # from a CPU-built tensor whose tail lanes are NOT zero: they must not leak into the next sample's channels
    if C % 8:
        dirty = lanes(block8(bfr(x), torch.bfloat16)).clone()
        dirty[:, C:] = 777.0
        N, nb8, Hh, W = dirty.shape
        d8 = dirty.view(N, nb8 // 8, 8, Hh, W).permute(0, 1, 3, 4, 2).contiguous()
        same(H.from_bf16_c8(d8.cuda(), C), bfr(x), f'from_bf16_c8 with dirty tail lanes C={C}')


@pytest.mark.parametrize('C', BRIDGE_CHANNELS)
def test_to_f16_c8_plain_and_pair(H, C):
    """to_f16_c8: half(clamp(v, +-65504)), NaN kept, +-inf -> +-65504, half subnormals as IEEE gives them.  hilo: hi as the plain form,
    lo = half(clamp(v - hi, +-65504)); every stored half finite unless v is NaN; hi + lo = v to 2^-21 |v| + 2^-25 inside half's range
    (lo rounds v - hi, itself <= 2^-11 |v|, to 11 bits: 2^-22 |v|, or to a half subnormal's 2^-25) and = clamp(v, +-131008) above it to
    lo's own half rounding 2^-11 |lo|."""
    x = _bridge_input(C)
    nb = (C + 7) // 8
    want_hi, want_lo = _pair_model(x)
    plain = H.to_f16_c8(x.cuda())
    pair = H.to_f16_c8(x.cuda(), hilo=True)
    torch.cuda.synchronize()
    assert plain.dtype == torch.float16 and tuple(plain.shape) == (2, nb, 5, 7, 8) and tuple(pair.shape) == (2, 2 * nb, 5, 7, 8)
    same(plain, block8(want_hi.float(), torch.float16), f'to_f16_c8 C={C}')
    hi, lo = lanes(pair[:, :nb]), lanes(pair[:, nb:])
    same(pair[:, :nb], block8(want_hi.float(), torch.float16), f'to_f16_c8 hilo, hi C={C}')
    num = ~torch.isnan(x)
    assert torch.isfinite(hi[:, :C][num]).all() and torch.isfinite(lo[:, :C][num]).all(), \
        (C, 'non-finite halves of a number', x[num][~torch.isfinite(lo[:, :C][num])].tolist())
    assert (bits(hi)[:, C:] == 0).all() and (bits(lo)[:, C:] == 0).all()
    # lo bit for bit where v is a number (where v is NaN hi is, and lo is free)
    lo_c, want_c = lo[:, :C].clone(), want_lo.clone()
    lo_c[~num], want_c[~num] = 0.0, 0.0
    same(lo_c, want_c, f'to_f16_c8 hilo, lo C={C}')
    s = hi[:, :C].double() + lo[:, :C].double()
    assert torch.isnan(s[~num]).all()
    v = x.double()
    inside = num & (x.abs() <= 65504)
    err = (s - v).abs()
    assert (err[inside] <= 2.0 ** -21 * v.abs()[inside] + 2.0 ** -25).all()
    print(f'RATIO pair value inside half range C={C}: {(err[inside] / (2.0 ** -21 * v.abs()[inside] + 2.0 ** -25)).max().item():.3f}')
    above = num & (x.abs() > 65504)
    tgt = v.clamp(-131008.0, 131008.0)
    assert ((s - tgt).abs()[above] <= 2.0 ** -11 * (tgt - hi[:, :C].double()).abs()[above]).all()
    big = num & (x.abs() >= 131008)
    assert big.sum().item() >= 10 * C and (s[big].abs() == 131008).all()


@pytest.mark.parametrize('C', BRIDGE_CHANNELS)
def test_bf16_c8_to_f16_c8(H, C):
    """half(clamp(b, +-65504)) of the bf16 values b (8 significant bits: exact inside half's normal range), tail lanes +0"""
    x = _bridge_input(C)
    b8 = block8(x, torch.bfloat16)
    got = H.bf16_c8_to_f16_c8(b8.cuda())
    torch.cuda.synchronize()
    want = _sat(b8.float()).to(torch.float16)
    same(got, want, f'bf16_c8_to_f16_c8 C={C}')
    v = b8.float()
    exact = torch.isfinite(v) & (v.abs() <= 65504) & (v.abs() >= 2.0 ** -14)
    assert torch.equal(got.cpu().float()[exact], v[exact]) and exact.sum().item() > 30 * C
    assert (bits(lanes(got))[:, C:] == 0).all()


@pytest.mark.parametrize('C', BRIDGE_CHANNELS)
def test_f16_c8_to_bf16_c8(H, C):
    """bfloat16(hi (+ lo)), the sum taken in fp32, one rounding to nearest even: from a plain F16_C8 tensor (inf / NaN halves kept), from a
    CPU-built saturated pair, and from the pair to_f16_c8(hilo=True) writes -- finite wherever v is a number"""
    x = _bridge_input(C)
    nb = (C + 7) // 8
    h = block8(x, torch.float16)   # (unsaturated: +-inf halves above 65520)
    got = H.f16_c8_to_bf16_c8(h.cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (2, nb, 5, 7, 8)
    same(got, h.float().to(torch.bfloat16), f'f16_c8_to_bf16_c8 C={C}')
    hi, lo = _pair_model(x)
    lo[torch.isnan(x)] = 0.0
    pair = torch.cat([block8(hi.float(), torch.float16), block8(lo.float(), torch.float16)], 1)
    want = (pair[:, :nb].float() + pair[:, nb:].float()).to(torch.bfloat16)
    got = H.f16_c8_to_bf16_c8(pair.cuda(), hilo=True)
    torch.cuda.synchronize()
    same(got, want, f'f16_c8_to_bf16_c8 hilo C={C}')
    dev_pair = H.to_f16_c8(x.cuda(), hilo=True)
    got = H.f16_c8_to_bf16_c8(dev_pair, hilo=True)
    torch.cuda.synchronize()
    same(got, want, f'f16_c8_to_bf16_c8 of the device pair C={C}')
    gl = lanes(got)[:, :C].float()
    assert torch.isfinite(gl[~torch.isnan(x)]).all() and torch.isnan(gl[torch.isnan(x)]).all()
    assert gl[~torch.isnan(x)].abs().max().item() == 131072.0   # bf16(131008)


# ---------------------------------------------------------------------------------------------------------------- pairs above half's range
def test_instance_norm_of_a_saturated_pair(H):
    """ess_instnorm_forward_c8_mixed (x_fmt = 2) on the pair to_f16_c8(hilo=True) writes for channels far above half's range (2e5 +
    noise and -3e5: stored as +-131008, lo saturated like hi) and one inside the pair's range but above half's (1e5 + noise: hi = 65504,
    lo ~ 34496): statistics and outputs finite everywhere, statistics within _check_stats' bounds of fp64 over the stored hi + lo,
    outputs within test_instance_norm_mixed_statistics' bounds"""
    N, C, Hh, W = 1, 16, 12, 20
    g = torch.Generator().manual_seed(16)
    x = torch.randn(N, C, Hh, W, generator=g) * 0.7 + torch.arange(C).view(1, C, 1, 1) * 0.5
    x[:, 3] = 2e5 + 100 * torch.randn(N, Hh, W, generator=g)
    x[:, 9] = -3e5
    x[:, 13] = 1e5 + 300 * torch.randn(N, Hh, W, generator=g)
    xs = H.to_f16_c8(x.cuda(), hilo=True)
    y, y16, stats = H.instnorm_forward_c8_mixed(xs, C, None, False, 1e-5, 2)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all(), ('non-finite statistics of channels', (~torch.isfinite(stats.cpu())).any(1).nonzero().view(-1).tolist())
    hi, lo = lanes(xs[:, :2]), lanes(xs[:, 2:])
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all(), 'the pair holds non-finite halves'
    xv = hi.double() + lo.double()
    assert (xv[:, 3] == 131008).all() and (xv[:, 9] == -131008).all() and (xv[:, 13] - 1e5).abs().max().item() < 2000
    g16, g8 = lanes(y16).double(), lanes(y).double()
    assert torch.isfinite(g16).all() and torch.isfinite(g8).all()
    r = _check_stats(stats, xv, (2, 3), 1e-5, 'IN of a saturated pair')
    print(f'RATIO instnorm on a saturated pair, rstd: {r / 1e-5:.3f}')
    mr = xv.mean((2, 3), keepdim=True)
    rs = 1.0 / torch.sqrt(((xv - mr) ** 2).mean((2, 3), keepdim=True) + 1e-5)
    ref = (xv - mr) * rs
    slack = (2 ** -20 * xv.abs().mean((2, 3), keepdim=True) + 1e-7) * rs + 1e-5 * ref.abs() + 1e-6
    within(g16, ref, 2.0 ** -11 * ref.abs() + slack, 'instnorm on a saturated pair, y16')
    within(g8, ref, 2.0 ** -8 * ref.abs() + slack, 'instnorm on a saturated pair, y')


def test_conv_epilogue_pair_above_half_range(H):
    """The convolution epilogue's pair writer (ess_cvt4 / ess_cvt4_lo): the decoder 3x3 of test_conv_f16_forms at N = 1, 64 -> 64, 12 x 20,
    with a per-channel affine whose shift puts channels at about 0, +-1e5, +-(131008 +- 32), +-2e5, +-1e6 (and 0.5, 1000, -60000, 65510,
    -65530).  v_ref = the fp64 convolution of the half-rounded operands, scaled and shifted.
      * every stored half is finite; hi = +-65504 where |v_ref| > 65520;
      * hi + lo = clamp(v_ref, +-131008) to within lo's half rounding 2^-11 |clamp(v_ref) - hi| plus the accumulation error
        test_conv_f16_forms allows a [hi | lo] output, (1.5 2^-20 + 3e-6) max(1, |v_ref|);
      * the pair keeps the model's shape hi = half(v), lo = half(v - hi): |lo| <= half an ulp of hi wherever |v_ref| < 65504 (v itself,
        the kernel's fp32 value, is not observable: the accumulation order decides its last bits)."""
    from ess_amd.functional import packed_weight
    N, Cin, Cout, Hv, Wv = 1, 64, 64, 12, 20
    g = torch.Generator().manual_seed(7 + Cout + 3)
    x = torch.randn(N, Cin, Hv, Wv, generator=g) + 1.5
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.0 / (3 * Cin ** 0.5))
    scale = torch.rand(Cout, generator=g) + 0.5
    base = [0.0, 1e5, -1e5, 131008.0 + 32, 131008.0 - 32, -(131008.0 + 32), -(131008.0 - 32), 2e5, -2e5, 1e6, -1e6, 0.5, 1000.0, -60000.0,
            65510.0, -65530.0]
    shift = torch.tensor(base * 4)
    h0 = H.to_f16_c8(x.cuda())
    v_ref = F.conv2d(x.to(torch.float16).double(), w.to(torch.float16).double(), None, 1, 1) * scale.double().view(1, -1, 1, 1) \
        + shift.double().view(1, -1, 1, 1)
    spec = H.conv_spec(N, Hv, Wv, Cin, 0, Cout, 3, 1, 1, act=H.ACT_NONE, compute=H.COMPUTE_F16)
    out = H.f16_blocks_empty(N, Cout, Hv, Wv, 'cuda', hilo=True).fill_(NAN)
    H.conv_forward_h16(spec, h0, None, packed_weight(spec, w.cuda()), H.pack_rows(spec, scale.cuda(), fill=1.0), H.pack_rows(spec, shift.cuda()),
                       out=out, out_fmt=H.FMT_F16_C8_HILO)
    torch.cuda.synchronize()
    nb = Cout // 8
    hi, lo = lanes(out[:, :nb]), lanes(out[:, nb:])
    assert not torch.isnan(hi).any() and not torch.isnan(lo).any(), 'unwritten halves'
    bad = ~(torch.isfinite(hi) & torch.isfinite(lo))
    assert not bad.any(), ('non-finite halves in channels', sorted(set(bad.nonzero()[:, 1].tolist())))
    over = v_ref.abs() > 65520
    assert over.sum().item() >= 40 * Hv * Wv and (hi.double()[over] == 65504 * torch.sign(v_ref[over])).all()
    tgt = v_ref.clamp(-131008.0, 131008.0)
    bound = 2.0 ** -11 * (tgt - hi.double()).abs() + (1.5 * 2.0 ** -20 + 3e-6) * v_ref.abs().clamp(min=1.0)
    within(hi.double() + lo.double(), tgt, bound, 'conv epilogue pair')
    inside = v_ref.abs() < 65504
    ulp = 2.0 ** (torch.floor(torch.log2(hi.double().abs())).clamp(min=-14.0) - 10)
    assert inside.sum().item() >= 16 * Hv * Wv and (lo.double().abs()[inside] <= 0.5 * ulp[inside]).all()
