"""GPU tier: the fused class head (ess_seg_head: 1x1 class convolution + nearest resize + first argmax, optional palette colours and
winner's softmax probability; reference semantics training/ess_trainer.py:424-493) against fp64 on the same rounded operands, and
SemSegE2VID.predict against SemSegE2VID.forward.

Label rule (derived, not measured).  With fp32 accumulation of C products and a bias in any order (bf16 x bf16 and half x half
products are exact in fp32, the fp32 source's are not: hence C + 2), |z_k - z_k^fp64| <= e_k = gamma_{C+2} (|b_k| + sum_c |w_kc x_c|),
gamma_n = n u / (1 - n u), u = 2^-24.  A label must equal the fp64 argmax wherever the fp64 top-two gap exceeds e_top1 + e_top2;
elsewhere it must be a class within that band of the maximum.  The excused pixels are capped at 0.1 % of a case (one pixel below
1000 pixels) as a condition on the fixture.

Confidence tolerance.  torch's own fp32 evaluation on the CPU (fp32 convolution of the same rounded operands, fp32 softmax) differs
from the fp64 softmax of the fp64 scores by at most 3.2e-7 over these cases (measured on the CPU over every (format, K, C) pair
at 200 x 352 and 3 x 37 x 53: 2.6e-7 fp32 / bf16 operands, 3.2e-7 half); four times that, 1.28e-6, is allowed for the
device (hardware exp2 with a first-order correction, one division), which itself measured 3.2e-7 (2.6e-7 with fp32 / bf16 operands)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TORCH_FP32_CONF_ERR = 3.2e-7
CONF_TOL = 4 * TORCH_FP32_CONF_ERR
FMTS = ('fp32', 'bf16', 'f16')
KS = (2, 6, 11, 19, 64)
CS = (8, 32, 40, 64, 12)


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


def round_to(t, fmt):
    if fmt == 'bf16':
        return t.to(torch.bfloat16).float()
    if fmt == 'f16':
        return t.to(torch.float16).float()
    return t


def make_operands(fmt, N, K, C, Hh, W, seed):
    """post-ReLU normal x in the stored format's values, w ~ N(0, 1/C) rounded to the operand type, b ~ 0.1 N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    x = round_to(torch.randn(N, C, Hh, W, generator=g).relu(), fmt)
    w = torch.randn(K, C, generator=g) / C ** 0.5
    b = 0.1 * torch.randn(K, generator=g)
    return x, w, b


def to_device_format(x, fmt, tail=1.0):
    """the device tensor of fp32 NCHW values in the given source format; C8 tail channels (c >= C) are filled with `tail`: the
    kernel must mask them on the weight side, not rely on zeros"""
    if fmt == 'fp32':
        return x.cuda().contiguous()
    N, C, Hh, W = x.shape
    CB = (C + 7) // 8
    p = torch.full((N, CB * 8, Hh, W), tail)
    p[:, :C] = x
    p = p.view(N, CB, 8, Hh, W).permute(0, 1, 3, 4, 2).contiguous()
    return p.to(torch.bfloat16 if fmt == 'bf16' else torch.float16).cuda()


def scores64(x, w, b, fmt):
    """fp64 scores and the bound e_k per pixel, [N, K, H, W] each"""
    wr = round_to(w, fmt).double()
    z = torch.einsum('kc,nchw->nkhw', wr, x.double()) + b.double().view(1, -1, 1, 1)
    n = x.shape[1] + 2
    gam = n * U / (1 - n * U)
    e = gam * (torch.einsum('kc,nchw->nkhw', wr.abs(), x.double().abs()) + b.double().abs().view(1, -1, 1, 1))
    return z, e


def src_index(out, size):
    """resize_nearest's source index in fp32: min(floor(dst * (float)in / out), in - 1)"""
    s = torch.tensor(float(size), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    return (torch.arange(out, dtype=torch.float32) * s).floor().long().clamp(max=size - 1)


def map_pixels(t, window, out_hw):
    """t [..., H, W] -> [..., H_out, W_out] by the nearest rule inside the window"""
    y0, x0, h, w = window
    iy = y0 + src_index(out_hw[0], h)
    ix = x0 + src_index(out_hw[1], w)
    return t[..., iy, :][..., ix]


def check_labels(labels, z, e, what, extra_share=None):
    """the label rule of the module docstring; labels [N, H, W] (any integer dtype, CPU), z / e [N, K, H, W] fp64"""
    labels = labels.long()
    top = z.argmax(1)
    zs, order = z.sort(1, descending=True)
    if z.shape[1] > 1:
        band = e.gather(1, order[:, :1]).squeeze(1) + e.gather(1, order[:, 1:2]).squeeze(1)
        gap = zs[:, 0] - zs[:, 1]
    else:
        band, gap = torch.zeros_like(zs[:, 0]), torch.full_like(zs[:, 0], float('inf'))
    strict = gap > band
    px = labels.numel()
    excused = int((~strict).sum())
    cap = max(1, int(px * 1e-3)) if extra_share is None else extra_share
    print(f'{what}: {px} pixels, {excused} inside the rounding band (cap {cap}), wrong outside: {int((labels != top)[strict].sum())}')
    assert excused <= cap, f'{what}: the fixture excuses {excused} of {px} pixels (cap {cap})'
    assert torch.equal(labels[strict], top[strict]), f'{what}: {int((labels != top)[strict].sum())} labels differ from the fp64 argmax outside the band'
    zl = z.gather(1, labels.unsqueeze(1)).squeeze(1)
    assert bool((zs[:, 0] - zl <= band)[~strict].all()), f'{what}: a label inside the band is not one of the classes within it'


def palette_for(K):
    g = torch.Generator().manual_seed(K)
    return torch.randint(0, 255, (K, 3), generator=g, dtype=torch.uint8)  # (no 0xFF: the pre-fill value)


def run_head(H, xd, C, w, b, fmt, window=None, out_hw=None, want_colour=True, want_conf=True):
    """launch through the C ABI into PRE-FILLED buffers (labels / colour 0xFF, confidence NaN) so unwritten pixels show"""
    import ctypes
    K = w.shape[0]
    N, Hs, Ws = xd.shape[0], xd.shape[2], xd.shape[3]
    y0, x0, h, ww = window if window is not None else (0, 0, Hs, Ws)
    Ho, Wo = out_hw if out_hw is not None else (h, ww)
    labels = torch.full((N, Ho, Wo), 0xFF, dtype=torch.uint8, device='cuda')
    colour = torch.full((N, Ho, Wo, 3), 0xFF, dtype=torch.uint8, device='cuda') if want_colour else None
    conf = torch.full((N, Ho, Wo), float('nan'), dtype=torch.float32, device='cuda') if want_conf else None
    pal = palette_for(K).cuda()
    wd, bd = w.cuda().contiguous(), b.cuda().contiguous()
    code = {'fp32': H.FMT_F32_NCHW, 'bf16': H.FMT_BF16_C8, 'f16': H.FMT_F16_C8}[fmt]
    rc = H.lib().ess_seg_head(H.ptr(xd, xd.dtype), code, H.ptr(wd), H.ptr(bd), H.ptr(pal if want_colour else None, torch.uint8),
                              H.ptr(labels, torch.uint8), H.ptr(colour, torch.uint8), H.ptr(conf), N, C, K, Hs, Ws, y0, x0, h, ww, Ho, Wo,
                              H.stream())
    assert rc == 0, H.lib().ess_last_error().decode()
    torch.cuda.synchronize()
    return labels.cpu(), None if colour is None else colour.cpu(), None if conf is None else conf.cpu(), pal.cpu()


def check_all(H, fmt, N, K, C, Hh, W, seed, window=None, out_hw=None, want_colour=True, want_conf=True):
    x, w, b = make_operands(fmt, N, K, C, Hh, W, seed)
    xd = to_device_format(x, fmt)
    labels, colour, conf, pal = run_head(H, xd, C, w, b, fmt, window, out_hw, want_colour, want_conf)
    z, e = scores64(x, w, b, fmt)
    win = window if window is not None else (0, 0, Hh, W)
    ohw = out_hw if out_hw is not None else (win[2], win[3])
    z, e = map_pixels(z, win, ohw), map_pixels(e, win, ohw)
    what = f'{fmt} N={N} K={K} C={C} {Hh}x{W} window={window} out={out_hw}'
    assert K < 255 and int(labels.max()) < K, f'{what}: unwritten or out-of-range labels'
    check_labels(labels, z, e, what)
    if want_colour:
        assert torch.equal(colour, pal[labels.long()]), f'{what}: colour != palette[labels]'
    if want_conf:
        assert not torch.isnan(conf).any(), f'{what}: unwritten confidence'
        ref = torch.softmax(z, 1).max(1).values
        err = (conf.double() - ref).abs().max().item()
        print(f'{what}: confidence max |err| {err:.3e} (allowed {CONF_TOL:.1e})')
        assert err <= CONF_TOL, (what, err)
    return labels


@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('fmt', FMTS)
def test_seg_head_vs_fp64(H, fmt, K, C):
    """every (format, K, C) on planes that are not a multiple of the workgroup's 256 pixels, N in {1, 3}, optional outputs on and off"""
    i = KS.index(K) + CS.index(C)
    check_all(H, fmt, 1, K, C, 200, 352, 100 + i, want_colour=i % 2 == 0, want_conf=i % 3 != 1)
    check_all(H, fmt, 3, K, C, 37, 53, 200 + i, want_colour=i % 2 == 1, want_conf=i % 3 == 1)
    check_all(H, fmt, 3, K, C, 1, 1, 300 + i)
    check_all(H, fmt, 1, K, C, 1, 1, 400 + i, want_colour=False, want_conf=False)


@pytest.mark.parametrize('fmt', FMTS)
def test_seg_head_window_and_resize(H, fmt):
    """a window off the plane's origin and smaller than it (the 2-row / 3-column margins of 60 x 90 in 64 x 96); out_hw equal, larger
    (440 x 640 -> 480 x 640) and smaller (64 x 96 -> 50 x 70) than the source; resized labels are BIT-equal to the source-size labels
    mapped by the same index rule on the host; fp32 format: equal to argmax(hip.resize_nearest(scores)) under the label rule"""
    for K, C in ((11, 32), (6, 12)):
        win = (2, 3, 60, 90)
        check_all(H, fmt, 3, K, C, 64, 96, 7, window=win)
        check_all(H, fmt, 1, K, C, 64, 96, 8, window=win, out_hw=(120, 180))
        check_all(H, fmt, 1, K, C, 64, 96, 9, window=win, out_hw=(50, 70), want_colour=False)
        for (Hh, W), ohw, seed in (((440, 640), (480, 640), 10), ((64, 96), (50, 70), 11), ((64, 96), (64, 96), 12)):
            resized = check_all(H, fmt, 1, K, C, Hh, W, seed, out_hw=ohw, want_conf=False)
            x, w, b = make_operands(fmt, 1, K, C, Hh, W, seed)
            at_src = run_head(H, to_device_format(x, fmt), C, w, b, fmt, want_colour=False, want_conf=False)[0]
            assert torch.equal(resized, map_pixels(at_src, (0, 0, Hh, W), ohw)), (fmt, K, C, Hh, W, ohw)
            if fmt == 'fp32':
                z, e = scores64(x, w, b, fmt)
                # the device's own resize of a plane of pixel indices (exact in fp32) gives ITS source pixel per output pixel
                idx = torch.arange(Hh * W, dtype=torch.float32).view(1, 1, Hh, W).cuda()
                src = H.resize_nearest(idx, ohw).cpu().long().view(-1)
                zr = z.view(1, K, -1)[:, :, src].view(1, K, *ohw)
                er = e.view(1, K, -1)[:, :, src].view(1, K, *ohw)
                check_labels(resized, zr, er, f'fp32 vs argmax(resize_nearest) K={K} C={C} {Hh}x{W}->{ohw}')


@pytest.mark.parametrize('fmt', FMTS)
def test_seg_head_exact_ties_take_the_lower_index(H, fmt):
    """two identical weight rows and biases (classes 3 and 7): 7 never wins and 3 wins wherever the pair leads by more than the band;
    all K rows identical: class 0 everywhere -- first maximum wins, as argmax_conf_kernel / torch.argmax"""
    K, C, Hh, W = 11, 32, 37, 53
    x, w, b = make_operands(fmt, 3, K, C, Hh, W, 21)
    w[7], b[7] = w[3], b[3]
    labels = run_head(H, to_device_format(x, fmt), C, w, b, fmt)[0].long()
    assert not bool((labels == 7).any())
    z, e = scores64(x, w, b, fmt)
    keep = [k for k in range(K) if k != 7]
    remap = torch.zeros(K, dtype=torch.long)
    remap[keep] = torch.arange(K - 1)
    check_labels(remap[labels], z[:, keep], e[:, keep], f'{fmt} tie of classes 3 and 7')
    w[:], b[:] = w[0].clone(), b[0].clone()
    labels, colour, conf, pal = run_head(H, to_device_format(x, fmt), C, w, b, fmt)
    assert int(labels.max()) == 0
    assert torch.equal(colour, pal[labels.long()])
    assert (conf - 1.0 / K).abs().max().item() <= CONF_TOL


@pytest.mark.parametrize('fmt', FMTS)
def test_seg_head_python_wrapper(H, fmt):
    """hip.seg_head: formats detected from the tensor (a float16 F16_C8 tensor and the bfloat16-typed f16_c8_empty container alike),
    the convolution's [K, C, 1, 1] weight accepted, outputs on and off"""
    K, C, Hh, W = 11, 32, 64, 96
    x, w, b = make_operands(fmt, 2, K, C, Hh, W, 31)
    xd = to_device_format(x, fmt, tail=0.0)
    z, e = scores64(x, w, b, fmt)
    pal = palette_for(K).cuda()
    lab, col, conf = H.seg_head(xd, C, w.cuda().view(K, C, 1, 1), b.cuda(), palette=pal, want_confidence=True)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (2, Hh, W) and tuple(col.shape) == (2, Hh, W, 3) and conf.dtype == torch.float32
    check_labels(lab.cpu(), z, e, f'wrapper {fmt}')
    assert torch.equal(col.cpu(), pal.cpu()[lab.cpu().long()])
    lab2, col2, conf2 = H.seg_head(xd, C, w.cuda(), b.cuda())
    assert col2 is None and conf2 is None and torch.equal(lab, lab2)
    if fmt == 'f16':
        box = H.f16_c8_empty(2, C, Hh, W, xd.device)
        box.view(torch.float16).copy_(xd)
        assert torch.equal(H.seg_head(box, C, w.cuda(), b.cuda())[0], lab)
    lab3 = H.seg_head(xd, C, w.cuda(), b.cuda(), window=(2, 3, 60, 90), out_hw=(30, 45))[0]
    assert torch.equal(lab3.cpu(), map_pixels(lab.cpu(), (2, 3, 60, 90), (30, 45)))


# ------------------------------------------------------------------------------------------------ SemSegE2VID.predict
def _latents(N, Hh, W, seed):
    g = torch.Generator().manual_seed(seed)
    # event latents are post-activation hidden states: (1: 32 ch, 2: 64, 4: 128, 8: 256)
    return {s: torch.tanh(torch.randn(N, c, Hh // s, W // s, generator=g)).cuda() for s, c in ((1, 32), (2, 64), (4, 128), (8, 256))}


def forward_with_last(dec, lat):
    """(logits, the tensor that enters decoder_scale_5) of dec.forward(lat).  forward calls the layer's forward_fused directly, which
    module hooks do not see: the spy wraps that method of decoder_scale_4's layer"""
    grabbed = []
    layer = dec.decoder_scale_4[0 if dec.skip_connect else 1]
    fused = layer.forward_fused
    layer.forward_fused = lambda *a, **k: (grabbed.append(fused(*a, **k)), grabbed[-1])[1]
    try:
        logits = dec(lat)[1].clone()
    finally:
        del layer.forward_fused
    return logits, grabbed[-1]


def head_scores(H, dec, last, mode):
    """fp64 scores z and bound e [N, K, H, W] of the class convolution on the operands forward's last contraction reads in `mode`
    (the half copy in 'mixed', the BF16_C8 tensor in 'bf16', fp32 otherwise; bf16x3: + 2^-15 sum_c |w_kc x_c|, its split operands
    keep 16 mantissa bits each and drop the lo x lo products) -> (z, e, w, x values)"""
    c5 = dec.decoder_scale_5[0]
    K, C = c5.out_channels, c5.in_channels
    w, b = c5.weight.detach().cpu().view(K, C), c5.bias.detach().cpu()
    if mode == 'mixed':
        h16, hilo = H.h16_of(last)
        assert not hilo
        N, _, Hh, W, _ = h16.shape
        xv, fmt = h16.float().permute(0, 1, 4, 2, 3).reshape(N, -1, Hh, W)[:, :C].cpu(), 'f16'
    elif mode == 'bf16':
        xv, fmt = H.from_bf16_c8(last, C).cpu(), 'bf16'
    else:
        xv, fmt = last.cpu(), 'fp32'
    z, e = scores64(xv, w, b, fmt)
    if mode == 'bf16x3':
        e = e + 2.0 ** -15 * torch.einsum('kc,nchw->nkhw', w.double().abs(), xv.double().abs())
    return z, e, w, xv


@pytest.mark.parametrize('skip', [True, False])
@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'mixed', 'bf16x3'])
def test_predict_vs_forward(H, mode, skip):
    """predict(latents).labels against argmax(forward(latents)[1]) under the label rule, with e_k from the tensor that enters
    decoder_scale_5 (a spy on decoder_scale_4's layer): the two paths contract the same operands, only the summation order
    differs.  bf16x3: forward contracts three-term split operands without the lo x lo products while the head runs plain fp32:
    2^-15 sum_c |w_kc x_c| is added to e_k.  forward's outputs before and after a predict call are bit-equal, no parameter gains a
    .grad, requires_grad flags stay; train and eval mode give the same labels."""
    from oracle import ess_oracle as O
    from ess_amd.models.style_networks import SemSegE2VID
    H.set_compute(mode)
    try:
        for K, (Hh, W), N in ((6, (64, 96), 2), (11, (64, 96), 1), (11, (440, 640), 1)):
            dec = SemSegE2VID(256, K, skip_connect=skip, skip_type='concat' if skip else 'sum').cuda()
            dec.load_state_dict(O.synth_state_dict(O.semseg_param_shapes(256, K, skip_connect=skip), 40 + K, decoder_style=True))
            lat = _latents(N, Hh, W, K)
            with torch.no_grad():
                logits0, last = forward_with_last(dec, lat)
            flags = [p.requires_grad for p in dec.parameters()]
            labels, colour, conf = dec.predict(lat, palette=palette_for(K).cuda(), want_confidence=True)
            dec.train()
            labels_t = dec.predict(lat)[0]
            dec.eval()
            with torch.no_grad():
                logits1 = dec(lat)[1]
            assert torch.equal(logits0, logits1)
            assert torch.equal(labels, labels_t)
            assert all(p.grad is None for p in dec.parameters()) and flags == [p.requires_grad for p in dec.parameters()]
            assert not labels.requires_grad and labels.dtype == torch.uint8 and tuple(labels.shape) == (N, Hh, W)
            z, e, w, xv = head_scores(H, dec, last, mode)
            zf = logits0.cpu().double()
            # forward's fp32 logits are themselves within e of the fp64 scores
            assert bool(((zf - z).abs() <= e).all()), (mode, skip, K, ((zf - z).abs() - e).max().item())
            check_labels(labels.cpu(), z, e, f'predict {mode} skip={skip} K={K} {Hh}x{W}')
            # ... and against forward's own argmax: equal wherever forward's top-two gap exceeds the two paths' bands
            fl = logits0.argmax(1).cpu()
            zs = zf.sort(1, descending=True).values
            band = 2 * e.gather(1, zf.argsort(1, descending=True)[:, :2]).sum(1)
            strict = (zs[:, 0] - zs[:, 1]) > band
            assert torch.equal(labels.cpu().long()[strict], fl[strict])
            assert torch.equal(colour.cpu(), palette_for(K)[labels.cpu().long()])
            ref = torch.softmax(z, 1).max(1).values
            assert (conf.cpu().double() - ref).abs().max().item() <= CONF_TOL + 2 * e.max().item()
    finally:
        H.set_compute('fp32')
