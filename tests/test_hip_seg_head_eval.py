"""GPU tier: the class head that scores itself (ess_seg_head_eval / hip.seg_head_eval / SemSegE2VID.predict(gt=, confusion=)).
Every check is an equality of bits or of integers: labels, colours and confidences are those of hip.seg_head on the same inputs
(one per-pixel code path), and the per-sample confusion matrix equals hip.label_confusion on the returned labels and a numpy
bincount.  Fixtures: tests/test_hip_seg_head.py's operands in the three source formats."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import test_hip_seg_head as SH  # noqa: E402  (operands, device formats, palette)

FMTS = SH.FMTS
KS = (1, 6, 11, 64)
CS = (8, 12, 32)  # (12: a tail block of 4 channels)
IGNORE = 255
GUARD = 64  # int64 words in front of and behind the confusion matrix
SENTINEL = 0x5A5A5A5A5A5A5A5A
BASE = 7  # what every cell of `confusion` holds before the first call: the kernel adds, it does not overwrite

# N = 3 on a 10 x 14 source, window (1, 2, 8, 10) resized to 13 x 17: 221 pixels a sample, fewer than one workgroup's 256, so a flat
# grid-stride loop over N * H_out * W_out would mix the samples of a workgroup's histogram
SMALL = dict(N=3, Hs=10, Ws=14, window=(1, 2, 8, 10), out_hw=(13, 17))
# N = 3 at 420 x 420: 529 200 pixels > 2048 * 256 = 524 288; per sample 176 400 > (2048 // 3 = 682) * 256 = 174 592: a second trip
LARGE = dict(N=3, Hs=420, Ws=420, window=None, out_hw=None)


@pytest.fixture(scope='module')
def H():
    from ess_amd import hip
    hip.lib()
    return hip


def ground_truth(N, K, Ho, Wo, seed, ignore=IGNORE):
    """uint8 [N, Ho, Wo]: 70 % classes below K, 15 % values >= K that are not the ignore value, 15 % ignore; sample 1 entirely ignore"""
    g = np.random.default_rng(seed)
    kind = g.random((N, Ho, Wo))
    gt = g.integers(0, K, (N, Ho, Wo))
    gt = np.where(kind > 0.70, K + g.integers(0, 3, (N, Ho, Wo)), gt)
    gt = np.where(kind > 0.85, ignore, gt)
    gt[1] = ignore
    return torch.from_numpy(gt.astype(np.uint8))


def guarded_confusion(N, K):
    buf = torch.full((2 * GUARD + N * K * K,), SENTINEL, dtype=torch.int64, device='cuda')
    cm = buf[GUARD:GUARD + N * K * K].view(N, K, K)
    cm.fill_(BASE)
    return buf, cm


def numpy_confusion(labels, gt, K, ignore=IGNORE):
    """[N, K, K] from uint8 labels and ground truth on the host"""
    out = []
    for lab, g in zip(labels.numpy().astype(np.int64), gt.numpy().astype(np.int64)):
        m = (g != ignore) & (g < K)
        out.append(np.bincount(g[m] * K + lab[m], minlength=K * K).reshape(K, K))
    return torch.from_numpy(np.stack(out))


def check_case(H, fmt, K, C, shape, seed, ignore=IGNORE):
    N, Hs, Ws, window, out_hw = (shape[k] for k in ('N', 'Hs', 'Ws', 'window', 'out_hw'))
    x, w, b = SH.make_operands(fmt, N, K, C, Hs, Ws, seed)
    xd = SH.to_device_format(x, fmt)
    wd, bd, pal = w.cuda(), b.cuda(), SH.palette_for(K).cuda()
    Ho, Wo = out_hw if out_hw is not None else (window[2], window[3]) if window is not None else (Hs, Ws)
    gt = ground_truth(N, K, Ho, Wo, seed + 1, ignore)
    gtd = gt.cuda()
    what = f'{fmt} K={K} C={C} {shape}'
    lab0, col0, conf0 = H.seg_head(xd, C, wd, bd, out_hw=out_hw, window=window, palette=pal, want_confidence=True)
    buf, cm = guarded_confusion(N, K)
    lab, col, conf = H.seg_head_eval(xd, C, wd, bd, gtd, cm, ignore_index=ignore, out_hw=out_hw, window=window, palette=pal,
                                     want_confidence=True)
    torch.cuda.synchronize()
    assert torch.equal(lab, lab0) and torch.equal(col, col0), f'{what}: labels / colours differ from seg_head'
    assert torch.equal(conf.view(torch.int32), conf0.view(torch.int32)), f'{what}: confidences differ from seg_head'
    first = (cm - BASE).cpu()
    want = numpy_confusion(lab.cpu(), gt, K, ignore)
    assert torch.equal(first, want), f'{what}: confusion != numpy bincount'
    for n in range(N):
        ref = torch.zeros(K, K, dtype=torch.int64, device='cuda')
        H.label_confusion(lab[n].long(), gtd[n].long(), ref, ignore)
        assert torch.equal(cm[n] - BASE, ref), f'{what}: sample {n} != hip.label_confusion'
        g = gt[n].long()
        countable = int(((g != ignore) & (g < K)).sum())
        assert int(first[n].sum()) == countable
        if n == 1:
            assert countable == 0 and not first[n].any(), f'{what}: the all-ignore sample moved its row'
            continue
        assert countable > g.numel() // 2
        assert bool((g == ignore).any()) and bool(((g >= K) & (g != ignore)).any())
        if K >= 6:
            assert len(lab[n].unique()) >= 4 and len(g[(g != ignore) & (g < K)].unique()) >= 4, f'{what}: sample {n} is too uniform a fixture'
    # a second call adds to the first; the words around the matrix keep their pre-fill
    H.seg_head_eval(xd, C, wd, bd, gtd, cm, ignore_index=ignore, out_hw=out_hw, window=window)
    torch.cuda.synchronize()
    assert torch.equal((cm - BASE).cpu(), 2 * want), f'{what}: the second call did not add'
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + N * K * K:] == SENTINEL).all()), f'{what}: guard words written'
    return lab


@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('fmt', FMTS)
def test_seg_head_eval_small_plane_several_samples(H, fmt, K, C):
    check_case(H, fmt, K, C, SMALL, 1000 * K + C)


@pytest.mark.parametrize('fmt', FMTS)
def test_seg_head_eval_second_trip_of_the_stride_loop(H, fmt):
    assert LARGE['N'] * 420 * 420 > 2048 * 256 and 420 * 420 > (2048 // LARGE['N']) * 256
    check_case(H, fmt, 11, 8, LARGE, 77)


def test_seg_head_eval_another_ignore_value(H):
    """ignore_index is an argument: with 3 as the ignore value class 3's ground truth is not counted, 255 is skipped as a value >= K"""
    lab = check_case(H, 'bf16', 11, 32, SMALL, 5, ignore=3)
    assert lab.dtype == torch.uint8


def test_predict_scores_itself(H):
    """SemSegE2VID.predict(gt=, confusion=): the labels, colours and confidences of predict() without them, and the matrix of those
    labels; one of the two alone is refused"""
    from oracle import ess_oracle as O
    from ess_amd.models.style_networks import SemSegE2VID
    K, Hh, W = 11, 64, 96
    dec = SemSegE2VID(256, K, skip_connect=True, skip_type='concat')
    dec.load_state_dict(O.synth_state_dict(O.semseg_param_shapes(256, K), 172, decoder_style=True))
    dec = dec.cuda().eval()
    lat = SH._latents(2, Hh, W, 3)
    pal = SH.palette_for(K).cuda()
    for mode in ('fp32', 'bf16', 'mixed'):
        H.set_compute(mode)
        try:
            plain = dec.predict(lat, palette=pal, want_confidence=True)
            gt = ground_truth(2, K, *plain[0].shape[1:], 9)
            gt[1] = gt[0].flip(0)  # (both samples scored here)
            cm = torch.zeros(2, K, K, dtype=torch.int64, device='cuda')
            got = dec.predict(lat, palette=pal, want_confidence=True, gt=gt.cuda(), confusion=cm)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
            assert torch.equal(got[2].view(torch.int32), plain[2].view(torch.int32))
            assert torch.equal(cm.cpu(), numpy_confusion(got[0].cpu(), gt, K)) and int(cm.sum()) > gt.numel() // 2
            with pytest.raises(H.EssHipError, match='gt and confusion come together'):
                dec.predict(lat, gt=gt.cuda())
        finally:
            H.set_compute('fp32')


def test_seg_head_eval_refusals(H):
    N, C, K = 2, 32, 11
    xd = torch.zeros(N, C, 4, 6, device='cuda')
    w, b = torch.zeros(K, C, device='cuda'), torch.zeros(K, device='cuda')
    gt = torch.zeros(N, 4, 6, dtype=torch.uint8, device='cuda')
    cm = torch.zeros(N, K, K, dtype=torch.int64, device='cuda')
    with pytest.raises(H.EssHipError, match='gt and confusion come together'):
        H.seg_head_eval(xd, C, w, b, gt, None)
    with pytest.raises(H.EssHipError, match='gt and confusion come together'):
        H.seg_head_eval(xd, C, w, b, None, cm)
    for bad in (gt.long(), gt[:1], gt[:, :3], gt.cpu(), torch.zeros(N, 6, 4, dtype=torch.uint8, device='cuda').transpose(1, 2)):
        with pytest.raises(H.EssHipError, match='seg_head_eval: gt must be'):
            H.seg_head_eval(xd, C, w, b, bad, cm)
    for bad in (cm.int(), cm[0], cm[:, :, :K - 1], cm.cpu(), torch.zeros(K, K, dtype=torch.int64, device='cuda')):
        with pytest.raises(H.EssHipError, match='seg_head_eval: confusion must be'):
            H.seg_head_eval(xd, C, w, b, gt, bad)
    assert not cm.any()
    # K = 64, C = 192: 49 600 bytes of weights, bias and palette fit the 64 KiB, the 16 384 of K x K counts on top do not
    K2, C2 = 64, 192
    x2 = torch.zeros(1, C2, 4, 6, device='cuda')
    w2, b2 = torch.zeros(K2, C2, device='cuda'), torch.zeros(K2, device='cuda')
    assert H.seg_head(x2, C2, w2, b2)[0].shape == (1, 4, 6)
    with pytest.raises(H.EssHipError, match=r'K=64 x C=192 weights and the K x K counts do not fit 64 KiB of LDS'):
        H.seg_head_eval(x2, C2, w2, b2, torch.zeros(1, 4, 6, dtype=torch.uint8, device='cuda'),
                        torch.zeros(1, K2, K2, dtype=torch.int64, device='cuda'))
    torch.cuda.synchronize()
