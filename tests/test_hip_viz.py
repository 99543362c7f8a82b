"""GPU tier of the segmentation display: ess_viz_semseg, ess_viz_events and ess_viz_overlay against the numpy float32 restatement
(tests/viz_ref.py; checked against the reference's outputs by the CPU tier) BIT for bit, into poisoned outputs (0xFF bytes for uint8,
NaN for fp32 -- the convention of test_hip_seg_head.py) so that an element left out or written outside a tile shows; and
viz_utils.panel on the validation layouts of the two trainers against viz_ref.panel.  No library convolution runs on the device here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import viz_ref as V  # noqa: E402

DEV = 'cuda'


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _poisoned_f32(shape, lead):
    """an fp32 view of `shape` inside a NaN buffer, `lead` elements in (lead = 1: no 16-byte store is possible), guard elements behind"""
    n = int(np.prod(shape))
    buf = torch.full((lead + n + 8,), float('nan'), device=DEV)
    return buf, buf[lead:lead + n].view(*shape)


def _guards_intact(buf, lead, n):
    h = buf.cpu().numpy()
    return np.isnan(h[:lead]).all() and np.isnan(h[lead + n:]).all()


@pytest.mark.parametrize('H,W', V.SIZES, ids=[f'{h}x{w}' for h, w in V.SIZES])
def test_semseg_tile_equals_the_restatement_bit_for_bit(H, W):
    """N = 1 / 3 / 5 with K = 6 / 11 / 19, uint8 and int64 labels holding 255 (ignore), K (out of range: the checkerboard too) and K - 1,
    the output 16-byte aligned and one element off; nothing outside the output is written"""
    from ess_amd import hip
    for (N, K) in V.NK:
        col = V.colour_table(V.palette_u8(K))
        for dtype in (np.uint8, np.int64):
            lab = V.labels_case(N, H, W, K, H + N, dtype)
            assert (lab == 255).any() and (lab == K).any() and (lab == K - 1).any()
            if dtype == np.int64:
                lab.reshape(-1)[2] = -1
                lab.reshape(-1)[3] = 2 ** 40
            want = V.semseg(lab, col)
            for lead in (4, 1):
                buf, out = _poisoned_f32((N, 3, H, W), lead)
                got = hip.viz_semseg(torch.from_numpy(lab).to(DEV), torch.from_numpy(col).to(DEV), 255, out=out)
                assert got is out
                assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (N, K, dtype, lead)
                assert _guards_intact(buf, lead, out.numel())
    # labels one byte off a 4-byte boundary (no 4-byte label load), and another ignore label
    lab = V.labels_case(2, H, W, 6, 77)
    col = V.colour_table(V.palette_u8(6))
    raw = torch.zeros(lab.size + 1, dtype=torch.uint8, device=DEV)
    raw[1:].copy_(torch.from_numpy(lab.reshape(-1)))
    got = hip.viz_semseg(raw[1:].view(2, H, W), torch.from_numpy(col).to(DEV), 255)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(V.semseg(lab, col)))
    got = hip.viz_semseg(torch.from_numpy(lab).to(DEV), torch.from_numpy(col).to(DEV), 3)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(V.semseg(lab, col, ignore=3)))


@pytest.mark.parametrize('H,W', V.SIZES, ids=[f'{h}x{w}' for h, w in V.SIZES])
def test_event_tiles_equal_the_restatement_bit_for_bit(H, W):
    """the histogram (C = 2), separate_pol at C = 4 / 6 / 10, signed at C = 5 with pixels that cancel to exactly 0 and pixels of -0.0,
    255 and the unit mark; N = 1 / 3 / 5; aligned and one element off"""
    from ess_amd import hip
    cases = [('histogram', V.histogram_case(3, H, W, 1), False)]
    cases += [('separate_pol', V.event_case(n, C, H, W, C + n), False) for C, n in zip(V.POL_CHANNELS, (1, 3, 5))]
    sg = V.signed_case(3, 5, H, W, 9)
    assert (sg[:, :, 0, 0].sum(1) == 0).all() and np.signbit(sg[:, :, 0, 1]).all()
    cases += [('signed', sg, False), ('signed', sg, True)]
    for mode, x, unit in cases:
        want = V.events(x, mode, unit=unit)
        N = x.shape[0]
        for lead in (4, 1):
            buf, out = _poisoned_f32((N, 3, H, W), lead)
            hip.viz_events(torch.from_numpy(x).to(DEV), mode, unit=unit, out=out)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (mode, x.shape, unit, lead)
            assert _guards_intact(buf, lead, out.numel())
    s = V.events(sg, 'signed')
    assert (s[:, :, 0, 0] == 0).all() and (s[:, :, 0, 1] == 0).all() and (s[:, 0, 0, 2] == 255).all() and (s[:, 2, 0, 3] == 255).all()
    # the input one element off a 16-byte boundary
    x = V.event_case(2, 4, H, W, 5)
    raw = torch.zeros(x.size + 1, device=DEV)
    raw[1:].copy_(torch.from_numpy(x.reshape(-1)))
    got = hip.viz_events(raw[1:].view(2, 4, H, W), 'separate_pol')
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(V.events(x, 'separate_pol')))


@pytest.mark.parametrize('H,W', V.SIZES, ids=[f'{h}x{w}' for h, w in V.SIZES])
def test_overlay_equals_the_restatement_bit_for_bit(H, W):
    """alpha 0 / 0.5 / 0.6 / 1, labels holding 255 and K (>= K: the gray value), the output 4-byte aligned and one byte off; the bytes
    around the output stay 0xFF"""
    from ess_amd import hip
    for (N, K) in V.NK:
        lab, gray, pal = V.labels_case(N, H, W, K, H + K), V.gray_case(N, H, W, W + K), V.palette_u8(K)
        n = N * H * W * 3
        for alpha in V.ALPHAS:
            want = V.overlay(lab, gray, pal, alpha)
            for lead in (4, 1):
                buf = torch.full((lead + n + 8,), 0xFF, dtype=torch.uint8, device=DEV)
                out = buf[lead:lead + n].view(N, H, W, 3)
                got = hip.viz_overlay(torch.from_numpy(lab).to(DEV), torch.from_numpy(gray).to(DEV), torch.from_numpy(pal).to(DEV), alpha, out=out)
                assert got is out and np.array_equal(out.cpu().numpy(), want), (N, K, alpha, lead)
                h = buf.cpu().numpy()
                assert (h[:lead] == 0xFF).all() and (h[lead + n:] == 0xFF).all()
        assert np.array_equal(V.overlay(lab, gray, pal, 0.0), np.repeat(gray[..., None], 3, -1))
        inside = lab < K
        assert np.array_equal(V.overlay(lab, gray, pal, 1.0)[inside], pal[lab[inside]])


@pytest.mark.parametrize('lead', [4, 1])
def test_tiles_written_into_panel_slots_leave_the_gaps_poisoned(lead):
    """5 tiles of 33 x 70 into slots 2 .. 6 of a 3-per-row grid inside a NaN buffer (row stride 3 * 72 + 2 = 218: no multiple of 4): the
    tiles hold the restatement's bits, every other element of the panel -- padding, slots 0, 1, 7, 8 -- and the guards stay NaN"""
    from ess_amd import hip
    H, W, N, xmaps, pad, tile0 = 33, 70, 5, 3, 2, 2
    Hg, Wg = 3 * (H + pad) + pad, xmaps * (W + pad) + pad
    lab = V.labels_case(N, H, W, 11, 5)
    col = V.colour_table(V.palette_u8(11))
    x = V.event_case(N, 6, H, W, 6)
    for which, want in (('semseg', V.semseg(lab, col)), ('events', V.events(x, 'separate_pol'))):
        buf, panel = _poisoned_f32((3, Hg, Wg), lead)
        if which == 'semseg':
            hip.viz_semseg(torch.from_numpy(lab).to(DEV), torch.from_numpy(col).to(DEV), 255, dst=(panel, tile0, xmaps, pad))
        else:
            hip.viz_events(torch.from_numpy(x).to(DEV), 'separate_pol', dst=(panel, tile0, xmaps, pad))
        expect = np.full((3, Hg, Wg), np.nan, np.float32)
        for n in range(N):
            y0, x0 = V.grid_slot(tile0 + n, xmaps, H, W, pad)
            expect[:, y0:y0 + H, x0:x0 + W] = want[n]
        assert np.array_equal(_bits(panel.cpu().numpy()), _bits(expect)), which
        assert _guards_intact(buf, lead, panel.numel())


def test_viz_utils_equal_the_restatement_and_keep_the_reference_shapes():
    from ess_amd.utils import viz_utils as U
    H, W, K = 33, 70, 11
    pal = V.palette_u8(K)
    lab = V.labels_case(2, H, W, K, 3, np.int64)
    got = U.prepare_semseg(torch.from_numpy(lab).to(DEV), pal.tolist(), 255)
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(V.semseg(lab, V.colour_table(pal))))
    got4 = U.prepare_semseg(torch.from_numpy(lab).to(DEV).unsqueeze(1), torch.from_numpy(pal).to(DEV), 255)  # (a device colour map)
    assert torch.equal(got, got4)
    assert np.array_equal(_bits(U.create_checkerboard(2, 3, 97, 65).cpu().numpy()), _bits(np.broadcast_to(V.checkerboard(97, 65), (2, 3, 97, 65))))
    ev = V.event_case(2, 6, H, W, 4)
    t = torch.from_numpy(ev).to(DEV)
    for sep, mode in ((True, 'separate_pol'), (False, 'signed')):
        assert np.array_equal(_bits(U.createRGBImage(t, separate_pol=sep).cpu().numpy()), _bits(V.events(ev, mode)))
    assert np.array_equal(_bits(U.visualizeTensors(t[:, :2]).cpu().numpy()), _bits(V.events(ev[:, :2], 'histogram')))
    assert U.createRGBImage(t[:, :3]) is not None and tuple(U.createRGBImage(t[:, :1]).shape) == (2, 3, H, W)
    grid = U.createRGBGrid([t, t[:, :1]], nrow=3)
    want = V.make_grid(np.concatenate([V.events(ev, 'separate_pol'), np.repeat(ev[:, :1], 3, 1)], 0), nrow=3)
    assert np.array_equal(_bits(grid.cpu().numpy()), _bits(want))


@pytest.mark.parametrize('B', [2, 5])
def test_panel_on_the_trainers_validation_layouts(B):
    """the four validation layouts at 16 x 24 tiles: viz_utils.panel == viz_ref.panel bit for bit (B = 2: tiles of different rows share a
    grid row, the row stride 4 * 26 + 2 = 106 or less; B = 5: the first four samples of every row)"""
    from ess_amd.utils import viz_utils as U
    pal = V.palette_u8(6)
    col = V.colour_table(pal)
    for name, rows in V.trainer_layouts(B).items():
        got = U.panel([(k, torch.from_numpy(np.asarray(a)).to(DEV)) for k, a in rows], nrow=4, color_map=pal.tolist(), ignore_label=255)
        want = V.panel(rows, 4, col)
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32, name
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (name, B)
    one = U.panel([('semseg', torch.from_numpy(V.labels_case(1, 16, 24, 6, 1)).to(DEV))], color_map=pal.tolist())
    assert tuple(one.shape) == (3, 16, 24)  # (a single image comes back unpadded, as from make_grid)
