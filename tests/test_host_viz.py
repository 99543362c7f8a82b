"""CPU tier of the segmentation display (hip.viz_semseg, hip.viz_events, hip.viz_overlay; ess_amd/utils/viz_utils.py): the three C entry
points and their refusals, the wrappers' refusals -- each raised before a device call --, and the numpy restatement (tests/viz_ref.py)
that the GPU tier compares bits against: checked here against the reference's own outputs (tests/golden/viz.npz, written by
tests/golden/make_golden_viz.py), make_grid and panel against a brute-force placement loop, and shown to be sensitive to six mutations."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import viz_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ess_viz_semseg', 'ess_viz_events', 'ess_viz_overlay')
EINVAL = -22
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'viz.npz'))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_three_entry_points_are_exported_declared_and_bound_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
        assert getattr(hip.lib(), name).argtypes is not None, name
    assert hip.lib().ess_version() == 110
    assert 'ESS_VIZ_HISTOGRAM = 0, ESS_VIZ_SEPARATE_POL = 1, ESS_VIZ_SIGNED = 2' in header
    assert 'ESS_VIZ_LABELS_U8 = 0, ESS_VIZ_LABELS_I64 = 1' in header
    assert hip.VIZ_EVENT_MODES == {'histogram': 0, 'separate_pol': 1, 'signed': 2}
    assert [f[0] for f in hip.EssVizDst._fields_] == ['plane_stride', 'row_stride', 'tile_stride_y', 'tile_stride_x', 'tile0', 'tiles_per_row']
    assert callable(hip.viz_semseg) and callable(hip.viz_events) and callable(hip.viz_overlay)


def test_the_c_entry_points_refuse_before_any_launch(built_lib):
    """the pointers are host addresses that no kernel may touch: every call below returns EINVAL from the argument checks"""
    from ess_amd import hip
    L = hip.lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    H, W = 4, 8

    def dst(**kw):
        d = dict(plane_stride=H * W, row_stride=W, tile_stride_y=3 * H * W, tile_stride_x=0, tile0=0, tiles_per_row=1)
        d.update(kw)
        return ctypes.byref(hip.EssVizDst(**d))

    def ev(C, mode, d=None, n=1, elems=4096):
        return L.ess_viz_events(p, p, elems, d or dst(), n, C, H, W, mode, 0, None)
    assert ev(5, 1) == EINVAL and b'even' in L.ess_last_error()          # odd C with separate_pol
    assert ev(2, 1) == EINVAL                                            # C < 4 with separate_pol
    assert ev(3, 0) == EINVAL and b'C = 2' in L.ess_last_error()         # the histogram needs C = 2
    assert ev(3, 2) == EINVAL                                            # the signed tile needs C > 3
    assert ev(4, 3) == EINVAL                                            # no such mode
    assert ev(4, 1, elems=3 * H * W - 1) == EINVAL and b'reach' in L.ess_last_error()   # one element short
    assert ev(4, 1, n=2, elems=2 * 3 * H * W - 1) == EINVAL
    assert ev(4, 1, dst(row_stride=W - 1)) == EINVAL
    assert ev(4, 1, dst(tiles_per_row=0)) == EINVAL
    assert ev(4, 1, dst(tile0=-1)) == EINVAL
    assert L.ess_viz_events(None, p, 4096, dst(), 1, 4, H, W, 1, 0, None) == EINVAL
    assert L.ess_viz_semseg(p, 2, p, p, 4096, dst(), 1, 6, H, W, 255, None) == EINVAL   # no such label type
    assert L.ess_viz_semseg(p, 0, p, p, 4096, dst(), 1, 0, H, W, 255, None) == EINVAL   # K = 0
    assert L.ess_viz_semseg(p, 0, p, p, 4096, None, 1, 6, H, W, 255, None) == EINVAL    # no destination
    assert L.ess_viz_semseg(p, 0, p, p, 95, dst(), 1, 6, H, W, 255, None) == EINVAL
    for alpha in (-0.01, 1.01, float('nan')):
        assert L.ess_viz_overlay(p, p, p, p, 1, 6, H, W, alpha, None) == EINVAL and b'alpha' in L.ess_last_error()
    assert L.ess_viz_overlay(p, p, p, p, 1, 257, H, W, 0.5, None) == EINVAL
    assert L.ess_viz_overlay(p, None, p, p, 1, 6, H, W, 0.5, None) == EINVAL


def test_the_wrappers_refuse_before_a_device_call():
    """CPU tensors throughout: a malformed argument is named first, whatever memory it lies in; a well-formed CPU tensor is refused as
    such"""
    from ess_amd import hip
    from ess_amd.utils import viz_utils
    E = hip.EssHipError
    z = torch.zeros
    with pytest.raises(E, match='even C'):
        hip.viz_events(z(1, 5, 4, 8), 'separate_pol')
    with pytest.raises(E, match='even C'):
        viz_utils.visualizeVoxelGrid(z(1, 7, 4, 8))
    with pytest.raises(E, match='C = 2'):
        hip.viz_events(z(1, 3, 4, 8), 'histogram')
    with pytest.raises(E, match='C > 3'):
        hip.viz_events(z(1, 3, 4, 8), 'signed')
    with pytest.raises(E, match='mode'):
        hip.viz_events(z(1, 4, 4, 8), 'polarity')
    with pytest.raises(E, match='fp32'):
        hip.viz_events(z(1, 4, 4, 8, dtype=torch.float64), 'signed')
    u8 = lambda *s: z(*s, dtype=torch.uint8)  # noqa: E731
    for alpha in (-0.1, 1.5, float('nan')):
        with pytest.raises(E, match='alpha'):
            hip.viz_overlay(u8(1, 4, 8), u8(1, 4, 8), u8(6, 3), alpha)
    with pytest.raises(E, match='differ in size'):
        hip.viz_overlay(u8(1, 4, 8), u8(1, 4, 9), u8(6, 3), 0.5)
    with pytest.raises(E, match='palette'):
        hip.viz_overlay(u8(1, 4, 8), u8(1, 4, 8), u8(6, 4), 0.5)
    with pytest.raises(E, match='labels'):
        hip.viz_semseg(z(1, 4, 8), z(6, 3))
    with pytest.raises(E, match='colours'):
        hip.viz_semseg(u8(1, 4, 8), z(6, 4))
    with pytest.raises(E, match='leave the'):
        hip.viz_semseg(u8(2, 4, 8), z(6, 3), dst=(z(3, 8, 22), 1, 2, 2))  # slots 1 and 2 of a one-row grid of two
    with pytest.raises(E, match='exclude'):
        hip.viz_semseg(u8(2, 4, 8), z(6, 3), out=z(2, 3, 4, 8), dst=(z(3, 14, 22), 0, 2, 2))
    # well-formed, but on the CPU
    for call in (lambda: hip.viz_events(z(1, 4, 4, 8), 'separate_pol'), lambda: hip.viz_events(z(1, 2, 4, 8), 'histogram'),
                 lambda: hip.viz_semseg(u8(1, 4, 8), z(6, 3)), lambda: hip.viz_semseg(u8(2, 4, 8), z(6, 3), dst=(z(3, 14, 22), 0, 2, 2)),
                 lambda: hip.viz_overlay(u8(1, 4, 8), u8(1, 4, 8), u8(6, 3), 0.5),
                 lambda: viz_utils.prepare_semseg(z(1, 4, 8, dtype=torch.int64), [[0, 0, 0], [255, 0, 0]], 255),
                 lambda: viz_utils.panel([('gray', z(2, 1, 4, 8)), ('events', z(2, 4, 4, 8))])):
        with pytest.raises(E, match='no CPU path'):
            call()
    with pytest.raises(E, match='color_map'):
        viz_utils.panel([('semseg', z(2, 4, 8, dtype=torch.int64))])
    with pytest.raises(E, match='differ in size'):
        viz_utils.panel([('gray', z(2, 1, 4, 8)), ('gray', z(2, 1, 4, 9))])
    with pytest.raises(E, match='kind'):
        viz_utils.panel([('grey', z(2, 1, 4, 8))])


def test_the_colour_table_rule():
    """divide by 255, in fp32, if the maximum exceeds 128 -- on the host for a host map"""
    from ess_amd import hip
    pal = V.palette_u8(11)
    t = hip.viz_colour_table(pal.tolist(), torch.device('cpu'))
    assert t.dtype == torch.float32 and _same_bits(t.numpy(), V.colour_table(pal)) and float(t.max()) <= 1.0
    small = (pal.astype(np.float32) / np.float32(512))
    assert _same_bits(hip.viz_colour_table(small, torch.device('cpu')).numpy(), small)
    assert hip.viz_colour_table(pal.tolist(), torch.device('cpu')) is t  # (uploaded once per content)
    with pytest.raises(hip.EssHipError):
        hip.viz_colour_table([[1, 2]], torch.device('cpu'))


# ---------------------------------------------------------------------------------------------- the restatement against the reference
def test_semseg_checkerboard_and_histogram_equal_the_reference_bit_for_bit():
    for i in range(4):
        lab, cmap, want = GOLD[f'semseg{i}_labels'], GOLD[f'semseg{i}_cmap'], GOLD[f'semseg{i}_out']
        assert (lab == V.IGNORE).any() and (lab == cmap.shape[0] - 1).any()
        assert _same_bits(V.semseg(lab, V.colour_table(cmap)), want), i
    assert GOLD['semseg0_cmap'].max() > 128 and GOLD['semseg3_cmap'].max() <= 128  # (both sides of the colour rule)
    for i in range(4):
        N, C, H, W = GOLD[f'board{i}_shape']
        want = GOLD[f'board{i}_out']
        assert _same_bits(np.broadcast_to(V.checkerboard(H, W), (N, C, H, W)), want), i
        # ... and as the tile of an all-ignore label map
        assert _same_bits(V.semseg(np.full((N, H, W), V.IGNORE), np.zeros((1, 3), np.float32))[:, :C], want[:, :min(C, 3)]), i
    for i in range(2):
        assert _same_bits(V.events(GOLD[f'hist{i}_in'], 'histogram'), GOLD[f'hist{i}_out']), i
        assert GOLD[f'hist{i}_in'].max() > 1  # (the clamp binds)
    assert GOLD['hist0_in'].min() < 0


def test_signed_and_power_of_two_polarity_tiles_equal_the_reference_bit_for_bit():
    """integer-valued grids, half a power of two: every product and sum is exact, so the summation order cannot show"""
    for i in range(3):
        x = GOLD[f'pol_exact{i}_in']
        assert (x == np.round(x)).all() and (x.shape[1] // 2) in (2, 4, 8)
        pos, neg = V.polarity_sums(x)
        assert _same_bits(pos, GOLD[f'pol_exact{i}_pos']) and _same_bits(neg, GOLD[f'pol_exact{i}_neg']), i
        assert _same_bits(V.events(x, 'separate_pol'), GOLD[f'pol_exact{i}_out']), i
    for i in range(2):
        x = GOLD[f'signed{i}_in']
        want = GOLD[f'signed{i}_out']
        assert _same_bits(V.events(x, 'signed'), want), i
        assert (want[:, 0] == 255).any() and (want[:, 2] == 255).any() and (x.sum(1) == 0).any()
        assert _same_bits(V.events(x, 'signed', unit=True), np.clip(want, 0, 1)), i


def test_polarity_tiles_with_half_3_and_5_within_the_summation_bound():
    """torch's CPU sum over the channels is not the sequential order (last-bit differences on random data), so the comparison is
    bounded by the standard summation bound applied to both sides.  A term x_c t_c passes through at most n = half + 1 roundings (the
    scale's division, its product, at most half - 1 sums), each at most 2^-24 relative, so either side is within n 2^-24 sum |x_c t_c| of
    the exact sum (to first order) and the two sides within twice that of each other.  Derived, not measured.  The clamp is 1-Lipschitz,
    so the same bound holds after it."""
    for i in range(2):
        x = GOLD[f'pol_rounded{i}_in'].astype(np.float64)
        half = x.shape[1] // 2
        assert half in (3, 5)
        t = (np.arange(1, half + 1) / half)[None, :, None, None]
        pos, neg = V.polarity_sums(GOLD[f'pol_rounded{i}_in'])
        worst = 0.0
        for mine, ref, part in ((pos, GOLD[f'pol_rounded{i}_pos'], x[:, :half]), (neg, GOLD[f'pol_rounded{i}_neg'], x[:, half:])):
            bound = 2 * (half + 1) * 2.0 ** -24 * np.abs(part * t).sum(1)
            err = np.abs(mine.astype(np.float64) - ref.astype(np.float64))
            assert (err <= bound).all(), (i, float((err - bound).max()))
            worst = max(worst, float(err.max()))
        print(f'half = {half}: max |restatement - torch| before the clamp {worst:.3e}')
        out, want = V.events(GOLD[f'pol_rounded{i}_in'], 'separate_pol'), GOLD[f'pol_rounded{i}_out']
        b_neg = 2 * (half + 1) * 2.0 ** -24 * np.abs(x[:, half:] * t).sum(1)
        b_pos = 2 * (half + 1) * 2.0 ** -24 * np.abs(x[:, :half] * t).sum(1)
        assert (np.abs(out[:, 0].astype(np.float64) - want[:, 0]) <= b_neg).all()
        assert (np.abs(out[:, 1].astype(np.float64) - want[:, 1]) <= b_pos).all()
        assert (out[:, 2] == 0).all() and (want[:, 2] == 0).all()
        assert out.min() >= 0 and out.max() <= 1 and (out == 1).any() and (out == 0).any()


# ---------------------------------------------------------------------------------------------- make_grid and panel
def _brute_grid(t, nrow, padding=2):
    n, C, H, W = t.shape
    if n == 1:
        return t[0]
    xmaps = min(nrow, n)
    ymaps = (n + xmaps - 1) // xmaps
    out = np.zeros((C, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), np.float32)
    for k in range(n):
        for c in range(C):
            for y in range(H):
                for x in range(W):
                    out[c, (k // xmaps) * (H + padding) + padding + y, (k % xmaps) * (W + padding) + padding + x] = t[k, c, y, x]
    return out


@pytest.mark.parametrize('n,nrow', [(1, 8), (3, 8), (4, 4), (6, 4), (9, 4), (5, 2)])
def test_make_grid_against_the_placement_loop(n, nrow):
    """n = 1 (unpadded), n < nrow, n a multiple of xmaps and not (empty slots zero) -- the restatement and viz_utils.make_grid (torch,
    here on the CPU)"""
    from ess_amd.utils import viz_utils
    H, W = 3, 5
    t = np.random.default_rng(n).random((n, 3, H, W)).astype(np.float32) + 1
    want = _brute_grid(t, nrow)
    assert want.shape == ((3, H, W) if n == 1 else (3, -(-n // min(nrow, n)) * (H + 2) + 2, min(nrow, n) * (W + 2) + 2))
    assert _same_bits(V.make_grid(t, nrow=nrow), want)
    assert _same_bits(viz_utils.make_grid(torch.from_numpy(t), nrow=nrow).numpy(), want)
    if n > 1:
        assert int((want == 0).sum()) == want.size - n * 3 * H * W  # (padding and empty slots are zero, nothing else)
        assert _same_bits(viz_utils.make_grid(torch.from_numpy(t), nrow=nrow, pad_value=0.5).numpy(), np.where(want == 0, np.float32(0.5), want))
    assert _same_bits(viz_utils.make_grid(torch.from_numpy(t[:, :1]), nrow=nrow).numpy(), _brute_grid(np.repeat(t[:, :1], 3, 1), nrow))
    assert V.grid_slot(n - 1, min(nrow, n), H, W) == (((n - 1) // min(nrow, n)) * (H + 2) + 2, ((n - 1) % min(nrow, n)) * (W + 2) + 2)


@pytest.mark.parametrize('B', [1, 2, 5])
def test_panel_restatement_against_the_placement_loop(B):
    """the trainers' layouts: B = 2 with three and more rows and nrow = 4 puts tiles of different rows into one grid row; B = 5
    contributes 4 samples per row; B = 1 with one row is a single unpadded image"""
    lay = V.trainer_layouts(B)
    col = V.colour_table(V.palette_u8(6))
    for name, rows in lay.items():
        tiles = np.concatenate([V.tiles(k, np.asarray(a)[:4], col) for k, a in rows], 0)
        assert tiles.shape[0] == len(rows) * min(B, 4)
        assert _same_bits(V.panel(rows, 4, col), _brute_grid(tiles, 4)), name
    if B == 2:
        got = V.panel(lay['ess_sensor_a'], 4, col)   # 6 tiles, 4 per grid row: the second semseg row straddles the two grid rows
        assert got.shape == (3, 2 * 18 + 2, 4 * 26 + 2)
        assert _same_bits(got[:, 2:18, 2 + 3 * 26:2 + 3 * 26 + 24], V.semseg(lay['ess_sensor_a'][1][1][1:2], col)[0])
        assert (got[:, 20:36, 2 + 2 * 26:] == 0).all()   # the two empty slots
    if B == 1:
        one = V.panel([lay['ess_sensor_a'][1]], 4, col)
        assert one.shape == (3, 16, 24)
    # the signed event row is the unit form of the reference's tile: createRGBImage(separate_pol=False).clamp(0, 1)
    ev = lay['ess_sensor_b_signed_no_gt'][0][1]
    assert _same_bits(V.tiles('events_signed', ev), np.clip(V.events(ev, 'signed'), 0, 1))
    assert _same_bits(V.tiles('events', ev), V.events(ev, 'separate_pol'))
    assert _same_bits(V.tiles('events', ev[:, :2]), V.events(ev[:, :2], 'histogram'))
    assert _same_bits(V.tiles('events_signed', ev[:, :2]), V.events(ev[:, :2], 'histogram'))


# ---------------------------------------------------------------------------------------------- sensitivity
def _gpu_tier_outputs(mutate=None):
    """the restatement on (a subset of) the GPU tier's inputs, under a mutation"""
    out = []
    for (H, W) in V.SIZES:
        lab = V.labels_case(1, H, W, 6, H)
        out.append(V.semseg(lab, V.colour_table(V.palette_u8(6)), mutate=mutate))
        out.append(V.events(V.event_case(1, 6, H, W, W), 'separate_pol', mutate=mutate))
        out.append(V.events(V.signed_case(1, 5, H, W, W + 1), 'signed', mutate=mutate))
        for a in V.ALPHAS:
            out.append(V.overlay(lab, V.gray_case(1, H, W, H + 1), V.palette_u8(6), a, mutate=mutate))
    return out


@pytest.mark.parametrize('mutation', ['parity', 'cell_from_max', 'swap_polarity', 'scale_from_c', 'ge_zero', 'truncate'])
def test_the_restatement_is_sensitive(mutation):
    """checkerboard parity flipped; cell from max(H, W); neg and pos swapped; c / half in place of (c + 1) / half; >= 0 in place of > 0 in
    the signed tile; truncation without the + 0.5 in the overlay: each changes at least one case's bits"""
    base, mut = _gpu_tier_outputs(), _gpu_tier_outputs(mutation)
    changed = [a.tobytes() != b.tobytes() for a, b in zip(base, mut)]
    assert any(changed), mutation
    if mutation == 'cell_from_max':  # (only where max(H, W) // 32 differs from min(H, W) // 32: not at 5 x 7)
        assert not changed[0] and any(changed[1:])
