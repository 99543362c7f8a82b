"""CPU tier: teeth for the checker of tests/test_hip_dgrad_edges.py.  For every row of its table, on the row's own shapes and seeded
inputs: an fp32 torch-CPU data gradient computed the way the kernel computes it (a stride-1 convolution of dy -- zero-inserted for a
stride-2 row -- with the flipped, transposed weights; pooled, split, skip-added, rounded to bf16 as the row says: a stand-in for a correct
kernel) passes dgrad_ref.check against the float64 autograd reference, and the same with ONE pixel of dy dropped -- all its channels, at
the last row and column of the last sample, where partial tiles live -- fails it by at least ten times the bound; for a zero-inserted
row so does ONE hole read as data.  A row too large or too benign for that would let a kernel lose a pixel unnoticed.  The rows' labels
(kernel, channel tile, chunk, epilogue selection, wide-tile pick) are checked against the library's planner, which runs without a GPU,
and the planner's refusals of malformed data-gradient descriptors are checked here too."""
import ctypes
import os
import sys

import pytest

from dgrad_ref import (BF16, C8, F16, NCHW, Case, case_inputs, case_reference, check, dgrad_fp32_standin, dgrad_reference, excess,
                       kernel_operands, restated, virtual_source, wide_pick)
from test_hip_dgrad_edges import CASE_IDS, DGRAD_EDGE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def hip():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_library(verbose=False)
    from ess_amd import hip
    hip.lib()
    return hip


def _teeth_case(row):
    """the row, its inputs and its float64 reference; pool_persistent on a cropped copy (same id, seed and channels: a persistent tile
    walk is a property of the launch, not of the checker)"""
    if row[0] == 'pool_persistent':
        c = Case(row).cropped(34, 38)
        dy, w, r = case_inputs(c)
        return c, (dy, w, r), dgrad_reference(c, *kernel_operands(c, dy, w), r)
    return case_reference(row)


@pytest.mark.parametrize('row', DGRAD_EDGE_CASES, ids=CASE_IDS)
def test_bound_passes_fp32_and_notices_one_dropped_pixel(row):
    c, (dy, w, r), refs = _teeth_case(row)
    dy_op, w_op = kernel_operands(c, dy, w)
    src = virtual_source(c, dy_op)
    good = dgrad_fp32_standin(c, src, w_op, r)
    cut = dy_op.clone()
    cut[-1, :, -1, -1] = 0
    mutants = [('one dropped pixel', dgrad_fp32_standin(c, virtual_source(c, cut), w_op, r))]
    if c.s == 2:  # one hole of the zero-inserted source read as data: an odd virtual position takes its even neighbour's value
        holed = src.clone()
        holed[-1, :, -1, -2] = holed[-1, :, -2, -2]
        assert (src[-1, :, -1, -2] == 0).all() and (src[-1, :, -2, -2] != 0).any()
        mutants.append(('one hole read as data', dgrad_fp32_standin(c, holed, w_op, r)))
    for j, name in enumerate(('first', 'second')):
        if refs[j] is None:
            assert good[j] is None
            continue
        e = check(good[j], refs[j], c.kind, f'{c.id} {name} output (fp32 stand-in)')
        line = f'{c.id} {name}: fp32 stand-in at {e:.3f} of the bound'
        for what, bad in mutants:
            m = excess(bad[j], refs[j], c.kind)
            line += f', {what} at {m:.1f}'
            assert m >= 10.0, (c.id, name, what, m)
            with pytest.raises(AssertionError):
                check(bad[j], refs[j], c.kind)
        print(line)


def _lds_bytes(c, want):
    """make_plan's lds_bytes from the restated tile geometry (choose_geom's row pitch rules, stride 1): ties the restated geometry to
    the planner's"""
    bwl, wxl, TW, TH, _, _ = want['geom']
    BW, IH, IW, ck, cot = 1 << bwl, TH - 1 + c.k, TW - 1 + c.k, want['ck'], want['cout_tile']
    rp = IW
    if c.compute == BF16:
        if BW == 16:
            rp = (rp + 15) & ~15
        if BW == 8:
            while (rp & 15) != 8:
                rp += 1
        return ((ck // 8) * IH * rp + c.k * c.k * (ck // 8) * cot) * 16
    if BW < 32:
        while (rp & 31) != BW:
            rp += 1
    return (ck * ((IH * rp + 3) & ~3) + c.k * c.k * ck * cot) * 4


@pytest.mark.parametrize('row', DGRAD_EDGE_CASES, ids=CASE_IDS)
def test_row_labels_restate_the_planner(hip, row):
    c = Case(row)
    cus = hip.tuning_get('device_cus')
    want = restated(c, cus)
    assert want['label'] == c.label, (c.id, want['label'])
    args, kw = c.spec_args()
    spec = hip.conv_spec(*args, **kw)
    assert (spec.H_out, spec.W_out) == (c.Hv, c.Wv)
    pl = hip.EssConvPlan()
    fmt = lambda f: hip.FMT_BF16_C8 if f == C8 else hip.FMT_F32_NCHW  # noqa: E731
    d = spec.desc_fmt(fmt(c.dyfmt), fmt(c.outfmt), fmt(c.outfmt) if c.skip else hip.FMT_F32_NCHW)
    assert hip.lib().ess_conv2d_plan(ctypes.byref(d), ctypes.byref(pl)) == 0, (c.id, hip.lib().ess_last_error())
    assert (pl.cout_tile, pl.ck, pl.n_cout_tiles) == (want['cout_tile'], want['ck'], want['n_cout_tiles']), c.id
    assert pl.n_chunks == -(-c.Cout // pl.ck) and pl.rows_padded == pl.n_cout_tiles * pl.cout_tile
    assert pl.lds_bytes == _lds_bytes(c, want), (c.id, want['geom'], pl.lds_bytes)
    # the epilogue selection follows from the restated conditions of conv_epilogue_c8_sel on the row's own columns
    rows, cot, bwl = c.Cin, pl.cout_tile, want['geom'][0]
    if c.outfmt == C8 and not want['kernel'].startswith('wide'):
        dgrad = (c.pool or c.split > 0) and not c.skip and (c.split & 15) == 0 and rows % cot == 0 and (not c.pool or bwl == 5)
        plain = c.split == 0 and not c.pool and rows % cot == 0
        assert want['epilogue'].startswith('dgrad') == bool(dgrad), c.id
        assert want['epilogue'].startswith('plain') == bool(plain and not dgrad), c.id
        assert want['epilogue'].startswith('general') == (not dgrad and not plain), c.id
        assert ('<pool>' in want['epilogue']) == bool(dgrad and c.pool) and ('<res>' in want['epilogue']) == bool(plain and c.skip), c.id
    if c.pool:  # 32-wide pixel blocks are forced from 32 columns on; below, the geometry is free
        assert (bwl == 5) or c.Wv < 32, c.id
        assert ('rows1' in c.label or 'dgrad<pool>' in c.label) == (bwl == 5) and ('lanes' in c.label) == (bwl != 5), (c.id, want['geom'])
    # wide rows: wide_pick names a candidate, and the launch satisfies the wide-tile kernel's epilogue forms
    if c.wide == 2:
        pick = wide_pick(c, pl.cout_tile, cus)
        assert pick is not None and c.label.startswith(f'wide<{pick[0]},{pick[1]}>'), (c.id, pick)
        assert c.Cin % (pick[0] * pick[1] * 32) == 0 and (not c.split or (c.split % (pick[0] * 32) == 0 and not c.skip)), c.id
    else:
        assert not c.label.startswith('wide'), c.id
    if 'persistent' in c.label:
        assert want['tiles'] > 2 * cus, (c.id, want['tiles'])
    print(f"{c.id}: {want['label']}  tile {want['geom'][2]} x {want['geom'][3]} (bwl {bwl}), {want['tiles']} tiles, "
          f"cout_tile {pl.cout_tile}, ck {pl.ck}, {pl.n_chunks} chunks, {pl.n_cout_tiles} channel tiles")


def test_table_covers_every_form():
    """every data-gradient form of Conv2dFn.backward has a row: each epilogue of a BF16_C8 output, both pooled pairings, both compute
    types of the fp32 NCHW form, zero-inserted sources on 3x3 and 1x1, both chunk widths of the 1x1 kernel, 32 / 64 / 128-row tiles"""
    labels = [r[-1] for r in DGRAD_EDGE_CASES]
    for piece in ('ws<1>', 'ws<2>', 'ws<4>', 'wide<', 'generic<1,1,1,ck16>', 'generic<1,1,2,ck16>', 'generic<1,1,2,ck32>', 'f32<',
                  '/plain', '/plain<res>', '/general', '/general<rows1>', '/general<lanes>', '/dgrad<split>', '/dgrad<pool>',
                  '/nchw_pool<rows1>', '/nchw_pool<lanes>', '/nchw_plain', '/nchw_rows<split>', '/nchw_rows<res>', '/persistent'):
        assert any(piece in lb for lb in labels), piece
    rows = [Case(r) for r in DGRAD_EDGE_CASES]
    assert any(c.s == 2 and c.k == 3 for c in rows) and any(c.s == 2 and c.k == 1 for c in rows)
    assert any(c.dyfmt == NCHW and c.outfmt == C8 for c in rows) and any(c.skip and c.wide for c in rows)
    assert any(c.pool and c.split for c in rows) and any(c.split & 15 for c in rows) and any(c.Cin % 8 for c in rows)
    assert len(set(CASE_IDS)) == len(CASE_IDS)


def test_refusals(hip):
    """malformed data-gradient descriptors are refused by the planner (hip.conv_spec raises EssHipError)"""
    with pytest.raises(hip.EssHipError, match=r'SUMPOOL2 needs'):   # pooled, odd output extent
        hip.conv_spec(1, 13, 20, 32, 0, 64, 3, 1, 1, act=hip.ACT_SUMPOOL2, compute=hip.COMPUTE_BF16)
    with pytest.raises(hip.EssHipError, match=r'SUMPOOL2 needs'):
        hip.conv_spec(1, 12, 21, 32, 0, 64, 3, 1, 1, act=hip.ACT_SUMPOOL2, compute=hip.COMPUTE_BF16)
    with pytest.raises(hip.EssHipError, match=r'x2 source needs even extent'):   # zero-inserted source of odd virtual extent
        hip.conv_spec(1, 17, 34, 128, 0, 64, 3, 1, 1, mode0=hip.SRC_ZERO_UP2, compute=hip.COMPUTE_BF16)
    # out_split that is no multiple of 8 with a BF16_C8 output (an fp32 NCHW output may split anywhere)
    spec = hip.conv_spec(1, 9, 17, 32, 0, 64, 3, 1, 1, out_split=20, compute=hip.COMPUTE_BF16)
    with pytest.raises(hip.EssHipError, match=r'BF16_C8 outputs need the LINEAR epilogue, out_split'):
        hip._check(hip.lib().ess_conv2d_plan(ctypes.byref(spec.desc_fmt(hip.FMT_BF16_C8, hip.FMT_BF16_C8)), ctypes.byref(hip.EssConvPlan())), 'plan')
    # half operands: forward forms only
    assert hip.COMPUTE_F16 == F16
    with pytest.raises(hip.EssHipError, match=r'no pooled \(data-gradient\) form'):
        hip.conv_spec(1, 12, 20, 32, 0, 64, 3, 1, 1, act=hip.ACT_SUMPOOL2, compute=hip.COMPUTE_F16)
    with pytest.raises(hip.EssHipError, match=r'no zero-inserted sources'):
        hip.conv_spec(1, 18, 34, 128, 0, 64, 3, 1, 1, mode0=hip.SRC_ZERO_UP2, compute=hip.COMPUTE_F16)
    with pytest.raises(hip.EssHipError, match=r'no zero-inserted sources'):
        hip.conv_spec(1, 18, 26, 128, 0, 64, 1, 1, 0, mode0=hip.SRC_ZERO_UP2, compute=hip.COMPUTE_F16)
