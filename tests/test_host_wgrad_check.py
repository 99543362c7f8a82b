"""CPU tier: teeth for the checker of tests/test_hip_wgrad_edges.py.  For every row of its table, on the row's own shapes and seeded
inputs: an fp32 torch-CPU weight gradient (a stand-in for a correct kernel) passes wgrad_ref.check against the float64 reference, and
the same with ONE output pixel of dY dropped -- one missing product per (co, ci, tap), at the last row and column, where partial tiles
live -- fails it by at least ten times the bound, in dw and in db.  A row too large or too benign for that would let a kernel lose a
pixel unnoticed.  The rows' route and slab-count labels are checked against the library's planner, which runs without a GPU."""
import ctypes
import os
import sys

import pytest

from test_hip_wgrad_edges import CASE_IDS, WGRAD_EDGE_CASES
from wgrad_ref import BF16, C8, X3, Case, case_reference, check, excess, kernel_operands, wgrad_fp32_standin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


def restated_route(c):
    """wroute() / split_via_c8() of csrc/conv_wgrad.hip for a descriptor wvalidate() accepts (a stride-2 BF16_C8 3x3 is planned as one
    stride-1 parity phase of it)"""
    xc8, dc8 = c.xfmt == C8, c.dyfmt == C8
    k3s1p1 = (c.k, c.s, c.p) == (3, 1, 1)
    if c.compute == X3 and k3s1p1 and (c.C1 == 0 or c.C0 % 8 == 0) and c.m0 != 2 and c.m1 != 2 and (c.C1 == 0 or c.m1 == 0):
        return 'X3_VIA_C8'
    bf16 = c.compute == BF16 or (c.compute == X3 and k3s1p1)
    if xc8 and dc8:
        return 'W_C8_K3' if c.k == 3 else 'W_C8_K1'
    if xc8:
        return 'W_SMALL1X1_C8X'
    k1s1p0 = (c.k, c.s, c.p) == (1, 1, 0)
    if k1s1p0 and c.C1 == 0 and c.m0 == 0 and c.Cout <= 16 and c.Cin <= 64:
        return 'W_SMALL1X1_MFMA' if c.Cin <= 32 and (c.Ho * c.Wo) % 64 == 0 else 'W_SMALL1X1'
    rows8 = c.Wv % 8 == 0 and c.Wo % 8 == 0 and c.m0 != 2 and c.m1 != 2
    if bf16 and k3s1p1:
        return 'W_BF16_K3_FAST' if rows8 else 'W_BF16_K3'
    if bf16 and k1s1p0 and rows8:
        return 'W_BF16_K1'
    if c.Cin == 1 and c.k == 7:
        return 'W_TAPS7'
    return 'W_F32_TILE'


@pytest.mark.parametrize('row', WGRAD_EDGE_CASES, ids=CASE_IDS)
def test_row_labels_restate_the_planner(built_lib, row):
    from ess_amd import hip
    c = Case(row)
    assert restated_route(c) == c.route, c.id
    assert ('phases' in c.flags) == (c.xfmt == C8 and c.dyfmt == C8 and (c.k, c.s) == (3, 2)), c.id
    d = hip.EssConvDesc(c.N, c.Hv, c.Wv, c.C0, c.C1, c.m0, c.m1, c.Cout, c.Ho, c.Wo, c.k, c.s, c.p, hip.EPI_LINEAR, hip.ACT_NONE, 0, 0,
                        c.compute, c.xfmt, c.xfmt, c.dyfmt, hip.FMT_F32_NCHW)
    assert hip.lib().ess_conv2d_wgrad_workspace(ctypes.byref(d)) == c.workspace_bytes(), (c.id, hip.lib().ess_last_error())
    if c.route == 'W_C8_K1':  # the pixel-tile width the plan picks (least padded area, 32-wide on a tie): its two kernel instantiations
        area = {tw: -(-c.Wo // tw) * tw * -(-c.Ho // (128 // tw)) * (128 // tw) for tw in (32, 16)}
        assert ('tw32' in c.flags) == (area[32] <= area[16]) and ('tw16' in c.flags) == (area[32] > area[16]), (c.id, area)


@pytest.mark.parametrize('row', WGRAD_EDGE_CASES, ids=CASE_IDS)
def test_bound_passes_fp32_and_notices_one_dropped_pixel(row):
    c, sets, refs = case_reference(row)
    ops = [kernel_operands(c, *q) for q in sets]
    geom = (c.k, c.s, c.p, c.m0, c.m1)
    fp32 = [wgrad_fp32_standin(*o, *geom) for o in ops]
    x0, x1, dy = ops[-1]
    dy_cut = dy.clone()
    dy_cut[-1, :, -1, -1] = 0
    mutant = wgrad_fp32_standin(x0, x1, dy_cut, *geom)
    # the plain call (set 0 alone; with one set, the last set is set 0) and the sum over the sets, mutant = one pixel of the LAST set lost
    for what, passes, picks in (('plain', 1, [len(sets) - 1]), ('sets', c.nsets, range(len(sets)))):
        for j, name in enumerate(('dw', 'db')):
            ref = sum(refs[i][j] for i in picks)
            good = sum(fp32[i][j] for i in picks)
            bad = good - fp32[-1][j] + mutant[j]
            check(good, ref, passes, c.kind, f'{c.id} {what} {name}')
            e = excess(bad, ref, passes, c.kind)
            print(f'{c.id} {what} {name}: fp32 at {excess(good, ref, passes, c.kind):.3f} of the bound, one dropped pixel at {e:.1f}')
            assert e >= 10.0, (c.id, what, name, e)
            with pytest.raises(AssertionError):
                check(bad, ref, passes, c.kind)
