"""CPU tier: teeth for the checker of tests/test_hip_norm_edges.py.  For every row of its table, on the row's own plane size, slice
counts and seeded inputs, a CPU fp32 restatement of the kernels' arithmetic (norm_ref.restate_*: fp32 partials of 4, fp64 running sums,
slices in order; the fused kernels' two-pass fp32 statistics) passes every bound of norm_ref, the ambiguous set of the affine-map mask
stays within its cap, and the same restatement with ONE defect injected misses a bound by at least four times on the rows named for
that defect (NAMED below).  The rows' route / slice-count labels are checked against norm_ref.plan, the restated dispatch.

Rows of more than 2^22 elements (the 256-group rows, 1024 fp32 planes) are restated on their first 16 (12 with a partial block)
channels: the planes, routes and slice counts are the row's, only fewer groups are evaluated.

A dropped pixel moves a mean by x_p / hw against a bound of 2^-20 mean|x|: on the exactly constant channel that is 2^20 / hw times the
bound, so the existing full-size rows of test_hip_mixed_edges.py (480 x 640: 3.4 times) cannot reach four times; the rows that carry this
defect are the split rows here (in8_split_*, in8_f1024_one_past, mix_hw5121_split, bn8_hw1200 / bn8_hw5121 and the fp32 split rows:
hw <= 76800, at least 13 times).  In an InstanceNorm backward the sums are not outputs and a lost pixel reaches dx only as
rstd dy_p / hw against 2^-12 rstd max|dy|: above ~1000 pixels it is carried by the statistics pass of the same kernel (the forward rows)
and by the BatchNorm rows, whose sums are the outputs dgamma / dbeta."""
import pytest
import torch

import norm_ref as R
from norm_ref import Row, row_inputs
from test_hip_norm_edges import NORM_EDGE_CASES

IDS = [c[0] for c in NORM_EDGE_CASES]


def reduced(row):
    r = Row(row)
    if r.N * r.C * r.hw <= 1 << 22:
        return row
    return row[:3] + (12 if r.partial else 16,) + row[4:]


def restated(row, defect=None, relu=1, res=True, form='y', x_fmt=None):
    """{output: error / bound} of the CPU restatement of a row (with one defect) under the checks the GPU test applies"""
    r = Row(row)
    fwd, bwd = r.label.split('/')
    row = reduced(row)
    r, d = Row(row), row_inputs(row)
    fp32 = r.family in ('in32', 'bn32')
    if x_fmt is None:
        x_fmt = 32 if fp32 else 2 if r.family == 'mix' else 0
    xv = R.stored(d['x'], x_fmt)
    q = (lambda t: t.double()) if fp32 else R.bfr
    dyv, rv = q(d['dy']), (q(d['res']) if res else None)
    x32, dy32, r32 = xv.float(), dyv.float(), (rv.float() if res else None)
    out = {}
    if r.family in ('in8', 'mix', 'in32'):
        key = 'y32' if fp32 else 'y16' if r.family == 'mix' else 'y'
        stats, y = R.restate_in_forward(x32, r32, relu, fwd, key, fp32_kernel=fp32, hilo=x_fmt == 2, defect=defect)
        out.update(R.in_forward_ratios(xv, rv, relu, stats, {key: y}, fp32_kernel=fp32))
        if relu < 2:
            xr = R.stored(d['x'], 1) if x_fmt == 2 else xv  # (the backward reads the hi parts of a pair)
            dx = R.restate_in_backward(xr.float(), dy32, stats, relu, bwd, fp32_kernel=fp32, defect=defect)
            out.update(R.in_backward_ratios(xr, dyv, relu, stats, dx, fp32_kernel=fp32))
        return out
    relu = int(form in ('y', 'y_res_dres', 'map'))
    res = form in ('none_res', 'y_res_dres')
    st, y, rm, rv_ = R.restate_bn_forward(x32, r32 if res else None, relu, d['gamma'], d['beta'], d['rm0'], d['rv0'], fwd, fp32_kernel=fp32,
                                          defect=defect)
    out.update(R.bn_forward_ratios(xv, rv if res else None, relu, d['gamma'], d['beta'], st, y, d['rm0'], d['rv0'], rm, rv_, fp32_kernel=fp32))
    off = amb = None
    if form in ('y', 'y_res_dres'):
        off = y <= 0
    elif form == 'map':
        off, amb = R.affine_mask(xv, st)
        out['ambiguous / cap'] = amb.sum((0, 2)).max().item() / (R.AMBIGUOUS_CAP * xv.shape[0] * xv.shape[2])  # (per channel, as the GPU test asserts it)
    acc = form in ('y', 'map')
    dx, dres, dg, db = R.restate_bn_backward(x32, y, dy32, st, d['gamma'], {'y_res_dres': 'y', 'none_res': 'none'}.get(form, form), bwd,
                                             d['dgamma0'], d['dbeta0'], acc, fp32_kernel=fp32, defect=defect)
    out.update(R.bn_backward_ratios(xv, dyv, st, d['gamma'], off, amb, dx, dg, db, d['dgamma0'], d['dbeta0'], acc, fp32_kernel=fp32))
    want = torch.where(off, torch.zeros_like(dyv), dyv) if off is not None else dyv
    out['dres'] = 0.0 if torch.equal(dres, want) else float('inf')
    return out


def combos(row):
    fam = row[1]
    if fam in ('in8', 'mix'):
        return [dict(relu=a, res=b) for a in (0, 1) for b in (False, True)]
    if fam == 'in32':
        return [dict(relu=a, res=b) for a in (0, 1, 2) for b in (False, True)]
    return [dict(form=f) for f in (['none', 'none_res', 'y', 'y_res_dres'] + (['map'] if fam == 'bn8' else []))]


@pytest.mark.parametrize('row', NORM_EDGE_CASES, ids=IDS)
def test_row_labels_restate_the_dispatch(row):
    r = Row(row)
    assert R.plan(r) == r.label, (r.id, R.plan(r))
    fwd, bwd = r.label.split('/')
    groups = {'in8': r.N * r.CB, 'mix': r.N * r.CB, 'bn8': r.CB, 'in32': r.N * r.C, 'bn32': r.C}[r.family]
    target = r.tune.get('norm_split_wgs', 1024)
    want = R.split_for8(groups, r.hw, groups if target == 'groups' else target) if r.family in ('in8', 'mix', 'bn8') else R.split_for(groups, r.hw)
    for route in (fwd, bwd):
        assert R.nslices(route) in (0, want), (r.id, route, want)


@pytest.mark.parametrize('row', NORM_EDGE_CASES, ids=IDS)
def test_restatement_passes_every_bound(row):
    for kw in combos(row):
        ratios = restated(row, **kw)
        print(row[0], kw, {k: round(v, 3) for k, v in ratios.items()})
        R.assert_ratios(ratios, (row[0], kw))
    if row[1] == 'in8':  # the F16_C8 form of x
        R.assert_ratios(restated(row, x_fmt=1), (row[0], 'x_f16'))
    if row[1] == 'mix':
        R.assert_ratios(restated(row, x_fmt=1), (row[0], 'x_fmt 1'))


def _rows(pred):
    return [c[0] for c in NORM_EDGE_CASES if pred(Row(c))]


split = lambda r: r.label.split('/')[0].startswith('split')
# defect -> (the rows named for it, the form it is injected in)
NAMED = {
    'drop_last': (_rows(lambda r: r.hw > 1), dict(relu=1, res=True, form='y')),
    'drop_max': (_rows(lambda r: r.hw > 1), dict(relu=0, res=False, form='none')),
    'slice_twice': (_rows(split), dict(relu=1, res=True, form='y')),
    'stats_sample0': (_rows(lambda r: r.family in ('in8', 'mix', 'in32') and r.N >= 2), dict(relu=0, res=False)),
    'mask_lt': (_rows(lambda r: r.hw > 1 or r.family in ('bn8', 'bn32')), dict(relu=1, res=False, form='y')),
    'res_before_relu': (_rows(lambda r: r.family in ('in8', 'mix', 'in32')), dict(relu=1, res=True)),
    'no_accumulate': (_rows(lambda r: r.family in ('bn8', 'bn32')), dict(form='y')),
    'no_unbiased': (_rows(lambda r: r.family in ('bn8', 'bn32') and 1 < r.N * r.hw <= 2400), dict(form='none')),
}
PAIRS = [(dfc, rid) for dfc in R.DEFECTS for rid in NAMED[dfc][0]]


@pytest.mark.parametrize('defect,rid', PAIRS, ids=[f'{a}-{b}' for a, b in PAIRS])
def test_each_defect_misses_its_bound_fourfold(defect, rid):
    row = NORM_EDGE_CASES[IDS.index(rid)]
    kw = dict(NAMED[defect][1])
    if row[1] in ('bn8', 'bn32'):
        kw = {'form': kw['form']}
    else:
        kw.pop('form', None)
    ratios = restated(row, defect=defect, **kw)
    w = max(v for v in ratios.values())
    print(rid, defect, f'worst error / bound {w:.1f}', {k: round(v, 2) for k, v in ratios.items() if v > 1})
    assert w >= 4.0, (rid, defect, ratios)
    with pytest.raises(AssertionError):
        R.assert_ratios(ratios, rid)
