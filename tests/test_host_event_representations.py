"""CPU tier of the event representations (hip.event_*_rep, representation= of EventBatchBuilder and the segmenters): the three C entry
points and their refusals, every refusal of the wrappers and of the three classes -- each raised before a device call --, and the numpy
RESTATEMENT (tests/event_rep_ref.py) that the GPU tier compares bits against, checked here against the reference's own outputs: the
histogram golden bit for bit, the voxel golden's separate_pol cases within the bound derived from the two sums' roundings."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import event_rep_ref as E
from tests import test_host_event_ingest as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAMES = ('ess_event_scatter_ring_rep', 'ess_event_ingest_ring_rep', 'ess_event_ingest_columns_rep')
EINVAL = -22


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


# ---------------------------------------------------------------------------------------------- ABI
def test_the_three_entry_points_are_exported_declared_and_the_abi_is_still_110(built_lib):
    from ess_amd import hip
    lib = ctypes.CDLL(built_lib)
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in hip.EXPORTS and f'int {name}(' in header, name
    assert hip.lib().ess_version() == 110
    assert set(hip.EXPORTS) == set(re.findall(r'\b(ess_[a-z0-9_]+)\s*\(', header))
    assert 'ESS_EVENT_REP_SIGNED = 0, ESS_EVENT_REP_SEPARATE = 1, ESS_EVENT_REP_HISTOGRAM = 2' in header
    assert (hip.EVENT_REP_SIGNED, hip.EVENT_REP_SEPARATE, hip.EVENT_REP_HISTOGRAM) == (0, 1, 2)


def test_event_rep_channels():
    from ess_amd import hip
    assert [hip.event_rep_channels(r, 5) for r in (0, 1, 2)] == [5, 10, 2]
    assert hip.event_rep_channels(hip.EVENT_REP_HISTOGRAM, 1) == 2 and hip.event_rep_channels(hip.EVENT_REP_SEPARATE, 1) == 2
    for bad in (3, -1, True, 'histogram', None, 1.0):
        with pytest.raises(hip.EssHipError, match='representation='):
            hip.event_rep_channels(bad, 5)
    for bad in (0, -2, True, 2.0):
        with pytest.raises(hip.EssHipError, match='bins='):
            hip.event_rep_channels(1, bad)


def test_the_library_refuses_in_front_of_any_launch(built_lib):
    """ESS_EINVAL with a message that names the argument; the pointers are never followed (no GPU is needed): any aligned address does"""
    from ess_amd import hip
    L = hip.lib()
    P, A = ctypes.c_void_p, 0x10000
    ptrs8, ptrs6 = [P(A)] * 8, [P(A)] * 6

    def ring(channels=4, rep=1, ring=64, acc_bytes=None, acc=A, out=A, which='ingest'):
        nbytes = 2 * max(channels, 1) * 6 * 8 * 8 if acc_bytes is None else acc_bytes
        if which == 'scatter':
            return L.ess_event_scatter_ring_rep(*ptrs8, ring, 1, 2, channels, 6, 8, P(acc), nbytes, rep, None)
        return L.ess_event_ingest_ring_rep(*ptrs8, ring, 1, 2, channels, 6, 8, P(acc), nbytes, P(out), rep, None)

    def columns(channels=4, rep=1, stride=64, acc_bytes=None, out=A):
        nbytes = 2 * max(channels, 1) * 6 * 8 * 8 if acc_bytes is None else acc_bytes
        return L.ess_event_ingest_columns_rep(*ptrs6, stride, 2, channels, 6, 8, P(A), nbytes, P(out), rep, None)

    for call in (ring, columns, lambda **kw: ring(which='scatter', **kw)):
        for rep in (3, -1, 1 << 20):
            assert call(rep=rep) == EINVAL and b'representation=' in L.ess_last_error()
        assert call(channels=5, rep=1) == EINVAL and b'channels=5 must be even' in L.ess_last_error()
        for c in (1, 3, 4):
            assert call(channels=c, rep=2) == EINVAL and f'channels={c} must be 2'.encode() in L.ess_last_error()
        assert call(channels=0, rep=0) == EINVAL and b'channels=0 must be positive' in L.ess_last_error()
        # the workspace follows from `channels`: one plane short is refused, in every representation
        for c, rep in ((5, 0), (4, 1), (2, 2)):
            assert call(channels=c, rep=rep, acc_bytes=2 * c * 6 * 8 * 8 - 8) == EINVAL and b'acc has' in L.ess_last_error()
    assert ring(ring=24) == EINVAL and b'multiple of 16' in L.ess_last_error()
    assert ring(ring=(1 << 22) + 16) == EINVAL and b'ring=' in L.ess_last_error()
    assert columns(stride=24) == EINVAL and b'multiple of 16' in L.ess_last_error()
    assert ring(out=0) == EINVAL and b'null' in L.ess_last_error()
    assert columns(out=A + 4) == EINVAL and b'16-byte aligned' in L.ess_last_error()
    assert ring(acc=0, which='scatter') == EINVAL and b'null' in L.ess_last_error()


# ---------------------------------------------------------------------------------------------- the wrappers
def _host_call(S=2, C=4, H=6, W=8, ring=32):
    z = lambda *s, d=torch.int32: torch.zeros(*s, dtype=d)  # noqa: E731
    return dict(t=z(S, ring, d=torch.int64), x=z(S, ring, d=torch.int16), y=z(S, ring, d=torch.int16), p=z(S, ring, d=torch.uint8),
                rows=z(S), starts=z(S), counts=z(S), formats=z(S), out=z(S, C, H, W, d=torch.float32), acc=z(S, C, H, W, d=torch.int64))


WRAPPER_REFUSALS = [
    (dict(representation=3), 'representation=3'),
    (dict(representation=True), 'representation=True'),
    (dict(representation='histogram'), "representation='histogram'"),
    (dict(representation=None), 'representation=None'),
    (dict(representation=2), 'EVENT_REP_HISTOGRAM fills 2 planes'),
    (dict(representation=1, C=5), 'EVENT_REP_SEPARATE fills 2 \\* bins planes'),
    (dict(t=torch.zeros(2, 32, dtype=torch.int32)), 't must be'),
    (dict(y=torch.zeros(2, 16, dtype=torch.int16)), 'y must be'),
    (dict(p=torch.zeros(2, 32, dtype=torch.int16)), 'p must be'),
    (dict(counts=torch.zeros(3, dtype=torch.int32)), 'counts must be int32'),
    (dict(formats=torch.zeros(2, dtype=torch.int64)), 'formats must be int32'),
    (dict(t=np.zeros((2, 32))), 'must be a CUDA'),
]


@pytest.mark.parametrize('which', ['scatter_ring', 'ingest_ring', 'ingest_columns'])
def test_wrapper_refusals_come_before_a_pointer_is_taken(which, monkeypatch):
    """CPU tensors reach every check of form; the last check is the device's, so the library is never loaded"""
    from ess_amd import hip
    monkeypatch.setattr(hip, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was reached')))

    def call(representation=1, C=4, **kw):
        a = {**_host_call(C=C), **kw}
        if which == 'scatter_ring':
            return hip.event_scatter_ring_rep(a['t'], a['x'], a['y'], a['p'], a['rows'], a['starts'], a['counts'], a['formats'], a['acc'],
                                              representation)
        if which == 'ingest_ring':
            return hip.event_ingest_ring_rep(a['t'], a['x'], a['y'], a['p'], a['rows'], a['starts'], a['counts'], a['formats'], a['out'],
                                             representation, acc=a['acc'])
        return hip.event_ingest_columns_rep(a['t'], a['x'], a['y'], a['p'], a['counts'], a['formats'], a['out'], representation,
                                            acc=a['acc'])
    for kw, match in WRAPPER_REFUSALS:
        with pytest.raises(hip.EssHipError, match=match):
            call(**kw)
    if which != 'ingest_columns':
        with pytest.raises(hip.EssHipError, match='rows must be int32'):
            call(rows=torch.zeros(2, dtype=torch.int64))
        with pytest.raises(hip.EssHipError, match='multiple of 16'):
            call(**{k: torch.zeros(2, 24, dtype=d) for k, d in zip('txyp', (torch.int64, torch.int16, torch.int16, torch.uint8))})
    if which == 'scatter_ring':
        with pytest.raises(hip.EssHipError, match='acc must be a non-empty int64'):
            call(acc=torch.zeros(2, 4, 6, 8, dtype=torch.int32))
    else:
        with pytest.raises(hip.EssHipError, match='out must be a non-empty fp32'):
            call(out=torch.zeros(2, 4, 6, 8, dtype=torch.float64))
        with pytest.raises(hip.EssHipError, match='acc must be int64'):
            call(acc=torch.zeros(2 * 4 * 6 * 8, dtype=torch.int32))
    with pytest.raises(hip.EssHipError, match='no CPU path'):  # nothing wrong with the form: the device check is what is left
        call()


# ---------------------------------------------------------------------------------------------- the keyword
def test_the_keyword_names_three_representations():
    from ess_amd import hip
    assert hip.EVENT_REPRESENTATIONS == {None: 0, 'separate_pol': 1, 'histogram': 2}
    assert hip.event_representation(None, 'trilinear', [object()]) == hip.EVENT_REP_SIGNED  # (None leaves the flavour alone)
    assert hip.event_representation('separate_pol', 'temporal', None) == 1 and hip.event_representation('histogram', 'temporal', None) == 2
    for bad in ('signed', 'voxel_grid', 1, True, ('histogram',)):
        with pytest.raises(hip.EssHipError, match='representation='):
            hip.event_representation(bad, 'temporal', None)
    for rep in ('separate_pol', 'histogram'):
        with pytest.raises(hip.EssHipError, match=f"representation='{rep}'.*voxel='trilinear'"):
            hip.event_representation(rep, 'trilinear', None)
        with pytest.raises(hip.EssHipError, match=f"representation='{rep}'.*rectify_maps given"):
            hip.event_representation(rep, 'temporal', [np.zeros((4, 4, 2), np.float32)])


GEO = dict(batch_size=2, sequence_steps=3, bins=3, event_capacity=64, grid_hw=(26, 34), grid_resize=(26, 36), height=20, width=36,
           label_hw=(20, 34), crop_hw=(12, 20), crop_band=(8, 12))


def test_the_builder_takes_and_refuses_the_keyword():
    from ess_amd import hip
    from ess_amd.datasets import event_batches as EB
    assert EB.VOXEL_FLAVOURS == ('temporal', 'trilinear')
    b = EB.EventBatchBuilder(**GEO)
    assert b.representation is None and b.channels == 3
    assert EB.EventBatchBuilder(**GEO, representation='separate_pol').channels == 6
    assert EB.EventBatchBuilder(**GEO, representation='histogram').channels == 2
    assert EB.EventBatchBuilder.dsec(2, representation='separate_pol').channels == 10
    assert EB.EventBatchBuilder.ddd17(2, representation='histogram').channels == 2
    assert EB.EventBatchBuilder.ddd17(2, bins=2, representation='separate_pol', grid_normalize='population').channels == 4
    maps = [np.zeros((26, 34, 2), np.float32)]
    for kw, match in ((dict(representation='signed'), "representation='signed'"),
                      (dict(representation=1), 'representation=1'),
                      (dict(representation='histogram', voxel='trilinear'), "representation='histogram'.*voxel='trilinear'"),
                      (dict(representation='separate_pol', voxel='trilinear', rectify_maps=maps), "voxel='trilinear'.*rectify_maps given"),
                      (dict(representation='separate_pol', rectify_maps=maps), "representation='separate_pol'.*rectify_maps given")):
        with pytest.raises(hip.EssHipError, match=match):
            EB.EventBatchBuilder(**GEO, **kw)
    with pytest.raises(hip.EssHipError, match='representation='):
        EB.EventBatchBuilder.dsec(2, representation='voxel_grid')


def _encoder(num_bins):
    return SimpleNamespace(num_bins=num_bins, to=lambda *a, **k: (_ for _ in ()).throw(AssertionError('the device was reached')))


SEGMENTER_REFUSALS = [
    (4, dict(representation='signed'), "representation='signed'"),
    (4, dict(representation='separate_pol', voxel='trilinear'), "representation='separate_pol'.*voxel='trilinear'"),
    (2, dict(representation='histogram', voxel='trilinear'), "representation='histogram'.*voxel='trilinear'"),
    (4, dict(representation='separate_pol', rectify_maps=[None] * 3), "representation='separate_pol'.*rectify_maps given"),
    (5, dict(representation='separate_pol'), 'num_bins=5 must be even'),
    (4, dict(representation='histogram'), 'num_bins=4 must be 2'),
    (1, dict(representation='histogram'), 'num_bins=1 must be 2'),
]


@pytest.mark.parametrize('num_bins,kw,match', SEGMENTER_REFUSALS)
def test_the_segmenters_refuse_before_the_models_reach_the_device(num_bins, kw, match):
    from ess_amd import hip
    from ess_amd.run_segmentation import MultiStreamSegmenter
    from ess_amd.run_sequence_segmentation import SequenceSegmenter
    with pytest.raises(hip.EssHipError, match=match):
        SequenceSegmenter(_encoder(num_bins), None, 64, 96, None, n_streams=3, sequence_steps=2, window_events=256, **kw)
    for layout in ('columns', 'ring'):
        with pytest.raises(hip.EssHipError, match=match):
            MultiStreamSegmenter(_encoder(num_bins), None, 64, 96, None, 3, event_capacity=256, event_layout=layout, **kw)


@pytest.mark.parametrize('rep,num_bins', [('separate_pol', 4), ('histogram', 2)])
def test_the_stream_segmenter_needs_raw_columns_for_a_representation(rep, num_bins):
    from ess_amd import hip
    from ess_amd.run_segmentation import MultiStreamSegmenter
    for kw in (dict(), dict(event_capacity=256), dict(event_capacity=256, event_layout='records'), dict(event_layout='columns'),
               dict(event_layout='ring')):
        with pytest.raises(hip.EssHipError, match=f"representation='{rep}'.*event_capacity=N.*event_layout='columns' or 'ring'"):
            MultiStreamSegmenter(_encoder(num_bins), None, 64, 96, None, 3, representation=rep, **kw)


def test_generate_input_representation_still_refuses_the_histogram():
    from ess_amd.datasets import data_util
    with pytest.raises(NotImplementedError):
        data_util.generate_input_representation(np.zeros((1, 4)), 'histogram', (4, 4))


# ---------------------------------------------------------------------------------------------- the restatement against the goldens
def _histogram_cols(n, seed, pm, H, W):
    """the golden's events (make_golden_representations.histogram_events) as raw columns: p is one byte, -1 -> 0xFF"""
    from oracle import ess_oracle as O
    x, y, pol, t = O.synth_events(n, H, W, seed, border=0.0)
    p = (pol * 2 - 1 if pm else pol).to(torch.int8).numpy()
    return E.Cols(t.double().numpy(), x.floor().to(torch.int16).numpy(), y.floor().to(torch.int16).numpy(), p)


def _histogram_golden():
    g = torch.load(os.path.join(GOLDEN, 'event_histogram.pt'))
    return g['H'], g['W'], g['cases']


def test_histogram_restatement_equals_the_reference_bit_for_bit():
    """counts are integers below 2^24: exact in fp32 on both sides, so nothing but equality is in order"""
    H, W, cases = _histogram_golden()
    assert (H, W) == (48, 64) and sorted(c['n'] for c in cases) == [1, 3000, 4096, 5000]
    for c in cases:
        got = E.restate(_histogram_cols(c['n'], c['seed'], c['pm'], H, W), 'histogram', 1, H, W)
        want = c['histogram'].numpy()
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (2, H, W)
        assert got.tobytes() == want.tobytes(), c['seed']
        assert float(want.sum()) == c['n'] and (c['n'] == 1 or (want[0].sum() > 0 and want[1].sum() > 0))
        if c['n'] >= 3000:
            assert want.max() >= 3  # several events a pixel


def _separate_cases():
    g = torch.load(os.path.join(GOLDEN, 'voxel.pt'))
    cases = [c for c in g['temporal'] if c['separate_pol']]
    assert sorted(c['seed'] for c in cases) == [11, 13, 14]
    return g['H'], g['W'], cases


def _separate_cols(c, H, W):
    """the golden's events (make_golden.gold_voxel) as raw columns; a few pixels lie outside the frame, as there"""
    from oracle import ess_oracle as O
    x, y, pol, t = O.synth_events(c['n'], H, W, c['seed'])
    p = (pol * 2 - 1 if c['pm'] else pol).to(torch.int8).numpy()
    return E.Cols(t.double().numpy(), x.floor().to(torch.int16).numpy(), y.floor().to(torch.int16).numpy(), p)


@pytest.mark.parametrize('seed', [11, 13, 14])
def test_separate_restatement_against_the_reference_within_the_derived_bound(seed):
    """Per voxel with n contributions c_i >= 0: the reference adds them one after the other in fp32, the restatement adds exact
    integers and rounds once -- gamma_n * sum |c_i| with gamma_n = n u / (1 - n u), u = 2^-24 -- and each c_i was quantised to a
    multiple of 2^-40: at most 2^-41 each (the bound test_restatement_against_the_oracle_within_the_derived_bound derives)."""
    H, W, cases = _separate_cases()
    c = next(k for k in cases if k['seed'] == seed)
    bins, cols = c['bins'], _separate_cols(c, H, W)
    fixed = E.restate(cols, 'separate_pol', bins, H, W).astype(np.float64).ravel()
    want = c['grid'].numpy().astype(np.float64).ravel()
    assert want.shape == fixed.shape == (2 * bins * H * W,)
    idx, v = E.contributions(cols, 'separate_pol', bins, H, W)
    n = np.bincount(idx, minlength=fixed.size).astype(np.float64)
    mag = np.bincount(idx, weights=np.abs(v.astype(np.float64)), minlength=fixed.size)
    u = 2.0 ** -24
    bound = (n * u / (1 - n * u)) * mag + n * 2.0 ** -41
    err = np.abs(fixed - want)
    print(f'seed {seed}: max n {int(n.max())}, max |fixed - reference| {err.max():.3e}, equal outright {np.mean(err == 0):.4f}, '
          f'min slack {np.min(bound - err):.3e}')
    assert np.all(err <= bound)
    assert np.all(fixed >= 0) and np.all(fixed[n == 0] == 0) and np.all(want[n == 0] == 0)
    assert fixed[:bins * H * W].sum() > 0 and fixed[bins * H * W:].sum() > 0


def test_three_mutations_of_the_restatement_each_miss_the_goldens():
    """what the goldens pin: no sign in the halves, [positive; negative] half order, [negative, positive] histogram order"""
    H, W, cases = _separate_cases()
    c = next(k for k in cases if k['seed'] == 14)
    cols, want = _separate_cols(c, H, W), c['grid'].numpy()
    for mutation in (dict(sign_halves=True), dict(swap_halves=True)):
        got = E.restate(cols, 'separate_pol', c['bins'], H, W, **mutation)
        assert np.abs(got - want).max() > 0.01, mutation
    assert np.abs(E.restate(cols, 'separate_pol', c['bins'], H, W) - want).max() < 1e-5
    H, W, hist = _histogram_golden()
    h = next(k for k in hist if k['n'] == 5000)
    hc = _histogram_cols(h['n'], h['seed'], h['pm'], H, W)
    assert E.restate(hc, 'histogram', 1, H, W, pos_first=True).tobytes() != h['histogram'].numpy().tobytes()
    assert E.restate(hc, 'histogram', 1, H, W).tobytes() == h['histogram'].numpy().tobytes()


@pytest.mark.parametrize('case', ['spread', 'one_pixel', 'edges'])
def test_positive_minus_negative_sums_are_the_signed_sums_exactly(case):
    """int64, no tolerance: sums_separate[b] - sums_separate[bins + b] == sums_signed[b]; and the restatement's 'signed' is
    test_host_event_ingest's own grid"""
    bins, H, W = 5, 24, 40
    if case == 'edges':  # pixels outside, a NaN time, an event at the window's end (the last bin: no right half), 0xFF polarity bytes
        ev = R.events(64, H, W, 9)
        cols = E.columns_of_rows(ev)
        cols.x[3], cols.y[4], cols.x[5], cols.y[6] = -1, H, W, -1
        cols.t[7] = np.nan
        cols.p[8:12] = 0xFF
    else:
        ev = R.events(3000, H, W, 5) if case == 'spread' else R.one_pixel_events(2000, 6)
        cols = E.columns_of_rows(ev)
    sep = E.restate_sums(cols, 'separate_pol', bins, H, W)
    signed = E.restate_sums(cols, 'signed', bins, H, W)
    assert sep.dtype == signed.dtype == np.int64 and sep.shape == (2 * bins, H, W) and signed.shape == (bins, H, W)
    assert np.array_equal(sep[:bins] - sep[bins:], signed) and sep.min() >= 0 and sep[:bins].any() and sep[bins:].any()
    if case != 'edges':
        assert E.dequantise(signed).tobytes() == R.restate(R.packed(ev), bins, H, W).tobytes()
    hist = E.restate_sums(cols, 'histogram', bins, H, W)
    inside = (cols.x >= 0) & (cols.x < W) & (cols.y >= 0) & (cols.y < H)
    assert hist.shape == (2, H, W) and int(hist.sum() >> 40) == int(inside.sum())  # (the NaN time counts)
    assert int(hist[1].sum() >> 40) == int((inside & (cols.p == 1)).sum())
