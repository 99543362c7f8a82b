"""CPU tier: the host side of the multi-stream display -- the two entry points it adds (ess_recon_post_bounds_steered,
ess_recon_post_frame_steered: declared, exported, bound, ABI version untouched), what the library, the wrappers and the driver refuse
before anything reaches a device, the display words of a round as a function on lists, and the host restatement of the steered
auto-HDR step (tests/multi_display_ref.py) with the PROOF that the schedules both tiers run separate three wrong steerings."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import multi_display_ref as M  # noqa: E402
from tests import recon_post_ref as R  # noqa: E402


@pytest.fixture(scope='module')
def built_lib():
    import __graft_entry__ as ge
    return ge.build_library(verbose=False)


class _FakeDevice(torch.Tensor):
    """a CPU tensor that claims to live on the device: the argument checks run in front of any pointer being taken"""
    @property
    def is_cuda(self):
        return True


def _dev(t):
    return t.as_subclass(_FakeDevice)


def test_symbols_are_declared_exported_and_bound(built_lib):
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    lib = ctypes.CDLL(built_lib)
    from ess_amd import hip
    for name, nargs in (('ess_recon_post_bounds_steered', 17), ('ess_recon_post_frame_steered', 16)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
        fn = getattr(hip.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert hip.lib().ess_version() == 110  # (purely additive: the ABI version stays)
    # the unsteered entry points keep their signatures
    assert len(hip.lib().ess_recon_post_bounds.argtypes) == 14 and len(hip.lib().ess_recon_post_frame.argtypes) == 15


# ---------------------------------------------------------------------------------------------- the restatement and its mutants
W = R.gkern(5, 1.0)
AMOUNT = 0.3


@pytest.mark.parametrize('size', R.HDR_FILTER_SIZES)
def test_schedules_separate_the_mutants(size):
    """Each mutant must change at least one bounds bit of a slot the right steering takes -- else the GPU tier's comparison
    could not fail for it.  The compact schedule sees all three at sizes 3 and 10, the ride-along schedule (identity rows) the two
    it can.  At size 0 the history holds one entry, the frame's own: no steering is visible and only equality is asserted."""
    good_c = M.run(M.COMPACT, size, W, AMOUNT)
    good_r = M.run(M.RIDE_ALONG, size, W, AMOUNT)
    for mutant in ('hold_pushes', 'zero_is_take', 'slot_as_row'):
        bad_c = M.run(M.COMPACT, size, W, AMOUNT, **{mutant: True})
        bad_r = M.run(M.RIDE_ALONG, size, W, AMOUNT, **{mutant: True})
        if size == 0:
            # slot_as_row reads another ROW's history, but the image decides the single entry: still equal
            assert not M.taken_bits_differ(good_c, bad_c) and not M.taken_bits_differ(good_r, bad_r), mutant
            continue
        assert M.taken_bits_differ(good_c, bad_c), (mutant, size)
        if mutant != 'slot_as_row':
            assert M.taken_bits_differ(good_r, bad_r), (mutant, size)


def test_schedules_are_of_the_kind_described():
    """ride-along: every row held at least once and taken again, rows 0 and 2 restarted once while holding >= 2 entries; compact: the
    rows of a call are distinct, a padded slot is on HOLD with an out-of-range row"""
    res = M.run(M.RIDE_ALONG, 10, W, AMOUNT)
    for r in range(M.N_ROWS):
        modes = [m[r] for _, m in M.RIDE_ALONG]
        first_hold = modes.index(M.H)
        assert any(m in (M.T, M.Z) for m in modes[first_hold + 1:]), r
    for r in (0, 2):
        t = [m[r] for _, m in M.RIDE_ALONG].index(M.Z)
        assert [m[r] for _, m in M.RIDE_ALONG].count(M.Z) == 1 and res[t - 1][2][r] >= 2 and res[t][2][r] == 1
    assert M.Z not in [m[1] for _, m in M.RIDE_ALONG]
    for rows, mode in M.COMPACT:
        named = [r for r in rows if 0 <= r < M.N_ROWS]
        assert len(set(named)) == len(named)
        assert all(m == M.H for r, m in zip(rows, mode) if not 0 <= r < M.N_ROWS)


def test_restatement_all_take_is_the_unsteered_history():
    """identity rows, every slot taken: the steered restatement is R.History(3, size), bit for bit"""
    for size in R.HDR_FILTER_SIZES:
        st, h = M.Steered(3, size), R.History(3, size)
        for img in R.hdr_images():
            got, taken = st.update(img, W, AMOUNT, [M.T] * 3)
            assert taken.all() and (got.view(np.uint32) == h.update(img, W, AMOUNT).view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------- the display words
def test_display_words():
    from ess_amd import hip
    from ess_amd import run_segmentation as S
    Hd, Tk, Zr = hip.CARRY_HOLD, hip.CARRY_TAKE, hip.CARRY_ZERO
    # ride-along: restart + active = ZERO; active = TAKE; idle = HOLD -- and a pending restart of an idle stream yields HOLD
    pending, active = [True, True, False, False], [True, False, True, False]
    assert S.display_words(pending, active) == ([Zr, Hd, Tk, Hd], None)
    _, _, after = S.stream_modes(pending, active)
    assert after == [False, True, False, False]  # (it stays pending ...)
    assert S.display_words(after, [True] * 4) == ([Tk, Zr, Tk, Tk], None)  # (... and empties the history when it is carried out)
    # compacted: per SLOT, the row is the stream's number, a padded slot is HOLD with a row outside every history
    pending, active = [False, True, False, True, True], [True, False, False, True, True]
    plan = S.compact_plan(pending, active, (1, 2, 4))
    assert plan.bucket == 4 and plan.rows == [0, 3, 4]
    words, rows = S.display_words(pending, active, plan)
    assert words == [Tk, Zr, Zr, Hd] and rows == [0, 3, 4, S.SCATTER_SKIP]
    assert not 0 <= S.SCATTER_SKIP < 5
    idle = [False] * 3
    assert S.display_words(idle, idle, S.compact_plan(idle, idle, (2,))) == ([Hd, Hd], [S.SCATTER_SKIP] * 2)
    with pytest.raises(hip.EssHipError, match=r'display_words: 2 pending flags for 3 streams'):
        S.display_words([True, False], [True] * 3)
    with pytest.raises(hip.EssHipError, match=r'display_words: the plan serves streams \[0, 3, 4\]'):
        S.display_words(pending, [True] * 5, plan)
    # the functions the host tests pin keep their values
    assert S.stream_modes([True, False], [True, True]) == ([Zr, Hd], [Tk, Tk], [False, False])
    assert plan._fields == ('bucket', 'rows', 'gather_dst', 'gather_src', 'norm_mode', 'scatter_dst', 'scatter_src', 'pending_after')


# ---------------------------------------------------------------------------------------------- refusals
def _bounds_args(N=2, Rn=3, size=3):
    return dict(img=_dev(torch.zeros(N, 1, 8, 12)), weights=W, amount=0.3, workspace=_dev(torch.zeros(N, 256, 2)),
                ring=_dev(torch.zeros(Rn, size + 1, 2, dtype=torch.float64)), ring_state=_dev(torch.zeros(Rn, 2, dtype=torch.int32)),
                filter_size=size, bounds=_dev(torch.zeros(N, 2)))


def test_bounds_wrapper_refuses_on_the_host(built_lib):
    from ess_amd import hip
    i32 = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt)  # noqa: E731
    a = _bounds_args()
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: mode must be a contiguous int32 \[2\].*int64'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2, torch.int64)), rows=[0, 1])
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: mode must be a contiguous int32 \[2\].*\(3,\)'):
        hip.recon_post_bounds(**a, mode=_dev(i32(3)), rows=[0, 1])
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: mode must be a contiguous int32 \[2\].*list'):
        hip.recon_post_bounds(**a, mode=[1, 1], rows=[0, 1])
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: mode must be a CUDA\(HIP\) tensor'):
        hip.recon_post_bounds(**a, mode=i32(2), rows=[0, 1])
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: rows must be a contiguous int32 \[2\].*float32'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)), rows=_dev(torch.zeros(2)))
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: rows must be a contiguous int32 \[2\].*\(3,\)'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)), rows=_dev(i32(3)))
    with pytest.raises(hip.EssHipError, match=r'recon_post_bounds: rows must be a CUDA\(HIP\) tensor'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)), rows=i32(2))
    with pytest.raises(hip.EssHipError, match=r'rows must be .* a host list of 2 ints'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)), rows=[0, 1, 2])
    with pytest.raises(hip.EssHipError, match=r'rows must be .* a host list of 2 ints'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)), rows=[0, 1.5])
    with pytest.raises(hip.EssHipError, match=r'rows=\[2, 2\] names a history row twice'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)), rows=[2, 2])
    with pytest.raises(hip.EssHipError, match=r'rows= belongs to the steered step'):
        hip.recon_post_bounds(**a, rows=[0, 1])
    # two padded slots share the out-of-range row: no duplicate -- the call gets as far as the (fake) device
    with pytest.raises(hip.EssHipError, match=r'ring must be a contiguous torch.float64 \[3, 4, 2\]'):
        hip.recon_post_bounds(**dict(a, ring=_dev(torch.zeros(2, 4, 2, dtype=torch.float64))), mode=_dev(i32(2)), rows=[-2, -2])
    # without rows the histories are the slots': R == N
    with pytest.raises(hip.EssHipError, match=r'ring must be a contiguous torch.float64 \[2, 4, 2\]'):
        hip.recon_post_bounds(**a, mode=_dev(i32(2)))


def test_frame_wrapper_refuses_on_the_host(built_lib):
    from ess_amd import hip
    img, b = _dev(torch.zeros(2, 1, 8, 12)), _dev(torch.zeros(2, 2))
    with pytest.raises(hip.EssHipError, match=r'recon_post_frame: mode must be a contiguous int32 \[2\].*int64'):
        hip.recon_post_frame(img, W, 0.3, b, mode=_dev(torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(hip.EssHipError, match=r'recon_post_frame: mode must be a contiguous int32 \[2\].*\(1,\)'):
        hip.recon_post_frame(img, W, 0.3, b, mode=_dev(torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(hip.EssHipError, match=r'recon_post_frame: mode must be a contiguous int32 \[2\]'):
        hip.recon_post_frame(img, W, 0.3, b, mode=_dev(torch.zeros(4, dtype=torch.int32)[::2]))
    with pytest.raises(hip.EssHipError, match=r'recon_post_frame: mode must be a CUDA\(HIP\) tensor'):
        hip.recon_post_frame(img, W, 0.3, b, mode=torch.zeros(2, dtype=torch.int32))


def test_library_refuses_bad_arguments(built_lib):
    """the C entry points themselves: errno-style return + ess_last_error(), nothing launched (the fake pointers never reach a kernel)"""
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(64)  # (never dereferenced: every call below is refused in front of the launch)
    w = (ctypes.c_float * 25)(*[0.04] * 25)

    def bounds(N=2, Rn=3, size=3, mode=one, rows=one, ws_bytes=2 * 256 * 2 * 4, ring=one):
        return L.ess_recon_post_bounds_steered(one, w, 1.3, 0.3, N, 8, 12, one, ws_bytes, ring, one, Rn, size, one, mode, rows, P(0))
    for kw, msg in ((dict(mode=P(0)), 'mode is null'), (dict(mode=P(66)), 'mode'), (dict(rows=P(66)), 'rows'), (dict(Rn=0), 'R=0'),
                    (dict(Rn=-1), 'R=-1'), (dict(size=64), 'filter_size=64'), (dict(N=0), 'N=0'), (dict(ws_bytes=100), 'workspace has 100 bytes'),
                    (dict(ring=P(0)), 'null workspace, ring')):
        assert bounds(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert 'recon_post_bounds_steered' in L.ess_last_error().decode()

    def frame(mode=one, N=2, win=(0, 0, 8, 12), u8=one):
        return L.ess_recon_post_frame_steered(one, w, 1.3, 0.3, one, u8, P(0), N, 8, 12, *win, mode, P(0))
    for kw, msg in ((dict(mode=P(0)), 'mode is null'), (dict(mode=P(65)), 'mode'), (dict(N=0), 'N=0'), (dict(win=(0, 0, 9, 12)), 'leaves the 8 x 12 source'),
                    (dict(u8=P(0)), 'both null')):
        assert frame(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert 'recon_post_frame_steered' in L.ess_last_error().decode()


def test_rescaler_refuses_on_the_host():
    from ess_amd import hip
    from ess_amd.e2vid.options.inference_options import default_options
    from ess_amd.e2vid.utils.inference_utils import IntensityRescaler
    opt = default_options()
    opt.auto_hdr = False
    r = IntensityRescaler(opt, n=3, device=torch.device('cpu'))
    mode = _dev(torch.zeros(2, dtype=torch.int32))
    with pytest.raises(hip.EssHipError, match=r'made for 3 history rows, got 2 slots without rows='):
        r.rescale(_dev(torch.zeros(2, 1, 8, 12)), mode=mode)
    with pytest.raises(hip.EssHipError, match=r'made for 3 history rows, got 4 slots'):
        r.rescale(_dev(torch.zeros(4, 1, 8, 12)), mode=_dev(torch.zeros(4, dtype=torch.int32)), rows=[0, 1, 2, -2])
    with pytest.raises(hip.EssHipError, match=r'rows= belongs to the steered call'):
        r.rescale(_dev(torch.zeros(3, 1, 8, 12)), rows=[0, 1, 2])
    with pytest.raises(hip.EssHipError, match=r'made for 3 samples, got 2'):  # (the unsteered refusal is as it was)
        r.rescale(_dev(torch.zeros(2, 1, 8, 12)))


def test_driver_refusals():
    from ess_amd import hip
    from ess_amd import run_segmentation as S
    mk = lambda **kw: S.MultiStreamSegmenter(None, None, 64, 96, None, 3, **kw)  # noqa: E731
    pal = np.zeros((6, 3), dtype=np.uint8)
    with pytest.raises(hip.EssHipError, match=r'MultiStreamSegmenter: postprocess=True needs reconstruct=True'):
        mk(postprocess=True)
    with pytest.raises(hip.EssHipError, match=r'MultiStreamSegmenter: overlay= needs postprocess=True .* and a palette'):
        mk(reconstruct=True, overlay=0.5, palette=pal)
    with pytest.raises(hip.EssHipError, match=r'MultiStreamSegmenter: overlay= needs postprocess=True .* and a palette'):
        mk(reconstruct=True, postprocess=True, overlay=0.5)
    for bad in (-0.1, 1.5):
        with pytest.raises(hip.EssHipError, match=re.escape(f'overlay={bad} outside [0, 1]')):
            mk(reconstruct=True, postprocess=True, overlay=bad, palette=pal)
    with pytest.raises(hip.EssHipError, match=r"overlay= needs labels at the frames' size \(64, 96\), out_hw is \(32, 48\)"):
        mk(reconstruct=True, postprocess=True, overlay=0.5, palette=pal, out_hw=(32, 48))
    # the result's new slots: None by default, covered by clone()
    r = S.MultiSegmentationResult(torch.zeros(2, 2, 2, dtype=torch.uint8), valid=[True, False])
    assert r.image is None and r.frame is None and r.overlay is None
    r = S.MultiSegmentationResult(torch.zeros(2, 2, 2, dtype=torch.uint8), valid=[True, False], image=torch.ones(2, 1, 2, 2),
                                  frame=torch.ones(2, 2, 2, dtype=torch.uint8), overlay=torch.ones(2, 2, 2, 3, dtype=torch.uint8))
    c = r.clone()
    for name in ('image', 'frame', 'overlay', 'labels'):
        assert getattr(c, name) is not getattr(r, name) and torch.equal(getattr(c, name), getattr(r, name))
    assert c.colour is None and c.valid == (True, False)
