"""CPU tier: the host side of multi-stream streaming segmentation -- the two entry points it adds (ess_event_normalize_samples,
ess_state_carry_masked: declared, exported, bound, ABI version untouched), what their wrappers and the library refuse before anything
reaches a device, what MultiStreamSegmenter refuses, and the per-round schedule of mode words as a function on lists."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built_lib():
    sys.path.insert(0, ROOT)
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
    for name, nargs in (('ess_event_normalize_samples', 7), ('ess_state_carry_masked', 7)):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
        fn = getattr(hip.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert hip.lib().ess_version() == 110  # (purely additive: the ABI version stays)
    assert (hip.CARRY_HOLD, hip.CARRY_TAKE, hip.CARRY_ZERO) == (0, 1, 2)
    for word, value in (('ESS_CARRY_HOLD', 0), ('ESS_CARRY_TAKE', 1), ('ESS_CARRY_ZERO', 2)):
        assert re.search(word + r'\s*=\s*%d\b' % value, header)


def test_event_normalize_samples_refuses_on_the_host(built_lib):
    from ess_amd import hip
    x = torch.zeros(3, 5, 8, 8)
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: x .*no CPU path'):
        hip.event_normalize_samples(x)
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: x must be .*\[S, C, H, W\].*\(5, 8, 8\)'):
        hip.event_normalize_samples(_dev(torch.zeros(5, 8, 8)))
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: x must be .*float64'):
        hip.event_normalize_samples(_dev(x.double()))
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: x must be'):
        hip.event_normalize_samples(_dev(x.permute(0, 1, 3, 2)[:, :, :, ::2]))
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: mode .*no CPU path'):
        hip.event_normalize_samples(_dev(x), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: mode must be a contiguous int32 \[3\]'):
        hip.event_normalize_samples(_dev(x), _dev(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: mode must be a contiguous int32 \[3\]'):
        hip.event_normalize_samples(_dev(x), _dev(torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(hip.EssHipError, match=r'event_normalize_samples: out must be'):
        hip.event_normalize_samples(_dev(x), None, out=_dev(torch.zeros(3, 5, 8, 4)))


def test_state_carry_masked_refuses_on_the_host(built_lib):
    from ess_amd import hip
    mode = _dev(torch.zeros(3, dtype=torch.int32))
    a, b = torch.zeros(3, 4, 2, 2), torch.zeros(3, 4, 2, 2)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: dst\[0\] .*no CPU path'):
        hip.state_carry_masked([a], [b], mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: src\[0\] .*no CPU path'):
        hip.state_carry_masked([_dev(a)], [b], mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: 17 tensors \(1\.\.16'):
        hip.state_carry_masked([_dev(a)] * 17, None, mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: 0 tensors'):
        hip.state_carry_masked([], None, mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: 2 source tensors for 1 destinations'):
        hip.state_carry_masked([_dev(a)], [_dev(b), _dev(b)], mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: src\[0\] is torch.float16'):
        hip.state_carry_masked([_dev(a)], [_dev(b.half())], mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: src\[0\] is .*\(3, 4, 2, 4\)'):
        hip.state_carry_masked([_dev(a)], [_dev(torch.zeros(3, 4, 2, 4))], mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: dst\[1\] has 2 streams, dst\[0\] has 3'):
        hip.state_carry_masked([_dev(a), _dev(torch.zeros(2, 4, 2, 2))], None, mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: dst\[0\] has 12 bytes per stream'):
        hip.state_carry_masked([_dev(torch.zeros(3, 3))], None, mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: dst\[0\] must be a non-empty contiguous'):
        hip.state_carry_masked([_dev(torch.zeros(3, 4, 8)[:, :, ::2])], None, mode)
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: mode .*no CPU path'):
        hip.state_carry_masked([_dev(a)], None, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(hip.EssHipError, match=r'state_carry_masked: mode must be a contiguous int32 \[3\]'):
        hip.state_carry_masked([_dev(a)], None, _dev(torch.zeros(2, dtype=torch.int32)))


def test_library_refuses_bad_arguments(built_lib):
    """the C entry points themselves: errno-style return + ess_last_error(), nothing launched (the fake pointers never reach a kernel)"""
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced: every call below is refused in front of the launch)

    def carry(n=1, S=2, nbytes=64, dst=16, src=32, mode=one, with_src=True):
        d = (P * max(n, 1))(*[dst] * max(n, 1))
        s = (P * max(n, 1))(*[src] * max(n, 1)) if with_src else None
        b = (ctypes.c_int64 * max(n, 1))(*[nbytes] * max(n, 1))
        return L.ess_state_carry_masked(d, s, b, n, S, mode, P(0))
    for kw, msg in ((dict(n=17), 'n_tensors=17'), (dict(n=0), 'n_tensors=0'), (dict(S=0), 'n_samples=0'), (dict(S=-3), 'n_samples=-3'),
                    (dict(nbytes=24), 'bytes_per_sample[0]=24'), (dict(nbytes=0), 'bytes_per_sample[0]=0'), (dict(dst=8), 'dst[0]'),
                    (dict(dst=0), 'dst[0]'), (dict(src=40), 'src[0]'), (dict(src=0), 'src[0]'), (dict(mode=P(0)), 'mode'),
                    (dict(dst=16, src=32), 'overlap'), (dict(dst=1024, src=1024 - 64), 'overlap'), (dict(dst=4096, src=4096), 'overlap')):
        assert carry(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())

    def norm(x=one, y=one, S=2, chunk=64, mode=P(0), ws=one):
        return L.ess_event_normalize_samples(x, y, S, chunk, mode, ws, P(0))
    for kw, msg in ((dict(S=0), 'S=0'), (dict(S=-1), 'S=-1'), (dict(S=70000), 'S=70000'), (dict(chunk=0), 'chunk=0'), (dict(x=P(0)), 'null'),
                    (dict(ws=P(0)), 'null')):
        assert norm(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())


def test_schedule_of_mode_words():
    """pure host logic: a pending restart of an idle stream stays pending; restart + active = ZERO in front of the step, TAKE behind
    it; idle = HOLD / HOLD; an advancing stream = HOLD / TAKE"""
    from ess_amd import hip
    from ess_amd.run_segmentation import stream_modes
    H, T, Z = hip.CARRY_HOLD, hip.CARRY_TAKE, hip.CARRY_ZERO
    #                pending               active
    pre, post, pend = stream_modes([True, True, False, False], [True, False, True, False])
    assert pre == [Z, H, H, H] and post == [T, H, T, H] and pend == [False, True, False, False]
    # the restart that stayed pending fires at the stream's next active window, once
    pre, post, pend = stream_modes(pend, [True, True, True, True])
    assert pre == [H, Z, H, H] and post == [T, T, T, T] and pend == [False] * 4
    pre, post, pend = stream_modes(pend, [True, True, True, True])
    assert pre == [H] * 4 and post == [T] * 4 and pend == [False] * 4
    pre, post, pend = stream_modes([True], [False])
    assert (pre, post, pend) == ([H], [H], [True])
    with pytest.raises(hip.EssHipError, match='2 pending flags for 3 streams'):
        stream_modes([True, False], [True, True, True])


def test_driver_refusals_name_the_offending_value():
    from ess_amd import hip
    from ess_amd import run_segmentation as R
    for bad in (0, -2, 1.5, None, True):
        with pytest.raises(hip.EssHipError, match=re.escape(f'n_streams={bad!r}')):
            R.MultiStreamSegmenter(None, None, 64, 96, None, bad)
    with pytest.raises(hip.EssHipError, match=r'expected \[3, 5, 64, 96\] voxel grids .* got \(1, 5, 64, 96\)'):
        R.check_stream_grids(torch.zeros(1, 5, 64, 96).shape, 3, 5, 64, 96)
    with pytest.raises(hip.EssHipError, match=r'got \(3, 5, 64, 95\)'):
        R.check_stream_grids((3, 5, 64, 95), 3, 5, 64, 96)
    R.check_stream_grids((3, 5, 64, 96), 3, 5, 64, 96)
    with pytest.raises(hip.EssHipError, match=r'active has 2 entries, .* n_streams=3'):
        R.check_active([True, False], 3)
    assert R.check_active(None, 3) == [True] * 3
    assert R.check_active(torch.tensor([1, 0, 1], dtype=torch.bool), 3) == [True, False, True]
    with pytest.raises(hip.EssHipError, match=r'got 2, .* n_streams=3'):
        R.check_stream_events([None, None], 3)
    with pytest.raises(hip.EssHipError, match=r'got Tensor'):
        R.check_stream_events(torch.zeros(3, 10, 4), 3)
    with pytest.raises(hip.EssHipError, match=r'events\[1\] must be \[N, 4\].* got \(10, 3\)'):
        R.check_stream_events([None, torch.zeros(10, 3), None], 3)
    evs, active = R.check_stream_events([torch.zeros(10, 4), None, torch.zeros(0, 4)], 3)
    assert active == [True, False, False] and evs[1] is None and evs[2] is None
    # update() itself runs these checks in front of any device work: the methods need no built state to refuse
    seg = R.MultiStreamSegmenter.__new__(R.MultiStreamSegmenter)
    seg.n_streams, seg.num_bins, seg.height, seg.width = 3, 5, 64, 96
    with pytest.raises(hip.EssHipError, match=r'got \(1, 5, 64, 96\)'):
        seg.update(torch.zeros(1, 5, 64, 96))
    with pytest.raises(hip.EssHipError, match=r'active has 4 entries'):
        seg.update(torch.zeros(3, 5, 64, 96), active=[True] * 4)
    with pytest.raises(hip.EssHipError, match=r'got 1, .* n_streams=3'):
        seg.update_from_events([None])
    r = R.MultiSegmentationResult(torch.zeros(2, 2, 2, dtype=torch.uint8), valid=[True, False])
    c = r.clone()
    assert c.colour is None and c.confidence is None and c.labels is not r.labels and c.valid == (True, False)


def test_norm_split_tuning_key_round_trip(built_lib):
    """'norm_split_wgs': set / get, the named value that makes the split independent of the batch size, and a value <= 0 returns to the
    process's own setting (the environment variable, else 1024) -- a set / restore pair leaves the process as it was"""
    from ess_amd import hip
    own = int(os.environ.get('ESS_NORM_SPLIT_WGS', 1024))
    prev = hip.tuning_get('norm_split_wgs')
    assert prev == own
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    assert re.search(r'#define\s+ESS_NORM_SPLIT_BY_PLANE\s+\(1\s*<<\s*30\)', header) and hip.NORM_SPLIT_BY_PLANE == 1 << 30
    try:
        hip.tuning_set('norm_split_wgs', hip.NORM_SPLIT_BY_PLANE)
        assert hip.tuning_get('norm_split_wgs') == 1 << 30
        hip.tuning_set('norm_split_wgs', 0)
        assert hip.tuning_get('norm_split_wgs') == own
        hip.tuning_set('norm_split_wgs', 77)
        assert hip.tuning_get('norm_split_wgs') == 77
    finally:
        hip.tuning_set('norm_split_wgs', prev)
    assert hip.tuning_get('norm_split_wgs') == own
