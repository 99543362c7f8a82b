"""CPU tier: the host side of the fused class head's binding (hip.seg_head / ess_seg_head) -- what it refuses before anything
reaches a device, that the library exports the declared symbol, and that the addition left the ABI version alone."""
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


def test_seg_head_symbol_is_declared_exported_and_bound(built_lib):
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    assert re.search(r'\bint\s+ess_seg_head\s*\(', header)
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, 'ess_seg_head')
    from ess_amd import hip
    assert 'ess_seg_head' in hip.EXPORTS
    assert hip.lib().ess_seg_head.argtypes is not None and len(hip.lib().ess_seg_head.argtypes) == 20
    assert hip.lib().ess_version() == 110  # (purely additive: the ABI version stays)


class _FakeDevice(torch.Tensor):
    """a CPU tensor that claims to live on the device: the argument checks run in front of any pointer being taken"""
    @property
    def is_cuda(self):
        return True


def _dev(t):
    return t.as_subclass(_FakeDevice)


def test_seg_head_refuses_on_the_host(built_lib):
    from ess_amd import hip
    C, K = 32, 11
    x = torch.zeros(1, C, 4, 6)
    w, b = torch.zeros(K, C), torch.zeros(K)
    with pytest.raises(hip.EssHipError, match=r'seg_head: x .*no CPU path'):
        hip.seg_head(x, C, w, b)
    xd = _dev(x)
    with pytest.raises(hip.EssHipError, match=r'seg_head: weight has K=65'):
        hip.seg_head(xd, C, torch.zeros(65, C), torch.zeros(65))
    with pytest.raises(hip.EssHipError, match=r'seg_head: weight must be \[K, C=32\]'):
        hip.seg_head(xd, C, torch.zeros(K, C + 8), b)
    with pytest.raises(hip.EssHipError, match=r'seg_head: palette must be a uint8 \[K=11, 3\]'):
        hip.seg_head(xd, C, w, b, palette=torch.zeros(K, 4, dtype=torch.uint8))
    with pytest.raises(hip.EssHipError, match=r'seg_head: palette must be a uint8 \[K=11, 3\]'):
        hip.seg_head(xd, C, w, b, palette=torch.zeros(K, 3, dtype=torch.int64))
    with pytest.raises(hip.EssHipError, match=r'seg_head: palette must be a uint8 \[K=11, 3\]'):
        hip.seg_head(xd, C, w, b, palette=torch.zeros(K + 1, 3, dtype=torch.uint8))
    with pytest.raises(hip.EssHipError, match=r'seg_head: bias must be \[K=11\]'):
        hip.seg_head(xd, C, w, torch.zeros(K + 1))
    with pytest.raises(hip.EssHipError, match=r'seg_head: window .* leaves the 4 x 6 source plane'):
        hip.seg_head(xd, C, w, b, window=(2, 0, 4, 6))
    with pytest.raises(hip.EssHipError, match=r'seg_head: C=24 but x has 32 channels'):
        hip.seg_head(xd, 24, torch.zeros(K, 24), b)
    with pytest.raises(hip.EssHipError, match=r'seg_head: C=40 channels do not fit'):
        hip.seg_head(_dev(torch.zeros(1, 4, 4, 6, 8, dtype=torch.bfloat16)), 40, torch.zeros(K, 40), b)
    with pytest.raises(hip.EssHipError, match=r'seg_head: x must be fp32 NCHW, BF16_C8 or F16_C8'):
        hip.seg_head(_dev(torch.zeros(1, C, 4, 6, dtype=torch.float64)), C, w, b)


def test_seg_head_library_refuses_bad_arguments(built_lib):
    """the C entry point itself: errno-style return + ess_last_error(), nothing launched (null pointers never reach a kernel)"""
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced: every call below is refused in front of the launch)
    def call(x=one, fmt=0, w=one, b=one, pal=P(0), lab=one, col=P(0), conf=P(0), N=1, C=32, K=11, H=4, W=6, win=(0, 0, 4, 6), out=(4, 6)):
        return L.ess_seg_head(x, fmt, w, b, pal, lab, col, conf, N, C, K, H, W, *win, *out, P(0))
    for kw, msg in ((dict(K=65), 'K=65'), (dict(K=0), 'K=0'), (dict(lab=P(0)), 'labels'), (dict(fmt=2), 'format 2'), (dict(col=one), 'palette'),
                    (dict(win=(1, 0, 4, 6)), 'window'), (dict(out=(0, 6)), 'H_out=0'), (dict(K=64, C=512), 'LDS'), (dict(x=P(8), fmt=1), 'aligned')):
        assert call(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())


def test_streaming_modules_import_without_a_gpu():
    from ess_amd.run_segmentation import SegmentationResult, StreamingSegmenter
    from ess_amd.e2vid.run_reconstruction import GraphedWindowState, StreamingReconstructor
    assert issubclass(StreamingSegmenter, GraphedWindowState) and issubclass(StreamingReconstructor, GraphedWindowState)
    r = SegmentationResult(torch.zeros(1, 2, 2, dtype=torch.uint8))
    assert r.colour is None and r.confidence is None and r.clone().labels is not r.labels
    from ess_amd.models.style_networks import SemSegE2VID
    assert callable(SemSegE2VID.predict)
