"""CPU tier: the host side of compacted multi-stream rounds -- the entry point they add (ess_state_carry_indexed: declared, exported,
bound, ABI version untouched), what its wrapper and the library refuse before anything reaches a device, and the two functions on
host lists that decide a round: compact_buckets (which batch sizes are prepared) and compact_plan (slots, index tables, restarts)."""
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


def test_symbol_is_declared_exported_and_bound(built_lib):
    header = open(os.path.join(ROOT, 'include', 'ess_hip.h')).read()
    lib = ctypes.CDLL(built_lib)
    from ess_amd import hip
    name = 'ess_state_carry_indexed'
    assert re.search(r'\bint\s+' + name + r'\s*\(', header)
    assert hasattr(lib, name)
    assert name in hip.EXPORTS
    fn = getattr(hip.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    assert hip.lib().ess_version() == 110  # (purely additive: the ABI version stays)
    assert hip.CARRY_SRC_ZERO == -1
    assert re.search(r'ESS_CARRY_SRC_ZERO\s*=\s*-1\b', header)


def test_state_carry_indexed_refuses_on_the_host(built_lib):
    from ess_amd import hip
    di, si = _dev(torch.zeros(3, dtype=torch.int32)), _dev(torch.zeros(3, dtype=torch.int32))
    a, b = torch.zeros(3, 4, 2, 2), torch.zeros(5, 4, 2, 2)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: dst\[0\] .*no CPU path'):
        hip.state_carry_indexed([a], [b], di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src\[0\] .*no CPU path'):
        hip.state_carry_indexed([_dev(a)], [b], di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: dst\[0\] must be a non-empty contiguous'):
        hip.state_carry_indexed([_dev(torch.zeros(3, 4, 8)[:, :, ::2])], None, di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src\[0\] must be a non-empty contiguous'):
        hip.state_carry_indexed([_dev(torch.zeros(3, 4, 4))], [_dev(torch.zeros(5, 4, 8)[:, :, ::2])], di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: 17 tensors \(1\.\.16'):
        hip.state_carry_indexed([_dev(a)] * 17, None, di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: 0 tensors'):
        hip.state_carry_indexed([], None, di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src\[0\] is torch.float16'):
        hip.state_carry_indexed([_dev(a)], [_dev(b.half())], di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src\[0\] is .*\(5, 4, 2, 4\)'):
        hip.state_carry_indexed([_dev(a)], [_dev(torch.zeros(5, 4, 2, 4))], di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: dst\[0\] has 12 bytes per stream'):
        hip.state_carry_indexed([_dev(torch.zeros(3, 3))], None, di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: dst\[1\] has 2 streams, dst\[0\] has 3'):
        hip.state_carry_indexed([_dev(a), _dev(torch.zeros(2, 4, 2, 2))], None, di, si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src\[1\] has 3 streams, src\[0\] has 5'):
        hip.state_carry_indexed([_dev(a), _dev(a)], [_dev(b), _dev(a.clone())], di, si)
    # the tables themselves take different first dimensions on the two sides
    table = hip.StateMoveTable([_dev(a)], [_dev(b)])
    assert (table.n, table.S_dst, table.S_src, table.bytes_per_sample) == (1, 3, 5, [64])
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: dst_index .*no CPU path'):
        table.run(torch.zeros(3, dtype=torch.int32), si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src_index .*no CPU path'):
        table.run(di, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: 3 dst_index entries for 4 src_index entries'):
        table.run(di, _dev(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: src_index must be a contiguous int32 .*int64'):
        table.run(di, _dev(torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: dst_index must be a contiguous int32'):
        table.run(_dev(torch.zeros(6, dtype=torch.int32)[::2]), si)
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: 0 moves \(1\.\.65535'):
        table.run(_dev(torch.zeros(0, dtype=torch.int32)), _dev(torch.zeros(0, dtype=torch.int32)))
    with pytest.raises(hip.EssHipError, match=r'state_carry_indexed: 65536 moves'):
        table.run(_dev(torch.zeros(65536, dtype=torch.int32)), _dev(torch.zeros(65536, dtype=torch.int32)))


def test_library_refuses_bad_arguments(built_lib):
    """the C entry point itself: errno-style return + ess_last_error(), nothing launched (the fake pointers never reach a kernel)"""
    from ess_amd import hip
    L = hip.lib()
    P = ctypes.c_void_p
    one = P(16)  # (never dereferenced: every call below is refused in front of the launch)

    def move(n=1, n_dst=2, n_src=3, n_moves=2, nbytes=64, dst=4096, src=8192, di=one, si=one, with_src=True):
        d = (P * max(n, 1))(*[dst] * max(n, 1))
        s = (P * max(n, 1))(*[src] * max(n, 1)) if with_src else None
        b = (ctypes.c_int64 * max(n, 1))(*[nbytes] * max(n, 1))
        return L.ess_state_carry_indexed(d, s, b, n, n_dst, n_src, n_moves, di, si, P(0))
    for kw, msg in ((dict(n=17), 'n_tensors=17'), (dict(n=0), 'n_tensors=0'), (dict(n_dst=0), 'n_dst_samples=0'),
                    (dict(n_dst=65536), 'n_dst_samples=65536'), (dict(n_src=0), 'n_src_samples=0'), (dict(n_src=-3), 'n_src_samples=-3'),
                    (dict(n_moves=0), 'n_moves=0'), (dict(n_moves=65536), 'n_moves=65536'),
                    (dict(nbytes=24), 'bytes_per_sample[0]=24'), (dict(nbytes=0), 'bytes_per_sample[0]=0'), (dict(dst=8), 'dst[0]'),
                    (dict(dst=0), 'dst[0]'), (dict(src=40), 'src[0]'), (dict(src=0), 'src[0]'), (dict(di=P(0)), 'dst_index'),
                    (dict(si=P(0)), 'src_index'),
                    # [dst, dst + n_dst * bytes) against [src, src + n_src * bytes): each side with its OWN record count
                    (dict(dst=4096, src=4096), 'overlap'), (dict(dst=4096, src=4096 + 64), 'overlap'),
                    (dict(dst=4096, src=4096 - 2 * 64), 'overlap'), (dict(dst=4096 + 2 * 64, src=4096), 'overlap')):
        assert move(**kw) == -22, kw
        assert msg in L.ess_last_error().decode(), (kw, L.ess_last_error().decode())
        assert 'state_carry_indexed' in L.ess_last_error().decode()


def test_compact_buckets():
    from ess_amd import hip
    from ess_amd.run_segmentation import compact_buckets
    assert compact_buckets(1) == ()
    assert compact_buckets(2) == (1,)
    assert compact_buckets(3) == (1, 2)
    assert compact_buckets(5) == (1, 2, 4)
    assert compact_buckets(8) == (1, 2, 4)
    assert compact_buckets(8, [2, 7]) == (2, 7)
    assert compact_buckets(8, ()) == ()
    # ... which is the helper MultiStreamSegmenter's constructor calls on its compact_buckets argument
    for bad in ([2, 2], [0], [8], [4, 2], [1.0], [True], 'ab', 3):
        with pytest.raises(hip.EssHipError, match='compact_buckets='):
            compact_buckets(8, bad)


def test_compact_plan():
    from ess_amd import hip
    from ess_amd.run_segmentation import compact_plan
    T, F = True, False
    p = compact_plan([T, F, T, F, F], [F, T, T, F, T], (1, 2, 4))
    assert p.bucket == 4
    assert p.rows == [1, 2, 4]
    assert p.gather_dst == [0, 1, 2, 3]
    assert p.gather_src == [1, -1, 4, -1] and hip.CARRY_SRC_ZERO == -1
    assert p.norm_mode == [1, 1, 1, 0]
    assert p.scatter_dst == [1, 2, 4, -2]
    assert p.scatter_src == [0, 1, 2, 3]
    assert p.pending_after == [T, F, F, F, F]
    # all five active: no bucket holds them, the round rides along
    assert compact_plan([F] * 5, [T] * 5, (1, 2, 4)) is None
    # none active: the smallest bucket, fully padded; pending restarts stay
    p = compact_plan([T, F, T, F, F], [F] * 5, (1, 2, 4))
    assert (p.bucket, p.rows, p.gather_dst, p.gather_src, p.norm_mode, p.scatter_dst, p.scatter_src) == (1, [], [0], [-1], [0], [-2], [0])
    assert p.pending_after == [T, F, T, F, F]
    assert compact_plan([F] * 5, [F] * 5, ()) is None
    # an exact fit has no padding; a restart requested while idle is served when the stream is next active
    p = compact_plan([F, T, F], [T, F, T], (1, 2))
    assert (p.bucket, p.rows, p.gather_src, p.norm_mode, p.scatter_dst, p.pending_after) == (2, [0, 2], [0, 2], [1, 1], [0, 2], [F, T, F])
    p = compact_plan(p.pending_after, [F, T, F], (1, 2))
    assert (p.bucket, p.rows, p.gather_src, p.scatter_dst, p.pending_after) == (1, [1], [-1], [1], [F, F, F])
    assert compact_plan([F] * 3, [T, T, T], (1, 2)) is None
    with pytest.raises(hip.EssHipError, match='2 pending flags for 3 streams'):
        compact_plan([T, F], [T, T, T], (1, 2))
