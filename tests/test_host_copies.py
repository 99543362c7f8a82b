"""CPU tier: the one validity rule of an activation's side copies (ess_amd/copies.py).  `_version` counts in-place writes of CPU
tensors as it does on the device, so the rule is checked here without one."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ess_amd import copies  # noqa: E402

COPY_FIELDS = ('c8', 'h16', 'f32c8', 'pair', 'mixed')


def _all_fields():
    return {'c8': torch.zeros(1), 'h16': (torch.zeros(2), True), 'f32c8': torch.zeros(3), 'pair': torch.zeros(4),
            'mixed': (torch.zeros(5), False)}


def test_no_record_reads_as_empty():
    t = torch.zeros(2, 8, 4, 4)
    r = copies.of(t)
    assert all(getattr(r, k) is None for k in COPY_FIELDS) and r.unwritten is False
    assert copies.of(None).c8 is None and copies.of(None).unwritten is False  # (an absent state reads as no copies)
    assert copies.of(t) is copies.of(torch.zeros(1))  # (one shared empty record: a miss allocates nothing)
    assert copies.require_fp32(t) is t
    with pytest.raises(AttributeError):  # (the shared empty record is read-only: a write on a miss must not reach every tensor)
        copies.of(t).c8 = torch.zeros(1)
    with pytest.raises(AttributeError):
        copies.of(t).unwritten = True


def test_in_place_write_expires_every_copy_but_not_unwritten():
    t = torch.zeros(2, 8, 4, 4)
    fields = _all_fields()
    copies.attach(t, unwritten=True, **fields)
    r = copies.of(t)
    assert all(getattr(r, k) is fields[k] for k in COPY_FIELDS) and r.unwritten is True
    t.add_(1.0)
    r = copies.of(t)
    assert all(getattr(r, k) is None for k in COPY_FIELDS)
    assert r.unwritten is True
    t.mul_(2.0)
    assert copies.of(t).unwritten is True and copies.of(t).c8 is None


def test_in_place_write_without_the_mark_leaves_nothing():
    t = torch.zeros(4)
    copies.attach(t, c8=torch.zeros(1))
    t.zero_()
    r = copies.of(t)
    assert r.c8 is None and r.unwritten is False


def test_attach_to_a_stale_record_starts_a_fresh_one():
    t = torch.zeros(2, 8, 4, 4)
    old, new = torch.zeros(1), torch.zeros(2)
    copies.attach(t, c8=old, f32c8=old, unwritten=True)
    t.add_(1.0)
    copies.attach(t, h16=(new, False))
    r = copies.of(t)
    assert r.h16[0] is new and r.h16[1] is False
    assert r.c8 is None and r.f32c8 is None  # (the stale copies did not come back with the new stamp)
    assert r.unwritten is True  # (kept: it describes the tensor's own storage)
    assert r.stamp == t._version


def test_two_fields_attached_at_the_same_version_are_both_readable():
    t = torch.zeros(2, 8, 4, 4)
    a, b = torch.zeros(1), torch.zeros(2)
    copies.attach(t, c8=a)
    copies.attach(t, h16=(b, True))
    r = copies.of(t)
    assert r.c8 is a and r.h16[0] is b and r.h16[1] is True
    copies.attach(t, c8=b)  # (same version: the field is replaced, the other one stays)
    assert copies.of(t).c8 is b and copies.of(t).h16[0] is b


def test_attach_returns_the_tensor_and_refuses_unknown_fields():
    t = torch.zeros(3)
    assert copies.attach(t, c8=torch.zeros(1)) is t
    with pytest.raises(AttributeError):
        copies.attach(t, c9=torch.zeros(1))


def test_carry_moves_only_the_named_fields_and_restamps():
    src = torch.zeros(2, 8, 4, 4)
    src.add_(1.0)
    src.add_(1.0)  # (source and destination versions differ)
    fields = _all_fields()
    copies.attach(src, unwritten=True, **fields)
    dst = src.detach()
    dst = dst.view(2, 8, 16)  # (any alias: a fresh python object without attributes)
    assert copies.of(dst).c8 is None
    assert copies.carry(dst, src, 'c8', 'h16', 'unwritten') is dst
    r = copies.of(dst)
    assert r.c8 is fields['c8'] and r.h16 is fields['h16'] and r.unwritten is True
    assert r.f32c8 is None and r.pair is None and r.mixed is None
    assert r.stamp == dst._version
    one = copies.carry(torch.zeros(3), src, 'h16')
    r = copies.of(one)
    assert r.h16 is fields['h16'] and r.c8 is None and r.unwritten is False
    assert r.stamp == one._version == 0 and copies.of(src).stamp == src._version == 2
    # the source's record is untouched, and a later write to the destination expires the destination's record alone
    one.add_(1.0)
    assert copies.of(one).h16 is None and copies.of(src).h16 is fields['h16']


def test_carry_from_a_stale_or_empty_source_moves_nothing():
    src = torch.zeros(4)
    copies.attach(src, c8=torch.zeros(1))
    src.add_(1.0)
    dst = copies.carry(torch.zeros(4), src, 'c8', 'h16', 'unwritten')
    r = copies.of(dst)
    assert r.c8 is None and r.h16 is None and r.unwritten is False
    dst = copies.carry(torch.zeros(4), torch.zeros(4), 'c8')
    assert copies.of(dst).c8 is None


def test_placeholder_has_stride_0_and_require_fp32_refuses_it():
    from ess_amd import hip
    c8 = torch.zeros(2, 1, 4, 4, 8, dtype=torch.bfloat16)
    t = copies.placeholder((2, 8, 4, 4), torch.device('cpu'), c8=c8)
    assert tuple(t.shape) == (2, 8, 4, 4) and t.dtype == torch.float32
    assert t.stride() == (0, 0, 0, 0)
    assert t.untyped_storage().nbytes() == 4  # (ONE element behind the whole shape)
    r = copies.of(t)
    assert r.unwritten is True and r.c8 is c8 and r.h16 is None
    with pytest.raises(hip.EssHipError, match='its fp32 values do not exist'):
        copies.require_fp32(t)
    bare = copies.placeholder(torch.Size([1, 8, 2, 2]), torch.device('cpu'))
    assert bare.stride() == (0, 0, 0, 0) and copies.of(bare).unwritten is True and copies.of(bare).c8 is None
    with pytest.raises(hip.EssHipError):
        copies.require_fp32(bare)
