"""
Side copies of an activation: one record per tensor, one validity rule.

An activation on the hot path can exist in several forms at once -- the tensor autograd and the callers see, plus copies its producer
wrote next to it for the consumers that stage from them -- and sometimes the tensor itself has no memory behind it at all.  All of
that lives in ONE record, the tensor attribute `ess_copies`, stamped with the tensor's `_version` when the record was started:

  c8         BF16_C8 staging copy of an fp32 tensor (bf16 configuration: what a following convolution stages from)
  h16        (F16_C8 tensor, hilo): the half copy of the 'mixed' configuration; hilo: a [hi | lo] pair
  f32c8      channel-blocked fp32 values (the lean ConvGRU state between time steps)
  pair       the [hi | lo] half pair of a pre-norm output whose own tensor is a bf16-typed placeholder (only the norm kernels read it)
  mixed      (BF16_C8 tensor, want_hilo): what functional.as_c8 made of this tensor in the 'mixed' configuration
  unwritten  the tensor's own values were never written (a stride-0 placeholder, or a buffer only the copies of which were computed)

The rule: a copy is readable while the tensor's `_version` equals the record's stamp -- an in-place write expires all of them at
once.  `unwritten` describes the tensor's own storage and never expires.  Attaching to a tensor whose record is stale starts a fresh
record (keeping `unwritten`).  A kernel that rewrites a tensor through its raw pointer (a graph replay, the state carry) moves no
version: whoever does that rewrites the copies too (the streaming drivers' static state).  The record dies with the tensor; python
attributes do not survive `detach()` or a pass through an autograd.Function, hence `carry`.  (`hip.is_f16_c8`'s `ess_f16` is no
copy but the format tag of a tensor's own bytes, and stays in hip.py.)
"""
import collections

import torch

_ATTR = 'ess_copies'


class Copies:
    __slots__ = ('stamp', 'c8', 'h16', 'f32c8', 'pair', 'mixed', 'unwritten')

    def __init__(self, stamp, unwritten):
        self.stamp, self.unwritten = stamp, unwritten
        self.c8 = self.h16 = self.f32c8 = self.pair = self.mixed = None


# what `of` answers without a valid record: shared, hence read-only (writing goes through `attach`, which never sees these)
_NONE = collections.namedtuple('NoCopies', Copies.__slots__)(None, None, None, None, None, None, False)
_UNWRITTEN = _NONE._replace(unwritten=True)


def of(t):
    """The valid record of `t`, else an empty one (that still says `unwritten`): `copies.of(t).c8` is the copy or None."""
    r = getattr(t, _ATTR, None)
    if r is None:
        return _NONE
    if r.stamp == t._version:
        return r
    return _UNWRITTEN if r.unwritten else _NONE


def attach(t, **fields):
    """Set fields of `t`'s record (a fresh one when there is none or `t` was modified since it was started) -> t."""
    r = getattr(t, _ATTR, None)
    if r is None or r.stamp != t._version:
        r = Copies(t._version, r is not None and r.unwritten)
        setattr(t, _ATTR, r)
    for k, v in fields.items():
        setattr(r, k, v)
    return t


def placeholder(shape, device, **fields):
    """The fp32 tensor of an activation that exists as copies only: a stride-0 view of ONE element (no memory behind it) carrying
    shape, device and the copies; marked unwritten, so `require_fp32` refuses its values."""
    return attach(torch.empty((), dtype=torch.float32, device=device).expand(*shape), unwritten=True, **fields)


def carry(dst, src, *names):
    """Hand the named fields of `src`'s record on to `dst`, an alias of the same values (detach, fork, a tensor handed through an
    autograd.Function), stamped with dst's version.  Only what is named travels: a carried buffer lives as long as `dst`. -> dst"""
    r = of(src)
    found = {k: getattr(r, k) for k in names if getattr(r, k) is not None and getattr(r, k) is not False}
    return attach(dst, **found) if found else dst


def require_fp32(t):
    """The fp32 tensor itself -- refused when only copies of it exist."""
    if of(t).unwritten:
        from .hip import EssHipError  # (the only thing here that is not torch: hip.py imports this module)
        raise EssHipError('this tensor was produced as a BF16_C8 copy only (lean recurrent state / internal activation); '
                          'its fp32 values do not exist')
    return t
