"""Shared by tests/test_hip_wgrad_edges.py (GPU tier) and tests/test_host_wgrad_check.py (CPU tier): the seeded inputs of a row of the
weight gradient's route-by-edge table, the float64 reference of one weight-gradient call, the bound every comparison uses and the
workspace poison.  A plain helper module: no fixtures, no collection hooks."""
import functools

import torch
import torch.nn.functional as F

NAN = float('nan')

# The project's own bounds, relative to max|ref|, per accumulated contribution:
#   'bf16': operands exact in bf16 (BF16_C8 tensors, fp32 tensors rounded while staged) -- only the fp32 summation order differs
#           (test_conv_wgrad_c8, test_conv_wgrad_head_and_stem_c8)
#   'fp32': unrounded fp32 operands on the exact-fp32 matrix core / VALU (test_conv_backward)
#   'x3'  : split operands, dY_hi X_hi + dY_hi X_lo + dY_lo X_hi against the unrounded operands (test_conv_wgrad_split_operand_bf16x3)
TOL = {'bf16': 2e-5, 'fp32': 5e-5, 'x3': 3e-5}

F32, BF16, X3 = 0, 1, 2      # ESS_COMPUTE_FP32 / BF16 / BF16X3
NCHW, C8 = 0, 1              # ESS_FMT_F32_NCHW / ESS_FMT_BF16_C8


class Case:
    """One row of WGRAD_EDGE_CASES (tests/test_hip_wgrad_edges.py) by name."""

    def __init__(self, row):
        (self.id, self.compute, self.xfmt, self.dyfmt, self.N, self.C0, self.C1, self.Cout, self.Hv, self.Wv, self.k, self.s, self.p,
         self.m0, self.m1, label, self.nsplit) = row
        self.route, *self.flags = label.split('/')
        self.Cin = self.C0 + self.C1
        self.Ho = (self.Hv + 2 * self.p - self.k) // self.s + 1
        self.Wo = (self.Wv + 2 * self.p - self.k) // self.s + 1
        self.bias = 'stem' not in self.flags
        self.nsets = 3 if 'sets3' in self.flags else 2
        self.misaligned = 'misaligned' in self.flags
        # what the kernel's operands are: BF16_C8 tensors hold bf16 values, the fp32-staged bf16 kernels round while staging
        self.rounds_f32 = self.route in ('W_BF16_K3', 'W_BF16_K3_FAST', 'W_BF16_K1')
        any_c8 = C8 in (self.xfmt, self.dyfmt)
        self.kind = 'x3' if self.compute == X3 else 'bf16' if (any_c8 or self.rounds_f32) else 'fp32'
        self.slab_floats = self.k * self.k * self.Cout * self.Cin + self.Cout

    def workspace_bytes(self):
        """What ess_conv2d_wgrad_workspace must answer if the row's route and nsplit hold (bf16x3 through BF16_C8 copies: split_layout of
        conv_wgrad.hip -- the slabs, then a hi and a lo BF16_C8 copy of X0, X1 and dY, each rounded up to 256 bytes)."""
        slabs = self.nsplit * self.slab_floats * 4
        if self.route != 'X3_VIA_C8':
            return slabs
        up = lambda v: (v + 255) & ~255
        d0, d1 = (2 if self.m0 else 1), (2 if self.m1 else 1)
        copies = [(self.C0, self.Hv // d0, self.Wv // d0), (self.C1, self.Hv // d1, self.Wv // d1), (self.Cout, self.Ho, self.Wo)]
        return up(slabs) + sum(2 * up(self.N * ((C + 7) // 8) * h * w * 16) for C, h, w in copies)


def bfr(x):
    """round to bf16 (nearest even, as cvt8 and ess_to_bf16_c8 do) and back"""
    return x.bfloat16().float()


def _up(x, mode):
    if mode == 1:
        return F.interpolate(x, scale_factor=2, mode='nearest')
    if mode == 2:
        z = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
        z[:, :, ::2, ::2] = x
        return z
    return x


def virtual_input(x0, x1, m0, m1):
    return _up(x0, m0) if x1 is None else torch.cat([_up(x0, m0), _up(x1, m1)], 1)


def _autograd(x0, x1, dy, k, s, p, m0, m1, dtype):
    xin = virtual_input(x0.to(dtype), None if x1 is None else x1.to(dtype), m0, m1)
    w = torch.zeros(dy.shape[1], xin.shape[1], k, k, dtype=dtype, requires_grad=True)
    b = torch.zeros(dy.shape[1], dtype=dtype, requires_grad=True)
    F.conv2d(xin, w, b, s, p).backward(dy.to(dtype))
    return w.grad, b.grad


def wgrad_reference(x0, x1, dy, k, s, p, m0, m1):
    """(dw, db) in float64 on the CPU: F.conv2d autograd over the virtual input (nearest / zero-insert upsampling, then the concat).
    The operands are the values the kernel reads (see kernel_operands)."""
    return _autograd(x0, x1, dy, k, s, p, m0, m1, torch.float64)


def wgrad_fp32_standin(x0, x1, dy, k, s, p, m0, m1):
    """The same in fp32: what a correct kernel is allowed to be (the CPU tier's stand-in for one)."""
    return _autograd(x0, x1, dy, k, s, p, m0, m1, torch.float32)


def case_sets(case):
    """The case's seeded (x0, x1, dy) sets as they are handed to the library: fp32 CPU tensors, already bf16 values where the tensor is
    stored as BF16_C8.  Set 0 is the plain call's."""
    c = case
    g = torch.Generator().manual_seed(sum(map(ord, c.id)))
    d0, d1 = (2 if c.m0 else 1), (2 if c.m1 else 1)
    rx = bfr if c.xfmt == C8 else (lambda t: t)
    ry = bfr if c.dyfmt == C8 else (lambda t: t)
    sets = []
    for _ in range(c.nsets):
        x0 = rx(torch.randn(c.N, c.C0, c.Hv // d0, c.Wv // d0, generator=g))
        x1 = rx(torch.randn(c.N, c.C1, c.Hv // d1, c.Wv // d1, generator=g)) if c.C1 else None
        dy = ry(torch.randn(c.N, c.Cout, c.Ho, c.Wo, generator=g))
        sets.append((x0, x1, dy))
    return sets


def kernel_operands(case, x0, x1, dy):
    """The values the kernel contracts: bf16-rounded where the route rounds fp32 tensors while staging them, the tensors themselves
    otherwise (BF16_C8 tensors are bf16 values already; the fp32 routes and split operands see every bit)."""
    if case.rounds_f32:
        return bfr(x0), None if x1 is None else bfr(x1), bfr(dy)
    return x0, x1, dy


@functools.lru_cache(maxsize=None)
def case_reference(row):
    """(case, sets, [(dw, db) float64 per set]) of a table row, computed once per process and shared by the tests that need it: do not
    write into what it returns."""
    case = Case(row)
    sets = case_sets(case)
    refs = [wgrad_reference(*kernel_operands(case, *q), case.k, case.s, case.p, case.m0, case.m1) for q in sets]
    return case, sets, refs


def excess(got, ref, passes, kind):
    """max|got - ref| as a multiple of the bound passes * tol * max|ref|"""
    got, ref = got.detach().double().cpu(), ref.double()
    return ((got - ref).abs().max() / (passes * TOL[kind] * ref.abs().max())).item()


def check(got, ref, passes, kind, what=''):
    """No element is NaN (an element a kernel left unwritten in a poisoned output or slab), then max|got - ref| <= passes * tol * max|ref|.
    passes: the number of accumulated contributions -- sets, plus one when accumulating onto a prior value."""
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f'{what}: {nan} of {got.numel()} elements are NaN'
    e = excess(got, ref, passes, kind)
    assert e <= 1.0, f'{what}: max|got - ref| is {e:.3g} x the bound {passes} * {TOL[kind]:g} * max|ref|'
    return e


def poison_workspace(H, spec, src0, dy):
    """Every byte of the cached weight-gradient workspace this call will use becomes 0xFF (every fp32 in it a NaN): a slab element the
    kernels do not write reaches dw / db as NaN instead of as an earlier call's value.  Call it before EVERY launch under test."""
    H.wgrad_workspace(spec, src0, dy).fill_(0xFF)
