"""CPU tier: what the glue wrappers of ess_amd/hip.py refuse before they take a pointer.  The kernels index every operand with the first
operand's extents (and the 2x2 sum pool strides its input by 2 W_out), so a mismatched second operand / destination or an odd pooled
extent would read or write the wrong elements without any error from the library.  The checks precede ptr(): CPU tensors reach them,
and neither a GPU nor the built library is needed -- each refusal must name the wrapper's own check, not ptr()'s "CPU tensor" one."""
import pytest
import torch

from ess_amd import hip


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


REFUSALS = [
    ('sumpool odd W', lambda: hip.sumpool2x2(z(2, 3, 6, 11)), 'sumpool2x2: input extents'),
    ('sumpool odd H', lambda: hip.sumpool2x2(z(2, 3, 7, 10)), 'sumpool2x2: input extents'),
    ('sumpool odd both', lambda: hip.sumpool2x2(z(1, 1, 1, 1)), 'sumpool2x2: input extents'),
    ('sumpool out of the input shape', lambda: hip.sumpool2x2(z(2, 3, 6, 10), out=z(2, 3, 6, 10)), 'sumpool2x2: out has shape'),
    ('sumpool out transposed', lambda: hip.sumpool2x2(z(2, 3, 6, 10), out=z(2, 3, 5, 3), accumulate=True), 'sumpool2x2: out has shape'),
    ('sumpool out flat', lambda: hip.sumpool2x2(z(2, 3, 6, 10), out=z(90)), 'sumpool2x2: out has shape'),
    ('add b shorter', lambda: hip.add(z(16), z(12)), 'add: b has shape'),
    ('add b same numel', lambda: hip.add(z(4, 6), z(6, 4)), 'add: b has shape'),
    ('add out shorter', lambda: hip.add(z(16), z(16), out=z(8)), 'add: out has shape'),
    ('add out same numel', lambda: hip.add(z(2, 8), z(2, 8), out=z(16)), 'add: out has shape'),
    ('bilinear b smaller', lambda: hip.upsample_bilinear2x_add(z(2, 3, 4, 6), z(2, 3, 4, 5)), 'upsample_bilinear2x_add: b has shape'),
    ('bilinear b fewer planes', lambda: hip.upsample_bilinear2x_add(z(2, 3, 4, 6), z(1, 3, 4, 6)), 'upsample_bilinear2x_add: b has shape'),
    ('bilinear c8 b smaller', lambda: hip.upsample_bilinear2x_add_c8(z(2, 8, 4, 6), z(2, 8, 3, 6)), 'upsample_bilinear2x_add_c8: b has shape'),
    ('bilinear c8c8 b fewer blocks', lambda: hip.upsample_bilinear2x_add_c8_from_c8(z(2, 2, 4, 6, 8, dtype=torch.bfloat16),
                                                                                   z(2, 1, 4, 6, 8, dtype=torch.bfloat16)),
     'upsample_bilinear2x_add_c8_from_c8: b8 has shape'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_wrapper_refuses_before_taking_a_pointer(case):
    _, call, message = case
    with pytest.raises(hip.EssHipError) as e:
        call()
    assert message in str(e.value), str(e.value)
    assert 'CPU tensor' not in str(e.value)


ACCEPTED = [
    ('sumpool', lambda: hip.sumpool2x2(z(2, 3, 6, 10))),
    ('sumpool out', lambda: hip.sumpool2x2(z(2, 3, 6, 10), out=z(2, 3, 3, 5), accumulate=True)),
    ('add', lambda: hip.add(z(4, 6), z(4, 6))),
    ('add out', lambda: hip.add(z(4, 6), z(4, 6), out=z(4, 6))),
    ('bilinear', lambda: hip.upsample_bilinear2x_add(z(2, 3, 4, 5), z(2, 3, 4, 5))),
    ('bilinear no b', lambda: hip.upsample_bilinear2x_add(z(2, 3, 4, 5))),
    ('bilinear c8', lambda: hip.upsample_bilinear2x_add_c8(z(2, 5, 4, 6), z(2, 5, 4, 6))),
    ('bilinear c8c8', lambda: hip.upsample_bilinear2x_add_c8_from_c8(z(2, 2, 4, 6, 8, dtype=torch.bfloat16), z(2, 2, 4, 6, 8, dtype=torch.bfloat16))),
]


@pytest.mark.parametrize('case', ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_well_formed_call_passes_the_shape_checks(case):
    """the same calls with matching shapes get past the shape checks: what stops them on CPU tensors is ptr() (no CPU path) -- or, in a
    tree that was never built, the missing library -- so the refusals above are not refusals of everything"""
    with pytest.raises(hip.EssHipError) as e:
        case[1]()
    assert 'CPU tensor' in str(e.value) or 'not found' in str(e.value), str(e.value)
