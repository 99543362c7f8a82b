"""
MI355X counterparts of the E2VID building blocks (reference: e2vid/model/submodules.py).

Same class names, constructor signatures and state_dict key layout as the reference, so checkpoints
(`unetrecurrent.encoders.0.conv.conv2d.weight`, ...) load unchanged.  The nn.Conv2d / nn.BatchNorm2d
children are parameter containers only: every forward is a fused libess_hip.so launch
(conv + eval-norm + activation, or conv + LSTM/GRU gate maths).  The encoder is frozen and runs
under no_grad in ESS (training/ess_trainer.py:52-54,277-280), so these modules are inference-only:
asking autograd to differentiate through them raises.
"""
import collections
import os

import torch
import torch.nn as nn
from torch.nn import init

from ... import copies, hip
from ...functional import columns, derived, packed_rows, packed_weight

_ACT = {None: hip.ACT_NONE, 'relu': hip.ACT_RELU, 'sigmoid': hip.ACT_SIGMOID, 'tanh': hip.ACT_TANH}
EPS = 1e-5


def _inference_only(*tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError('the E2VID encoder kernels are forward-only (the encoder is frozen and runs under '
                                  'torch.no_grad() in ESS: training/ess_trainer.py:52-54,277-280)')


def _fp32_any(t):
    """fp32 values of `t`: the tensor itself, or -- when only its BF16_C8 copy was produced -- the copy converted back."""
    r = copies.of(t)
    return hip.from_bf16_c8(r.c8, t.shape[1]) if r.unwritten and r.c8 is not None else copies.require_fp32(t)


def _fold(spec, bias, norm_kind, norm_layer):
    """Per-output-channel (packed scale, packed shift) of an eval-mode norm folded behind a conv (None, None without either)."""
    src = [bias]
    if norm_kind in ('BN', 'IN'):
        src += [norm_layer.running_mean, norm_layer.running_var]
    if norm_kind == 'BN':
        src += [norm_layer.weight, norm_layer.bias]
    src = [t for t in src if t is not None]
    if not src:
        return None, None

    def build():
        with torch.no_grad():
            scale = shift = None
            if norm_kind == 'BN':  # y = (x - rm) / sqrt(rv + eps) * g + b
                scale = norm_layer.weight / torch.sqrt(norm_layer.running_var + EPS)
                shift = norm_layer.bias - norm_layer.running_mean * scale
            elif norm_kind == 'IN':  # InstanceNorm2d(track_running_stats=True).eval(): running stats, no affine
                scale = 1.0 / torch.sqrt(norm_layer.running_var + EPS)
                shift = -norm_layer.running_mean * scale
            if bias is not None:
                shift = bias * scale + shift if scale is not None else bias
            return (hip.pack_rows(spec, scale.contiguous(), fill=1.0) if scale is not None else None,
                    hip.pack_rows(spec, shift.contiguous()) if shift is not None else None)
    return derived(src, ('fold', spec.key), build)


def _norm_container(norm, ch):
    if norm == 'BN':
        return nn.BatchNorm2d(ch)
    if norm == 'IN':
        return nn.InstanceNorm2d(ch, track_running_stats=True)
    return None


def _check_eval(mod, norm):
    if mod.training and norm in ('BN', 'IN'):
        raise NotImplementedError('E2VID norm layers only exist in eval mode here (front_sensor_b.eval(), '
                                  'training/ess_trainer.py:54); call .eval() on the encoder')


_S2D_MODE = os.environ.get('ESS_CONV5_S2D', '1')[:1]  # (read once: 0 = never, 1 = where faster, 2 = wherever the form exists)


def set_s2d_mode(mode):
    """'0' | '1' | '2' (see _S2D_MODE) -> the previous value: pin one form of the encoder's 5x5 / stride-2 convolutions for a model whose
    outputs must not depend on the batch size in the last bit (tests; a deployment that validates at B = 1 what it trained at B = 8)"""
    global _S2D_MODE
    prev, _S2D_MODE = _S2D_MODE, str(mode)[:1]
    return prev


def _s2d_spec(N, k, stride, pad, cin, cout, H, W, act, compute=None):
    """The ESS_SRC_S2D spec of a 5x5 / stride-2 / pad-2 convolution where that form exists AND is the faster one for this launch
    (hip.s2d_preferred: it needs a launch that fills the chip), else None.  Switch ESS_CONV5_S2D: 0 = never, 2 = wherever it exists.
    The two forms add the same products in different orders: the choice depends on the batch size and on the device's compute-unit
    count, so the encoder's output for one sample may differ in the last bf16 bit between a B >= 4 training batch and a B < 4
    validation / streaming call (include/ess_hip.h, ess_conv2d_s2d_preferred); ESS_CONV5_S2D=0 / 2 pins one form."""
    mode = _S2D_MODE
    if (k, stride, pad) != (5, 2, 2) or cin % 32 or cout % 64 or H % 2 or W % 2 or mode == '0':
        return None
    s2 = hip.conv_spec(N, H // 2, W // 2, 4 * cin, 0, cout, 3, 1, 1, mode0=hip.SRC_S2D, act=act, compute=compute)
    return s2 if (mode == '2' or hip.s2d_preferred(s2)) else None


# ---- The 16-bit operand kind of an encoder step.  The recurrent part of the frozen encoder -- head, the stride-2 convolutions, the
# ConvLSTM / ConvGRU gates -- contracts either bf16 operands (configurations 'bf16', and 'fp32' / 'bf16x3', which are this kind with the
# copies switched off) or IEEE-half operands (configuration 'mixed', ESS_COMPUTE_F16).  Either way an activation travels between the
# launches as a channel-blocked 16-bit copy in its record (copies.py): field `c8`, or field `h16` = (tensor, hilo).  Only the half kind
# writes [hi | lo] pairs: the convolution in front of a recurrent block (its post-ReLU values carry means far above their spread:
# rounding THEM to 11 bits was the largest term of the encoder's error, tools/hybrid_rounding_ablation.py) and the last time step's
# h' -- the event latents.  A pair enters a convolution as 2 C channels against a weight whose input columns are repeated.
# Whoever STARTS a step chooses the kind (operand_kind) and hands it down; ConvLayer defaults to bf16 -- the tail that only feeds the
# reconstruction runs on the bf16 kernels in every configuration.
Kind = collections.namedtuple('Kind', 'compute field fmt pairs')  # (conv_spec's compute, the record field, the source format, pairs?)
BF16 = Kind(None, 'c8', hip.FMT_BF16_C8, False)
HALF = Kind(hip.COMPUTE_F16, 'h16', hip.FMT_F16_C8, True)


def operand_kind():
    return HALF if hip.mixed() else BF16


def _copies_on(k, *channels):
    """Does a launch of kind k read / write 16-bit copies?  half: always; bf16: in bf16 arithmetic, over whole 8-channel blocks."""
    return k is HALF or (hip.get_compute() == 'bf16' and not any(c % 8 for c in channels))


def _source(k, t, staged=True):
    """Source of kind k -> (tensor, hilo, format): the producer's copy; without one the half kind converts the fp32 values, the bf16
    kind (or `staged` off: copies switched off, a geometry that cannot stage BF16_C8) stages the fp32 tensor itself."""
    r = copies.of(t)
    if k is HALF:
        s, hilo = r.h16 or (hip.to_f16_c8(copies.require_fp32(t).contiguous()), False)
        return s, hilo, k.fmt
    if staged and r.c8 is not None:
        return r.c8, False, k.fmt
    return copies.require_fp32(t), False, hip.FMT_F32_NCHW


def _copy_empty(k, N, C, H, W, device, hilo=False):
    return hip.f16_blocks_empty(N, C, H, W, device, hilo=hilo) if k is HALF else hip.bf16_c8_empty(N, C, H, W, device)


def _attach_copy(k, t, copy, hilo=False):
    return copies.attach(t, **{k.field: (copy, hilo) if k is HALF else copy})


def _fp32_out(shape, device, skip):
    """The fp32 tensor of an output -- with `skip` one that exists as copies only (copies.require_fp32 refuses its values)."""
    return copies.placeholder(shape, device) if skip else torch.empty(shape, dtype=torch.float32, device=device)


def _gate_weight(w, C, hid, x_pair, h_pair, first):
    """The weight of a convolution over cat(x [C channels], h [hid channels]) for the operands as they arrive: the x columns alone on the
    first step of a sequence (h = 0 adds exact zeros: half the MFMA work, no zero state tensors), repeated for a [hi | lo] source."""
    cols = [(0, C)] * (2 if x_pair else 1) + ([] if first else [(C, C + hid)] * (2 if h_pair else 1))
    return w if cols == [(0, C), (C, C + hid)] else columns(w, cols)


def _launch(k, spec, src0, src1, packed_w, scale, shift, residual=None, copy=None, src_fmt=hip.FMT_F32_NCHW, **kw):
    """Launch of kind k (through the module attributes: bench.py times them in the step); copy: the output's 16-bit copy."""
    if k is HALF:
        return hip.conv_forward_h16(spec, src0, src1, packed_w, scale, shift, residual, out_h16=copy,
                                    src_fp32=src_fmt == hip.FMT_F32_NCHW, **kw)
    return hip.conv_forward(spec, src0, src1, packed_w, scale, shift, residual, out_bf=copy, src_fmt=src_fmt, **kw)


class ConvLayer(nn.Module):
    """conv2d (+BN/IN eval) (+activation) in one kernel.  Reference: submodules.py:7-31."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation='relu', norm=None):
        super().__init__()
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=(norm != 'BN'))
        self.activation = activation
        self.norm = norm
        nl = _norm_container(norm, out_channels)
        if nl is not None:
            self.norm_layer = nl

    def forward_of_sum(self, x, skip):
        """conv(x + skip) without the elementwise pass: W (x + skip) = [W W] [x; skip], i.e. the two tensors are the two
        concat sources of one convolution whose weight is W repeated along the input channels (sum-skip ahead of the
        prediction layer, reference unet.py:8-13,178-179).  Sums the same products in a different order."""
        w = self.conv2d.weight
        return self.forward(x, x1=skip, weight=columns(w, [(0, w.shape[1])] * 2))

    def forward(self, x, x1=None, residual=None, want_c8=False, c8_only=False, weight=None, hilo_out=False, kind=BF16):
        """x1: optional second source, channel-concatenated on the fly (bf16 kind).
        want_c8: also emit the output as a 16-bit staging copy of `kind` (bf16 kind: in bf16 arithmetic only), attached to the returned
        tensor (`copies.of(out).c8` / `.h16`), for a following 3x3 / 5x5 convolution to stage from (see ConvLSTM.forward).
        c8_only: (with want_c8) do not write the fp32 output at all -- for an activation whose only consumer stages from the copy;
        the returned tensor is a placeholder that refuses fp32 use (`copies.require_fp32`).
        hilo_out: (half kind, c8_only) the copy as a [hi | lo] pair.
        The half kind has two forms: the 5x5 head over the fp32 voxel grid (rounded to half inside the kernel), whose fp32 output
        exists unless c8_only, and an encoder convolution from its source's half copy, copy-only."""
        _inference_only(x, x1)
        _check_eval(self, self.norm)
        k, c = kind, self.conv2d
        wt = c.weight if weight is None else weight  # (forward_of_sum: the weight repeated for the two sources)
        ks, st, p, Cout, act = c.kernel_size[0], c.stride[0], c.padding[0], c.out_channels, _ACT[self.activation]
        N, C0, H, W = x.shape
        C1 = 0 if x1 is None else x1.shape[1]
        Ho, Wo = (H + 2 * p - ks) // st + 1, (W + 2 * p - ks) // st + 1
        on = _copies_on(k)
        stage = on and hip.c8_stageable(ks, st, p)
        r, src1 = copies.of(x), None
        if k is HALF and r.h16 is None and (ks, st) == (5, 1) and C0 <= 5 and not r.unwritten:
            src, hl, fmt = x.contiguous(), False, hip.FMT_F32_NCHW  # (the head: the image itself)
        elif x1 is None:
            src, hl, fmt = _source(k, x, stage)  # the producer's copy: bit-identical operands, cheaper loads
        else:
            # both concat sources from their producers' BF16_C8 copies (the prediction layer over decoder output + head: half the
            # bytes of the two fp32 tensors, and the decoder output need not exist in fp32 at all); bit-identical operands
            a8, b8 = (r.c8, copies.of(x1).c8) if stage and C0 % 8 == 0 else (None, None)
            if a8 is not None and b8 is not None:
                src, src1, hl, fmt = a8, b8, False, k.fmt
            else:
                src, src1, hl, fmt = copies.require_fp32(x), copies.require_fp32(x1), False, hip.FMT_F32_NCHW
        hilo = k.pairs and bool(hilo_out)
        copy = _copy_empty(k, N, Cout, Ho, Wo, x.device, hilo) if want_c8 and on else None
        skip = c8_only and copy is not None
        # copy-only outputs without a residual leave through the 16-bit-OUTPUT epilogue (16-byte stores, 32-bit offsets) instead of
        # the fp32 epilogue's optional copy (8-byte stores): the same values (acc * scale + shift, ReLU, round to nearest even)
        as_out = skip and residual is None and self.activation in (None, 'relu')
        if k is HALF and (x1 is not None or not (as_out or fmt == hip.FMT_F32_NCHW)):
            raise hip.EssHipError('ConvLayer(half operands): one source, and fp32 outputs exist for the head only')
        Ce = C0 * (2 if hl else 1)
        w = columns(wt, [(0, C0)] * 2) if hl else wt
        # 5x5 / stride 2 (the three downsampling convolutions of the frozen encoder, reference submodules.py:176-186) as a 3x3 over the
        # space-to-depth view of the 16-bit source, on the wide-tile 3x3 kernel (ESS_SRC_S2D: 16-channel chunks, the 25 real taps
        # only) instead of the tap-paired 5x5 kernel; the same products, summed in a different order
        spec = _s2d_spec(N, ks, st, p, Ce, Cout, H, W, act, k.compute) if as_out and x1 is None and fmt == k.fmt else None
        wkind = hip.W_CONV if spec is None else hip.W_CONV5_S2D
        if spec is None:
            spec = hip.conv_spec(N, H, W, Ce, C1, Cout, ks, st, p, act=act, compute=k.compute)
        scale, shift = _fold(spec, c.bias, self.norm, getattr(self, 'norm_layer', None))
        pw = packed_weight(spec, w, kind=wkind)
        out = _fp32_out((N, Cout, Ho, Wo), x.device, skip)
        if as_out:
            _launch(k, spec, src, src1, pw, scale, shift, out=copy, src_fmt=fmt, out_fmt=hip.FMT_F16_C8_HILO if hilo else k.fmt)
        else:
            _launch(k, spec, src, src1, pw, scale, shift, residual, out=None if skip else out, copy=copy, src_fmt=fmt)
        if copy is not None:
            _attach_copy(k, out, copy, hilo)
        return out


class TransposedConvLayer(nn.Module):
    """ConvTranspose2d(k, stride 2, output_padding 1) (+norm) (+activation): the zero-insertion is done
    while staging the LDS tile.  Reference: submodules.py:34-62."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation='relu', norm=None):
        super().__init__()
        self.transposed_conv2d = nn.ConvTranspose2d(in_channels, out_channels, kernel_size, stride=2, padding=padding,
                                                    output_padding=1, bias=(norm != 'BN'))
        self.activation = activation
        self.norm = norm
        nl = _norm_container(norm, out_channels)
        if nl is not None:
            self.norm_layer = nl

    def forward(self, x, x1=None):
        """x1: a second source -- the layer acts on the channel concat (x, x1) (skip_type 'concat'), read by the kernel's
        two-source loader, both zero-inserted while staged: the concatenated tensor never exists."""
        _inference_only(x)
        _check_eval(self, self.norm)
        t = self.transposed_conv2d
        N, C, H, W = x.shape
        C1 = 0 if x1 is None else x1.shape[1]
        if x1 is not None and (x1.shape[0], x1.shape[2], x1.shape[3]) != (N, H, W):
            raise hip.EssHipError('TransposedConvLayer: the two sources of a concat disagree on batch / extent')
        k, p = t.kernel_size[0], t.padding[0]
        if k != 2 * p + 1:
            raise hip.EssHipError('TransposedConvLayer: only k = 2p+1 geometries (output = 2x input) are supported')
        spec = hip.conv_spec(N, 2 * H, 2 * W, C, C1, t.out_channels, k, 1, k - 1 - p, hip.SRC_ZERO_UP2,
                             hip.SRC_ZERO_UP2 if x1 is not None else hip.SRC_DIRECT, act=_ACT[self.activation])
        scale, shift = _fold(spec, t.bias, self.norm, getattr(self, 'norm_layer', None))
        out = torch.empty(N, t.out_channels, spec.H_out, spec.W_out, dtype=torch.float32, device=x.device)
        return hip.conv_forward(spec, x, x1, packed_weight(spec, t.weight, kind=hip.W_TRANSPOSED), scale, shift, out=out)

    def forward_sum(self, x, skip):
        return self.forward(hip.add(x, skip))

    def forward_cat(self, x, skip):
        return self.forward(x.contiguous(), skip.contiguous())


class UpsampleConvLayer(nn.Module):
    """bilinear x2 (align_corners=False) -> conv (+norm) (+activation).  Reference: submodules.py:65-93."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, activation='relu', norm=None):
        super().__init__()
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=(norm != 'BN'))
        self.activation = activation
        self.norm = norm
        nl = _norm_container(norm, out_channels)
        if nl is not None:
            self.norm_layer = nl

    def _conv(self, up0, up1=None, c8_only=False):
        """c8_only (bf16 arithmetic, BF16_C8 staging): the output leaves as a BF16_C8 copy only -- for a decoder whose output is
        consumed by the next decoder's upsampling pass and nothing else (the returned fp32 tensor is a placeholder)."""
        c = self.conv2d
        c8 = hip.is_c8(up0)
        N, C0, H, W = up0.shape[0], (up0.shape[1] * 8 if c8 else up0.shape[1]), up0.shape[2], up0.shape[3]
        C1 = 0 if up1 is None else (up1.shape[1] * 8 if c8 else up1.shape[1])
        spec = hip.conv_spec(N, H, W, C0, C1, c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0],
                             act=_ACT[self.activation])
        scale, shift = _fold(spec, c.bias, self.norm, getattr(self, 'norm_layer', None))
        out = torch.empty(N, c.out_channels, spec.H_out, spec.W_out, dtype=torch.float32, device=up0.device)
        copy = hip.bf16_c8_empty(N, c.out_channels, spec.H_out, spec.W_out, up0.device) if (c8_only and c8) else None
        if copy is not None and self.activation in (None, 'relu'):  # (the BF16_C8-output epilogue: see ConvLayer.forward)
            hip.conv_forward(spec, up0, up1, packed_weight(spec, c.weight), scale, shift, out=copy, src_fmt=hip.FMT_BF16_C8,
                             out_fmt=hip.FMT_BF16_C8)
        else:
            hip.conv_forward(spec, up0, up1, packed_weight(spec, c.weight), scale, shift, out=None if copy is not None else out,
                             out_bf=copy, src_fmt=hip.FMT_BF16_C8 if c8 else hip.FMT_F32_NCHW)
        if copy is not None:
            copies.attach(out, c8=copy, unwritten=True)
        return out

    def _up(self, x, skip=None):
        """bilinear x2 of (x [+ skip]).  bf16 arithmetic: written as the BF16_C8 tensor the convolution stages (it would round
        the fp32 tensor to exactly these values anyway; half the bytes written, contiguous pixel vectors read back) -- and READ
        from the sources' BF16_C8 copies when their producers left them (resblock / previous decoder output, recurrent state)."""
        k = self.conv2d.kernel_size[0]
        if hip.get_compute() == 'bf16' and x.shape[1] % 8 == 0 and not (x.shape[3] & 1) and \
                hip.c8_stageable(k, self.conv2d.stride[0], self.conv2d.padding[0]):
            x8, s8 = copies.of(x).c8, (None if skip is None else copies.of(skip).c8)
            if x8 is not None and skip is not None and s8 is None:
                s8 = hip.to_bf16_c8(copies.require_fp32(skip))
            if x8 is not None:
                return hip.upsample_bilinear2x_add_c8_from_c8(x8, s8)
            return hip.upsample_bilinear2x_add_c8(_fp32_any(x), _fp32_any(skip))
        return hip.upsample_bilinear2x_add(_fp32_any(x), _fp32_any(skip))  # (odd widths, channel counts that are no multiple of 8)

    def forward(self, x, c8_only=False):
        _inference_only(x)
        _check_eval(self, self.norm)
        return self._conv(self._up(x), c8_only=c8_only)

    def forward_sum(self, x, skip, c8_only=False):
        """decoder(skip_sum(x, skip)) with the sum fused into the upsampling pass (unet.py:12-13,176)."""
        _inference_only(x, skip)
        _check_eval(self, self.norm)
        return self._conv(self._up(x, skip), c8_only=c8_only)

    def forward_cat(self, x, skip, c8_only=False):
        """decoder(skip_concat(x, skip)): bilinear commutes with the channel concat."""
        _inference_only(x, skip)
        _check_eval(self, self.norm)
        return self._conv(self._up(x), self._up(skip), c8_only=c8_only)


class ConvLSTM(nn.Module):
    """Gates conv over cat(x, h) + sigmoid/tanh + cell/hidden update in ONE kernel; the concat and the
    4*hidden gate tensor never exist in memory.  Reference: submodules.py:175-230."""

    def __init__(self, input_size, hidden_size, kernel_size):
        super().__init__()
        if kernel_size != 3:
            raise hip.EssHipError('ConvLSTM: the fused kernel is 3x3 (as used by RecurrentConvLayer)')
        self.input_size, self.hidden_size = input_size, hidden_size
        self.zero_tensors = {}
        self.Gates = nn.Conv2d(input_size + hidden_size, 4 * hidden_size, kernel_size, padding=kernel_size // 2)

    def forward(self, input_, prev_state=None, lean=False, hilo_out=False, kind=None):
        """lean: (16-bit copies on) do not write the fp32 hidden state -- only its 16-bit copy and the fp32 cell; for a time step
        whose state is consumed by the next step of this module and nothing else.
        hilo_out: (half kind, lean) the copy of h' as a [hi | lo] pair -- the latents of a sequence's last step."""
        _inference_only(input_)
        k = kind or operand_kind()
        N, C, H, W = input_.shape
        hid, dev = self.hidden_size, input_.device
        # first step of a sequence: h = 0 and c = 0 (a NULL cell pointer reads as zeros), so the h half of the contraction adds exact
        # zeros -- the gate conv runs over x alone with the x columns of the weight (_gate_weight; the reference caches zero state
        # tensors instead, submodules.py:196-207)
        first = prev_state is None
        prev_hidden, prev_cell = (None, None) if first else prev_state
        # x and h from their 16-bit copies when the producers left them (the encoder conv and the previous step of this kernel do),
        # and one of h' for the next time step.  bf16 kind: bit-identical to staging from the fp32 tensors -- the copies hold exactly
        # the bf16 operands the MFMA would be fed anyway -- but the tile loads are 16-byte vectors instead of 8 strided dwords.  A
        # state tensor that went through user code (clone, detach, arithmetic) simply has no copy any more: then BOTH sources are
        # staged from fp32 (half kind: the one without a copy is converted).
        on = _copies_on(k, C)
        xs, xhl, fmt = _source(k, input_, on)
        hs, hhl, hfmt = (None, False, fmt) if first else _source(k, prev_hidden, on)
        if hfmt != fmt:
            xs, hs, fmt = copies.require_fp32(input_), copies.require_fp32(prev_hidden), hip.FMT_F32_NCHW
        Cx, C1 = C * (2 if xhl else 1), 0 if first else hid * (2 if hhl else 1)
        w = _gate_weight(self.Gates.weight, C, hid, xhl, hhl, first)
        hilo = k.pairs and bool(hilo_out and lean)
        spec = hip.conv_spec(N, H, W, Cx, C1, 4 * hid, 3, 1, 1, epi=hip.EPI_LSTM, hidden=hid, act=hip.LSTM_H_HILO if hilo else 0,
                             compute=k.compute)
        if hilo and (hid % (8 * (spec.plan.cout_tile // 32)) or spec.plan.cout_tile < 64):  # (no pair copy of h' on such tiles)
            hilo = False
            spec = hip.conv_spec(N, H, W, Cx, C1, 4 * hid, 3, 1, 1, epi=hip.EPI_LSTM, hidden=hid, compute=k.compute)
        b = packed_rows(spec, self.Gates.bias)
        new = _copy_empty(k, N, hid, H, W, dev, hilo) if on else None
        # a lean step's cell state travels to the next time step only: channel-blocked fp32 (FMT_F32_C8 -- the epilogue reads and
        # writes a lane's 4 channels of a pixel as ONE 16-byte access instead of four 4-byte ones into four planes)
        cell, sfmt = _new_cell(N, hid, H, W, dev, lean and on)
        cfmt = hip.FMT_F32_C8 if prev_cell is not None and prev_cell.dim() == 5 else hip.FMT_F32_NCHW
        # (the half kernels drop the fp32 h' next to a channel-blocked cell only: with ESS_CELL_C8=0 the half kind writes it)
        skip = lean and on and (k is BF16 or sfmt == hip.FMT_F32_C8)
        hidden = _fp32_out((N, hid, H, W), dev, skip)
        _launch(k, spec, xs, hs, packed_weight(spec, w), None, b, aux0=prev_cell, out=None if skip else hidden, out2=cell, copy=new,
                src_fmt=fmt, out_fmt=sfmt, aux_fmt=cfmt)
        if new is not None:
            _attach_copy(k, hidden, new, hilo)
        return hidden, cell


def _new_cell(N, hid, H, W, device, blocked):
    """-> (cell tensor, its state format): FMT_F32_C8 for a lean step (switch ESS_CELL_C8=0: always fp32 NCHW planes)."""
    if blocked and os.environ.get('ESS_CELL_C8', '1')[:1] != '0':
        return hip.f32_c8_empty(N, hid, H, W, device), hip.FMT_F32_C8
    return torch.empty(N, hid, H, W, dtype=torch.float32, device=device), hip.FMT_F32_NCHW


class ConvGRU(nn.Module):
    """Two fused kernels: (update, reset) gates -> (u, r*h); candidate -> h'.  Reference: submodules.py:233-273.

    With 16-bit copies on, the recurrent state exists in three forms, as the ConvLSTM's does with (h, c): the 16-bit copy the gate /
    candidate convolutions stage (`copies.of(h).c8` / `.h16`), the fp32 values the epilogues blend with (`h' = h (1 - u) + o u` stays an
    fp32 recurrence: channel-blocked fp32 `f32c8` between lean time steps, plain NCHW planes otherwise), and -- unless the step is
    lean -- the fp32 NCHW tensor the reference returns.  u travels between the two kernels as a channel-blocked tensor, r*h as the
    16-bit tensor the candidate convolution would round it to anyway; neither the concat nor an fp32 r*h exist in memory."""

    def __init__(self, input_size, hidden_size, kernel_size):
        super().__init__()
        if kernel_size != 3:
            raise hip.EssHipError('ConvGRU: the fused kernels are 3x3 (as used by RecurrentConvLayer)')
        padding = kernel_size // 2
        self.input_size, self.hidden_size = input_size, hidden_size
        self.reset_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=padding)
        self.update_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=padding)
        self.out_gate = nn.Conv2d(input_size + hidden_size, hidden_size, kernel_size, padding=padding)
        for g in (self.reset_gate, self.update_gate, self.out_gate):
            init.orthogonal_(g.weight)
            init.constant_(g.bias, 0.)

    def forward(self, input_, prev_state, lean=False, hilo_out=False, kind=None):
        """lean: (16-bit copies on) do not write the fp32 NCHW state -- only its 16-bit copy and the channel-blocked fp32 form; for a
        time step whose state is consumed by the next step of this module and nothing else.
        hilo_out: (half kind, lean) the copy of h' as a [hi | lo] pair."""
        _inference_only(input_)
        k = kind or operand_kind()
        N, C, H, W = input_.shape
        hid, dev = self.hidden_size, input_.device
        # first step of a sequence: h = 0, so r*h = 0 whatever r is and the h halves of all three contractions add exact zeros --
        # both kernels run over x alone with the x columns of the weights (half the MFMA work, no zero tensors; the reset rows of
        # the first kernel are computed and dropped)
        first = prev_state is None
        on = _copies_on(k, C, hid)
        xs, xhl, fmt = _source(k, input_, on)
        hs, hhl, hfmt = (None, False, fmt) if first else _source(k, prev_state, on)
        if hhl:
            raise hip.EssHipError('ConvGRU: a [hi | lo] hidden state feeds the decoder, not the next time step')
        Cx, C1 = C * (2 if xhl else 1), 0 if first else hid
        # the update gate travels between the two launches rounded to IEEE half (ESS_GRU_U_F16: an F16_C8 tensor where the states are
        # channel-blocked, the rounded value in the fp32 tensor otherwise -- the same bits either way); bf16 kind: in bf16 arithmetic,
        # switch ESS_GRU_U16=0 (the half kind does not read the switch)
        u16 = k is HALF or (hip.get_compute() == 'bf16' and os.environ.get('ESS_GRU_U16', '1')[:1] != '0')
        uact = hip.GRU_U_F16 if u16 else hip.GRU_U_F32
        s1 = hip.conv_spec(N, H, W, Cx, C1, 2 * hid, 3, 1, 1, epi=hip.EPI_GRU_UR, act=uact, hidden=hid, compute=k.compute)
        if u16 and hid % (s1.plan.cout_tile // 2):
            # (an F16_C8 u exists in the straight-line epilogues only: every hidden channel of a workgroup's tile real -- the library
            # refuses the combination otherwise; E2VID's 64 / 128 / 256 hidden channels qualify)
            uact = hip.GRU_U_F32
            s1 = hip.conv_spec(N, H, W, Cx, C1, 2 * hid, 3, 1, 1, epi=hip.EPI_GRU_UR, act=uact, hidden=hid, compute=k.compute)
        hb = None if first else copies.of(prev_state).f32c8  # channel-blocked fp32 h (left by a lean step)
        blocked = first or hb is not None
        hilo = k.pairs and bool(hilo_out and lean and blocked)
        s2 = hip.conv_spec(N, H, W, Cx, C1, hid, 3, 1, 1, epi=hip.EPI_GRU_OUT, act=uact | (hip.GRU_H_HILO if hilo else 0), hidden=hid,
                           compute=k.compute)
        if hilo and hid % s2.plan.cout_tile:
            hilo = False
            s2 = hip.conv_spec(N, H, W, Cx, C1, hid, 3, 1, 1, epi=hip.EPI_GRU_OUT, act=uact, hidden=hid, compute=k.compute)
        b1, b2 = packed_rows(s1, self.update_gate.bias, self.reset_gate.bias), packed_rows(s2, self.out_gate.bias)
        wu, wr, wo = (_gate_weight(g.weight, C, hid, xhl, False, first) for g in (self.update_gate, self.reset_gate, self.out_gate))
        pw1, pw2 = packed_weight(s1, wu, wr), packed_weight(s2, wo)
        shape = (N, hid, H, W)
        if fmt == hip.FMT_F32_NCHW or hfmt != fmt:
            # ---- fp32 NCHW sources (bf16 kind: exact-fp32 arithmetic; or a state that went through user code and lost its copies)
            x = copies.require_fp32(input_)
            h = None if first else copies.require_fp32(prev_state)
            u = torch.empty(shape, dtype=torch.float32, device=dev)
            rh = None if first else torch.empty_like(u)
            _launch(k, s1, x, h, pw1, None, b1, aux0=h, out=u, out2=rh)
            new_state = torch.empty_like(u)
            new = _copy_empty(k, N, hid, H, W, dev) if on else None
            _launch(k, s2, x, rh, pw2, None, b2, aux0=h, aux1=u, out=new_state, copy=new)
            return new_state if new is None else _attach_copy(k, new_state, new)
        # ---- 16-bit sources: x / h / r*h staged as 16-byte pixel vectors, fp32 state operands channel-blocked where they can be
        afmt = hip.FMT_F32_C8 if blocked else hip.FMT_F32_NCHW
        h32 = hb if blocked else copies.require_fp32(prev_state)
        if blocked:
            u = hip.f16_c8_raw_empty(N, hid, H, W, dev) if uact == hip.GRU_U_F16 else hip.f32_c8_empty(N, hid, H, W, dev)
        else:
            u = torch.empty(shape, dtype=torch.float32, device=dev)
        rh = None if first else _copy_empty(k, N, hid, H, W, dev)
        _launch(k, s1, xs, hs, pw1, None, b1, aux0=h32, out=u, out2=None, copy=rh, src_fmt=fmt, out_fmt=afmt, aux_fmt=afmt)
        new = _copy_empty(k, N, hid, H, W, dev, hilo)
        # (the half kind's lean form reads channel-blocked states only; the bf16 kind's also starts from fp32 NCHW planes)
        skip = lean and (k is BF16 or blocked)
        new_state = _fp32_out(shape, dev, skip)
        if skip:
            nb = hip.f32_c8_empty(N, hid, H, W, dev)
            _launch(k, s2, xs, rh, pw2, None, b2, aux0=h32, aux1=u, out=nb, copy=new, src_fmt=fmt, out_fmt=hip.FMT_F32_C8, aux_fmt=afmt)
            copies.attach(new_state, f32c8=nb)
        else:
            _launch(k, s2, xs, rh, pw2, None, b2, aux0=h32, aux1=u, out=new_state, copy=new, src_fmt=fmt, out_fmt=hip.FMT_F32_NCHW,
                    aux_fmt=afmt)
        return _attach_copy(k, new_state, new, hilo)


class RecurrentConvLayer(nn.Module):
    """ConvLayer (k5, s2) followed by a ConvLSTM / ConvGRU.  Reference: submodules.py:96-115."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=0, recurrent_block_type='convlstm',
                 activation='relu', norm=None):
        super().__init__()
        assert recurrent_block_type in ['convlstm', 'convgru']
        self.recurrent_block_type = recurrent_block_type
        block = ConvLSTM if recurrent_block_type == 'convlstm' else ConvGRU
        self.conv = ConvLayer(in_channels, out_channels, kernel_size, stride, padding, activation, norm)
        self.recurrent_block = block(input_size=out_channels, hidden_size=out_channels, kernel_size=3)

    def _prev_has_c8(self, prev_state):
        """True when the recurrent block will take the BF16_C8 path for this step (zero state, or a state that still carries its copy)."""
        if prev_state is None:
            return True
        return copies.of(prev_state[0] if self.recurrent_block_type == 'convlstm' else prev_state).c8 is not None

    def forward(self, x, prev_state, lean=False, x_conv=None, hilo_out=False, x_hilo=False, kind=None):
        """x_conv: the conv output computed ahead of time (time-batched prefix, UNetRecurrent.forward_prefix): a placeholder
        carrying its BF16_C8 copy; `x` is then ignored.
        x_hilo / hilo_out (half kind): the conv output / the copy of a lean step's h' as a [hi | lo] pair."""
        k = kind or operand_kind()
        # the conv output never leaves this module: the recurrent block stages it from the 16-bit copy (a 64 | 128 | 256-channel
        # tensor, always a whole number of 8-channel blocks), so its fp32 form is not written (bf16 kind: unless the block will stage
        # fp32 tensors this step; the half kind converts a state that lost its copy instead)
        if x_conv is None:
            x_conv = self.conv(x, want_c8=True, hilo_out=x_hilo, kind=k, c8_only=k is HALF or (
                self.conv.conv2d.out_channels % 8 == 0 and hip.c8_stageable(3, 1, 1) and self._prev_has_c8(prev_state)))
        state = self.recurrent_block(x_conv, prev_state, lean=lean, hilo_out=hilo_out, kind=k)
        return (state[0] if self.recurrent_block_type == 'convlstm' else state), state


class ResidualBlock(nn.Module):
    """conv3x3 -norm-ReLU- conv3x3 -norm- (+x) -ReLU as two fused kernels (BN/no norm), or with the
    InstanceNorm plane kernel in between (norm='IN').  Reference: submodules.py:140-172."""

    def __init__(self, in_channels, out_channels, stride=1, downsample=None, norm=None):
        super().__init__()
        if downsample is not None or stride != 1:
            raise hip.EssHipError('ResidualBlock: E2VID only builds stride-1 blocks without downsample')
        bias = norm != 'BN'
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=bias)
        self.norm = norm
        if norm == 'BN':
            self.bn1 = nn.BatchNorm2d(out_channels)
            self.bn2 = nn.BatchNorm2d(out_channels)
        elif norm == 'IN':
            self.bn1 = nn.InstanceNorm2d(out_channels)
            self.bn2 = nn.InstanceNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=bias)
        self.downsample = downsample

    def forward(self, x, c8_only=False):
        """c8_only (bf16 arithmetic, fused norms, x carries a BF16_C8 copy): both convolutions read and write BF16_C8 tensors --
        the block's output exists as a copy only (for a consumer that stages from it: the next block, a decoder's upsampling
        pass); bf16-rounded where the fp32 form kept the accumulator."""
        _inference_only(x)
        N, C, H, W = x.shape
        bn = self.norm == 'BN'
        if bn and self.training:
            raise NotImplementedError('E2VID BatchNorm only exists in eval mode here; call .eval() on the encoder')
        fused = self.norm != 'IN'
        x8 = copies.of(x).c8 if (c8_only and fused and hip.get_compute() == 'bf16' and C % 8 == 0 and hip.c8_stageable(3, 1, 1)) else None
        if x8 is not None:
            s1 = hip.conv_spec(N, H, W, C, 0, self.conv1.out_channels, 3, 1, 1, act=hip.ACT_RELU)
            s2 = hip.conv_spec(N, H, W, self.conv1.out_channels, 0, self.conv2.out_channels, 3, 1, 1, act=hip.ACT_RELU)
            sc1, sh1 = _fold(s1, self.conv1.bias, 'BN' if bn else None, getattr(self, 'bn1', None))
            sc2, sh2 = _fold(s2, self.conv2.bias, 'BN' if bn else None, getattr(self, 'bn2', None))
            o8 = hip.bf16_c8_empty(N, self.conv1.out_channels, H, W, x.device)
            hip.conv_forward(s1, x8, None, packed_weight(s1, self.conv1.weight), sc1, sh1, out=o8, src_fmt=hip.FMT_BF16_C8,
                             out_fmt=hip.FMT_BF16_C8)
            out8 = hip.bf16_c8_empty(N, self.conv2.out_channels, H, W, x.device)
            hip.conv_forward(s2, o8, None, packed_weight(s2, self.conv2.weight), sc2, sh2, x8, out=out8, src_fmt=hip.FMT_BF16_C8,
                             out_fmt=hip.FMT_BF16_C8)
            out = torch.empty(N, self.conv2.out_channels, H, W, dtype=torch.float32, device=x.device)
            copies.attach(out, c8=out8, unwritten=True)
            return out
        s1 = hip.conv_spec(N, H, W, C, 0, self.conv1.out_channels, 3, 1, 1, act=hip.ACT_RELU if fused else hip.ACT_NONE)
        s2 = hip.conv_spec(N, H, W, self.conv1.out_channels, 0, self.conv2.out_channels, 3, 1, 1,
                           act=hip.ACT_RELU if fused else hip.ACT_NONE)
        sc1, sh1 = _fold(s1, self.conv1.bias, 'BN' if bn else None, getattr(self, 'bn1', None))
        sc2, sh2 = _fold(s2, self.conv2.bias, 'BN' if bn else None, getattr(self, 'bn2', None))
        o = torch.empty(N, self.conv1.out_channels, H, W, dtype=torch.float32, device=x.device)
        x = copies.require_fp32(x)  # (an unwritten lean-state placeholder must not be read as fp32)
        hip.conv_forward(s1, x, None, packed_weight(s1, self.conv1.weight), sc1, sh1, out=o)
        if not fused:
            o, _ = hip.instnorm_forward(o, None, 1, EPS)
        out = torch.empty(N, self.conv2.out_channels, H, W, dtype=torch.float32, device=x.device)
        hip.conv_forward(s2, o, None, packed_weight(s2, self.conv2.weight), sc2, sh2, x if fused else None, out=out)
        if not fused:
            out, _ = hip.instnorm_forward(out, x, 2, EPS)
        return out

