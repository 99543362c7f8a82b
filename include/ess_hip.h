/*
 * ess_hip.h -- C ABI of libess_hip.so: the MI355X (gfx950) kernels under the ESS hot path.
 *
 * The reference (uzh-rpg/ess) has no FFI: its hot path is PyTorch modules calling cuDNN through
 * torch ops.  Each entry point below names the torch op sequence of the reference it replaces
 * (file:line under the reference root) so that a maintainer can bind it from the reference's own
 * nn.Module.forward (see INTEGRATION.md for the ctypes stub).
 *
 * Conventions:
 *   - all pointers are DEVICE pointers into caller-owned storage (PyTorch caching allocator);
 *     nothing is allocated, freed or retained by the library; workspaces are caller-provided;
 *   - tensors are dense NCHW fp32 unless stated; labels are int64;
 *   - `stream` is the caller's hipStream_t (torch.cuda.current_stream().cuda_stream); the library
 *     never synchronises, never calls hipSetDevice and keeps no mutable global state that can change a result (re-entrant).
 *     What it does keep: read-once constants (environment tuning variables, the device's compute-unit count, per-kernel LDS
 *     opt-ins) and the documented process-wide switches of ess_tuning_set, which select between kernels of equal arithmetic
 *     ("conv_wide": bit-identical results; "in_small_threads": equal up to the summation order of the norm statistics);
 *   - return value: 0 on success, negative ESS_E* otherwise; ess_last_error() gives a thread-local
 *     message.  Nothing throws across the ABI.
 */
#ifndef ESS_HIP_H
#define ESS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ess_stream_t; /* hipStream_t */

enum { ESS_OK = 0, ESS_EINVAL = -22, ESS_ENOTSUP = -95, ESS_ELAUNCH = -5 };

/* how a conv source is read (fused into the LDS tile load) */
enum { ESS_SRC_DIRECT = 0, ESS_SRC_NEAREST_UP2 = 1, ESS_SRC_ZERO_UP2 = 2,
       ESS_SRC_S2D = 3 /* space-to-depth view of a BF16_C8 tensor stored at (2 H_in, 2 W_in) with C0 / 4 channels: the virtual channels
                        * of parity class q = (row parity) + 2 (column parity) at virtual pixel (y, x) are the stored channels at
                        * (2y + (q & 1), 2x + (q >> 1)); their ORDER (which virtual channel index is which class / stored channel) is
                        * internal to the ESS_W_CONV5_S2D weight pack and the kernel that reads it.  With weights
                        * packed as ESS_W_CONV5_S2D a 3x3 / stride 1 / pad 1 descriptor over this view IS the 5x5 / stride 2 / pad 2
                        * convolution of the stored tensor (nn.Conv2d(k=5, s=2, p=2) of the frozen encoder,
                        * e2vid/model/submodules.py:176-186, e2vid/model/unet.py:40-47): mode0 only, C1 = 0, fmt0 = fmt_out =
                        * ESS_FMT_BF16_C8, LINEAR epilogue, bf16 compute, C0 % 128 == 0, C_out % 64 == 0.                       */ };
/* conv epilogues (fused into the accumulator write-out) */
enum {
  ESS_EPI_LINEAR = 0,  /* y = act(acc*scale + shift (+ residual))                                   */
  ESS_EPI_LSTM = 1,    /* ConvLSTM gates -> (h', c')            e2vid/model/submodules.py:212-230     */
  ESS_EPI_GRU_UR = 2,  /* ConvGRU update/reset -> (u, r*h)      e2vid/model/submodules.py:268-270     */
  ESS_EPI_GRU_OUT = 3  /* ConvGRU candidate -> h'               e2vid/model/submodules.py:270-271     */
};
/* output transform of the LINEAR epilogue.  SUMPOOL2: no activation, and the first output (channels < out_split, or all
 * of them) is written as the 2x2 sum of its pixels, [N][C][H_out/2][W_out/2] -- the data-gradient of a nearest-x2-upsampled
 * source (mode ESS_SRC_NEAREST_UP2 of the forward convolution) without the full-resolution tensor in between.        */
enum { ESS_ACT_NONE = 0, ESS_ACT_RELU = 1, ESS_ACT_SIGMOID = 2, ESS_ACT_TANH = 3, ESS_ACT_SUMPOOL2 = 4 };
/* arithmetic of the convolution contraction.  Tensors in HBM are fp32 either way; BF16 rounds the MFMA operands
 * (activations while staging the LDS tile, weights at pack time) to bfloat16 and accumulates in fp32.         */
enum { ESS_COMPUTE_FP32 = 0, ESS_COMPUTE_BF16 = 1,
       /* split-operand bf16 ("bf16x3"): fp32 tensors; every operand x of a 3x3 / stride-1 contraction (forward, data-gradient,
        * recurrent gates, weight gradient) enters the matrix cores as hi = bf16(x), lo = bf16(x - hi), and a product is
        * w_hi x_hi + w_hi x_lo + w_lo x_hi in fp32 accumulators: ~2^-16 relative operand error against bf16's 2^-8, at three bf16
        * MFMAs per product (the exact fp32 MFMA costs sixteen).  Every other convolution of such a descriptor runs the exact-fp32
        * kernels.  The parity-grade configuration with a matrix-core-rate step.                                          */
       ESS_COMPUTE_BF16X3 = 2,
       /* IEEE-half operands (round 6; the forward arithmetic of the "mixed" configuration): the matrix cores run
        * v_mfma_f32_32x32x16_f16 at the bf16 rate with 11 instead of 8 significant operand bits; fp32 accumulators.  Every 16-bit
        * tensor of such a call is an ESS_FMT_F16_C8 tensor (sources, residual, LINEAR output, the recurrent epilogues' copies), the
        * weights are rounded to half at pack time, conversions saturate at +-65504 (NaN kept).  Forward forms only (no SUMPOOL2, no
        * zero-inserted source, no weight gradient): gradients stay bfloat16 -- their magnitudes (1e-7 for a mean loss over 2.5 M
        * pixels) are below half's normal range.  fp32 NCHW sources only for the 2-channel 5x5 head.                         */
       ESS_COMPUTE_F16 = 3 };
/* storage format of a convolution source.  BF16_C8 = the "staging copy" a producing kernel can emit next to its
 * fp32 NCHW output (out_bf16 of ess_conv2d_forward, or ess_to_bf16_c8): bfloat16 [N][ceil(C/8)][H][W][8], i.e. the
 * 8 channels of a pixel are one 16-byte vector = one MFMA K-fragment; channels past C are zero.  A consumer conv
 * stages it with plain 16-byte copies: 4x fewer cache-line touches and half the bytes of the fp32 NCHW path.      */
/* ESS_FMT_F16_C8: the BF16_C8 layout with IEEE half elements.  ONLY as a convolution OUTPUT (fmt_out, LINEAR epilogue) that a norm
 * kernel reads (x of ess_instnorm_* / ess_batchnorm_train_*_c8 with x_f16 = 1): pre-normalisation tensors keep 11 significant bits. */
/* ESS_COMPUTE_F16 convolutions read and write F16_C8 tensors throughout.  ESS_FMT_F16_C8_HILO (fmt_out of such a LINEAR convolution; act in
 * {none, relu}, no residual, no out_split, C_out % 64 == 0): the output is [N][2 ceil(C/8)][H][W][8] halfs -- blocks [0, CB) hold
 * hi = half(v), blocks [CB, 2 CB) lo = half(v - hi), ~22 significant bits in the pair; both parts saturate at +-65504 (the pair holds
 * clamp(v, +-131008), never an inf; NaN is kept in hi).  A consumer reads it as a plain F16_C8 source of 2 C
 * channels against a weight whose input columns are repeated ([w | w]): w (hi + lo) on the half matrix cores.  Used where an
 * activation's mean is large against its spread: the encoder convolution in front of a recurrent block, the event latents.   */
enum { ESS_FMT_F32_NCHW = 0, ESS_FMT_BF16_C8 = 1, ESS_FMT_F16_C8 = 3, ESS_FMT_F16_C8_HILO = 4,
       ESS_FMT_F32_C8 = 2 /* fp32 [N][ceil(C/8)][H][W][8]: ConvLSTM cell / ConvGRU hidden states between time steps (recurrent epilogues only) */ };
/* ConvGRU: the update gate u between the (update, reset) kernel and the candidate kernel (EssConvDesc.act of the two GRU epilogues).
 * ESS_GRU_U_F16: u is rounded to IEEE half (11 significant bits of a value in (0, 1); the gates come from bf16 operands) -- with
 * fmt_out / fmt_res = ESS_FMT_F32_C8 the tensor itself is an F16_C8 tensor ([N][hid/8][H][W][8] halfs: half the bytes of the launch
 * pair's most bandwidth-bound operand), with fp32 NCHW states the fp32 tensor carries the rounded value, so that a sequence gives the
 * same bits whichever storage its steps use.  bf16 compute only.  Reference: e2vid/model/submodules.py:255-273 (`update`).          */
enum { ESS_GRU_U_F32 = 0, ESS_GRU_U_F16 = 1 };
/* ConvLSTM with ESS_COMPUTE_F16 (EssConvDesc.act of the LSTM epilogue; 0 otherwise): the half copy of h' (out_bf16) leaves as a
 * [hi | lo] pair, [N][2 hid/8][H][W][8] (see ESS_FMT_F16_C8_HILO) -- the event latents the semantic decoder reads.  Lean form only
 * (channel-blocked cell states, hidden % 16 == 0).                                                                       */
enum { ESS_LSTM_H_HILO = 1 };
/* ... and the ConvGRU candidate launch (ESS_EPI_GRU_OUT, ESS_COMPUTE_F16): OR'ed into act next to ESS_GRU_U_*; straight-line form only
 * (channel-blocked states, hidden % 64 == 0).                                                                                     */
enum { ESS_GRU_H_HILO = 2 };
/* weight sources for ess_conv2d_pack_weights */
enum {
  ESS_W_CONV = 0,        /* nn.Conv2d weight [C_out][C_in][k][k]                                     */
  ESS_W_TRANSPOSED = 1,  /* weight [C_in][C_out][k][k] used spatially flipped: nn.ConvTranspose2d
                            forward, or the data-gradient of a Conv2d (pass its weight)              */
  ESS_W_ROWS = 2,        /* ess_conv2d_pack_weights_multi only: the job's `w` is a per-output-channel vector (a bias,
                            C_out floats) and `packed` the float buffer of ess_conv2d_pack_rows (fill 0) -- the
                            biases of the trainable convolutions ride in the weights' re-pack launch       */
  ESS_W_CONV5_S2D = 3    /* ess_conv2d_pack_weights with an ESS_SRC_S2D descriptor (and only then): w is the 5x5 / stride-2
                            convolution's weight [C_out][C0 / 4][5][5]; packed as the 3x3 taps of the four parity classes
                            (tap (ty, tx) of class (py, px) = w[..][2 ty + py][2 tx + px], absent where that index is 5)  */
};

/* One 2-D convolution over the channel-concatenation of up to two sources.
 * Replaces nn.Conv2d / torch.cat / F.interpolate(nearest) / BatchNorm2d(eval) / activation chains:
 *   ConvLayer.forward            e2vid/model/submodules.py:24-31
 *   ResidualBlock.forward        e2vid/model/submodules.py:157-172
 *   ConvLSTM.forward             e2vid/model/submodules.py:190-230
 *   ConvGRU.forward              e2vid/model/submodules.py:255-273
 *   ReLUINSConv2d / INSResBlock convs, cat+nearest-up of SemSegE2VID.forward
 *                                models/style_networks.py:69-88,158-193                             */
typedef struct EssConvDesc {
  int32_t N;
  int32_t H_in, W_in;   /* extent the filter slides over (i.e. AFTER per-source x2 upsampling)       */
  int32_t C0, C1;       /* channels of source 0 / source 1 (C1 = 0: single source)                   */
  int32_t mode0, mode1; /* ESS_SRC_*: a *_UP2 source is stored at (H_in/2, W_in/2)                   */
  int32_t C_out, H_out, W_out;
  int32_t ksize, stride, pad;
  int32_t epilogue;     /* ESS_EPI_*                                                                 */
  int32_t act;          /* ESS_ACT_* (LINEAR epilogue); GRU epilogues: ESS_GRU_U_* -- how the update gate u travels
                           from the GRU_UR launch to the GRU_OUT launch (both launches carry the same value)  */
  int32_t hidden;       /* recurrent epilogues: hidden channels (C_out = 4*hidden LSTM, 2*hidden
                           GRU_UR, hidden GRU_OUT)                                                   */
  int32_t out_split;    /* LINEAR: >0 writes channels [0,out_split) to `out` and the rest to `out2`
                           (data-gradient of a two-source conv)                                      */
  int32_t compute;      /* ESS_COMPUTE_*                                                             */
  int32_t fmt0, fmt1;   /* ESS_FMT_* of source 0 / 1.  BF16_C8 needs bf16 compute, a 1x1 / 3x3 (any source mode) or a
                           5x5 (DIRECT sources) filter, and the same format for both sources of a concat        */
  int32_t fmt_out;      /* ESS_FMT_BF16_C8 (LINEAR epilogue, bf16 compute): `out` -- and `out2` of an out_split --
                           ARE BF16_C8 tensors and no fp32 tensor is written: the stored form of the trainable
                           networks' activations and activation gradients in the bf16 configuration.  With
                           ESS_ACT_SUMPOOL2 the first output is the pooled BF16_C8 tensor.  out_split % 8 == 0.       */
  int32_t fmt_res;      /* format of `residual` (BF16_C8 only together with a BF16_C8 output).
                           LSTM epilogue: fmt_res = format of aux0 (the cell state c), fmt_out = format of out / out2
                           (h', c'): ESS_FMT_F32_NCHW or ESS_FMT_F32_C8 (a lane's 4 channels of a pixel are one 16-byte
                           access; for states that only travel to the next time step).
                           GRU epilogues: fmt_res = format of aux0 (h_prev) and aux1 (u), fmt_out = format of the fp32
                           outputs (GRU_UR: u, r*h; GRU_OUT: h'), each ESS_FMT_F32_NCHW or ESS_FMT_F32_C8               */
} EssConvDesc;

typedef struct EssConvPlan {
  int32_t cout_tile;    /* output channels per workgroup (32 or 64)                                  */
  int32_t ck;           /* input channels per LDS chunk                                              */
  int32_t n_chunks, n_cout_tiles;
  int64_t packed_elems; /* elements in the packed weight buffer (fp32 or bf16 by `compute`)          */
  int64_t packed_bytes; /* size of that buffer                                                       */
  int32_t rows_padded;  /* n_cout_tiles * cout_tile = length of packed scale/shift vectors           */
  int32_t lds_bytes;
} EssConvPlan;

const char* ess_last_error(void);
int ess_version(void);

int ess_conv2d_plan(const EssConvDesc* d, EssConvPlan* plan);

/* 1 when `d` is a valid ESS_SRC_S2D descriptor AND the space-to-depth form is the faster way to run that 5x5 / stride-2 convolution
 * on this device (its one-workgroup-per-CU tiles need a launch of at least 3/4 of the compute units' worth of tiles: B >= 4 at the
 * DSEC shape; below that the tap-paired 5x5 kernel wins), else 0.  The caller picks the descriptor (and the weight pack) by it:
 * ConvLayer.forward of the frozen encoder, e2vid/model/submodules.py:7-31,176-186.  NOTE: the two forms add the same products in
 * different orders, so a caller that follows this answer gets results that depend on N and on the device's compute-unit count in
 * the last bf16 / half bit (training batch vs a B < 4 validation or streaming call); pin one form per model where that matters.  */
int ess_conv2d_s2d_preferred(const EssConvDesc* d);

/* Re-layout a weight tensor for ess_conv2d_forward (tile-major, epilogue row permutation applied).
 * w_kind ESS_W_CONV: w is [C_out][C0+C1][k][k]; ESS_W_TRANSPOSED: w is [C0+C1][C_out][k][k].
 * For ESS_EPI_GRU_UR pass w = update_gate.weight and w2 = reset_gate.weight.                        */
int ess_conv2d_pack_weights(const EssConvDesc* d, int w_kind, const float* w, const float* w2,
                            void* packed, ess_stream_t stream);
/* ess_conv2d_pack_weights for `count` tensors in one launch (the re-pack of every trainable convolution after an optimiser
 * step).  bf16 compute, LINEAR epilogue, 1x1 / 3x3 / 7x7 layouts (and ESS_W_ROWS jobs) only; anything else is refused and nothing is launched.
 * descs / w_kinds / w / packed: host arrays of `count` entries.                                                      */
int ess_conv2d_pack_weights_multi(const EssConvDesc* descs, const int32_t* w_kinds, const float* const* w,
                                  void* const* packed, int32_t count, ess_stream_t stream);

/* Same permutation/padding for a per-output-channel vector (bias, folded BN scale/shift).
 * v2: second vector for GRU_UR (reset gate); fill: value for padded rows.                           */
int ess_conv2d_pack_rows(const EssConvDesc* d, const float* v, const float* v2, float fill,
                         float* packed, ess_stream_t stream);

/* src1 may be NULL when C1 == 0.  scale/shift: packed (ess_conv2d_pack_rows) or NULL.
 * residual: [N][C_out][H_out][W_out] or NULL (LINEAR).
 * aux0: LSTM c_prev | GRU_UR h_prev | GRU_OUT h_prev (NULL = zeros: first time step) ; aux1: GRU_OUT u.
 * out : LINEAR y | LSTM h' | GRU_UR u | GRU_OUT h' ;   out2: LSTM c' | GRU_UR r*h (fp32) | LINEAR split.
 * Recurrent epilogues take the bias as `shift`, no scale, no residual.                              */
int ess_conv2d_forward(const EssConvDesc* d, const void* src0, const void* src1, const void* packed_w,
                       const float* scale, const float* shift, const void* residual, const float* aux0,
                       const float* aux1, void* out, void* out2, void* out_bf16, ess_stream_t stream);
/* out / out2 / residual: fp32 NCHW, or BF16_C8 tensors when d->fmt_out (d->fmt_res) says so.                    */
/* src0/src1: fp32 NCHW or bf16 C8 per d->fmt0/fmt1.  out_bf16 (nullable): additionally receives `out` (LINEAR y,
 * LSTM h', GRU_OUT h') as a BF16_C8 tensor [N][ceil(C/8)][H_out][W_out][8] for the next convolution to stage from
 * (bf16 compute only; not with out_split).  With out_bf16 given, `out` may be NULL for the LINEAR, LSTM and GRU_OUT
 * epilogues: the fp32 tensor is then not written at all (a producer whose only consumer stages from the copy).
 * GRU_UR: out_bf16 receives r*h as a BF16_C8 tensor -- the second source of the candidate convolution (reference
 * e2vid/model/submodules.py:268-270) -- and out2 may then be NULL; with aux0 == NULL both may be NULL (r*h = 0).    */

/* fp32 NCHW -> BF16_C8 (round to nearest even; tail channels zero).  y: N*ceil(C/8)*H*W*8 bfloat16.        */
int ess_to_bf16_c8(const float* x, void* y, int32_t N, int32_t C, int32_t H, int32_t W, ess_stream_t stream);
/* BF16_C8 -> fp32 NCHW (exact).                                                                                  */
int ess_from_bf16_c8(const void* x, float* y, int32_t N, int32_t C, int32_t H, int32_t W, ess_stream_t stream);
/* Format bridges of the "mixed" configuration (ESS_COMPUTE_F16 convolutions read F16_C8 tensors):
 *   ess_to_f16_c8          fp32 NCHW -> F16_C8 [N][ceil(C/8)][H][W][8] halfs, or (hilo != 0) the [hi | lo] pair of ESS_FMT_F16_C8_HILO,
 *                          [N][2 ceil(C/8)][H][W][8] (event latents handed over as fp32 tensors: models/style_networks.py:69-88);
 *   ess_bf16_c8_to_f16_c8  BF16_C8 -> F16_C8, n_vec 16-byte vectors (exact but for |v| > 65504 / < 6e-8; the image encoder's latents);
 *   ess_f16_c8_to_bf16_c8  F16_C8, or (hilo != 0) a [hi | lo] pair summed, -> BF16_C8 (round to nearest even): the form the weight
 *                          gradient, the skip connection and the L1 terms of the trainable decoder keep reading.                    */
int ess_to_f16_c8(const float* x, void* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t hilo, ess_stream_t stream);
int ess_bf16_c8_to_f16_c8(const void* x, void* y, int64_t n_vec, ess_stream_t stream);
int ess_f16_c8_to_bf16_c8(const void* x, void* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t hilo, ess_stream_t stream);

/* Weight gradient of the same convolution (replaces cuDNN wgrad under autograd for
 * models/style_networks.py:158-193 and the ResNet prefix :116-121).
 * dy: [N][C_out][H_out][W_out].  dw: [C_out][C0+C1][k][k] (overwritten, or accumulated when
 * accumulate != 0).  db: [C_out] or NULL.  workspace: ess_conv2d_wgrad_workspace() bytes.          */
/* Storage formats (bf16 compute): d->fmt0 (= fmt1) is the sources' format, d->fmt_out that of dy.  Both BF16_C8: 3x3 / stride 1 /
 * pad 1 (direct or nearest-upsampled, one or two sources) and 1x1 / pad 0 (stride 1 or 2) convolutions -- the tiles are
 * transposed to channel-major in registers while they are staged; X BF16_C8 + dy fp32: the 1x1 head (C_in, C_out <= 32);
 * X fp32 + dy BF16_C8: the single-channel 7x7 stem.                                                          */
size_t ess_conv2d_wgrad_workspace(const EssConvDesc* d);
int ess_conv2d_wgrad(const EssConvDesc* d, const void* src0, const void* src1, const void* dy,
                     float* dw, float* db, int accumulate, void* workspace, size_t workspace_bytes,
                     ess_stream_t stream);
/* The weight gradient over n_sets (1..3) tensor sets of the same convolution: dw (+)= sum_s wgrad(src0[s], src1[s], dy[s]).  BF16_C8
 * 3x3 / stride 1 / pad 1: one launch for all sets (one split-K slab set, one reduce); otherwise one accumulating call per set.
 * No reference counterpart (autograd accumulates per backward pass): the decoder's two weight-gradient passes of a UDA step.       */
int ess_conv2d_wgrad_sets(const EssConvDesc* d, int32_t n_sets, const void* const* src0, const void* const* src1,
                          const void* const* dy, float* dw, float* db, int32_t accumulate, void* workspace,
                          size_t workspace_bytes, ess_stream_t stream);

/* InstanceNorm2d(affine=False, eps) (+residual)(+ReLU): models/style_networks.py:163-164,180-182,192.
 * relu = 0: y = IN(x) + residual; 1: y = relu(IN(x)) + residual; 2 (forward only): y = relu(IN(x) +
 * residual) (ResidualBlock with norm='IN', e2vid/model/submodules.py:157-172).
 * stats: [N*C][2] = (mean, rstd) saved for backward.                                                */
size_t ess_norm_workspace(int32_t groups); /* groups = planes (InstanceNorm) or channels (BatchNorm) */
int ess_instnorm_forward(const float* x, const float* residual, float* y, float* stats, int32_t planes,
                         int32_t hw, float eps, int32_t relu, void* workspace, size_t workspace_bytes,
                         ess_stream_t stream);
/* dx from dy (gradient w.r.t. y; the residual branch gradient is dy itself, handled by the caller). */
int ess_instnorm_backward(const float* x, const float* dy, const float* stats, float* dx, int32_t planes,
                          int32_t hw, int32_t relu, void* workspace, size_t workspace_bytes, ess_stream_t stream);

/* ---- the same norms on BF16_C8 tensors (bfloat16 [N][ceil(C/8)][hw][8]; bf16 configuration: the stored form of the trainable
 * networks' activations and activation gradients).  fp32 arithmetic and statistics; stats: fp32 [N*C][2] (InstanceNorm) =
 * (mean, rstd); BatchNorm: fp32 [2][C][2] = C pairs (mean, rstd) followed by C pairs (a, b), the affine map y = x a + b the
 * forward applied (a = rstd gamma, b = beta - mean a): the backward takes its dx scale and -- beta != NULL -- its ReLU mask from
 * that saved map, never from the live gamma / beta.  relu: 0 / 1 as above.  workspace: ess_norm_workspace_c8(N*ceil(C/8)) (InstanceNorm) /
 * ess_norm_workspace_c8(ceil(C/8)) (BatchNorm) bytes.                                                          */
size_t ess_norm_workspace_c8(int32_t groups);
int ess_instnorm_forward_c8(const void* x, const void* residual, void* y, float* stats, int32_t N, int32_t C, int32_t hw,
                            float eps, int32_t relu, int32_t x_f16, void* workspace, size_t workspace_bytes, ess_stream_t stream);
/* InstanceNorm forward of the "mixed" configuration: as ess_instnorm_forward_c8, plus y16 = the result as an F16_C8 tensor (required;
 * what the next ESS_COMPUTE_F16 convolution reads), y (BF16_C8) optional; x_fmt: 0 BF16_C8, 1 F16_C8, 2 the [hi | lo] pair of
 * ESS_FMT_F16_C8_HILO (x = hi + lo); res_f16: 0 the residual is BF16_C8, 1 F16_C8, 2 a [hi | lo] pair (its hi parts are added).  The statistics
 * are those of the values read.  ess_instnorm_backward_c8 takes the same x with x_f16 = x_fmt (2: the hi parts are read).     */
int ess_instnorm_forward_c8_mixed(const void* x, const void* residual, void* y, void* y16, float* stats, int32_t N, int32_t C, int32_t hw,
                                  float eps, int32_t relu, int32_t x_fmt, int32_t res_f16, void* workspace, size_t workspace_bytes,
                                  ess_stream_t stream);
int ess_instnorm_backward_c8(const void* x, const void* dy, const float* stats, void* dx, int32_t N, int32_t C, int32_t hw,
                             int32_t relu, int32_t x_f16, void* workspace, size_t workspace_bytes, ess_stream_t stream);
int ess_batchnorm_train_forward_c8(const void* x, const void* residual, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float momentum, float eps, void* y, float* stats,
                                   int32_t N, int32_t C, int32_t hw, int32_t relu, int32_t x_f16, void* workspace,
                                   size_t workspace_bytes, ess_stream_t stream);
int ess_batchnorm_train_backward_c8(const void* x, const void* y, const void* dy, const float* gamma, const float* beta,
                                    const float* stats, void* dx, void* d_residual, float* dgamma, float* dbeta, int32_t accumulate,
                                    int32_t N, int32_t C, int32_t hw, int32_t relu, int32_t x_f16, void* workspace,
                                    size_t workspace_bytes, ess_stream_t stream);
/* beta: NULL -- the ReLU mask is read from the saved output y (a forward with a residual).  Non-NULL with relu = 1 -- the forward was
 * relu(bn(x)) without a residual: the mask is recomputed from x as (x a + b <= 0) with the forward's a = rstd gamma, b = beta - mean a,
 * y is not read (may be NULL), d_residual must be NULL: two tensor passes less per launch.                                          */
/* x_f16 = 1: x (the pre-normalisation tensor) is an ESS_FMT_F16_C8 tensor; every other tensor stays BF16_C8.          */

/* BatchNorm2d, training mode (ResNet prefix of StyleEncoderE2VID, models/style_networks.py:116-121):
 * batch statistics, running-stat update with momentum (unbiased var), y = act(bn(x) + residual).
 * stats: [C][2] = (mean, rstd).                                                                     */
int ess_batchnorm_train_forward(const float* x, const float* residual, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps, float* y,
                                float* stats, int32_t N, int32_t C, int32_t hw, int32_t relu, void* workspace,
                                size_t workspace_bytes, ess_stream_t stream);
/* dy is the gradient w.r.t. y; `y` is needed for the ReLU mask; d_residual (nullable) receives the
 * masked gradient.  dgamma/dbeta: [C] overwritten or accumulated.                                   */
int ess_batchnorm_train_backward(const float* x, const float* y, const float* dy, const float* gamma,
                                 const float* stats, float* dx, float* d_residual, float* dgamma, float* dbeta,
                                 int32_t accumulate, int32_t N, int32_t C, int32_t hw, int32_t relu,
                                 void* workspace, size_t workspace_bytes, ess_stream_t stream);

/* y = bilinear_x2(a + b), align_corners=False (UpsampleConvLayer input: e2vid/model/submodules.py:84,
 * skip_sum e2vid/model/unet.py:12-13,176).  b may be NULL.  a: [planes][H][W] -> y: [planes][2H][2W] */
int ess_upsample_bilinear2x_add(const float* a, const float* b, float* y, int32_t planes, int32_t H,
                                int32_t W, ess_stream_t stream);
/* The same map written as a BF16_C8 tensor [N][ceil(C/8)][2H][2W][8] for a bf16 convolution to stage (the 5x5 decoder convs of
 * the frozen encoder: identical MFMA operands, half the bytes).  a, b: fp32 [N][C][H][W]; W even.                          */
int ess_upsample_bilinear2x_add_c8(const float* a, const float* b, void* y, int32_t N, int32_t C, int32_t H, int32_t W,
                                   ess_stream_t stream);

/* The same map from BF16_C8 SOURCES a (and b, or NULL), [N][ceil(C/8)][H][W][8] bfloat16: what the frozen encoder's kernels leave
 * as staging copies.  Bit-identical to ess_upsample_bilinear2x_add_c8 applied to the sources' values.
 * Replaces: the same reference lines (e2vid/model/submodules.py:83-93, unet.py:12-13,176). */
int ess_upsample_bilinear2x_add_c8_from_c8(const void* a, const void* b, void* y, int32_t N, int32_t C, int32_t H, int32_t W,
                                           ess_stream_t stream);
/* 2x2 sum pooling = backward of nearest x2 upsampling (F.interpolate, models/style_networks.py:77).
 * accumulate != 0 adds into y.                                                                      */
int ess_sumpool2x2(const float* x, float* y, int32_t planes, int32_t H_out, int32_t W_out, int32_t accumulate,
                   ess_stream_t stream);
/* y = a + b (skip_sum, e2vid/model/unet.py:12-13); in place allowed.                                */
int ess_add(const float* a, const float* b, float* y, int64_t n, ess_stream_t stream);
/* y = a + b (+ c when c != NULL) over bfloat16 tensors of n_vectors x 8 elements (16-byte aligned; any layout, e.g. BF16_C8):
 * fp32 sum, one round to nearest even; in place allowed.  Replaces autograd's gradient accumulation for an activation with
 * several consumers (models/style_networks.py:69-88: out[2] / out[4] feed the next stage and a loss).            */
/* out = sum of n (<= 16) device scalars, added in the order given: the reported total of a train step's weighted loss terms
 * (training/ess_trainer.py:116-138 adds them with one torch op per term).  `terms` is a HOST array of device pointers.  */
int ess_sum_scalars(const float* const* terms, int32_t n, float* out, ess_stream_t stream);
int ess_add_bf16(const void* a, const void* b, const void* c, void* y, int64_t n_vectors, ess_stream_t stream);

/* EventPreprocessor.__call__ normalisation (e2vid/utils/inference_utils.py:96-107) over the whole
 * tensor of n floats: non-zero mean/std, y = (x!=0)*(x-mean)/std; identity copy when all-zero.
 * workspace: >= 32 bytes, zeroed by the call.  No host synchronisation.                             */
int ess_event_normalize(const float* x, float* y, int64_t n, void* workspace, ess_stream_t stream);
/* The same normalisation for all T time slices of a batch in two launches (training/ess_trainer.py:277-280 runs it once per
 * slice data_b[:, t*C:(t+1)*C]): x = [B][T][chunk] with chunk = C*H*W (the event tensor [B, T*C, H, W] as it is: no slice
 * copies), y = [T][B][chunk] (slice t = a contiguous [B, C, H, W] tensor), statistics per slice over the whole batch.
 * workspace: T * 24 bytes.                                                                          */
int ess_event_normalize_slices(const float* x, float* y, int32_t B, int32_t T, int64_t chunk, void* workspace, ess_stream_t stream);
/* The same normalisation PER SAMPLE, for S independent event streams batched into one tensor -- PURELY ADDITIVE to ABI 110:
 * x, y = [S][chunk] with chunk = C*H*W; sample s gets its own non-zero mean / std (an all-zero sample is copied unchanged).
 * Per sample the call repeats ess_event_normalize(x + s*chunk, y + s*chunk, chunk) exactly: the reduction gives every sample the
 * workgroup count, the per-thread element walk and the block sums that call uses for n = chunk (its grid is sized from the element
 * count, so a grid sized from S*chunk would add other partial sums), and the map is the same expression.  A stream's values then do
 * not depend on whether or with whom it was batched -- to the extent ess_event_normalize repeats itself: both add their <= 128
 * workgroup partial sums with fp64 atomics in arrival order, so the fp64 totals can differ in their last bit from run to run before
 * they are rounded to fp32 (no difference has been seen in the results).  mode (device, int32 [S], nullable = every sample active): a sample with mode[s] == 0 is NOT READ and
 * its y is zero-filled (a stream without a window this round: the encoder still sees a defined input).
 * workspace: S * 24 bytes, zeroed by the call.  Three stream operations (memset, reduce, map); no host synchronisation.          */
int ess_event_normalize_samples(const float* x, float* y, int32_t S, int64_t chunk, const int32_t* mode, void* workspace,
                                ess_stream_t stream);

/* Masked carry of a batched recurrent state -- PURELY ADDITIVE to ABI 110.  All levels and all parts of the state (fp32 NCHW h and
 * c, the BF16_C8 copy, the F16_C8 copy incl. its [hi | lo] form, F32_C8) in ONE launch, steered per sample by a mode word in
 * DEVICE memory, so that a captured launch stays valid while the set of advancing / idle / restarting streams changes.
 * dst, src, bytes_per_sample: HOST arrays of n_tensors (1..16) entries; they reach the kernel by value (nothing of them needs to
 * outlive the call, also under stream capture).  Every carried form has the sample index outermost: tensor i = n_samples
 * contiguous records of bytes_per_sample[i] bytes.  mode: device int32 [n_samples]:
 *   ESS_CARRY_HOLD (0, and any other word)  the sample's dst bytes are neither read nor written;
 *   ESS_CARRY_TAKE (1)                      dst record = src record;
 *   ESS_CARRY_ZERO (2)                      dst record = 0; src is not read.
 * src may be NULL when no sample is TAKE; the mode words live on the device, so the entry point cannot refuse a TAKE word that
 * meets a NULL src: such a sample is left as it was (a HOLD).  With a src table every entry must be a pointer.
 * Pointers and bytes_per_sample must be multiples of 16 (every state form is: planes are padded to /8), and the ranges
 * [dst[i], dst[i] + n_samples * bytes) and [src[i], src[i] + n_samples * bytes) must be disjoint; each is checked on the host,
 * ESS_EINVAL with a message otherwise.  A workgroup owns one (tensor, sample, segment), reads mode[sample] once and
 * moves 16-byte vectors; no host synchronisation.                                                                                */
enum { ESS_CARRY_HOLD = 0, ESS_CARRY_TAKE = 1, ESS_CARRY_ZERO = 2 };
int ess_state_carry_masked(void* const* dst, const void* const* src, const int64_t* bytes_per_sample, int32_t n_tensors,
                           int32_t n_samples, const int32_t* mode, ess_stream_t stream);
/* Its indexed sibling -- PURELY ADDITIVE to ABI 110: record moves between two batches of DIFFERENT sizes (the home state of S
 * streams and the compact batch of a round's active streams), steered by two index arrays in DEVICE memory, so that one captured
 * launch serves every set of active streams.  Host tables as above (by value in the kernel arguments).  Tensor i = n_dst_samples
 * (dst) / n_src_samples (src) contiguous records of bytes_per_sample[i] bytes.  dst_index, src_index: device int32 [n_moves]
 * (1..65535).  For move p, on every tensor:
 *   dst_index[p] outside [0, n_dst_samples)   nothing is read or written (a skipped move: a padded slot);
 *   src_index[p] == ESS_CARRY_SRC_ZERO (-1)   dst record dst_index[p] = 0; no source is read;
 *   src_index[p] in [0, n_src_samples)        dst record dst_index[p] = src record src_index[p];
 *   any other src_index[p]                    nothing is read or written.
 * No index word takes the kernel outside the two ranges.  Two moves with the same valid dst_index are the caller's error (the
 * content is unspecified, the bounds hold).  src may be NULL (zero-fills and skips only; a valid src_index then moves nothing).
 * Host checks as above, the disjointness with each side's own record count; ESS_EINVAL with a message otherwise.  A workgroup owns
 * one (tensor, move, segment), reads its two index words once and moves 16-byte vectors; no host synchronisation.               */
enum { ESS_CARRY_SRC_ZERO = -1 };
int ess_state_carry_indexed(void* const* dst, const void* const* src, const int64_t* bytes_per_sample, int32_t n_tensors,
                            int32_t n_dst_samples, int32_t n_src_samples, int32_t n_moves, const int32_t* dst_index,
                            const int32_t* src_index, ess_stream_t stream);

/* ---- events -> voxel grid on the device (the step in front of the encoder) --------------------
 * All slices of a batch in one launch: events concatenated structure-of-arrays, slice s = [slice_offsets[s],
 * slice_offsets[s+1]) (int64, device, n_slices+1 entries); `out` is zeroed by the call.
 *
 * ess_voxel_grid_trilinear replaces VoxelGrid.convert (DSEC/dataset/representations.py:15-55) as driven by
 * Sequence.events_to_voxel_grid (DSEC/dataset/sequence.py:144-154): x, y float pixel coordinates, pol in {0,1},
 * t = any increasing fp32 time; each slice is mapped to [0, channels-1] from its own first/last event.
 * out: [n_slices][channels][height][width].                                                          */
int ess_voxel_grid_trilinear(const float* x, const float* y, const float* pol, const float* t,
                             const int64_t* slice_offsets, int64_t n_events, int32_t n_slices, int32_t channels,
                             int32_t height, int32_t width, float* out, void* workspace, size_t workspace_bytes,
                             int64_t max_events_per_slice, ess_stream_t stream);
/* workspace NULL: every event issues its (up to) 8 atomic adds straight to `out`.  With a workspace of
 * ess_voxel_grid_trilinear_workspace() bytes and max_events_per_slice = the longest slice (host knowledge: it sizes the
 * launch), events are first grouped by 32x32-pixel tile and each tile is accumulated in LDS (about 8x faster).      */
size_t ess_voxel_grid_trilinear_workspace(int64_t n_events, int32_t n_slices, int32_t height, int32_t width);
/* ess_voxel_grid_temporal replaces generate_voxel_grid (datasets/data_util.py:54-126): integer pixels, fp64
 * timestamps, polarity +1 / -1 (0 counts as -1), bilinear in time only.
 * out: [n_slices][separate_pol ? 2*bins : bins][height][width] (positive bins first; else positive - negative). */
int ess_voxel_grid_temporal(const int32_t* x, const int32_t* y, const double* t, const float* pol,
                            const int64_t* slice_offsets, int64_t n_events, int32_t n_slices, int32_t bins,
                            int32_t height, int32_t width, int32_t separate_pol, float* out, ess_stream_t stream);
/* Per-slice normalisation over the non-zero voxels, in place.  mode 0: VoxelGrid(normalize=True)
 * (representations.py:45-53: unbiased std, divide only if std > 0); mode 1: normalize_voxel_grid
 * (data_util.py:38-51: sqrt(E[v^2]-mean^2), no guard).  workspace: ess_voxel_normalize_workspace() bytes.        */
size_t ess_voxel_normalize_workspace(int32_t n_slices);
int ess_voxel_normalize(float* grid, int32_t n_slices, int64_t elems_per_slice, int32_t mode, void* workspace,
                        size_t workspace_bytes, ess_stream_t stream);

/* Event ingest for a captured round -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing entry point changes).
 * The temporal flavour above, one signed grid per stream (separate_pol = 0), with a sum that does not depend on arrival order, in
 * two launches whose shape follows from `capacity` and the grid size alone: no memset, no host-side count, no synchronisation.
 * records (device, 16-byte aligned): [n_streams][capacity] packed 16-byte records {double t; int16_t x; int16_t y; int32_t p},
 * p = +1 / -1 (any other word counts as -1).  counts (device, int32 [n_streams]), read by the kernels:
 *   counts[s] >  0: stream s has min(counts[s], capacity) events; its grid is built from them;
 *   counts[s] == 0: an empty window: an all-zero grid;
 *   counts[s] <  0 (ESS_INGEST_KEEP): nothing of stream s is read or written; the grid already in `out` stays.
 * Per event the two contributions are those of ess_voxel_grid_temporal bit for bit (the same fp64 expressions rounded to fp32, the
 * same validity test, first / last = the timestamps of the stream's records 0 and count - 1); each is added as the 64-bit integer
 * llrint(c * 2^40) into acc (int64 [n_streams][bins][height][width], ess_event_ingest_workspace() bytes, 16-byte aligned), and
 * out[v] = (float)acc[v] * 2^-40.  acc must be ALL ZERO on entry (the owner zeroes it once) and is all zero again behind the call.
 * capacity <= 2^22 keeps every sum inside int64.  out: fp32 [n_streams][bins][height][width], 16-byte aligned.                  */
enum { ESS_INGEST_KEEP = -1 };
size_t ess_event_ingest_workspace(int32_t n_streams, int32_t bins, int32_t height, int32_t width);
int ess_event_ingest(const void* records, const int32_t* counts, int64_t capacity, int32_t n_streams, int32_t bins, int32_t height,
                     int32_t width, void* acc, size_t acc_bytes, float* out, ess_stream_t stream);
/* The same ingest from the raw event columns a camera or a DSEC / DDD17 file delivers -- ADDITIVE as well, ess_version() unchanged.
 * t, x, y, p (device, 16-byte aligned): [n_streams][stride] each; t 8 bytes, x and y 2 bytes, p 1 byte per event.  stride: the
 * per-stream capacity, a multiple of 16 (so every stream's row of every column starts 16-byte aligned), 16..2^22.  counts: as
 * above (a count above stride counts as stride).  formats (device, int32 [n_streams]), read by the kernel like the counts, so one
 * captured launch serves streams whose formats change from round to round:
 *   bit 0 (ESS_EVCOL_T_I64):  t is int64 (it enters as (double)t, exact below 2^53), else float64;
 *   bit 1 (ESS_EVCOL_XY_U16): x / y are uint16 (32768.. lie outside every grid: dropped, not wrapped), else int16;
 *   any other bit set: the stream is treated as count 0 (nothing of it is read, an all-zero grid).
 * p: +1 where the byte equals 1, -1 otherwise (uint8 / bool {0, 1} and int8 {-1, +1} alike).  From there on every per-event
 * expression is that of ess_event_ingest: the grids are bit-equal to its grids on the same events.  acc / out: as above.     */
enum { ESS_EVCOL_T_I64 = 1, ESS_EVCOL_XY_U16 = 2 };
int ess_event_ingest_columns(const void* t, const void* x, const void* y, const void* p, const int32_t* counts, const int32_t* formats,
                             int64_t stride, int32_t n_streams, int32_t bins, int32_t height, int32_t width, void* acc,
                             size_t acc_bytes, float* out, ess_stream_t stream);
/* The same ingest from per-stream event RINGS in device memory -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing
 * entry point changes).  t, x, y, p (device, 16-byte aligned): [n_rows][ring] raw columns as above, row r the ring that stream r's
 * packets are appended to as they arrive.  ring: a multiple of 16, 16..2^22 (so no aligned group of 4 events straddles the wrap).
 * rows, starts, counts, formats (device, int32 [n_slots] each), all read by the kernels, so one captured launch serves every round:
 * slot i's window is the counts[i] events of row rows[i] at the positions (starts[i] + k) mod ring, k = 0 .. counts[i] - 1; first /
 * last = the times at starts[i] and at (starts[i] + counts[i] - 1) mod ring; formats[i] as above.  Two slots may name the same row
 * (the columns are only read).
 *   counts[i] == 0: an all-zero grid;  counts[i] < 0 (ESS_INGEST_KEEP): out[i] is neither read nor written;
 *   counts[i] > ring counts as ring;
 *   rows[i] outside [0, n_rows), starts[i] outside [0, ring) or an unknown format bit: the slot counts as empty (nothing of it is
 *   read, an all-zero grid).
 * Every per-event expression is that of ess_event_ingest_columns: the grids are bit-equal to its grids on the same windows.
 * acc: int64 [n_slots][bins][height][width], all zero on entry and again behind the call; out: fp32 [n_slots][bins][height][width]. */
int ess_event_ingest_ring(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                          const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots, int32_t bins,
                          int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out, ess_stream_t stream);
/* The TRILINEAR flavour of the column and the ring ingest -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing
 * entry point changes): the grid the DSEC loader builds (the raw pixel through the camera's rectify map, then VoxelGrid.convert, the
 * trilinear flavour above), from the same raw columns, with the same order-independent sum.  The arguments of ess_event_ingest_columns
 * / ess_event_ingest_ring, and in front of the stream:
 *   maps (device, 16-byte aligned): fp32 [n_maps][map_height][map_width][2], entry [y][x] = the rectified (x, y) of raw pixel (x, y);
 *     null iff n_maps == 0.  n_maps >= 0; map_height, map_width in 1..32768: the SENSOR's size, whatever the grid's height and width
 *     are (a 480-row map over a 440-row grid cuts the bottom 40 rows).
 *   map_of (device, int32 [n_streams] / [n_slots]), read by the kernel like counts and formats:
 *     ESS_RECTIFY_NONE (-1): xe = (float)x, ye = (float)y;
 *     0 .. n_maps - 1: a raw (x, y) outside [0, map_width) x [0, map_height) drops the event, else (xe, ye) = maps[m][y][x];
 *     any other word: the stream / slot counts as empty (nothing of it is read, an all-zero grid).
 * Per event, every step in fp32 and without contraction unless said otherwise; first / last = the window's first and last event:
 *   d = t - t_first in the column's own type (ESS_EVCOL_T_I64: int64 subtraction of the raw words, else fp64), rounded once to fp32;
 *   u = d / d_last;  tn = ((float)(bins - 1) * (u - u_first)) / (u_last - u_first), u_first and u_last formed the same way.  A window
 *   whose last time equals its first gives NaN for every event: an all-zero grid (there is no dT = 1 rescue in this flavour);
 *   the event is dropped unless xe > -2 && xe < width && ye > -2 && ye < height && tn > -2 && tn < bins -- comparisons that NaN fails,
 *   made in front of every float -> int conversion.  These are exactly the events of which some corner lands in the grid under
 *   truncation toward zero (a coordinate in (-2, -1] still reaches index 0, with a weight <= 0: VoxelGrid.convert's quirk, kept);
 *   value = +1 where the polarity byte equals 1, else -1;  x0 = (int)xe, y0 = (int)ye, t0 = (int)tn;  for the up to eight corners
 *   (xl, yl, tb) in {x0, x0 + 1} x {y0, y0 + 1} x {t0, t0 + 1} inside the grid:  wx = value * (1 - |xl - xe|),
 *   wxy = wx * (1 - |yl - ye|), c = wxy * (1 - |tb - tn|) -- ess_voxel_grid_trilinear's expressions -- added as llrint(c * 2^40).
 * |c| <= 1 and an event's corners are distinct voxels: stride / ring <= 2^22 keeps every sum inside int64.  counts, formats, rows,
 * starts, ESS_INGEST_KEEP, acc and out: as for the temporal flavour.  NOT applied: VoxelGrid(normalize=True)'s own per-grid
 * normalisation (ess_voxel_normalize mode 0 does it).                                                                              */
enum { ESS_RECTIFY_NONE = -1 };
int ess_event_ingest_columns_trilinear(const void* t, const void* x, const void* y, const void* p, const int32_t* counts,
                                       const int32_t* formats, int64_t stride, int32_t n_streams, int32_t bins, int32_t height,
                                       int32_t width, void* acc, size_t acc_bytes, float* out, const float* maps, const int32_t* map_of,
                                       int32_t n_maps, int32_t map_height, int32_t map_width, ess_stream_t stream);
int ess_event_ingest_ring_trilinear(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                    const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows,
                                    int32_t n_slots, int32_t bins, int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out,
                                    const float* maps, const int32_t* map_of, int32_t n_maps, int32_t map_height, int32_t map_width,
                                    ess_stream_t stream);

/* The LOADER's grid from the ring ingest -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing entry point changes).
 * The reference loaders do not hand the network the grid they voxelise: DSEC's VoxelGrid(normalize=True) normalises it over its
 * non-zero voxels, both loaders cut rows and resize bilinearly (DSEC resize=True: 480 rows -> the top 440 -> 448 x 640; DDD17: 260 x 346
 * -> 260 x 352 -> the top 200 rows).  All of that sits between the ingest's int64 sums and the fp32 grid, so the ingest is offered in
 * its two halves:
 *
 * ess_event_scatter_ring / ess_event_scatter_ring_trilinear: the arguments of ess_event_ingest_ring / _trilinear without `out`, the
 * same scatter launch, and nothing behind it: acc (all zero before, [n_slots][bins][height][width]) keeps the sums.
 *
 * ess_event_grid_finish: acc [n_slots][bins][src_height][src_width] -> out fp32 [n_slots][bins][out_rows][resize_width].  Per slot,
 * in this order:
 *   1. v = (float)acc * 2^-40 (what ess_event_ingest_ring stores);
 *   2. normalize, over ALL src_height rows of the slot's grid (the loader takes its statistics before it cuts rows):
 *        ESS_GRID_NORM_NONE;
 *        ESS_GRID_NORM_UNBIASED   VoxelGrid(normalize=True): mean and n - 1 std of the non-zero voxels, a non-zero v becomes
 *                                 (v - mean) / std where std > 0, else v - mean (one non-zero voxel: NaN std, the else branch);
 *        ESS_GRID_NORM_POPULATION normalize_voxel_grid: std = sqrt(E[v^2] - mean^2), a non-zero v becomes (v - mean) / std, unguarded;
 *      the case analysis and the fp32 expressions are ess_voxel_normalize's (mode 0 / mode 1), evaluated without fused multiply-add
 *      (equal non-zero voxels give a population std of exactly 0).  Zeros stay zero.  The statistics are exact: count and
 *      sum of the integer-valued (float)acc as int64, sum of squares in fp64 in a FIXED order (per-workgroup partials in `workspace`,
 *      the number of workgroups a function of the slot's size alone, added in workgroup order) -- no atomics, no memset;
 *   3. rows [0, crop_rows) are kept;
 *   4. bilinear resize [crop_rows, src_width] -> [resize_height, resize_width], align_corners=True, torch's fp32 coordinates:
 *      scale = (in - 1) / (out - 1) (0 where out == 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0,
 *      l0 = 1 - l1;  value = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11), no fused multiply-add;
 *   5. rows [0, out_rows) of the resized grid are stored.
 * counts[i] < 0 (ESS_INGEST_KEEP): out[i] is neither read nor written;  counts[i] == 0: acc is zero, so is the grid.  acc is ALL ZERO
 * behind the call.  A slot's grid is a pure function of its sums: the same bits run to run, alone or among other slots.  With
 * crop_rows == src_height == resize_height == out_rows, resize_width == src_width and ESS_GRID_NORM_NONE the grid has the bits of
 * ess_event_ingest_ring's.  Launches shaped by the sizes alone, counts read on the device, no synchronisation: capturable.
 * workspace: ess_event_grid_finish_workspace() bytes, 16-byte aligned, written before it is read (needs no initial value).       */
enum { ESS_GRID_NORM_NONE = 0, ESS_GRID_NORM_UNBIASED = 1, ESS_GRID_NORM_POPULATION = 2 };
int ess_event_scatter_ring(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                           const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots, int32_t bins,
                           int32_t height, int32_t width, void* acc, size_t acc_bytes, ess_stream_t stream);
int ess_event_scatter_ring_trilinear(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                     const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows,
                                     int32_t n_slots, int32_t bins, int32_t height, int32_t width, void* acc, size_t acc_bytes,
                                     const float* maps, const int32_t* map_of, int32_t n_maps, int32_t map_height, int32_t map_width,
                                     ess_stream_t stream);
size_t ess_event_grid_finish_workspace(int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width);
int ess_event_grid_finish(const int32_t* counts, int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width, void* acc,
                          size_t acc_bytes, int32_t crop_rows, int32_t resize_height, int32_t resize_width, int32_t out_rows,
                          int32_t normalize, float* out, void* workspace, size_t workspace_bytes, ess_stream_t stream);

/* The event REPRESENTATIONS of the column / ring ingest -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing entry
 * point changes).  The reference's loaders hand the network one of three representations of a window's events; the entry points
 * above build the first.  These three take the arguments of ess_event_scatter_ring, ess_event_ingest_ring and
 * ess_event_ingest_columns with `channels` -- the planes C of one grid, acc [n][channels][height][width] -- where those take `bins`,
 * and, in front of the stream, a representation word (host side, fixed per call):
 *   ESS_EVENT_REP_SIGNED (0):    C = bins.  The signed temporal grid: the very kernel, and the bits, of the entry points above.
 *   ESS_EVENT_REP_SEPARATE (1):  C = 2 * bins, [positive bins; negative bins] (generate_voxel_grid(separate_pol=True)); channels
 *     must be even.  first, dT (dT == 0 -> 1), ts = ((bins - 1) * (t - first)) / dT, the validity test, ti = (int)ts, dts = ts - ti,
 *     left = (float)(1 - dts), right = (float)dts are ess_event_ingest_columns' own; no sign is applied.  A positive event (polarity
 *     byte == 1) adds llrint(left * 2^40) to plane ti and llrint(right * 2^40) to plane ti + 1 if ti + 1 < bins; any other polarity
 *     adds them to planes bins + ti and bins + ti + 1 under the same test.  Both halves are non-negative, and
 *     acc[b] - acc[bins + b] equals the signed grid's sum exactly.
 *   ESS_EVENT_REP_HISTOGRAM (2): C = 2, [negative counts, positive counts] (generate_event_histogram); channels must be 2.  Every
 *     event whose (x, y) lies in [0, width) x [0, height) adds 2^40 to plane 1 where its polarity byte == 1, else to plane 0.  The
 *     time column is NOT READ (t must still be a valid 16-byte aligned pointer): 5 instead of 13 bytes an event, and an event counts
 *     whatever its time is, a NaN included.  A coordinate outside the grid drops the event; the reference neither checks nor drops
 *     (x + width * y wraps into a neighbouring row, or raises): that is not reproduced.
 * An event adds to a voxel at most once, at most 2^40 in magnitude: ring / stride <= 2^22 keep the sums inside int64 as above, and
 * acc stays a pure function of the SET of events.  Counts, rows, starts, format words, ESS_INGEST_KEEP, alignment, acc (all zero
 * before; all zero again behind the two ingest calls, the sums behind the scatter) and out: as for the entry points above.
 * ess_event_grid_finish / _window take acc with bins = channels: they normalise over all C planes of a slot, as the DDD17 loader
 * normalises the concatenated representation.  Any other representation word, an odd channels with 1, channels != 2 with 2:
 * ESS_EINVAL.                                                                                                                   */
enum { ESS_EVENT_REP_SIGNED = 0, ESS_EVENT_REP_SEPARATE = 1, ESS_EVENT_REP_HISTOGRAM = 2 };
int ess_event_scatter_ring_rep(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                               const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots,
                               int32_t channels, int32_t height, int32_t width, void* acc, size_t acc_bytes, int32_t representation,
                               ess_stream_t stream);
int ess_event_ingest_ring_rep(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                              const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots,
                              int32_t channels, int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out,
                              int32_t representation, ess_stream_t stream);
int ess_event_ingest_columns_rep(const void* t, const void* x, const void* y, const void* p, const int32_t* counts,
                                 const int32_t* formats, int64_t stride, int32_t n_streams, int32_t channels, int32_t height,
                                 int32_t width, void* acc, size_t acc_bytes, float* out, int32_t representation, ess_stream_t stream);

/* HOT-PIXEL MASKS in the column / ring ingest -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing entry point
 * changes, and the unmasked entry points launch the kernels they launched before).  The reference removes hot pixels from the
 * finished grid (events[:, :, y, x] = 0 for every line of hot_pixels_file).  Here a hot pixel's events are dropped where (x, y) is
 * still the RAW sensor coordinate, before a rectify map moves them or a resize blends them: one mask per sensor, picked per slot.
 *   masks (device, 16-byte aligned): uint32 [n_masks][mask_height][mask_words], mask_words = ceil(mask_width / 32); pixel (x, y) is
 *     bit x & 31 of word x >> 5 of row y, a set bit means hot.  null iff n_masks == 0.  mask_height, mask_width in 1..32768: the
 *     SENSOR's size, whatever the grid's, as for the rectify maps.
 *   mask_of (device, int32 [n_slots]), read by the kernel like counts and formats:
 *     ESS_MASK_NONE (-1): no mask;   0 .. n_masks - 1: that mask;
 *     any other word: the slot counts as empty (nothing of it is read, an all-zero grid), as an unknown map word does.
 * Per event: x, y are decoded from the raw words as the format says; the event is DROPPED when it lies inside
 * [0, mask_width) x [0, mask_height) and its bit is set; every other event -- one outside the mask's rectangle included -- goes
 * through the flavour with its words unchanged, and the flavour decides about it as in the unmasked entry points.  The window's
 * time base (first / last, d_last) is taken from the window's first and last event WHETHER THEY ARE MASKED OR NOT: the
 * reference voxelises first and zeroes the pixel afterwards, so its time base counts hot events too.  A masked call therefore gives,
 * bit for bit, what the unmasked entry point gives on columns in which every masked event's x was replaced by a value outside
 * every grid and map (-1, or 65535 under ESS_EVCOL_XY_U16); for the integer-pixel flavours with a mask of the grid's size that is
 * the unmasked grid followed by the reference's zeroing.
 *
 * ess_event_ingest_masked: one entry point for both sources, every flavour and both halves.  t .. acc_bytes: the arguments of
 * ess_event_ingest_ring_rep (`channels` planes a slot).  rows == starts == NULL selects the COLUMN source: slot s's window lies at
 * the head of row s, `ring` is the stride (a multiple of 16), n_rows is not read -- ess_event_ingest_columns*'s launch.  Only one of
 * the two null: ESS_EINVAL.  representation: ESS_EVENT_REP_*.  trilinear: 0, or 1: the trilinear flavour, maps .. map_width are
 * read as by ess_event_ingest_ring_trilinear and representation must be ESS_EVENT_REP_SIGNED (with 0 they are not read).  out:
 * nullable.  NULL: scatter only, acc keeps the sums for ess_event_grid_finish / _finish_window, as behind ess_event_scatter_ring*;
 * else the plain finish follows as in ess_event_ingest_*, and acc is all zero again.  Counts, ESS_INGEST_KEEP, format words, rows,
 * starts, alignment and the 2^22 bound: as they stand -- a mask only removes contributions.  NOT reproduced: a mask applied to
 * the packed-record source (ess_event_ingest); rectified histograms.
 *
 * ess_event_hot_pixel_mask: per-pixel event counts -> masks.  sums (device, 16-byte aligned, READ ONLY): int64
 * [n][2][height][width], the sums the histogram flavour leaves behind a scatter (ESS_EVENT_REP_HISTOGRAM: exact multiples of
 * 2^40, one per event).  thresholds (device, int64 [n], in EVENTS), read by the kernel:
 *   thresholds[i] >= 0: bit (y, x) of masks[i] is set iff (sums[i][0][y][x] + sums[i][1][y][x]) >> 40 > thresholds[i] -- exact
 *     integer arithmetic, both polarities counted together;
 *   thresholds[i] <  0: masks[i] is neither read nor written.
 * masks (device, 16-byte aligned): uint32 [n][height][ceil(width / 32)], the layout above.  mode:
 *   ESS_MASK_REPLACE (0): whole words are written; the bits at x >= width of a row's last word are written as 0;
 *   ESS_MASK_OR (1):      the new bits are or-ed onto the words that are there; the tail bits stay as they were.
 * A wave packs 64 consecutive x of a row with one ballot; plain stores, no atomics, no memset, one launch shaped by n, height and
 * width alone: capturable.  The sums of SEVERAL scatters onto one acc (acc not finished in between) may be thresholded as long
 * as no pixel of a slot collects more than 2^22 events (the int64 bound above).  height, width in 1..32768, n in 1..65535; any
 * other mode: ESS_EINVAL.  NOT provided: a mean + k * sigma rule -- thresholds are the caller's, in events.                      */
enum { ESS_MASK_NONE = -1 };
enum { ESS_MASK_REPLACE = 0, ESS_MASK_OR = 1 };
int ess_event_ingest_masked(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                            const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots,
                            int32_t channels, int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out,
                            int32_t representation, int32_t trilinear, const float* maps, const int32_t* map_of, int32_t n_maps,
                            int32_t map_height, int32_t map_width, const uint32_t* masks, const int32_t* mask_of, int32_t n_masks,
                            int32_t mask_height, int32_t mask_width, ess_stream_t stream);
int ess_event_hot_pixel_mask(const int64_t* sums, int32_t n, int32_t height, int32_t width, const int64_t* thresholds, uint32_t* masks,
                             int32_t mode, ess_stream_t stream);

/* Training batches from events: the loaders' augmentation where the grid is written -- PURELY ADDITIVE to ABI 110.
 * DSEC flips horizontally with p = 0.5 (DSEC/dataset/sequence.py:291-295); DDD17 flips, then crops 120 x 216 at random inside the
 * bottom 120 rows (datasets/ddd17_events_loader.py:87-96, 173-183).  Both are index permutations of the finished grid and of its
 * label, driven by one table:  words: device int32 [n_groups][4] = (flip, y0, x0, reserved), drawn by the host.
 *
 * ess_event_grid_finish_window: ess_event_grid_finish with a sixth step.  Steps 1-5 are its own, word for word (statistics over ALL
 * source rows, the row cuts, the fp32 align-corners blend without fused multiply-add); call the grid they store
 * g[bins][out_rows][resize_width].  Per slot i, with (flip, y0, x0) = words[i / slots_per_group]:
 *   6. out[b][y][x] = g[b][y0 + y][flip ? resize_width - 1 - (x0 + x) : x0 + x]      -- the flip first, then the crop --
 * out: fp32 [n_slots][bins][win_height][win_width], 1 <= win_height <= out_rows, 1 <= win_width <= resize_width (else ESS_EINVAL).
 * The device reads flip as != 0 and clamps y0 into [0, out_rows - win_height], x0 into [0, resize_width - win_width]: no word reads
 * or writes outside a slot.  Only the window's voxels are computed (four neighbours a thread, one 16-byte store, where win_width is
 * a multiple of 4).  Everything else is ess_event_grid_finish's contract: counts[i] < 0 keeps out[i] untouched, counts[i] == 0 gives
 * zeros, acc is ALL ZERO behind the call (the sums no output read included: the clear is a pass of its own in every geometry), a
 * slot's output is a pure function of its sums and its words, launches shaped by the sizes alone, words and counts read on the device,
 * no synchronisation: capturable.  workspace: ess_event_grid_finish_workspace() bytes.
 *
 * ess_label_window: src uint8 [n][src_height][src_width] -> out int64 [n][win_height][win_width]: nearest resize to
 * [resize_height][resize_width] by the integer rule sy = min(floor(dy * src_height / resize_height), src_height - 1) (x alike), then
 * step 6 with sample i's row words[i] and the same clamps.  Values pass unchanged (255 stays 255).                              */
int ess_event_grid_finish_window(const int32_t* counts, int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width, void* acc,
                                 size_t acc_bytes, int32_t crop_rows, int32_t resize_height, int32_t resize_width, int32_t out_rows,
                                 int32_t normalize, const int32_t* words, int32_t slots_per_group, int32_t win_height, int32_t win_width,
                                 float* out, void* workspace, size_t workspace_bytes, ess_stream_t stream);
int ess_label_window(const uint8_t* src, int32_t n, int32_t src_height, int32_t src_width, int32_t resize_height, int32_t resize_width,
                     const int32_t* words, int32_t win_height, int32_t win_width, int64_t* out, ess_stream_t stream);

/* DEVICE EVENT STORE: training windows cut on the device out of recordings uploaded once -- PURELY ADDITIVE to ABI 110.
 * The store is ONE flat set of the four columns in device memory (t 8 bytes, x / y 2, p 1 per event, each 16-byte aligned):
 * `capacity` events, a multiple of 16 up to 2^40, of which the first `total` are filled, recordings laid one behind the other.
 *
 * ess_event_scatter_store: the scatter half of the ingest (ess_event_scatter_ring*) on the store.  Slot s's window is counts[s]
 * events from ABSOLUTE event index starts[s] (int64, device), read under formats[s] (ESS_EVCOL_*); nothing wraps.  Counted as
 * count 0 (the slot's planes of acc stay as they are): starts[s] < 0, starts[s] + counts[s] > total, counts[s] > window_capacity,
 * an unknown format bit, and under ESS_EVENT_STORE_TRILINEAR an unknown map word.  window_capacity (1 .. 2^22, the int64 sums'
 * bound) shapes the launch, NOT the store's size; every index on the path is 64-bit.  flavour: ESS_EVENT_STORE_SIGNED, _SEPARATE,
 * _HISTOGRAM (the ESS_EVENT_REP_* words and their rules for `channels`) or _TRILINEAR (maps .. map_width as for
 * ess_event_scatter_ring_trilinear; with any other flavour they are not read).  The sums are, bit for bit, what the ring source
 * leaves for the same events.  Hot-pixel masks on this source: ess_event_ingest_store, below.
 *
 * ess_event_store_windows: a batch's sample table -> the n_samples * T slot words.  table (device, int64 [n_recordings][4]):
 * (begin, end, format, reserved) per recording, absolute indices with 0 <= begin <= end <= total; a negative format word marks an
 * unused row.  recording (int32 [n_samples]): the sample's row.  bounds (8-byte words, [n_samples][1], or [n_samples][T + 1] under
 * ESS_EVENT_STORE_RULE_DURATION): time bounds in the recording's OWN time type (int64, or fp64 bits), prepared by the host; the
 * device finds "the first index in [begin, end) with t >= bound, end where there is none".  rule:
 *   ESS_EVENT_STORE_RULE_COUNT_TIME (0):  e = that index for bounds[b][0];  start = max(begin, e - T * n_per_window);
 *                                         n = (e - start) / T;  window i = (start + i n, n); the remainder at the END is unused
 *   ESS_EVENT_STORE_RULE_COUNT_INDEX (1): the same with e = begin + bounds[b][0], an int64 index relative to the recording; no search
 *   ESS_EVENT_STORE_RULE_DURATION (2):    idx_j = that index for bounds[b][j];  window i = (idx_i, idx_(i+1) - idx_i)
 * starts (int64), counts, formats (int32 [n_samples * T]) and flags (int32 [n_samples]) are WRITTEN for every sample; sample_map
 * (int32 [n_samples]) and map_of (int32 [n_samples * T]) are both given -- map_of[b T + i] = sample_map[b] -- or both null.  flags:
 *   ESS_EVENT_STORE_FLAG_EMPTY (1):    n == 0, or every window is empty;
 *   ESS_EVENT_STORE_FLAG_OVERFLOW (2): a window holds more than window_capacity events: ALL T counts of the sample are 0;
 *   ESS_EVENT_STORE_FLAG_RANGE (4):    the recording number is outside the table (or names an unused or malformed row), e is outside
 *                                      the recording: starts, counts and formats are 0; or the bounds descend: the counts are 0.
 * One workgroup a sample, one wave a bound (a 64-ary search: <= 7 dependent loads over 2^40 events); no synchronisation, nothing
 * read back: capturable.  n_samples * T in 1..65535, n_per_window in 1..window_capacity under the count rules.               */
enum { ESS_EVENT_STORE_SIGNED = 0, ESS_EVENT_STORE_SEPARATE = 1, ESS_EVENT_STORE_HISTOGRAM = 2, ESS_EVENT_STORE_TRILINEAR = 3 };
enum { ESS_EVENT_STORE_RULE_COUNT_TIME = 0, ESS_EVENT_STORE_RULE_COUNT_INDEX = 1, ESS_EVENT_STORE_RULE_DURATION = 2 };
enum { ESS_EVENT_STORE_FLAG_EMPTY = 1, ESS_EVENT_STORE_FLAG_OVERFLOW = 2, ESS_EVENT_STORE_FLAG_RANGE = 4 };
int ess_event_scatter_store(const void* t, const void* x, const void* y, const void* p, const int64_t* starts, const int32_t* counts,
                            const int32_t* formats, int64_t capacity, int64_t total, int64_t window_capacity, int32_t n_slots,
                            int32_t channels, int32_t height, int32_t width, void* acc, size_t acc_bytes, int32_t flavour,
                            const float* maps, const int32_t* map_of, int32_t n_maps, int32_t map_height, int32_t map_width,
                            ess_stream_t stream);
int ess_event_store_windows(const void* t, int64_t capacity, int64_t total, const int64_t* table, int32_t n_recordings,
                            const int32_t* recording, const int64_t* bounds, const int32_t* sample_map, int32_t n_samples, int32_t T,
                            int32_t rule, int64_t n_per_window, int64_t window_capacity, int64_t* starts, int32_t* counts,
                            int32_t* formats, int32_t* map_of, int32_t* flags, ess_stream_t stream);

/* HOT-PIXEL MASKS ON THE STORE SOURCE, and masks calibrated from a stored recording -- PURELY ADDITIVE to ABI 110 (no enumerator is
 * added: the ESS_EVENT_STORE_* flavours, ESS_MASK_* and ESS_EVCOL_* words above are reused; ess_event_scatter_store launches the
 * kernels it launched before).
 *
 * ess_event_ingest_store: ess_event_ingest_masked's counterpart on the store -- one entry point for the four flavours, both halves,
 * with or without masks.  t .. acc_bytes, flavour, maps .. map_width: the arguments of ess_event_scatter_store, with its slot
 * refusals (a negative start, start + count > total, count > window_capacity, an unknown format bit or map word: the slot counts as
 * empty); with a flavour other than ESS_EVENT_STORE_TRILINEAR maps and map_of must be null and n_maps 0 (ESS_EINVAL otherwise).
 * out (nullable, 16-byte aligned): fp32 [n_slots][channels][height][width] -- the plain finish follows the scatter as behind
 * ess_event_ingest_ring*: the same bits, acc all zero again; NULL: scatter only, acc keeps the sums for ess_event_grid_finish*.
 * masks .. mask_width: the five mask arguments of ess_event_ingest_masked, with its semantics word for word -- a hot event is dropped
 * on its RAW (x, y), before a rectify map sees it; the window's time base comes from its first and last event, masked or not; a
 * mask word that is neither ESS_MASK_NONE nor in 0 .. n_masks - 1 makes the slot empty.  mask_of is never null; masks null with
 * n_masks 0 and every word ESS_MASK_NONE: no masking, the sums of ess_event_scatter_store bit for bit.
 *
 * ess_event_store_pixel_counts: plain per-pixel event counts of n index ranges of the store.  Job j: the events begins[j] ..
 * ends[j] - 1 (device int64 words, ABSOLUTE indices, a range as long as the store: up to 2^40 events), decoded under formats[j]
 * (device int32, ESS_EVCOL_XY_U16 read; ESS_EVCOL_T_I64 accepted, the time column is not read).  counts (device, int64
 * [n][height][width], 8-byte aligned) is ADDED TO: one per event, both polarities together; an event whose decoded coordinate lies
 * outside [0, width) x [0, height) is dropped.  A range outside [0, total], begins[j] > ends[j] or an unknown format bit: the job
 * counts nothing.  Only x and y are read (4 bytes an event); every index is 64-bit; the launch follows from capacity, n alone:
 * capturable.  Plain counts hold what the histogram flavour's sums cannot: more than 2^22 events on one pixel.
 *
 * ess_event_count_mask: ess_event_hot_pixel_mask's rule on such counts -- int64 [n][height][width], one plane, no 2^40 scale: bit
 * (y, x) of masks[i] is set iff counts[i][y][x] > thresholds[i]; thresholds[i] < 0: masks[i] is neither read nor written.  masks,
 * mode, the word layout, the tail-bit rule and the limits: as for ess_event_hot_pixel_mask (the same kernel).                  */
int ess_event_ingest_store(const void* t, const void* x, const void* y, const void* p, const int64_t* starts, const int32_t* counts,
                           const int32_t* formats, int64_t capacity, int64_t total, int64_t window_capacity, int32_t n_slots,
                           int32_t channels, int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out, int32_t flavour,
                           const float* maps, const int32_t* map_of, int32_t n_maps, int32_t map_height, int32_t map_width,
                           const uint32_t* masks, const int32_t* mask_of, int32_t n_masks, int32_t mask_height, int32_t mask_width,
                           ess_stream_t stream);
int ess_event_store_pixel_counts(const void* x, const void* y, int64_t capacity, int64_t total, const int64_t* begins,
                                 const int64_t* ends, const int32_t* formats, int32_t n, int32_t height, int32_t width, int64_t* counts,
                                 ess_stream_t stream);
int ess_event_count_mask(const int64_t* counts, int32_t n, int32_t height, int32_t width, const int64_t* thresholds, uint32_t* masks,
                         int32_t mode, ess_stream_t stream);

/* ---- image-branch augmentation on the device: the geometric + photometric core of the albumentations
 * pipeline of datasets/cityscapes_loader.py:39-74 (HorizontalFlip, ShiftScaleRotate with rotate 0 and a constant-0 border,
 * centred PadIfNeeded, RandomCrop, GaussNoise, RandomBrightnessContrast), uint8 quantisation, ToTensor (/255), and for the label
 * map nearest sampling + the id -> trainId table of utils/labels.py:123-127 -- a whole batch in one launch.
 * img: fp32 [N][H_src][W_src] on the 0..255 scale; label (nullable): int64 [N][H_src][W_src] raw ids; id_lut (nullable):
 * int64[256]; params: fp32 [N][12] = flip, scale, dx, dy (pixels), pad_top, pad_left, crop_y, crop_x, alpha, beta (levels),
 * noise sigma (levels, 0 = off), noise seed -- drawn by the host.  out_img: fp32 [N][1][H][W] in [0,1]; out_label: int64.   */
int ess_augment_image_label(const float* img, const int64_t* label, const float* params, const int64_t* id_lut, float* out_img,
                            int64_t* out_label, int32_t N, int32_t H_src, int32_t W_src, int32_t H, int32_t W,
                            ess_stream_t stream);

/* second stage of the same pipeline (datasets/cityscapes_loader.py:45-57): A.Perspective(p=0.2) -- the homography of a jittered
 * quadrilateral onto a max_w x max_h rectangle (bilinear, constant-0 border; label nearest) followed by the resize back to
 * H x W (keep_size) --, then RandomBrightnessContrast, then A.OneOf([Sharpen, Blur(3), MotionBlur(3)], p=0.5) as one 3 x 3
 * correlation with BORDER_REFLECT_101, rounded to nearest-even like cv2.filter2D; ToTensor.  When this stage follows, stage 1 runs
 * with alpha = 1, beta = 0 and id_lut = NULL (the id -> trainId table is applied here, after the geometry, as the reference does).
 * img: fp32 [N][1][H][W] in [0,1] (stage 1's output, levels / 255); label (nullable): int64 [N][H][W] raw ids;
 * params: fp32 [N][24] = perspective fired, inverse homography (9, row-major: rectangle pixel -> source position), max_w, max_h,
 * alpha, beta (levels), stencil fired, 3 x 3 kernel (9); scratch: fp32 [N][H][W]; out_img: fp32 [N][1][H][W]; out_label int64. */
int ess_augment_perspective_filter(const float* img, const int64_t* label, const float* params, const int64_t* id_lut,
                                   float* scratch, float* out_img, int64_t* out_label, int32_t N, int32_t H, int32_t W,
                                   ess_stream_t stream);

/* stage 1 of the pipeline above (ess_augment_image_label: the same kernel body, another pixel source) reading uint8 STORE SLOTS
 * through an index: sample n is slot index[n] of images / labels, uint8 [n_slots][H_slot][W_slot] (datasets/image_store.py), of
 * which only the top `rows` rows exist for the augmentation (the loader's img[:height] under random_crop): H_src = rows,
 * W_src = W_slot.  No float [N][H_src][W_src] copy is made.  index: int32 [N] on the device; a word outside [0, n_slots) gives an
 * all-zero sample (image 0, label id 0).  labels (nullable, with out_label).  The output bits are those of
 * ess_augment_image_label on (float) images[index][:, :rows] and (int64) labels[index][:, :rows].                              */
int ess_augment_image_label_store(const uint8_t* images, const uint8_t* labels, const int32_t* index, int32_t n_slots,
                                  int32_t H_slot, int32_t W_slot, int32_t rows, const float* params, const int64_t* id_lut,
                                  float* out_img, int64_t* out_label, int32_t N, int32_t H, int32_t W, ess_stream_t stream);

/* ---- image ingest for the device image store (csrc/image_store.hip; datasets/cityscapes_loader.py:26-29, 86-96): one decoded
 * frame -> its uint8 [Hr][Wr] slot in PIL's own integer arithmetic: convert('L') (channels == 3:
 * L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16), Image.resize(BILINEAR) in two passes with an 8-bit intermediate,
 * horizontal first -- pixel = clip8((2^21 + sum_i k_i p_i) >> 22) over the window (first, count) of an output index --, the
 * label's Image.resize(NEAREST) as a gather, and (standardize != 0) the loader's stretch
 * v -> (uint8) trunc(255.0 * (v - min) / (max - min)) in IEEE fp64 over the whole resized frame (a constant frame: all 0).
 * frame: uint8 [H][W][channels], channels 1 | 3.  h_table: int32 [2 + h_taps][Wr] = first input index, count, then h_taps planes of
 * 22-bit fixed-point coefficients (count <= h_taps <= ESS_IMAGE_MAX_TAPS), built by the host in float64; NULL exactly where
 * W == Wr (PIL skips a pass that changes nothing); v_table: int32 [2 + v_taps][Hr] likewise.  scratch: uint8 [H][Wr] (needed with
 * channels == 3 or a horizontal pass).  minmax (nullable; needed with standardize): 2 int32 words that receive the resized frame's
 * min and max BEFORE the stretch.  label (nullable, with out_label, label_rows int32 [Hr], label_cols int32 [Wr]): uint8 [H][W]
 * -> out_label uint8 [Hr][Wr] = label[label_rows[y]][label_cols[x]].  Every buffer on the device; up to five launches.            */
#define ESS_IMAGE_MAX_TAPS 33     /* 2 * ceil(in / out) + 1: a side shrinks by at most 16 */
#define ESS_IMAGE_MAX_SIDE 32768
int ess_image_ingest(const uint8_t* frame, int32_t channels, int32_t H, int32_t W, const int32_t* h_table, int32_t h_taps,
                     const int32_t* v_table, int32_t v_taps, uint8_t* scratch, uint8_t* out, int32_t Hr, int32_t Wr,
                     int32_t standardize, int32_t* minmax, const uint8_t* label, const int32_t* label_rows,
                     const int32_t* label_cols, uint8_t* out_label, ess_stream_t stream);

/* ---- PAIRED CAMERA FRAMES of the event loaders (DSEC/dataset/sequence.py:166-176, datasets/ddd17_events_loader.py:187-213) --
 * PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing entry point changes).  The loaders call Image.resize without a
 * filter -- PIL's default is BICUBIC there, whose tables hold negative coefficients -- on the RGB image, and transforms.Grayscale()
 * behind it; DDD17 keeps the top 200 of its 260 resized rows.  One frame -> the top out_rows (<= Hr) rows of its resized gray
 * image, uint8 [out_rows][Wr], with the tables of either filter (the layout above, built by the host):
 *   channels == 3, gray_last == 1   the horizontal pass on all three channels with one window's coefficients, each channel to
 *                                   clip8((2^21 + sum k p) >> 22), into scratch uint8 [H][Wr][3]; the vertical pass per channel
 *                                   likewise, and L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16 at its end.  A pass whose side
 *                                   stays is skipped (its table NULL); the conversion still runs last.
 *   channels == 1, or gray_last == 0  ess_image_ingest's arithmetic on one channel (channels == 3: gray first), scratch uint8 [H][Wr]
 * The sums are int32, the shift of a negative sum is arithmetic and the clip cuts on both sides: a bicubic window overshoots.  A
 * table must keep 2^21 + 255 sum |k| below 2^31 (bicubic: sum |k| <= 1.3 x 2^22).  Only the source rows that a kept output row's
 * window reads go through the horizontal pass; rows of `out` behind out_rows are not written.  scratch is needed where a horizontal
 * pass runs (h_table, or channels == 3 with gray_last == 0).  Every buffer on the device; one or two launches, no float.          */
int ess_image_ingest_frame(const uint8_t* frame, int32_t channels, int32_t H, int32_t W, const int32_t* h_table, int32_t h_taps,
                           const int32_t* v_table, int32_t v_taps, uint8_t* scratch, uint8_t* out, int32_t Hr, int32_t Wr,
                           int32_t out_rows, int32_t gray_last, ess_stream_t stream);

/* transforms.ToTensor() on B stored frames -- ADDITIVE as well: out fp32 [B][1][Hs][Ws] = images[index[b]] / 255, images uint8
 * [capacity][Hs][Ws], one IEEE fp32 division per byte value (the bits of torch's .float().div(255) on the host; no reciprocal).
 * index: B words on the device, int32 (index_i64 == 0) or int64 (1), read by the kernel; a word outside [0, capacity) gives an
 * all-zero frame.  One launch.                                                                                                   */
int ess_image_gather_unit(const uint8_t* images, int64_t capacity, int32_t Hs, int32_t Ws, const void* index, int32_t index_i64,
                          int32_t B, float* out, ess_stream_t stream);

/* TaskLoss = Dice + CrossEntropy (utils/loss_functions.py:6-24,96-135), forward AND gradient w.r.t.
 * logits in one pass pair.  logits [N][K][H][W], labels int64 [N][H][W].  loss: 1 float.
 * dlogits (nullable): d(loss*loss_scale)/dlogits.  workspace: ess_task_loss_workspace(K) bytes.     */
size_t ess_task_loss_workspace(int32_t K);
int ess_task_loss(const float* logits, const int64_t* labels, float* loss, float* dlogits, float loss_scale,
                  int32_t N, int32_t K, int32_t hw, int32_t ignore_index, int32_t use_dice, int32_t use_ce,
                  void* workspace, size_t workspace_bytes, ess_stream_t stream);
/* Workspace of the mean-type losses below (ess_sym_js_loss, ess_l1_loss, ess_l1_loss_c8): one partial sum per workgroup.  Each loss is
 * TWO launches: the kernel proper (every workgroup stores its partial: no atomics, no memset in front) and a one-workgroup finalize
 * that adds the partials in workgroup order -- the value does not depend on scheduling.  Nothing to initialise.  Do not share the
 * buffer between streams.  ABI 110 (round 6): every loss entry point takes workspace_bytes and returns ESS_EINVAL when the buffer is
 * smaller than it needs (ABI 100 callers passed 8 bytes here until round 5 made it one partial per workgroup).                  */
#define ESS_LOSS_WORKSPACE_BYTES (8 * (1 + 2048))
/* symJSDivLoss (utils/loss_functions.py:27-37): loss (1 float) and gradient w.r.t. `a` only
 * (the other argument is always computed under no_grad by the trainers).  workspace: ESS_LOSS_WORKSPACE_BYTES (see above). */
int ess_sym_js_loss(const float* a, const float* b, float* loss, float* da, float loss_scale, int32_t N,
                    int32_t K, int32_t hw, void* workspace, size_t workspace_bytes, ess_stream_t stream);
/* L1Loss mean (training/ess_trainer.py:217-229): loss and gradient w.r.t. a.  workspace: ESS_LOSS_WORKSPACE_BYTES.  */
int ess_l1_loss(const float* a, const float* b, float* loss, float* da, float loss_scale, int64_t n,
                void* workspace, size_t workspace_bytes, ess_stream_t stream);

/* L1Loss mean over BF16_C8 operands (bf16 configuration: the latents / intermediate predictions the cycle losses compare are
 * stored as BF16_C8); da (nullable): BF16_C8 gradient.  n_vectors 16-byte pixel vectors, n REAL elements (the mean's
 * denominator; padded tail channels are zero in both operands).  workspace: ESS_LOSS_WORKSPACE_BYTES.               */
int ess_l1_loss_c8(const void* a, const void* b, float* loss, void* da, float loss_scale, int64_t n_vectors, int64_t n,
                   void* workspace, size_t workspace_bytes, ess_stream_t stream);

/* RAdam.step over ONE flat parameter buffer (utils/radam.py:15-80, weight_decay = 0).
 * step_size / n_sma_ge5 are computed by the host exactly as radam.py:49-64.                         */
int ess_radam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                   float beta1, float beta2, float eps, float step_size, int32_t n_sma_ge5,
                   ess_stream_t stream);

/* The same update with the two step-dependent scalars in device memory: hyper[0] = -step_size * lr, hyper[1] != 0 in the
 * rectified phase (N_sma >= 5).  For a train step captured in a hipGraph: the host writes `hyper` before each replay.       */
int ess_radam_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1, float beta2,
                       float eps, const float* hyper, ess_stream_t stream);

/* F.interpolate(x, size=(H_out, W_out), mode='nearest') on fp32 [planes][H_in][W_in] -- the resize of the validation
 * logits to img_size_b (training/ess_trainer.py:484,525; training/ess_supervised_trainer.py:284).               */
int ess_resize_nearest(const float* x, float* y, int32_t planes, int32_t H_in, int32_t W_in, int32_t H_out,
                       int32_t W_out, ess_stream_t stream);

/* argmax over K + confusion-matrix accumulation (training/ess_trainer.py:485; evaluation/metrics.py:4-24)
 * pred_lbl (nullable): int64 [N][H][W]; conf: int64 [K][K], accumulated (conf[label][pred]).         */
int ess_argmax_confusion(const float* logits, const int64_t* labels, int64_t* pred_lbl, int64_t* conf,
                         int32_t N, int32_t K, int32_t hw, int32_t ignore_index, ess_stream_t stream);

/* Fused class head at inference -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no existing entry point changes):
 * per output pixel z_k = bias[k] + sum_c weight[k][c] x[c] (the 1x1 convolution decoder_scale_5 of SemSegE2VID,
 * models/style_networks.py:66,87), label = the FIRST argmax_k z_k -- without writing the scores.  Replaces, for a caller that wants
 * labels and not logits, conv1x1 -> F.interpolate(nearest) -> argmax (training/ess_trainer.py:424-493).
 * x: fmt ESS_FMT_F32_NCHW [N][C][H][W] fp32, ESS_FMT_BF16_C8 or ESS_FMT_F16_C8 [N][ceil(C/8)][H][W][8].  weight [K][C], bias [K]: the
 * plain fp32 parameters; the kernel rounds the weight to the operand type of the source while loading it (bfloat16 / IEEE half
 * saturating at +-65504 / none) and masks c >= C; fp32 accumulation.  K <= 64; K x C must fit 64 KiB of LDS as floats.
 * Source pixel of output pixel (oy, ox): (win_y0 + min(floor(oy * (float)win_h / H_out), win_h - 1), win_x0 + ...) -- the index rule
 * of ess_resize_nearest inside the window (win_y0, win_x0, win_h, win_w) of the source plane, so that labels equal "resize the
 * scores, then argmax"; the identity plus an offset when the sizes agree.
 * labels: uint8 [N][H_out][W_out] (required).  colour (nullable; needs palette, uint8 [K][3]): uint8 [N][H_out][W_out][3] =
 * palette[label].  confidence (nullable): fp32 [N][H_out][W_out] = 1 / sum_k exp(z_k - z_max), the winner's softmax probability. */
int ess_seg_head(const void* x, int32_t fmt, const float* weight, const float* bias, const uint8_t* palette, uint8_t* labels,
                 uint8_t* colour, float* confidence, int32_t N, int32_t C, int32_t K, int32_t H, int32_t W, int32_t win_y0,
                 int32_t win_x0, int32_t win_h, int32_t win_w, int32_t H_out, int32_t W_out, ess_stream_t stream);

/* The class head that scores itself -- PURELY ADDITIVE to ABI 110: ess_seg_head (the same per-pixel code, so labels, colour and
 * confidence are its bits) plus, per sample, confusion[n][gt][label] += 1 over the output pixels whose ground truth is neither
 * ignore_index nor >= K (the rule of ess_label_confusion).  gt: uint8 [N][H_out][W_out]; confusion: int64 [N][K][K], ACCUMULATED
 * (the caller zeroes it): integer sums, so the result does not depend on the order of the additions.  One grid row per sample, a
 * K x K histogram in LDS per workgroup, one 64-bit atomic per non-zero cell.  Both gt and confusion are required (ess_seg_head is the
 * head without them); the K x K x 4 bytes of counts come on top of the weights in the 64 KiB of LDS; N <= 65535.                */
int ess_seg_head_eval(const void* x, int32_t fmt, const float* weight, const float* bias, const uint8_t* palette, uint8_t* labels,
                      uint8_t* colour, float* confidence, const uint8_t* gt, int64_t* confusion, int32_t ignore_index, int32_t N,
                      int32_t C, int32_t K, int32_t H, int32_t W, int32_t win_y0, int32_t win_x0, int32_t win_h, int32_t win_w,
                      int32_t H_out, int32_t W_out, ess_stream_t stream);

/* ---- Post-processing of an E2VID reconstruction (e2vid/image_reconstructor.py:166-185 PostProcessor; e2vid/utils/inference_utils.py
 * :18-53 make_event_preview, :112-153 IntensityRescaler, :261-279 UnsharpMaskFilter) -- PURELY ADDITIVE to ABI 110.  All three are
 * capture-safe: no allocation, copy or synchronisation; the only workspace is the caller's.
 *
 * The pixel arithmetic is fixed: fp32 multiply, add and IEEE divide, each rounded once, never fused, in this order:
 *   blur = sum_ky sum_kx weights[ky * 5 + kx] * v(y + ky - 2, x + kx - 2)   from 0.f, row-major taps; a tap outside the SOURCE plane
 *                                                                            contributes weights * 0.f (F.conv2d(padding=2))
 *   s    = c1 * v - amount * blur                                            c1 = (float)(1 + amount), rounded by the caller
 *   q    = (255.f * (s - Imin)) / range;   u8 = (uint8)min(max(q, 0), 255)   truncation; a NaN gives 0
 * amount <= 0 skips the stencil (s = v, the reference's `if amount > 0`), and `weights` may then be null.
 * weights: 25 floats in HOST memory, read during the call and passed to the kernel by value (a captured launch keeps its copy).
 *
 * ess_recon_post_frame: img fp32 [N][1][Hs][Ws] (the model's output, possibly at the reflection-padded size); bounds fp32 [N][2] in
 * DEVICE memory = (Imin, Imax - Imin) per sample; the stencil runs over the whole source, only the window (win_y0, win_x0, win_h, win_w)
 * is written: frame_u8 uint8 [N][win_h][win_w] and / or frame_f32 fp32 [N][1][win_h][win_w] = (float)u8 / 255.f (what IntensityRescaler
 * returns); each nullable, not both.  One 4-byte / 16-byte store per 4 pixels when win_w % 4 == 0 and the pointer is aligned so.   */
int ess_recon_post_frame(const float* img, const float* weights, float c1, float amount, const float* bounds, uint8_t* frame_u8,
                         float* frame_f32, int32_t N, int32_t Hs, int32_t Ws, int32_t win_y0, int32_t win_x0, int32_t win_h,
                         int32_t win_w, ess_stream_t stream);

/* The auto-HDR step of IntensityRescaler with its state in device memory, two launches:
 * (a) min / max of s over the WHOLE source plane of each sample (NaN pixels skipped -- fminf / fmaxf; torch.min / max would return
 *     NaN), one partial pair per workgroup: workspace fp32 [N][ESS_RECON_POST_PARTIALS][2], every slot written on every call
 *     (of THIS entry point; the steered one below writes the taken slots only);
 * (b) per sample, in fp64: Imin = clip(min, 0, 0.45), Imax = clip(max, 0.55, 1); the pair is pushed into the sample's history -- ring
 *     fp64 [N][filter_size + 1][2], ring_state int32 [N][2] = (head, count): the reference pops only when the history is LONGER than
 *     filter_size, so it settles at filter_size + 1 entries --; bounds[n] = ((float)median(mins), (float)(median(maxs) - median(mins)))
 *     with np.median's rule (mean of the two middle values for an even count).  ring_state all zero = empty histories.
 * 0 <= filter_size <= ESS_RECON_POST_MAX_FILTER; N <= 65535.  Per-sample histories are this library's extension (N = 1: the reference). */
#define ESS_RECON_POST_PARTIALS 256
#define ESS_RECON_POST_MAX_FILTER 63
int ess_recon_post_bounds(const float* img, const float* weights, float c1, float amount, int32_t N, int32_t Hs, int32_t Ws,
                          float* workspace, size_t workspace_bytes, double* ring, int32_t* ring_state, int32_t filter_size,
                          float* bounds, ess_stream_t stream);

/* The two calls above STEERED per slot of the batch by words in device memory -- what a multi-stream round needs, whose one captured
 * graph serves every mix of advancing, idle and restarting streams.  PURELY ADDITIVE to ABI 110: ess_version() is unchanged, and the
 * unsteered entry points keep their signatures and their kernels.
 *
 * ess_recon_post_bounds_steered: img fp32 [N][1][Hs][Ws] holds N SLOTS; workspace fp32 [N][ESS_RECON_POST_PARTIALS][2] and bounds fp32
 * [N][2] are indexed by slot (bounds[n] is what the frame call reads for slot n); ring fp64 [R][filter_size + 1][2] and ring_state int32
 * [R][2] hold R HISTORY ROWS.  mode int32 [N] and rows int32 [N] lie in device memory; rows == NULL: the row of slot n is n.  Per slot
 * n, with r = rows ? rows[n] : n:
 *   mode[n] == ESS_CARRY_TAKE (1)   ess_recon_post_bounds' step on history row r, expression for expression; the new pair -> bounds[n];
 *   mode[n] == ESS_CARRY_ZERO (2)   the same with head = count = 0 taken in place of the stored state: the restart -- the history is
 *                                   emptied, then takes this frame;
 *   ESS_CARRY_HOLD (0), any other word, or r outside [0, R)
 *                                   the slot is skipped: its min / max workgroups return after reading the words (no image read, no
 *                                   workspace write), its wave of the median pass returns; no ring, state or bounds is touched.
 * So the workspace slots of the TAKEN slots only are written by a call (the unsteered call writes every slot).  Two taken slots that
 * name one row in one call are the caller's error (the row's history is then that of either).  R >= 1; the other limits as above.
 *
 * ess_recon_post_frame_steered: ess_recon_post_frame plus mode int32 [N] in device memory.  A slot whose word is neither TAKE nor
 * ZERO is neither read (image, bounds) nor written: its output rows keep what they held.  Every other slot gets ess_recon_post_frame's
 * bits.                                                                                                                          */
int ess_recon_post_bounds_steered(const float* img, const float* weights, float c1, float amount, int32_t N, int32_t Hs, int32_t Ws,
                                  float* workspace, size_t workspace_bytes, double* ring, int32_t* ring_state, int32_t R,
                                  int32_t filter_size, float* bounds, const int32_t* mode, const int32_t* rows, ess_stream_t stream);
int ess_recon_post_frame_steered(const float* img, const float* weights, float c1, float amount, const float* bounds, uint8_t* frame_u8,
                                 float* frame_f32, int32_t N, int32_t Hs, int32_t Ws, int32_t win_y0, int32_t win_x0, int32_t win_h,
                                 int32_t win_w, const int32_t* mode, ess_stream_t stream);

/* make_event_preview for every sample: s = sum of the last num_bins_to_show planes of grids fp32 [N][C][H][W] in plane order (fp32;
 * num_bins_to_show < 0, 0 or >= C: all planes, as the reference's slice).  ESS_PREVIEW_RED_BLUE: out uint8 [N][H][W][3] in BGR order,
 * blue = 255 where s > 0, red = 255 where s < 0.  ESS_PREVIEW_GRAYSCALE: out uint8 [N][H][W] = (255.f * (s + 10.f)) / 20.f clamped
 * to [0, 255], THEN truncated (the reference casts first and lets values outside the range wrap).                                   */
enum { ESS_PREVIEW_RED_BLUE = 0, ESS_PREVIEW_GRAYSCALE = 1 };
int ess_event_preview(const float* grids, uint8_t* out, int32_t N, int32_t C, int32_t H, int32_t W, int32_t num_bins_to_show,
                      int32_t mode, ess_stream_t stream);

/* ---- Segmentation display (utils/viz_utils.py:19-73 createRGBImage / visualizeHistogram / visualizeVoxelGrid, :105-145
 * create_checkerboard / prepare_semseg; the overlay is this library's own) -- PURELY ADDITIVE to ABI 110 (ess_version() is unchanged; no
 * existing entry point changes).  All three are capture-safe: explicit stream, no allocation, copy or synchronisation, no host state;
 * every argument is checked before the launch.  fp32 arithmetic, each operation rounded once, never fused, sums in ascending channel
 * order from 0.f: a numpy float32 restatement defines the bits.
 *
 * The two TILE WRITERS write sample n as an RGB tile of three planes: element (c, y, x) of sample n goes to
 *   out[ ((tile0 + n) / tiles_per_row) * tile_stride_y + ((tile0 + n) % tiles_per_row) * tile_stride_x
 *        + c * plane_stride + y * row_stride + x ]                                              (all strides in ELEMENTS)
 * A contiguous [N][3][H][W] tensor: plane_stride = H * W, row_stride = W, tiles_per_row = 1, tile_stride_y = 3 * H * W.  A make_grid
 * panel [3][Hg][Wg] with `padding` and xmaps tiles per grid row: out = panel + padding * Wg + padding, plane_stride = Hg * Wg,
 * row_stride = Wg, tiles_per_row = xmaps, tile_stride_y = (H + padding) * Wg, tile_stride_x = W + padding.
 * out_elems: the elements the caller owns from `out` on; a call whose tiles would reach beyond is refused.  16-byte stores are used
 * only where `out`, every stride and W are multiples of 4 elements; single elements otherwise (a panel's row stride is odd in general). */
typedef struct EssVizDst {
  int64_t plane_stride, row_stride, tile_stride_y, tile_stride_x;
  int32_t tile0, tiles_per_row;
} EssVizDst;

/* prepare_semseg: labels uint8 or int64 [N][H][W]; colours fp32 [K][3] ALREADY on the 0..1 scale (the caller applies the reference's
 * "divide by 255 if the maximum exceeds 128").  A pixel whose label is ignore_label shows create_checkerboard's value: with
 * cell = max(min(H, W) / 32, 1), 0.75f where (y / cell + x / cell) is even, else 0.25f, in all three planes.  DEVIATION: a label
 * outside [0, K) that is not ignore_label shows the checkerboard as well (the reference asserts on the host).                    */
enum { ESS_VIZ_LABELS_U8 = 0, ESS_VIZ_LABELS_I64 = 1 };
int ess_viz_semseg(const void* labels, int32_t label_type, const float* colours, float* out, size_t out_elems, const EssVizDst* dst,
                   int32_t N, int32_t K, int32_t H, int32_t W, int32_t ignore_label, ess_stream_t stream);

/* x fp32 [N][C][H][W] -> RGB tiles.  clamp(v) = v < 0 ? 0 : v > 1 ? 1 : v (a NaN stays).
 * ESS_VIZ_HISTOGRAM (C == 2): (clamp(x0), clamp(x1), 0).
 * ESS_VIZ_SEPARATE_POL (C even, >= 4; half = C / 2): pos = sum_{c < half} x[c] * ((float)(c + 1) / (float)half),
 *   neg = sum_{c < half} x[half + c] * (same scale); tile = (clamp(neg), clamp(pos), 0).
 * ESS_VIZ_SIGNED (C > 3; the reference's separate_pol = False branch): s = sum_c x[c]; plane 0 = 255 where s > 0, plane 2 = 255 where
 *   s < 0, else 0; unit != 0 writes 1 in place of 255 (the .clamp(0, 1) the trainers apply to the event row).                  */
enum { ESS_VIZ_HISTOGRAM = 0, ESS_VIZ_SEPARATE_POL = 1, ESS_VIZ_SIGNED = 2 };
int ess_viz_events(const float* x, float* out, size_t out_elems, const EssVizDst* dst, int32_t N, int32_t C, int32_t H, int32_t W,
                   int32_t mode, int32_t unit, ess_stream_t stream);

/* Label colours over a gray frame: labels, gray uint8 [N][H][W]; palette uint8 [K][3], K <= 256; 0 <= alpha <= 1;
 * out uint8 [N][H][W][3] in the palette's channel order (as ess_seg_head's colour): v = (1.0f - alpha) * g + alpha * palette[label][c]
 * (two products, one sum), out = (uint8)min(v + 0.5f, 255.f).  A label >= K shows g in all three channels.                      */
int ess_viz_overlay(const uint8_t* labels, const uint8_t* gray, const uint8_t* palette, uint8_t* out, int32_t N, int32_t K, int32_t H,
                    int32_t W, float alpha, ess_stream_t stream);

/* confusion-matrix accumulation from GIVEN predictions (evaluation/metrics.py:4-24, semseg_compute_confusion): pred_lbl,
 * labels int64 [total]; conf int64 [K][K] accumulated (conf[label][pred]) over labels != ignore_index.          */
int ess_label_confusion(const int64_t* pred_lbl, const int64_t* labels, int64_t* conf, int64_t total, int32_t K,
                        int32_t ignore_index, ess_stream_t stream);

/* ---- tuning switches: process-wide kernel choices that run the same arithmetic ("conv_wide": in the same order, bit-identical
 * results; the norm keys below: in another summation order).  "conv_wide": 0 = the 64 x 256-pixel-tile 3x3 kernel always, 1 = the wide-tile kernel where its round count wins
 * (default; environment ESS_CONV_WIDE), 2 = the wide-tile kernel wherever it applies.  ess_tuning_get also answers the read-only
 * key "device_cus" (the compute-unit count the dispatcher's round model uses: queried from the device, 256 on MI355X).
 * "in_small_threads": 256 | 512 (default; environment ESS_IN_SMALL_THREADS) | 1024 -- threads of the fused single-plane InstanceNorm
 * kernels on planes of at most 5120 pixels; the settings differ in the summation order of the statistics only (fp32 rounding).
 * "norm_split_wgs": the workgroups the split statistics pass of the BF16_C8 norm kernels aims at (default 1024; environment
 * ESS_NORM_SPLIT_WGS).  The slices a plane is summed in follow from it and from N * ceil(C/8): the statistics of ONE sample depend, in
 * the summation order of their fp64 partial sums, on the batch size it came in.  ESS_NORM_SPLIT_BY_PLANE lets the plane size alone
 * decide -- for a caller whose per-sample results must not depend on the batch size in the last bit (multi-stream serving against a
 * B = 1 check); a value <= 0 returns to the process's own setting (the environment variable, else 1024).  Unlike "conv_wide", the
 * last two keys DO change results in the last bits: same sums, another order.  */
#define ESS_NORM_SPLIT_BY_PLANE (1 << 30)
int ess_tuning_set(const char* key, int32_t value);
int ess_tuning_get(const char* key, int32_t* value);

#ifdef __cplusplus
}
#endif
#endif /* ESS_HIP_H */
