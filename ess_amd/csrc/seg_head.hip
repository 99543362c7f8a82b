// Fused class head of the semantic decoder at inference: the 1x1 convolution to K class scores (decoder_scale_5 of SemSegE2VID,
// models/style_networks.py:66,87), the nearest resize of the scores to the output size (training/ess_trainer.py:484) and the argmax
// over classes (:485) in ONE pass that never writes the scores: per output pixel one read of the C-channel activation vector, one
// label byte (+ 3 colour bytes, + the winning class's softmax probability) out.
//
// An HBM-bound map.  One lane per output pixel; a C8 source gives the lane one 16-byte vector per 8 channels, the fp32 NCHW source one
// coalesced dword per channel.  The K x C weights are rounded to the operand type of the source and laid out in LDS once per
// workgroup, rows k >= K zero with bias -inf: every lane reads the same LDS address (broadcast), the scores live in KM registers and
// the padded classes can neither win the argmax nor add to the softmax sum, so the inner loops carry no predicate.  fp32 accumulation.
#include "common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct SegHeadArgs {
  const void* x;
  const float* w;
  const float* b;
  const uint8_t* palette;
  uint8_t* labels;
  uint8_t* colour;
  float* conf;
  int N, C, K, Hs, Ws, y0, x0, h, w_, Ho, Wo;
};

template <int FMT>
__device__ __forceinline__ float round_operand(float v) {
  if constexpr (FMT == ESS_FMT_BF16_C8) return (float)(__bf16)v;
  else if constexpr (FMT == ESS_FMT_F16_C8) {  // (saturating at +-65504, NaN kept: the weight packs' half conversion)
    const float c = __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);
    return (float)(_Float16)(v != v ? v : c);
  } else return v;
}

constexpr int SH_PALETTE_BYTES = 64 * 3;

// exp(x) for x <= 0 on the hardware exp2 unit (v_exp_f32, 1 ulp) with the rounding error of x log2(e) carried as a first-order
// correction (t + e = x log2(e) to ~2^-48 relative; 2^(t + e) = 2^t (1 + e ln 2)): ~1.5 ulp, branch-free.  x is clamped at -87.3
// (2^-126, the smallest normal): the probability is an output, so no fast-math exponential here.
__device__ __forceinline__ float exp_nonpos(float x) {
  x = fmaxf(x, -87.3f);
  const float L2E_HI = 1.44269502e+0f, L2E_LO = 1.92596299e-8f;
  const float t = x * L2E_HI;
  const float e = fmaf(x, L2E_HI, -t) + x * L2E_LO;
  const float p = __builtin_amdgcn_exp2f(t);
  return fmaf(p, e * 0.693147181f, p);
}

// The weights, bias and palette of a workgroup in LDS: [CB][KM][8] weights, [KM] bias, [K][3] palette bytes (lds_of(K, C) bytes).
template <int FMT, int KM>
__device__ __forceinline__ void seg_head_stage(const SegHeadArgs& a, float* lds) {
  const int CB = (a.C + 7) >> 3, CP = CB * 8;
  float* lw = lds;
  float* lb = lds + KM * CP;
  uint8_t* lp = (uint8_t*)(lb + KM);
  for (int i = threadIdx.x; i < KM * CP; i += blockDim.x) {
    const int cb = i / (KM * 8), k = (i >> 3) % KM, c = cb * 8 + (i & 7);  // [CB][KM][8]: a class's offset inside a block is a constant
    lw[i] = (k < a.K && c < a.C) ? round_operand<FMT>(a.w[k * a.C + c]) : 0.f;  // (c >= C: the layout's tail channels, masked here)
  }
  for (int i = threadIdx.x; i < KM; i += blockDim.x) lb[i] = i < a.K ? a.b[i] : -INFINITY;
  if (a.palette)
    for (int i = threadIdx.x; i < a.K * 3; i += blockDim.x) lp[i] = a.palette[i];
}

// One output pixel (sample n, row oy, column ox; i its index in the outputs): the label, colour and confidence stores, and the label
// back to the caller.  The ONE per-pixel code path of the class head: ess_seg_head and ess_seg_head_eval both run it.
template <int FMT, int KM>
__device__ __forceinline__ int seg_head_pixel(const SegHeadArgs& a, const float* lds, float sy, float sx, size_t plane, size_t n,
                                              int oy, int ox, size_t i) {
  const int CB = (a.C + 7) >> 3, CP = CB * 8;
  const float* lw = lds;
  const float* lb = lds + KM * CP;
  const uint8_t* lp = (const uint8_t*)(lb + KM);
  const int iy = a.y0 + min((int)floorf(oy * sy), a.h - 1), ix = a.x0 + min((int)floorf(ox * sx), a.w_ - 1);
  const size_t px = (size_t)iy * a.Ws + ix;
  float z[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) z[k] = lb[k];
  for (int cb = 0; cb < CB; ++cb) {
    float v[8];
    if constexpr (FMT == ESS_FMT_F32_NCHW) {
      const float* xp = (const float*)a.x + (n * a.C + (size_t)cb * 8) * plane + px;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (cb * 8 + j < a.C) ? xp[(size_t)j * plane] : 0.f;  // (never past the last channel plane)
    } else {
      const uint4 q = ((const uint4*)a.x)[(n * CB + cb) * plane + px];
      if constexpr (FMT == ESS_FMT_BF16_C8) {
        const bf16x8 t = __builtin_bit_cast(bf16x8, q);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
      } else {
        const f16x8 t = __builtin_bit_cast(f16x8, q);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
      }
    }
    const float* wr = lw + cb * (KM * 8);
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const f32x4 w0 = *(const f32x4*)(wr + k * 8), w1 = *(const f32x4*)(wr + k * 8 + 4);
      float s = z[k];
      s = fmaf(w0[0], v[0], s);
      s = fmaf(w0[1], v[1], s);
      s = fmaf(w0[2], v[2], s);
      s = fmaf(w0[3], v[3], s);
      s = fmaf(w1[0], v[4], s);
      s = fmaf(w1[1], v[5], s);
      s = fmaf(w1[2], v[6], s);
      s = fmaf(w1[3], v[7], s);
      z[k] = s;
    }
  }
  float best = z[0];
  int bi = 0;
#pragma unroll
  for (int k = 1; k < KM; ++k)
    if (z[k] > best) { best = z[k]; bi = k; }  // first maximum wins, as argmax_conf_kernel / torch.argmax
  a.labels[i] = (uint8_t)bi;
  if (a.colour) {
    uint8_t* cp = a.colour + i * 3;
    cp[0] = lp[bi * 3];
    cp[1] = lp[bi * 3 + 1];
    cp[2] = lp[bi * 3 + 2];
  }
  if (a.conf) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) s += exp_nonpos(z[k] - best);  // (padded classes: 2^-126 each, absorbed by a sum >= 1)
    a.conf[i] = 1.0f / s;
  }
  return bi;
}

template <int FMT, int KM>
__global__ __launch_bounds__(256) void seg_head_kernel(const SegHeadArgs a) {
  extern __shared__ float lds[];
  seg_head_stage<FMT, KM>(a, lds);
  __syncthreads();

  // source pixel of an output pixel: resize_nearest_kernel's rule (pointwise.hip) inside the window
  const float sy = (float)a.h / (float)a.Ho, sx = (float)a.w_ / (float)a.Wo;
  const size_t plane = (size_t)a.Hs * a.Ws;
  const size_t total = (size_t)a.N * a.Ho * a.Wo;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % a.Wo);
    const size_t r = i / a.Wo;
    const int oy = (int)(r % a.Ho);
    const size_t n = r / a.Ho;
    seg_head_pixel<FMT, KM>(a, lds, sy, sx, plane, n, oy, ox, i);
  }
}

// The class head that scores itself: seg_head_kernel's pixels, plus confusion[n, gt, label] += 1 over the pixels whose ground truth
// is neither ignore_index nor >= K (ess_label_confusion's rule).  blockIdx.y is the sample, so a workgroup's K x K LDS histogram
// belongs to one row of `confusion`; it leaves as one 64-bit atomic per non-zero cell (integer sums: order-independent).
template <int FMT, int KM>
__global__ __launch_bounds__(256) void seg_head_eval_kernel(const SegHeadArgs a, const uint8_t* __restrict__ gt,
                                                            unsigned long long* confusion, int ignore, int hist_off) {
  extern __shared__ float lds[];  // seg_head_stage's lds_of(K, C) bytes, then [K][K] counts
  unsigned int* hist = (unsigned int*)lds + hist_off;
  seg_head_stage<FMT, KM>(a, lds);
  for (int i = threadIdx.x; i < a.K * a.K; i += blockDim.x) hist[i] = 0;
  __syncthreads();

  const float sy = (float)a.h / (float)a.Ho, sx = (float)a.w_ / (float)a.Wo;
  const size_t plane = (size_t)a.Hs * a.Ws;
  const size_t n = blockIdx.y, hw = (size_t)a.Ho * a.Wo;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(p % a.Wo), oy = (int)(p / a.Wo);
    const size_t i = n * hw + p;
    const int bi = seg_head_pixel<FMT, KM>(a, lds, sy, sx, plane, n, oy, ox, i);
    const int g = gt[i];
    if (g != ignore && g < a.K) atomicAdd(&hist[g * a.K + bi], 1u);  // (bi < K: the padded classes cannot win)
  }
  __syncthreads();
  unsigned long long* row = confusion + n * (size_t)(a.K * a.K);
  for (int i = threadIdx.x; i < a.K * a.K; i += blockDim.x)
    if (hist[i]) atomicAdd(row + i, (unsigned long long)hist[i]);
}

inline unsigned wave_uniform_grid(size_t total, int cap) {
  // blocks of 256 threads such that grid*256 divides the work into equal trip counts where possible (as loss.hip)
  size_t g = (total + 255) / 256;
  if (g > (size_t)cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

inline int km_of(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : K <= 12 ? 12 : K <= 16 ? 16 : K <= 20 ? 20 : K <= 32 ? 32 : 64; }
inline size_t lds_of(int K, int C) { return (size_t)km_of(K) * (((C + 7) >> 3) * 8) * 4 + (size_t)km_of(K) * 4 + SH_PALETTE_BYTES; }

template <int FMT>
int launch(const SegHeadArgs& a, hipStream_t st) {
  const size_t total = (size_t)a.N * a.Ho * a.Wo;
  const unsigned grid = wave_uniform_grid(total, 2048);
  const size_t lds = lds_of(a.K, a.C);
#define ESS_SH(KM_) hipLaunchKernelGGL((seg_head_kernel<FMT, KM_>), dim3(grid), dim3(256), lds, st, a)
  switch (km_of(a.K)) {
    case 4: ESS_SH(4); break;
    case 8: ESS_SH(8); break;
    case 12: ESS_SH(12); break;
    case 16: ESS_SH(16); break;
    case 20: ESS_SH(20); break;
    case 32: ESS_SH(32); break;
    default: ESS_SH(64); break;
  }
#undef ESS_SH
  return ess_launch_status("seg_head");
}

// one grid row per sample; the columns share seg_head's cap of 2048 workgroups among the samples
template <int FMT>
int launch_eval(const SegHeadArgs& a, const uint8_t* gt, int64_t* confusion, int ignore, hipStream_t st) {
  const int cap = 2048 / a.N;
  const unsigned gx = wave_uniform_grid((size_t)a.Ho * a.Wo, cap < 1 ? 1 : cap);
  const size_t head = lds_of(a.K, a.C), lds = head + (size_t)a.K * a.K * 4;
#define ESS_SH(KM_)                                                                                                             \
  hipLaunchKernelGGL((seg_head_eval_kernel<FMT, KM_>), dim3(gx, a.N), dim3(256), lds, st, a, gt, (unsigned long long*)confusion, \
                     ignore, (int)(head / 4))
  switch (km_of(a.K)) {
    case 4: ESS_SH(4); break;
    case 8: ESS_SH(8); break;
    case 12: ESS_SH(12); break;
    case 16: ESS_SH(16); break;
    case 20: ESS_SH(20); break;
    case 32: ESS_SH(32); break;
    default: ESS_SH(64); break;
  }
#undef ESS_SH
  return ess_launch_status("seg_head_eval");
}

// the argument checks of both entry points
int check_args(const char* who, const void* x, int32_t fmt, const float* weight, const float* bias, const uint8_t* palette,
               const uint8_t* labels, const uint8_t* colour, int32_t N, int32_t C, int32_t K, int32_t H, int32_t W, int32_t win_y0,
               int32_t win_x0, int32_t win_h, int32_t win_w, int32_t H_out, int32_t W_out, size_t extra_lds) {
  ESS_CHECK_ARG(x && weight && bias && labels, "%s: x, weight, bias and labels are required", who);
  ESS_CHECK_ARG(fmt == ESS_FMT_F32_NCHW || fmt == ESS_FMT_BF16_C8 || fmt == ESS_FMT_F16_C8, "%s: source format %d unsupported", who, fmt);
  ESS_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && H_out > 0 && W_out > 0, "%s: bad extents N=%d C=%d H=%d W=%d H_out=%d W_out=%d", who, N,
                C, H, W, H_out, W_out);
  ESS_CHECK_ARG(K > 0 && K <= 64, "%s: K=%d unsupported (1..64)", who, K);
  ESS_CHECK_ARG(C <= 4096 && lds_of(K, C) + extra_lds <= 64 * 1024, "%s: K=%d x C=%d weights%s do not fit 64 KiB of LDS", who, K, C,
                extra_lds ? " and the K x K counts" : "");
  ESS_CHECK_ARG(win_y0 >= 0 && win_x0 >= 0 && win_h > 0 && win_w > 0 && (int64_t)win_y0 + win_h <= H && (int64_t)win_x0 + win_w <= W,
                "%s: window (%d, %d, %d, %d) leaves the %d x %d plane", who, win_y0, win_x0, win_h, win_w, H, W);
  ESS_CHECK_ARG(!colour || palette, "%s: colour needs a palette", who);
  ESS_CHECK_ARG(fmt == ESS_FMT_F32_NCHW || ((uintptr_t)x & 15) == 0, "%s: a C8 source must be 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" int ess_seg_head(const void* x, int32_t fmt, const float* weight, const float* bias, const uint8_t* palette, uint8_t* labels,
                            uint8_t* colour, float* confidence, int32_t N, int32_t C, int32_t K, int32_t H, int32_t W, int32_t win_y0,
                            int32_t win_x0, int32_t win_h, int32_t win_w, int32_t H_out, int32_t W_out, ess_stream_t stream) {
  if (int rc = check_args("seg_head", x, fmt, weight, bias, palette, labels, colour, N, C, K, H, W, win_y0, win_x0, win_h, win_w, H_out,
                          W_out, 0))
    return rc;
  SegHeadArgs a{x, weight, bias, palette, labels, colour, confidence, N, C, K, H, W, win_y0, win_x0, win_h, win_w, H_out, W_out};
  hipStream_t st = (hipStream_t)stream;
  if (fmt == ESS_FMT_BF16_C8) return launch<ESS_FMT_BF16_C8>(a, st);
  if (fmt == ESS_FMT_F16_C8) return launch<ESS_FMT_F16_C8>(a, st);
  return launch<ESS_FMT_F32_NCHW>(a, st);
}

extern "C" int ess_seg_head_eval(const void* x, int32_t fmt, const float* weight, const float* bias, const uint8_t* palette,
                                 uint8_t* labels, uint8_t* colour, float* confidence, const uint8_t* gt, int64_t* confusion,
                                 int32_t ignore_index, int32_t N, int32_t C, int32_t K, int32_t H, int32_t W, int32_t win_y0,
                                 int32_t win_x0, int32_t win_h, int32_t win_w, int32_t H_out, int32_t W_out, ess_stream_t stream) {
  ESS_CHECK_ARG(gt || !confusion, "seg_head_eval: confusion needs gt");
  ESS_CHECK_ARG(confusion || !gt, "seg_head_eval: gt needs confusion");
  if (int rc = check_args("seg_head_eval", x, fmt, weight, bias, palette, labels, colour, N, C, K, H, W, win_y0, win_x0, win_h, win_w,
                          H_out, W_out, K > 0 && K <= 64 ? (size_t)K * K * 4 : 0))
    return rc;
  ESS_CHECK_ARG(N <= 65535, "seg_head_eval: N=%d samples exceed the grid's 65535 rows", N);
  SegHeadArgs a{x, weight, bias, palette, labels, colour, confidence, N, C, K, H, W, win_y0, win_x0, win_h, win_w, H_out, W_out};
  hipStream_t st = (hipStream_t)stream;
  if (fmt == ESS_FMT_BF16_C8) return launch_eval<ESS_FMT_BF16_C8>(a, gt, confusion, ignore_index, st);
  if (fmt == ESS_FMT_F16_C8) return launch_eval<ESS_FMT_F16_C8>(a, gt, confusion, ignore_index, st);
  return launch_eval<ESS_FMT_F32_NCHW>(a, gt, confusion, ignore_index, st);
}
