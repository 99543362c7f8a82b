// Image ingest for the device image store (datasets/image_store.py): one decoded source frame -> its uint8 store slot, in the
// integer arithmetic of the library the reference's loader calls (datasets/cityscapes_loader.py:26-29, 86-96: transforms.Grayscale,
// transforms.Resize on a PIL image = PIL's antialiased bilinear resize, label.resize(NEAREST), the `standardization` stretch):
//   gray        L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
//   resize      two passes with an 8-bit intermediate, horizontal first; per output index a window (first, count) of the input and
//               `count` 22-bit fixed-point coefficients k, the pixel = clip8((2^21 + sum k_i p_i) >> 22)
//   label       a gather through one index table per axis
//   stretch     v -> (uint8) trunc(255.0 * (v - min) / (max - min)) in IEEE fp64, through a 256-entry table per image
// The coefficient and index tables are built on the HOST in float64 (pil_bilinear_tables, pil_nearest_table): no float is
// evaluated here that could disagree with PIL; the kernels multiply and add int32.  Launches of one frame:
//   image_hpass_kernel   gray + horizontal pass, the source row segment of a workgroup converted ONCE into LDS: the 6 MB frame is
//                        read once, its 9-tap windows (overlapping byte loads) are served from LDS      -> scratch [H][Wr]
//   image_vpass_kernel   vertical pass (+ min / max of the frame: wave reduction, one atomic pair a wave) -> slot [Hr][Wr]
//   image_stretch_kernel only with standardisation, in place
//   image_label_kernel   the label's gather
#include "common.h"

namespace {

constexpr int HP_THREADS = 256;
constexpr int HP_SPAN = HP_THREADS * (ESS_IMAGE_MAX_TAPS / 2) + 64;  // source pixels one workgroup's windows can span (scale <= MAX_TAPS / 2)
constexpr int PRECISION_BITS = 22;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// tab: int32 [2 + ksize][n_out] -- plane 0: first input index, plane 1: count, planes 2..: the coefficients (lanes read neighbours)
template <int CH>
__global__ __launch_bounds__(HP_THREADS) void image_hpass_kernel(const uint8_t* __restrict__ frame, const int32_t* __restrict__ tab,
                                                                 uint8_t* __restrict__ out, int H, int W, int Wr, int taps) {
  __shared__ uint8_t row[HP_SPAN];
  const int y = blockIdx.y;
  const int x0 = blockIdx.x * HP_THREADS, xo = x0 + threadIdx.x;
  const int x_last = min(x0 + HP_THREADS, Wr) - 1;
  int lo, hi;  // the source pixels [lo, hi) of this workgroup's windows
  if (tab) {
    lo = tab[x0];
    hi = tab[x_last] + tab[Wr + x_last];
  } else {
    lo = x0;
    hi = x_last + 1;
  }
  lo = max(lo, 0);
  hi = min(min(hi, W), lo + HP_SPAN);
  const uint8_t* src = frame + (size_t)y * W * CH;
  for (int j = lo + threadIdx.x; j < hi; j += HP_THREADS) {
    int v;
    if constexpr (CH == 3) {
      const uint8_t* p = src + (size_t)j * 3;
      v = ((int)p[0] * 19595 + (int)p[1] * 38470 + (int)p[2] * 7471 + 0x8000) >> 16;
    } else {
      v = src[j];
    }
    row[j - lo] = (uint8_t)v;
  }
  __syncthreads();
  if (xo >= Wr) return;
  int v;
  if (tab) {
    const int first = tab[xo], count = min(tab[Wr + xo], taps);  // (a count beyond the table's planes is not followed)
    int ss = 1 << (PRECISION_BITS - 1);
    for (int i = 0; i < count; ++i) {
      const int j = first + i - lo;
      if (j >= 0 && j < hi - lo) ss += tab[(size_t)(2 + i) * Wr + xo] * (int)row[j];
    }
    v = clip8(ss >> PRECISION_BITS);
  } else {
    v = row[xo - lo];
  }
  out[(size_t)y * Wr + xo] = (uint8_t)v;
}

// tab: int32 [2 + ksize][Hr] (one output row reads one column of it: uniform over the workgroup)
template <bool MINMAX>
__global__ __launch_bounds__(256) void image_vpass_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ tab,
                                                          uint8_t* __restrict__ out, int32_t* __restrict__ minmax, int H, int Hr, int Wr, int taps) {
  const int yo = blockIdx.y;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  int v = 0;
  const bool live = x < Wr;
  if (live) {
    if (tab) {
      const int first = tab[yo], count = min(tab[Hr + yo], taps);
      int ss = 1 << (PRECISION_BITS - 1);
      for (int i = 0; i < count; ++i) {
        const int yy = first + i;
        if (yy >= 0 && yy < H) ss += tab[(size_t)(2 + i) * Hr + yo] * (int)src[(size_t)yy * Wr + x];
      }
      v = clip8(ss >> PRECISION_BITS);
    } else {
      v = src[(size_t)yo * Wr + x];
    }
    out[(size_t)yo * Wr + x] = (uint8_t)v;
  }
  if constexpr (MINMAX) {
    int lo = live ? v : 255, hi = live ? v : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(minmax, lo);
      atomicMax(minmax + 1, hi);
    }
  }
}

__global__ void image_minmax_init_kernel(int32_t* __restrict__ minmax) {
  minmax[0] = 255;
  minmax[1] = 0;
}

// cityscapes_loader.py:92-96 on a uint8 frame: 255.0 * (v - min) is exact in fp64, the quotient is one IEEE division; a constant
// frame (the reference divides by zero) becomes all 0
__global__ __launch_bounds__(256) void image_stretch_kernel(uint8_t* __restrict__ img, const int32_t* __restrict__ minmax, int64_t total) {
#pragma clang fp contract(off)
  __shared__ uint8_t lut[256];
  const int mn = minmax[0], mx = minmax[1];
  {
    const int v = threadIdx.x;
    int r = 0;
    if (mx > mn && v >= mn && v <= mx) {
      const double num = 255.0 * (double)(v - mn);
      const double q = num / (double)(mx - mn);
      r = (int)q;
    }
    lut[v] = (uint8_t)clip8(r);
  }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) img[i] = lut[img[i]];
}

__global__ __launch_bounds__(256) void image_label_kernel(const uint8_t* __restrict__ lab, const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ cols, uint8_t* __restrict__ out, int H, int W,
                                                          int Hr, int Wr) {
  const int yo = blockIdx.y;
  const int xo = blockIdx.x * blockDim.x + threadIdx.x;
  if (xo >= Wr) return;
  const int ys = rows[yo], xs = cols[xo];
  out[(size_t)yo * Wr + xo] = (ys >= 0 && ys < H && xs >= 0 && xs < W) ? lab[(size_t)ys * W + xs] : (uint8_t)0;
}

}  // namespace

extern "C" int ess_image_ingest(const uint8_t* frame, int32_t channels, int32_t H, int32_t W, const int32_t* h_table, int32_t h_taps,
                                const int32_t* v_table, int32_t v_taps, uint8_t* scratch, uint8_t* out, int32_t Hr, int32_t Wr,
                                int32_t standardize, int32_t* minmax, const uint8_t* label, const int32_t* label_rows,
                                const int32_t* label_cols, uint8_t* out_label, ess_stream_t stream) {
  const char* me = "image_ingest";
  ESS_CHECK_ARG(frame && out, "%s: null frame or out", me);
  ESS_CHECK_ARG(channels == 1 || channels == 3, "%s: channels=%d must be 1 (gray) or 3 (RGB)", me, channels);
  ESS_CHECK_ARG(H >= 1 && W >= 1 && Hr >= 1 && Wr >= 1 && H <= ESS_IMAGE_MAX_SIDE && W <= ESS_IMAGE_MAX_SIDE && Hr <= ESS_IMAGE_MAX_SIDE &&
                    Wr <= ESS_IMAGE_MAX_SIDE,
                "%s: source %d x %d, slot %d x %d: every side must lie in [1, %d]", me, H, W, Hr, Wr, ESS_IMAGE_MAX_SIDE);
  ESS_CHECK_ARG((h_table != nullptr) == (W != Wr), "%s: h_table is given exactly where the width changes (%d -> %d): an unchanged pass is skipped", me, W, Wr);
  ESS_CHECK_ARG((v_table != nullptr) == (H != Hr), "%s: v_table is given exactly where the height changes (%d -> %d): an unchanged pass is skipped", me, H, Hr);
  ESS_CHECK_ARG(!h_table || (h_taps >= 1 && h_taps <= ESS_IMAGE_MAX_TAPS), "%s: h_taps=%d must lie in [1, %d]", me, h_taps, ESS_IMAGE_MAX_TAPS);
  ESS_CHECK_ARG(!v_table || (v_taps >= 1 && v_taps <= ESS_IMAGE_MAX_TAPS), "%s: v_taps=%d must lie in [1, %d]", me, v_taps, ESS_IMAGE_MAX_TAPS);
  const bool hpass = channels == 3 || h_table != nullptr;
  ESS_CHECK_ARG(!hpass || scratch, "%s: null scratch: the gray / horizontal pass writes uint8 [H][Wr] there", me);
  ESS_CHECK_ARG(scratch != out && (const uint8_t*)scratch != frame && frame != out, "%s: frame, scratch and out must be distinct buffers", me);
  ESS_CHECK_ARG(!standardize || minmax, "%s: standardize needs minmax (2 int32 words on the device)", me);
  ESS_CHECK_ARG(((uintptr_t)h_table | (uintptr_t)v_table | (uintptr_t)minmax | (uintptr_t)label_rows | (uintptr_t)label_cols) % 4 == 0,
                "%s: the tables and minmax must be 4-byte aligned", me);
  ESS_CHECK_ARG((label != nullptr) == (out_label != nullptr), "%s: label and out_label come together", me);
  ESS_CHECK_ARG(!label || (label_rows && label_cols), "%s: a label needs label_rows [Hr] and label_cols [Wr]", me);
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* vsrc = frame;
  if (hpass) {
    const dim3 grid((unsigned)ceil_div(Wr, HP_THREADS), (unsigned)H);
    if (channels == 3)
      hipLaunchKernelGGL(image_hpass_kernel<3>, grid, dim3(HP_THREADS), 0, s, frame, h_table, scratch, H, W, Wr, h_taps);
    else
      hipLaunchKernelGGL(image_hpass_kernel<1>, grid, dim3(HP_THREADS), 0, s, frame, h_table, scratch, H, W, Wr, h_taps);
    vsrc = scratch;
  }
  const dim3 vgrid((unsigned)ceil_div(Wr, 256), (unsigned)Hr);
  if (minmax) {
    hipLaunchKernelGGL(image_minmax_init_kernel, dim3(1), dim3(1), 0, s, minmax);
    hipLaunchKernelGGL(image_vpass_kernel<true>, vgrid, dim3(256), 0, s, vsrc, v_table, out, minmax, H, Hr, Wr, v_taps);
  } else {
    hipLaunchKernelGGL(image_vpass_kernel<false>, vgrid, dim3(256), 0, s, vsrc, v_table, out, minmax, H, Hr, Wr, v_taps);
  }
  if (standardize) {
    const int64_t total = (int64_t)Hr * Wr;
    int64_t blocks = ceil_div64(total, 256 * 4);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(image_stretch_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, (const int32_t*)minmax, total);
  }
  if (label)
    hipLaunchKernelGGL(image_label_kernel, vgrid, dim3(256), 0, s, label, label_rows, label_cols, out_label, H, W, Hr, Wr);
  return ess_launch_status(me);
}
