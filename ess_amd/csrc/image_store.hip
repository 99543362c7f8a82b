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
// and of one PAIRED frame of an event loader (ess_image_ingest_frame; bicubic tables, RGB resized before the gray conversion):
//   frame_hpass_kernel        the horizontal pass on one or on three channels, only the rows a kept output row reads -> scratch
//   frame_vpass_gray_kernel   the vertical pass per channel + the gray conversion (one channel: image_vpass_kernel) -> the slot's rows
// A batch reads the slots through image_gather_unit_kernel (ess_image_gather_unit): slot / 255 in fp32.
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

// ---- paired camera frames (ess_image_ingest_frame): the event loaders' Image.resize -- PIL's default filter there is BICUBIC, whose
// tables hold NEGATIVE coefficients -- applied to the RGB image, transforms.Grayscale() behind it.  The arithmetic is the one above;
// what is new: a sum can be negative (ss >> 22 is an arithmetic shift of an int, clip8 cuts on both sides), three channels share a
// window's coefficients, and the gray conversion runs at the end of the vertical pass.  The sums stay int32: 2^21 + sum |k| 255 < 2^31
// needs sum |w| < 2 over a window, and the normalised bicubic weights (a = -0.5) stay below 1.3 (the host builder checks its tables).

__device__ __forceinline__ int gray_of(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// The source rows the kept output rows [0, out_rows) read: the windows' first indices never decrease, so the last kept row's ends them.
__device__ __forceinline__ int rows_read(const int32_t* __restrict__ vtab, int H, int Hr, int out_rows) {
  return vtab ? min(max(vtab[out_rows - 1], 0) + max(vtab[Hr + out_rows - 1], 0), H) : out_rows;
}

// The horizontal pass of a frame: CH_IN source channels -> CH_OUT channels of scratch [H][Wr][CH_OUT].  (1, 1) gray, (3, 1) gray FIRST
// (image_hpass_kernel's arithmetic), (3, 3) every channel on its own.  The source row segment is staged once in LDS, CH_OUT bytes a
// pixel (the RGB form keeps the frame's interleaved bytes: HP_SPAN pixels are 3 HP_SPAN bytes).  A row no kept output row reads returns.
template <int CH_IN, int CH_OUT>
__global__ __launch_bounds__(HP_THREADS) void frame_hpass_kernel(const uint8_t* __restrict__ frame, const int32_t* __restrict__ tab,
                                                                 const int32_t* __restrict__ vtab, uint8_t* __restrict__ out, int H, int W,
                                                                 int Wr, int taps, int Hr, int out_rows) {
  __shared__ uint8_t row[HP_SPAN * CH_OUT];
  const int y = blockIdx.y;
  if (y >= rows_read(vtab, H, Hr, out_rows)) return;  // (uniform over the workgroup)
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
  lo = min(max(lo, 0), W);
  hi = min(min(hi, W), lo + HP_SPAN);
  const uint8_t* src = frame + (size_t)y * W * CH_IN;
  if constexpr (CH_IN == CH_OUT) {
    const uint8_t* seg = src + (size_t)lo * CH_IN;
    for (int j = threadIdx.x; j < (hi - lo) * CH_IN; j += HP_THREADS) row[j] = seg[j];
  } else {
    for (int j = lo + threadIdx.x; j < hi; j += HP_THREADS) {
      const uint8_t* p = src + (size_t)j * 3;
      row[j - lo] = (uint8_t)gray_of(p[0], p[1], p[2]);
    }
  }
  __syncthreads();
  if (xo >= Wr) return;
  int v[CH_OUT];
  if (tab) {
    const int first = tab[xo], count = min(tab[Wr + xo], taps);  // (a count beyond the table's planes is not followed)
    int ss[CH_OUT];
#pragma unroll
    for (int c = 0; c < CH_OUT; ++c) ss[c] = 1 << (PRECISION_BITS - 1);
    for (int i = 0; i < count; ++i) {
      const int j = first + i - lo;
      if (j >= 0 && j < hi - lo) {
        const int k = tab[(size_t)(2 + i) * Wr + xo];
#pragma unroll
        for (int c = 0; c < CH_OUT; ++c) ss[c] += k * (int)row[j * CH_OUT + c];
      }
    }
#pragma unroll
    for (int c = 0; c < CH_OUT; ++c) v[c] = clip8(ss[c] >> PRECISION_BITS);
  } else {
#pragma unroll
    for (int c = 0; c < CH_OUT; ++c) v[c] = xo < hi ? row[(xo - lo) * CH_OUT + c] : 0;
  }
  uint8_t* dst = out + ((size_t)y * Wr + xo) * CH_OUT;
#pragma unroll
  for (int c = 0; c < CH_OUT; ++c) dst[c] = (uint8_t)v[c];
}

// The vertical pass of an RGB frame, gray LAST: src uint8 [H][Wr][3] (the horizontal pass's scratch, or the frame where the width
// stays) -> out uint8 [out_rows][Wr].  Each channel ends as an 8-bit value before the conversion, as PIL's resized RGB image holds it;
// no RGB image of the output size is written.  tab NULL: the height stays, the conversion alone.
__global__ __launch_bounds__(256) void frame_vpass_gray_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ tab,
                                                               uint8_t* __restrict__ out, int H, int Hr, int Wr, int taps) {
  const int yo = blockIdx.y;
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= Wr) return;
  int r, g, b;
  if (tab) {
    const int first = tab[yo], count = min(tab[Hr + yo], taps);
    int sr = 1 << (PRECISION_BITS - 1), sg = sr, sb = sr;
    for (int i = 0; i < count; ++i) {
      const int yy = first + i;
      if (yy >= 0 && yy < H) {
        const int k = tab[(size_t)(2 + i) * Hr + yo];
        const uint8_t* p = src + ((size_t)yy * Wr + x) * 3;
        sr += k * (int)p[0];
        sg += k * (int)p[1];
        sb += k * (int)p[2];
      }
    }
    r = clip8(sr >> PRECISION_BITS);
    g = clip8(sg >> PRECISION_BITS);
    b = clip8(sb >> PRECISION_BITS);
  } else {
    const uint8_t* p = src + ((size_t)yo * Wr + x) * 3;
    r = p[0];
    g = p[1];
    b = p[2];
  }
  out[(size_t)yo * Wr + x] = (uint8_t)gray_of(r, g, b);
}

// transforms.ToTensor() on the stored slots: out[b][0] = images[index[b]] / 255 in fp32 -- one IEEE division per byte VALUE, 256 of
// them a workgroup, kept in LDS (the bits of torch's .float().div(255) on the host; no reciprocal).  A slot number outside
// [0, capacity) gives an all-zero frame.  grid (chunks, B).
template <typename INDEX>
__global__ __launch_bounds__(256) void image_gather_unit_kernel(const uint8_t* __restrict__ images, const INDEX* __restrict__ index,
                                                                float* __restrict__ out, int64_t capacity, int64_t hw) {
#pragma clang fp contract(off)
  __shared__ float unit[256];
  unit[threadIdx.x] = (float)(int)threadIdx.x / 255.0f;
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t slot = (int64_t)index[b];
  const bool live = slot >= 0 && slot < capacity;
  const uint8_t* src = images + (live ? slot : 0) * hw;
  float* dst = out + (int64_t)b * hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = live ? unit[src[i]] : 0.0f;
}

}  // namespace

extern "C" int ess_image_ingest_frame(const uint8_t* frame, int32_t channels, int32_t H, int32_t W, const int32_t* h_table, int32_t h_taps,
                                      const int32_t* v_table, int32_t v_taps, uint8_t* scratch, uint8_t* out, int32_t Hr, int32_t Wr,
                                      int32_t out_rows, int32_t gray_last, ess_stream_t stream) {
  const char* me = "image_ingest_frame";
  ESS_CHECK_ARG(frame && out, "%s: null frame or out", me);
  ESS_CHECK_ARG(channels == 1 || channels == 3, "%s: channels=%d must be 1 (gray) or 3 (RGB)", me, channels);
  ESS_CHECK_ARG(gray_last == 0 || gray_last == 1, "%s: gray_last=%d must be 0 (gray, then resize) or 1 (resize the RGB image, then gray)", me, gray_last);
  ESS_CHECK_ARG(H >= 1 && W >= 1 && Hr >= 1 && Wr >= 1 && H <= ESS_IMAGE_MAX_SIDE && W <= ESS_IMAGE_MAX_SIDE && Hr <= ESS_IMAGE_MAX_SIDE &&
                    Wr <= ESS_IMAGE_MAX_SIDE,
                "%s: source %d x %d, resized %d x %d: every side must lie in [1, %d]", me, H, W, Hr, Wr, ESS_IMAGE_MAX_SIDE);
  ESS_CHECK_ARG(out_rows >= 1 && out_rows <= Hr, "%s: out_rows=%d: the top rows of the %d resized rows that are stored", me, out_rows, Hr);
  ESS_CHECK_ARG((h_table != nullptr) == (W != Wr), "%s: h_table is given exactly where the width changes (%d -> %d): an unchanged pass is skipped", me, W, Wr);
  ESS_CHECK_ARG((v_table != nullptr) == (H != Hr), "%s: v_table is given exactly where the height changes (%d -> %d): an unchanged pass is skipped", me, H, Hr);
  ESS_CHECK_ARG(!h_table || (h_taps >= 1 && h_taps <= ESS_IMAGE_MAX_TAPS), "%s: h_taps=%d must lie in [1, %d]", me, h_taps, ESS_IMAGE_MAX_TAPS);
  ESS_CHECK_ARG(!v_table || (v_taps >= 1 && v_taps <= ESS_IMAGE_MAX_TAPS), "%s: v_taps=%d must lie in [1, %d]", me, v_taps, ESS_IMAGE_MAX_TAPS);
  const bool rgb_last = channels == 3 && gray_last == 1;
  const bool hpass = h_table != nullptr || (channels == 3 && !rgb_last);
  ESS_CHECK_ARG(!hpass || scratch, "%s: null scratch: the horizontal pass writes uint8 [H][Wr]([3] with gray_last) there", me);
  ESS_CHECK_ARG(scratch != out && (const uint8_t*)scratch != frame && frame != out, "%s: frame, scratch and out must be distinct buffers", me);
  ESS_CHECK_ARG(((uintptr_t)h_table | (uintptr_t)v_table) % 4 == 0, "%s: the tables must be 4-byte aligned", me);
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* vsrc = frame;
  if (hpass) {
    const dim3 grid((unsigned)ceil_div(Wr, HP_THREADS), (unsigned)H);
    if (rgb_last)
      hipLaunchKernelGGL((frame_hpass_kernel<3, 3>), grid, dim3(HP_THREADS), 0, s, frame, h_table, v_table, scratch, H, W, Wr, h_taps, Hr, out_rows);
    else if (channels == 3)
      hipLaunchKernelGGL((frame_hpass_kernel<3, 1>), grid, dim3(HP_THREADS), 0, s, frame, h_table, v_table, scratch, H, W, Wr, h_taps, Hr, out_rows);
    else
      hipLaunchKernelGGL((frame_hpass_kernel<1, 1>), grid, dim3(HP_THREADS), 0, s, frame, h_table, v_table, scratch, H, W, Wr, h_taps, Hr, out_rows);
    vsrc = scratch;
  }
  const dim3 vgrid((unsigned)ceil_div(Wr, 256), (unsigned)out_rows);
  if (rgb_last)
    hipLaunchKernelGGL(frame_vpass_gray_kernel, vgrid, dim3(256), 0, s, vsrc, v_table, out, H, Hr, Wr, v_taps);
  else  // (one channel: image_ingest's vertical pass over the kept rows)
    hipLaunchKernelGGL(image_vpass_kernel<false>, vgrid, dim3(256), 0, s, vsrc, v_table, out, (int32_t*)nullptr, H, Hr, Wr, v_taps);
  return ess_launch_status(me);
}

extern "C" int ess_image_gather_unit(const uint8_t* images, int64_t capacity, int32_t Hs, int32_t Ws, const void* index, int32_t index_i64,
                                     int32_t B, float* out, ess_stream_t stream) {
  const char* me = "image_gather_unit";
  ESS_CHECK_ARG(images && index && out, "%s: null images, index or out", me);
  ESS_CHECK_ARG(capacity >= 1 && Hs >= 1 && Ws >= 1 && Hs <= ESS_IMAGE_MAX_SIDE && Ws <= ESS_IMAGE_MAX_SIDE,
                "%s: capacity=%lld slots of %d x %d: a positive count, sides in [1, %d]", me, (long long)capacity, Hs, Ws, ESS_IMAGE_MAX_SIDE);
  ESS_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%d must lie in [1, 65535]", me, B);
  ESS_CHECK_ARG(index_i64 == 0 || index_i64 == 1, "%s: index_i64=%d must be 0 (int32 index) or 1 (int64)", me, index_i64);
  ESS_CHECK_ARG((uintptr_t)index % (index_i64 ? 8 : 4) == 0 && (uintptr_t)out % 4 == 0, "%s: index and out must be aligned to their elements", me);
  const int64_t hw = (int64_t)Hs * Ws;
  int64_t chunks = ceil_div64(hw, 256 * 4);
  if (chunks > 1024) chunks = 1024;
  const dim3 grid((unsigned)chunks, (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
  if (index_i64)
    hipLaunchKernelGGL(image_gather_unit_kernel<int64_t>, grid, dim3(256), 0, s, images, (const int64_t*)index, out, capacity, hw);
  else
    hipLaunchKernelGGL(image_gather_unit_kernel<int32_t>, grid, dim3(256), 0, s, images, (const int32_t*)index, out, capacity, hw);
  return ess_launch_status(me);
}

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
