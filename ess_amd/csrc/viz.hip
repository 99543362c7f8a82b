// Segmentation display on the device (reference utils/viz_utils.py:19-73,105-145: createRGBImage, visualizeHistogram,
// visualizeVoxelGrid, create_checkerboard, prepare_semseg): the tiles of the trainers' validation panels and the label overlay of the
// streaming segmenter.  Three entry points, all capture-safe (no allocation, copy or synchronisation, no host state):
//
//   ess_viz_semseg   labels uint8 / int64 [N][H][W] + colour table fp32 [K][3] (0..1) -> fp32 RGB tiles; the ignore label -- and any
//                    label outside [0, K) -- shows the reference's checkerboard.
//   ess_viz_events   fp32 [N][C][H][W] -> fp32 RGB tiles: the histogram, the separate-polarity voxel grid or the signed sum.
//   ess_viz_overlay  labels uint8 + gray frame uint8 + palette uint8 [K][3] + alpha -> uint8 [N][H][W][3].
//
// The two tile writers place sample n as tile t = tile0 + n of a grid of tiles (EssVizDst below): a plain [N][3][H][W] tensor is the grid
// of one column, a make_grid panel is a grid of xmaps columns whose slots are H + padding rows and W + padding columns apart.
//
// Streaming maps without reuse: one lane per 4 consecutive pixels of a row, coalesced along x; 16-byte loads and stores where every
// pointer, stride and W allow it, single elements otherwise (a panel slot's row stride is odd in general).  The arithmetic of a pixel is
// FIXED -- fp32 multiply, add and IEEE divide, each rounded once, never fused, sums in ascending channel order from 0.f -- so that a
// numpy float32 restatement reproduces every output bit.
#include "common.h"

namespace {

struct Dst {  // where sample n's tile goes, in elements from `out`
  int64_t plane, row, tile_y, tile_x;
  int32_t tile0, per_row;
  __host__ __device__ int64_t origin(int64_t n) const {
    const int64_t t = (int64_t)tile0 + n;
    return (t / per_row) * tile_y + (t % per_row) * tile_x;
  }
};

// the three planes of 4 pixels -> the tile; cnt: the pixels of this group inside the row
template <bool VEC>
__device__ __forceinline__ void store3(float* __restrict__ out, int64_t o, int64_t plane, const float v[3][4], int cnt) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (VEC) {
      f32x4 f;
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = v[c][j];
      *(f32x4*)(out + o + c * plane) = f;
    } else {
      for (int j = 0; j < cnt; ++j) out[o + c * plane + j] = v[c][j];
    }
  }
}

// prepare_semseg + create_checkerboard.  L: uint8_t or int64_t.
template <typename L, bool VEC>
__global__ __launch_bounds__(256) void semseg_kernel(const L* __restrict__ labels, const float* __restrict__ colours, float* __restrict__ out,
                                                     int N, int K, int H, int W, int64_t ignore, Dst d) {
  const int G = (W + 3) >> 2;
  const size_t total = (size_t)N * H * G;
  const int cell = max(min(H, W) / 32, 1);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x0 = (int)(i % G) * 4;
    const size_t r = i / G;
    const int y = (int)(r % H);
    const int64_t n = (int64_t)(r / H);
    const int cnt = min(4, W - x0);
    const L* p = labels + ((size_t)n * H + y) * (size_t)W + x0;
    int64_t l[4];
    if constexpr (VEC && sizeof(L) == 1) {
      const uint32_t w = *(const uint32_t*)p;
#pragma unroll
      for (int j = 0; j < 4; ++j) l[j] = (w >> (8 * j)) & 0xFF;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) l[j] = j < cnt ? (int64_t)p[j] : ignore;
    }
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (l[j] == ignore || l[j] < 0 || l[j] >= K) {
        const float c = ((y / cell + (x0 + j) / cell) & 1) ? 0.25f : 0.75f;
        v[0][j] = v[1][j] = v[2][j] = c;
      } else {
        v[0][j] = colours[l[j] * 3];
        v[1][j] = colours[l[j] * 3 + 1];
        v[2][j] = colours[l[j] * 3 + 2];
      }
    }
    store3<VEC>(out, d.origin(n) + (int64_t)y * d.row + x0, d.plane, v, cnt);
  }
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }  // (a NaN stays a NaN, as torch.clamp)

// visualizeHistogram / visualizeVoxelGrid.  hi: 255.f or 1.f (the signed tile's mark).
template <bool VEC>
__global__ __launch_bounds__(256) void events_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int C, int H, int W, int mode,
                                                     float hi, Dst d) {
#pragma clang fp contract(off)  // (every product and sum below is rounded on its own: the outputs are compared as bits)
  const int G = (W + 3) >> 2;
  const size_t total = (size_t)N * H * G, hw = (size_t)H * W;
  const int half = C / 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x0 = (int)(i % G) * 4;
    const size_t r = i / G;
    const int y = (int)(r % H);
    const int64_t n = (int64_t)(r / H);
    const int cnt = min(4, W - x0);
    const float* p = x + (size_t)n * C * hw + (size_t)y * W + x0;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};  // (histogram: x0, x1; separate_pol: pos, neg; signed: s, -)
    for (int c = 0; c < C; ++c, p += hw) {
      float in[4];
      if constexpr (VEC) {
        const f32x4 f = *(const f32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) in[j] = f[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) in[j] = j < cnt ? p[j] : 0.f;
      }
      if (mode == ESS_VIZ_HISTOGRAM) {
#pragma unroll
        for (int j = 0; j < 4; ++j) (c == 0 ? a : b)[j] = in[j];
      } else if (mode == ESS_VIZ_SEPARATE_POL) {
        const int k = c < half ? c : c - half;
        const float t = (float)(k + 1) / (float)half;  // (IEEE division, as arange(1, half + 1) / half)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float prod = in[j] * t;
          if (c < half) a[j] = a[j] + prod;
          else b[j] = b[j] + prod;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = a[j] + in[j];
      }
    }
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (mode == ESS_VIZ_HISTOGRAM) {
        v[0][j] = clamp01(a[j]);
        v[1][j] = clamp01(b[j]);
        v[2][j] = 0.f;
      } else if (mode == ESS_VIZ_SEPARATE_POL) {
        v[0][j] = clamp01(b[j]);
        v[1][j] = clamp01(a[j]);
        v[2][j] = 0.f;
      } else {
        v[0][j] = a[j] > 0.f ? hi : 0.f;
        v[1][j] = 0.f;
        v[2][j] = a[j] < 0.f ? hi : 0.f;
      }
    }
    store3<VEC>(out, d.origin(n) + (int64_t)y * d.row + x0, d.plane, v, cnt);
  }
}

// v = (1 - alpha) g + alpha colour, two products and one sum; (uint8) min(v + 0.5f, 255.f).  A label >= K shows the gray value.
// VEC: 4 pixels per lane over the flat pixel index (total % 4 == 0, pointers 4-byte aligned): one 4-byte load of the labels and of the
// frame, three 4-byte stores.
template <bool VEC>
__global__ __launch_bounds__(256) void overlay_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ gray,
                                                      const uint8_t* __restrict__ palette, uint8_t* __restrict__ out, size_t total, int K,
                                                      float alpha) {
#pragma clang fp contract(off)
  constexpr int PX = VEC ? 4 : 1;
  const float beta = 1.0f - alpha;
  const size_t groups = total / PX;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += (size_t)gridDim.x * blockDim.x) {
    const size_t o = i * PX;
    uint32_t l[PX], g[PX];
    if constexpr (VEC) {
      const uint32_t lw = *(const uint32_t*)(labels + o), gw = *(const uint32_t*)(gray + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        l[j] = (lw >> (8 * j)) & 0xFF;
        g[j] = (gw >> (8 * j)) & 0xFF;
      }
    } else {
      l[0] = labels[o];
      g[0] = gray[o];
    }
    uint8_t b[PX * 3];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (l[j] >= (uint32_t)K) {
          b[3 * j + c] = (uint8_t)g[j];
        } else {
          const float col = (float)palette[l[j] * 3 + c];
          const float p0 = beta * (float)g[j], p1 = alpha * col;
          const float v = p0 + p1;
          b[3 * j + c] = (uint8_t)fminf(v + 0.5f, 255.f);
        }
      }
    }
    if constexpr (VEC) {
      uint32_t* o32 = (uint32_t*)(out + o * 3);  // (o % 4 == 0: 12 bytes per lane, 4-byte aligned)
#pragma unroll
      for (int w = 0; w < 3; ++w)
        o32[w] = b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
    } else {
      out[o * 3] = b[0];
      out[o * 3 + 1] = b[1];
      out[o * 3 + 2] = b[2];
    }
  }
}

inline unsigned capped_grid(size_t items, int cap) {
  size_t g = (items + 255) / 256;
  if (g > (size_t)cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

// the destination checks both tile writers share: every element a launch may write lies inside the caller's out_elems
int check_dst(const char* who, const float* out, size_t out_elems, const EssVizDst* dst, int32_t N, int32_t H, int32_t W, Dst* d) {
  ESS_CHECK_ARG(out && dst, "%s: null out or dst", who);
  ESS_CHECK_ARG(((uintptr_t)out & 3) == 0, "%s: out must be 4-byte aligned", who);
  ESS_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: bad extents N=%d H=%d W=%d", who, N, H, W);
  ESS_CHECK_ARG(dst->tile0 >= 0 && dst->tiles_per_row > 0, "%s: tile0=%d / tiles_per_row=%d", who, dst->tile0, dst->tiles_per_row);
  ESS_CHECK_ARG(dst->row_stride >= W && dst->plane_stride >= 0 && dst->tile_stride_y >= 0 && dst->tile_stride_x >= 0,
                "%s: row_stride=%lld must be >= W=%d and no stride negative", who, (long long)dst->row_stride, W);
  d->plane = dst->plane_stride;
  d->row = dst->row_stride;
  d->tile_y = dst->tile_stride_y;
  d->tile_x = dst->tile_stride_x;
  d->tile0 = dst->tile0;
  d->per_row = dst->tiles_per_row;
  // the largest offset written: the last pixel of plane 2 of the tile in the last grid row and the right-most column any tile takes
  const int64_t t_last = (int64_t)dst->tile0 + N - 1;
  const int64_t col_max = t_last / dst->tiles_per_row > (int64_t)dst->tile0 / dst->tiles_per_row ? dst->tiles_per_row - 1 : t_last % dst->tiles_per_row;
  const int64_t last = (t_last / dst->tiles_per_row) * d->tile_y + col_max * d->tile_x + 2 * d->plane + (int64_t)(H - 1) * d->row + (W - 1);
  ESS_CHECK_ARG(last >= 0 && (uint64_t)last < (uint64_t)out_elems, "%s: the tiles reach element %lld of an output of %zu", who, (long long)last,
                out_elems);
  return 0;
}

inline bool dst_vec(const float* out, const Dst& d, int W) {
  return W % 4 == 0 && ((uintptr_t)out & 15) == 0 && d.plane % 4 == 0 && d.row % 4 == 0 && d.tile_y % 4 == 0 && d.tile_x % 4 == 0;
}

}  // namespace

extern "C" int ess_viz_semseg(const void* labels, int32_t label_type, const float* colours, float* out, size_t out_elems,
                              const EssVizDst* dst, int32_t N, int32_t K, int32_t H, int32_t W, int32_t ignore_label, ess_stream_t stream) {
  Dst d;
  if (int rc = check_dst("viz_semseg", out, out_elems, dst, N, H, W, &d)) return rc;
  ESS_CHECK_ARG(labels && colours, "viz_semseg: null labels or colours");
  ESS_CHECK_ARG(label_type == ESS_VIZ_LABELS_U8 || label_type == ESS_VIZ_LABELS_I64, "viz_semseg: label_type=%d is neither uint8 (0) nor int64 (1)",
                label_type);
  ESS_CHECK_ARG(K > 0, "viz_semseg: K=%d", K);
  ESS_CHECK_ARG(((uintptr_t)colours & 3) == 0 && (label_type == ESS_VIZ_LABELS_U8 || ((uintptr_t)labels & 7) == 0),
                "viz_semseg: colours must be 4-byte and int64 labels 8-byte aligned");
  const unsigned grid = capped_grid((size_t)N * H * ((W + 3) >> 2), 2048);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = dst_vec(out, d, W) && (label_type == ESS_VIZ_LABELS_I64 || ((uintptr_t)labels & 3) == 0);
#define ESS_SS(L_, V_)                                                                                                                  \
  hipLaunchKernelGGL((semseg_kernel<L_, V_>), dim3(grid), dim3(256), 0, st, (const L_*)labels, colours, out, N, K, H, W, (int64_t)ignore_label, d)
  if (label_type == ESS_VIZ_LABELS_U8) {
    if (vec) ESS_SS(uint8_t, true);
    else ESS_SS(uint8_t, false);
  } else {
    if (vec) ESS_SS(int64_t, true);
    else ESS_SS(int64_t, false);
  }
#undef ESS_SS
  return ess_launch_status("viz_semseg");
}

extern "C" int ess_viz_events(const float* x, float* out, size_t out_elems, const EssVizDst* dst, int32_t N, int32_t C, int32_t H, int32_t W,
                              int32_t mode, int32_t unit, ess_stream_t stream) {
  Dst d;
  if (int rc = check_dst("viz_events", out, out_elems, dst, N, H, W, &d)) return rc;
  ESS_CHECK_ARG(x, "viz_events: null x");
  ESS_CHECK_ARG(((uintptr_t)x & 3) == 0, "viz_events: x must be 4-byte aligned");
  ESS_CHECK_ARG(mode == ESS_VIZ_HISTOGRAM || mode == ESS_VIZ_SEPARATE_POL || mode == ESS_VIZ_SIGNED,
                "viz_events: mode=%d is none of histogram (0), separate_pol (1), signed (2)", mode);
  ESS_CHECK_ARG(mode != ESS_VIZ_HISTOGRAM || C == 2, "viz_events: the histogram tile needs C = 2, got %d", C);
  ESS_CHECK_ARG(mode != ESS_VIZ_SEPARATE_POL || (C >= 4 && C % 2 == 0), "viz_events: the separate_pol tile needs an even C >= 4, got %d", C);
  ESS_CHECK_ARG(mode != ESS_VIZ_SIGNED || C > 3, "viz_events: the signed tile needs C > 3, got %d", C);
  const unsigned grid = capped_grid((size_t)N * H * ((W + 3) >> 2), 2048);
  hipStream_t st = (hipStream_t)stream;
  const float hi = unit ? 1.f : 255.f;
  if (dst_vec(out, d, W) && ((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(events_kernel<true>, dim3(grid), dim3(256), 0, st, x, out, N, C, H, W, mode, hi, d);
  else
    hipLaunchKernelGGL(events_kernel<false>, dim3(grid), dim3(256), 0, st, x, out, N, C, H, W, mode, hi, d);
  return ess_launch_status("viz_events");
}

extern "C" int ess_viz_overlay(const uint8_t* labels, const uint8_t* gray, const uint8_t* palette, uint8_t* out, int32_t N, int32_t K,
                               int32_t H, int32_t W, float alpha, ess_stream_t stream) {
  ESS_CHECK_ARG(labels && gray && palette && out, "viz_overlay: null labels, gray, palette or out");
  ESS_CHECK_ARG(N > 0 && H > 0 && W > 0 && K > 0 && K <= 256, "viz_overlay: bad extents N=%d K=%d H=%d W=%d", N, K, H, W);
  ESS_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "viz_overlay: alpha=%g outside [0, 1]", (double)alpha);
  const size_t total = (size_t)N * H * W;
  const bool vec = total % 4 == 0 && (((uintptr_t)labels | (uintptr_t)gray | (uintptr_t)out) & 3) == 0;
  const unsigned grid = capped_grid(vec ? total / 4 : total, 2048);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(overlay_kernel<true>, dim3(grid), dim3(256), 0, st, labels, gray, palette, out, total, K, alpha);
  else hipLaunchKernelGGL(overlay_kernel<false>, dim3(grid), dim3(256), 0, st, labels, gray, palette, out, total, K, alpha);
  return ess_launch_status("viz_overlay");
}
