// Post-processing of an E2VID reconstruction on the device (reference e2vid/image_reconstructor.py:166-185 `PostProcessor`,
// e2vid/utils/inference_utils.py:18-53,112-153,261-299): the 5 x 5 Gaussian unsharp mask, the intensity rescale to 8 bit with fixed or
// auto-HDR bounds, and the event preview.  Three entry points, all capture-safe (no allocation, copy or synchronisation):
//
//   ess_recon_post_frame   unsharp mask + rescale + quantisation in ONE pass over the output window: fp32 in, uint8 (and / or the
//                          reference's float(u8) / 255) out.  The bounds (Imin, Imax - Imin) are read from device memory per sample.
//   ess_recon_post_bounds  the auto-HDR step: (a) min / max of the SHARPENED source per sample, one partial pair per workgroup into the
//                          caller's workspace (every slot written on every call -- steered: every TAKEN slot --, no atomics); (b) one wave per sample: clip in fp64,
//                          push into the sample's ring of filter_size + 1 entries, np.median of the held mins / maxs, write the bounds.
//   ess_event_preview      make_event_preview: bin sum -> red-blue BGR bytes or the grey ramp.
//
// ess_recon_post_bounds_steered / ess_recon_post_frame_steered are the same kernel text with STEER = true: a mode word per SLOT of the
// batch in device memory (the state carry's HOLD / TAKE / ZERO) decides whether the slot is processed at all, and an optional index
// table names the HISTORY ROW a slot's frame belongs to -- what a multi-stream round needs, whose one captured graph serves every mix
// of advancing, idle and restarting streams.  The STEER = false instantiations are the unsteered entry points' kernels, unchanged.
//
// The arithmetic of a pixel is FIXED -- fp32 multiply, add and divide, each rounded once, in the order written in sharpen4 / quantise
// (no fused multiply-add, no reciprocal) -- so that a numpy float32 restatement reproduces every output bit; 50 VALU instructions per
// pixel instead of 25 do not matter on a 0.3 M-pixel frame whose launches are bound by latency.  The source stays in L2 (1.2 MB at
// 480 x 640): each lane produces 4 consecutive pixels from a 5 x 8 register window, no LDS tile.
#include "common.h"

namespace {

constexpr int PARTIALS = ESS_RECON_POST_PARTIALS;

struct Taps {
  float w[25];  // (kernel arguments: the weights arrive in scalar registers)
};

// The sharpened values s[0..3] of source pixels (sy, sx0 .. sx0 + 3) of one plane p [Hs][Ws]; sy is a row of the plane and sx0 >= 0.
//   blur = sum_ky sum_kx w[ky][kx] * v(sy + ky - 2, sx + kx - 2), accumulated from 0.f in row-major tap order, a tap outside the plane
//          contributing w * 0.f (F.conv2d(padding=2) on the uncropped frame);  s = c1 * v - a * blur.
// A pixel with sx >= Ws gets a value nobody uses.  SHARP = false (amount <= 0, the reference's `if amount > 0`): s = v.
template <bool SHARP>
__device__ __forceinline__ void sharpen4(const float* __restrict__ p, int Hs, int Ws, int sy, int sx0, const Taps& k, float c1, float a,
                                         float s[4]) {
#pragma clang fp contract(off)  // (every product and sum below is rounded on its own: the outputs are compared as bits)
  if constexpr (!SHARP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = sx0 + j < Ws ? p[(size_t)sy * Ws + sx0 + j] : 0.f;
  } else {
    float win[5][8];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int y = sy + r - 2;
      const bool row_in = (unsigned)y < (unsigned)Hs;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int x = sx0 + c - 2;
        win[r][c] = (row_in && (unsigned)x < (unsigned)Ws) ? p[(size_t)y * Ws + x] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float blur = 0.f;
#pragma unroll
      for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) blur = blur + k.w[ky * 5 + kx] * win[ky][j + kx];
      s[j] = c1 * win[2][j + 2] - a * blur;
    }
  }
}

// q = (255 (s - Imin)) / range, clamped to [0, 255], truncated.  A NaN becomes 0 (fmaxf returns its other operand).
__device__ __forceinline__ uint32_t quantise(float s, float imin, float range) {
#pragma clang fp contract(off)
  const float q = (255.f * (s - imin)) / range;  // (IEEE division: the v_div_scale / v_div_fmas / v_div_fixup sequence, not v_rcp)
  return (uint32_t)fminf(fmaxf(q, 0.f), 255.f);
}

// The steering words (ess_hip.h: ESS_CARRY_HOLD / TAKE / ZERO, as ess_state_carry_masked reads them).  A slot is processed when its
// word is TAKE or ZERO; HOLD and every other word skip it.
constexpr int32_t MODE_TAKE = 1, MODE_ZERO = 2;
__device__ __forceinline__ bool mode_taken(int32_t m) { return m == MODE_TAKE || m == MODE_ZERO; }

// The steering arguments of a kernel: a trailing parameter pack STEER that is EMPTY for the unsteered entry points -- their kernels
// then have the parameter lists and the code they had before steering existed -- and one Steer for the steered ones.
struct Steer {
  const int32_t* mode;  // [N] per slot
  const int32_t* rows;  // [N] the slot's history row, or null: row = slot (the frame kernel reads neither rows nor R)
  int R;                // history rows
};
__device__ __forceinline__ const Steer& the(const Steer& st) { return st; }  // (the one member of a non-empty pack)

// The history row of slot n in a steered bounds step, or -1 where the slot is skipped: its word does not take it, or its row lies
// outside [0, R).  Both words depend on the slot alone: every lane of a workgroup gets the same answer (scalar loads).
__device__ __forceinline__ int steered_row(const Steer& st, size_t n) {
  if (!mode_taken(st.mode[n])) return -1;
  const int r = st.rows ? st.rows[n] : (int)n;
  return (unsigned)r < (unsigned)st.R ? r : -1;
}

// One lane = 4 consecutive pixels of one output row.  vec8 / vec32: W % 4 == 0 and the output pointer aligned for one 4-byte / 16-byte
// store per lane; otherwise single elements (DDD17's W = 346).  STEER: the items of a slot whose mode word does not take it are
// neither read nor written.
template <bool SHARP, typename... STEER>
__global__ __launch_bounds__(256) void frame_kernel(const float* __restrict__ img, const Taps k, float c1, float a,
                                                    const float* __restrict__ bounds, uint8_t* __restrict__ out8,
                                                    float* __restrict__ out32, int N, int Hs, int Ws, int y0, int x0, int H, int W,
                                                    int vec8, int vec32, const STEER... steer) {
  const int G = (W + 3) >> 2;
  const size_t total = (size_t)N * H * G, plane = (size_t)Hs * Ws;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ox = (int)(i % G) * 4;
    const size_t r = i / G;
    const int oy = (int)(r % H);
    const size_t n = r / H;
    if constexpr (sizeof...(STEER) > 0) {
      if (!mode_taken(the(steer...).mode[n])) continue;
    }
    float s[4];
    sharpen4<SHARP>(img + n * plane, Hs, Ws, y0 + oy, x0 + ox, k, c1, a, s);
    const float imin = bounds[2 * n], range = bounds[2 * n + 1];
    uint32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = quantise(s[j], imin, range);
    const size_t o = (n * H + oy) * (size_t)W + ox;
    const int cnt = min(4, W - ox);
    if (out8) {
      if (vec8) *(uint32_t*)(out8 + o) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
      else
        for (int j = 0; j < cnt; ++j) out8[o + j] = (uint8_t)q[j];
    }
    if (out32) {
      f32x4 f;
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = (float)q[j] / 255.f;  // (IntensityRescaler: img.byte().float().div(255))
      if (vec32) *(f32x4*)(out32 + o) = f;
      else
        for (int j = 0; j < cnt; ++j) out32[o + j] = f[j];
    }
  }
}

// Pass (a) of the auto-HDR step: min and max of the sharpened plane of sample blockIdx.y over this workgroup's share of the 4-pixel
// groups -> part[(n * PARTIALS + blockIdx.x) * 2 + {0, 1}].  A workgroup without pixels writes (+inf, -inf); NaN pixels are skipped.
// STEER: the workgroups of a skipped slot return at once -- no image read, no partial written; the exit depends on blockIdx.y
// only and comes before the barrier.
template <bool SHARP, typename... STEER>
__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ img, const Taps k, float c1, float a, int Hs, int Ws,
                                                     float* __restrict__ part, const STEER... steer) {
  __shared__ float red[2][4];
  const size_t n = blockIdx.y;
  if constexpr (sizeof...(STEER) > 0) {
    if (steered_row(the(steer...), n) < 0) return;
  }
  const int G = (Ws + 3) >> 2;
  const size_t total = (size_t)Hs * G;
  const float* p = img + n * (size_t)Hs * Ws;
  float mn = INFINITY, mx = -INFINITY;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int sx0 = (int)(i % G) * 4, sy = (int)(i / G);
    float s[4];
    sharpen4<SHARP>(p, Hs, Ws, sy, sx0, k, c1, a, s);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (sx0 + j < Ws) {
        mn = fminf(mn, s[j]);
        mx = fmaxf(mx, s[j]);
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][w] = mn;
    red[1][w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = part + (n * PARTIALS + blockIdx.x) * 2;
    o[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    o[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__device__ __forceinline__ double wave_pick_sum(double v) {  // (all addends but one or two are +0.0: the sum is theirs, rounded once)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Pass (b): one wave per sample.  ring [N][cap][2] doubles (min, max), state [N][2] int32 (head, count), cap = filter_size + 1 <= 64.
// The reference pops the oldest entry only when the history is LONGER than filter_size and then appends, so the history settles at
// filter_size + 1 entries: a ring of that capacity whose oldest entry the new one overwrites.  The median does not depend on the
// order of the entries, so lane i holds physical slot i; the lane of the slot written in this call takes the new pair from
// registers, not from memory.
// STEER: the partials and the bounds are indexed by the SLOT n, ring and state by the slot's history row (R rows); a skipped slot's
// wave returns without touching anything; a ZERO slot takes head = count = 0 in place of the stored state, which empties the row's
// history before this frame enters it.
template <typename... STEER>
__global__ __launch_bounds__(64) void bounds_kernel(const float* __restrict__ part, double* __restrict__ ring, int32_t* __restrict__ state,
                                                    int cap, float* __restrict__ bounds, const STEER... steer) {
  const size_t n = blockIdx.x;
  size_t row = n;
  bool restart = false;
  if constexpr (sizeof...(STEER) > 0) {
    const int r = steered_row(the(steer...), n);
    if (r < 0) return;
    row = (size_t)r;
    restart = the(steer...).mode[n] == MODE_ZERO;
  }
  const int lane = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = lane; i < PARTIALS; i += 64) {
    mn = fminf(mn, part[(n * PARTIALS + i) * 2]);
    mx = fmaxf(mx, part[(n * PARTIALS + i) * 2 + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  const double lo = fmin(fmax((double)mn, 0.0), 0.45);  // np.clip(Imin, 0.0, 0.45)
  const double hi = fmin(fmax((double)mx, 0.55), 1.0);  // np.clip(Imax, 0.55, 1.0)
  int head = state[2 * row], count = state[2 * row + 1];
  if (restart) head = count = 0;
  head = min(max(head, 0), cap - 1);  // (a state the caller corrupted must not send a store outside the ring)
  count = min(max(count, 0), cap);
  int slot;
  if (count == cap) {
    slot = head;
    head = head + 1 == cap ? 0 : head + 1;
  } else {
    slot = head + count >= cap ? head + count - cap : head + count;
    ++count;
  }
  double* rg = ring + row * (size_t)cap * 2;
  // the held entries are the `count` slots from `head` on (cyclically); with count < cap they need not start at slot 0
  int phys = head + lane;
  if (phys >= cap) phys -= cap;
  const bool held = lane < count;
  double vmin = 0.0, vmax = 0.0;
  if (held) {
    if (phys == slot) {
      vmin = lo;
      vmax = hi;
    } else {
      vmin = rg[2 * phys];
      vmax = rg[2 * phys + 1];
    }
  }
  int rank_min = 0, rank_max = 0;
  for (int j = 0; j < count; ++j) {
    const double a = __shfl(vmin, j, 64), b = __shfl(vmax, j, 64);
    rank_min += (a < vmin || (a == vmin && j < lane)) ? 1 : 0;
    rank_max += (b < vmax || (b == vmax && j < lane)) ? 1 : 0;
  }
  // np.median: the middle value, or the mean of the two middle values for an even count
  const int m1 = count >> 1, m0 = (count & 1) ? m1 : m1 - 1;
  double smin = wave_pick_sum(held && (rank_min == m0 || rank_min == m1) ? vmin : 0.0);
  double smax = wave_pick_sum(held && (rank_max == m0 || rank_max == m1) ? vmax : 0.0);
  if (!(count & 1)) {
    smin = smin / 2.0;
    smax = smax / 2.0;
  }
  if (lane == 0) {
    rg[2 * slot] = lo;
    rg[2 * slot + 1] = hi;
    state[2 * row] = head;
    state[2 * row + 1] = count;
    bounds[2 * n] = (float)smin;
    bounds[2 * n + 1] = (float)(smax - smin);
  }
}

// make_event_preview: s = sum of planes c0 .. C - 1 in plane order (fp32, each sum rounded).  Red-blue: BGR bytes, blue where s > 0,
// red where s < 0.  Greyscale: (255 (s + 10)) / 20 clamped to [0, 255], then truncated.  VEC: 4 pixels per lane (H W % 4 == 0, aligned).
__device__ __forceinline__ uint32_t preview_grey(float s) {
#pragma clang fp contract(off)
  const float q = (255.f * (s + 10.f)) / 20.f;
  return (uint32_t)fminf(fmaxf(q, 0.f), 255.f);
}

template <bool VEC, bool GREY>
__global__ __launch_bounds__(256) void preview_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int N, int C, int c0,
                                                      size_t hw) {
#pragma clang fp contract(off)
  constexpr int PX = VEC ? 4 : 1;
  const size_t per = hw / PX, total = (size_t)N * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t n = i / per, px = (i % per) * PX;
    const float* p = x + (n * C + c0) * hw + px;
    float s[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) s[j] = 0.f;
    for (int c = c0; c < C; ++c, p += hw) {
      if constexpr (VEC) {
        const f32x4 v = *(const f32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s[j] + v[j];
      } else {
        s[0] = s[0] + p[0];
      }
    }
    const size_t o = n * hw + px;
    if constexpr (GREY) {
      if constexpr (VEC)
        *(uint32_t*)(out + o) = preview_grey(s[0]) | (preview_grey(s[1]) << 8) | (preview_grey(s[2]) << 16) | (preview_grey(s[3]) << 24);
      else
        out[o] = (uint8_t)preview_grey(s[0]);
    } else {
      uint8_t b[PX * 3];
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        b[3 * j] = s[j] > 0.f ? 255 : 0;
        b[3 * j + 1] = 0;
        b[3 * j + 2] = s[j] < 0.f ? 255 : 0;
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
}

inline unsigned capped_grid(size_t items, int cap) {
  size_t g = (items + 255) / 256;
  if (g > (size_t)cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

// the checks both image entry points share
int check_image(const char* who, const float* img, const float* weights, float c1, float amount, int32_t N, int32_t Hs, int32_t Ws) {
  ESS_CHECK_ARG(img, "%s: null img", who);
  ESS_CHECK_ARG(((uintptr_t)img & 3) == 0, "%s: img must be 4-byte aligned", who);
  ESS_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0, "%s: bad extents N=%d Hs=%d Ws=%d", who, N, Hs, Ws);
  ESS_CHECK_ARG(amount == amount && c1 == c1, "%s: amount / c1 is NaN", who);
  ESS_CHECK_ARG(!(amount > 0.f) || weights, "%s: amount=%g > 0 needs the 25 weights", who, (double)amount);
  return 0;
}

// the kernel's copy of the weights: `weights` is HOST memory, read here, after every check has passed
Taps taps_of(const float* weights, float amount) {
  Taps k;
  for (int i = 0; i < 25; ++i) k.w[i] = (amount > 0.f) ? weights[i] : 0.f;
  return k;
}

}  // namespace

// both frame entry points: mode null = the unsteered kernels (named first here and in launch_bounds: the instantiations then keep
// their places at the head of the code object)
static int launch_frame(const char* who, const float* img, const float* weights, float c1, float amount, const float* bounds,
                        uint8_t* frame_u8, float* frame_f32, int32_t N, int32_t Hs, int32_t Ws, int32_t win_y0, int32_t win_x0,
                        int32_t win_h, int32_t win_w, const int32_t* mode, ess_stream_t stream) {
  if (int rc = check_image(who, img, weights, c1, amount, N, Hs, Ws)) return rc;
  ESS_CHECK_ARG(bounds, "%s: null bounds", who);
  ESS_CHECK_ARG(((uintptr_t)bounds & 3) == 0 && ((uintptr_t)frame_f32 & 3) == 0, "%s: bounds and frame_f32 must be 4-byte aligned", who);
  ESS_CHECK_ARG(frame_u8 || frame_f32, "%s: frame_u8 and frame_f32 are both null", who);
  ESS_CHECK_ARG(win_y0 >= 0 && win_x0 >= 0 && win_h > 0 && win_w > 0 && (int64_t)win_y0 + win_h <= Hs && (int64_t)win_x0 + win_w <= Ws,
                "%s: window (%d, %d, %d, %d) leaves the %d x %d source", who, win_y0, win_x0, win_h, win_w, Hs, Ws);
  const size_t items = (size_t)N * win_h * ((win_w + 3) >> 2);
  const unsigned grid = capped_grid(items, 2048);
  const int vec8 = win_w % 4 == 0 && ((uintptr_t)frame_u8 & 3) == 0, vec32 = win_w % 4 == 0 && ((uintptr_t)frame_f32 & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const Taps k = taps_of(weights, amount);
  if (!mode) {
    if (amount > 0.f)
      hipLaunchKernelGGL(frame_kernel<true>, dim3(grid), dim3(256), 0, st, img, k, c1, amount, bounds, frame_u8, frame_f32, N, Hs, Ws,
                         win_y0, win_x0, win_h, win_w, vec8, vec32);
    else
      hipLaunchKernelGGL(frame_kernel<false>, dim3(grid), dim3(256), 0, st, img, k, c1, amount, bounds, frame_u8, frame_f32, N, Hs, Ws,
                         win_y0, win_x0, win_h, win_w, vec8, vec32);
  } else {
    const Steer steer{mode, nullptr, N};
    if (amount > 0.f)
      hipLaunchKernelGGL((frame_kernel<true, Steer>), dim3(grid), dim3(256), 0, st, img, k, c1, amount, bounds, frame_u8, frame_f32, N, Hs,
                         Ws, win_y0, win_x0, win_h, win_w, vec8, vec32, steer);
    else
      hipLaunchKernelGGL((frame_kernel<false, Steer>), dim3(grid), dim3(256), 0, st, img, k, c1, amount, bounds, frame_u8, frame_f32, N, Hs,
                         Ws, win_y0, win_x0, win_h, win_w, vec8, vec32, steer);
  }
  return ess_launch_status(who);
}

extern "C" int ess_recon_post_frame(const float* img, const float* weights, float c1, float amount, const float* bounds,
                                    uint8_t* frame_u8, float* frame_f32, int32_t N, int32_t Hs, int32_t Ws, int32_t win_y0,
                                    int32_t win_x0, int32_t win_h, int32_t win_w, ess_stream_t stream) {
  return launch_frame("recon_post_frame", img, weights, c1, amount, bounds, frame_u8, frame_f32, N, Hs, Ws, win_y0, win_x0, win_h, win_w,
                      nullptr, stream);
}

extern "C" int ess_recon_post_frame_steered(const float* img, const float* weights, float c1, float amount, const float* bounds,
                                            uint8_t* frame_u8, float* frame_f32, int32_t N, int32_t Hs, int32_t Ws, int32_t win_y0,
                                            int32_t win_x0, int32_t win_h, int32_t win_w, const int32_t* mode, ess_stream_t stream) {
  ESS_CHECK_ARG(mode && ((uintptr_t)mode & 3) == 0, "recon_post_frame_steered: mode is null or not 4-byte aligned");
  return launch_frame("recon_post_frame_steered", img, weights, c1, amount, bounds, frame_u8, frame_f32, N, Hs, Ws, win_y0, win_x0, win_h,
                      win_w, mode, stream);
}

// both bounds entry points: mode null = the unsteered kernels on R = N histories
static int launch_bounds(const char* who, const float* img, const float* weights, float c1, float amount, int32_t N, int32_t Hs,
                         int32_t Ws, float* workspace, size_t workspace_bytes, double* ring, int32_t* ring_state, int32_t R,
                         int32_t filter_size, float* bounds, const int32_t* mode, const int32_t* rows, ess_stream_t stream) {
  if (int rc = check_image(who, img, weights, c1, amount, N, Hs, Ws)) return rc;
  ESS_CHECK_ARG(filter_size >= 0 && filter_size <= ESS_RECON_POST_MAX_FILTER, "%s: filter_size=%d outside 0..%d", who, filter_size,
                ESS_RECON_POST_MAX_FILTER);
  ESS_CHECK_ARG(N <= 65535, "%s: N=%d samples exceed the grid's 65535 rows", who, N);
  ESS_CHECK_ARG(R > 0, "%s: R=%d history rows", who, R);
  ESS_CHECK_ARG(workspace && ring && ring_state && bounds, "%s: null workspace, ring, ring_state or bounds", who);
  ESS_CHECK_ARG(workspace_bytes >= (size_t)N * PARTIALS * 2 * sizeof(float), "%s: workspace has %zu bytes, N=%d needs %zu", who,
                workspace_bytes, N, (size_t)N * PARTIALS * 2 * sizeof(float));
  ESS_CHECK_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)ring & 7) == 0 && ((uintptr_t)ring_state & 3) == 0 && ((uintptr_t)bounds & 3) == 0,
                "%s: workspace, ring_state, bounds must be 4-byte and ring 8-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const Taps k = taps_of(weights, amount);
  const Steer steer{mode, rows, R};
  if (!mode) {
    if (amount > 0.f)
      hipLaunchKernelGGL(minmax_kernel<true>, dim3(PARTIALS, N), dim3(256), 0, st, img, k, c1, amount, Hs, Ws, workspace);
    else
      hipLaunchKernelGGL(minmax_kernel<false>, dim3(PARTIALS, N), dim3(256), 0, st, img, k, c1, amount, Hs, Ws, workspace);
  } else if (amount > 0.f)
    hipLaunchKernelGGL((minmax_kernel<true, Steer>), dim3(PARTIALS, N), dim3(256), 0, st, img, k, c1, amount, Hs, Ws, workspace, steer);
  else
    hipLaunchKernelGGL((minmax_kernel<false, Steer>), dim3(PARTIALS, N), dim3(256), 0, st, img, k, c1, amount, Hs, Ws, workspace, steer);
  if (int rc = ess_launch_status(mode ? "recon_post_bounds_steered (min / max)" : "recon_post_bounds (min / max)")) return rc;
  if (!mode)
    hipLaunchKernelGGL(bounds_kernel<>, dim3(N), dim3(64), 0, st, (const float*)workspace, ring, ring_state, filter_size + 1, bounds);
  else
    hipLaunchKernelGGL(bounds_kernel<Steer>, dim3(N), dim3(64), 0, st, (const float*)workspace, ring, ring_state, filter_size + 1, bounds,
                       steer);
  return ess_launch_status(mode ? "recon_post_bounds_steered (median)" : "recon_post_bounds (median)");
}

extern "C" int ess_recon_post_bounds(const float* img, const float* weights, float c1, float amount, int32_t N, int32_t Hs, int32_t Ws,
                                     float* workspace, size_t workspace_bytes, double* ring, int32_t* ring_state, int32_t filter_size,
                                     float* bounds, ess_stream_t stream) {
  return launch_bounds("recon_post_bounds", img, weights, c1, amount, N, Hs, Ws, workspace, workspace_bytes, ring, ring_state, N,
                       filter_size, bounds, nullptr, nullptr, stream);
}

extern "C" int ess_recon_post_bounds_steered(const float* img, const float* weights, float c1, float amount, int32_t N, int32_t Hs,
                                             int32_t Ws, float* workspace, size_t workspace_bytes, double* ring, int32_t* ring_state,
                                             int32_t R, int32_t filter_size, float* bounds, const int32_t* mode, const int32_t* rows,
                                             ess_stream_t stream) {
  ESS_CHECK_ARG(mode && ((uintptr_t)mode & 3) == 0 && ((uintptr_t)rows & 3) == 0, "recon_post_bounds_steered: mode is null, or mode / rows not 4-byte aligned");
  return launch_bounds("recon_post_bounds_steered", img, weights, c1, amount, N, Hs, Ws, workspace, workspace_bytes, ring, ring_state, R,
                       filter_size, bounds, mode, rows, stream);
}

extern "C" int ess_event_preview(const float* grids, uint8_t* out, int32_t N, int32_t C, int32_t H, int32_t W, int32_t num_bins_to_show,
                                 int32_t mode, ess_stream_t stream) {
  ESS_CHECK_ARG(grids && out, "event_preview: null grids or out");
  ESS_CHECK_ARG(((uintptr_t)grids & 3) == 0, "event_preview: grids must be 4-byte aligned");
  ESS_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0, "event_preview: bad extents N=%d C=%d H=%d W=%d", N, C, H, W);
  ESS_CHECK_ARG(mode == ESS_PREVIEW_RED_BLUE || mode == ESS_PREVIEW_GRAYSCALE, "event_preview: mode=%d is neither red-blue (0) nor grayscale (1)",
                mode);
  // events[0, -num_bins_to_show:]: a negative count shows every bin, and so do 0 (`-0:`) and a count above C (the slice saturates)
  const int c0 = (num_bins_to_show <= 0 || num_bins_to_show >= C) ? 0 : C - num_bins_to_show;
  const size_t hw = (size_t)H * W;
  const bool vec = hw % 4 == 0 && ((uintptr_t)grids & 15) == 0 && ((uintptr_t)out & 3) == 0;
  const unsigned grid = capped_grid((size_t)N * (vec ? hw / 4 : hw), 2048);
  hipStream_t st = (hipStream_t)stream;
#define ESS_PV(V_, G_) hipLaunchKernelGGL((preview_kernel<V_, G_>), dim3(grid), dim3(256), 0, st, grids, out, N, C, c0, hw)
  if (mode == ESS_PREVIEW_GRAYSCALE) {
    if (vec) ESS_PV(true, true);
    else ESS_PV(false, true);
  } else {
    if (vec) ESS_PV(true, false);
    else ESS_PV(false, false);
  }
#undef ESS_PV
  return ess_launch_status("event_preview");
}
