// Masked carry of a batched recurrent state: every level and every part of it in ONE launch, steered per sample by a mode word in
// device memory (ess_state_carry_masked, include/ess_hip.h), and its indexed sibling, which moves record src_index[p] of one batch to
// record dst_index[p] of another (ess_state_carry_indexed: gather / scatter between the home state of S streams and a compact batch).
// HBM-bound: 16-byte vector loads and stores, nothing else.
#include "common.h"

namespace {

constexpr int CARRY_MAX_TENSORS = 16;
constexpr int CARRY_THREADS = 256;
constexpr int CARRY_UNROLL = 4;            // 16-byte loads in flight per thread before the first store
constexpr int CARRY_MAX_BLOCKS = 4096;     // 256 CUs x 16: enough workgroups to hide HBM latency, few enough to launch quickly
constexpr int64_t CARRY_SEG_BYTES = 128 * 1024;  // bytes of one sample record a workgroup walks, before the block cap widens it

// The three host tables by value (a captured launch keeps them: no device table to keep alive) + where each tensor's workgroups
// start in the grid: tensor i owns blocks [first[i], first[i + 1]) = n_samples x segs(i), sample-major.
struct CarryArgs {
  void* dst[CARRY_MAX_TENSORS];
  const void* src[CARRY_MAX_TENSORS];
  int64_t bytes[CARRY_MAX_TENSORS];
  int32_t first[CARRY_MAX_TENSORS + 1];
  int32_t n_tensors, n_samples;
};

__global__ __launch_bounds__(CARRY_THREADS) void state_carry_masked_kernel(const CarryArgs a, const int32_t* __restrict__ mode) {
  // a workgroup = one (tensor, sample, segment); everything up to the walk is uniform (scalar registers)
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < a.n_tensors && b >= a.first[t + 1]) ++t;
  const int local = b - a.first[t];
  const int segs = (a.first[t + 1] - a.first[t]) / a.n_samples;
  const int smp = local / segs, seg = local - smp * segs;  // (smp < n_samples: the grid is exactly first[n_tensors] workgroups)
  const int m = mode[smp];
  if (m != 1 && m != 2) return;  // HOLD (and any other word): this sample's bytes are neither read nor written
  const int64_t nv = a.bytes[t] >> 4;
  uint4* __restrict__ d = (uint4*)((char*)a.dst[t] + (int64_t)smp * a.bytes[t]);
  const int64_t stride = (int64_t)segs * CARRY_THREADS;
  int64_t i = (int64_t)seg * CARRY_THREADS + threadIdx.x;
  if (m == 2) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (; i < nv; i += stride) d[i] = z;
    return;
  }
  if (a.src[t] == nullptr) return;  // (TAKE without a source moves nothing: the entry point documents it)
  const uint4* __restrict__ s = (const uint4*)((const char*)a.src[t] + (int64_t)smp * a.bytes[t]);
  for (; i + (CARRY_UNROLL - 1) * stride < nv; i += CARRY_UNROLL * stride) {
    uint4 v[CARRY_UNROLL];
#pragma unroll
    for (int k = 0; k < CARRY_UNROLL; ++k) v[k] = s[i + k * stride];
#pragma unroll
    for (int k = 0; k < CARRY_UNROLL; ++k) d[i + k * stride] = v[k];
  }
  for (; i < nv; i += stride) d[i] = s[i];
}

// The indexed sibling: a workgroup = one (tensor, MOVE, segment); tensor i owns blocks [first[i], first[i + 1]) = n_moves x segs(i),
// move-major.  dst has n_dst records per tensor, src n_src.
struct MoveArgs {
  void* dst[CARRY_MAX_TENSORS];
  const void* src[CARRY_MAX_TENSORS];
  int64_t bytes[CARRY_MAX_TENSORS];
  int32_t first[CARRY_MAX_TENSORS + 1];
  int32_t n_tensors, n_moves, n_dst, n_src;
};

__global__ __launch_bounds__(CARRY_THREADS) void state_carry_indexed_kernel(const MoveArgs a, const int32_t* __restrict__ dst_index,
                                                                            const int32_t* __restrict__ src_index) {
  const int b = blockIdx.x;
  int t = 0;
  while (t + 1 < a.n_tensors && b >= a.first[t + 1]) ++t;
  const int local = b - a.first[t];
  const int segs = (a.first[t + 1] - a.first[t]) / a.n_moves;
  const int mv = local / segs, seg = local - mv * segs;  // (mv < n_moves: the grid is exactly first[n_tensors] workgroups)
  // the two index words, read once and range-checked in front of any vector access: no word takes the walk outside the two tensors
  const int di = dst_index[mv], si = src_index[mv];
  if ((unsigned)di >= (unsigned)a.n_dst) return;  // a skipped move (a padded slot): nothing read, nothing written
  const int64_t nv = a.bytes[t] >> 4;
  uint4* __restrict__ d = (uint4*)((char*)a.dst[t] + (int64_t)di * a.bytes[t]);
  const int64_t stride = (int64_t)segs * CARRY_THREADS;
  int64_t i = (int64_t)seg * CARRY_THREADS + threadIdx.x;
  if (si == -1) {  // ESS_CARRY_SRC_ZERO
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (; i < nv; i += stride) d[i] = z;
    return;
  }
  if ((unsigned)si >= (unsigned)a.n_src || a.src[t] == nullptr) return;  // (any other word, or no source: moves nothing)
  const uint4* __restrict__ s = (const uint4*)((const char*)a.src[t] + (int64_t)si * a.bytes[t]);
  for (; i + (CARRY_UNROLL - 1) * stride < nv; i += CARRY_UNROLL * stride) {
    uint4 v[CARRY_UNROLL];
#pragma unroll
    for (int k = 0; k < CARRY_UNROLL; ++k) v[k] = s[i + k * stride];
#pragma unroll
    for (int k = 0; k < CARRY_UNROLL; ++k) d[i + k * stride] = v[k];
  }
  for (; i < nv; i += stride) d[i] = s[i];
}

// Where each tensor's workgroups start, for `rows` records (samples / moves) per tensor -> the grid size.  Segments per record:
// ~CARRY_SEG_BYTES each, widened until the whole grid fits the block cap (a tensor keeps >= 1).  first: n_tensors + 1 entries; the
// last is only meaningful when the result fits an int32, which the callers check.
int64_t carry_grid(const int64_t* bytes, int n_tensors, int rows, int64_t total, int32_t* first) {
  int64_t seg_bytes = CARRY_SEG_BYTES;
  for (;;) {
    int64_t blocks = 0;
    for (int i = 0; i < n_tensors; ++i) blocks += ceil_div64(bytes[i], seg_bytes) * rows;
    if (blocks <= CARRY_MAX_BLOCKS || seg_bytes >= total) break;
    seg_bytes *= 2;
  }
  int64_t at = 0;
  for (int i = 0; i < n_tensors; ++i) {
    first[i] = (int32_t)at;
    at += ceil_div64(bytes[i], seg_bytes) * rows;
  }
  first[n_tensors] = (int32_t)at;
  return at;
}

}  // namespace

extern "C" int ess_state_carry_masked(void* const* dst, const void* const* src, const int64_t* bytes_per_sample, int32_t n_tensors,
                                      int32_t n_samples, const int32_t* mode, ess_stream_t stream) {
  ESS_CHECK_ARG(n_tensors >= 1 && n_tensors <= CARRY_MAX_TENSORS, "state_carry_masked: n_tensors=%d (1..%d)", (int)n_tensors, CARRY_MAX_TENSORS);
  ESS_CHECK_ARG(n_samples >= 1 && n_samples <= 65535, "state_carry_masked: n_samples=%d (1..65535)", (int)n_samples);
  ESS_CHECK_ARG(dst && bytes_per_sample && mode, "state_carry_masked: null dst / bytes_per_sample table or mode");
  CarryArgs a{};
  a.n_tensors = n_tensors;
  a.n_samples = n_samples;
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const int64_t nb = bytes_per_sample[i];
    ESS_CHECK_ARG(nb > 0 && (nb & 15) == 0, "state_carry_masked: bytes_per_sample[%d]=%lld is not a positive multiple of 16", i, (long long)nb);
    ESS_CHECK_ARG(dst[i] && (((uintptr_t)dst[i]) & 15) == 0, "state_carry_masked: dst[%d] is null or not 16-byte aligned", i);
    ESS_CHECK_ARG(!src || (src[i] && (((uintptr_t)src[i]) & 15) == 0), "state_carry_masked: src[%d] is null or not 16-byte aligned", i);
    if (src) {  // (the kernel's pointers are __restrict__: a record must not be copied onto itself or a neighbour)
      const uintptr_t d0 = (uintptr_t)dst[i], s0 = (uintptr_t)src[i], span = (uintptr_t)nb * (uintptr_t)n_samples;
      ESS_CHECK_ARG(d0 + span <= s0 || s0 + span <= d0, "state_carry_masked: dst[%d] and src[%d] overlap", i, i);
    }
    a.dst[i] = dst[i];
    a.src[i] = src ? src[i] : nullptr;
    a.bytes[i] = nb;
    total += nb;
  }
  const int64_t first = carry_grid(a.bytes, n_tensors, n_samples, total, a.first);
  ESS_CHECK_ARG(first < ((int64_t)1 << 31), "state_carry_masked: %lld workgroups do not fit one launch", (long long)first);
  hipLaunchKernelGGL(state_carry_masked_kernel, dim3((unsigned)first), dim3(CARRY_THREADS), 0, (hipStream_t)stream, a, mode);
  return ess_launch_status("state_carry_masked");
}

extern "C" int ess_state_carry_indexed(void* const* dst, const void* const* src, const int64_t* bytes_per_sample, int32_t n_tensors,
                                       int32_t n_dst_samples, int32_t n_src_samples, int32_t n_moves, const int32_t* dst_index,
                                       const int32_t* src_index, ess_stream_t stream) {
  ESS_CHECK_ARG(n_tensors >= 1 && n_tensors <= CARRY_MAX_TENSORS, "state_carry_indexed: n_tensors=%d (1..%d)", (int)n_tensors, CARRY_MAX_TENSORS);
  ESS_CHECK_ARG(n_dst_samples >= 1 && n_dst_samples <= 65535, "state_carry_indexed: n_dst_samples=%d (1..65535)", (int)n_dst_samples);
  ESS_CHECK_ARG(n_src_samples >= 1 && n_src_samples <= 65535, "state_carry_indexed: n_src_samples=%d (1..65535)", (int)n_src_samples);
  ESS_CHECK_ARG(n_moves >= 1 && n_moves <= 65535, "state_carry_indexed: n_moves=%d (1..65535)", (int)n_moves);
  ESS_CHECK_ARG(dst && bytes_per_sample && dst_index && src_index, "state_carry_indexed: null dst / bytes_per_sample table, dst_index or src_index");
  MoveArgs a{};
  a.n_tensors = n_tensors;
  a.n_moves = n_moves;
  a.n_dst = n_dst_samples;
  a.n_src = n_src_samples;
  int64_t total = 0;
  for (int i = 0; i < n_tensors; ++i) {
    const int64_t nb = bytes_per_sample[i];
    ESS_CHECK_ARG(nb > 0 && (nb & 15) == 0, "state_carry_indexed: bytes_per_sample[%d]=%lld is not a positive multiple of 16", i, (long long)nb);
    ESS_CHECK_ARG(dst[i] && (((uintptr_t)dst[i]) & 15) == 0, "state_carry_indexed: dst[%d] is null or not 16-byte aligned", i);
    ESS_CHECK_ARG(!src || (src[i] && (((uintptr_t)src[i]) & 15) == 0), "state_carry_indexed: src[%d] is null or not 16-byte aligned", i);
    if (src) {  // (the kernel's pointers are __restrict__: no dst record may be a src record or part of one)
      const uintptr_t d0 = (uintptr_t)dst[i], s0 = (uintptr_t)src[i];
      const uintptr_t dspan = (uintptr_t)nb * (uintptr_t)n_dst_samples, sspan = (uintptr_t)nb * (uintptr_t)n_src_samples;
      ESS_CHECK_ARG(d0 + dspan <= s0 || s0 + sspan <= d0, "state_carry_indexed: dst[%d] and src[%d] overlap", i, i);
    }
    a.dst[i] = dst[i];
    a.src[i] = src ? src[i] : nullptr;
    a.bytes[i] = nb;
    total += nb;
  }
  const int64_t first = carry_grid(a.bytes, n_tensors, n_moves, total, a.first);  // (n_moves in place of n_samples)
  ESS_CHECK_ARG(first < ((int64_t)1 << 31), "state_carry_indexed: %lld workgroups do not fit one launch", (long long)first);
  hipLaunchKernelGGL(state_carry_indexed_kernel, dim3((unsigned)first), dim3(CARRY_THREADS), 0, (hipStream_t)stream, a, dst_index, src_index);
  return ess_launch_status("state_carry_indexed");
}
