// The window search of the device event store (ess_event_store_windows): a batch's sample table -> the B * T slot words starts
// (int64), counts, formats (and map_of) that ess_event_scatter_store and ess_event_grid_finish_window read (include/ess_hip.h).
// What the reference's loaders do between a file and the voxeliser -- EventSlicer's time -> index search, the cut of the last
// T * n events before it into T windows, or the T + 1 searches of the fixed-duration cut -- restated on the device, so that a
// captured graph serves batches whose samples change.  The host prepares every time bound (datasets.event_feed's rules: the
// recording's offset subtracted, a fractional bound on integer times raised to the next integer); the device only searches:
// "the first index in [begin, end) with t >= bound, end where there is none", comparing in the column's own type.
//
// One workgroup a sample, one WAVE a bound: a 64-ary search.  Each round the 64 lanes probe the last events of 64 equal chunks of
// the open range, one ballot counts the chunks that lie wholly before the bound, and the range narrows to the next chunk:
// ceil(log64) dependent loads -- 6 over 2^32 events, 7 over 2^40 -- where a binary search makes 32 or 40.  Times are
// non-decreasing inside a recording (the store refuses any other), so the votes of a round are monotone over the lanes.
// Every index is 64-bit.  No atomics, no memset, nothing read back; the launch follows from the sample count alone.
#include "common.h"

namespace {

constexpr int STORE_THREADS = 256;
constexpr int STORE_WAVES = STORE_THREADS / 64;
constexpr int EVCOL_T_I64 = 1, EVCOL_XY_U16 = 2;                            // (ESS_EVCOL_* of include/ess_hip.h)
constexpr int RULE_COUNT_TIME = 0, RULE_COUNT_INDEX = 1, RULE_DURATION = 2;  // (ESS_EVENT_STORE_RULE_*)
constexpr int FLAG_EMPTY = 1, FLAG_OVERFLOW = 2, FLAG_RANGE = 4;             // (ESS_EVENT_STORE_FLAG_*)
constexpr int TABLE_WORDS = 4;                                               // begin, end, format, reserved
constexpr int64_t STORE_MAX_CAPACITY = (int64_t)1 << 40;
constexpr int64_t WINDOW_MAX_CAPACITY = (int64_t)1 << 22;

__device__ __forceinline__ bool before(long long word, long long bound, bool t_i64) {
  return t_i64 ? word < bound : __longlong_as_double(word) < __longlong_as_double(bound);
}

// the first index in [lo, hi) with t >= bound, hi where there is none; the whole wave calls it with the same arguments.
// Kept true: every event before lo lies before the bound, and every event from hi on (inside the extent) does not.
__device__ __forceinline__ int64_t first_at_or_after(const long long* __restrict__ t, int64_t lo, int64_t hi, long long bound, bool t_i64) {
  const int lane = threadIdx.x & 63;
  while (hi > lo) {
    const int64_t step = (hi - lo + 63) >> 6;                 // events a chunk (>= 1): 64 chunks cover the range
    const int64_t probe = lo + (int64_t)lane * step + (step - 1);  // the lane's chunk's last event
    const bool less = probe < hi ? before(t[probe], bound, t_i64) : false;
    const int c = __popcll(__ballot(less));                   // the chunks 0 .. c - 1 lie wholly before the bound
    const int64_t next = lo + (int64_t)c * step;              // the answer is in chunk c, or is hi
    if (next >= hi) return hi;
    // chunk c's last event -- where it lies inside the range -- is at or after the bound: the answer is at most its index
    const int64_t last = next + step - 1;
    lo = next;
    hi = last < hi ? last : hi;
  }
  return lo;
}

__global__ __launch_bounds__(STORE_THREADS) void event_store_windows_kernel(const long long* __restrict__ t, int64_t total,
                                                                            const long long* __restrict__ table, int n_recordings,
                                                                            const int32_t* __restrict__ recording,
                                                                            const long long* __restrict__ bounds,
                                                                            const int32_t* __restrict__ sample_map, int T, int rule,
                                                                            int64_t n_per_window, int64_t window_capacity,
                                                                            long long* __restrict__ starts, int32_t* __restrict__ counts,
                                                                            int32_t* __restrict__ formats, int32_t* __restrict__ map_of,
                                                                            int32_t* __restrict__ flags) {
  __shared__ long long s_last;
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n_bounds = rule == RULE_DURATION ? T + 1 : 1;
  const long long* __restrict__ bd = bounds + (size_t)b * n_bounds;
  const size_t slot0 = (size_t)b * T;
  // every thread reads the sample's own words: what follows is decided alike by the whole workgroup
  const int rec = recording[b];
  long long begin = 0, end = 0, fmt = -1;
  if (rec >= 0 && rec < n_recordings) {
    const long long* __restrict__ row = table + (size_t)rec * TABLE_WORDS;
    begin = row[0];
    end = row[1];
    fmt = row[2];
  }
  bool fine = fmt >= 0 && (fmt & ~(long long)(EVCOL_T_I64 | EVCOL_XY_U16)) == 0 && begin >= 0 && begin <= end && end <= total;
  if (fine && rule == RULE_COUNT_INDEX) fine = bd[0] >= 0 && bd[0] <= end - begin;  // e, relative to the recording
  if (map_of != nullptr)
    for (int i = threadIdx.x; i < T; i += STORE_THREADS) map_of[slot0 + i] = sample_map[b];
  if (!fine) {  // an unused row, a recording outside the table, an e outside the recording: T empty windows
    for (int i = threadIdx.x; i < T; i += STORE_THREADS) {
      starts[slot0 + i] = 0;
      counts[slot0 + i] = 0;
      formats[slot0 + i] = 0;
    }
    if (threadIdx.x == 0) flags[b] = FLAG_RANGE;
    return;
  }
  const bool t_i64 = (fmt & EVCOL_T_I64) != 0;
  for (int i = threadIdx.x; i < T; i += STORE_THREADS) formats[slot0 + i] = (int32_t)fmt;
  if (rule == RULE_DURATION) {
    for (int j = wave; j <= T; j += STORE_WAVES) {
      const int64_t at = first_at_or_after(t, begin, end, bd[j], t_i64);
      if (lane == 0) {
        if (j < T) starts[slot0 + j] = at;
        else s_last = at;
      }
    }
    __syncthreads();  // (the starts other waves stored are read below)
    auto count_of = [&](int i) { return (i + 1 < T ? starts[slot0 + i + 1] : s_last) - starts[slot0 + i]; };
    int mine = 0;
    for (int i = threadIdx.x; i < T; i += STORE_THREADS) {
      const int64_t c = count_of(i);
      mine |= c < 0 ? FLAG_RANGE : (c > window_capacity ? FLAG_OVERFLOW : 0);  // (descending bounds: no cut of any loader)
      mine |= c > 0 ? 8 : 0;
    }
    // (__syncthreads_or answers "any thread's word is non-zero", not the or of the words: one question a bit)
    const bool descend = __syncthreads_or(mine & FLAG_RANGE) != 0, over = __syncthreads_or(mine & FLAG_OVERFLOW) != 0;
    const bool filled = __syncthreads_or(mine & 8) != 0;
    const int flag = descend ? FLAG_RANGE : (over ? FLAG_OVERFLOW : (filled ? 0 : FLAG_EMPTY));
    for (int i = threadIdx.x; i < T; i += STORE_THREADS) counts[slot0 + i] = (flag & (FLAG_RANGE | FLAG_OVERFLOW)) ? 0 : (int32_t)count_of(i);
    if (threadIdx.x == 0) flags[b] = flag;
    return;
  }
  // the count rules: e by one search or as given, then the last T * n_per_window events before it, clamped at begin
  int64_t e;
  if (rule == RULE_COUNT_INDEX) {
    e = begin + bd[0];  // (checked above: inside the recording)
  } else {
    if (wave == 0) {
      const int64_t at = first_at_or_after(t, begin, end, bd[0], t_i64);
      if (lane == 0) s_last = at;
    }
    __syncthreads();
    e = s_last;
  }
  const int64_t back = e - (int64_t)T * n_per_window;  // (T <= 65535, n_per_window <= 2^22: inside int64)
  const int64_t start = back > begin ? back : begin;
  const int64_t n = (e - start) / T;
  const int flag = n == 0 ? FLAG_EMPTY : (n > window_capacity ? FLAG_OVERFLOW : 0);
  for (int i = threadIdx.x; i < T; i += STORE_THREADS) {
    starts[slot0 + i] = start + (int64_t)i * n;
    counts[slot0 + i] = flag ? 0 : (int32_t)n;
  }
  if (threadIdx.x == 0) flags[b] = flag;
}

}  // namespace

extern "C" int ess_event_store_windows(const void* t, int64_t capacity, int64_t total, const int64_t* table, int32_t n_recordings,
                                       const int32_t* recording, const int64_t* bounds, const int32_t* sample_map, int32_t n_samples,
                                       int32_t T, int32_t rule, int64_t n_per_window, int64_t window_capacity, int64_t* starts,
                                       int32_t* counts, int32_t* formats, int32_t* map_of, int32_t* flags, ess_stream_t stream) {
  const char* what = "event_store_windows";
  ESS_CHECK_ARG(t && table && recording && bounds && starts && counts && formats && flags,
                "%s: null t, table, recording, bounds, starts, counts, formats or flags", what);
  ESS_CHECK_ARG((sample_map == nullptr) == (map_of == nullptr),
                "%s: sample_map and map_of are both given (the map words are passed through) or both null: sample_map %s, map_of %s", what,
                sample_map ? "given" : "null", map_of ? "given" : "null");
  ESS_CHECK_ARG(rule == RULE_COUNT_TIME || rule == RULE_COUNT_INDEX || rule == RULE_DURATION,
                "%s: rule=%d (0 count, end by time; 1 count, end by index; 2 duration)", what, (int)rule);
  ESS_CHECK_ARG(T >= 1, "%s: T=%d must be positive", what, (int)T);
  ESS_CHECK_ARG(n_samples >= 1 && (int64_t)n_samples * T <= 65535, "%s: n_samples=%d x T=%d = n_slots=%lld (1..65535)", what, (int)n_samples,
                (int)T, (long long)n_samples * T);
  ESS_CHECK_ARG(n_recordings >= 1, "%s: n_recordings=%d must be positive", what, (int)n_recordings);
  ESS_CHECK_ARG(window_capacity >= 1 && window_capacity <= WINDOW_MAX_CAPACITY,
                "%s: window_capacity=%lld events per window (1..%lld: the int64 sums hold 2^22 contributions of magnitude 1 at scale 2^40)",
                what, (long long)window_capacity, (long long)WINDOW_MAX_CAPACITY);
  ESS_CHECK_ARG(rule == RULE_DURATION || (n_per_window >= 1 && n_per_window <= window_capacity),
                "%s: n_per_window=%lld (1..window_capacity=%lld) with a count rule", what, (long long)n_per_window,
                (long long)window_capacity);
  ESS_CHECK_ARG(capacity >= 16 && capacity <= STORE_MAX_CAPACITY && capacity % 16 == 0,
                "%s: capacity=%lld events must be a multiple of 16 in [16, 2^40]", what, (long long)capacity);
  ESS_CHECK_ARG(total >= 0 && total <= capacity, "%s: total=%lld events (0..capacity=%lld)", what, (long long)total, (long long)capacity);
  ESS_CHECK_ARG((((uintptr_t)t) & 15) == 0 && ((((uintptr_t)table) | ((uintptr_t)bounds) | ((uintptr_t)starts)) & 7) == 0 &&
                    ((((uintptr_t)recording) | ((uintptr_t)sample_map) | ((uintptr_t)counts) | ((uintptr_t)formats) | ((uintptr_t)map_of) |
                      ((uintptr_t)flags)) & 3) == 0,
                "%s: t must be 16-byte, table, bounds and starts 8-byte, the int32 words 4-byte aligned", what);
  hipLaunchKernelGGL(event_store_windows_kernel, dim3((unsigned)n_samples), dim3(STORE_THREADS), 0, (hipStream_t)stream,
                     (const long long*)t, total, (const long long*)table, (int)n_recordings, recording, (const long long*)bounds, sample_map,
                     (int)T, (int)rule, n_per_window, window_capacity, (long long*)starts, counts, formats, map_of, flags);
  return ess_launch_status(what);
}
