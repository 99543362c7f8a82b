// Event ingest for the captured multi-stream round: packed 16-byte event records (ess_event_ingest) or the raw event columns a
// camera delivers, one window per row (ess_event_ingest_columns) or windows named inside per-stream rings (ess_event_ingest_ring)
// -> the round's voxel grids, with a sum that does not depend on the order the events arrive in (include/ess_hip.h).  The sources
// differ in how an event is LOADED; what an event adds is one function per FLAVOUR: scatter_event (temporal: integer pixels, bilinear
// in time) for all three sources, scatter_event_trilinear (the DSEC grid: rectified float coordinates, eight corners) for the column
// and the ring source, which share ONE loader, event_scatter_columns_kernel<Flavour, RING>: a template on the flavour and on whether
// a window lies at the head of its row or anywhere inside a ring.  Two more flavours of that loader fill the reference loaders' other
// event representations (ess_event_*_rep): SeparateFlavour (2 * bins planes, the polarities kept apart) and HistogramFlavour (two
// planes of per-pixel counts, the time column not read); the finish kernels take a plane count, not a meaning.  Masked<Flavour>
// puts a per-sensor hot-pixel bit mask in front of any of the four (ess_event_ingest_masked: an event on a masked raw pixel never
// reaches the flavour); hot_pixel_mask_kernel turns the histogram's counts into such masks (ess_event_hot_pixel_mask).  A third
// source, the device event store (ess_event_scatter_store: windows at absolute 64-bit indices of one flat set of columns), hands
// the same four flavours its events through event_scatter_store_kernel, the ring loader's walk without a row or a wrap.
//
// Behind the scatter, one kernel per job: event_finish_kernel<VEC, TAP> turns sums into a grid and zeroes them where each sum has
// one reader -- the plain ingest (TAP false) and the loader finish at the identity geometry (TAP true); grid_map_kernel<VEC,
// IDENTITY, WINDOW> is the loader finish's crop / resize pass, with or without the training window.  One routine checks the
// arguments of every source's entry points (check_source), one drives both loader finishes (grid_finish), and the twelve column,
// ring and store entry points are wrappers that describe their call to one routine a source (ingest_call, store_call), which
// picks the flavour through one visitor (visit_flavour).
//
// voxel_temporal_kernel (voxel.hip) adds its fp32 contributions with fp32 global atomics: a voxel's value depends on which event
// got there first, two builds of one window differ in the last bits.  Here every contribution is the SAME fp32 value (the same
// double expressions, rounded to fp32 once), but it is added as a 64-bit integer: q = llrint(c * 2^40) into int64 acc[S][bins][H][W]
// with global_atomic_add_x2.  Integer addition is associative, so acc -- and out = (float)acc * 2^-40, one round-to-nearest
// conversion and an exact scaling -- is a pure function of the SET of events.  |c| in [2^-16, 1] is exact at this scale, a smaller
// one is off by at most 2^-41.  An event adds to a voxel at most once (its two halves go to two bins), each time at most 2^40 in
// magnitude, so capacity <= 2^22 events per stream keep |acc| <= 2^62: inside int64.
//
// Two launches, both shaped by the CAPACITY and the grid size alone, the per-stream event counts read on the device: no memset, no
// host-side size, no synchronisation -- a hipGraph captures them once and replays them for every round.  acc is zeroed once by its
// owner; the finish pass leaves it all zero again (it stores zeros back only where a sum was, so an empty region costs reads only).
#include "common.h"

namespace {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_EVENTS_PER_THREAD = 4;  // scatter: records a thread walks at full capacity, before the block cap widens it
constexpr int INGEST_MAX_BLOCKS_X = 1024;
constexpr int INGEST_QUADS_PER_THREAD = 4;  // finish: 4-voxel groups (2 x 16 B of acc, 16 B of out) per thread
constexpr int64_t INGEST_MAX_CAPACITY = (int64_t)1 << 22;
constexpr double INGEST_SCALE = 0x1p40;
constexpr float INGEST_INV_SCALE = 0x1p-40f;

// {double t; int16 x; int16 y; int32 p}, little endian, as one 16-byte word
__device__ __forceinline__ void unpack_record(const uint4 v, double& t, int& x, int& y, int& p) {
  t = __hiloint2double((int)v.y, (int)v.x);
  x = (int)(short)(v.z & 0xffffu);
  y = (int)(short)(v.z >> 16);
  p = (int)v.w;
}

__device__ __forceinline__ double record_time(const uint4* __restrict__ rec, int64_t e) {
  const uint4 v = rec[e];
  return __hiloint2double((int)v.y, (int)v.x);
}

// c -> q = llrint(c * 2^40): the product is exact in fp64 (24 significant bits, exponent shift), one rounding to the integer
__device__ __forceinline__ long long quantise(float c) { return __double2ll_rn((double)c * INGEST_SCALE); }

// One event's two contributions, whatever source it was loaded from: the fp64 expressions of voxel_temporal_kernel rounded to fp32,
// each added as a 64-bit integer.  p: +1 where the word equals 1, -1 otherwise.
__device__ __forceinline__ void scatter_event(double t, int xs, int ys, int p, double first, double dT, int nb, int H, int W, size_t plane,
                                              long long* __restrict__ g) {
#pragma clang fp contract(off)  // (no fused multiply-add may change a per-event value: the results are compared as bits)
  const double ts = ((double)(nb - 1) * (t - first)) / dT;
  if (!(xs < W && xs >= 0 && ys < H && ys >= 0 && ts >= 0 && ts < nb)) return;  // (a NaN time fails both comparisons)
  const int ti = (int)ts;
  const double dts = ts - ti;
  // |polarity| = 1: the record carries -1 / +1 (any other word counts as -1, so no record can leave the int64 range)
  const float left = (float)(1.0 - dts), right = (float)dts;
  const float sign = p == 1 ? 1.f : -1.f;
  long long* gp = g + (size_t)ys * W + xs;
  const long long ql = quantise(sign * left), qr = quantise(sign * right);
  // (ti < nb holds; a zero adds nothing)
  if (ql != 0) atomicAdd((unsigned long long*)(gp + (size_t)ti * plane), (unsigned long long)ql);
  if (ti + 1 < nb && qr != 0) atomicAdd((unsigned long long*)(gp + (size_t)(ti + 1) * plane), (unsigned long long)qr);
}

__global__ __launch_bounds__(INGEST_THREADS) void event_scatter_kernel(const uint4* __restrict__ records, const int32_t* __restrict__ counts,
                                                                       int64_t capacity, int nb, int H, int W,
                                                                       long long* __restrict__ acc) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const int cnt = counts[s];
  if (cnt <= 0) return;  // an empty window, or INGEST_KEEP: nothing of this stream is read
  const int64_t n = (int64_t)cnt < capacity ? (int64_t)cnt : capacity;
  const uint4* __restrict__ rec = records + (size_t)s * capacity;
  const double first = record_time(rec, 0);
  double dT = record_time(rec, n - 1) - first;
  if (dT == 0) dT = 1.0;
  const size_t plane = (size_t)H * W;
  long long* __restrict__ g = acc + (size_t)s * nb * plane;
  for (int64_t e = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * INGEST_THREADS) {
    double t;
    int xs, ys, p;
    unpack_record(rec[e], t, xs, ys, p);
    scatter_event(t, xs, ys, p, first, dT, nb, H, W, plane, g);
  }
}

// ---- the column source: t [S][stride] 8 bytes, x / y [S][stride] 2 bytes, p [S][stride] 1 byte per event, as a camera or a DSEC file
// delivers them.  formats[s] says how stream s's words are read (ESS_EVCOL_*): a device word, so one captured launch serves rounds
// whose streams change their formats.  stride is a multiple of COLUMN_GROUP * 4, so every row of every column starts 16-byte aligned
// and a lane's group of COLUMN_GROUP consecutive events -- 2 x 16 B of t, 8 B of x, 8 B of y, 4 B of p -- never reaches the stride.
typedef long long i64x2 __attribute__((ext_vector_type(2)));
constexpr int COLUMN_GROUP = 4;
constexpr int COLUMN_STRIDE_ALIGN = 16;
constexpr int EVCOL_T_I64 = 1, EVCOL_XY_U16 = 2;  // (ESS_EVCOL_T_I64, ESS_EVCOL_XY_U16 of include/ess_hip.h)

// an int64 time enters as (double)t: exact below 2^53
__device__ __forceinline__ double column_time(long long word, bool t_i64) { return t_i64 ? (double)word : __longlong_as_double(word); }

// a uint16 coordinate enters as its unsigned value (32768.. lie outside every grid: dropped, never wrapped)
__device__ __forceinline__ int column_coordinate(unsigned half, bool xy_u16) { return xy_u16 ? (int)half : (int)(short)half; }

// ---- the trilinear flavour: VoxelGrid.convert on coordinates that went through the camera's rectify map, as the DSEC loader builds
// its grids (the reference's behaviour restated, not its code).  One event adds up to eight contributions c, each the fp32 value of
// voxel_trilinear_kernel's expression sequence (voxel.hip) -- wx = value * (1 - |xl - xe|), wxy = wx * (1 - |yl - ye|),
// c = wxy * (1 - |tb - tn|) -- added as llrint(c * 2^40) like the temporal halves.  Every factor has magnitude <= 1 (a corner lies
// within 1 of its coordinate, but for a coordinate in (-2, -1], whose only corner in the grid is 0 or -0 away from -1: factor in
// (-1, 0]), so |c| <= 1, and an event's eight corners are eight distinct voxels: an event adds to a voxel at most once, at most
// 2^40 in magnitude, and capacity <= 2^22 events per stream keep |acc| <= 2^62 as above.
//
// The test in front of the conversions keeps exactly the events of which some corner can land in the grid under truncation toward
// zero: x0 = (int)xe lies in [-1, W - 1] iff -2 < xe < W (coordinates in (-2, -1] still reach column 0, with a weight <= 0: the
// reference's quirk, kept), and alike for ye and tn.  The comparisons are written so that NaN fails them: no NaN, infinity or value
// beyond int reaches a float -> int conversion.
__device__ __forceinline__ void scatter_event_trilinear(float xe, float ye, float tn, int p, int nb, int H, int W, size_t plane,
                                                        long long* __restrict__ g) {
#pragma clang fp contract(off)
  if (!(xe > -2.f && xe < (float)W && ye > -2.f && ye < (float)H && tn > -2.f && tn < (float)nb)) return;
  const float value = p == 1 ? 1.f : -1.f;  // 2 * pol - 1 with pol = (byte == 1)
  const int x0 = (int)xe, y0 = (int)ye, t0 = (int)tn;
#pragma unroll
  for (int dx = 0; dx < 2; ++dx) {
    const int xl = x0 + dx;
    if (xl < 0 || xl >= W) continue;
    const float wx = value * (1.f - fabsf((float)xl - xe));
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const int yl = y0 + dy;
      if (yl < 0 || yl >= H) continue;
      const float wxy = wx * (1.f - fabsf((float)yl - ye));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int tb = t0 + dt;
        if (tb < 0 || tb >= nb) continue;
        const long long q = quantise(wxy * (1.f - fabsf((float)tb - tn)));
        if (q != 0) atomicAdd((unsigned long long*)(g + (size_t)tb * plane + (size_t)yl * W + xl), (unsigned long long)q);
      }
    }
  }
}

// the rectify maps of a call: maps [n_maps][map_h][map_w] (x, y) pairs, map_of[slot] = the slot's map, RECTIFY_NONE or anything else
struct Rectify {
  const float2* maps;
  const int32_t* map_of;
  int n_maps, map_h, map_w;
};
constexpr int RECTIFY_NONE = -1;  // (ESS_RECTIFY_NONE of include/ess_hip.h)

// What the two column loaders hand their events to.  open(): the slot's own words beyond count and format, false: the slot counts as
// empty;  window(): the raw time words of the window's first and last event;  add(): one event's raw words.  READS_TIME false: the
// loader issues no load of the time column -- neither window()'s two words nor the groups' 2 x 16 B -- and hands add() a zero word.
struct TemporalFlavour {
  static constexpr bool READS_TIME = true;
  double first, dT;
  __device__ __forceinline__ bool open(int) { return true; }
  __device__ __forceinline__ void window(long long w_first, long long w_last, bool t_i64, int) {
#pragma clang fp contract(off)
    first = column_time(w_first, t_i64);
    dT = column_time(w_last, t_i64) - first;
    if (dT == 0) dT = 1.0;
  }
  __device__ __forceinline__ void add(long long tw, unsigned xh, unsigned yh, int p, bool t_i64, bool xy_u16, int nb, int H, int W,
                                      size_t plane, long long* __restrict__ g) const {
    scatter_event(column_time(tw, t_i64), column_coordinate(xh, xy_u16), column_coordinate(yh, xy_u16), p, first, dT, nb, H, W, plane, g);
  }
};

// ---- the two further event representations of the reference's loaders (generate_voxel_grid(separate_pol=True),
// generate_event_histogram; the behaviour restated, not the code).  The kernel's plane count nb is the representation's C.
//
// Separate polarity, C = 2 * bins planes [positive bins; negative bins]: scatter_event's window, validity test, bin and weights --
// left = fp32(1 - dts), right = fp32(dts) -- with NO sign (the reference adds |pol| * weight): a positive event (word == 1) adds to
// planes ti and ti + 1, any other to planes bins + ti and bins + ti + 1, the right half only where ti + 1 < bins.  An event adds to
// a voxel at most once (its two halves go to two planes), at most 2^40 in magnitude, and left + right = 1 up to rounding as for the
// signed grid: check_source's 2^22-event bound (|acc| <= 2^62) and the statistics pass's sum |acc| <= 2^62 hold as they stand.
struct SeparateFlavour {
  static constexpr bool READS_TIME = true;
  double first, dT;
  __device__ __forceinline__ bool open(int) { return true; }
  __device__ __forceinline__ void window(long long w_first, long long w_last, bool t_i64, int) {
#pragma clang fp contract(off)
    first = column_time(w_first, t_i64);
    dT = column_time(w_last, t_i64) - first;
    if (dT == 0) dT = 1.0;
  }
  __device__ __forceinline__ void add(long long tw, unsigned xh, unsigned yh, int p, bool t_i64, bool xy_u16, int nb, int H, int W,
                                      size_t plane, long long* __restrict__ g) const {
#pragma clang fp contract(off)
    const int bins = nb >> 1;  // (nb is even: the entry points refuse any other)
    const int xs = column_coordinate(xh, xy_u16), ys = column_coordinate(yh, xy_u16);
    const double ts = ((double)(bins - 1) * (column_time(tw, t_i64) - first)) / dT;
    if (!(xs < W && xs >= 0 && ys < H && ys >= 0 && ts >= 0 && ts < bins)) return;  // (a NaN time fails both comparisons)
    const int ti = (int)ts;
    const double dts = ts - ti;
    const float left = (float)(1.0 - dts), right = (float)dts;
    long long* gp = g + (size_t)(p == 1 ? ti : bins + ti) * plane + (size_t)ys * W + xs;
    const long long ql = quantise(left), qr = quantise(right);
    // (ti < bins holds: both planes lie inside the event's own half; a zero adds nothing)
    if (ql != 0) atomicAdd((unsigned long long*)gp, (unsigned long long)ql);
    if (ti + 1 < bins && qr != 0) atomicAdd((unsigned long long*)(gp + plane), (unsigned long long)qr);
  }
};

// The histogram, C = 2 planes [negative counts, positive counts]: every event inside [0, W) x [0, H) adds 2^40 -- one count -- to
// plane 1 where its polarity word equals 1, else to plane 0, whatever its time is (the time column is never loaded: 5 bytes an
// event instead of 13).  One add of exactly 2^40 per event: 2^22 events keep |acc| <= 2^62.  A coordinate outside the grid drops the
// event; the reference's x + width * y would wrap it into a neighbouring row or raise: not reproduced.
struct HistogramFlavour {
  static constexpr bool READS_TIME = false;
  __device__ __forceinline__ bool open(int) { return true; }
  __device__ __forceinline__ void add(long long, unsigned xh, unsigned yh, int p, bool, bool xy_u16, int, int H, int W, size_t plane,
                                      long long* __restrict__ g) const {
    const int xs = column_coordinate(xh, xy_u16), ys = column_coordinate(yh, xy_u16);
    if (!(xs < W && xs >= 0 && ys < H && ys >= 0)) return;
    atomicAdd((unsigned long long*)(g + (p == 1 ? plane : (size_t)0) + (size_t)ys * W + xs), (unsigned long long)INGEST_SCALE);
  }
};

struct TrilinearFlavour {
  static constexpr bool READS_TIME = true;
  const float2* map;  // the slot's map, nullptr: RECTIFY_NONE
  int map_h, map_w;
  long long w_first;
  float d_last, u_first, den, cm1;
  __device__ __forceinline__ bool open(int s, const Rectify r) {
    const int m = r.map_of[s];
    map_h = r.map_h;
    map_w = r.map_w;
    map = m >= 0 && m < r.n_maps ? r.maps + (size_t)m * r.map_h * r.map_w : nullptr;
    return m == RECTIFY_NONE || map != nullptr;  // any other map word: as an unknown format bit
  }
  // d = t - t_first in the column's own type (int64: the raw words, modulo 2^64; else fp64), rounded ONCE to fp32
  __device__ __forceinline__ float since_first(long long tw, bool t_i64) const {
#pragma clang fp contract(off)
    return t_i64 ? (float)(long long)((unsigned long long)tw - (unsigned long long)w_first)
                 : (float)(__longlong_as_double(tw) - __longlong_as_double(w_first));
  }
  // u = d / d_last, tn = ((C - 1) * (u - u_first)) / (u_last - u_first): a window whose last time equals its first gives 0 / 0 = NaN
  // for every event and an all-zero grid (there is no dT = 1 rescue in this flavour)
  __device__ __forceinline__ void window(long long first_word, long long last_word, bool t_i64, int nb) {
#pragma clang fp contract(off)
    w_first = first_word;
    d_last = since_first(last_word, t_i64);
    u_first = since_first(first_word, t_i64) / d_last;
    den = d_last / d_last - u_first;
    cm1 = (float)(nb - 1);
  }
  __device__ __forceinline__ void add(long long tw, unsigned xh, unsigned yh, int p, bool t_i64, bool xy_u16, int nb, int H, int W,
                                      size_t plane, long long* __restrict__ g) const {
#pragma clang fp contract(off)
    const int x = column_coordinate(xh, xy_u16), y = column_coordinate(yh, xy_u16);
    float xe = (float)x, ye = (float)y;
    if (map != nullptr) {
      if (x < 0 || x >= map_w || y < 0 || y >= map_h) return;  // a raw pixel outside the sensor the map was made for: dropped
      const float2 v = map[(size_t)y * map_w + x];
      xe = v.x;
      ye = v.y;
    }
    const float tn = (cm1 * (since_first(tw, t_i64) / d_last - u_first)) / den;
    scatter_event_trilinear(xe, ye, tn, p, nb, H, W, plane, g);
  }
};

// ---- hot-pixel masks: one more per-slot table, in FRONT of the flavour.  masks [n_masks][mask_h][mask_words] 32-bit words,
// mask_words = ceil(mask_w / 32), pixel (x, y) = bit x & 31 of word x >> 5 of row y, set: hot;  mask_of[slot] = the slot's mask,
// MASK_NONE or anything else (the slot counts as empty, as for an unknown map word).  mask_h x mask_w is the SENSOR's size.
struct Masks {
  const uint32_t* masks;
  const int32_t* mask_of;
  int n_masks, mask_h, mask_w;
};
constexpr int MASK_NONE = -1;  // (ESS_MASK_NONE of include/ess_hip.h)

// Any flavour behind a mask: an event whose RAW pixel lies inside the mask's rectangle with its bit set never reaches the flavour's
// add(); every other event reaches it with its words unchanged (one outside the rectangle is the flavour's to judge).  window() is
// the flavour's own: the time base comes from the window's first and last event whether they are hot or not -- the reference
// voxelises first and zeroes the pixel afterwards, so its time base counts hot events too.  A type of its own: the four flavours
// and their instantiations stay what they are.
template <class Flavour>
struct Masked {
  static constexpr bool READS_TIME = Flavour::READS_TIME;
  Flavour f;
  const uint32_t* mask;  // the slot's mask, nullptr: MASK_NONE
  int mask_h, mask_w, mask_words;
  template <class... Extra>
  __device__ __forceinline__ bool open(int s, const Masks m, const Extra... extra) {
    const int k = m.mask_of[s];
    mask_h = m.mask_h;
    mask_w = m.mask_w;
    mask_words = (m.mask_w + 31) >> 5;
    mask = k >= 0 && k < m.n_masks ? m.masks + (size_t)k * m.mask_h * mask_words : nullptr;
    if (!(k == MASK_NONE || mask != nullptr)) return false;
    return f.open(s, extra...);
  }
  __device__ __forceinline__ void window(long long w_first, long long w_last, bool t_i64, int nb) { f.window(w_first, w_last, t_i64, nb); }
  __device__ __forceinline__ void add(long long tw, unsigned xh, unsigned yh, int p, bool t_i64, bool xy_u16, int nb, int H, int W,
                                      size_t plane, long long* __restrict__ g) const {
    if (mask != nullptr) {
      const int x = column_coordinate(xh, xy_u16), y = column_coordinate(yh, xy_u16);
      if (x >= 0 && x < mask_w && y >= 0 && y < mask_h && ((mask[(size_t)y * mask_words + (x >> 5)] >> (x & 31)) & 1u) != 0) return;
    }
    f.add(tw, xh, yh, p, t_i64, xy_u16, nb, H, W, plane, g);
  }
};

// ---- counts -> mask (ess_event_hot_pixel_mask): a wave takes 64 consecutive x of one row of one sensor, every lane compares its
// pixel's count with the sensor's threshold, one wave-wide ballot packs the 64 answers into the row's two words, lanes 0 and 1
// store them with plain stores (the second only where the row has that word).  A lane at x >= W votes 0: REPLACE writes the tail
// bits as 0, OR leaves them.  No atomics, no memset; the launch follows from the sizes alone.
constexpr int MASK_REPLACE = 0, MASK_OR = 1;  // (ESS_MASK_REPLACE, ESS_MASK_OR of include/ess_hip.h)
constexpr int MASK_WAVES = INGEST_THREADS / 64;

// PLAIN: sums are plain counts, one plane a sensor (ess_event_count_mask: what ess_event_store_pixel_counts leaves), compared as they
// stand; else the histogram flavour's two planes at scale 2^40.
template <bool OR, bool PLAIN>
__global__ __launch_bounds__(INGEST_THREADS) void hot_pixel_mask_kernel(const long long* __restrict__ sums, const long long* __restrict__ thresholds,
                                                                        int H, int W, uint32_t* __restrict__ masks) {
  const int i = blockIdx.y;
  const long long thr = thresholds[i];
  if (thr < 0) return;  // this sensor's mask is neither read nor written
  const int chunks = (W + 63) >> 6, mask_words = (W + 31) >> 5;
  const int64_t c = (int64_t)blockIdx.x * MASK_WAVES + (threadIdx.x >> 6);  // (the same for a whole wave)
  if (c >= (int64_t)H * chunks) return;
  const int y = (int)(c / chunks), lane = threadIdx.x & 63;
  const int x0 = (int)(c % chunks) << 6, x = x0 + lane;
  const size_t plane = (size_t)H * W;
  const long long* __restrict__ s = sums + (size_t)i * (PLAIN ? 1 : 2) * plane + (size_t)y * W;
  bool hot = false;
  if constexpr (PLAIN) {
    if (x < W) hot = s[x] > thr;
  } else {
    if (x < W) hot = ((s[x] + s[plane + x]) >> 40) > thr;
  }
  const unsigned long long votes = __ballot(hot);
  const int word = (x0 >> 5) + lane;
  if (lane < 2 && word < mask_words) {
    uint32_t* __restrict__ m = masks + ((size_t)i * H + y) * mask_words + word;
    const uint32_t bits = (uint32_t)(votes >> (32 * lane));
    if constexpr (OR) *m |= bits;
    else *m = bits;
  }
}

// ---- the ring source (RING): the same four columns, [n_rows][ring], as per-stream RINGS that packets are appended to as they
// arrive.  A slot's window is counts[i] events of row rows[i] from position starts[i] on, modulo ring; all four words are device
// words.  A start is no multiple of COLUMN_GROUP, so a lane walks the aligned groups from starts - starts % COLUMN_GROUP on and masks
// the head of the first and the tail of the last: the loads stay 2 x 16 B, 8 B, 8 B, 4 B.  ring is a multiple of
// COLUMN_STRIDE_ALIGN, so no group straddles the wrap and the wrap falls between two groups; a full ring from an unaligned start
// reads its first group twice, once under each mask.
// The column source is the ring source with slot s's window at the head of row s -- rows, starts and n_rows are not read, nothing
// wraps, no head is masked -- and `ring` its stride: one loader serves both.
template <class Flavour, bool RING, class... Extra>
__global__ __launch_bounds__(INGEST_THREADS) void event_scatter_columns_kernel(const long long* __restrict__ t, const unsigned short* __restrict__ x,
                                                                               const unsigned short* __restrict__ y,
                                                                               const unsigned char* __restrict__ p,
                                                                               const int32_t* __restrict__ rows, const int32_t* __restrict__ starts,
                                                                               const int32_t* __restrict__ counts,
                                                                               const int32_t* __restrict__ formats, int64_t ring, int n_rows,
                                                                               int nb, int H, int W, long long* __restrict__ acc,
                                                                               const Extra... extra) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const int cnt = counts[s];
  const int fmt = formats[s];  // (read beside the count, not behind the test on it, like rows and starts: the scalar loads issue together)
  int r = s, start = 0;
  if constexpr (RING) {
    r = rows[s];
    start = starts[s];
  }
  if (cnt <= 0) return;  // an empty window, or INGEST_KEEP: nothing is read for this slot
  if ((fmt & ~(EVCOL_T_I64 | EVCOL_XY_U16)) != 0) return;  // an unknown format: as count 0
  if constexpr (RING)
    if (r < 0 || r >= n_rows || start < 0 || (int64_t)start >= ring) return;  // a row or a start outside the rings: as count 0
  Flavour f;
  if (!f.open(s, extra...)) return;
  const bool t_i64 = (fmt & EVCOL_T_I64) != 0, xy_u16 = (fmt & EVCOL_XY_U16) != 0;
  const int64_t n = (int64_t)cnt < ring ? (int64_t)cnt : ring;
  const size_t row = (size_t)r * ring;
  const long long* __restrict__ ts = t + row;
  int64_t last_at = (int64_t)start + n - 1;  // (< 2 * ring)
  if constexpr (RING)
    if (last_at >= ring) last_at -= ring;
  if constexpr (Flavour::READS_TIME) f.window(ts[start], ts[last_at], t_i64, nb);
  const size_t plane = (size_t)H * W;
  long long* __restrict__ g = acc + (size_t)s * nb * plane;
  const i64x2* __restrict__ t2 = (const i64x2*)ts;               // two events
  const uint2* __restrict__ x4 = (const uint2*)(x + row);        // COLUMN_GROUP events
  const uint2* __restrict__ y4 = (const uint2*)(y + row);
  const unsigned* __restrict__ p4 = (const unsigned*)(p + row);
  const int64_t head = start % COLUMN_GROUP, group0 = start / COLUMN_GROUP, ring_groups = ring / COLUMN_GROUP;
  const int64_t groups = (head + n + COLUMN_GROUP - 1) / COLUMN_GROUP;  // (<= ring_groups + 1; the last one may be partial)
  for (int64_t q = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; q < groups; q += (int64_t)gridDim.x * INGEST_THREADS) {
    int64_t at = group0 + q;  // (< 2 * ring_groups: one subtraction wraps it; every group lies inside the row)
    if constexpr (RING)
      if (at >= ring_groups) at -= ring_groups;
    i64x2 ta = {0, 0}, tb = {0, 0};
    if constexpr (Flavour::READS_TIME) {
      ta = t2[2 * at];
      tb = t2[2 * at + 1];
    }
    const uint2 xv = x4[at], yv = y4[at];
    const unsigned pv = p4[at];
    const long long tw[COLUMN_GROUP] = {ta[0], ta[1], tb[0], tb[1]};
    const unsigned xh[COLUMN_GROUP] = {xv.x & 0xffffu, xv.x >> 16, xv.y & 0xffffu, xv.y >> 16};
    const unsigned yh[COLUMN_GROUP] = {yv.x & 0xffffu, yv.x >> 16, yv.y & 0xffffu, yv.y >> 16};
#pragma unroll
    for (int j = 0; j < COLUMN_GROUP; ++j) {
      const int64_t k = q * COLUMN_GROUP + j - head;  // the event's number inside the window
      if (k < 0 || k >= n) continue;                  // (the head and the tail: loaded, inside the row, never summed)
      f.add(tw[j], xh[j], yh[j], (int)((pv >> (8 * j)) & 0xffu), t_i64, xy_u16, nb, H, W, plane, g);
    }
  }
}

__device__ __forceinline__ float dequantise(long long a) { return (float)a * INGEST_INV_SCALE; }

// the scatter grid: from the capacity alone (a captured launch), INGEST_EVENTS_PER_THREAD events a thread at full capacity
unsigned scatter_blocks(int64_t capacity) {
  const int64_t bx = ceil_div64(capacity, (int64_t)INGEST_THREADS * INGEST_EVENTS_PER_THREAD);
  return (unsigned)(bx > INGEST_MAX_BLOCKS_X ? INGEST_MAX_BLOCKS_X : bx);
}

// one launch for the column (RING false: rows, starts null, n_rows unused) and the ring source, in either flavour
template <class Flavour, bool RING, class... Extra>
void launch_scatter(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                    const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots, int32_t bins, int32_t height,
                    int32_t width, void* acc, hipStream_t st, const Extra... extra) {
  hipLaunchKernelGGL((event_scatter_columns_kernel<Flavour, RING, Extra...>), dim3(scatter_blocks(ring), (unsigned)n_slots),
                     dim3(INGEST_THREADS), 0, st, (const long long*)t, (const unsigned short*)x, (const unsigned short*)y,
                     (const unsigned char*)p, rows, starts, counts, formats, ring, (int)n_rows, (int)bins, (int)height, (int)width,
                     (long long*)acc, extra...);
}

// ---- the store source (ess_event_scatter_store): the same four columns as ONE flat set of `capacity` events, recordings laid one
// behind the other (a training split uploaded once).  A slot's window is counts[s] events from ABSOLUTE event index starts[s], an
// int64 device word; nothing wraps and there is no row.  The walk is the ring source's -- aligned groups of COLUMN_GROUP from
// starts - starts % COLUMN_GROUP on, the head of the first and the tail of the last masked, loads of 2 x 16 B, 8 B, 8 B, 4 B -- with
// every index, group number and offset 64-bit: total and capacity reach 2^40 events.  capacity is a multiple of COLUMN_STRIDE_ALIGN,
// so the last group of a window that ends on event total - 1 lies inside the columns.  A start < 0, start + count > total,
// count > window_capacity or an unknown format: as count 0.  A kernel of its own, not a third value of RING: the column and the ring
// instantiations of the loader above stay what they are.
constexpr int64_t STORE_MAX_CAPACITY = (int64_t)1 << 40;

template <class Flavour, class... Extra>
__global__ __launch_bounds__(INGEST_THREADS) void event_scatter_store_kernel(const long long* __restrict__ t, const unsigned short* __restrict__ x,
                                                                             const unsigned short* __restrict__ y,
                                                                             const unsigned char* __restrict__ p,
                                                                             const long long* __restrict__ starts,
                                                                             const int32_t* __restrict__ counts,
                                                                             const int32_t* __restrict__ formats, int64_t total,
                                                                             int64_t window_capacity, int nb, int H, int W,
                                                                             long long* __restrict__ acc, const Extra... extra) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const int cnt = counts[s];
  const int fmt = formats[s];
  const int64_t start = starts[s];
  if (cnt <= 0) return;  // an empty window: nothing is read for this slot
  if ((fmt & ~(EVCOL_T_I64 | EVCOL_XY_U16)) != 0) return;  // an unknown format: as count 0
  const int64_t n = cnt;
  if (start < 0 || n > window_capacity || start > total - n) return;  // a window outside the store or above the capacity: as count 0
  Flavour f;
  if (!f.open(s, extra...)) return;
  const bool t_i64 = (fmt & EVCOL_T_I64) != 0, xy_u16 = (fmt & EVCOL_XY_U16) != 0;
  if constexpr (Flavour::READS_TIME) f.window(t[start], t[start + n - 1], t_i64, nb);
  const size_t plane = (size_t)H * W;
  long long* __restrict__ g = acc + (size_t)s * nb * plane;
  const i64x2* __restrict__ t2 = (const i64x2*)t;         // two events
  const uint2* __restrict__ x4 = (const uint2*)x;         // COLUMN_GROUP events
  const uint2* __restrict__ y4 = (const uint2*)y;
  const unsigned* __restrict__ p4 = (const unsigned*)p;
  const int64_t head = start % COLUMN_GROUP, group0 = start / COLUMN_GROUP;
  const int64_t groups = (head + n + COLUMN_GROUP - 1) / COLUMN_GROUP;  // (the last one may be partial; it ends below capacity)
  for (int64_t q = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; q < groups; q += (int64_t)gridDim.x * INGEST_THREADS) {
    const int64_t at = group0 + q;
    i64x2 ta = {0, 0}, tb = {0, 0};
    if constexpr (Flavour::READS_TIME) {
      ta = t2[2 * at];
      tb = t2[2 * at + 1];
    }
    const uint2 xv = x4[at], yv = y4[at];
    const unsigned pv = p4[at];
    const long long tw[COLUMN_GROUP] = {ta[0], ta[1], tb[0], tb[1]};
    const unsigned xh[COLUMN_GROUP] = {xv.x & 0xffffu, xv.x >> 16, xv.y & 0xffffu, xv.y >> 16};
    const unsigned yh[COLUMN_GROUP] = {yv.x & 0xffffu, yv.x >> 16, yv.y & 0xffffu, yv.y >> 16};
#pragma unroll
    for (int j = 0; j < COLUMN_GROUP; ++j) {
      const int64_t k = q * COLUMN_GROUP + j - head;  // the event's number inside the window
      if (k < 0 || k >= n) continue;                  // (the head and the tail: loaded, inside the columns, never summed)
      f.add(tw[j], xh[j], yh[j], (int)((pv >> (8 * j)) & 0xffu), t_i64, xy_u16, nb, H, W, plane, g);
    }
  }
}

// the grid follows window_capacity, not the store's size
template <class Flavour, class... Extra>
void launch_scatter_store(const void* t, const void* x, const void* y, const void* p, const int64_t* starts, const int32_t* counts,
                          const int32_t* formats, int64_t total, int64_t window_capacity, int32_t n_slots, int32_t channels, int32_t height,
                          int32_t width, void* acc, hipStream_t st, const Extra... extra) {
  hipLaunchKernelGGL((event_scatter_store_kernel<Flavour, Extra...>), dim3(scatter_blocks(window_capacity), (unsigned)n_slots),
                     dim3(INGEST_THREADS), 0, st, (const long long*)t, (const unsigned short*)x, (const unsigned short*)y,
                     (const unsigned char*)p, (const long long*)starts, counts, formats, total, window_capacity, (int)channels,
                     (int)height, (int)width, (long long*)acc, extra...);
}

// ---- plain per-pixel counts of an index range of the store (ess_event_store_pixel_counts): job j counts the events begins[j] ..
// ends[j] - 1 (absolute int64 indices, device words; a range as long as the store, not a window: no 2^22 bound) into counts[j], int64
// [H][W], ONE per event whatever its polarity -- a whole recording's counts for a hot-pixel rule, which the histogram flavour's sums
// (2^40 an event) cannot hold beyond 2^22 events a pixel.  Only x and y are loaded, 4 bytes an event; the walk is
// event_scatter_store_kernel's -- aligned groups of COLUMN_GROUP, the head and the tail masked, every index 64-bit -- strided by the
// grid over the range.  A range outside [0, total], begin > end or an unknown format bit: the job counts nothing.
__global__ __launch_bounds__(INGEST_THREADS) void event_store_pixel_counts_kernel(const unsigned short* __restrict__ x,
                                                                                  const unsigned short* __restrict__ y,
                                                                                  const long long* __restrict__ begins,
                                                                                  const long long* __restrict__ ends,
                                                                                  const int32_t* __restrict__ formats, int64_t total, int H,
                                                                                  int W, long long* __restrict__ counts) {
  const int job = blockIdx.y;
  const int64_t begin = begins[job], end = ends[job];
  const int fmt = formats[job];
  if ((fmt & ~(EVCOL_T_I64 | EVCOL_XY_U16)) != 0) return;
  if (begin < 0 || begin >= end || end > total) return;  // (begin == end: nothing to count)
  const bool xy_u16 = (fmt & EVCOL_XY_U16) != 0;
  const int64_t n = end - begin;
  long long* __restrict__ c = counts + (size_t)job * H * W;
  const uint2* __restrict__ x4 = (const uint2*)x;  // COLUMN_GROUP events
  const uint2* __restrict__ y4 = (const uint2*)y;
  const int64_t head = begin % COLUMN_GROUP, group0 = begin / COLUMN_GROUP;
  const int64_t groups = (head + n + COLUMN_GROUP - 1) / COLUMN_GROUP;  // (the last one may be partial; it ends below capacity)
  for (int64_t q = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; q < groups; q += (int64_t)gridDim.x * INGEST_THREADS) {
    const uint2 xv = x4[group0 + q], yv = y4[group0 + q];
    const unsigned xh[COLUMN_GROUP] = {xv.x & 0xffffu, xv.x >> 16, xv.y & 0xffffu, xv.y >> 16};
    const unsigned yh[COLUMN_GROUP] = {yv.x & 0xffffu, yv.x >> 16, yv.y & 0xffffu, yv.y >> 16};
#pragma unroll
    for (int j = 0; j < COLUMN_GROUP; ++j) {
      const int64_t k = q * COLUMN_GROUP + j - head;  // the event's number inside the range
      if (k < 0 || k >= n) continue;
      const int xs = column_coordinate(xh[j], xy_u16), ys = column_coordinate(yh[j], xy_u16);
      if (!(xs < W && xs >= 0 && ys < H && ys >= 0)) continue;
      atomicAdd((unsigned long long*)(c + (size_t)ys * W + xs), 1ull);
    }
  }
}

// ---- the loader finish (ess_event_grid_finish): what the reference loaders do to a grid between voxelising it and handing it to
// the network -- normalise it over its non-zero voxels, cut rows, resize bilinearly, cut rows again -- from the int64 sums, so that
// the grid stays a pure function of the set of events.  Up to four launches, all shaped by the sizes alone:
//   grid_stats_kernel (when normalising): GRID_STATS_BLOCKS(src_per) workgroups a slot, each leaves {count, sum, sum of squares} of its
//     share of the slot's non-zero voxels in the workspace.  Count and sum are EXACT: f = (float)acc is an integer-valued float, so it
//     is summed as an int64 -- sum |f| <= (1 + 2^-24) sum |acc|, and sum |acc| <= 2^22 events x (sum |c| of an event <= 1: the two
//     temporal halves, the eight trilinear corners) x 2^40 = 2^62: inside int64.  The squares v * v of v = f * 2^-40 are exact in
//     fp64 (48 bits); their sum is rounded, in an order that the launch shape fixes: a thread's voxels in index order, the wave
//     butterfly, the waves in order.
//   grid_stats_finalize_kernel: a slot's partials added IN WORKGROUP ORDER (the scheme of loss.hip's mean losses: plain stores, no
//     atomic, no memset in front) -> the slot's GridStat: voxel_apply_kernel's (voxel.hip) case analysis and fp32 expressions.
//   grid_map_kernel: every output voxel reads its <= 4 taps of acc, dequantises and normalises each, blends.  Several outputs read
//     one sum, so the sums are cleared behind it by grid_clear_kernel -- but for the identity geometry, where each sum has one
//     reader: event_finish_kernel<VEC, TAP = true> maps and clears in one pass, with a tap where the plain ingest (TAP = false)
//     dequantises, and gives the plain ingest's bits where nothing is normalised.
constexpr int GRID_NORM_NONE = 0, GRID_NORM_UNBIASED = 1, GRID_NORM_POPULATION = 2;  // (ESS_GRID_NORM_* of include/ess_hip.h)
constexpr int GRID_STATS_MAX_BLOCKS = 64;
constexpr int GRID_STATS_PER_THREAD = 16;  // voxels a thread of the statistics pass walks before the block cap widens it

struct GridStat {  // 16 bytes a slot, at the head of the workspace
  float fm, fs;
  int32_t divide;  // (v - fm) / fs, else v - fm
  int32_t active;  // 0: the slot has no non-zero voxel (or nothing is normalised): v stays
};

// workgroups a slot in the statistics pass: from the slot's size alone, so a slot's partials -- and its bits -- are the same
// however many slots the call has
int grid_stats_blocks(int64_t src_per) {
  const int64_t bx = ceil_div64(src_per, (int64_t)INGEST_THREADS * GRID_STATS_PER_THREAD);
  return (int)(bx > GRID_STATS_MAX_BLOCKS ? GRID_STATS_MAX_BLOCKS : bx);
}

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  unsigned long long t = 0;
  for (int i = 0; i < INGEST_THREADS / 64; ++i) t += red[i];
  return t;
}

// partials: [n_slots][blocks][3] 8-byte words {count, sum of (float)acc as int64, sum of squares as fp64 bits}
// VEC: src_per is even, so every slot's acc starts 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(INGEST_THREADS) void grid_stats_kernel(const int32_t* __restrict__ counts, int64_t src_per,
                                                                    const long long* __restrict__ acc,
                                                                    unsigned long long* __restrict__ partials) {
  __shared__ double red[16];
  __shared__ unsigned long long redu[INGEST_THREADS / 64];
  const int s = blockIdx.y;
  if (counts[s] < 0) return;  // INGEST_KEEP: no statistics are read for this slot
  const long long* __restrict__ a = acc + (size_t)s * src_per;
  unsigned long long n = 0, sum = 0;  // (unsigned: a sum outside the stated bound wraps, it is not undefined)
  double sq = 0;
  auto add = [&](long long q) {
    if (q == 0) return;
    const float f = (float)q;
    const double v = (double)(f * INGEST_INV_SCALE);
    n += 1;
    sum += (unsigned long long)(long long)f;
    sq += v * v;
  };
  const int64_t stride = (int64_t)gridDim.x * INGEST_THREADS;
  const int64_t i0 = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x;
  if constexpr (VEC) {
    const i64x2* __restrict__ a2 = (const i64x2*)a;
    for (int64_t i = i0; i < (src_per >> 1); i += stride) {
      const i64x2 q = a2[i];
      add(q[0]);
      add(q[1]);
    }
  } else {
    for (int64_t i = i0; i < src_per; i += stride) add(a[i]);
  }
  n = block_sum_u64(n, redu);
  sum = block_sum_u64(sum, redu);
  sq = block_sum_d(sq, red);
  if (threadIdx.x == 0) {
    unsigned long long* __restrict__ w = partials + ((size_t)s * gridDim.x + blockIdx.x) * 3;
    w[0] = n;
    w[1] = sum;
    w[2] = (unsigned long long)__double_as_longlong(sq);
  }
}

// one thread a slot: the partials in workgroup order -> GridStat.  The expressions below are voxel_apply_kernel's, on exact n and sum,
// evaluated WITHOUT fused multiply-add: a slot whose non-zero voxels are all equal (one voxel, say) then has E[v^2] and mean^2 rounded
// alike and a population std of exactly 0, as the loader's own fp32 arithmetic gives it -- not the rounding residual of v^2.
__global__ __launch_bounds__(64) void grid_stats_finalize_kernel(const int32_t* __restrict__ counts, int n_slots, int blocks, int mode,
                                                                 const unsigned long long* __restrict__ partials,
                                                                 GridStat* __restrict__ stats) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n_slots || counts[s] < 0) return;
  unsigned long long cnt = 0, isum = 0;
  double sq = 0;
  for (int b = 0; b < blocks; ++b) {
    const unsigned long long* __restrict__ w = partials + ((size_t)s * blocks + b) * 3;
    cnt += w[0];
    isum += w[1];
    sq += __longlong_as_double((long long)w[2]);
  }
  GridStat r = {0.f, 1.f, 0, 0};
  if (cnt > 0) {
    const double n = (double)cnt;
    const double mean = ((double)(long long)isum * 0x1p-40) / n;
    float fm, fs;
    bool divide = true;
    if (mode == GRID_NORM_UNBIASED) {
      // torch.std(): sqrt(sum((v-mean)^2) / (n-1)); one non-zero voxel -> NaN -> "std > 0" is false -> subtract only
      const double var = n > 1 ? (sq - n * mean * mean) / (n - 1) : -1.0;
      const double sd = var > 0 ? sqrt(var) : 0.0;
      divide = sd > 0;
      fm = (float)mean;
      fs = (float)sd;
    } else {
      fm = (float)mean;
      fs = sqrtf((float)(sq / n) - fm * fm);
    }
    r = GridStat{fm, fs, divide ? 1 : 0, 1};
  }
  stats[s] = r;
}

// one tap: the dequantised sum, normalised where it is not zero
__device__ __forceinline__ float grid_tap(long long q, const GridStat st) {
#pragma clang fp contract(off)
  const float v = dequantise(q);
  if (st.active == 0 || v == 0.f) return v;
  return st.divide ? (v - st.fm) / st.fs : v - st.fm;
}

struct GridGeometry {
  int bins, src_h, src_w;  // the slot's sums
  int in_h;                // rows [0, in_h) of them enter the resize
  int rh, rw;              // the resized grid
  int out_rows;            // rows [0, out_rows) of it are stored
  float scale_y, scale_x;  // (in - 1) / (out - 1), 0 where out == 1: fp32 divisions, as torch's area_pixel_compute_scale
};

// torch's align_corners=True source index and weights of output index d (fp32, no contraction); i0 is clamped into the source
// (the product can exceed in - 1 by an ulp, never by one: the clamp changes no value, it only bounds the index)
__device__ __forceinline__ void grid_source(float scale, int d, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  const float src = scale * (float)d;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// zeros where a sum was; VEC: src_per is even
template <bool VEC>
__global__ __launch_bounds__(INGEST_THREADS) void grid_clear_kernel(const int32_t* __restrict__ counts, int64_t src_per,
                                                                    long long* __restrict__ acc) {
  const int s = blockIdx.y;
  if (counts[s] < 0) return;  // INGEST_KEEP: acc of this slot is zero and stays so
  long long* __restrict__ a = acc + (size_t)s * src_per;
  const int64_t stride = (int64_t)gridDim.x * INGEST_THREADS;
  const int64_t i0 = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x;
  if constexpr (VEC) {
    i64x2* __restrict__ a2 = (i64x2*)a;
    const i64x2 z = {0, 0};
    for (int64_t i = i0; i < (src_per >> 1); i += stride) {
      const i64x2 q = a2[i];
      if ((q[0] | q[1]) != 0) a2[i] = z;
    }
  } else {
    for (int64_t i = i0; i < src_per; i += stride)
      if (a[i] != 0) a[i] = 0;
  }
}

// The finish of a slot whose every sum has one reader: out = the sum dequantised (the plain ingest) or, TAP, tapped (the loader
// finish at the identity geometry: the same bits where st.active == 0), and zeros stored back where a sum was.  stats is read only
// under TAP.  VEC: per_stream is a multiple of 4, so every stream's acc / out rows start 16-byte aligned
template <bool VEC, bool TAP>
__global__ __launch_bounds__(INGEST_THREADS) void event_finish_kernel(const int32_t* __restrict__ counts, int64_t per_stream,
                                                                      long long* __restrict__ acc, float* __restrict__ out,
                                                                      const GridStat* __restrict__ stats) {
  const int s = blockIdx.y;
  if (counts[s] < 0) return;  // INGEST_KEEP: the grid already in `out` is the caller's; acc of this stream is zero and stays so
  const GridStat st = TAP && stats != nullptr ? stats[s] : GridStat{0.f, 1.f, 0, 0};
  auto value = [&](long long q) {
    if constexpr (TAP) return grid_tap(q, st);
    else return dequantise(q);
  };
  long long* __restrict__ a = acc + (size_t)s * per_stream;
  float* __restrict__ o = out + (size_t)s * per_stream;
  const int64_t stride = (int64_t)gridDim.x * INGEST_THREADS;
  const int64_t i0 = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x;
  if constexpr (VEC) {
    i64x2* __restrict__ a2 = (i64x2*)a;
    f32x4* __restrict__ o4 = (f32x4*)o;
    const i64x2 z = {0, 0};
    for (int64_t i = i0; i < (per_stream >> 2); i += stride) {
      const i64x2 lo = a2[2 * i], hi = a2[2 * i + 1];
      f32x4 v;
      v[0] = value(lo[0]); v[1] = value(lo[1]); v[2] = value(hi[0]); v[3] = value(hi[1]);
      o4[i] = v;
      if ((lo[0] | lo[1]) != 0) a2[2 * i] = z;
      if ((hi[0] | hi[1]) != 0) a2[2 * i + 1] = z;
    }
  } else {
    for (int64_t i = i0; i < per_stream; i += stride) {
      const long long q = a[i];
      o[i] = value(q);
      if (q != 0) a[i] = 0;
    }
  }
}

// the grid of a pass over `items` items a slot, INGEST_QUADS_PER_THREAD a thread before the block cap widens it
dim3 grid_pass(int64_t items, int32_t n_slots) {
  int64_t bx = ceil_div64(items, (int64_t)INGEST_THREADS * INGEST_QUADS_PER_THREAD);
  if (bx > INGEST_MAX_BLOCKS_X) bx = INGEST_MAX_BLOCKS_X;
  return dim3((unsigned)bx, (unsigned)n_slots);
}

// the status of the launch in front, named "<entry point>(<stage>)" (the name is put together only for a launch that failed)
int stage_status(const char* what, const char* stage) {
  if (hipPeekAtLastError() == hipSuccess) return ESS_OK;
  char name[64];
  snprintf(name, sizeof name, "%s(%s)", what, stage);
  return ess_launch_status(name);
}

// TAP false: the plain ingest's finish (stats unused);  true: the loader finish at the identity geometry (stats null: nothing normalised)
template <bool TAP>
void launch_finish(const int32_t* counts, int32_t n_slots, int64_t per, void* acc, const GridStat* stats, float* out, hipStream_t st) {
  const bool vec = (per & 3) == 0;
  const dim3 grid = grid_pass(vec ? per >> 2 : per, n_slots);
  if (vec)
    hipLaunchKernelGGL((event_finish_kernel<true, TAP>), grid, dim3(INGEST_THREADS), 0, st, counts, per, (long long*)acc, out, stats);
  else
    hipLaunchKernelGGL((event_finish_kernel<false, TAP>), grid, dim3(INGEST_THREADS), 0, st, counts, per, (long long*)acc, out, stats);
}

// torch's area_pixel_compute_scale<float>(in, out, align_corners=true)
float grid_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// ---- the training window (ess_event_grid_finish_window, ess_label_window): the loaders' horizontal flip and random crop, applied
// where the grid (and its label) is written.  One row of `words` = (flip, y0, x0, reserved) serves a group of slots (the T windows
// of a sample) and the sample's label; the device clamps it, so no word reads or writes outside a slot.
struct Window {
  int y0, x0;  // the window's first row and column in the FLIPPED grid
  bool flip;
};

__device__ __forceinline__ Window window_of(const int32_t* __restrict__ words, int group, int grid_h, int grid_w, int win_h, int win_w) {
  const int32_t* __restrict__ w = words + (size_t)group * 4;
  int y0 = w[1], x0 = w[2];
  y0 = y0 < 0 ? 0 : (y0 > grid_h - win_h ? grid_h - win_h : y0);
  x0 = x0 < 0 ? 0 : (x0 > grid_w - win_w ? grid_w - win_w : x0);
  return Window{y0, x0, w[0] != 0};
}

// The map pass of the loader finish.  Call g [bins][out_rows][rw] the loader's grid: every voxel reads its <= 4 taps of acc (IDENTITY,
// no crop and no resize: its one sum), dequantises and normalises each, blends.  WINDOW: out[b][y][x] =
// g[b][y0 + y][flip ? rw - 1 - (x0 + x) : x0 + x], the same expressions evaluated for the window's voxels alone; else the window is
// the whole grid, unflipped, and words .. win_width are not read (the identity geometry then goes to event_finish_kernel: each sum
// has one reader).  The sums stay; grid_clear_kernel runs behind it.
// VEC: win_w is a multiple of 4, so every row of out starts 16-byte aligned and a thread stores four neighbours at once
template <bool VEC, bool IDENTITY, bool WINDOW>
__global__ __launch_bounds__(INGEST_THREADS) void grid_map_kernel(const int32_t* __restrict__ counts, const GridGeometry g,
                                                                  const int32_t* __restrict__ words, int slots_per_group, int win_height,
                                                                  int win_width, const long long* __restrict__ acc,
                                                                  const GridStat* __restrict__ stats, float* __restrict__ out) {
#pragma clang fp contract(off)
  static_assert(WINDOW || !IDENTITY, "the identity geometry without a window is event_finish_kernel's");
  const int s = blockIdx.y;
  if (counts[s] < 0) return;  // INGEST_KEEP
  const GridStat st = stats != nullptr ? stats[s] : GridStat{0.f, 1.f, 0, 0};
  int win_h = g.out_rows, win_w = g.rw;
  Window win = {0, 0, false};
  if constexpr (WINDOW) {
    win_h = win_height;
    win_w = win_width;
    win = window_of(words, s / slots_per_group, g.out_rows, g.rw, win_h, win_w);
  }
  const size_t src_plane = (size_t)g.src_h * g.src_w;
  const long long* __restrict__ a = acc + (size_t)s * g.bins * src_plane;
  float* __restrict__ o = out + (size_t)s * g.bins * win_h * win_w;
  constexpr int PER = VEC ? 4 : 1;
  const int64_t row_items = win_w / PER;
  const int64_t items = (int64_t)g.bins * win_h * row_items;
  for (int64_t i = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * INGEST_THREADS) {
    const int xq = (int)(i % row_items);
    const int64_t br = i / row_items;  // bin * win_h + row
    const int oy = win.y0 + (int)(br % win_h), b = (int)(br / win_h);
    int y0 = oy, y1 = oy;
    float ly0 = 1.f, ly1 = 0.f;
    if constexpr (!IDENTITY) grid_source(g.scale_y, oy, g.in_h, y0, y1, ly0, ly1);
    const long long* __restrict__ r0 = a + (size_t)b * src_plane + (size_t)y0 * g.src_w;
    const long long* __restrict__ r1 = a + (size_t)b * src_plane + (size_t)y1 * g.src_w;
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int wx = win.x0 + xq * PER + j;
      const int ox = win.flip ? g.rw - 1 - wx : wx;  // (four neighbours of a flipped row: the same four of the grid, reversed)
      if constexpr (IDENTITY) {
        v[j] = grid_tap(r0[ox], st);
      } else {
        int x0, x1;
        float lx0, lx1;
        grid_source(g.scale_x, ox, g.src_w, x0, x1, lx0, lx1);
        const float v00 = grid_tap(r0[x0], st), v01 = grid_tap(r0[x1], st), v10 = grid_tap(r1[x0], st), v11 = grid_tap(r1[x1], st);
        v[j] = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
      }
    }
    if constexpr (VEC) {
      f32x4 w;
      w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
      ((f32x4*)o)[i] = w;  // (item i of the slot is its i-th group of four floats)
    } else {
      o[i] = v[0];
    }
  }
}

// the label's side: nearest resize [hs][ws] -> [rh][rw] by the integer rule s = min(d * in / out, in - 1), then the same flip and
// window; one int64 a thread
__global__ __launch_bounds__(INGEST_THREADS) void label_window_kernel(const unsigned char* __restrict__ src, int hs, int ws, int rh, int rw,
                                                                      const int32_t* __restrict__ words, int win_h, int win_w,
                                                                      long long* __restrict__ out) {
  const int s = blockIdx.y;
  const Window win = window_of(words, s, rh, rw, win_h, win_w);
  const unsigned char* __restrict__ a = src + (size_t)s * hs * ws;
  long long* __restrict__ o = out + (size_t)s * win_h * win_w;
  const int64_t items = (int64_t)win_h * win_w;
  for (int64_t i = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; i < items; i += (int64_t)gridDim.x * INGEST_THREADS) {
    const int dy = win.y0 + (int)(i / win_w);
    const int wx = win.x0 + (int)(i % win_w);
    const int dx = win.flip ? rw - 1 - wx : wx;
    int64_t sy = (int64_t)dy * hs / rh, sx = (int64_t)dx * ws / rw;
    if (sy > hs - 1) sy = hs - 1;
    if (sx > ws - 1) sx = ws - 1;
    o[i] = (long long)a[sy * ws + sx];
  }
}


// ---- the argument checks.  The three sources' entry points check one list; SourceNames holds the words their messages differ in,
// `what` names the entry point in every message.
struct SourceNames {
  const char* pointers;      // the source's own pointers, as the null message lists them
  const char* aligned;       // those of them that must be 16-byte aligned
  const char* n_name;        // how many grids the call fills
  const char* span_name;     // the events a row holds ...
  const char* span_unit;     // ... per what ...
  int span_low;              // ... and the least value the message names
  const char* multiple_why;  // why the span is a multiple of COLUMN_STRIDE_ALIGN; nullptr: it need not be
};
static_assert(COLUMN_STRIDE_ALIGN == 16 && COLUMN_GROUP == 4, "the texts below name them");
constexpr SourceNames SOURCE_RECORDS = {"records, counts", "records", "n_streams", "capacity", "stream", 1, nullptr};
constexpr SourceNames SOURCE_COLUMNS = {"t, x, y, p, counts, formats", "t, x, y, p", "n_streams", "stride", "stream", 1,
                                        "every stream's row of every column starts 16-byte aligned"};
constexpr SourceNames SOURCE_RING = {"t, x, y, p, rows, starts, counts, formats", "t, x, y, p", "n_slots", "ring", "row", 16,
                                     "every row of every column starts 16-byte aligned, no group of 4 events straddles the wrap"};

// given: none of the source's own pointers is null;  addresses: those that must be aligned, or-ed;  n_rows: 1 but for the rings;
// with_out false: the scatter-only entry points, which have no out
int check_source(const char* what, const SourceNames& k, bool given, uintptr_t addresses, int64_t span, int32_t n_rows, int32_t n,
                 int32_t bins, int32_t height, int32_t width, const void* acc, size_t acc_bytes, const float* out, bool with_out = true) {
  ESS_CHECK_ARG(given && acc && (out || !with_out), "%s: null %s%s", what, k.pointers, with_out ? ", acc or out" : " or acc");
  ESS_CHECK_ARG(n >= 1 && n <= 65535, "%s: %s=%d (1..65535)", what, k.n_name, (int)n);
  ESS_CHECK_ARG(n_rows >= 1, "%s: n_rows=%d must be positive", what, (int)n_rows);
  ESS_CHECK_ARG(bins > 0 && height > 0 && width > 0, "%s: bins=%d height=%d width=%d must be positive", what, (int)bins, (int)height,
                (int)width);
  ESS_CHECK_ARG(span >= 1 && span <= INGEST_MAX_CAPACITY,
                "%s: %s=%lld events per %s (%d..%lld: the int64 sums hold 2^22 contributions of magnitude 1 at scale 2^40)", what,
                k.span_name, (long long)span, k.span_unit, k.span_low, (long long)INGEST_MAX_CAPACITY);
  ESS_CHECK_ARG(k.multiple_why == nullptr || span % COLUMN_STRIDE_ALIGN == 0, "%s: %s=%lld must be a multiple of %d (%s)", what,
                k.span_name, (long long)span, COLUMN_STRIDE_ALIGN, k.multiple_why);
  const size_t need = ess_event_ingest_workspace(n, bins, height, width);
  ESS_CHECK_ARG(acc_bytes >= need, "%s: acc has %zu bytes, %zu are needed", what, acc_bytes, need);
  ESS_CHECK_ARG(((addresses | (uintptr_t)acc | (uintptr_t)out) & 15) == 0, "%s: %s, acc%s must be 16-byte aligned", what, k.aligned,
                with_out ? " and out" : "");
  return ESS_OK;
}

// the training window's arguments of ess_event_grid_finish_window
struct WindowArgs {
  const int32_t* words;
  int32_t slots_per_group, win_height, win_width;
};

// The loader finish behind ess_event_grid_finish (win null) and ess_event_grid_finish_window: the checks, the statistics, the map --
// event_finish_kernel where every sum has one reader, else grid_map_kernel and the clear as a pass of its own.  With a window the
// map computes the window's voxels alone, so some sums may have no reader: the clear always runs.
int grid_finish(const char* what, const int32_t* counts, int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width, void* acc,
                size_t acc_bytes, int32_t crop_rows, int32_t resize_height, int32_t resize_width, int32_t out_rows, int32_t normalize,
                const WindowArgs* win, float* out, void* workspace, size_t workspace_bytes, hipStream_t st) {
  ESS_CHECK_ARG(counts && acc && out && workspace && (!win || win->words), "%s: null counts, acc, out%s", what,
                win ? ", workspace or words" : " or workspace");
  ESS_CHECK_ARG(n_slots >= 1 && n_slots <= 65535, "%s: n_slots=%d (1..65535)", what, (int)n_slots);
  ESS_CHECK_ARG(bins > 0 && src_height > 0 && src_width > 0, "%s: bins=%d src_height=%d src_width=%d must be positive", what, (int)bins,
                (int)src_height, (int)src_width);
  ESS_CHECK_ARG(resize_height > 0 && resize_width > 0, "%s: resize_height=%d resize_width=%d must be positive", what, (int)resize_height,
                (int)resize_width);
  ESS_CHECK_ARG(crop_rows >= 1 && crop_rows <= src_height, "%s: crop_rows=%d (1..src_height=%d)", what, (int)crop_rows, (int)src_height);
  ESS_CHECK_ARG(out_rows >= 1 && out_rows <= resize_height, "%s: out_rows=%d (1..resize_height=%d)", what, (int)out_rows,
                (int)resize_height);
  ESS_CHECK_ARG(normalize == GRID_NORM_NONE || normalize == GRID_NORM_UNBIASED || normalize == GRID_NORM_POPULATION,
                "%s: normalize=%d (0 none, 1 unbiased, 2 population)", what, (int)normalize);
  if (win) {
    ESS_CHECK_ARG(win->slots_per_group >= 1, "%s: slots_per_group=%d must be positive", what, (int)win->slots_per_group);
    ESS_CHECK_ARG(win->win_height >= 1 && win->win_height <= out_rows, "%s: win_height=%d (1..out_rows=%d)", what, (int)win->win_height,
                  (int)out_rows);
    ESS_CHECK_ARG(win->win_width >= 1 && win->win_width <= resize_width, "%s: win_width=%d (1..resize_width=%d)", what,
                  (int)win->win_width, (int)resize_width);
  }
  const size_t need = ess_event_ingest_workspace(n_slots, bins, src_height, src_width);
  ESS_CHECK_ARG(acc_bytes >= need, "%s: acc has %zu bytes, %zu are needed", what, acc_bytes, need);
  const size_t ws_need = ess_event_grid_finish_workspace(n_slots, bins, src_height, src_width);
  ESS_CHECK_ARG(workspace_bytes >= ws_need, "%s: workspace has %zu bytes, %zu are needed", what, workspace_bytes, ws_need);
  ESS_CHECK_ARG(((((uintptr_t)acc) | ((uintptr_t)out) | ((uintptr_t)workspace)) & 15) == 0,
                "%s: acc, out and workspace must be 16-byte aligned", what);
  ESS_CHECK_ARG(!win || (((uintptr_t)win->words) & 3) == 0, "%s: words must be 4-byte aligned", what);
  const int64_t src_per = (int64_t)bins * src_height * src_width;
  GridStat* stats = nullptr;
  int rc;
  if (normalize != GRID_NORM_NONE) {
    stats = (GridStat*)workspace;
    unsigned long long* partials = (unsigned long long*)(stats + n_slots);
    const int blocks = grid_stats_blocks(src_per);
    const dim3 sgrid((unsigned)blocks, (unsigned)n_slots);
    if ((src_per & 1) == 0)
      hipLaunchKernelGGL(grid_stats_kernel<true>, sgrid, dim3(INGEST_THREADS), 0, st, counts, src_per, (const long long*)acc, partials);
    else
      hipLaunchKernelGGL(grid_stats_kernel<false>, sgrid, dim3(INGEST_THREADS), 0, st, counts, src_per, (const long long*)acc, partials);
    rc = stage_status(what, "statistics");
    if (rc) return rc;
    hipLaunchKernelGGL(grid_stats_finalize_kernel, dim3((unsigned)ceil_div(n_slots, 64)), dim3(64), 0, st, counts, (int)n_slots, blocks,
                       (int)normalize, (const unsigned long long*)partials, stats);
    rc = stage_status(what, "finalize");
    if (rc) return rc;
  }
  const bool identity = crop_rows == src_height && resize_height == src_height && out_rows == src_height && resize_width == src_width;
  if (identity && !win) {  // each sum has one reader: map and clear in one kernel
    launch_finish<true>(counts, n_slots, src_per, acc, stats, out, st);
    return stage_status(what, "identity");
  }
  const GridGeometry g = {bins,         src_height, src_width, crop_rows, resize_height, resize_width, out_rows,
                          grid_scale(crop_rows, resize_height), grid_scale(src_width, resize_width)};
  const WindowArgs w = win ? *win : WindowArgs{nullptr, 1, out_rows, resize_width};
  const bool vec = (w.win_width & 3) == 0;
  const dim3 grid = grid_pass((int64_t)bins * w.win_height * (vec ? w.win_width >> 2 : w.win_width), n_slots);
#define ESS_LAUNCH_MAP(VEC, IDENTITY, WINDOW)                                                                                   \
  hipLaunchKernelGGL((grid_map_kernel<VEC, IDENTITY, WINDOW>), grid, dim3(INGEST_THREADS), 0, st, counts, g, w.words,              \
                     (int)w.slots_per_group, (int)w.win_height, (int)w.win_width, (const long long*)acc, (const GridStat*)stats, out)
  if (!win && vec) ESS_LAUNCH_MAP(true, false, false);
  else if (!win) ESS_LAUNCH_MAP(false, false, false);
  else if (vec && identity) ESS_LAUNCH_MAP(true, true, true);
  else if (vec) ESS_LAUNCH_MAP(true, false, true);
  else if (identity) ESS_LAUNCH_MAP(false, true, true);
  else ESS_LAUNCH_MAP(false, false, true);
#undef ESS_LAUNCH_MAP
  rc = stage_status(what, "map");
  if (rc) return rc;
  const bool cvec = (src_per & 1) == 0;
  const dim3 cgrid = grid_pass(cvec ? src_per >> 1 : src_per, n_slots);
  if (cvec)
    hipLaunchKernelGGL(grid_clear_kernel<true>, cgrid, dim3(INGEST_THREADS), 0, st, counts, src_per, (long long*)acc);
  else
    hipLaunchKernelGGL(grid_clear_kernel<false>, cgrid, dim3(INGEST_THREADS), 0, st, counts, src_per, (long long*)acc);
  return stage_status(what, "clear");
}

}  // namespace

extern "C" size_t ess_event_ingest_workspace(int32_t n_streams, int32_t bins, int32_t height, int32_t width) {
  if (n_streams <= 0 || bins <= 0 || height <= 0 || width <= 0) return 0;
  return (size_t)n_streams * bins * height * width * sizeof(long long);
}

extern "C" int ess_event_ingest(const void* records, const int32_t* counts, int64_t capacity, int32_t n_streams, int32_t bins,
                                int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out, ess_stream_t stream) {
  int rc = check_source("event_ingest", SOURCE_RECORDS, records && counts, (uintptr_t)records, capacity, 1, n_streams, bins, height, width,
                        acc, acc_bytes, out);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(event_scatter_kernel, dim3(scatter_blocks(capacity), (unsigned)n_streams), dim3(INGEST_THREADS), 0, st,
                     (const uint4*)records, counts, capacity, bins, height, width, (long long*)acc);
  rc = ess_launch_status("event_ingest(scatter)");
  if (rc) return rc;
  launch_finish<false>(counts, n_streams, (int64_t)bins * height * width, acc, nullptr, out, st);
  return ess_launch_status("event_ingest(finish)");
}

// ---- the column, ring and store entry points.  Twelve of them -- two sources with or without rows, the trilinear flavour, the
// representations (`channels` planes a slot and a word that picks the flavour), the scatter-only halves (acc keeps the sums for
// ess_event_grid_finish*), hot-pixel masks -- are ONE description of a call (IngestCall, StoreCall) carried out by ONE routine a
// source (ingest_call, store_call): the checks in the order that decides which refusal a caller sees, the flavour picked by one
// visitor (visit_flavour), the launch, and the plain finish exactly where there is an out.  An entry point fills the description.
namespace {

constexpr int EVENT_REP_SIGNED = 0, EVENT_REP_SEPARATE = 1, EVENT_REP_HISTOGRAM = 2;  // (ESS_EVENT_REP_* of include/ess_hip.h)
constexpr int STORE_SIGNED = 0, STORE_SEPARATE = 1, STORE_HISTOGRAM = 2, STORE_TRILINEAR = 3;  // (ESS_EVENT_STORE_* of include/ess_hip.h)
static_assert(STORE_SIGNED == EVENT_REP_SIGNED && STORE_SEPARATE == EVENT_REP_SEPARATE && STORE_HISTOGRAM == EVENT_REP_HISTOGRAM,
              "the first three flavour words are the representation words");
constexpr int MASK_MAX_SIDE = 32768;

// (in front of check_source, which sizes the workspace from `channels` where the signed entry points pass bins)
int check_representation(const char* what, int32_t representation, int32_t channels) {
  ESS_CHECK_ARG(channels > 0, "%s: channels=%d must be positive", what, (int)channels);
  ESS_CHECK_ARG(representation == EVENT_REP_SIGNED || representation == EVENT_REP_SEPARATE || representation == EVENT_REP_HISTOGRAM,
                "%s: representation=%d (0 signed, 1 separate polarity, 2 histogram)", what, (int)representation);
  ESS_CHECK_ARG(representation != EVENT_REP_SEPARATE || channels % 2 == 0,
                "%s: channels=%d must be even with representation=1 (separate polarity: 2 * bins planes)", what, (int)channels);
  ESS_CHECK_ARG(representation != EVENT_REP_HISTOGRAM || channels == 2,
                "%s: channels=%d must be 2 with representation=2 (histogram: negative counts, positive counts)", what, (int)channels);
  return ESS_OK;
}

// the rectify arguments of the trilinear flavour, as an entry point takes them -> the kernels' Rectify
struct RectifyArgs {
  const float* maps;
  const int32_t* map_of;
  int32_t n_maps, map_height, map_width;
};

int check_rectify(const char* what, const RectifyArgs& a, Rectify& r) {
  ESS_CHECK_ARG(a.map_of, "%s: null map_of", what);
  ESS_CHECK_ARG(a.n_maps >= 0, "%s: n_maps=%d must not be negative", what, (int)a.n_maps);
  ESS_CHECK_ARG((a.maps != nullptr) == (a.n_maps > 0), "%s: maps must be null with n_maps=0 and only then (n_maps=%d, maps %s)", what,
                (int)a.n_maps, a.maps ? "given" : "null");
  ESS_CHECK_ARG(a.map_height >= 1 && a.map_height <= 32768 && a.map_width >= 1 && a.map_width <= 32768,
                "%s: map_height=%d map_width=%d (1..32768 each: the sensor's size, whatever the grid's)", what, (int)a.map_height,
                (int)a.map_width);
  ESS_CHECK_ARG((((uintptr_t)a.maps) & 15) == 0, "%s: maps must be 16-byte aligned", what);
  r = Rectify{(const float2*)a.maps, a.map_of, a.n_maps, a.map_height, a.map_width};
  return ESS_OK;
}

// the mask arguments -> the kernels' Masks
struct MaskArgs {
  const uint32_t* masks;
  const int32_t* mask_of;
  int32_t n_masks, mask_height, mask_width;
};

int check_masks(const char* what, const MaskArgs& a, Masks& m) {
  ESS_CHECK_ARG(a.mask_of, "%s: null mask_of", what);
  ESS_CHECK_ARG(a.n_masks >= 0, "%s: n_masks=%d must not be negative", what, (int)a.n_masks);
  ESS_CHECK_ARG((a.masks != nullptr) == (a.n_masks > 0), "%s: masks must be null with n_masks=0 and only then (n_masks=%d, masks %s)", what,
                (int)a.n_masks, a.masks ? "given" : "null");
  ESS_CHECK_ARG(a.mask_height >= 1 && a.mask_height <= MASK_MAX_SIDE && a.mask_width >= 1 && a.mask_width <= MASK_MAX_SIDE,
                "%s: mask_height=%d mask_width=%d (1..32768 each: the sensor's size, whatever the grid's)", what, (int)a.mask_height,
                (int)a.mask_width);
  ESS_CHECK_ARG((((uintptr_t)a.masks) & 15) == 0, "%s: masks must be 16-byte aligned", what);
  m = Masks{a.masks, a.mask_of, a.n_masks, a.mask_height, a.mask_width};
  return ESS_OK;
}

// The one flavour ladder: (flavour word, masked?) -> launch(type tag, the kernel's Extra... in their order).  Every launch behind a
// mask is a Masked<Flavour> instantiation; without one the four flavours' own instantiations stay what they are.
template <class Flavour>
struct FlavourTag {
  using type = Flavour;
};

template <class Launch>
void visit_flavour(int32_t flavour, const Masks* m, const Rectify& r, Launch&& launch) {
  if (!m) {
    if (flavour == STORE_TRILINEAR) launch(FlavourTag<TrilinearFlavour>{}, r);
    else if (flavour == STORE_SEPARATE) launch(FlavourTag<SeparateFlavour>{});
    else if (flavour == STORE_HISTOGRAM) launch(FlavourTag<HistogramFlavour>{});
    else launch(FlavourTag<TemporalFlavour>{});
  } else if (flavour == STORE_TRILINEAR) launch(FlavourTag<Masked<TrilinearFlavour>>{}, *m, r);
  else if (flavour == STORE_SEPARATE) launch(FlavourTag<Masked<SeparateFlavour>>{}, *m);
  else if (flavour == STORE_HISTOGRAM) launch(FlavourTag<Masked<HistogramFlavour>>{}, *m);
  else launch(FlavourTag<Masked<TemporalFlavour>>{}, *m);
}

// The column / ring loader's sixteen instantiations, named in the order the code object has held them since each was added.  The
// visitor reaches every one of them whatever stands here; naming them first keeps their ORDER in the code object, and so the code
// object byte for byte, independent of the order the host code below happens to reach them in.  (The store loader's eight follow
// the visitor's order.)
template <class Flavour, bool RING, class... Extra>
const void* const LOADER = (const void*)&event_scatter_columns_kernel<Flavour, RING, Extra...>;
[[maybe_unused]] const void* const LOADERS[] = {
    LOADER<TemporalFlavour, false>, LOADER<TrilinearFlavour, false, Rectify>, LOADER<TemporalFlavour, true>,
    LOADER<TrilinearFlavour, true, Rectify>, LOADER<SeparateFlavour, true>, LOADER<HistogramFlavour, true>,
    LOADER<SeparateFlavour, false>, LOADER<HistogramFlavour, false>,
    LOADER<Masked<TrilinearFlavour>, true, Masks, Rectify>, LOADER<Masked<SeparateFlavour>, true, Masks>,
    LOADER<Masked<HistogramFlavour>, true, Masks>, LOADER<Masked<TemporalFlavour>, true, Masks>,
    LOADER<Masked<TrilinearFlavour>, false, Masks, Rectify>, LOADER<Masked<SeparateFlavour>, false, Masks>,
    LOADER<Masked<HistogramFlavour>, false, Masks>, LOADER<Masked<TemporalFlavour>, false, Masks>};

// what every flavoured call runs behind its source's own checks: the rectify and the mask arguments where the call has them
int check_flavour(const char* what, const RectifyArgs* rectify, const MaskArgs* masks, Rectify& r, Masks& m) {
  int rc = rectify ? check_rectify(what, *rectify, r) : ESS_OK;
  if (rc) return rc;
  return masks ? check_masks(what, *masks, m) : ESS_OK;
}

// ... and behind its launch: the scatter's status, and with an out the plain finish, the stages named in the status strings
int finish_call(const char* what, const int32_t* counts, int32_t n, int64_t per, void* acc, float* out, hipStream_t st) {
  if (!out) return ess_launch_status(what);
  int rc = stage_status(what, "scatter");
  if (rc) return rc;
  launch_finish<false>(counts, n, per, acc, nullptr, out, st);
  return stage_status(what, "finish");
}

// One column (ring false: rows, starts null, n_rows 1) or ring call.
struct IngestCall {
  const char* what;  // the entry point's name in every message
  bool ring;
  const void *t, *x, *y, *p;
  const int32_t *rows, *starts, *counts, *formats;
  int64_t span;  // stride / ring
  int32_t n_rows, n, planes, height, width;
  void* acc;
  size_t acc_bytes;
  float* out;
  bool with_out;      // false: scatter only -- an entry point without an out, or one whose out may be null and is
  int32_t flavour;    // a STORE_* word
  bool check_rep;     // check_representation runs (else a bad plane count is check_source's to report)
  const RectifyArgs* rectify;  // nullptr: the call has no rectify arguments (to check)
  const MaskArgs* masks;       // nullptr: an unmasked entry point
};

int ingest_call(const IngestCall& c, ess_stream_t stream) {
  int rc = c.check_rep ? check_representation(c.what, c.flavour, c.planes) : ESS_OK;
  if (rc) return rc;
  rc = check_source(c.what, c.ring ? SOURCE_RING : SOURCE_COLUMNS,
                    c.t && c.x && c.y && c.p && c.counts && c.formats && (!c.ring || (c.rows && c.starts)),
                    (uintptr_t)c.t | (uintptr_t)c.x | (uintptr_t)c.y | (uintptr_t)c.p, c.span, c.n_rows, c.n, c.planes, c.height, c.width,
                    c.acc, c.acc_bytes, c.out, c.with_out);
  if (rc) return rc;
  Rectify rect = {nullptr, nullptr, 0, 1, 1};
  Masks m;
  rc = check_flavour(c.what, c.rectify, c.masks, rect, m);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  visit_flavour(c.flavour, c.masks ? &m : nullptr, rect, [&](auto tag, auto... extra) {
    using Flavour = typename decltype(tag)::type;
    if (c.ring)
      launch_scatter<Flavour, true>(c.t, c.x, c.y, c.p, c.rows, c.starts, c.counts, c.formats, c.span, c.n_rows, c.n, c.planes, c.height,
                                    c.width, c.acc, st, extra...);
    else
      launch_scatter<Flavour, false>(c.t, c.x, c.y, c.p, nullptr, nullptr, c.counts, c.formats, c.span, 1, c.n, c.planes, c.height,
                                     c.width, c.acc, st, extra...);
  });
  return finish_call(c.what, c.counts, c.n, (int64_t)c.planes * c.height * c.width, c.acc, c.out, st);
}

// the store's own sizes, as every entry point that reads its columns takes them
int check_store_extent(const char* what, int64_t capacity, int64_t total) {
  ESS_CHECK_ARG(capacity >= COLUMN_STRIDE_ALIGN && capacity <= STORE_MAX_CAPACITY && capacity % COLUMN_STRIDE_ALIGN == 0,
                "%s: capacity=%lld events must be a multiple of %d in [%d, 2^40] (a window's last group of 4 events stays inside the columns)",
                what, (long long)capacity, COLUMN_STRIDE_ALIGN, COLUMN_STRIDE_ALIGN);
  ESS_CHECK_ARG(total >= 0 && total <= capacity, "%s: total=%lld events (0..capacity=%lld)", what, (long long)total, (long long)capacity);
  return ESS_OK;
}

// One store call.  Its list of checks differs from check_source's in texts and order (the store has a capacity, a total and a window
// capacity where a ring has a span), so it stays a list of its own; what follows it is ingest_call's.
struct StoreCall {
  const char* what;
  const void *t, *x, *y, *p;
  const int64_t* starts;
  const int32_t *counts, *formats;
  int64_t capacity, total, window_capacity;
  int32_t n, planes, height, width;
  void* acc;
  size_t acc_bytes;
  float* out;
  bool with_out;  // false: the scatter-only entry point, which has no out;  else out is nullable (NULL: scatter only)
  int32_t flavour;
  RectifyArgs rectify;    // read with STORE_TRILINEAR alone; with_out: given with any other flavour they are refused, else ignored
  const MaskArgs* masks;  // nullptr: the unmasked entry point
};

int store_call(const StoreCall& c, ess_stream_t stream) {
  const char* what = c.what;
  const bool trilinear = c.flavour == STORE_TRILINEAR;
  ESS_CHECK_ARG(c.flavour >= STORE_SIGNED && c.flavour <= STORE_TRILINEAR,
                "%s: flavour=%d (0 signed, 1 separate polarity, 2 histogram, 3 trilinear)", what, (int)c.flavour);
  int rc = check_representation(what, trilinear ? EVENT_REP_SIGNED : c.flavour, c.planes);
  if (rc) return rc;
  ESS_CHECK_ARG(c.t && c.x && c.y && c.p && c.starts && c.counts && c.formats && c.acc,
                "%s: null t, x, y, p, starts, counts, formats or acc", what);
  ESS_CHECK_ARG(c.n >= 1 && c.n <= 65535, "%s: n_slots=%d (1..65535)", what, (int)c.n);
  ESS_CHECK_ARG(c.height > 0 && c.width > 0, "%s: height=%d width=%d must be positive", what, (int)c.height, (int)c.width);
  ESS_CHECK_ARG(c.window_capacity >= 1 && c.window_capacity <= INGEST_MAX_CAPACITY,
                "%s: window_capacity=%lld events per window (1..%lld: the int64 sums hold 2^22 contributions of magnitude 1 at scale 2^40)",
                what, (long long)c.window_capacity, (long long)INGEST_MAX_CAPACITY);
  rc = check_store_extent(what, c.capacity, c.total);
  if (rc) return rc;
  const size_t need = ess_event_ingest_workspace(c.n, c.planes, c.height, c.width);
  ESS_CHECK_ARG(c.acc_bytes >= need, "%s: acc has %zu bytes, %zu are needed", what, c.acc_bytes, need);
  ESS_CHECK_ARG((((uintptr_t)c.t | (uintptr_t)c.x | (uintptr_t)c.y | (uintptr_t)c.p | (uintptr_t)c.acc | (uintptr_t)c.out) & 15) == 0 &&
                    (((uintptr_t)c.starts) & 7) == 0 && ((((uintptr_t)c.counts) | ((uintptr_t)c.formats)) & 3) == 0,
                "%s: t, x, y, p%s acc must be 16-byte, starts 8-byte, counts and formats 4-byte aligned", what,
                c.with_out ? ", out and" : " and");
  ESS_CHECK_ARG(!c.with_out || trilinear || (c.rectify.maps == nullptr && c.rectify.map_of == nullptr && c.rectify.n_maps == 0),
                "%s: maps, map_of and n_maps belong to flavour=3 (trilinear): flavour=%d needs them null and 0", what, (int)c.flavour);
  Rectify rect = {nullptr, nullptr, 0, 1, 1};
  Masks m;
  rc = check_flavour(what, trilinear ? &c.rectify : nullptr, c.masks, rect, m);
  if (rc) return rc;
  ESS_CHECK_ARG(!c.masks || (((uintptr_t)c.masks->mask_of) & 3) == 0, "%s: mask_of must be 4-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  visit_flavour(c.flavour, c.masks ? &m : nullptr, rect, [&](auto tag, auto... extra) {
    launch_scatter_store<typename decltype(tag)::type>(c.t, c.x, c.y, c.p, c.starts, c.counts, c.formats, c.total, c.window_capacity, c.n,
                                                       c.planes, c.height, c.width, c.acc, st, extra...);
  });
  return finish_call(what, c.counts, c.n, (int64_t)c.planes * c.height * c.width, c.acc, c.out, st);
}

}  // namespace

extern "C" int ess_event_ingest_columns(const void* t, const void* x, const void* y, const void* p, const int32_t* counts,
                                        const int32_t* formats, int64_t stride, int32_t n_streams, int32_t bins, int32_t height,
                                        int32_t width, void* acc, size_t acc_bytes, float* out, ess_stream_t stream) {
  return ingest_call({"event_ingest_columns", false, t, x, y, p, nullptr, nullptr, counts, formats, stride, 1, n_streams, bins, height, width,
                      acc, acc_bytes, out, true, STORE_SIGNED, false, nullptr, nullptr},
                     stream);
}

extern "C" int ess_event_ingest_columns_trilinear(const void* t, const void* x, const void* y, const void* p, const int32_t* counts,
                                                  const int32_t* formats, int64_t stride, int32_t n_streams, int32_t bins,
                                                  int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out,
                                                  const float* maps, const int32_t* map_of, int32_t n_maps, int32_t map_height,
                                                  int32_t map_width, ess_stream_t stream) {
  const RectifyArgs rect = {maps, map_of, n_maps, map_height, map_width};
  return ingest_call({"event_ingest_columns_trilinear", false, t, x, y, p, nullptr, nullptr, counts, formats, stride, 1, n_streams, bins,
                      height, width, acc, acc_bytes, out, true, STORE_TRILINEAR, false, &rect, nullptr},
                     stream);
}

extern "C" int ess_event_ingest_ring(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                                     const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots,
                                     int32_t bins, int32_t height, int32_t width, void* acc, size_t acc_bytes, float* out,
                                     ess_stream_t stream) {
  return ingest_call({"event_ingest_ring", true, t, x, y, p, rows, starts, counts, formats, ring, n_rows, n_slots, bins, height, width, acc,
                      acc_bytes, out, true, STORE_SIGNED, false, nullptr, nullptr},
                     stream);
}

extern "C" int ess_event_ingest_ring_trilinear(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                               const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring,
                                               int32_t n_rows, int32_t n_slots, int32_t bins, int32_t height, int32_t width, void* acc,
                                               size_t acc_bytes, float* out, const float* maps, const int32_t* map_of, int32_t n_maps,
                                               int32_t map_height, int32_t map_width, ess_stream_t stream) {
  const RectifyArgs rect = {maps, map_of, n_maps, map_height, map_width};
  return ingest_call({"event_ingest_ring_trilinear", true, t, x, y, p, rows, starts, counts, formats, ring, n_rows, n_slots, bins, height,
                      width, acc, acc_bytes, out, true, STORE_TRILINEAR, false, &rect, nullptr},
                     stream);
}

// the ring ingest in two halves: scatter alone (acc keeps the sums), and the loader finish that turns sums into the loader's grid
extern "C" int ess_event_scatter_ring(const void* t, const void* x, const void* y, const void* p, const int32_t* rows, const int32_t* starts,
                                      const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows, int32_t n_slots,
                                      int32_t bins, int32_t height, int32_t width, void* acc, size_t acc_bytes, ess_stream_t stream) {
  return ingest_call({"event_scatter_ring", true, t, x, y, p, rows, starts, counts, formats, ring, n_rows, n_slots, bins, height, width, acc,
                      acc_bytes, nullptr, false, STORE_SIGNED, false, nullptr, nullptr},
                     stream);
}

extern "C" int ess_event_scatter_ring_trilinear(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                                const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring,
                                                int32_t n_rows, int32_t n_slots, int32_t bins, int32_t height, int32_t width, void* acc,
                                                size_t acc_bytes, const float* maps, const int32_t* map_of, int32_t n_maps,
                                                int32_t map_height, int32_t map_width, ess_stream_t stream) {
  const RectifyArgs rect = {maps, map_of, n_maps, map_height, map_width};
  return ingest_call({"event_scatter_ring_trilinear", true, t, x, y, p, rows, starts, counts, formats, ring, n_rows, n_slots, bins, height,
                      width, acc, acc_bytes, nullptr, false, STORE_TRILINEAR, false, &rect, nullptr},
                     stream);
}

// the event representations: ESS_EVENT_REP_SIGNED launches the very kernel of the entry points above
extern "C" int ess_event_scatter_ring_rep(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                          const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring,
                                          int32_t n_rows, int32_t n_slots, int32_t channels, int32_t height, int32_t width, void* acc,
                                          size_t acc_bytes, int32_t representation, ess_stream_t stream) {
  return ingest_call({"event_scatter_ring_rep", true, t, x, y, p, rows, starts, counts, formats, ring, n_rows, n_slots, channels, height,
                      width, acc, acc_bytes, nullptr, false, representation, true, nullptr, nullptr},
                     stream);
}

extern "C" int ess_event_ingest_ring_rep(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                         const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring,
                                         int32_t n_rows, int32_t n_slots, int32_t channels, int32_t height, int32_t width, void* acc,
                                         size_t acc_bytes, float* out, int32_t representation, ess_stream_t stream) {
  return ingest_call({"event_ingest_ring_rep", true, t, x, y, p, rows, starts, counts, formats, ring, n_rows, n_slots, channels, height,
                      width, acc, acc_bytes, out, true, representation, true, nullptr, nullptr},
                     stream);
}

extern "C" int ess_event_ingest_columns_rep(const void* t, const void* x, const void* y, const void* p, const int32_t* counts,
                                            const int32_t* formats, int64_t stride, int32_t n_streams, int32_t channels, int32_t height,
                                            int32_t width, void* acc, size_t acc_bytes, float* out, int32_t representation,
                                            ess_stream_t stream) {
  return ingest_call({"event_ingest_columns_rep", false, t, x, y, p, nullptr, nullptr, counts, formats, stride, 1, n_streams, channels,
                      height, width, acc, acc_bytes, out, true, representation, true, nullptr, nullptr},
                     stream);
}

// hot-pixel masks: ONE entry point for both sources, all four flavours and both halves.  Its own checks stand in front of the
// routine's: which source the call names decides the texts of every check behind them.
extern "C" int ess_event_ingest_masked(const void* t, const void* x, const void* y, const void* p, const int32_t* rows,
                                       const int32_t* starts, const int32_t* counts, const int32_t* formats, int64_t ring, int32_t n_rows,
                                       int32_t n_slots, int32_t channels, int32_t height, int32_t width, void* acc, size_t acc_bytes,
                                       float* out, int32_t representation, int32_t trilinear, const float* maps, const int32_t* map_of,
                                       int32_t n_maps, int32_t map_height, int32_t map_width, const uint32_t* masks,
                                       const int32_t* mask_of, int32_t n_masks, int32_t mask_height, int32_t mask_width,
                                       ess_stream_t stream) {
  const char* what = "event_ingest_masked";
  int rc = check_representation(what, representation, channels);
  if (rc) return rc;
  ESS_CHECK_ARG(trilinear == 0 || trilinear == 1, "%s: trilinear=%d (0 integer pixels, 1 the trilinear flavour)", what, (int)trilinear);
  ESS_CHECK_ARG(!trilinear || representation == EVENT_REP_SIGNED,
                "%s: trilinear=1 builds the signed grid alone: representation=%d must be 0", what, (int)representation);
  ESS_CHECK_ARG((rows == nullptr) == (starts == nullptr),
                "%s: rows and starts are both given (the ring source) or both null (the column source): rows %s, starts %s", what,
                rows ? "given" : "null", starts ? "given" : "null");
  const bool is_ring = rows != nullptr;
  const RectifyArgs rect = {maps, map_of, n_maps, map_height, map_width};
  const MaskArgs mask = {masks, mask_of, n_masks, mask_height, mask_width};
  return ingest_call({what, is_ring, t, x, y, p, rows, starts, counts, formats, ring, is_ring ? n_rows : 1, n_slots, channels, height, width,
                      acc, acc_bytes, out, out != nullptr, trilinear ? STORE_TRILINEAR : representation, false, trilinear ? &rect : nullptr,
                      &mask},
                     stream);
}

// the store source: the four flavours, scatter only (acc keeps the sums for ess_event_grid_finish*) ...
extern "C" int ess_event_scatter_store(const void* t, const void* x, const void* y, const void* p, const int64_t* starts,
                                       const int32_t* counts, const int32_t* formats, int64_t capacity, int64_t total,
                                       int64_t window_capacity, int32_t n_slots, int32_t channels, int32_t height, int32_t width,
                                       void* acc, size_t acc_bytes, int32_t flavour, const float* maps, const int32_t* map_of,
                                       int32_t n_maps, int32_t map_height, int32_t map_width, ess_stream_t stream) {
  return store_call({"event_scatter_store", t, x, y, p, starts, counts, formats, capacity, total, window_capacity, n_slots, channels, height,
                     width, acc, acc_bytes, nullptr, false, flavour, {maps, map_of, n_maps, map_height, map_width}, nullptr},
                    stream);
}

// ... and behind hot-pixel masks, both halves: every launch a Masked<Flavour> instantiation of event_scatter_store_kernel; with out,
// the plain finish follows as behind the ring ingest
extern "C" int ess_event_ingest_store(const void* t, const void* x, const void* y, const void* p, const int64_t* starts,
                                      const int32_t* counts, const int32_t* formats, int64_t capacity, int64_t total,
                                      int64_t window_capacity, int32_t n_slots, int32_t channels, int32_t height, int32_t width, void* acc,
                                      size_t acc_bytes, float* out, int32_t flavour, const float* maps, const int32_t* map_of,
                                      int32_t n_maps, int32_t map_height, int32_t map_width, const uint32_t* masks, const int32_t* mask_of,
                                      int32_t n_masks, int32_t mask_height, int32_t mask_width, ess_stream_t stream) {
  const MaskArgs mask = {masks, mask_of, n_masks, mask_height, mask_width};
  return store_call({"event_ingest_store", t, x, y, p, starts, counts, formats, capacity, total, window_capacity, n_slots, channels, height,
                     width, acc, acc_bytes, out, true, flavour, {maps, map_of, n_maps, map_height, map_width}, &mask},
                    stream);
}

extern "C" int ess_event_store_pixel_counts(const void* x, const void* y, int64_t capacity, int64_t total, const int64_t* begins,
                                            const int64_t* ends, const int32_t* formats, int32_t n, int32_t height, int32_t width,
                                            int64_t* counts, ess_stream_t stream) {
  const char* what = "event_store_pixel_counts";
  ESS_CHECK_ARG(x && y && begins && ends && formats && counts, "%s: null x, y, begins, ends, formats or counts", what);
  ESS_CHECK_ARG(n >= 1 && n <= 65535, "%s: n=%d (1..65535)", what, (int)n);
  ESS_CHECK_ARG(height >= 1 && height <= MASK_MAX_SIDE && width >= 1 && width <= MASK_MAX_SIDE,
                "%s: height=%d width=%d (1..32768 each: the sensor's size)", what, (int)height, (int)width);
  int rc = check_store_extent(what, capacity, total);
  if (rc) return rc;
  ESS_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((((uintptr_t)begins) | ((uintptr_t)ends) | ((uintptr_t)counts)) & 7) == 0 &&
                    (((uintptr_t)formats) & 3) == 0,
                "%s: x and y must be 16-byte, begins, ends and counts 8-byte, formats 4-byte aligned", what);
  // the grid follows the store's capacity, capped as the scatters': a range of any length is strided over
  hipLaunchKernelGGL(event_store_pixel_counts_kernel, dim3(scatter_blocks(capacity), (unsigned)n), dim3(INGEST_THREADS), 0,
                     (hipStream_t)stream, (const unsigned short*)x, (const unsigned short*)y, (const long long*)begins,
                     (const long long*)ends, formats, total, (int)height, (int)width, (long long*)counts);
  return ess_launch_status(what);
}

namespace {
// counts -> masks behind ess_event_hot_pixel_mask (PLAIN false: the histogram flavour's two planes at scale 2^40) and
// ess_event_count_mask (PLAIN true: plain counts, one plane); sums_name: what the entry point calls its first argument
template <bool PLAIN>
int count_mask(const char* what, const char* sums_name, const int64_t* sums, int32_t n, int32_t height, int32_t width,
               const int64_t* thresholds, uint32_t* masks, int32_t mode, hipStream_t st) {
  ESS_CHECK_ARG(sums && thresholds && masks, "%s: null %s, thresholds or masks", what, sums_name);
  ESS_CHECK_ARG(n >= 1 && n <= 65535, "%s: n=%d (1..65535)", what, (int)n);
  ESS_CHECK_ARG(height >= 1 && height <= MASK_MAX_SIDE && width >= 1 && width <= MASK_MAX_SIDE,
                "%s: height=%d width=%d (1..32768 each: the sensor's size)", what, (int)height, (int)width);
  ESS_CHECK_ARG(mode == MASK_REPLACE || mode == MASK_OR, "%s: mode=%d (0 replace, 1 or)", what, (int)mode);
  ESS_CHECK_ARG(((((uintptr_t)sums) | ((uintptr_t)masks)) & 15) == 0 && (((uintptr_t)thresholds) & 7) == 0,
                "%s: %s and masks must be 16-byte, thresholds 8-byte aligned", what, sums_name);
  const int64_t chunks = (int64_t)height * ((width + 63) >> 6);  // (<= 2^24)
  const dim3 grid((unsigned)ceil_div64(chunks, (int64_t)MASK_WAVES), (unsigned)n);
  if (mode == MASK_OR)
    hipLaunchKernelGGL((hot_pixel_mask_kernel<true, PLAIN>), grid, dim3(INGEST_THREADS), 0, st, (const long long*)sums,
                       (const long long*)thresholds, (int)height, (int)width, masks);
  else
    hipLaunchKernelGGL((hot_pixel_mask_kernel<false, PLAIN>), grid, dim3(INGEST_THREADS), 0, st, (const long long*)sums,
                       (const long long*)thresholds, (int)height, (int)width, masks);
  return ess_launch_status(what);
}
}  // namespace

extern "C" int ess_event_hot_pixel_mask(const int64_t* sums, int32_t n, int32_t height, int32_t width, const int64_t* thresholds,
                                        uint32_t* masks, int32_t mode, ess_stream_t stream) {
  return count_mask<false>("event_hot_pixel_mask", "sums", sums, n, height, width, thresholds, masks, mode, (hipStream_t)stream);
}

// ess_event_hot_pixel_mask's rule on plain counts: int64 [n][height][width], no 2^40 scale, one plane
extern "C" int ess_event_count_mask(const int64_t* counts, int32_t n, int32_t height, int32_t width, const int64_t* thresholds,
                                    uint32_t* masks, int32_t mode, ess_stream_t stream) {
  return count_mask<true>("event_count_mask", "counts", counts, n, height, width, thresholds, masks, mode, (hipStream_t)stream);
}

// workspace: [n_slots] GridStat, then [n_slots][grid_stats_blocks][3] 8-byte partials
extern "C" size_t ess_event_grid_finish_workspace(int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width) {
  if (n_slots <= 0 || bins <= 0 || src_height <= 0 || src_width <= 0) return 0;
  const int64_t src_per = (int64_t)bins * src_height * src_width;
  return (size_t)n_slots * (sizeof(GridStat) + (size_t)grid_stats_blocks(src_per) * 3 * sizeof(unsigned long long));
}

extern "C" int ess_event_grid_finish(const int32_t* counts, int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width, void* acc,
                                     size_t acc_bytes, int32_t crop_rows, int32_t resize_height, int32_t resize_width, int32_t out_rows,
                                     int32_t normalize, float* out, void* workspace, size_t workspace_bytes, ess_stream_t stream) {
  return grid_finish("event_grid_finish", counts, n_slots, bins, src_height, src_width, acc, acc_bytes, crop_rows, resize_height,
                     resize_width, out_rows, normalize, nullptr, out, workspace, workspace_bytes, (hipStream_t)stream);
}

// ess_event_grid_finish with the training window fused into its map pass
extern "C" int ess_event_grid_finish_window(const int32_t* counts, int32_t n_slots, int32_t bins, int32_t src_height, int32_t src_width,
                                            void* acc, size_t acc_bytes, int32_t crop_rows, int32_t resize_height, int32_t resize_width,
                                            int32_t out_rows, int32_t normalize, const int32_t* words, int32_t slots_per_group,
                                            int32_t win_height, int32_t win_width, float* out, void* workspace, size_t workspace_bytes,
                                            ess_stream_t stream) {
  const WindowArgs win = {words, slots_per_group, win_height, win_width};
  return grid_finish("event_grid_finish_window", counts, n_slots, bins, src_height, src_width, acc, acc_bytes, crop_rows, resize_height,
                     resize_width, out_rows, normalize, &win, out, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int ess_label_window(const uint8_t* src, int32_t n, int32_t src_height, int32_t src_width, int32_t resize_height,
                                int32_t resize_width, const int32_t* words, int32_t win_height, int32_t win_width, int64_t* out,
                                ess_stream_t stream) {
  ESS_CHECK_ARG(src && words && out, "label_window: null src, words or out");
  ESS_CHECK_ARG(n >= 1 && n <= 65535, "label_window: n=%d (1..65535)", (int)n);
  ESS_CHECK_ARG(src_height > 0 && src_width > 0 && resize_height > 0 && resize_width > 0,
                "label_window: src_height=%d src_width=%d resize_height=%d resize_width=%d must be positive", (int)src_height,
                (int)src_width, (int)resize_height, (int)resize_width);
  ESS_CHECK_ARG(win_height >= 1 && win_height <= resize_height, "label_window: win_height=%d (1..resize_height=%d)", (int)win_height,
                (int)resize_height);
  ESS_CHECK_ARG(win_width >= 1 && win_width <= resize_width, "label_window: win_width=%d (1..resize_width=%d)", (int)win_width,
                (int)resize_width);
  ESS_CHECK_ARG(((((uintptr_t)words) & 3) | (((uintptr_t)out) & 7)) == 0, "label_window: words must be 4-byte, out 8-byte aligned");
  hipLaunchKernelGGL(label_window_kernel, grid_pass((int64_t)win_height * win_width, n), dim3(INGEST_THREADS), 0, (hipStream_t)stream,
                     (const unsigned char*)src, (int)src_height, (int)src_width, (int)resize_height, (int)resize_width, words,
                     (int)win_height, (int)win_width, (long long*)out);
  return ess_launch_status("label_window");
}
