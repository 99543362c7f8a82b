// Stand-alone host program: the argument checks of every entry point of voxel_ingest.hip -- the ingest from records, columns and
// rings in both flavours, the scatter-only ring calls, the three representation calls, the masked ingest (both sources, with and
// without out), the two store calls, the two loader finishes and the label window.  The checks all come in front
// of any launch, so no device is needed.  Meant to be built with the host sanitizers and run on its own (a library loaded into python
// is out of their reach):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -x hip ess_amd/csrc/voxel_ingest.hip tools/host_checks/event_ring_args_main.cpp \
//         -x none ess_amd/libess_hip.so -Wl,-rpath,$PWD/ess_amd -o event_ring_args
//   ./event_ring_args            (--texts: print every refusal's text as well, one a line, to compare two builds)
//
// voxel_ingest.hip -- the code under test -- is compiled into the program with the sanitizers; the built library only supplies the
// error text (api.cpp), and the program's own entry points take precedence over the library's.
// Every refused call must return ESS_EINVAL and leave a text in ess_last_error(); the pointers handed over are never dereferenced.
// Each entry point is refused at least once for a null pointer, a count out of range, a short acc (or workspace) and a misalignment.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ess_hip.h"

namespace {
int failures = 0, refusals = 0;
bool texts = false;

void expect_refused(int rc, const char* needle, const char* entry, const char* what) {
  const char* msg = ess_last_error();
  ++refusals;
  if (rc != -22 || !msg || !std::strstr(msg, needle) || !std::strstr(msg, entry)) {
    std::printf("FAIL %s, %s: rc=%d, message '%s' (wanted -22, '%s' and '%s')\n", entry, what, rc, msg ? msg : "(null)", entry, needle);
    ++failures;
  } else if (texts) {
    std::printf("%s | %s | %s\n", entry, what, msg);
  }
}

alignas(16) unsigned char block[64];
void* const a = block;  // 16-byte aligned, never read
const int32_t* const w = (const int32_t*)block;
const int32_t NB = 5, H = 24, W = 40;

// what a refusal changes of an otherwise good call: one pointer of each kind, the span (capacity / stride / ring), the count
// (n_streams / n_slots), acc's size, out
struct Args {
  const void* t = a;         // the source's first pointer (records / t)
  const void* p = a;         // its last column (the polarity bytes)
  const int32_t* words = w;  // its last device word (formats; the ring's rows too)
  int64_t span = 32;
  int32_t n_rows = 1, n = 1;
  void* acc = a;
  size_t acc_bytes = (size_t)NB * H * W * 8;
  void* out = a;
  const float* maps = nullptr;  // (n_maps = 0: maps must be null)
  const int32_t* map_of = w;
  int32_t channels = NB, representation = 0;  // (the _rep entry points: the signed grid of NB planes; the store's flavour word)
  // the masked ingest and the store calls alone
  const int32_t* rows = w;    // (the masked ring calls: words is their formats alone)
  const int32_t* starts = w;
  int32_t trilinear = 0;
  const uint32_t* masks = nullptr;  // (n_masks = 0: masks must be null)
  const int32_t* mask_of = w;
  int64_t capacity = 64, total = 48;  // the store's; span is its window_capacity
};

struct Source {
  const char* entry;
  const char* span;  // the span's name in the messages
  const char* n;     // the count's
  bool ring, with_out, rectify;
  int (*call)(const Args&);
  bool rep = false;           // takes channels and a representation word
  bool nullable_out = false;  // out NULL: scatter only, no refusal
  bool masked = false, store = false, paired = false;  // paired: the masked ingest with rows and starts
};

int masked(const Args& g, const int32_t* rows, const int32_t* starts, int32_t n_rows, void* out) {
  return ess_event_ingest_masked(g.t, a, a, g.p, rows, starts, w, g.words, g.span, n_rows, g.n, g.channels, H, W, g.acc, g.acc_bytes,
                                 (float*)out, g.representation, g.trilinear, g.maps, g.map_of, 0, 28, 44, g.masks, g.mask_of, 0, 28, 44,
                                 nullptr);
}

const Source SOURCES[] = {
    {"event_ingest:", "capacity=", "n_streams=", false, true, false,
     [](const Args& g) { return ess_event_ingest(g.t, g.words, g.span, g.n, NB, H, W, g.acc, g.acc_bytes, (float*)g.out, nullptr); }},
    {"event_ingest_columns:", "stride=", "n_streams=", false, true, false,
     [](const Args& g) {
       return ess_event_ingest_columns(g.t, a, a, g.p, w, g.words, g.span, g.n, NB, H, W, g.acc, g.acc_bytes, (float*)g.out, nullptr);
     }},
    {"event_ingest_columns_trilinear:", "stride=", "n_streams=", false, true, true,
     [](const Args& g) {
       return ess_event_ingest_columns_trilinear(g.t, a, a, g.p, w, g.words, g.span, g.n, NB, H, W, g.acc, g.acc_bytes, (float*)g.out,
                                                 g.maps, g.map_of, 0, 28, 44, nullptr);
     }},
    {"event_ingest_ring:", "ring=", "n_slots=", true, true, false,
     [](const Args& g) {
       return ess_event_ingest_ring(g.t, a, a, g.p, g.words, w, w, g.words, g.span, g.n_rows, g.n, NB, H, W, g.acc, g.acc_bytes,
                                    (float*)g.out, nullptr);
     }},
    {"event_ingest_ring_trilinear:", "ring=", "n_slots=", true, true, true,
     [](const Args& g) {
       return ess_event_ingest_ring_trilinear(g.t, a, a, g.p, g.words, w, w, g.words, g.span, g.n_rows, g.n, NB, H, W, g.acc, g.acc_bytes,
                                              (float*)g.out, g.maps, g.map_of, 0, 28, 44, nullptr);
     }},
    {"event_scatter_ring:", "ring=", "n_slots=", true, false, false,
     [](const Args& g) {
       return ess_event_scatter_ring(g.t, a, a, g.p, g.words, w, w, g.words, g.span, g.n_rows, g.n, NB, H, W, g.acc, g.acc_bytes, nullptr);
     }},
    {"event_scatter_ring_trilinear:", "ring=", "n_slots=", true, false, true,
     [](const Args& g) {
       return ess_event_scatter_ring_trilinear(g.t, a, a, g.p, g.words, w, w, g.words, g.span, g.n_rows, g.n, NB, H, W, g.acc, g.acc_bytes,
                                               g.maps, g.map_of, 0, 28, 44, nullptr);
     }},
    {"event_scatter_ring_rep:", "ring=", "n_slots=", true, false, false,
     [](const Args& g) {
       return ess_event_scatter_ring_rep(g.t, a, a, g.p, g.words, w, w, g.words, g.span, g.n_rows, g.n, g.channels, H, W, g.acc, g.acc_bytes,
                                         g.representation, nullptr);
     },
     true},
    {"event_ingest_ring_rep:", "ring=", "n_slots=", true, true, false,
     [](const Args& g) {
       return ess_event_ingest_ring_rep(g.t, a, a, g.p, g.words, w, w, g.words, g.span, g.n_rows, g.n, g.channels, H, W, g.acc, g.acc_bytes,
                                        (float*)g.out, g.representation, nullptr);
     },
     true},
    {"event_ingest_columns_rep:", "stride=", "n_streams=", false, true, false,
     [](const Args& g) {
       return ess_event_ingest_columns_rep(g.t, a, a, g.p, w, g.words, g.span, g.n, g.channels, H, W, g.acc, g.acc_bytes, (float*)g.out,
                                           g.representation, nullptr);
     },
     true},
    {"event_ingest_masked:", "ring=", "n_slots=", true, true, false,
     [](const Args& g) { return masked(g, g.rows, g.starts, g.n_rows, g.out); }, true, true, true, false, true},
    {"event_ingest_masked:", "ring=", "n_slots=", true, false, false,
     [](const Args& g) { return masked(g, g.rows, g.starts, g.n_rows, nullptr); }, true, true, true, false, true},
    {"event_ingest_masked:", "stride=", "n_streams=", false, true, false,
     [](const Args& g) { return masked(g, nullptr, nullptr, g.n_rows, g.out); }, true, true, true},
    {"event_ingest_masked:", "stride=", "n_streams=", false, false, false,
     [](const Args& g) { return masked(g, nullptr, nullptr, g.n_rows, nullptr); }, true, true, true},
    {"event_scatter_store:", "window_capacity=", "n_slots=", false, false, false,
     [](const Args& g) {
       return ess_event_scatter_store(g.t, a, a, g.p, (const int64_t*)a, w, g.words, g.capacity, g.total, g.span, g.n, g.channels, H, W, g.acc,
                                      g.acc_bytes, g.representation, g.maps, g.map_of, 0, 28, 44, nullptr);
     },
     false, false, false, true},
    {"event_ingest_store:", "window_capacity=", "n_slots=", false, true, false,
     [](const Args& g) {
       return ess_event_ingest_store(g.t, a, a, g.p, (const int64_t*)a, w, g.words, g.capacity, g.total, g.span, g.n, g.channels, H, W, g.acc,
                                     g.acc_bytes, (float*)g.out, g.representation, g.maps, g.representation == 3 ? g.map_of : nullptr, 0, 28, 44,
                                     g.masks, g.mask_of, 0, 28, 44, nullptr);
     },
     false, true, true, true},
};

template <class F>
Args with(F&& change) {
  Args g;
  change(g);
  return g;
}

void check_source(const Source& s) {
  auto refused = [&](const Args& g, const char* needle, const char* what) { expect_refused(s.call(g), needle, s.entry, what); };
  const char* aligned = s.store ? "must be 16-byte, starts 8-byte" : "16-byte aligned";
  refused(with([](Args& g) { g.t = nullptr; }), "null", "a null first pointer");
  refused(with([](Args& g) { g.words = nullptr; }), "null", "a null device word");
  refused(with([](Args& g) { g.acc = nullptr; }), "null", "a null acc");
  if (s.with_out && !s.nullable_out) refused(with([](Args& g) { g.out = nullptr; }), "null", "a null out");
  for (int32_t n : {0, -1, 65536}) refused(with([&](Args& g) { g.n = n; }), s.n, "a count out of range");
  const int64_t bad_spans[] = {0, -16, ((int64_t)1 << 22) + 16, INT64_MAX, INT64_MIN};
  for (int64_t span : bad_spans) refused(with([&](Args& g) { g.span = span; }), s.span, "a span out of range");
  if (std::strcmp(s.span, "capacity=") != 0 && !s.store)
    for (int64_t span : {8, 24, 1003}) refused(with([&](Args& g) { g.span = span; }), "multiple of 16", "a span that misaligns the rows");
  if (s.ring) refused(with([](Args& g) { g.n_rows = 0; }), "n_rows=0", "n_rows 0");
  refused(with([](Args& g) { g.acc_bytes -= 8; }), "acc has", "a short acc");
  refused(with([](Args& g) { g.n = 2; }), "acc has", "acc sized for one grid of two");
  refused(with([](Args& g) { g.t = block + 8; }), aligned, "a misaligned first pointer");
  if (std::strcmp(s.span, "capacity=") != 0) refused(with([](Args& g) { g.p = block + 1; }), aligned, "a misaligned p");
  refused(with([](Args& g) { g.acc = block + 8; }), aligned, "a misaligned acc");
  if (s.with_out) refused(with([](Args& g) { g.out = block + 4; }), aligned, "a misaligned out");
  if (s.paired) {
    refused(with([](Args& g) { g.rows = nullptr; }), "rows null, starts given", "starts without rows");
    refused(with([](Args& g) { g.starts = nullptr; }), "rows given, starts null", "rows without starts");
  }
  if (s.masked) {
    refused(with([](Args& g) { g.mask_of = nullptr; }), "null mask_of", "a null mask_of");
    refused(with([](Args& g) { g.masks = (const uint32_t*)block; }), "masks must be null", "masks with n_masks 0");
  }
  if (s.masked && !s.store) {  // (trilinear is a word of its own, in front of the representation's checks of the source)
    for (int32_t v : {-1, 2}) refused(with([&](Args& g) { g.trilinear = v; }), "trilinear=", "an unknown trilinear word");
    for (int32_t r : {1, 2})
      refused(with([&](Args& g) { g.trilinear = 1; g.representation = r; g.channels = 2; }), "trilinear=1 builds the signed grid alone",
              "trilinear with a non-signed representation");
    refused(with([](Args& g) { g.trilinear = 1; g.map_of = nullptr; }), "null map_of", "a null map_of");
    refused(with([](Args& g) { g.trilinear = 1; g.maps = (const float*)block; }), "maps must be null", "maps with n_maps 0");
  }
  if (s.store) {
    for (int32_t f : {-1, 4, 1 << 20}) refused(with([&](Args& g) { g.representation = f; }), "flavour=", "an unknown flavour");
    refused(with([](Args& g) { g.representation = 1; }), "channels=5 must be even", "separate polarity with an odd channels");
    for (int32_t c : {1, 4}) refused(with([&](Args& g) { g.representation = 2; g.channels = c; }), "must be 2", "a histogram of other than 2 planes");
    refused(with([](Args& g) { g.channels = 0; }), "channels=0 must be positive", "channels 0");
    const int64_t bad_capacities[] = {0, 8, 72, ((int64_t)1 << 40) + 16};
    for (int64_t c : bad_capacities) refused(with([&](Args& g) { g.capacity = c; g.total = 0; }), "capacity=", "a capacity out of range");
    for (int64_t t : {-1, 65}) refused(with([&](Args& g) { g.total = t; }), "total=", "a total outside the capacity");
    refused(with([](Args& g) { g.representation = 3; g.map_of = nullptr; }), "null map_of", "a null map_of");
    refused(with([](Args& g) { g.representation = 3; g.maps = (const float*)block; }), "maps must be null", "maps with n_maps 0");
    if (s.masked) {
      for (int32_t f : {0, 1, 2})
        refused(with([&](Args& g) { g.representation = f; g.channels = 2; g.maps = (const float*)block; }), "belong to flavour=3",
                "maps with a non-trilinear flavour");
      refused(with([](Args& g) { g.mask_of = (const int32_t*)(block + 2); }), "mask_of must be 4-byte aligned", "a misaligned mask_of");
    }
  }
  if (s.rectify) {
    refused(with([](Args& g) { g.map_of = nullptr; }), "null map_of", "a null map_of");
    refused(with([](Args& g) { g.maps = (const float*)block; }), "maps must be null", "maps with n_maps 0");
  }
  if (s.rep) {
    for (int32_t r : {-1, 3, 1 << 20}) refused(with([&](Args& g) { g.representation = r; }), "representation=", "an unknown representation");
    refused(with([](Args& g) { g.representation = 1; }), "channels=5 must be even", "separate polarity with an odd channels");
    for (int32_t c : {1, 4}) refused(with([&](Args& g) { g.representation = 2; g.channels = c; }), "must be 2", "a histogram of other than 2 planes");
    refused(with([](Args& g) { g.channels = 0; }), "channels=0 must be positive", "channels 0");
    // the workspace follows from channels: acc sized for 5 planes does not hold 6
    refused(with([](Args& g) { g.representation = 1; g.channels = 6; }), "acc has", "acc sized for fewer planes");
  }
}

// the two loader finishes: window false -> ess_event_grid_finish
struct Finish {
  const int32_t* counts = w;
  int32_t n_slots = 1, crop_rows = 20, resize_height = 26, resize_width = 44, out_rows = 22, normalize = 1;
  void* acc = a;
  size_t acc_bytes = (size_t)NB * H * W * 8;
  const int32_t* words = w;
  int32_t slots_per_group = 1, win_height = 12, win_width = 20;
  void* out = a;
  void* workspace = a;
  size_t workspace_bytes = ess_event_grid_finish_workspace(1, NB, H, W);
};

int finish(bool window, const Finish& f) {
  if (window)
    return ess_event_grid_finish_window(f.counts, f.n_slots, NB, H, W, f.acc, f.acc_bytes, f.crop_rows, f.resize_height, f.resize_width,
                                        f.out_rows, f.normalize, f.words, f.slots_per_group, f.win_height, f.win_width, (float*)f.out,
                                        f.workspace, f.workspace_bytes, nullptr);
  return ess_event_grid_finish(f.counts, f.n_slots, NB, H, W, f.acc, f.acc_bytes, f.crop_rows, f.resize_height, f.resize_width, f.out_rows,
                               f.normalize, (float*)f.out, f.workspace, f.workspace_bytes, nullptr);
}

void check_finish(bool window) {
  const char* entry = window ? "event_grid_finish_window:" : "event_grid_finish:";
  auto refused = [&](auto&& change, const char* needle, const char* what) {
    Finish f;
    change(f);
    expect_refused(finish(window, f), needle, entry, what);
  };
  refused([](Finish& f) { f.counts = nullptr; }, "null", "null counts");
  refused([](Finish& f) { f.acc = nullptr; }, "null", "a null acc");
  refused([](Finish& f) { f.out = nullptr; }, "null", "a null out");
  refused([](Finish& f) { f.workspace = nullptr; }, "null", "a null workspace");
  for (int32_t n : {0, 65536}) refused([&](Finish& f) { f.n_slots = n; }, "n_slots=", "a count out of range");
  for (int32_t v : {0, H + 1}) refused([&](Finish& f) { f.crop_rows = v; }, "crop_rows=", "crop_rows out of range");
  refused([](Finish& f) { f.resize_width = 0; }, "resize_width=0", "resize_width 0");
  for (int32_t v : {0, 27}) refused([&](Finish& f) { f.out_rows = v; }, "out_rows=", "out_rows out of range");
  for (int32_t v : {-1, 3}) refused([&](Finish& f) { f.normalize = v; }, "normalize=", "an unknown normalisation");
  refused([](Finish& f) { f.acc_bytes -= 8; }, "acc has", "a short acc");
  refused([](Finish& f) { f.n_slots = 2; }, "acc has", "acc sized for one slot of two");
  refused([](Finish& f) { f.workspace_bytes -= 1; }, "workspace has", "a short workspace");
  refused([](Finish& f) { f.acc = block + 8; }, "16-byte aligned", "a misaligned acc");
  refused([](Finish& f) { f.out = block + 4; }, "16-byte aligned", "a misaligned out");
  refused([](Finish& f) { f.workspace = block + 8; }, "16-byte aligned", "a misaligned workspace");
  if (!window) return;
  refused([](Finish& f) { f.words = nullptr; }, "null", "null words");
  refused([](Finish& f) { f.slots_per_group = 0; }, "slots_per_group=0", "slots_per_group 0");
  for (int32_t v : {0, 23}) refused([&](Finish& f) { f.win_height = v; }, "win_height=", "win_height out of range");
  for (int32_t v : {0, 45}) refused([&](Finish& f) { f.win_width = v; }, "win_width=", "win_width out of range");
  refused([](Finish& f) { f.words = (const int32_t*)(block + 2); }, "4-byte aligned", "misaligned words");
}

void check_label() {
  struct Label {
    const uint8_t* src = block;
    int32_t n = 2, src_height = 7, resize_height = 5, win_height = 4, win_width = 6;
    const int32_t* words = w;
    int64_t* out = (int64_t*)block;
  };
  auto refused = [&](auto&& change, const char* needle, const char* what) {
    Label l;
    change(l);
    expect_refused(ess_label_window(l.src, l.n, l.src_height, 5, l.resize_height, 9, l.words, l.win_height, l.win_width, l.out, nullptr),
                   needle, "label_window:", what);
  };
  refused([](Label& l) { l.src = nullptr; }, "null", "a null src");
  refused([](Label& l) { l.words = nullptr; }, "null", "null words");
  refused([](Label& l) { l.out = nullptr; }, "null", "a null out");
  for (int32_t n : {0, 65536}) refused([&](Label& l) { l.n = n; }, "n=", "a count out of range");
  refused([](Label& l) { l.src_height = 0; }, "must be positive", "src_height 0");
  refused([](Label& l) { l.resize_height = 0; }, "must be positive", "resize_height 0");
  for (int32_t v : {0, 6}) refused([&](Label& l) { l.win_height = v; }, "win_height=", "win_height out of range");
  for (int32_t v : {0, 10}) refused([&](Label& l) { l.win_width = v; }, "win_width=", "win_width out of range");
  refused([](Label& l) { l.words = (const int32_t*)(block + 2); }, "4-byte", "misaligned words");
  refused([](Label& l) { l.out = (int64_t*)(block + 4); }, "8-byte aligned", "a misaligned out");
}
}  // namespace

int main(int argc, char** argv) {
  texts = argc > 1 && std::strcmp(argv[1], "--texts") == 0;
  const size_t need = ess_event_ingest_workspace(1, NB, H, W);
  if (need != (size_t)NB * H * W * 8 || ess_event_grid_finish_workspace(1, NB, H, W) == 0 || ess_event_ingest_workspace(0, NB, H, W) != 0) {
    std::printf("FAIL workspace: %zu\n", need);
    ++failures;
  }
  for (const Source& s : SOURCES) check_source(s);
  check_finish(false);
  check_finish(true);
  check_label();
  if (failures) return 1;
  std::printf("event_ring_args: every refusal as expected (%d refusals)\n", refusals);
  return 0;
}
