// Stand-alone host program: the argument checks of ess_event_ingest_ring, which all come in front of any launch, so no device is
// needed.  Meant to be built with the host sanitizers and run on its own (a library loaded into python is out of their reach):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -x hip ess_amd/csrc/voxel_ingest.hip tools/host_checks/event_ring_args_main.cpp \
//         -x none ess_amd/libess_hip.so -Wl,-rpath,$PWD/ess_amd -o event_ring_args
//   ./event_ring_args
//
// voxel_ingest.hip -- the code under test -- is compiled into the program with the sanitizers; the built library only supplies the
// error text (api.cpp), and the program's own ess_event_ingest_ring takes precedence over the library's.
// Every refused call must return ESS_EINVAL and leave a text in ess_last_error(); the pointers handed over are never dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ess_hip.h"

namespace {
int failures = 0;

void expect_refused(int rc, const char* needle, const char* what) {
  const char* msg = ess_last_error();
  if (rc != -22 || !msg || !std::strstr(msg, needle)) {
    std::printf("FAIL %s: rc=%d, message '%s' (wanted -22 and '%s')\n", what, rc, msg ? msg : "(null)", needle);
    ++failures;
  }
}
}  // namespace

int main() {
  alignas(16) static unsigned char block[64];
  void* a = block;  // 16-byte aligned, never read
  const int32_t* w = (const int32_t*)block;
  const int32_t NB = 5, H = 24, W = 40;
  const size_t need = ess_event_ingest_workspace(1, NB, H, W);
  if (need != (size_t)NB * H * W * 8) {
    std::printf("FAIL workspace: %zu\n", need);
    ++failures;
  }
  // one null pointer at a time
  for (int k = 0; k < 10; ++k) {
    const void* p[10] = {a, a, a, a, w, w, w, w, a, a};
    p[k] = nullptr;
    const int rc = ess_event_ingest_ring(p[0], p[1], p[2], p[3], (const int32_t*)p[4], (const int32_t*)p[5], (const int32_t*)p[6],
                                         (const int32_t*)p[7], 32, 1, 1, NB, H, W, (void*)p[8], need, (float*)p[9], nullptr);
    char what[32];
    std::snprintf(what, sizeof what, "null pointer %d", k);
    expect_refused(rc, "null", what);
  }
  auto call = [&](int64_t ring, int32_t n_rows, int32_t n_slots, size_t acc_bytes, const void* p, void* out) {
    return ess_event_ingest_ring(a, a, a, p, w, w, w, w, ring, n_rows, n_slots, NB, H, W, a, acc_bytes, (float*)out, nullptr);
  };
  const int64_t bad_rings[] = {0, -16, 8, 24, 1003, ((int64_t)1 << 22) + 16, INT64_MAX, INT64_MIN};
  for (int64_t ring : bad_rings) expect_refused(call(ring, 1, 1, need, a, a), "ring=", "a bad ring");
  expect_refused(call(24, 1, 1, need, a, a), "multiple of 16", "ring 24");
  expect_refused(call(32, 0, 1, need, a, a), "n_rows", "n_rows 0");
  expect_refused(call(32, 1, 0, need, a, a), "n_slots", "n_slots 0");
  expect_refused(call(32, 1, 65536, need, a, a), "n_slots", "n_slots 65536");
  expect_refused(call(32, 1, 1, need - 8, a, a), "acc has", "a short acc");
  expect_refused(call(32, 1, 2, need, a, a), "acc has", "acc sized for one slot of two");
  expect_refused(call(32, 1, 1, need, block + 1, a), "16-byte aligned", "a misaligned p");
  expect_refused(call(32, 1, 1, need, a, block + 4), "16-byte aligned", "a misaligned out");
  if (failures) return 1;
  std::printf("event_ring_args: every refusal as expected\n");
  return 0;
}
