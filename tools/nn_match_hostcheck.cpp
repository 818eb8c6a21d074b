// Host-side check of oetr_nn_match (include/oetr_nn_match.h) under AddressSanitizer and UBSan, on a machine WITHOUT a
// GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible these calls are SKIPPED - they would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-nn_match
#include <cstdint>

#include "../include/oetr_nn_match.h"
#include "hostcheck.h"

namespace {

const char ENTRY[] = "oetr_nn_match";

struct Args {
  const float* desc0;
  const int32_t* off0;
  int64_t n_kp0;
  const float* desc1;
  const int32_t* off1;
  int64_t n_kp1;
  int n_pairs, D, max_k0, max_k1;
  float ratio_sq, distance_sq;
  unsigned flags;
  void* workspace;
  size_t workspace_bytes;
  int32_t* matches0;
  float* scores0;
  int32_t *matches1, *counts;
};

Args pointing_at(void* p) {
  Args a;
  a.desc0 = a.desc1 = static_cast<const float*>(p);
  a.off0 = a.off1 = static_cast<const int32_t*>(p);
  a.n_kp0 = 5;
  a.n_kp1 = 4;
  a.n_pairs = 2;
  a.D = 128;
  a.max_k0 = 3;
  a.max_k1 = 2;
  a.ratio_sq = 0.64f;
  a.distance_sq = 0.49f;
  a.flags = OETR_NN_MATCH_RATIO | OETR_NN_MATCH_DISTANCE | OETR_NN_MATCH_MUTUAL;
  a.workspace = p;
  a.workspace_bytes = 1 << 20;
  a.matches0 = a.matches1 = a.counts = static_cast<int32_t*>(p);
  a.scores0 = static_cast<float*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_nn_match(a.desc0, a.off0, a.n_kp0, a.desc1, a.off1, a.n_kp1, a.n_pairs, a.D, a.max_k0, a.max_k1,
                       a.ratio_sq, a.distance_sq, a.flags, a.workspace, a.workspace_bytes, a.matches0, a.scores0,
                       a.matches1, a.counts, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_nn_match_abi_version() != OETR_NN_MATCH_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_nn_match_abi_version(), OETR_NN_MATCH_ABI_VERSION);
    return 1;
  }
  if (oetr_nn_match_workspace_bytes(0) != 0 || oetr_nn_match_workspace_bytes(-1) != 0 ||
      oetr_nn_match_workspace_bytes(INT64_MIN) != 0 || oetr_nn_match_workspace_bytes(1000) < 4000 ||
      oetr_nn_match_workspace_bytes(INT32_MAX) < (size_t)INT32_MAX * 4) {
    std::printf("oetr_nn_match_workspace_bytes FAILED\n");
    ++hostcheck::failures;
  }
  const Args good = pointing_at(hostcheck::keep);
  Args a;
  REJECT("desc0 = NULL", a.desc0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("off0 = NULL", a.off0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("desc1 = NULL", a.desc1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("off1 = NULL", a.off1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("matches0 = NULL", a.matches0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("scores0 = NULL", a.scores0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL, no rows", (a.counts = nullptr, a.n_kp0 = a.n_kp1 = 0), OETR_ERR_BAD_ARG);
  REJECT("no matches1, no workspace", (a.matches1 = nullptr, a.workspace = nullptr), OETR_ERR_BAD_ARG);
  REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
  REJECT("n_kp0 = -1", a.n_kp0 = -1, OETR_ERR_BAD_ARG);
  REJECT("n_kp1 = INT64_MIN", a.n_kp1 = INT64_MIN, OETR_ERR_BAD_ARG);
  REJECT("max_k0 = -1", a.max_k0 = -1, OETR_ERR_BAD_ARG);
  REJECT("max_k1 = INT32_MIN", a.max_k1 = INT32_MIN, OETR_ERR_BAD_ARG);
  REJECT("D = 0", a.D = 0, OETR_ERR_BAD_ARG);
  REJECT("D = -128", a.D = -128, OETR_ERR_BAD_ARG);
  REJECT("D = 130", a.D = 130, OETR_ERR_BAD_ARG);
  REJECT("D = 516", a.D = 516, OETR_ERR_BAD_ARG);
  REJECT("D = INT32_MAX", a.D = INT32_MAX, OETR_ERR_BAD_ARG);
  REJECT("flags = 8", a.flags = 8u, OETR_ERR_BAD_ARG);
  REJECT("flags = all ones", a.flags = ~0u, OETR_ERR_BAD_ARG);
  REJECT("desc0 at 8 bytes", a.desc0 = reinterpret_cast<const float*>(hostcheck::keep + 8), OETR_ERR_BAD_ARG);
  REJECT("desc1 at 4 bytes", a.desc1 = reinterpret_cast<const float*>(hostcheck::keep + 4), OETR_ERR_BAD_ARG);
  REJECT("matches0 at 2 bytes", a.matches0 = reinterpret_cast<int32_t*>(hostcheck::keep + 2), OETR_ERR_BAD_ARG);
  REJECT("counts at 1 byte", a.counts = reinterpret_cast<int32_t*>(hostcheck::keep + 1), OETR_ERR_BAD_ARG);
  REJECT("n_kp0 = 2^31", a.n_kp0 = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
  REJECT("n_kp1 = INT64_MAX", a.n_kp1 = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("too many workgroups", (a.n_pairs = 1 << 20, a.max_k0 = a.max_k1 = INT32_MAX), OETR_ERR_BAD_SHAPE);
  REJECT("workspace_bytes = 0", (a.matches1 = nullptr, a.workspace_bytes = 0), OETR_ERR_WORKSPACE);
  REJECT("workspace one byte short",
         (a.matches1 = nullptr, a.n_kp1 = 100000, a.workspace_bytes = oetr_nn_match_workspace_bytes(100000) - 1),
         OETR_ERR_WORKSPACE);

  if (char* none = hostcheck::no_device_page()) {
    for (int variant = 0; variant < 5; ++variant) {
      a = pointing_at(none + 256);
      if (variant == 1) a.n_kp0 = a.n_kp1 = 0, a.desc0 = a.desc1 = nullptr, a.matches0 = a.matches1 = nullptr, a.scores0 = nullptr;
      if (variant == 2) a.n_kp0 = a.n_kp1 = INT32_MAX, a.n_pairs = 40000, a.max_k0 = a.max_k1 = 1 << 20, a.D = 512;
      if (variant == 3) a.matches1 = nullptr, a.flags = 0, a.D = 4;
      if (variant == 4) a.workspace = nullptr, a.workspace_bytes = 0, a.max_k0 = a.max_k1 = 0;
      char label[16];
      std::snprintf(label, sizeof label, "variant %d", variant);
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
