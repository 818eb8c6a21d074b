// Host-side check of oetr_assemble_matches (include/oetr_match_assembly.h) under AddressSanitizer and UBSan, on a
// machine WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible these calls are SKIPPED - they would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-assembly
#include <cstdint>

#include "../include/oetr_match_assembly.h"
#include "hostcheck.h"

namespace {

const char ENTRY[] = "oetr_assemble_matches";

struct Args {
  const oetr_crop_info* info;
  const double* scales;
  int n_pairs;
  const float* kp0;
  const int32_t* off0;
  int64_t n_kp0;
  const float* kp1;
  const int32_t* off1;
  int64_t n_kp1;
  const void* matches;
  int match_bytes;
  const float* conf;
  int min_matches;
  void* workspace;
  size_t workspace_bytes;
  double *origin0, *origin1;
  int32_t *index0, *index1;
  float *k1, *k2, *mconf;
  int32_t *offsets, *counts, *few, *n_few;
};

Args pointing_at(void* p) {
  Args a;
  a.info = static_cast<const oetr_crop_info*>(p);
  a.scales = static_cast<const double*>(p);
  a.n_pairs = 2;
  a.kp0 = a.kp1 = a.conf = static_cast<const float*>(p);
  a.off0 = a.off1 = static_cast<const int32_t*>(p);
  a.n_kp0 = 5;
  a.n_kp1 = 4;
  a.matches = p;
  a.match_bytes = 4;
  a.min_matches = 30;
  a.workspace = p;
  a.workspace_bytes = 1 << 20;
  a.origin0 = a.origin1 = static_cast<double*>(p);
  a.index0 = a.index1 = a.offsets = a.counts = a.few = a.n_few = static_cast<int32_t*>(p);
  a.k1 = a.k2 = a.mconf = static_cast<float*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_assemble_matches(a.info, a.scales, a.n_pairs, a.kp0, a.off0, a.n_kp0, a.kp1, a.off1, a.n_kp1, a.matches,
                               a.match_bytes, a.conf, a.min_matches, a.workspace, a.workspace_bytes, a.origin0,
                               a.origin1, a.index0, a.index1, a.k1, a.k2, a.mconf, a.offsets, a.counts, a.few, a.n_few,
                               nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_match_assembly_abi_version() != OETR_MATCH_ASSEMBLY_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_match_assembly_abi_version(), OETR_MATCH_ASSEMBLY_ABI_VERSION);
    return 1;
  }
  if (oetr_match_assembly_workspace_bytes(0) != 0 || oetr_match_assembly_workspace_bytes(-1) != 0 ||
      oetr_match_assembly_workspace_bytes(1000) < 4000 ||
      oetr_match_assembly_workspace_bytes(INT32_MAX) < (size_t)INT32_MAX * 4) {
    std::printf("oetr_match_assembly_workspace_bytes FAILED\n");
    ++hostcheck::failures;
  }
  const Args good = pointing_at(hostcheck::keep);
  Args a;
  REJECT("info = NULL", a.info = nullptr, OETR_ERR_BAD_ARG);
  REJECT("scales = NULL", a.scales = nullptr, OETR_ERR_BAD_ARG);
  REJECT("kp0 = NULL", a.kp0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("off0 = NULL", a.off0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("kp1 = NULL", a.kp1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("off1 = NULL", a.off1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("matches = NULL", a.matches = nullptr, OETR_ERR_BAD_ARG);
  REJECT("workspace = NULL", a.workspace = nullptr, OETR_ERR_BAD_ARG);
  REJECT("origin0 = NULL", a.origin0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("origin1 = NULL", a.origin1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("index0 = NULL", a.index0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("index1 = NULL", a.index1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("k1 = NULL", a.k1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("k2 = NULL", a.k2 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("offsets = NULL", a.offsets = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL, no keypoints", (a.counts = nullptr, a.n_kp0 = a.n_kp1 = 0), OETR_ERR_BAD_ARG);
  REJECT("conf without mconf", a.mconf = nullptr, OETR_ERR_BAD_ARG);
  REJECT("mconf without conf", a.conf = nullptr, OETR_ERR_BAD_ARG);
  REJECT("few without n_few", a.n_few = nullptr, OETR_ERR_BAD_ARG);
  REJECT("n_few without few", a.few = nullptr, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
  REJECT("n_kp0 = -1", a.n_kp0 = -1, OETR_ERR_BAD_ARG);
  REJECT("n_kp1 = INT64_MIN", a.n_kp1 = INT64_MIN, OETR_ERR_BAD_ARG);
  REJECT("match_bytes = 0", a.match_bytes = 0, OETR_ERR_BAD_ARG);
  REJECT("match_bytes = 2", a.match_bytes = 2, OETR_ERR_BAD_ARG);
  REJECT("match_bytes = 16", a.match_bytes = 16, OETR_ERR_BAD_ARG);
  REJECT("match_bytes = -8", a.match_bytes = -8, OETR_ERR_BAD_ARG);
  REJECT("min_matches = -1", a.min_matches = -1, OETR_ERR_BAD_ARG);
  REJECT("kp0 at 4 bytes", a.kp0 = reinterpret_cast<const float*>(hostcheck::keep + 4), OETR_ERR_BAD_ARG);
  REJECT("origin0 at 8 bytes", a.origin0 = reinterpret_cast<double*>(hostcheck::keep + 8), OETR_ERR_BAD_ARG);
  REJECT("int64 matches at 4 bytes", (a.matches = hostcheck::keep + 4, a.match_bytes = 8), OETR_ERR_BAD_ARG);
  REJECT("n_kp0 = 2^31", a.n_kp0 = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
  REJECT("n_kp1 = INT64_MAX", a.n_kp1 = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("workspace_bytes = 0", a.workspace_bytes = 0, OETR_ERR_WORKSPACE);
  REJECT("workspace one byte short", (a.n_pairs = 100000, a.workspace_bytes = oetr_match_assembly_workspace_bytes(100000) - 1),
         OETR_ERR_WORKSPACE);

  if (char* none = hostcheck::no_device_page()) {
    for (int variant = 0; variant < 4; ++variant) {
      a = pointing_at(none + 256);
      if (variant == 1) a.n_kp0 = a.n_kp1 = 0, a.kp0 = a.kp1 = nullptr, a.matches = nullptr, a.origin0 = nullptr;
      if (variant == 2) a.n_kp0 = a.n_kp1 = INT32_MAX, a.n_pairs = 40000, a.match_bytes = 8;
      if (variant == 3) a.conf = nullptr, a.mconf = nullptr, a.few = a.n_few = nullptr;
      char label[16];
      std::snprintf(label, sizeof label, "variant %d", variant);
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
