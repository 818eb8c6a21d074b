// Host-side check of oetr_match_score (include/oetr_match_score.h) under AddressSanitizer and UBSan, on a machine
// WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. one call with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible this call is SKIPPED - it would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck
#include <cmath>
#include <cstdint>

#include "../include/oetr_match_score.h"
#include "hostcheck.h"

namespace {

const char ENTRY[] = "oetr_match_score";

struct Args {
  const oetr_covis_map* maps;
  int n_maps;
  const int32_t *idx1, *idx2;
  const double* params;
  const int32_t* offsets;
  int n_pairs;
  const float *k1, *k2;
  int64_t n_matches;
  double epi, sym, px;
  double* values;
  uint8_t* flags;
  int32_t* counts;
};

Args pointing_at(void* p) {
  Args a;
  a.maps = static_cast<const oetr_covis_map*>(p);
  a.n_maps = 3;
  a.idx1 = a.idx2 = a.offsets = static_cast<const int32_t*>(p);
  a.params = static_cast<const double*>(p);
  a.n_pairs = 2;
  a.k1 = a.k2 = static_cast<const float*>(p);
  a.n_matches = 5;
  a.epi = 5e-4;
  a.sym = std::nan("");
  a.px = 3.0;
  a.values = static_cast<double*>(p);
  a.flags = static_cast<uint8_t*>(p);
  a.counts = static_cast<int32_t*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_match_score(a.maps, a.n_maps, a.idx1, a.idx2, a.params, a.offsets, a.n_pairs, a.k1, a.k2, a.n_matches,
                          a.epi, a.sym, a.px, a.values, a.flags, a.counts, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_match_score_abi_version() != OETR_MATCH_SCORE_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_match_score_abi_version(), OETR_MATCH_SCORE_ABI_VERSION);
    return 1;
  }
  const Args good = pointing_at(hostcheck::keep);
  Args a;
  REJECT("maps = NULL", a.maps = nullptr, OETR_ERR_BAD_ARG);
  REJECT("idx1 = NULL", a.idx1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("idx2 = NULL", a.idx2 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("params = NULL", a.params = nullptr, OETR_ERR_BAD_ARG);
  REJECT("offsets = NULL", a.offsets = nullptr, OETR_ERR_BAD_ARG);
  REJECT("k1 = NULL", a.k1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("k2 = NULL", a.k2 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("flags = NULL", a.flags = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL, no matches", (a.counts = nullptr, a.n_matches = 0), OETR_ERR_BAD_ARG);
  REJECT("n_maps = 0", a.n_maps = 0, OETR_ERR_BAD_ARG);
  REJECT("n_maps = -1", a.n_maps = -1, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
  REJECT("n_matches = -1", a.n_matches = -1, OETR_ERR_BAD_ARG);
  REJECT("n_matches = INT64_MIN", a.n_matches = INT64_MIN, OETR_ERR_BAD_ARG);
  REJECT("n_matches = 2^31", a.n_matches = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
  REJECT("n_matches = INT64_MAX", a.n_matches = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);

  if (char* none = hostcheck::no_device_page()) {
    for (int64_t n : {(int64_t)5, (int64_t)0, (int64_t)INT32_MAX}) {
      a = pointing_at(none + 256);
      a.n_matches = n;
      a.n_pairs = n == 5 ? 2 : 40000;
      char label[32];
      std::snprintf(label, sizeof label, "n_matches %lld", (long long)n);
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
