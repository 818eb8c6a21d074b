// Host-side check of oetr_keypoint_repeatability (include/oetr_keypoint_score.h) under AddressSanitizer and UBSan, on
// a machine WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every DEVICE pointer points into a PROT_NONE page (the thresholds are
//      host memory by contract and stay readable): the host code dereferences none of them, so the call comes back
//      with a status (OETR_ERR_HIP: there is no device to enqueue on), not with a signal.  Where a GPU is visible
//      these calls are SKIPPED - they would enqueue kernels on host addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-keypoints
#include <cmath>
#include <cstdint>

#include "../include/oetr_keypoint_score.h"
#include "hostcheck.h"

namespace {

const char ENTRY[] = "oetr_keypoint_repeatability";
const double thresholds[8] = {1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 21.0, 34.0};

struct Args {
  const oetr_covis_map* maps;
  int n_maps;
  const float* keypoints;
  int64_t n_keypoints;
  const int32_t *kp_offsets, *idx1, *idx2;
  const double* params;
  int n_pairs;
  const double* thr;
  int n_thr, max_kp;
  int32_t *counts, *nearest;
  double* dist_sq;
};

Args pointing_at(void* p) {
  Args a;
  a.maps = static_cast<const oetr_covis_map*>(p);
  a.n_maps = 3;
  a.keypoints = static_cast<const float*>(p);
  a.n_keypoints = 7;
  a.kp_offsets = a.idx1 = a.idx2 = static_cast<const int32_t*>(p);
  a.params = static_cast<const double*>(p);
  a.n_pairs = 2;
  a.thr = thresholds;
  a.n_thr = 4;
  a.max_kp = 5;
  a.counts = a.nearest = static_cast<int32_t*>(p);
  a.dist_sq = static_cast<double*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_keypoint_repeatability(a.maps, a.n_maps, a.keypoints, a.n_keypoints, a.kp_offsets, a.idx1, a.idx2, a.params,
                                     a.n_pairs, a.thr, a.n_thr, a.max_kp, a.counts, a.nearest, a.dist_sq, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_keypoint_score_abi_version() != OETR_KEYPOINT_SCORE_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_keypoint_score_abi_version(), OETR_KEYPOINT_SCORE_ABI_VERSION);
    return 1;
  }
  const Args good = pointing_at(hostcheck::keep);
  Args a;
  REJECT("maps = NULL", a.maps = nullptr, OETR_ERR_BAD_ARG);
  REJECT("kp_offsets = NULL", a.kp_offsets = nullptr, OETR_ERR_BAD_ARG);
  REJECT("idx1 = NULL", a.idx1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("idx2 = NULL", a.idx2 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("params = NULL", a.params = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL, no keypoints", (a.counts = nullptr, a.n_keypoints = 0, a.max_kp = 0), OETR_ERR_BAD_ARG);
  REJECT("keypoints = NULL", a.keypoints = nullptr, OETR_ERR_BAD_ARG);
  REJECT("thresholds = NULL", a.thr = nullptr, OETR_ERR_BAD_ARG);
  REJECT("n_thresholds = -1", a.n_thr = -1, OETR_ERR_BAD_ARG);
  REJECT("n_thresholds = 9", a.n_thr = 9, OETR_ERR_BAD_ARG);
  REJECT("n_maps = 0", a.n_maps = 0, OETR_ERR_BAD_ARG);
  REJECT("n_maps = -1", a.n_maps = -1, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
  REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
  REJECT("n_keypoints = -1", a.n_keypoints = -1, OETR_ERR_BAD_ARG);
  REJECT("n_keypoints = INT64_MIN", a.n_keypoints = INT64_MIN, OETR_ERR_BAD_ARG);
  REJECT("max_kp = -1", a.max_kp = -1, OETR_ERR_BAD_ARG);
  REJECT("max_kp = INT32_MIN", a.max_kp = INT32_MIN, OETR_ERR_BAD_ARG);
  REJECT("n_keypoints = 2^31", a.n_keypoints = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
  REJECT("n_keypoints = INT64_MAX", a.n_keypoints = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_pairs = 2^28, 8 thresholds", (a.n_pairs = 1 << 28, a.n_thr = 8, a.max_kp = 1), OETR_ERR_BAD_SHAPE);
  REJECT("max_kp = INT32_MAX, 2^20 pairs", (a.max_kp = INT32_MAX, a.n_pairs = 1 << 20), OETR_ERR_BAD_SHAPE);

  if (char* none = hostcheck::no_device_page()) {
    struct Case {
      const char* name;
      int64_t n_keypoints;
      int n_pairs, n_thr, max_kp;
      bool outputs;
    };
    const Case cases[] = {{"plain", 7, 2, 4, 5, true},
                          {"counters only", 7, 2, 8, 5, false},
                          {"no keypoints, no thresholds", 0, 2, 0, 0, true},
                          {"largest", INT32_MAX, 40000, 8, 6000, true},
                          {"widest", INT32_MAX, 1, 1, INT32_MAX, true}};
    for (const Case& c : cases) {
      a = pointing_at(none + 256);
      a.n_keypoints = c.n_keypoints;
      a.n_pairs = c.n_pairs;
      a.n_thr = c.n_thr;
      a.max_kp = c.max_kp;
      if (c.n_thr == 0) a.thr = nullptr;
      if (c.n_keypoints == 0) a.keypoints = nullptr;
      if (!c.outputs) {
        a.nearest = nullptr;
        a.dist_sq = nullptr;
      }
      hostcheck::expect_no_device(c.name, a);
    }
  }
  return hostcheck::finish();
}
