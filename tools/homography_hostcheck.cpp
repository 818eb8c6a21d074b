// Host-side check of oetr_homography_match_score and oetr_homography_boxes (include/oetr_homography.h) under
// AddressSanitizer and UBSan, on a machine WITHOUT a GPU: a stand-alone program, linked with the library's host code,
// never loaded into Python.  For each of the two entries:
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them (`thresholds` is HOST memory and is a real array), so the call comes back with a
//      status (OETR_ERR_HIP: there is no device to enqueue on), not with a signal.  Where a GPU is visible these calls
//      are SKIPPED - they would enqueue kernels on host addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-homography
#include <cmath>
#include <cstdint>

#include "../include/oetr_homography.h"
#include "hostcheck.h"

namespace {

const double THRESHOLDS[OETR_HOMOGRAPHY_MAX_THRESHOLDS] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, NAN};

struct Args {                 // oetr_homography_match_score
  const double* params;
  const int32_t* offsets;
  int n_pairs;
  const float *k1, *k2;
  int64_t n_matches;
  const double* thresholds;   // host
  int n_thresholds;
  double* dist_sq;
  int32_t* counts;
};

Args pointing_at(void* p) {
  Args a;
  a.params = static_cast<const double*>(p);
  a.offsets = static_cast<const int32_t*>(p);
  a.n_pairs = 2;
  a.k1 = a.k2 = static_cast<const float*>(p);
  a.n_matches = 5;
  a.thresholds = THRESHOLDS;
  a.n_thresholds = 15;
  a.dist_sq = static_cast<double*>(p);
  a.counts = static_cast<int32_t*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_homography_match_score(a.params, a.offsets, a.n_pairs, a.k1, a.k2, a.n_matches, a.thresholds,
                                     a.n_thresholds, a.dist_sq, a.counts, nullptr);
}

struct BoxArgs {              // oetr_homography_boxes
  const double* params;
  int n_pairs, max_h1, max_w1;
  void* workspace;
  size_t workspace_bytes;
  float *box1, *box2;
  uint8_t* valid;
  int32_t* count;
};

BoxArgs boxes_pointing_at(void* p, int n_pairs) {
  BoxArgs a;
  a.params = static_cast<const double*>(p);
  a.n_pairs = n_pairs;
  a.max_h1 = 480;
  a.max_w1 = 640;
  a.workspace = p;
  a.workspace_bytes = oetr_homography_workspace_bytes(n_pairs);
  a.box1 = a.box2 = static_cast<float*>(p);
  a.valid = static_cast<uint8_t*>(p);
  a.count = static_cast<int32_t*>(p);
  return a;
}

oetr_status call(const BoxArgs& a) {
  return oetr_homography_boxes(a.params, a.n_pairs, a.max_h1, a.max_w1, a.workspace, a.workspace_bytes, a.box1, a.box2,
                               a.valid, a.count, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_homography_abi_version() != OETR_HOMOGRAPHY_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_homography_abi_version(), OETR_HOMOGRAPHY_ABI_VERSION);
    return 1;
  }
  if (oetr_homography_workspace_bytes(0) != 0 || oetr_homography_workspace_bytes(-3) != 0 ||
      oetr_homography_workspace_bytes(3) == 0) {
    std::printf("oetr_homography_workspace_bytes: 0 / -3 / 3 pairs give %zu / %zu / %zu\n",
                oetr_homography_workspace_bytes(0), oetr_homography_workspace_bytes(-3),
                oetr_homography_workspace_bytes(3));
    return 1;
  }
  {
    const char ENTRY[] = "oetr_homography_match_score";
    const Args good = pointing_at(hostcheck::keep);
    Args a;
    REJECT("params = NULL", a.params = nullptr, OETR_ERR_BAD_ARG);
    REJECT("offsets = NULL", a.offsets = nullptr, OETR_ERR_BAD_ARG);
    REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
    REJECT("counts = NULL, no matches", (a.counts = nullptr, a.n_matches = 0), OETR_ERR_BAD_ARG);
    REJECT("k1 = NULL", a.k1 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("k2 = NULL", a.k2 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("thresholds = NULL", a.thresholds = nullptr, OETR_ERR_BAD_ARG);
    REJECT("n_thresholds = -1", a.n_thresholds = -1, OETR_ERR_BAD_ARG);
    REJECT("n_thresholds = 17", a.n_thresholds = 17, OETR_ERR_BAD_ARG);
    REJECT("n_thresholds = INT32_MAX", a.n_thresholds = INT32_MAX, OETR_ERR_BAD_ARG);
    REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
    REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
    REJECT("n_matches = -1", a.n_matches = -1, OETR_ERR_BAD_ARG);
    REJECT("n_matches = INT64_MIN", a.n_matches = INT64_MIN, OETR_ERR_BAD_ARG);
    REJECT("n_matches = 2^31", a.n_matches = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
    REJECT("n_matches = INT64_MAX", a.n_matches = INT64_MAX, OETR_ERR_BAD_SHAPE);
    REJECT("n_pairs = INT32_MAX / 17 + 1", a.n_pairs = INT32_MAX / 17 + 1, OETR_ERR_BAD_SHAPE);
    REJECT("n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);
  }
  {
    const char ENTRY[] = "oetr_homography_boxes";
    const BoxArgs good = boxes_pointing_at(hostcheck::keep, 2);
    BoxArgs a;
    REJECT("boxes: params = NULL", a.params = nullptr, OETR_ERR_BAD_ARG);
    REJECT("boxes: box1 = NULL", a.box1 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("boxes: box2 = NULL", a.box2 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("boxes: valid = NULL", a.valid = nullptr, OETR_ERR_BAD_ARG);
    REJECT("boxes: n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
    REJECT("boxes: n_pairs = -1", a.n_pairs = -1, OETR_ERR_BAD_ARG);
    REJECT("boxes: workspace = NULL", a.workspace = nullptr, OETR_ERR_BAD_ARG);
    REJECT("boxes: workspace one byte short", a.workspace_bytes -= 1, OETR_ERR_BAD_ARG);
    REJECT("boxes: workspace of 0 bytes", a.workspace_bytes = 0, OETR_ERR_BAD_ARG);
    REJECT("boxes: n_pairs = INT32_MAX / 17 + 1", (a.n_pairs = INT32_MAX / 17 + 1, a.workspace_bytes = SIZE_MAX),
           OETR_ERR_BAD_SHAPE);
    REJECT("boxes: max_h1 = 0", a.max_h1 = 0, OETR_ERR_BAD_SHAPE);
    REJECT("boxes: max_w1 = 0", a.max_w1 = 0, OETR_ERR_BAD_SHAPE);
    REJECT("boxes: max_h1 = -5", a.max_h1 = -5, OETR_ERR_BAD_SHAPE);
    REJECT("boxes: max_h1 = 8193", a.max_h1 = OETR_COVIS_MAX_SIDE + 1, OETR_ERR_BAD_SHAPE);
    REJECT("boxes: max_w1 = INT32_MAX", a.max_w1 = INT32_MAX, OETR_ERR_BAD_SHAPE);
  }

  if (char* none = hostcheck::no_device_page()) {
    for (int64_t n : {(int64_t)5, (int64_t)0, (int64_t)INT32_MAX}) {
      Args a = pointing_at(none + 256);
      a.n_matches = n;
      a.n_pairs = n == 5 ? 2 : INT32_MAX / 17;
      a.n_thresholds = n == 0 ? 0 : 16;
      if (n == 0) a.thresholds = nullptr, a.k1 = a.k2 = nullptr, a.dist_sq = nullptr;
      char label[32];
      std::snprintf(label, sizeof label, "n_matches %lld", (long long)n);
      hostcheck::expect_no_device(label, a);
    }
    for (int n : {1, 70000, INT32_MAX / 17}) {
      BoxArgs a = boxes_pointing_at(none + 256, n);
      if (n != 1) a.max_h1 = a.max_w1 = OETR_COVIS_MAX_SIDE, a.count = nullptr;
      char label[32];
      std::snprintf(label, sizeof label, "boxes, n_pairs %d", n);
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
