// Host-side check of oetr_pose_refit (include/oetr_pose_refit.h) under AddressSanitizer and UBSan, on a machine
// WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible these calls are SKIPPED - they would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-pose_refit
#include <cmath>
#include <cstdint>

#include "../include/oetr_pose_refit.h"
#include "hostcheck.h"

namespace {

struct Args {
  const double* params;
  const int32_t* offsets;
  int n_pairs;
  const float *k1, *k2;
  int64_t n_matches;
  const double* model_in;
  double px_thr;
  int refit_iters;
  double *model, *pose, *cosines;
  int32_t* counts;
  uint8_t* inliers;
};

Args pointing_at(void* p) {
  Args a;
  a.params = a.model_in = static_cast<const double*>(p);
  a.offsets = static_cast<const int32_t*>(p);
  a.n_pairs = 2;
  a.k1 = a.k2 = static_cast<const float*>(p);
  a.n_matches = 5;
  a.px_thr = 1.0;
  a.refit_iters = 4;
  a.model = a.pose = a.cosines = static_cast<double*>(p);
  a.counts = static_cast<int32_t*>(p);
  a.inliers = static_cast<uint8_t*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_pose_refit(a.params, a.offsets, a.n_pairs, a.k1, a.k2, a.n_matches, a.model_in, a.px_thr, a.refit_iters,
                         a.model, a.pose, a.cosines, a.counts, a.inliers, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_pose_refit_abi_version() != OETR_POSE_REFIT_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_pose_refit_abi_version(), OETR_POSE_REFIT_ABI_VERSION);
    return 1;
  }
  {
    const char ENTRY[] = "oetr_pose_refit";
    const Args good = pointing_at(hostcheck::keep);
    Args a;
    REJECT("params = NULL", a.params = nullptr, OETR_ERR_BAD_ARG);
    REJECT("offsets = NULL", a.offsets = nullptr, OETR_ERR_BAD_ARG);
    REJECT("model_in = NULL", a.model_in = nullptr, OETR_ERR_BAD_ARG);
    REJECT("model = NULL", a.model = nullptr, OETR_ERR_BAD_ARG);
    REJECT("pose = NULL", a.pose = nullptr, OETR_ERR_BAD_ARG);
    REJECT("cosines = NULL", a.cosines = nullptr, OETR_ERR_BAD_ARG);
    REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
    REJECT("k1 = NULL", a.k1 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("k2 = NULL", a.k2 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
    REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
    REJECT("n_matches = -1", a.n_matches = -1, OETR_ERR_BAD_ARG);
    REJECT("n_matches = INT64_MIN", a.n_matches = INT64_MIN, OETR_ERR_BAD_ARG);
    REJECT("refit_iters = -1", a.refit_iters = -1, OETR_ERR_BAD_ARG);
    REJECT("refit_iters = 9", a.refit_iters = 9, OETR_ERR_BAD_ARG);
    REJECT("refit_iters = INT32_MAX", a.refit_iters = INT32_MAX, OETR_ERR_BAD_ARG);
    REJECT("refit_iters = INT32_MIN", a.refit_iters = INT32_MIN, OETR_ERR_BAD_ARG);
    REJECT("px_thr = 0", a.px_thr = 0.0, OETR_ERR_BAD_ARG);
    REJECT("px_thr = -1", a.px_thr = -1.0, OETR_ERR_BAD_ARG);
    REJECT("px_thr = NaN", a.px_thr = NAN, OETR_ERR_BAD_ARG);
    REJECT("px_thr = inf", a.px_thr = INFINITY, OETR_ERR_BAD_ARG);
    REJECT("n_matches = 2^31", a.n_matches = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
    REJECT("n_matches = INT64_MAX", a.n_matches = INT64_MAX, OETR_ERR_BAD_SHAPE);
  }

  if (char* none = hostcheck::no_device_page()) {
    for (int route = 0; route < 4; ++route) {
      Args a = pointing_at(none + 256);
      const char* label = "2 pairs, 4 rounds";
      if (route == 1) {
        label = "largest call";
        a.n_pairs = INT32_MAX, a.n_matches = INT32_MAX, a.refit_iters = OETR_POSE_REFIT_MAX_ITERS;
      } else if (route == 2) {
        label = "no rounds, no inliers";
        a.refit_iters = 0, a.inliers = nullptr;
      } else if (route == 3) {
        label = "no matches";
        a.n_matches = 0, a.k1 = a.k2 = nullptr;
      }
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
