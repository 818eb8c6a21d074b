// Host-side check of oetr_homography_ransac (include/oetr_homography_ransac.h) under AddressSanitizer and UBSan, on a machine
// WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible these calls are SKIPPED - they would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-homography_ransac
#include <cmath>
#include <cstdint>

#include "../include/oetr_homography_ransac.h"
#include "hostcheck.h"

namespace {

struct Args {
  const double* params;
  const int32_t *offsets, *pair_ids;
  int n_pairs;
  const float *k1, *k2;
  int64_t n_matches;
  int n_hyp;
  uint32_t seed;
  double px_thr;
  int refit_iters;
  const double* models_in;
  int n_models_in;
  void* workspace;
  size_t workspace_bytes;
  double *model, *H, *corner_sq;
  int32_t* counts;
  uint8_t* inliers;
};

Args pointing_at(void* p) {
  Args a;
  a.params = static_cast<const double*>(p);
  a.offsets = a.pair_ids = static_cast<const int32_t*>(p);
  a.n_pairs = 2;
  a.k1 = a.k2 = static_cast<const float*>(p);
  a.n_matches = 5;
  a.n_hyp = 8;
  a.seed = 1;
  a.px_thr = 3.0;
  a.refit_iters = 2;
  a.models_in = nullptr;
  a.n_models_in = 0;
  a.workspace = p;
  a.workspace_bytes = oetr_homography_ransac_workspace_bytes(2, 8);
  a.model = a.H = a.corner_sq = static_cast<double*>(p);
  a.counts = static_cast<int32_t*>(p);
  a.inliers = static_cast<uint8_t*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_homography_ransac(a.params, a.offsets, a.pair_ids, a.n_pairs, a.k1, a.k2, a.n_matches, a.n_hyp, a.seed,
                                a.px_thr, a.refit_iters, a.models_in, a.n_models_in, a.workspace, a.workspace_bytes,
                                a.model, a.H, a.corner_sq, a.counts, a.inliers, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_homography_ransac_abi_version() != OETR_HOMOGRAPHY_RANSAC_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_homography_ransac_abi_version(), OETR_HOMOGRAPHY_RANSAC_ABI_VERSION);
    return 1;
  }
  if (oetr_homography_ransac_workspace_bytes(0, 3) != 0 || oetr_homography_ransac_workspace_bytes(3, -1) != 0 ||
      oetr_homography_ransac_workspace_bytes(1, 1) != 76 ||
      oetr_homography_ransac_workspace_bytes(INT32_MAX / 4096, 4096) != (size_t)(INT32_MAX / 4096) * 4096 * 76) {
    std::printf("oetr_homography_ransac_workspace_bytes: unexpected sizes\n");
    return 1;
  }
  {
    const char ENTRY[] = "oetr_homography_ransac";
    const Args good = pointing_at(hostcheck::keep);
    void* keep = hostcheck::keep;
    Args a;
    REJECT("params = NULL", a.params = nullptr, OETR_ERR_BAD_ARG);
    REJECT("offsets = NULL", a.offsets = nullptr, OETR_ERR_BAD_ARG);
    REJECT("model = NULL", a.model = nullptr, OETR_ERR_BAD_ARG);
    REJECT("H = NULL", a.H = nullptr, OETR_ERR_BAD_ARG);
    REJECT("corner_sq = NULL", a.corner_sq = nullptr, OETR_ERR_BAD_ARG);
    REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
    REJECT("k1 = NULL", a.k1 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("k2 = NULL", a.k2 = nullptr, OETR_ERR_BAD_ARG);
    REJECT("n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
    REJECT("n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
    REJECT("n_matches = -1", a.n_matches = -1, OETR_ERR_BAD_ARG);
    REJECT("n_matches = INT64_MIN", a.n_matches = INT64_MIN, OETR_ERR_BAD_ARG);
    REJECT("n_hyp = 0", a.n_hyp = 0, OETR_ERR_BAD_ARG);
    REJECT("n_hyp = -1", a.n_hyp = -1, OETR_ERR_BAD_ARG);
    REJECT("n_hyp = 4097", a.n_hyp = 4097, OETR_ERR_BAD_ARG);
    REJECT("n_hyp = INT32_MAX", a.n_hyp = INT32_MAX, OETR_ERR_BAD_ARG);
    REJECT("n_models_in = 0", (a.models_in = static_cast<const double*>(keep), a.n_models_in = 0), OETR_ERR_BAD_ARG);
    REJECT("n_models_in = -1", (a.models_in = static_cast<const double*>(keep), a.n_models_in = -1), OETR_ERR_BAD_ARG);
    REJECT("n_models_in = 4097", (a.models_in = static_cast<const double*>(keep), a.n_models_in = 4097),
           OETR_ERR_BAD_ARG);
    REJECT("refit_iters = -1", a.refit_iters = -1, OETR_ERR_BAD_ARG);
    REJECT("refit_iters = 5", a.refit_iters = 5, OETR_ERR_BAD_ARG);
    REJECT("refit_iters = INT32_MAX", a.refit_iters = INT32_MAX, OETR_ERR_BAD_ARG);
    REJECT("px_thr = 0", a.px_thr = 0.0, OETR_ERR_BAD_ARG);
    REJECT("px_thr = -1", a.px_thr = -1.0, OETR_ERR_BAD_ARG);
    REJECT("px_thr = NaN", a.px_thr = NAN, OETR_ERR_BAD_ARG);
    REJECT("px_thr = inf", a.px_thr = INFINITY, OETR_ERR_BAD_ARG);
    REJECT("workspace = NULL", a.workspace = nullptr, OETR_ERR_BAD_ARG);
    REJECT("workspace one byte short", a.workspace_bytes -= 1, OETR_ERR_BAD_ARG);
    REJECT("workspace of 0 bytes", a.workspace_bytes = 0, OETR_ERR_BAD_ARG);
    REJECT("workspace short for models_in", (a.models_in = static_cast<const double*>(keep), a.n_models_in = 9),
           OETR_ERR_BAD_ARG);
    REJECT("n_matches = 2^31", a.n_matches = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
    REJECT("n_matches = INT64_MAX", a.n_matches = INT64_MAX, OETR_ERR_BAD_SHAPE);
    REJECT("n_pairs * n_models = 2^31 + ...", (a.n_pairs = INT32_MAX / 8 + 1, a.workspace_bytes = SIZE_MAX),
           OETR_ERR_BAD_SHAPE);
    REJECT("n_pairs = INT32_MAX, n_hyp = 2", (a.n_pairs = INT32_MAX, a.n_hyp = 2, a.workspace_bytes = SIZE_MAX),
           OETR_ERR_BAD_SHAPE);
  }

  if (char* none = hostcheck::no_device_page()) {
    for (int route = 0; route < 4; ++route) {
      Args a = pointing_at(none + 256);
      const char* label = "sampled, 2 pairs";
      if (route == 1) {
        label = "largest sampled call";
        a.n_pairs = INT32_MAX / 4096, a.n_hyp = 4096, a.n_matches = INT32_MAX, a.pair_ids = nullptr;
        a.workspace_bytes = oetr_homography_ransac_workspace_bytes(a.n_pairs, 4096);
      } else if (route == 2) {
        label = "models_in, no inliers";
        a.models_in = reinterpret_cast<const double*>(none + 512), a.n_models_in = 257, a.n_hyp = 0, a.inliers = nullptr;
        a.workspace_bytes = oetr_homography_ransac_workspace_bytes(a.n_pairs, 257);
      } else if (route == 3) {
        label = "no matches, no refit";
        a.n_matches = 0, a.k1 = a.k2 = nullptr, a.refit_iters = 0;
      }
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
