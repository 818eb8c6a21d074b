// Host-side check of oetr_fine_windows and oetr_fine_refine (include/oetr_fine_match.h) under AddressSanitizer and
// UBSan, on a machine WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into
// Python.
//
//   1. every rejected-argument path of both entries returns its status, sets oetr_last_error, and leaves a 64-byte
//      host buffer that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible these calls are SKIPPED - they would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-fine_match
#include <cmath>
#include <cstdint>

#include "../include/oetr_fine_match.h"
#include "hostcheck.h"

namespace {

const char ENTRY[] = "oetr_fine_";       // both entries' errors open with their own name

struct Args {
  bool refine;                           // which entry
  // oetr_fine_windows
  const int32_t *matches0, *off0, *off1, *grids0, *grids1;
  int64_t n_tok0, n_tok1;
  int n_pairs, max_k0;
  const float* fine0;
  const int32_t *foff0, *fgrids0;
  int64_t n_fine0;
  const float* fine1;
  const int32_t *foff1, *fgrids1;
  int64_t n_fine1;
  int C, W, stride;
  int64_t max_matches;
  void* workspace;
  size_t workspace_bytes;
  int32_t *rows, *moffsets, *counts;
  float *win0, *win1;
  // oetr_fine_refine
  const int32_t* wcounts;
  const float *keypoints0, *keypoints1;
  float fine_cell;
  float *expec, *mkpts0, *mkpts1, *keypoints1_f;
};

Args pointing_at(void* p) {
  Args a;
  a.refine = false;
  a.matches0 = a.off0 = a.off1 = a.grids0 = a.grids1 = a.foff0 = a.foff1 = a.fgrids0 = a.fgrids1 = a.wcounts =
      static_cast<const int32_t*>(p);
  a.n_tok0 = 5;
  a.n_tok1 = 4;
  a.n_pairs = 2;
  a.max_k0 = 3;
  a.fine0 = a.fine1 = a.keypoints0 = a.keypoints1 = static_cast<const float*>(p);
  a.n_fine0 = 80;
  a.n_fine1 = 64;
  a.C = 128;
  a.W = 5;
  a.stride = 4;
  a.max_matches = 6;
  a.workspace = p;
  a.workspace_bytes = 1 << 20;
  a.rows = a.moffsets = a.counts = static_cast<int32_t*>(p);
  a.win0 = a.win1 = a.expec = a.mkpts0 = a.mkpts1 = a.keypoints1_f = static_cast<float*>(p);
  a.fine_cell = 2.0f;
  return a;
}

oetr_status call(const Args& a) {
  if (a.refine)
    return oetr_fine_refine(a.win0, a.win1, a.rows, a.moffsets, a.wcounts, a.n_pairs, a.max_matches, a.keypoints0,
                            a.off0, a.n_tok0, a.keypoints1, a.off1, a.n_tok1, a.C, a.W, a.fine_cell, a.expec, a.mkpts0,
                            a.mkpts1, a.keypoints1_f, a.counts, nullptr);
  return oetr_fine_windows(a.matches0, a.off0, a.off1, a.grids0, a.grids1, a.n_tok0, a.n_tok1, a.n_pairs, a.max_k0,
                           a.fine0, a.foff0, a.fgrids0, a.n_fine0, a.fine1, a.foff1, a.fgrids1, a.n_fine1, a.C, a.W,
                           a.stride, a.max_matches, a.workspace, a.workspace_bytes, a.rows, a.moffsets, a.counts,
                           a.win0, a.win1, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_fine_match_abi_version() != OETR_FINE_MATCH_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_fine_match_abi_version(), OETR_FINE_MATCH_ABI_VERSION);
    return 1;
  }
  if (oetr_fine_match_workspace_bytes(0) != 0 || oetr_fine_match_workspace_bytes(INT32_MIN) != 0 ||
      oetr_fine_match_workspace_bytes(1) < 4 || oetr_fine_match_workspace_bytes(INT32_MAX / 3) < (size_t)INT32_MAX / 3 * 4) {
    std::printf("oetr_fine_match_workspace_bytes FAILED\n");
    ++hostcheck::failures;
  }
  unsigned char* const keep = hostcheck::keep;
  Args good = pointing_at(keep);
  Args a;
  // ---- oetr_fine_windows
  REJECT("w: matches0 = NULL", a.matches0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: off0 = NULL", a.off0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: off1 = NULL", a.off1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: grids0 = NULL", a.grids0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: grids1 = NULL", a.grids1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: foff0 = NULL", a.foff0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: foff1 = NULL", a.foff1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: fgrids0 = NULL", a.fgrids0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: fgrids1 = NULL", a.fgrids1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: fine0 = NULL", a.fine0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: fine1 = NULL", a.fine1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: rows = NULL", a.rows = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: win0 = NULL", a.win0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: win1 = NULL", a.win1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: moffsets = NULL", a.moffsets = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: workspace = NULL", a.workspace = nullptr, OETR_ERR_BAD_ARG);
  REJECT("w: n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
  REJECT("w: n_pairs = -7", a.n_pairs = -7, OETR_ERR_BAD_ARG);
  REJECT("w: n_tok0 = -1", a.n_tok0 = -1, OETR_ERR_BAD_ARG);
  REJECT("w: n_tok1 = INT64_MIN", a.n_tok1 = INT64_MIN, OETR_ERR_BAD_ARG);
  REJECT("w: n_fine0 = -1", a.n_fine0 = -1, OETR_ERR_BAD_ARG);
  REJECT("w: n_fine1 = -1", a.n_fine1 = -1, OETR_ERR_BAD_ARG);
  REJECT("w: max_k0 = -1", a.max_k0 = -1, OETR_ERR_BAD_ARG);
  REJECT("w: max_matches = -1", a.max_matches = -1, OETR_ERR_BAD_ARG);
  REJECT("w: W = 4", a.W = 4, OETR_ERR_BAD_ARG);
  REJECT("w: W = 1", a.W = 1, OETR_ERR_BAD_ARG);
  REJECT("w: W = 9", a.W = 9, OETR_ERR_BAD_ARG);
  REJECT("w: W = INT32_MIN", a.W = INT32_MIN, OETR_ERR_BAD_ARG);
  REJECT("w: stride = 0", a.stride = 0, OETR_ERR_BAD_ARG);
  REJECT("w: stride = 9", a.stride = 9, OETR_ERR_BAD_ARG);
  REJECT("w: C = 0", a.C = 0, OETR_ERR_BAD_ARG);
  REJECT("w: C = 130", a.C = 130, OETR_ERR_BAD_ARG);
  REJECT("w: C = 516", a.C = 516, OETR_ERR_BAD_ARG);
  REJECT("w: C = INT32_MAX", a.C = INT32_MAX, OETR_ERR_BAD_ARG);
  REJECT("w: fine0 at 8 bytes", a.fine0 = reinterpret_cast<const float*>(keep + 8), OETR_ERR_BAD_ARG);
  REJECT("w: fine1 at 4 bytes", a.fine1 = reinterpret_cast<const float*>(keep + 4), OETR_ERR_BAD_ARG);
  REJECT("w: win0 at 8 bytes", a.win0 = reinterpret_cast<float*>(keep + 8), OETR_ERR_BAD_ARG);
  REJECT("w: win1 at 4 bytes", a.win1 = reinterpret_cast<float*>(keep + 4), OETR_ERR_BAD_ARG);
  REJECT("w: matches0 at 2 bytes", a.matches0 = reinterpret_cast<const int32_t*>(keep + 2), OETR_ERR_BAD_ARG);
  REJECT("w: fgrids1 at 1 byte", a.fgrids1 = reinterpret_cast<const int32_t*>(keep + 1), OETR_ERR_BAD_ARG);
  REJECT("w: rows at 2 bytes", a.rows = reinterpret_cast<int32_t*>(keep + 2), OETR_ERR_BAD_ARG);
  REJECT("w: workspace at 2 bytes", a.workspace = keep + 2, OETR_ERR_BAD_ARG);
  REJECT("w: n_tok0 = 2^31", a.n_tok0 = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
  REJECT("w: n_fine1 = INT64_MAX", a.n_fine1 = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("w: n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("w: max_matches past INT32_MAX/25", a.max_matches = INT32_MAX / 25 + 1, OETR_ERR_BAD_SHAPE);
  REJECT("w: max_matches = INT64_MAX", a.max_matches = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("w: workspace_bytes = 0", a.workspace_bytes = 0, OETR_ERR_WORKSPACE);
  REJECT("w: workspace one byte short",
         (a.n_pairs = 100000, a.workspace_bytes = oetr_fine_match_workspace_bytes(100000) - 1), OETR_ERR_WORKSPACE);
  // ---- oetr_fine_refine
  good.refine = true;
  REJECT("r: win0 = NULL", a.win0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: win1 = NULL", a.win1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: rows = NULL", a.rows = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: moffsets = NULL", a.moffsets = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: wcounts = NULL", a.wcounts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: keypoints0 = NULL", a.keypoints0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: keypoints1 = NULL", a.keypoints1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: off0 = NULL", a.off0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: off1 = NULL", a.off1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: expec = NULL", a.expec = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: mkpts0 = NULL", a.mkpts0 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: mkpts1 = NULL", a.mkpts1 = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: keypoints1_f = NULL", a.keypoints1_f = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("r: n_pairs = 0", a.n_pairs = 0, OETR_ERR_BAD_ARG);
  REJECT("r: n_tok0 = -1", a.n_tok0 = -1, OETR_ERR_BAD_ARG);
  REJECT("r: n_tok1 = -1", a.n_tok1 = -1, OETR_ERR_BAD_ARG);
  REJECT("r: max_matches = -1", a.max_matches = -1, OETR_ERR_BAD_ARG);
  REJECT("r: W = 6", a.W = 6, OETR_ERR_BAD_ARG);
  REJECT("r: C = 2", a.C = 2, OETR_ERR_BAD_ARG);
  REJECT("r: C = 1024", a.C = 1024, OETR_ERR_BAD_ARG);
  REJECT("r: fine_cell = 0", a.fine_cell = 0.0f, OETR_ERR_BAD_ARG);
  REJECT("r: fine_cell = -2", a.fine_cell = -2.0f, OETR_ERR_BAD_ARG);
  REJECT("r: fine_cell = inf", a.fine_cell = INFINITY, OETR_ERR_BAD_ARG);
  REJECT("r: fine_cell = NaN", a.fine_cell = NAN, OETR_ERR_BAD_ARG);
  REJECT("r: win0 at 8 bytes", a.win0 = reinterpret_cast<float*>(keep + 8), OETR_ERR_BAD_ARG);
  REJECT("r: keypoints1 at 4 bytes", a.keypoints1 = reinterpret_cast<const float*>(keep + 4), OETR_ERR_BAD_ARG);
  REJECT("r: mkpts1 at 4 bytes", a.mkpts1 = reinterpret_cast<float*>(keep + 4), OETR_ERR_BAD_ARG);
  REJECT("r: keypoints1_f at 4 bytes", a.keypoints1_f = reinterpret_cast<float*>(keep + 4), OETR_ERR_BAD_ARG);
  REJECT("r: expec at 2 bytes", a.expec = reinterpret_cast<float*>(keep + 2), OETR_ERR_BAD_ARG);
  REJECT("r: rows at 1 byte", a.rows = reinterpret_cast<int32_t*>(keep + 1), OETR_ERR_BAD_ARG);
  REJECT("r: n_tok1 = 2^31", a.n_tok1 = (int64_t)1 << 31, OETR_ERR_BAD_SHAPE);
  REJECT("r: n_pairs = INT32_MAX", a.n_pairs = INT32_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("r: max_matches past INT32_MAX/49", (a.W = 7, a.max_matches = INT32_MAX / 49 + 1), OETR_ERR_BAD_SHAPE);

  if (char* none = hostcheck::no_device_page()) {
    for (int variant = 0; variant < 8; ++variant) {
      a = pointing_at(none + 256);
      a.refine = variant >= 4;
      const int v = variant & 3;
      if (v == 1)
        a.n_tok0 = a.n_tok1 = a.n_fine0 = a.n_fine1 = 0, a.max_matches = 0, a.matches0 = nullptr,
        a.fine0 = a.fine1 = nullptr, a.rows = nullptr, a.win0 = a.win1 = nullptr, a.keypoints0 = a.keypoints1 = nullptr,
        a.expec = a.mkpts0 = a.mkpts1 = a.keypoints1_f = nullptr;
      if (v == 2)
        a.n_tok0 = a.n_tok1 = a.n_fine0 = a.n_fine1 = INT32_MAX, a.n_pairs = INT32_MAX / 3, a.max_k0 = INT32_MAX,
        a.C = 512, a.W = 7, a.stride = 8, a.max_matches = INT32_MAX / 49,
        a.workspace_bytes = oetr_fine_match_workspace_bytes(INT32_MAX / 3);
      if (v == 3) a.W = 3, a.C = 4, a.stride = 1, a.max_k0 = 0, a.fine_cell = 1e-30f;
      char label[24];
      std::snprintf(label, sizeof label, "%s variant %d", a.refine ? "refine" : "windows", v);
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
