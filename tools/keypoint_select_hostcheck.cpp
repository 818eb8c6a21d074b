// Host-side check of oetr_keypoint_select (include/oetr_keypoint_select.h) under AddressSanitizer and UBSan, on a
// machine WITHOUT a GPU: a stand-alone program, linked with the library's host code, never loaded into Python.
//
//   1. every rejected-argument path returns its status, sets oetr_last_error, and leaves a 64-byte host buffer
//      that stands in for the device untouched;
//   2. calls with acceptable arguments whose every "device" pointer points into a PROT_NONE page: the host code
//      dereferences none of them, so the call comes back with a status (OETR_ERR_HIP: there is no device to enqueue
//      on), not with a signal.  Where a GPU is visible these calls are SKIPPED - they would enqueue kernels on host
//      addresses - and the program says so.
//
// Build and run (tools/README.md):  make -C imagematching_oetr_amd/csrc hostcheck-keypoint_select
#include <cmath>
#include <cstdint>

#include "../include/oetr_keypoint_select.h"
#include "hostcheck.h"

namespace {

const char ENTRY[] = "oetr_keypoint_select";

struct Args {
  const oetr_keypoint_map* maps;
  int n_maps;
  int64_t max_pixels, total_pixels;
  int D, nms_radius;
  float threshold;
  int remove_borders, max_keypoints, cell;
  void* workspace;
  size_t workspace_bytes;
  float *keypoints, *scores, *descriptors;
  int32_t *offsets, *counts;
};

Args pointing_at(void* p) {
  Args a;
  a.maps = static_cast<const oetr_keypoint_map*>(p);
  a.n_maps = 3;
  a.max_pixels = 480 * 640;
  a.total_pixels = 3 * 480 * 640;
  a.D = 256;
  a.nms_radius = 4;
  a.threshold = 0.005f;
  a.remove_borders = 4;
  a.max_keypoints = 2048;
  a.cell = 8;
  a.workspace = p;
  a.workspace_bytes = (size_t)1 << 30;
  a.keypoints = a.scores = a.descriptors = static_cast<float*>(p);
  a.offsets = a.counts = static_cast<int32_t*>(p);
  return a;
}

oetr_status call(const Args& a) {
  return oetr_keypoint_select(a.maps, a.n_maps, a.max_pixels, a.total_pixels, a.D, a.nms_radius, a.threshold,
                              a.remove_borders, a.max_keypoints, a.cell, a.workspace, a.workspace_bytes, a.keypoints,
                              a.scores, a.descriptors, a.offsets, a.counts, nullptr);
}

}  // namespace

int main() {
  hostcheck::begin();
  if (oetr_keypoint_select_abi_version() != OETR_KEYPOINT_SELECT_ABI_VERSION) {
    std::printf("ABI version %d != %d\n", oetr_keypoint_select_abi_version(), OETR_KEYPOINT_SELECT_ABI_VERSION);
    return 1;
  }
  if (oetr_keypoint_select_workspace_bytes(0, 1, 1) != 0 || oetr_keypoint_select_workspace_bytes(-1, 1, 1) != 0 ||
      oetr_keypoint_select_workspace_bytes(INT64_MIN, 1, 1) != 0 || oetr_keypoint_select_workspace_bytes(INT64_MAX, 1, 1) != 0 ||
      oetr_keypoint_select_workspace_bytes(100, 0, 1) != 0 || oetr_keypoint_select_workspace_bytes(100, -1, 1) != 0 ||
      oetr_keypoint_select_workspace_bytes(100, INT32_MAX, 4096) != 0 || oetr_keypoint_select_workspace_bytes(100, 1, 0) != 0 ||
      oetr_keypoint_select_workspace_bytes(100, 1, 4097) != 0 ||
      oetr_keypoint_select_workspace_bytes(1000, 2, 16) < 7 * 1000 + 4 * 2 * 16 ||
      oetr_keypoint_select_workspace_bytes((int64_t)1 << 40, 1 << 19, 4096) != 0 ||
      oetr_keypoint_select_workspace_bytes((int64_t)1 << 40, 1 << 19, 4095) < ((size_t)7 << 40)) {
    std::printf("oetr_keypoint_select_workspace_bytes FAILED\n");
    ++hostcheck::failures;
  }
  const Args good = pointing_at(hostcheck::keep);
  Args a;
  REJECT("maps = NULL", a.maps = nullptr, OETR_ERR_BAD_ARG);
  REJECT("workspace = NULL", a.workspace = nullptr, OETR_ERR_BAD_ARG);
  REJECT("keypoints = NULL", a.keypoints = nullptr, OETR_ERR_BAD_ARG);
  REJECT("scores = NULL", a.scores = nullptr, OETR_ERR_BAD_ARG);
  REJECT("descriptors = NULL", a.descriptors = nullptr, OETR_ERR_BAD_ARG);
  REJECT("offsets = NULL", a.offsets = nullptr, OETR_ERR_BAD_ARG);
  REJECT("counts = NULL", a.counts = nullptr, OETR_ERR_BAD_ARG);
  REJECT("n_maps = 0", a.n_maps = 0, OETR_ERR_BAD_ARG);
  REJECT("n_maps = INT32_MIN", a.n_maps = INT32_MIN, OETR_ERR_BAD_ARG);
  REJECT("max_pixels = 0", a.max_pixels = 0, OETR_ERR_BAD_ARG);
  REJECT("total_pixels = INT64_MIN", a.total_pixels = INT64_MIN, OETR_ERR_BAD_ARG);
  REJECT("D = 0", a.D = 0, OETR_ERR_BAD_ARG);
  REJECT("D = 130", a.D = 130, OETR_ERR_BAD_ARG);
  REJECT("D = 516", a.D = 516, OETR_ERR_BAD_ARG);
  REJECT("D = INT32_MIN", a.D = INT32_MIN, OETR_ERR_BAD_ARG);
  REJECT("nms_radius = -1", a.nms_radius = -1, OETR_ERR_BAD_ARG);
  REJECT("nms_radius = 9", a.nms_radius = 9, OETR_ERR_BAD_ARG);
  REJECT("nms_radius = INT32_MAX", a.nms_radius = INT32_MAX, OETR_ERR_BAD_ARG);
  REJECT("threshold = -0.5", a.threshold = -0.5f, OETR_ERR_BAD_ARG);
  REJECT("threshold = NaN", a.threshold = std::nanf(""), OETR_ERR_BAD_ARG);
  REJECT("remove_borders = -1", a.remove_borders = -1, OETR_ERR_BAD_ARG);
  REJECT("max_keypoints = 0", a.max_keypoints = 0, OETR_ERR_BAD_ARG);
  REJECT("max_keypoints = 4097", a.max_keypoints = 4097, OETR_ERR_BAD_ARG);
  REJECT("max_keypoints = INT32_MIN", a.max_keypoints = INT32_MIN, OETR_ERR_BAD_ARG);
  REJECT("cell = 0", a.cell = 0, OETR_ERR_BAD_ARG);
  REJECT("maps at 4 bytes", a.maps = reinterpret_cast<const oetr_keypoint_map*>(hostcheck::keep + 4), OETR_ERR_BAD_ARG);
  REJECT("keypoints at 4 bytes", a.keypoints = reinterpret_cast<float*>(hostcheck::keep + 4), OETR_ERR_BAD_ARG);
  REJECT("scores at 2 bytes", a.scores = reinterpret_cast<float*>(hostcheck::keep + 2), OETR_ERR_BAD_ARG);
  REJECT("descriptors at 1 byte", a.descriptors = reinterpret_cast<float*>(hostcheck::keep + 1), OETR_ERR_BAD_ARG);
  REJECT("offsets at 2 bytes", a.offsets = reinterpret_cast<int32_t*>(hostcheck::keep + 2), OETR_ERR_BAD_ARG);
  REJECT("counts at 3 bytes", a.counts = reinterpret_cast<int32_t*>(hostcheck::keep + 3), OETR_ERR_BAD_ARG);
  REJECT("workspace at 1 byte", a.workspace = hostcheck::keep + 1, OETR_ERR_BAD_ARG);
  REJECT("max_pixels = 8192^2 + 1", a.max_pixels = (int64_t)8192 * 8192 + 1, OETR_ERR_BAD_SHAPE);
  REJECT("max_pixels = INT64_MAX", a.max_pixels = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("total_pixels = 2^40 + 1", a.total_pixels = ((int64_t)1 << 40) + 1, OETR_ERR_BAD_SHAPE);
  REJECT("total_pixels = INT64_MAX", a.total_pixels = INT64_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_maps = INT32_MAX", a.n_maps = INT32_MAX, OETR_ERR_BAD_SHAPE);
  REJECT("n_maps * max_keypoints = 2^31", (a.n_maps = 1 << 20, a.max_keypoints = 2048), OETR_ERR_BAD_SHAPE);
  REJECT("workspace_bytes = 0", a.workspace_bytes = 0, OETR_ERR_WORKSPACE);
  REJECT("workspace one byte short",
         a.workspace_bytes = oetr_keypoint_select_workspace_bytes(a.total_pixels, a.n_maps, a.max_keypoints) - 1,
         OETR_ERR_WORKSPACE);

  if (char* none = hostcheck::no_device_page()) {
    for (int variant = 0; variant < 5; ++variant) {
      a = pointing_at(none + 256);
      if (variant == 1) a.n_maps = 65538, a.max_pixels = 9, a.total_pixels = (int64_t)65538 * 64, a.max_keypoints = 4, a.D = 4;
      if (variant == 2) a.n_maps = 1 << 19, a.max_keypoints = 4095, a.max_pixels = (int64_t)8192 * 8192,
                        a.total_pixels = (int64_t)1 << 40, a.workspace_bytes = SIZE_MAX, a.D = 512, a.nms_radius = 8;
      if (variant == 3) a.nms_radius = 0, a.threshold = 0.0f, a.remove_borders = INT32_MAX, a.max_keypoints = 1, a.cell = INT32_MAX;
      if (variant == 4) a.threshold = INFINITY, a.max_keypoints = 4096, a.n_maps = 1;
      char label[16];
      std::snprintf(label, sizeof label, "variant %d", variant);
      hostcheck::expect_no_device(label, a);
    }
  }
  return hostcheck::finish();
}
