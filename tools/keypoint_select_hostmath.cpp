// The descriptor arithmetic of oetr_keypoint_select on the HOST: imagematching_oetr_amd/csrc/keypoint_select_math.h -
// the one copy the kernel uses - compiled as plain C++, with k_ks_emit's wave restated serially (a loop over the 64
// "lanes", the shuffle tree over an array).  tests/test_keypoint_select_cpu.py loads it and compares the coordinates
// and the descriptors with the numpy specification bit for bit, so a slip between the specification and the header
// shows on a machine without a GPU.
//
// Build (tools/README.md):  make -C imagematching_oetr_amd/csrc hostmath-keypoint_select
#include <cstdint>
#include <stddef.h>

#include "../imagematching_oetr_amd/csrc/keypoint_select_math.h"

using namespace oetr;

extern "C" {

float ks_host_load_score(float s) { return ks::load_score(s); }

float ks_host_coordinate(float kp, int n, int cell) { return ks::coordinate(kp, n, cell); }

// K keypoints (x[i], y[i]) on the map `desc` [D][h][w] read through its three element strides; out [K][D].
void ks_host_descriptors(const float* desc, int D, int h, int w, int64_t sd, int64_t sy, int64_t sx, const float* x,
                         const float* y, int K, int cell, float* out) {
  for (int i = 0; i < K; ++i) {
    const ks::Taps taps = ks::taps(x[i], y[i], w, h, cell);
    float val[512], part[64], next[64];
    for (int lane = 0; lane < 64; ++lane) {
      part[lane] = 0.0f;
      for (int d = lane; d < D; d += 64) {
        val[d] = ks::interpolate(taps, desc + (int64_t)d * sd, sy, sx);
        part[lane] = ks::add_square(part[lane], val[d]);
      }
    }
    for (int stride = 32; stride >= 1; stride >>= 1) {               // __shfl_down: a lane past the end reads itself
      for (int lane = 0; lane < 64; ++lane)
        next[lane] = ks::tree_step(part[lane], part[lane + stride < 64 ? lane + stride : lane]);
      for (int lane = 0; lane < 64; ++lane) part[lane] = next[lane];
    }
    const float norm = ks::norm_of(part[0]);
    for (int d = 0; d < D; ++d) out[(size_t)i * D + d] = val[d] / norm;
  }
}

}  // extern "C"
