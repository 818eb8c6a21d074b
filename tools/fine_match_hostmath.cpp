// The arithmetic of oetr_fine_refine on the HOST: imagematching_oetr_amd/csrc/fine_match_math.h - the one copy the
// kernels use - compiled as plain C++, with k_fr_head's walk restated serially (the 16 lanes of a window row as a
// loop over partials, the four shuffle levels as the tree, wave 0's lanes as loops over the window's positions).
// tests/test_fine_match_cpu.py loads it and compares every dot product, every expectation and every refined keypoint
// with the numpy specification bit for bit, so a slip between the specification and the header shows on a machine
// without a GPU.
//
// Build (tools/README.md):  make -C imagematching_oetr_amd/csrc hostmath-fine_match
#include <cmath>
#include <cstdint>
#include <stddef.h>

#include "../imagematching_oetr_amd/csrc/fine_match_math.h"

using namespace oetr;

namespace {

// one window row against the centre row: lane l owns partial l and the float4 groups l, l + 16, ...
float dot_row(const float* centre, const float* row, int C) {
  float lane[fm::PARTIALS];
  for (int l = 0; l < fm::PARTIALS; ++l) {
    float acc = 0.0f;
    for (int c4 = l; c4 < C / 4; c4 += fm::PARTIALS) {
      const float *x = centre + 4 * c4, *y = row + 4 * c4;
      acc = fm::chain4(acc, x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]);
    }
    lane[l] = acc;
  }
  for (int d = 1; d < fm::PARTIALS; d <<= 1) {                      // __shfl_xor(acc, d): every lane adds its partner
    float next[fm::PARTIALS];
    for (int l = 0; l < fm::PARTIALS; ++l) next[l] = fm::tree_node(lane[l], lane[l ^ d]);
    for (int l = 0; l < fm::PARTIALS; ++l) lane[l] = next[l];
  }
  return lane[0];
}

}  // namespace

extern "C" {

int fm_host_partials(void) { return fm::PARTIALS; }

void fm_host_partial_of(int n, int32_t* out) {
  for (int c = 0; c < n; ++c) out[c] = fm::partial_of(c);
}

// G and its rounded squares, W entries each
void fm_host_grid(int W, float* g, float* g2) {
  for (int k = 0; k < W; ++k) g[k] = fm::grid(W, k), g2[k] = fm::grid2(W, k);
}

float fm_host_scale(int C) { return fm::scale_of(C); }

float fm_host_radius(int W, float fine_cell) { return fm::radius_of(W, fine_cell); }

// win0, win1 [M][W*W][C] -> s [M][W*W], expec [M][3], has [M]
void fm_host_head(const float* win0, const float* win1, int M, int W, int C, float* s, float* expec, int32_t* has) {
  const int WW = W * W;
  const float scale = fm::scale_of(C);
  for (int m = 0; m < M; ++m) {
    const float* centre = win0 + ((size_t)m * WW + WW / 2) * C;
    float t[64], q[64], heat[64];
    float mx = -INFINITY;
    for (int r = 0; r < WW; ++r) {
      s[(size_t)m * WW + r] = dot_row(centre, win1 + ((size_t)m * WW + r) * C, C);
      t[r] = fm::t_of(s[(size_t)m * WW + r], scale);
      mx = fm::max_push(mx, t[r]);
    }
    const bool any = mx > -INFINITY;
    for (int r = 0; r < WW; ++r) q[r] = any ? fm::q_of(t[r], mx) : 0.0f;
    const float Z = fm::sum_q(q, WW);
    for (int r = 0; r < WW; ++r) heat[r] = any ? fm::heat_of(q[r], Z) : 0.0f;
    const fm::Expec e = any ? fm::finish(fm::moment(heat, W, 0), fm::moment(heat, W, 1), fm::moment(heat, W, 2),
                                         fm::moment(heat, W, 3))
                            : fm::none();
    expec[3 * (size_t)m] = e.x, expec[3 * (size_t)m + 1] = e.y, expec[3 * (size_t)m + 2] = e.sd;
    has[m] = any;
  }
}

// out[i] = kp[i] + v[i] * radius
void fm_host_refined(const float* kp, const float* v, int n, float radius, float* out) {
  for (int i = 0; i < n; ++i) out[i] = fm::refined(kp[i], v[i], radius);
}

}  // extern "C"
